"""The rectification kernels (csrc/rectify.hip: k_remap_linear, k_remap_gather) under the CPU SIMT emulator, through
rgbl_remap and rgbl_remap_batch_device, bit for bit against tests/remap_ref.py (a restatement of cv::remap, unpinned).
The NaN / huge / random-map cases are where a bad address would show: they run here before they run on a GPU.
tests/test_remap_gpu.py runs the same cases on the MI355X."""
import numpy as np
import pytest

import remap_cases as RC
import remap_ref as R


@pytest.mark.parametrize("channels", RC.CHANNELS)
@pytest.mark.parametrize("name", RC.SMALL_CASES)
def test_host_call(emu_lib, name, channels):
    info = RC.check_host_case(emu_lib, name, channels)
    if name == "random":
        assert info["staged_tiles"] == 0 and info["direct_tiles"] == 4
    if name == "minify":
        assert info["direct_tiles"] > 0
    if name == "mixed":
        assert info["staged_tiles"] > 0 and info["direct_tiles"] > 0
    if name in ("identity", "smooth", "wild"):
        assert info["direct_tiles"] == 0, "a few wild entries must not push a tile off the staged path"
    assert info["map_bytes"] == 16 * (info["staged_tiles"] + info["direct_tiles"]) + 8192 * info["staged_tiles"] + 16384 * info["direct_tiles"]


def test_full_frame(emu_lib):
    info = RC.check_host_case(emu_lib, "big", 1)
    assert info["staged_tiles"] == 12 * 15 and info["direct_tiles"] == 0


@pytest.mark.parametrize("batch", [8, 9])
@pytest.mark.parametrize("channels", RC.CHANNELS)
def test_batches_with_frame_strides(emu_lib, channels, batch):
    info = RC.check_batch_case(emu_lib, None, "mixed", channels, batch)
    assert info["staged_tiles"] > 0 and info["direct_tiles"] > 0


def test_error_returns(emu_lib):
    RC.check_errors(emu_lib)


@pytest.mark.parametrize("channels", [1, 3])
def test_extract_rectified_equals_extract_on_the_restated_image(emu_lib, channels):
    RC.check_extract_rectified(emu_lib, 160, 128, channels)
