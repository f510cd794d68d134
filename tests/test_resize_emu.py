"""The image-resize kernel (csrc/resize.hip: k_resize_image) under the CPU SIMT emulator, through rgbl_resize,
rgbl_resize_batch_device and rgbl_extract_resized, bit for bit against tests/resize_ref.py (a restatement of cv::resize = the
oracle's at one channel, unpinned).  The thin sources, the clamps and the shrunken tiles are where a bad address would show:
they run here before they run on a GPU.  tests/test_resize_gpu.py runs the same cases on the MI355X."""
import pytest

import resize_cases as RC


@pytest.mark.parametrize("channels", RC.CHANNELS)
@pytest.mark.parametrize("name,sizes", RC.SMALL, ids=RC.SMALL_IDS)
def test_host_call(emu_lib, name, sizes, channels):
    info = RC.check_host_case(emu_lib, sizes, channels)
    assert info["area_fast"] == (1 if name == "half" else 0)
    assert info["table_bytes"] > 0


def test_full_frame(emu_lib):
    info = RC.check_host_case(emu_lib, RC.BIG, 1)
    assert info["area_fast"] == 0


@pytest.mark.parametrize("batch", [8, 9])
@pytest.mark.parametrize("channels", RC.CHANNELS)
def test_batches_with_frame_strides(emu_lib, channels, batch):
    RC.check_batch_case(emu_lib, None, channels, batch)


def test_error_returns(emu_lib):
    RC.check_errors(emu_lib)


@pytest.mark.parametrize("channels", [1, 3])
def test_extract_resized_equals_extract_on_the_restated_image(emu_lib, channels):
    RC.check_extract_resized(emu_lib, 200, 160, 160, 128, channels)
