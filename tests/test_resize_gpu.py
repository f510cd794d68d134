"""The image-resize kernel (csrc/resize.hip) on a real MI355X: every case of tests/resize_cases.py through rgbl_resize and
rgbl_resize_batch_device, bit for bit against tests/resize_ref.py (a restatement of cv::resize = the oracle's at one channel,
unpinned); the raw-image extraction rgbl_extract_resized against rgbl_extract on the restated image; a raw stereo pair through
two rgbl_extract_resized calls into rgbl_stereo_matches.  tests/test_resize_emu.py runs the same cases under the SIMT emulator
first."""
import pytest
import torch

import resize_cases as RC

DEV = torch.device("cuda", 0)
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("channels", RC.CHANNELS)
@pytest.mark.parametrize("name,sizes", RC.SMALL, ids=RC.SMALL_IDS)
def test_host_call(gpu_lib, name, sizes, channels):
    info = RC.check_host_case(gpu_lib, sizes, channels)
    assert info["area_fast"] == (1 if name == "half" else 0)


@pytest.mark.parametrize("channels", [1, 3])
def test_full_frame(gpu_lib, channels):
    RC.check_host_case(gpu_lib, RC.BIG, channels)


@pytest.mark.parametrize("batch", [8, 9])
@pytest.mark.parametrize("channels", RC.CHANNELS)
def test_batches_with_frame_strides(gpu_lib, channels, batch):
    RC.check_batch_case(gpu_lib, DEV, channels, batch)


def test_error_returns(gpu_lib):
    RC.check_errors(gpu_lib)


def test_extract_resized_full_frame(gpu_lib):
    RC.check_extract_resized(gpu_lib, 752, 480, 600, 350, 1, nfeatures=1000, nlevels=8)


@pytest.mark.parametrize("channels", [3, 4])
def test_extract_resized_colour(gpu_lib, channels):
    RC.check_extract_resized(gpu_lib, 400, 300, 320, 240, channels, nfeatures=500, nlevels=4)


def test_stereo_pair_through_two_resized_extractions(gpu_lib):
    RC.check_stereo_pair(gpu_lib)
