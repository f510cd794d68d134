"""The blurred working images are stored in tiles of 32 px x 4 rows (extractor_kernels.h: blur_offset): k_gauss7 writes them,
k_orient_brief gathers its 37 x 37 neighbourhoods from them, rgbl_extractor_get_level(blurred = 1) rebuilds the rows.  These
checks aim at what a tiled layout can get wrong: levels whose sizes are not multiples of the tile, keypoints at the extreme
positions, every alignment of a neighbourhood inside the tiles.  On the emulator build and, marked gpu, on the device;
everything is compared bit for bit with the CPU oracle."""
import numpy as np
import pytest

import parity_checks as pc
from oracle import oracle_py as O
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import synth

KITTI_LEVEL_HEIGHTS = [376, 313, 261, 218, 181, 151, 126, 105]   # one of them a multiple of the tile height


def check_blurred_levels(lib, w, h, nfeatures, nlevels, batch, seq, heights=None):
    ex = F.ORBextractor(nfeatures, 1.2, nlevels, 12, 7, w, h, max_batch=batch, lib=lib)
    orc = O.Extractor(nfeatures, 1.2, nlevels, 12, 7)
    if heights is not None:
        assert [ex.level_size(l)[1] for l in range(nlevels)] == heights
    s = synth.Sequence(seq, w, h, n_frames=batch)
    imgs = np.stack([s.frame(i) for i in range(batch)])
    res = ex.extract_batch(imgs) if batch > 1 else [ex(imgs[0])]
    compared = 0
    for i, (kps, desc, mono) in enumerate(res):
        okps, odesc, omono = orc(imgs[i])
        pc.assert_keypoints_equal(kps, okps, "frame %d" % i)
        assert np.array_equal(desc, odesc) and mono == omono
        for l in range(nlevels):
            if len(orc.level_keypoints(l)):   # the reference blurs the levels that have keypoints
                got, want = ex.image_pyramid(l, frame=i, blurred=True), orc.level_blurred(l)
                assert got.shape == want.shape and np.array_equal(got, want), "frame %d: blurred level %d differs" % (i, l)
                compared += 1
    ex.close()
    return compared


def textured(w, h, seed):
    """A ramp plus two bits of noise: differences over a FAST circle stay below minThFAST (no corner of its own), but the
    blurred neighbourhoods differ from pixel to pixel, so a descriptor gathered from the wrong bytes does not match."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return (40 + 0.1 * xx + 0.2 * yy + rng.integers(0, 4, (h, w))).astype(np.uint8)


def level_coordinates(kps, scale):
    s = np.asarray(scale, np.float32)[kps["octave"]]
    return np.rint(kps["x"] / s).astype(int), np.rint(kps["y"] / s).astype(int)


def run_and_compare(lib, img, nfeatures, nlevels):
    h, w = img.shape
    ex = F.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, w, h, lib=lib)
    orc = O.Extractor(nfeatures, 1.2, nlevels, 20, 7)
    kps, desc, mono = ex(img)
    okps, odesc, omono = orc(img)
    pc.assert_keypoints_equal(kps, okps, "corner frame")
    assert np.array_equal(desc, odesc) and mono == omono
    sizes = [ex.level_size(l) for l in range(nlevels)]
    lx, ly = level_coordinates(kps, ex.mvScaleFactor)
    ex.close()
    return kps, lx, ly, sizes


def check_extreme_positions(lib, w=400, h=300):
    """Keypoints lie in 19 <= x <= w - 20, 19 <= y <= h - 20 of their level.  Single bright pixels are FAST corners of level 0
    exactly where they are put; 2 x 2 blobs at stepped offsets along the four borders put corners of level 1 onto its limits."""
    img = textured(w, h, 1)
    for x, y in ((19, 19), (w - 20, 19), (19, h - 20), (w - 20, h - 20), (19, 150), (w - 20, 151), (200, 19), (201, h - 20)):
        img[y, x] = 255
    for k in range(12):
        img[60 + 15 * k:62 + 15 * k, 22 + k % 6:24 + k % 6] = 255                   # left
        img[60 + 15 * k:62 + 15 * k, w - 29 + k % 6:w - 27 + k % 6] = 255           # right
        img[22 + k % 6:24 + k % 6, 60 + 15 * k:62 + 15 * k] = 255                   # top
        img[h - 29 + k % 6:h - 27 + k % 6, 60 + 15 * k:62 + 15 * k] = 255           # bottom
    kps, lx, ly, sizes = run_and_compare(lib, img, 2000, 3)
    for l in (0, 1):
        m = kps["octave"] == l
        lw, lh = sizes[l]
        assert (lx[m] == 19).any() and (lx[m] == lw - 20).any(), "level %d: no keypoint at the x limits" % l
        assert (ly[m] == 19).any() and (ly[m] == lh - 20).any(), "level %d: no keypoint at the y limits" % l
    at = set(zip(lx[kps["octave"] == 0].tolist(), ly[kps["octave"] == 0].tolist()))
    assert {(19, 19), (w - 20, 19), (19, h - 20), (w - 20, h - 20)} <= at
    return len(kps)


def check_every_alignment(lib, w=400, h=340):
    """Level-0 keypoints at 32 consecutive x and 4 consecutive y: every position of the neighbourhood's origin inside a tile
    (and inside the aligned pieces the reader fetches)."""
    img = textured(w, h, 2)
    want = set()
    for i in range(32):
        for j in range(4):
            x, y = 48 + i + 64 * j, 36 + j + 8 * i
            img[y, x] = 255
            want.add((x, y))
    kps, lx, ly, _ = run_and_compare(lib, img, 2000, 2)
    m = kps["octave"] == 0
    at = set(zip(lx[m].tolist(), ly[m].tolist()))
    assert want <= at, "missing: %s" % sorted(want - at)[:8]
    assert {(x % 32, y % 4) for x, y in want} == {(a, b) for a in range(32) for b in range(4)}
    return len(kps)


# ---- emulator build (the same kernel sources on the CPU)
def test_blurred_levels_kitti_emu(emu_lib):
    assert check_blurred_levels(emu_lib, 1241, 376, 2000, 8, 1, seq=3, heights=KITTI_LEVEL_HEIGHTS) == 8


def test_blurred_levels_small_emu(emu_lib):
    assert check_blurred_levels(emu_lib, 160, 120, 300, 4, 1, seq=4) >= 3
    assert check_blurred_levels(emu_lib, 160, 120, 300, 4, 8, seq=5) >= 24


def test_extreme_positions_emu(emu_lib):
    assert check_extreme_positions(emu_lib) > 50


def test_every_alignment_emu(emu_lib):
    assert check_every_alignment(emu_lib) >= 128


# ---- device
@pytest.mark.gpu
def test_blurred_levels_kitti_gpu(gpu_lib):
    assert check_blurred_levels(gpu_lib, 1241, 376, 2000, 8, 1, seq=3, heights=KITTI_LEVEL_HEIGHTS) == 8
    assert check_blurred_levels(gpu_lib, 1241, 376, 2000, 8, 8, seq=6, heights=KITTI_LEVEL_HEIGHTS) == 64


@pytest.mark.gpu
def test_blurred_levels_small_gpu(gpu_lib):
    assert check_blurred_levels(gpu_lib, 160, 120, 300, 4, 1, seq=4) >= 3
    assert check_blurred_levels(gpu_lib, 160, 120, 300, 4, 8, seq=5) >= 24


@pytest.mark.gpu
def test_blurred_levels_4k_gpu(gpu_lib):
    assert check_blurred_levels(gpu_lib, 3840, 2160, 8000, 8, 1, seq=9) == 8


@pytest.mark.gpu
def test_extreme_positions_gpu(gpu_lib):
    assert check_extreme_positions(gpu_lib) > 50


@pytest.mark.gpu
def test_every_alignment_gpu(gpu_lib):
    assert check_every_alignment(gpu_lib) >= 128
