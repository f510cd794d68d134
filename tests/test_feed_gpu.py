"""Host-fed batches on the MI355X: KITTI-size frames through rgbl_feeder (three slots, consecutive batches in flight), every
frame bit-identical to rgbl_extract_color + rgbl_depth_compute_xyzi on the same inputs (those are held to the oracle by
test_parity_gpu.py), a sample checked against the CPU oracle directly, and the variable-length projection at KITTI size."""
import numpy as np
import pytest

import feed_cases as fc
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import synth

pytestmark = pytest.mark.gpu
KW, KH = synth.KITTI_W, synth.KITTI_H
MAXP = 130000


def lengths(seed, batches, per_batch):
    """Scan lengths 0 - 130 k, varying per frame; one scan per run at exactly the feeder's max_points, one empty."""
    rng = np.random.default_rng(seed)
    out = [[int(v) for v in rng.integers(0, MAXP + 1, per_batch + (k % 3) * 2)] for k in range(batches)]
    out[0][0] = MAXP
    out[1][1] = 0
    out[-1][-1] = 115000
    return out


def test_feeder_kitti_bgr_seven_batches(gpu_lib):
    stats = fc.feeder_vs_single(gpu_lib, KW, KH, 2000, 8, 3, 1, lengths(1, 7, 8), max_points=MAXP, slots=3, seed=100)
    assert len(stats) >= 7 * 8
    assert np.mean([n for n, _ in stats]) > 1000 and sum(d for _, d in stats) > 1000


@pytest.mark.parametrize("channels,blue_first", [(3, 0), (4, 1), (4, 0), (1, 0)])
def test_feeder_kitti_channels(gpu_lib, channels, blue_first):
    fc.feeder_vs_single(gpu_lib, KW, KH, 2000, 8, channels, blue_first, lengths(channels * 2 + blue_first, 3, 8), max_points=MAXP,
                        slots=3, seed=7 * channels + blue_first)


@pytest.mark.parametrize("w,h,method", [(1241, 376, F.UPS_INVERSE_DILATION), (1242, 375, F.UPS_AVERAGE_FILTERING),
                                         (1226, 370, F.UPS_NEAREST_NEIGHBOR_PIXEL)])
def test_feeder_on_the_kitti_image_sizes(gpu_lib, w, h, method):
    """The image sizes of the KITTI odometry sequences (00-02: 1241 x 376, 03: 1242 x 375, 04-12: 1226 x 370; 1226 leaves a
    one-pixel-wide last detection cell), each with another of the three up-sampling methods the reference implements."""
    fc.feeder_vs_single(gpu_lib, w, h, 2000, 8, 3, 1, lengths(w, 2, 12), max_points=MAXP, slots=3, method=method, seed=w)


def test_feeder_undistorts_kitti(gpu_lib):
    K = (718.856, 718.856, 607.1928, 185.2157)
    stats = fc.feeder_vs_single(gpu_lib, KW, KH, 2000, 8, 3, 1, lengths(5, 3, 8), max_points=MAXP, slots=3, K=K,
                                dist=(-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), seed=55)
    assert sum(d for _, d in stats) > 1000


@pytest.mark.parametrize("method,sparse", [(F.UPS_INVERSE_DILATION, False), (F.UPS_INVERSE_DILATION, True),
                                           (F.UPS_AVERAGE_FILTERING, False), (F.UPS_NEAREST_NEIGHBOR_PIXEL, False)])
def test_varlen_kitti(gpu_lib, method, sparse):
    fc.varlen_batch(gpu_lib, True, KW, KH, method, [MAXP, 0, 1, 1025, 121000, 115000, 256, 129999], sparse=sparse, n_kp=1500)


def test_feeder_sample_against_the_oracle(gpu_lib, oracle):
    """Feeder outputs of a few frames straight against the CPU oracle (extraction and depth)."""
    O = oracle
    lib = gpu_lib
    from orb_slam3_rgbl_amd import feed as FD
    ex = F.ORBextractor(2000, 1.2, 8, 20, 7, KW, KH, max_batch=4, lib=lib)
    proj = fc.projection(lib, KW, KH)
    dm = F.DepthModule(proj, KW, KH, max_points=MAXP, max_keypoints=ex.max_keypoints, max_batch=4, lib=lib)
    fd = FD.HostFeeder(ex, dm, channels=1, max_batch=4, max_points=MAXP, slots=3, lib=lib)
    imgs = fc.colour_frames(3, KW, KH, 4, 1)
    scans = [fc.bin_scan(60 + b, n) for b, n in enumerate([125000, 0, 90000, MAXP])]
    out = next(fd.run([list(zip(imgs, scans))]))
    orc = O.Extractor(2000, 1.2, 8, 20, 7)
    P = O.make_depth_params(proj)
    for b in (0, 3):
        okps, odesc, omono = orc(imgs[b])
        got = out[b]
        assert got["n"] == len(okps) and got["mono"] == omono
        for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
            assert np.array_equal(got["kp"][f].view(np.uint32), okps[f].view(np.uint32)), f
        assert np.array_equal(got["desc"], odesc)
        cloud = np.ascontiguousarray(np.concatenate([scans[b][:, :3].T, np.ones((1, len(scans[b])), np.float32)]))
        xy = np.stack([got["kp"]["x"], got["kp"]["y"]], 1).astype(np.float32)
        d, u, _, _ = O.depth(P, cloud, KW, KH, xy, got["kp"]["x"].astype(np.float32))
        assert np.array_equal(fc.bits(got["depth"]), fc.bits(d)) and np.array_equal(fc.bits(got["uright"]), fc.bits(u))
    fd.close()
    ex.close()
    dm.close()
