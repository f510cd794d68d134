"""bench.py --dump-outputs on the host: which frames of a step are written, in what layout, and that the files stay within
their size bound whatever the batch and the keypoint capacity."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_frames_are_a_fixed_sample_within_the_byte_bound():
    assert np.array_equal(bench.dump_frames(10, 2100), np.arange(10))
    a, b = bench.dump_frames(1024, 2100), bench.dump_frames(1024, 2100)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_FRAMES and len(np.unique(a)) == len(a)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 1024
    for B, cap in ((1024, 2100), (64, 8100), (64, 40000), (4096, 65535)):
        k = len(bench.dump_frames(B, cap))
        assert 1 <= k <= min(B, bench.DUMP_FRAMES)
        assert k * cap * 4 * (7 + 32 + 5) <= bench.DUMP_BYTES                    # per-keypoint arrays
        assert k * cap * 4 * (7 + 32 + 5) + 4 * (2 * B + k) <= 64 << 20          # + n, mono, frames


def test_dump_outputs_layout(tmp_path):
    rng = np.random.default_rng(3)
    B, cap = 6, 5
    n = np.array([3, 0, 5, 7, -1, 2], np.int32)       # 7 > cap and -1 are clamped as the gather clamps them
    mono = np.arange(B, dtype=np.int32)
    kp = rng.standard_normal((B, cap, 7)).astype(np.float32)
    kp.view(np.int32)[..., 5] = rng.integers(0, 8, (B, cap))          # octave
    kp.view(np.int32)[..., 6] = -1                                    # class_id
    desc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    depth, uright = (rng.standard_normal((B, cap)).astype(np.float32) for _ in range(2))
    bi, bd, sd = (rng.integers(-1, 300, (B, cap)).astype(np.int32) for _ in range(3))
    sel = np.array([0, 2, 3, 5])
    shapes = bench.dump_outputs(str(tmp_path), n, mono, kp[sel], desc[sel], depth[sel], uright[sel], bi[sel], bd[sel], sd[sel],
                                frames=sel)
    a = {p.stem: np.load(str(p)) for p in tmp_path.iterdir()}
    assert set(a) == set(shapes) and all(v.dtype == np.float32 and list(v.shape) == shapes[k] for k, v in a.items())
    assert np.array_equal(a["n"], n) and np.array_equal(a["mono"], mono) and np.array_equal(a["frames"], sel)
    cnt = [3, 5, 5, 2]
    assert len(a["depth"]) == sum(cnt)
    o = 0
    for f, c in zip(sel, cnt):
        r = slice(o, o + c)
        assert np.array_equal(a["keypoints"][r, :5].view(np.uint32), kp[f, :c, :5].view(np.uint32))
        assert np.array_equal(a["keypoints"][r, 5:], kp[f, :c, 5:].view(np.int32).astype(np.float32))
        assert np.array_equal(a["descriptors"][r], desc[f, :c].astype(np.float32))
        assert np.array_equal(a["depth"][r].view(np.uint32), depth[f, :c].view(np.uint32))
        assert np.array_equal(a["uright"][r].view(np.uint32), uright[f, :c].view(np.uint32))
        for name, src in (("match_index", bi), ("match_distance", bd), ("match_second_distance", sd)):
            assert np.array_equal(a[name][r], src[f, :c].astype(np.float32))
        o += c
