"""The best / second-best tracker of the FP4 matrix-core scan (k_hamming_fp4), bit for bit against oracle_py.hamming_bf.

Small shapes chosen for what the tracker can get wrong: the masked last tile (nb not a multiple of 32), one and two LDS
stages, a partial wave of queries, a sweep boundary (8192 train rows: relative keys, their decrement, the re-basing in
close_sweep), ties (lowest index wins, second == best), the extreme distances 0 and 256 and an empty train set.  Every case
goes through ORBmatcher.BruteForce with the train-set slices on (RGBL_BF_SPLIT unset) and off (=0); the batch entry point
(rgbl_hamming_bf_batch_device, the flagship step's call) gets three pairs of unequal sizes.

The same checks run on the CPU emulation of the kernel sources and, marked gpu, on the device."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F

NA = (1, 63, 64, 65, 257)
NB = (1, 2, 31, 32, 33, 64, 65, 97)
SWEEP = 8192


def _desc(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _near(a, nb, seed):
    """nb train rows: random ones, every third a query with a few bits flipped (so that best and second are close)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    for j in range(0, nb, 3):
        b[j] = a[(7 * j) % len(a)]
        for bit in rng.integers(0, 256, int(rng.integers(0, 6))):
            b[j, bit // 8] ^= np.uint8(1 << (bit % 8))
    return b


class _Matchers:
    """One handle with the train-set slices as built, one with RGBL_BF_SPLIT=0 (the switch is read when the handle is created)."""

    def __init__(self, lib):
        saved = os.environ.pop("RGBL_BF_SPLIT", None)
        try:
            self.ms = [F.ORBmatcher(0.6, False, lib=lib)]
            os.environ["RGBL_BF_SPLIT"] = "0"
            self.ms.append(F.ORBmatcher(0.6, False, lib=lib))
        finally:
            os.environ.pop("RGBL_BF_SPLIT", None)
            if saved is not None:
                os.environ["RGBL_BF_SPLIT"] = saved

    def check(self, a, b, what=""):
        want = O.hamming_bf(a, b)
        for k, m in enumerate(self.ms):
            got = m.BruteForce(a, b)
            for g, w, name in zip(got, want, ("best index", "best distance", "second distance")):
                assert np.array_equal(g, w), "%s: %s differs (na=%d nb=%d split=%s)" % (what, name, len(a), len(b), "on" if k == 0 else "off")
        return want

    def close(self):
        for m in self.ms:
            m.close()


def check_shapes(lib, na):
    ms = _Matchers(lib)
    a = _desc(na, 100 + na)
    for nb in NB:
        ms.check(a, _near(a, nb, 1000 * na + nb), "shapes")
    ms.close()


def check_sweep_boundary(lib):
    ms = _Matchers(lib)
    a = _desc(64, 5)
    nb = SWEEP + 33
    b = _near(a, nb, 6)
    ms.check(a, b, "sweep")
    # the best match in row 0, in the last row and in the first row after the boundary; the runner-up on the other side of it
    far = np.bitwise_not(a[:1])
    for best_row, second_row in ((0, SWEEP), (nb - 1, 0), (SWEEP, SWEEP - 1)):
        t = np.repeat(far, nb, 0)
        t[best_row] = a[0]
        t[second_row] = a[0]
        t[second_row, 3] ^= 0x21
        bi, bd, sd = ms.check(a[:1], t, "sweep rows")
        assert (bi[0], bd[0], sd[0]) == (best_row, 0, 2)
        t[second_row] = a[0]   # a tie across the boundary: the lower index wins, second == best
        bi, bd, sd = ms.check(a[:1], t, "sweep tie")
        assert (bi[0], bd[0], sd[0]) == (min(best_row, second_row), 0, 0)
    ms.close()


def check_ties_and_extremes(lib):
    ms = _Matchers(lib)
    a = _desc(65, 9)
    # duplicated train rows: best == second, the lowest index wins
    for nb in (2, 33, 65, 97):
        b = _near(a, nb, 20 + nb)
        dup = np.concatenate([b, b])
        bi, bd, sd = ms.check(a, dup, "duplicates")
        assert np.array_equal(bd, sd) and (bi < nb).all()
    # all descriptors identical
    same = np.repeat(a[:1], 97, 0)
    bi, bd, sd = ms.check(same[:65], same, "identical")
    assert not bi.any() and not bd.any() and not sd.any()
    # the best match in row 0 / in the last row of one tile, two tiles, two stages
    for nb in (1, 31, 32, 33, 64, 65, 97):
        for row in (0, nb - 1):
            t = _desc(nb, 40 + nb)
            t[row] = a[3]
            bi, bd, sd = ms.check(a[3:4], t, "row")
            assert (bi[0], bd[0]) == (row, 0)
    # distances 0 and 256: a descriptor and its complement
    comp = np.bitwise_not(a)
    bi, bd, sd = ms.check(a, np.concatenate([comp[:33], a[:33]]), "0 and 256")
    assert (bd[:33] == 0).all() and np.array_equal(bi[:33], np.arange(33) + 33)
    bi, bd, sd = ms.check(a[:1], np.concatenate([a[:1], comp[:1]]), "0 then 256")
    assert (bi[0], bd[0], sd[0]) == (0, 0, 256)
    bi, bd, sd = ms.check(a[:1], np.concatenate([comp[:1], a[:1]]), "256 then 0")
    assert (bi[0], bd[0], sd[0]) == (1, 0, 256)
    # nothing but complements: the selection starts at 256 with a strict '<', so there is no best row
    for nb in (1, 2, 33, 97):
        bi, bd, sd = ms.check(a[:1], np.repeat(comp[:1], nb, 0), "256 only")
        assert (bi[0], bd[0], sd[0]) == (-1, 256, 256)
    # an empty train set
    bi, bd, sd = ms.check(a, np.zeros((0, 32), np.uint8), "empty")
    assert (bi == -1).all() and (bd == 256).all() and (sd == 256).all()
    ms.close()


# ---- the 16-bit train index: nb = 65535 is the most a call accepts (tests/limit_cases.py) ------------------------------------
LIMIT_NB = 65535
LAST, TOP_BIT = LIMIT_NB - 1, 32768


def limit_near_rows(a, seed=7):
    """LIMIT_NB _near rows in which query 0 has its only exact copy in the last row and query 1 in row 32768 (_near alone leaves
    every exact copy at a low index: the lowest one wins)"""
    b = _near(a, LIMIT_NB, seed)
    for q, row in ((0, LAST), (1, TOP_BIT)):
        same = (b == a[q]).all(1)
        b[same, 5] ^= np.uint8(0x10)
        b[row] = a[q]
    return b


def limit_directed(a0):
    """(what, train rows, expected (best index, best distance, second distance) of the one query a0[0]) at nb = LIMIT_NB"""
    far = np.bitwise_not(a0[:1])
    for best_row, second_row in ((LAST, TOP_BIT), (TOP_BIT, LAST)):
        t = np.repeat(far, LIMIT_NB, 0)
        t[best_row] = a0[0]
        t[second_row] = a0[0]
        t[second_row, 3] ^= 0x21
        yield "best in row %d, second in row %d" % (best_row, second_row), t, (best_row, 0, 2)
    t = np.repeat(far, LIMIT_NB, 0)
    t[TOP_BIT - 1] = a0[0]
    t[LAST] = a0[0]
    yield "a tie between rows 32767 and 65534", t, (TOP_BIT - 1, 0, 0)
    # distance 256 in every row, the last one included: the key 256 << 16 | 0xfffe is one below kNone = 256 << 16 | 0xffff
    # (no row is nearer than 256, where the selection starts: there is no best row)
    yield "complements only", np.repeat(far, LIMIT_NB, 0), (-1, 256, 256)
    # ... and 256 as the runner-up's distance: the best in the last row at 255
    t = np.repeat(far, LIMIT_NB, 0)
    t[LAST, 0] ^= 1
    yield "255 in row 65534 among complements", t, (LAST, 255, 256)


def check_limit_rows(lib, first_only=False):
    """nb = LIMIT_NB.  first_only: one query row and the first directed case (what the emulator tier can afford)."""
    ms = _Matchers(lib)
    a = _desc(65, 13)
    cases_ = list(limit_directed(a))
    for what, t, expect in cases_[:1] if first_only else cases_:
        bi, bd, sd = ms.check(a[:1], t, what)
        if expect is not None:
            assert (bi[0], bd[0], sd[0]) == expect, (what, bi[0], bd[0], sd[0])
    if not first_only:
        b = limit_near_rows(a)
        bi, bd, sd = ms.check(a, b, "near rows at the limit")
        assert (bi[0], bd[0]) == (LAST, 0) and (bi[1], bd[1]) == (TOP_BIT, 0), (bi[:2], bd[:2])
    ms.close()


def check_limit_refused(lib):
    """nb = 65536: RGBL_ERR_INVALID, the outputs keep the caller's pattern, the handle still works"""
    m = F.ORBmatcher(0.6, False, lib=lib)
    a = _desc(3, 17)
    b = np.zeros((LIMIT_NB + 1, 32), np.uint8)
    out = [np.full(3, -7, np.int32) for _ in range(3)]
    rc = lib.rgbl_hamming_bf(m.h, L.ptr(a), 3, L.ptr(b), LIMIT_NB + 1, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]))
    assert rc == L.ERR_INVALID and b"65535" in lib.rgbl_last_error(), (rc, lib.rgbl_last_error())
    assert all((o == -7).all() for o in out)
    # the batch entry point tests cap before it touches a pointer
    one = C.c_void_p(a.ctypes.data)
    rc = lib.rgbl_hamming_bf_batch_device(m.h, one, one, LIMIT_NB + 1, one, one, 1, one, one, one)
    assert rc == L.ERR_INVALID and b"65535" in lib.rgbl_last_error(), (rc, lib.rgbl_last_error())
    t = _near(a, 40, 3)
    for g, w in zip(m.BruteForce(a, t), O.hamming_bf(a, t)):
        assert np.array_equal(g, w)
    m.close()


def check_batch_device_at_limit(lib, dev):
    """rgbl_hamming_bf_batch_device with cap = 65535: one pair whose train frame is full (d_n = 65535), one the other way round"""
    a = _desc(65, 13)
    check_batch_device(lib, dev, n=(65, LIMIT_NB), pairs=((0, 1), (1, 0)), cap=LIMIT_NB, frames=[a, limit_near_rows(a)],
                       expect={0: ((0, LAST), (1, TOP_BIT))})


def check_batch_device(lib, dev, n=(65, 257, 33, 130), pairs=((0, 1), (1, 2), (3, 0)), cap=300, frames=None, expect=None):
    """rgbl_hamming_bf_batch_device: three pairs of unequal n in one launch.  expect: {pair: ((query, best index), ...)}"""
    import torch
    if frames is None:
        frames = [_desc(n[0], 70)]
        for k in (1, 2, 3):
            frames.append(_near(frames[0], n[k], 70 + k))
    desc = np.zeros((len(n), cap, 32), np.uint8)
    for k, f in enumerate(frames):
        desc[k, : n[k]] = f
    up = lambda x: torch.from_numpy(x).to(dev)
    d_desc, d_n = up(desc), up(np.asarray(n, np.int32))
    d_pa, d_pb = up(np.asarray([p[0] for p in pairs], np.int32)), up(np.asarray([p[1] for p in pairs], np.int32))
    d_out = [torch.full((len(pairs), cap), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    p = lambda t: C.c_void_p(t.data_ptr())
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    m = F.ORBmatcher(0.6, False, lib=lib)
    sync()
    L.check(lib, lib.rgbl_hamming_bf_batch_device(m.h, p(d_desc), p(d_n), cap, p(d_pa), p(d_pb), len(pairs), p(d_out[0]), p(d_out[1]), p(d_out[2])))
    sync()
    got = [t.cpu().numpy() for t in d_out]
    for k, (fa, fb) in enumerate(pairs):
        want = O.hamming_bf(frames[fa], frames[fb])
        for g, w, name in zip(got, want, ("best index", "best distance", "second distance")):
            assert np.array_equal(g[k, : n[fa]], w), "pair %d: %s differs" % (k, name)
        for q, row in (expect or {}).get(k, ()):
            assert want[0][q] == row, (k, q, want[0][q])
    m.close()


# ---- CPU emulation of the kernel sources ----------------------------------------------------------------------------
@pytest.mark.parametrize("na", NA)
def test_emu_shapes(emu_lib, na):
    check_shapes(emu_lib, na)


def test_emu_sweep_boundary(emu_lib):
    check_sweep_boundary(emu_lib)


def test_emu_ties_and_extremes(emu_lib):
    check_ties_and_extremes(emu_lib)


def test_emu_batch_device(emu_lib):
    import torch
    check_batch_device(emu_lib, torch.device("cpu"))


def test_emu_train_set_of_65536_rows_is_refused(emu_lib):
    check_limit_refused(emu_lib)


# ---- the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("na", NA)
def test_gpu_shapes(gpu_lib, na):
    check_shapes(gpu_lib, na)


@pytest.mark.gpu
def test_gpu_sweep_boundary(gpu_lib):
    check_sweep_boundary(gpu_lib)


@pytest.mark.gpu
def test_gpu_ties_and_extremes(gpu_lib):
    check_ties_and_extremes(gpu_lib)


@pytest.mark.gpu
def test_gpu_batch_device(gpu_lib):
    import torch
    check_batch_device(gpu_lib, torch.device("cuda", 0))


@pytest.mark.gpu
def test_gpu_train_set_of_65536_rows_is_refused(gpu_lib):
    check_limit_refused(gpu_lib)
