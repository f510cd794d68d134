"""The two-phase tile pipeline of the FP4 matrix-core scan (k_hamming_fp4), bit for bit against oracle_py.hamming_bf.

A wave tracks its second column tile (queries 32 - 63 of its 64) one phase late: the tile stays in registers across the next
tile's first MFMAs and across the stage barrier, and is drained at the end of a sweep and of the scan; the partial last stage of a
train set is scanned behind the stage loop.  The shapes are the smallest at which that structure can go wrong:

  slots    na = 64, nb = 160 (two full stages and a last stage of one tile): the best match in every row r, the runner-up at
           r +- 1, r +- 32, r +- 64 (the other phase, the other tile of the stage, the other side of the stage barrier), every
           other row far away; once for query 0 (column tile 0), once for query 40 (column tile 1); exact (index, distance, second)
  drained  nb = 32 .. 128 (the last tile full) and 33 .. 127 (the last tile masked), the best match in the last row, query >= 32
  queries  na = 1, 33, 65 against nb = 97: waves without queries, a partial column tile
  sweep    nb = 8192 + 33, a query >= 32, best and runner-up on either side of the sweep boundary
  slices   nb = 2000 through the train-set slices (slices of whole stages, so they end on stage boundaries): best and runner-up in the last row of one
           slice and the first row of the next, query >= 32; and the slot case at this size, reduced: every row of 2000 is minutes on
           the emulator, so the best match sits in the last row of a slice, the first row of the next and one tile further, around
           every cut, and in the last row of the train set, each with all six runner-up offsets (slices on only:
           with them off this size runs the loop that the nb = 160 case covers row by row)
  tiny     nb = 0, 1, 2

Every case goes through ORBmatcher.BruteForce with the train-set slices on (RGBL_BF_SPLIT unset) and off (=0); the batch entry point
(rgbl_hamming_bf_batch_device) gets the slot shape among its pairs.  The same checks run on the CPU emulation of the kernel sources
and, marked gpu, on the device."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F

SWEEP = 8192
STAGE = 64           # train rows per LDS stage of k_hamming_fp4
SLOT_NB = 160
SLOT_OFFSETS = (-64, -32, -1, 1, 32, 64)
SLOT_CHUNKS = 5      # the slot case in chunks of 32 best rows: each a few seconds on the emulator


def _desc(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _two_bits(d):
    """A copy of descriptor d at Hamming distance 2."""
    e = d.copy()
    e[3] ^= 0x21
    return e


class _Matchers:
    """One handle with the train-set slices as built, one with RGBL_BF_SPLIT=0 (the switch is read when the handle is created)."""

    def __init__(self, lib, slices_only=False):
        saved = os.environ.pop("RGBL_BF_SPLIT", None)
        try:
            self.ms = [F.ORBmatcher(0.6, False, lib=lib)]
            if slices_only:
                return
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


def _planted(a, q, nb, best_row, second_row):
    """nb train rows, all at distance 256 from query q except its copy in best_row and a copy two bits away in second_row."""
    t = np.repeat(np.bitwise_not(a[q : q + 1]), nb, 0)
    t[second_row] = _two_bits(a[q])
    t[best_row] = a[q]
    return t


def _slot_pairs(nb, rows):
    for r in rows:
        for s in sorted({min(max(r + o, 0), nb - 1) for o in SLOT_OFFSETS} - {r}):
            yield r, s


def check_slots(lib, nb, rows, slices_only=False):
    ms = _Matchers(lib, slices_only)
    a = _desc(64, 11)
    for q in (0, 40):
        for r, s in _slot_pairs(nb, rows):
            bi, bd, sd = ms.check(a, _planted(a, q, nb, r, s), "slots q=%d best=%d second=%d" % (q, r, s))
            assert (bi[q], bd[q], sd[q]) == (r, 0, 2), (q, r, s)
    ms.close()


def check_drained(lib):
    ms = _Matchers(lib)
    a = _desc(64, 12)
    for nb in (32, 64, 96, 128, 33, 65, 95, 127):
        for q in (32, 47, 63):
            t = _desc(nb, 200 + nb)
            t[nb - 1] = a[q]
            bi, bd, sd = ms.check(a, t, "drained")
            assert (bi[q], bd[q]) == (nb - 1, 0)
        # the runner-up in the tile before the drained one, and the reverse
        if nb > 32:
            for r, s in ((nb - 1, nb - 33), (nb - 33, nb - 1)):
                bi, bd, sd = ms.check(a, _planted(a, 40, nb, r, s), "drained pair")
                assert (bi[40], bd[40], sd[40]) == (r, 0, 2)
    ms.close()


def check_queries(lib):
    ms = _Matchers(lib)
    nb = 97
    for na in (1, 33, 65):
        a = _desc(na, 300 + na)
        t = _desc(nb, 400 + na)
        t[nb - 1] = a[na - 1]            # the last query: best in the last row (the masked tile), runner-up two stages earlier
        t[5] = _two_bits(a[na - 1])
        bi, bd, sd = ms.check(a, t, "queries")
        assert (bi[na - 1], bd[na - 1], sd[na - 1]) == (nb - 1, 0, 2)
    ms.close()


def check_sweep_pending(lib):
    ms = _Matchers(lib)
    a = _desc(64, 13)
    nb = SWEEP + 33
    for q in (32, 40):
        for r, s in ((SWEEP - 1, SWEEP), (SWEEP, SWEEP - 1), (SWEEP - 1, nb - 1), (nb - 1, SWEEP - 1)):
            bi, bd, sd = ms.check(a, _planted(a, q, nb, r, s), "sweep pending")
            assert (bi[q], bd[q], sd[q]) == (r, 0, 2)
    ms.close()


SLICE_NB = 2000
SLICE_CASES = 8  # the 7 cuts between the 8 slices of SLICE_NB rows, and the last tile


def _slice_cuts():
    """First rows of the second to the last slice of SLICE_NB train rows, as rgbl_hamming_bf cuts them for one block of queries."""
    stages = (SLICE_NB + STAGE - 1) // STAGE
    splits = max(1, min(16, stages // 4, 128))
    per = (stages + splits - 1) // splits * STAGE  # train rows per slice
    assert splits > 1 and per * (splits - 1) < SLICE_NB
    assert splits == SLICE_CASES
    return [k * per for k in range(1, splits)]


def check_slices(lib):
    ms = _Matchers(lib)
    a = _desc(64, 14)
    nb = SLICE_NB
    for q in (33, 40):
        cuts = _slice_cuts()
        for cut in (cuts[0], cuts[len(cuts) // 2], cuts[-1]):
            for r, s in ((cut - 1, cut), (cut, cut - 1)):
                bi, bd, sd = ms.check(a, _planted(a, q, nb, r, s), "slices")
                assert (bi[q], bd[q], sd[q]) == (r, 0, 2)
        for r, s in ((nb - 1, nb - 17), (nb - 17, nb - 1), (nb - 1, nb - 33), (0, nb - 1)):   # the masked last tile
            bi, bd, sd = ms.check(a, _planted(a, q, nb, r, s), "slices, last tile")
            assert (bi[q], bd[q], sd[q]) == (r, 0, 2)
    ms.close()


def check_slice_slots(lib, k):
    """The slot case through the slice path, reduced (see the module's docstring): around cut k, or (behind the last cut) the masked last tile."""
    cuts = _slice_cuts()
    rows = (SLICE_NB - 1,) if k == len(cuts) else [cuts[k] + d for d in (-1, 0, 32)]
    check_slots(lib, SLICE_NB, rows, slices_only=True)


def check_tiny(lib):
    ms = _Matchers(lib)
    a = _desc(65, 15)
    bi, bd, sd = ms.check(a, np.zeros((0, 32), np.uint8), "empty")
    assert (bi == -1).all() and (bd == 256).all() and (sd == 256).all()
    bi, bd, sd = ms.check(a, a[40:41].copy(), "one row")
    assert (bi == 0).all() and bd[40] == 0 and (sd == 256).all()
    bi, bd, sd = ms.check(a, np.stack([_two_bits(a[40]), a[40]]), "two rows")
    assert (bi[40], bd[40], sd[40]) == (1, 0, 2)
    ms.close()


def check_batch_device(lib, dev):
    """rgbl_hamming_bf_batch_device (the flagship step's call): the slot shape, a masked last tile and a one-tile train set."""
    import torch
    a = _desc(64, 16)
    frames = [a, _planted(a, 40, SLOT_NB, 127, 128), _planted(a, 40, 97, 96, 63), _planted(a, 40, 32, 31, 0)]
    n = [len(f) for f in frames]
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2))
    cap = 192
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
    for k, (r, s) in enumerate(((127, 128), (96, 63), (31, 0))):
        assert (got[0][k, 40], got[1][k, 40], got[2][k, 40]) == (r, 0, 2)
    m.close()


def _chunk(k):
    return range(k * SLOT_NB // SLOT_CHUNKS, (k + 1) * SLOT_NB // SLOT_CHUNKS)


# ---- CPU emulation of the kernel sources ----------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", range(SLOT_CHUNKS))
def test_emu_slots(emu_lib, chunk):
    check_slots(emu_lib, SLOT_NB, _chunk(chunk))


def test_emu_drained(emu_lib):
    check_drained(emu_lib)


def test_emu_queries(emu_lib):
    check_queries(emu_lib)


def test_emu_sweep_pending(emu_lib):
    check_sweep_pending(emu_lib)


def test_emu_slices(emu_lib):
    check_slices(emu_lib)


@pytest.mark.parametrize("cut", range(SLICE_CASES))
def test_emu_slice_slots(emu_lib, cut):
    check_slice_slots(emu_lib, cut)


def test_emu_tiny(emu_lib):
    check_tiny(emu_lib)


def test_emu_batch_device(emu_lib):
    import torch
    check_batch_device(emu_lib, torch.device("cpu"))


# ---- the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(SLOT_CHUNKS))
def test_gpu_slots(gpu_lib, chunk):
    check_slots(gpu_lib, SLOT_NB, _chunk(chunk))


@pytest.mark.gpu
def test_gpu_drained(gpu_lib):
    check_drained(gpu_lib)


@pytest.mark.gpu
def test_gpu_queries(gpu_lib):
    check_queries(gpu_lib)


@pytest.mark.gpu
def test_gpu_sweep_pending(gpu_lib):
    check_sweep_pending(gpu_lib)


@pytest.mark.gpu
def test_gpu_slices(gpu_lib):
    check_slices(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", range(SLICE_CASES))
def test_gpu_slice_slots(gpu_lib, cut):
    check_slice_slots(gpu_lib, cut)


@pytest.mark.gpu
def test_gpu_tiny(gpu_lib):
    check_tiny(gpu_lib)


@pytest.mark.gpu
def test_gpu_batch_device(gpu_lib):
    import torch
    check_batch_device(gpu_lib, torch.device("cuda", 0))
