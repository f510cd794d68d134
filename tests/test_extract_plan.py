"""The extractor's launch plans order what must be ordered.

The emulator runs every launch synchronously and ignores streams and events, so no other CPU test can see a missing
hipStreamWaitEvent.  extractor.hip writes every schedule down as data (build_plan: launch / record / wait steps on the
main, auxiliary and level stream); the emulation build exports that list (rgbl_test_extract_plan, no kernel runs), and this
test computes happens-before on it - issue order on one stream, plus record -> wait of the same mark - and checks it
against what the kernels read and write (from their arguments in enqueue_extract, per frame):

  k_resize_linear(l)  reads pyramid level l - 1 (level 0 = the caller's image), writes pyramid level l
  k_fast_cells(l)     reads pyramid level l; writes the cell counters / slots / candidate list / level counter of level l
  k_compact_cells(l)  (same step, same stream, behind k_fast_cells) reads the cells' slots, writes the list and its counter
  k_gauss7(l)         reads pyramid level l, writes blurred level l
  k_octree(l)         reads the candidates of level l, writes kp_key / kp_count of level l (node scratch is per level)
  k_orient_brief over the slots of the levels [b, e): reads kp_key, pyramid and blurred level of those levels and kp_count
                      of every level below e (a keypoint's output position is behind the lower levels' keypoints); the
                      launch that writes the frame totals reads kp_count of ALL levels; writes keypoints, descriptors, totals
  k_lapping_permute   reads the keypoints and descriptors of every k_orient_brief launch and the totals, writes the outputs

Hence: resize(l) after resize(l - 1); fast(l) and gauss(l) after resize(l) for l >= 1; octree(l) after fast(l); a
descriptor step over [b, e) after gauss(l), resize(l) of its levels and after octree(j) for every j < e; the totals step after
every octree; the permute after every descriptor step.  Besides: everything on another stream lies between the start and
the end of the call on the main stream, and every mark is recorded once, before every wait for it, and waited for.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from orb_slam3_rgbl_amd import _lib

RESIZE, FAST, GAUSS, OCTREE, DESC, PERMUTE, RECORD, WAIT = range(8)
MAIN, AUX, LVL = range(3)
STEP = np.dtype([("kind", "u1"), ("stream", "u1"), ("mark", "u1"), ("flag", "u1"), ("begin", "<i4"), ("end", "<i4")])
MAX_MARKS = 6
W, H, MAX_BATCH = 1241, 376, 16   # eight levels at scale 1.2 build; max_batch 16 reaches the batch schedules (>= 8 frames)


def _handle(lib, nlevels):
    cfg = _lib.ExtractorCfg(2000, 1.2, nlevels, 20, 7, W, H, MAX_BATCH)
    h = C.c_void_p()
    _lib.check(lib, lib.rgbl_extractor_create(C.byref(cfg), 0, C.byref(h)))
    return h


def _plan(lib, h, batch, timer, lapping):
    fn = lib.rgbl_test_extract_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    buf = np.zeros(256, STEP)
    n = fn(h, batch, timer, lapping, buf.ctypes.data, len(buf))
    assert 0 < n <= len(buf), "no plan, or one that uses more marks than the handle has events"
    return [tuple(int(v) for v in s) for s in buf[:n]]


def check_plan(steps, nlevels, lapping):
    """Raises AssertionError unless `steps` (kind, stream, mark, flag, begin, end) is a complete, correctly ordered plan."""
    L = nlevels
    # nodes: START, the steps (a resize step is one launch per level, in order), END; START / END sit on the main stream
    nodes = [("start", MAIN, None, None)]
    for kind, stream, mark, flag, begin, end in steps:
        assert stream in (MAIN, AUX, LVL) and kind <= WAIT
        if kind in (RECORD, WAIT):
            assert mark < MAX_MARKS
            nodes.append((kind, stream, mark, None))
        elif kind == RESIZE:
            assert 1 <= begin < end <= L
            nodes.extend((RESIZE, stream, (l, l + 1), 0) for l in range(begin, end))
        else:
            assert 0 <= begin < end <= L
            nodes.append((kind, stream, (begin, end), flag))
    nodes.append(("end", MAIN, None, None))
    n = len(nodes)
    # happens-before: the next node of the same stream, and record -> every wait for the mark
    hb = np.zeros((n, n), bool)
    last = {}
    recorded = {}
    waited = set()
    for i, (kind, stream, arg, _) in enumerate(nodes):
        if stream in last:
            hb[last[stream], i] = True
        last[stream] = i
        if kind == RECORD:
            assert arg not in recorded, "mark %d is recorded twice" % arg
            recorded[arg] = i
        elif kind == WAIT:
            assert arg in recorded, "mark %d is waited for before it is recorded" % arg
            assert nodes[recorded[arg]][1] != stream, "a stream waits for its own mark %d" % arg
            hb[recorded[arg], i] = True
            waited.add(arg)
    assert waited == set(recorded), "marks recorded but never waited for: %s" % sorted(set(recorded) - waited)
    for k in range(n):   # transitive closure (edges only point forward in issue order)
        hb |= np.outer(hb[:, k], hb[k, :])

    def launches(kind):
        return [i for i, nd in enumerate(nodes) if nd[0] == kind]

    def of_level(kind, l):
        ids = [i for i in launches(kind) if nodes[i][2][0] <= l < nodes[i][2][1]]
        assert len(ids) == 1, "%d launches of kind %d cover level %d" % (len(ids), kind, l)
        return ids[0]

    def after(a, b, what):
        assert hb[b, a], "%s: step %d %s is not ordered behind step %d %s" % (what, a, nodes[a], b, nodes[b])

    # everything exactly once
    for l in range(L):
        for kind in (FAST, GAUSS, OCTREE, DESC):
            of_level(kind, l)
        if l >= 1:
            of_level(RESIZE, l)
    assert sum(nodes[i][2][1] - nodes[i][2][0] for i in launches(RESIZE)) == L - 1
    totals = [i for i in launches(DESC) if nodes[i][3]]
    assert len(totals) == 1, "the frame totals are written by %d launches" % len(totals)
    assert len(launches(PERMUTE)) == (1 if lapping else 0)
    # data dependences
    for l in range(1, L):
        if l >= 2:
            after(of_level(RESIZE, l), of_level(RESIZE, l - 1), "resize(%d) reads level %d" % (l, l - 1))
        after(of_level(FAST, l), of_level(RESIZE, l), "fast(%d)" % l)
        after(of_level(GAUSS, l), of_level(RESIZE, l), "gauss(%d)" % l)
    for l in range(L):
        after(of_level(OCTREE, l), of_level(FAST, l), "octree(%d)" % l)
    for d in launches(DESC):
        b, e = nodes[d][2]
        for l in range(b, e):
            after(d, of_level(GAUSS, l), "descriptors of level %d read its blurred image" % l)
            if l >= 1:
                after(d, of_level(RESIZE, l), "descriptors of level %d read the level" % l)
        for j in range(L if nodes[d][3] else e):
            after(d, of_level(OCTREE, j), "descriptors of the levels [%d, %d) read the keypoint count of level %d" % (b, e, j))
    for p in launches(PERMUTE):
        assert nodes[p][1] == MAIN
        for d in launches(DESC):
            after(p, d, "the lapping permute reads every descriptor step's output")
    # fork and join: the other streams work between the call's start and its end on the main stream
    for i, nd in enumerate(nodes):
        if nd[1] != MAIN:
            after(i, 0, "a step on another stream may run before the call's start on the main stream")
            after(n - 1, i, "a step on another stream is still running when the main stream is done")


CASES = list(itertools.product((1, 2, 5, 6, 8), (None, "0", "3"), (None, "0"), ("0", "1"), (0, 1), (1, 4, 8, 16)))


@pytest.mark.parametrize("nlevels,split_pyr,level_split,compact,timer,batch", CASES)
def test_plan_orders_reads_behind_writes(emu_lib, monkeypatch, nlevels, split_pyr, level_split, compact, timer, batch):
    for name, value in (("RGBL_SPLIT_PYR", split_pyr), ("RGBL_LEVEL_SPLIT", level_split), ("RGBL_COMPACT", compact)):
        monkeypatch.delenv(name, raising=False)
        if value is not None:
            monkeypatch.setenv(name, value)
    h = _handle(emu_lib, nlevels)   # the switches are read here
    try:
        for lapping in (0, 1):
            steps = _plan(emu_lib, h, batch, timer, lapping)
            check_plan(steps, nlevels, lapping)
            streams = {s[1] for s in steps}
            if timer:
                assert streams == {MAIN}, "per-kernel timing keeps everything on one stream"
            elif nlevels == 8 and batch >= 8:
                assert streams == {MAIN, AUX}
            elif nlevels == 8 and level_split is None:
                assert streams == {MAIN, AUX, LVL}
    finally:
        emu_lib.rgbl_extractor_destroy(h)


@pytest.mark.parametrize("batch,level_split", [(16, None), (1, None), (1, "0")])
def test_checker_catches_a_dropped_wait(emu_lib, monkeypatch, batch, level_split):
    """The check above bites: without any one of its waits a schedule fails it - except for the one wait per schedule that a
    later wait of the same stream covers (level 0's mark is recorded on the auxiliary stream in front of the blurred levels')."""
    for name in ("RGBL_SPLIT_PYR", "RGBL_LEVEL_SPLIT", "RGBL_COMPACT"):
        monkeypatch.delenv(name, raising=False)
    if level_split is not None:
        monkeypatch.setenv("RGBL_LEVEL_SPLIT", level_split)
    h = _handle(emu_lib, 8)
    try:
        steps = _plan(emu_lib, h, batch, 0, 1)
    finally:
        emu_lib.rgbl_extractor_destroy(h)
    check_plan(steps, 8, 1)
    waits = [i for i, s in enumerate(steps) if s[0] == WAIT]
    caught = 0
    for i in waits:
        try:
            check_plan(steps[:i] + steps[i + 1:], 8, 1)
        except AssertionError:
            caught += 1
    assert len(waits) >= 4 and caught >= len(waits) - 1
    # a launch moved in front of the wait it needs is caught as well: the last wait of the main stream behind the step after it
    i = max(i for i in waits if steps[i][1] == MAIN)
    with pytest.raises(AssertionError):
        check_plan(steps[:i] + [steps[i + 1], steps[i]] + steps[i + 2:], 8, 1)
