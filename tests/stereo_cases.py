"""Directed cases for Frame::ComputeStereoMatches (k_stereo_match / k_stereo_filter, rgbl_stereo_matches and
rgbl_stereo_matches_batch_device): keypoint sets BUILT by the test, matched on the resident pyramids of a small rectified pair and
compared bit for bit (uRight and depth as uint32) with oracle_py.stereo_matches.  The ABI takes keypoints and descriptors from the
caller and reads only the two pyramids, so one small extraction per extractor makes any keypoint set matchable: right tiles beyond
the first (Nr > 2048), the filter's tail (N > 2048), ties, exact gate boundaries, SAD windows on the image border - none of which an
extraction's own keypoints reach.  Every case also asserts, on the ORACLE's output alone, that it reached what it aims at.

Functions take (lib, dev) like parity_checks.check_pipeline_gather: the emulator (torch.device("cpu")) and the card run the same cases.
Every keypoint stays inside the image, 0 <= (int)y < H (the oracle indexes its row table unchecked, as the reference does)."""
import ctypes as C

import numpy as np

import parity_checks as pc
from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import synth

W, H, LEVELS = 384, 160, 5
BANDS = (2, 12, 25)              # disparity of the three row bands of the main pair: right[y, x] = left[y, x + BANDS[3 y / H]]
KITTI = (0.54, 386.1448)         # mb, mbf: maxD = 715 px, every u to the left of the keypoint is inside the window
NAN_BITS = 0x7fc00123            # what the output buffers hold before a call


def band_of(y):
    return min(int(y) * 3 // H, 2)


def band_pair(seq, frame=0, noise=1.0):
    full = synth.Sequence(seq, W + 128, H, n_frames=frame + 1).frame(frame).astype(np.int32)
    left = full[:, 64:64 + W]
    right = np.empty_like(left)
    for y in range(H):
        d = BANDS[band_of(y)]
        right[y] = full[y, 64 + d:64 + d + W]
    rng = np.random.default_rng(seq * 77 + frame)
    right = np.clip(right + np.rint(noise * rng.standard_normal(right.shape)).astype(np.int32), 0, 255)
    return np.ascontiguousarray(left.astype(np.uint8)), np.ascontiguousarray(right.astype(np.uint8))


SYM_C, SYM_HALF = 192, 30


def symmetric_pair(seq=5):
    """left mirror-symmetric about column SYM_C within +-SYM_HALF; right = left there, left + noise elsewhere (true disparity 0)."""
    left = synth.Sequence(seq, W, H, n_frames=1).frame(0).copy()
    for a in range(1, SYM_HALF + 1):
        left[:, SYM_C + a] = left[:, SYM_C - a]
    rng = np.random.default_rng(seq + 1)
    noise = np.rint(1.5 * rng.standard_normal(left.shape)).astype(np.int32)
    noise[:, SYM_C - SYM_HALF:SYM_C + SYM_HALF + 1] = 0
    return left, np.clip(left.astype(np.int32) + noise, 0, 255).astype(np.uint8)


DELTA_D = 7
GRID = [(48 + 32 * i, 20 + 24 * j) for j in range(6) for i in range(10)]   # 11 x 11 windows (21 wide on the right) that do not overlap
DELTAS = [0] * 4 + [10] * 8 + [20] * 8 + [21, 22, 41, 42, 43, 44, 50, 55, 5, 15, 30, 60]
DELTAS += [7] * (len(GRID) - len(DELTAS))


def delta_pair(seq=9):
    """right[y, x] = left[y, x + DELTA_D] exactly, then ONE pixel per grid point moved by DELTAS[k]: an octave-0 keypoint on grid point k
    matched to (x - DELTA_D, y) has SAD == DELTAS[k] at the true shift, so the filter's inputs are known exactly."""
    full = synth.Sequence(seq, W + 128, H, n_frames=1).frame(0)
    left = np.ascontiguousarray(full[:, 64:64 + W])
    right = np.ascontiguousarray(full[:, 64 + DELTA_D:64 + DELTA_D + W])
    for (x, y), d in zip(GRID, DELTAS):
        p = int(right[y, x - DELTA_D])
        right[y, x - DELTA_D] = p + d if p + d <= 255 else p - d
    return left, right


class Rig:
    """Two extractors (and two oracle extractors per frame) that hold the pyramids of a pair, or of a batch of pairs."""

    def __init__(self, lib, lefts, rights, nfeatures=1000, levels=LEVELS, extract=True):
        self.lib = lib
        lefts, rights = np.asarray(lefts), np.asarray(rights)
        self.batch = lefts.shape[0] if lefts.ndim == 3 else 0
        h, w = lefts.shape[-2:]
        args = (nfeatures, 1.2, levels, 20, 7)
        self.exl = F.ORBextractor(*args, w, h, max_batch=max(self.batch, 1), lib=lib)
        self.exr = F.ORBextractor(*args, w, h, max_batch=max(self.batch, 1), lib=lib)
        self.levels = levels
        self._good = {}
        self.scale = self.exl.mvScaleFactor.copy()
        self.inv = self.exl.mvInvScaleFactor.copy()
        self.size = [self.exl.level_size(l) for l in range(levels)]
        if not extract:
            return
        ls, rs = (lefts, rights) if self.batch else (lefts[None], rights[None])
        self.ol = [O.Extractor(*args) for _ in ls]
        self.orr = [O.Extractor(*args) for _ in ls]
        want = [o(im)[:2] for o, im in zip(self.ol, ls)]
        for o, im in zip(self.orr, rs):
            o(im)
        got = [r[:2] for r in self.exl.extract_batch(lefts)] if self.batch else [self.exl(lefts)[:2]]
        if self.batch:
            self.exr.extract_batch(rights)
        else:
            self.exr(rights)
        for (k, d), (ok, od) in zip(got, want):
            pc.assert_keypoints_equal(k, ok, "left")
            assert np.array_equal(d, od)
        self.kps = [k for k, _ in want]     # the real left keypoints: textured places with real descriptors
        self.desc = [d for _, d in want]

    def match(self, kl, dl, kr, dr, mb=KITTI[0], mbf=KITTI[1], what=""):
        """host-pointer call == oracle (frame 0); returns the oracle's (uRight, depth)"""
        ur, dp = F.ComputeStereoMatches(self.exl, self.exr, kl, dl, kr, dr, mb, mbf)
        our, odp = O.stereo_matches(self.ol[0], self.orr[0], kl, dl, kr, dr, mb, mbf)
        assert np.array_equal(pc.bits(ur), pc.bits(our)), "%s: mvuRight differs at %s" % (what, np.flatnonzero(pc.bits(ur) != pc.bits(our))[:8])
        assert np.array_equal(pc.bits(dp), pc.bits(odp)), "%s: mvDepth differs at %s" % (what, np.flatnonzero(pc.bits(dp) != pc.bits(odp))[:8])
        return our, odp

    def good(self, frame=0, octave=None, band=None, steady=True):
        """real left keypoints whose SAD window lies inside one disparity band, whose true match is well inside the level and whose
        (steady: for cases with several matches) SADs at the true match lie within a factor 1.9 of each other: in any subset of
        them the median cut (2.1 x median) keeps them all"""
        if frame not in self._good:
            self._good[frame] = self._find_good(frame)
        idx, octv, bnd, calm = self._good[frame]
        keep = calm.copy() if steady else np.ones(len(idx), bool)
        if octave is not None:
            keep &= octv == octave
        if band is not None:
            keep &= bnd == band
        assert keep.any(), "no usable left keypoint at octave %s in band %s (broken case)" % (octave, band)
        return idx[keep]

    def pick(self, octave, band):
        """one left keypoint of `octave` inside `band`: a real one, or (the coarse levels keep 19 level pixels from the border, which
        leaves none in the outer bands) a real one moved to the middle row of the band"""
        idx, octv, bnd, _ = self._good.get(0) or self._good.setdefault(0, self._find_good(0))
        both = idx[(octv == octave) & (bnd == band)]
        i = both[0] if len(both) else self.good(octave=octave, steady=False)[0]
        k = self.kps[0][i].copy()
        if not len(both):
            k["y"] = H * (band + 0.5) / 3.0
        return k, self.desc[0][i]

    def _find_good(self, frame):
        k = self.kps[frame]
        out = []
        for i in range(len(k)):
            s = self.scale[k["octave"][i]]
            b = band_of(k["y"][i])
            lo, hi = H * b / 3.0, H * (b + 1) / 3.0
            if k["y"][i] - 7 * s < lo or k["y"][i] + 7 * s > hi:
                continue
            xr = (k["x"][i] - BANDS[b]) / s
            if xr < 16 or xr > self.size[k["octave"][i]][0] - 28:
                continue
            out.append(i)
        out = np.array(out, np.int64)
        # the SAD the true match will have (only to CHOOSE inputs: the windows of these keypoints lie inside their levels)
        lv = [(self.ol[frame].level_image(l).astype(np.int32), self.orr[frame].level_image(l).astype(np.int32)) for l in range(self.levels)]
        sad = []
        for i in out:
            o = k["octave"][i]
            xl, yl = int(np.round(k["x"][i] * self.inv[o])), int(np.round(k["y"][i] * self.inv[o]))
            xr = int(np.round(np.float32(k["x"][i] - BANDS[band_of(k["y"][i])]) * self.inv[o]))
            a = lv[o][0][yl - 5:yl + 6, xl - 5:xl + 6]
            sad.append(min(int(np.abs(a - lv[o][1][yl - 5:yl + 6, xr + inc - 5:xr + inc + 6]).sum()) for inc in range(-5, 6)))
        sad = np.array(sad)
        srt = np.sort(sad)
        lo = srt[int(np.argmax([np.searchsorted(srt, 1.9 * v) - j for j, v in enumerate(srt)]))]
        calm = (sad >= lo) & (sad < 1.9 * lo)
        assert len(set(k["octave"][out[calm]])) >= 2 and calm.sum() > 20
        return out, k["octave"][out], np.array([band_of(y) for y in k["y"][out]]), calm


_RIGS = {}


def rig(lib, name):
    """one extraction per extractor and session: the cases share the resident pyramids and leave them unchanged"""
    key = (id(lib), name)
    if key not in _RIGS:
        if name == "bands":
            _RIGS[key] = Rig(lib, *band_pair(61))
        elif name == "symmetric":
            _RIGS[key] = Rig(lib, *symmetric_pair())
        elif name == "delta":
            _RIGS[key] = Rig(lib, *delta_pair())
        elif name == "single":      # re-extracts the frames of the batch one by one for the host-pointer call
            _RIGS[key] = Rig(lib, np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), extract=False)
        elif name == "batch":
            pairs = [band_pair(62 + f, noise=1.0) for f in range(5)]
            _RIGS[key] = Rig(lib, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
            _RIGS[key].images = pairs
    return _RIGS[key]


# ---- building keypoint sets ------------------------------------------------------------------------------------------
def make_kps(x, y, octave):
    x = np.atleast_1d(np.asarray(x, np.float32))
    k = np.zeros(len(x), L.KP_DTYPE)
    k["x"], k["y"], k["octave"] = x, np.asarray(y, np.float32), np.asarray(octave, np.int32)
    k["size"], k["angle"], k["response"], k["class_id"] = 31.0, 0.0, 1.0, -1
    return k


def flipped(desc, bits, start=0):
    """`desc` with the `bits` bits from bit `start` on flipped: Hamming distance exactly `bits`"""
    b = np.unpackbits(np.asarray(desc, np.uint8))
    idx = (start + np.arange(bits)) % 256
    b[idx] ^= 1
    return np.packbits(b)


def filler(r, kL, dL, kind, rng, max_d=None):
    """a right keypoint that fails exactly ONE gate for left keypoint kL and would win it at distance 0 (or, kind 3, is too far)"""
    o = int(kL["octave"])
    x, y = float(kL["x"]) - BANDS[band_of(kL["y"])], float(kL["y"])
    desc = dL
    if kind == 0:      # row band
        off = 2.0 * float(r.scale[o]) + 2.0 + float(rng.integers(0, 4))
        y = y + off if y + off < H - 1 else y - off
    elif kind == 1:    # octave +-2
        o = o + 2 if o + 2 < r.levels else o - 2
    elif kind == 2:    # u outside [minU, maxU]
        x = float(kL["x"]) + 1.0 + float(rng.integers(0, 10)) if max_d is None or rng.integers(0, 2) else float(kL["x"]) - max_d - 1.0 - float(rng.integers(0, 10))
    else:              # descriptor distance >= 100
        desc = flipped(dL, int(rng.integers(100, 200)), int(rng.integers(0, 256)))
    return make_kps(x, y, o)[0], desc


def right_set(r, kl, dl, n_right, placed, rng, max_d=None, kinds=(0, 1, 2, 3)):
    """`placed`: index -> (iL, dx, bits[, start[, doct[, y]]]): the right keypoint of left keypoint iL at true disparity + dx (level-0 px),
    its descriptor with `bits` bits flipped; every other index holds a filler aimed at some left keypoint."""
    kr = np.zeros(n_right, L.KP_DTYPE)
    dr = np.zeros((n_right, 32), np.uint8)
    for j in range(n_right):
        if j in placed:
            v = tuple(placed[j])
            iL, dx, bits, start, doct, y = v + (0, 0, None)[len(v) - 3:]
            x = float(kl["x"][iL]) - BANDS[band_of(kl["y"][iL])] + dx
            kr[j] = make_kps(x, kl["y"][iL] if y is None else y, int(kl["octave"][iL]) + doct)[0]
            dr[j] = flipped(dl[iL], bits, start)
        else:
            iL = int(rng.integers(0, len(kl)))
            kr[j], dr[j] = filler(r, kl[iL], dl[iL], kinds[j % len(kinds)], rng, max_d)
    return kr, dr


def lefts_from(r, idx, n, frame=0):
    """n left keypoints: the real ones `idx`, repeated as often as needed"""
    idx = np.resize(idx, n)
    return r.kps[frame][idx].copy(), r.desc[frame][idx].copy()


def assert_matched(r, kl, kr, our, odp, iL, jR, what=""):
    s = float(r.scale[kl["octave"][iL]])
    assert odp[iL] > 0, "%s: left %d has no depth in the oracle's output (broken case)" % (what, iL)
    assert abs(float(our[iL]) - float(kr["x"][jR])) <= 6.0 * s, "%s: left %d was not matched to right %d (broken case)" % (what, iL, jR)


def candidates(r, kL, kr, mb, mbf):
    """the cheap gates of the reference, restated only to COUNT candidates in a case's reach assertion"""
    max_d = np.float32(mbf) / np.float32(mb)
    rr = (np.float32(2.0) * r.scale[kr["octave"]]).astype(np.float32)
    row = int(kL["y"])
    band = (np.floor(kr["y"] - rr) <= row) & (row <= np.ceil(kr["y"] + rr))
    octv = np.abs(kr["octave"] - int(kL["octave"])) <= 1
    u = (kr["x"] >= np.float32(kL["x"]) - max_d) & (kr["x"] <= np.float32(kL["x"]))
    return band & octv & u


def intended_indices(n_right, n):
    """where the intended matches sit: last valid index, index 0, both sides of every tile boundary, one index per lane, ..."""
    want = [n_right - 1, 0, 2047, 2048, 4095, 4096, 32 + 5, 64 + 5, 96 + 5, 5, 128 + 7, 2048 + 37, 2048 + 69, 4096 + 101, 6143, 6144, 1000, 3000, 5000]
    out = []
    for j in want + list(range(1, n_right, 97)) + list(range(min(n_right, n))):
        if 0 <= j < n_right and j not in out:
            out.append(j)
    return out[:n]


# ---- tiles and groups -------------------------------------------------------------------------------------------------
def case_tiles(lib, dev, n_left, n_right):
    r = rig(lib, "bands")
    rng = np.random.default_rng(1000 * n_left + n_right)
    kl, dl = lefts_from(r, rng.permutation(r.good()), n_left)
    # the first 19 left keypoints (all distinct) own one intended match each, at most 8 bits away: distinct real keypoints are further apart
    idx = intended_indices(n_right, min(n_left, 19))
    placed = {j: (k, 0.0, int(rng.integers(0, 9)), int(rng.integers(0, 256))) for k, j in enumerate(idx)}
    kr, dr = right_set(r, kl, dl, n_right, placed, rng)
    our, odp = r.match(kl, dl, kr, dr, what="tiles %d x %d" % (n_left, n_right))
    for j, p in placed.items():
        assert_matched(r, kl, kr, our, odp, p[0], j, "tiles %d x %d" % (n_left, n_right))
    return len(placed)


# ---- ties: the lowest right index wins --------------------------------------------------------------------------------
TIES = {"two_lanes": (200, (37, 69)), "three_lanes": (200, (37, 69, 101)), "same_lane": (200, (37, 38)), "two_tiles": (2100, (37, 2048 + 37)),
        "second_flush_same_lane": (200, (3, 130)), "later_flushed_lower_index": (200, (40, 130))}


def case_ties(lib, dev, name):
    n_right, tied = TIES[name]
    r = rig(lib, "bands")
    rng = np.random.default_rng(len(name))
    g = r.good()
    kl, dl = lefts_from(r, g[[0, len(g) // 2, len(g) - 1, 5, 9]], 5)   # left 0 carries the tie, four plain matches beside it
    s = float(r.scale[kl["octave"][0]])
    placed = {tied[0]: (0, 0.0, 10, 0)}
    for k, j in enumerate(tied[1:]):          # same distance through OTHER bits, more than 12 s away in u
        placed[j] = (0, -(14.0 + 14.0 * k) * s, 10, 10 * (k + 1))
    if name in ("second_flush_same_lane", "later_flushed_lower_index"):
        for j in range(16):                   # lane 0 flushes a full batch of poor candidates before it meets index 130
            if j not in placed:
                placed[j] = (0, -40.0 - j, 90, 30)
    for k in range(1, 5):
        placed[150 + k] = (k, 0.0, 5, 0)
    kr, dr = right_set(r, kl, dl, n_right, placed, rng)
    c = candidates(r, kl[0], kr, *KITTI)
    assert c[list(tied)].all() and (name not in ("second_flush_same_lane", "later_flushed_lower_index") or c[:16].all())
    our, odp = r.match(kl, dl, kr, dr, what=name)
    assert_matched(r, kl, kr, our, odp, 0, tied[0], name)
    for j in tied[1:]:
        assert abs(float(our[0]) - float(kr["x"][j])) > 6.0 * s, "%s: uRight cannot tell the tied keypoints apart (broken case)" % name
    return 1


# ---- flush: exact candidate counts of one lane ------------------------------------------------------------------------
def case_flush(lib, dev, n_cand, lane=1):
    r = rig(lib, "bands")
    rng = np.random.default_rng(n_cand)
    kl, dl = lefts_from(r, r.good(octave=0, band=1, steady=False)[:1], 1)
    mine = [j for j in range(400) if (j // 32) % 4 == lane][:n_cand]
    placed = {j: (0, -20.0 - (k % 30), 80 + k % 19, k) for k, j in enumerate(mine)}
    placed[mine[-1]] = (0, 0.0, 7, 0)       # the last candidate is the match: the 16th ends a batch, the 17th starts the next one
    kr, dr = right_set(r, kl, dl, 400, placed, rng, kinds=(0, 1, 2))   # (a filler that is only too far in Hamming distance IS a candidate)
    c = candidates(r, kl[0], kr, *KITTI)
    assert int(c.sum()) == n_cand and c[mine].all(), "lane %d holds %d candidates, wanted %d (broken case)" % (lane, int(c.sum()), n_cand)
    our, odp = r.match(kl, dl, kr, dr, what="flush %d" % n_cand)
    assert_matched(r, kl, kr, our, odp, 0, mine[-1], "flush %d" % n_cand)
    return n_cand


def case_flush_everything(lib, dev, n_right=2049):
    """every right keypoint is a candidate; the match is the lone keypoint of the second tile"""
    r = rig(lib, "bands")
    kl, dl = lefts_from(r, r.good(octave=0, band=1, steady=False)[:1], 1)
    placed = {j: (0, -20.0 - (j % 30), 80 + j % 19, j) for j in range(n_right)}
    placed[n_right - 1] = (0, 0.0, 7, 0)
    kr, dr = right_set(r, kl, dl, n_right, placed, np.random.default_rng(0))
    assert candidates(r, kl[0], kr, *KITTI).all()
    our, odp = r.match(kl, dl, kr, dr, what="all candidates")
    assert_matched(r, kl, kr, our, odp, 0, n_right - 1, "all candidates")
    # and with the match in the first tile: the best of 2048 candidates must survive a second tile of one poor candidate
    placed[n_right - 1], placed[1234] = placed[1234], placed[n_right - 1]
    kr, dr = right_set(r, kl, dl, n_right, placed, np.random.default_rng(0))
    our, odp = r.match(kl, dl, kr, dr, what="all candidates, match in tile 0")
    assert_matched(r, kl, kr, our, odp, 0, 1234, "all candidates, match in tile 0")
    return n_right


# ---- gates at equality ------------------------------------------------------------------------------------------------
def probe(r, kL, dL, kR, dR, mb=KITTI[0], mbf=KITTI[1], what=""):
    """one left against one right keypoint: True when the oracle accepts the match"""
    kl, kr = np.array([kL], L.KP_DTYPE), np.array([kR], L.KP_DTYPE)
    our, odp = r.match(kl, np.asarray(dL, np.uint8).reshape(1, 32), kr, np.asarray(dR, np.uint8).reshape(1, 32), mb, mbf, what)
    return bool(odp[0] > 0)


def true_right(r, kL, dx=0.0, y=None, octave=None):
    return make_kps(float(kL["x"]) - BANDS[band_of(kL["y"])] + dx, kL["y"] if y is None else y, kL["octave"] if octave is None else octave)[0]


def case_gate_rows(lib, dev):
    r = rig(lib, "bands")
    f32 = np.float32
    n = 0
    for o in (0, 1, LEVELS - 1):
        i = r.good(octave=o, steady=False)[0]
        kL, dL = r.kps[0][i], r.desc[0][i]
        rr, row = f32(2.0) * r.scale[o], int(kL["y"])
        ys = []
        for y0 in (f32(kL["y"] + rr), f32(kL["y"] - rr)):    # exactly y_L +- 2 s, one ulp either side
            ys += [y0, np.nextafter(y0, f32(np.inf)), np.nextafter(y0, f32(-np.inf))]
        y = f32(row + 1 + rr)                                # the largest y whose band still starts on the row, and its neighbour
        while np.floor(f32(y - rr)) > row:
            y = np.nextafter(y, f32(-np.inf))
        while np.floor(f32(np.nextafter(y, f32(np.inf)) - rr)) <= row:
            y = np.nextafter(y, f32(np.inf))
        ys += [y, np.nextafter(y, f32(np.inf))]
        y = f32(row - 1 - rr)                                # the same at the band's upper end
        while np.ceil(f32(y + rr)) < row:
            y = np.nextafter(y, f32(np.inf))
        while np.ceil(f32(np.nextafter(y, f32(-np.inf)) + rr)) >= row:
            y = np.nextafter(y, f32(-np.inf))
        ys += [y, np.nextafter(y, f32(-np.inf))]
        seen = set()
        for y in ys:
            want = bool(np.floor(f32(y - rr)) <= row <= np.ceil(f32(y + rr)))
            got = probe(r, kL, dL, true_right(r, kL, y=y), flipped(dL, 3), what="row gate, octave %d, y %r" % (o, y))
            assert got == want, "row gate, octave %d, y %r: the oracle %s the match (broken case)" % (o, y, "accepts" if got else "refuses")
            seen.add(want)
            n += 1
        assert seen == {True, False}
    # bands clipped at row 0 and at H - 1
    for y_left, y_right, want in ((0.3, 1.7, True), (0.3, 0.0, True), (0.9, 3.5, False), (H - 0.5, H - 2.5, True), (H - 0.5, H - 0.25, True), (H - 0.5, H - 4.25, False)):
        i = r.good(octave=0, band=0 if y_left < 5 else 2, steady=False)[0]
        kL, dL = r.kps[0][i].copy(), r.desc[0][i]
        kL["y"] = y_left
        got = probe(r, kL, dL, true_right(r, kL, y=y_right), dL, what="clipped band %g / %g" % (y_left, y_right))
        assert got == want, "clipped band %g / %g (broken case)" % (y_left, y_right)
        n += 1
    return n


def case_gate_octaves(lib, dev):
    r = rig(lib, "bands")
    n = 0
    for o, probes in ((0, ((0, True), (1, True), (2, False))), (LEVELS - 1, ((LEVELS - 1, True), (LEVELS - 2, True), (LEVELS - 3, False))),
                      (2, ((0, False), (1, True), (3, True), (4, False)))):
        i = r.good(octave=o, steady=False)[0]
        kL, dL = r.kps[0][i], r.desc[0][i]
        for octr, want in probes:
            got = probe(r, kL, dL, true_right(r, kL, octave=octr), dL, what="octave gate %d / %d" % (o, octr))
            assert got == want, "octave gate %d / %d (broken case)" % (o, octr)
            n += 1
    return n


def case_gate_u(lib, dev):
    """uR == minU and uR == maxU are inside, one ulp beyond is outside; mbf / mb = 14 px exactly"""
    r = rig(lib, "bands")
    f32 = np.float32
    n = 0
    for o in (0, 1):
        i = r.good(octave=o, band=1, steady=False)[0]       # true disparity 12: a right keypoint AT minU = uL - 14 is refined back by two pixels
        kL, dL = r.kps[0][i], r.desc[0][i]
        min_u = f32(kL["x"]) - f32(14.0) / f32(1.0)
        for x, want in ((min_u, True), (np.nextafter(min_u, f32(-np.inf)), False), (np.nextafter(min_u, f32(np.inf)), True)):
            got = probe(r, kL, dL, make_kps(x, kL["y"], o)[0], dL, 1.0, 14.0, "minU, octave %d" % o)
            assert got == want, "minU gate, octave %d, u %r (broken case)" % (o, x)
        i = r.good(octave=o, band=0, steady=False)[0]       # true disparity 2: a right keypoint AT maxU = uL
        kL, dL = r.kps[0][i], r.desc[0][i]
        max_u = f32(kL["x"])
        for x, want in ((max_u, True), (np.nextafter(max_u, f32(np.inf)), False), (np.nextafter(max_u, f32(-np.inf)), True)):
            got = probe(r, kL, dL, make_kps(x, kL["y"], o)[0], dL, 1.0, 14.0, "maxU, octave %d" % o)
            assert got == want, "maxU gate, octave %d, u %r (broken case)" % (o, x)
        n += 6
    return n


def case_gate_distance(lib, dev):
    r = rig(lib, "bands")
    i = r.good(octave=1, steady=False)[0]
    kL, dL = r.kps[0][i], r.desc[0][i]
    for bits, want in ((0, True), (74, True), (75, False), (99, False), (100, False), (256, False)):
        got = probe(r, kL, dL, true_right(r, kL), flipped(dL, bits, 17), what="distance %d" % bits)
        assert got == want, "distance %d (broken case)" % bits
    return 6


# ---- SAD window -------------------------------------------------------------------------------------------------------
def level_x(r, t, o):
    """a level-0 coordinate that rounds to column t of level o"""
    x = np.float32(t * float(r.scale[o]))
    assert np.round(x * r.inv[o]) == t
    return x


def case_sad_right_border(lib, dev):
    """right keypoint at level-x = g.w - 11 (endu == cols: refused), g.w - 12 and g.w - 13 (slow path, inside the image), g.w - 14 (first fast one)"""
    r = rig(lib, "bands")
    n = 0
    for o in (0, 1, LEVELS - 1):
        gw = r.size[o][0]
        k0, dL = r.pick(o, 0)
        for t, want in ((gw - 11, False), (gw - 12, True), (gw - 13, True), (gw - 14, True), (gw - 15, True)):
            kL = k0.copy()
            xr = level_x(r, t, o)
            kL["x"] = xr + BANDS[0]
            got = probe(r, kL, dL, make_kps(xr, kL["y"], o)[0], dL, what="right border, octave %d, column %d" % (o, t))
            assert got == want, "right keypoint at column g.w - %d of octave %d (broken case)" % (gw - t, o)
            n += 1
    return n


def case_sad_left_border(lib, dev):
    """right keypoint at level-x < 10 (xr0 < 0) and left keypoint at level-x < 5 (xl0 < 0): reflected columns"""
    r = rig(lib, "bands")
    n = 0
    for o in (0, 1, LEVELS - 1):
        k0, dL = r.pick(o, 0)
        for t in (0, 1, 4, 9, 10):
            kL = k0.copy()
            xr = level_x(r, t, o)
            kL["x"] = xr + BANDS[0]
            assert probe(r, kL, dL, make_kps(xr, kL["y"], o)[0], dL, what="left border, octave %d, column %d" % (o, t)), "right keypoint at column %d of octave %d (broken case)" % (t, o)
            n += 1
        for t in (3, 4, 5):   # the left keypoint itself next to the border; its match two pixels further left
            kL = k0.copy()
            kL["x"] = level_x(r, t, o)
            assert probe(r, kL, dL, true_right(r, kL), dL, what="left keypoint at column %d, octave %d" % (t, o)), "left keypoint at column %d of octave %d (broken case)" % (t, o)
            n += 1
    return n


def case_sad_rows(lib, dev):
    """left keypoints at level-y < 5 and > g.h - 6: reflected rows on both pyramids"""
    r = rig(lib, "bands")
    n = 0
    for o in (0, 1, LEVELS - 1):
        gh = r.size[o][1]
        for t in (0, 2, 4, 5, gh - 7, gh - 6, gh - 5, gh - 3, gh - 1):
            y = np.float32(t * float(r.scale[o]))
            assert np.round(y * r.inv[o]) == t and 0 <= int(y) < H
            kL, dL = r.pick(o, 0 if t < 6 else 2)
            kL["y"] = y
            assert probe(r, kL, dL, true_right(r, kL), dL, what="row %d of octave %d" % (t, o)), "left keypoint at row %d of octave %d (broken case)" % (t, o)
            n += 1
    return n


def case_sad_bestinc(lib, dev):
    """a right keypoint five level pixels off the true match puts the best shift on the window's end: refused; four is refined"""
    r = rig(lib, "bands")
    n = 0
    for o in (0, 1):
        i = r.good(octave=o, band=1, steady=False)[0]
        kL, dL = r.kps[0][i], r.desc[0][i]
        s = float(r.scale[o])
        # (the true shift is fractional on level 1: no stated expectation next to the window's end there)
        for off, want in ((-6, False), (-5, False), (-4, True), (-3, True), (0, True), (3, True), (4, True), (5, False), (6, False)) if o == 0 else \
                ((-7, False), (-3, True), (0, True), (3, True), (7, False)):
            got = probe(r, kL, dL, true_right(r, kL, dx=off * s), dL, what="bestinc %+d, octave %d" % (off, o))
            assert got == want, "right keypoint %+d level pixels off, octave %d (broken case)" % (off, o)
            n += 1
    return n


# ---- zero disparity ---------------------------------------------------------------------------------------------------
def case_zero_disparity(lib, dev):
    r = rig(lib, "symmetric")
    rng = np.random.default_rng(3)
    ys = (30, 60, 90, 120)
    kz = make_kps([SYM_C] * len(ys), ys, [0] * len(ys))
    dz = rng.integers(0, 256, (len(ys), 32)).astype(np.uint8)
    # alone: every SAD is 0, the median is 0, thDist is 0 and everything is cut, as in the reference
    our, odp = r.match(kz, dz, kz, dz, what="zero disparity alone")
    assert (odp == -1).all() and (our == -1).all()
    # among matches with SAD > 0 (real keypoints outside the noise-free strip, true disparity 0) they survive
    k = r.kps[0]
    far = np.flatnonzero(np.abs(k["x"] - SYM_C) > SYM_HALF + 12 * r.scale[k["octave"]] + 8)[:120]
    kl = np.concatenate([kz, k[far]])
    dl = np.concatenate([dz, r.desc[0][far]])
    our, odp = r.match(kl, dl, kl.copy(), dl.copy(), what="zero disparity")
    nz = len(ys)
    assert (our[:nz] == np.float32(np.float64(np.float32(SYM_C)) - 0.01)).all(), "disparity <= 0 branch not taken (broken case)"
    assert (odp[:nz] == np.float32(KITTI[1]) / np.float32(0.01)).all()
    assert int((odp[nz:] > 0).sum()) > 2 * nz, "too few matches with SAD > 0 (broken case)"
    return nz


# ---- filter -----------------------------------------------------------------------------------------------------------
def delta_sets(r, values):
    """left keypoints on grid points with the SADs `values` (None = a keypoint without any candidate) and their right keypoints"""
    by = {}
    for k, d in enumerate(DELTAS):
        by.setdefault(d, []).append(k)
    used, pts = {}, []
    for v in values:
        if v is None:
            pts.append(-1)
            continue
        k = by[v][used.get(v, 0) % len(by[v])]
        used[v] = used.get(v, 0) + 1
        pts.append(k)
    gd = np.random.default_rng(77).integers(0, 256, (len(GRID), 32)).astype(np.uint8)
    pts = np.array(pts)
    kl = make_kps([GRID[max(k, 0)][0] for k in pts], [GRID[max(k, 0)][1] for k in pts], np.zeros(len(pts), np.int32))
    dl = gd[np.maximum(pts, 0)]
    dl[pts < 0] = ~dl[pts < 0]                       # 256 bits from its grid point's right keypoint
    g = sorted(set(int(k) for k in pts if k >= 0))
    kr = make_kps([GRID[k][0] - DELTA_D for k in g], [GRID[k][1] for k in g], np.zeros(len(g), np.int32))
    return kl, dl, kr, gd[g]


def expect_filter(values):
    acc = sorted(v for v in values if v is not None)
    if not acc:
        return [False] * len(values)
    th = np.float32(1.5) * np.float32(1.4) * np.float32(acc[len(acc) // 2])
    return [v is not None and bool(np.float32(v) < th) for v in values]


FILTER_SMALL = {"none": [None, None, None], "one": [10], "one_among_unmatched": [None, 20, None], "two": [10, 20], "two_zero": [0, 10], "three": [10, 20, 50],
                "all_zero": [0, 0, 0, 0], "all_equal": [10] * 8, "at_thdist": [10, 20, 42], "below_thdist": [10, 20, 41], "at_and_below": [20, 42, 41, 20, 10, 43, 20],
                "median_21": [21, 44, 10, 43, 21, 5, 15, 30, 60, 22, 44]}
assert np.float32(1.5) * np.float32(1.4) * np.float32(20) == 42 and np.float32(1.5) * np.float32(1.4) * np.float32(21) > 44   # "at thDist" is exact


def case_filter_small(lib, dev, name):
    r = rig(lib, "delta")
    values = FILTER_SMALL[name]
    kl, dl, kr, dr = delta_sets(r, values)
    if name == "none":
        kr, dr = kr[:0], dr[:0]
    our, odp = r.match(kl, dl, kr, dr, what="filter " + name)
    assert [bool(d > 0) for d in odp] == expect_filter(values), "filter %s: the SADs are not the stated ones (broken case): %s" % (name, odp)
    return int((odp > 0).sum())


def case_filter_tail(lib, dev, n_left):
    """the median element, the outliers and more than half of the accepted matches at the END of the left keypoints: beyond
    index 2048 for n_left = 2300, exactly one of them there for 2049"""
    r = rig(lib, "delta")
    tail = [20] * 80 + [41] + [50] * 40 + [42]
    values = [None] * (n_left - len(tail)) + tail
    for j in np.linspace(0, n_left - len(tail) - 1, 100).astype(int):
        values[j] = 10
    assert sum(v == 10 for v in values) == 100
    kl, dl, kr, dr = delta_sets(r, values)
    assert len(kr) <= 40
    our, odp = r.match(kl, dl, kr, dr, what="filter tail %d" % n_left)
    want = expect_filter(values)       # median 20 (rank 111 of 222), thDist 42: the 42 and the forty 50s are cut, the 41 stays
    assert [bool(d > 0) for d in odp] == want and sum(want) == 181 and not want[-1] and want[n_left - 42]
    return 181


# ---- host path sizes --------------------------------------------------------------------------------------------------
def sized(r, n_left, n_right, seed):
    rng = np.random.default_rng(seed)
    g = rng.permutation(r.good())
    kl, dl = lefts_from(r, g, n_left)
    k = min(n_left, n_right, len(g), 12)
    placed = {j: (i, 0.0, int(rng.integers(0, 9)), int(rng.integers(0, 256))) for i, j in enumerate(intended_indices(n_right, k))}
    kr, dr = right_set(r, kl, dl, n_right, placed, rng) if n_left else (make_kps(np.zeros(n_right), np.zeros(n_right), np.zeros(n_right)), np.zeros((n_right, 32), np.uint8))
    return kl, dl, kr, dr, placed


def case_host_sizes(lib, dev):
    r = rig(lib, "bands")
    for n_left, n_right in ((700, 3), (3, 3000), (40, 0), (0, 40), (0, 0), (50, 50), (5000, 5000), (50, 50)):   # the staging block grows, then is reused
        kl, dl, kr, dr, placed = sized(r, n_left, n_right, 7 * n_left + n_right)
        our, odp = r.match(kl, dl, kr, dr, what="sizes %d x %d" % (n_left, n_right))
        for j, p in placed.items():
            assert_matched(r, kl, kr, our, odp, p[0], j, "sizes %d x %d" % (n_left, n_right))
        if n_right == 0:
            assert (odp == -1).all() and len(odp) == n_left
    return 8


# ---- 65535 keypoints in a view: the lane merge keeps the right index in 16 bits (the refusals: case_argument_errors) ---------
LIMIT = 65535


def case_limit(lib, dev, side):
    """side "right": 65535 right keypoints, the intended matches at right indices 65534 (the last), 32768 and 32767; side "left":
    65535 left keypoints of which the last and number 32768 own an intended match"""
    r = rig(lib, "bands")
    rng = np.random.default_rng(LIMIT + len(side))
    g = rng.permutation(r.good())
    if side == "right":
        n_left, n_right = 130, LIMIT
        placed = {j: (i, 0.0, int(rng.integers(0, 9)), int(rng.integers(0, 256))) for i, j in enumerate((LIMIT - 1, 32768, 32767, 0, 2048, 40000))}
    else:
        n_left, n_right = LIMIT, 2049
        placed = {j: (i, 0.0, int(rng.integers(0, 9)), int(rng.integers(0, 256))) for i, j in ((LIMIT - 1, 2048), (32768, 37), (0, 0))}
    kl, dl = lefts_from(r, g, n_left)
    kr, dr = right_set(r, kl, dl, n_right, placed, rng)
    our, odp = r.match(kl, dl, kr, dr, what="limit, %s" % side)
    for j, p in placed.items():
        assert_matched(r, kl, kr, our, odp, p[0], j, "limit, %s" % side)
    return int((odp > 0).sum())


# ---- batch entry point ------------------------------------------------------------------------------------------------
BATCH_CAP = 2200
BATCHES = {5: [(BATCH_CAP, 40), (0, 7), (1, 2049), (130, 0), (2100, BATCH_CAP)], 3: [(65, 2049), (0, 5), (BATCH_CAP, 33)], 1: [(130, 2051)]}


def batch_call(lib, dev, r, kpl, ddl, n_left, kpr, ddr, n_right):
    """rgbl_stereo_matches_batch_device on [batch, cap] arrays; returns uRight and depth, which held NAN_BITS before the call"""
    import torch
    batch, cap = kpl.shape
    t = [torch.from_numpy(a).to(dev) for a in (kpl.view(np.uint8).reshape(batch, cap, 28), ddl, np.array(n_left, np.int32),
                                              kpr.view(np.uint8).reshape(batch, cap, 28), ddr, np.array(n_right, np.int32))]
    ur, dp = (torch.from_numpy(np.full((batch, cap), NAN_BITS, np.uint32).view(np.float32)).to(dev) for _ in range(2))
    if dev.type != "cpu":
        torch.cuda.synchronize(dev)
    p = [C.c_void_p(a.data_ptr()) for a in t]
    L.check(lib, lib.rgbl_stereo_matches_batch_device(r.exl.h, r.exr.h, batch, p[0], p[1], p[2], p[3], p[4], p[5], cap, KITTI[0], KITTI[1],
                                                      C.c_void_p(ur.data_ptr()), C.c_void_p(dp.data_ptr())))
    L.check(lib, lib.rgbl_extractor_sync(r.exl.h))
    return ur.cpu().numpy(), dp.cpu().numpy()


def case_batch_stale_tile_entries(lib, dev, n_right=2048 + 5):
    """A last tile of five right keypoints: what the first tile left behind in LDS entries 8 .. 31 passes every gate of left keypoint 0,
    and the slots 2048 + 8 .. 2048 + 31 of the right arrays, behind n_right, hold its descriptor exactly at another disparity.
    Neither may be looked at: the match is right keypoint 2050, five bits away."""
    r = rig(lib, "batch")
    cap = BATCH_CAP
    kl, dl = lefts_from(r, r.good(frame=0)[:3], 3, frame=0)
    s = float(r.scale[kl["octave"][0]])
    placed = {2050: (0, 0.0, 5, 0), 2049: (1, 0.0, 3, 0), 100: (2, 0.0, 3, 0)}
    placed.update({j: (0, -(30.0 + j) * s, 90, 40) for j in range(8, 32)})
    kr, dr = right_set(r, kl, dl, n_right, placed, np.random.default_rng(11))
    assert candidates(r, kl[0], kr, *KITTI)[8:32].all()
    kpl, kpr = np.zeros((1, cap), L.KP_DTYPE), np.zeros((1, cap), L.KP_DTYPE)
    ddl, ddr = np.zeros((1, cap, 32), np.uint8), np.zeros((1, cap, 32), np.uint8)
    kpl[0, :3], ddl[0, :3], kpr[0, :n_right], ddr[0, :n_right] = kl, dl, kr, dr
    kpr[0, n_right:] = true_right(r, kl[0], dx=-20.0 * s)
    ddr[0, n_right:] = dl[0]
    ur, dp = batch_call(lib, dev, r, kpl, ddl, [3], kpr, ddr, [n_right])
    our, odp = O.stereo_matches(r.ol[0], r.orr[0], kl, dl, kr, dr, *KITTI)
    for i, j in ((0, 2050), (1, 2049), (2, 100)):
        assert_matched(r, kl, kr, our, odp, i, j, "stale tile entries")
    assert np.array_equal(pc.bits(ur[0, :3]), pc.bits(our)) and np.array_equal(pc.bits(dp[0, :3]), pc.bits(odp))
    assert (pc.bits(ur[0, 3:]) == NAN_BITS).all() and (pc.bits(dp[0, 3:]) == NAN_BITS).all()
    return 3


def case_batch(lib, dev, batch):
    """rgbl_stereo_matches_batch_device with fewer frames than the extractors' last batch (5), per-frame counts that differ, frames
    without keypoints in the middle: every frame == the oracle == the host-pointer call, slots behind n_left[f] untouched"""
    r, one = rig(lib, "batch"), rig(lib, "single")
    cap, counts = BATCH_CAP, BATCHES[batch]
    rng = np.random.default_rng(batch)
    kpl, kpr = np.zeros((batch, cap), L.KP_DTYPE), np.zeros((batch, cap), L.KP_DTYPE)
    ddl, ddr = np.zeros((batch, cap, 32), np.uint8), np.zeros((batch, cap, 32), np.uint8)
    sets = []
    for f, (n_left, n_right) in enumerate(counts):
        g = rng.permutation(r.good(frame=f))
        kl, dl = lefts_from(r, g, n_left, frame=f)
        k = min(n_left, n_right, len(g), 12)
        placed = {j: (i, 0.0, int(rng.integers(0, 9)), int(rng.integers(0, 256))) for i, j in enumerate(intended_indices(n_right, k))}
        kr, dr = right_set(r, kl, dl, n_right, placed, rng) if n_left else right_set(r, *lefts_from(r, g, 3, frame=f), n_right, {}, rng)
        sets.append((kl, dl, kr, dr, placed))
        # the slots behind the counts hold keypoints that WOULD match (or be matched) if they were read
        kpl[f], ddl[f] = lefts_from(r, g, cap, frame=f)
        kpr[f] = kpl[f]
        kpr[f]["x"] -= np.array([BANDS[band_of(y)] for y in kpl[f]["y"]], np.float32)
        ddr[f] = ddl[f]
        kpl[f, :n_left], ddl[f, :n_left], kpr[f, :n_right], ddr[f, :n_right] = kl, dl, kr, dr
    ur, dp = batch_call(lib, dev, r, kpl, ddl, [c[0] for c in counts], kpr, ddr, [c[1] for c in counts])
    total = 0
    for f, ((n_left, n_right), (kl, dl, kr, dr, placed)) in enumerate(zip(counts, sets)):
        our, odp = O.stereo_matches(r.ol[f], r.orr[f], kl, dl, kr, dr, *KITTI)
        for j, q in placed.items():
            assert_matched(r, kl, kr, our, odp, q[0], j, "batch %d frame %d" % (batch, f))
        assert np.array_equal(pc.bits(ur[f, :n_left]), pc.bits(our)), "batch %d frame %d: mvuRight" % (batch, f)
        assert np.array_equal(pc.bits(dp[f, :n_left]), pc.bits(odp)), "batch %d frame %d: mvDepth" % (batch, f)
        assert (pc.bits(ur[f, n_left:]) == NAN_BITS).all() and (pc.bits(dp[f, n_left:]) == NAN_BITS).all(), "batch %d frame %d: slots behind n_left written" % (batch, f)
        if n_left:   # the host-pointer call on the same data: it reads frame 0 of its extractors' last call
            one.exl(r.images[f][0])
            one.exr(r.images[f][1])
            hur, hdp = F.ComputeStereoMatches(one.exl, one.exr, kl, dl, kr, dr, *KITTI)
            assert np.array_equal(pc.bits(hur), pc.bits(our)) and np.array_equal(pc.bits(hdp), pc.bits(odp)), "batch %d frame %d: host-pointer call" % (batch, f)
        total += int((odp > 0).sum())
    assert total > 0
    return total


# ---- argument errors --------------------------------------------------------------------------------------------------
def case_argument_errors(lib, dev):
    r = rig(lib, "bands")
    kl, dl, kr, dr, placed = sized(r, 40, 60, 5)

    def valid_call_still_matches():
        our, odp = r.match(kl, dl, kr, dr, what="valid call after a refusal")
        for j, q in placed.items():
            assert_matched(r, kl, kr, our, odp, q[0], j)

    def refused(exl, exr, a, b, c, d, mb=KITTI[0], mbf=KITTI[1], says=None):
        ur, dp = (np.full(len(a), NAN_BITS, np.uint32).view(np.float32) for _ in range(2))
        rc = lib.rgbl_stereo_matches(exl.h, exr.h, L.ptr(a), L.ptr(b), len(a), L.ptr(c), L.ptr(d), len(c), mb, mbf, L.ptr(ur), L.ptr(dp))
        assert rc == L.ERR_INVALID, "returned %d" % rc
        msg = lib.rgbl_last_error().decode()
        assert says is None or says in msg, msg
        assert (pc.bits(ur) == NAN_BITS).all() and (pc.bits(dp) == NAN_BITS).all(), "outputs written by a refused call"
        valid_call_still_matches()

    fresh = Rig(lib, np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), extract=False)
    refused(fresh.exl, fresh.exr, kl, dl, kr, dr)                     # stereo before any extraction
    refused(r.exl, fresh.exr, kl, dl, kr, dr)
    other = Rig(lib, np.zeros((H, W + 16), np.uint8), np.zeros((H, W + 16), np.uint8), extract=False)
    refused(r.exl, other.exr, kl, dl, kr, dr, says="geometry")       # extractors of different geometry
    fewer = Rig(lib, np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), levels=LEVELS - 1, extract=False)
    refused(r.exl, fewer.exr, kl, dl, kr, dr, says="geometry")
    for mb in (0.0, -0.54, float("nan")):
        refused(r.exl, r.exr, kl, dl, kr, dr, mb=mb)
    big = np.resize(kr, 65536)
    refused(r.exl, r.exr, kl, dl, big, np.resize(dr, (65536, 32)), says="65535")   # the lane merge keeps the right index in 16 bits
    refused(r.exl, r.exr, np.resize(kl, 65536), np.resize(dl, (65536, 32)), kr, dr, says="65535")
    for side in (0, 1):
        for octave in (-1, LEVELS, 16, 1 << 20):
            for at in (0, -1):
                bad = (kl.copy(), kr.copy())
                bad[side]["octave"][at] = octave
                refused(r.exl, r.exr, bad[0], dl, bad[1], dr, says="octave")
    # the batch entry point: cap = 0 and cap > 65535 (the device arrays are not looked at before the refusal)
    import torch
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    q = C.c_void_p(z.data_ptr())
    for cap, says in ((0, None), (-3, None), (65536, "65535")):
        rc = lib.rgbl_stereo_matches_batch_device(r.exl.h, r.exr.h, 1, q, q, q, q, q, q, cap, KITTI[0], KITTI[1], q, q)
        assert rc == L.ERR_INVALID and (says is None or says in lib.rgbl_last_error().decode())
    for batch in (0, 2):   # more frames than the extractors' last call processed
        assert lib.rgbl_stereo_matches_batch_device(r.exl.h, r.exr.h, batch, q, q, q, q, q, q, 8, KITTI[0], KITTI[1], q, q) == L.ERR_INVALID
    assert int(z.cpu().abs().sum()) == 0
    valid_call_still_matches()
    for x in (fresh, other, fewer):
        x.exl.close(); x.exr.close()
    return 1
