"""Edge points for the isInFrustum tests: map points placed exactly ON the comparisons of Frame::isInFrustum and
MapPoint::PredictScale, by construction (tests/frustum_golden.py, tests/local_map_checks.py).  TEST INFRASTRUCTURE."""
import numpy as np

from orb_slam3_rgbl_amd.frontend import frustum_restatement, frustum_terms


def predict_scale_unclamped(ratio, log_scale_factor):
    """ceil(logf(ratio) / mfLogScaleFactor) before MapPoint::PredictScale clamps it (float; the C library's logf)."""
    import ctypes as C
    libm = C.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = C.c_float, [C.c_float]
    return np.array([np.ceil(np.float32(libm.logf(float(r))) / np.float32(log_scale_factor)) for r in np.atleast_1d(ratio)], np.float32)


def _step(x, k):
    """float32 x moved by k units in the last place (k: int array), away from zero for k > 0."""
    return (np.full(np.shape(k), x, np.float32).view(np.int32) + np.asarray(k, np.int32)).view(np.float32)


def add_frustum_edge_points(case):
    """A copy of a make_local_map_case dict (>= 400 points) in which points sit exactly ON the comparisons of isInFrustum and
    PredictScale, by construction: the image bounds pass through the projections of four points in view (u, v on each
    bound: inclusive); dist == 0.8f * mfMinDistance and == 1.2f * mfMaxDistance, and one step outside either; viewCos ==
    the limit and one step below; Pc.z == 0 with x != 0 (an infinite projection); mfMaxDistance / dist == scale factor k and
    one step to either side (the level changes between them), k = 1 .. 7.  Returns (case, {name: point index})."""
    f = np.float32
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    c["consider1"] = np.ones(len(c["world_pos1"]), np.uint8)
    _, rec, st = frustum_restatement(c)
    seen = np.nonzero(st == 5)[0]
    named = {}
    u, v = rec["proj_x"][seen], rec["proj_y"][seen]
    k = max(len(seen) // 20, 1)
    mid_v = seen[(v > np.percentile(v, 25)) & (v < np.percentile(v, 75))]   # the points on the u bounds lie inside the v bounds
    mid_u = seen[(u > np.percentile(u, 25)) & (u < np.percentile(u, 75))]   # ... and the other way round
    by_u, by_v = mid_v[np.argsort(rec["proj_x"][mid_v])], mid_u[np.argsort(rec["proj_y"][mid_u])]
    named["u_min"], named["u_max"], named["v_min"], named["v_max"] = int(by_u[k // 2]), int(by_u[-1 - k // 2]), int(by_v[k // 2]), int(by_v[-1 - k // 2])
    minX, maxX = rec["proj_x"][named["u_min"]], rec["proj_x"][named["u_max"]]
    minY, maxY = rec["proj_y"][named["v_min"]], rec["proj_y"][named["v_max"]]
    c["grid"] = np.array([minX, minY, maxX, maxY, f(64) / (maxX - minX), f(48) / (maxY - minY)], f)
    _, rec, st = frustum_restatement(c)
    free = [int(i) for i in np.nonzero(st == 5)[0] if int(i) not in named.values()]
    T = frustum_terms(c)
    ks = np.arange(-64, 65)

    def take():
        return free.pop(0)
    # dist against the invariance range: the stored raw value is searched so that 0.8f * min (1.2f * max) hits dist exactly
    for name, key, fac, outside in (("min", "min_dist1", f(0.8), 1), ("max", "max_dist1", f(1.2), -1)):
        # ("max on": the ratio is 1 / 1.2 up to rounding, where PredictScale's ceil is -1 or -0 - six of them, so that the lower clamp is met)
        for which in ("on", "out") + (("on2", "on3", "on4", "on5", "on6") if name == "max" else ()):
            while True:
                i = take()
                d = T["dist"][i]
                cand = _step(d / fac, ks)
                bound = fac * cand
                hit = np.nonzero(bound == (d if which.startswith("on") else _step(d, np.array(outside))))[0]
                if len(hit):
                    c[key][i] = cand[hit[0]]
                    named["dist_%s_%s" % (name, which)] = i
                    break
    # viewCos: the normal is laid at 60 degrees to PO, then its z component is stepped until PO.dot(Pn) / dist is the limit
    lim = f(c["viewing_cos_limit"])
    Ow = np.asarray(c["Ow"], f)
    for which, target in (("on", lim), ("below", _step(lim, np.array(-1)))):
        while True:
            i = take()
            PO = (c["world_pos1"][i] - Ow).astype(f)
            d = T["dist"][i]
            tang = np.cross(PO.astype(np.float64), [0.3, 1.0, 0.2])
            tang /= np.linalg.norm(tang)
            n = (0.5 * PO.astype(np.float64) / float(d) + np.sqrt(0.75) * tang).astype(f)
            ks2 = np.arange(-30000, 30001)
            n2 = _step(n[2], ks2)
            vc = ((PO[0] * n[0] + PO[1] * n[1]) + PO[2] * n2) / d
            hit = np.nonzero(vc == target)[0]
            if len(hit):
                c["normal1"][i] = [n[0], n[1], n2[hit[0]]]
                named["view_cos_" + which] = i
                break
    # Pc.z == 0: z of the world point is stepped until the third row of Rcw P + tcw cancels
    R, t = np.asarray(c["Rcw"], f), np.asarray(c["tcw"], f)
    while True:
        i = take()
        p = c["world_pos1"][i].copy()
        p[2] = f(-(float(R[6]) * p[0] + float(R[7]) * p[1] + float(t[2])) / float(R[8]))
        ks3 = np.arange(-4000, 4001)
        p2 = _step(p[2], ks3)
        zc = ((R[6] * p[0] + R[7] * p[1]) + R[8] * p2) + t[2]
        xc = ((R[0] * p[0] + R[1] * p[1]) + R[2] * p2) + t[0]
        hit = np.nonzero((zc == 0) & (xc != 0))[0]
        if len(hit):
            c["world_pos1"][i] = [p[0], p[1], p2[hit[0]]]
            named["zero_depth"] = i
            break
    # the ratio on a scale factor and one step to either side
    sf = np.asarray(c["scale_factors"], f)
    for lv in range(1, len(sf)):
        for which, target in (("on", sf[lv]), ("below", _step(sf[lv], np.array(-1))), ("above", _step(sf[lv], np.array(1)))):
            while True:
                i = take()
                d = T["dist"][i]
                cand = _step(f(target * d), ks)
                hit = np.nonzero(cand / d == target)[0]
                if len(hit):
                    c["max_dist1"][i] = cand[hit[0]]
                    c["min_dist1"][i] = f(cand[hit[0]] / f(4.0))   # dist well inside the range
                    named["ratio_%d_%s" % (lv, which)] = i
                    break
    return c, named
