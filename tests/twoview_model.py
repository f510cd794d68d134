"""A numpy model of TwoViewReconstruction written from src/TwoViewReconstruction.cc, in float64 (or, for the noise estimate, in
float32) with LAPACK's svd for every JacobiSVD.  It is a SECOND READING of the same text, not the reference: it shares no code with
csrc/twoview_math.h, orders its sums as numpy does and takes its singular vectors from another algorithm.  tests/test_twoview_math.py
holds the host build to it within a tolerance measured on the model alone (tests/golden/two_view/README.md).

    python tests/twoview_model.py        # measures the noise on the cases of test_twoview_math.CASES and rewrites tolerance.json
"""
import json
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(TESTS, "golden", "two_view")
RATIO = 1e-3          # a hypothesis is compared when s[7] / s[0] of its A is at least this (golden/two_view/README.md)
FACTOR = 16.0         # tolerance = FACTOR x the model's own noise, as for the other solvers


def normalize(xy, dt, reverse=False):
    xy = xy.astype(dt)
    o = slice(None, None, -1) if reverse else slice(None)
    mean = xy[o].mean(0, dtype=dt)
    c = xy - mean
    dev = np.abs(c)[o].mean(0, dtype=dt)
    s = (dt(1.0) / dev).astype(dt)
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1]], dt)
    return c * s, T


def unit(M):
    """unit Frobenius norm, the entry of largest magnitude positive"""
    M = np.asarray(M, np.float64)
    n = np.linalg.norm(M)
    if not np.isfinite(n) or n == 0:
        return np.full_like(M, np.nan)
    M = M / n
    return M if M.reshape(-1)[np.argmax(np.abs(M))] > 0 else -M


def compute_h21(p1, p2, dt, reverse=False):
    A = np.zeros((16, 9), dt)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A[0::2, 3], A[0::2, 4], A[0::2, 5] = -u1, -v1, -1
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = v2 * u1, v2 * v1, v2
    A[1::2, 0], A[1::2, 1], A[1::2, 2] = u1, v1, 1
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = -u2 * u1, -u2 * v1, -u2
    s, vt = np.linalg.svd(A[::-1] if reverse else A)[1:]
    return vt[8].reshape(3, 3), s[7] / s[0]


def compute_f21(p1, p2, dt, reverse=False):
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(8, dt)], 1).astype(dt)
    s, vt = np.linalg.svd(A[::-1] if reverse else A)[1:]
    u, w, vt2 = np.linalg.svd(vt[8].reshape(3, 3))
    w[2] = 0
    return (u * w) @ vt2, s[7] / s[0]


def check_homography(H21, H12, x1, x2, sigma, dt, reverse=False):
    th = dt(5.991)
    inv = dt(1.0) / dt(sigma * sigma)
    with np.errstate(all="ignore"):
        def transfer(H, a, b):
            w = dt(1.0) / (H[2, 0] * a[:, 0] + H[2, 1] * a[:, 1] + H[2, 2])
            u = (H[0, 0] * a[:, 0] + H[0, 1] * a[:, 1] + H[0, 2]) * w
            v = (H[1, 0] * a[:, 0] + H[1, 1] * a[:, 1] + H[1, 2]) * w
            return ((b[:, 0] - u) ** 2 + (b[:, 1] - v) ** 2) * inv
        c1, c2 = transfer(H12, x2, x1), transfer(H21, x1, x2)
        o = slice(None, None, -1) if reverse else slice(None)
        s = np.where(c1 > th, 0, th - c1)[o].sum() + np.where(c2 > th, 0, th - c2)[o].sum()
    return s, ~(c1 > th) & ~(c2 > th)


def check_fundamental(F, x1, x2, sigma, dt, reverse=False):
    th, ths = dt(3.841), dt(5.991)
    inv = dt(1.0) / dt(sigma * sigma)
    h1 = np.c_[x1, np.ones(len(x1), dt)]
    h2 = np.c_[x2, np.ones(len(x2), dt)]
    with np.errstate(all="ignore"):
        l2 = h1 @ F.T
        c1 = (l2 * h2).sum(1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2) * inv
        l1 = h2 @ F
        c2 = (l1 * h1).sum(1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2) * inv
        o = slice(None, None, -1) if reverse else slice(None)
        s = np.where(c1 > th, 0, ths - c1)[o].sum() + np.where(c2 > th, 0, ths - c2)[o].sum()
    return s, ~(c1 > th) & ~(c2 > th)


def first_max(scores):
    best, at = 0.0, -1
    for i, c in enumerate(scores):
        if c > best:
            best, at = c, i
    return at, best


def check_rt(R, t, K, x1, x2, inl, th2, dt):
    """nGood, parallax, the flags, the points, and the smallest distance of a decision of a counted or rejected point to its bound"""
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dt)
    P1 = Km @ np.c_[np.eye(3, dtype=dt), np.zeros(3, dt)]
    P2 = Km @ np.c_[R, t]
    O2 = -R.T @ t
    idx = np.nonzero(inl)[0]
    good = np.zeros(len(x1), bool)
    P = np.zeros((len(x1), 3), dt)
    cos, sq = [], []
    for i in idx:
        A = np.stack([x1[i, 0] * P1[2] - P1[0], x1[i, 1] * P1[2] - P1[1], x2[i, 0] * P2[2] - P2[0], x2[i, 1] * P2[2] - P2[1]])
        v = np.linalg.svd(A)[2][3]
        with np.errstate(all="ignore"):
            X = v[:3] / v[3]
        if not np.isfinite(X).all():
            continue
        n1, n2 = X, X - O2
        c = n1 @ n2 / (np.linalg.norm(n1) * np.linalg.norm(n2))
        if X[2] <= 0 and c < 0.99998:
            continue
        X2 = R @ X + t
        if X2[2] <= 0 and c < 0.99998:
            continue
        e1 = (K[0] * X[0] / X[2] + K[2] - x1[i, 0]) ** 2 + (K[1] * X[1] / X[2] + K[3] - x1[i, 1]) ** 2
        e2 = (K[0] * X2[0] / X2[2] + K[2] - x2[i, 0]) ** 2 + (K[1] * X2[1] / X2[2] + K[3] - x2[i, 1]) ** 2
        sq.extend([e1, e2])
        if e1 > th2 or e2 > th2:
            continue
        cos.append(c)
        P[i] = X
        good[i] = c < 0.99998
    par = 0.0
    if cos:
        cs = np.sort(cos)
        par = float(np.degrees(np.arccos(min(1.0, cs[min(50, len(cs) - 1)]))))
    near = int((np.abs(np.array(sq) - th2) < 0.05 * th2).sum()) if sq else 0
    return len(cos), par, good, P, near


def motions_f(F21, K, dt):
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dt)
    E = Km.T @ F21 @ Km
    u, _, vt = np.linalg.svd(E)
    t = u[:, 2] / np.linalg.norm(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dt)
    R1, R2 = u @ W @ vt, u @ W.T @ vt
    R1 = -R1 if np.linalg.det(R1) < 0 else R1
    R2 = -R2 if np.linalg.det(R2) < 0 else R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def motions_h(H21, K, dt):
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dt)
    A = np.linalg.inv(Km) @ H21 @ Km
    U, w, Vt = np.linalg.svd(A)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = w
    if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return None
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    ast = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [ast, -ast, -ast, ast]
    out = []
    for i in range(4):
        Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]], dt)
        t = U @ (np.array([x1[i], 0, -x3[i]], dt) * (d1 - d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    asp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [asp, -asp, -asp, asp]
    for i in range(4):
        Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]], dt)
        t = U @ (np.array([x1[i], 0, x3[i]], dt) * (d1 + d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out


def reconstruct(pr, dt=np.float64, reverse=False):
    """the whole of Reconstruct on a problem dict of twoview_cases; dt: the precision of every step; reverse: every sum over keys,
    over the rows of A and over matches runs backwards"""
    from orb_slam3_rgbl_amd import twoview_cases as tc
    first, second = tc.matches(pr)
    xy1, xy2 = np.asarray(pr["xy1"], np.float32), np.asarray(pr["xy2"], np.float32)
    K, sigma = np.asarray(pr["K"], np.float32).astype(dt), dt(pr["sigma"])
    n1, T1 = normalize(xy1, dt, reverse)
    n2, T2 = normalize(xy2, dt, reverse)
    x1, x2 = xy1[first].astype(dt), xy2[second].astype(dt)
    sets = np.asarray(pr["samples"]).reshape(-1, 8)
    nh = len(sets)
    out = dict(H=np.zeros((nh, 3, 3)), F=np.zeros((nh, 3, 3)), ratio=np.zeros((nh, 2)), scores=np.zeros((nh, 2)), N=len(first))
    masks = [[None, None] for _ in range(nh)]
    for k, s in enumerate(sets):
        Hn, out["ratio"][k, 0] = compute_h21(n1[first[s]], n2[second[s]], dt, reverse)
        Fn, out["ratio"][k, 1] = compute_f21(n1[first[s]], n2[second[s]], dt, reverse)
        with np.errstate(all="ignore"):
            H21 = (np.linalg.inv(T2) @ Hn @ T1).astype(dt)
            try:
                H12 = np.linalg.inv(H21).astype(dt)
            except np.linalg.LinAlgError:
                H12 = np.full((3, 3), np.nan, dt)
        F21 = (T2.T @ Fn @ T1).astype(dt)
        out["H"][k], out["F"][k] = H21, F21
        out["scores"][k, 0], masks[k][0] = check_homography(H21, H12, x1, x2, sigma, dt, reverse)
        out["scores"][k, 1], masks[k][1] = check_fundamental(F21, x1, x2, sigma, dt, reverse)
    bh, SH = first_max(out["scores"][:, 0])
    bf, SF = first_max(out["scores"][:, 1])
    out.update(best_h=bh, best_f=bf, SH=SH, SF=SF, found=0, model=-1, n_good=np.zeros(8, int), parallax=np.zeros(8), near=np.zeros(8, int), R=None, t=None)
    if SH + SF == 0:
        return out
    th2 = dt(4.0) * sigma * sigma
    if SH / (SH + SF) > 0.5:
        out["model"] = 0
        inl = masks[bh][0]
        mo = motions_h(out["H"][bh].astype(dt), K, dt)
        if mo is None:
            return out
    else:
        out["model"] = 1
        inl = masks[bf][1]
        mo = motions_f(out["F"][bf].astype(dt), K, dt)
    N = int(inl.sum())
    res = [check_rt(R.astype(dt), t.astype(dt), K, x1, x2, inl, th2, dt) for R, t in mo]
    g = np.array([r[0] for r in res])
    out["n_good"][:len(g)], out["parallax"][:len(g)], out["near"][:len(g)] = g, [r[1] for r in res], [r[4] for r in res]
    out["n_inliers"] = N
    if out["model"] == 1:
        mx = g.max()
        if mx < max(int(0.9 * N), 50) or (g > 0.7 * mx).sum() > 1:
            return out
        j = int(np.nonzero(g == mx)[0][0])
        if res[j][1] > 1.0:
            out.update(found=1, R=mo[j][0], t=mo[j][1], best=j)
    else:
        best, second_best, j, par = 0, 0, -1, -1.0
        for i, r in enumerate(res):
            if r[0] > best:
                second_best, best, j, par = best, r[0], i, r[1]
            elif r[0] > second_best:
                second_best = r[0]
        if second_best < 0.75 * best and par >= 1.0 and best > 50 and best > 0.9 * N:
            out.update(found=1, R=mo[j][0], t=mo[j][1], best=j)
    return out


def noise(pr):
    """the model against itself, two ways: float64 against float32, and float64 as drawn against float64 with every sum reversed.
    Per model kind both distances of the unit-norm matrices over the compared hypotheses and their larger (`noise`), the same for
    the scores, and whether the runs decide alike."""
    a, b, r = reconstruct(pr, np.float64), reconstruct(pr, np.float32), reconstruct(pr, np.float64, reverse=True)
    out = {}
    for md, key in ((0, "H"), (1, "F")):
        keep = a["ratio"][:, md] >= RATIO
        idx = np.nonzero(keep)[0]
        d32 = float(np.nanmax([np.abs(unit(a[key][k]) - unit(b[key][k])).max() for k in idx])) if len(idx) else 0.0
        drev = float(np.nanmax([np.abs(unit(a[key][k]) - unit(r[key][k])).max() for k in idx])) if len(idx) else 0.0
        s32 = float(np.abs(a["scores"][keep, md] - b["scores"][keep, md]).max()) if keep.any() else 0.0
        srev = float(np.abs(a["scores"][keep, md] - r["scores"][keep, md]).max()) if keep.any() else 0.0
        out[key] = dict(compared=int(keep.sum()), of=len(keep), noise_float32=d32, noise_reversed=drev, noise=max(d32, drev),
                        score_noise_float32=s32, score_noise_reversed=srev, score_noise=max(s32, srev))

    def alike(p, q):
        return bool(p["model"] == q["model"] and p["found"] == q["found"] and p["best_h"] == q["best_h"] and p["best_f"] == q["best_f"])
    out["same_decision"] = alike(a, b) and alike(a, r)
    if a["found"] and out["same_decision"]:
        out["T21_noise"] = float(max(max(np.abs(a["R"] - q["R"]).max(), np.abs(a["t"] - q["t"]).max()) for q in (b, r)))
    return a, out


def main():
    import test_twoview_math as tm
    rec = dict(ratio=RATIO, factor=FACTOR, cases={})
    for name in tm.CASES:
        pr = tm.case_problem(name)
        _, n = noise(pr)
        rec["cases"][name] = n
    for key in ("H", "F"):
        rec[key + "_noise"] = max(c[key]["noise"] for c in rec["cases"].values())
        rec[key + "_noise_float32"] = max(c[key]["noise_float32"] for c in rec["cases"].values())
        rec[key + "_noise_reversed"] = max(c[key]["noise_reversed"] for c in rec["cases"].values())
        rec[key + "_tolerance"] = FACTOR * rec[key + "_noise"]
        rec[key + "_score_margin"] = FACTOR * max(c[key]["score_noise"] for c in rec["cases"].values())
    t = [c["T21_noise"] for c in rec["cases"].values() if "T21_noise" in c]
    rec["T21_noise"] = max(t)
    rec["T21_tolerance"] = FACTOR * rec["T21_noise"]
    os.makedirs(GOLDEN, exist_ok=True)
    with open(os.path.join(GOLDEN, "tolerance.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    sys.path.insert(0, TESTS)
    main()
