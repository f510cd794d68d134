"""A numpy model of Sim3Solver (src/Sim3Solver.cc:302-439, :461-487) written from the reference's source, not from
csrc/sim3_math.h: ComputeCentroid, ComputeSim3 (Horn's closed form with numpy.linalg.eigh for the eigenvector, always in
float64), Project / FromCameraToImage with Pinhole::project, CheckInliers, and the stopping rule of iterate as a scan.  `dtype`
(float32 or float64) is the precision of everything outside the eigen solve.  The float64 run is the yardstick of
tests/test_sim3_math.py and tests/test_sim3_gpu.py; the float32 run measures how far float arithmetic alone moves the result,
which is where the tolerance comes from (tests/golden/sim3/README.md)."""
import numpy as np

# a hypothesis is compared only if its sample triangles are not degenerate and the top eigenvalue is separated:
TRIANGLE_BOUND = 0.02   # 2 * area / (longest side)^2 of the sample triangle, in both point sets
GAP_BOUND = 0.004       # (lambda_1 - lambda_2) / (lambda_1 - lambda_4) of the 4 x 4 matrix N: rounding is amplified by its inverse
FACTOR = 16             # tolerance = FACTOR x the float32 / float64 difference of this model


def _quat_matrix(w, x, y, z):
    """Eigen's Quaternion::toRotationMatrix of a quaternion that is not re-normalised (SO3f::exp(...).matrix())"""
    R = np.empty(w.shape + (3, 3), w.dtype)
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)   # noqa: E702
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)   # noqa: E702
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)   # noqa: E702
    return R


def _triangle(P):
    """2 * area / (longest side)^2 of the triangles P[h, k, :] (k = 0, 1, 2), in float64"""
    P = P.astype(np.float64)
    a, b, c = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 2] - P[:, 1]
    area2 = np.linalg.norm(np.cross(a, b), axis=1)
    longest = np.maximum(np.maximum((a * a).sum(1), (b * b).sum(1)), (c * c).sum(1))
    with np.errstate(all="ignore"):
        return np.where(longest > 0, area2 / longest, 0.0)


def compute_sim3(P1, P2, fix_scale, dtype):
    """ComputeSim3 for H sample triples at once: P1, P2 [H, 3 points, 3]; returns R [H,3,3], t [H,3], s [H] in dtype and the
    relative eigenvalue gap"""
    P1, P2 = P1.astype(dtype), P2.astype(dtype)
    O1, O2 = P1.sum(1) / dtype(3), P2.sum(1) / dtype(3)                 # step 1
    Pr1, Pr2 = P1 - O1[:, None, :], P2 - O2[:, None, :]
    M = np.einsum("hki,hkj->hij", Pr2, Pr1).astype(dtype)               # step 2: M = Pr2 * Pr1^T (points as columns)
    N = np.empty((len(M), 4, 4), dtype)                                 # step 3
    N[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    N[:, 0, 1] = M[:, 1, 2] - M[:, 2, 1]
    N[:, 0, 2] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = M[:, 0, 1] - M[:, 1, 0]
    N[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    N[:, 1, 2] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = M[:, 2, 0] + M[:, 0, 2]
    N[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]
    N[:, 2, 3] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    for i in range(4):
        for j in range(i):
            N[:, i, j] = N[:, j, i]
    with np.errstate(all="ignore"):
        ok = np.isfinite(N).all((1, 2))
        lam, vec = np.linalg.eigh(np.where(ok[:, None, None], N, 0).astype(np.float64))   # step 4; ascending
        q = vec[:, :, 3]
        q = np.where(q[:, :1] < 0, -q, q).astype(dtype)                    # the sign the header fixes: w >= 0
        spread = lam[:, 3] - lam[:, 0]
        gap = np.where(ok & (spread > 0), (lam[:, 3] - lam[:, 2]) / np.where(spread > 0, spread, 1), 0.0)
        v = q[:, 1:]
        nrm = np.sqrt((v * v).sum(1)).astype(dtype)
        ang = np.arctan2(nrm.astype(np.float64), q[:, 0].astype(np.float64))
        om = (dtype(1) * (2 * ang).astype(dtype))[:, None] * v / nrm[:, None]
        theta = np.sqrt((om * om).sum(1)).astype(dtype)                      # SO3f::exp
        half = dtype(0.5) * theta
        small = theta * theta < dtype(1e-10)
        imag = np.where(small, dtype(0.5) - theta * theta / dtype(48), np.sin(half) / np.where(small, dtype(1), theta)).astype(dtype)
        real = np.where(small, dtype(1) - theta * theta / dtype(8), np.cos(half)).astype(dtype)
        R = _quat_matrix(real, imag * om[:, 0], imag * om[:, 1], imag * om[:, 2]).astype(dtype)
        P3 = np.einsum("hij,hkj->hki", R, Pr2).astype(dtype)                # step 5
        if fix_scale:
            s = np.ones(len(M), dtype)
        else:                                                              # step 6, the quotient in double
            nom, den = (Pr1 * P3).sum((1, 2)).astype(dtype), (P3 * P3).sum((1, 2)).astype(dtype)
            s = (nom.astype(np.float64) / den.astype(np.float64)).astype(dtype)
        t = (O1 - np.einsum("hij,hj->hi", s[:, None, None] * R, O2)).astype(dtype)   # step 7
    return R, t, s, gap


def _project(K, X):
    with np.errstate(all="ignore"):
        return np.stack([K[0] * X[..., 0] / X[..., 2] + K[2], K[1] * X[..., 1] / X[..., 2] + K[3]], -1)


def select(c, best_inliers, min_inliers):
    """the loop of iterate over the counts (:192-209)"""
    b, held = best_inliers, -1
    for k, ck in enumerate(c):
        if ck >= b:
            b, held = int(ck), k
            if ck > min_inliers:
                return dict(selected=held, converged=1, n_inliers=b, iterations_run=k + 1)
    return dict(selected=held, converged=0, n_inliers=b if held >= 0 else 0, iterations_run=len(c))


def run(pr, dtype=np.float64):
    """every hypothesis of a problem dict (host arrays).  Returns R, t, s per hypothesis, err1 / err2 [H, n], the flags, the
    counts, `compared` (the well-conditioned hypotheses), the scene's extent and the selection"""
    dtype = np.dtype(dtype).type
    x1, x2 = np.asarray(pr["x1c"], np.float32).astype(dtype), np.asarray(pr["x2c"], np.float32).astype(dtype)
    K1, K2 = np.asarray(pr["K1"], np.float32).astype(dtype), np.asarray(pr["K2"], np.float32).astype(dtype)
    e1, e2 = np.asarray(pr["max_err1"], np.float32).astype(dtype), np.asarray(pr["max_err2"], np.float32).astype(dtype)
    S = np.asarray(pr["samples"], np.int64).reshape(-1, 3)
    R, t, s, gap = compute_sim3(x1[S], x2[S], bool(pr["fix_scale"]), dtype)
    with np.errstate(all="ignore"):
        sR = s[:, None, None] * R
        iR = (dtype(1) / s)[:, None, None] * np.swapaxes(R, 1, 2)           # step 8.2
        it = -np.einsum("hij,hj->hi", iR, t)
        p1, p2 = _project(K1, x1), _project(K2, x2)                         # FromCameraToImage
        a = _project(K1, np.einsum("hij,nj->hni", sR, x2) + t[:, None, :])   # Project(mvX3Dc2, vP2im1, mT12i, pCamera1)
        b = _project(K2, np.einsum("hij,nj->hni", iR, x1) + it[:, None, :])  # Project(mvX3Dc1, vP1im2, mT21i, pCamera2)
        err1 = ((p1[None] - a) ** 2).sum(-1).astype(dtype)
        err2 = ((b - p2[None]) ** 2).sum(-1).astype(dtype)
        inl = (err1 < e1[None]) & (err2 < e2[None])
    counts = inl.sum(1).astype(np.int32)
    tri = np.minimum(_triangle(x1[S]), _triangle(x2[S]))
    compared = (tri >= TRIANGLE_BOUND) & (gap >= GAP_BOUND) & np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
    extent = float(np.abs(np.asarray(pr["x1c"], np.float64)).max())
    out = dict(R=R, t=t, s=s, err1=err1, err2=err2, e1=e1, e2=e2, inlier=inl, counts=counts, compared=compared, extent=extent)
    out.update(select(counts, int(pr.get("best_inliers", 0)), int(pr["min_inliers"])))
    return out


def transform_difference(R, t, s, R0, t0, s0, extent):
    """per hypothesis: the largest of |R - R0| (any entry of sR / s), |s - s0| / s0 and |t - t0| / extent"""
    R, t, s, R0, t0, s0 = [np.asarray(v, np.float64) for v in (R, t, s, R0, t0, s0)]
    with np.errstate(all="ignore"):
        return np.maximum(np.maximum(np.abs(R - R0).max((1, 2)), np.abs(s - s0) / np.abs(s0)), np.abs(t - t0).max(1) / extent)


def error_difference(err, err0, thr):
    """per pair: |err - err0| relative to the larger of err0 and the pair's threshold (an error far above its threshold is
    measured against itself, one below against the threshold it is compared with)"""
    err, err0 = np.asarray(err, np.float64), np.asarray(err0, np.float64)
    with np.errstate(all="ignore"):
        return np.abs(err - err0) / np.maximum(err0, np.asarray(thr, np.float64)[None])


def decided(m, margin):
    """the pairs of the float64 run m whose two errors both lie further than `margin` (relative) from their thresholds, or that
    are outliers by a decided error alone"""
    with np.errstate(all="ignore"):
        far1 = np.abs(m["err1"].astype(np.float64) - m["e1"][None]) > margin * m["e1"][None]
        far2 = np.abs(m["err2"].astype(np.float64) - m["e2"][None]) > margin * m["e2"][None]
        out1 = far1 & ~(m["err1"] < m["e1"][None])
        out2 = far2 & ~(m["err2"] < m["e2"][None])
    return (far1 & far2) | out1 | out2
