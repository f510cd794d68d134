"""A float64 numpy model of MLPnPsolver (src/MLPnPsolver.cpp) for pinhole cameras without covariances, written from the
reference's text: the yardstick of csrc/mlpnp_math.h's host build (tests/test_mlpnp_math.py).  It shares no code with the
header: numpy.linalg.eigh for the eigenvectors, numpy.linalg.svd for the nearest rotation, a Cholesky solve, numpy's sin / cos /
arccos / cbrt, plain numpy sums.  What it takes from the header is only what the header DEFINES where the reference leaves a
choice open: the null-space basis of a bearing, the sign rule of the eigen frame, the rank rule (Eigen's), and the rule that a
failed solve or a non-finite step ends Gauss-Newton.  The Jacobian is analytic (derived, not the reference's generated text) and
is checked against central differences in tests/test_mlpnp_math.py.

reverse=True runs the same computation with every sum over the correspondences of a set taken in the opposite order (the six-sets
reversed); the sign tests still read the first six of the set as given.  That is pure reordering: the
difference between the two runs is what tests/golden/mlpnp/tolerance.json is measured from."""
import numpy as np

f32 = np.float32
EPS = np.finfo(np.float64).eps


def correspondences(pr):
    """the constructor (:55-97): per correspondence the bearing (float arithmetic, widened), the world point, the pixel and
    mvMaxError = sigma2 * th2 (float)"""
    mp = np.asarray(pr["mp_index"], np.int32)
    feat = np.nonzero(mp >= 0)[0]
    xy = np.asarray(pr["xy"], f32).reshape(-1, 2)[feat]
    K = np.asarray(pr["K"], f32)
    f = np.stack([(xy[:, 0] - K[2]) / K[0], (xy[:, 1] - K[3]) / K[1], np.ones(len(feat), f32)], 1).astype(np.float64)
    X = np.asarray(pr["world_pos"], f32).reshape(-1, 3)[mp[feat]]
    max_err = np.asarray(pr["level_sigma2"], f32)[np.asarray(pr["octave"], np.int32)[feat]] * f32(pr["th2"])
    return dict(feat=feat, f=f, X=X.astype(np.float64), X32=X, xy=xy, K=K, max_err=max_err.astype(f32), n=len(mp))


def nullspace(f):
    """the header's basis of the plane orthogonal to f = (x, y, 1): r = (0, -1, y) / |.|, s = f x r / |.|; rows"""
    f = np.atleast_2d(f)
    r = np.stack([np.zeros(len(f)), -np.ones(len(f)), f[:, 1]], 1)
    r /= np.linalg.norm(r, axis=1)[:, None]
    s = np.cross(f, r)
    s /= np.linalg.norm(s, axis=1)[:, None]
    return r, s


def rank3(M):
    """Eigen::FullPivHouseholderQR<Matrix3d>::rank() with the default threshold: full pivoting, Householder reflections, the
    count of |R_kk| > (largest pivot candidate met) * 3 * epsilon"""
    a = np.array(M, np.float64)
    maxpivot, diag = 0.0, []
    for k in range(3):
        sub = np.abs(a[k:, k:])
        if not np.isfinite(sub).all():
            return 0
        j, i = np.unravel_index(np.argmax(sub.T), sub.T.shape)      # column-major: the first maximum
        big = sub[i, j]
        maxpivot = max(maxpivot, big)
        a[[k, k + i]] = a[[k + i, k]]
        a[:, [k, k + j]] = a[:, [k + j, k]]
        x = a[k:, k].copy()
        tail2 = float(x[1:] @ x[1:])
        if tail2 > np.finfo(np.float64).tiny:
            beta = -np.copysign(np.sqrt(x[0] * x[0] + tail2), x[0]) if x[0] != 0 else -np.sqrt(tail2)
            v = np.concatenate([[1.0], x[1:] / (x[0] - beta)])
            tau = (beta - x[0]) / beta
            a[k:, k + 1:] -= tau * np.outer(v, v @ a[k:, k + 1:])
        else:
            beta = x[0]
        diag.append(beta)
    return int(sum(abs(d) > maxpivot * 3 * EPS for d in diag))


def eigen_frame(M):
    """SelfAdjointEigenSolver(planarTest).eigenvectors().transpose(): ascending, each vector's largest entry positive"""
    _, v = np.linalg.eigh(M)
    E = v.T.copy()
    for c in range(3):
        if E[c, np.argmax(np.abs(E[c]))] < 0:
            E[c] = -E[c]
    return E


def nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ Vt


def rodrigues2rot(w):
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    n = np.linalg.norm(w)
    R = np.eye(3)
    if n > EPS:
        R = R + np.sin(n) / n * K + (1 - np.cos(n)) / (n * n) * (K @ K)
    return R


def rot2rodrigues(R):
    w = np.zeros(3)
    with np.errstate(invalid="ignore"):
        wn = np.arccos((np.trace(R) - 1.0) / 2.0)
    if wn > EPS:
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wn / (2.0 * np.sin(wn)))
    return w


def residuals(x, f, X):
    """mlpnp_residuals_and_jacs' r (:771-777): 2 per correspondence, rows (r_i, s_i)"""
    nr, ns = nullspace(f)
    v = X @ rodrigues2rot(x[:3]).T + x[3:]
    g = v / np.linalg.norm(v, axis=1)[:, None]
    return np.stack([np.sum(nr * g, 1), np.sum(ns * g, 1)], 1)


def jacobian(x, f, X):
    """d residuals / d (w, t), analytic: with v = R(w) X + t and g = v / |v|, d(n.g)/dv = (n - (n.g) g) / |v|; R = I + a K + b K^2,
    a = sin|w| / |w|, b = (1 - cos|w|) / |w|^2, so dv/dw_k = a' (w_k/|w|) K X + a E_k X + b' (w_k/|w|) K^2 X + b (E_k K + K E_k) X.
    At w = 0 the quotient w_k / |w| is 0 / 0: NaN, as the reference's expressions are there.  Shape (m, 2, 6)."""
    w, T = x[:3], x[3:]
    nr, ns = nullspace(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        th = np.linalg.norm(w)
        a, b = np.sin(th) / th, (1 - np.cos(th)) / (th * th)
        da, db = (th * np.cos(th) - np.sin(th)) / (th * th), (th * np.sin(th) - 2 * (1 - np.cos(th))) / (th ** 3)
        u = w / th
        v = X @ rodrigues2rot(w).T + T
        nv = np.linalg.norm(v, axis=1)
        g = v / nv[:, None]
        J = np.zeros((len(X), 2, 6))
        KX = np.cross(w, X)
        KKX = np.cross(w, KX)
        for row, n in enumerate((nr, ns)):
            m = (n - np.sum(n * g, 1)[:, None] * g) / nv[:, None]
            for k in range(3):
                e = np.zeros(3)
                e[k] = 1.0
                dv = da * u[k] * KX + a * np.cross(e, X) + db * u[k] * KKX + b * (np.cross(e, KX) + np.cross(w, np.cross(e, X)))
                J[:, row, k] = np.sum(m * dv, 1)
            J[:, row, 3:] = m
    return J


def gauss_newton(x, f, X, order):
    """mlpnp_gn (:694-758).  Returns x and the path: updates + 8 (break rule), + 16 (stop rule), + 32 (failed solve)."""
    path = 0
    for _ in range(5):
        J = jacobian(x, f, X).reshape(-1, 6)
        r = residuals(x, f, X).reshape(-1)
        rows = np.stack([2 * order, 2 * order + 1], 1).reshape(-1)
        Jo, ro = J[rows], r[rows]
        A, g = Jo.T @ Jo, Jo.T @ ro
        try:
            if not (np.isfinite(A).all() and np.isfinite(g).all()):
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(A)
            dx = np.linalg.solve(L.T, np.linalg.solve(L, g))
            if not np.isfinite(dx).all():
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            return x, path + 32
        if np.abs(dx).max() > 5.0 or np.abs(dx).min() > 1.0:
            return x, path + 8
        dl = J @ dx
        x = x - dx
        path += 1
        if np.abs(dl).max() < 1e-5:
            return x, path + 16
    return x, path


def compute_pose(f, X, reverse=False):
    """computePose (:356-658) over the set (f, X) in the given order; (R, t, path, planar)"""
    m = len(X)
    order = np.arange(m)[::-1] if reverse else np.arange(m)
    Xo = X[order]
    M = Xo.T @ Xo
    planar = rank3(M) == 2
    E = eigen_frame(M) if planar else np.eye(3)
    pts = Xo @ E.T
    nr, ns = nullspace(f[order])
    if planar:
        A = np.zeros((2 * m, 9))
        for half, n in enumerate((nr, ns)):
            for a in range(3):
                A[half::2, 2 * a] = n[:, a] * pts[:, 1]
                A[half::2, 2 * a + 1] = n[:, a] * pts[:, 2]
                A[half::2, 6 + a] = n[:, a]
    else:
        A = np.zeros((2 * m, 12))
        for half, n in enumerate((nr, ns)):
            for a in range(3):
                for b in range(3):
                    A[half::2, 3 * a + b] = n[:, a] * pts[:, b]
                A[half::2, 9 + a] = n[:, a]
    AtA = A.T @ A
    if not np.isfinite(AtA).all():
        nan = np.full((3, 3), np.nan)
        return nan, np.full(3, np.nan), 32, planar
    r1 = np.linalg.eigh(AtA)[1][:, 0]
    f6, X6 = f[:6], X[:6]
    with np.errstate(invalid="ignore", divide="ignore"):
        if planar:
            tmp = np.array([[0.0, r1[0], r1[1]], [0.0, r1[2], r1[3]], [0.0, r1[4], r1[5]]])
            tmp[:, 0] = np.cross(tmp[:, 1], tmp[:, 2])
            tmp = tmp.T.copy()
            scale = 1.0 / np.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
            R1 = nearest_rotation(tmp)
            if np.linalg.det(R1) < 0:
                R1 = -R1
            R1 = E.T @ R1
            t = scale * r1[6:9]
            R1 = -R1.T
            if np.linalg.det(R1) < 0:
                R1[:, 2] = -R1[:, 2]
            R2 = R1 * np.array([-1.0, -1.0, 1.0])
            cands = [(R1, t), (R1, -t), (R2, t), (R2, -t)]
            vals = []
            for Rc, tc in cands:
                v = X6 @ Rc.T + tc
                v /= np.linalg.norm(v, axis=1)[:, None]
                vals.append(float(np.sum(1.0 - np.sum(v * f6, 1))))
            idx = 0
            for i in range(1, 4):
                if vals[i] < vals[idx]:
                    idx = i
            Rout, tout = cands[idx]
        else:
            tmp = r1[:9].reshape(3, 3).T.copy()
            scale = 1.0 / np.cbrt(abs(np.linalg.norm(tmp[:, 0]) * np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
            Rn = nearest_rotation(tmp)
            if np.linalg.det(Rn) < 0:
                Rn = -Rn
            t0 = Rn @ (scale * r1[9:12])
            err = []
            for sg in (1.0, -1.0):
                Ri, ti = Rn.T, -Rn.T @ (sg * t0)
                v = X6 @ Ri.T + ti
                v /= np.linalg.norm(v, axis=1)[:, None]
                err.append(float(np.sum(1.0 - np.sum(v * f6, 1))))
            tout = -Rn.T @ t0 if err[0] < err[1] else Rn.T @ t0
            Rout = Rn.T
        x = np.concatenate([rot2rodrigues(Rout), tout])
        x, path = gauss_newton(x, f, X, order)
    return rodrigues2rot(x[:3]), x[3:].copy(), path, planar


def check_inliers(c, R, t):
    """CheckInliers (:262-293) in the reference's number formats: (flags, error2 as float32)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        X = c["X32"].astype(np.float64)
        cam = [((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2] + t[i]).astype(f32) for i in range(3)]
        K = c["K"]
        u = K[0] * cam[0] / cam[2] + K[2]
        v = K[1] * cam[1] / cam[2] + K[3]
        dx, dy = c["xy"][:, 0] - u, c["xy"][:, 1] - v
        e2 = dx * dx + dy * dy
        return e2 < c["max_err"], e2


def iterate(pr, reverse=False):
    """one call of iterate (:100-223) over the given samples; the result dict mirrors frontend.ORBmatcher.MLPnPRansac, plus
    flags / err2 (n_hyp x N) and `selected` (the hypothesis a successful call returns, -1 after a run-through)"""
    c = correspondences(pr)
    N, n_hyp, mn = len(c["feat"]), int(pr["n_hyp"]), int(pr["min_inliers"])
    out = dict(found=0, no_more=0, n_inliers=0, iterations_run=0, Tcw=np.eye(4, dtype=f32), refines=0, best_inliers=int(pr.get("best_inliers", 0)),
               inlier=None, N=N)
    if N < mn:
        out["no_more"] = 1
        return out
    if n_hyp == 0:
        return out
    samples = np.asarray(pr["samples"], np.int32).reshape(-1, 6)
    T = np.zeros((n_hyp, 3, 4))
    counts, paths = np.zeros(n_hyp, np.int32), np.zeros(n_hyp, np.int32)
    flags, err2 = np.zeros((n_hyp, N), bool), np.zeros((n_hyp, N), f32)
    for k in range(n_hyp):
        s = samples[k]
        R, t, paths[k], _ = compute_pose(c["f"][s], c["X"][s], reverse)
        T[k, :, :3], T[k, :, 3] = R, t
        flags[k], err2[k] = check_inliers(c, R, t)
        counts[k] = flags[k].sum()
    out.update(counts=counts, Tcw_all=T, gn_path=paths, flags=flags, err2=err2)
    best = out["best_inliers"]
    best_mask = np.asarray(pr["best_mask"], bool)[:N].copy() if best > 0 else np.zeros(N, bool)
    best_T = np.asarray(pr.get("best_Tcw") if pr.get("best_Tcw") is not None else np.eye(4), f32).reshape(4, 4).copy()

    def as_float(k):
        Tk = np.eye(4, dtype=f32)
        Tk[:3] = T[k].astype(f32)
        return Tk
    for k in range(n_hyp):
        if counts[k] < mn:
            continue
        if counts[k] > best:
            best, best_mask, best_T = int(counts[k]), flags[k].copy(), as_float(k)
        # Refine (:295-353) as it compiles: computePose's `result` is never copied into mRi / mti, so the CheckInliers of :331
        # sees hypothesis k's pose again: mnRefinedInliers = counts[k], the flags and mRefinedTcw are hypothesis k's
        out["refines"] += 1
        if counts[k] > mn:
            out.update(found=1, n_inliers=int(counts[k]), iterations_run=k + 1, Tcw=as_float(k), flags_out=flags[k], selected=k,
                       best_inliers=best, best_mask=best_mask, best_Tcw=best_T)
            return out
    out.update(no_more=1, iterations_run=n_hyp, best_inliers=best, best_mask=best_mask, best_Tcw=best_T, selected=-1)
    if best >= mn:
        out.update(found=1, n_inliers=best, Tcw=best_T, flags_out=best_mask)
    return out
