"""A float64 numpy model of Optimizer::LocalBundleAdjustment from :1188 on, written from the g2o sources (base_binary_edge.hpp,
block_solver.hpp, optimization_algorithm_levenberg.cpp, sparse_optimizer.cpp, types_six_dof_expmap.cpp) and
src/OptimizableTypes.cpp - a second reading, not a copy of csrc/lba_math.h: the FULL normal equations over cameras and points
are assembled densely and solved by LAPACK (Cholesky), with matrix products where the header writes sums out.  schur=True
eliminates the points first (also with LAPACK); perm reorders the edges before every sum.  The difference between those runs
is the model's own reordering noise, the yardstick of tests/golden/lba/README.md."""
import numpy as np

DELTA = {False: float(np.float32(np.sqrt(5.991))), True: float(np.float32(np.sqrt(7.815)))}


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def rot_of_quat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257): update = (omega, upsilon)"""
    om, up = u[:3], u[3:]
    th = np.linalg.norm(om)
    O = skew(om)
    if th < 1e-5:
        R = np.eye(3) + O + O @ O
        V = R
    else:
        R = np.eye(3) + np.sin(th) / th * O + (1 - np.cos(th)) / th ** 2 * (O @ O)
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * O + (th - np.sin(th)) / th ** 3 * (O @ O)
    return rot_of_quat(quat_of_rot(R)), V @ up   # SE3Quat(Quaterniond(R), t): the quaternion is normalised (matters below 1e-5)


def quat_of_rot(R):
    """x, y, z, w by the largest of the four candidates"""
    c = np.array([1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2],
                  1 + R[0, 0] + R[1, 1] + R[2, 2]])
    k = int(c.argmax())
    s = 2 * np.sqrt(c[k])
    if k == 3:
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4]
    elif k == 0:
        q = [s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif k == 1:
        q = [(R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4, (R[1, 0] - R[0, 1]) / s]
    return np.array(q)


class Model:
    def __init__(self, case, perm=None):
        c = case
        self.nf, self.nx = int(c["n_free"]), int(c["n_fixed"])
        nC = self.nf + self.nx
        self.R = np.array([rot_of_quat(np.asarray(q, np.float64)) for q in np.asarray(c["cam_q"], np.float32).reshape(nC, 4)]).reshape(nC, 3, 3)
        self.t = np.asarray(c["cam_t"], np.float32).reshape(nC, 3).astype(np.float64)
        self.K = np.asarray(c["cam_K"], np.float32).reshape(nC, 4).astype(np.float64)
        self.bf = np.asarray(c["cam_bf"], np.float32).astype(np.float64)
        self.X = np.asarray(c["world_pos"], np.float32).reshape(-1, 3).astype(np.float64)
        self.ep = np.asarray(c["edge_point"], np.int64)
        self.ec = np.asarray(c["edge_cam"], np.int64)
        self.obs = np.asarray(c["edge_obs"], np.float32).reshape(-1, 3).astype(np.float64)
        self.info = np.asarray(c["edge_inv_sigma2"], np.float32).astype(np.float64)
        self.stereo = ~(np.asarray(c["edge_obs"], np.float32).reshape(-1, 3)[:, 2] < 0)
        nE = len(self.ep)
        self.order = np.arange(nE) if perm is None else np.asarray(perm)
        fixed = np.ones(nC, bool)
        fif = c.get("free_is_fixed")
        for k in range(self.nf):
            fixed[k] = bool(fif[k]) if fif is not None else False
        self.any_fixed = self.nx > 0 or fixed[:self.nf].any()
        touched = np.zeros(nC, bool)
        touched[self.ec] = True
        self.cols = [k for k in range(nC) if not fixed[k] and touched[k]]
        self.col = -np.ones(nC, np.int64)
        self.col[self.cols] = np.arange(len(self.cols))
        pt_touched = np.zeros(len(self.X), bool)
        pt_touched[self.ep] = True
        self.pts = np.flatnonzero(pt_touched)
        self.prow = -np.ones(len(self.X), np.int64)
        self.prow[self.pts] = np.arange(len(self.pts))
        self.n = 6 * len(self.cols)
        self.N = self.n + 3 * len(self.pts)
        self.chi2 = np.zeros(nE)

    def errors(self, R, t, X):
        """computeError and chi2 of every edge; the stereo edge's invz is a float (types_six_dof_expmap.cpp:189)"""
        P = np.einsum("eij,ej->ei", R[self.ec], X[self.ep]) + t[self.ec]
        K, bf = self.K[self.ec], self.bf[self.ec]
        err = np.zeros((len(self.ep), 3))
        with np.errstate(all="ignore"):
            invz = (1.0 / P[:, 2]).astype(np.float32).astype(np.float64)
            us = P[:, 0] * invz * K[:, 0] + K[:, 2]
            vs = P[:, 1] * invz * K[:, 1] + K[:, 3]
            um = K[:, 0] * P[:, 0] / P[:, 2] + K[:, 2]
            vm = K[:, 1] * P[:, 1] / P[:, 2] + K[:, 3]
        s = self.stereo
        err[:, 0] = self.obs[:, 0] - np.where(s, us, um)
        err[:, 1] = self.obs[:, 1] - np.where(s, vs, vm)
        err[:, 2] = np.where(s, self.obs[:, 2] - (us - bf * invz), 0.0)
        return P, err, self.info * (err ** 2).sum(1)

    def robust(self, chi2):
        d = np.where(self.stereo, DELTA[True], DELTA[False])
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi2)
            big = ~(chi2 <= d * d)
            rho0 = np.where(big, 2 * sq * d - d * d, chi2)
            rho1 = np.where(big, d / sq, 1.0)
        return rho0, rho1

    def build(self):
        P, err, chi2 = self.errors(self.R, self.t, self.X)
        self.chi2 = chi2
        rho0, rho1 = self.robust(chi2)
        H = np.zeros((self.N, self.N))
        b = np.zeros(self.N)
        for e in self.order:
            c, p = self.ec[e], self.ep[e]
            x, y, z = P[e]
            fx, fy = self.K[c, 0], self.K[c, 1]
            R = self.R[c]
            if self.stereo[e]:
                bf = self.bf[c]
                A = np.zeros((3, 3)); B = np.zeros((3, 6))
                A[0] = -fx * R[0] / z + fx * x * R[2] / z ** 2
                A[1] = -fy * R[1] / z + fy * y * R[2] / z ** 2
                A[2] = A[0] - bf * R[2] / z ** 2
                B[0] = [x * y / z ** 2 * fx, -(1 + x * x / z ** 2) * fx, y / z * fx, -1 / z * fx, 0, x / z ** 2 * fx]
                B[1] = [(1 + y * y / z ** 2) * fy, -x * y / z ** 2 * fy, -x / z * fy, 0, -1 / z * fy, y / z ** 2 * fy]
                B[2] = [B[0, 0] - bf * y / z ** 2, B[0, 1] + bf * x / z ** 2, B[0, 2], B[0, 3], 0, B[0, 5] - bf / z ** 2]
                r = err[e]
            else:
                J = -np.array([[fx / z, 0, -fx * x / z ** 2], [0, fy / z, -fy * y / z ** 2]])
                A = J @ R
                B = J @ np.hstack([-skew([x, y, z]), np.eye(3)])
                r = err[e, :2]
            w = rho1[e] * self.info[e]
            g = -self.info[e] * r * rho1[e]
            ip = self.n + 3 * self.prow[p]
            H[ip:ip + 3, ip:ip + 3] += w * A.T @ A
            b[ip:ip + 3] += A.T @ g
            a = self.col[c]
            if a >= 0:
                ic = 6 * a
                H[ic:ic + 6, ic:ic + 6] += w * B.T @ B
                H[ic:ic + 6, ip:ip + 3] += w * B.T @ A
                H[ip:ip + 3, ic:ic + 6] += w * A.T @ B
                b[ic:ic + 6] += B.T @ g
        return H, b, float(rho0[self.order].sum())

    def solve(self, H, b, lam, schur):
        """(H + lambda I) x = b; None when a factorisation fails (not positive definite, or not finite)"""
        n, M = self.n, H + lam * np.eye(self.N)
        if not np.isfinite(M).all() or not np.isfinite(b).all():
            return None
        try:
            if not schur:
                L = np.linalg.cholesky(M)
                return np.linalg.solve(L.T, np.linalg.solve(L, b))
            Hll_inv = np.zeros((self.N - n, self.N - n))
            for k in range(len(self.pts)):
                s = slice(3 * k, 3 * k + 3)
                Hll_inv[s, s] = np.linalg.inv(M[n:, n:][s, s])
            Hpl = M[:n, n:]
            S = M[:n, :n] - Hpl @ Hll_inv @ Hpl.T
            bs = b[:n] - Hpl @ Hll_inv @ b[n:]
            if n:
                L = np.linalg.cholesky(S)
                xc = np.linalg.solve(L.T, np.linalg.solve(L, bs))
            else:
                xc = np.zeros(0)
            xl = Hll_inv @ (b[n:] - Hpl.T @ xc)
            return np.concatenate([xc, xl])
        except np.linalg.LinAlgError:
            return None

    def updated(self, x):
        R, t, X = self.R.copy(), self.t.copy(), self.X.copy()
        for a, c in enumerate(self.cols):
            dR, dt = se3_exp(x[6 * a:6 * a + 6])
            R[c] = dR @ self.R[c]
            t[c] = dt + dR @ self.t[c]
        for k, p in enumerate(self.pts):
            X[p] = self.X[p] + x[self.n + 3 * k:self.n + 3 * k + 3]
        return R, t, X

    def run(self, max_iterations=10, user_lambda_init=0.0, stop_after_polls=0, schur=False):
        """dict(ran, iterations, trials, accepted (one bool per trial), failed, first_chi2, last_chi2, R, t, X, chi2, flags, polls)"""
        polls = [0]

        def terminate():
            polls[0] += 1
            return stop_after_polls > 0 and polls[0] >= stop_after_polls
        out = dict(ran=0, iterations=0, trials=0, accepted=[], per_iteration=[], failed=0, first_chi2=0.0, last_chi2=0.0, polls=0)
        if not self.any_fixed:
            return out
        if terminate():
            out["polls"] = polls[0]
            return out
        out["ran"] = 1
        lam, ni, n_bad, x = 0.0, 2.0, 0, np.zeros(self.N)
        for it in range(max_iterations if len(self.ep) else 0):
            if terminate():
                break
            H, b, chi = self.build()
            ini = chi
            if it == 0:
                lam = user_lambda_init if user_lambda_init > 0 else 1e-5 * float(np.abs(np.diag(H)).max())
                ni, n_bad = 2.0, 0
                out["first_chi2"] = chi
            q = 0
            while True:
                sol = self.solve(H, b, lam, schur)
                if sol is not None:
                    x = sol
                R, t, X = self.updated(x)
                _, _, c2 = self.errors(R, t, X)
                self.chi2 = c2
                temp = float(self.robust(c2)[0][self.order].sum())
                if sol is None:
                    temp = np.finfo(np.float64).max
                    out["failed"] += 1
                with np.errstate(all="ignore"):
                    rho = (chi - temp) / (float(x @ (lam * x + b)) + 1e-3)
                good = bool(rho > 0 and np.isfinite(temp))
                out["accepted"].append(good)
                out["trials"] += 1
                if good:
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    chi = temp
                    self.R, self.t, self.X = R, t, X
                else:
                    lam *= ni
                    ni *= 2.0
                q += 1
                if not (rho < 0 and q < 10 and not terminate()):
                    break
            out["iterations"] += 1
            out["per_iteration"].append(q)
            out["last_chi2"] = chi
            if q == 10 or rho == 0:
                break
            n_bad = n_bad + 1 if (ini - chi) * 1e3 < ini else 0
            if n_bad >= 3:
                break
        P = np.einsum("eij,ej->ei", self.R[self.ec], self.X[self.ep]) + self.t[self.ec]
        th = np.where(self.stereo, 7.815, 5.991)
        behind = ~(P[:, 2] > 0)
        out.update(R=self.R, t=self.t, X=self.X, chi2=self.chi2.copy(), depth=P[:, 2],
                   flags=((self.chi2 > th) | behind).astype(np.uint8) | (behind.astype(np.uint8) << 1), polls=polls[0])
        return out


def run(case, perm=None, schur=False):
    return Model(case, perm).run(int(case.get("max_iterations", 10)), float(case.get("user_lambda_init", 0.0)),
                                 int(case.get("stop_after_polls", 0)), schur)
