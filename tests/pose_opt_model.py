"""A float64 numpy model of Optimizer::PoseOptimization (src/Optimizer.cc:814-1114) for single-camera pinhole frames, written
from the reference's g2o sources (core/optimization_algorithm_levenberg.cpp:61-194, core/sparse_optimizer.cpp:354-419,
core/robust_kernel_impl.cpp:78-91, core/base_unary_edge.hpp:43-72, types/se3quat.h:223-257, types/types_six_dof_expmap.cpp:
339-404, src/OptimizableTypes.cpp:49-63) INDEPENDENTLY of csrc/poseopt_math.h: the pose is a rotation matrix and a translation
(no quaternion anywhere), the 6 x 6 system goes through numpy's Cholesky, sin / cos are numpy's, the Jacobians are built as
matrix products, and the edges are summed in an order the caller gives.  tests/test_pose_opt_math.py holds the header's host
build to it within the model's own reordering noise x 100.

run(case, order=None) -> dict(R, t, outlier (per feature), result, rounds, iterations, active, chi2, events, margin)
  events: what the quirk tests assert happened - "stale" (a round whose last trial was rejected), "rho_zero", "ten_trials" (ten trials in a row rejected),
          "nbad_stop", "float_flip" (an edge whose chi2 and its float rounding lie on different sides of the threshold)
  margin: the smallest |chi2 - threshold| / threshold over every classification made
  edge_chi2: per round, the chi2 every correspondence was classified by"""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def quat_to_rot(q):
    x, y, z, w = [float(v) for v in np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257) without the detour through a quaternion"""
    omega, upsilon = u[:3], u[3:]
    theta = np.linalg.norm(omega)
    O = skew(omega)
    if theta < 0.00001:
        # g2o never applies I + Omega + Omega^2 as a rotation: SE3Quat(Quaterniond(R), ...) turns it into a unit quaternion, which
        # keeps the antisymmetric part (Omega) and the trace (3 - 2 theta^2) only.  With s = sqrt(trace + 1) that quaternion is
        # (omega / s, s / 2) before it is normalised: the rotation about omega by 2 atan2(theta / s, s / 2), written here with
        # Rodrigues' formula.  V stays the matrix.
        V = np.eye(3) + O + O @ O
        if theta == 0.0:
            return np.eye(3), V @ upsilon
        s = np.sqrt(4.0 - 2.0 * theta * theta)
        phi = 2.0 * np.arctan2(theta / s, s / 2.0)
        A = O / theta
        return np.eye(3) + np.sin(phi) * A + (1 - np.cos(phi)) * (A @ A), V @ upsilon
    else:
        O2 = O @ O
        R = np.eye(3) + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
        V = np.eye(3) + (1 - np.cos(theta)) / (theta * theta) * O + (theta - np.sin(theta)) / theta ** 3 * O2
    return R, V @ upsilon


class Model:
    def __init__(self, case, order=None):
        mp = np.asarray(case["mp_index"])
        self.feat = np.nonzero(mp >= 0)[0]
        self.n = len(mp)
        m = self.m = len(self.feat)
        self.Xw = np.asarray(case["world_pos"], np.float32).reshape(-1, 3)[mp[self.feat]].astype(np.float64)
        xy = np.asarray(case["xy"], np.float32).reshape(-1, 2)[self.feat].astype(np.float64)
        ur = np.asarray(case["uright"], np.float32)[self.feat]
        self.stereo = ur >= 0
        self.obs = np.concatenate([xy, ur.astype(np.float64)[:, None]], 1)
        self.info = np.asarray(case["inv_level_sigma2"], np.float32)[np.asarray(case["octave"])[self.feat]].astype(np.float64)
        self.fx, self.fy, self.cx, self.cy = [float(v) for v in np.asarray(case["K"], np.float32)]
        self.bf = float(np.float32(case["bf"]))
        self.delta = np.where(self.stereo, float(np.float32(np.sqrt(7.815))), float(np.float32(np.sqrt(5.991))))
        self.thr = np.where(self.stereo, np.float32(7.815), np.float32(5.991)).astype(np.float32)
        self.order = np.arange(m) if order is None else np.asarray(order)
        self.R0, self.t0 = quat_to_rot(case["q"]), np.asarray(case["t"], np.float32).astype(np.float64)

    def ordered_sum(self, contrib, mask):
        sel = self.order[mask[self.order]]
        if len(sel) == 0:
            return np.zeros(contrib.shape[1:])
        return np.cumsum(contrib[sel], 0)[-1]   # one after the other, in the caller's order

    def errors(self, R, t):
        """computeError of every edge (rows beyond an edge's dimension are 0), and the mapped points"""
        P = self.Xw @ R.T + t
        with np.errstate(all="ignore"):
            u = self.fx * P[:, 0] / P[:, 2] + self.cx
            v = self.fy * P[:, 1] / P[:, 2] + self.cy
            invz = (1.0 / P[:, 2]).astype(np.float32).astype(np.float64)   # `const float invz`, types_six_dof_expmap.cpp:340
            us = P[:, 0] * invz * self.fx + self.cx
            vs = P[:, 1] * invz * self.fy + self.cy
            e = np.where(self.stereo[:, None], self.obs - np.stack([us, vs, us - self.bf * invz], 1),
                         np.concatenate([self.obs[:, :2] - np.stack([u, v], 1), np.zeros((self.m, 1))], 1))
        return e, P

    def chi2_of(self, e):
        with np.errstate(all="ignore"):
            return np.einsum("ij,ij->i", e, self.info[:, None] * e)

    def robust(self, chi2, on):
        """RobustKernelHuber::robustify: rho[0], rho[1]"""
        if not on:
            return chi2.copy(), np.ones_like(chi2)
        d = self.delta
        with np.errstate(all="ignore"):
            s = np.sqrt(chi2)
            inl = chi2 <= d * d
            return np.where(inl, chi2, 2 * s * d - d * d), np.where(inl, 1.0, d / s)

    def jacobians(self, P):
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        A = np.zeros((self.m, 3, 6))
        with np.errstate(all="ignore"):
            # monocular: -projectJac * SE3deriv
            J = np.zeros((self.m, 2, 3))
            J[:, 0, 0], J[:, 0, 2] = self.fx / z, -self.fx * x / (z * z)
            J[:, 1, 1], J[:, 1, 2] = self.fy / z, -self.fy * y / (z * z)
            S = np.zeros((self.m, 3, 6))
            S[:, 0, 1], S[:, 0, 2], S[:, 0, 3] = z, -y, 1
            S[:, 1, 0], S[:, 1, 2], S[:, 1, 4] = -z, x, 1
            S[:, 2, 0], S[:, 2, 1], S[:, 2, 5] = y, -x, 1
            A[:, :2] = -np.einsum("mij,mjk->mik", J, S)
            # stereo: the table of types_six_dof_expmap.cpp:384-403
            iz = 1.0 / z
            iz2 = iz * iz
            B = np.zeros((self.m, 3, 6))
            B[:, 0] = np.stack([x * y * iz2 * self.fx, -(1 + x * x * iz2) * self.fx, y * iz * self.fx, -iz * self.fx, 0 * z, x * iz2 * self.fx], 1)
            B[:, 1] = np.stack([(1 + y * y * iz2) * self.fy, -x * y * iz2 * self.fy, -x * iz * self.fy, 0 * z, -iz * self.fy, y * iz2 * self.fy], 1)
            B[:, 2] = B[:, 0] + np.stack([-self.bf * y * iz2, self.bf * x * iz2, 0 * z, 0 * z, 0 * z, -self.bf * iz2], 1)
        A[self.stereo] = B[self.stereo]
        return A

    def run(self):
        m = self.m
        ev = dict(stale=0, rho_zero=0, ten_trials=0, nbad_stop=0, float_flip=0)
        res = dict(R=self.R0, t=self.t0, outlier=np.zeros(self.n, np.uint8), result=0, rounds=0, iterations=np.zeros(4, np.int32),
                   active=np.zeros(4, np.int32), chi2=np.zeros(4), events=ev, margin=np.inf, edge_chi2=[])
        if m < 3:
            return res
        level = np.zeros(m, bool)
        chi2 = np.zeros(m)
        x = np.zeros(6)
        n_bad = 0
        for rnd in range(4):
            R, t = self.R0, self.t0
            on = rnd < 3
            act = ~level
            n_act = int(act.sum())
            iters, cur = 0, 0.0
            last_rejected = False
            if n_act > 0:
                lam, ni, lm_bad = 0.0, 2.0, 0
                for it in range(10):
                    e, P = self.errors(R, t)
                    c = self.chi2_of(e)
                    chi2[act] = c[act]
                    rho0, rho1 = self.robust(c, on)
                    A = self.jacobians(P)
                    with np.errstate(all="ignore"):
                        Hc = np.einsum("mri,m,mrj->mij", A, rho1 * self.info, A).reshape(m, 36)
                        bc = -rho1[:, None] * np.einsum("mri,mr->mi", A, self.info[:, None] * e)
                    S = self.ordered_sum(np.concatenate([Hc, bc, rho0[:, None]], 1), act)
                    H, b, cur = S[:36].reshape(6, 6), S[36:42], S[42]
                    ini = cur
                    if it == 0:
                        lam, ni, lm_bad = 1e-5 * np.max(np.abs(np.diag(H))), 2.0, 0
                    rho, qmax = 0.0, 0
                    while True:
                        ok = True
                        try:
                            if not np.all(np.isfinite(H)):
                                raise np.linalg.LinAlgError
                            Lc = np.linalg.cholesky(H + lam * np.eye(6))
                            x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
                        except np.linalg.LinAlgError:
                            ok = False
                        Re, te = se3_exp(x)
                        Rt, tt = Re @ R, te + Re @ t
                        e2, _ = self.errors(Rt, tt)
                        c2 = self.chi2_of(e2)
                        chi2[act] = c2[act]
                        tmp = self.ordered_sum(self.robust(c2, on)[0][:, None], act)[0]
                        if not ok:
                            tmp = DBL_MAX
                        with np.errstate(all="ignore"):
                            rho = (cur - tmp) / (float(np.sum(x * (lam * x + b))) + 1e-3)
                        if rho > 0 and np.isfinite(tmp):
                            alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                            lam *= max(1.0 / 3.0, alpha)
                            ni = 2.0
                            cur, R, t = tmp, Rt, tt
                            last_rejected = False
                        else:
                            lam *= ni
                            ni *= 2
                            last_rejected = True
                        qmax += 1
                        if not (rho < 0 and qmax < 10):
                            break
                    iters += 1
                    if qmax == 10 or rho == 0:
                        ev["ten_trials"] += int(qmax == 10 and last_rejected)
                        ev["rho_zero"] += int(rho == 0)
                        break
                    lm_bad = lm_bad + 1 if (ini - cur) * 1e3 < ini else 0
                    if lm_bad >= 3:
                        ev["nbad_stop"] += 1
                        break
                ev["stale"] += int(last_rejected)
            # Optimizer.cc:1014-1100: outliers are re-evaluated at the round's estimate, active edges keep what they have
            e, _ = self.errors(R, t)
            c = self.chi2_of(e)
            chi2[level] = c[level]
            f32 = chi2.astype(np.float32)
            new_level = f32 > self.thr
            with np.errstate(all="ignore"):
                ev["float_flip"] += int(np.sum(new_level != (chi2 > self.thr.astype(np.float64))))
                res["margin"] = min(res["margin"], float(np.nanmin(np.abs(chi2 - self.thr) / self.thr)))
            res["edge_chi2"].append(chi2.copy())
            level = new_level
            n_bad = int(level.sum())
            res["iterations"][rnd], res["active"][rnd], res["chi2"][rnd], res["rounds"] = iters, n_act, cur, rnd + 1
            res["R"], res["t"] = R, t
            if m < 10:
                break
        res["outlier"][self.feat] = level
        res["result"] = m - n_bad
        return res


def run(case, order=None):
    return Model(case, order).run()
