"""A float64 numpy model of Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381) for pinhole key frames, written from the
reference's sources (include/OptimizableTypes.h:146-215, Thirdparty/g2o/g2o/types/sim3.h:70-146, :233-272,
core/base_binary_edge.hpp:55-205, core/optimization_algorithm_levenberg.cpp:61-194, core/robust_kernel_impl.cpp:78-91)
INDEPENDENTLY of csrc/sim3opt_math.h: the estimate is a rotation matrix, a translation and a scale (no quaternion anywhere),
the 7 x 7 system goes through numpy's Cholesky, exp / sin / cos are numpy's, and the edge pairs are summed in an order the
caller gives.  The numeric Jacobian is computed exactly as base_binary_edge.hpp does it - central differences, delta = 1e-9 -:
it is part of the function, not an approximation of it (jacobian="analytic" exists to record how far the two are apart).

run(case, descending=False, inverse="parts", jacobian="numeric") -> dict(R, t, s, result, cleared (per feature, 2 = no pair),
    the set-up counters, n_bad, iterations, active, chi2, rounds, events, margin, classified)
  inverse   "parts": the inverse edge maps through (R^T, -R^T t / s, 1 / s); "matrix": through the inverted 4 x 4 similarity
            matrix - two roundings of the same mathematics
  events    what the quirk tests assert happened: "stale" (round 1 classified by a rejected last trial), "ten_trials",
            "failed_solve", "nan_chi2" (a NaN chi2 that was classified as an inlier), "exhausted" (an optimize() that no
            stop criterion ended: it ran its max_it iterations)
  margin    the smallest |chi2 - th2| / th2 over every chi2 that is classified
  classified  those chi2, in the order they are classified (round 1: e12, e21 of every pair; the final loop likewise)"""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
f32 = np.float32


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def to_camera(R, t, X):
    """R * X + t in fp32 as Eigen evaluates it for a 3 x 3 times a 3-vector: ((r0 x + r1 y) + r2 z) + t"""
    R, t, X = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32), np.asarray(X, f32)
    return np.array([((R[i, 0] * X[0] + R[i, 1] * X[1]) + R[i, 2] * X[2]) + t[i] for i in range(3)], f32)


def sim3_exp(u):
    """Sim3(const Vector7d&) (sim3.h:70-142) as (R, t, s)"""
    omega, ups, sigma = u[:3], u[3:6], float(u[6])
    theta = float(np.linalg.norm(omega))
    O = skew(omega)
    O2 = O @ O
    s = float(np.exp(sigma))
    eps = 0.00001
    if theta < eps:
        # g2o never applies I + Omega + Omega^2: Quaterniond(R) keeps its antisymmetric part and its trace only, q = (omega / c,
        # c / 2) with c = sqrt(4 - 2 theta^2), and is NOT normalised; Eigen's q * v = v + 2 w (u x v) + 2 u x (u x v) then is
        # the matrix I + 2 w [u] + 2 [u]^2
        c = np.sqrt(4.0 - 2.0 * theta * theta)
        U = O / c
        R = np.eye(3) + c * U + 2.0 * (U @ U)
    else:
        R = np.eye(3) + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 0.5, 1.0 / 6.0
        else:
            A, B = (1 - np.cos(theta)) / theta ** 2, (theta - np.sin(theta)) / theta ** 3
    else:
        C = (s - 1) / sigma
        if theta < eps:
            A = ((sigma - 1) * s + 1) / sigma ** 2
            B = ((0.5 * sigma ** 2 - sigma + 1) * s) / sigma ** 3
        else:
            a, b, c = s * np.sin(theta), s * np.cos(theta), theta ** 2 + sigma ** 2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
    return R, (A * O + B * O2 + C * np.eye(3)) @ ups, s


def compose(a, b):
    """Sim3::operator* (sim3.h:266-272)"""
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


class Model:
    def __init__(self, case, descending=False, inverse="parts", jacobian="numeric"):
        self.inverse, self.jacobian = inverse, jacobian
        self.fix = bool(case["fix_scale"])
        self.th2 = float(f32(case["th2"]))
        self.delta = float(f32(np.sqrt(f32(case["th2"]))))
        self.K1 = [float(v) for v in np.asarray(case["K1"], f32)]
        self.K2 = [float(v) for v in np.asarray(case["K2"], f32)]
        self.S0 = (np.asarray(case["R"], np.float64).reshape(3, 3), np.asarray(case["t"], np.float64), float(case["s"]))
        # the set-up loop (:2167-2304)
        mp1, mt, i2s, lv2 = (np.asarray(case[k]) for k in ("mp1_index", "match_index", "i2", "track_level2"))
        bad, W = np.asarray(case["bad"]), np.asarray(case["world_pos"], f32).reshape(-1, 3)
        xy1, xy2 = np.asarray(case["xy1"], f32).reshape(-1, 2), np.asarray(case["xy2"], f32).reshape(-1, 2)
        o1, o2 = np.asarray(case["octave1"]), np.asarray(case["octave2"])
        sg1, sg2 = np.asarray(case["inv_level_sigma2_1"], f32), np.asarray(case["inv_level_sigma2_2"], f32)
        self.n = len(mt)
        cnt = dict(n_correspondences=0, n_bad_mps=0, n_in_kf2=0, n_out_kf2=0, n_without_mp=0)
        feat, X1, X2, ob1, ob2, in1, in2 = [], [], [], [], [], [], []
        for i in range(self.n):
            if mt[i] < 0:
                continue
            if mp1[i] < 0:
                cnt["n_without_mp"] += 1
                continue
            if bad[mp1[i]] or bad[mt[i]]:
                cnt["n_bad_mps"] += 1
                continue
            P1 = to_camera(case["Rcw1"], case["tcw1"], W[mp1[i]])
            P2 = to_camera(case["Rcw2"], case["tcw2"], W[mt[i]])
            if i2s[i] < 0 and not case["all_points"]:
                continue
            if P2[2] < 0:
                continue
            cnt["n_correspondences"] += 1
            if i2s[i] >= 0:
                cnt["n_in_kf2"] += 1
                obs2, lvl = xy2[i2s[i]], o2[i2s[i]]
            else:
                cnt["n_out_kf2"] += 1
                with np.errstate(all="ignore"):
                    invz = f32(1) / P2[2]
                    obs2, lvl = np.array([P2[0] * invz, P2[1] * invz], f32), lv2[i]
            feat.append(i); X1.append(P1); X2.append(P2); ob1.append(xy1[i]); ob2.append(obs2)
            in1.append(sg1[o1[i]]); in2.append(sg2[lvl])
        self.counters = cnt
        m = self.m = len(feat)
        self.feat = np.array(feat, np.int64)
        as64 = lambda a, w: np.array(a, np.float64).reshape(m, w) if w else np.array(a, np.float64).reshape(m)   # noqa: E731
        self.X1, self.X2, self.obs1, self.obs2 = as64(X1, 3), as64(X2, 3), as64(ob1, 2), as64(ob2, 2)
        self.info1, self.info2 = as64(in1, 0), as64(in2, 0)
        self.order = np.arange(m)[::-1] if descending else np.arange(m)

    # ---- the two edges ---------------------------------------------------------------------------------------------------
    @staticmethod
    def project(K, P):
        with np.errstate(all="ignore"):
            return np.stack([K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]], 1)

    def inverse_map(self, S, X):
        R, t, s = S
        if self.inverse == "parts":      # Sim3::inverse (:233-236) and map
            return (1.0 / s) * (X @ R) + (R.T @ ((-1.0 / s) * t))
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = s * R, t
        Mi = np.linalg.inv(M)
        return X @ Mi[:3, :3].T + Mi[:3, 3]

    def errors(self, S):
        R, t, s = S
        e12 = self.obs1 - self.project(self.K1, s * (self.X2 @ R.T) + t)
        e21 = self.obs2 - self.project(self.K2, self.inverse_map(S, self.X1))
        return e12, e21

    def chi2_of(self, e12, e21):
        with np.errstate(all="ignore"):
            # information() * _error is the full product: an infinite component makes the other one NaN
            c12 = np.einsum("ij,ij->i", e12, self.info1[:, None] * e12) + 0.0 * e12[:, 0] * e12[:, 1]
            c21 = np.einsum("ij,ij->i", e21, self.info2[:, None] * e21) + 0.0 * e21[:, 0] * e21[:, 1]
        return c12, c21

    def oplus(self, u, S):
        u = np.array(u, np.float64)
        if self.fix:
            u[6] = 0.0
        return compose(sim3_exp(u), S)

    def jacobians(self, S):
        """2 x 7 blocks of both edges: linearizeOplus of base_binary_edge.hpp, or the derivative in closed form"""
        m = self.m
        J12, J21 = np.zeros((m, 2, 7)), np.zeros((m, 2, 7))
        if self.jacobian == "numeric":
            delta = 1e-9
            scalar = 1.0 / (2 * delta)
            for d in range(7):
                u = np.zeros(7)
                u[d] = delta
                p12, p21 = self.errors(self.oplus(u, S))
                u[d] = -delta
                m12, m21 = self.errors(self.oplus(u, S))
                with np.errstate(all="ignore"):
                    J12[:, :, d], J21[:, :, d] = scalar * (p12 - m12), scalar * (p21 - m21)
            return J12, J21
        R, t, s = S
        for J, K, P, G in ((J12, self.K1, s * (self.X2 @ R.T) + t, None), (J21, self.K2, self.inverse_map(S, self.X1), self.X1)):
            with np.errstate(all="ignore"):
                x, y, z = P[:, 0], P[:, 1], P[:, 2]
                Jp = np.zeros((m, 2, 3))
                Jp[:, 0, 0], Jp[:, 0, 2] = K[0] / z, -K[0] * x / (z * z)
                Jp[:, 1, 1], Jp[:, 1, 2] = K[1] / z, -K[1] * y / (z * z)
                Q = P if G is None else G
                D = np.zeros((m, 3, 7))      # d(exp(u) Q) / du = [-[Q]x, I, Q]
                D[:, 0, 1], D[:, 0, 2], D[:, 1, 0], D[:, 1, 2], D[:, 2, 0], D[:, 2, 1] = Q[:, 2], -Q[:, 1], -Q[:, 2], Q[:, 0], Q[:, 1], -Q[:, 0]
                D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = 1.0
                D[:, :, 6] = Q
                if G is not None:            # S^-1 exp(-u) X1
                    D = -(1.0 / s) * np.einsum("ij,mjk->mik", R.T, D)
                if self.fix:
                    D[:, :, 6] = 0.0
                J[:] = -np.einsum("mij,mjk->mik", Jp, D)
        return J12, J21

    def robust(self, chi2, on):
        if not on:
            return chi2.copy(), np.ones_like(chi2)
        d = self.delta
        with np.errstate(all="ignore"):
            r = np.sqrt(chi2)
            inl = chi2 <= d * d
            return np.where(inl, chi2, 2 * r * d - d * d), np.where(inl, 1.0, d / r)

    def ordered_sum(self, contrib, mask):
        sel = self.order[mask[self.order]]
        if len(sel) == 0:
            return np.zeros(contrib.shape[1:])
        return np.cumsum(contrib[sel], 0)[-1]   # one after the other, in the caller's order

    # ---- SparseOptimizer::optimize with OptimizationAlgorithmLevenberg ----------------------------------------------------------
    def optimize(self, S, act, on, max_it, st):
        m = self.m
        iters, cur = 0, 0.0
        lam, ni, lm_bad = 0.0, 2.0, 0
        last_rejected = False
        for it in range(max_it):
            e12, e21 = self.errors(S)
            c12, c21 = self.chi2_of(e12, e21)
            st["c12"][act], st["c21"][act] = c12[act], c21[act]
            J12, J21 = self.jacobians(S)
            contrib = np.zeros((m, 49 + 7 + 1))
            with np.errstate(all="ignore"):
                for e, c, J, info in ((e12, c12, J12, self.info1), (e21, c21, J21, self.info2)):
                    rho0, rho1 = self.robust(c, on)
                    contrib[:, :49] += np.einsum("mri,m,mrj->mij", J, rho1 * info, J).reshape(m, 49)
                    contrib[:, 49:56] += np.einsum("mri,mr->mi", J, -(info[:, None] * e) * rho1[:, None])
                    contrib[:, 56] += rho0
            Sm = self.ordered_sum(contrib, act)
            H, b, cur = Sm[:49].reshape(7, 7), Sm[49:56], Sm[56]
            ini = cur
            if it == 0:
                lam, ni, lm_bad = 1e-5 * np.max(np.abs(np.diag(H))), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                ok = True
                try:
                    if not np.all(np.isfinite(H)) or not np.all(np.isfinite(b)):
                        raise np.linalg.LinAlgError
                    Lc = np.linalg.cholesky(H + lam * np.eye(7))
                    st["x"] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
                except np.linalg.LinAlgError:
                    ok = False
                    st["events"]["failed_solve"] += 1
                x = st["x"]
                if self.fix:
                    x[6] = 0.0
                St = self.oplus(x, S)
                t12, t21 = self.chi2_of(*self.errors(St))
                st["c12"][act], st["c21"][act] = t12[act], t21[act]
                tmp = self.ordered_sum((self.robust(t12, on)[0] + self.robust(t21, on)[0])[:, None], act)[0]
                if not ok:
                    tmp = DBL_MAX
                with np.errstate(all="ignore"):
                    rho = (cur - tmp) / (float(np.sum(x * (lam * x + b))) + 1e-3)
                if rho > 0 and np.isfinite(tmp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur, S = tmp, St
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
                st["events"]["ten_trials"] += int(qmax == 10)
                break
            lm_bad = lm_bad + 1 if (ini - cur) * 1e3 < ini else 0
            if lm_bad >= 3:
                break
        else:
            st["events"]["exhausted"] += 1   # no stop criterion met: max_it ended the loop
        return S, iters, cur, last_rejected

    def run(self):
        m, th2 = self.m, self.th2
        ev = dict(stale=0, ten_trials=0, failed_solve=0, nan_chi2=0, exhausted=0)
        st = dict(c12=np.zeros(m), c21=np.zeros(m), x=np.zeros(7), events=ev)
        res = dict(R=self.S0[0], t=self.S0[1], s=self.S0[2], result=0, cleared=np.full(self.n, 2, np.uint8), n_bad=0,
                   iterations=np.zeros(2, np.int32), active=np.zeros(2, np.int32), chi2=np.zeros(2), rounds=1, events=ev,
                   margin=np.inf, classified=[], **self.counters)
        S = self.S0
        gone = np.zeros(m, bool)
        res["active"][0] = m
        if m > 0:
            S, res["iterations"][0], res["chi2"][0], rejected = self.optimize(S, ~gone, True, 5, st)
            ev["stale"] += int(rejected)

        def classify(mask):
            c = np.stack([st["c12"][mask], st["c21"][mask]], 1).reshape(-1)
            res["classified"].append(c)
            ev["nan_chi2"] += int(np.isnan(c).sum())
            with np.errstate(all="ignore"):
                if np.isfinite(c).any():
                    res["margin"] = min(res["margin"], float(np.nanmin(np.abs(c[np.isfinite(c)] - th2) / th2)))
                return (st["c12"] > th2) | (st["c21"] > th2)
        over = classify(~gone)
        gone = over.copy()
        cleared = over.copy()
        n_bad = res["n_bad"] = int(gone.sum())
        res["cleared"][self.feat] = cleared
        if m - n_bad < 10:
            return res
        res["active"][1] = m - n_bad
        S, res["iterations"][1], res["chi2"][1], _ = self.optimize(S, ~gone, False, 10 if n_bad > 0 else 5, st)
        c12, c21 = self.chi2_of(*self.errors(S))
        st["c12"][~gone], st["c21"][~gone] = c12[~gone], c21[~gone]
        over = classify(~gone) & ~gone
        cleared |= over
        res["cleared"][self.feat] = cleared
        res.update(R=S[0], t=S[1], s=S[2], result=int((~gone & ~over).sum()), rounds=2)
        return res


def run(case, descending=False, inverse="parts", jacobian="numeric"):
    return Model(case, descending, inverse, jacobian).run()


def quat_to_rot(q):
    """the matrix Eigen's q * v applies (the quaternion is not normalised: g2o::Sim3 never does)"""
    x, y, z, w = [float(v) for v in np.asarray(q, np.float64)]
    U = skew([x, y, z])
    return np.eye(3) + 2.0 * w * U + 2.0 * (U @ U)


def difference(a, b):
    """the largest difference of two estimates (dicts with R, t, s): any entry of R, t relative to max(1, |t|), s relative"""
    dt = float(np.abs(a["t"] - b["t"]).max() / max(1.0, float(np.linalg.norm(b["t"]))))
    return max(float(np.abs(a["R"] - b["R"]).max()), dt, abs(a["s"] - b["s"]) / abs(b["s"]))
