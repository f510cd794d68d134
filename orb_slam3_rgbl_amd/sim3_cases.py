"""Seeded problems for rgbl_sim3_ransac (Sim3Solver, src/Sim3Solver.cc): two key frames that see the same points, related by a
planted similarity, as the solver's constructor (:35-121) leaves them."""
import numpy as np

from . import cases

f32 = np.float32


def to_camera(R, t, Xw):
    """Rcw * Xw + tcw in fp32, in the order of csrc/sim3_math.h (s3_transform): ((r0 x + r1 y) + r2 z) + t"""
    R, t, Xw = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32), np.asarray(Xw, f32).reshape(-1, 3)
    out = np.empty_like(Xw)
    for i in range(3):
        out[:, i] = ((R[i, 0] * Xw[:, 0] + R[i, 1] * Xw[:, 1]) + R[i, 2] * Xw[:, 2]) + t[i]
    return out


def draw_samples(rng, n, n_hyp):
    """n_hyp triples as Sim3Solver::iterate draws them (:172-186): an index into the available ones, swap with the last, pop"""
    out = np.zeros((n_hyp, 3), np.int32)
    for k in range(n_hyp):
        avail = list(range(n))
        for i in range(3):
            r = int(rng.integers(0, len(avail)))
            out[k, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def make_sim3_case(n=150, n_hyp=300, seed=1, fix_scale=False, outlier_share=0.3, pixel_noise=0.3, n_levels=8, scale_factor=1.2,
                   min_inliers=20, best_inliers=0, scale=None):
    """n correspondences of key frame 1 (KITTI camera, points 4 - 40 m in front) and key frame 2, X1c = s R X2c + t with a planted
    (R, t, s); the inliers carry `pixel_noise` x their level's sigma of lateral noise in image 2, a share of outliers is displaced
    by 30 - 80 px; octaves 0 .. n_levels - 1 on both sides give the thresholds (size_t)(9.210 * sigma2) (:99-100).  The points live in a world frame
    (Xw1, Xw2, float) under two key-frame poses; x1c / x2c are Rcw * Xw + tcw in fp32, which is what the pool form computes.
    Keys: the problem dict of frontend.ORBmatcher.Sim3Ransac plus the plant (R_true, t_true, s_true, planted_outlier) and the
    world form (Xw1, Xw2, Rcw1, tcw1, Rcw2, tcw2)."""
    rng = np.random.default_rng(seed)
    cam = cases._kitti_camera()
    fx, fy, cx, cy = [float(v) for v in cam.K]
    K = np.array([fx, fy, cx, cy], f32)
    # the plant
    R12 = cases._rot(cases._quat(rng.normal(size=3), rng.uniform(0.05, 0.3)))
    t12 = rng.uniform(-1.0, 1.0, 3)
    s12 = 1.0 if fix_scale else (float(scale) if scale is not None else float(rng.uniform(0.8, 1.25)))
    # camera frame 1, then camera frame 2: X2 = R^T (X1 - t) / s
    z = rng.uniform(4.0, 40.0, n)
    u = rng.uniform(40.0, cam.w - 40.0, n)
    v = rng.uniform(40.0, cam.h - 40.0, n)
    X1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    X2 = (X1 - t12) @ R12 / s12
    oct1 = rng.integers(0, n_levels, n)
    oct2 = rng.integers(0, n_levels, n)
    sigma2 = np.array([scale_factor ** i for i in range(n_levels)], f32) ** 2
    # mvnMaxError1 / 2 are std::vector<size_t> (include/Sim3Solver.h:78-79): 9.210 * sigma2 is truncated before the comparison
    max_err1 = np.floor(9.210 * sigma2[oct1].astype(np.float64)).astype(f32)
    max_err2 = np.floor(9.210 * sigma2[oct2].astype(np.float64)).astype(f32)
    # lateral noise in image 2, in pixels
    px = rng.normal(size=(n, 2)) * (pixel_noise * np.sqrt(sigma2[oct2].astype(np.float64)))[:, None]
    gross = rng.random(n) < outlier_share
    ng = int(gross.sum())
    ang = rng.uniform(0, 2 * np.pi, ng)
    px[gross] += (rng.uniform(30.0, 80.0, ng)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))
    X2 = X2 + np.stack([px[:, 0] * X2[:, 2] / fx, px[:, 1] * X2[:, 2] / fy, np.zeros(n)], 1)
    # the world form: two key-frame poses, world points stored as float
    Rcw1 = cases._rot(cases._quat(rng.normal(size=3), rng.uniform(0.0, 0.5))).astype(f32)
    tcw1 = rng.uniform(-3.0, 3.0, 3).astype(f32)
    Rcw2 = cases._rot(cases._quat(rng.normal(size=3), rng.uniform(0.0, 0.5))).astype(f32)
    tcw2 = rng.uniform(-3.0, 3.0, 3).astype(f32)
    Xw1 = ((X1 - tcw1.astype(np.float64)) @ Rcw1.astype(np.float64)).astype(f32)
    Xw2 = ((X2 - tcw2.astype(np.float64)) @ Rcw2.astype(np.float64)).astype(f32)
    samples = draw_samples(rng, n, n_hyp) if n >= 3 else np.zeros((n_hyp, 3), np.int32)
    return dict(x1c=to_camera(Rcw1, tcw1, Xw1), x2c=to_camera(Rcw2, tcw2, Xw2), max_err1=max_err1, max_err2=max_err2, K1=K, K2=K.copy(),
                fix_scale=int(bool(fix_scale)), min_inliers=int(min_inliers), best_inliers=int(best_inliers), samples=samples,
                n=n, n_hyp=n_hyp,
                R_true=R12, t_true=t12, s_true=s12, planted_outlier=gross.astype(np.uint8),
                Xw1=Xw1, Xw2=Xw2, Rcw1=Rcw1, tcw1=tcw1, Rcw2=Rcw2, tcw2=tcw2)


PROBLEM_KEYS = ("x1c", "x2c", "max_err1", "max_err2", "K1", "K2", "fix_scale", "min_inliers", "best_inliers", "samples", "n", "n_hyp")


def problem(case, **over):
    """the C ABI's part of a case (host arrays)"""
    return dict({k: case[k] for k in PROBLEM_KEYS}, **over)


def pool_problem(case, pool, slot1, slot2, **over):
    """the same problem with the points taken from a MapPointPool that holds Xw1 at slot1 and Xw2 at slot2"""
    p = {k: case[k] for k in PROBLEM_KEYS if k not in ("x1c", "x2c")}
    p.update(pool=pool, slot1=slot1, slot2=slot2, Rcw1=case["Rcw1"], tcw1=case["tcw1"], Rcw2=case["Rcw2"], tcw2=case["tcw2"])
    p.update(over)
    return p
