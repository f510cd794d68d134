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


def _small_rot(rng, lo, hi):
    return cases._rot(cases._quat(rng.normal(size=3), rng.uniform(lo, hi)))


def make_sim3_opt_case(n=300, matched=150, seed=1, fix_scale=False, all_points=False, th2=10.0, outlier_share=0.1, pixel_noise=0.5,
                       n_levels=8, scale_factor=1.2, out_kf2_share=0.0, null_mp1_share=0.0, bad_share=0.0, n_behind=0, n_on_plane=0,
                       identity_poses=False, rot_noise=(0.02, 0.06), trans_noise=0.03, scale_noise=0.03, depth=(4.0, 60.0)):
    """Two key frames as Optimizer::OptimizeSim3 reads them (Optimizer.cc:2115-2381), deterministic by seed: `matched` of key frame
    1's n features carry a match; the frames are 0.5 - 3 m apart and see the common points at `depth` metres (KITTI camera, octaves
    0 .. n_levels - 1, `pixel_noise` x the level's sigma of noise on both observations); `outlier_share` of the matches are gross
    outliers (30 - 80 px).  The entry estimate (R, t, s) is the truth perturbed by rot_noise radians, trans_noise metres and
    scale_noise relative (s = 1 exactly under fix_scale).  Shares of the matches are not observed in key frame 2 (i2 = -1), have
    no map point in key frame 1 (mp1_index = -1) or name a bad point; with identity_poses (Rcw = I, tcw = 0: the world
    positions are the camera-frame points) n_behind matches get P3D2c(2) < 0 and n_on_plane get exactly 0; the latter are the
    first to lose their index in key frame 2 (with i2 < 0 their normalised observation is not finite).
    Keys: the problem dict of frontend.ORBmatcher.OptimizeSim3 plus the plant (R_true, t_true, s_true, planted_outlier per
    feature)."""
    rng = np.random.default_rng(seed)
    cam = cases._kitti_camera()
    fx, fy, cx, cy = [float(v) for v in cam.K]
    K = np.array([fx, fy, cx, cy], f32)
    assert matched <= n and (identity_poses or n_behind + n_on_plane == 0) and n_behind + n_on_plane <= matched
    R12 = _small_rot(rng, 0.02, 0.3)
    d = rng.normal(size=3)
    t12 = d / np.linalg.norm(d) * rng.uniform(0.5, 3.0)
    s12 = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    z = rng.uniform(depth[0], depth[1], matched)
    u = rng.uniform(60.0, cam.w - 60.0, matched)
    v = rng.uniform(60.0, cam.h - 60.0, matched)
    X1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    X2 = (X1 - t12) @ R12 / s12
    if identity_poses:
        Rcw1, tcw1, Rcw2, tcw2 = np.eye(3, dtype=f32), np.zeros(3, f32), np.eye(3, dtype=f32), np.zeros(3, f32)
    else:
        Rcw1, tcw1 = _small_rot(rng, 0.0, 0.5).astype(f32), rng.uniform(-3.0, 3.0, 3).astype(f32)
        Rcw2, tcw2 = _small_rot(rng, 0.0, 0.5).astype(f32), rng.uniform(-3.0, 3.0, 3).astype(f32)
    Xw1 = ((X1 - tcw1.astype(np.float64)) @ Rcw1.astype(np.float64)).astype(f32)
    Xw2 = ((X2 - tcw2.astype(np.float64)) @ Rcw2.astype(np.float64)).astype(f32)
    sigma2 = np.array([scale_factor ** i for i in range(n_levels)], f32) ** 2
    inv_sigma2 = (f32(1.0) / sigma2).astype(f32)
    feat = np.sort(rng.permutation(n)[:matched])          # the matched features of key frame 1, ascending
    n2 = matched + matched // 4 + 3
    i2 = rng.permutation(n2)[:matched].astype(np.int32)
    oct1 = rng.integers(0, n_levels, n).astype(np.int32)
    oct2 = rng.integers(0, n_levels, n2).astype(np.int32)
    xy1 = np.stack([rng.uniform(0, cam.w, n), rng.uniform(0, cam.h, n)], 1)
    xy2 = np.stack([rng.uniform(0, cam.w, n2), rng.uniform(0, cam.h, n2)], 1)
    p1 = np.stack([fx * X1[:, 0] / X1[:, 2] + cx, fy * X1[:, 1] / X1[:, 2] + cy], 1)
    p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    p1 += rng.normal(size=(matched, 2)) * (pixel_noise * np.sqrt(sigma2[oct1[feat]].astype(np.float64)))[:, None]
    p2 += rng.normal(size=(matched, 2)) * (pixel_noise * np.sqrt(sigma2[oct2[i2]].astype(np.float64)))[:, None]
    gross = rng.random(matched) < outlier_share
    ng = int(gross.sum())
    ang = rng.uniform(0, 2 * np.pi, ng)
    off = rng.uniform(30.0, 80.0, ng)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    side = rng.random(ng) < 0.5
    p1[gross] += off * side[:, None]
    p2[gross] += off * ~side[:, None]
    xy1[feat] = p1
    xy2[i2] = p2
    # the special matches, from the front of a seeded order
    order = rng.permutation(matched)
    take = iter(order)
    behind = np.array([next(take) for _ in range(n_behind)], np.int64)
    plane = np.array([next(take) for _ in range(n_on_plane)], np.int64)
    Xw2[behind, 2] = -np.abs(Xw2[behind, 2])
    Xw2[plane, 2] = 0.0
    n_out, n_null, n_badp = (int(round(sh * matched)) for sh in (out_kf2_share, null_mp1_share, bad_share))
    out_kf2 = order[n_behind:n_behind + n_out]            # the matches on the plane are the first not to be seen in key frame 2
    rest = order[n_behind + max(n_on_plane, n_out):]
    null1, badp = rest[:n_null], rest[n_null:n_null + n_badp]
    i2 = i2.copy()
    i2[out_kf2] = -1
    mp1_index = np.full(n, -1, np.int32)
    match_index = np.full(n, -1, np.int32)
    i2_f = np.full(n, -1, np.int32)
    lvl2_f = np.zeros(n, np.int32)
    mp1_index[feat] = np.arange(matched)
    mp1_index[feat[null1]] = -1
    match_index[feat] = matched + np.arange(matched)
    i2_f[feat] = i2
    lvl2_f[feat] = rng.integers(0, n_levels, matched)
    # unmatched features of key frame 1 may still hold a map point of their own
    bad = np.zeros(2 * matched, np.uint8)
    bad[np.where(rng.random(len(badp)) < 0.5, badp, matched + badp)] = 1
    planted = np.zeros(n, np.uint8)
    planted[feat] = gross
    # the entry estimate
    Re = _small_rot(rng, rot_noise[0], rot_noise[1]) @ R12 if rot_noise[1] > 0 else R12.copy()
    te = t12 + rng.normal(size=3) * trans_noise
    se = 1.0 if fix_scale else s12 * (1.0 + float(rng.uniform(-scale_noise, scale_noise)))
    return dict(mp1_index=mp1_index, match_index=match_index, i2=i2_f, track_level2=lvl2_f, bad=bad,
                world_pos=np.concatenate([Xw1, Xw2]), Rcw1=Rcw1, tcw1=tcw1, Rcw2=Rcw2, tcw2=tcw2,
                xy1=xy1.astype(f32), octave1=oct1, xy2=xy2.astype(f32), octave2=oct2, n2=n2,
                inv_level_sigma2_1=inv_sigma2, inv_level_sigma2_2=inv_sigma2.copy(), K1=K, K2=K.copy(),
                R=Re, t=te, s=float(se), th2=f32(th2), fix_scale=int(bool(fix_scale)), all_points=int(bool(all_points)),
                R_true=R12, t_true=t12, s_true=s12, planted_outlier=planted)
