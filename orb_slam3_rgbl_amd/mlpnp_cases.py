"""Seeded problems for rgbl_mlpnp_ransac (MLPnPsolver, src/MLPnPsolver.cpp): a frame whose features carry map-point matches, as
Tracking::Relocalization hands them to the solver's constructor (:55-97), with a planted pose."""
import math

import numpy as np

from . import cases

f32 = np.float32


def ransac_parameters(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5):
    """SetRansacParameters (:225-260) with the values Tracking::Relocalization passes (0.99, 10, 300, 6, 0.5, 5.991):
    (mRansacMinInliers, mRansacMaxIts).  The iteration count uses pow(epsilon, 3) although the minimal set is 6."""
    n_min = max(int(N * f32(epsilon)), min_inliers, min_set)
    eps = f32(epsilon)
    if N > 0 and eps < f32(n_min) / f32(N):
        eps = f32(n_min) / f32(N)
    if n_min == N:
        its = 1
    elif float(eps) ** 3 >= 1.0:     # N < mRansacMinInliers: the logarithm of a negative number; iterate leaves before it matters
        its = max_iterations
    else:
        its = int(math.ceil(math.log(1 - probability) / math.log(1 - float(eps) ** 3)))
    return n_min, max(1, min(its, max_iterations))


def calls_n_hyp(max_its, iterations_so_far, n_iterations):
    """what a call that does not succeed runs: the loop condition is `mnIterations < mRansacMaxIts || nCurrentIterations <
    nIterations` (:115)"""
    return max(max_its - iterations_so_far, n_iterations)


def draw_samples(rng, N, n_hyp):
    """n_hyp six-sets as MLPnPsolver::iterate draws them (:128-140): an index into the available ones, swap with the last, pop"""
    out = np.zeros((n_hyp, 6), np.int32)
    for k in range(n_hyp):
        avail = list(range(N))
        for i in range(6):
            r = int(rng.integers(0, len(avail)))
            out[k, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def make_mlpnp_case(N=100, n_hyp=35, seed=1, outlier_share=0.3, pixel_noise=0.3, n_levels=8, scale_factor=1.2, th2=5.991,
                    min_inliers=None, planar=False, n_on_plane=0, identity=False, n_behind=0, extra_features=None):
    """A frame of n features (KITTI camera) of which N carry a map point (the others: mp_index = -1); the points lie 4 - 40 m in
    front of the planted pose Tcw_true; the inliers carry `pixel_noise` x their level's sigma of noise, a share of outliers is
    displaced by 30 - 80 px.  planar: every world point has z == 0 exactly and x, y on a grid of 1 / 64 (the uncentred
    planarity matrix then has an exactly zero third pivot); n_on_plane: only the first n_on_plane correspondences do;
    identity: Tcw_true is exactly the identity and the inliers carry no noise; n_behind: the last n_behind correspondences lie
    behind the camera and are observed where their mirror image projects (no depth-sign test: they can be inliers).
    min_inliers: default SetRansacParameters' value for N.  Keys: the problem dict of frontend.ORBmatcher.MLPnPRansac plus the
    plant (R_true, t_true, planted_outlier per correspondence, feat: the feature of each correspondence, extent)."""
    rng = np.random.default_rng(seed)
    cam = cases._kitti_camera()
    fx, fy, cx, cy = [float(v) for v in cam.K]
    K = np.array([fx, fy, cx, cy], f32)
    if identity:
        R, t = np.eye(3), np.zeros(3)
    elif planar:
        R = cases._rot(cases._quat(rng.normal(size=3), rng.uniform(0.1, 0.4)))
        t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(10.0, 14.0)])
    else:
        R = cases._rot(cases._quat(rng.normal(size=3), rng.uniform(0.05, 0.6)))
        t = rng.uniform(-2.0, 2.0, 3)
    if planar:
        Xw = np.stack([np.round(rng.uniform(-6.0, 6.0, N) * 64) / 64, np.round(rng.uniform(-2.5, 2.5, N) * 64) / 64, np.zeros(N)], 1)
    else:
        z = rng.uniform(4.0, 40.0, N)
        u = rng.uniform(40.0, cam.w - 40.0, N)
        v = rng.uniform(40.0, cam.h - 40.0, N)
        Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        Xw = (Xc - t) @ R
        k = min(n_on_plane, N)
        Xw[:k] = np.stack([np.round(Xw[:k, 0] * 64) / 64, np.round(Xw[:k, 1] * 64) / 64, np.zeros(k)], 1)
    Xw = Xw.astype(f32)
    Xc = Xw.astype(np.float64) @ R.T + t
    if n_behind:
        Xc[N - n_behind:] = -Xc[N - n_behind:]            # the mirror image: the same projection
        Xw[N - n_behind:] = ((Xc[N - n_behind:] - t) @ R).astype(f32)
        Xc = Xw.astype(np.float64) @ R.T + t
    n = N + (extra_features if extra_features is not None else N // 4 + 2)
    feat = np.sort(rng.permutation(n)[:N]).astype(np.int32)
    octave = rng.integers(0, n_levels, n).astype(np.int32)
    sigma2 = (np.array([scale_factor ** i for i in range(n_levels)], f32) ** 2).astype(f32)
    xy = np.stack([rng.uniform(0, cam.w, n), rng.uniform(0, cam.h, n)], 1)
    p = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    if not identity:
        p += rng.normal(size=(N, 2)) * (pixel_noise * np.sqrt(sigma2[octave[feat]].astype(np.float64)))[:, None]
    gross = rng.random(N) < outlier_share
    ng = int(gross.sum())
    ang = rng.uniform(0, 2 * np.pi, ng)
    p[gross] += rng.uniform(30.0, 80.0, ng)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    xy[feat] = p
    mp_index = np.full(n, -1, np.int32)
    order = rng.permutation(N).astype(np.int32)           # the map side is not in feature order
    mp_index[feat] = order
    world_pos = np.zeros((N, 3), f32)
    world_pos[order] = Xw
    if min_inliers is None:
        min_inliers = ransac_parameters(N)[0]
    samples = draw_samples(rng, N, n_hyp) if N >= 6 else np.zeros((n_hyp, 6), np.int32)
    extent = float(np.abs(Xw).max()) if N else 1.0
    return dict(mp_index=mp_index, world_pos=world_pos, xy=xy.astype(f32), octave=octave, K=K, level_sigma2=sigma2, th2=f32(th2),
                min_inliers=int(min_inliers), best_inliers=0, best_mask=None, best_Tcw=np.eye(4, dtype=f32), samples=samples,
                n_hyp=n_hyp, R_true=R, t_true=t, planted_outlier=gross.astype(np.uint8), feat=feat, extent=extent, N=N)


def make_exact_identity_case(N=40, n_hyp=35, seed=3):
    """A scene whose true pose is exactly the identity and whose observations are exact in float: K = (512, 512, 320, 240), depths
    4 .. 10 and lateral coordinates on a grid, one level, every feature with its map point.  The linear solution is then the
    identity up to rounding; where its trace rounds to 3 or past it, rot2rodrigues gives w = 0 (acos of an argument past 1 is
    NaN and fails the guard), the Jacobian there is NaN, the solve fails and x stays: the w = 0 path."""
    rng = np.random.default_rng(seed)
    K = f32([512, 512, 320, 240])
    z = rng.integers(2, 6, N).astype(f32) * 2
    X = np.stack([rng.integers(-16, 17, N) / 8 * z / 4, rng.integers(-12, 13, N) / 8 * z / 4, z], 1).astype(f32)
    xy = np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1).astype(f32)
    return dict(mp_index=np.arange(N, dtype=np.int32), world_pos=X, xy=xy, octave=np.zeros(N, np.int32), K=K, level_sigma2=f32([1.0]),
                th2=f32(5.991), min_inliers=N // 2, best_inliers=0, best_mask=None, best_Tcw=np.eye(4, dtype=f32),
                samples=draw_samples(rng, N, n_hyp), n_hyp=n_hyp, N=N)


PROBLEM_KEYS = ("mp_index", "world_pos", "xy", "octave", "K", "level_sigma2", "th2", "min_inliers", "best_inliers", "best_mask", "best_Tcw",
                "samples", "n_hyp")


def problem(case, **over):
    """the C ABI's part of a case (host arrays)"""
    return dict({k: case[k] for k in PROBLEM_KEYS}, **over)


def pool_problem(case, pool, slot, **over):
    """the same problem with the map side taken from a MapPointPool that holds world_pos[i] at slot[i]"""
    p = {k: case[k] for k in PROBLEM_KEYS if k != "world_pos"}
    p.update(pool=pool, slot=slot, n_points=len(slot))
    p.update(over)
    return p


def correspondences(pr):
    """what the constructor collects, per correspondence in ascending feature index: feature, pixel, octave, world point"""
    mp = np.asarray(pr["mp_index"], np.int32)
    feat = np.nonzero(mp >= 0)[0].astype(np.int32)
    return feat, np.asarray(pr["xy"], f32)[feat], np.asarray(pr["octave"], np.int32)[feat], np.asarray(pr["world_pos"], f32).reshape(-1, 3)[mp[feat]]
