"""Seeded problems for rgbl_local_bundle_adjustment (Optimizer::LocalBundleAdjustment, src/Optimizer.cc:1116-1498): a local
window of key frames on a KITTI-like forward drive, the map points they see and the fixed key frames around them, as the
vertices and edges the reference hands to g2o."""
import numpy as np

from . import cases

f32 = np.float32


def make_lba_case(n_free=3, n_fixed=2, n_points=40, obs_per_point=3, seed=1, stereo_share=0.6, pixel_noise=0.4,
                  pose_noise=(0.004, 0.03), point_noise=0.03, outlier_share=0.0, n_levels=8, scale_factor=1.2, step=0.7,
                  max_iterations=10):
    """n_free + n_fixed pinhole cameras (KITTI's K and bf) `step` metres apart along the viewing direction, the fixed ones
    first on the road and the free ones ahead of them; n_points points 6 - 40 m in front of the window, each observed by
    obs_per_point cameras (an int, or a (low, high) range drawn per point; at most one edge per camera, in ascending camera
    index).  A stereo_share of the edges carries mvuRight, the others are monocular (ur = -1).  Observations carry
    pixel_noise x their level's sigma of noise and an outlier_share of them 15 - 60 px more; the free cameras start
    pose_noise = (radians, metres) and the points point_noise metres off the plant.  Fixed cameras are given at the plant.
    Keys: the case dict of frontend.local_bundle_adjustment_call plus the plant (q_true, t_true, X_true, planted_outlier)."""
    rng = np.random.default_rng(seed)
    cam = cases._kitti_camera()
    fx, fy, cx, cy = [float(v) for v in cam.K]
    bf = float(cam.mbf)
    nC = n_free + n_fixed
    # the plant: world = the first camera's frame; camera c sits at z = step * road[c], with a small rotation
    road = np.concatenate([np.arange(n_fixed, nC), np.arange(n_fixed)])   # free cameras (list order) ahead, fixed behind
    q_true = np.zeros((nC, 4))
    t_true = np.zeros((nC, 3))
    R_true = np.zeros((nC, 3, 3))
    for c in range(nC):
        q = cases._quat(rng.normal(size=3), rng.uniform(0.0, 0.05)).astype(np.float64)
        R = cases._rot(q)
        centre = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05), step * road[c]])
        q_true[c], R_true[c], t_true[c] = q, R, -R @ centre
    z = rng.uniform(6.0, 40.0, n_points) + step * (nC - 1)
    u = rng.uniform(60.0, cam.w - 60.0, n_points)
    v = rng.uniform(40.0, cam.h - 40.0, n_points)
    zc = z - step * (nC - 1) / 2.0
    X_true = np.stack([(u - cx) / fx * zc, (v - cy) / fy * zc, z], 1)
    sigma2 = np.array([scale_factor ** i for i in range(n_levels)], np.float64) ** 2
    edge_point, edge_cam, edge_obs, edge_info, planted = [], [], [], [], []
    for p in range(n_points):
        k = obs_per_point if np.isscalar(obs_per_point) else int(rng.integers(obs_per_point[0], obs_per_point[1] + 1))
        k = min(int(k), nC)
        for c in sorted(rng.choice(nC, k, replace=False)):
            P = R_true[c] @ X_true[p] + t_true[c]
            octave = int(rng.integers(0, n_levels))
            sd = pixel_noise * np.sqrt(sigma2[octave])
            out = rng.uniform() < outlier_share
            d = rng.normal(size=3) * sd
            if out:
                d[:2] += rng.choice([-1.0, 1.0], 2) * rng.uniform(15.0, 60.0, 2)
            uu = fx * P[0] / P[2] + cx + d[0]
            vv = fy * P[1] / P[2] + cy + d[1]
            ur = uu - bf / P[2] + d[2] if rng.uniform() < stereo_share else -1.0
            edge_point.append(p); edge_cam.append(int(c)); edge_obs.append([uu, vv, ur])
            edge_info.append(1.0 / sigma2[octave]); planted.append(out)
    # where the optimisation starts
    cam_q = q_true.copy()
    cam_t = t_true.copy()
    for c in range(n_free):
        dq = cases._quat(rng.normal(size=3), rng.normal() * pose_noise[0]).astype(np.float64)
        R = cases._rot(dq) @ R_true[c]
        cam_q[c] = _quat_of(R)
        cam_t[c] = cases._rot(dq) @ t_true[c] + rng.normal(size=3) * pose_noise[1]
    world_pos = X_true + rng.normal(size=X_true.shape) * point_noise
    return dict(n_free=n_free, n_fixed=n_fixed, free_is_fixed=np.zeros(n_free, np.uint8), cam_q=cam_q.astype(f32),
                cam_t=cam_t.astype(f32), cam_K=np.tile(np.array([fx, fy, cx, cy], f32), (nC, 1)),
                cam_bf=np.full(nC, bf, f32), world_pos=world_pos.astype(f32),
                edge_point=np.array(edge_point, np.int32), edge_cam=np.array(edge_cam, np.int32),
                edge_obs=np.array(edge_obs, f32).reshape(-1, 3), edge_inv_sigma2=np.array(edge_info, f32),
                max_iterations=max_iterations, user_lambda_init=0.0, stop_after_polls=0,
                q_true=q_true, t_true=t_true, X_true=X_true, planted_outlier=np.array(planted, bool))


def make_ba_case(n_cams=5, n_fixed=1, robust=1, max_iterations=10, **kw):
    """make_lba_case's scene as Optimizer::BundleAdjustment sees it (src/Optimizer.cc:52-390): ONE camera list in the order
    of the road, the first n_fixed of them flagged fixed (the map's initial key frame, :125) and given at the plant, the
    others free.  kw goes to make_lba_case (n_points, obs_per_point, seed, ...).  Keys: the case dict of
    frontend.bundle_adjustment_call plus the plant."""
    c = make_lba_case(n_free=n_cams - n_fixed, n_fixed=n_fixed, max_iterations=max_iterations, **kw)
    nf = n_cams - n_fixed
    order = np.concatenate([np.arange(nf, n_cams), np.arange(nf)])      # fixed cameras first
    new_index = np.empty(n_cams, np.int64)
    new_index[order] = np.arange(n_cams)
    out = {k: c[k] for k in ("world_pos", "edge_point", "edge_obs", "edge_inv_sigma2", "max_iterations", "stop_after_polls",
                             "X_true", "planted_outlier")}
    for k in ("cam_q", "cam_t", "cam_K", "cam_bf", "q_true", "t_true"):
        out[k] = c[k][order]
    # a point's edges stay in ascending camera index (the order the reference walks GetObservations is the caller's)
    cam = new_index[c["edge_cam"]]
    key = np.lexsort((cam, c["edge_point"]))
    for k in ("edge_obs", "edge_inv_sigma2", "planted_outlier"):
        out[k] = c[k][key]
    out["edge_point"] = c["edge_point"][key]
    out["edge_cam"] = cam[key].astype(np.int32)
    fixed = np.zeros(n_cams, np.uint8)
    fixed[:n_fixed] = 1
    out.update(n_cams=n_cams, cam_is_fixed=fixed, robust=robust)
    return out


def as_lba_case(ba):
    """a make_ba_case dict as the rgbl_local_bundle_adjustment call on the same vertices and edges: every camera in the free
    list, the fixed ones flagged"""
    out = {k: v for k, v in ba.items() if k not in ("n_cams", "cam_is_fixed", "robust")}
    out.update(n_free=ba["n_cams"], n_fixed=0, free_is_fixed=ba["cam_is_fixed"], user_lambda_init=0.0)
    return out


def _quat_of(R):
    """x, y, z, w of a rotation matrix (w >= 0)"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-6:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0
    return np.array([x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x), 0.0])


def drop_edges(case, keep):
    """the case with only the edges where keep is true (order kept)"""
    keep = np.asarray(keep, bool)
    out = dict(case)
    for k in ("edge_point", "edge_cam", "edge_obs", "edge_inv_sigma2", "planted_outlier"):
        out[k] = case[k][keep]
    return out


def local_mapping_case(seed=5):
    """the shape tools/lba_bench.py measures: 30 free and 30 fixed key frames, 3 000 points, about 5 observations per point"""
    return make_lba_case(n_free=30, n_fixed=30, n_points=3000, obs_per_point=(3, 7), seed=seed, outlier_share=0.02, step=0.4)
