"""Synthetic inputs for the matcher entry points: key-frame pairs with FeatureVectors (SearchForTriangulation, SearchByBoW),
a LastFrame / CurrentFrame pair with map points (SearchByProjection), local map points against a frame
(Tracking::SearchLocalPoints).  Shared by the parity tests (tests/parity_checks.py) and bench.py's per-call latency legs,
so that what is timed is what is checked.  numpy only."""
import numpy as np

from . import frontend as F
from . import synth


def make_triangulation_case(n=1500, seed=11, n_nodes=100):
    rng = np.random.default_rng(seed)
    a = synth.descriptors(n, seed)
    b, perm = synth.perturbed_descriptors(a, flip_p=0.04, seed=seed + 1)
    # a few exact duplicates in image 2 to exercise "ties -> later candidate wins"
    dup = rng.integers(0, n, 40)
    b[dup] = b[(dup + 1) % n]
    key1 = (a[:, 0].astype(np.int64) * 131 + a[:, 1] * 31 + a[:, 2]) % n_nodes
    key2 = key1[perm]  # a feature of image 2 falls into the node of the feature it was derived from
    key2[dup] = key2[(dup + 1) % n]

    def csr(key):
        order = np.argsort(key, kind="stable").astype(np.int32)
        ids, cnt = np.unique(key, return_counts=True)
        off = np.zeros(len(ids) + 1, np.int32)
        off[1:] = np.cumsum(cnt)
        return ids.astype(np.int32), off, order

    xy1 = np.stack([rng.uniform(20, 1200, n), rng.uniform(20, 350, n)], 1).astype(np.float32)
    disp = rng.uniform(2, 60, n).astype(np.float32)
    xy2 = xy1[perm].copy()
    xy2[:, 0] -= disp[perm]
    xy2[:, 1] += rng.normal(0, 1.2, n).astype(np.float32)  # some pairs violate the epipolar bound
    oct1 = rng.integers(0, 8, n).astype(np.int32)
    oct2 = rng.integers(0, 8, n).astype(np.int32)
    ang1 = rng.uniform(0, 360, n).astype(np.float32)
    ang2 = (ang1[perm] + rng.normal(0, 25, n)).astype(np.float32) % 360
    ur1 = np.where(rng.random(n) < 0.5, xy1[:, 0] - 5, -1).astype(np.float32)
    ur2 = np.where(rng.random(n) < 0.5, xy2[:, 0] - 5, -1).astype(np.float32)
    mp1 = (rng.random(n) < 0.3).astype(np.uint8)
    mp2 = (rng.random(n) < 0.3).astype(np.uint8)
    id1, off1, f1 = csr(key1)
    id2, off2, f2 = csr(key2)
    # drop a few nodes from each side so the merge walk has to skip
    keep1 = rng.random(len(id1)) < 0.9
    keep2 = rng.random(len(id2)) < 0.9

    def drop(ids, off, feat, keep):
        nid, noff, nfeat = [], [0], []
        for i, k in enumerate(keep):
            if k:
                nid.append(ids[i])
                nfeat.extend(feat[off[i]:off[i + 1]])
                noff.append(len(nfeat))
        return np.array(nid, np.int32), np.array(noff, np.int32), np.array(nfeat, np.int32)

    id1, off1, f1 = drop(id1, off1, f1, keep1)
    id2, off2, f2 = drop(id2, off2, f2, keep2)
    kf1 = dict(desc=a, xy=xy1, octave=oct1, angle=ang1, uright=ur1, has_mp=mp1, node_id=id1, node_off=off1, node_feat=f1)
    kf2 = dict(desc=b, xy=xy2, octave=oct2, angle=ang2, uright=ur2, has_mp=mp2, node_id=id2, node_off=off2, node_feat=f2)
    K = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
    R = np.eye(3, dtype=np.float32).reshape(9)
    t = np.array([-0.54, 0.002, 0.001], np.float32)
    ep = np.array([900.0, 185.0], np.float32)  # inside the image so the epipole guard rejects some pairs
    sf = (1.2 ** np.arange(8)).astype(np.float32)
    return kf1, kf2, K, R, t, ep, sf, (sf * sf).astype(np.float32)


def make_bow_rig_case(n=1500, seed=11, n_nodes=100):
    """A key frame and a TWO-CAMERA frame (F.Nleft != -1) for SearchByBoW: the frame of make_triangulation_case as the left
    camera's features and a second, more strongly perturbed and shuffled copy of them as the right camera's; a right feature sits
    in the vocabulary node of the left feature it was derived from.  Returns (kf, frame, Nleft)."""
    kf, left, *_ = make_triangulation_case(n, seed, n_nodes)
    rng = np.random.default_rng(seed + 1000)
    n2 = len(left["desc"])
    right_desc, perm = synth.perturbed_descriptors(left["desc"], flip_p=0.05, seed=seed + 3)
    node_of = np.full(n2, -1, np.int64)   # position of the left feature's node in the frame's FeatureVector, -1: in none
    for k in range(len(left["node_id"])):
        node_of[left["node_feat"][left["node_off"][k]:left["node_off"][k + 1]]] = k
    node_r = node_of[perm]
    feat, off = [], [0]
    for k in range(len(left["node_id"])):
        feat.extend(left["node_feat"][left["node_off"][k]:left["node_off"][k + 1]])
        feat.extend((np.nonzero(node_r == k)[0] + n2).tolist())   # ascending inside a node, as DBoW2 fills it
        off.append(len(feat))
    ang_r = (left["angle"][perm] + rng.normal(0, 10, n2)).astype(np.float32) % 360
    frame = dict(desc=np.concatenate([left["desc"], right_desc]), xy=np.concatenate([left["xy"], left["xy"][perm]]),
                 octave=np.concatenate([left["octave"], left["octave"][perm]]), angle=np.concatenate([left["angle"], ang_r]),
                 uright=np.full(2 * n2, -1, np.float32), has_mp=np.zeros(2 * n2, np.uint8), node_id=left["node_id"],
                 node_off=np.array(off, np.int32), node_feat=np.array(feat, np.int32))
    return kf, frame, n2


def _quat(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]]).astype(np.float32)


def _rot(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class Camera:
    """What a projection search needs of a camera: the image size, K = (fx, fy, cx, cy), the bounds of the undistorted image
    (Frame::mnMinX / mnMinY / mnMaxX / mnMaxY - the frame grid spans them) and mbf."""

    def __init__(self, w, h, K, min_x, min_y, max_x, max_y, mbf):
        self.w, self.h, self.K, self.mbf = w, h, np.array(K, np.float32), mbf
        self.min_x, self.min_y, self.max_x, self.max_y = min_x, min_y, max_x, max_y

    def grid(self):
        """mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv as Frame.cc computes them (float)."""
        f = np.float32
        x0, y0, x1, y1 = f(self.min_x), f(self.min_y), f(self.max_x), f(self.max_y)
        return np.array([x0, y0, x1, y1, f(64) / (x1 - x0), f(48) / (y1 - y0)], np.float32)


def _kitti_camera(w=synth.KITTI_W, h=synth.KITTI_H):
    return Camera(w, h, [718.856, 718.856, 607.1928, 185.2157], 0, 0, w, h, 386.1448)


EUROC_K = (458.654, 457.296, 367.215, 248.375)                      # cam0 of the EuRoC settings files
EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
CAMERA_NAMES = ("kitti", "euroc_undistorted", "resized", "small_offset")
PYRAMIDS = ((8, 1.2), (1, 1.2), (12, 1.2), (16, 1.1))                # (levels, scale factor); 16 levels is the library's limit


def named_camera(name, undistort=None):
    """kitti: what every generator uses by default.  euroc_undistorted: 752 x 480, the bounds Frame::ComputeImageBounds makes of
    the four undistorted image corners (off the origin, fractional, not symmetric); undistort(xy, K, dist) is the
    cv::undistortPoints to use (the tests pass their checker's; this package holds none that runs on the host).  resized: a KITTI frame after
    Camera.newWidth / newHeight = 600 x 350, bounds at the origin.  small_offset: 320 x 240 with bounds a few fractional pixels
    off the origin on every side and grid cells of 5 x 5 px (search windows wider than the grid clamp on both sides at once)."""
    if name == "kitti":
        return _kitti_camera()
    if name == "euroc_undistorted":
        w, h = 752, 480
        c = undistort(np.array([[0, 0], [w, 0], [0, h], [w, h]], np.float32), EUROC_K, EUROC_DIST)
        # Frame::ComputeImageBounds: min of the left / top corners, max of the right / bottom ones
        return Camera(w, h, EUROC_K, min(c[0, 0], c[2, 0]), min(c[0, 1], c[1, 1]), max(c[1, 0], c[3, 0]), max(c[2, 1], c[3, 1]),
                      47.90639384423901)
    if name == "resized":
        sx, sy = 600 / synth.KITTI_W, 350 / synth.KITTI_H
        return Camera(600, 350, [718.856 * sx, 718.856 * sy, 607.1928 * sx, 185.2157 * sy], 0, 0, 600, 350, 386.1448 * sx)
    if name == "small_offset":
        return Camera(320, 240, [260.0, 260.0, 159.5, 119.5], -3.25, -2.625, 316.75, 237.375, 26.0)
    raise KeyError(name)


def _camera(camera, w=synth.KITTI_W, h=synth.KITTI_H):
    if camera is None:
        return _kitti_camera(w, h)
    if camera == "euroc_undistorted":
        raise ValueError("euroc_undistorted needs an undistortion: pass named_camera('euroc_undistorted', undistort=...) instead of the name")
    return named_camera(camera) if isinstance(camera, str) else camera


def _aim_spread(octave, scale_factors):
    """Factor on the noise with which a point is aimed at a feature of `octave`: 1 on the levels the default pyramid has, the
    level's scale factor above them - there the feature lies where only a window of radius th * scale[level] finds it, not one of
    radius th * scale[level - 8] or th."""
    octave = np.asarray(octave)
    return np.where(octave >= 8, scale_factors[octave].astype(np.float64), 1.0)


def _pyramid(pyramid):
    """(levels, factor, mvScaleFactors as the generators have always built them)"""
    n_levels, factor = (8, 1.2) if pyramid is None else pyramid
    return int(n_levels), factor, (factor ** np.arange(int(n_levels))).astype(np.float32)


def make_projection_case(n1=1800, n2=2000, seed=21, motion="forward", w=synth.KITTI_W, h=synth.KITTI_H, frame2=None, camera=None,
                         pyramid=None):
    """A LastFrame with map points and a CurrentFrame whose features they should re-find.  Clusters of near-identical
    current features and several map points aiming at the same feature exercise the 'feature already holds an observed
    map point' rule (later points fall back to their second choice); unobserved (temporal) points get overwritten.
    frame2 (optional): dict(xy, desc, octave, angle[, uright]) of a real extraction to use as the CurrentFrame instead of
    the synthetic features (n2 = its size; no clusters are added).
    camera (a Camera, or the name of one that named_camera builds without an undistortion; None: KITTI intrinsics on a w x h image) and pyramid ((levels, factor); None:
    (8, 1.2)): the features lie inside the camera's bounds, the octaves in the pyramid."""
    rng = np.random.default_rng(seed)
    cam = _camera(camera, w, h)
    n_levels, _, scale_factors = _pyramid(pyramid)
    K, mbf = cam.K, cam.mbf
    x0, y0, x1, y1 = cam.min_x, cam.min_y, cam.max_x, cam.max_y
    if frame2 is not None:
        xy2 = np.ascontiguousarray(frame2["xy"], np.float32)
        n2 = len(xy2)
        desc2 = np.ascontiguousarray(frame2["desc"], np.uint8)
        oct2 = np.ascontiguousarray(frame2["octave"], np.int32)
        ang2 = np.ascontiguousarray(frame2["angle"], np.float32)
        depth2 = rng.uniform(4, 70, n2)
        if frame2.get("uright") is not None:
            uright2 = np.ascontiguousarray(frame2["uright"], np.float32)
            depth2 = np.where(uright2 > 0, mbf / np.maximum(xy2[:, 0] - uright2, 1e-3), depth2)
        else:
            uright2 = np.where(rng.random(n2) < 0.6, xy2[:, 0] - mbf / depth2 + rng.normal(0, 1.0, n2), -1).astype(np.float32)
    else:
        xy2 = np.stack([rng.uniform(x0 + 5, x1 - 5, n2), rng.uniform(y0 + 5, y1 - 5, n2)], 1).astype(np.float32)
        desc2 = synth.descriptors(n2, seed)
        # clusters: copies of a feature a few pixels away with almost the same descriptor
        ncl = n2 // 10
        src = rng.integers(0, n2, ncl)
        dst = rng.permutation(n2)[:ncl]
        xy2[dst] = xy2[src] + rng.uniform(-4, 4, (ncl, 2)).astype(np.float32)
        flips = rng.random((ncl, 256)) < 0.02
        desc2[dst] = desc2[src] ^ np.packbits(flips, axis=1, bitorder="little")
        xy2[:, 0] = np.clip(xy2[:, 0], x0 + 1, x1 - 2)
        xy2[:, 1] = np.clip(xy2[:, 1], y0 + 1, y1 - 2)
        oct2 = rng.integers(0, n_levels, n2).astype(np.int32)
        oct2[dst] = oct2[src]
        ang2 = rng.uniform(0, 360, n2).astype(np.float32)
        depth2 = rng.uniform(4, 70, n2)
        uright2 = np.where(rng.random(n2) < 0.6, xy2[:, 0] - mbf / depth2 + rng.normal(0, 1.0, n2), -1).astype(np.float32)
    # poses
    qc = _quat([0.1, 1.0, 0.05], 0.02)
    tc = np.array([0.05, -0.02, 0.3], np.float32)
    dz = {"forward": 0.9, "backward": -0.9, "none": 0.05}[motion]
    ql = _quat([0.0, 1.0, 0.0], 0.01)
    Rc, Rl = _rot(qc), _rot(ql)
    Cc = -Rc.T @ tc.astype(np.float64)                       # current camera centre in the world
    # last camera: dz metres behind (forward motion) along its own optical axis
    tl = (-Rl @ Cc + np.array([0.02, 0.0, dz])).astype(np.float32)
    # map points: most aim at a current feature (several at the same one), the rest are elsewhere
    target = rng.integers(0, n2, n1)
    target[: n1 // 6] = target[n1 // 6: 2 * (n1 // 6)]        # duplicates
    aimed = rng.random(n1) < 0.8
    z = depth2[target] * rng.uniform(0.97, 1.03, n1)
    uv = xy2[target] + rng.normal(0, 1.5, (n1, 2)) * _aim_spread(oct2[target], scale_factors)[:, None]
    uv[~aimed] = np.stack([rng.uniform(x0 - 50, x1 + 50, (~aimed).sum()), rng.uniform(y0 - 50, y1 + 50, (~aimed).sum())], 1)
    z[rng.random(n1) < 0.03] *= -1                            # behind the camera
    xc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], 1)
    world = ((xc - tc.astype(np.float64)) @ Rc).astype(np.float32)   # Rc^T (xc - tc)
    flips = rng.random((n1, 256)) < 0.03
    mp_desc = desc2[target] ^ np.packbits(flips, axis=1, bitorder="little")
    mp_desc[~aimed] = synth.descriptors(int((~aimed).sum()), seed + 1)
    oct1 = np.clip(oct2[target] + rng.integers(-1, 2, n1), 0, n_levels - 1).astype(np.int32)
    ang1 = ((ang2[target] + rng.normal(0, 20, n1)) % 360).astype(np.float32)
    ang1[rng.random(n1) < 0.1] = rng.uniform(0, 360, 1).astype(np.float32)[0]
    grid = cam.grid()
    return dict(valid1=(rng.random(n1) < 0.9).astype(np.uint8), world_pos1=world, mp_desc1=mp_desc,
                mp_observed1=(rng.random(n1) < 0.75).astype(np.uint8), octave1=oct1, angle1=ang1,
                kp2_xy=xy2, kp2_octave=oct2, kp2_angle=ang2, uright2=uright2, desc2=desc2, grid=grid,
                Tcw_q=qc, Tcw_t=tc, Tlw_q=ql, Tlw_t=tl, K=K, mb=0.54, mbf=mbf,
                scale_factors=scale_factors)


def make_local_points_case(n1=3000, n2=2000, seed=41, w=synth.KITTI_W, h=synth.KITTI_H, frame2=None, camera=None, pyramid=None):
    """Local map points with predicted projections (what Frame::isInFrustum leaves in the MapPoint) against a frame in which
    a part of the features already holds tracked points.  Clusters of look-alike features make the ratio test bite,
    several map points aim at the same feature (the later one is blocked and falls back or fails its ratio test).
    frame2 (optional): dict(xy, desc, octave[, uright]) of a real extraction to use as the frame (no clusters added).
    camera, pyramid: as for make_projection_case."""
    rng = np.random.default_rng(seed)
    cam = _camera(camera, w, h)
    n_levels, _, scale_factors = _pyramid(pyramid)
    mbf = cam.mbf
    x0, y0, x1, y1 = cam.min_x, cam.min_y, cam.max_x, cam.max_y
    if frame2 is not None:
        xy2 = np.ascontiguousarray(frame2["xy"], np.float32)
        n2 = len(xy2)
        desc2 = np.ascontiguousarray(frame2["desc"], np.uint8)
        oct2 = np.ascontiguousarray(frame2["octave"], np.int32)
        depth2 = rng.uniform(4, 70, n2)
        if frame2.get("uright") is not None:
            uright2 = np.ascontiguousarray(frame2["uright"], np.float32)
            depth2 = np.where(uright2 > 0, mbf / np.maximum(xy2[:, 0] - uright2, 1e-3), depth2)
        else:
            uright2 = np.where(rng.random(n2) < 0.6, xy2[:, 0] - mbf / depth2, -1).astype(np.float32)
    else:
        xy2 = np.stack([rng.uniform(x0 + 5, x1 - 5, n2), rng.uniform(y0 + 5, y1 - 5, n2)], 1).astype(np.float32)
        desc2 = synth.descriptors(n2, seed)
        ncl = n2 // 6
        src = rng.integers(0, n2, ncl)
        dst = rng.permutation(n2)[:ncl]
        xy2[dst] = xy2[src] + rng.uniform(-3, 3, (ncl, 2)).astype(np.float32)
        flips = rng.random((ncl, 256)) < rng.choice([0.01, 0.05, 0.15], ncl)[:, None]
        desc2[dst] = desc2[src] ^ np.packbits(flips, axis=1, bitorder="little")
        xy2[:, 0] = np.clip(xy2[:, 0], x0 + 1, x1 - 2)
        xy2[:, 1] = np.clip(xy2[:, 1], y0 + 1, y1 - 2)
        oct2 = rng.integers(0, n_levels, n2).astype(np.int32)
        oct2[dst] = np.where(rng.random(ncl) < 0.7, oct2[src], np.clip(oct2[src] - 1, 0, n_levels - 1))
        depth2 = rng.uniform(4, 70, n2)
        uright2 = np.where(rng.random(n2) < 0.6, xy2[:, 0] - mbf / depth2, -1).astype(np.float32)
    blocked2 = (rng.random(n2) < 0.3).astype(np.uint8)          # already tracked by the motion model
    target = rng.integers(0, n2, n1)
    target[: n1 // 5] = target[n1 // 5: 2 * (n1 // 5)]
    aimed = rng.random(n1) < 0.8
    uv = xy2[target] + rng.normal(0, 1.0, (n1, 2)).astype(np.float32) * _aim_spread(oct2[target], scale_factors)[:, None].astype(np.float32)
    uv[~aimed] = np.stack([rng.uniform(x0, x1, (~aimed).sum()), rng.uniform(y0, y1, (~aimed).sum())], 1)
    xr = (uv[:, 0] - mbf / depth2[target] + rng.normal(0, 1.5, n1)).astype(np.float32)
    proj = np.concatenate([uv, xr[:, None]], 1).astype(np.float32)
    level = np.clip(oct2[target] + rng.integers(0, 2, n1), 0, n_levels - 1).astype(np.int32)   # window accepts level-1 .. level
    flips = rng.random((n1, 256)) < 0.04
    mp_desc = desc2[target] ^ np.packbits(flips, axis=1, bitorder="little")
    mp_desc[~aimed] = synth.descriptors(int((~aimed).sum()), seed + 1)
    grid = cam.grid()
    return dict(valid1=(rng.random(n1) < 0.85).astype(np.uint8), proj1=proj, level1=level,
                view_cos1=np.where(rng.random(n1) < 0.5, 0.9995, 0.9).astype(np.float32), mp_desc1=mp_desc,
                mp_observed1=(rng.random(n1) < 0.9).astype(np.uint8), kp2_xy=xy2, kp2_octave=oct2, uright2=uright2, desc2=desc2,
                blocked2=blocked2, grid=grid, scale_factors=scale_factors)


def make_relocalization_case(n1=1500, n2=2000, seed=61, camera=None, pyramid=None):
    """A key frame whose map points are searched in a frame with a (PnP-refined) pose: SearchByProjection(CurrentFrame, pKF,
    sAlreadyFound, th, ORBdist).  Built on the Frame-to-Frame case: same clusters / duplicate targets; on top of it points
    without a map point, bad and already-found ones, scale-invariance ranges that exclude some points, features of the
    frame that hold a map point on entry, and points behind the camera (the overload does not test the sign of the depth)."""
    c = make_projection_case(n1, n2, seed, "none", camera=camera, pyramid=pyramid)
    n_levels, factor, _ = _pyramid(pyramid)
    rng = np.random.default_rng(seed + 1000)
    qc, tc = c["Tcw_q"], c["Tcw_t"]
    Rc = _rot(qc)
    Ow = (-Rc.T @ tc.astype(np.float64))
    dist = np.linalg.norm(c["world_pos1"].astype(np.float64) - Ow, axis=1)
    # mfMaxDistance = dist * scale^level of the observation that made the point: predicted levels spread over the pyramid
    lvl = c["octave1"].astype(np.int64)                          # near the octave of the feature the point aims at
    max_d = (dist * factor ** lvl * rng.uniform(0.85, 1.0, n1)).astype(np.float32)
    min_d = (max_d / np.float32(factor ** (n_levels - 1))).astype(np.float32)
    far = rng.random(n1) < 0.05
    max_d[far] = (dist[far] * 0.5).astype(np.float32)          # outside the invariance range (too far)
    near = rng.random(n1) < 0.03
    min_d[near] = (dist[near] * 2.0).astype(np.float32)        # too close
    return dict(has_mp1=(rng.random(n1) < 0.85).astype(np.uint8), bad1=(rng.random(n1) < 0.05).astype(np.uint8),
                found1=(rng.random(n1) < 0.15).astype(np.uint8), world_pos1=c["world_pos1"], mp_desc1=c["mp_desc1"],
                min_dist1=min_d, max_dist1=max_d, angle1=c["angle1"], kp2_xy=c["kp2_xy"], kp2_octave=c["kp2_octave"],
                kp2_angle=c["kp2_angle"], desc2=c["desc2"], occupied2=(rng.random(n2) < 0.1).astype(np.uint8),
                grid=c["grid"], Tcw_q=qc, Tcw_t=tc, K=c["K"], scale_factors=c["scale_factors"],
                log_scale_factor=np.float32(np.log(np.float32(factor))))


def relocalization_prepass(case):
    """What the shim evaluates with the MapPoint objects, written with numpy float32 + the C library's logf
    (F.ORBmatcher.PredictScale): must equal the oracle's prepass bit for bit."""
    q, t = np.asarray(case["Tcw_q"], np.float32), np.asarray(case["Tcw_t"], np.float32)

    def rotate(qv, p):  # Eigen QuaternionBase::_transformVector in float32
        u = np.float32(2) * np.cross(qv[:3], p).astype(np.float32)
        return (p + qv[3] * u + np.cross(qv[:3], u).astype(np.float32)).astype(np.float32)
    qinv = np.array([-q[0], -q[1], -q[2], q[3]], np.float32)
    Ow = rotate(qinv, (-t).astype(np.float32))
    PO = (np.asarray(case["world_pos1"], np.float32) - Ow).astype(np.float32)
    sq = (PO * PO).astype(np.float32)
    dist = np.sqrt((sq[:, 0] + (sq[:, 1] + sq[:, 2]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    max_inv = (np.float32(1.2) * case["max_dist1"]).astype(np.float32)
    min_inv = (np.float32(0.8) * case["min_dist1"]).astype(np.float32)
    valid = (case["has_mp1"] != 0) & (case["bad1"] == 0) & (case["found1"] == 0) & ~(dist < min_inv) & ~(dist > max_inv)
    level = F.ORBmatcher.PredictScale(dist, case["max_dist1"], case["log_scale_factor"], len(case["scale_factors"]))
    return valid.astype(np.uint8), np.where(valid, level, 0).astype(np.int32)


def make_fuse_case(n1=2500, n2=2000, seed=91, camera=None, pyramid=None):
    """Map points of neighbouring key frames projected into a key frame (LocalMapping::SearchInNeighbors -> ORBmatcher::Fuse):
    built on the relocalisation case (same clusters, points behind the camera, invariance ranges) plus normals (some seen
    under more than 60 degrees), points already in the key frame, stereo / mono key-frame features (both chi-square gates)."""
    c = make_relocalization_case(n1, n2, seed, camera=camera, pyramid=pyramid)
    base = make_projection_case(n1, n2, seed, "none", camera=camera, pyramid=pyramid)
    rng = np.random.default_rng(seed + 2000)
    q, t = c["Tcw_q"], c["Tcw_t"]
    Rc = _rot(q)
    Ow = (-Rc.T @ t.astype(np.float64)).astype(np.float32)
    PO = c["world_pos1"].astype(np.float64) - Ow
    dist = np.linalg.norm(PO, axis=1, keepdims=True)
    normal = PO / np.maximum(dist, 1e-6) + rng.normal(0, 0.35, PO.shape)       # roughly towards the camera ...
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    flip = rng.random(n1) < 0.08
    normal[flip] *= -1                                                           # ... some from behind
    sf = c["scale_factors"]
    return dict(has_mp1=c["has_mp1"], bad1=c["bad1"], in_kf1=(rng.random(n1) < 0.1).astype(np.uint8),
                world_pos1=c["world_pos1"], normal1=normal.astype(np.float32), mp_desc1=c["mp_desc1"],
                min_dist1=c["min_dist1"], max_dist1=c["max_dist1"], kp2_xy=c["kp2_xy"], kp2_octave=c["kp2_octave"],
                uright2=base["uright2"], desc2=c["desc2"], grid=c["grid"], Tcw_q=q, Tcw_t=t, Ow=Ow, K=c["K"],
                bf=np.float32(base["mbf"]), scale_factors=sf,
                inv_level_sigma2=(np.float32(1.0) / (sf * sf).astype(np.float32)).astype(np.float32),
                log_scale_factor=c["log_scale_factor"])


def fuse_prepass(case):
    """The tests of the Fuse loop that need the MapPoint object, numpy float32 + the C library's logf."""
    Ow = np.asarray(case["Ow"], np.float32)
    PO = (np.asarray(case["world_pos1"], np.float32) - Ow).astype(np.float32)
    sq = (PO * PO).astype(np.float32)
    dist = np.sqrt((sq[:, 0] + (sq[:, 1] + sq[:, 2]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    Pn = np.asarray(case["normal1"], np.float32)
    pr = (PO * Pn).astype(np.float32)
    dot = (pr[:, 0] + (pr[:, 1] + pr[:, 2]).astype(np.float32)).astype(np.float32)
    max_inv = (np.float32(1.2) * case["max_dist1"]).astype(np.float32)
    min_inv = (np.float32(0.8) * case["min_dist1"]).astype(np.float32)
    valid = ((case["has_mp1"] != 0) & (case["bad1"] == 0) & (case["in_kf1"] == 0) & ~(dist < min_inv) & ~(dist > max_inv) &
             ~(dot.astype(np.float64) < 0.5 * dist.astype(np.float64)))
    level = F.ORBmatcher.PredictScale(dist, case["max_dist1"], case["log_scale_factor"], len(case["scale_factors"]))
    return valid.astype(np.uint8), np.where(valid, level, 0).astype(np.int32)


def make_project_search_case(n1=2500, n2=2000, seed=111, camera=None, pyramid=None):
    """Camera-frame map points over a key frame (what Fuse(pKF, Scw, ...) and SearchBySim3 hand to the search): the fuse case with
    the points moved into the camera frame in float64 and rounded once (the product and the oracle both start from these)."""
    c = make_fuse_case(n1, n2, seed, camera=camera, pyramid=pyramid)
    valid, level = fuse_prepass(c)
    R = _rot(c["Tcw_q"]).astype(np.float64)
    cam = (c["world_pos1"].astype(np.float64) @ R.T + c["Tcw_t"].astype(np.float64)).astype(np.float32)
    return dict(valid1=valid, cam_pos1=cam, mp_desc1=c["mp_desc1"], level1=level, kp2_xy=c["kp2_xy"], kp2_octave=c["kp2_octave"],
                desc2=c["desc2"], grid=c["grid"], K=c["K"], scale_factors=c["scale_factors"])


def make_sim3_case(n=1500, seed=121, w=synth.KITTI_W, h=synth.KITTI_H, camera=None, pyramid=None):
    """Two key frames that see the same place (all poses identities, so one common camera frame): KF2's features are KF1's,
    permuted, moved by a pixel or two and with a few descriptor bits flipped; every feature's map point sits on the ray of its
    counterpart in the OTHER key frame, so that the two directed searches of SearchBySim3 mostly agree.  Some features have no
    or a bad map point, some points fall outside their invariance range, some lie behind the camera.
    camera, pyramid: as for make_projection_case."""
    rng = np.random.default_rng(seed)
    cm = _camera(camera, w, h)
    n_levels, factor, sf = _pyramid(pyramid)
    K = cm.K
    x0, y0, x1, y1 = cm.min_x, cm.min_y, cm.max_x, cm.max_y
    xy1 = np.stack([rng.uniform(x0 + 20, x1 - 20, n), rng.uniform(y0 + 20, y1 - 20, n)], 1).astype(np.float32)
    oct1 = rng.integers(0, n_levels, n).astype(np.int32)
    desc1 = synth.descriptors(n, seed)
    perm = rng.permutation(n)
    inv = np.argsort(perm)                                   # feature i1 of KF1 <-> feature inv[i1] of KF2
    xy2 = (xy1[perm] + rng.normal(0, 1.0, (n, 2))).astype(np.float32)
    oct2 = oct1[perm].copy()
    desc2 = desc1[perm] ^ np.packbits(rng.random((n, 256)) < 0.03, axis=1, bitorder="little")

    def side(xy_self, octave, desc, xy_other, partner):
        z = rng.uniform(4, 60, n)
        z[rng.random(n) < 0.03] *= -1
        tgt = xy_other[partner] + rng.normal(0, 1.0, (n, 2)) * _aim_spread(octave, sf)[:, None]
        pos = np.stack([(tgt[:, 0] - K[2]) / K[0] * z, (tgt[:, 1] - K[3]) / K[1] * z, z], 1).astype(np.float32)
        dist = np.linalg.norm(pos.astype(np.float64), axis=1)
        lvl = np.clip(octave + rng.integers(0, 2, n), 0, n_levels - 1)   # predicted level = octave or octave + 1: band [l - 1, l] holds the octave
        max_d = (dist * factor ** lvl * rng.uniform(0.86, 0.99, n)).astype(np.float32)
        min_d = (max_d / np.float32(factor ** (n_levels - 1))).astype(np.float32)
        far = rng.random(n) < 0.04
        max_d[far] = (dist[far] * 0.5).astype(np.float32)
        normal = -pos / np.maximum(np.linalg.norm(pos, axis=1, keepdims=True), 1e-6) + rng.normal(0, 0.3, pos.shape)
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        state = rng.choice([0, 1, 2], n, p=[0.12, 0.8, 0.08]).astype(np.uint8)
        mp_desc = desc ^ np.packbits(rng.random((n, 256)) < 0.02, axis=1, bitorder="little")
        return dict(kp_xy=xy_self, kp_octave=octave, desc=desc, mp_state=state, mp_pos=pos, mp_normal=(-normal).astype(np.float32),
                    mp_desc=mp_desc, mp_min_dist=min_d, mp_max_dist=max_d)
    a1 = side(xy1, oct1, desc1, xy2, inv)
    a2 = side(xy2, oct2, desc2, xy1, perm)
    prior = np.where(rng.random(n) < 0.1, inv, -1).astype(np.int32)      # matches found earlier (by SearchByBoW)
    return dict(a1=a1, a2=a2, K=K, grid=cm.grid(), scale_factors=sf, log_scale_factor=np.float32(np.log(np.float32(factor))),
                prior12=prior, inv=inv)


def make_initialization_case(n1=5000, seed=61, w=synth.KITTI_W, h=synth.KITTI_H, motion=(14.0, -6.0), camera=None, pyramid=None):
    """Two monocular frames: F2's features are F1's moved by `motion` plus noise, descriptors with a few flipped bits;
    vbPrevMatched = F1's positions (Tracking.cc:2493-2495).  Look-alike neighbours make the ratio test bite, and pairs of F1
    features aim at one F2 feature with the later one closer, so that matches are taken over (vMatchedDistance)."""
    rng = np.random.default_rng(seed)
    cam = _camera(camera, w, h)
    n_levels = _pyramid(pyramid)[0]
    x0, y0, x1, y1 = cam.min_x, cam.min_y, cam.max_x, cam.max_y
    xy1 = np.stack([rng.uniform(x0 + 5, x1 - 5, n1), rng.uniform(y0 + 5, y1 - 5, n1)], 1).astype(np.float32)
    level_p = [0.45, 0.2, 0.1, 0.08, 0.06, 0.05, 0.03, 0.03]      # level 0 is what the search matches
    if n_levels != 8:
        rest = 0.8 ** np.arange(n_levels - 1)
        level_p = [1.0] if n_levels == 1 else [0.45] + list(0.55 * rest / rest.sum())
    oct1 = rng.choice(n_levels, n1, p=level_p).astype(np.int32)
    desc1 = synth.descriptors(n1, seed)
    ang1 = rng.uniform(0, 360, n1).astype(np.float32)
    n2 = n1
    perm = rng.permutation(n1)                      # F2 feature j comes from F1 feature perm[j]
    xy2 = (xy1[perm] + np.array(motion, np.float32) + rng.normal(0, 1.5, (n2, 2))).astype(np.float32)
    oct2 = oct1[perm].copy()
    oct2[rng.random(n2) < 0.1] = min(1, n_levels - 1)
    rate = rng.choice([0.01, 0.04, 0.1, 0.3], n2, p=[0.3, 0.4, 0.2, 0.1])
    desc2 = desc1[perm] ^ np.packbits(rng.random((n2, 256)) < rate[:, None], axis=1, bitorder="little")
    dang = np.where(rng.random(n2) < 0.8, rng.normal(5, 3, n2), rng.uniform(0, 360, n2))
    ang2 = np.mod(ang1[perm] - dang, 360).astype(np.float32)
    # look-alike neighbours in F2 (second-best close to best)
    ncl = n2 // 8
    src = rng.integers(0, n2, ncl)
    dst = rng.permutation(n2)[:ncl]
    xy2[dst] = xy2[src] + rng.uniform(-20, 20, (ncl, 2)).astype(np.float32)
    oct2[dst] = oct2[src]
    desc2[dst] = desc2[src] ^ np.packbits(rng.random((ncl, 256)) < rng.choice([0.01, 0.06], ncl)[:, None], axis=1, bitorder="little")
    # take-overs: F1 feature a (lower index) resembles what F1 feature b (higher index) matches even better
    inv = np.empty(n1, np.int64)
    inv[perm] = np.arange(n1)
    pairs = rng.permutation(n1)[: 2 * (n1 // 10)].reshape(-1, 2)
    a, b = pairs.min(1), pairs.max(1)
    oct1[a] = 0; oct1[b] = 0
    c = inv[b]
    oct2[c] = 0
    xy1[a] = xy1[b] + rng.uniform(-30, 30, (len(a), 2)).astype(np.float32)
    desc2[c] = desc1[b] ^ np.packbits(rng.random((len(a), 256)) < 0.02, axis=1, bitorder="little")
    desc1[a] = desc2[c] ^ np.packbits(rng.random((len(a), 256)) < rng.choice([0.03, 0.08], len(a))[:, None], axis=1, bitorder="little")
    xy2[:, 0] = np.clip(xy2[:, 0], x0 + 1, x1 - 2)
    xy2[:, 1] = np.clip(xy2[:, 1], y0 + 1, y1 - 2)
    prev = xy1.copy()
    prev[rng.random(n1) < 0.01] = np.float32(-500)   # window outside of the grid
    grid = cam.grid()
    return dict(kp1_octave=oct1, kp1_angle=ang1, desc1=desc1, prev_matched=prev, kp2_xy=xy2, kp2_octave=oct2, kp2_angle=ang2,
                desc2=desc2, grid=grid)


def _rotation_matrix_f32(q):
    """Eigen QuaternionBase::toRotationMatrix in float32 (what SE3f::rotationMatrix() returns), row-major, 9 floats."""
    f = np.float32
    x, y, z, w = [f(v) for v in q]
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([f(1) - (tyy + tzz), txy - twz, txz + twy, txy + twz, f(1) - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, f(1) - (txx + tyy)], np.float32)


def make_local_map_case(n1=3000, n2=2000, seed=71, w=synth.KITTI_W, h=synth.KITTI_H):
    """The local map of Tracking::SearchLocalPoints BEFORE Frame::isInFrustum has run: world points (most aimed at features of
    the frame, as in make_relocalization_case), normals, scale-invariance ranges, descriptors - and the frame with its pose as
    Frame::UpdatePoseMatrices leaves it.  Every exit of isInFrustum gets its share of the points: behind the camera, outside
    the image, outside the invariance range (too far, too close), seen from the side or from behind, and in view with
    predicted levels over the whole pyramid, including ratios beyond its top (upper clamp).  n1, n2 >= 1."""
    c = make_projection_case(n1, n2, seed, "none", w, h)
    rng = np.random.default_rng(seed + 3000)
    K, q, t = c["K"], c["Tcw_q"], c["Tcw_t"]
    Rc = _rot(q)
    Cw = -Rc.T @ t.astype(np.float64)                          # camera centre
    world = c["world_pos1"].astype(np.float64)
    cat = rng.random(n1)
    behind = cat < 0.07
    world[behind] = 2 * Cw - world[behind]                     # mirrored through the camera centre: Pc -> -Pc
    outside = (cat >= 0.07) & (cat < 0.16)
    no = int(outside.sum())
    side = rng.integers(0, 4, no)
    off = rng.uniform(0.5, 80, no)
    u = np.where(side == 0, -off, np.where(side == 1, w + off, rng.uniform(0, w, no)))
    v = np.where(side == 2, -off, np.where(side == 3, h + off, rng.uniform(0, h, no)))
    z = rng.uniform(4, 70, no)
    xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
    world[outside] = (xc - t.astype(np.float64)) @ Rc
    world = world.astype(np.float32)
    PO = world.astype(np.float64) - Cw
    dist = np.linalg.norm(PO, axis=1)
    # mfMaxDistance = dist * scale^level of the observation that made the point: near the octave of the feature it aims at
    lvl = c["octave1"].astype(np.int64)
    max_d = dist * 1.2 ** lvl * rng.uniform(0.85, 1.0, n1)
    rcat = rng.random(n1)
    top = rcat < 0.06
    max_d[top] = dist[top] * 1.2 ** 7 * rng.uniform(1.02, 1.2, int(top.sum()))    # ratio beyond the top level, still in range
    far = (rcat >= 0.06) & (rcat < 0.14)
    max_d[far] = dist[far] * rng.uniform(0.4, 0.8, int(far.sum()))               # dist > 1.2 max
    min_d = max_d / 1.2 ** 7
    near = (rcat >= 0.14) & (rcat < 0.21)
    min_d[near] = dist[near] * rng.uniform(1.3, 2.0, int(near.sum()))            # dist < 0.8 min
    normal = PO / np.maximum(dist, 1e-6)[:, None] + rng.normal(0, 0.3, PO.shape)  # roughly towards the camera ...
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    ncat = rng.random(n1)
    normal[ncat < 0.08] *= -1                                                    # ... some from behind
    sideways = (ncat >= 0.08) & (ncat < 0.16)
    tang = np.cross(PO, rng.normal(0, 1, PO.shape))
    tang /= np.maximum(np.linalg.norm(tang, axis=1, keepdims=True), 1e-9)
    mix = rng.uniform(0.0, 0.45, (n1, 1))                                        # viewCos below the limit of 0.5
    side_n = mix * PO / np.maximum(dist, 1e-6)[:, None] + np.sqrt(1 - mix * mix) * tang
    normal[sideways] = side_n[sideways]
    qf = np.asarray(q, np.float32)

    def rotate(qv, p):  # Eigen QuaternionBase::_transformVector in float32
        uu = np.float32(2) * np.cross(qv[:3], p).astype(np.float32)
        return (p + qv[3] * uu + np.cross(qv[:3], uu).astype(np.float32)).astype(np.float32)
    Ow = rotate(np.array([-qf[0], -qf[1], -qf[2], qf[3]], np.float32), (-np.asarray(t, np.float32)).astype(np.float32))
    return dict(world_pos1=world, normal1=normal.astype(np.float32), min_dist1=min_d.astype(np.float32),
                max_dist1=max_d.astype(np.float32), mp_desc1=c["mp_desc1"], mp_observed1=c["mp_observed1"],
                consider1=(rng.random(n1) < 0.92).astype(np.uint8),
                kp2_xy=c["kp2_xy"], kp2_octave=c["kp2_octave"], uright2=c["uright2"], desc2=c["desc2"],
                blocked2=(rng.random(len(c["kp2_xy"])) < 0.3).astype(np.uint8), grid=c["grid"], scale_factors=c["scale_factors"],
                Rcw=_rotation_matrix_f32(qf), tcw=np.asarray(t, np.float32), Ow=Ow, K=K, mbf=np.float32(c["mbf"]),
                log_scale_factor=np.float32(np.log(np.float32(1.2))), viewing_cos_limit=np.float32(0.5), far_points=0,
                th_far_points=np.float32(40.0))


def local_points_from_cull(case, in_view, rec):
    """(in_view, rec: what frontend.frustum_restatement or ORBmatcher.FrustumCull returned.)  The make_local_points_case-style dict that ORBmatcher::SearchByProjection(F, vpMapPoints, ...) sees after the loop:
    valid1 = mbTrackInView && !(bFarPoints && mTrackDepth > thFarPoints) (ORBmatcher.cc:52-59; isBad is part of consider1)."""
    valid = (np.asarray(in_view) != 0)
    if int(case["far_points"]):
        valid = valid & ~(rec["depth"] > np.float32(case["th_far_points"]))
    return dict(valid1=valid.astype(np.uint8), proj1=np.stack([rec["proj_x"], rec["proj_y"], rec["proj_xr"]], 1).astype(np.float32),
                level1=rec["level"].astype(np.int32), view_cos1=rec["view_cos"].astype(np.float32), mp_desc1=case["mp_desc1"],
                mp_observed1=case["mp_observed1"], kp2_xy=case["kp2_xy"], kp2_octave=case["kp2_octave"], uright2=case["uright2"],
                desc2=case["desc2"], blocked2=case["blocked2"], grid=case["grid"], scale_factors=case["scale_factors"])


def make_map_refresh_case(n_points=1500, n_kfs=40, seed=5, obs_counts=None, features=None, base_desc=None):
    """Map points and the key frames that observe them, as rgbl_map_points_refresh reads them (MapPoint::UpdateNormalAndDepth,
    ComputeDistinctiveDescriptors): key frames on a trajectory, each with its own feature count (`features`: one count for all,
    or (low, high)), about 5 % of them bad; per point a base descriptor, every observation that base with each bit flipped
    with probability 0.08 (`base_desc`: the bases instead of random ones), some observations exact copies of an earlier one
    (ties); observation counts mostly 2 .. 30, with 0
    and 1 present and a few up to 200 (`obs_counts`: the count of every point instead); a key frame is listed once per point
    while the count allows it, in ascending order; some points have a reference key frame that does not observe them (its
    level is then the octave of that frame's feature 0, the reference's quirk).  The first observation of the case is on
    feature 0 of its key frame, the last one on the last feature of its.  Slots 0 .. n_points - 1; normal0, min_dist0,
    max_dist0, desc0 are what the pool holds before the refresh."""
    rng = np.random.default_rng(seed)
    n_levels = 8
    scale = np.ones(n_levels, np.float32)
    for l in range(1, n_levels):
        scale[l] = scale[l - 1] * np.float32(1.2)
    if features is None:
        features = (300, 2000)
    if np.isscalar(features):
        kf_n = np.full(n_kfs, features, np.int64)
    else:   # all different where the range allows it
        span = np.arange(features[0], features[1] + 1)
        kf_n = rng.choice(span, n_kfs, replace=len(span) < n_kfs).astype(np.int64)
    k = np.arange(n_kfs, dtype=np.float64)
    kf_center = np.stack([0.9 * k, 0.1 * np.sin(0.7 * k), 4.0 * np.sin(0.11 * k)], 1).astype(np.float32)
    kf_bad = (rng.random(n_kfs) < 0.05).astype(np.uint8)
    if n_kfs >= 20 and not kf_bad.any():
        kf_bad[int(rng.integers(0, n_kfs))] = 1
    kf_desc = [rng.integers(0, 256, (int(n), 32), dtype=np.uint8) for n in kf_n]
    kf_octave = [rng.integers(0, n_levels, int(n)).astype(np.int32) for n in kf_n]
    kf_xy = [rng.uniform(0, 1200, (int(n), 2)).astype(np.float32) for n in kf_n]
    next_feat = [rng.permutation(int(n)) for n in kf_n]
    used = np.zeros(n_kfs, np.int64)
    if obs_counts is None:
        cat = rng.random(n_points)
        counts = rng.integers(2, 31, n_points)
        counts[cat < 0.03] = 0
        counts[(cat >= 0.03) & (cat < 0.07)] = 1
        few = cat > 0.985
        counts[few] = rng.integers(100, 201, int(few.sum()))
    else:
        counts = np.broadcast_to(np.asarray(obs_counts, np.int64), (n_points,)).copy()
    if n_kfs == 0:
        counts[:] = 0
    anchor = rng.integers(0, max(n_kfs, 1), n_points)
    world = (kf_center[anchor].astype(np.float64) if n_kfs else np.zeros((n_points, 3))) + \
        rng.normal(0, 1, (n_points, 3)) * rng.uniform(2, 40, (n_points, 1))
    obs_off = np.zeros(n_points + 1, np.int32)
    obs_off[1:] = np.cumsum(counts)
    obs_kf = np.zeros(int(obs_off[-1]), np.int32)
    obs_feat = np.zeros(int(obs_off[-1]), np.int32)
    ref_kf = np.zeros(n_points, np.int32)
    ref_level = np.zeros(n_points, np.int32)
    base = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    if base_desc is not None:
        base = np.ascontiguousarray(base_desc, np.uint8).reshape(n_points, 32)
    for p in range(n_points):
        c, b = int(counts[p]), int(obs_off[p])
        kfs = np.sort(rng.choice(n_kfs, c, replace=c > n_kfs)) if c else np.zeros(0, np.int64)
        flips = np.packbits(rng.random((c, 256)) < 0.08, axis=1)
        rows = base[p][None, :] ^ flips
        for i in range(1, c):
            if rng.random() < 0.15:
                rows[i] = rows[int(rng.integers(0, i))]
        for i in range(c):
            kf = int(kfs[i])
            f = int(next_feat[kf][used[kf] % kf_n[kf]])
            if b + i == 0:
                f = 0
            if b + i == len(obs_kf) - 1:
                f = int(kf_n[kf]) - 1
            used[kf] += 1
            obs_kf[b + i], obs_feat[b + i] = kf, f
            kf_desc[kf][f] = rows[i]
        outsider = n_kfs > 0 and (c == 0 or (rng.random() < 0.1 and c < n_kfs))
        if outsider:
            rest = np.setdiff1d(np.arange(n_kfs), kfs)
            ref_kf[p] = int(rest[rng.integers(0, len(rest))])
            ref_level[p] = kf_octave[ref_kf[p]][0]          # observations[pRefKF] default-inserts (0, 0)
        elif n_kfs > 0:
            i = int(rng.integers(0, c))
            ref_kf[p] = obs_kf[b + i]
            ref_level[p] = kf_octave[obs_kf[b + i]][obs_feat[b + i]]
    normal0 = rng.normal(0, 1, (n_points, 3)).astype(np.float32)
    return dict(slot=np.arange(n_points, dtype=np.int32), world_pos=world.astype(np.float32), normal0=normal0,
                min_dist0=rng.uniform(1, 5, n_points).astype(np.float32), max_dist0=rng.uniform(20, 90, n_points).astype(np.float32),
                desc0=rng.integers(0, 256, (n_points, 32), dtype=np.uint8), obs_off=obs_off, obs_kf=obs_kf, obs_feat=obs_feat,
                ref_kf=ref_kf, ref_level=ref_level, kf_n=kf_n.astype(np.int32), kf_desc=kf_desc, kf_octave=kf_octave, kf_xy=kf_xy,
                kf_center=kf_center, kf_bad=kf_bad, scale_factors=scale, n_levels=n_levels)


def make_new_points_case(n=600, n_neigh=10, seed=7, n_nodes=None, th_far_points=None, report_rejected=1, monocular=0, inertial=0):
    """A key frame and its covisible neighbours for LocalMapping::CreateNewMapPoints: a world of n 3-D points, 4 - 90 m in front
    of the key frame, seen by every neighbour (about three quarters of them each, shuffled, the rest clutter).  KITTI K and bf;
    neighbour baselines 0.6 - 1.1 m in ascending order, so that a far point is of low parallax at an early neighbour and
    triangulates at a later one; pixel noise of 0.5 px times the level's scale factor; about 20 % of a neighbour's pixels are
    outliers ALONG the epipolar line (a wrong depth on the key frame's ray, a quarter of them beyond infinity, and for the
    neighbours 4 and 9, which moved ahead, some between the two image planes: the search accepts them, the triangulation lands
    behind one camera or both, or fails a reprojection test); LiDAR depth (mvDepth, mvuRight = u - bf / depth)
    on about half the features, a few with depth == 0 and uright >= 0; about 6 % of the octaves break the scale consistency;
    2 % of the key frame's features are doubles of another one (two idx1 for one idx2).  Descriptors: a world point's own with
    3 % of the bits flipped per view; the FeatureVector node is a hash of the world point, so the search finds the geometric
    matches.  With n_neigh >= 4, neighbour 1 is closer than mb (left out by the baseline test), neighbour 2 shares no
    vocabulary node with the key frame and neighbour 3 is left out by skip[].
    Returns dict(kf1, neighbours = [dict(kf, F12, ep, coarse, only_stereo)], skip, prm)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    w, h = synth.KITTI_W, synth.KITTI_H
    K = np.array([718.856, 718.856, 607.1928, 185.2157], f32)
    mbf = f32(386.1448)
    mb = f32(mbf / K[0])
    n_levels = 8
    sf = (1.2 ** np.arange(n_levels)).astype(f32)
    s2 = (sf * sf).astype(f32)
    n_nodes = n_nodes or max(2, n // 15)
    fx, fy, cx, cy = [float(v) for v in K]

    def pose(center, axis, angle):
        q = _quat(axis, angle)                     # of Rcw, (x, y, z, w): what the reference tier builds its Sophus pose from
        R = _rot(q)
        t = -R @ np.asarray(center, np.float64)
        Tcw = np.concatenate([R, t[:, None]], 1).astype(f32)
        R32 = Tcw[:, :3].astype(np.float64)
        Ow = (-R32.T @ Tcw[:, 3].astype(np.float64)).astype(f32)
        quats[id(Tcw)] = q
        return Tcw, Ow
    quats = {}

    def project(Tcw, X):
        Xc = X @ Tcw[:, :3].astype(np.float64).T + Tcw[:, 3].astype(np.float64)
        z = Xc[:, 2]
        with np.errstate(all="ignore"):
            return np.stack([fx * Xc[:, 0] / z + cx, fy * Xc[:, 1] / z + cy], 1), z

    def flip(desc):
        bits = np.unpackbits(desc, axis=1)
        return np.packbits(bits ^ (rng.random(bits.shape) < 0.03).astype(np.uint8), axis=1)

    def csr(key):
        order = np.argsort(key, kind="stable").astype(np.int32)
        ids, cnt = np.unique(key, return_counts=True)
        off = np.zeros(len(ids) + 1, np.int32)
        off[1:] = np.cumsum(cnt)
        return ids.astype(np.int32), off, order

    def lidar(xy, z, level):
        """mvDepth / mvuRight for about half the features; a few stereo features carry depth 0"""
        m = len(xy)
        has = rng.random(m) < 0.5
        depth = np.where(has, z, -1.0).astype(f32)
        with np.errstate(all="ignore"):
            ur = np.where(has, xy[:, 0] - float(mbf) / np.where(has, depth, 1.0), -1.0).astype(f32)
        zero = has & (rng.random(m) < 0.04)
        depth[zero] = 0.0
        return depth, ur

    # the key frame: world points from its own pixels and depths
    Tcw1, Ow1 = pose([3.0, -0.5, 12.0], [0.1, 1.0, 0.05], 0.08)
    n_dbl = n // 50
    n_pts = n - n_dbl
    pix = np.stack([rng.uniform(30, w - 30, n_pts), rng.uniform(30, h - 30, n_pts)], 1)
    depth_true = np.exp(rng.uniform(np.log(4.0), np.log(90.0), n_pts))
    Xc = np.stack([(pix[:, 0] - cx) / fx * depth_true, (pix[:, 1] - cy) / fy * depth_true, depth_true], 1)
    R1 = Tcw1[:, :3].astype(np.float64)
    X = (Xc - Tcw1[:, 3].astype(np.float64)) @ R1                      # world
    wid1 = np.concatenate([np.arange(n_pts), rng.integers(0, max(n_pts, 1), n_dbl)]).astype(np.int64) if n_pts else np.zeros(0, np.int64)
    wid1 = wid1[:n]
    lvl1 = rng.integers(0, n_levels, len(wid1))
    base_desc = synth.descriptors(max(n_pts, 1), seed + 1)
    desc1 = flip(base_desc[wid1[:n_pts]]) if n_pts else np.zeros((0, 32), np.uint8)
    desc1 = np.concatenate([desc1, desc1[wid1[n_pts:]]]) if n_dbl else desc1     # a double carries the very same descriptor
    p1, z1 = project(Tcw1, X[wid1]) if len(wid1) else (np.zeros((0, 2)), np.zeros(0))
    xy1 = (p1 + rng.normal(0, 0.5, p1.shape) * sf[lvl1][:, None]).astype(f32)
    d1, ur1 = lidar(xy1, z1, lvl1)
    node_of = (wid1 * 2654435761 % 1000003) % n_nodes
    id1, off1, f1 = csr(node_of)
    kf1 = dict(desc=desc1, xy=xy1, octave=lvl1.astype(np.int32), angle=rng.uniform(0, 360, len(wid1)).astype(f32), uright=ur1,
               has_mp=(rng.random(len(wid1)) < 0.25).astype(np.uint8), node_id=id1, node_off=off1, node_feat=f1, depth=d1,
               xy_raw=(xy1 + f32(0.25)).astype(f32), Tcw=Tcw1.reshape(-1), Ow=Ow1, q=quats[id(Tcw1)], K=K, mb=mb, mbf=mbf, scale_factors=sf, level_sigma2=s2)

    baselines = np.sort(rng.uniform(0.6, 1.1, n_neigh))
    neighbours, skip = [], np.zeros(n_neigh, np.uint8)
    for k in range(n_neigh):
        special = k if n_neigh >= 4 else -1
        b = float(rng.uniform(0.3, 0.5)) if special == 1 else float(baselines[k])
        forward = k % 5 == 4   # the camera moved ahead: the epipole lies in the image
        direction = np.array([0.1, 0.02, 1.0]) if forward else np.array([np.cos(0.5 * k), 0.15 * np.sin(1.3 * k), 0.6 * np.sin(0.5 * k)])
        direction /= np.linalg.norm(direction)
        center = Ow1.astype(np.float64) + b * (R1.T @ direction)
        Tcw2, Ow2 = pose(center, [0.1, 1.0, 0.05], 0.08 + 0.01 * np.sin(2.0 * k))
        seen = np.nonzero(rng.random(n_pts) < 0.75)[0]
        Xs = X[seen].copy()
        outl = rng.random(len(seen)) < 0.2
        factor = np.where(rng.random(len(seen)) < 0.25, -rng.uniform(0.5, 4.0, len(seen)), np.exp(rng.uniform(np.log(0.3), np.log(3.0), len(seen))))
        # a wrong depth on the key frame's ray; a negative one is a pixel beyond the ray's point at infinity
        if forward:   # and a point between the two centres' planes is in front of the key frame and behind this neighbour
            near = rng.random(len(seen)) < 0.3
            factor = np.where(near, rng.uniform(0.1, 0.8, len(seen)) * b / depth_true[seen], factor)
            outl = outl | near
        Xs[outl] = Ow1.astype(np.float64) + (X[seen][outl] - Ow1.astype(np.float64)) * factor[outl][:, None]
        p2, z2 = project(Tcw2, Xs)
        behind = z2 <= 0
        if behind.any():   # the mirror image of a point behind the camera: still on the epipolar line, beyond infinity
            z2 = np.abs(z2)
        ok = np.isfinite(p2).all(1) & (p2[:, 0] > 5) & (p2[:, 0] < w - 5) & (p2[:, 1] > 5) & (p2[:, 1] < h - 5) & (z2 > 0.05)
        seen, p2, z2 = seen[ok], p2[ok], z2[ok]
        n_true = min(len(seen), n)
        seen, p2, z2 = seen[:n_true], p2[:n_true], z2[:n_true]
        n_junk = n - n_true
        wid2 = np.concatenate([seen, np.full(n_junk, -1)]).astype(np.int64)
        with np.errstate(all="ignore"):
            shift = np.rint(np.log(np.maximum(z2, 0.1) / depth_true[seen]) / np.log(1.2)).astype(np.int64) if n_true else np.zeros(0, np.int64)
        lvl_true = np.clip(lvl1[seen] - shift + rng.integers(-1, 2, n_true), 0, n_levels - 1) if n_true else np.zeros(0, np.int64)
        off_scale = rng.random(n_true) < 0.06
        lvl_true = np.where(off_scale, (lvl_true + 4) % n_levels, lvl_true)
        lvl2 = np.concatenate([lvl_true, rng.integers(0, n_levels, n_junk)]).astype(np.int64)
        xy2 = np.concatenate([p2, np.stack([rng.uniform(5, w - 5, n_junk), rng.uniform(5, h - 5, n_junk)], 1)])
        xy2 = (xy2 + rng.normal(0, 0.5, xy2.shape) * sf[lvl2][:, None]).astype(f32)
        zz = np.concatenate([z2, rng.uniform(4, 90, n_junk)])
        desc2 = np.concatenate([flip(base_desc[seen]) if n_true else np.zeros((0, 32), np.uint8), synth.descriptors(n_junk, seed + 100 + k)])
        node2 = np.where(wid2 >= 0, (wid2 * 2654435761 % 1000003) % n_nodes, rng.integers(0, n_nodes, n)) + (100000 if special == 2 else 0)
        perm = rng.permutation(n)
        xy2, zz, lvl2, desc2, node2 = xy2[perm], zz[perm], lvl2[perm], desc2[perm], node2[perm]
        d2, ur2 = lidar(xy2, zz, lvl2)
        id2, off2, f2 = csr(node2)
        kf2 = dict(desc=desc2, xy=xy2, octave=lvl2.astype(np.int32), angle=rng.uniform(0, 360, n).astype(f32), uright=ur2,
                   has_mp=(rng.random(n) < 0.25).astype(np.uint8), node_id=id2, node_off=off2, node_feat=f2, depth=d2,
                   xy_raw=(xy2 - f32(0.125)).astype(f32), Tcw=Tcw2.reshape(-1), Ow=Ow2, q=quats[id(Tcw2)], K=K, mb=mb, mbf=mbf, scale_factors=sf,
                   level_sigma2=s2)
        # F12 = K1^-T [t12]x R12 K2^-1 and the epipole project(T2w * Ow1) (ORBmatcher.cc:913-931, Pinhole.cpp:109-112)
        Ra, ta = Tcw1[:, :3].astype(np.float64), Tcw1[:, 3].astype(np.float64)
        Rb, tb = Tcw2[:, :3].astype(np.float64), Tcw2[:, 3].astype(np.float64)
        R12 = Ra @ Rb.T
        t12 = ta - R12 @ tb
        Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        F12 = (np.linalg.inv(Km).T @ tx @ R12 @ np.linalg.inv(Km)).astype(f32).reshape(-1)
        C2 = Rb @ Ow1.astype(np.float64) + tb
        ep = np.array([fx * C2[0] / C2[2] + cx, fy * C2[1] / C2[2] + cy], f32)
        neighbours.append(dict(kf=kf2, F12=F12, ep=ep, coarse=0, only_stereo=0))
        skip[k] = 1 if special == 3 else 0
    prm = dict(n_levels=n_levels, ratio_factor=float(f32(1.5) * f32(1.2)), far_points=int(th_far_points is not None),
               th_far_points=float(th_far_points or 0.0), inertial=int(inertial), monocular=int(monocular), report_rejected=int(report_rejected))
    return dict(kf1=kf1, neighbours=neighbours, skip=skip, prm=prm)


def make_pose_opt_case(n=2000, matched=300, seed=3, mono_share=0.2, outlier_share=0.1, n_levels=8, scale_factor=1.2,
                       rot_noise=0.01, trans_noise=0.15, pixel_noise=1.0):
    """A frame as Optimizer::PoseOptimization reads it (Optimizer.cc:814-1114), deterministic by seed: `matched` of the n features
    have a map point 4 - 60 m in front of a KITTI camera (stored as float), octaves 0 .. n_levels - 1, pixel noise proportional to
    the level's sigma, a planted share of gross outliers (+-40 px), a share of monocular features (uright = -1), and an entry
    pose that is the planted one perturbed by about rot_noise rad and trans_noise m.
    Keys: the frame dict of frontend.ORBmatcher.PoseOptimization (mp_index, world_pos, xy, octave, uright, q, t, K, bf,
    inv_level_sigma2) plus the plant: q_true, t_true, planted_outlier (per feature)."""
    rng = np.random.default_rng(seed)
    cam = _kitti_camera()
    fx, fy, cx, cy = [float(v) for v in cam.K]
    bf = float(np.float32(cam.mbf))
    sf = np.array([scale_factor ** i for i in range(n_levels)], np.float32)
    inv_sigma2 = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    axis = rng.normal(size=3)
    q_true = _quat(axis, rng.uniform(0.0, 0.3))
    t_true = rng.uniform(-2.0, 2.0, 3).astype(np.float32)
    R = _rot(q_true)
    matched = min(matched, n)
    feat = np.sort(rng.choice(n, matched, replace=False)) if matched else np.zeros(0, np.int64)
    # points in the camera frame, then to the world: Xw = R^T (Xc - t)
    z = rng.uniform(4.0, 60.0, matched)
    u = rng.uniform(20.0, cam.w - 20.0, matched)
    v = rng.uniform(20.0, cam.h - 20.0, matched)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = ((Xc - t_true.astype(np.float64)) @ R).astype(np.float32)
    order = rng.permutation(matched)               # the map side is not in feature order
    world_pos = np.zeros((matched, 3), np.float32)
    world_pos[order] = Xw
    mp_index = np.full(n, -1, np.int32)
    mp_index[feat] = order
    octave = rng.integers(0, n_levels, n).astype(np.int32)
    xy = np.stack([rng.uniform(0, cam.w, n), rng.uniform(0, cam.h, n)], 1).astype(np.float32)
    uright = np.full(n, -1.0, np.float32)
    # observations of the float points under the planted pose
    Pc = Xw.astype(np.float64) @ R.T + t_true.astype(np.float64)
    pu, pv = fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy
    pr = pu - bf / Pc[:, 2]
    sig = sf[octave[feat]].astype(np.float64) * pixel_noise
    noise = rng.normal(size=(matched, 3)) * sig[:, None]
    gross = rng.random(matched) < outlier_share
    noise[gross, :2] += rng.choice([-40.0, 40.0], (int(gross.sum()), 2))
    mono = rng.random(matched) < mono_share
    xy[feat] = np.stack([pu + noise[:, 0], pv + noise[:, 1]], 1).astype(np.float32)
    ur = (pr + noise[:, 0] + 0.5 * noise[:, 2]).astype(np.float32)
    uright[feat] = np.where(mono | (ur < 0), np.float32(-1.0), ur)
    planted = np.zeros(n, np.uint8)
    planted[feat] = gross
    # the entry pose
    dq = _quat(rng.normal(size=3), rot_noise)
    a, b = dq.astype(np.float64), q_true.astype(np.float64)
    q = np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                  a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])
    q = (q / np.linalg.norm(q)).astype(np.float32)
    d = rng.normal(size=3)
    t = (t_true + trans_noise * d / np.linalg.norm(d)).astype(np.float32)
    return dict(mp_index=mp_index, world_pos=world_pos, xy=xy, octave=octave, uright=uright, q=q, t=t,
                K=np.array([fx, fy, cx, cy], np.float32), bf=np.float32(bf), inv_level_sigma2=inv_sigma2, n_levels=n_levels,
                q_true=q_true, t_true=t_true, planted_outlier=planted)
