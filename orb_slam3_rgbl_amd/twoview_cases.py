"""Seeded problems for rgbl_two_view_reconstruct (TwoViewReconstruction, src/TwoViewReconstruction.cc): two frames of undistorted
keys, the matches SearchForInitialization would hand over (mvIniMatches: per key of frame 1 an index into frame 2 or -1) and the
eight-point sets, drawn as Reconstruct draws them (:78-98)."""
import numpy as np

from . import cases

f32 = np.float32
SCENES = ("general", "planar", "rotation", "forward", "outliers", "mirror")


class GlibcRand:
    """glibc's rand() (random_r, TYPE_3: r[i] = r[i - 3] + r[i - 31]) with a state of its own; srand(0) seeds like srand(1).
    DUtils::Random::SeedRandOnce(0) (:81) calls srand(0) once per process, so a fresh GlibcRand(0) is the stream of a process's
    first Reconstruct and the same object, kept, the stream of its later ones."""
    RAND_MAX = 2147483647

    def __init__(self, seed=0):
        seed = int(seed) & 0xffffffff
        if seed == 0:
            seed = 1
        r = [0] * 34
        r[0] = seed
        for i in range(1, 31):
            word = r[i - 1] if r[i - 1] < 2 ** 31 else r[i - 1] - 2 ** 32      # int32
            hi, lo = int(word / 127773), word - int(word / 127773) * 127773   # C division truncates
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            r[i] = word
        for i in range(31, 34):
            r[i] = r[i - 31]
        self.r = r[3:]              # the last 31 values
        for _ in range(310):
            self._step()

    def _step(self):
        v = (self.r[0] + self.r[28]) & 0xffffffff
        self.r = self.r[1:] + [v]
        return v

    def rand(self):
        return self._step() >> 1

    def random_int(self, lo, hi):
        """DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50)"""
        d = hi - lo + 1
        return int((float(self.rand()) / (float(self.RAND_MAX) + 1.0)) * d) + lo


def draw_sets(N, n_hyp, rand=None):
    """mvSets (:79-98): per iteration eight draws from the available indices, each replaced by the last and popped"""
    rand = rand if rand is not None else GlibcRand(0)
    out = np.zeros((n_hyp, 8), np.int32)
    for it in range(n_hyp):
        avail = list(range(N))
        for j in range(8):
            r = rand.random_int(0, len(avail) - 1)
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def _points(rng, scene, N, cam, fx, fy, cx, cy):
    u = rng.uniform(40.0, cam.w - 40.0, N)
    v = rng.uniform(40.0, cam.h - 40.0, N)
    x, y = (u - cx) / fx, (v - cy) / fy
    if scene == "planar":
        # a tilted plane n . X = d seen from camera 1
        n, d = np.array([0.25, -0.1, 1.0]), 9.0
        z = d / (n[0] * x + n[1] * y + n[2])
    elif scene == "mirror":
        z = np.where(np.arange(N) % 5 == 0, rng.uniform(4.0, 12.0, N), rng.uniform(1500.0, 2500.0, N))
    else:
        z = rng.uniform(4.0, 40.0, N)
    return np.stack([x * z, y * z, z], 1)


def make_two_view_case(N=100, n_hyp=200, seed=1, scene="general", outlier_share=0.2, pixel_noise=0.3, extra1=None, extra2=None, sigma=1.0,
                       rand=None):
    """Two frames of a KITTI camera: n1 = N + extra1 keys in frame 1 of which N are matched, n2 = N + extra2 keys in frame 2
    (default extras: N // 4 + 3 and N // 3 + 5, so n1 != n2; the unmatched keys lie between the matched ones in index order).
    scene: general (3-D points 4 - 40 m, a sideways baseline), planar (a tilted plane), rotation (no translation: no
    parallax), forward (motion along the optical axis), outliers (the keys of frame 2 are unrelated), mirror (four points of
    five beyond 1.5 km, where the depth tests of CheckRT do not apply: several motion hypotheses count them - nsimilar > 1).
    The inliers carry `pixel_noise` px of noise in both frames; a share of outliers is displaced by 30 - 80 px in frame 2.
    Keys: the problem dict of frontend.ORBmatcher.TwoViewReconstruct plus the plant (R_true, t_true, planted_outlier, idx1, idx2)."""
    assert scene in SCENES, scene
    rng = np.random.default_rng(seed)
    cam = cases._kitti_camera()
    fx, fy, cx, cy = [float(v) for v in cam.K]
    K = np.array([fx, fy, cx, cy], f32)
    X = _points(rng, scene, N, cam, fx, fy, cx, cy)
    if scene == "rotation":
        R, t = cases._rot(cases._quat(np.array([0.1, 1.0, 0.05]), 0.06)), np.zeros(3)
    elif scene == "forward":
        R, t = cases._rot(cases._quat(rng.normal(size=3), 0.01)), np.array([0.02, -0.01, -1.5])
    else:
        R, t = cases._rot(cases._quat(rng.normal(size=3), rng.uniform(0.02, 0.08))), np.array([-1.2, 0.1, 0.15])
    X2 = X @ R.T + t
    p1 = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
    p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    p1 += rng.normal(size=(N, 2)) * pixel_noise
    p2 += rng.normal(size=(N, 2)) * pixel_noise
    gross = rng.random(N) < outlier_share
    if scene == "outliers":
        gross[:] = True
        p2 = np.stack([rng.uniform(0, cam.w, N), rng.uniform(0, cam.h, N)], 1)
    else:
        ng = int(gross.sum())
        ang = rng.uniform(0, 2 * np.pi, ng)
        p2[gross] += rng.uniform(30.0, 80.0, ng)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    n1 = N + (extra1 if extra1 is not None else N // 4 + 3)
    n2 = N + (extra2 if extra2 is not None else N // 3 + 5)
    idx1 = np.sort(rng.permutation(n1)[:N]).astype(np.int32)
    idx2 = rng.permutation(n2)[:N].astype(np.int32)            # frame 2 is not in the order of frame 1
    xy1 = np.stack([rng.uniform(0, cam.w, n1), rng.uniform(0, cam.h, n1)], 1)
    xy2 = np.stack([rng.uniform(0, cam.w, n2), rng.uniform(0, cam.h, n2)], 1)
    xy1[idx1] = p1
    xy2[idx2] = p2
    matches12 = np.full(n1, -1, np.int32)
    matches12[idx1] = idx2
    samples = draw_sets(N, n_hyp, rand) if N >= 8 else np.zeros((n_hyp, 8), np.int32)
    return dict(xy1=xy1.astype(f32), xy2=xy2.astype(f32), matches12=matches12, K=K, sigma=f32(sigma), samples=samples, n_hyp=n_hyp,
                R_true=R, t_true=t, planted_outlier=gross.astype(np.uint8), idx1=idx1, idx2=idx2, N=N, scene=scene)


PROBLEM_KEYS = ("xy1", "xy2", "matches12", "K", "sigma", "samples", "n_hyp")


def problem(case, **over):
    """the C ABI's part of a case (host arrays)"""
    return dict({k: case[k] for k in PROBLEM_KEYS}, **over)


def matches(pr):
    """mvMatches12 (:55-64): (index in frame 1, index in frame 2) per match, ascending in frame 1"""
    m = np.asarray(pr["matches12"], np.int32)
    first = np.nonzero(m >= 0)[0].astype(np.int32)
    return first, m[first]
