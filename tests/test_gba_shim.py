"""The C++ drop-ins rgbl_shim::BundleAdjustment / GlobalBundleAdjustemnt (orb_slam3_rgbl_amd/shim/GlobalBundleAdjuster.h),
compiled with stand-in KeyFrame / MapPoint / Map types (tests/gba_shim_test.cpp).  This side walks the same scene as
Optimizer.cc:116-275 does - written here a second time, from the reference's lines -, hands the lists to the C ABI's host build
and holds what the program left to it bit for bit: every pose and position, and WHICH members were written - SetPose /
SetWorldPos / UpdateNormalAndDepth with nLoopKF == the origin key frame's id (:293, :379), mTcwGBA / mPosGBA / mnBAGlobalForKF
otherwise.  The scenes hold vpKFs and vpMP in an order that is not the pointer order, a bad key frame inside vpKFs, a key frame
outside vpKFs whose id is beyond maxKFid (:154) and one whose id is not (:156: no vertex), a bad point, a point that only those
two see (removed, :266-270: nothing written), a point seen only through left index -1 (included without an edge), a NaN
mvuRight, and the stop flag set.  A key frame with a second camera makes the drop-in return false with nothing written."""
import fcntl
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import lba_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim")
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "gba_shim_test.cpp")
SIGMA = np.array([1.0 / 1.2 ** (2 * i) for i in range(8)], np.float32)


def build(libdir, libname, exe):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "rgbl_frontend.h"), os.path.join(libdir, "lib%s.so" % libname)] + glob.glob(os.path.join(SHIM, "*.h"))
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            return
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + SHIM, SRC, "-o", tmp, "-L" + libdir,
                               "-l" + libname, "-Wl,-rpath," + libdir, "-pthread"])
        os.replace(tmp, exe)


def make_scene(seed, initialisation, robust, iterations, stop=0, second_camera=False, through_map=0):
    c = lc.make_ba_case(n_cams=7, n_fixed=1, n_points=60, obs_per_point=(2, 5), seed=seed, outlier_share=0.1)
    nC = 7
    ids = [40 + 3 * ((5 * k) % nC) for k in range(nC)]   # ids are not in index order
    kfs = [dict(id=ids[k], bad=0, cam2=0, q=c["cam_q"][k], t=c["cam_t"][k], K=c["cam_K"][k], bf=c["cam_bf"][k], feats=[]) for k in range(nC)]
    octave = np.abs(c["edge_inv_sigma2"][:, None] - SIGMA[None, :]).argmin(1)
    for e in range(len(c["edge_point"])):
        o = c["edge_obs"][e]
        kfs[c["edge_cam"][e]]["feats"].append((o[0], o[1], int(octave[e]), o[2], int(c["edge_point"][e])))
    for k in kfs:   # features without a map point in between
        k["feats"].insert(min(2, len(k["feats"])), (5.0, 5.0, 0, -1.0, -1))
    mps = [dict(id=7 * p, bad=0, pos=c["world_pos"][p]) for p in range(60)]
    kfs[3]["bad"] = 1                              # inside vpKFs, bad: no vertex, its observations skipped, nothing written
    mps[4]["bad"] = 1
    # two key frames outside vpKFs: one beyond maxKFid, one not
    for new_id, src in ((900, 5), (41, 6)):
        kfs.append(dict(id=new_id, bad=0, cam2=0, q=kfs[src]["q"], t=kfs[src]["t"], K=kfs[src]["K"], bf=kfs[src]["bf"],
                        feats=[(100.0 + i, 80.0, 1, -1.0, p) for i, p in enumerate((8, 9, 21))]))
    for k in kfs[:nC]:                             # point 21: only those two see it
        k["feats"] = [f for f in k["feats"] if f[4] != 21]
    for k in kfs:                                  # point 30: only through a left index of -1
        k["feats"] = [f for f in k["feats"] if f[4] != 30]
    extra = [(1, 30), (2, 11)]                     # ... and point 11 loses key frame 2's edge to such an observation
    x, y, o, _, p = kfs[0]["feats"][5]
    kfs[0]["feats"][5] = (x, y, o, float("nan"), p)
    if second_camera:
        kfs[2]["cam2"] = 1
    list_kf = [6, 2, 0, 3, 5, 1, 4]
    list_mp = list(np.random.default_rng(seed).permutation(60))
    origin = 2
    init_id = kfs[0]["id"]
    loop_kf = kfs[origin]["id"] if initialisation else 77
    return dict(kfs=kfs, mps=mps, extra=extra, list_kf=list_kf, list_mp=[int(p) for p in list_mp], init_id=init_id, origin=origin, stop=stop,
                loop_kf=loop_kf, robust=robust, iterations=iterations, through_map=through_map)


def write_scene(s, path):
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", len(s["kfs"]), len(s["mps"]), s["init_id"], s["origin"], s["stop"], s["loop_kf"], s["robust"], s["iterations"],
                            s["through_map"]))
        for k in s["kfs"]:
            f.write(struct.pack("<3i", k["id"], k["bad"], k["cam2"]))
            f.write(np.concatenate([k["q"], k["t"], k["K"], [k["bf"]]]).astype(np.float32).tobytes())
            f.write(struct.pack("<i", len(k["feats"])))
            for x, y, o, ur, p in k["feats"]:
                f.write(struct.pack("<2fifi", x, y, o, ur, p))
        for m in s["mps"]:
            f.write(struct.pack("<2i3f", m["id"], m["bad"], *[float(v) for v in m["pos"]]))
        f.write(struct.pack("<i", len(s["extra"])))
        for k, p in s["extra"]:
            f.write(struct.pack("<2i", k, p))
        for lst in (s["list_kf"], s["list_mp"]):
            f.write(struct.pack("<i", len(lst)))
            f.write(np.array(lst, np.int32).tobytes())
        f.write(SIGMA.tobytes())


def reference_walk(s):
    """Optimizer.cc:116-275 on the scene: (cameras, fixed flags, points, included flags, edges as (point row, camera row, key frame, feature))"""
    kfs, mps = s["kfs"], s["mps"]
    cams = [k for k in s["list_kf"] if not kfs[k]["bad"]]
    max_id = max(kfs[k]["id"] for k in cams)
    vertex = {kfs[k]["id"]: c for c, k in enumerate(cams)}
    fixed = [kfs[k]["id"] == s["init_id"] for k in cams]
    observations = {p: {} for p in range(len(mps))}   # a std::map keyed by the key frame's pointer = index: one entry per key frame
    for k in range(len(kfs)):
        for i, f in enumerate(kfs[k]["feats"]):
            if f[4] >= 0:
                observations[f[4]][k] = i
    for k, p in s["extra"]:
        observations[p][k] = -1
    pts, included, edges = [], [], []
    for p in s["list_mp"]:
        if mps[p]["bad"]:
            continue
        n_edges = 0
        for k in sorted(observations[p]):
            if kfs[k]["bad"] or kfs[k]["id"] > max_id or kfs[k]["id"] not in vertex:
                continue
            n_edges += 1
            i = observations[p][k]
            ur = kfs[k]["feats"][i][3] if i >= 0 else 0.0
            if i >= 0 and ur == ur:
                edges.append((len(pts), vertex[kfs[k]["id"]], k, i))
        pts.append(p)
        included.append(n_edges > 0)
    return cams, fixed, pts, included, edges


def expected(s, lib):
    cams, fixed, pts, included, edges = reference_walk(s)
    kfs = s["kfs"]
    case = dict(n_cams=len(cams), cam_is_fixed=np.array(fixed, np.uint8), cam_q=np.array([kfs[k]["q"] for k in cams], np.float32),
                cam_t=np.array([kfs[k]["t"] for k in cams], np.float32), cam_K=np.array([kfs[k]["K"] for k in cams], np.float32),
                cam_bf=np.array([kfs[k]["bf"] for k in cams], np.float32),
                world_pos=np.array([s["mps"][p]["pos"] for p in pts], np.float32).reshape(-1, 3), n_points=len(pts),
                edge_point=np.array([e[0] for e in edges], np.int32), edge_cam=np.array([e[1] for e in edges], np.int32),
                edge_obs=np.array([[kfs[k]["feats"][i][0], kfs[k]["feats"][i][1], kfs[k]["feats"][i][3]] for _, _, k, i in edges], np.float32).reshape(-1, 3),
                edge_inv_sigma2=np.array([SIGMA[kfs[k]["feats"][i][2]] for _, _, k, i in edges], np.float32),
                robust=s["robust"], max_iterations=s["iterations"], stop_byte=np.array([s["stop"]], np.uint8))
    return cams, pts, included, edges, case, F.bundle_adjustment_host(case, lib=lib)


def run(exe, s, tmp_path, name):
    path, out = os.path.join(str(tmp_path), name + ".bin"), os.path.join(str(tmp_path), name + ".out")
    write_scene(s, path)
    res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "GBA_SHIM_OK" in res.stdout, name + ": " + res.stdout[-3000:] + res.stderr[-3000:]
    buf = open(out, "rb").read()
    nk, nm = len(s["kfs"]), len(s["mps"])
    done = struct.unpack_from("<i", buf)[0]
    kf = np.frombuffer(buf, np.float32, 16 * nk, 4).reshape(nk, 16)
    mp = np.frombuffer(buf, np.float32, 9 * nm, 4 + 64 * nk).reshape(nm, 9)
    return done, kf, mp


def run_and_check(exe, lib, tmp_path):
    seen = {}
    scenes = (("loop_closing", make_scene(4, False, 0, 10)), ("initialisation", make_scene(6, True, 1, 20)),
              ("through_the_map", make_scene(7, False, 1, 5, through_map=1)), ("stop_set", make_scene(4, False, 0, 10, stop=1)))
    for name, s in scenes:
        done, kf, mp = run(exe, s, tmp_path, name)
        cams, pts, included, edges, case, r = expected(s, lib)
        assert done == 1, name
        nk, nm = len(s["kfs"]), len(s["mps"])
        init = s["loop_kf"] == s["kfs"][s["origin"]]["id"]
        # the walk reached what the scenes plant
        assert 3 not in cams and 7 not in cams and 8 not in cams and len(cams) == 6 and sum(case["cam_is_fixed"]) == 1, name
        assert 21 in pts and not included[pts.index(21)] and included[pts.index(30)] and 4 not in pts, name
        assert not (case["edge_point"] == pts.index(30)).any() and r["included"][pts.index(30)] == 0, name
        mono = case["edge_obs"][:, 2] < 0
        assert mono.any() and (~mono).any() and not np.isnan(case["edge_obs"]).any(), name
        assert (r["iterations"] == 0 and r["polls"] == 1) if s["stop"] else 1 < r["iterations"] <= s["iterations"], (name, r["iterations"])
        written_kf = np.zeros(nk, bool)
        written_kf[cams] = True
        written_pt = np.zeros(nm, bool)
        written_pt[[p for p, inc in zip(pts, included) if inc]] = True
        q0 = np.array([k["q"] for k in s["kfs"]], np.float32)
        t0 = np.array([k["t"] for k in s["kfs"]], np.float32)
        x0 = np.array([m["pos"] for m in s["mps"]], np.float32)
        inc = np.array(included)
        if init:   # :295, :381-382
            assert kf[cams, :4].tobytes() == r["cam_q"].tobytes() and kf[cams, 4:7].tobytes() == r["cam_t"].tobytes(), name
            assert (kf[:, 7] == written_kf).all() and (kf[:, 8:11] == 0).all() and (kf[:, 15] == 0).all(), name
            assert mp[np.array(pts)[inc], :3].tobytes() == r["point"][inc].tobytes(), name
            assert (mp[:, 3] == written_pt).all() and (mp[:, 4] == written_pt).all() and (mp[:, 5:] == 0).all(), name
        else:      # :299-300, :386-387
            assert kf[cams, 8:12].tobytes() == r["cam_q"].tobytes() and kf[cams, 12:15].tobytes() == r["cam_t"].tobytes(), name
            assert (kf[:, 15] == np.where(written_kf, s["loop_kf"], 0)).all() and (kf[:, 7] == 0).all(), name
            assert kf[:, :4].tobytes() == q0.tobytes() and kf[:, 4:7].tobytes() == t0.tobytes(), name
            assert mp[np.array(pts)[inc], 5:8].tobytes() == r["point"][inc].tobytes(), name
            assert (mp[:, 8] == np.where(written_pt, s["loop_kf"], 0)).all() and (mp[:, 3] == 0).all() and (mp[:, 4] == 0).all(), name
            assert mp[:, :3].tobytes() == x0.tobytes(), name
        for k in np.flatnonzero(~written_kf):
            assert kf[k, :4].tobytes() == q0[k].tobytes() and kf[k, 4:7].tobytes() == t0[k].tobytes(), name
        for p in np.flatnonzero(~written_pt):
            assert mp[p, :3].tobytes() == x0[p].tobytes(), name
        seen[name] = (len(cams), len(pts), int(inc.sum()), len(edges), int(r["iterations"]), int(r["trials"]))
    # robust and plain runs are told apart, and so are 5, 10 and 20 iterations, by the bits above: here only that they differ
    assert seen["loop_closing"][4] != seen["stop_set"][4]
    # a second camera: false, nothing written
    s = make_scene(4, True, 1, 10, second_camera=True)
    done, kf, mp = run(exe, s, tmp_path, "second_camera")
    assert done == 0 and (kf[:, 7] == 0).all() and (kf[:, 15] == 0).all() and (mp[:, 3] == 0).all() and (mp[:, 8] == 0).all()
    assert kf[:, :4].tobytes() == np.array([k["q"] for k in s["kfs"]], np.float32).tobytes()
    return seen


def test_cpp_bundle_adjustment_under_emulation(emu_lib, tmp_path):
    exe = os.path.join(BUILD, "gba_shim_test_emu")
    build(BUILD, "rgbl_frontend_emu", exe)
    print(run_and_check(exe, emu_lib, tmp_path))


@pytest.mark.gpu
def test_cpp_bundle_adjustment_on_mi355x(gpu_lib, tmp_path):
    exe = os.path.join(BUILD, "gba_shim_test_gpu")
    build(os.path.join(ROOT, "orb_slam3_rgbl_amd"), "rgbl_frontend", exe)
    print(run_and_check(exe, gpu_lib, tmp_path))
