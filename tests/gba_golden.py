"""The golden BundleAdjustment runs.  tests/golden/gba/<case>.json hold what the reference's OWN lines src/Optimizer.cc:60-390
did on a generated scene (tests/test_gba_shim.py's make_scene): every key frame's pose, SetPose count, mTcwGBA and
mnBAGlobalForKF, every point's position, SetWorldPos / UpdateNormalAndDepth counts, mPosGBA and mnBAGlobalForKF afterwards, and
what the stand-in optimiser recorded - the vertices (id, kind, fixed, marginalized) and the edges (type, both vertex ids) in the
order added, the ids handed to removeVertex, the optimize() call, whether the edges had a kernel, both Huber deltas.

    python tests/gba_golden.py         # rewrites the fixtures (needs the reference sources)

The lines are copied at test time into tests/_build/gba_ref_body.inc (never committed) and compiled unmodified against
tests/gba_ref_types.h (tests/gba_ref_glue.cpp).  This pins which key frames and points get a vertex, the vertex ids, the fixed
flag, the skips at :154 / :156, the monocular / stereo split, the edge order, bRobust and the deltas of :131-132, removeVertex,
nIterations and both write-back branches.  It does NOT pin g2o's arithmetic: the stand-in SparseOptimizer::optimize runs
rgbl_bundle_adjustment_host.  A scene is regenerated from the parameters in its fixture."""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for _p_ in (ROOT, TESTS):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

import test_gba_shim as shim  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "gba")
BUILD = os.path.join(TESTS, "_build")
REF = "/root/reference"
SOURCE, FIRST, LAST = "src/Optimizer.cc", 60, 390

# every scene of make_scene holds a bad key frame and a bad point, a key frame beyond maxKFid and one without a vertex, a point
# that only those two see and one seen only through a left index of -1; the cases differ in the call
CASES = {
    "loop_closing": dict(seed=4, initialisation=False, robust=0, iterations=10),        # LoopClosing.cc:2284
    "initialisation": dict(seed=6, initialisation=True, robust=1, iterations=20),       # Tracking.cc:2614
    "bad_skipped": dict(seed=7, initialisation=False, robust=1, iterations=5),
    "beyond_max_kfid": dict(seed=8, initialisation=True, robust=0, iterations=5),
    "point_left_out": dict(seed=9, initialisation=False, robust=1, iterations=10),
    "stop_set": dict(seed=4, initialisation=False, robust=0, iterations=10, stop=1),
}


def have_reference():
    return os.path.exists(os.path.join(REF, SOURCE))


def build_reference():
    """tests/_build/gba_ref: the reference's lines behind tests/gba_ref_glue.cpp, on the emulator library's host build"""
    exe, inc = os.path.join(BUILD, "gba_ref"), os.path.join(BUILD, "gba_ref_body.inc")
    os.makedirs(BUILD, exist_ok=True)
    lines = open(os.path.join(REF, SOURCE), errors="replace").read().splitlines(True)
    body = "".join(lines[FIRST - 1:LAST])
    assert body.startswith("void Optimizer::BundleAdjustment(") and body.rstrip().endswith("}"), body[:80]
    if not os.path.exists(inc) or open(inc).read() != body:
        with open(inc, "w") as f:
            f.write(body)
    glue, lib = os.path.join(TESTS, "gba_ref_glue.cpp"), os.path.join(BUILD, "librgbl_frontend_emu.so")
    deps = [inc, glue, lib, os.path.join(TESTS, "gba_ref_types.h"), os.path.join(ROOT, "include", "rgbl_frontend.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w", "-o", tmp, "-I" + TESTS, "-I" + BUILD, glue,
                               "-L" + BUILD, "-lrgbl_frontend_emu", "-Wl,-rpath," + BUILD, "-pthread"])
        os.replace(tmp, exe)
    return exe


def hex32(a):
    u = np.ascontiguousarray(a, np.float32).reshape(-1)
    u = np.where(np.isnan(u), np.uint32(0x7fc00000), u.view(np.uint32))
    return "".join("%08x" % int(v) for v in u)


def parse(buf, scene, with_record):
    """out.bin of tests/gba_shim_test.cpp (the drop-in) or tests/gba_ref_glue.cpp (the reference's lines, with the record)"""
    nk, nm = len(scene["kfs"]), len(scene["mps"])
    done = struct.unpack_from("<i", buf)[0]
    assert done == 1, "the drop-in refused the scene"
    kf = np.frombuffer(buf, np.float32, 16 * nk, 4).reshape(nk, 16)
    mp = np.frombuffer(buf, np.float32, 9 * nm, 4 + 64 * nk).reshape(nm, 9)
    off = 4 + 64 * nk + 36 * nm
    r = dict(pose=hex32(kf[:, :7]), set_pose=[int(v) for v in kf[:, 7]], gba_pose=hex32(kf[:, 8:15]), kf_gba_for=[int(v) for v in kf[:, 15]],
             point=hex32(mp[:, :3]), set_pos=[int(v) for v in mp[:, 3]], updated=[int(v) for v in mp[:, 4]], gba_point=hex32(mp[:, 5:8]),
             mp_gba_for=[int(v) for v in mp[:, 8]])
    if with_record:
        tail = struct.unpack_from("<9i", buf, off)
        off += 36
        lists = []
        for n in tail[:3]:
            lists.append([int(v) for v in np.frombuffer(buf, np.int32, n, off)])
            off += 4 * n
        dbl = struct.unpack_from("<2d", buf, off)
        off += 16
        r.update(vertex=lists[0], edge=lists[1], removed=lists[2], optimize=list(tail[3:7]), robust=tail[7], polls=tail[8],
                 delta=[np.float64(dbl[0]).tobytes().hex(), np.float64(dbl[1]).tobytes().hex()])
    assert off == len(buf)
    return r


def run(exe, params, with_record):
    scene = shim.make_scene(**params)
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
        shim.write_scene(scene, path)
        res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and ("GBA_REF_OK" in res.stdout or "GBA_SHIM_OK" in res.stdout), res.stdout[-3000:] + res.stderr[-3000:]
        return parse(open(out, "rb").read(), scene, with_record)


def reference_run(exe, params):
    return dict(params=params, **run(exe, params, True))


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def host_build_from_record(fx, lib):
    """rgbl_bundle_adjustment_host on the vertices and edges the fixture RECORDED (no walk of this project's is involved), with
    the recorded kernel flag and iteration count.  Returns the estimates per key frame and point index of the scene (float, as
    either write-back casts them), and which key frames and points had a vertex when optimize() ran."""
    from orb_slam3_rgbl_amd import frontend as F
    s = shim.make_scene(**fx["params"])
    kfs, mps = s["kfs"], s["mps"]
    kf_of = {k["id"]: i for i, k in enumerate(kfs)}
    V = np.array(fx["vertex"], np.int64).reshape(-1, 4)
    E = np.array(fx["edge"], np.int64).reshape(-1, 3)
    cams = [kf_of[int(v[0])] for v in V if v[1] == 0]
    max_kf_id = max(int(v[0]) for v in V if v[1] == 0)
    mp_of = {m["id"] + max_kf_id + 1: i for i, m in enumerate(mps)}
    assert all(v[3] == 1 and v[2] == 0 for v in V if v[1] == 1) and all(v[3] == 0 for v in V if v[1] == 0)
    pts = [mp_of[int(v[0])] for v in V if v[1] == 1 and int(v[0]) not in fx["removed"]]
    cam_col = {kfs[k]["id"]: c for c, k in enumerate(cams)}
    pt_col = {mps[p]["id"] + max_kf_id + 1: j for j, p in enumerate(pts)}
    obs, info = [], []
    for typ, pid, cid in E:
        k, p = kf_of[int(cid)], pts[pt_col[int(pid)]]
        feat = [f for f in kfs[k]["feats"] if f[4] == p]
        assert len(feat) == 1 and (feat[0][3] >= 0) == (typ == 1) and (feat[0][3] < 0) == (typ == 0)
        obs.append([feat[0][0], feat[0][1], feat[0][3] if typ == 1 else -1.0])
        info.append(shim.SIGMA[feat[0][2]])
    case = dict(n_cams=len(cams), cam_is_fixed=np.array([v[2] for v in V if v[1] == 0], np.uint8),
                cam_q=np.array([kfs[k]["q"] for k in cams], np.float32), cam_t=np.array([kfs[k]["t"] for k in cams], np.float32),
                cam_K=np.array([kfs[k]["K"] for k in cams], np.float32), cam_bf=np.array([kfs[k]["bf"] for k in cams], np.float32),
                world_pos=np.array([mps[p]["pos"] for p in pts], np.float32).reshape(-1, 3), n_points=len(pts),
                edge_point=np.array([pt_col[int(e[1])] for e in E], np.int32), edge_cam=np.array([cam_col[int(e[2])] for e in E], np.int32),
                edge_obs=np.array(obs, np.float32).reshape(-1, 3), edge_inv_sigma2=np.array(info, np.float32),
                robust=fx["robust"], max_iterations=fx["optimize"][1], stop_byte=np.array([fx["params"].get("stop", 0)], np.uint8))
    r = F.bundle_adjustment_host(case, lib=lib)
    return dict(cams=cams, pts=pts, pose=np.concatenate([r["cam_q"], r["cam_t"]], 1), point=r["point"], iterations=int(r["iterations"]),
                trials=int(r["trials"]), polls=int(r["polls"]), scene=s)


def main():
    exe = build_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    for name, params in CASES.items():
        fx = reference_run(exe, params)
        path = os.path.join(GOLDEN, name + ".json")
        with open(path, "w") as f:
            json.dump(fx, f, separators=(",", ":"))
            f.write("\n")
        assert os.path.getsize(path) <= 16 * 1024, (path, os.path.getsize(path))
        print("%s: optimize %s, robust %d, %d vertices, %d edges, %d removed, %d bytes" % (
            name, fx["optimize"], fx["robust"], len(fx["vertex"]) // 4, len(fx["edge"]) // 3, len(fx["removed"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
