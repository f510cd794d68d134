"""The golden LocalBundleAdjustment runs.  tests/golden/lba/<case>.json hold what the reference's OWN lines
src/Optimizer.cc:1116-1498 did on a generated scene (tests/test_lba_shim.py's make_scene): num_fixedKF, num_OptKF, num_edges, the
change index, every key frame's pose and every point's position afterwards with their SetPose / SetWorldPos /
UpdateNormalAndDepth counts, the erase calls in order, and what the stand-in optimiser recorded - the vertices (id, kind, fixed,
marginalized) and the edges (type, both vertex ids) in the order added, the optimize() call, user_lambda_init, both Huber deltas.

    python tests/lba_golden.py         # rewrites the fixtures (needs the reference sources)

The lines are copied at test time into tests/_build/lba_ref_body.inc (never committed) and compiled unmodified against
tests/lba_ref_types.h (tests/lba_ref_glue.cpp).  This pins the three lists, num_fixedKF, the vertex ids, the monocular / stereo
split, the edge order, the stop return, the erase order and the write-back.  It does NOT pin g2o's arithmetic: the stand-in
SparseOptimizer::optimize runs rgbl_local_bundle_adjustment_host.  A scene is regenerated from the parameters in its fixture."""
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

import test_lba_shim as shim  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "lba")
BUILD = os.path.join(TESTS, "_build")
REF = "/root/reference"
SOURCE, FIRST, LAST = "src/Optimizer.cc", 1116, 1498

CASES = {
    "main": dict(seed=4),
    "foreign_neighbour": dict(seed=7),
    "initial_kf": dict(seed=6, init_in_local=True),
    "stop_set": dict(seed=4, stop=1),
    "no_fixed": dict(seed=8, no_fixed=True),
    "inertial": dict(seed=10, inertial=1),
}


def have_reference():
    return os.path.exists(os.path.join(REF, SOURCE))


def build_reference():
    """tests/_build/lba_ref: the reference's lines behind tests/lba_ref_glue.cpp, on the emulator library's host build"""
    exe, inc = os.path.join(BUILD, "lba_ref"), os.path.join(BUILD, "lba_ref_body.inc")
    os.makedirs(BUILD, exist_ok=True)
    lines = open(os.path.join(REF, SOURCE), errors="replace").read().splitlines(True)
    body = "".join(lines[FIRST - 1:LAST])
    assert body.startswith("void Optimizer::LocalBundleAdjustment(") and body.rstrip().endswith("}"), body[:80]
    if not os.path.exists(inc) or open(inc).read() != body:
        with open(inc, "w") as f:
            f.write(body)
    glue, lib = os.path.join(TESTS, "lba_ref_glue.cpp"), os.path.join(BUILD, "librgbl_frontend_emu.so")
    deps = [inc, glue, lib, os.path.join(TESTS, "lba_ref_types.h"), os.path.join(ROOT, "include", "rgbl_frontend.h")]
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
    """out.bin of tests/lba_shim_test.cpp (the drop-in) or tests/lba_ref_glue.cpp (the reference's lines, with the record)"""
    nk, nm = len(scene["kfs"]), len(scene["mps"])
    head = list(struct.unpack_from("<6i", buf))
    pose = np.frombuffer(buf, np.float32, 8 * nk, 24).reshape(nk, 8)
    pt = np.frombuffer(buf, np.float32, 5 * nm, 24 + 32 * nk).reshape(nm, 5)
    off = 24 + 32 * nk + 20 * nm
    n_calls = struct.unpack_from("<i", buf, off)[0]
    calls = [int(v) for v in np.frombuffer(buf, np.int32, n_calls, off + 4)]
    off += 4 + 4 * n_calls
    r = dict(head=head[1:], pose=hex32(pose[:, :7]), set_pose=[int(v) for v in pose[:, 7]], point=hex32(pt[:, :3]),
             set_pos=[int(v) for v in pt[:, 3]], updated=[int(v) for v in pt[:, 4]], erase=calls)
    if with_record:
        tail = struct.unpack_from("<8i", buf, off)
        off += 32
        vertex = [int(v) for v in np.frombuffer(buf, np.int32, tail[0], off)]
        off += 4 * tail[0]
        edge = [int(v) for v in np.frombuffer(buf, np.int32, tail[1], off)]
        off += 4 * tail[1]
        dbl = struct.unpack_from("<3d", buf, off)
        off += 24
        r.update(vertex=vertex, edge=edge, optimize=list(tail[2:7]), mutex_held=tail[7], user_lambda_init=dbl[0],
                 delta=[np.float64(dbl[1]).tobytes().hex(), np.float64(dbl[2]).tobytes().hex()])
    else:
        assert head[0] == 1, "the drop-in refused the scene"
    assert off == len(buf)
    return r


def run(exe, params, with_record):
    scene = shim.make_scene(**params)
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
        shim.write_scene(scene, path)
        res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and ("LBA_REF_OK" in res.stdout or "LBA_SHIM_OK" in res.stdout), res.stdout[-3000:] + res.stderr[-3000:]
        return parse(open(out, "rb").read(), scene, with_record)


def reference_run(exe, params):
    return dict(params=params, **run(exe, params, True))


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def host_build_from_record(fx, lib):
    """rgbl_local_bundle_adjustment_host on the vertices and edges the fixture RECORDED (no walk of this project's is involved):
    the local key frames are the first num_OptKF camera vertices.  Returns what the fixture must hold: poses, positions, erase calls."""
    from orb_slam3_rgbl_amd import frontend as F
    s = shim.make_scene(**fx["params"])
    kfs = s["kfs"]
    kf_of = {k["id"]: i for i, k in enumerate(kfs)}
    V = np.array(fx["vertex"], np.int64).reshape(-1, 4)
    E = np.array(fx["edge"], np.int64).reshape(-1, 3)
    cams = [kf_of[int(v[0])] for v in V if v[1] == 0]
    max_kf_id = max(int(v[0]) for v in V if v[1] == 0)
    pts = [(int(v[0]) - max_kf_id - 1 - 1000) // 7 for v in V if v[1] == 1]
    assert all(v[3] == 1 and v[2] == 0 for v in V if v[1] == 1) and all(v[3] == 0 for v in V if v[1] == 0)
    n_opt = fx["head"][1]
    cam_col = {kfs[k]["id"]: c for c, k in enumerate(cams)}
    pt_col = {1000 + 7 * p + max_kf_id + 1: j for j, p in enumerate(pts)}
    obs, info = [], []
    for typ, pid, cid in E:
        k, p = kf_of[int(cid)], pts[pt_col[int(pid)]]
        feat = [f for f in kfs[k]["feats"] if f[4] == p]
        assert len(feat) == 1 and (feat[0][3] >= 0) == (typ == 1) and (feat[0][3] < 0) == (typ == 0)
        obs.append([feat[0][0], feat[0][1], feat[0][3] if typ == 1 else -1.0])
        info.append(shim.SIGMA[feat[0][2]])
    case = dict(n_free=len(cams), n_fixed=0, free_is_fixed=np.array([v[2] for v in V if v[1] == 0], np.uint8),
                cam_q=np.array([kfs[k]["q"] for k in cams], np.float32), cam_t=np.array([kfs[k]["t"] for k in cams], np.float32),
                cam_K=np.array([kfs[k]["K"] for k in cams], np.float32), cam_bf=np.array([kfs[k]["bf"] for k in cams], np.float32),
                world_pos=np.array([s["mps"][p]["pos"] for p in pts], np.float32).reshape(-1, 3), n_points=len(pts),
                edge_point=np.array([pt_col[int(e[1])] for e in E], np.int32), edge_cam=np.array([cam_col[int(e[2])] for e in E], np.int32),
                edge_obs=np.array(obs, np.float32).reshape(-1, 3), edge_inv_sigma2=np.array(info, np.float32),
                user_lambda_init=fx["user_lambda_init"], max_iterations=fx["optimize"][1])
    r = F.local_bundle_adjustment_host(case, lib=lib)
    pose = np.array([np.concatenate([k["q"], k["t"]]) for k in kfs], np.float32)
    point = np.array([m["pos"] for m in s["mps"]], np.float32)
    for c in range(n_opt):
        pose[cams[c]] = np.concatenate([r["cam_q"][c], r["cam_t"][c]])
    point[pts] = r["point"]
    stereo = E[:, 0] == 1
    order = [e for e in np.flatnonzero(~stereo) if r["flags"][e] & 1] + [e for e in np.flatnonzero(stereo) if r["flags"][e] & 1]
    erase = []
    for e in order:
        k, p = kf_of[int(E[e, 2])], pts[pt_col[int(E[e, 1])]]
        erase += [0, k, p, 1, k, p]
    return dict(pose=hex32(pose), point=hex32(point), erase=erase, iterations=int(r["iterations"]), trials=int(r["trials"]), local=cams[:n_opt], pts=pts)


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
        print("%s: head %s, optimize %s, %d erase calls, %d bytes" % (name, fx["head"], fx["optimize"], len(fx["erase"]) // 6, os.path.getsize(path)))


if __name__ == "__main__":
    main()
