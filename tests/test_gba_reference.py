"""BundleAdjustment's control flow and constants against the reference's own lines.  The fixtures under tests/golden/gba are what
src/Optimizer.cc:60-390 - copied at test time and compiled unmodified against tests/gba_ref_types.h (tests/gba_golden.py) - did on
generated scenes: the vertices and edges in the order added, the removed vertices, the optimize() call, bRobust and both Huber
deltas, every pose and position with the member it was written to.  Checked here, without the reference: the host build run on
the RECORDED vertices and edges reproduces every fixture's poses and positions bit for bit, and so does the drop-in
rgbl_shim::BundleAdjustment (tests/gba_shim_test.cpp) on the scene, with every write count and mark.  With the reference: its
lines reproduce the fixtures, and agree with the drop-in on fresh seeds.
This pins the vertex ids, the fixed flag, the edge order and split, bRobust, the deltas sqrt(5.99) / sqrt(7.815), nIterations and
both write-back branches; NOT g2o's arithmetic (tests/gba_ref_types.h)."""
import os

import numpy as np
import pytest

import gba_golden as gg
import test_gba_shim as shim

needs_reference = pytest.mark.skipif(not gg.have_reference(), reason="the reference sources are not on this machine")
DROP_IN = ("pose", "set_pose", "gba_pose", "kf_gba_for", "point", "set_pos", "updated", "gba_point", "mp_gba_for")
DELTAS = [np.float64(np.float32(np.sqrt(5.99))).tobytes().hex(), np.float64(np.float32(np.sqrt(7.815))).tobytes().hex()]


def drop_in_exe():
    exe = os.path.join(shim.BUILD, "gba_shim_test_emu")
    shim.build(shim.BUILD, "rgbl_frontend_emu", exe)
    return exe


def floats(hexed, cols):
    return np.frombuffer(bytes.fromhex(hexed), ">u4").astype(np.uint32).view(np.float32).reshape(-1, cols)


@pytest.mark.parametrize("name", sorted(gg.CASES))
def test_host_build_reproduces_golden_run(emu_lib, name):
    fx = gg.load(name)
    assert fx["params"] == gg.CASES[name] and os.path.getsize(os.path.join(gg.GOLDEN, name + ".json")) <= 16 * 1024
    got = gg.host_build_from_record(fx, emu_lib)
    s = got["scene"]
    nk, nm = len(s["kfs"]), len(s["mps"])
    assert fx["optimize"] == [1, fx["params"]["iterations"], got["iterations"], got["trials"]] and fx["polls"] == got["polls"]
    pose0 = np.array([np.concatenate([k["q"], k["t"]]) for k in s["kfs"]], np.float32)
    point0 = np.array([m["pos"] for m in s["mps"]], np.float32)
    identity = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (nk, 1))
    in_cams = [int(k in got["cams"]) for k in range(nk)]
    in_pts = [int(p in got["pts"]) for p in range(nm)]
    want_pose, want_point = pose0.copy(), point0.copy()
    want_gba_pose, want_gba_point = identity.copy(), np.zeros((nm, 3), np.float32)
    loop_kf = s["loop_kf"]
    if fx["params"]["initialisation"]:   # :295, :381-382
        want_pose[got["cams"]] = got["pose"]
        want_point[got["pts"]] = got["point"]
        assert fx["set_pose"] == in_cams and fx["set_pos"] == fx["updated"] == in_pts
        assert not any(fx["kf_gba_for"]) and not any(fx["mp_gba_for"])
    else:                                # :299-300, :386-387
        want_gba_pose[got["cams"]] = got["pose"]
        want_gba_point[got["pts"]] = got["point"]
        assert not any(fx["set_pose"]) and not any(fx["set_pos"]) and not any(fx["updated"])
        assert fx["kf_gba_for"] == [loop_kf * v for v in in_cams] and fx["mp_gba_for"] == [loop_kf * v for v in in_pts]
    assert fx["pose"] == gg.hex32(want_pose) and fx["gba_pose"] == gg.hex32(want_gba_pose)
    assert fx["point"] == gg.hex32(want_point) and fx["gba_point"] == gg.hex32(want_gba_point)


@pytest.mark.parametrize("name", sorted(gg.CASES))
def test_drop_in_reproduces_golden_run(emu_lib, name):
    fx = gg.load(name)
    got = gg.run(drop_in_exe(), fx["params"], False)
    for key in DROP_IN:
        assert got[key] == fx[key], (name, key)


def test_fixture_conditions():
    """what the fixtures have to contain: the deltas of :131-132 (5.99, not LocalBundleAdjustment's 5.991) where bRobust is set and
    no kernel where it is not; 5, 10 and 20 iterations; monocular and stereo edges mixed; exactly one fixed camera, the one whose
    id is the map's GetInitKFid(); no vertex for the bad key frame nor for the two outside vpKFs, no edge to them; no vertex for
    the bad point; the point only those two see removed and not written; the point seen only through a left index of -1 kept
    and written as it came; both write-back branches; the stop flag set: optimize() called, one poll, no iteration"""
    fx = {name: gg.load(name) for name in gg.CASES}
    for name, f in fx.items():
        s = shim.make_scene(**f["params"])
        V = np.array(f["vertex"]).reshape(-1, 4)
        E = np.array(f["edge"]).reshape(-1, 3)
        cam_ids = [int(v) for v in V[V[:, 1] == 0][:, 0]]
        assert f["robust"] == f["params"]["robust"] and f["delta"] == (DELTAS if f["robust"] else ["0" * 16, "0" * 16]), name
        assert f["optimize"][0] == 1 and f["optimize"][1] == f["params"]["iterations"], name
        assert (E[:, 0] == 0).any() and (E[:, 0] == 1).any(), name
        assert cam_ids == [s["kfs"][k]["id"] for k in s["list_kf"] if not s["kfs"][k]["bad"]], name     # vpKFs' order, without the bad one
        assert [int(v[0]) for v in V if v[2] == 1] == [s["init_id"]], name
        assert not {s["kfs"][3]["id"], 900, 41} & (set(cam_ids) | set(int(c) for c in E[:, 2])), name
        max_id = max(cam_ids)
        pt_ids = [int(v) for v in V[V[:, 1] == 1][:, 0]]
        assert pt_ids == [s["mps"][p]["id"] + max_id + 1 for p in s["list_mp"] if not s["mps"][p]["bad"]], name     # vpMP's order
        assert f["removed"] == [s["mps"][21]["id"] + max_id + 1], name
        id30 = s["mps"][30]["id"] + max_id + 1
        assert id30 in pt_ids and id30 not in E[:, 1], name
        point = floats(f["point"], 3) if f["params"]["initialisation"] else floats(f["gba_point"], 3)
        assert point[30].tobytes() == np.asarray(s["mps"][30]["pos"], np.float32).tobytes(), name
        written = f["set_pos"] if f["params"]["initialisation"] else f["mp_gba_for"]
        assert written[30] and not written[21] and not written[4], name
    assert sorted(f["params"]["iterations"] for f in fx.values()) == [5, 5, 10, 10, 10, 20]
    assert fx["stop_set"]["optimize"][2:] == [0, 0] and fx["stop_set"]["polls"] == 1 and any(fx["stop_set"]["kf_gba_for"])
    assert fx["loop_closing"]["optimize"][2] > 1 and fx["initialisation"]["optimize"][2] > 1
    assert any(fx["initialisation"]["set_pose"]) and any(fx["beyond_max_kfid"]["set_pos"]) and any(fx["loop_closing"]["kf_gba_for"])


@needs_reference
@pytest.mark.parametrize("name", sorted(gg.CASES))
def test_reference_lines_reproduce_golden(emu_lib, name):
    """the committed fixtures are what Optimizer.cc:60-390, compiled unmodified, does"""
    assert gg.reference_run(gg.build_reference(), gg.CASES[name]) == gg.load(name)


@needs_reference
def test_drop_in_equals_reference_lines_on_fresh_seeds(emu_lib):
    ref, exe = gg.build_reference(), drop_in_exe()
    for params in (dict(seed=21, initialisation=False, robust=1, iterations=10), dict(seed=22, initialisation=True, robust=0, iterations=20),
                   dict(seed=23, initialisation=True, robust=1, iterations=5, stop=1), dict(seed=24, initialisation=False, robust=0, iterations=5)):
        want, got = gg.reference_run(ref, params), gg.run(exe, params, False)
        for key in DROP_IN:
            assert got[key] == want[key], (params, key)
