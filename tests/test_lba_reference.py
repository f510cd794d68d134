"""LocalBundleAdjustment's control flow against the reference's own lines.  The fixtures under tests/golden/lba are what
src/Optimizer.cc:1116-1498 - copied at test time and compiled unmodified against tests/lba_ref_types.h (tests/lba_golden.py) - did
on generated scenes: the counters, the vertices and edges in the order added, the optimize() call, every pose and position with
its write counts, and the erase calls in order.  Checked here, without the reference: the host build run on the RECORDED vertices
and edges reproduces every fixture's poses, positions and erase calls bit for bit, and so does the drop-in
rgbl_shim::LocalBundleAdjustment (tests/lba_shim_test.cpp) on the scene, with the counters and the write counts.  With the
reference: its lines reproduce the fixtures, and agree with the drop-in on fresh seeds.
This pins the three lists, num_fixedKF, the vertex ids, the monocular / stereo split, the edge order, the stop return, the erase
order and the write-back; NOT g2o's arithmetic (tests/lba_ref_types.h)."""
import os

import numpy as np
import pytest

import lba_golden as lg
import test_lba_shim as shim

needs_reference = pytest.mark.skipif(not lg.have_reference(), reason="the reference sources are not on this machine")
DROP_IN = ("head", "pose", "set_pose", "point", "set_pos", "updated", "erase")


def drop_in_exe():
    exe = os.path.join(shim.BUILD, "lba_shim_test_emu")
    shim.build(shim.BUILD, "rgbl_frontend_emu", exe)
    return exe


@pytest.mark.parametrize("name", sorted(lg.CASES))
def test_host_build_reproduces_golden_run(emu_lib, name):
    fx = lg.load(name)
    assert fx["params"] == lg.CASES[name] and os.path.getsize(os.path.join(lg.GOLDEN, name + ".json")) <= 16 * 1024
    if fx["optimize"][0] == 0:    # the returns at :1182 and :1406: nothing was optimised, nothing written
        s = shim.make_scene(**fx["params"])
        assert not any(fx["set_pose"]) and not any(fx["set_pos"]) and not fx["erase"] and fx["head"][3] == 0
        assert fx["pose"] == lg.hex32(np.array([np.concatenate([k["q"], k["t"]]) for k in s["kfs"]], np.float32))
        return
    got = lg.host_build_from_record(fx, emu_lib)
    assert fx["optimize"] == [1, 10, 1, got["iterations"], got["trials"]] and fx["mutex_held"] == 1
    assert got["pose"] == fx["pose"] and got["point"] == fx["point"] and got["erase"] == fx["erase"]
    nk, nm = len(fx["set_pose"]), len(fx["set_pos"])
    assert fx["set_pose"] == [int(k in got["local"]) for k in range(nk)]
    assert fx["set_pos"] == fx["updated"] == [int(p in got["pts"]) for p in range(nm)]


@pytest.mark.parametrize("name", sorted(lg.CASES))
def test_drop_in_reproduces_golden_run(emu_lib, name):
    fx = lg.load(name)
    got = lg.run(drop_in_exe(), fx["params"], False)
    for key in DROP_IN:
        assert got[key] == fx[key], (name, key)


def test_fixture_conditions():
    """what the fixtures have to contain: monocular and stereo edges mixed and erase calls of both kinds, monocular first; a
    covisible key frame that is bad or of another map left out; a fixed camera without any edge (seen through a left index of
    -1 only); the initial key frame fixed inside the local list; the returns at :1182 (no fixed key frame: num_OptKF and
    num_edges untouched) and :1406 (num_edges set, nothing optimised); user_lambda_init 100 on an inertial map"""
    fx = {name: lg.load(name) for name in lg.CASES}
    m = fx["main"]
    E = np.array(m["edge"]).reshape(-1, 3)
    V = np.array(m["vertex"]).reshape(-1, 4)
    assert (E[:, 0] == 0).any() and (E[:, 0] == 1).any() and m["head"][2] == len(E) and m["head"][1] == 3 and m["head"][0] == 3
    cam_ids = V[V[:, 1] == 0][:, 0]
    assert len(cam_ids) == 6 and len(set(cam_ids) - set(E[:, 2])) == 1            # a fixed camera without an edge
    assert m["delta"] == [np.float64(np.float32(np.sqrt(5.991))).tobytes().hex(), np.float64(np.float32(np.sqrt(7.815))).tobytes().hex()]
    calls = np.array(m["erase"]).reshape(-1, 3)
    assert len(calls) > 20 and (calls[0::2, 0] == 0).all() and (calls[1::2, 0] == 1).all() and (calls[0::2, 1:] == calls[1::2, 1:]).all()
    assert fx["foreign_neighbour"]["head"][1] == 2 and fx["main"]["user_lambda_init"] == 0.0
    i = fx["initial_kf"]
    Vi = np.array(i["vertex"]).reshape(-1, 4)
    assert i["head"][0] == 1 + (Vi[Vi[:, 1] == 0][i["head"][1]:, 2] == 1).sum() and Vi[Vi[:, 1] == 0][:i["head"][1], 2].sum() == 1
    assert fx["no_fixed"]["head"] == [0, -7, -7, 0, -7] and fx["no_fixed"]["optimize"][0] == 0
    assert fx["stop_set"]["head"][2] > 0 and fx["stop_set"]["optimize"][0] == 0 and fx["stop_set"]["head"][3] == 0
    assert fx["inertial"]["user_lambda_init"] == 100.0 and fx["inertial"]["optimize"][0] == 1


@needs_reference
@pytest.mark.parametrize("name", sorted(lg.CASES))
def test_reference_lines_reproduce_golden(emu_lib, name):
    """the committed fixtures are what Optimizer.cc:1116-1498, compiled unmodified, does"""
    assert lg.reference_run(lg.build_reference(), lg.CASES[name]) == lg.load(name)


@needs_reference
def test_drop_in_equals_reference_lines_on_fresh_seeds(emu_lib):
    ref, exe = lg.build_reference(), drop_in_exe()
    erased = 0
    for params in (dict(seed=21), dict(seed=22, init_in_local=True), dict(seed=23, inertial=1), dict(seed=24, stop=1)):
        want, got = lg.reference_run(ref, params), lg.run(exe, params, False)
        for key in DROP_IN:
            assert got[key] == want[key], (params, key)
        erased += len(want["erase"])
    assert erased > 0
