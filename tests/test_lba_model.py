"""The host build of csrc/lba_math.h (rgbl_local_bundle_adjustment_host) against tests/lba_model.py, the float64 numpy model
written from the g2o sources with the full normal equations and a LAPACK solve.  Poses and points are held within 16 x the
model's OWN reordering noise - the larger of (edges permuted) and (solved with the Schur complement) against the plain run,
measured here per case and recorded in tests/golden/lba/README.md -, with 2^-52 of the quantity's size as the floor of that
noise.  Decisions are equal: iterations, the accept / reject sequence (through every prefix of iterations), failed factorisations, and the erase and
depth flags; each case first shows on the model alone that no decision lies inside the margin around 5.991 / 7.815 / 0."""
import numpy as np
import pytest

import lba_checks as lk
import lba_model as M
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import lba_cases as lc

MARGIN = 16.0   # the project's margin (sim3_opt, mlpnp)


def mid_size():
    return lc.make_lba_case(n_free=9, n_fixed=4, n_points=200, obs_per_point=(2, 7), seed=31, outlier_share=0.03)


CASES = dict(minimal=lk.minimal, mixed=lk.mixed, single_observations=lk.single_observations,
             initial_kf=lk.initial_kf_is_the_only_fixed, free_camera_without_edges=lk.free_camera_without_edges,
             fixed_only_points=lk.points_seen_by_fixed_cameras_only, mid_size=mid_size, rejected_trials=lk.far_start,
             ends_on_rejected=lk.ends_on_rejected,
             user_lambda_init=lambda: dict(lk.mixed(), user_lambda_init=100.0), one_iteration=lambda: dict(lk.mixed(), max_iterations=1))


def measure(case):
    """the model three ways and the host build: dict(noise=, diff=) per quantity, and the four results"""
    base = M.run(case)
    perm = M.run(case, perm=np.random.default_rng(7).permutation(len(case["edge_point"])))
    schur = M.run(case, schur=True)
    nf = case["n_free"]
    host = F.local_bundle_adjustment_host(case, lib=measure.lib)
    hR = np.array([M.rot_of_quat(q) for q in host["q"]]).reshape(nf, 3, 3)
    fig = {}
    for key, get, h in (("R", lambda r: r["R"][:nf], hR), ("t", lambda r: r["t"][:nf], host["t"]), ("X", lambda r: r["X"], host["X"]),
                        ("chi2", lambda r: r["chi2"], host["chi2"])):
        b = get(base)
        floor = 2.0 ** -52 * max(float(np.abs(b).max()), 1.0)
        noise = max(float(np.abs(get(perm) - b).max()), float(np.abs(get(schur) - b).max()), floor)
        fig[key] = (noise, float(np.abs(h - b).max()))
    return fig, base, perm, schur, host


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_build_within_the_models_own_noise(emu_lib, name):
    measure.lib = emu_lib
    case = CASES[name]()
    fig, base, perm, schur, host = measure(case)
    print(name, " ".join("%s: noise %.3g diff %.3g" % (k, v[0], v[1]) for k, v in fig.items()))
    # the model alone: the same decisions three ways, none of them inside the margin
    for other in (perm, schur):
        assert (other["iterations"], other["accepted"], other["failed"]) == (base["iterations"], base["accepted"], base["failed"])
        assert (other["flags"] == base["flags"]).all()
    stereo = ~(case["edge_obs"][:, 2] < 0)
    assert (np.abs(base["chi2"] - np.where(stereo, 7.815, 5.991)) > MARGIN * fig["chi2"][0]).all()
    assert (np.abs(base["depth"]) > MARGIN * fig["X"][0]).all()
    # the host build: the model's decisions, the model's numbers
    assert host["ran"] == base["ran"] == 1
    assert (host["iterations"], host["trials"], host["rejected"], host["failed"]) == \
        (base["iterations"], base["trials"], base["accepted"].count(False), base["failed"])
    assert (host["flags"] == base["flags"]).all()
    # the accept / reject SEQUENCE: the host build stopped after every prefix of k iterations has run the model's trials of
    # those iterations; inside an iteration the rejected trials come first and at most the last one is accepted
    assert sum(base["per_iteration"]) == base["trials"]
    for k in range(1, base["iterations"] + 1):
        prefix = F.local_bundle_adjustment_host(dict(case, max_iterations=k), lib=emu_lib)
        trials = sum(base["per_iteration"][:k])
        assert (prefix["iterations"], prefix["trials"], prefix["rejected"]) == (k, trials, base["accepted"][:trials].count(False)), (name, k)
    for key in ("R", "t", "X"):
        assert fig[key][1] <= MARGIN * fig[key][0], (key, fig[key])


def test_runs_that_return_early(emu_lib):
    for case in (lk.no_fixed_camera(), dict(lk.mixed(), stop_after_polls=1)):
        assert M.run(case)["ran"] == 0 and F.local_bundle_adjustment_host(case, lib=emu_lib)["ran"] == 0
    case = dict(lk.far_start(), stop_after_polls=5)
    m, h = M.run(case), F.local_bundle_adjustment_host(case, lib=emu_lib)
    assert (h["iterations"], h["trials"], h["rejected"], h["polls"]) == (m["iterations"], m["trials"], m["accepted"].count(False), m["polls"])
    assert m["accepted"][-1] is False   # the run ended inside the trial loop
