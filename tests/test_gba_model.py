"""The host build of rgbl_bundle_adjustment (csrc/lba_math.h with lm_solve_panel) against tests/lba_model.py, the float64 numpy
model written from the g2o sources with the full normal equations and a LAPACK solve - imported, not edited, and extended in
tests/gba_model.py for what Optimizer::BundleAdjustment does differently: its own Huber deltas (:131-132: sqrt(5.99), not
sqrt(5.991)), edges without a kernel (bRobust = false: rho = (chi2, 1, 0)) and no early return (no fixed camera, or a stop flag
set on entry, still run optimize()).  Margin and procedure are those of
tests/golden/lba/README.md: poses and points within 16 x the model's OWN reordering noise - the larger of (edges permuted) and
(solved with the Schur complement) against the plain run, 2^-52 of the quantity's size as its floor -, decisions equal
(iterations, the accept / reject sequence through every prefix of iterations, failed factorisations).  A case is admitted only
if the model's three runs agree on every decision among themselves; the test asserts it.  The function has no erase flags, so
no chi2 is compared with a threshold.  tests/golden/gba/README.md has the measured table.

The cross-check: with at most 128 active cameras, robust edges and a fixed camera, rgbl_local_bundle_adjustment_host on the
same vertices and edges differs from the new call in the order of the backward substitution and in the monocular Huber delta
(sqrt(5.991) there, sqrt(5.99) here).  Where no kernel ever acts - asserted per case - only the order is left, and the two are
held within the same noise."""
import numpy as np
import pytest

import gba_checks as gk
import lba_model as M
from gba_model import figures, model_run, three_runs
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import lba_cases as lc

MARGIN = 16.0   # the project's margin (tests/golden/lba/README.md)


CASES = dict(one_camera=lambda: gk.sized(1, n_points=12, obs_per_point=2), panel_below=lambda: gk.sized(gk.PANEL_SIZES[1]),
             panel_above=lambda: gk.sized(gk.PANEL_SIZES[2]), panels_3=lambda: gk.sized(gk.PANEL_SIZES[-1]),
             robust=lambda: gk.mixed(robust=1), plain=lambda: gk.mixed(robust=0),
             monocular=lambda: lc.make_ba_case(n_cams=6, n_fixed=1, n_points=60, obs_per_point=(3, 5), seed=31, stereo_share=0.0),
             mixed_edges=lambda: lc.make_ba_case(n_cams=6, n_fixed=1, n_points=60, obs_per_point=(3, 5), seed=31, stereo_share=0.5),
             plain_20_iterations=lambda: gk.mixed(robust=0, max_iterations=20),
             no_fixed_camera=lambda: gk.sized(4, n_fixed=0, max_iterations=4), rejected_trials=gk.far_start)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_build_within_the_models_own_noise(emu_lib, name):
    case = CASES[name]()
    base, perm, schur = three_runs(case)
    host = F.bundle_adjustment_host(case, lib=emu_lib)
    fig = figures(case, base, perm, schur, host)
    print(name, " ".join("%s: noise %.3g diff %.3g" % (k, v[0], v[1]) for k, v in fig.items()))
    assert host["ran"] == base["ran"] == 1
    assert (host["iterations"], host["trials"], host["rejected"], host["failed"], host["polls"]) == \
        (base["iterations"], base["trials"], base["accepted"].count(False), base["failed"], base["polls"])
    assert sum(base["per_iteration"]) == base["trials"]
    for k in range(1, base["iterations"] + 1):
        prefix = F.bundle_adjustment_host(dict(case, max_iterations=k), lib=emu_lib)
        trials = sum(base["per_iteration"][:k])
        assert (prefix["iterations"], prefix["trials"], prefix["rejected"]) == (k, trials, base["accepted"][:trials].count(False)), (name, k)
    for key in ("R", "t", "X"):
        assert fig[key][1] <= MARGIN * fig[key][0], (key, fig[key])


def test_a_stop_is_no_early_return(emu_lib):
    c = gk.far_start()
    for n in (1, 2, 5):
        case = dict(c, stop_after_polls=n)
        m, h = model_run(case), F.bundle_adjustment_host(case, lib=emu_lib)
        assert m["ran"] == h["ran"] == 1
        assert (h["iterations"], h["trials"], h["rejected"], h["polls"]) == (m["iterations"], m["trials"], m["accepted"].count(False), m["polls"]), n
    assert model_run(dict(c, stop_after_polls=1))["iterations"] == 0


def near_the_plant(nA, **kw):
    """a start so close to the plant, with so little pixel noise, that no edge ever reaches a Huber delta"""
    return gk.sized(nA, pose_noise=(2e-4, 2e-3), point_noise=2e-3, pixel_noise=0.15, **kw)


NEAR = dict(panel_below=lambda: near_the_plant(gk.PANEL_SIZES[1]), panel_above=lambda: near_the_plant(gk.PANEL_SIZES[2]),
            panels_3=lambda: near_the_plant(gk.PANEL_SIZES[-1]), mixed_edges=lambda: near_the_plant(6, stereo_share=0.5, max_iterations=10),
            monocular=lambda: near_the_plant(6, stereo_share=0.0, max_iterations=10))


@pytest.mark.parametrize("name", sorted(NEAR))
def test_local_bundle_adjustment_differs_only_by_the_backward_order(emu_lib, name):
    """The two calls differ in the backward order AND in the monocular delta (sqrt(5.991) there, sqrt(5.99) here), so they are
    compared where no kernel ever acts: a case is admitted only if the new call gives the same bytes with and without its
    kernels - then no chi2 of the run was beyond sqrt(5.99)^2, let alone beyond local BA's larger delta."""
    case = NEAR[name]()
    assert int(case["robust"]) == 1 and case["cam_is_fixed"].any() and int(case["n_cams"]) <= 128
    base, perm, schur = three_runs(case)
    ba = F.bundle_adjustment_host(case, lib=emu_lib)
    plain = F.bundle_adjustment_host(dict(case, robust=0), lib=emu_lib)
    assert ba["X"].tobytes() == plain["X"].tobytes() and ba["chi2"].tobytes() == plain["chi2"].tobytes() and ba["iterations"] > 1, "a kernel acted"
    lba = F.local_bundle_adjustment_host(lc.as_lba_case(case), lib=emu_lib)
    assert lba["ran"] == 1
    assert [lba[k] for k in ("iterations", "trials", "rejected", "failed")] == [ba[k] for k in ("iterations", "trials", "rejected", "failed")]
    fig = figures(case, base, perm, schur, ba)
    nc = int(case["n_cams"])
    R = lambda r: np.array([M.rot_of_quat(q) for q in r["q"]]).reshape(nc, 3, 3)
    diff = dict(R=float(np.abs(R(ba) - R(lba)).max()), t=float(np.abs(ba["t"] - lba["t"]).max()), X=float(np.abs(ba["X"] - lba["X"]).max()))
    print(name, " ".join("%s: noise %.3g ba-lba %.3g" % (k, fig[k][0], diff[k]) for k in diff))
    for key in diff:
        assert diff[key] <= MARGIN * fig[key][0], (key, diff[key], fig[key][0])
    if 6 * ba["active_cams"] > 2:
        assert ba["X"].tobytes() != lba["X"].tobytes() or ba["t"].tobytes() != lba["t"].tobytes(), "the two orders gave the same bits"
