"""The recorded bits of the two optimisers' HOST builds (rgbl_pose_optimization_host, rgbl_optimize_sim3_host):
tests/golden/pose_opt/host_bits.json and tests/golden/sim3_opt/host_bits.json, written by tests/golden/make_host_bits.py.
The device tests compare the kernel with the host build of the same library, so a change that moves both together would pass
them; these records hold the host build, the emulated kernel and the MI355X to what the code computed when they were written.

A record: the return value, rounds, iterations and active, the counters (OptimizeSim3), the estimate and chi2 as hex of their
fp64 bits (PoseOptimization: the fp32 pose as well) with NaN written as "nan" - NaN is compared as NaN, not by payload, as
same() of the two *_checks.py does -, and a SHA-256 of the flag array."""
import hashlib
import json
import os

import numpy as np

import pose_opt_checks as pc
import sim3_opt_checks as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL = 7   # what the flags hold before a call: a byte no call writes
EMU_MAX = 257   # the emulated kernel is held to the records up to this many correspondences; beyond it is slow


def path(which):
    return os.path.join(GOLDEN, which, "host_bits.json")


def recorded(which):
    return json.load(open(path(which)))


def bits(a):
    a = np.atleast_1d(np.asarray(a))
    u = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return ["nan" if np.isnan(x) else "%0*x" % (2 * a.dtype.itemsize, int(w)) for x, w in zip(a, u)]


def pose_size_cases():
    """[(name, case, correspondences)] of pose_opt_checks.SIZES x KINDS"""
    return [("%d matched, %s" % (m, kind), pc.sized_case(m, kind), m) for m in pc.SIZES for kind in pc.KINDS]


def pose_cases():
    import test_pose_opt_math as pmath
    out = pose_size_cases()
    out.append(("all outliers", pc.all_outliers_case(), 60))
    out += [("degenerate depth, stereo %d" % s, pc.degenerate_depth_case(s), 30) for s in (False, True)]
    out += [("math: " + name, case, int((np.asarray(case["mp_index"]) >= 0).sum())) for name, case in pmath.all_cases()]
    return out


def pose_record(res):
    return dict(result=int(res["result"]), rounds=int(res["rounds"]), iterations=[int(v) for v in res["iterations"]],
                active=[int(v) for v in res["active"]], chi2=bits(res["chi2"]), q64=bits(res["q64"]), t64=bits(res["t64"]),
                q=bits(res["q"]), t=bits(res["t"]), outlier_sha256=hashlib.sha256(np.ascontiguousarray(res["outlier"]).tobytes()).hexdigest())


def sim3_size_cases():
    """[(name, case, matches)] of sim3_opt_checks.SIZES x fix_scale"""
    return [("%d matched, fix_scale %d" % (m, fs), oc.sized_case(m, fs), m) for m in oc.SIZES for fs in (False, True)]


def sim3_cases():
    out = sim3_size_cases()
    out.append(("degenerate", oc.degenerate_case(), 60))
    out += [("no edge: " + name, case, 30) for name, case in oc.no_edge_cases().items()]
    out += [("batch problem %d" % b, case, int((np.asarray(case["match_index"]) >= 0).sum())) for b, case in enumerate(oc.batch_problems(11))]
    return out


def sim3_record(res):
    out = dict(result=int(res["result"]), rounds=int(res["rounds"]), iterations=[int(v) for v in res["iterations"]],
               active=[int(v) for v in res["active"]], chi2=bits(res["chi2"]), q=bits(res["q"]), t=bits(res["t"]), s=bits(np.float64(res["s"])),
               cleared_sha256=hashlib.sha256(np.ascontiguousarray(res["cleared"]).tobytes()).hexdigest())
    out.update({k: int(res[k]) for k in oc.COUNTERS})
    return out
