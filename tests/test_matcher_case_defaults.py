"""The matcher case generators with default arguments are what bench.py / bench_calls.py time and what every older parity test
checks: the camera= / pyramid= keywords must not move them.  tests/matcher_case_digests.json holds a SHA-256 per returned array,
computed with the generators as they were BEFORE the keywords existed (run this file as a script against that tree to
regenerate: `python test_matcher_case_defaults.py out.json` with the old package on PYTHONPATH)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "matcher_case_digests.json")


def generators():
    from orb_slam3_rgbl_amd import cases
    if hasattr(cases, "make_sim3_case"):
        sim3, project = cases.make_sim3_case, cases.make_project_search_case
    else:   # the tree the digests come from kept these two with the tests
        import parity_checks as pc
        sim3, project = pc.make_sim3_case, pc.make_project_search_case
    return {
        "projection": lambda: cases.make_projection_case(),
        "projection_backward_small": lambda: cases.make_projection_case(300, 400, 5, "backward"),
        "projection_640x360": lambda: cases.make_projection_case(200, 300, 7, "none", 640, 360),
        "local_points": lambda: cases.make_local_points_case(),
        "local_points_400x300": lambda: cases.make_local_points_case(300, 200, 43, 400, 300),
        "relocalization": lambda: cases.make_relocalization_case(),
        "fuse": lambda: cases.make_fuse_case(),
        "initialization": lambda: cases.make_initialization_case(),
        "initialization_small": lambda: cases.make_initialization_case(600, 62, 640, 360),
        "sim3": lambda: sim3(),
        "sim3_640x360": lambda: sim3(400, 123, 640, 360),
        "project_search": lambda: project(),
    }


def digest(value):
    a = np.ascontiguousarray(value)
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def case_digests(case, prefix=""):
    out = {}
    for k in sorted(case):
        if isinstance(case[k], dict):
            out.update(case_digests(case[k], prefix + k + "."))
        else:
            out[prefix + k] = digest(case[k])
    return out


def all_digests():
    return {name: case_digests(make()) for name, make in generators().items()}


def test_default_arguments_return_what_they_always_returned():
    want = json.load(open(DIGESTS))
    got = all_digests()
    assert sorted(got) == sorted(want)
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        for key in want[name]:
            assert got[name][key] == want[name][key], "%s: %s moved" % (name, key)


def test_the_control_camera_and_pyramid_are_the_defaults():
    """camera="kitti", pyramid=(8, 1.2) spelled out is the default case: one code path, not a copy of it."""
    from orb_slam3_rgbl_amd import cases
    want = json.load(open(DIGESTS))
    kw = dict(camera="kitti", pyramid=(8, 1.2))
    for name, case in (("projection", cases.make_projection_case(**kw)), ("local_points", cases.make_local_points_case(**kw)),
                       ("relocalization", cases.make_relocalization_case(**kw)), ("fuse", cases.make_fuse_case(**kw)),
                       ("initialization", cases.make_initialization_case(**kw)), ("sim3", cases.make_sim3_case(**kw)),
                       ("project_search", cases.make_project_search_case(**kw))):
        assert case_digests(case) == want[name], name


if __name__ == "__main__":
    json.dump(all_digests(), open(sys.argv[1], "w"), indent=1, sort_keys=True)
