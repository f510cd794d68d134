"""The golden KeyFrameDatabase cases: one script of adds, erases, re-adds and queries, run on any of three back ends -
the reference's own KeyFrameDatabase.cc (tests/kfdb_ref_glue.cpp, where the reference is present), the restatement
(tests/kfdb_ref.py) and the device library.  tests/golden/kfdb/*.json hold what the reference's own code returned:

    python tests/kfdb_golden.py         # rewrites the fixtures (needs the reference sources)

A fixture stores the case's generator parameters (seeds), and per query the candidates in order plus, for every key frame
the query stamped, its id (ascending), its common-word count, whether it was scored and the score's bits.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for _p_ in (ROOT, TESTS):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

import kfdb_ref  # noqa: E402
from orb_slam3_rgbl_amd import frontend as F  # noqa: E402
from orb_slam3_rgbl_amd import kfdb_cases as kc  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "kfdb")
REF = "/root/reference"

CASES = {
    "loop": dict(n_kf=150, n_words=60, n_vocab=5000, seed=101, n_maps=2),
    "three_maps": dict(n_kf=120, n_words=90, n_vocab=3000, seed=202, n_maps=3),
    "dense": dict(n_kf=90, n_words=150, n_vocab=1500, seed=303, n_maps=2),
    # key frames change map after they were added (KeyFrame::UpdateMap after a merge), then their old map is cleared
    "map_change": dict(n_kf=80, n_words=60, n_vocab=3000, seed=404, n_maps=2, script="map_change"),
}


def have_reference():
    return os.path.isdir(os.path.join(REF, "src")) and os.path.isdir(os.path.join(REF, "Thirdparty", "DBoW2"))


def build_reference_glue():
    """The reference's KeyFrameDatabase.cc, ScoringObject.cpp and BowVector.cpp, unmodified, into tests/_build."""
    out = os.path.join(TESTS, "_build", "libref_kfdb.so")
    srcs = [os.path.join(TESTS, "kfdb_ref_glue.cpp"), os.path.join(REF, "src", "KeyFrameDatabase.cc"),
            os.path.join(REF, "Thirdparty", "DBoW2", "DBoW2", "ScoringObject.cpp"),
            os.path.join(REF, "Thirdparty", "DBoW2", "DBoW2", "BowVector.cpp")]
    deps = srcs + [os.path.join(TESTS, "kfdb_ref_types.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-shared", "-o", tmp,
                               "-include", os.path.join(TESTS, "kfdb_ref_types.h"), "-I" + os.path.join(TESTS, "kfdb_compat"),
                               "-I" + os.path.join(ROOT, "oracle", "cvcompat"), "-I" + REF, "-I" + os.path.join(REF, "include")] + srcs)
        os.replace(tmp, out)
    lib = C.CDLL(out)
    lib.ref_kfdb_create.restype = C.c_void_p
    lib.ref_kfdb_last_call_seconds.restype = C.c_double
    V, I, LL = C.c_void_p, C.c_int, C.c_longlong
    lib.ref_kfdb_create.argtypes = [I]
    lib.ref_kfdb_destroy.argtypes = [V]
    lib.ref_kfdb_add.argtypes = [V, LL, I, I, V, V]
    lib.ref_kfdb_erase.argtypes = [V, LL]
    lib.ref_kfdb_clear_map.argtypes = [V, I]
    lib.ref_kfdb_clear.argtypes = [V]
    lib.ref_kfdb_set_map.argtypes = [V, LL, I]
    lib.ref_kfdb_set_covisible.argtypes = [V, LL, I, V]
    lib.ref_kfdb_set_map_bad.argtypes = [V, I, I]
    lib.ref_kfdb_reloc.argtypes = [V, LL, I, V, V, I, V, I]
    lib.ref_kfdb_last_call_seconds.argtypes = [V]
    lib.ref_kfdb_reloc_order.argtypes = [V, LL, I, V, V, V, I]
    lib.ref_kfdb_nbest.argtypes = [V, LL, I, V, V, I, I, V, I, V, V, V, V]
    lib.ref_kfdb_stamps.argtypes = [V, I, I, V, V, V, V]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class ReferenceBackend:
    """The reference's own code."""

    def __init__(self, n_vocab, lib=None):
        self.lib = lib or build_reference_glue()
        self.h = C.c_void_p(self.lib.ref_kfdb_create(n_vocab))
        self.known = []

    def close(self):
        self.lib.ref_kfdb_destroy(self.h)

    def add(self, kf, m, wid, wval):
        wid, wval = np.ascontiguousarray(wid, np.uint32), np.ascontiguousarray(wval, np.float64)
        self.lib.ref_kfdb_add(self.h, kf, m, len(wid), _p(wid), _p(wval))
        if kf not in self.known:
            self.known.append(kf)

    def erase(self, kf):
        self.lib.ref_kfdb_erase(self.h, kf)

    def clear_map(self, m):
        self.lib.ref_kfdb_clear_map(self.h, m)

    def set_map(self, kf, m):
        self.lib.ref_kfdb_set_map(self.h, kf, m)

    def set_covisibility(self, covis, kf_map):
        for kf in self.known:
            ids = np.ascontiguousarray(covis.get(kf, []), np.int64)
            self.lib.ref_kfdb_set_covisible(self.h, kf, len(ids), _p(ids))

    def _stamps(self, which, qid):
        ids = np.array(sorted(self.known), np.int64)
        q, w, s = np.zeros(len(ids), np.int64), np.zeros(len(ids), np.int32), np.zeros(len(ids), np.float32)
        self.lib.ref_kfdb_stamps(self.h, which, len(ids), _p(ids), _p(q), _p(w), _p(s))
        hit = q == qid
        return ids[hit], w[hit], s[hit]

    def reloc(self, fid, wid, wval, m):
        wid, wval = np.ascontiguousarray(wid, np.uint32), np.ascontiguousarray(wval, np.float64)
        out = np.zeros(len(self.known) + 1, np.int64)
        n = self.lib.ref_kfdb_reloc(self.h, fid, len(wid), _p(wid), _p(wval), m, _p(out), len(out))
        return out[:n].tolist(), self._stamps(0, fid)

    def reloc_order(self, fid, wid, wval):
        wid, wval = np.ascontiguousarray(wid, np.uint32), np.ascontiguousarray(wval, np.float64)
        out = np.zeros(len(self.known) + 1, np.int64)
        n = self.lib.ref_kfdb_reloc_order(self.h, fid, len(wid), _p(wid), _p(wval), _p(out), len(out))
        return out[:n].tolist()

    def nbest(self, kid, wid, wval, m, conn, n_cand, bad_maps=()):
        wid, wval = np.ascontiguousarray(wid, np.uint32), np.ascontiguousarray(wval, np.float64)
        conn = np.ascontiguousarray(sorted(conn), np.int64)
        for b in bad_maps:
            self.lib.ref_kfdb_set_map_bad(self.h, b, 1)
        lo, me, nl, nm = np.zeros(n_cand, np.int64), np.zeros(n_cand, np.int64), C.c_int(0), C.c_int(0)
        self.lib.ref_kfdb_nbest(self.h, kid, len(wid), _p(wid), _p(wval), m, len(conn), _p(conn), n_cand, _p(lo), C.byref(nl), _p(me), C.byref(nm))
        return (lo[:nl.value].tolist(), me[:nm.value].tolist()), self._stamps(1, kid)


class RestatementBackend:
    def __init__(self, n_vocab):
        self.db = kfdb_ref.Database(n_vocab)

    def close(self):
        pass

    def add(self, kf, m, wid, wval):
        self.db.add(kf, m, wid, wval)

    def erase(self, kf):
        self.db.erase(kf)

    def clear_map(self, m):
        self.db.clearMap(m)

    def set_map(self, kf, m):
        self.db.objects[kf].map = m

    def set_covisibility(self, covis, kf_map):
        self.db.set_covisibility(covis)

    def _stamps(self, which, qid):
        Q, W, S = (("mnRelocQuery", "mnRelocWords", "mRelocScore"), ("mnPlaceRecognitionQuery", "mnPlaceRecognitionWords", "mPlaceRecognitionScore"))[which]
        kfs = [kf for _, kf in sorted(self.db.objects.items()) if getattr(kf, Q) == qid]
        return (np.array([kf.mnId for kf in kfs], np.int64), np.array([getattr(kf, W) for kf in kfs], np.int32),
                np.array([getattr(kf, S) for kf in kfs], np.float32))

    def reloc(self, fid, wid, wval, m):
        return self.db.DetectRelocalizationCandidates(fid, wid, wval, m), self._stamps(0, fid)

    def reloc_order(self, fid, wid, wval):
        return order_of(self.db.sharing(fid, wid, wval, which="reloc"))

    def nbest(self, kid, wid, wval, m, conn, n_cand, bad_maps=()):
        lo, me = self.db.DetectNBestCandidates(kid, wid, wval, m, conn, n_cand, bad_maps=bad_maps)
        return (lo, me), self._stamps(1, kid)


class DeviceBackend:
    """frontend.KeyFrameDatabase on the library handed in (the emulator build or the product)."""

    def __init__(self, n_vocab, lib):
        self.db = F.KeyFrameDatabase(n_vocab, lib=lib)

    def close(self):
        self.db.close()

    def add(self, kf, m, wid, wval):
        self.db.add(kf, m, wid, wval)

    def erase(self, kf):
        self.db.erase(kf)

    def clear_map(self, m):
        self.db.clearMap(m)

    def set_map(self, kf, m):
        self.db.setMap(kf, m)
        self.kf_map[kf] = m

    def set_covisibility(self, covis, kf_map):
        self.covis, self.kf_map = covis, dict(kf_map)

    def _stamps(self, which, qid):
        rows = sorted((kf, e[1], e[2]) for kf, e in self.db.stamps[which].items() if e[0] == qid)
        return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.float32))

    def reloc(self, fid, wid, wval, m):
        return self.db.DetectRelocalizationCandidates(fid, wid, wval, m, self.covis, self.kf_map), self._stamps("reloc", fid)

    def reloc_order(self, fid, wid, wval):
        r = self.db.query(wid, wval)
        self.db._stamp("reloc", fid, r)
        return order_of(r)

    def nbest(self, kid, wid, wval, m, conn, n_cand, bad_maps=()):
        lo, me = self.db.DetectNBestCandidates(kid, wid, wval, m, conn, n_cand, self.covis, self.kf_map, bad_maps=bad_maps)
        return (lo, me), self._stamps("place", kid)


def order_of(r):
    """What `reloc_order` returns, from a query result in lKFsSharingWords order: the scored key frames whose score is above
    0.75 x the best score, in that order (DetectRelocalizationCandidates without covisibility lists and map filter)."""
    sc = [(np.float32(s), int(k)) for k, s, ok in zip(r["kf"], r["score"], r["scored"]) if ok]
    best = max([s for s, _ in sc] + [np.float32(0)])
    keep = np.float32(np.float32(0.75) * best)
    return [k for s, k in sc if s > keep]


def _record(stamps):
    ids, words, score = stamps
    mx = int(words.max()) if len(words) else 0
    minc = int(np.float32(mx) * np.float32(0.8))
    scored = words > minc
    return dict(kf=ids.tolist(), words=words.tolist(), scored=scored.astype(int).tolist(),
                score_bits=score.view(np.uint32)[scored].tolist())


def run_case(name, make_backend, n_queries=4):
    """The case's script on a back end; returns the JSON-able record the fixtures hold."""
    p = CASES[name]
    db = kc.make_database(p["n_kf"], p["n_words"], p["n_vocab"], seed=p["seed"], n_maps=p["n_maps"])
    ent = db["entries"]
    covis = kc.covisibility(db, seed=p["seed"])
    kf_map = {e["kf_id"]: e["map_id"] for e in ent}
    be = make_backend(p["n_vocab"])
    for e in ent:
        be.add(e["kf_id"], e["map_id"], e["word_id"], e["word_val"])
    for i in range(3, len(ent), 7):                      # erase every 7th ...
        be.erase(ent[i]["kf_id"])
    for i in range(3, len(ent), 14):                     # ... and bring every other one of them back: they go to the end
        be.add(ent[i]["kf_id"], ent[i]["map_id"], ent[i]["word_id"], ent[i]["word_val"])
    be.set_covisibility(covis, kf_map)
    if p.get("script") == "map_change":
        for i in range(10, 25):                          # these were added as map 0 ...
            ent[i]["map_id"] = 1
            be.set_map(ent[i]["kf_id"], 1)
        be.clear_map(0)                                  # ... and must survive the clearing of map 0
    queries = []
    for k in range(n_queries):
        place = (23 * k + 1) % db["n_places"]
        wid, wval = kc.make_query(db, place, seed=p["seed"] + k)
        m = ent[place]["map_id"] if k % 2 == 0 else p["n_maps"] - 1      # the place's own map / the last map
        cand, st = be.reloc(100 + k, wid, wval, m)
        queries.append(dict(kind="reloc", place=place, map=m, candidates=[int(c) for c in cand], **_record(st)))
        # the order of lKFsSharingWords itself, as far as the reference's function shows it: no covisibility lists, every key
        # frame in the query's map - the candidates are then the scored key frames above 0.75 x best, in list order
        queries.append(dict(kind="order", place=place, order=[int(c) for c in be.reloc_order(700 + k, wid, wval)]))
        # a key frame in the middle of the trajectory, then one of the stretch that drives through the first places again
        i = (31 * k + 20) % db["n_places"] if k % 2 == 0 else db["n_places"] + (5 * k) % (len(ent) - db["n_places"])
        if (i - 3) % 7 == 0:
            i += 1                                       # entry i was erased or moved: take its neighbour
        e = ent[i]
        conn = kc.connected(db, i) | {e["kf_id"]}
        (lo, me), st = be.nbest(500 + k, e["word_id"], e["word_val"], e["map_id"], conn, 3)
        queries.append(dict(kind="nbest", entry=i, loop=[int(c) for c in lo], merge=[int(c) for c in me], **_record(st)))
    if p.get("script") == "map_change":
        be.clear_map(1)                                  # now everything is gone
        wid, wval = kc.make_query(db, 1, seed=p["seed"])
        cand, st = be.reloc(900, wid, wval, 1)
        queries.append(dict(kind="reloc", place=1, map=1, candidates=[int(c) for c in cand], **_record(st)))
    be.close()
    return dict(case=name, params=p, queries=queries)


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def assert_matches_golden(name, make_backend):
    got, exp = run_case(name, make_backend), load(name)
    assert got["params"] == exp["params"]
    assert len(got["queries"]) == len(exp["queries"])
    n_scored = 0
    for k, (g, e) in enumerate(zip(got["queries"], exp["queries"])):
        for key in e:
            assert g[key] == e[key], (name, k, e["kind"], key)
        n_scored += len(e.get("score_bits", ()))
    assert n_scored > 0
    return n_scored


if __name__ == "__main__":
    os.makedirs(GOLDEN, exist_ok=True)
    for name in CASES:
        rec = run_case(name, ReferenceBackend)
        with open(os.path.join(GOLDEN, name + ".json"), "w") as f:
            json.dump(rec, f, separators=(",", ":"))
            f.write("\n")
        print(name, sum(len(q.get("kf", ())) for q in rec["queries"]), "stamped,", sum(len(q.get("score_bits", ())) for q in rec["queries"]), "scored,",
              [q["candidates"] if q["kind"] == "reloc" else q["order"] if q["kind"] == "order" else (q["loop"], q["merge"]) for q in rec["queries"]])
