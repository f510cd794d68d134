"""KeyFrameDatabase checks shared by the emulator tests (tests/test_kfdb_emu.py) and the MI355X tests (tests/test_kfdb_gpu.py).

Every comparison is exact: ids, counts and order element-wise, scores as uint32 views.  The expected values come from
tests/kfdb_ref.py, the restatement of the reference's inverted file.
"""
import ctypes as C
import threading

import numpy as np

import kfdb_ref
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import kfdb_cases as kc
from orb_slam3_rgbl_amd import synth


def assert_same(got, exp, what=""):
    """One query result against the restatement's."""
    assert got["max_common_words"] == exp["max_common_words"], (what, got["max_common_words"], exp["max_common_words"])
    assert got["min_common_words"] == exp["min_common_words"], (what, got["min_common_words"], exp["min_common_words"])
    assert np.array_equal(got["kf"], exp["kf"]), (what, "lKFsSharingWords", got["kf"][:8], exp["kf"][:8])
    assert np.array_equal(got["words"], exp["words"]), (what, "common words")
    assert np.array_equal(got["scored"], exp["scored"]), (what, "scored")
    s = exp["scored"]
    assert np.array_equal(got["score"][s].view(np.uint32), exp["score"][s].view(np.uint32)), (what, "scores")


def both(lib, n_vocab):
    return F.KeyFrameDatabase(n_vocab, lib=lib), kfdb_ref.Database(n_vocab)


def add_both(dev, ref, e):
    dev.add(e["kf_id"], e["map_id"], e["word_id"], e["word_val"])
    ref.add(e["kf_id"], e["map_id"], e["word_id"], e["word_val"])


def fill(lib, db):
    dev, ref = both(lib, db["n_vocab"])
    for e in db["entries"]:
        add_both(dev, ref, e)
    return dev, ref


class Ids:
    """Fresh query ids (Frame::mnId / KeyFrame::mnId never repeat)."""
    n = 0

    @classmethod
    def next(cls):
        cls.n += 1
        return cls.n


def check_query_sizes(lib, sizes=(1, 2, 63, 300, 2000), n_words=40, n_vocab=4000, places=(0, 3)):
    """Queries against the restatement on databases of 1 .. 2000 entries."""
    total = 0
    for n in sizes:
        db = kc.make_database(n, n_words, n_vocab, seed=n)
        dev, ref = fill(lib, db)
        assert dev.size() == (n, sum(len(e["word_id"]) for e in db["entries"]))
        for p in places:
            wid, wval = kc.make_query(db, p, seed=n)
            got = dev.query(wid, wval)
            exp = ref.sharing(Ids.next(), wid, wval)
            assert_same(got, exp, "n=%d place=%d" % (n, p))
            total += int(exp["scored"].sum())
        dev.close()
    assert total > 0
    return total


def check_empty_and_disjoint(lib):
    dev, ref = both(lib, 1000)
    wid, wval = np.array([1, 5, 9], np.uint32), np.array([0.2, 0.3, 0.5])
    r = dev.query(wid, wval)
    assert len(r["kf"]) == 0 and r["max_common_words"] == 0 and r["min_common_words"] == 0      # empty database
    add_both(dev, ref, dict(kf_id=1, map_id=0, word_id=np.array([2, 6, 10], np.uint32), word_val=np.array([0.5, 0.25, 0.25])))
    add_both(dev, ref, dict(kf_id=2, map_id=0, word_id=np.zeros(0, np.uint32), word_val=np.zeros(0)))   # a key frame without words
    r = dev.query(wid, wval)
    assert len(r["kf"]) == 0 and r["max_common_words"] == 0                                      # shares nothing
    assert_same(r, ref.sharing(Ids.next(), wid, wval))
    r = dev.query(np.zeros(0, np.uint32), np.zeros(0))                                           # a query without words
    assert len(r["kf"]) == 0
    dev.close()


def _norm(v):
    v = np.asarray(v, np.float64)
    return v / v.sum()


def check_ties_and_threshold(lib):
    """Ties at the maximum; a count exactly equal to minCommonWords is not scored (strict >); the floor."""
    dev, ref = both(lib, 1000)
    q = np.arange(0, 40, 2, dtype=np.uint32)                   # 20 words: 0, 2, .. 38
    qv = _norm(np.arange(1, 21))
    rng = np.random.default_rng(5)

    def entry(kf, common, first=0):
        ids = np.concatenate([q[first:first + common], np.arange(101 + 50 * kf, 101 + 50 * kf + 7, dtype=np.uint32)])
        return dict(kf_id=kf, map_id=0, word_id=np.sort(ids).astype(np.uint32), word_val=_norm(rng.uniform(1, 2, len(ids))))
    # max = 10 -> minCommonWords = int(10 * 0.8f) = 8: 8 common words are NOT scored, 9 are
    for e in (entry(1, 10), entry(2, 10, first=3), entry(3, 8), entry(4, 9, first=1), entry(5, 1, first=19), entry(6, 10)):
        add_both(dev, ref, e)
    got, exp = dev.query(q, qv), ref.sharing(Ids.next(), q, qv)
    assert_same(got, exp, "ties")
    assert got["max_common_words"] == 10 and got["min_common_words"] == 8
    by = dict(zip(got["kf"].tolist(), got["scored"].tolist()))
    assert by == {1: True, 2: True, 3: False, 4: True, 5: False, 6: True}
    assert got["kf"].tolist() == [1, 3, 6, 4, 2, 5]            # first common word 0, 0, 0, then 2, then 6, then 38
    # the floor raises minCommonWords
    got, exp = dev.query(q, qv, min_words_floor=9), ref.sharing(Ids.next(), q, qv, min_words_floor=9)
    assert_same(got, exp, "floor")
    assert got["min_common_words"] == 9 and dict(zip(got["kf"].tolist(), got["scored"].tolist()))[4] is False
    # thresholds where the float product truncates: max = 6 -> int(4.8f) = 4, max = 5 -> int(4.0f) = 4
    for mx in (5, 6, 7, 15):
        dev.clear()
        ref.clear()
        for kf, c in enumerate(range(1, mx + 1)):
            add_both(dev, ref, entry(kf + 1, c))
        assert_same(dev.query(q, qv), ref.sharing(Ids.next(), q, qv), "max=%d" % mx)
    dev.close()


def check_excluded(lib, n=120):
    db = kc.make_database(n, 40, 3000, seed=3)
    dev, ref = fill(lib, db)
    hits = 0
    for i in (n - 1, n // 2, 5):
        e = db["entries"][i]
        conn = kc.connected(db, i) | {e["kf_id"], 999999}       # the key frame itself and one that is not stored
        got = dev.query(e["word_id"], e["word_val"], excluded=conn)
        exp = ref.sharing(Ids.next(), e["word_id"], e["word_val"], excluded=conn)
        assert_same(got, exp, "excluded %d" % i)
        assert not (set(got["kf"].tolist()) & conn)
        free = dev.query(e["word_id"], e["word_val"])
        hits += len(free["kf"]) - len(got["kf"])
        assert free["max_common_words"] == len(e["word_id"])     # unexcluded, the key frame finds itself
    assert hits > 0
    dev.close()


def run_script(lib, db, ops):
    """A mutation script on both; every query is compared.  Returns the number of queries."""
    dev, ref = both(lib, db["n_vocab"])
    nq = 0
    for k, (op, a) in enumerate(ops):
        if op == "add":
            add_both(dev, ref, db["entries"][a])
        elif op == "erase":
            dev.erase(db["entries"][a]["kf_id"])
            ref.erase(db["entries"][a]["kf_id"])
        elif op == "clear_map":
            dev.clearMap(a)
            ref.clearMap(a)
        else:
            wid, wval = kc.make_query(db, a, seed=k)
            assert_same(dev.query(wid, wval), ref.sharing(Ids.next(), wid, wval), "op %d" % k)
            nq += 1
        assert dev.size()[0] == len(ref.kfs)
    info = dev.arena_info()
    dev.close()
    return nq, info


def check_mutation_order(lib):
    """Erase, re-add (goes to the end of the order) and clearMap."""
    db = kc.make_database(60, 30, 1500, seed=9, n_maps=3)
    nq, _ = run_script(lib, db, kc.mutation_script(db, seed=1, n_ops=80))
    assert nq > 10
    # the order itself: three key frames sharing one word
    dev, ref = both(lib, 100)
    for kf in (5, 3, 9):
        add_both(dev, ref, dict(kf_id=kf, map_id=kf % 2, word_id=np.array([7, 50 + kf], np.uint32), word_val=np.array([0.5, 0.5])))
    q, qv = np.array([7], np.uint32), np.array([1.0])
    assert dev.query(q, qv)["kf"].tolist() == [5, 3, 9]
    dev.erase(5)
    ref.erase(5)
    add_both(dev, ref, dict(kf_id=5, map_id=1, word_id=np.array([7, 55], np.uint32), word_val=np.array([0.5, 0.5])))
    assert dev.query(q, qv)["kf"].tolist() == [3, 9, 5]
    assert_same(dev.query(q, qv), ref.sharing(Ids.next(), q, qv))
    dev.clearMap(1)
    ref.clearMap(1)
    assert_same(dev.query(q, qv), ref.sharing(Ids.next(), q, qv))
    assert dev.query(q, qv)["kf"].tolist() == []
    dev.erase(12345)                                              # not stored: nothing happens
    dev.clear()
    assert dev.size() == (0, 0)
    dev.close()


def check_compaction(lib, n=80):
    """Compaction forced between two identical queries: junk key frames over words the query does not have are erased until
    more than half of the arena is dead."""
    db = kc.make_database(n, 40, 2000, seed=4)
    dev, ref = both(lib, 4000)
    junk = []
    rng = np.random.default_rng(8)
    for i, e in enumerate(db["entries"]):
        add_both(dev, ref, e)
        ids = np.unique(rng.integers(2000, 4000, 90)).astype(np.uint32)      # words no query holds
        j = dict(kf_id=50000 + i, map_id=0, word_id=ids, word_val=_norm(np.ones(len(ids))))
        add_both(dev, ref, j)
        junk.append(j["kf_id"])
    wid, wval = kc.make_query(db, 2, seed=1)
    before = dev.query(wid, wval)
    i0 = dev.arena_info()
    assert i0["n_compactions"] == 0
    for k, kf in enumerate(junk):
        dev.erase(kf)
        ref.erase(kf)
        if k == len(junk) // 3:
            assert dev.arena_info()["n_compactions"] == 0
            assert_same(dev.query(wid, wval), before, "tombstones")       # tombstones in the arena
    i1 = dev.arena_info()
    assert i1["n_compactions"] >= 1 and i1["used_words"] < i0["used_words"] and i1["n_slots"] < i0["n_slots"]
    after = dev.query(wid, wval)
    assert_same(after, before, "compaction")
    assert_same(after, ref.sharing(Ids.next(), wid, wval), "compaction vs restatement")
    assert len(after["kf"]) > 0 and after["scored"].any()
    # adds after a compaction land behind the survivors
    add_both(dev, ref, dict(kf_id=77777, map_id=0, word_id=wid, word_val=wval))
    got = dev.query(wid, wval)
    assert_same(got, ref.sharing(Ids.next(), wid, wval), "add after compaction")
    assert got["max_common_words"] == len(wid)
    dev.close()


def check_arena_growth(lib, n=60, n_words=1500):
    """More words than the first arena holds: it doubles and the stored vectors move along."""
    db = kc.make_database(n, n_words, 200000, seed=6)
    dev, ref = both(lib, db["n_vocab"])
    cap0 = dev.arena_info()["cap_words"]
    for e in db["entries"]:
        add_both(dev, ref, e)
    info = dev.arena_info()
    assert info["used_words"] > cap0 and info["cap_words"] >= info["used_words"] and info["cap_words"] > cap0
    for p in (0, n // 2):
        wid, wval = kc.make_query(db, p, seed=2)
        assert_same(dev.query(wid, wval), ref.sharing(Ids.next(), wid, wval), "grown arena, place %d" % p)
    dev.close()


def check_batch(lib, n=150, Q=5):
    """rgbl_kfdb_query_batch = Q single queries (with and without excluded sets and floors)."""
    db = kc.make_database(n, 40, 3000, seed=12)
    dev, ref = fill(lib, db)
    queries = []
    for k in range(Q):
        wid, wval = kc.make_query(db, 11 * k, seed=k, n_words=20 + 15 * k)
        queries.append(dict(word_id=wid, word_val=wval, excluded=kc.connected(db, 11 * k) if k % 2 else None, min_words_floor=3 * (k == 2)))
    queries.append(dict(word_id=np.zeros(0, np.uint32), word_val=np.zeros(0)))      # an empty query inside a batch
    got = dev.query_batch(queries)
    for k, q in enumerate(queries):
        single = dev.query(q["word_id"], q["word_val"], excluded=q.get("excluded"), min_words_floor=q.get("min_words_floor", 0))
        assert_same(got[k], single, "batch row %d" % k)
        assert_same(got[k], ref.sharing(Ids.next(), q["word_id"], q["word_val"], excluded=q.get("excluded") or (),
                                        min_words_floor=q.get("min_words_floor", 0)), "batch row %d vs restatement" % k)
    assert sum(len(g["kf"]) for g in got) > 0
    dev.close()


def check_errors(lib):
    h = C.c_void_p()
    assert lib.rgbl_kfdb_create(0, 0, C.byref(h)) == L.ERR_INVALID
    assert lib.rgbl_kfdb_create(99, 10, C.byref(h)) == L.ERR_INVALID
    assert lib.rgbl_kfdb_create(0, 10, None) == L.ERR_INVALID
    dev = F.KeyFrameDatabase(100, lib=lib)
    ids, val = np.array([1, 5, 9], np.uint32), np.array([0.2, 0.3, 0.5])
    dev.add(1, 0, ids, val)
    for bad in (np.array([1, 9, 5], np.uint32), np.array([1, 5, 5], np.uint32), np.array([1, 5, 100], np.uint32)):
        assert lib.rgbl_kfdb_add(dev.h, 2, 0, 3, L.ptr(bad), L.ptr(val)) == L.ERR_INVALID      # not ascending / beyond the vocabulary
    assert lib.rgbl_kfdb_add(dev.h, 1, 0, 3, L.ptr(ids), L.ptr(val)) == L.ERR_INVALID          # a live key frame a second time
    assert b"already" in lib.rgbl_last_error()
    assert lib.rgbl_kfdb_add(dev.h, 2, 0, 3, None, L.ptr(val)) == L.ERR_INVALID
    assert lib.rgbl_kfdb_add(None, 2, 0, 3, L.ptr(ids), L.ptr(val)) == L.ERR_INVALID
    assert lib.rgbl_kfdb_erase(None, 1) == L.ERR_INVALID and lib.rgbl_kfdb_query(dev.h, None, None) == L.ERR_INVALID
    assert dev.size() == (1, 3)
    for k in range(2, 6):
        dev.add(k, 0, ids, val)
    # room for fewer key frames than share a word: reported, count returned
    kf, words, score, scored = np.zeros(2, np.int64), np.zeros(2, np.int32), np.full(2, 7.0, np.float32), np.zeros(2, np.uint8)
    qin = L.KfdbQueryInput(3, L.ptr(ids).value, L.ptr(val).value, 0, None, 0)
    out = L.KfdbQueryOutput(2, L.ptr(kf).value, L.ptr(words).value, L.ptr(score).value, L.ptr(scored).value, 0, 0, 0)
    assert lib.rgbl_kfdb_query(dev.h, C.byref(qin), C.byref(out)) == L.ERR_CAPACITY and out.n_share == 5
    bad = np.array([5, 1], np.uint32)
    qin = L.KfdbQueryInput(2, L.ptr(bad).value, L.ptr(val).value, 0, None, 0)
    assert lib.rgbl_kfdb_query(dev.h, C.byref(qin), C.byref(out)) == L.ERR_INVALID
    # the score slot of an unscored key frame is not written
    dev.add(9, 0, np.array([1, 50, 51, 52], np.uint32), np.array([0.25, 0.25, 0.25, 0.25]))
    kf, words, score, scored = np.zeros(8, np.int64), np.zeros(8, np.int32), np.full(8, 7.0, np.float32), np.zeros(8, np.uint8)
    qin = L.KfdbQueryInput(3, L.ptr(ids).value, L.ptr(val).value, 0, None, 0)
    out = L.KfdbQueryOutput(8, L.ptr(kf).value, L.ptr(words).value, L.ptr(score).value, L.ptr(scored).value, 0, 0, 0)
    assert lib.rgbl_kfdb_query(dev.h, C.byref(qin), C.byref(out)) == L.RGBL_OK and out.n_share == 6
    assert kf[5] == 9 and scored[5] == 0 and score[5] == 7.0 and scored[:5].all()
    assert np.array_equal(score[:5].view(np.uint32), np.full(5, 1.0, np.float32).view(np.uint32))   # identical vectors score 1
    dev.close()


def check_detect(lib, n=160, n_queries=6):
    """Both Detect* mirrors end to end against the restatement, with persistent stamps across queries."""
    db = kc.make_database(n, 50, 3000, seed=21, n_maps=3)
    dev, ref = fill(lib, db)
    covis = kc.covisibility(db, seed=2)
    ref.set_covisibility(covis)
    kf_map = {e["kf_id"]: e["map_id"] for e in db["entries"]}
    n_cand = 0
    for k in range(n_queries):
        place = (17 * k) % db["n_places"]
        wid, wval = kc.make_query(db, place, seed=40 + k)
        fid = Ids.next()
        for m in (0, 2):
            fid = Ids.next()
            got = dev.DetectRelocalizationCandidates(fid, wid, wval, m, covis, kf_map)
            exp = ref.DetectRelocalizationCandidates(fid, wid, wval, m)
            assert got == exp, ("reloc", k, m, got, exp)
            n_cand += len(got)
        i = (29 * k + n - 1) % n
        e = db["entries"][i]
        kid = Ids.next()
        conn = kc.connected(db, i) | {e["kf_id"]}
        got = dev.DetectNBestCandidates(kid, e["word_id"], e["word_val"], e["map_id"], conn, 3, covis, kf_map, bad_maps={1})
        exp = ref.DetectNBestCandidates(kid, e["word_id"], e["word_val"], e["map_id"], conn, 3, bad_maps={1})
        assert got == exp, ("nbest", k, got, exp)
        n_cand += len(got[0]) + len(got[1])
    assert n_cand > 0
    dev.close()
    return n_cand


def check_vocabulary_end_to_end(lib):
    """Descriptors -> rgbl_bow_transform -> database -> query: the whole BoW path on the device."""
    voc = synth.make_vocabulary(6, 3, 1)
    V = F.ORBVocabulary(lib=lib).from_arrays(synth.vocabulary_arrays(voc))
    n_vocab = V.info()["n_words"]
    dev, ref = both(lib, n_vocab)
    base = synth.descriptors(300, 7)
    for k in range(12):
        desc = np.concatenate([synth.perturbed_descriptors(base[20 * k:20 * k + 120], 0.03, seed=k)[0], synth.descriptors(40, 100 + k)])
        wid, wval = V.transform(desc)[:2]
        add_both(dev, ref, dict(kf_id=k, map_id=0, word_id=wid, word_val=wval))
    wid, wval = V.transform(synth.perturbed_descriptors(base[60:200], 0.03, seed=99)[0])[:2]
    got = dev.query(wid, wval)
    assert_same(got, ref.sharing(Ids.next(), wid, wval), "vocabulary")
    assert len(got["kf"]) > 3 and got["scored"].any()
    dev.close()
    V.close()


def check_threads(lib, n=40, rounds=12):
    """add / erase from one thread, queries from two others (the reference's mMutex).  The mutator toggles key frame X,
    which shares every word with the query, and a few key frames over words no query holds.  Whatever the interleaving, a
    query sees the database either with X or without it: it must equal one of those two serial results, whole - ids,
    order, counts, threshold and scores (X moves the maximum, so a torn view would score the wrong set)."""
    db = kc.make_database(n, 30, 1500, seed=33)
    dev, ref = both(lib, 3000)
    for e in db["entries"]:
        add_both(dev, ref, e)
    wid, wval = kc.make_query(db, 4, seed=3)
    X = dict(kf_id=88888, map_id=0, word_id=wid, word_val=wval)
    without = ref.sharing(Ids.next(), wid, wval)
    ref.add(X["kf_id"], 0, wid, wval)
    with_x = ref.sharing(Ids.next(), wid, wval)
    ref.erase(X["kf_id"])
    assert with_x["max_common_words"] == len(wid) > without["max_common_words"]
    assert not np.array_equal(with_x["scored"][:-1], without["scored"]) or len(with_x["kf"]) != len(without["kf"])
    errors, seen = [], set()

    def mutate():
        try:
            rng = np.random.default_rng(1)
            for r in range(rounds):
                ids = np.unique(rng.integers(1500, 3000, 200)).astype(np.uint32)
                dev.add(X["kf_id"], 0, wid, wval)
                for k in range(4):
                    dev.add(90000 + k, 0, ids, _norm(np.ones(len(ids))))
                dev.erase(X["kf_id"])
                for k in range(4):
                    dev.erase(90000 + k)
        except Exception as ex:   # noqa: BLE001
            errors.append(ex)

    def ask():
        try:
            for r in range(2 * rounds):
                got = dev.query(wid, wval, cap=n + 16)
                which = "with" if got["max_common_words"] == len(wid) else "without"
                assert_same(got, with_x if which == "with" else without, "threaded query %d (%s X)" % (r, which))
                seen.add(which)
        except Exception as ex:   # noqa: BLE001
            errors.append(ex)

    ts = [threading.Thread(target=mutate), threading.Thread(target=ask), threading.Thread(target=ask)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert_same(dev.query(wid, wval), without, "after the threads")
    dev.add(X["kf_id"], 0, wid, wval)
    assert_same(dev.query(wid, wval), with_x, "with X")
    assert dev.size()[0] == n + 1
    dev.close()
