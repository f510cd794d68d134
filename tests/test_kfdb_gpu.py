"""KeyFrameDatabase on a real MI355X: the checks of tests/kfdb_checks.py on the product library, the fixtures recorded from the
reference's own code (tests/golden/kfdb), and one database of KITTI-00 size."""
import numpy as np
import pytest

import kfdb_checks as kc
import kfdb_golden as kg
import kfdb_ref
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import kfdb_cases

pytestmark = pytest.mark.gpu


def test_query_against_restatement_1_to_2000_entries(gpu_lib):
    kc.check_query_sizes(gpu_lib, n_words=120, n_vocab=20000)


def test_empty_database_and_disjoint_query(gpu_lib):
    kc.check_empty_and_disjoint(gpu_lib)


def test_ties_strict_threshold_and_floor(gpu_lib):
    kc.check_ties_and_threshold(gpu_lib)


def test_excluded_sets(gpu_lib):
    kc.check_excluded(gpu_lib)


def test_erase_readd_clear_map_order(gpu_lib):
    kc.check_mutation_order(gpu_lib)


def test_compaction_changes_no_result(gpu_lib):
    kc.check_compaction(gpu_lib)


def test_arena_growth(gpu_lib):
    kc.check_arena_growth(gpu_lib)


def test_batch_equals_single_queries(gpu_lib):
    kc.check_batch(gpu_lib, n=400, Q=16)


def test_error_returns(gpu_lib):
    kc.check_errors(gpu_lib)


def test_detect_mirrors_end_to_end(gpu_lib):
    kc.check_detect(gpu_lib)


def test_vocabulary_to_candidates(gpu_lib):
    kc.check_vocabulary_end_to_end(gpu_lib)


def test_threaded_add_erase_query(gpu_lib):
    kc.check_threads(gpu_lib)


@pytest.mark.parametrize("name", sorted(kg.CASES))
def test_golden_fixtures(gpu_lib, name):
    assert kg.assert_matches_golden(name, lambda n_vocab: kg.DeviceBackend(n_vocab, gpu_lib)) > 10


def test_kitti00_sized_database(gpu_lib):
    """1 500 key frames of about 1 800 words over a 10^6-word vocabulary: single queries, an excluded set, a batch of 16."""
    db = kfdb_cases.make_database(1500, 1800, 1000000, seed=77, n_maps=2)
    dev, ref = F.KeyFrameDatabase(db["n_vocab"], lib=gpu_lib), kfdb_ref.Database(db["n_vocab"])
    for e in db["entries"]:
        kc.add_both(dev, ref, e)
    n_alive, n_words = dev.size()
    assert n_alive == 1500 and 1500 * 1600 < n_words < 1500 * 1900
    queries = []
    for k, place in enumerate((0, 400, 1199, 37)):
        wid, wval = kfdb_cases.make_query(db, place, seed=k)
        got, exp = dev.query(wid, wval), ref.sharing(kc.Ids.next(), wid, wval)
        kc.assert_same(got, exp, "place %d" % place)
        assert exp["scored"].sum() >= 1 and len(exp["kf"]) > 10
        queries.append(dict(word_id=wid, word_val=wval))
    e = db["entries"][1400]                                   # a key frame of the stretch that revisits the start
    conn = kfdb_cases.connected(db, 1400) | {e["kf_id"]}
    kc.assert_same(dev.query(e["word_id"], e["word_val"], excluded=conn), ref.sharing(kc.Ids.next(), e["word_id"], e["word_val"], excluded=conn), "nbest")
    queries += [dict(word_id=db["entries"][i]["word_id"], word_val=db["entries"][i]["word_val"], excluded=kfdb_cases.connected(db, i))
                for i in range(20, 1500, 125)]
    queries = queries[:16]
    for k, got in enumerate(dev.query_batch(queries)):
        q = queries[k]
        kc.assert_same(got, ref.sharing(kc.Ids.next(), q["word_id"], q["word_val"], excluded=q.get("excluded") or ()), "batch row %d" % k)
    dev.close()
