"""KeyFrameDatabase: the restatement (tests/kfdb_ref.py) against the reference's own KeyFrameDatabase.cc and DBoW2 scoring, and
everything against the fixtures under tests/golden/kfdb that the reference's own code produced (tests/kfdb_golden.py)."""
import pytest

import kfdb_golden as kg


@pytest.mark.parametrize("name", sorted(kg.CASES))
def test_restatement_matches_golden(name):
    assert kg.assert_matches_golden(name, kg.RestatementBackend) > 10


@pytest.mark.parametrize("name", sorted(kg.CASES))
def test_emulated_kernels_match_golden(emu_lib, name):
    assert kg.assert_matches_golden(name, lambda n_vocab: kg.DeviceBackend(n_vocab, emu_lib)) > 10


@pytest.mark.skipif(not kg.have_reference(), reason="the reference sources are not on this machine")
@pytest.mark.parametrize("name", sorted(kg.CASES))
def test_reference_code_reproduces_golden(name):
    """The committed fixtures are what src/KeyFrameDatabase.cc + ScoringObject.cpp, compiled unmodified, return."""
    lib = kg.build_reference_glue()
    kg.assert_matches_golden(name, lambda n_vocab: kg.ReferenceBackend(n_vocab, lib))


@pytest.mark.skipif(not kg.have_reference(), reason="the reference sources are not on this machine")
def test_restatement_equals_reference_code_on_fresh_cases(monkeypatch):
    """Beyond the three fixtures: other seeds and sizes, restatement and reference side by side."""
    lib = kg.build_reference_glue()
    fresh = {"a": dict(n_kf=60, n_words=25, n_vocab=600, seed=7, n_maps=2), "b": dict(n_kf=200, n_words=80, n_vocab=8000, seed=8, n_maps=4),
             "c": dict(n_kf=40, n_words=300, n_vocab=2500, seed=9, n_maps=1)}
    monkeypatch.setattr(kg, "CASES", fresh)
    n = 0
    for name in fresh:
        ref = kg.run_case(name, lambda n_vocab: kg.ReferenceBackend(n_vocab, lib), n_queries=6)
        mine = kg.run_case(name, kg.RestatementBackend, n_queries=6)
        assert mine == ref, name
        n += sum(len(q.get("score_bits", ())) for q in ref["queries"])
    assert n > 30
