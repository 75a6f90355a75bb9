"""The restatement of the k-mer correction (tests/kcorrect_reference.py) against
what the reference did (tests/golden/golden_correct.json, made by
tests/golden/make_golden_correct.py), and every rule of it broken once: some
golden or generated set must notice.  No GPU."""
import json
import os

import numpy as np
import pytest

import kcorrect_reference as kr
import oracle_util as ou

GOLDEN = os.path.join(ou.GOLDEN_DIR, "golden_correct.json")
FASTA = os.path.join(ou.GOLDEN_DIR, "correct")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def decoded(strings):
    return [np.array(["acgt".index(ch) for ch in s], dtype=np.uint8) for s in strings]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


NAMES = ("errors_1", "planted", "clean", "c1", "k_is_length", "k_above_length", "k1", "none_trusted", "live", "chain",
         "conflict", "group_once")


def test_the_golden_sets_are_those_named_here(golden):
    assert sorted(golden["sets"]) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_golden_call(golden, name):
    e = golden["sets"][name]
    reads = kr.parse_fasta(os.path.join(FASTA, e["file"]))
    assert len(reads) == e["reads"]
    got, triples, info = kr.correct_reads(reads, e["k"], e["c"])
    assert same(got, decoded(e["first"]["reads"]))
    assert info["records"] == e["first"]["records"] == len(triples) and info["changed"] == e["first"]["changed"]
    assert e["first"]["stdout"] == "" and e["first"]["exit"] == 0
    assert (e["first"]["esq"] == e["esq_before"]) == (info["changed"] == 0)


def test_errors_1_is_the_reference_s_own_pair_of_files():
    reads = kr.parse_fasta(os.path.join(FASTA, "errors_1.fas"))
    want = kr.parse_fasta(os.path.join(FASTA, "errors_1.corrected.fas"))
    got, triples, info = kr.correct_reads(reads, 12, 2)
    assert same(got, want) and info["records"] == 1 and info["changed"] == 1


def test_the_order_sets_have_their_property(golden):
    sets = golden["sets"]
    assert sets["live"]["first"]["chain"] == 1 and sets["chain"]["first"]["chain"] >= 2
    assert sets["conflict"]["first"]["conflicts"] >= 1
    for name in ("live", "chain"):
        e = sets[name]
        reads = kr.parse_fasta(os.path.join(FASTA, e["file"]))
        assert not same(kr.correct_reads(reads, e["k"], e["c"], original_sources=True)[0], decoded(e["first"]["reads"]))
    for name in ("clean", "c1", "k_is_length", "k_above_length", "k1", "none_trusted"):
        assert sets[name]["first"]["records"] == 0


def test_the_refusal_is_recorded_with_its_sentence(golden):
    e = golden["refusals"]["two_lengths"]
    assert e["exit"] != 0 and e["stdout"] == ""
    assert e["message"] == "twobitencoding correction is currently only implemented if the sequence access type is EQUALLENGTH"
    assert len({r.size for r in kr.parse_fasta(os.path.join(FASTA, e["file"]))}) == 2


def _generated():
    return [kr.width_reads(), kr.invalid_tail_reads(8), kr.mixed_reads()]


@pytest.mark.parametrize("rule", kr.RULES)
def test_every_rule_is_noticed_when_broken(golden, rule):
    noticed = []
    for name in NAMES:
        e = golden["sets"][name]
        reads = kr.parse_fasta(os.path.join(FASTA, e["file"]))
        if not same(kr.correct_reads(reads, e["k"], e["c"], broken=(rule,))[0], decoded(e["first"]["reads"])):
            noticed.append(name)
    for reads, k, c in _generated():
        broken, whole = kr.correct_reads(reads, k, c, broken=(rule,)), kr.correct_reads(reads, k, c)
        if not same(broken[0], whole[0]) or broken[1] != whole[1]:      # the reads, or the records
            noticed.append("generated")
    assert noticed, rule


def test_the_tables_of_the_restatement_are_the_oracle_s():
    reads, _, _ = kr.mixed_reads()
    text = kr.mirrored(kr.joined(reads))
    suf, lcp = kr.tables(text)
    t = ou.esa(text, 4)
    assert np.array_equal(suf, t["suf"]) and np.array_equal(lcp, t["lcpfull"])


def test_the_generated_sets_have_their_shapes():
    tile = 256
    for seed, kind in ((79, "head"), (0, "child")):
        layout = []
        kr.correct(kr.mirrored(kr.joined(kr.coverage_reads(seed, 20, 60))), 6, 2, True, layout=layout)
        assert kr.tile_border(layout, tile, kind)
    reads, k, c = kr.invalid_tail_reads(tile)
    layout = []
    kr.correct(kr.mirrored(kr.joined(reads)), k, c, True, layout=layout)
    assert any(len(heads) - valid > tile and recs for _, _, heads, valid, recs in layout)
    reads, k, c = kr.many_records_reads()
    layout = []
    text = kr.mirrored(kr.joined(reads))
    _, _, info = kr.correct(text, k, c, True, layout=layout)
    assert info["records"] > 4096 and layout[0][0] == 0 and layout[-1][1] == int((text < 254).sum())
    assert layout[0][4] and layout[-1][4]
    reads, k, c = kr.chain_reads()
    assert kr.correct_reads(reads, k, c)[2]["chain"] >= 3
