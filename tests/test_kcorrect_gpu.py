"""The k-mer correction on the device (include/gtamd_kcorrect.h,
genometools_amd/kcorrect.py) against the restatement tests/kcorrect_reference.py
and, for the golden sets, against what the reference did: the records, the
corrected symbols and the info.  The tables come from the engine, in this
process, resident or handed over as 8- and as 4-byte entries, of the mirrored
and of the unmirrored set.

The shapes are the smallest at which each part can go wrong: a workgroup takes
TILE table entries, children or records (kcorrect.geometry()), the flags of a
tile are one ballot a wave, the sort takes 4096 records a chunk, .lcp holds a
byte 255 from 255 letters on."""
import functools
import json
import os

import numpy as np
import pytest

import kcorrect_reference as kr
import oracle_util as ou
from genometools_amd import _lib, esa, kcorrect

pytestmark = pytest.mark.gpu

TILE = kcorrect.geometry()


@pytest.fixture(scope="module")
def corrector(gpu):
    with kcorrect.KmerCorrection() as kc:
        yield kc


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(ou.GOLDEN_DIR, "golden_correct.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _set(name):
    """(reads, k, c) of a named set"""
    kind, _, arg = name.partition(":")
    if kind == "golden":
        e = _golden()["sets"][arg]
        return kr.parse_fasta(os.path.join(ou.GOLDEN_DIR, "correct", e["file"])), e["k"], e["c"]
    if kind == "coverage":
        return kr.coverage_reads(int(arg), 20, 60), 6, 2
    if kind == "widths":
        return kr.width_reads()
    if kind == "tail":
        return kr.invalid_tail_reads(TILE)
    if kind == "many":
        return kr.many_records_reads()
    if kind == "chain":
        return kr.chain_reads()
    if kind == "mixed":
        return kr.mixed_reads()
    if kind == "long":
        return kr.long_reads(), int(arg), 2
    if kind == "clean":
        k, c = arg.split(",")
        return kr.coverage_reads(8, 40, 120, errors=0.0, genome=200), int(k), int(c)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def _expected(name, mirror):
    """(text, corrected symbols, triples, info, layout) of the restatement; shared, never written to"""
    reads, k, c = _set(name)
    text = kr.joined(reads)
    if mirror:
        text = kr.mirrored(text)
    layout = []
    want, triples, info = kr.correct(text, k, c, mirror, layout=layout)
    triples = np.array(triples, dtype=np.uint64).reshape(-1, 3)
    for a in (text, want, triples):
        a.setflags(write=False)
    return text, want, triples, info, layout


FIGURES = ("table_entries", "groups", "untrusted_groups", "records", "dependent", "rounds", "changed", "delta")


def _check(kc, name, mirror):
    text, want, triples, info, _ = _expected(name, mirror)
    _, k, c = _set(name)
    got = kc.decide(k, c)
    assert {f: got[f] for f in FIGURES} == {f: info[f] for f in FIGURES}
    assert got == kc.info() and (got["k"], got["c"]) == (k, c)
    assert got["suffixes"] == int((text < 254).sum()) and got["device_bytes"] > 0 and got["device_ms"] >= 0
    assert np.array_equal(kc.records(), triples)
    out = kc.corrected()
    assert np.array_equal(out, want), np.flatnonzero(out != want)[:10]
    unmirrored = np.array(text[:want.size])
    assert np.array_equal(kc.corrected(unmirrored), want)
    assert int((out != unmirrored).sum()) == got["changed"]
    letters = unmirrored < 4
    delta = np.bincount(out[letters], minlength=4)[:4] - np.bincount(unmirrored[letters], minlength=4)[:4]
    assert delta.tolist() == got["delta"]
    return got


def _agree(kc, name, mirrors=(True, False), widths=(np.uint32,)):
    """the set through the resident engine and through host tables of the given widths"""
    import torch
    last = None
    for mirror in mirrors:
        text = _expected(name, mirror)[0]
        dev = torch.from_numpy(np.array(text)).cuda()
        with esa.EsaEngine(dev.numel(), 4) as eng:
            eng.set_sequence_device(dev.data_ptr(), dev.numel())
            eng.run(esa.WANT_SUF | esa.WANT_LCP)
            kc.set_index_engine(eng, dev.data_ptr(), dev.numel(), mirrored=mirror)
            last = _check(kc, name, mirror)
            tables = (eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP))
        for width in widths:
            kc.set_index(np.array(text), tables[0].astype(width), tables[1], mirrored=mirror)
            _check(kc, name, mirror)
    return last


@pytest.mark.parametrize("name", ["errors_1", "planted", "live", "chain", "conflict", "group_once"])
def test_golden_sets_are_the_reference_s(corrector, name):
    _agree(corrector, "golden:" + name, mirrors=(True,), widths=(np.uint32, np.uint64))
    e = _golden()["sets"][name]
    want = kr.joined([np.array(["acgt".index(ch) for ch in s], dtype=np.uint8) for s in e["first"]["reads"]])
    assert np.array_equal(corrector.corrected(), want)
    _agree(corrector, "golden:" + name, mirrors=(False,), widths=())


@pytest.mark.parametrize("seed,kind", [(79, "head"), (0, "child")])
def test_tile_borders(corrector, seed, kind):
    """a group whose head is the last entry of a tile and whose second child starts the next; a child on both sides"""
    name = "coverage:%d" % seed
    assert kr.tile_border(_expected(name, True)[4], TILE, kind)
    _agree(corrector, name, widths=(np.uint32, np.uint64))


def test_the_first_and_the_last_group_and_more_records_than_a_chunk_of_the_sort(corrector):
    text, _, _, info, layout = _expected("many", True)
    assert layout[0][0] == 0 and layout[-1][1] == int((text < 254).sum()) and layout[0][4] and layout[-1][4]
    assert info["records"] > 4096 > TILE
    _agree(corrector, "many", widths=(np.uint64,))


def test_child_widths(corrector):
    """children of c - 1, c and c + 1 entries; four trusted; three trusted and one absent; one untrusted alone"""
    assert _agree(corrector, "widths", widths=(np.uint32, np.uint64))["records"] >= 2


def test_more_invalid_children_than_a_tile(corrector):
    layout = _expected("tail", True)[4]
    assert any(len(heads) - valid > TILE and recs for _, _, heads, valid, recs in layout)
    assert _agree(corrector, "tail")["records"] >= 1


def test_chains_of_three(corrector):
    info = _expected("chain", True)[3]
    assert info["chain"] >= 3 and info["rounds"] >= 2 and info["records"] > TILE
    _agree(corrector, "chain", mirrors=(True,), widths=(np.uint64,))


@pytest.mark.parametrize("k", [254, 255])
def test_k_up_to_255(corrector, k):
    got = _agree(corrector, "long:%d" % k, mirrors=(True,), widths=(np.uint32,))
    assert got["records"] == 2


def test_k_256_is_refused(corrector):
    import torch
    text = _expected("long:255", True)[0]
    dev = torch.from_numpy(np.array(text)).cuda()
    with esa.EsaEngine(dev.numel(), 4) as eng:
        eng.set_sequence_device(dev.data_ptr(), dev.numel())
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        assert (eng.table(esa.TAB_LCP) == 255).sum() > 10
        corrector.set_index_engine(eng, dev.data_ptr(), dev.numel(), mirrored=True)
        for k in (256, 1000, 0):
            with pytest.raises(_lib.EsaError, match="k-mer length from 1 to 255"):
                corrector.decide(k, 2)
        with pytest.raises(_lib.EsaError, match="trusted count of 1 at least"):
            corrector.decide(31, 0)
        with pytest.raises(_lib.EsaError, match="nothing is decided"):
            corrector.records()


@pytest.mark.parametrize("kc", ["13,3", "1,2", "41,2", "40,2", "13,1000", "13,1"])
def test_no_record(corrector, kc):
    got = _agree(corrector, "clean:" + kc, mirrors=(True,), widths=(np.uint32,))
    assert got["records"] == got["changed"] == got["untrusted_groups"] == got["dependent"] == got["rounds"] == 0
    assert got["delta"] == [0, 0, 0, 0] and corrector.records().shape == (0, 3)
    assert np.array_equal(corrector.corrected(), kr.joined(_set("clean:" + kc)[0]))


def test_reads_of_several_lengths_and_a_wildcard(corrector):
    assert _agree(corrector, "mixed", widths=(np.uint32, np.uint64))["records"] >= 5


def test_two_decisions_on_one_index(corrector):
    import torch
    reads = _set("golden:planted")[0]
    text = kr.mirrored(kr.joined(reads))
    dev = torch.from_numpy(text).cuda()
    with esa.EsaEngine(dev.numel(), 4) as eng:
        eng.set_sequence_device(dev.data_ptr(), dev.numel())
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        corrector.set_index_engine(eng, dev.data_ptr(), dev.numel(), mirrored=True)
        for k, c in ((13, 3), (9, 2), (13, 3)):
            want, triples, info = kr.correct(text, k, c, True)
            got = corrector.decide(k, c)
            assert got["records"] == info["records"] and got["changed"] == info["changed"]
            assert np.array_equal(corrector.corrected(), want)
            assert corrector.records(device=True).cpu().numpy().tolist() == [list(t) for t in triples]
            assert np.array_equal(corrector.corrected(device=True).cpu().numpy(), want)


def test_what_is_no_mirrored_set_is_refused(corrector):
    text = kr.joined(_set("golden:errors_1")[0][:3])
    assert text.size % 2 == 0 or text[text.size >> 1] != 255
    t = ou.esa(text, 4)
    with pytest.raises(_lib.EsaError, match="no mirrored set"):
        corrector.set_index(text, t["suf"], t["lcp"], mirrored=True)
    with pytest.raises(_lib.EsaError, match="no index is set"):
        corrector.decide(12, 2)
    corrector.set_index(text, t["suf"], t["lcp"], mirrored=False)
    corrector.decide(12, 2)
    with pytest.raises(_lib.EsaError, match="symbols given"):
        corrector.corrected(text[:-1])


def test_correct_does_all_of_it(gpu):
    reads, k, c = _set("golden:planted")
    want, triples, info = kr.correct_reads(reads, k, c)
    out, records, got = kcorrect.correct(kr.joined(reads), k, c)
    assert np.array_equal(out, kr.joined(want)) and records.tolist() == [list(t) for t in triples]
    assert got["records"] == info["records"]
    # the tool run twice: the restatement applied twice
    again, _, _ = kr.correct_reads(want, k, c)
    assert np.array_equal(kcorrect.correct(out, k, c)[0], kr.joined(again))
