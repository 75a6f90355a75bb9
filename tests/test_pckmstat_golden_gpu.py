"""matstat and uniquesub through a packed index (mstat.MatchStats.set_index_packed
over pck.PackedIndexReader) against the reference: for every call recorded from
`gt matstat -pck` and `gt uniquesub -pck` in tests/golden/golden_pckmstat.json
(tests/golden/make_golden_pckmstat.py: the option set of the reference's index
searches for all 72 pairs of its nine DNA fixtures and a protein pair, four more
index flavours for three subjects), the lengths and witnesses of the device,
written out by the line formatter of tests/mstat_reference.py, have the md5 and
the line count of the reference's stdout; three outputs are compared whole.

The index is built on the device with the options of the recorded flavour
(its image is the reference's file byte for byte: tests/test_pck_gpu.py) and
opened from host memory, as a file would be."""
import hashlib
import json
import os

import pytest

import mstat_reference as mr
import oracle_util as ou
from genometools_amd import _lib, esa, mstat, pck

pytestmark = pytest.mark.gpu

CHARACTERS = {"dna": "acgt", "protein": "LVIFKREDAGSTNQYWPHMC"}
SUITE = dict(bsize=10, blbuck=8, locfreq=32, sprank=True, mkindex=True)
# flavour of make_golden_pckmstat.py -> (read mode of -dir, options of the builder)
FLAVOURS = {"suite": (1, SUITE), "defaults": (1, dict(mkindex=True)), "locbitmap": (1, dict(locbitmap=True, mkindex=True)),
            "locfreq0": (1, dict(locfreq=0, mkindex=True)), "fwd": (0, SUITE)}
SHOW = {"matstat": {"querypos", "subjectpos", "sequence"}, "uniquesub": {"querypos", "sequence"},
        "matstat_max20": {"querypos"}, "uniquesub_max20": {"querypos"}}

with open(os.path.join(ou.GOLDEN_DIR, "golden_pckmstat.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def tools(gpu):
    with pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, mstat.MatchStats() as searcher:
        yield builder, reader, searcher


def _open(tools, subject, flavour, kind):
    """the searcher over the packed index of a fixture"""
    builder, reader, searcher = tools
    protein = kind == "protein"
    readmode, kw = FLAVOURS[flavour]
    if protein:      # mkindex falls back to block size 3 over 20 letters (src/match/sfx-run.c:389-393)
        kw = dict(kw, bsize=3)
    enc = mr.encoded(subject, protein)
    with esa.EsaEngine(enc.size, 20 if protein else 4) as eng:
        eng.set_readmode(readmode)
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        builder.build_from_esa(eng, **kw)
    reader.open(builder.image())
    assert reader.info()["rows"] == enc.size + 1
    searcher.set_index_packed(reader)
    return searcher


def _stdout(searcher, call, query_name, kind):
    """what the reference prints for this call: GOLDEN["calls"][call] are its options"""
    args = GOLDEN["calls"][call]
    assert args[:1] == ["-output"] and args[-2:] in (["-min", "1"], ["-max", "20"])
    maxlen = 20 if args[-2] == "-max" else None
    query = mr.encoded(query_name, kind == "protein")
    if call.startswith("matstat"):
        if "subjectpos" in SHOW[call]:
            length, pos = searcher.matstat(query, maxlen or 0)
        else:        # (an index without locate information answers lengths only)
            import torch
            q = torch.from_numpy(query.copy()).to("cuda:0")
            out = torch.zeros(max(1, query.size), dtype=torch.int32, device="cuda:0")
            searcher.matstat_device(q.data_ptr(), query.size, out.data_ptr(), None, maxlen or 0)
            length, pos = out.cpu().numpy()[:query.size], None
    else:
        length, pos = searcher.uniquesub(query, maxlen or 0), None
    text = mr.tool_output(query, mr.read_descriptions(ou.fixture_path(query_name)), length, pos, CHARACTERS[kind],
                          SHOW[call], minlen=1, maxlen=maxlen)
    return text.encode("latin-1")


def _cases():
    return sorted({tuple(k.split("|")[:2]) for k in GOLDEN["dna"]})


def test_what_is_recorded():
    assert len(GOLDEN["dna"]) == 72 + 4 * 24 and len(GOLDEN["protein"]) == 1 and len(GOLDEN["texts"]) == 3
    assert {k.split("|")[0] for k in GOLDEN["dna"]} == set(FLAVOURS)
    assert GOLDEN["calls"]["matstat"] == ["-output", "querypos", "subjectpos", "sequence", "-min", "1"]
    assert GOLDEN["calls"]["uniquesub"] == ["-output", "querypos", "sequence", "-min", "1"]
    assert GOLDEN["calls"]["matstat_max20"] == GOLDEN["calls"]["uniquesub_max20"] == \
        ["-output", "querypos", "-min", "1", "-max", "20"]


@pytest.mark.parametrize("flavour,subject", _cases())
def test_every_recorded_call(tools, flavour, subject):
    searcher = _open(tools, subject, flavour, "dna")
    keys = [k for k in sorted(GOLDEN["dna"]) if tuple(k.split("|")[:2]) == (flavour, subject)]
    assert len(keys) == 8
    for key in keys:
        calls = sorted(GOLDEN["dna"][key])
        assert len(calls) == (2 if flavour == "locfreq0" else 4)
        for call in calls:
            out = _stdout(searcher, call, key.split("|")[2], "dna")
            want = GOLDEN["dna"][key][call]
            assert (hashlib.md5(out).hexdigest(), out.count(b"\n")) == (want["md5"], want["lines"]), (key, call)


def test_the_protein_pair(tools):
    (key, entry), = GOLDEN["protein"].items()
    flavour, subject, query = key.split("|")
    searcher = _open(tools, subject, flavour, "protein")
    for call, want in sorted(entry.items()):
        out = _stdout(searcher, call, query, "protein")
        assert (hashlib.md5(out).hexdigest(), out.count(b"\n")) == (want["md5"], want["lines"]), call


@pytest.mark.parametrize("name", sorted(GOLDEN["texts"]))
def test_whole_outputs(tools, name):
    t = GOLDEN["texts"][name]
    searcher = _open(tools, t["subject"], t["flavour"], t["alphabet"])
    with open(os.path.join(ou.GOLDEN_DIR, "pckmstat", name), "rb") as f:
        assert _stdout(searcher, t["call"], t["query"], t["alphabet"]) == f.read()


def test_an_index_without_locate_information(tools):
    searcher = _open(tools, "Atinsert.fna", "locfreq0", "dna")
    query = mr.encoded("Random160.fna", False)
    assert searcher.uniquesub(query).size == query.size
    with pytest.raises(_lib.EsaError, match="no locate information"):
        searcher.matstat(query)
