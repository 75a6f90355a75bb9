"""Tag matches through a packed index (tagmatch.TagMatches.set_index_packed over
pck.PackedIndexReader) against the reference: for every call recorded from `gt
tagerator -pck` in tests/golden/golden_pcktagmatch.json
(tests/golden/make_golden_pcktagmatch.py: the calls of golden_tagmatch.json
without a wildcard option on a -dir rev index with the options of the reference's
index searches, and on two more index flavours for two subjects) the records of
the device, written out by the line formatter of tests/tagmatch_reference.py,
have the md5 and the line count of the reference's stdout, the match lines of one
tag sorted on both sides.  Three outputs are compared whole, and the INDEX.bdx
the reference itself wrote for one fixture gives the records of the image built
here.

The reference aborts ("Requesting LF-map for symbol from range of undefined
sorting") in the calls with K > 0 on the two flavours without -sprank of
Atinsert.fna, whose single walks run into wildcards: there the device is held to
the recording of the same call on the -sprank flavour."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_util as ou
import tagmatch_reference as tr
from genometools_amd import esa, pck, tagmatch
from test_tagmatch_host import parse_call

pytestmark = pytest.mark.gpu

TAGDIR = os.path.join(ou.GOLDEN_DIR, "tagmatch")
OUTDIR = os.path.join(ou.GOLDEN_DIR, "pcktagmatch")
FLAVOURS = {"suite": dict(bsize=10, blbuck=8, locfreq=32, sprank=True, mkindex=True),
            "defaults": dict(mkindex=True), "locbitmap": dict(locbitmap=True, mkindex=True)}

with open(os.path.join(ou.GOLDEN_DIR, "golden_pcktagmatch.json")) as _f:
    GOLDEN = json.load(_f)
INDEXES = sorted({tuple(k.split("|")[i] for i in (0, 1, 4)) for k in GOLDEN["calls"]})


@pytest.fixture(scope="module")
def tools(gpu):
    with pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, tagmatch.TagMatches() as matcher:
        yield dict(builder=builder, reader=reader, matcher=matcher)


def _image(tools, enc, sigma, flavour):
    kw = FLAVOURS[flavour]
    if sigma == 20:      # mkindex falls back to block size 3 over 20 letters (src/match/sfx-run.c:389-393)
        kw = dict(kw, bsize=3)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_readmode(1)
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        tools["builder"].build_from_esa(eng, **kw)
        return tools["builder"].image()


def _device_text(matcher, enc, key):
    """what the reference prints for this call, from the records of the device"""
    subject, protein, K, flags, output, tagfiles = parse_call(key.rsplit("|", 1)[0])
    letters = tr.PROTEIN if protein else tr.DNA
    tags = tr.read_tags([os.path.join(TAGDIR, t + ".tags.fna") for t in tagfiles])
    stop = next((i for i, t in enumerate(tags) if K > 0 and len(t) <= K), len(tags))
    rec = matcher.all_records([tr.encode_tag(t, letters) for t in tags[:stop]], K, flags)
    starts = np.concatenate([[0], np.flatnonzero(enc == 255) + 1])
    pre = tr.preamble(K, "", [], output)
    lines = [pre[0], pre[-1]]
    for t, tag in enumerate(tags[:stop + 1]):
        lines.append("#" + ("\t%d" % t if "tagnum" in output else "") +
                     (("\t" if "tagnum" in output else "") + (tag.upper() if protein else tag.lower())
                      if "tagseq" in output else ""))
        if t < stop:
            for r in rec[(rec[:, 0] >> np.uint64(1)) == t]:
                line = tr.match_line(enc, starts, letters, r, output)
                if line is not None:
                    lines.append(line)
    return "".join(l + "\n" for l in tr.block_sorted(lines)).encode("latin-1")


@pytest.mark.parametrize("subject,alphabet,flavour", INDEXES)
def test_the_recorded_calls(tools, subject, alphabet, flavour):
    assert len(GOLDEN["calls"]) == 67 and len(INDEXES) == 11
    protein = alphabet == "protein"
    enc = ou.encode_fasta(ou.fixture_path(subject), protein)
    reader = tools["reader"].open(_image(tools, enc, 20 if protein else 4, flavour))
    tools["matcher"].set_index_packed(reader)
    calls = [k for k in sorted(GOLDEN["calls"]) if tuple(k.split("|")[i] for i in (0, 1, 4)) == (subject, alphabet, flavour)]
    assert len(calls) in (2, 6, 7, 8)
    for key in calls:
        want = GOLDEN["calls"][key]
        K = parse_call(key.rsplit("|", 1)[0])[2]
        if want["exit"] < 0:
            # the reference aborted: only on Atinsert without -sprank, with K > 0
            assert (subject, K > 0) == ("Atinsert.fna", True) and flavour != "suite", key
            want = GOLDEN["calls"][key.rsplit("|", 1)[0] + "|suite"]
        assert (want["exit"], "must be longer than the allowed number of errors" in want["error"]) == \
            ((1, True) if K > 0 else (0, False)), key
        text = _device_text(tools["matcher"], enc, key)
        assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key


def test_what_the_recording_says_about_the_suffix_table(gpu):
    """after the block sort the reference prints the same through -pck and -esa,
    but where it aborted; of the wildcard calls, which the device is not held to,
    one differs"""
    aborted = sorted(k for k, c in GOLDEN["calls"].items() if c["exit"] < 0)
    assert len(aborted) == 12 and all(k.startswith("Atinsert.fna|") and not k.endswith("|suite") for k in aborted)
    assert all(c["as_esa"] == (c["exit"] >= 0) for c in GOLDEN["calls"].values())
    assert sorted(k for k, c in GOLDEN["wildcard_calls"].items() if not c["as_esa"]) == \
        ["Atinsert.fna|dna|-e 2 -withwildcards no|Atinsert.fna|suite"]
    assert len(GOLDEN["wildcard_calls"]) == 4


def test_three_outputs_whole(tools):
    assert len(GOLDEN["texts"]) == 3
    for name, key in sorted(GOLDEN["texts"].items()):
        subject = key.split("|")[0]
        enc = ou.encode_fasta(ou.fixture_path(subject))
        tools["matcher"].set_index_packed(tools["reader"].open(_image(tools, enc, 4, "suite")))
        with open(os.path.join(OUTDIR, name), "rb") as f:
            raw = f.read()
        assert raw.count(b"\n") == GOLDEN["calls"][key]["lines"] > 30
        assert _device_text(tools["matcher"], enc, key) == raw


def test_the_index_file_the_reference_wrote(tools):
    subject, flavour, name = GOLDEN["image"]
    enc = ou.encode_fasta(ou.fixture_path(subject))
    tags = [tr.encode_tag(t) for t in tr.read_tags([os.path.join(TAGDIR, subject + ".tags.fna")])][:-1]
    matcher = tools["matcher"]
    matcher.set_index_packed(tools["reader"].open(_image(tools, enc, 4, flavour)))
    ours = [matcher.all_records(tags, K, flags) for K, flags in ((0, 3), (2, 3), (2, 7))]
    with open(os.path.join(OUTDIR, name), "rb") as f:
        raw = f.read()
    assert 1000 < len(raw) < 20000
    matcher.set_index_packed(tools["reader"].open(raw))
    info = tools["reader"].info()
    assert (info["rows"], info["locate_interval"], info["block_size"]) == (enc.size + 1, 32, 10)
    theirs = [matcher.all_records(tags, K, flags) for K, flags in ((0, 3), (2, 3), (2, 7))]
    assert ours[1].shape[0] > 30 and all(np.array_equal(a, b) for a, b in zip(ours, theirs))
