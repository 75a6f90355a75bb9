"""The recorded calls of `gt dev idxlocali ... -pck INDEX`
(tests/golden/golden_pcklocali.json, written by
tests/golden/make_golden_pcklocali.py) against the records of the device, written
out as the reference prints them and compared in the normal form of
tests/locali_golden.py: the two path lines dropped, the match blocks of one
query sorted.  The index is built here as `gt packedindex mkindex ... -dir rev`
builds it, in the three flavours of the recording.  The reference aborted in the
twelve calls on Atinsert.fna without -sprank ("Requesting LF-map for symbol from
range of undefined sorting"); there the device is held to the
recording of the same call with -esa, which every other call equals.  Three
outputs are compared whole.  Only tests/golden/ is read."""
import hashlib
import json
import os

import numpy as np
import pytest

import locali_golden as lg
import locali_reference as lr
import oracle_util as ou
from genometools_amd import esa, locali, pck

pytestmark = pytest.mark.gpu

OUTDIR = os.path.join(ou.GOLDEN_DIR, "pcklocali")
FLAVOURS = {"suite": dict(bsize=10, blbuck=8, locfreq=32, sprank=True, mkindex=True),
            "defaults": dict(mkindex=True), "locbitmap": dict(locbitmap=True, mkindex=True)}

with open(os.path.join(ou.GOLDEN_DIR, "golden_pcklocali.json")) as _f:
    GOLDEN = json.load(_f)
INDEXES = sorted({tuple(k.split("|")[i] for i in (0, 1, 4)) for k in GOLDEN["calls"]})


@pytest.fixture(scope="module")
def tools(gpu):
    with pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, locali.LocalAlignments() as aligner:
        yield dict(builder=builder, reader=reader, aligner=aligner)


def _set_index(tools, enc, sigma, flavour):
    kw = FLAVOURS[flavour]
    if sigma == 20:      # mkindex falls back to block size 3 over 20 letters (src/match/sfx-run.c:389-393)
        kw = dict(kw, bsize=3)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_readmode(1)
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        tools["builder"].build_from_esa(eng, **kw)
        tools["aligner"].set_index_packed(tools["reader"].open(tools["builder"].image()))


def _alignments(enc, query, p, dblen, e, scores, letters, wildcardshow, width=70):
    """lr.alignment_lines for all matches of one query at once: the columns of the
    statement (lr.column) for every start position together, then each traceback"""
    history, prev = [], None
    for d in range(1, int(dblen.max()) + 1):
        c = enc[np.minimum(p + d - 1, enc.size - 1)]          # (beyond a match's dblen: not read again)
        prev, tr = lr.column(prev, c, query, *scores)
        history.append(tr)
    show = lambda c: letters[c] if c < lr.WILDCARD else wildcardshow
    blocks = []
    for k in range(p.size):
        ops, d, i = [], int(dblen[k]), int(e[k])
        while d > 0:
            bit = history[d - 1][k, i]
            ops.append(bit)
            d -= bit != lr.DELETE
            i -= bit != lr.INSERT
        top, mid, low, iv = "", "", "", int(p[k])
        for bit in reversed(ops):
            a = query[i] if bit != lr.INSERT else None
            b = enc[iv] if bit != lr.DELETE else None
            top += "-" if a is None else show(a)
            low += "-" if b is None else show(b)
            mid += "|" if bit == lr.REPLACE and a == b and a < lr.WILDCARD else " "
            i += bit != lr.INSERT
            iv += bit != lr.DELETE
        lines = []
        for at in range(0, len(top), width):
            lines += [top[at:at + width], mid[at:at + width], low[at:at + width]]
        blocks.append(lines)
    return blocks


def _device_text(aligner, enc, key):
    """what the reference prints for this call behind its two path lines, from the
    records of the device, in the normal form"""
    subject, protein, args, files = lg.parse(key.rsplit("|", 1)[0])
    T, match, mismatch, gapextend, show = lg.options(args)
    queries = lg.read_queries(files, protein)
    rec = aligner.all_records(queries, T, match, mismatch, gapextend)
    seqstart = np.concatenate([[0], np.flatnonzero(enc == lr.SEPARATOR) + 1])
    letters, wildcardshow = (lg.PROTEIN_LETTERS, "X") if protein else ("acgt", "n")
    out = ["# threshold=%d" % T]
    number, dbstart, dblen, score, qstart, qlen = (c.astype(np.int64) for c in locali.unpack(rec))
    for qn, query in enumerate(queries):
        out.append("process sequence %d of length %d" % (qn, len(query)))
        mine = np.flatnonzero(number == qn)
        if show and mine.size:
            blocks = _alignments(enc, query, dbstart[mine], dblen[mine], qstart[mine] + qlen[mine],
                                 (match, mismatch, gapextend), letters, wildcardshow)
        for at, k in enumerate(mine):
            p = int(dbstart[k])
            seq = int(np.searchsorted(seqstart, p, side="right")) - 1
            out.append("%d\t%d\t%d\t\t%d\t%d\t%d\t%d" % (seq, p - seqstart[seq], dblen[k], qn, qstart[k], qlen[k], score[k]))
            if show:
                out += blocks[at]
    return lg.compared("".join(line + "\n" for line in out).encode("latin-1"))


@pytest.mark.parametrize("subject,alphabet,flavour", INDEXES)
def test_the_recorded_calls(tools, subject, alphabet, flavour):
    assert len(GOLDEN["calls"]) == 51 and len(INDEXES) == 11
    protein = alphabet == "protein"
    enc = ou.encode_fasta(ou.fixture_path(subject), protein)
    _set_index(tools, enc, 20 if protein else 4, flavour)
    calls = [k for k in sorted(GOLDEN["calls"]) if tuple(k.split("|")[i] for i in (0, 1, 4)) == (subject, alphabet, flavour)]
    assert len(calls) in (2, 4, 5, 6, 7)
    for key in calls:
        want = GOLDEN["calls"][key]
        if want["exit"] != 0:
            # the reference aborted: only on Atinsert without -sprank
            assert subject == "Atinsert.fna" and flavour != "suite" and want["exit"] < 0, key
            assert "LF-map for symbol from range of undefined sorting" in want["error"]
            want = lg.GOLDEN["calls"][key.rsplit("|", 1)[0]]
        assert want["exit"] == 0
        text = _device_text(tools["aligner"], enc, key)
        assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key


def test_what_the_recording_says_about_the_suffix_table(gpu):
    """after the block sort the reference prints the same through -pck and -esa, but
    where it aborted"""
    aborted = sorted(k for k, c in GOLDEN["calls"].items() if c["exit"] != 0)
    assert len(aborted) == 12 and all(k.startswith("Atinsert.fna|") and not k.endswith("|suite") for k in aborted)
    assert all(c["as_esa"] == (c["exit"] == 0) for c in GOLDEN["calls"].values())
    for key, c in GOLDEN["calls"].items():
        other = lg.GOLDEN["calls"][key.rsplit("|", 1)[0]]
        assert c["as_esa"] == ((c["md5"], c["exit"]) == (other["md5"], other["exit"])), key


def test_three_outputs_whole(tools):
    assert len(GOLDEN["texts"]) == 3
    for name, key in sorted(GOLDEN["texts"].items()):
        subject = key.split("|")[0]
        enc = ou.encode_fasta(ou.fixture_path(subject))
        _set_index(tools, enc, 4, "suite")
        with open(os.path.join(OUTDIR, name), "rb") as f:
            raw = f.read()
        assert raw.count(b"\n") == GOLDEN["calls"][key]["lines"] > 10 and len(raw) < 8000
        assert _device_text(tools["aligner"], enc, key) == raw
