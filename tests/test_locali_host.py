"""CPU-side checks of the local-alignment boundary: include/gtamd_locali.h is
exported and bound, its host-only entry point works without a device,
`gt-suffixerator-amd idxlocali` words the errors that end before the device as
`gt dev idxlocali` does and refuses what this path does not do, and the numpy
statement with its line formatter (tests/locali_reference.py) reproduces every
output of the reference recorded in tests/golden/golden_locali.json (the match
blocks of one query sorted) -- before a device is involved."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import locali_golden as lg
import locali_reference as lr
import oracle_util as ou
from genometools_amd import _lib, locali

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_locali.h")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
# (the statement is numpy: the calls on the 100 k symbols of the protein fixture and the two with some
# ten thousand lines are left to tests/test_locali_cli_gpu.py, which runs them all)
RUNNING = sorted(k for k, v in lg.GOLDEN["calls"].items()
                 if v["exit"] == 0 and v["lines"] < 2000 and not k.startswith("sw100K1") and
                 k not in lg.GOLDEN["texts"].values())          # (those: test_the_texts_kept_whole)
ENDING = sorted(k for k, v in lg.GOLDEN["calls"].items() if v["exit"] != 0)


def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _tool(*args):
    ou.build()
    p = subprocess.run([CLI, "idxlocali"] + list(args), capture_output=True)
    return p.returncode, p.stdout, p.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(gtamd_[a-z_0-9]+)\s*\(", _header_text())))
    assert len(declared) == 10, declared
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.LOCALI_ABI[name][1], name
    assert sorted(_lib.LOCALI_ABI) == declared
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_locali.hip") in _lib.SOURCES
    assert os.path.join(_lib.HERE, "csrc", "esa_locali_core.h") in _lib.HEADERS


def test_info_structure_matches_the_header():
    text = _header_text()
    body = text[text.index("typedef struct {\n  uint64_t jobs"):text.index("} gtamd_locali_info;")]
    names = re.findall(r"\b(?:u?int\d+_t|float)\s+([a-z_]+);", body)
    assert names == [n for n, _ in _lib.LocaliInfo._fields_]
    assert ctypes.sizeof(_lib.LocaliInfo) == 10 * 8 + 16
    assert "#define GTAMD_LOCALI_AUTO 0xffffffffu" in text and locali.AUTO == 0xffffffff


def test_geometry_needs_no_device():
    waves, least, longest, stack = locali.geometry()
    assert waves >= 1 and least >= 1 and longest >= 1024 and stack >= 1


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_locali_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()


def test_pack_and_unpack():
    symbols, offsets = locali.pack_queries([[0, 1, 254], [3], []])
    assert symbols.tolist() == [0, 1, 254, 3] and offsets.tolist() == [0, 3, 4, 4] and offsets.dtype == np.uint64
    q, p, dblen, score, qstart, qlen = locali.unpack([[7, 5, 12 | 9 << 32, 3 | 11 << 32]])
    assert (q[0], p[0], dblen[0], score[0], qstart[0], qlen[0]) == (7, 5, 12, 9, 3, 11)


# ---- the tool, up to where a device is needed ----

@pytest.mark.parametrize("key", ENDING)
def test_calls_that_end_before_a_query_is_read(key):
    """the reference's exit code and words"""
    subject, _, args, files = lg.parse(key)
    want = lg.GOLDEN["calls"][key]
    rc, out, err = _tool(*args, "-esa", "nowhere", "-q", *files)
    assert rc == want["exit"] == 1 and out == b""
    assert err == "gt dev idxlocali: error: %s\n" % want["error"]


def test_refusals_of_the_tool(tmp_path):
    for option in ("-pck", "-online", "-cmp"):
        rc, out, err = _tool("-th", "5", "-esa", "x", "-q", "y", option)
        assert rc == 1 and err == 'gt dev idxlocali: error: option "%s" is not supported by the MI355X engine\n' % option
    for scores in (("-match", "0"), ("-mismatch", "0"), ("-gapextend", "1"), ("-match", "40000")):
        rc, out, err = _tool("-th", "5", "-esa", "x", "-q", "y", *scores)
        assert rc == 1 and out == b"" and "the match score must be in 1..32767" in err
    assert _tool("-th", "5", "-esa", "x")[2] == 'gt dev idxlocali: error: option "-q" is mandatory\n'
    assert _tool("-th", "5", "-q", "y")[2] == 'gt dev idxlocali: error: either option "-esa" or option "-pck" is mandatory\n'
    assert _tool("-th", "5", "-esa", "x", "-q", "y", "-frob")[2].startswith("gt dev idxlocali: error: unknown option: -frob")
    assert _tool("-th", "5", "-esa", "x", "-q", "y", "-match")[2] == 'gt dev idxlocali: error: missing argument to option "-match"\n'
    rc, out, err = _tool("-th", "5", "-esa", str(tmp_path / "none"), "-q", "y")
    assert rc == 1 and out.decode().endswith("# threshold=5\n") and out.startswith(b"# indexname(esa)=")
    assert "none" in err
    rc, out, _ = _tool("-help")
    assert rc == 0 and b"-gapstart" in out and b"without effect" in out


# ---- the numpy statement against the recorded calls of the reference ----

def _index(subject, protein):
    enc = ou.encode_fasta(ou.fixture_path(subject), protein=protein)
    return enc, ou.esa(enc, 20 if protein else 4)["suf"]


@pytest.mark.parametrize("key", RUNNING)
def test_the_statement_reproduces_the_reference(key):
    subject, protein, args, files = lg.parse(key)
    T, match, mismatch, gapextend, show = lg.options(args)
    enc, suf = _index(subject, protein)
    text = lr.tool_stdout(enc, suf, lg.read_queries(files, protein), T, match, mismatch, gapextend, show,
                          lg.PROTEIN_LETTERS if protein else "acgt", "X" if protein else "n")
    got = lg.compared(text.encode("latin-1"))
    want = lg.GOLDEN["calls"][key]
    assert got.count(b"\n") == want["lines"]
    assert hashlib.md5(got).hexdigest() == want["md5"]


@pytest.mark.parametrize("name", sorted(lg.GOLDEN["texts"]))
def test_the_texts_kept_whole(name):
    """byte for byte, the one with -s among them: the formatter of the alignments"""
    key = lg.GOLDEN["texts"][name]
    subject, protein, args, files = lg.parse(key)
    T, match, mismatch, gapextend, show = lg.options(args)
    enc, suf = _index(subject, protein)
    text = lr.tool_stdout(enc, suf, lg.read_queries(files, protein), T, match, mismatch, gapextend, show)
    with open(os.path.join(lg.QUERYDIR, name), "rb") as f:
        assert lg.compared(text.encode("latin-1")) == f.read()


def test_gapstart_changes_nothing():
    calls = lg.GOLDEN["calls"]
    assert calls["Atinsert.fna|dna|-th 25 -gapstart -1|Atinsert.fna"]["md5"] == calls["Atinsert.fna|dna|-th 25|Atinsert.fna"]["md5"]
    assert calls["Random.fna|dna|-th 14 -gapstart -20|Random.fna"]["md5"] == calls["Random.fna|dna|-th 14|Random.fna"]["md5"]
