"""CPU-side checks of the matching statistics boundary: include/gtamd_mstat.h is
exported and bound, its host-only entry point works without a device,
`gt-suffixerator-amd matstat` / `uniquesub` word their argument errors as the
reference does, and the brute-force restatement with its line formatter
(tests/mstat_reference.py) reproduces every output of the reference recorded in
tests/golden/golden_mstat.json -- before a device is involved."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mstat_reference as mr
import oracle_util as ou
from genometools_amd import _lib, mstat

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_mstat.h")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
CHARACTERS = {"dna": "acgt", "protein": "LVIFKREDAGSTNQYWPHMC"}

with open(os.path.join(ou.GOLDEN_DIR, "golden_mstat.json")) as _f:
    GOLDEN = json.load(_f)


def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_every_declared_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(gtamd_[a-z_0-9]+)\s*\(", _header_text())))
    assert len(declared) == 9, declared
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.MSTAT_ABI[name][1], name
    assert sorted(_lib.MSTAT_ABI) == declared
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_mstat.hip") in _lib.SOURCES


def test_info_structure_matches_the_header():
    text = _header_text()
    body = text[text.index("typedef struct {"):text.index("} gtamd_mstat_info;")]
    names = re.findall(r"\b(?:u?int\d+_t|float)\s+([a-z_]+);", body)
    assert names == [n for n, _ in _lib.MstatInfo._fields_]
    assert ctypes.sizeof(_lib.MstatInfo) == 4 + 4 + 3 * 8


def test_geometry_needs_no_device():
    tile, word, word_min = mstat.geometry()
    assert tile >= 64 and tile % 64 == 0          # whole waves
    assert 1 < word_min <= word <= 64


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_mstat_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    with pytest.raises(_lib.EsaError, match="no HIP device"):
        mstat.MatchStats()


# ---- the tools: what ends before a device is asked for ----

@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """a project without tables, written by the tool's host side"""
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    idx = str(tmp_path_factory.mktemp("mstat") / "at")
    subprocess.run([CLI, "-dna", "-db", ou.fixture_path("Atinsert.fna"), "-indexname", idx], check=True)
    return idx


def _error(tool, *args):
    p = subprocess.run([CLI, tool] + list(args), capture_output=True, text=True)
    prefix = "gt %s: error: " % tool
    assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith(prefix) and \
        p.stderr.endswith("\n"), (p.returncode, p.stdout, p.stderr)
    return p.stderr[len(prefix):-1]


@pytest.mark.parametrize("tool", ["matstat", "uniquesub"])
def test_argument_errors(index, tool):
    q = ou.fixture_path("Random159.fna")
    assert _error(tool, "-min", "1", "-query", q) == "one of the options -esa, -pck must be used"
    assert _error(tool, "-esa", index, "-query", q) == "one of the options -min or -max must be set"
    assert _error(tool, "-esa", index, "-query", q, "-min", "5", "-max", "4") == \
        "minvalue must be smaller or equal than maxvalue"
    assert _error(tool, "-esa", index, "-query", q, "-min", "1", "-output") == \
        "missing arguments to option -output"
    assert _error(tool, "-esa", index, "-min", "1", "-output", "-query", q) == \
        "missing arguments to option -output"
    assert _error(tool, "-esa", index, "-min", "1") == 'option "-query" is mandatory'
    assert _error(tool) == 'option "-query" is mandatory'
    for opt in ("-fmi", "-pck"):
        assert _error(tool, opt, index, "-query", q, "-min", "1") == \
            'option "%s" is not supported by the MI355X engine' % opt
    assert _error(tool, "-esa", index, "-query", q, "-min", "1", "-frobnicate") == \
        "unknown option: -frobnicate (try -help)"
    assert _error(tool, "-esa", index, "-query", q, "-min", "0") == \
        'argument to option "-min" must be an integer >= 1'
    assert _error(tool, "-esa", index, "-query", q, "-max") == 'missing argument to option "-max"'
    assert _error(tool, "-esa", index, "-query", q, "-min", "1", "-output", "sideways").startswith(
        'illegal argument "sideways" to option -output')


def test_subjectpos_is_a_flag_of_matstat_only(index):
    q = ou.fixture_path("Random159.fna")
    assert _error("uniquesub", "-esa", index, "-query", q, "-min", "1", "-output", "subjectpos").startswith(
        'illegal argument "subjectpos" to option -output')


def test_file_errors_end_before_the_device(index, tmp_path):
    q = ou.fixture_path("Random159.fna")
    missing = str(tmp_path / "nosuch")
    assert _error("matstat", "-esa", missing, "-query", q, "-min", "1") == "cannot open file '%s.prj'" % missing
    # the project has no tables
    assert _error("matstat", "-esa", index, "-query", q, "-min", "1") == "cannot open file '%s.suf'" % index
    # the query is read with the index's alphabet: a protein file is no DNA
    n = int(dict(l.split("=") for l in open(index + ".prj").read().splitlines())["totallength"])
    with open(index + ".suf", "wb") as f:
        f.write(bytes(8 * (n + 1)))
    msg = _error("uniquesub", "-esa", index, "-query", ou.fixture_path("sw100K1.fsa"), "-min", "1")
    assert msg.startswith("illegal character '") and "sw100K1.fsa" in msg
    noquery = str(tmp_path / "noquery")
    assert _error("matstat", "-esa", index, "-query", noquery, "-min", "1") == "cannot open file '%s'" % noquery
    os.remove(index + ".suf")


# ---- the restatement against the reference's outputs ----

def expected_output(kind, subject, query, call):
    protein = kind == "protein"
    ms, w, mu = mr.expected(subject, query, protein)
    args = GOLDEN["calls"][call]
    show = set(args[args.index("-output") + 1:args.index("-min")])
    maxlen = int(args[args.index("-max") + 1]) if "-max" in args else None
    return mr.tool_output(mr.encoded(query, protein), mr.read_descriptions(ou.fixture_path(query)),
                          ms if call.startswith("matstat") else mu, w, CHARACTERS[kind], show,
                          minlen=int(args[args.index("-min") + 1]), maxlen=maxlen)


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_brute_force_and_formatter_reproduce_the_reference(kind):
    assert len(GOLDEN[kind]) == (72 if kind == "dna" else 1)
    calls = 0
    for pair, entry in sorted(GOLDEN[kind].items()):
        subject, query = pair.split("|")
        assert sorted(entry) == sorted(GOLDEN["calls"])
        for call, want in sorted(entry.items()):
            text = expected_output(kind, subject, query, call).encode("latin-1")
            assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), \
                (pair, call)
            calls += 1
    assert calls == 4 * len(GOLDEN[kind])


def test_text_fixtures_are_those_of_the_json():
    assert len(GOLDEN["texts"]) == 3
    for name, t in GOLDEN["texts"].items():
        raw = open(os.path.join(ou.GOLDEN_DIR, "mstat", name), "rb").read()
        want = GOLDEN[t["alphabet"]]["%s|%s" % (t["subject"], t["query"])][t["call"]]
        assert (hashlib.md5(raw).hexdigest(), raw.count(b"\n")) == (want["md5"], want["lines"]), name
        assert raw.decode("latin-1") == expected_output(t["alphabet"], t["subject"], t["query"], t["call"])


def test_brute_force_on_a_case_worked_by_hand():
    """subject acgtacg$ (suffix table by hand), query acgx / cgta|t: x is a letter
    the subject lacks, | a separator"""
    enc = np.array([0, 1, 2, 3, 0, 1, 2], dtype=np.uint8)
    suf = ou.esa(enc, 4)["suf"]
    assert suf.tolist() == [0, 4, 1, 5, 2, 6, 3, 7]       # acgtacg acg cgtacg cg gtacg g tacg $
    ms, w, mu = mr.brute_force(enc, suf, np.array([0, 1, 2, 5, 255, 1, 2, 3, 0, 255, 3], dtype=np.uint8))
    assert ms.tolist() == [3, 2, 1, 0, 0, 4, 3, 2, 1, 0, 1]
    assert w.tolist() == [0, 1, 2, 0, 0, 1, 2, 3, 0, 0, 3]
    assert mu.tolist() == [0, 0, 0, 0, 0, 3, 2, 1, 0, 0, 1]
