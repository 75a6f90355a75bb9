"""CPU-side checks of the suffix-prefix match boundary: include/gtamd_spm.h is
exported and bound, its host-only entry point works without a device, the
brute-force restatement (tests/spm_reference.py) over the mirrored read sets
reproduces, as sorted lines, every output of `gt encseq2spm` recorded in
tests/golden/golden_spm.json and every count, `spm.mirrored` is gtamd_mirror, and
`gt-suffixerator-amd encseq2spm` words the errors that end before the device as
the reference does -- before a device is involved."""
import ctypes
import functools
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import spm_reference as sr
from genometools_amd import _lib, spm

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_spm.h")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
REFUSED = ["-parts", "-memlimit", "-checksuftab", "-onlyaccum", "-onlyallfirstcodes", "-addbscachedepth",
           "-phase2extra", "-radixlarge", "-radixparts", "-singlescan", "-forcek"]

with open(os.path.join(ou.GOLDEN_DIR, "golden_spm.json")) as _f:
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
        assert getattr(lib, name).argtypes == _lib.SPM_ABI[name][1], name
    assert sorted(_lib.SPM_ABI) == declared
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_spm.hip") in _lib.SOURCES
    assert os.path.join(_lib.HERE, "csrc", "esa_spm_core.h") in _lib.HEADERS


def test_info_structure_matches_the_header():
    text = _header_text()
    body = text[text.index("typedef struct {\n  uint64_t table_entries"):text.index("} gtamd_spm_info;")]
    names = re.findall(r"\b(?:u?int\d+_t|float)\s+([a-z_]+);", body)
    assert names == [n for n, _ in _lib.SpmInfo._fields_]
    assert ctypes.sizeof(_lib.SpmInfo) == 8 * 8 + 8


def test_geometry_needs_no_device():
    tile, least = spm.geometry()
    assert tile >= 64 and tile % 64 == 0          # whole waves
    assert least >= 1 and least % tile == 0       # whole workgroups of records


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_spm_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    with pytest.raises(_lib.EsaError, match="no HIP device"):
        spm.SuffixPrefixMatches()


# ---- the mirrored set ----

@functools.lru_cache(maxsize=None)
def reads(name):
    """the encoded reads of a golden call's file, e.g. spm/mixed.fna or fixtures/Reads1.fna"""
    enc = ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, name))
    enc.setflags(write=False)
    return enc


def test_mirrored_is_gtamd_mirror():
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True, stdout=subprocess.DEVNULL)
    _lib.load()                                   # (libgtamd_host.so links it)
    host = ctypes.CDLL(os.path.join(_lib.HERE, "libgtamd_host.so"))
    host.gtamd_mirror.restype = ctypes.c_void_p
    host.gtamd_mirror.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    free = ctypes.CDLL(None).free
    free.argtypes = [ctypes.c_void_p]
    wild = reads("spm/mixed.fna")[:300].copy()
    wild[[0, 17, 299]] = 254
    for enc in (reads("spm/mixed.fna"), reads("fixtures/Reads1.fna"), wild, np.array([2], dtype=np.uint8)):
        enc = np.ascontiguousarray(enc)
        p = host.gtamd_mirror(enc.ctypes.data, enc.size)
        want = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(2 * enc.size + 1,)).copy()
        free(p)
        assert np.array_equal(spm.mirrored(enc), want) and np.array_equal(sr.mirrored(enc), want)
        assert spm.mirrored(enc).dtype == np.uint8
    # R reads become 2R sequences, number R + j the reverse complement of number R - 1 - j
    enc = reads("spm/mixed.fna")
    both = spm.mirrored(enc)
    units, R = sr.units(both), len(sr.units(enc))
    assert len(units) == 2 * R
    for j in (0, 1, R - 1):
        a, b = units[R + j], units[R - 1 - j]
        assert np.array_equal(both[a[0]:a[0] + a[1]], 3 - both[b[0]:b[0] + b[1]][::-1])


# ---- the definition, on a set worked by hand ----

_CODE = {"a": 0, "c": 1, "g": 2, "t": 3, "n": 254, "|": 255}


def _coded(text):
    return np.array([_CODE[c] for c in text], dtype=np.uint8)


def test_brute_force_on_a_case_worked_by_hand():
    """L = 3.  acgtac ends with tac and with gtac; tacgg and tacna start with tac,
    gtacc with gtac; acgtac overlaps itself by ac only, too short; tacgg occurs
    twice (sequences 1 and 4): four trivial triples of a kind, every one with the
    other copy; ggtac ends with gtac and tac; the suffix a of tacna is cut off by
    the wildcard, its prefix tac is not"""
    enc = _coded("acgtac|tacgg|gtacc|tacna|tacgg|ggtac")
    rows, terminals, starts = sr.brute_force(enc, 3)
    assert sorted(rows[:, :3].tolist()) == sorted([
        [0, 1, 3], [0, 3, 3], [0, 4, 3], [0, 2, 4],
        [5, 1, 3], [5, 3, 3], [5, 4, 3], [5, 2, 4],
        [1, 1, 5], [1, 4, 5], [4, 1, 5], [4, 4, 5]])
    assert starts == 6
    # suffixes of 3 letters or more that end their sequence and stand elsewhere too:
    # tac, gtac (0); cgg, acgg, tacgg (1 and 4); tac, gtac (5)
    assert terminals == 2 + 3 + 3 + 2
    assert sr.sorted_lines(rows)[:2] == ["0 1 3", "0 2 4"]
    assert sr.brute_force(enc, 6)[0].shape == (0, 5)
    # one sequence alone: its whole length occurs once, no trivial triple
    assert sr.brute_force(_coded("acacac"), 2)[0][:, :3].tolist() == [[0, 0, 2], [0, 0, 4]]


# ---- the restatement against the reference's outputs ----

@functools.lru_cache(maxsize=None)
def expected_rows(name, min_len):
    rows = sr.brute_force(sr.mirrored(reads(name)), min_len)[0]
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("key", sorted(GOLDEN["calls"]))
def test_brute_force_reproduces_the_reference(key):
    assert len(GOLDEN["calls"]) == 11
    name, min_len = key.split("|")
    rows, want = expected_rows(name, int(min_len)), GOLDEN["calls"][key]
    text = sr.sorted_text(rows)
    assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key
    assert sr.count_line(rows) == b"number of suffix-prefix matches=%d\n" % want["count"]
    seqlen = [l for _, l in sr.units(sr.mirrored(reads(name)))]
    assert sum(s == t and k == seqlen[s] for s, t, k in rows[:, :3].tolist()) == want["trivial"]
    assert len(set(map(tuple, rows[:, :3].tolist()))) == rows.shape[0]          # no line twice


def test_the_goldens_cover_what_they_are_meant_to():
    calls = GOLDEN["calls"]
    assert {k: calls[k]["lines"] for k in calls if k.startswith("fixtures/")} == {
        "fixtures/Reads1.fna|20": 13088, "fixtures/Reads2.fna|20": 8422, "fixtures/Reads3.fna|20": 12798}
    for name in ("spm/mixed.fna", "spm/equal.fna"):
        mine = sorted((int(k.split("|")[1]), calls[k]) for k in calls if k.startswith(name))
        assert len(mine) >= 3 and mine[0][1]["lines"] - mine[0][1]["trivial"] > 100
        longest = max(l for _, l in sr.units(reads(name)))
        assert mine[-1][0] > longest and mine[-1][1]["lines"] == 0
    assert any(c["trivial"] > 0 for c in calls.values())
    assert len({l for _, l in sr.units(reads("spm/equal.fna"))}) == 1
    assert len({l for _, l in sr.units(reads("spm/mixed.fna"))}) > 20
    assert not (reads("spm/mixed.fna") == 254).any() and not (reads("spm/equal.fna") == 254).any()


def test_text_fixtures_are_those_of_the_json():
    assert len(GOLDEN["texts"]) == 2
    for name, key in GOLDEN["texts"].items():
        raw = open(os.path.join(ou.GOLDEN_DIR, "spm", name), "rb").read()
        want = GOLDEN["calls"][key]
        assert (hashlib.md5(raw).hexdigest(), raw.count(b"\n")) == (want["md5"], want["lines"]) and want["lines"] > 0
        assert raw == sr.sorted_text(expected_rows(key.split("|")[0], int(key.split("|")[1])))


# ---- the tool: what ends before a device is asked for ----

@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """projects without tables, written by the tool's host side: DNA reads, protein"""
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    root = tmp_path_factory.mktemp("spm")
    out = {}
    for kind, name in (("dna", "Reads1.fna"), ("protein", "sw100K1.fsa")):
        out[kind] = str(root / kind)
        subprocess.run([CLI, "-" + kind, "-tis", "-ssp", "-db", ou.fixture_path(name), "-indexname", out[kind]],
                       check=True)
    return out


def _error(*args):
    p = subprocess.run([CLI, "encseq2spm"] + list(args), capture_output=True, text=True)
    prefix = "gt encseq2spm: error: "
    assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith(prefix) and \
        p.stderr.endswith("\n") and p.stderr.count("\n") == 1, (p.returncode, p.stdout, p.stderr)
    return p.stderr[len(prefix):-1]


def test_argument_errors(index):
    idx = index["dna"]
    assert _error("-ii", idx, "-spm", "count") == 'option "-l" is mandatory'
    assert _error("-ii", idx) == 'option "-l" is mandatory'
    assert _error("-l", "20", "-spm", "count") == 'option "-ii" is mandatory'
    assert _error("-ii", idx, "-l") == 'missing argument to option "-l"'
    assert _error("-ii", idx, "-l", "0") == 'argument to option "-l" must be an integer >= 1'
    assert _error("-l", "20", "-ii") == 'missing argument to option "-ii"'
    assert _error("-l", "20", "-ii", idx, "-spm") == 'missing argument to option "-spm"'
    assert _error("-l", "20", "-ii", idx, "-spm", "foo") == 'illegal argument "foo" to option -spm'
    assert _error("-l", "20", "-ii", idx, "-spm", "count", "extra") == "unnecessary arguments"
    assert _error("-l", "20", "-ii", idx, "-nosuch") == "unknown option: -nosuch (-help shows possible options)"


@pytest.mark.parametrize("option", REFUSED)
def test_refused_options(index, option):
    assert _error("-l", "20", "-ii", index["dna"], "-spm", "count", option) == \
        'option "%s" is not supported by the MI355X engine' % option


def test_single_strand_is_answered_as_by_the_reference(index):
    for args in (("-singlestrand",), ("-singlestrand", "yes"), ("-singlestrand", "-spm", "count")):
        assert _error("-l", "20", "-ii", index["dna"], *args) == "option -singlestand is not implemented"


def test_protein_is_refused_with_the_reference_s_message(index):
    for args in ((), ("-spm", "count"), ("-spm", "show")):
        assert _error("-l", "10", "-ii", index["protein"], *args) == \
            "mirroring can only be enabled for DNA sequences, this encoded sequence has alphabet: LVIFKREDAGSTNQYWPHMC"


def test_file_errors_end_before_the_device(index, tmp_path):
    missing = str(tmp_path / "nosuch")
    assert _error("-l", "20", "-ii", missing, "-spm", "count") == "cannot open file '%s.prj'" % missing


def test_without_spm_nothing_is_computed(index):
    """what the reference does after its sort: no output, exit code 0 -- and no device is asked for"""
    p = subprocess.run([CLI, "encseq2spm", "-l", "20", "-ii", index["dna"]], capture_output=True)
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"")
    p = subprocess.run([CLI, "encseq2spm", "-l", "20", "-singlestrand", "no", "-v", "-ii", index["dna"]],
                       capture_output=True)
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"")


def test_other_sub_commands_keep_refusing_spm(index):
    for tool in ("repfind", "querymatch"):
        p = subprocess.run([CLI, tool, "-l", "20", "-ii", index["dna"], "-spm"], capture_output=True, text=True)
        assert p.returncode == 1 and p.stderr == \
            'gt repfind: error: option "-spm" is not supported by the MI355X engine\n'
