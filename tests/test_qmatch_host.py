"""CPU-side checks of the query match boundary: include/gtamd_qmatch.h is
exported and bound, its host-only entry point works without a device,
`gt-suffixerator-amd querymatch` words the errors that end before the device as
`gt repfind` does, and the brute-force restatement with its line formatter
(tests/qmatch_reference.py) reproduces, line for line and in order, the result
the reference records for `gt repfind -l 8 -r -ii Duplicate.fna` and every
output of the reference recorded in tests/golden/golden_qmatch.json -- before a
device is involved."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import qmatch_reference as qr
from genometools_amd import _lib, qmatch

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_qmatch.h")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
REFUSED = ["-qii", "-scan", "-spm", "-samples", "-maxfreq", "-seedlength", "-extendxdrop", "-extendgreedy",
           "-xdropbelow", "-minidentity", "-history", "-outfmt", "-evalue"]

with open(os.path.join(ou.GOLDEN_DIR, "golden_qmatch.json")) as _f:
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
        assert getattr(lib, name).argtypes == _lib.QMATCH_ABI[name][1], name
    assert sorted(_lib.QMATCH_ABI) == declared
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_qmatch.hip") in _lib.SOURCES
    assert os.path.join(_lib.HERE, "csrc", "esa_qmatch_core.h") in _lib.HEADERS


def test_info_structure_matches_the_header():
    text = _header_text()
    body = text[text.index("typedef struct {\n  uint64_t positions"):text.index("} gtamd_qmatch_info;")]
    names = re.findall(r"\b(?:u?int\d+_t|float)\s+([a-z_]+);", body)
    assert names == [n for n, _ in _lib.QmatchInfo._fields_]
    assert ctypes.sizeof(_lib.QmatchInfo) == 8 * 8 + 8


def test_geometry_needs_no_device():
    tile, least = qmatch.geometry()
    assert tile >= 64 and tile % 64 == 0          # whole waves
    assert least >= tile and least % tile == 0    # a chunk is whole workgroups


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_qmatch_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    with pytest.raises(_lib.EsaError, match="no HIP device"):
        qmatch.QueryMatches()


def test_value_selects_of_the_kernels_take_scc_from_a_compare(tmp_path):
    """the ISA audit of tests/test_isa_audit.py over the new source"""
    import shutil
    from test_isa_audit import _audit
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    csrc = os.path.join(_lib.HERE, "csrc")
    out = str(tmp_path / "k.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I", csrc,
                    "-o", out, os.path.join(csrc, "esa_qmatch.hip")], check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        asm = f.read()
    assert "k_qm_intervals" in asm and "k_qm_emit" in asm
    bad, after_label = _audit(asm)
    assert not bad and not after_label, "\n".join(bad + after_label)


def test_the_package_transformation_is_the_reference_s():
    query = qr.joined(("Atinsert.fna", "RandomN.fna"))
    for mode in ("fwd", "rev", "rcl"):
        assert np.array_equal(qmatch.transformed(query, mode), qr.transformed(query, mode))
    with pytest.raises(ValueError):
        qmatch.transformed(query, "cpl")


# ---- the definition, on a text worked by hand ----

_CODE = {"a": 0, "c": 1, "g": 2, "t": 3, "n": 254, "|": 255}
SUBJECT = "acgtcnttgca|ggatccaagtctagctacaagt"
QUERY = "acgtg|cttgcat|gt|atgcac|tcaagta|aggat"


def _coded(text):
    return np.array([_CODE[c] for c in text], dtype=np.uint8)


def test_brute_force_on_a_case_worked_by_hand():
    """L = 4.  In query order: acgt at p = 0 and i = 0; ttgca behind the
    wildcard, up to the separator (tgca inside it is not left-maximal); tgca up
    to the separator again; caagt twice, the occurrence that ends at n behind the
    one followed by c (the end sorts behind every letter); ggat up to the query's
    end; the unit gt is shorter than L"""
    enc, query = _coded(SUBJECT), _coded(QUERY)
    suf = ou.esa(enc, 4)["suf"]
    rec = qr.expected(enc, suf, query, 4)
    assert rec.tolist() == [[0, 0, 4], [6, 7, 5], [7, 18, 4], [17, 25, 5], [29, 25, 5], [12, 33, 4]]
    assert rec[4, 0] + rec[4, 2] == enc.size and rec[5, 1] + rec[5, 2] == query.size
    assert qr.tool_lines(enc, suf, query, 4, ("fwd",)) == [
        "4 0 0 F 4 0 0", "5 0 6 F 5 1 1", "4 0 7 F 4 3 1", "5 1 5 F 5 4 1", "5 1 17 F 5 4 1", "4 1 0 F 4 5 1"]
    # gtgca, tacgttc and cacgta read backwards: the start on the forward strand
    assert qr.tool_lines(enc, suf, query, 4, ("rev",)) == ["4 0 7 R 4 0 0", "4 0 0 R 4 1 2", "4 0 0 R 4 3 1"]
    assert qr.expected(enc, suf, query, 6).shape == (0, 3)
    # (acgt)' = acgt: the reverse complement of unit 0, cacgt, holds it
    assert qr.tool_lines(enc, suf, query, 4, ("rcl",))[0] == "4 0 0 P 4 0 0"


# ---- the restatement against the reference's outputs ----

def _call(key):
    subject, alphabet, args, queries = key.split("|")
    args = args.split()
    # -f is on unless -r or -p is given without it (gt_repfind_arguments_check)
    fwd = "-f" in args or not ("-r" in args or "-p" in args)
    modes = tuple(m for m, on in (("fwd", fwd), ("rev", "-r" in args), ("rcl", "-p" in args)) if on)
    return subject, alphabet == "protein", int(args[args.index("-l") + 1]), modes, \
        tuple(queries.split(",")) if queries else ()


def expected_text(key):
    subject, protein, min_len, modes, queries = _call(key)
    return "".join(l + "\n" for l in qr.call_lines(subject, queries, min_len, modes, protein)).encode("latin-1")


def test_brute_force_gives_the_result_the_reference_records():
    with open(os.path.join(ou.GOLDEN_DIR, "repfind", "Duplicate.fna-r.result"), "rb") as f:
        want = qr.normalised(f.read())
    assert len(want) == 64
    assert qr.call_lines("Duplicate.fna", (), 8, ("rev",)) == want


SUBJECTS = sorted({k.split("|")[0] for k in GOLDEN["calls"]})


@pytest.mark.parametrize("subject", SUBJECTS)
def test_brute_force_and_formatter_reproduce_the_reference(subject):
    assert len(GOLDEN["calls"]) == 65 and len(SUBJECTS) == 6
    calls = [k for k in sorted(GOLDEN["calls"]) if k.split("|")[0] == subject]
    assert len(calls) in (4, 12, 13)
    for key in calls:
        text, want = expected_text(key), GOLDEN["calls"][key]
        assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key


def test_the_goldens_cover_every_mode():
    most = {}
    for key, entry in GOLDEN["calls"].items():
        subject, protein, _, modes, queries = _call(key)
        if len(modes) == 1:
            kind = "protein" if protein else ("" if queries else "self-") + modes[0]
            most[kind] = max(most.get(kind, 0), entry["lines"])
    assert sorted(most) == ["fwd", "protein", "rcl", "rev", "self-rcl", "self-rev"]
    assert all(v > 100 for v in most.values()), most
    assert any(e["lines"] == 0 for e in GOLDEN["calls"].values())


def test_text_fixtures_are_those_of_the_json():
    assert len(GOLDEN["texts"]) == 3
    assert sorted(_call(k)[3] for k in GOLDEN["texts"].values()) == [("fwd",), ("rcl",), ("rev",)]
    for name, key in GOLDEN["texts"].items():
        raw = open(os.path.join(ou.GOLDEN_DIR, "qmatch", name), "rb").read()
        want = GOLDEN["calls"][key]
        assert (hashlib.md5(raw).hexdigest(), raw.count(b"\n")) == (want["md5"], want["lines"]) and want["lines"] > 0
        assert raw == expected_text(key)


# ---- the tool: what ends before a device is asked for ----

@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """projects without tables, written by the tool's host side: DNA, protein"""
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    root = tmp_path_factory.mktemp("qmatch")
    out = {}
    for kind, name in (("dna", "Atinsert.fna"), ("protein", "sw100K1.fsa")):
        out[kind] = str(root / kind)
        subprocess.run([CLI, "-" + kind, "-db", ou.fixture_path(name), "-indexname", out[kind]], check=True)
    return out


def _error(*args):
    p = subprocess.run([CLI, "querymatch"] + list(args), capture_output=True, text=True)
    prefix = "gt repfind: error: "
    assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith(prefix) and \
        p.stderr.endswith("\n") and p.stderr.count("\n") == 1, (p.returncode, p.stdout, p.stderr)
    return p.stderr[len(prefix):-1]


def test_argument_errors(index):
    idx, q = index["dna"], ou.fixture_path("Random159.fna")
    assert _error("-l", "8", "-q", q) == 'option "-ii" is mandatory'
    assert _error("-ii", idx, "-q", q, "-l") == 'missing argument to option "-l"'
    assert _error("-ii", idx, "-q", q, "-l", "0") == 'argument to option "-l" must be an integer >= 1'
    assert _error("-ii", idx, "-l", "8", "-q") == 'missing argument to option "-q"'
    assert _error("-ii", idx, "-l", "8", "-q", "-r") == 'missing argument to option "-q"'
    assert _error("-ii") == 'missing argument to option "-ii"'
    assert _error("-ii", idx, "-r", "extra") == 'superfluous arguments: "extra"'
    assert _error("-ii", idx, "-r", "-nosuch").startswith("unknown option: -nosuch")
    for option in REFUSED:
        assert _error("-ii", idx, "-l", "8", "-q", q, option) == \
            'option "%s" is not supported by the MI355X engine' % option


def test_forward_repeats_of_the_index_belong_to_repfind(index):
    for args in ((), ("-f",), ("-f", "-r"), ("-l", "8")):
        msg = _error("-ii", index["dna"], *args)
        assert "repfind" in msg and "sub-command" in msg, msg


def test_file_errors_end_before_the_device(index, tmp_path):
    idx, q = index["dna"], ou.fixture_path("Random159.fna")
    missing = str(tmp_path / "nosuch")
    assert _error("-ii", missing, "-r") == "cannot open file '%s.prj'" % missing
    # the project has no tables
    assert _error("-ii", idx, "-l", "8", "-q", q) == \
        'cannot open file "%s.suf": No such file or directory' % idx
    n = int(dict(l.split("=") for l in open(idx + ".prj").read().splitlines())["totallength"])
    with open(idx + ".suf", "wb") as f:
        f.write(bytes(8 * (n + 1)))
    try:
        # the queries are read with the index's alphabet: a protein file is no DNA
        msg = _error("-ii", idx, "-l", "8", "-q", ou.fixture_path("sw100K1.fsa"))
        assert msg.startswith("illegal character '") and "sw100K1.fsa" in msg
        noquery = str(tmp_path / "noquery")
        assert _error("-ii", idx, "-l", "8", "-q", noquery) == "cannot open file '%s'" % noquery
        with open(idx + ".suf", "ab") as f:
            f.write(b"\0")
        assert "-suftabuint" in _error("-ii", idx, "-l", "8", "-q", q)
    finally:
        os.remove(idx + ".suf")


def test_reverse_complement_needs_dna(index):
    msg = _error("-ii", index["protein"], "-l", "6", "-p", "-q", ou.fixture_path("sw100K2.fsa"))
    assert '"-p"' in msg and "DNA" in msg
    assert '"-p"' in _error("-ii", index["protein"], "-f", "-p", "-q", ou.fixture_path("sw100K2.fsa"))
