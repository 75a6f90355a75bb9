"""`gt-suffixerator-amd sfxmap -suf -lcp -bwt -esa INDEX` (`gt dev sfxmap`) on
indexes this tool wrote and on indexes the reference wrote
(oracle/_ref/gt_ref_sfx), intact and damaged; the verdicts on the damaged ones
are those of the reference's own checkers (oracle/_ref/gt_ref_check)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_util as ou
from check_criteria import first_suf_failure
from genometools_amd import _lib, check

pytestmark = pytest.mark.gpu

GOLDEN = ou.golden()
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
REF_CHECK = os.path.join(ou.ORACLE_DIR, "_ref", "gt_ref_check")
ALL = ["-suf", "-lcp", "-bwt"]


@pytest.fixture(scope="module")
def cli(gpu):
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    return CLI


def _sfxmap(cli, idx, tables=ALL, extra=()):
    return subprocess.run([cli, "sfxmap"] + list(tables) + list(extra) + ["-esa", idx],
                          capture_output=True, text=True)


def _rejected(cli, idx, tables=ALL):
    p = _sfxmap(cli, idx, tables)
    assert p.returncode == 1 and p.stdout == "", (p.returncode, p.stdout, p.stderr)
    start = "gt dev sfxmap: error: index '%s': " % idx
    assert p.stderr.startswith(start) and p.stderr.endswith("\n"), p.stderr
    return p.stderr[len(start):-1]


def _build(cli, name, idx, extra=()):
    src = ou.fixture_path(name)
    subprocess.run([cli, "-" + GOLDEN[name]["alphabet"], "-suf", "-lcp", "-bwt", "-indexname", idx, "-db",
                    os.path.basename(src)] + list(extra), check=True, cwd=os.path.dirname(src))


@pytest.mark.parametrize("name,extra", [
    ("Atinsert.fna", []), ("Duplicate.fna", []), ("RandomN.fna", []), ("sw100K1.fsa", []),
    ("Atinsert.fna", ["-suftabuint"]), ("sw100K1.fsa", ["-suftabuint"]),
    ("Atinsert.fna", ["-dir", "rcl"]), ("RandomN.fna", ["-dir", "rev"]), ("Duplicate.fna", ["-mirrored"]),
    ("Duplicate.fna", ["-mirrored", "-dir", "cpl", "-suftabuint"]),
])
def test_sfxmap_accepts_our_index(cli, name, extra, tmp_path):
    idx = str(tmp_path / "idx")
    _build(cli, name, idx, extra)
    p = _sfxmap(cli, idx)
    assert (p.returncode, p.stdout, p.stderr) == (0, "", "")          # success is silent
    p = _sfxmap(cli, idx, extra=["-v"])
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and p.stderr == "" and len(lines) == 6, p.stdout
    assert all(l.startswith("# ") and " ms" in l for l in lines) and lines[-1].startswith("# total")
    for tables in (["-suf"], ["-suf", "-bwt"], ["-suf", "-lcp"]):
        p = _sfxmap(cli, idx, tables)
        assert (p.returncode, p.stdout, p.stderr) == (0, "", ""), tables


@pytest.mark.parametrize("name", ["Atinsert.fna", "sw100K1.fsa", "RandomN.fna"])
def test_sfxmap_accepts_an_index_the_reference_wrote(cli, name, tmp_path):
    assert os.path.exists(ou.REF_BIN), "build oracle/_ref first (python -c 'import __graft_entry__ as g; g.build()')"
    idx = str(tmp_path / "ref")
    subprocess.run([ou.REF_BIN, "-" + GOLDEN[name]["alphabet"], "-suf", "-lcp", "-bwt", "-db",
                    ou.fixture_path(name), "-indexname", idx], check=True)
    p = _sfxmap(cli, idx)
    assert (p.returncode, p.stdout, p.stderr) == (0, "", "")


def _reference_accepts(idx):
    assert os.path.exists(REF_CHECK), "build oracle/_ref first (python -c 'import __graft_entry__ as g; g.build()')"
    return subprocess.run([REF_CHECK, idx], capture_output=True, text=True).returncode == 0


def test_sfxmap_rejects_what_the_reference_checker_rejects(cli, tmp_path):
    """the two damages of test_cli_gpu.py::test_reference_checker_rejects_a_damaged_index"""
    idx = str(tmp_path / "idx")
    _build(cli, "Atinsert.fna", idx)
    assert _reference_accepts(idx) and _sfxmap(cli, idx).returncode == 0
    enc = ou.encode_fasta(ou.fixture_path("Atinsert.fna"))
    good = {ext: open(idx + "." + ext, "rb").read() for ext in ("suf", "lcp", "llv", "prj")}

    def restore():
        for ext, raw in good.items():
            with open(idx + "." + ext, "wb") as f:
                f.write(raw)
    # one wrong LCP value: the low bit of byte 1000
    lcp = bytearray(good["lcp"])
    lcp[1000] ^= 1
    open(idx + ".lcp", "wb").write(bytes(lcp))
    assert not _reference_accepts(idx)
    msg = _rejected(cli, idx)
    suf = np.frombuffer(good["suf"], dtype=np.uint64)
    assert msg.startswith("lcp: value at table index 1000 (suffixes %d, %d) is %d, too %s: the suffixes share %d "
                          % (suf[999], suf[1000], lcp[1000], "large" if lcp[1000] & 1 else "small",
                             good["lcp"][1000])), msg
    assert _sfxmap(cli, idx, ["-suf", "-bwt"]).returncode == 0       # (the other tables are intact)
    restore()
    # one swapped pair of suffixes
    bad = suf.copy()
    bad[[500, 501]] = suf[[501, 500]]
    open(idx + ".suf", "wb").write(bad.tobytes())
    assert not _reference_accepts(idx)
    crit, index = first_suf_failure(enc, bad)
    assert crit == check.CRIT_ORDER and index <= 501
    for tables in (ALL, ["-suf"]):
        msg = _rejected(cli, idx, tables)
        assert msg == "suf: suffixes out of order at table index %d (suffixes %d, %d)" % (
            index, bad[index - 1], bad[index]), msg
    restore()
    # the project file: longest, and the two LCP statistics
    prj = good["prj"].decode()
    values = dict(l.split("=") for l in prj.splitlines())
    for key, words in (("longest", "says longest=%d, suffix 0 stands at table index %s"),
                       ("largelcpvalues", "says largelcpvalues=%d, the .lcp table holds %s"),
                       ("maxbranchdepth", "says maxbranchdepth=%d, the largest value of the tables is %s")):
        wrong = int(values[key]) + 1
        open(idx + ".prj", "w").write(prj.replace("%s=%s\n" % (key, values[key]), "%s=%d\n" % (key, wrong)))
        p = _sfxmap(cli, idx)
        assert p.returncode == 1 and p.stderr == "gt dev sfxmap: error: file '%s.prj' %s\n" % (
            idx, words % (wrong, values[key])), p.stderr
        if key != "longest":
            assert _sfxmap(cli, idx, ["-suf", "-bwt"]).returncode == 0   # (-lcp checks them)
    restore()
    assert _sfxmap(cli, idx).returncode == 0


def test_sfxmap_rejects_a_truncated_llv(cli, tmp_path):
    """the last pair gone, and half gone (Duplicate.fna: 586 pairs)"""
    idx = str(tmp_path / "idx")
    _build(cli, "Duplicate.fna", idx)
    assert _sfxmap(cli, idx).returncode == 0
    raw = open(idx + ".llv", "rb").read()
    llv = np.frombuffer(raw, dtype=np.uint64).reshape(-1, 2)
    assert len(llv) >= 2
    open(idx + ".llv", "wb").write(raw[:-16])
    assert _rejected(cli, idx) == "llv: %d lcp bytes of 255, %d .llv entries: none for table index %d" % (
        len(llv), len(llv) - 1, llv[-1, 0])
    assert _sfxmap(cli, idx, ["-suf", "-bwt"]).returncode == 0
    open(idx + ".llv", "wb").write(raw[:-8])
    p = _sfxmap(cli, idx)
    assert p.returncode == 1 and p.stderr == "gt dev sfxmap: error: file '%s.llv' has %d bytes, not a multiple " \
        "of 16 (pairs of two 64-bit numbers)\n" % (idx, len(raw) - 8)


def test_sfxmap_wrong_sequence_is_rejected(cli, tmp_path):
    """the tables of one sequence beside the encoded sequence of another of the same length"""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _build(cli, "Atinsert.fna", a)
    _build(cli, "Atinsert.fna", b, ["-dir", "rev"])
    for ext in ("suf", "lcp", "llv", "bwt"):
        shutil.copy(b + "." + ext, a + "." + ext)
    assert _rejected(cli, a).startswith("suf: ")
