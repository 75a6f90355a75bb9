"""CPU-side checks of the index checker's boundary: include/gtamd_check.h is
exported and bound, its host-only entry points work without a device, and
`gt-suffixerator-amd sfxmap` (`gt dev sfxmap`) words its host-only errors."""
import ctypes
import os
import re
import subprocess

import pytest

import oracle_util as ou
from genometools_amd import _lib, check

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_check.h")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")


def _declared_symbols():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gtamd_[a-z_0-9]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) == 7, declared
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.CHECK_ABI[name][1], name
    assert sorted(_lib.CHECK_ABI) == declared
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_check.hip") in _lib.SOURCES


def test_report_structure_matches_the_header():
    """field for field, in order: the names of the C struct are those of the binding"""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = text[text.index("typedef struct {"):text.index("} gtamd_check_report;")]
    names = [n for decl in re.findall(r"\b(?:u?int\d+_t|float)\s+([^;]+);", body)
             for n in re.findall(r"\b([a-z_]+)\b(?:\[\w+\])?", decl)]
    assert names == [n for n, _ in _lib.CheckReport._fields_]
    assert ctypes.sizeof(_lib.CheckReport) == 4 * 4 + 10 * 8 + 4 * 6


def test_geometry_needs_no_device():
    tile, long_claim = check.geometry()
    assert tile >= 256 and tile % 256 == 0       # whole workgroups of 256 lanes
    assert 255 < long_claim < tile


def test_message_of_a_report_needs_no_device():
    lib = _lib.load()
    rep = _lib.CheckReport(ok=0, table=check.LCP, criterion=check.CRIT_LCP_LARGE, index=7, pos_a=3,
                           pos_b=9, claimed=5, found=4)
    buf = ctypes.create_string_buffer(256)
    assert lib.gtamd_check_message(ctypes.byref(rep), buf, 256) == len(buf.value)
    assert buf.value == b"lcp: value at table index 7 (suffixes 3, 9) is 5, too large: the suffixes share 4 symbols"
    rep.ok = 1
    assert lib.gtamd_check_message(ctypes.byref(rep), buf, 256) == 0 and buf.value == b""


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_check_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    with pytest.raises(_lib.EsaError, match="no HIP device"):
        check.EsaChecker()


# ---- the tool: what ends before a device is asked for ----

@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """a project without tables, written by the tool's host side"""
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    idx = str(tmp_path_factory.mktemp("sfxmap") / "at")
    subprocess.run([CLI, "-dna", "-db", ou.fixture_path("Atinsert.fna"), "-indexname", idx], check=True)
    return idx


def _sfxmap(*args):
    p = subprocess.run([CLI, "sfxmap"] + list(args), capture_output=True, text=True)
    assert p.stdout == ""
    return p.returncode, p.stderr


def _error(*args):
    rc, err = _sfxmap(*args)
    assert rc == 1 and err.startswith("gt dev sfxmap: error: ") and err.endswith("\n"), (rc, err)
    return err[len("gt dev sfxmap: error: "):-1]


def test_sfxmap_option_errors(index):
    assert _error() == 'option "-esa" is mandatory'
    assert _error("-suf") == 'option "-esa" is mandatory'
    assert _error("-suf", "-esa") == 'missing argument to option "-esa"'
    assert _error("-suf", "-esa", index, "-frobnicate") == "unknown option: -frobnicate (try -help)"
    assert _error("-suf", "-esa", index, "extra") == 'superfluous argument "extra"'
    for mode in ("-pck", "-stream", "-bfcheck", "-bck", "-wholeleafcheck", "-enumlcpitvs",
                 "-enumlcpitvtree", "-enumlcpitvtreeBU", "-sortmaxdepth", "-compressedesa", "-scanesa",
                 "-spmitv", "-cmpsuf", "-diffcover"):
        assert _error("-suf", mode, "-esa", index) == \
            'option "%s" is not supported by the MI355X engine' % mode
    assert _error("-lcp", "-esa", index).startswith('option "-lcp" requires option "-suf"')
    assert _error("-bwt", "-esa", index).startswith('option "-bwt" requires option "-suf"')


def test_sfxmap_file_errors(index, tmp_path):
    missing = str(tmp_path / "nosuch")
    assert _error("-suf", "-esa", missing) == "cannot open file '%s.prj'" % missing
    assert _error("-suf", "-esa", index) == "cannot open file '%s.suf'" % index
    # without a table option the project file and the sequence are read, nothing else
    assert _sfxmap("-esa", index) == (0, "")
    n = int(dict(l.split("=") for l in open(index + ".prj").read().splitlines())["totallength"])
    with open(index + ".suf", "wb") as f:
        f.write(bytes(8 * (n + 1) - 8))
    assert _error("-suf", "-esa", index) == \
        "file '%s.suf' has %d bytes, %d (-suftabuint) or %d expected for %d entries" % (
            index, 8 * n, 4 * (n + 1), 8 * (n + 1), n + 1)
    with open(index + ".suf", "wb") as f:
        f.write(bytes(4 * (n + 1)))
    with open(index + ".lcp", "wb") as f:
        f.write(bytes(n))
    assert _error("-suf", "-lcp", "-esa", index) == "file '%s.lcp' has %d bytes, %d expected" % (index, n, n + 1)
    with open(index + ".lcp", "wb") as f:
        f.write(bytes(n + 1))
    with open(index + ".llv", "wb") as f:
        f.write(bytes(24))
    assert _error("-suf", "-lcp", "-esa", index) == \
        "file '%s.llv' has 24 bytes, not a multiple of 16 (pairs of two 64-bit numbers)" % index
    for ext in ("suf", "lcp", "llv"):
        os.remove(index + "." + ext)


def test_sfxmap_project_files_it_refuses(index, tmp_path):
    prj = open(index + ".prj").read()
    other = str(tmp_path / "other")
    for ext in ("esq", "ssp"):
        if os.path.exists(index + "." + ext):
            os.symlink(index + "." + ext, other + "." + ext)
    n = int(dict(l.split("=") for l in prj.splitlines())["totallength"])

    def with_prj(text):
        with open(other + ".prj", "w") as f:
            f.write(text)
        return _error("-suf", "-esa", other)
    assert "describes the project of a packed index (numberofallsortedsuffixes=0)" in \
        with_prj(prj.replace("numberofallsortedsuffixes=%d" % (n + 1), "numberofallsortedsuffixes=0"))
    big = (1 << 32) - 4096
    assert with_prj(prj.replace("totallength=%d" % n, "totallength=%d" % big).replace(
        "numberofallsortedsuffixes=%d" % (n + 1), "numberofallsortedsuffixes=%d" % (big + 1))).startswith(
            "sequence of %d symbols is beyond the limit of a single build" % big)
    assert "disagree on the total length" in \
        with_prj(prj.replace("totallength=%d" % n, "totallength=%d" % (n + 1)).replace(
            "numberofallsortedsuffixes=%d" % (n + 1), "numberofallsortedsuffixes=%d" % (n + 2)))
