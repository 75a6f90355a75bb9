"""`gt-suffixerator-amd readjoiner prefilter` without a device: the option parser,
the refusals and -help; and what the tool writes from figures and symbols in
host memory -- the file table and the raw-length words of X.esq, X.esq itself
and X.cnt -- against the reference's files recorded in
tests/golden/golden_prefilter.json, with the kept reads and the figures per
file given by the brute force of tests/prefilter_reference.py."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import prefilter_reference as pr
import spm_reference as sr
from genometools_amd import _lib

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
HOST_LIB = os.path.join(_lib.HERE, "libgtamd_host.so")
DATA = os.path.join(ou.GOLDEN_DIR, "prefilter")

with open(os.path.join(ou.GOLDEN_DIR, "golden_prefilter.json")) as _f:
    GOLDEN = json.load(_f)


class PrefilterFile(ctypes.Structure):      # gtamd_prefilter_file, csrc/host/host_internal.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("filesize", "invalid_reads", "invalid_letters", "kept_reads", "kept_letters")]


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(HOST_LIB)
    P = ctypes.c_void_p
    lib.gtamd_prefilter_filetable.argtypes = [P, ctypes.c_size_t, P]
    lib.gtamd_prefilter_filetable.restype = None
    lib.gtamd_prefilter_write_readset.argtypes = [ctypes.c_char_p, P, ctypes.c_size_t, P, P, ctypes.c_uint64,
                                                  ctypes.c_char_p, ctypes.c_size_t]
    lib.gtamd_prefilter_write_cntlist.argtypes = [ctypes.c_char_p, P, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    return lib


def _error(*args):
    p = subprocess.run([CLI, "readjoiner", "prefilter"] + list(args), capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith("gt readjoiner prefilter: error: ")
    return p.stderr[len("gt readjoiner prefilter: error: "):].rstrip("\n")


def test_help_needs_no_device():
    p = subprocess.run([CLI, "readjoiner", "prefilter", "-help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout.startswith("Usage: gt-suffixerator-amd readjoiner prefilter -db FILE...")
    for word in ("-readset", "-encodeonly", "-fasta", "-cnt", "-strict", "-q ", "-v ", "X.rlt", "-libtable is refused",
                 "differs from run to run", "follows the definition"):
        assert word in p.stdout, word


def test_the_parser_s_refusals():
    assert _error("-q") == 'option "-db" is mandatory'
    assert _error("-readset", "X") == 'option "-db" is mandatory'
    assert _error("-db") == 'missing argument to option "-db"'
    assert _error("-db", "a.fna", "-readset") == 'missing argument to option "-readset"'
    assert _error("-db", "a.fna", "-v", "-q") == 'option "-v" and option "-q" exclude each other'
    assert _error("-db", "a.fna", "-cnt", "-encodeonly") == 'option "-encodeonly" and option "-cnt" exclude each other'
    assert _error("-db", "a.fna", "-nosuch") == "unknown option: -nosuch (-help shows possible options)"
    assert _error("-db", "a.fna", "-q", "word") == "unnecessary arguments"
    assert "library 'a.fna:300' is a paired one" in _error("-db", "a.fna:300")
    assert "library 'f.fq:r.fq:300,20' is a paired one" in _error("-db", "a.fna", "f.fq:r.fq:300,20", "-q")
    # a switch takes yes|no: `-v no -q` is no conflict, and ends at the file that is not there
    assert _error("-db", "/nonexistent/a.fna", "-v", "no", "-q") == "cannot open file '/nonexistent/a.fna'"


@pytest.mark.parametrize("option", ["-singlestrand", "-maxlow", "-lowqual", "-phred64", "-des", "-clipdes", "-memdes",
                                    "-copynum", "-seqnums", "-encseq", "-libtable", "-testrs", "-testrs-print",
                                    "-testrs-depth", "-testrs-maxdepth"])
def test_options_refused_by_name(option):
    assert _error("-db", "a.fna", option) == 'option "%s" is not supported by the MI355X engine' % option


def test_the_command_without_a_tool_s_options_answers_as_before():
    """`readjoiner`, another tool's name, and the bare `readjoiner prefilter` keep the dispatcher's words"""
    for args in (["readjoiner"], ["readjoiner", "assembly"], ["readjoiner", "prefilter"]):
        p = subprocess.run([CLI] + args, capture_output=True, text=True)
        assert (p.returncode, p.stdout, p.stderr) == (1, "", "gt readjoiner: error: tool overlap expected\n")


def _figures(name, encodeonly=False):
    """(files, the tool's figures per file, kept reads, removed flags of the valid reads) by the brute force"""
    files = GOLDEN["equal"][name]["files"]
    paths = [os.path.join(DATA, f) for f in files]
    figures, valid = pr.file_figures(paths)
    reads = [r for r, _ in valid]
    v = pr.verdicts(reads)
    gone = np.zeros(len(reads), dtype=bool) if encodeonly else (pr.DEFAULT_MASK >> v & 1).astype(bool)
    tab = (PrefilterFile * len(files))()
    for f, fig in enumerate(figures):
        mine = [r for (r, at), g in zip(valid, gone.tolist()) if at == f and not g]
        tab[f] = PrefilterFile(fig["filesize"], fig["invalid_reads"], fig["invalid_letters"], len(mine),
                               sum(r.size for r in mine))
    return files, tab, [r for r, g in zip(reads, gone.tolist()) if not g], gone


def test_the_file_table_worked_out(host):
    """36-letter reads: 31 and 27 in two files, of which 2 and 1 hold a wildcard and 20 and 12 are left"""
    tab = (PrefilterFile * 3)(PrefilterFile(1500, 2, 72, 20, 720), PrefilterFile(2300, 1, 36, 12, 432),
                              PrefilterFile(40, 0, 0, 0, 0))
    out = np.zeros(6, dtype=np.uint64)
    host.gtamd_prefilter_filetable(tab, 3, out.ctypes.data)
    assert out.tolist() == [1500 - 72 - 6, 37 * 20 - 1, 2300 - 36 - 3, 37 * 12 - 1, 40, 2 ** 64 - 1]


@pytest.mark.parametrize("name", sorted(GOLDEN["equal"]))
def test_readset_and_list_are_the_reference_s(host, name, tmp_path):
    golden = GOLDEN["equal"][name]
    err = ctypes.create_string_buffer(1024)
    for encodeonly in (False, True):
        files, tab, kept, gone = _figures(name, encodeonly)
        assert len(kept) == (sum(f.kept_reads for f in tab))
        enc = np.ascontiguousarray(sr.joined(kept))
        names = (ctypes.c_char_p * len(files))(*[f.encode() for f in files])
        readset = str(tmp_path / name)
        rc = host.gtamd_prefilter_write_readset(readset.encode(), names, len(files), tab, enc.ctypes.data, enc.size, err,
                                                len(err))
        assert rc == 0, err.value
        raw = open(readset + ".esq", "rb").read()
        want = golden["esq_encodeonly" if encodeonly else "esq"]
        assert (len(raw), hashlib.md5(raw).hexdigest()) == (want["size"], want["md5"])
        assert not os.path.exists(readset + ".ssp")
        # and the project's reader gives the symbols back
        back = ou.lib() and _read_esq(readset)
        assert np.array_equal(back, enc)
    files, tab, kept, gone = _figures(name)
    assert len(kept) == golden["kept"]
    flags = np.ascontiguousarray(gone, dtype=np.uint8)
    path = str(tmp_path / (name + ".cnt"))
    assert host.gtamd_prefilter_write_cntlist(path.encode(), flags.ctypes.data, flags.size, err, len(err)) == 0
    raw = open(path, "rb").read()
    assert raw == pr.cntlist(gone)
    assert (len(raw), hashlib.md5(raw).hexdigest()) == (golden["cnt"]["size"], golden["cnt"]["md5"])
    raw = pr.p_fas(kept)
    assert (len(raw), hashlib.md5(raw).hexdigest()) == (golden["p.fas"]["size"], golden["p.fas"]["md5"])


def _read_esq(readset):
    lib = ctypes.CDLL(HOST_LIB)
    enc, n, protein = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64(), ctypes.c_int()
    err = ctypes.create_string_buffer(1024)
    lib.gtamd_read_esq.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_char_p, ctypes.c_size_t]
    assert lib.gtamd_read_esq(readset.encode(), ctypes.byref(enc), ctypes.byref(n), ctypes.byref(protein), None, err,
                              len(err)) == 0, err.value
    out = np.ctypeslib.as_array(enc, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.uint8)
    ctypes.CDLL(None).free(enc)
    return out


def test_the_expected_lines_are_the_reference_s():
    """the writer of tests/prefilter_reference.py, which the tests of the tool compare with on sets of several
    lengths, words the reference's lines: every recorded stdout"""
    cwd = os.getcwd()
    os.chdir(DATA)
    try:
        for name, golden in GOLDEN["equal"].items():
            assert pr.expected_stdout(name, golden["files"]).decode() == golden["stdout"], name
            assert pr.expected_stdout(name, golden["files"], "verbose", fasta=True, cnt=True).decode() == \
                golden["stdout_v"], name
            assert pr.expected_stdout(name, golden["files"], "encodeonly").decode() == golden["stdout_encodeonly"], name
    finally:
        os.chdir(cwd)


def test_the_reference_departs_on_reads_of_several_lengths():
    """what the golden file documents: the reference keeps reads the definition removes"""
    for name, golden in GOLDEN["variable"].items():
        reads = pr.parse_reads(os.path.join(DATA, golden["files"][0]))
        kept = pr.kept_reads(reads, pr.verdicts(reads))
        assert len(kept) == golden["definition_keeps"] == golden["reference_keeps"] - golden["more"]
        assert golden["more"] > 0
