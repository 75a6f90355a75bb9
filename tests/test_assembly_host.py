"""The host code of `gt-suffixerator-amd assembly` without a device: the option
parser, every refusal by name, the dispatcher's unchanged answer to `readjoiner
assembly`, the reader of Readjoiner's bin32 list on hand-made and damaged lists,
and the statistics block on hand-made lists of lengths -- in the tool and, under
AddressSanitizer and UBSan, in a stand-alone program
(tests/assembly_san_driver.c) that never asks for a device, over the golden
lists and their truncations."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import assembly_golden as ag
import oracle_util as ou
import strgraph_reference as sg
from genometools_amd import _lib, strgraph

ROOT = ou.ROOT
HEADER = os.path.join(ROOT, "include", "gtamd_strgraph.h")
HOST_DIR = os.path.join(_lib.HERE, "csrc", "host")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
DRIVER_SRC = os.path.join(ROOT, "tests", "assembly_san_driver.c")
REFUSED = ["-redtrans", "-errors", "-bubble", "-deadend", "-deadend-depth", "-paths2seq", "-buffersize", "-vd", "-astat",
           "-cov", "-copynum", "-load", "-save", "-cinfo", "-v"]
# the flags of tests/test_host_sanitized.py
STD_FLAGS = ["-Wall", "-Wextra", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-D_DEFAULT_SOURCE",
             "-I" + os.path.join(ROOT, "include"), "-I" + HOST_DIR]
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"]
HOST_FILES = tuple(sorted(f for f in os.listdir(HOST_DIR) if f.endswith(".c") and f != "suffixerator_main.c"))
PREFIX = "gt readjoiner assembly: error: "


def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_every_declared_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(gtamd_strgraph_[a-z_0-9]+)\s*\(", _header_text())))
    assert len(declared) == 9, declared
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.STRGRAPH_ABI[name][1], name
    assert sorted(_lib.STRGRAPH_ABI) == declared
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_strgraph.hip") in _lib.SOURCES
    assert os.path.join(_lib.HERE, "csrc", "esa_strgraph_core.h") in _lib.HEADERS


def test_info_structure_and_defaults_match_the_header():
    text = _header_text()
    end = text.index("} gtamd_strgraph_info;")
    body = text[text.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == [n for n, _ in _lib.StrgraphInfo._fields_]
    assert ctypes.sizeof(_lib.StrgraphInfo) == 14 * 8 + 2 * 4 + 6 * 4
    cut = dict(re.findall(r"#define GTAMD_STRGRAPH_([A-Z]+)\s+(\d+)u", text))
    assert (int(cut["DEPTHCUTOFF"]), int(cut["LENGTHCUTOFF"])) == (strgraph.DEPTHCUTOFF, strgraph.LENGTHCUTOFF) == \
        (sg.DEPTHCUTOFF, sg.LENGTHCUTOFF)
    assert strgraph.geometry() == (256, 4096, 256)


RULE_WORDS = {
    "min_len": "len >= L", "self_match": "no match of a read with itself", "edge_cases": "suffix direct, prefix reverse",
    "edge_length": "length of its destination read minus len", "insertion_order": "INSERTION ORDER",
    "internal": "are both 1", "orientation": "the one with the smaller start is written", "hairpin_tie": "the smaller j is written",
    "single_edge_marks": "skipped when t < i", "cycle_start": "starts and ends there", "cycles_last": "come last",
    "strand": "a B vertex its reverse", "depth": "number of\n  vertices", "cutoffs": "depth >=\n  depthcutoff and length >= lengthcutoff",
    "numbering": "numbered in the order of the paths"}


def test_the_header_words_every_rule_the_restatement_names():
    """a list of words only: that a broken rule is noticed is what
    tests/test_assembly_reference.py::test_every_rule_is_pinned holds"""
    with open(HEADER) as f:
        text = f.read()
    assert sorted(RULE_WORDS) == sorted(sg.RULES)
    for rule, words in RULE_WORDS.items():
        assert words in text, rule


# ---- the tool: what ends before a device is asked for ----

@pytest.fixture(scope="module")
def readset(tmp_path_factory):
    """a readset as the tool's host side writes it, with a copy of the golden list beside it"""
    subprocess.run(["make", "-C", HOST_DIR], check=True, stdout=subprocess.DEVNULL)
    root = tmp_path_factory.mktemp("assembly")
    idx = str(root / "rep3")
    subprocess.run([CLI, "-dna", "-tis", "-ssp", "-db", os.path.join(ag.DIR, "rep3.p.fas"), "-indexname", idx], check=True,
                   stdout=subprocess.DEVNULL)
    return idx


def _error(*args):
    """(message, stdout) of the tool itself"""
    p = subprocess.run([CLI, "assembly"] + list(args), capture_output=True, text=True)
    assert p.returncode == 1 and p.stderr.startswith(PREFIX) and p.stderr.endswith("\n") and p.stderr.count("\n") == 1, \
        (p.returncode, p.stdout, p.stderr)
    return p.stderr[len(PREFIX):-1], p.stdout


def test_help_and_the_words_readjoiner_assembly(readset):
    p = subprocess.run([CLI, "assembly", "-help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("Usage: gt-suffixerator-amd assembly -readset X") and p.stderr == ""
    assert "X.paths" in p.stdout and "not written" in p.stdout
    for args in (["readjoiner", "assembly"], ["readjoiner", "assembly", "-readset", readset]):
        p = subprocess.run([CLI] + args, capture_output=True, text=True)
        assert (p.returncode, p.stdout, p.stderr) == (1, "", "gt readjoiner: error: tool overlap expected\n")


def test_option_parser(readset):
    assert _error() == ('option "-readset" is mandatory', "")
    assert _error("-readset") == ('missing argument to option "-readset"', "")
    assert _error("-l", "30") == ('option "-readset" is mandatory', "")
    for name, least in (("-l", 2), ("-depthcutoff", 1), ("-lengthcutoff", 1), ("-spmfiles", 1)):
        assert _error("-readset", readset, name) == ('missing argument to option "%s"' % name, "")
        assert _error("-readset", readset, name, "x") == ('argument to option "%s" must be a non-negative integer' % name, "")
        assert _error("-readset", readset, name, str(least - 1)) == \
            ('argument to option "%s" must be an integer >= %d' % (name, least), "")
    assert _error("-readset", readset, "-nosuch") == ("unknown option: -nosuch (-help shows possible options)", "")
    assert _error("-readset", readset, "word") == ("unnecessary arguments", "")


@pytest.mark.parametrize("name", REFUSED)
def test_every_other_option_of_the_reference_is_refused_by_name(readset, name):
    assert _error("-readset", readset, name) == ('option "%s" is not supported by the MI355X engine' % name, "")


def test_more_than_one_list_is_refused(readset):
    message, out = _error("-readset", readset, "-spmfiles", "2")
    assert message.startswith('option "-spmfiles" above 1 is not supported by the MI355X engine') and out == ""


def test_files_that_are_not_there(readset, tmp_path):
    opening = "# gt readjoiner assembly (version 1.2)\n"
    assert _error("-readset", str(tmp_path / "none")) == ("cannot open file '%s.esq'" % (tmp_path / "none"), opening)
    message, out = _error("-readset", readset)
    assert message == "cannot open file '%s.0.spm'" % readset
    assert out == opening + "# number of reads in filtered readset = %d\n# calculate edges space for each vertex\n" \
        % ag.GOLDEN["rep3"]["reads"]
    assert _error("-readset", readset, "-q")[1] == ""


def _list(records):
    return b"\x02" + b"".join(struct.pack("<III", a, b, k << 2 | f) for a, b, k, f in records)


def test_damaged_lists_are_refused_by_the_tool(readset):
    """each with a message of its own, before a device is asked for"""
    good = [(0, 1, 25, 3), (2, 1, 30, 2)]
    cases = [(b"", "is empty"), (b"\x03" + _list(good)[1:], "starts with byte 3"), (_list(good)[:-1], "is truncated: 23 bytes"),
             (_list(good)[:2], "is truncated: 1 bytes"), (_list(good + [(0, 99999, 25, 3)]), "match 2 names read 99999"),
             (_list([(0, 1, 41, 3)]), "match 0 of reads 0 and 1 has 41 letters"), (_list([(0, 1, 25, 0)]), "both reads reversed")]
    for raw, words in cases:
        with open(readset + ".0.spm", "wb") as f:
            f.write(raw)
        message, _ = _error("-readset", readset, "-q")
        assert words in message and (readset + ".0.spm") in message, (words, message)
    os.remove(readset + ".0.spm")


# ---- the same code under the sanitizers, in a program of its own ----

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/assembly_san_driver.c with every file of the host layer, all under the sanitizers, linked against the
    ordinary libgtamd_esa.so, which is loaded and never asked for a device"""
    out = tmp_path_factory.mktemp("assemblysan")
    probe = out / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc"] + SAN_FLAGS + ["-o", str(out / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("gcc cannot build a program with -fsanitize=address,undefined -static-libasan here: " + p.stderr[-300:])
    jobs = []
    for src in [os.path.join(HOST_DIR, f) for f in HOST_FILES] + [DRIVER_SRC]:
        obj = str(out / (os.path.basename(src) + ".o"))
        jobs.append((obj, subprocess.Popen(["gcc"] + SAN_FLAGS + STD_FLAGS + ["-c", "-o", obj, src],
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    logs = [(proc.communicate()[0], proc.returncode) for _, proc in jobs]
    assert all(rc == 0 for _, rc in logs), "".join(text for text, _ in logs)
    exe = str(out / "assembly_san_driver")
    subprocess.run(["gcc"] + SAN_FLAGS + ["-o", exe] + [obj for obj, _ in jobs] +
                   ["-L" + _lib.HERE, "-lgtamd_esa", "-lpthread", "-lz", "-ldl", "-Wl,-rpath," + _lib.HERE], check=True)
    return exe


def _san_env():
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "allocator_may_return_null=1:detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    return env


def _driven(driver, *args):
    """(rc, message, stdout before the last line) of the sanitized program; no report, no leak"""
    p = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, env=_san_env())
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    rc, _, message = lines[-1].partition("\t")
    return int(rc), message, lines[:-1]


def test_the_sanitizers_are_awake(driver):
    p = subprocess.run([driver, "canary"], capture_output=True, text=True, env=_san_env())
    assert p.returncode != 0 and "heap-buffer-overflow" in p.stderr


@pytest.mark.parametrize("name", sorted(ag.GOLDEN))
def test_the_reader_on_the_golden_lists_and_their_truncations(driver, name, tmp_path):
    lengths = [len(r) for r in ag.reads_of(name)]
    for which in ("calls", "shuffled"):
        want = ag.records_of(name, which).tolist()
        rc, message, lines = _driven(driver, "list", ag.list_path(name, which), *lengths)
        assert (rc, message) == (0, "") and [[int(x) for x in l.split()] for l in lines] == want
    with open(ag.list_path(name), "rb") as f:
        raw = f.read()
    cut = str(tmp_path / "cut.spm")
    for size in sorted({0, 1, 2, 12, 13, 14, 24, 25, len(raw) - 13, len(raw) - 12, len(raw) - 1} & set(range(len(raw)))):
        with open(cut, "wb") as f:
            f.write(raw[:size])
        rc, message, lines = _driven(driver, "list", cut, *lengths)
        if size == 0:
            assert rc == -1 and "is empty" in message and lines == []
        elif (size - 1) % 12:
            assert rc == -1 and "is truncated: %d bytes" % (size - 1) in message and lines == []
        else:
            assert (rc, message) == (0, "") and len(lines) == (size - 1) // 12
    # the reads of another set: a read number beyond it, or a match longer than a read
    if len(raw) > 1:
        rc, message, lines = _driven(driver, "list", ag.list_path(name), *lengths[:1])
        assert rc == -1 and "the read set holds 1 reads" in message and lines == []
        rc, message, lines = _driven(driver, "list", ag.list_path(name), *([3] * len(lengths)))
        assert rc == -1 and "more than a read of 3 and one of 3 hold" in message


def test_the_parser_under_the_sanitizers(driver, readset):
    for args, words in ((["-readset", readset, "-errors"], "-errors"), (["-readset", readset, "-spmfiles", "3"], "above 1"),
                        (["-readset"], "missing argument"), (["-readset", readset, "-l", "1"], ">= 2"),
                        (["-readset", readset], "cannot open file '%s.0.spm'" % readset)):
        rc, message, _ = _driven(driver, "tool", *args)
        assert rc == -1 and words in message


def _stats(driver, lengths):
    rc, message, lines = _driven(driver, "stats", *lengths)
    assert (rc, message) == (0, "")
    return lines


def test_the_statistics_block(driver):
    assert _stats(driver, []) == ["# no contigs respect the given cutoff parameters"]
    one = _stats(driver, [487])
    assert one == ["# number of contigs:     1", "# total contigs length:  487", "# mean contig size:      487.00",
                   "# contig size first quartile: 487", "# median contig size:         487",
                   "# contig size third quartile: 487", "# longest contig:             487",
                   "# shortest contig:            487", "# contigs > 500 nt:           0 (0.00 %)",
                   "# contigs > 1K nt:            0 (0.00 %)", "# contigs > 10K nt:           0 (0.00 %)",
                   "# contigs > 100K nt:          0 (0.00 %)", "# contigs > 1M nt:            0 (0.00 %)",
                   "# N50                487", "# L50                1", "# N80                487", "# L80                1"]
    # three contigs as the reference printed them for a set of this project's survey: 487, 248, 200
    three = _stats(driver, [200, 248, 487])
    assert three[3:6] == ["# contig size first quartile: 487", "# median contig size:         487",
                          "# contig size third quartile: 487"]
    assert three[-4:] == ["# N50                487", "# L50                1", "# N80                200", "# L80                3"]
    rng = np.random.default_rng(8)
    cases = [[100, 100], [100, 200], [5, 5, 5, 5, 5], [1, 2, 3, 4, 5], [7, 7, 9, 9, 9], [501, 500, 1001, 1000, 1000001],
             [3, 3, 3, 3, 8, 8, 8, 8], list(range(1, 30)), [10 ** 7] * 3 + [1]]
    cases += [rng.integers(1, 2000, k).tolist() for k in (2, 5, 6, 7, 8, 9, 33)]
    for lengths in cases:
        assert _stats(driver, lengths) == ["# " + l for l in sg.statistics(lengths)], lengths
    # every statistics block the reference printed is that of the lengths of its contigs
    for name, which, key in ag.CALLS:
        reads, records, want = ag.call(name, which, key)
        lengths = [c[0].size for c in sg.contigs(reads, records, *ag.options(name, key))]
        assert _stats(driver, lengths) == want["stdout"].splitlines()[7:]
