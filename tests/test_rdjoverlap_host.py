"""CPU-side checks of the irreducible suffix-prefix match boundary:
include/gtamd_spmred.h is exported and bound and its host-only entry point works
without a device; the brute-force restatement of the definition
(tests/spmred_reference.py) over the mirrored read sets reproduces every output
of `gt readjoiner overlap` recorded in tests/golden/golden_rdjoverlap.json, the
match lines sorted and the `#` lines verbatim; and the host code of
`gt-suffixerator-amd readjoiner overlap` -- option parser, refusals, readset
reader, the writer of the bin32 list -- does what it says, in the tool and, under
AddressSanitizer and UBSan, in a stand-alone program (tests/rdj_san_driver.c)
that never asks for a device."""
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
import spmred_reference as rr
from genometools_amd import _lib, spmred

ROOT = ou.ROOT
HEADER = os.path.join(ROOT, "include", "gtamd_spmred.h")
HOST_DIR = os.path.join(_lib.HERE, "csrc", "host")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
DRIVER_SRC = os.path.join(ROOT, "tests", "rdj_san_driver.c")
REFUSED = ["-parts", "-memlimit", "-wmax", "-phase2extra", "-radixparts", "-radixsmall", "-onlyallfirstcodes"]
# the flags of tests/test_host_sanitized.py
STD_FLAGS = ["-Wall", "-Wextra", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-D_DEFAULT_SOURCE",
             "-I" + os.path.join(ROOT, "include"), "-I" + HOST_DIR]
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"]
# every file of the host layer but the one with the tool's main
HOST_FILES = tuple(sorted(f for f in os.listdir(HOST_DIR) if f.endswith(".c") and f != "suffixerator_main.c"))

with open(os.path.join(ou.GOLDEN_DIR, "golden_rdjoverlap.json")) as _f:
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
        assert getattr(lib, name).argtypes == _lib.SPMRED_ABI[name][1], name
    assert sorted(_lib.SPMRED_ABI) == declared
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_spmred.hip") in _lib.SOURCES
    for h in ("esa_spmred_core.h", "esa_spm_state.h"):
        assert os.path.join(_lib.HERE, "csrc", h) in _lib.HEADERS


def test_info_structure_and_flags_match_the_header():
    text = _header_text()
    end = text.index("} gtamd_spmred_info;")
    body = text[text.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    names = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.SpmredInfo._fields_]
    assert ctypes.sizeof(_lib.SpmredInfo) == 15 * 8 + 4 * 4           # (three floats and padding)
    flags = dict(re.findall(r"#define GTAMD_SPMRED_([A-Z_]+)\s+(\d+)u", text))
    assert (int(flags["ELIMTRANS"]), int(flags["MIRRORED"])) == (spmred.ELIMTRANS, spmred.MIRRORED)
    assert (int(flags["PREFIX_DIRECT"]), int(flags["SUFFIX_DIRECT"])) == (spmred.PREFIX_DIRECT, spmred.SUFFIX_DIRECT) \
        == (rr.PREFIX_DIRECT, rr.SUFFIX_DIRECT)


def test_geometry_needs_no_device():
    chunk, least = spmred.geometry()
    assert chunk >= 64 and chunk % 64 == 0        # a wave's ballot is one whole word of the bitmap
    assert least >= 64 and least % 64 == 0


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_spmred_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    with pytest.raises(_lib.EsaError, match="no HIP device"):
        spmred.IrreducibleMatches()


def test_closing_figures():
    info = dict(kept=190, transitive_same_read=3, transitive_other=1481)
    assert spmred.closing_figures(info, 189) == (190, 3 + 740, "1.01")
    assert spmred.closing_figures(dict(info, kept=933), 189)[2] == "4.94"


# ---- the restatement against the reference's outputs ----

@functools.lru_cache(maxsize=None)
def mirrored_reads(name):
    enc = sr.mirrored(ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, "rdj", name)))
    enc.setflags(write=False)
    return enc


@functools.lru_cache(maxsize=None)
def all_matches(name, min_len):
    enc = mirrored_reads(name)
    rows = sr.brute_force(enc, min_len)[0]
    return rows, rr.transitive(enc, rows)


@pytest.mark.parametrize("key", sorted(GOLDEN["calls"]))
def test_brute_force_reproduces_the_reference(key):
    assert len(GOLDEN["calls"]) == 12
    name, min_len, elim = key.split("|")
    want = GOLDEN["calls"][key]
    rows, trans = all_matches(name, int(min_len))
    kept, figures = rr.brute_force(mirrored_reads(name), int(min_len), elim == "yes", True, rows=rows, trans=trans)
    text = rr.sorted_text(kept)
    assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key
    assert rr.opening_lines(want["reads"]) + rr.closing_lines(figures, want["reads"], elim == "yes") == \
        want["hash_lines"]
    assert figures["contained_sequences"] == 0
    # the list file holds the same records
    assert hashlib.md5(rr.sorted_text(np.array(rr.parse_bin32(rr.bin32(kept))).reshape(-1, 4))).hexdigest() == \
        want["spm_md5"]


def test_the_goldens_cover_what_they_are_meant_to():
    calls = GOLDEN["calls"]
    for name in ("equal.fna", "mixed.fna", "long.fna"):
        enc = ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, "rdj", name))
        lengths = [k for _, k in sr.units(enc)]
        assert not (enc == 254).any() and calls["%s|%d|yes" % (name, 12 if name != "long.fna" else 100)]["reads"] == \
            len(lengths)
        assert {"equal.fna": lambda: set(lengths) == {36} and len(lengths) > 180,
                "mixed.fna": lambda: 25 <= min(lengths) and max(lengths) <= 60 and len(set(lengths)) > 20,
                "long.fna": lambda: 300 <= min(lengths) and max(lengths) <= 600}[name]()
        mine = sorted((int(k.split("|")[1]), calls[k]) for k in calls if k.startswith(name) and k.endswith("yes"))
        assert len(mine) == 2
        first = mine[0][1]
        assert first["lines"] >= 50 and int(first["hash_lines"][4].split("=")[1]) >= 100
        rows, trans = all_matches(name, mine[0][0])
        kept = rr.brute_force(mirrored_reads(name), mine[0][0], True, True, rows=rows, trans=trans)[0]
        forms = {f for f in kept[:, 3].tolist()}
        assert {3, 2, 1} <= forms                     # + +, + -, - +
        # a read with two irreducible successors, counted over both images of every match: the border of
        # the repeat
        after = {}
        for sn, pn, _, f, _, _ in kept.tolist():
            after.setdefault((sn, f & 2), set()).add((pn, f & 1))
            after.setdefault((pn, 0 if f & 1 else 2), set()).add((sn, 0 if f & 2 else 1))
        assert max(len(v) for v in after.values()) >= 2
    assert calls["long.fna|260|yes"]["lines"] > 50


def test_text_fixtures_are_those_of_the_json():
    assert len(GOLDEN["texts"]) == 2
    for name, key in GOLDEN["texts"].items():
        raw = open(os.path.join(ou.GOLDEN_DIR, "rdj", name), "rb").read()
        want = GOLDEN["calls"][key]
        assert (hashlib.md5(raw).hexdigest(), raw.count(b"\n")) == (want["md5"], want["lines"]) and want["lines"] > 0


# ---- the tool: what ends before a device is asked for ----

@pytest.fixture(scope="module")
def readsets(tmp_path_factory):
    """readsets as the tool's host side writes them: DNA reads, protein"""
    subprocess.run(["make", "-C", HOST_DIR], check=True, stdout=subprocess.DEVNULL)
    root = tmp_path_factory.mktemp("rdj")
    out = {}
    for kind, path in (("dna", os.path.join(ou.GOLDEN_DIR, "rdj", "equal.fna")), ("protein", ou.fixture_path("sw100K1.fsa"))):
        out[kind] = str(root / kind)
        subprocess.run([CLI, "-" + kind, "-tis", "-ssp", "-db", path, "-indexname", out[kind]], check=True)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory, readsets):
    """tests/rdj_san_driver.c with every file of the host layer, all under the sanitizers, linked against the
    ordinary libgtamd_esa.so, which is loaded and never asked for a device"""
    out = tmp_path_factory.mktemp("rdjsan")
    probe = out / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc"] + SAN_FLAGS + ["-o", str(out / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("gcc cannot build a program with -fsanitize=address,undefined -static-libasan here: "
                    + p.stderr[-300:])
    jobs = []
    for src in [os.path.join(HOST_DIR, f) for f in HOST_FILES] + [DRIVER_SRC]:
        obj = str(out / (os.path.basename(src) + ".o"))
        jobs.append((obj, subprocess.Popen(["gcc"] + SAN_FLAGS + STD_FLAGS + ["-c", "-o", obj, src],
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    logs = [(proc.communicate()[0], proc.returncode) for _, proc in jobs]
    assert all(rc == 0 for _, rc in logs), "".join(text for text, _ in logs)
    exe = str(out / "rdj_san_driver")
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
    p = subprocess.run([driver] + list(args), capture_output=True, text=True, env=_san_env())
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    rc, _, message = lines[-1].partition("\t")
    return int(rc), message, lines[:-1]


def _error(*args):
    """the message of the tool itself"""
    p = subprocess.run([CLI, "readjoiner", "overlap"] + list(args), capture_output=True, text=True)
    prefix = "gt readjoiner overlap: error: "
    assert p.returncode == 1 and p.stderr.startswith(prefix) and p.stderr.endswith("\n") and \
        p.stderr.count("\n") == 1, (p.returncode, p.stdout, p.stderr)
    return p.stderr[len(prefix):-1], p.stdout


def test_the_canary_is_reported(driver):
    p = subprocess.run([driver, "canary"], capture_output=True, text=True, env=_san_env())
    assert p.returncode != 0 and "survived" not in p.stdout
    assert "AddressSanitizer: heap-buffer-overflow" in p.stderr, p.stderr[-2000:]


ARGUMENT_ERRORS = [
    (("-l", "20"), 'option "-readset" is mandatory'),
    (("-readset", "{dna}"), 'option "-l" is mandatory'),
    (("-readset", "{dna}", "-l"), 'missing argument to option "-l"'),
    (("-readset", "{dna}", "-l", "-3"), 'missing argument to option "-l"'),
    (("-readset", "{dna}", "-l", "0"), 'argument to option "-l" must be an integer >= 2'),
    (("-readset", "{dna}", "-l", "1"), 'argument to option "-l" must be an integer >= 2'),
    (("-readset", "{dna}", "-l", "abc"), 'argument to option "-l" must be a non-negative integer <= 4294967295'),
    (("-readset", "{dna}", "-l", "4294967296"),
     'argument to option "-l" must be a non-negative integer <= 4294967295'),
    (("-l", "20", "-readset"), 'missing argument to option "-readset"'),
    (("-l", "20", "-readset", "{dna}", "extra"), "unnecessary arguments"),
    (("-l", "20", "-readset", "{dna}", "-nosuch"), "unknown option: -nosuch (-help shows possible options)"),
    (("-l", "20", "-readset", "{dna}", "-q", "-v"), 'option "-v" and option "-q" exclude each other'),
    (("-l", "20", "-readset", "{dna}", "-singlestrand"), "option -singlestrand is not implemented"),
    (("-l", "20", "-readset", "{dna}", "-singlestrand", "yes", "-showspm"), "option -singlestrand is not implemented"),
] + [(("-l", "20", "-readset", "{dna}", "-showspm", opt), 'option "%s" is not supported by the MI355X engine' % opt)
     for opt in REFUSED]


def test_argument_errors(driver, readsets):
    """every refusal with its message, from the sanitized program and from the tool: nothing on stdout"""
    for args, message in ARGUMENT_ERRORS:
        args = [a.format(**readsets) for a in args]
        assert _driven(driver, "tool", *args) == (-1, message, []), args
    for args, message in ARGUMENT_ERRORS[::4]:
        assert _error(*[a.format(**readsets) for a in args]) == (message, "")


def test_file_errors_end_before_the_device(driver, readsets, tmp_path):
    """the first `#` line is out when the readset is opened, as in the reference"""
    missing = str(tmp_path / "nosuch")
    opening = ["# gt readjoiner overlap (version 1.2)"]
    assert _driven(driver, "tool", "-l", "20", "-readset", missing) == \
        (-1, "cannot open file '%s.esq'" % missing, opening)
    assert _driven(driver, "tool", "-l", "20", "-q", "-readset", missing) == \
        (-1, "cannot open file '%s.esq'" % missing, [])
    protein = "mirroring can only be enabled for DNA sequences, this encoded sequence has alphabet: LVIFKREDAGSTNQYWPHMC"
    assert _driven(driver, "tool", "-l", "20", "-readset", readsets["protein"], "-v") == \
        (-1, protein, opening + ["# verbose output activated"])
    assert _error("-l", "20", "-readset", readsets["protein"], "-elimtrans", "no") == (protein, opening[0] + "\n")
    # a damaged readset: the reader's message, no report
    raw = open(readsets["dna"] + ".esq", "rb").read()
    cut = str(tmp_path / "cut")
    open(cut + ".esq", "wb").write(raw[:len(raw) // 2])
    rc, message, _ = _driven(driver, "tool", "-l", "20", "-readset", cut)
    assert rc == -1 and "truncated or inconsistent" in message


def test_help_and_the_other_tools_of_readjoiner(readsets):
    p = subprocess.run([CLI, "readjoiner", "overlap", "-help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("Usage: gt-suffixerator-amd readjoiner overlap") and p.stderr == ""
    for args in (["readjoiner"], ["readjoiner", "prefilter"], ["readjoiner", "assembly", "-readset", readsets["dna"]]):
        p = subprocess.run([CLI] + args, capture_output=True, text=True)
        assert (p.returncode, p.stdout, p.stderr) == (1, "", "gt readjoiner: error: tool overlap expected\n")


def test_the_bin32_writer_on_records_made_by_hand(driver, tmp_path):
    records = [(0, 1, 12, 3), (5, 0, 2, 2), (7, 7, 36, 1), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 30 - 1, 0), (3, 4, 255, 3)]
    records += [(k, k + 1, 20 + k % 7, k % 4) for k in range(3000)]           # more than one buffer of the writer
    src, out = str(tmp_path / "records.txt"), str(tmp_path / "hand.0.spm")

    def write(recs):
        with open(src, "w") as f:
            f.write("".join("%d %d %d %d\n" % r for r in recs))
        return _driven(driver, "list", src, out)

    assert write(records) == (0, "", [])
    raw = open(out, "rb").read()
    assert raw == rr.bin32(np.array(records, dtype=np.uint64)) and len(raw) == 1 + 12 * len(records)
    assert raw[0] == 2 and raw[1:13] == np.array([0, 1, 12 << 2 | 3], dtype="<u4").tobytes()
    assert rr.parse_bin32(raw) == sorted(records)
    assert write([]) == (0, "", []) and open(out, "rb").read() == b"\x02"
    # what three 32-bit numbers cannot hold is refused by name, whichever field it is
    for bad in ((2 ** 32, 1, 20, 3), (1, 2 ** 32, 20, 3), (1, 2, 2 ** 30, 3)):
        rc, message, _ = write(records[:3] + [bad])
        assert rc == -1 and message == ("match %d %d %d does not fit the bin32 list format (three 32-bit numbers a "
                                        "match, the length in 30 bits); the bin64 format is not written" % bad[:3])
