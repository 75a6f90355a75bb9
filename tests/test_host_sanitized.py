"""The host layer's readers and writers (genometools_amd/csrc/host) and the CPU
oracle (oracle/) under AddressSanitizer and UBSan.  No GPU needed, and no
sanitized code ever opens one: tests/host_san_driver.c is compiled here, by gcc
with -fsanitize=address,undefined and the sanitizer runtime linked statically,
once with the reader core of the host layer and once with the oracle, and runs
as a child process that takes a whole list of work items.  The child inherits
the environment; only ASAN_OPTIONS and UBSAN_OPTIONS are added.

What is asserted, besides "no sanitizer report and no leak" everywhere:
  * a canary (one byte read past a heap block) IS reported -- inert sanitizers
    would pass everything else;
  * parity: every fixture through encoder, file writers (every access type) and
    the .esq reader gives the files and symbols of the unsanitized library;
  * a deterministic mutation corpus over every file of tests/golden/esq: each
    mutant is rejected with a message or accepted with n valid symbols, and a
    truncated file is accepted exactly where only trailing padding is missing;
  * malformed text input and symbol maps: the library's encoding or a message;
  * the oracle on the fuzzer's inputs: byte-equal to the unsanitized oracle.
"""
import ctypes
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle_util as ou

ROOT = ou.ROOT
HOST_DIR = os.path.join(ROOT, "genometools_amd", "csrc", "host")
DRIVER_SRC = os.path.join(ROOT, "tests", "host_san_driver.c")
# -std/-D flags of genometools_amd/csrc/host/Makefile
STD_FLAGS = ["-Wall", "-Wextra", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-D_DEFAULT_SOURCE",
             "-I" + os.path.join(ROOT, "include")]
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-static-libasan"]
READER_CORE = ("esq_host.c", "alphabet_host.c", "encseq_host.c", "md5_host.c", "ois_host.c", "cli_host.c",
               "project_host.c")
# every other file of the directory: the tools and what calls the engine
TOOL_ONLY = tuple(sorted(f for f in os.listdir(HOST_DIR) if f.endswith(".c") and f not in READER_CORE))
ORACLE = ("esa_oracle.c", "pck_oracle.c")
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))
REPORT_WORDS = ("Sanitizer", "runtime error")


def san_env():
    """the child's environment: the caller's, plus the two option variables.
    malloc returns NULL for a request it cannot serve, as glibc's does; leak
    detection stays on."""
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "allocator_may_return_null=1:detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    return env


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """{"host": path, "oracle": path, "tool_objects": [...]}: the two sanitized
    builds of the driver -- the reader core of the host layer, which links
    without libgtamd_esa.so and never sees the HIP runtime, and the oracle --
    and the objects of a sanitized gt-suffixerator-amd (fixture `tool`)"""
    out = tmp_path_factory.mktemp("san")
    # can this toolchain link the sanitizer runtime at all?
    probe = out / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    probing = subprocess.Popen(["gcc"] + SAN_FLAGS + ["-o", str(out / "probe"), str(probe)],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    # every source file on its own, side by side; then one link per set
    compiles = {}

    def compile_(tag, src, flags):
        obj = str(out / (tag + ".o"))
        compiles[tag] = (obj, subprocess.Popen(
            ["gcc"] + SAN_FLAGS + STD_FLAGS + flags + ["-c", "-o", obj, src],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))

    for f in sorted(READER_CORE + TOOL_ONLY, key=lambda f: -os.path.getsize(os.path.join(HOST_DIR, f))):
        compile_(f, os.path.join(HOST_DIR, f), ["-I" + HOST_DIR])           # (the longest first)
    for f in ORACLE:
        compile_(f, os.path.join(ou.ORACLE_DIR, f), [])
    compile_("driver_host", DRIVER_SRC, ["-DDRIVER_HOST", "-I" + HOST_DIR])
    compile_("driver_oracle", DRIVER_SRC, ["-DDRIVER_ORACLE", "-I" + ou.ORACLE_DIR])
    log = probing.communicate()[0]
    logs = [(p.communicate()[0], p.returncode) for _, p in compiles.values()]
    if probing.returncode != 0:
        pytest.skip("gcc cannot build a program with -fsanitize=address,undefined "
                    "-static-libasan here (no sanitizer runtime?): " + log[-300:])
    assert all(rc == 0 for _, rc in logs), "the driver does not compile:\n" + \
        "".join(text for text, _ in logs)
    built = {"tool_objects": [compiles[f][0] for f in READER_CORE + TOOL_ONLY]}
    for name, objs, libs in (("host", ("driver_host",) + READER_CORE, ["-lz", "-lpthread", "-ldl"]),
                             ("oracle", ("driver_oracle",) + ORACLE, ["-lz", "-ldl"])):
        built[name] = str(out / name)
        subprocess.run(["gcc"] + SAN_FLAGS + ["-o", built[name]] + [compiles[o][0] for o in objs] +
                       libs, check=True)
    return built


def start(exe, items, workdir, tag):
    """a driver process over a list of work items (tuples of fields); its output
    goes to files, so that several of them run side by side without anyone
    reading their pipes"""
    base = os.path.join(str(workdir), "work_%s" % tag)
    with open(base + ".txt", "w") as f:
        f.write("".join("\t".join(map(str, it)) + "\n" for it in items))
    with open(base + ".out", "wb") as out, open(base + ".err", "wb") as err:
        proc = subprocess.Popen([exe, "run", base + ".txt"], stdout=out, stderr=err, env=san_env())
    proc.outputs = (base + ".out", base + ".err")
    return proc


def finish(proc, items):
    """the driver's lines, one per item as (rc, message, size, crc, more...);
    fails with the sanitizer's own text and the item it stopped in"""
    proc.wait()
    out, err = (open(p, errors="replace").read() for p in proc.outputs)
    lines = out.splitlines()
    where = "" if len(lines) >= len(items) else " in item %d: %r" % (len(lines), items[len(lines)])
    assert proc.returncode == 0 and not any(w in err for w in REPORT_WORDS), \
        "driver ended with status %d%s\n%s" % (proc.returncode, where, err[-6000:])
    assert len(lines) == len(items)
    res = []
    for line in lines:
        f = line.split("\t")
        res.append((int(f[0]), f[1], int(f[2]), int(f[3], 16)) + tuple(f[4:]))
    return res


def run(exe, items, workdir, tag="one"):
    return finish(start(exe, items, workdir, tag), items)


def test_canary_is_reported(drivers):
    """one byte read past a heap block: AddressSanitizer must say so, in both builds"""
    for exe in (drivers["host"], drivers["oracle"]):
        p = subprocess.run([exe, "canary"], capture_output=True, text=True, env=san_env())
        assert p.returncode != 0 and "survived" not in p.stdout
        assert "AddressSanitizer: heap-buffer-overflow" in p.stderr, p.stderr[-2000:]
        assert "canary" in p.stderr


# ---- parity with the unsanitized library ----

import test_host as th          # noqa: E402  (its ctypes declarations of libgtamd_host.so)
from test_host import host      # noqa: E402,F401  (fixture)

SATS = ["direct", "bytecompress", "eqlen", "bit", "uchar", "ushort", "uint32"]
SEQ_EXTS = ("esq", "ssp", "des", "sds", "md5", "ois")


def _files_of(idx):
    return {ext: open(idx + "." + ext, "rb").read() for ext in SEQ_EXTS
            if os.path.exists(idx + "." + ext)}


def _lib_write_forced(host, paths, protein, idx, sat):
    """th._write_esq_forced for any number of input files: (rc, message) of the
    library's gtamd_write_esq_sat, names stored without directories"""
    arr = (ctypes.c_char_p * len(paths))(*[p.encode() for p in paths])
    names = (ctypes.c_char_p * len(paths))(*[os.path.basename(p).encode() for p in paths])
    ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
    info, ss = th.EncInfo(), th.SeqStats()
    err = ctypes.create_string_buffer(2048)
    assert host.gtamd_encode_files_info(arr, len(paths), int(protein), ctypes.byref(ptr),
                                        ctypes.byref(n), None, None, ctypes.byref(info),
                                        err, 2048) == 0, err.value
    rc = host.gtamd_write_esq_sat(idx.encode(), names, len(paths), ptr, n.value, int(protein),
                                  ctypes.byref(info), 1, sat.encode(), ctypes.byref(ss), err, 2048)
    host.gtamd_encinfo_free(ctypes.byref(info))
    ctypes.CDLL(None).free(ptr)
    return rc, err.value.decode()


def _golden_inputs():
    """(key, paths, protein, expected sequence files or None)"""
    out = []
    for name, e in sorted(th.GOLDEN.items()):
        out.append((name, [ou.fixture_path(name)], e["alphabet"] == "protein", e["seqfiles"]))
    for key, e in sorted(th.MULTI.items()):
        out.append((key, [os.path.join(ou.GOLDEN_DIR, "multi", f) for f in e["files"]], False,
                    e["seqfiles"]))
    return out


def test_parity_with_the_unsanitized_library(drivers, host, tmp_path):
    """every fixture of golden.json / golden_multi.json / golden_lossless.json:
    encoded, written with the chosen and with every forced access type, and read
    back by the sanitized build; files, symbols and messages are those of
    libgtamd_host.so, and the golden sums where test_host.py compares them"""
    import hashlib
    items, checks = [], []
    inputs = _golden_inputs()
    for k, (key, paths, protein, expected) in enumerate(inputs):
        alpha = "protein" if protein else "dna"
        lib_idx, san_idx = str(tmp_path / ("lib%d" % k)), str(tmp_path / ("san%d" % k))
        th._write_all_seqfiles(host, paths, protein, lib_idx)
        want_enc = th._encode(host, paths, protein)
        th._check_seqfiles(lib_idx, expected)          # the library itself against the goldens
        items.append(("encode", alpha, "-", 0, san_idx, san_idx + ".sym") + tuple(paths))
        checks.append(("encode", key, lib_idx, san_idx, want_enc, None))
        items.append(("read", san_idx, san_idx + ".back"))
        checks.append(("read", key, lib_idx, san_idx, want_enc, None))
        for sat in SATS:
            lib_f, san_f = "%s_%s" % (lib_idx, sat), "%s_%s" % (san_idx, sat)
            rc, msg = _lib_write_forced(host, paths, protein, lib_f, sat)
            items.append(("encode", alpha, sat, 0, san_f, "-") + tuple(paths))
            checks.append(("forced", key + " -sat " + sat, lib_f, san_f, want_enc, (rc, msg)))
            if rc == 0:
                items.append(("read", san_f, san_f + ".back"))
                checks.append(("read", key + " -sat " + sat, lib_f, san_f, want_enc, None))
    for k, name in enumerate(sorted(th.LOSSLESS)):
        src = ou.fixture_path(name)
        protein = th.GOLDEN[name]["alphabet"] == "protein"
        lib_idx, san_idx = str(tmp_path / ("libl%d" % k)), str(tmp_path / ("sanl%d" % k))
        assert th._run_tool(host, "-protein" if protein else "-dna", "-lossless", "-indexname",
                            lib_idx, "-db", os.path.basename(src),
                            cwd=os.path.dirname(src)) == (0, "")
        for ext, v in th.LOSSLESS[name].items():
            raw = open(lib_idx + "." + ext, "rb").read()
            assert (len(raw), hashlib.md5(raw).hexdigest()) == (v["bytes"], v["md5"]), (name, ext)
        items.append(("encode", "protein" if protein else "dna", "-", 1, san_idx, "-", src))
        checks.append(("lossless", name, lib_idx, san_idx, None, None))
    res = run(drivers["host"], items, tmp_path)
    forced_ok = 0
    for (kind, key, lib_idx, san_idx, want_enc, want_rc), r in zip(checks, res):
        rc, msg, size, crc = r[:4]
        if kind == "forced" and want_rc[0] != 0:
            assert (rc, msg.replace(san_idx, lib_idx)) == want_rc, key
            continue
        assert rc == 0, (key, msg)
        if kind == "read":
            got = np.fromfile(san_idx + ".back", dtype=np.uint8)
            assert np.array_equal(got, want_enc), key
            assert (size, crc) == (want_enc.size, zlib.crc32(want_enc.tobytes())), key
            continue
        if kind == "encode":
            assert np.array_equal(np.fromfile(san_idx + ".sym", dtype=np.uint8), want_enc), key
        want_files, got_files = _files_of(lib_idx), _files_of(san_idx)
        if kind == "forced":
            forced_ok += 1
            want_files = {e: v for e, v in want_files.items() if e in ("esq", "ssp")}
            got_files = {e: v for e, v in got_files.items() if e in ("esq", "ssp")}
        assert sorted(got_files) == sorted(want_files), key
        for ext in want_files:
            assert got_files[ext] == want_files[ext], (key, ext)
        if kind == "lossless":
            assert "ois" in got_files
    assert len(inputs) == 52 and len(th.LOSSLESS) == 12 and forced_ok >= 4 * len(inputs)
    print("parity: %d fixtures, %d lossless, %d work items, %d forced access types written"
          % (len(inputs), len(th.LOSSLESS), len(items), forced_ok))


def test_reader_on_the_reference_files_under_the_sanitizer(drivers, host, tmp_path):
    """every stem of tests/golden/esq through the sanitized reader: the symbols
    the library's reader returns"""
    items = [("read", os.path.join(th.ESQ_DIR, stem), str(tmp_path / (stem + ".sym")))
             for stem in th.REF_ESQ]
    res = run(drivers["host"], items, tmp_path)
    assert len(items) == 31
    for stem, (rc, msg, size, crc, numofchars, bad) in zip(th.REF_ESQ, res):
        want, protein, _ = th._read_esq(host, os.path.join(th.ESQ_DIR, stem))
        assert rc == 0 and int(bad) == 0 and int(numofchars) == (20 if protein else 4), (stem, msg)
        assert np.array_equal(np.fromfile(str(tmp_path / (stem + ".sym")), dtype=np.uint8), want), stem


# ---- the project reader ----

def _project(host, tmp_path, stem, flag, fixture):
    """(index, symbols) of a project the unsanitized tool's host side writes;
    the reader checks the size of a table, not its entries: the tables are
    zeros of the right size, .suf with 8 bytes an entry, .llv with one pair"""
    idx = str(tmp_path / stem)
    assert th._run_tool(host, flag, "-db", ou.fixture_path(fixture), "-indexname", idx) == (0, "")
    enc = th._read_esq(host, idx)[0]
    for ext, size in (("suf", 8 * (enc.size + 1)), ("lcp", enc.size + 1), ("llv", 16), ("bwt", enc.size + 1)):
        with open("%s.%s" % (idx, ext), "wb") as f:
            f.write(bytes(size))
    return idx, enc


def _damaged(idx, name, prj_lines=(), **tables):
    """a copy of project idx under `name`: the sequence files linked, INDEX.prj
    with prj_lines appended (the last line of a key counts), every table
    linked but those of `tables`: {ext: size in bytes, or None for no file}"""
    other = os.path.join(os.path.dirname(idx), name)
    for ext in ("esq", "ssp", "suf", "lcp", "llv", "bwt"):
        if ext in tables:
            if tables[ext] is not None:
                with open("%s.%s" % (other, ext), "wb") as f:
                    f.write(bytes(tables[ext]))
        elif os.path.exists("%s.%s" % (idx, ext)):
            os.symlink("%s.%s" % (idx, ext), "%s.%s" % (other, ext))
    with open(other + ".prj", "w") as f:
        f.write(open(idx + ".prj").read() + "".join(line + "\n" for line in prj_lines))
    return other


def test_project_reader_under_the_sanitizer(drivers, host, tmp_path):
    """gtamd_project_open / _map / _sequence_starts / _close of project_host.c on
    a DNA and a protein project and on damaged copies of them: the symbols, the
    entry size and the number of sequences, or -1 with the message the tools
    gave for such a file before they shared this reader -- the strings below are
    those of the tools' own copies of these checks, word for word.  No report,
    no leak."""
    ANY, FORWARD, FORWARD_TWO = 0, 1, 2
    dna, dna_enc = _project(host, tmp_path, "dna", "-dna", "Atinsert.fna")
    prot, prot_enc = _project(host, tmp_path, "prot", "-protein", "sw100K1.fsa")
    n, N = dna_enc.size, dna_enc.size + 1
    reversed_enc = dna_enc.copy()
    host.gtamd_apply_readmode(reversed_enc.ctypes.data, reversed_enc.size, 1)
    assert not np.array_equal(reversed_enc, dna_enc)
    forward_one = ("file '%s.prj' describes a mirrored index or one of a read mode other than forward: such an "
                   "index is not supported by the MI355X engine's %s")
    cases = []         # (index, verb, which, tool, required, tables, expected)

    def ok(index, which, tool, required, tables, enc, suf_bytes):
        cases.append((index, "searched", which, tool, required, tables,
                      (0, "", enc.size, zlib.crc32(enc.tobytes()), str(suf_bytes),
                       str(1 + int(np.count_nonzero(enc == 255))))))

    def bad(index, which, tool, required, tables, message, verb="searched"):
        cases.append((index, verb, which, tool, required, tables, (-1, message, 0, 0)))

    ok(dna, ANY, "-", 0, "slvb", dna_enc, 8)
    ok(dna, FORWARD, "tagerator", 1, "s", dna_enc, 8)
    ok(dna, FORWARD_TWO, "repfind", 1, "slv", dna_enc, 8)
    ok(dna, ANY, "-", 0, "-", dna_enc, 0)
    ok(prot, ANY, "-", 0, "slvb", prot_enc, 8)
    ok(prot, FORWARD_TWO, "querymatch", 1, "s", prot_enc, 8)
    ok(_damaged(dna, "suf4", suf=4 * N), FORWARD, "idxlocali", 1, "s", dna_enc, 4)
    ok(_damaged(dna, "suf8", suf=8 * N), ANY, "-", 0, "s", dna_enc, 8)
    ok(_damaged(dna, "llv0", llv=0), ANY, "-", 0, "slv", dna_enc, 8)
    short = _damaged(dna, "short", suf=8 * N - 1)
    for which, tool, required in ((ANY, "-", 0), (FORWARD, "tagerator", 1)):
        bad(short, which, tool, required, "s",
            "file '%s.suf' has %d bytes, %d (-suftabuint) or %d expected for %d entries"
            % (short, 8 * N - 1, 4 * N, 8 * N, N))
    llv8 = _damaged(dna, "llv8", llv=8)
    bad(llv8, ANY, "-", 0, "slvb",
        "file '%s.llv' has 8 bytes, not a multiple of 16 (pairs of two 64-bit numbers)" % llv8)
    bad(llv8, FORWARD_TWO, "repfind", 1, "slv",
        "file '%s.llv' has 8 bytes, not a multiple of 16 (pairs of two 64-bit numbers)" % llv8)
    lcp = _damaged(dna, "lcp", lcp=N - 1)
    bad(lcp, ANY, "-", 0, "slvb", "file '%s.lcp' has %d bytes, %d expected" % (lcp, N - 1, N))
    bwt = _damaged(dna, "bwt", bwt=N + 1)
    bad(bwt, ANY, "-", 0, "slvb", "file '%s.bwt' has %d bytes, %d expected" % (bwt, N + 1, N))
    nosuf = _damaged(dna, "nosuf", suf=None)
    bad(nosuf, ANY, "-", 0, "s", "cannot open file '%s.suf'" % nosuf)
    bad(nosuf, FORWARD, "tagerator", 1, "s", 'cannot open file "%s.suf": No such file or directory' % nosuf)
    nollv = _damaged(dna, "nollv", llv=None)
    bad(nollv, FORWARD_TWO, "repfind", 1, "slv", 'cannot open file "%s.llv": No such file or directory' % nollv)
    bad(str(tmp_path / "nosuch"), ANY, "-", 0, "s", "cannot open file '%s.prj'" % (tmp_path / "nosuch"))
    rev = _damaged(dna, "rev", ["readmode=1"])
    ok(rev, ANY, "-", 0, "slvb", reversed_enc, 8)
    bad(rev, FORWARD, "tagerator", 1, "s", forward_one % (rev, "tagerator"))
    bad(rev, FORWARD, "idxlocali", 1, "s", forward_one % (rev, "idxlocali"))
    bad(rev, FORWARD_TWO, "repfind", 1, "slv",
        "file '%s.prj' gives a read mode other than forward: such an index is not supported by the MI355X "
        "engine's repfind" % rev)
    mir = _damaged(prot, "mir", ["mirrored=1"])
    bad(mir, ANY, "-", 0, "s",
        "file '%s.prj' asks for complemented symbols of an alphabet that is not DNA" % mir, verb="checked")
    bad(mir, FORWARD, "tagerator", 1, "s", forward_one % (mir, "tagerator"))
    bad(mir, FORWARD_TWO, "querymatch", 1, "s",
        "file '%s.prj' describes a mirrored index: such an index is not supported by the MI355X engine's "
        "querymatch" % mir)
    packed = _damaged(dna, "packed", ["numberofallsortedsuffixes=0"])
    bad(packed, ANY, "-", 0, "s",
        "file '%s.prj' describes the project of a packed index (numberofallsortedsuffixes=0): it has no tables "
        "to check" % packed, verb="checked")
    big = (1 << 32) - 4096
    parts = _damaged(dna, "parts", ["totallength=%d" % big, "numberofallsortedsuffixes=%d" % (big + 1)])
    for verb in ("checked", "searched"):
        bad(parts, ANY, "-", 0, "s",
            "sequence of %d symbols is beyond the limit of a single build (%d table entries); the slices of a "
            "build in parts are not %s" % (big, big, verb), verb=verb)
    longer = _damaged(dna, "longer", ["totallength=%d" % (n + 1), "numberofallsortedsuffixes=%d" % (n + 2)])
    bad(longer, ANY, "-", 0, "s", "INDEX.esq and INDEX.prj of '%s' disagree on the total length" % longer)
    res = run(drivers["host"], [("project",) + c[:6] for c in cases], tmp_path, "project")
    for c, r in zip(cases, res):
        assert r == c[6], c[:6]
    assert len(cases) == 30 and sum(c[6][0] == 0 for c in cases) == 10


# ---- the command line tool ----

@pytest.fixture(scope="module")
def tool(drivers, host, tmp_path_factory):
    """a sanitized gt-suffixerator-amd: every file of csrc/host with the
    sanitizers, linked against the ordinary libgtamd_esa.so.  It is run only on
    command lines that end before a device is asked for: option errors, and
    builds and -ii runs without a table option."""
    exe = str(tmp_path_factory.mktemp("tool") / "gt-suffixerator-amd")
    pkg = th._lib.HERE
    subprocess.run(["gcc"] + SAN_FLAGS + ["-o", exe] + drivers["tool_objects"] +
                   ["-L" + pkg, "-lgtamd_esa", "-lpthread", "-lz", "-ldl", "-Wl,-rpath," + pkg],
                   check=True)
    return exe


def tool_cases():
    """chains of (arguments, working directory or None); {d} is a directory of the
    side that runs them, library or sanitized tool.  The cases of a chain run in
    order, later ones read what earlier ones wrote; chains do not depend on each
    other"""
    fx, extra = ou.fixture_path, os.path.join(ou.GOLDEN_DIR, "extra")
    at = fx("Atinsert.fna")
    first = [
        (("-db", at, "-indexname", "{d}/first"), None),
        (("-ii", "{d}/first", "-indexname", "{d}/second"), None),
        (("-ii", "{d}/first", "-db", "x.fna"), None),
        (("-ii", "{d}/first", "-dna"), None),
        (("-ii", "{d}/nosuch"), None),
    ]
    single = [
        (("-suf",), None),
        (("-db", "a.fna", "b.fna", "-suf"), None),
        (("-db", at, "-dir", "sideways", "-suf"), None),
        (("-protein", "-db", fx("sw100K1.fsa"), "-dir", "rcl", "-suf"), None),
        (("-db", at, "-frobnicate"), None),
        (("-dna", "-indexname", "{d}/knobs", "-db", at, "-cmpcharbychar", "-dc", "32", "-algbds", "3",
          "31", "80", "-maxwidthrealmedian", "1", "-noshortreadsort", "-storespecialcodes", "yes",
          "-withradixsort", "-iterscan", "no", "-parts", "2", "-memlimit", "1GB", "-showprogress",
          "no", "-dccheck"), None),
        (("-db", at, "-indexname", "{d}/nossp", "-ssp", "no", "-des", "no", "-md5", "no"), None),
        (("-db", at, "-indexname", "{d}/mirror", "-mirrored"), None),
        (("-db", at, "-indexname", "{d}/rcl", "-dir", "rcl"), None),
        (("-smap", "{d}/nothing", "-indexname", "{d}/x", "-db", at), None),
        (("-smap", os.path.join(extra, "TransAnum"), "-indexname", "{d}/x", "-db", at), None),
        (("-smap", os.path.join(extra, "prot5.map"), "-dir", "rcl", "-indexname", "{d}/x", "-db",
          fx("extra/protein_specials.faa")), None),
        (("-db", at, "-sat", "fast", "-indexname", "{d}/x"), None),
        (("-db", at, "-sat", "bytecompress", "-indexname", "{d}/x"), None),
        (("-db", at, "-sat", "eqlen", "-indexname", "{d}/x"), None),
    ]
    for opt in ("-plain", "-kys", "-lcpdist", "-compressedoutput", "-genomediff", "-sortmaxdepth",
                "-spmopt"):
        single.append((("-dna", "-indexname", "{d}/x", "-db", at, opt), None))
    chains = [first] + [[c] for c in single]
    for sat in SATS:
        chains.append([(("-db", fx("Duplicate.fna"), "-sat", sat, "-indexname", "{d}/dup_" + sat), None),
                       (("-ii", "{d}/dup_" + sat, "-indexname", "{d}/dup2_" + sat), None)])
    for k, name in enumerate(sorted(th.CLIPDESC)):
        chains.append([(("-dna", "-clipdesc", "-indexname", "{d}/clip%d" % k, "-db",
                         os.path.basename(fx(name))), os.path.dirname(fx(name)))])
    for k, key in enumerate(sorted(th.SMAP)):
        mapname, name = key.split("|")
        chains.append([(("-smap", os.path.join(extra, mapname), "-indexname", "{d}/smap%d" % k, "-db",
                         os.path.basename(fx(name))), os.path.dirname(fx(name))),
                       (("-ii", "{d}/smap%d" % k, "-indexname", "{d}/smapagain%d" % k), None)])
    for k, name in enumerate(sorted(th.LOSSLESS)):
        flag = "-protein" if th.GOLDEN[name]["alphabet"] == "protein" else "-dna"
        chains.append([((flag, "-lossless", "-indexname", "{d}/lossless%d" % k, "-db",
                         os.path.basename(fx(name))), os.path.dirname(fx(name)))])
    for stem in th.REF_ESQ:
        chains.append([(("-ii", os.path.join(th.ESQ_DIR, stem), "-indexname", "{d}/ref_" + stem), None)])
    return chains


def test_tool_under_the_sanitizer(tool, host, tmp_path):
    """the command lines test_host.py runs without a GPU -- option errors, -db ...
    -indexname with the sequence-side switches, -smap, -lossless, -sat, -ii --
    through a sanitized gt-suffixerator-amd, one process each: exit status,
    message and every file written are those of the library called in this
    process.  Leak detection stays on: the HIP runtime is loaded with
    libgtamd_esa.so but never initialised by these command lines."""
    lib_dir, san_dir = tmp_path / "lib", tmp_path / "san"
    lib_dir.mkdir()
    san_dir.mkdir()
    from concurrent.futures import ThreadPoolExecutor
    chains = tool_cases()

    def sanitized(chain):
        return [subprocess.run([tool] + [a.format(d=san_dir) for a in args], cwd=cwd, env=san_env(),
                               capture_output=True, text=True, errors="replace")
                for args, cwd in chain]

    with ThreadPoolExecutor(WORKERS) as pool:
        runs = pool.map(sanitized, chains)         # (started now, side by side)
        ok = cases = 0
        for chain in chains:
            wants = [th._run_tool(host, *[a.format(d=lib_dir) for a in args], cwd=cwd)
                     for args, cwd in chain]
            for (args, cwd), (rc, msg), p in zip(chain, wants, next(runs)):
                want_err = "" if rc == 0 else "gt suffixerator: error: %s\n" % msg.replace(
                    str(lib_dir), str(san_dir))
                assert (p.returncode, p.stderr) == (0 if rc == 0 else 1, want_err), \
                    (args, p.stderr[-3000:])
                ok += rc == 0
                cases += 1
    names = sorted(os.listdir(lib_dir))
    assert names == sorted(os.listdir(san_dir))
    for name in names:
        assert open(lib_dir / name, "rb").read() == open(san_dir / name, "rb").read(), name
    assert cases >= 120 and ok >= 80 and cases - ok >= 25 and len(names) >= 300
    print("tool: %d command lines, %d without error, %d files compared" % (cases, ok, len(names)))


# ---- the mutation corpus for INDEX.esq / INDEX.ssp ----

SWEEP_VALUES = [0, 1, 2, 255, 256, 65535, 65536, 2**31, 2**32, 2**61, 2**62, 2**63, 2**64 - 8,
                2**64 - 1]
SWEEP_WORDS = 60
PINS = [(13, 2**62), (13, 2**63), (13, 2**64 - 1), (4, 2**62), (5, 2**60), (6, 2**64 - 64)]
# the two overflows a sanitized probe of the reader found before it was fixed:
# wildcardranges (word 13, sci[6]) so large that width * items wrapped
NAMED = {"Atinsert_seqrange_3-7.fna.uchar": [("E", 13, 2**64 - 8)],
         "TTTN.fna.uint32": [("E", 13, 2**62), ("E", 37, 2**32)]}
SAT_NUMBER = {"direct": 0, "bytecompress": 1, "eqlen": 2, "bit": 3, "uchar": 4, "ushort": 5,
              "uint32": 6}


def cut_lengths(size):
    """every length up to 512 bytes, every multiple of 8 and its neighbours
    beyond that, and the last 64 bytes; the whole file is no cut"""
    cuts = set(range(0, min(size, 513)))
    for m in range(512, size, 8):
        cuts.update((m - 1, m, m + 1))
    cuts.update(range(max(0, size - 64), size))
    return sorted(c for c in cuts if 0 <= c < size)


def trailing_padding(words, sat):
    """bytes of padding behind the last section of an INDEX.esq (sections are
    padded to 8 bytes, src/core/mapspec.c:350-457): the symbols themselves with
    direct access, 5 bits per symbol for the protein alphabet with
    bytecompress; the last section of every other access type (two-bit words,
    special bits, endidxinpage) consists of 8-byte words"""
    n = int(words[3])
    if sat == "direct":
        return -n % 8
    if sat == "bytecompress":
        return -((5 * n + 7) // 8) % 8
    return 0


def corpus(stem):
    """(kind, fields of the work item) for one stem; the items of a stem follow
    its `base` item"""
    esq = open(os.path.join(th.ESQ_DIR, stem + ".esq"), "rb").read()
    ssp_path = os.path.join(th.ESQ_DIR, stem + ".ssp")
    ssp = open(ssp_path, "rb").read() if os.path.exists(ssp_path) else None
    nwords = min(SWEEP_WORDS, len(esq) // 8)
    out = []
    for w in range(nwords):
        for v in SWEEP_VALUES:
            out.append(("single", ("mut", "E", w, v)))
    for pw, pv in PINS:
        for w in range(nwords):
            if w != pw:
                for v in SWEEP_VALUES:
                    out.append(("pair", ("mut", "E", pw, pv, "E", w, v)))
    for c in cut_lengths(len(esq)):
        out.append(("cut", ("cut", "E", c)))
    if ssp is not None:
        for w in range(min(SWEEP_WORDS, len(ssp) // 8)):
            for v in SWEEP_VALUES:
                out.append(("ssp", ("mut", "S", w, v)))
        for c in range(len(ssp)):
            out.append(("sspcut", ("cut", "S", c)))
    return esq, ssp, out


@pytest.mark.parametrize("stem", sorted(NAMED))
def test_overflows_of_the_range_table_sizes(drivers, tmp_path, stem):
    """the two mutants with which a sanitized probe of the reader first found it
    reading past the file (heap-buffer-overflow in sw_load): each in a process
    of its own, rejected as inconsistent, no report"""
    ssp = os.path.join(th.ESQ_DIR, stem + ".ssp")
    items = [("base", os.path.join(th.ESQ_DIR, stem + ".esq"), ssp if os.path.exists(ssp) else "-",
              str(tmp_path / "scratch")),
             ("mut",) + tuple(x for edit in NAMED[stem] for x in edit)]
    res = run(drivers["host"], items, tmp_path)
    assert res[1][0] == -1 and res[1][1].endswith(".esq' is truncated or inconsistent"), res[1]


def test_mutation_corpus(drivers, tmp_path):
    """every mutant is rejected with a message or accepted with the n symbols of
    its header, all of the alphabet or special; no report, no leak.  Truncated
    files are accepted exactly where the cut takes trailing padding only"""
    per_stem = {stem: corpus(stem) for stem in th.REF_ESQ}
    # stems to workers, the long ones first
    loads = [[] for _ in range(WORKERS)]
    for stem in sorted(per_stem, key=lambda s: -len(per_stem[s][2])):
        min(loads, key=lambda l: sum(len(per_stem[s][2]) for s in l)).append(stem)
    procs = []
    for k, stems in enumerate(loads):
        items = []
        for stem in stems:
            ssp_path = os.path.join(th.ESQ_DIR, stem + ".ssp")
            items.append(("base", os.path.join(th.ESQ_DIR, stem + ".esq"),
                          ssp_path if per_stem[stem][1] is not None else "-",
                          str(tmp_path / ("scratch%d" % k))))
            items.extend(fields for _, fields in per_stem[stem][2])
        procs.append((stems, items, start(drivers["host"], items, tmp_path, "mut%d" % k)))
    counts = {}
    for stems, items, proc in procs:
        res = iter(finish(proc, items))
        for stem in stems:
            esq, ssp, muts = per_stem[stem]
            sat = stem.rsplit(".", 1)[1]
            words = np.frombuffer(esq[:len(esq) // 8 * 8], dtype="<u8")
            assert int(words[2]) == SAT_NUMBER[sat]
            needs_ssp = sat in ("uchar", "ushort", "uint32") and int(words[4]) > 1
            pad = trailing_padding(words, sat)
            assert next(res)[0] == 0
            accepted_cuts, all_cuts = set(), set()
            for kind, fields in muts:
                r = next(res)
                rc, msg, size = r[0], r[1], r[2]
                c = counts.setdefault(kind, [0, 0])
                c[rc == 0] += 1
                if rc != 0:
                    assert rc == -1 and msg != "" and size == 0, (stem, fields, r)
                else:
                    # accepted: the n of the (mutated) header, every symbol valid
                    hdr = {w: int(words[w]) for w in (3, 5, 6, 24)}
                    if kind not in ("cut", "sspcut"):
                        for j in range(1, len(fields), 3):
                            if fields[j] == "E" and fields[j + 1] in hdr:
                                hdr[fields[j + 1]] = fields[j + 2]
                    assert size == hdr[3] and int(r[5]) == 0, (stem, fields, r)
                    # ... and a header whose sections the file can hold: n symbols of
                    # at least two bits, 16 bytes per input file, the file names, the
                    # symbol map text (a reader whose sums wrap walks backwards instead)
                    assert (hdr[3] <= 4 * len(esq) and 16 * hdr[5] <= len(esq) and
                            hdr[6] <= len(esq) and hdr[24] <= len(esq)), (stem, fields, r)
                if kind == "cut":
                    all_cuts.add(fields[2])
                    if rc == 0:
                        accepted_cuts.add(fields[2])
                    else:
                        assert ("truncated or inconsistent" in msg or "unsupported format version" in msg
                                or "not written for 64-bit" in msg), (stem, fields, msg)
                if kind == "sspcut":
                    # the separator table ends in 8-byte words: no cut of a file that
                    # is read at all leaves it whole
                    assert (rc == 0) == (not needs_ssp), (stem, fields, r)
                    if rc != 0:
                        assert "does not fit index" in msg, (stem, fields, msg)
            assert accepted_cuts == {c for c in all_cuts if c >= len(esq) - pad}, \
                (stem, pad, sorted(accepted_cuts))
    print("mutants [rejected, accepted] by kind: %s" % json.dumps(counts, sort_keys=True))
    total = {k: sum(v) for k, v in counts.items()}
    nwords = sum(min(SWEEP_WORDS, os.path.getsize(os.path.join(th.ESQ_DIR, s + ".esq")) // 8)
                 for s in th.REF_ESQ)
    assert len(th.REF_ESQ) == 31 and nwords >= 31 * 37
    assert total["single"] == nwords * len(SWEEP_VALUES)
    assert total["pair"] == len(PINS) * (nwords - len(th.REF_ESQ)) * len(SWEEP_VALUES)
    assert total["cut"] >= 31 * 296 and total["ssp"] >= 29 * 2 * len(SWEEP_VALUES)
    # the corpus is no row of rejections: words the reader does not use leave the file valid
    assert counts["single"][1] > 1000 and counts["single"][0] > 1000


# ---- malformed text input and symbol maps ----

class Alphabet(ctypes.Structure):          # gtamd_alphabet, include/gtamd_host.h
    _fields_ = [("symbolmap", ctypes.c_uint8 * 256), ("numofchars", ctypes.c_uint32),
                ("characters", ctypes.c_char * 64), ("wildcardshow", ctypes.c_char),
                ("alphatype", ctypes.c_int), ("bitspersymbol", ctypes.c_uint),
                ("alphadef", ctypes.c_void_p), ("lengthofalphadef", ctypes.c_uint64)]


def _lib_encode_smap(host, mapfile, paths):
    """(symbols, None) or (None, message) of the unsanitized library for a
    symbol map, with the tool's limit of 28 letters"""
    a = Alphabet()
    err = ctypes.create_string_buffer(2048)
    host.gtamd_alphabet_from_file.argtypes = [ctypes.c_char_p, ctypes.POINTER(Alphabet),
                                              ctypes.c_char_p, ctypes.c_size_t]
    host.gtamd_alphabet_free.argtypes = [ctypes.POINTER(Alphabet)]
    host.gtamd_encode_files_alpha.argtypes = [
        ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.POINTER(Alphabet),
        ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    if host.gtamd_alphabet_from_file(mapfile.encode(), ctypes.byref(a), err, 2048) != 0:
        return None, err.value.decode(errors="replace")
    try:
        if a.numofchars > 28:
            return None, "symbol map '%s' defines more than 28 letters" % mapfile
        arr = (ctypes.c_char_p * len(paths))(*[p.encode() for p in paths])
        ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
        if host.gtamd_encode_files_alpha(arr, len(paths), ctypes.byref(a), ctypes.byref(ptr),
                                         ctypes.byref(n), None, None, None, err, 2048) != 0:
            return None, err.value.decode(errors="replace")
        enc = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)),
                                    shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint8)
        ctypes.CDLL(None).free(ptr)
        return enc, None
    finally:
        host.gtamd_alphabet_free(ctypes.byref(a))


TEXT_CASES = {          # the error inputs of test_host.py and test_encode_gpu.py
    "illegal.fna": (b">a\nACGT\nACXT\n", False),
    "empty_first.fna": (b">a\n>b\nACGT\n", False),
    "empty_last.fna": (b">a\nacgt\n>b\n", False),
    "lowercase.faa": (b">p\nlvif\n", True),
    "headless.fna": (b"ACGT\nAC\n>second\nGG\n>third no newline", False),
    "no_header.fna": (b"ACGT\nACGT\n", False),
    "midline.fna": (b">a\nACGT>b rest of line\nTTTT\n", False),
    "blanks.fna": (b">x y\r\nAC GT\r\n\r\n\tNN\x0cA\r\n>z\r\nT\r\n", False),
    "crlf.fna": (b">a\r\nACGT\r\nNNAC\r\n>b\r\nTT\r\n", False),
    "no_final_newline.fna": (b">a\nACGT\n>b\nAC", False),
    "header_only": (b">", False),
    "nothing.fna": (b"", False),
    "q_at.fastq": (b"@a\nACGT\n+\nIIII\nX\n", False),
    "q_cut.fastq": (b"@a\nACGT\n+\nII", False),
    "q_ok_multiline.fastq": (b"@r1\nACGT\nAC\n+r1\nII\nII@+\n@r2\nNNA\n+\n@@@\n", False),
    "multiline.fastq": (b"@a\nAC\nGT\n+\nII\nII\n", False),
    "no_last_newline.fastq": (b"@a\nACGT\n+\nIIII", False),
    "crlf.fastq": (b"@a\r\nACGT\r\n+\r\nIIII\r\n", False),
    "blank_in_sequence.fastq": (b"@a\nAC GT\n+\nIIII\n", False),
    "blank_in_qualities.fastq": (b"@a\nACGT\n+\nII II\n", False),
    "short_qualities.fastq": (b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIII\n", False),
    "long_qualities.fastq": (b"@a\nACGT\n+\nIIIII\n@a\nACGT\n+\nIIII\n", False),
    "other_name.fastq": (b"@a\nACGT\n+b\nIIII\n", False),
    "illegal_symbol.fastq": (b"@a\nACGT\n+\nIIII\n@b\nACXT\n+\nIIII\n", False),
    "empty_sequence.fastq": (b"@a\n\n+\n\n", False),
    "no_at.fastq": (b"@a\nACGT\n+\nIIII\nb\nACGT\n+\nIIII\n", False),
    "no_plus.fastq": (b"@a\nACGT\nIIII\nIIII\n", False),
    "three_lines.fastq": (b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\n", False),
    "blank_line_between.fastq": (b"@a\nACGT\n+\nIIII\n\n@a\nACGT\n+\nIIII\n", False),
    "at_only.fastq": (b"@", False),
}


def smap_mutants(text):
    letters = bytes(c for c in range(33, 127) if chr(c).isalnum() or chr(c) in "!$%&*+-/<=>?@^_|~")
    return {
        "control": text,
        "long_line": text.replace(b"\n", b" " + b"x" * 5000 + b"\n", 1),
        "long_class": b"".join(bytes([c]) for c in letters) + b"\n" + text,
        "many_classes": b"".join(bytes([c]) + b"\n" for c in letters),
        "over_255_lines": b"".join(bytes([letters[i % len(letters)]]) + b"\n" for i in range(300)),
        "over_255_symbols_one_line": bytes(range(1, 256)) * 2 + b"\n" + text,
        "empty": b"",
        "only_newlines": b"\n\n\n",
        "nul_inside": text[:len(text) // 2] + b"\0" + text[len(text) // 2:],
        "nul_first": b"\0" + text,
        "only_nul": b"\0" * 64,
        "no_final_newline": text.rstrip(b"\n"),
        "blank_at_end": text.rstrip(b"\n") + b" \n",
    }


def test_malformed_text_under_the_sanitizer(drivers, host, tmp_path):
    """gtamd_encode_files_info on broken FASTA/FASTQ, on cut .gz and .bz2 files,
    and the symbol map reader on damaged maps: the encoding of the unsanitized
    library, or a message -- the library's own, where it has one"""
    items, want = [], []

    def add(alpha, path, lib_result):
        items.append(("encode", alpha, "-", 0, "-", "-", path))
        want.append((path, lib_result))

    def lib(path, protein):
        try:
            return th._encode(host, [path], protein), None
        except ValueError as e:
            return None, str(e)

    for name, (raw, protein) in sorted(TEXT_CASES.items()):
        p = str(tmp_path / name)
        open(p, "wb").write(raw)
        add("protein" if protein else "dna", p, lib(p, protein))
    for name in ("ebola-genomes.fna.gz", "extra/duplicate_copy.fna.bz2"):
        raw = open(ou.fixture_path(name), "rb").read()
        ext = name[name.rindex("."):]
        for cut in (0, 1, 9, 10, 11, 18, 100, len(raw) // 2, len(raw) - 9, len(raw) - 8,
                    len(raw) - 1, len(raw)):
            p = str(tmp_path / ("cut%d.fna%s" % (cut, ext)))
            open(p, "wb").write(raw[:cut])
            add("dna", p, lib(p, False))
    smap_cases = 0
    for key in sorted(th.SMAP):
        mapname, fixture = key.split("|")
        if not mapname.startswith("Trans"):
            continue
        text = open(os.path.join(ou.GOLDEN_DIR, "extra", mapname), "rb").read()
        for mname, raw in sorted(smap_mutants(text).items()):
            p = str(tmp_path / ("%s.%s.map" % (mapname, mname)))
            open(p, "wb").write(raw)
            add("smap:" + p, ou.fixture_path(fixture), _lib_encode_smap(host, p, [ou.fixture_path(fixture)]))
            smap_cases += 1
    res = run(drivers["host"], items, tmp_path)
    accepted = 0
    for (path, (enc, msg)), it, r in zip(want, items, res):
        rc, got_msg, size, crc = r[:4]
        if enc is not None:
            accepted += 1
            assert (rc, size, crc) == (0, enc.size, zlib.crc32(enc.tobytes())), (it, got_msg)
        else:
            assert rc == -1 and got_msg != "", it
            assert got_msg == msg.translate({9: 32, 10: 32, 13: 32}), it
    controls = [w for w, it in zip(want, items) if it[1].endswith(".control.map")]
    assert controls and all(enc is not None for _, (enc, _) in controls)
    assert len(TEXT_CASES) == 30 and smap_cases >= 13 and accepted >= 10
    print("malformed text: %d items, %d accepted, %d symbol map cases" % (len(items), accepted,
                                                                          smap_cases))


# ---- the oracle on the fuzzer's inputs ----

FUZZ_CASES = 200


def fuzz_chunk(exe, outdir, seed, first, step, count):
    """cases first, first + step, ... below count of the fuzzer with `seed`: the
    sequence, the FASTA file the fuzzer writes for it, the prefix length and the
    packed-index options it draws; the results of the unsanitized oracle, and the
    sanitized driver over the same inputs.  Runs in a process of its own (see
    __main__) so that the chunks go side by side."""
    from fuzz_cases import pck_options, prefix_length, random_sequence, write_fasta
    items, expected, drawn = [], [], []
    for case in range(first, count, step):
        rng = np.random.default_rng(seed * 1000003 + case)
        sigma = 20 if rng.integers(0, 4) == 0 else 4
        enc = random_sequence(rng, sigma)
        k = prefix_length(rng, sigma)
        fa = os.path.join(outdir, "%d.fa" % case)
        info = write_fasta(rng, enc, sigma, fa)
        kw = pck_options(rng, sigma)
        encfile = os.path.join(outdir, "%d.enc" % case)
        enc.tofile(encfile)
        drawn.append({"case": case, "sigma": sigma, "n": int(enc.size), "k": k,
                      "crlf": info["crlf"], "widths": sorted(info["widths"])})
        # the FASTA written decodes to the sequence: unsanitized here, sanitized below
        assert np.array_equal(ou.encode_fasta(fa, sigma == 20), enc), case
        items.append(("fasta", int(sigma == 20), fa))
        expected.append([0, "", int(enc.size), zlib.crc32(enc.tobytes())])
        ora = ou.esa(enc, sigma)
        parts = [ora["suf"], ora["lcp"], ora["llv"], ora["bwt"]] + \
            [np.ascontiguousarray(t, dtype=np.uint32) for t in ou.bcktab(enc, sigma, k)]
        raw = [np.ascontiguousarray(p).tobytes() for p in parts] + \
            [ou.pck_bdx(enc, sigma, ora["suf"], ora["bwt"], **kw)]
        items.append(("tables", sigma, k, encfile, kw["bsize"], kw["blbuck"], kw["locfreq"],
                      -1 if kw["locbitmap"] is None else int(kw["locbitmap"]),
                      int(kw["mkindex"]), int(kw["sprank"])))
        expected.append([0, "", sum(len(r) for r in raw), zlib.crc32(b"".join(raw))] +
                        ["%d:%08x" % (len(r), zlib.crc32(r)) for r in raw])
    proc = start(exe, items, outdir, "fuzz%d" % first)
    proc.wait()
    out, err = (open(p, errors="replace").read() for p in proc.outputs)
    with open(os.path.join(outdir, "result%d.json" % first), "w") as f:
        json.dump({"status": proc.returncode, "stderr": err[-6000:], "lines": out.splitlines(),
                   "items": items, "expected": expected, "drawn": drawn}, f)


def test_oracle_on_the_fuzzer_inputs(drivers, tmp_path):
    """the first FUZZ_CASES cases of test_switches_gpu.test_fuzz_replay (its seed;
    sequence and prefix length as there, then the fuzzer's FASTA writer and
    packed-index options): the sanitized oracle decodes the FASTA to the sequence
    and computes suf/lcp/llv/bwt, the bucket table and one INDEX.bdx image byte for
    byte as the unsanitized libesa_oracle.so does"""
    from fuzz_cases import LINE_WIDTHS
    from test_switches_gpu import REPLAY_CASES, REPLAY_SEED
    assert FUZZ_CASES <= REPLAY_CASES
    ou.build()
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in sys.path if p])
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), drivers["oracle"],
                               str(tmp_path), str(REPLAY_SEED), str(first), str(WORKERS),
                               str(FUZZ_CASES)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
             for first in range(WORKERS)]
    cases, crlf, widths, sigmas = 0, 0, set(), set()
    for first, p in enumerate(procs):
        log = p.communicate()[0]
        assert p.returncode == 0, log[-4000:]
        r = json.load(open(str(tmp_path / ("result%d.json" % first))))
        where = "" if len(r["lines"]) >= len(r["items"]) else \
            " in item %r" % (r["items"][len(r["lines"])],)
        assert r["status"] == 0 and not any(w in r["stderr"] for w in REPORT_WORDS), \
            "driver ended with status %d%s\n%s" % (r["status"], where, r["stderr"])
        assert len(r["lines"]) == len(r["items"]) == 2 * len(r["drawn"])
        for line, want, item in zip(r["lines"], r["expected"], r["items"]):
            f = line.split("\t")
            got = [int(f[0]), f[1], int(f[2]), int(f[3], 16)] + f[4:]
            assert got == want, item
        for d in r["drawn"]:
            cases += 1
            crlf += d["crlf"]
            widths.update(d["widths"])
            sigmas.add(d["sigma"])
    assert cases == FUZZ_CASES >= 200
    assert sigmas == {4, 20} and crlf >= 1 and widths == set(LINE_WIDTHS)
    print("fuzz cases: %d, with CRLF %d, line widths %s" % (cases, crlf, sorted(widths)))


if __name__ == "__main__":
    fuzz_chunk(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]),
               int(sys.argv[6]))
