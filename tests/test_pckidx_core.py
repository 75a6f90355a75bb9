"""The reader of the packed index without a device: the lane code of
genometools_amd/csrc/esa_pckidx_core.h -- field extraction, both unrankings, the
walk of the var part, the locate records of both flavours -- compiled with g++
(tests/pckidx_core_shim.cpp) and run over every bucket of images the oracle
makes (oracle/pck_oracle.c, ora_pck_bdx); the checks the host makes of the
headers before a kernel runs (gtamd_pckidx_check_image); and the decoder as a
program of its own under ASan and UBSan on buckets that lie."""
import ctypes
import itertools
import os
import re
import struct
import subprocess
from math import comb, factorial

import numpy as np
import pytest

import oracle_util as ou
from device_check import read_bits
from genometools_amd import _lib, pck

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "pckidx_core_shim.cpp")
CORE = os.path.join(ROOT, "genometools_amd", "csrc", "esa_pckidx_core.h")
SHIM = os.path.join(ROOT, "oracle", "_build", "libpckidx_core_shim.so")
NONE = np.uint64(2 ** 64 - 1)
GEOM = ("rows", "buckets", "sigma", "B", "K", "locint", "bitmap", "count", "reversible", "rot0",
        "first_special_row", "regions", "cw_base_bit", "cw_bits", "pre_var_idx", "var_off_bits", "pre_cb_off",
        "cb_off_bits", "var_base_bit", "var_end_bit", "bits_orig_pos", "bits_orig_rank", "pre_cw_ext",
        "range_enc_pos", "offsets_wrap")


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in (SHIM_SRC, CORE)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SHIM_SRC],
                       check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.pkx_shim_open.restype = P
    lib.pkx_shim_open.argtypes = [P, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    lib.pkx_shim_close.argtypes = [P]
    lib.pkx_shim_geom.argtypes = [P, P]
    lib.pkx_shim_decode.argtypes = [P, P, P]
    lib.pkx_shim_decode.restype = ctypes.c_uint32
    lib.pkx_shim_marks.argtypes = [P, P, P]
    lib.pkx_shim_marks.restype = ctypes.c_uint32
    return lib


def test_every_declared_symbol_is_exported_and_bound():
    header = os.path.join(_lib.ROOT, "include", "gtamd_pckidx.h")
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(gtamd_[a-z_0-9]+)\s*\(", text)))
    assert sorted(_lib.PCKIDX_ABI) == declared and len(declared) == 12
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.PCKIDX_ABI[name][1], name
    body = text[text.index("typedef struct {"):text.index("} gtamd_pckidx_info;")]
    names = re.findall(r"\b(?:u?int\d+_t|float)\s+([a-z_0-9]+);", body)
    assert names == [n for n, _ in _lib.PckidxInfo._fields_] and ctypes.sizeof(_lib.PckidxInfo) == 8 * 8 + 8 * 4
    assert header in _lib.HEADERS and os.path.join(_lib.HERE, "csrc", "esa_pckidx.hip") in _lib.SOURCES
    assert os.path.join(_lib.HERE, "csrc", "esa_pckidx_core.h") in _lib.HEADERS


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_pckidx_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()


def shim_open(lib, raw):
    msg = ctypes.create_string_buffer(512)
    h = lib.pkx_shim_open(raw, len(raw), msg, 512)
    assert h, msg.value.decode()
    geom = np.zeros(len(GEOM), dtype=np.uint64)
    lib.pkx_shim_geom(h, geom.ctypes.data)
    return h, dict(zip(GEOM, (int(x) for x in geom)))


def text(n, sigma, seed, special=0.06):
    """n symbols over sigma letters with wildcards and separators, some of them in
    runs and next to each other"""
    rng = np.random.default_rng(seed)
    enc = rng.integers(0, sigma, n).astype(np.uint8)
    k = int(n * special)
    if k:
        at = rng.integers(0, n, k)
        enc[at] = rng.choice([254, 255], k, p=[0.7, 0.3])
        for a in at[::3]:
            enc[a:a + int(rng.integers(1, 4))] = 254
    return enc


def builder_accepts(sigma, B):
    """esa_pck.hip: composition indices of at most 18 bits, permutation indices of at most 40"""
    even = [B // sigma + (1 if s < B % sigma else 0) for s in range(sigma)]
    perms = factorial(B)
    for c in even:
        perms //= factorial(c)
    return max(1, (comb(B + sigma - 1, sigma - 1) - 1).bit_length()) <= 18 and max(1, (perms - 1).bit_length()) <= 40


_tables = {}


def tables(n, sigma, seed):
    key = (n, sigma, seed)
    if key not in _tables:
        enc = text(n, sigma, seed)
        _tables[key] = (enc, ou.esa(enc, sigma))
    return _tables[key]


def check_image(lib, enc, ora, sigma, **kw):
    raw = ou.pck_bdx(enc, sigma, ora["suf"], ora["bwt"], **kw)
    h, g = shim_open(lib, raw)
    try:
        N = enc.size + 1
        assert g["rows"] == N and g["sigma"] == sigma and g["B"] == kw["bsize"] and g["K"] == kw["blbuck"]
        assert g["locint"] == kw["locfreq"] and g["reversible"] == int(bool(kw.get("sprank")) and kw["locfreq"] > 0)
        bwt = np.full(N, 77, dtype=np.uint8)
        totals = np.zeros(32, dtype=np.uint64)
        assert lib.pkx_shim_decode(h, bwt.ctypes.data, totals.ctypes.data) == 0
        assert np.array_equal(bwt, ora["bwt"])
        assert totals[:sigma].tolist() == np.bincount(ora["bwt"], minlength=256)[:sigma].tolist()
        stored = np.full(N, NONE, dtype=np.uint64)
        rank = np.full(N, NONE, dtype=np.uint64)
        assert lib.pkx_shim_marks(h, stored.ctypes.data, rank.ctypes.data) == 0
        suf = ora["suf"]
        marked = stored != NONE
        if not kw["locfreq"]:
            assert not marked.any() and not (rank != NONE).any()
            return
        special = ora["bwt"] >= 254
        want = suf % np.uint64(kw["locfreq"]) == 0
        if not g["reversible"]:
            want |= special != (np.arange(N) >= g["first_special_row"])
        assert np.array_equal(marked, want)
        assert np.array_equal(stored[marked], suf[marked])
        assert g["rot0"] == int(np.flatnonzero(suf == 0)[0]) and marked[g["rot0"]]
        if g["reversible"]:
            # the rank of a special among the specials of the text; the undefined
            # symbol before suffix 0 comes behind them all
            before = np.concatenate([[0], np.cumsum(enc >= 254)])
            rows = np.flatnonzero(special)
            pos = suf[rows].astype(np.int64) - 1
            expect = np.where(pos >= 0, before[np.maximum(pos, 0)], before[-1])
            assert np.array_equal(rank[rows], expect.astype(np.uint64))
            assert not (rank[~special] != NONE).any()
        else:
            assert not (rank != NONE).any()
    finally:
        lib.pkx_shim_close(h)


def lengths(L):
    """n for n + 1 = L - 1, L, L + 1, 2 L and 257 buckets + 3"""
    return [max(1, v - 1) for v in (L - 1, L, L + 1, 2 * L, 257 * L + 3)]


FLAVOURS = [dict(locfreq=f, locbitmap=b, sprank=s) for f, b, s in
            itertools.product((0, 1, 7, 32), (True, False), (False, True)) if f or (b and not s)]
GEOMETRIES = [(B, K, sigma) for B, K, sigma in itertools.product((1, 5, 8, 10, 16), (1, 3, 8), (2, 4, 5, 20))
              if builder_accepts(sigma, B)]


def test_the_geometries_cover_what_is_asked():
    assert {g[0] for g in GEOMETRIES} == {1, 5, 8, 10, 16} and {g[1] for g in GEOMETRIES} == {1, 3, 8}
    assert {g[2] for g in GEOMETRIES} == {2, 4, 5, 20} and len(FLAVOURS) == 13


@pytest.mark.parametrize("B,K,sigma", GEOMETRIES)
def test_every_bucket_and_every_locate_record(shim, B, K, sigma):
    """each geometry with every sequence length: all 13 flavours at n + 1 = L - 1, L,
    L + 1 and 2 L; at 257 buckets + 3 three flavours, which take turns over the
    geometries (all 13 there: test_every_flavour_at_every_length)"""
    L = B * K
    turn = GEOMETRIES.index((B, K, sigma))
    for i, n in enumerate(lengths(L)):
        enc, ora = tables(n, sigma, 100 + n % 7)
        flavours = FLAVOURS if i < 4 else [FLAVOURS[(turn * 3 + j) % len(FLAVOURS)] for j in range(3)]
        for j, fl in enumerate(flavours):
            check_image(shim, enc, ora, sigma, bsize=B, blbuck=K, mkindex=bool((turn + i + j) % 2), **fl)


@pytest.mark.parametrize("flavour", FLAVOURS, ids=lambda f: "f%d%s%s" % (f["locfreq"], "b" if f["locbitmap"] else "c",
                                                                          "r" if f["sprank"] else ""))
def test_every_flavour_at_every_length(shim, flavour):
    """the option set of the reference's index searches (-bsize 10, 8 blocks) and
    the defaults, with every locate flavour, at every length"""
    for B, K in ((10, 8), (8, 8)):
        for n in lengths(B * K):
            enc, ora = tables(n, 4, 3)
            check_image(shim, enc, ora, 4, bsize=B, blbuck=K, mkindex=True, **flavour)
    enc, ora = tables(257 * 128 + 2, 5, 4)
    check_image(shim, enc, ora, 5, bsize=16, blbuck=8, mkindex=False, **flavour)


def test_specials_next_to_each_other_and_at_both_ends(shim):
    enc = text(3000, 4, 9)
    enc[0], enc[1], enc[-1], enc[-2] = 254, 255, 255, 254
    enc[100:140] = 254
    enc[140:143] = 255
    ora = ou.esa(enc, 4)
    for fl in FLAVOURS:
        check_image(shim, enc, ora, 4, bsize=10, blbuck=8, mkindex=True, **fl)
    one = np.zeros(1, dtype=np.uint8)
    check_image(shim, one, ou.esa(one, 4), 4, bsize=8, blbuck=8, locfreq=16, locbitmap=None, mkindex=True)


# ---- header validation ----------------------------------------------------------

def header_fields(raw):
    """(name, offset, bytes, limit) of every field the reader validates; limit
    None: the field has one valid value, its own"""
    B, = struct.unpack_from("<I", raw, 12)
    sigma, = struct.unpack_from("<I", raw, 80)
    spbt, = struct.unpack_from("<I", raw, 64)
    out = [("magic", 0, 4, None), ("header size", 4, 4, None),
           ("tag BKSZ", 8, 4, None), ("block size", 12, 4, 16), ("tag BBLK", 16, 4, None),
           ("blocks per bucket", 20, 4, 16384 // B), ("tag VOFF", 24, 4, None), ("var data position", 28, 8, None),
           ("tag ROFF", 36, 4, None), ("region list position", 40, 8, len(raw) - 24),
           ("tag SELE", 48, 4, None), ("sequence length", 52, 8, 2 ** 32 - 4096),
           ("tag SPBT", 60, 4, None), ("bits per position", 64, 4, None),
           ("tag VDOB", 68, 4, None), ("var offset bits", 72, 4, 64),
           ("tag SSBT", 76, 4, None), ("alphabet size", 80, 4, 30)]
    o = 84
    for s in range(sigma):
        out.append(("counter bits of letter %d" % s, o, 4, spbt))
        o += 4
    out += [("tag BEFB", o, 4, None), ("BEFB", o + 4, 4, 0), ("tag REFB", o + 8, 4, None), ("REFB", o + 12, 4, 0),
            ("tag NMRN", o + 16, 4, None), ("range modes", o + 20, 4, None), ("mode of letters", o + 24, 4, None),
            ("mode of specials", o + 28, 4, None)]
    o += 32
    if struct.unpack_from("<I", raw, o)[0] == 0x43424d42:
        out += [("tag CBMB", o, 4, None), ("permutation bits width", o + 4, 4, None), ("tag CEXB", o + 8, 4, None),
                ("record extension bits", o + 12, 8, None), ("tag MEXB", o + 20, 4, None)]
        o += 32
        N, = struct.unpack_from("<Q", raw, 52)
        out += [("tag of the locate header", o, 4, None), ("locate header size", o + 4, 4, None),
                ("row of suffix 0", o + 8, 8, N - 1), ("locate interval", o + 16, 4, "nonzero"),
                ("feature toggles", o + 20, 4, None)]
        o += 24
        if struct.unpack_from("<I", raw, o)[0] == (0x45480000 | 1112):
            out += [("tag of the sort-mode header", o, 4, None), ("sort-mode header size", o + 4, 4, None),
                    ("rank bits", o + 8, 4, None), ("sort modes", o + 12, 4, None)]
    return out


def good_images():
    enc, ora = tables(5000, 4, 21)
    assert ora["bwt"][0] < 254              # (so that row 0 is no row for suffix 0)
    yield ou.pck_bdx(enc, 4, ora["suf"], ora["bwt"], bsize=10, blbuck=8, locfreq=32, sprank=True, mkindex=True)
    yield ou.pck_bdx(enc, 4, ora["suf"], ora["bwt"])
    yield ou.pck_bdx(enc, 4, ora["suf"], ora["bwt"], locfreq=0)
    yield ou.pck_bdx(enc, 4, ora["suf"], ora["bwt"], locbitmap=True, mkindex=True)


def refused(raw):
    with pytest.raises(_lib.EsaError, match="packed index reader: .{10,}"):
        pck.check_image(bytes(raw))


def test_header_fields_are_validated_one_at_a_time():
    tried = 0
    for raw in good_images():
        pck.check_image(raw)
        for name, off, size, limit in header_fields(raw):
            fmt = "<I" if size == 4 else "<Q"
            own, = struct.unpack_from(fmt, raw, off)
            ones = 2 ** (8 * size) - 1
            if limit == "nonzero":
                variants = [0]
            else:
                variants = [0, (own if limit is None else limit) + 1, ones]
            for v in variants:
                if v == own:
                    continue
                bad = bytearray(raw)
                struct.pack_into(fmt, bad, off, v)
                try:
                    refused(bad)
                except BaseException:
                    print("field %r set to %d (was %d)" % (name, v, own))
                    raise
                tried += 1
    assert tried > 300


def test_truncated_images_are_refused(shim):
    for raw in good_images():
        h, g = shim_open(shim, raw)
        shim.pkx_shim_close(h)
        borders = [8, 100, g["cw_base_bit"] // 8, g["var_base_bit"] // 8, g["range_enc_pos"], g["range_enc_pos"] + 8,
                   g["range_enc_pos"] + 24, len(raw) - 16, len(raw) - 1]
        for cut in borders:
            assert 0 < cut < len(raw)
            refused(raw[:cut])
        refused(raw + b"\0")


# ---- the decoder as a program under the sanitizers ---------------------------------

SAN_FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-static-libasan", "-DPKX_SHIM_MAIN"]


def write_bits(raw, pos, n, v):
    for k in range(n):
        bit = (v >> (n - 1 - k)) & 1
        byte, sh = (pos + k) >> 3, 7 - ((pos + k) & 7)
        raw[byte] = (raw[byte] & ~(1 << sh)) | (bit << sh)


def lying_buckets(raw, g, suf_marks):
    """(what, image) for buckets whose var offset, mark count and mark rows are
    made to decrease, to point behind the var part (behind the bucket) and to all ones"""
    L, N, nb = g["B"] * g["K"], g["rows"], g["buckets"]
    var_bits = g["var_end_bit"] - g["var_base_bit"]

    def field(bucket, pre, width, v, what):
        bad = bytearray(raw)
        at = g["cw_base_bit"] + bucket * g["cw_bits"] + pre
        if read_bits(raw, at, width) != v & (2 ** width - 1):
            write_bits(bad, at, width, v & (2 ** width - 1))
            yield "%s of bucket %d" % (what, bucket), bytes(bad)

    last = (N - 1) // L
    for b in sorted({0, 1, nb // 2, last}):
        rec = g["cw_base_bit"] + b * g["cw_bits"]
        own = read_bits(raw, rec + g["pre_var_idx"], g["var_off_bits"])
        for v, what in ((own - 1, "var offset decreased"), (var_bits + 9, "var offset behind the var part"),
                        (2 ** g["var_off_bits"] - 1, "var offset of all ones")):
            if v >= 0:
                yield from field(b, g["pre_var_idx"], g["var_off_bits"], v, what)
        if not g["count"]:
            continue
        ln = min(L, N - b * L)
        bc, bw = ln.bit_length(), max(1, (ln - 1).bit_length())
        at = g["var_base_bit"] + own + read_bits(raw, rec + g["pre_cb_off"], g["cb_off_bits"])
        nm = read_bits(raw, at, bc)
        for v, what in ((nm - 1, "mark count decreased"), (2 ** bc - 1, "mark count of all ones"),
                        (nm + 1, "mark count increased")):
            if 0 <= v < 2 ** bc and v != nm:
                bad = bytearray(raw)
                write_bits(bad, at, bc, v)
                yield "%s in bucket %d" % (what, b), bytes(bad)
        if nm >= 2:
            step = bw + g["bits_orig_pos"]
            first = read_bits(raw, at + bc, bw)
            for k, v, what in ((1, first, "mark row decreased"), (0, 2 ** bw - 1, "mark row of all ones"),
                               (0, ln, "mark row behind the bucket")):
                if v < 2 ** bw:
                    bad = bytearray(raw)
                    write_bits(bad, at + bc + k * step, bw, v)
                    yield "%s in bucket %d" % (what, b), bytes(bad)


def test_the_decoder_as_a_program_under_asan_and_ubsan(shim, tmp_path):
    exe = str(tmp_path / "pckidx_decoder")
    subprocess.run(["g++"] + SAN_FLAGS + ["-o", exe, SHIM_SRC], check=True)
    enc, ora = tables(5000, 4, 21)
    cases = []
    for kw in (dict(bsize=10, blbuck=8, locfreq=32, sprank=True, mkindex=True, locbitmap=False),
               dict(bsize=8, blbuck=8, locfreq=7, locbitmap=False), dict(locfreq=16, locbitmap=True),
               dict(locfreq=0), dict(bsize=5, blbuck=3, locfreq=1, locbitmap=False, sprank=True)):
        raw = ou.pck_bdx(enc, 4, ora["suf"], ora["bwt"], **kw)
        h, g = shim_open(shim, raw)
        shim.pkx_shim_close(h)
        cases.append(("good", raw))
        cases += list(lying_buckets(raw, g, ora["suf"]))
    assert len(cases) > 60 and {w.split(" in ")[0].split(" of bucket")[0] for w, _ in cases} >= {
        "var offset decreased", "var offset behind the var part", "var offset of all ones", "mark count decreased",
        "mark count of all ones", "mark row decreased", "mark row of all ones"}
    paths = []
    for i, (_, raw) in enumerate(cases):
        paths.append(str(tmp_path / ("case%03d.bdx" % i)))
        with open(paths[-1], "wb") as f:
            f.write(raw)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for (what, _), line in zip(cases, lines):
        _, rc, err, msg = line.split("\t")
        if what == "good":
            assert (rc, err) == ("0", "0"), line
        else:
            assert rc == "-1" and (int(err) > 0 or msg), (what, line)
