"""The device-wide primitives of genometools_amd/csrc/esa_prims.hip -- scan_u32,
offsets_u64(_counted), radix_sort_pairs in its four instances,
radix_partition_u32, radix_pass_group_heads, radix_scan_tile_rows / _hist --
called directly, as libgtamd_esa.so exports them, through the host glue of
tests/prims_shim.cpp (host arrays in, one primitive on a stream, host arrays
out; no torch buffers), and compared EXACTLY with numpy:

  scan            np.cumsum / np.maximum.accumulate in 64 bits, cut to 32
  offsets         np.cumsum in 64 bits
  row scan        out[t][d] = sum_{d'<d} total[d'] + sum_{t'<t} hist[t'][d]
  sort            a loop over the passes of np.argsort(digit, kind="stable")
  partition       the same pairs per digit, in any order inside a digit
  group heads     head of entry i = the largest j <= i whose tie bit is clear

Values of a sort are the original indices, so stability shows.  Every workspace
has exactly the words its *_workspace_words function names and 64 guard words
behind them, which have to come back unchanged.  Every test counts the cases it
ran in TALLY; the last test of the module holds the tally against the lists
below, so that a list that went empty cannot pass."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou

pytestmark = pytest.mark.gpu

ROOT = ou.ROOT
CSRC = os.path.join(ROOT, "genometools_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "prims_shim.cpp")] + \
      [os.path.join(CSRC, h) for h in ("esa_prims.h", "esa_own.h", "esa_common.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libprims_shim.so")

TILE = 4096                       # pairs of a sort tile, elements of a scan tile
TALLY = collections.Counter()     # (primitive, instance or form, size) -> calls checked

# key and value types of the four instances, and the shim's code for each
INSTANCES = {"u64_u32": (84, np.uint64, np.uint32), "u32_u32": (44, np.uint32, np.uint32),
             "u32_u64": (48, np.uint32, np.uint64), "u64_u64": (88, np.uint64, np.uint64)}
SCAN_SIZES = (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8191,
              TILE * TILE - 1, TILE * TILE, TILE * TILE + 1)      # the last: a third level
OFFSET_COUNTS = (1, 2, 255, 256, 257, 65535, 65536, 65537, 3 * 65536 + 5)
ROW_COUNTS = (1, 7, 8, 9, 511, 512, 513, 1024, 2047, 2048, 2049, 5 * 512 + 3)
# 9 tiles + 70: the XCD tile order leaves workgroups without a tile
SORT_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8 * TILE - 1, 8 * TILE, 8 * TILE + 1,
              9 * TILE + 70)
SORT_SIZE_CHUNKS = 512 * TILE - 1                           # a column-scan chunk, full but for one pair
SORT_SIZES_LARGE = (512 * TILE + 1, 2049 * TILE + 5)        # two chunks; five, in uneven quarters
LARGE_INSTANCES = ("u64_u32", "u32_u32")
LAST_TILE = (1, 5, 64, 70, 1030, 4095)
FAMILIES = ("uniform", "equal", "two", "ones", "sorted", "reverse")
PASS_COUNTS = (1, 2, 3, 8)


def _stale():
    return not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in SRC)


@pytest.fixture(scope="module")
def shim(gpu):
    """the glue, built by its goal of oracle/Makefile if it is missing or older
    than its sources; behind `gpu`, which has loaded the library the way the
    package does"""
    if _stale():
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "prims_shim"], capture_output=True, text=True)
        if p.returncode != 0:
            pytest.fail("tests/prims_shim.cpp does not build:\n" + p.stdout + p.stderr)
    lib = ctypes.CDLL(SHIM)
    P, U32, U64, INT = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    lib.ps_guard_seed.restype = U32
    lib.ps_workspace_words.argtypes = [U64, P]
    lib.ps_workspace_words.restype = None
    lib.ps_scan.argtypes = [INT, P, P, U64, U64, INT, INT, P]
    lib.ps_offsets.argtypes = [INT, P, U64, P, P, P]
    lib.ps_scan_rows.argtypes = [INT, P, U32, U64, P]
    lib.ps_sort.argtypes = [INT, P, P, P, P, P, P, U64, U64, P, P, INT, INT, P, P]
    lib.ps_sort_no_pointers.argtypes = [INT, U64, INT]
    lib.ps_partition.argtypes = [P, P, P, P, U64, U64, INT, INT, P]
    lib.ps_group_heads.argtypes = [P, P, P, U64, U32, P, P, P, U64, INT, INT, P]
    assert lib.ps_guard_words() == 64
    lib.last_error = lambda: gpu.gtamd_esa_last_error().decode()
    lib.guard = np.arange(64, dtype=np.uint32) + np.uint32(lib.ps_guard_seed())
    return lib


def _p(a):
    return a.ctypes.data


def _ok(shim, rc, guard, what):
    assert rc == 0, (what, rc, shim.last_error() if rc == -1 else "the glue failed: its message is on stderr")
    assert np.array_equal(guard, shim.guard), (what, "the words behind the workspace were written")


def _rng(*seed):
    return np.random.default_rng([20240607] + [int(s) for s in seed])


# ---------------------------------------------------------------------------
# workspace sizes (host only)
# ---------------------------------------------------------------------------
def test_workspace_sizes(shim):
    """scan: ceil(n / 4096) + 16 words per level above the first, and 16; sort: 256
    counters per tile, (ntiles / 512 + 2) rows of chunk sums, and 64"""
    got = np.zeros(3, dtype=np.uint64)
    for n in sorted(set(SCAN_SIZES + SORT_SIZES + SORT_SIZES_LARGE + (0, SORT_SIZE_CHUNKS))):
        shim.ps_workspace_words(n, _p(got))
        words, m = 16, n
        while m > TILE:
            m = -(-m // TILE)
            words += m + 16
        tiles = -(-n // TILE)
        assert got.tolist() == [words, tiles * 256 + (tiles // 512 + 2) * 256 + 64, (n // 512 + 2) * 256 + 64], n
        TALLY["sizes", "host", n] += 1


# ---------------------------------------------------------------------------
# scan_u32
# ---------------------------------------------------------------------------
SCAN_FAMILIES = {"sum": ("random", "sparse"), "max": ("sparse", "edges")}


def _scan_input(op, family, n):
    """(input, inclusive scan in 64 bits cut to 32); sums stay below 2^32"""
    rng = _rng(n, op == "max", family == "sparse")
    if op == "sum":
        v = rng.integers(0, max(2, (2 ** 32 - 1) // n), size=n, dtype=np.uint64)
        if family == "sparse":                   # runs of zeros, longer than a tile where n allows
            v[rng.random(n) < 0.999] = 0
        incl = np.cumsum(v, dtype=np.uint64)
        assert int(incl[-1]) < 2 ** 32
    else:
        v = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
        if family == "sparse":                   # runs of zeros between rare values of every size
            v >>= rng.integers(0, 32, size=n, dtype=np.uint64)
            v[rng.random(n) < 0.99] = 0
        else:                                    # a new maximum in the first and in the last element of every tile
            v >>= np.uint64(2)
            first = np.arange(0, n, TILE, dtype=np.uint64)
            v[::TILE] = np.uint64(1 << 31) + np.uint64(2) * (first // np.uint64(TILE))
            last = np.arange(TILE - 1, n, TILE, dtype=np.uint64)
            v[TILE - 1::TILE] = np.uint64(1 << 31) + np.uint64(2) * (last // np.uint64(TILE)) + np.uint64(1)
        incl = np.maximum.accumulate(v)
    return v.astype(np.uint32), incl.astype(np.uint32)


@pytest.mark.parametrize("op,family", [(op, f) for op in ("sum", "max") for f in SCAN_FAMILIES[op]])
def test_scan(shim, op, family):
    """exclusive and inclusive, in == out and separate, at every size"""
    poison = np.uint32(0xDEADBEEF)
    guard = np.zeros(64, dtype=np.uint32)
    variants = [(inclusive, inplace) for inclusive in (False, True) for inplace in (False, True)]
    ran = set()
    for n in SCAN_SIZES:
        v, incl = _scan_input(op, family, n)
        excl = np.concatenate([np.zeros(1, np.uint32), incl[:-1]])
        for inclusive, inplace in variants:
            want = incl if inclusive else excl
            out = np.full(n + 3, poison, dtype=np.uint32)
            rc = shim.ps_scan(int(op == "max"), _p(v), _p(out), n, n + 3, int(inclusive), int(inplace), _p(guard))
            _ok(shim, rc, guard, (op, family, n, inclusive, inplace))
            bad = np.flatnonzero(out[:n] != want)
            assert bad.size == 0, (op, family, n, inclusive, inplace, "first wrong element", int(bad[0]),
                                   int(out[bad[0]]), int(want[bad[0]]))
            assert (out[n:] == poison).all(), (op, family, n, "written behind the end")
            ran.add(n)
            TALLY["scan", op, n] += 1
    # n = 0: nothing is launched, `out` stays as it was
    for inclusive, inplace in variants:
        out = np.full(3, poison, dtype=np.uint32)
        rc = shim.ps_scan(int(op == "max"), _p(out), _p(out), 0, 3, int(inclusive), int(inplace), _p(guard))
        _ok(shim, rc, guard, (op, 0))
        assert (out == poison).all()
        TALLY["scan", op, 0] += 1
    assert ran == set(SCAN_SIZES)


# ---------------------------------------------------------------------------
# offsets_u64, offsets_u64_counted
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["all_ones_32", "below_2_20"])
@pytest.mark.parametrize("form", ["plain", "counted"])
def test_offsets(shim, form, family):
    ran = set()
    for count in OFFSET_COUNTS:
        if family == "all_ones_32":
            cnt = np.full(count, 0xFFFFFFFF, dtype=np.uint32)
        else:
            cnt = _rng(count, 7).integers(0, 1 << 20, size=count, dtype=np.uint32)
        want = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])
        tile_sums = np.add.reduceat(cnt.astype(np.uint64), np.arange(0, count, 256))
        # plain: the caller's kernel has summed the tiles; counted: the primitive does, over whatever is there
        tsum = tile_sums.copy() if form == "plain" else np.full(tile_sums.size, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        off = np.zeros(count + 1, dtype=np.uint64)
        total = np.zeros(1, dtype=np.uint64)
        rc = shim.ps_offsets(int(form == "counted"), _p(cnt), count, _p(tsum), _p(off), _p(total))
        assert rc == 0, (count, rc, shim.last_error())
        bad = np.flatnonzero(off != want)
        assert bad.size == 0, (count, "first wrong offset", int(bad[0]), int(off[bad[0]]), int(want[bad[0]]))
        assert int(total[0]) == int(off[count]) == int(cnt.astype(np.uint64).sum())
        # afterwards tsum holds the sum of the tiles in front of each tile
        assert np.array_equal(tsum, np.cumsum(tile_sums) - tile_sums), count
        ran.add(count)
        TALLY["offsets", form, count] += 1
    assert int(want[-1]) > 2 ** 32          # (the largest count's total does not fit 32 bits)
    assert ran == set(OFFSET_COUNTS)


# ---------------------------------------------------------------------------
# radix_scan_tile_rows, radix_scan_tile_hist
# ---------------------------------------------------------------------------
def _tile_histogram(rows, rng):
    """counts per row that sum to at most 4096: spread over all digits, over a
    few, or all 4096 pairs of a tile in one digit"""
    hist = np.zeros((rows, 256), dtype=np.uint32)
    kind = rng.integers(0, 4, size=rows)
    few = rng.dirichlet(np.full(256, 0.05))
    for t in range(rows):
        if kind[t] == 0:
            hist[t, rng.integers(0, 256)] = TILE
        elif kind[t] == 1:
            hist[t] = rng.multinomial(TILE, few)
        else:
            hist[t] = rng.multinomial(rng.integers(0, TILE + 1), np.full(256, 1 / 256))
    return hist


@pytest.mark.parametrize("form", ["rows", "hist"])
def test_scan_tile_rows(shim, form):
    guard = np.zeros(64, dtype=np.uint32)
    ran = set()
    for rows in ROW_COUNTS:
        hist = _tile_histogram(rows, _rng(rows, 11))
        h = hist.astype(np.uint64)
        total = h.sum(axis=0)
        want = (np.cumsum(total) - total)[None, :] + (np.cumsum(h, axis=0) - h)
        assert int(h.sum()) < 2 ** 32
        got = hist.copy()
        # (as the histogram of a sort of n pairs: n anywhere inside the last tile)
        n = rows * TILE - (rows * 37) % TILE
        rc = shim.ps_scan_rows(int(form == "hist"), _p(got), rows, n, _p(guard))
        _ok(shim, rc, guard, (form, rows))
        bad = np.argwhere(got != want)
        assert bad.size == 0, (form, rows, "first wrong (row, digit)", bad[0].tolist(),
                               int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))
        ran.add(rows)
        TALLY["rows", form, rows] += 1
    assert ran == set(ROW_COUNTS)


# ---------------------------------------------------------------------------
# radix_sort_pairs
# ---------------------------------------------------------------------------
def _passes(bits, npasses):
    """(shifts, widths): a pass at the highest shift (56 / 24); two passes whose
    digits skip bits of the key; the widths 1 to 8 mixed in one call"""
    return {1: ([bits - 8], [8]),
            2: ([3, bits - 19], [7, 5]),
            3: ([0, 1, 4], [1, 3, 8]),
            8: ([0, 1, 3, 6, 10, 15, 21, bits - 8], [1, 2, 3, 4, 5, 6, 7, 8])}[npasses]


def _keys(family, n, dtype, rng):
    bits = 8 * np.dtype(dtype).itemsize
    if family == "uniform":
        return rng.integers(0, 2 ** bits, size=n, dtype=dtype)
    if family == "equal":                 # every full tile: 4096 pairs on one digit
        return np.full(n, rng.integers(0, 2 ** bits, dtype=dtype), dtype=dtype)
    if family == "two":                   # two keys that differ in every digit
        a = rng.integers(0, 2 ** bits, dtype=dtype)
        return np.where(rng.random(n) < 0.5, a, ~a).astype(dtype)
    if family == "ones":
        return np.full(n, 2 ** bits - 1, dtype=dtype)
    k = np.sort(rng.integers(0, 2 ** bits, size=n, dtype=dtype))
    return k if family == "sorted" else k[::-1].copy()


def _digit(keys, shift, width):
    return ((keys >> keys.dtype.type(shift)) & keys.dtype.type((1 << width) - 1)).astype(np.uint8)


def _sorted_order(keys, shifts, widths):
    """the reference: one stable argsort per pass, least significant digit first"""
    perm = np.arange(keys.size)
    for shift, width in zip(shifts, widths):
        perm = perm[np.argsort(_digit(keys[perm], shift, width), kind="stable")]
    return perm


def _sort(shim, inst, keys, shifts, widths, off=0, events=False):
    """sorts (keys, original indices); returns the pairs from the buffer the header
    names for the parity of the pass count, and *n_ev"""
    code, K, V = INSTANCES[inst]
    n = keys.size
    vals = np.arange(n, dtype=V)
    ka, kb = np.zeros(n, dtype=K), np.zeros(n, dtype=K)
    va, vb = np.zeros(n, dtype=V), np.zeros(n, dtype=V)
    guard = np.zeros(64, dtype=np.uint32)
    n_ev = ctypes.c_int(-1)
    sh = (ctypes.c_int * len(shifts))(*shifts)
    wd = (ctypes.c_int * len(widths))(*widths)
    rc = shim.ps_sort(code, _p(keys), _p(vals), _p(ka), _p(va), _p(kb), _p(vb), n, off, sh, wd, len(shifts),
                      int(events), ctypes.byref(n_ev), _p(guard))
    _ok(shim, rc, guard, (inst, n, shifts, widths, off))
    return (ka, va) if len(shifts) % 2 == 0 else (kb, vb), n_ev.value


def _check_sort(shim, inst, keys, npasses, what, **kw):
    bits = 8 * keys.dtype.itemsize
    shifts, widths = _passes(bits, npasses)
    (got_k, got_v), n_ev = _sort(shim, inst, keys, shifts, widths, **kw)
    perm = _sorted_order(keys, shifts, widths)
    bad = np.flatnonzero((got_v != perm.astype(got_v.dtype)) | (got_k != keys[perm]))
    assert bad.size == 0, (inst, what, npasses, "first wrong pair at", int(bad[0]), "of", keys.size,
                           hex(int(got_k[bad[0]])), int(got_v[bad[0]]), "expected",
                           hex(int(keys[perm[bad[0]]])), int(perm[bad[0]]))
    return n_ev


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_sort_sizes_families_and_passes(shim, inst):
    """every size around the wave, the wave chunk and the tile, in every family
    of keys, with 1, 2, 3 and 8 passes"""
    K = INSTANCES[inst][1]
    ran = set()
    for n in SORT_SIZES:
        for f, family in enumerate(FAMILIES):
            keys = _keys(family, n, K, _rng(n, f, INSTANCES[inst][0]))
            for npasses in PASS_COUNTS:
                _check_sort(shim, inst, keys, npasses, (family, n))
                ran.add((n, family, npasses))
                TALLY["sort", inst, n] += 1
    assert len(ran) == len(SORT_SIZES) * len(FAMILIES) * len(PASS_COUNTS)


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_sort_a_full_column_scan_chunk(shim, inst):
    """512 tiles, the last one pair short: one chunk of the column scan, and
    the scatter's last tile with 4095 pairs"""
    K = INSTANCES[inst][1]
    for f, family in enumerate(FAMILIES):
        keys = _keys(family, SORT_SIZE_CHUNKS, K, _rng(SORT_SIZE_CHUNKS, f))
        _check_sort(shim, inst, keys, 2, family)
        TALLY["sort", inst, SORT_SIZE_CHUNKS] += 1


@pytest.mark.parametrize("n", SORT_SIZES_LARGE)
@pytest.mark.parametrize("inst", LARGE_INSTANCES)
def test_sort_several_column_scan_chunks(shim, inst, n):
    """two chunks (k_cs_chunkbase: two of its four parts have one each), and
    five chunks (parts of 2, 2, 1 and 0); an odd pass count"""
    K = INSTANCES[inst][1]
    for f, family in enumerate(("uniform", "equal")):
        keys = _keys(family, n, K, _rng(n, f))
        _check_sort(shim, inst, keys, 3, family)
        TALLY["sort", inst, n] += 1


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_sort_unaligned_pointers(shim, inst):
    """key and value pointers one element off: k_rs_hist cannot load 16 bytes
    and takes its element-wise path over full tiles"""
    K = INSTANCES[inst][1]
    for n in (TILE, 8 * TILE + 1, 9 * TILE + 70):
        for f, family in enumerate(("uniform", "two")):
            keys = _keys(family, n, K, _rng(n, f, 3))
            for npasses in (2, 3):
                _check_sort(shim, inst, keys, npasses, (family, n, "off by one"), off=1)
                TALLY["sort_unaligned", inst, n] += 1


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_sort_last_tile_of_all_ones(shim, inst):
    """a part-filled last tile whose valid keys are all ones: with 8-bit digits
    they share digit 255 with the invalid pairs the scatter parks there, and
    must come out in front of them, in input order; alone and behind full tiles"""
    K = INSTANCES[inst][1]
    bits = 8 * np.dtype(K).itemsize
    for full_tiles in (0, 2):
        for r in LAST_TILE:
            n = full_tiles * TILE + r
            keys = np.full(n, 2 ** bits - 1, dtype=K)
            for npasses in PASS_COUNTS:
                _check_sort(shim, inst, keys, npasses, ("ones", n))
            # and the same behind tiles of other keys
            if full_tiles:
                keys[:full_tiles * TILE] = _keys("uniform", full_tiles * TILE, K, _rng(r, 5))
                _check_sort(shim, inst, keys, 1, ("uniform then ones", n))
            TALLY["sort_last_tile", inst, r] += 1


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_sort_records_an_event_pair_per_pass(shim, inst):
    K = INSTANCES[inst][1]
    keys = _keys("uniform", TILE + 1, K, _rng(17))
    for npasses in PASS_COUNTS:
        assert _check_sort(shim, inst, keys, npasses, "events", events=True) == npasses
        assert _check_sort(shim, inst, keys, npasses, "no events") == 0
        TALLY["sort_events", inst, npasses] += 1


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_sort_refuses_2_32_pairs_and_ignores_none(shim, inst):
    """both answers come before anything is launched or read (radix_sort_pairs
    tests n first), so the call is made without a single valid pointer"""
    code = INSTANCES[inst][0]
    assert shim.ps_sort_no_pointers(code, 0, 3) == 0
    assert shim.ps_sort_no_pointers(code, 1 << 32, 3) == -1
    assert "4294967296 pairs exceed the 32-bit index range" in shim.last_error()
    TALLY["sort_refusal", inst, 1 << 32] += 1


# ---------------------------------------------------------------------------
# radix_partition_u32
# ---------------------------------------------------------------------------
def _packed(keys, vals):
    return np.sort((keys.astype(np.uint64) << np.uint64(32)) | vals.astype(np.uint64))


def _check_partitioned(got_k, got_v, keys, vals, shift, width, what):
    """what an unstable partition shares with the reference (a stable argsort on
    the digit): the digits come out in order, and every digit holds the same
    multiset of (key, value) pairs.  With the digits in order, the pairs of digit
    d are one stretch of the output and all its pairs of that digit, so the
    multisets agree digit by digit exactly if they agree over the whole array"""
    d = _digit(got_k, shift, width)
    assert (d[1:] >= d[:-1]).all(), (what, "digits are not in order")
    assert np.array_equal(np.bincount(d, minlength=256), np.bincount(_digit(keys, shift, width), minlength=256)), what
    got, want = _packed(got_k, got_v), _packed(keys, vals)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first difference of the sorted pairs at", int(bad[0]), hex(int(got[bad[0]])),
                           hex(int(want[bad[0]])))


PARTITION_DIGITS = ((0, 8), (24, 8), (5, 3), (13, 1))


def _check_partition(shim, keys, shift, width, what, off=0):
    n = keys.size
    vals = np.arange(n, dtype=np.uint32)
    got_k, got_v = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    guard = np.zeros(64, dtype=np.uint32)
    rc = shim.ps_partition(_p(keys), _p(vals), _p(got_k), _p(got_v), n, off, shift, width, _p(guard))
    _ok(shim, rc, guard, what)
    _check_partitioned(got_k, got_v, keys, vals, shift, width, what)


def test_partition_sizes_and_families(shim):
    ran = set()
    for n in SORT_SIZES:
        for f, family in enumerate(FAMILIES):
            keys = _keys(family, n, np.uint32, _rng(n, f, 21))
            for shift, width in PARTITION_DIGITS:
                _check_partition(shim, keys, shift, width, (family, n, shift, width))
            ran.add((n, family))
            TALLY["partition", "u32_u32", n] += 1
        _check_partition(shim, _keys("uniform", n, np.uint32, _rng(n, 22)), 0, 8, ("off by one", n), off=1)
    assert len(ran) == len(SORT_SIZES) * len(FAMILIES)


@pytest.mark.parametrize("n", (SORT_SIZE_CHUNKS,) + SORT_SIZES_LARGE)
def test_partition_column_scan_chunks(shim, n):
    for f, family in enumerate(("uniform", "equal")):
        keys = _keys(family, n, np.uint32, _rng(n, f, 23))
        _check_partition(shim, keys, 24 if f else 0, 8, (family, n))
        TALLY["partition", "u32_u32", n] += 1


def test_partition_last_tile_of_all_ones(shim):
    for full_tiles in (0, 2):
        for r in LAST_TILE:
            keys = np.full(full_tiles * TILE + r, 0xFFFFFFFF, dtype=np.uint32)
            for shift, width in PARTITION_DIGITS:
                _check_partition(shim, keys, shift, width, ("ones", keys.size, shift, width))
            TALLY["partition_last_tile", "u32_u32", r] += 1


def test_partition_of_no_pairs(shim):
    guard = np.zeros(64, dtype=np.uint32)
    a = np.zeros(1, dtype=np.uint32)
    assert shim.ps_partition(_p(a), _p(a), _p(a), _p(a), 0, 0, 0, 8, _p(guard)) == 0
    assert np.array_equal(guard, shim.guard)
    TALLY["partition", "u32_u32", 0] += 1


# ---------------------------------------------------------------------------
# radix_pass_group_heads
# ---------------------------------------------------------------------------
def _pack_bits(bits, nwords):
    padded = np.zeros(nwords * 64, dtype=np.uint8)
    padded[:bits.size] = bits
    return np.packbits(padded.reshape(nwords, 64), axis=1, bitorder="little").view("<u8").ravel().copy()


def _check_group_heads(shim, n, starts, offset, with_swaps, shift, width, rng, what):
    """starts: the entries that begin a tie group (entry 0 always does)"""
    tie = np.ones(n, dtype=bool)          # "entry i has the key of entry i - 1"
    tie[0] = False
    tie[np.asarray(starts, dtype=np.int64)] = False
    nwords = (n + 63) // 64
    idx = np.arange(n, dtype=np.int64)
    head = np.maximum.accumulate(np.where(tie, 0, idx))     # the largest j <= i whose bit is clear
    carry = np.zeros(nwords, dtype=np.uint32)
    carry[1:] = head[64 * np.arange(1, nwords) - 1]         # the head of entry 64 w - 1
    tiebits = _pack_bits(tie, nwords)
    vals = (offset + head).astype(np.uint32)
    swp = None
    if with_swaps:
        first = rng.random(n) < 0.2
        second = (rng.random(n) < 0.2) & ~first
        swp = np.stack([_pack_bits(first, nwords), _pack_bits(second, nwords)], axis=1).ravel().copy()
        vals = (vals.astype(np.int64) + first - second).astype(np.uint32)
    keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
    got_k, got_v = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    guard = np.zeros(64, dtype=np.uint32)
    rc = shim.ps_group_heads(_p(keys), _p(tiebits), _p(carry), nwords, offset, None if swp is None else _p(swp),
                             _p(got_k), _p(got_v), n, shift, width, _p(guard))
    _ok(shim, rc, guard, what)
    _check_partitioned(got_k, got_v, keys, vals, shift, width, what)


# entries of a last tile in which some lane j of the first wave has no entry of
# item j (entry 65 j) while other lanes have one: 64 j < entries <= 65 j; and
# the same in the second wave (entries 1024 + ...)
LANE_SITS_OUT = (65, 129, 130, 325, 449, 455, 1024 + 65, 1024 + 130)
HEADS_LAST_TILE = (1, 5, 64, 70, 1030) + LANE_SITS_OUT


@pytest.mark.parametrize("with_swaps", [False, True], ids=["swp_null", "swp"])
@pytest.mark.parametrize("offset", [0, 3_000_000_000])
def test_group_heads(shim, offset, with_swaps):
    rng = _rng(offset, with_swaps)
    digits = ((0, 8), (11, 5))
    # groups of length 1; groups of up to a few words; n around the word, the tile and the XCD tile order
    for n in (1, 2, 63, 64, 65, 100, 1000, TILE - 1, TILE, TILE + 1, 3 * TILE + 77, 9 * TILE + 70):
        for j, (shift, width) in enumerate(digits):
            _check_group_heads(shim, n, np.arange(n), offset, with_swaps, shift, width, rng, ("singles", n))
            starts = np.flatnonzero(rng.random(n) < (0.3, 0.004)[j])
            _check_group_heads(shim, n, starts, offset, with_swaps, shift, width, rng, ("random groups", n))
        TALLY["group_heads", "sizes", n] += 1
    # one group over a whole tile and more: from inside tile 0 to inside tile 2
    n = 3 * TILE + 100
    _check_group_heads(shim, n, [5, 3000, 2 * TILE + 9, 2 * TILE + 11], offset, with_swaps, 0, 8, rng, "a whole tile")
    # the whole table one group
    _check_group_heads(shim, n, [], offset, with_swaps, 24, 8, rng, "one group")
    TALLY["group_heads", "whole_tile", n] += 1
    # a group that begins in the tile before and reaches into the table's last word, the last tile part-filled
    for r in HEADS_LAST_TILE:
        n = 2 * TILE + r
        for starts in ([TILE + 4000], [3, 2 * TILE - 1], [7, 2 * TILE]):
            _check_group_heads(shim, n, starts, offset, with_swaps, 0, 8, rng, ("into the last word", r, starts))
        # and a last tile that is the only one
        if r > 1:
            _check_group_heads(shim, r, [r // 2], offset, with_swaps, 3, 4, rng, ("one part-filled tile", r))
        TALLY["group_heads", "last_tile", r] += 1


# ---------------------------------------------------------------------------
def test_every_case_ran():
    """judges the run of the whole module: every size of every primitive and
    instance has been checked at least once (more often where families, pass
    counts or digits multiply)"""
    want = {("sizes", "host", n): 1 for n in set(SCAN_SIZES + SORT_SIZES + SORT_SIZES_LARGE + (0, SORT_SIZE_CHUNKS))}
    for op in ("sum", "max"):
        want.update({("scan", op, n): 4 * len(SCAN_FAMILIES[op]) for n in SCAN_SIZES})
        want["scan", op, 0] = 4 * len(SCAN_FAMILIES[op])
    for form in ("plain", "counted"):
        want.update({("offsets", form, c): 2 for c in OFFSET_COUNTS})
    for form in ("rows", "hist"):
        want.update({("rows", form, r): 1 for r in ROW_COUNTS})
    for inst in INSTANCES:
        want.update({("sort", inst, n): len(FAMILIES) * len(PASS_COUNTS) for n in SORT_SIZES})
        want["sort", inst, SORT_SIZE_CHUNKS] = len(FAMILIES)
        if inst in LARGE_INSTANCES:
            want.update({("sort", inst, n): 2 for n in SORT_SIZES_LARGE})
        want.update({("sort_unaligned", inst, n): 4 for n in (TILE, 8 * TILE + 1, 9 * TILE + 70)})
        want.update({("sort_last_tile", inst, r): 2 for r in LAST_TILE})
        want.update({("sort_events", inst, p): 1 for p in PASS_COUNTS})
        want["sort_refusal", inst, 1 << 32] = 1
    want.update({("partition", "u32_u32", n): len(FAMILIES) for n in SORT_SIZES})
    want.update({("partition", "u32_u32", n): 2 for n in (SORT_SIZE_CHUNKS,) + SORT_SIZES_LARGE})
    want["partition", "u32_u32", 0] = 1
    want.update({("partition_last_tile", "u32_u32", r): 2 for r in LAST_TILE})
    want.update({("group_heads", "sizes", n): 4 for n in (1, 2, 63, 64, 65, 100, 1000, TILE - 1, TILE, TILE + 1,
                                                          3 * TILE + 77, 9 * TILE + 70)})
    want["group_heads", "whole_tile", 3 * TILE + 100] = 4
    want.update({("group_heads", "last_tile", r): 4 for r in HEADS_LAST_TILE})
    assert len(want) >= 270
    assert dict(TALLY) == want, sorted(set(want.items()) ^ set(TALLY.items()))[:20]
