"""The match finders on the device past their FIRST tile -- maximal pairs
(genometools_amd/maxpairs.py), query matches (qmatch.py) and suffix-prefix
matches (spm.py) -- against tests/seed_reference.py, which sorts L-mers and
extends and is held to the brute forces by tests/test_seed_reference.py.  The
small suites (test_maxpairs_gpu.py, test_qmatch_gpu.py, test_spm_gpu.py) stop
at what a brute force can do; here every case crosses the second level of one
structure, and asserts from info() and the array sizes that it does:

  - the carry loop of the one-workgroup 64-bit scan of the tile sums
    (block_scan_excl_array_u64): more than 256 tiles, that is more than 65,536
    run suffixes, terminal suffixes or query positions -- twice that here;
  - the two-level scan_u32 over the select tiles: more than 4096 * 1024 table
    entries;
  - a second piece of the host-to-device upload: a table of more than 64 MiB;
  - the host's bisection over the offsets of maxpairs' emit, over more than
    131,072 entries;
  - a second launch of one emit call: more than 2^24 records (spm) or
    candidates (qmatch, whose chunk of 2^24 candidates also takes the two-level
    scan over its 65,536 tiles).

Every record is compared, none sampled, in the stated order; the tables come
from the engine, in this process.  Matching statistics (mstat) and the index
check have no second level of their own beyond the upload loop, which is the one
of csrc/esa_index.h for all of them: they are left out.  Record places past 2^32
are tests/test_wide_places_gpu.py; still untested: n near the single-build
limit."""
import functools

import numpy as np
import pytest

import maxpairs_reference as mp
import qmatch_reference as qr
import seed_reference as seed
import spm_reference as sr
from genometools_amd import esa, maxpairs, qmatch, spm

pytestmark = pytest.mark.gpu

TILE = 256                         # entries of one workgroup, and tile sums of one round of the 64-bit scan
ROUND = TILE * TILE                # entries behind which that scan carries
SELECT_LEVEL = 4096 * 1024         # table entries from which the scan over the select tiles has two levels
PIECE = 64 << 20                   # bytes of one piece of an upload
CHUNK = 1 << 24                    # records or candidates of one launch of an emit call
L_SEED = 14


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _engine_tables(enc):
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        return _frozen(enc, eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV))


def _device_copy(a, skew=0):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


# ---- the large random subject: maxpairs and qmatch ------------------------------

@functools.lru_cache(maxsize=None)
def large_subject():
    """2^23 + 2^18 random letters; a copy of 600 and one of 300 letters with
    flanks that differ (LCP values behind the byte 255), a wildcard run, three
    separators; shared, never written to"""
    enc = np.random.default_rng(7).integers(0, 4, (1 << 23) + (1 << 18), dtype=np.uint8)
    for src, dst, k in ((1000, 5000000, 600), (2000000, 7000000, 300)):
        enc[dst:dst + k] = enc[src:src + k]
        enc[dst - 1], enc[dst + k] = (enc[src - 1] + 1) % 4, (enc[src + k] + 1) % 4
    enc[3000000:3000020] = 254
    enc[[1234567, 4444444, 8000000]] = 255
    return _frozen(enc)[0]


@functools.lru_cache(maxsize=None)
def _large_tables():
    return _engine_tables(large_subject())


@functools.lru_cache(maxsize=None)
def large_seeds():
    """the sorted 14-mers of the large subject, for maxpairs and qmatch alike"""
    return _frozen(*seed.sorted_seeds(*seed.lmer_keys(large_subject(), L_SEED)))


def test_maxpairs_of_a_large_random_subject(gpu):
    """The 69 MB of .suf go up in two pieces through the upload of
    csrc/esa_index.h, and the counts of more than 131,072 run suffixes through
    the carry loop of offsets_u64 (csrc/esa_prims.hip): the one upload and the
    one 64-bit scan of every consumer, so this case crosses their second level
    for the checker, the matching statistics, the query matches and the
    suffix-prefix matches as well."""
    enc, suf, lcp, llv = _large_tables()
    want = seed.maxpairs(enc, L_SEED, large_seeds())
    in_order = mp.table_order(want, suf)
    assert 10 ** 5 <= want.shape[0] <= 10 ** 6 and want[:, 2].max() == 600
    assert (lcp == 255).sum() == llv.shape[0] >= (600 - 254) + (300 - 254)
    with maxpairs.MaxPairs() as f:
        f.set_index(enc, suf, lcp, llv)
        info = f.prepare(L_SEED)
        print("maxpairs: %d entries, %d bytes of .suf uploaded, %d run suffixes, %d pairs"
              % (suf.size, suf.nbytes, info["run_suffixes"], info["pairs"]))
        assert info["run_suffixes"] > 2 * ROUND and suf.size > SELECT_LEVEL
        assert suf.dtype == np.uint64 and suf.nbytes > PIECE
        assert (info["pairs"], info["max_len"]) == (want.shape[0], 600)
        assert info["runs"] <= info["segments"] <= info["run_suffixes"]
        assert info["walk_steps"] <= 2 * info["pairs"] + 2 * info["run_suffixes"]
        chunks = list(f.pairs())
        assert len(chunks) == 1 and chunks[0].dtype == np.uint64
        single = chunks[0]
        assert np.array_equal(single.astype(np.int64), in_order)
        # chunks of whole suffixes: the host's bisection over the offsets of all run suffixes
        assert info["max_pairs_of_one_suffix"] <= 50000 < info["pairs"] // 2
        pieces = list(f.pairs(50000))
        assert len(pieces) >= 3 and all(0 < c.shape[0] <= 50000 for c in pieces)
        assert np.concatenate(pieces).tobytes() == single.tobytes()
        # the same index as 4-byte entries in the caller's device memory
        keep = [_device_copy(enc), _device_copy(suf.astype(np.uint32), 8), _device_copy(lcp, 5), _device_copy(llv, 16)]
        f.set_index_device(keep[0][1], enc.size, keep[1][1], 4, keep[2][1], keep[3][1], llv.shape[0])
        narrow = f.prepare(L_SEED)
        assert all(narrow[k] == info[k] for k in info if k not in ("device_ms", "device_bytes"))
        assert f.all_pairs().tobytes() == single.tobytes()


@functools.lru_cache(maxsize=None)
def long_query():
    """150,000 positions: slices of the large subject and of its reverse
    complement with a point mutation every 40 to 200 letters, random stretches,
    two separators, a wildcard run"""
    enc = large_subject()
    rng = np.random.default_rng(11)
    parts = []
    for k in range(12):
        at = int(rng.integers(0, enc.size - 10000))
        piece = enc[at:at + 10000].copy()
        if k in (3, 8):
            piece = np.where(piece < 254, 3 - piece, piece)[::-1].astype(np.uint8)
        hits = np.cumsum(rng.integers(40, 201, 260))
        hits = hits[hits < piece.size]
        piece[hits] = np.where(piece[hits] < 254, (piece[hits] + 1) % 4, piece[hits])
        parts += [piece, rng.integers(0, 4, 2500, dtype=np.uint8)]
    parts[5] = np.concatenate([parts[5], [255]]).astype(np.uint8)
    parts[13] = np.concatenate([parts[13], [255]]).astype(np.uint8)
    query = np.concatenate(parts)[:150000].copy()
    query[70000:70012] = 254
    return _frozen(query)[0]


@pytest.mark.parametrize("mode", ["fwd", "rcl"])
def test_qmatch_of_a_long_query(gpu, mode):
    enc, suf, _, _ = _large_tables()
    query = long_query()
    assert (query == 255).sum() == 2 and (query == 254).sum() >= 12
    want = qr.in_order(seed.qmatch(enc, qr.transformed(query, mode), L_SEED, large_seeds()), suf)
    assert want.shape[0] > 1000 and want[:, 2].max() >= 150
    with qmatch.QueryMatches() as f:
        f.set_index(enc, suf)
        got = f.all_matches(query, L_SEED, mode)
        info = f.info()
        print("qmatch %s: %d positions, %d bytes of .suf uploaded, %d candidates, %d matches"
              % (mode, info["positions"], suf.nbytes, info["candidates"], info["matches"]))
        assert info["positions"] == query.size > 2 * ROUND and suf.nbytes > PIECE
        assert got.dtype == np.uint64 and got.shape == want.shape
        assert np.array_equal(got.astype(np.int64), want)
        assert info["matches"] == want.shape[0] <= info["candidates"] and info["seeds"] <= info["candidates"]


def test_qmatch_of_more_candidates_than_one_launch_takes(gpu):
    """A^70000 against A^300, L = 16: 285 seeds of 69,985 occurrences each.  One
    emit call of capacity 2^25 goes through a chunk of 2^24 candidates and a
    second one"""
    n, m, L = 70000, 300, 16
    enc, suf, _, _ = _engine_tables(np.zeros(n, dtype=np.uint8))
    query = np.zeros(m, dtype=np.uint8)
    want = qr.in_order(seed.homopolymer_qmatch(n, m, L), suf)
    assert want.shape[0] == (n - L + 1) + (m - L + 1) - 1
    least = qmatch.geometry()[1]
    with qmatch.QueryMatches() as f:
        f.set_index(enc, suf)
        info = f.prepare(query, L)
        print("qmatch: %d candidates of one emit call" % info["candidates"])
        assert info["candidates"] == (m - L + 1) * (n - L + 1) > CHUNK
        assert (info["seeds"], info["max_width"]) == (m - L + 1, n - L + 1)
        calls = list(f.emit(2 * CHUNK))
        assert len(calls) == 1 and np.array_equal(calls[0].astype(np.int64), want)
        assert f.info()["matches"] == want.shape[0]
        f.prepare(query, L)
        small = list(f.emit(least))
        assert len(small) > 100 and np.concatenate(small).tobytes() == calls[0].tobytes()


# ---- read sets: spm ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def large_read_set():
    """41,600 reads of 100 letters, 4,201,599 symbols: 41,200 cut at a stride of
    50 from a random text, 400 exact duplicates (three of them of one read),
    eight reads with a wildcard, one of them at its start; in random order"""
    rng = np.random.default_rng(13)
    cut, extra = 41200, 400
    text = rng.integers(0, 4, 50 * cut + 50, dtype=np.uint8)
    reads = np.lib.stride_tricks.sliding_window_view(text, 100)[::50][:cut]
    twice = rng.integers(0, cut, extra)
    twice[:3] = twice[0]
    reads = np.concatenate([reads, reads[twice]])
    column = rng.integers(1, 100, 8)
    column[:2] = [0, 99]
    reads[rng.choice(cut, 8, replace=False), column] = 254
    reads = reads[rng.permutation(reads.shape[0])]
    enc = np.concatenate([reads, np.full((reads.shape[0], 1), 255, dtype=np.uint8)], axis=1).reshape(-1)[:-1].copy()
    return _frozen(enc)[0]


def test_spm_of_a_large_read_set(gpu):
    L = 20
    enc, suf, lcp, llv = _engine_tables(large_read_set())
    rows, terminals, starts = seed.spm(enc, L)
    want = sr.in_order(rows, suf)
    most = int(np.unique(rows[:, 3], return_counts=True)[1].max())
    assert terminals > 41000 * 31 and starts == 41600 - 1 and want.shape[0] > 41600 and most >= 4
    with spm.SuffixPrefixMatches() as f:
        for width in (np.uint64, np.uint32):
            f.set_index(enc, suf.astype(width), lcp, llv)
            got = f.all_matches(L)
            info = f.info()
            print("spm: %d entries of %d bytes, %d terminal suffixes, %d read starts, %d matches"
                  % (suf.size, np.dtype(width).itemsize, info["terminal_suffixes"], info["read_starts"],
                     info["matches"]))
            assert info["terminal_suffixes"] > 2 * ROUND and info["table_entries"] == suf.size > SELECT_LEVEL
            assert got.dtype == np.uint64 and got.shape == want.shape
            assert np.array_equal(got.astype(np.int64), want)
            assert (info["matches"], info["terminal_suffixes"], info["read_starts"]) == (want.shape[0], terminals, starts)
            assert info["max_matches_of_one_suffix"] == most <= info["max_width"]


def test_spm_of_more_records_than_one_launch_takes(gpu):
    """2,900 copies of the 40-letter read of tests/test_spm_gpu.py that overlaps
    itself by 12: every (s, t, 40) and every (s, t, 12), 16,820,000 records, in
    one emit call"""
    copies, Z = 2900, 2 * 2900 * 2900
    read = np.random.default_rng(3).integers(0, 4, 40, dtype=np.uint8)
    read[28:] = read[:12]
    enc, suf, lcp, llv = _engine_tables(sr.copies(read, copies))
    N = suf.size
    rank = np.empty(N, dtype=np.int64)
    rank[suf.astype(np.int64)] = np.arange(N)
    least = spm.geometry()[1]
    with spm.SuffixPrefixMatches() as f:
        f.set_index(enc, suf, lcp, llv)
        info = f.prepare(10)
        assert info["matches"] == Z > CHUNK and info["max_matches_of_one_suffix"] == copies
        calls = list(f.matches(Z))
        print("spm: %d records of one emit call" % calls[0].shape[0])
        assert len(calls) == 1 and calls[0].shape == (Z, 3) and calls[0].dtype == np.uint64
        got = calls[0].view(np.int64)
        del calls
        s, t, length = got[:, 0], got[:, 1], got[:, 2]
        assert s.min() == 0 == t.min() and s.max() == copies - 1 == t.max()
        assert ((length == 40) | (length == 12)).all()
        # the set: every (s, t, len) once
        key = (s * copies + t) * 2 + (length == 40)
        key.sort()
        assert np.array_equal(key, np.arange(Z))
        # the order: table index of the matching suffix, then of the other sequence's start
        key = rank[s * 41 + 40 - length] * N + rank[t * 41]
        assert (key[1:] > key[:-1]).all()
        del key
        head = []
        for chunk in f.matches(least):
            head.append(chunk)
            if len(head) * least >= 1 << 16:
                break
        assert len(head) == (1 << 16) // least and np.concatenate(head).tobytes() == got[:1 << 16].tobytes()
