"""tests/seed_reference.py, the reference of tests/test_scale_gpu.py, against the
three brute forces (maxpairs_reference, qmatch_reference, spm_reference), which
know nothing of seeds: every record of seeded random cases of 200 to 800
symbols over 2, 3 and 4 letters with wildcards, separators and duplicated
reads, at several minimum lengths, one of them beyond every match; the tandem
and homopolymer subjects; the building blocks on their own.  No GPU."""
import numpy as np
import pytest

import maxpairs_reference as mp
import qmatch_reference as qr
import seed_reference as seed
import spm_reference as sr

CASES = list(range(64))
NONE = 200             # a minimum length no random case below reaches: beyond every slice and read


def _rows_sorted(rows):
    rows = np.asarray(rows).astype(np.int64)
    return rows[np.lexsort(rows.T[::-1])]


def _subject(case):
    """200 to 800 symbols over 2, 3 or 4 letters: a planted copy, wildcards, separators"""
    rng = np.random.default_rng(9000 + case)
    sigma, n = 2 + case % 3, int(rng.integers(200, 801))
    enc = rng.integers(0, sigma, n, dtype=np.uint8)
    k = int(rng.integers(10, 26))
    src, dst = rng.integers(0, n - k, 2)
    enc[dst:dst + k] = enc[src:src + k].copy()
    enc[rng.integers(0, n, case % 4)] = 254
    enc[rng.integers(0, n, case % 3)] = 255
    if case % 8 == 5:
        enc[[0, n - 1]] = [254, 255]
    if case % 16 == 7:
        at = int(rng.integers(1, n - 4))
        enc[at:at + 3] = 254
        enc[at + 3] = 255
    return enc, sigma


def _lengths(sigma):
    """short enough for hundreds of records, a middle one, one without a record"""
    return {2: (7, 12, NONE), 3: (5, 9, NONE), 4: (3, 8, NONE)}[sigma]


@pytest.mark.parametrize("case", CASES)
def test_maxpairs_against_the_brute_force(case):
    enc, sigma = _subject(case)
    counts = []
    for L in _lengths(sigma):
        want = mp.brute_force(enc, L)
        assert np.array_equal(seed.maxpairs(enc, L), want), L
        counts.append(want.shape[0])
    assert counts[0] >= 20 and counts[2] == 0


@pytest.mark.parametrize("name", ["tandem:250", "homopolymer:300", "homopolymer:1", "leftspecials", "copies:600",
                                  "small:64"])
def test_maxpairs_on_the_subjects_of_the_brute_force(name):
    enc = mp.subject(name)[0]
    for L in (1, 16, 32) if enc.size <= 300 else (8, 32):
        assert np.array_equal(seed.maxpairs(enc, L), mp.brute_force(enc, L)), L


def _query(case, enc, sigma):
    """slices of the subject with point mutations, a random stretch, specials"""
    rng = np.random.default_rng(9500 + case)
    parts = []
    for _ in range(3):
        k = int(rng.integers(20, 120))
        at = int(rng.integers(0, enc.size - k))
        piece = enc[at:at + k].copy()
        hit = int(rng.integers(0, k))
        if piece[hit] < 254:
            piece[hit] = (piece[hit] + 1) % sigma
        parts.append(piece)
    parts.insert(1, rng.integers(0, sigma, int(rng.integers(10, 200)), dtype=np.uint8))
    parts.insert(2, np.array([255] if case % 2 else [254, 254], dtype=np.uint8))
    if case % 5 == 0:
        parts.append(enc[-30:])                    # up to the subject's end
    if case % 7 == 0:
        parts.insert(0, enc[:25])                  # both from position 0
    return np.concatenate(parts).astype(np.uint8)


@pytest.mark.parametrize("case", CASES)
def test_qmatch_against_the_brute_force(case):
    enc, sigma = _subject(case)
    query = _query(case, enc, sigma)
    assert 200 <= enc.size <= 800
    counts = []
    for mode in ("fwd", "rcl") if sigma == 4 and case % 2 else ("fwd",):
        q = qr.transformed(query, mode)
        for L in _lengths(sigma):
            want = _rows_sorted(qr.brute_force(enc, q, L))
            assert np.array_equal(_rows_sorted(seed.qmatch(enc, q, L)), want), (mode, L)
            counts.append(want.shape[0])
    assert counts[0] >= 20 and counts[2] == 0


@pytest.mark.parametrize("name", ["tandem:200", "homopolymer:400"])
def test_qmatch_on_repeats_of_one_unit(name):
    enc = mp.subject(name)[0]
    query = np.concatenate([enc[:100], [255], enc[1:61], [254], enc[:17]]).astype(np.uint8)
    for L in (4, 16, 17, 61, 101):
        want = _rows_sorted(qr.brute_force(enc, query, L))
        assert np.array_equal(_rows_sorted(seed.qmatch(enc, query, L)), want), L
    assert want.shape[0] == 0


@pytest.mark.parametrize("n,m,L", [(5000, 24, 16), (300, 40, 16), (40, 300, 16), (50, 50, 1), (20, 30, 31)])
def test_the_analytic_matches_of_a_homopolymer(n, m, L):
    """A^n against A^m; 5000 / 24 / 16 is the case of tests/test_qmatch_gpu.py"""
    want = _rows_sorted(qr.brute_force(np.zeros(n, dtype=np.uint8), np.zeros(m, dtype=np.uint8), L))
    got = seed.homopolymer_qmatch(n, m, L)
    assert np.array_equal(_rows_sorted(got), want)
    assert got.shape[0] == max(0, n - L + 1 + m - L + 1 - 1)
    if (n, m, L) == (5000, 24, 16):
        assert got.shape[0] == 4985 + 8


def _reads(case):
    """a read set of 200 to 800 symbols: reads cut from one text so that they
    overlap, duplicates, a read inside another, wildcards, empty sequences"""
    rng = np.random.default_rng(9700 + case)
    sigma = 2 + case % 3
    text = rng.integers(0, sigma, 400, dtype=np.uint8)
    reads, total, target = [], 0, int(rng.integers(200, 500))
    while total < target:
        k = int(rng.integers(12, 60))
        at = int(rng.integers(0, text.size - k))
        reads.append(text[at:at + k].copy())
        total += k + 1
    for _ in range(1 + case % 3):
        reads.append(reads[int(rng.integers(0, len(reads)))].copy())             # duplicates
    long = max(range(len(reads)), key=lambda r: reads[r].size)
    reads.append(reads[long][3:-2].copy())                                        # inside another
    if case % 4 == 1:
        r = reads[int(rng.integers(0, len(reads)))]
        r[int(rng.integers(0, r.size))] = 254
    if case % 4 == 2:
        reads[0][0] = 254
        reads[1][-1] = 254
        reads.append(reads[1].copy())              # a duplicate with a wildcard: no trivial triple
    if case % 8 == 3:
        reads.insert(2, np.zeros(0, dtype=np.uint8))                              # two separators in a row
        reads.append(np.zeros(0, dtype=np.uint8))                                 # a separator at the end
    order = rng.permutation(len(reads))
    return sr.joined([reads[k] for k in order]), sigma


@pytest.mark.parametrize("case", CASES)
def test_spm_against_the_brute_force(case):
    enc, sigma = _reads(case)
    assert 200 <= enc.size <= 800
    counts = []
    for L in _lengths(sigma):
        want, terminals, starts = sr.brute_force(enc, L)
        got, got_terminals, got_starts = seed.spm(enc, L)
        assert np.array_equal(_rows_sorted(got), _rows_sorted(want)), L
        assert (got_terminals, got_starts) == (terminals, starts), L
        counts.append(want.shape[0])
    assert counts[0] >= 4 and counts[2] == 0


@pytest.mark.parametrize("name", ["tandem", "homopolymer", "copies", "alone", "nomatch", "wildcards", "long"])
def test_spm_on_repeats_and_the_read_sets_of_the_brute_force(name):
    unit = {"tandem": np.tile(np.array([0, 1, 2], dtype=np.uint8), 12), "homopolymer": np.zeros(30, dtype=np.uint8)}
    if name in unit:
        enc = sr.joined([unit[name], unit[name][:20], unit[name][1:], unit[name]])
    elif name == "copies":
        read = np.random.default_rng(3).integers(0, 4, 40, dtype=np.uint8)
        read[28:] = read[:12]
        enc = sr.copies(read, 7)
    elif name == "alone":
        enc = np.array([0, 1] * 20, dtype=np.uint8)
    elif name == "nomatch":
        enc = sr.joined([[2, 2, 0, 1, 2, 3], [3, 3, 0, 1, 2, 3, 1, 1], [1, 0, 1, 0, 2, 2, 3, 0]])
    else:
        enc = sr.wildcard_reads() if name == "wildcards" else sr.long_reads()
    for L in (1, 4, 10, 30):
        want, terminals, starts = sr.brute_force(enc, L)
        got, got_terminals, got_starts = seed.spm(enc, L)
        assert np.array_equal(_rows_sorted(got), _rows_sorted(want)), L
        assert (got_terminals, got_starts) == (terminals, starts), L


# ---- the building blocks ----

def test_keys_are_exact_or_refused():
    enc = np.array([3, 2, 1, 0, 254, 0, 1, 255, 2, 3, 3], dtype=np.uint8)
    keys, valid = seed.lmer_keys(enc, 3)
    assert valid.tolist() == [True, True, False, False, False, False, False, False, True]
    assert keys[valid].tolist() == [0b111001, 0b100100, 0b101111]
    # 32 letters of two bits fill the key; two windows that differ in their first letter alone
    rng = np.random.default_rng(1)
    a = rng.integers(0, 4, 40, dtype=np.uint8)
    b = a.copy()
    b[0] = (b[0] + 1) % 4
    ka, kb = seed.lmer_keys(a, 32)[0], seed.lmer_keys(b, 32)[0]
    assert ka[0] != kb[0] and np.array_equal(ka[1:], kb[1:])
    with pytest.raises(AssertionError, match="do not fit"):
        seed.lmer_keys(a, 33)
    with pytest.raises(AssertionError, match="more than 2 bits"):
        seed.lmer_keys(np.array([0, 4, 1], dtype=np.uint8), 2)
    assert seed.letter_bits(np.array([0, 19, 254], dtype=np.uint8)) == 5 and seed.letter_bits(a, b) == 2
    assert seed.lmer_keys(a[:5], 6)[0].size == 0
    assert seed.maxpairs(a[:5], 6).shape == (0, 3) and seed.qmatch(a, a[:5], 6).shape == (0, 3)


def test_pairs_are_all_pairs_of_equal_keys():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 2, 300, dtype=np.uint8), rng.integers(0, 2, 120, dtype=np.uint8)
    a[[50, 200]], b[60] = 254, 255
    L = 4
    seeds = seed.sorted_seeds(*seed.lmer_keys(a, L))

    def word(t, p):
        w = t[p:p + L]
        return w.tobytes() if w.size == L and (w < 254).all() else None

    p, q = seed.self_pairs(seeds)
    want = {(x, y) for x in range(a.size) for y in range(x + 1, a.size) if word(a, x) and word(a, x) == word(a, y)}
    assert len(want) == p.size > 1000 and set(zip(p.tolist(), q.tolist())) == want
    p, i = seed.cross_pairs(seeds, *seed.lmer_keys(b, L))
    want = {(x, y) for x in range(a.size) for y in range(b.size) if word(a, x) and word(a, x) == word(b, y)}
    assert len(want) == p.size > 1000 and set(zip(p.tolist(), i.tolist())) == want


def test_the_extension_stops_at_a_mismatch_a_special_and_either_end():
    a = np.array([0, 1, 2, 3, 0, 1, 254, 0, 1, 2, 3, 0, 1], dtype=np.uint8)
    b = np.array([0, 1, 2, 3, 0, 1, 2, 255, 0, 1, 2, 3], dtype=np.uint8)
    p, q = np.array([0, 7, 7, 0, 9]), np.array([0, 0, 8, 8, 2])
    assert seed.extend_right(a, p, b, q, 2).tolist() == [6, 6, 4, 4, 4]
