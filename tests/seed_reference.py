"""A reference for the three match finders that scales to millions of symbols:
sort the L-mers, pair up equal ones, extend.  Plain numpy, independent of any
suffix or LCP table, and neither the device's route (binary search in .suf, walk
over .lcp) nor that of the diagonal brute forces of maxpairs_reference,
qmatch_reference and spm_reference, which tests/test_seed_reference.py holds it
to.  A suffix table is used for the ORDER of the records alone, by the helpers
of those modules.  Test infrastructure only.

Three building blocks:

  lmer_keys      the L letters of every window packed into an exact integer key;
                 a window that holds a special (a symbol >= 254) has none
  self_pairs,    every pair of positions with equal keys, within one text or
  cross_pairs    between two, from a stable sort and the expansion of the groups
  extend_right   letter by letter, only the pairs that still match stay active;
                 it stops at a mismatch, a special or the end of either text

and on top of them `maxpairs`, `qmatch` and `spm`, each a restatement of its
header.  A minimum length beyond what one key holds (32 letters of DNA) is
seeded with the letters that fit and the extensions are filtered for it."""
import numpy as np

SPECIAL = 254          # symbols from here on are specials: 254 wildcard, 255 separator


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def letter_bits(*texts):
    """bits that hold every letter of the texts, 2 at least (four letters)"""
    most = 3
    for t in texts:
        letters = _u8(t)
        letters = letters[letters < SPECIAL]
        if letters.size:
            most = max(most, int(letters.max()))
    return most.bit_length()


def lmer_keys(enc, L, bits=2):
    """(keys, valid) of the n - L + 1 windows of L symbols: uint64 keys that are
    exact (bits * L <= 64 and every letter below 2^bits are asserted, nothing is
    hashed); valid: the window holds letters only"""
    enc = _u8(enc)
    assert L >= 1 and bits * L <= 64, "L = %d symbols of %d bits do not fit a 64-bit key" % (L, bits)
    special = enc >= SPECIAL
    assert special.all() or int(enc[~special].max()) < (1 << bits), "a letter needs more than %d bits" % bits
    w = enc.size - L + 1
    if w <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    upto = np.concatenate([[0], np.cumsum(special)])
    valid = upto[L:] == upto[:w]
    sym = np.where(special, 0, enc).astype(np.uint64)
    keys = np.zeros(w, dtype=np.uint64)
    for j in range(L):
        keys = (keys << np.uint64(bits)) | sym[j:j + w]
    return keys, valid


def seed_length(L, bits=2):
    """the letters of a seed for minimum length L: L, or what fits a key if that is
    less; the extensions of such seeds are then filtered for L letters"""
    return min(L, 64 // bits)


def sorted_seeds(keys, valid):
    """(keys, positions) of the valid windows, sorted by key, equal keys by position"""
    pos = np.flatnonzero(valid)
    kv = keys[pos]
    order = np.argsort(kv, kind="stable")
    return kv[order], pos[order]


def _expand(first, count):
    """first[k], first[k] + 1, .. first[k] + count[k] - 1 for every k, and the k of each"""
    owner = np.repeat(np.arange(count.size), count)
    begin = np.cumsum(count) - count
    return first[owner] + (np.arange(owner.size) - begin[owner]), owner


def self_pairs(seeds):
    """(p, q), p < q: every pair of positions of one text with equal keys"""
    kv, pos = seeds
    m = kv.size
    if m == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    new = np.concatenate([[True], kv[1:] != kv[:-1]])
    start = np.flatnonzero(new)
    end = np.concatenate([start[1:], [m]])[np.cumsum(new) - 1]      # of the group of every entry
    here = np.arange(m)
    partner, owner = _expand(here + 1, end - here - 1)              # the entries behind it in its group
    return pos[owner], pos[partner]


def cross_pairs(seeds, keys, valid):
    """(p, i): every position p of the sorted text and i of the other with equal keys"""
    kv, pos = seeds
    at = np.flatnonzero(valid)
    lo = np.searchsorted(kv, keys[at], side="left")
    hi = np.searchsorted(kv, keys[at], side="right")
    k, owner = _expand(lo, hi - lo)
    return pos[k], at[owner]


def extend_right(a, p, b, q, L):
    """the letters a from p on shares with b from q on, of which L are known"""
    a, b = _u8(a), _u8(b)
    pa, pb = np.concatenate([a, [255]]).astype(np.uint8), np.concatenate([b, [255]]).astype(np.uint8)
    length = np.full(p.size, L, dtype=np.int64)
    act = np.arange(p.size)
    x, y = p + L, q + L                      # (of the active pairs; a window lies inside its text)
    while act.size:
        s, t = pa[x], pb[y]
        go = (s == t) & (s < SPECIAL)
        act, x, y = act[go], x[go] + 1, y[go] + 1
        length[act] += 1
    return length


def _before(text, p):
    """the symbol in front of p, 255 in front of position 0"""
    return np.where(p > 0, text[np.maximum(p, 1) - 1], 255)


def maxpairs(enc, L, seeds=None):
    """include/gtamd_maxpairs.h, "A MAXIMAL PAIR of minimum length L" (lines
    20-29): the self pairs p < q that are left-maximal -- p = 0, or the symbols
    in front differ, or one of them is a special -- extended to the right, which
    makes them right-maximal.  int64 rows (p, q, len), sorted like
    maxpairs_reference.sort_records; seeds: sorted_seeds of the keys of
    seed_length(L, letter_bits(enc)) letters, if the caller has them already"""
    enc = _u8(enc)
    bits = letter_bits(enc)
    K = seed_length(L, bits)
    if seeds is None:
        seeds = sorted_seeds(*lmer_keys(enc, K, bits))
    p, q = self_pairs(seeds)
    lp, lq = _before(enc, p), _before(enc, q)
    keep = (lp != lq) | (lp >= SPECIAL) | (lq >= SPECIAL)
    p, q = p[keep], q[keep]
    rec = np.stack([p, q, extend_right(enc, p, enc, q, K)], axis=1).astype(np.int64).reshape(-1, 3)
    rec = rec[rec[:, 2] >= L]
    return rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]


def qmatch(enc, query, L, seeds=None):
    """include/gtamd_qmatch.h, "A MATCH of minimum length L" (lines 24-35): the
    seed pairs of subject position p and query position i that are left-maximal
    -- i = 0, or p = 0, or enc[p-1] is a special, or enc[p-1] != q[i-1] --
    extended to the right.  int64 rows (dbpos, qpos, len) in no stated order;
    seeds: sorted_seeds of the subject's keys at letter_bits(enc, query), if the
    caller has them already (of seed_length(L, bits) letters)"""
    enc, query = _u8(enc), _u8(query)
    bits = letter_bits(enc, query)
    K = seed_length(L, bits)
    if seeds is None:
        seeds = sorted_seeds(*lmer_keys(enc, K, bits))
    p, i = cross_pairs(seeds, *lmer_keys(query, K, bits))
    lp, li = _before(enc, p), _before(query, i)
    keep = (i == 0) | (p == 0) | (lp >= SPECIAL) | (lp != li)
    p, i = p[keep], i[keep]
    rec = np.stack([p, i, extend_right(enc, p, query, i, K)], axis=1).astype(np.int64).reshape(-1, 3)
    return rec[rec[:, 2] >= L]


def spm(enc, L):
    """include/gtamd_spm.h, "A MATCH of minimum length L" (lines 23-34): a seed
    pair (p, q) with q the start of a sequence is a match if and only if its
    extension reaches the end of p's sequence; it stays inside q's, since it
    stops at a special.  The trivial triple (s, s, |S_s|) has no seed pair of
    two positions: it is kept when the whole of S_s is found at another place by
    the same seeds.  Returns what spm_reference.brute_force returns: int64 rows
    (s, t, len, p, q) in no stated order, the terminal suffixes -- the pairs
    (s, len >= L) whose suffix is all letters and stands at another place too --
    and the read starts, the sequences that start with a letter"""
    enc = _u8(enc)
    n = enc.size
    starts = np.concatenate([[0], np.flatnonzero(enc == 255) + 1]).astype(np.int64)
    is_start = np.zeros(n + 1, dtype=bool)
    is_start[starts] = True
    read_starts = int((enc[starts[starts < n]] < SPECIAL).sum())
    # reach[p]: the letters from p to the end of its sequence, -1 if a wildcard comes first
    nxt = np.full(n + 1, n, dtype=np.int64)
    special = np.flatnonzero(enc >= SPECIAL)
    nxt[special] = special
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]             # the next special at or behind p
    ends_sequence = np.concatenate([enc, [255]])[nxt] == 255
    reach = np.where(ends_sequence, nxt - np.arange(n + 1), -1)

    bits = letter_bits(enc)
    K = seed_length(L, bits)
    a, b = self_pairs(sorted_seeds(*lmer_keys(enc, K, bits)))
    length = extend_right(enc, a, enc, b, K)
    # either side of a pair whose extension reaches the end of its sequence, L letters at least
    suffix = np.concatenate([a, b])
    other = np.concatenate([b, a])
    length = np.concatenate([length, length])
    to_end = (length == reach[suffix]) & (length >= L)
    suffix, other = suffix[to_end], other[to_end]
    terminal = np.unique(suffix)
    match = is_start[other]
    p, q = suffix[match], other[match]
    whole = terminal[is_start[terminal]]                     # sequences that stand elsewhere too
    p, q = np.concatenate([p, whole]), np.concatenate([q, whole])
    s = np.searchsorted(starts, p, side="right") - 1
    t = np.searchsorted(starts, q, side="right") - 1
    rows = np.stack([s, t, reach[p], p, q], axis=1).astype(np.int64).reshape(-1, 5)
    return rows, int(terminal.size), read_starts


def homopolymer_qmatch(n, m, L):
    """qmatch of A^n against the query A^m, analytically: one maximal run on
    every diagonal p - i, from where the diagonal enters the rectangle to where
    it leaves it; int64 rows (dbpos, qpos, len) of the runs of at least L letters"""
    d = np.arange(-(m - 1), n, dtype=np.int64)
    p0, i0 = np.maximum(d, 0), np.maximum(-d, 0)
    length = np.minimum(n, m + d) - p0
    keep = length >= L
    return np.stack([p0[keep], i0[keep], length[keep]], axis=1)
