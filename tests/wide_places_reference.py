"""A WINDOWED reference for the four consumers that enumerate by 64-bit places
-- query matches, suffix-prefix matches, tag matches without differences and
maximal pairs -- for enumerations far too large to expand (4 * 10^9 records
and more): the exact count of every item in the enumeration's order, and the
records of any window of places, made by expanding only the items the window
touches.  tests/test_wide_places_reference.py holds it to the references that
expand everything (seed_reference, qmatch_reference, spm_reference,
maxpairs_reference, tagmatch_reference) on small inputs.

Built from seed_reference.lmer_keys and stable sorts of the keys, which give
the sizes of the groups of equal L-mers without expanding them; a suffix table
is used for the ORDER alone (its inverse, the rank of a position), as in those
modules, so this is neither the device's binary search in .suf nor its walk over
.lcp.  Counts are int64 numpy arrays, offsets their int64 running sums (asserted
to stay far below 2^63), totals Python ints.  Test infrastructure only.

An ITEM is what the device counts for: a query position (qmatch), a terminal
suffix (spm), a job (tagmatch), a suffix in a run (maxpairs)."""
import numpy as np

import seed_reference as seed

SPECIAL = seed.SPECIAL


def rank_of(suf):
    """table index of every position"""
    suf = np.asarray(suf).astype(np.int64)
    rank = np.empty(suf.size, dtype=np.int64)
    rank[suf] = np.arange(suf.size)
    return rank


def offsets_of(counts):
    """off[i] = the counts in front of item i, off[items] = the total; int64"""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.size == 0 or (counts.min() >= 0 and int(counts.max()) * counts.size < 1 << 62)
    return np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)


def places(off, a, b):
    """(item, k) of every place of [a, b), ascending: the item it belongs to and
    its number inside that item.  Only the touched items are looked at, and of
    the first and the last only the part inside the window"""
    total = int(off[-1])
    a, b = max(0, min(int(a), total)), max(0, min(int(b), total))
    if a >= b:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    i0 = int(np.searchsorted(off, a, side="right")) - 1          # the last item that starts at or before a
    i1 = int(np.searchsorted(off, b, side="left"))               # the first that starts at or behind b
    item = np.arange(i0, i1, dtype=np.int64)
    first = np.maximum(a - off[i0:i1], 0)
    stop = np.minimum(b, off[i0 + 1:i1 + 1]) - off[i0:i1]
    many = np.maximum(stop - first, 0)
    owner = np.repeat(np.arange(item.size), many)
    begin = np.cumsum(many) - many
    k = first[owner] + (np.arange(owner.size) - begin[owner])
    return item[owner], k


class Enumeration:
    """what the four have in common: counts per item, off, total"""

    def _set_counts(self, counts):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.counts.setflags(write=False)
        self.off = offsets_of(self.counts)
        self.off.setflags(write=False)
        self.total = int(self.off[-1])                           # a Python int
        self.most = int(self.counts.max()) if self.counts.size else 0


# ---- query matches: include/gtamd_qmatch.h ----------------------------------------

class QueryMatches(Enumeration):
    """items: the m query positions; the places are CANDIDATE numbers: the k-th
    candidate of position i is the k-th suffix, in table order, that starts with
    the L letters q[i..i+L).  A candidate is a record if it is left-maximal"""

    def __init__(self, enc, suf, query, L):
        self.enc, self.query, self.L = seed._u8(enc), seed._u8(query), L
        bits = seed.letter_bits(self.enc, self.query)
        rank = rank_of(suf)
        keys, valid = seed.lmer_keys(self.enc, L, bits)
        pos = np.flatnonzero(valid)
        order = np.lexsort((rank[pos], keys[pos]))               # by key, equal keys in table order
        self.seed_keys, self.seed_pos = keys[pos][order], pos[order]
        qkeys, qvalid = seed.lmer_keys(self.query, L, bits)
        lo = np.zeros(self.query.size, dtype=np.int64)
        counts = np.zeros(self.query.size, dtype=np.int64)
        at = np.flatnonzero(qvalid)
        lo[at] = np.searchsorted(self.seed_keys, qkeys[at], side="left")
        counts[at] = np.searchsorted(self.seed_keys, qkeys[at], side="right") - lo[at]
        self.lo = lo
        self._set_counts(counts)
        self.seeds = int((counts > 0).sum())

    def candidates(self, a, b):
        """(kept, records) of the candidates [a, b): which are records, and those,
        int64 rows (dbpos, qpos, len) in order"""
        i, k = places(self.off, a, b)
        p = self.seed_pos[self.lo[i] + k]
        lp, li = seed._before(self.enc, p), seed._before(self.query, i)
        kept = (i == 0) | (p == 0) | (lp >= SPECIAL) | (lp != li)
        p, i = p[kept], i[kept]
        length = seed.extend_right(self.enc, p, self.query, i, self.L)
        return kept, np.stack([p, i, length], axis=1).astype(np.int64).reshape(-1, 3)

    def emit_call(self, cursor, capacity, least, largest=1 << 24):
        """(records, cursor afterwards) of one gtamd_qmatch_emit: chunks of at most
        capacity - (records so far) candidates, until that room falls below `least`
        (gtamd_qmatch_geometry) or no candidate is left; largest: of one chunk"""
        assert capacity >= least
        out, written = [], 0
        while cursor < self.total and capacity - written >= least:
            chunk = min(capacity - written, self.total - cursor, largest)
            _, rec = self.candidates(cursor, cursor + chunk)
            out.append(rec)
            written += rec.shape[0]
            cursor += chunk
        return (np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)), cursor


# ---- suffix-prefix matches: include/gtamd_spm.h -----------------------------------

class SuffixPrefixMatches(Enumeration):
    """items: the terminal suffixes in table order -- a position p from which h >=
    L letters run to the end of p's sequence, and whose h letters stand at another
    place too; the records of one: the sequences that start with those h letters,
    in table order of their starts.  The places are record numbers"""

    def __init__(self, enc, suf, L):
        enc = self.enc = seed._u8(enc)
        n = enc.size
        self.rank = rank_of(suf)
        self.bits = seed.letter_bits(enc)
        self.seq_starts = np.concatenate([[0], np.flatnonzero(enc == 255) + 1]).astype(np.int64)
        inside = self.seq_starts[self.seq_starts < n]
        self.read_starts = inside[enc[inside] < SPECIAL]          # sequences that start with a letter
        # letters[p]: the letters from p to the next special; reach[p]: that, if a separator or the end follows
        nxt = np.full(n + 1, n, dtype=np.int64)
        special = np.flatnonzero(enc >= SPECIAL)
        nxt[special] = special
        nxt = np.minimum.accumulate(nxt[::-1])[::-1]
        self.letters = nxt - np.arange(n + 1)
        reach = np.where(np.concatenate([enc, [255]])[nxt] == 255, self.letters, -1)[:n]
        cand = np.flatnonzero(reach >= L)
        assert cand.size == 0 or int(reach[cand].max()) * self.bits <= 64, "a suffix too long for one key"
        occurs = np.zeros(cand.size, dtype=np.int64)
        counts = np.zeros(cand.size, dtype=np.int64)
        for h in np.unique(reach[cand]).tolist():
            keys, valid = seed.lmer_keys(enc, h, self.bits)
            everywhere = np.sort(keys[valid])
            mine = np.flatnonzero(reach[cand] == h)
            key = keys[cand[mine]]
            occurs[mine] = np.searchsorted(everywhere, key, side="right") - np.searchsorted(everywhere, key, side="left")
            heads = np.sort(keys[self._heads(h)])
            counts[mine] = np.searchsorted(heads, key, side="right") - np.searchsorted(heads, key, side="left")
        terminal = occurs >= 2
        p, counts, occurs = cand[terminal], counts[terminal], occurs[terminal]
        order = np.argsort(self.rank[p], kind="stable")
        self.p, self.h = p[order], reach[p[order]]
        self.max_width = int(occurs.max()) if occurs.size else 0
        self._set_counts(counts[order])

    def _heads(self, h):
        """the read starts with at least h letters"""
        return self.read_starts[self.letters[self.read_starts] >= h]

    def _keys_at(self, pos, h):
        key = np.zeros(pos.size, dtype=np.uint64)
        for j in range(h):
            key = (key << np.uint64(self.bits)) | self.enc[pos + j].astype(np.uint64)
        return key

    def records(self, a, b):
        """the records [a, b): int64 rows (suffix_seq, prefix_seq, len) in order"""
        item, k = places(self.off, a, b)
        q = np.zeros(item.size, dtype=np.int64)
        for h in np.unique(self.h[item]).tolist():
            mine = np.flatnonzero(self.h[item] == h)
            heads = self._heads(h)
            hk = self._keys_at(heads, h)
            order = np.lexsort((self.rank[heads], hk))            # by key, equal keys in table order
            heads, hk = heads[order], hk[order]
            lo = np.searchsorted(hk, self._keys_at(self.p[item[mine]], h), side="left")
            q[mine] = heads[lo + k[mine]]
        s = np.searchsorted(self.seq_starts, self.p[item], side="right") - 1
        t = np.searchsorted(self.seq_starts, q, side="right") - 1
        return np.stack([s, t, self.h[item]], axis=1).astype(np.int64).reshape(-1, 3)


# ---- tag matches without differences: include/gtamd_tagmatch.h --------------------

class ExactTagMatches(Enumeration):
    """items: the tags, read forward only (one job a tag), K = 0: the records of
    one are the positions where its letters stand, in table order, with len = its
    length and dist = 0.  The places are record numbers"""

    def __init__(self, enc, suf, tags):
        enc = seed._u8(enc)
        rank = rank_of(suf)
        bits = seed.letter_bits(enc, *tags)
        self.tags = [seed._u8(t) for t in tags]
        self.length = np.array([t.size for t in self.tags], dtype=np.int64)
        self.lo = np.zeros(len(tags), dtype=np.int64)
        self.sorted_pos = {}
        counts = np.zeros(len(tags), dtype=np.int64)
        for m in np.unique(self.length).tolist():
            keys, valid = seed.lmer_keys(enc, m, bits)
            pos = np.flatnonzero(valid)
            order = np.lexsort((rank[pos], keys[pos]))
            skeys, self.sorted_pos[m] = keys[pos][order], pos[order]
            mine = np.flatnonzero(self.length == m)
            letters = np.stack([self.tags[t] for t in mine.tolist()]).astype(np.uint64)
            assert int(letters.max()) < 1 << bits                 # (a tag holds letters only)
            tkeys = np.zeros(mine.size, dtype=np.uint64)
            for j in range(m):                                    # the key of lmer_keys, a tag a row
                tkeys = (tkeys << np.uint64(bits)) | letters[:, j]
            self.lo[mine] = np.searchsorted(skeys, tkeys, side="left")
            counts[mine] = np.searchsorted(skeys, tkeys, side="right") - self.lo[mine]
        self._set_counts(counts)

    def records(self, a, b):
        """the records [a, b): uint64 rows (tag, dbstart, lendist) in order"""
        item, k = places(self.off, a, b)
        p = np.zeros(item.size, dtype=np.int64)
        for m in np.unique(self.length[item]).tolist():
            mine = np.flatnonzero(self.length[item] == m)
            p[mine] = self.sorted_pos[m][self.lo[item[mine]] + k[mine]]
        return np.stack([2 * item, p, self.length[item]], axis=1).astype(np.uint64).reshape(-1, 3)


# ---- maximal pairs: include/gtamd_maxpairs.h ----------------------------------------

UNIQUE = 255


class MaximalPairs(Enumeration):
    """items: the suffixes in runs, in table order -- a run is a group of two or
    more suffixes that start with the same L letters; the records of one: the
    suffixes behind it in its run whose left class differs (unique differs from
    everything).  The device's cursor counts ITEMS, not records: `emit_call`"""

    def __init__(self, enc, suf, L):
        enc = self.enc = seed._u8(enc)
        self.L = L
        rank = rank_of(suf)
        bits = seed.letter_bits(enc)
        keys, valid = seed.lmer_keys(enc, L, bits)
        pos = np.flatnonzero(valid)
        order = np.lexsort((rank[pos], keys[pos]))
        keys, pos = keys[pos][order], pos[order]
        new = np.concatenate([[True], keys[1:] != keys[:-1]]) if keys.size else np.zeros(0, dtype=bool)
        group = np.cumsum(new) - 1
        size = np.bincount(group) if keys.size else np.zeros(0, dtype=np.int64)
        inrun = size[group] >= 2 if keys.size else np.zeros(0, dtype=bool)
        pos, new = pos[inrun], new[inrun]
        # (a key order that groups equal keys and, inside a group, the table order:
        # the runs themselves follow each other in table order)
        order = np.argsort(rank[pos], kind="stable")
        pos, new = pos[order], new[order]
        M = pos.size
        self.pos = pos
        first = np.flatnonzero(new)                                # of every run
        run = np.cumsum(new) - 1
        self.run_end = np.concatenate([first[1:], [M]])[run] if M else np.zeros(0, dtype=np.int64)
        left = seed._before(enc, pos)
        self.cls = np.where(left >= SPECIAL, UNIQUE, left).astype(np.int64)
        behind = self.run_end - np.arange(M) - 1                   # suffixes behind it in its run
        same = np.zeros(M, dtype=np.int64)
        for c in np.unique(self.cls[self.cls != UNIQUE]).tolist():
            is_c = (self.cls == c).astype(np.int64)
            upto = np.concatenate([[0], np.cumsum(is_c)])          # of class c in front of entry k
            mine = np.flatnonzero(is_c)
            same[mine] = upto[self.run_end[mine]] - upto[mine + 1]
        self.runs = int(first.size)
        starts = new | (self.cls == UNIQUE)
        if M > 1:
            starts[1:] |= self.cls[1:] != self.cls[:-1]
        self.segments = int(starts.sum())
        self._set_counts(behind - same)

    def records(self, k0, k1):
        """the records of the items [k0, k1): int64 rows (pos1, pos2, len) in order"""
        i = np.arange(k0, k1, dtype=np.int64)
        i = i[self.counts[i] > 0]                                  # (a run of one class is not gone through)
        j, owner = seed._expand(i + 1, self.run_end[i] - i - 1)
        i = i[owner]
        keep = (self.cls[i] != self.cls[j]) | (self.cls[i] == UNIQUE)
        p, q = self.pos[i[keep]], self.pos[j[keep]]
        length = seed.extend_right(self.enc, p, self.enc, q, self.L)
        return np.stack([np.minimum(p, q), np.maximum(p, q), length], axis=1).astype(np.int64).reshape(-1, 3)

    def emit_call(self, k0, capacity):
        """(records, cursor afterwards) of one gtamd_maxpairs_emit: whole items from
        k0 on, as many as fit `capacity` records; the cursor ends at the number of
        items when no record is left"""
        assert capacity >= self.most
        if self.off[k0] == self.total:
            return np.zeros((0, 3), dtype=np.int64), self.counts.size
        k1 = int(np.searchsorted(self.off, self.off[k0] + capacity, side="right")) - 1
        return self.records(k0, k1), k1
