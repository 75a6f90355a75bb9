"""Brute-force restatement of include/gtamd_spm.h, independent of any table: for
every sequence and every length, the suffix of that length is looked up among
the prefixes of all sequences.  A suffix table is used for the ORDER alone
(ascending table index of the matching suffix, then of the start of the other
sequence).  Also the mirrored sequence set `gt encseq2spm` works on and the
lines it prints.  Test infrastructure only."""
import numpy as np


def mirrored(enc):
    """sequence + separator + its reverse complement (gtamd_mirror)"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    out = np.empty(2 * enc.size + 1, dtype=np.uint8)
    out[:enc.size] = enc
    out[enc.size] = 255
    for k in range(enc.size):
        c = enc[enc.size - 1 - k]
        out[enc.size + 1 + k] = 3 - c if c < 254 else c
    return out


def units(enc):
    """the sequences of a set: (start, length) between the separators"""
    enc = np.asarray(enc)
    cuts = np.flatnonzero(enc == 255)
    starts = np.concatenate([[0], cuts + 1])
    ends = np.concatenate([cuts, [enc.size]])
    return list(zip(starts.tolist(), (ends - starts).tolist()))


def _occurs_twice(text, word):
    first = text.find(word)
    return first >= 0 and text.find(word, first + 1) >= 0


def brute_force(enc, min_len):
    """(rows (s, t, len, p, q), terminal suffixes, read starts): the matches with
    the position p of the suffix of S_s and the start q of S_t, sequence by
    sequence; the number of pairs (s, len >= min_len) whose suffix is all letters
    and occurs at another place too; the sequences that start with a letter"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    text = enc.tobytes()
    seqs = units(enc)
    seeds, words, lead = {}, [], []     # the first min_len letters of a sequence -> sequences
    for t, (q, length) in enumerate(seqs):
        word = text[q:q + length]
        letters = 0
        while letters < length and word[letters] < 254:
            letters += 1
        words.append(word)
        lead.append(letters)
        if letters >= min_len:
            seeds.setdefault(word[:min_len], []).append(t)
    starts = sum(k > 0 for k in lead)
    rows, terminals = [], 0
    for s, (start, length) in enumerate(seqs):
        word = words[s]
        letters = 0
        while letters < length and word[length - 1 - letters] < 254:
            letters += 1
        for k in range(min_len, letters + 1):
            tail = word[length - k:]
            twice = _occurs_twice(text, tail)
            terminals += twice
            for t in seeds.get(tail[:min_len], ()):
                if lead[t] < k or words[t][:k] != tail:
                    continue
                # the trivial triple: only if the letters stand at another place too
                if t == s and k == length and not twice:
                    continue
                rows.append((s, t, k, start + length - k, seqs[t][0]))
    return np.array(rows, dtype=np.int64).reshape(-1, 5), terminals, starts


def in_order(rows, suf):
    """rows (s, t, len) in the library's order"""
    suf = np.asarray(suf).astype(np.int64)
    rank = np.empty(suf.size, dtype=np.int64)
    rank[suf] = np.arange(suf.size)
    return rows[np.lexsort((rank[rows[:, 4]], rank[rows[:, 3]]))][:, :3]


def sorted_lines(rows):
    """the lines `gt encseq2spm -spm show` prints for the rows, sorted as text"""
    return sorted("%d %d %d" % (s, t, k) for s, t, k in np.asarray(rows)[:, :3].tolist())


def sorted_text(rows):
    return "".join(l + "\n" for l in sorted_lines(rows)).encode()


def count_line(rows):
    return b"number of suffix-prefix matches=%d\n" % len(rows)


# ---- read sets the tests share ----

def joined(reads):
    """reads as one sequence set: a separator between two of them"""
    parts = []
    for k, r in enumerate(reads):
        if k:
            parts.append(np.array([255], dtype=np.uint8))
        parts.append(np.asarray(r, dtype=np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def wildcard_reads():
    """35 reads of 50 letters, each overlapping the next by 40, with wildcards inside
    reads and at their ends, a read of wildcards only, and a duplicate of a read
    that holds a wildcard (which is no trivial triple)"""
    text = np.random.default_rng(17).integers(0, 4, 400, dtype=np.uint8)
    reads = [text[k:k + 50].copy() for k in range(0, 350, 10)]
    reads[3][20] = 254                  # inside
    reads[5][0] = 254                   # at the start
    reads[8][49] = 254                  # at the end
    reads[11][[0, 49]] = 254
    reads[14][:] = 254                  # nothing else
    reads[17][30:33] = 254
    reads.append(reads[3].copy())
    return joined(reads)


def long_reads():
    """reads of 600 letters that overlap by 400 and by 200, reads of 300 that overlap
    by 280, duplicates of both: LCP values beyond a byte"""
    text = np.random.default_rng(23).integers(0, 4, 3000, dtype=np.uint8)
    return joined([text[0:600], text[200:800], text[400:1000], text[1500:1800], text[1520:1820], text[1500:1800],
                   text[2000:2600], text[2000:2600]])


def copies(read, count):
    return joined([read] * count)


def counted_terminals(count, length=30):
    """reads of `length` letters with exactly `count` terminal suffixes at minimum
    length `length`: pairs of duplicates (two each) and, for an odd count, one
    read that also lies inside a longer one"""
    rng = np.random.default_rng(1000 + count)
    reads = []
    for _ in range(count // 2):
        r = rng.integers(0, 4, length, dtype=np.uint8)
        reads += [r, r]
    if count % 2:
        r = rng.integers(0, 4, length, dtype=np.uint8)
        reads += [r, np.concatenate([rng.integers(0, 4, 5, dtype=np.uint8), r, rng.integers(0, 4, 5, dtype=np.uint8)])]
    order = rng.permutation(len(reads))
    return joined([reads[k] for k in order])
