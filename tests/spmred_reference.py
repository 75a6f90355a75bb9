"""Brute-force restatement of include/gtamd_spmred.h, independent of any table:
over the suffix-prefix matches of tests/spm_reference.py, a match (r, w, l) is
transitive when some match (t, w, l') with l' > l has a left part -- S_t without
its last l' symbols -- that ends the left part of r, compared as byte strings
of letters (a special equals nothing).
Also the mirror filter, the records, the three closing figures and the lines
`gt readjoiner overlap` prints, the bin32 list it writes, and read sets the
tests share.  A suffix table is used for the ORDER alone.  Test infrastructure
only."""
import struct

import numpy as np

import spm_reference as sr

PREFIX_DIRECT, SUFFIX_DIRECT = 1, 2
BIN32 = 2                       # GT_SPMLIST_BIN32, the header byte of the list


def transitive(enc, rows):
    """for every row (s, t, len, p, q) of spm_reference.brute_force: is it transitive?"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    text = enc.tobytes()
    words = [text[a:a + k] for a, k in sr.units(enc)]
    into = {}                                   # w -> [(l', t)]
    for s, t, k, _, _ in rows.tolist():
        into.setdefault(t, []).append((k, s))
    out = np.zeros(rows.shape[0], dtype=bool)
    for at, (r, w, l, _, _) in enumerate(rows.tolist()):
        left_r = words[r][:len(words[r]) - l]
        for lp, t in into[w]:
            left_t = words[t][:len(words[t]) - lp]
            # (a special equals nothing, itself included: a left part with one ends no other)
            if lp > l and (not left_t or max(left_t) < 254) and left_r.endswith(left_t):
                out[at] = True
                break
    return out


def read_of(s, K):
    """(read number, direct) of sequence s of the mirrored set of K / 2 reads"""
    return (s, True) if s < K // 2 else (K - 1 - s, False)


def mirror_kept(sn, sd, pn, pd):
    """of the two mirror images of an overlap, the one `gt readjoiner overlap` gives"""
    return (sd and pd) or (sn == pn and not (not sd and not pd)) or (sd and not pd and pn > sn) or \
        (not sd and pd and pn < sn)


def brute_force(enc, min_len, elimtrans=True, mirrored=True, rows=None, trans=None):
    """(kept rows (suffix_read, prefix_read, len, flags, p, q), figures): the
    records of include/gtamd_spmred.h with the two positions that order them, and
    matches, transitive_same_read, transitive_other, contained_sequences.  rows,
    trans: spm_reference.brute_force(enc, min_len)[0] and transitive(enc, rows)
    where the caller has them"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    rows = sr.brute_force(enc, min_len)[0] if rows is None else rows
    units = sr.units(enc) if enc.size else []
    K = len(units)
    assert not mirrored or K % 2 == 0
    if not elimtrans:
        trans = np.zeros(rows.shape[0], dtype=bool)
    elif trans is None:
        trans = transitive(enc, rows)
    kept, same, other = [], 0, 0
    for (s, t, k, p, q), tr in zip(rows.tolist(), trans.tolist()):
        (sn, sd), (pn, pd) = (read_of(s, K), read_of(t, K)) if mirrored else ((s, True), (t, True))
        if tr:
            same += sn == pn
            other += sn != pn
        elif not mirrored or mirror_kept(sn, sd, pn, pd):
            kept.append((sn, pn, k, (SUFFIX_DIRECT if sd else 0) | (PREFIX_DIRECT if pd else 0), p, q))
    # a sequence of min_len letters or more, all letters, that stands at another place too
    text = enc.tobytes()
    contained = 0
    for a, k in units:
        word = text[a:a + k]
        if k >= min_len and k > 0 and max(word) < 254:
            first = text.find(word)
            contained += text.find(word, first + 1) >= 0
    figures = dict(matches=rows.shape[0], transitive_same_read=same, transitive_other=other,
                   contained_sequences=contained, kept=len(kept))
    return np.array(kept, dtype=np.int64).reshape(-1, 6), figures


def in_order(kept, suf):
    """kept rows as records (suffix_read, prefix_read, len, flags) in the library's order"""
    suf = np.asarray(suf).astype(np.int64)
    rank = np.empty(suf.size, dtype=np.int64)
    rank[suf] = np.arange(suf.size)
    return kept[np.lexsort((rank[kept[:, 5]], rank[kept[:, 4]]))][:, :4]


def lines(records):
    """the lines `gt readjoiner overlap -showspm` prints for the records, in their order"""
    return ["%d %s %d %s %d" % (sn, "+" if f & SUFFIX_DIRECT else "-", pn, "+" if f & PREFIX_DIRECT else "-", k)
            for sn, pn, k, f in np.asarray(records)[:, :4].tolist()]


def sorted_text(records):
    return "".join(l + "\n" for l in sorted(lines(records))).encode()


def closing_lines(figures, reads, elimtrans=True):
    """the `#` lines behind the matches"""
    kept = figures["kept"]
    per_read = "%.2f" % (np.float32(kept) / np.float32(reads))
    if not elimtrans:
        return ["# number of suffix-prefix matches = %d" % kept, "# average SPM/read = %s" % per_read]
    return ["# number of irreducible suffix-prefix matches = %d" % kept,
            "# average irreducible SPM/read = %s" % per_read,
            "# number of transitive suffix-prefix matches = %d"
            % (figures["transitive_same_read"] + (figures["transitive_other"] >> 1))]


def opening_lines(reads):
    return ["# gt readjoiner overlap (version 1.2)", "# number of reads in filtered readset = %d" % reads]


def bin32(records):
    """Readjoiner's binary list of the records (src/match/rdj-spmlist.c): a format
    byte, then three uint32 a record, the third len << 2 | suffix_direct << 1 |
    prefix_direct"""
    out = [struct.pack("<B", BIN32)]
    for sn, pn, k, f in np.asarray(records)[:, :4].tolist():
        out.append(struct.pack("<III", sn, pn, k << 2 | f))
    return b"".join(out)


def parse_bin32(raw):
    """the records of a bin32 list as a sorted list of (suffix_read, prefix_read, len, flags)"""
    assert raw[0] == BIN32 and (len(raw) - 1) % 12 == 0
    words = np.frombuffer(raw[1:], dtype="<u4").reshape(-1, 3)
    return sorted((int(a), int(b), int(c) >> 2, int(c) & 3) for a, b, c in words)


# ---- read sets the tests share ----

def revcomp(r):
    r = np.asarray(r, dtype=np.uint8)[::-1]
    return np.where(r < 254, 3 - r, r).astype(np.uint8)


def containment_free(reads):
    """the reads without those that stand whole inside another one or its reverse
    complement, or equal their own reverse complement; of duplicates the first stays"""
    keep = []
    texts = [np.asarray(r, dtype=np.uint8).tobytes() for r in reads]
    backs = [revcomp(r).tobytes() for r in reads]
    for a, (t, b) in enumerate(zip(texts, backs)):
        if t == b:
            continue
        inside = False
        for c, (u, v) in enumerate(zip(texts, backs)):
            if c == a:
                continue
            if (t in u or t in v) and (len(u) > len(t) or c < a):
                inside = True
                break
        if not inside:
            keep.append(reads[a])
    return keep


def tiled_reads(seed, text_len, length, step, flip=0.4, repeat=0):
    """reads cut every `step` letters (a seeded jitter of one) from a random text
    with a planted repeat of `repeat` letters and its reverse complement; `flip`
    of them reverse-complemented; containment-free on both strands.  length: a
    number or (least, most)"""
    rng = np.random.default_rng(seed)
    text = rng.integers(0, 4, text_len, dtype=np.uint8)
    if repeat:
        a, b, c = text_len // 5, text_len // 2, 4 * text_len // 5
        text[b:b + repeat] = text[a:a + repeat]
        text[c:c + repeat] = revcomp(text[a:a + repeat])
    reads, at = [], 0
    while True:
        k = length if isinstance(length, int) else int(rng.integers(length[0], length[1] + 1))
        if at + k > text_len:
            break
        r = text[at:at + k].copy()
        reads.append(revcomp(r) if rng.random() < flip else r)
        at += step + int(rng.integers(0, 2))
    order = rng.permutation(len(reads))
    return containment_free([reads[k] for k in order])


def fan_reads(count, marked, seed=71):
    """(reads, rows (s, t, len, p, q), transitive) worked out, not searched for:
    `count` reads A_i = U_i C and `count` reads B_j = C V_j of 40 letters that
    share the 20 letters C, every A_i with every B_j by 20, count * count matches
    of one interval; and `marked` reads T_k = the last 10 of U_k, C, the first 10
    of V_k, which make (A_k, B_k, 20) transitive and add (A_k, T_k, 30) and (T_k,
    B_k, 30).  Minimum length 20.  tests/test_spmred_core.py holds the worked-out
    rows against the brute force at a small count"""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 4, 20, dtype=np.uint8)
    U = rng.integers(0, 4, (count, 20), dtype=np.uint8)
    V = rng.integers(0, 4, (count, 20), dtype=np.uint8)
    reads = [np.concatenate([U[i], C]) for i in range(count)] + [np.concatenate([C, V[j]]) for j in range(count)] + \
        [np.concatenate([U[k][10:], C, V[k][:10]]) for k in range(marked)]
    at = 41 * np.arange(len(reads), dtype=np.int64)
    i, j = np.divmod(np.arange(count * count, dtype=np.int64), count)
    k = np.arange(marked, dtype=np.int64)
    rows = np.concatenate([
        np.stack([i, count + j, np.full(i.size, 20), at[i] + 20, at[count + j]], axis=1),
        np.stack([k, 2 * count + k, np.full(marked, 30), at[k] + 10, at[2 * count + k]], axis=1),
        np.stack([2 * count + k, count + k, np.full(marked, 30), at[2 * count + k] + 10, at[count + k]], axis=1)])
    trans = np.zeros(rows.shape[0], dtype=bool)
    trans[:count * count] = (i == j) & (i < marked)
    return reads, rows, trans


def tandem_reads(seed=73):
    """reads of 120 letters cut every 5 letters from 60 random letters, 30 copies
    of a unit of 7, 60 random letters: at minimum length 30 a read inside the
    tandem region has 91 terminal suffixes of its own, more than a wave is wide,
    and matches at most of their lengths"""
    rng = np.random.default_rng(seed)
    text = np.concatenate([rng.integers(0, 4, 60, dtype=np.uint8), np.tile(rng.integers(0, 4, 7, dtype=np.uint8), 30),
                           rng.integers(0, 4, 60, dtype=np.uint8)])
    return [text[a:a + 120].copy() for a in range(0, text.size - 120 + 1, 5)]


def border_reads(seed=47):
    """r, t1, t2, w: the longest overlap of r goes to t1, which leaves the text in
    front of w; the shorter one to t2 proves (r, w, 15) transitive"""
    rng = np.random.default_rng(seed)
    text = rng.integers(0, 4, 120, dtype=np.uint8)
    other = rng.integers(0, 4, 40, dtype=np.uint8)
    return [text[0:50], np.concatenate([text[10:50], other[:10]]), text[20:70], text[35:85]]


def short_implied_reads(seed=53):
    """r, t, w: r and w overlap by 15, t overlaps w by 30 with a left part of 8
    letters that is not r's: no overlap from r to t is implied, of 15 letters or
    of fewer, and (r, w, 15) is irreducible"""
    rng = np.random.default_rng(seed)
    text = rng.integers(0, 4, 100, dtype=np.uint8)
    return [text[0:40], np.concatenate([3 - text[17:25], text[25:55]]), text[25:65]]


def mirrored_set(reads):
    return sr.mirrored(sr.joined(reads))
