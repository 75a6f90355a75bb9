"""The brute force behind the tag match tests, without tables: the definition of
include/gtamd_tagmatch.h applied to every start position at once.  Per tag and
strand Myers' bit-vector column runs over all p together (numpy uint64 across
p, at most m + K steps), keeping only the value of row m; the first depth at
which it is <= K is the match of p.  The suffix table is used for nothing but
the order of the records.  Also the line formatter of `gt tagerator`
(tgr_showmatch, src/match/tagerator.c:81-189) and the table of edit distances
that judges both this file and the device's column."""
import numpy as np

import oracle_util as ou

FORWARD, REVCOMP, BEST, WITH_WILDCARDS = 1, 2, 4, 8
NO_K = 0xffffffff
DNA = "acgt"
PROTEIN = "LVIFKREDAGSTNQYWPHMC"          # the order of the codes (src/core/alphabet.c)
OUTPUT_KEYWORDS = ("tagnum", "tagseq", "dblength", "dbstartpos", "abspos", "dbsequence", "strand", "edist")
DEFAULT_OUTPUT = ("tagnum", "tagseq", "dblength", "dbstartpos", "strand")
_ONE = np.uint64(1)


def revcomp(tag):
    return (3 - np.asarray(tag, dtype=np.uint8))[::-1].copy()


def dp_table(tag, text):
    """D[i][d]: the edit distance of tag[:i] and text[:d]; a symbol >= 254
    equals nothing"""
    m, L = len(tag), len(text)
    D = np.zeros((m + 1, L + 1), dtype=np.int64)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(L + 1)
    for i in range(1, m + 1):
        for d in range(1, L + 1):
            same = tag[i - 1] == text[d - 1] and text[d - 1] < 254
            D[i, d] = min(D[i - 1, d] + 1, D[i, d - 1] + 1, D[i - 1, d - 1] + (0 if same else 1))
    return D


def dp_match(tag, enc, p, K, wild):
    """(len, dist) of start position p by the definition and the table, or None"""
    stop = p
    while stop < len(enc) and stop - p < len(tag) + K and (enc[stop] < 254 or (wild and enc[stop] == 254)):
        stop += 1
    row = dp_table(tag, enc[p:stop])[len(tag)]
    for d in range(1, stop - p + 1):
        if row[d] <= K:
            return d, int(row[d])
    return None


def strand_matches(enc, tag, K, wild):
    """(p, len, dist) arrays of one tag as given (one strand), ascending p"""
    enc = np.asarray(enc, dtype=np.uint8)
    n, m = enc.size, len(tag)
    assert 1 <= m <= 64 and 0 <= K < m
    eq = np.zeros(256, dtype=np.uint64)
    for i, c in enumerate(tag):
        eq[int(c)] |= _ONE << np.uint64(i)
    eq[254] = eq[255] = 0
    padded = np.concatenate([enc, np.full(m + K + 1, 255, dtype=np.uint8)])
    top = np.uint64(m - 1)
    Pv = np.full(n, ~np.uint64(0), dtype=np.uint64)
    Mv = np.zeros(n, dtype=np.uint64)
    score = np.full(n, m, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    length = np.zeros(n, dtype=np.int64)
    dist = np.zeros(n, dtype=np.int64)
    for d in range(m + K):
        s = padded[d:d + n]
        alive &= (s != 255) & ((s != 254) | wild)
        if not alive.any():
            break
        Eq = eq[s]
        Xv = Eq | Mv
        Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq
        Ph = Mv | ~(Xh | Pv)
        Mh = Pv & Xh
        score += ((Ph >> top) & _ONE).astype(np.int64) - ((Mh >> top) & _ONE).astype(np.int64)
        Ph = (Ph << _ONE) | _ONE
        Mh = Mh << _ONE
        Pv = Mh | ~(Xv | Ph)
        Mv = Ph & Xv
        hit = alive & (score <= K)
        length[hit] = d + 1
        dist[hit] = score[hit]
        alive &= ~hit
    p = np.flatnonzero(length)
    return p, length[p], dist[p]


def expected(enc, suf, tags, K, flags=FORWARD | REVCOMP):
    """(records of shape (R, 3) in the order of the header, K' per tag)"""
    enc = np.asarray(enc, dtype=np.uint8)
    rank = np.empty(enc.size + 1, dtype=np.int64)
    rank[np.asarray(suf, dtype=np.int64)] = np.arange(enc.size + 1)
    wild = bool(flags & WITH_WILDCARDS)
    out, best = [], np.full(len(tags), NO_K, dtype=np.uint32)
    for t, tag in enumerate(tags):
        tag = np.asarray(tag, dtype=np.uint8)
        for k in (range(K + 1) if flags & BEST else (K,)):
            found = []
            for strand, bit in ((0, FORWARD), (1, REVCOMP)):
                if flags & bit:
                    p, length, dist = strand_matches(enc, revcomp(tag) if strand else tag, k, wild)
                    order = np.argsort(rank[p], kind="stable")
                    found.append(np.stack([np.full(p.size, 2 * t + strand, dtype=np.uint64),
                                           p[order].astype(np.uint64),
                                           length[order].astype(np.uint64) | (dist[order].astype(np.uint64) << np.uint64(32))],
                                          axis=1))
            if sum(f.shape[0] for f in found):
                best[t] = k
                out.extend(found)
                break
    return (np.concatenate(out) if out else np.zeros((0, 3), dtype=np.uint64)), best


# ---- the tool's stdout ----

def read_tags(paths):
    """the tags of FASTA files as strings, in order"""
    tags = []
    for path in paths:
        cur = None
        with open(path) as f:
            for line in f:
                if line.startswith(">"):
                    if cur is not None:
                        tags.append(cur)
                    cur = ""
                elif cur is not None:
                    cur += "".join(line.split())
        if cur is not None:
            tags.append(cur)
    return tags


def encode_tag(text, letters=DNA):
    return np.array([letters.index(c) for c in text.lower()] if letters == DNA else
                    [letters.index(c) for c in text.upper()], dtype=np.uint8)


def match_line(enc, starts, letters, rec, output):
    """one line of tgr_showmatch; starts: where the subject's sequences begin"""
    p, length, dist = int(rec[1]), int(rec[2]) & 0xffffffff, int(rec[2]) >> 32
    items = []
    if "dblength" in output:
        items.append("%d" % length)
    if "dbstartpos" in output:
        if "abspos" in output:
            items.append("%d" % p)
        else:
            seq = int(np.searchsorted(starts, p, side="right")) - 1
            items.append("%d\t%d" % (seq, p - int(starts[seq])))
    if "dbsequence" in output:
        items.append("".join(letters[c] if c < 254 else "n" if letters == DNA else "X" for c in enc[p:p + length]))
    if "strand" in output:
        items.append("-" if int(rec[0]) & 1 else "+")
    if "edist" in output:
        items.append("%d" % dist)
    return "\t".join(items) if items else None


def preamble(K, index, tagfiles, output):
    shown = [k for k in OUTPUT_KEYWORDS if k in output]
    return ["# computing complete matches " + ("without differences (exact matches)" if K == 0 else
                                               "with up to %d differences" % K),
            "# indexname(esa)=%s" % index] + ["# queryfile=%s" % f for f in tagfiles] + \
           ["# for each match show: " + "".join(k + " " for k in shown)]


def tool_lines(enc, suf, letters, tags, K, flags, output=DEFAULT_OUTPUT):
    """the lines `gt tagerator` prints behind its preamble for tags given as
    strings of letters: per tag its `#` line and its matches"""
    enc = np.asarray(enc, dtype=np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(enc == 255) + 1])
    coded = [encode_tag(t, letters) for t in tags]
    rec, _ = expected(enc, suf, coded, K, flags)
    lines = []
    for t, tag in enumerate(tags):
        lines.append("#" + ("\t%d" % t if "tagnum" in output else "") +
                     (("\t" if "tagnum" in output else "") + (tag.lower() if letters == DNA else tag.upper())
                      if "tagseq" in output else ""))
        for r in rec[(rec[:, 0] >> np.uint64(1)) == t]:
            line = match_line(enc, starts, letters, r, output)
            if line is not None:
                lines.append(line)
    return lines


def block_sorted(lines):
    """the lines with those between two `#` lines sorted: the order inside one
    tag's block is the reference's by-product, not part of the comparison"""
    out, block = [], []
    for line in list(lines) + ["#"]:
        if line.startswith("#"):
            out.extend(sorted(block))
            block = []
            out.append(line)
        else:
            block.append(line)
    return out[:-1]


def fixture(name, protein=False):
    """(enc, suf) of a fixture file"""
    enc = ou.encode_fasta(ou.fixture_path(name), protein)
    return enc, ou.esa(enc, 20 if protein else 4)["suf"]
