"""Brute-force restatement of include/gtamd_contained.h, independent of any
table: the verdict of every read of a set by the definition as written, with
the reads compared as byte strings, and the set that is left.  Also the seeded
read sets the tests share, with the planted cases the definition names.  Test
infrastructure only."""
import numpy as np

import spm_reference as sr
from spmred_reference import revcomp

KEPT, DUPLICATE, AFFIX, INTERNAL, SELF_COMPLEMENTARY = range(5)
NAMES = ("kept", "duplicates", "affixes", "internal", "self_complementary")
DEFAULT_MASK = 1 << DUPLICATE | 1 << AFFIX
STRICT_MASK = DEFAULT_MASK | 1 << INTERNAL | 1 << SELF_COMPLEMENTARY


def verdicts(reads):
    """the verdict of every read, all of letters, in input order: the first that applies"""
    texts = [np.asarray(r, dtype=np.uint8).tobytes() for r in reads]
    backs = [revcomp(r).tobytes() for r in reads]
    assert all(t and max(t) < 4 for t in texts)
    first = {}                                  # a read or its reverse complement -> the lowest read that is it
    for a, (t, b) in enumerate(zip(texts, backs)):
        first.setdefault(t, a)
        first.setdefault(b, a)
    out = np.zeros(len(reads), dtype=np.uint8)
    for a, t in enumerate(texts):
        others = [w for c in range(len(reads)) if c != a for w in (texts[c], backs[c])]
        if first[t] < a:
            out[a] = DUPLICATE
        elif any(len(w) > len(t) and (w.startswith(t) or w.endswith(t)) for w in others):
            out[a] = AFFIX
        elif any(t in w[1:-1] for w in others):
            out[a] = INTERNAL
        elif t == backs[a]:
            out[a] = SELF_COMPLEMENTARY
    return out


def tallies(v):
    return dict(zip(NAMES, np.bincount(v, minlength=5).tolist()))


def kept_reads(reads, v, strict=False):
    mask = STRICT_MASK if strict else DEFAULT_MASK
    return [r for r, x in zip(reads, v.tolist()) if not mask >> x & 1]


def kept_symbols(reads, v, strict=False):
    """the encoded set that is left: the kept reads in input order, a separator between two"""
    return sr.joined(kept_reads(reads, v, strict))


def self_complementary(rng, length):
    half = rng.integers(0, 4, length // 2, dtype=np.uint8)
    return np.concatenate([half, revcomp(half)])


def seeded_reads(seed, length):
    """60 to 80 reads: cut from a random text of 400 letters, 40 % of them
    reverse-complemented, and planted ones: duplicates, reverse-complement
    duplicates (of a later read too: the lower number is then the mirror copy),
    self-complementary reads, one of them twice, and -- length (least, most) --
    prefixes, suffixes and inner pieces of reads, on either strand.  length: a
    number, or (least, most)"""
    rng = np.random.default_rng(seed)
    text = rng.integers(0, 4, 400, dtype=np.uint8)
    total = int(rng.integers(60, 81))
    variable = not isinstance(length, int)
    reads = []
    for _ in range(total - (26 if variable else 12)):
        k = int(rng.integers(length[0], length[1] + 1)) if variable else length
        at = int(rng.integers(0, text.size - k + 1))
        r = text[at:at + k].copy()
        reads.append(revcomp(r) if rng.random() < 0.4 else r)
    cut = len(reads)

    def pick():
        return reads[int(rng.integers(0, cut))]

    def either(r):
        return revcomp(r) if rng.random() < 0.5 else r.copy()

    for _ in range(4):
        reads.append(pick().copy())
    for _ in range(4):
        reads.append(revcomp(pick()))
    even = length if not variable else 2 * int(rng.integers(length[0] // 2, length[1] // 2 + 1))
    palindrome = self_complementary(rng, even)
    reads += [palindrome, palindrome.copy(), self_complementary(rng, even)]
    reads.append(either(reads[0]))
    if variable:
        for _ in range(4):
            r = pick()
            reads.append(either(r[:int(rng.integers(5, r.size))]))
        for _ in range(4):
            r = pick()
            reads.append(either(r[int(rng.integers(1, r.size - 4)):]))
        for _ in range(4):
            r = pick()
            a = int(rng.integers(1, r.size - 6))
            reads.append(either(r[a:int(rng.integers(a + 5, r.size))]))
        # the blind spot of the reference: a duplicate that is a prefix of a third read, and one that is a suffix
        r = pick()
        reads += [r[:r.size - 3].copy(), r[:r.size - 3].copy()]
    assert len(reads) == total
    return [reads[k] for k in rng.permutation(total)]


def copies_on_both_strands(seed, count, length=36, others=8):
    """one read `count` times, about half of them reverse-complemented, among `others` other reads"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 4, length, dtype=np.uint8)
    reads = [revcomp(r) if rng.random() < 0.5 else r.copy() for _ in range(count)]
    reads += [rng.integers(0, 4, length, dtype=np.uint8) for _ in range(others)]
    return [reads[k] for k in rng.permutation(len(reads))]


def llv_reads(seed=11):
    """(reads, verdicts of the last five): 18 reads of 256 to 300 letters cut every
    150 letters, then a 260-letter prefix of one, the reverse complement of a
    suffix of 270, an inner piece of 270, a duplicate and a reverse-complement
    duplicate: LCP values beyond a byte decide"""
    rng = np.random.default_rng(seed)
    text = rng.integers(0, 4, 3000, dtype=np.uint8)
    lengths = rng.integers(256, 301, 18)
    lengths[[4, 7, 9]] = 300
    reads = [text[150 * k:150 * k + int(lengths[k])].copy() for k in range(18)]
    reads += [reads[4][:260].copy(), revcomp(reads[7][-270:]), reads[9][10:280].copy(), reads[2].copy(),
              revcomp(reads[3])]
    return reads, [AFFIX, AFFIX, INTERNAL, DUPLICATE, DUPLICATE]


def wide_interval_reads(width, seed=13):
    """(reads, inner): `width` reads that start with the same 24 letters, those 24
    letters as a read of their own at number 41, their reverse complement at number
    20, one other read; inner: the `width` reads each behind 30 other letters, and
    the 24 letters last, which stand inside every one of them"""
    rng = np.random.default_rng(seed)
    head = rng.integers(0, 4, 24, dtype=np.uint8)
    long = [np.concatenate([head, rng.integers(0, 4, 20, dtype=np.uint8)]) for _ in range(width)]
    reads = list(long)
    reads.insert(40, head.copy())
    reads.insert(20, revcomp(head))
    reads.append(rng.integers(0, 4, 44, dtype=np.uint8))
    inner = [np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), r]) for r in long] + [head]
    return reads, inner


def blind_spot_sets(seed=17):
    """[(reads, verdicts)]: a duplicate that is also a prefix, a suffix or an inner
    piece of a third read, on either strand: both copies go, of which the
    reference keeps one"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 4, 50, dtype=np.uint8), rng.integers(0, 4, 40, dtype=np.uint8)
    out = []
    for piece in (a[:30], a[20:], revcomp(a[:30]), revcomp(a[20:])):
        out.append(([piece, b, a, piece], [AFFIX, KEPT, KEPT, DUPLICATE]))
        out.append(([b, piece, revcomp(piece), a], [KEPT, AFFIX, DUPLICATE, KEPT]))
    out.append(([a[10:40], b, a, a[10:40]], [INTERNAL, KEPT, KEPT, DUPLICATE]))
    return out


def sized_reads(count, seed=29, length=24):
    """`count` reads of one length, every fifth a duplicate of an earlier one on
    either strand, every 37th self-complementary"""
    rng = np.random.default_rng(seed + count)
    reads = []
    for k in range(count):
        if k % 5 == 4:
            r = reads[int(rng.integers(0, k))]
            reads.append(revcomp(r) if rng.random() < 0.5 else r.copy())
        elif k % 37 == 11:
            reads.append(self_complementary(rng, length))
        else:
            reads.append(rng.integers(0, 4, length, dtype=np.uint8))
    return reads


# ---- the tool: its input files, and what it prints and writes ----

LETTERS = "acgt"
CODES = {c: k for k, c in enumerate(LETTERS)}
VERSION = "1.2"                 # GT_READJOINER_VERSION


def text_of(read):
    return "".join(LETTERS[c] if c < 4 else "n" for c in np.asarray(read).tolist())


def write_fasta(path, reads, width=None):
    """reads as FASTA, the letters of a read on one line or on lines of `width`"""
    with open(path, "w") as f:
        for k, r in enumerate(reads):
            t = text_of(r)
            lines = [t] if not width else [t[a:a + width] for a in range(0, len(t), width)]
            f.write(">read%d\n%s\n" % (k, "\n".join(lines)))


def write_fastq(path, reads):
    """reads as FASTQ in the four-line form"""
    with open(path, "w") as f:
        for k, r in enumerate(reads):
            f.write("@q%d\n%s\n+\n%s\n" % (k, text_of(r), "I" * len(r)))


def parse_reads(path):
    """the reads of a FASTA or a four-line FASTQ file, a wildcard as 254"""
    with open(path) as f:
        lines = f.read().split("\n")
    out = []
    if lines[0].startswith("@"):
        texts = lines[1::4]
        texts = texts[:len(lines) // 4]
    else:
        texts = []
        for line in lines:
            if line.startswith(">"):
                texts.append("")
            elif texts:
                texts[-1] += line.strip()
    for t in texts:
        out.append(np.array([CODES.get(c, 254) for c in t.lower()], dtype=np.uint8))
    return out


def file_figures(paths):
    """per input file what the tool's file table is made of, before the verdicts:
    (reads, [dict(filesize, invalid_reads, invalid_letters)], valid reads with their file)"""
    import os
    figures, valid = [], []
    for f, path in enumerate(paths):
        reads = parse_reads(path)
        bad = [r for r in reads if (r >= 254).any()]
        figures.append(dict(filesize=os.path.getsize(path), reads=len(reads), invalid_reads=len(bad),
                            invalid_letters=sum(r.size for r in bad)))
        valid += [(r, f) for r in reads if not (r >= 254).any()]
    return figures, valid


def p_fas(kept):
    """X.p.fas: `>` and the read on a line each, lower case"""
    return "".join(">\n%s\n" % text_of(r) for r in kept).encode()


def cntlist(removed):
    """X.cnt in Readjoiner's bit format: a 0 byte, the size of a word, the number of
    reads, the bits of the removed ones, read k bit 63 - k % 64 of word k // 64"""
    removed = np.asarray(removed, dtype=bool)
    words = np.zeros((removed.size + 63) // 64, dtype=np.uint64)
    for k in np.flatnonzero(removed).tolist():
        words[k // 64] |= np.uint64(1) << np.uint64(63 - k % 64)
    return b"\x00\x08" + np.uint64(removed.size).tobytes() + words.tobytes()


def _percent(count, total):
    return "%.2f" % (np.float32(count) * np.float32(100) / np.float32(total))


def expected_stdout(readset, paths, mode="default", strict=False, fasta=False, cnt=False):
    """the lines of the tool, as the reference words them
    (gt_readjoiner_prefilter.c:296-505, without the line of X.rlt): mode default,
    verbose, quiet or encodeonly (which is verbose too, as the goldens record it)"""
    if mode == "quiet":
        return b""
    verbose = mode in ("verbose", "encodeonly")
    figures, valid = file_figures(paths)
    total = sum(f["reads"] for f in figures)
    invalid = sum(f["invalid_reads"] for f in figures)
    lengths = [r.size for r, _ in valid]
    varlen = not lengths or min(lengths) != max(lengths)
    out = ["gt readjoiner prefilter (version %s)" % VERSION]
    if verbose:
        out += ["readset name = %s" % readset, "input files = %s" % ", ".join(paths)]
    out.append("number of reads in complete readset = %d" % total)
    if verbose:
        out.append("read length = variable [%d..%d]" % (min(lengths) + 1, max(lengths) + 1) if varlen
                   else "read length = %d" % lengths[0])
        out.append("total length of complete readset = %d"
                   % (sum(lengths) - 1 + sum(f["invalid_letters"] for f in figures)))
        out.append("low-quality reads = %d [%s %% of input]" % (invalid, _percent(invalid, total)))
    else:
        out.append("low-quality reads = %d" % invalid)
    saved = "%s.%s" % (readset, "(esq|ssp)" if varlen else "esq")
    if mode == "encodeonly":
        if fasta:
            out.append("readset saved: %s.p.fas" % readset)
        out += ["readset saved: %s" % saved, "number of reads in output readset = %d" % len(valid)]
        return "".join("# %s\n" % l for l in out).encode()
    v = verdicts([r for r, _ in valid])
    fig = tallies(v)
    contained = fig["duplicates"] + fig["affixes"]
    left = len(valid) - contained - (fig["internal"] + fig["self_complementary"] if strict else 0)
    out.append("contained reads = %d [%s %% of input]" % (contained, _percent(contained, total)) if verbose
               else "contained reads = %d" % contained)
    out.append("number of reads in filtered readset = %d" % left)
    if verbose and cnt:
        out.append("contained reads list saved: %s.cnt" % readset)
    if verbose and fasta:
        out.append("suffix-prefix-free readset saved: %s.p.fas" % readset)
    if left and verbose:
        out.append("suffix-prefix-free readset saved: %s" % saved)
    if not left:
        out.append("no readset saved as no sequence passed the filters")
    if strict:
        out += ["reads inside other reads removed = %d" % fig["internal"],
                "self-complementary reads removed = %d" % fig["self_complementary"]]
    return "".join("# %s\n" % l for l in out).encode()
