"""Plain numpy restatement of what the device encoder derives from encoded
symbols (0..sigma-1, 254 wildcard, 255 separator): the sequence statistics and
the sections of INDEX.esq, written from include/gtamd_encode.h and the layout
comments it cites (src/core/encseq.c:85-99, 2594-2607, 2771-2835, 2324-2447),
not from the kernels.  No device, no C.  Test infrastructure only;
tests/test_esq_sections_reference.py holds it to the host writer's files."""
import numpy as np

WILDCARD, SEPARATOR = 254, 255


def _runs(mask):
    """lengths of the maximal runs of True"""
    m = np.concatenate([[False], mask, [False]]).astype(np.int8)
    d = np.diff(m)
    return np.flatnonzero(d == -1) - np.flatnonzero(d == 1)


def _expected_summary(enc, sigma):
    sp, wc = _runs(enc >= 254), _runs(enc == 254)
    seqs, nonsp = _runs(enc != 255), _runs(enc < 254)

    def lead(mask):
        return int(np.argmin(mask)) if not mask.all() else mask.size

    def pieces(r, maxv):
        return int(((r + maxv) // (maxv + 1)).sum())
    return {
        "totallength": enc.size, "numofsequences": int((enc == 255).sum()) + 1,
        "specialcharacters": int((enc >= 254).sum()), "realspecialranges": sp.size,
        "specialrangestab": [pieces(sp, 255), pieces(sp, 65535), sp.size],
        "lengthofspecialprefix": lead(enc >= 254),
        "lengthofspecialsuffix": lead((enc >= 254)[::-1]),
        "wildcards": int((enc == 254).sum()), "realwildcardranges": wc.size,
        "wildcardrangestab": [pieces(wc, 255), pieces(wc, 65535), wc.size],
        "lengthofwildcardprefix": lead(enc == 254),
        "lengthofwildcardsuffix": lead((enc == 254)[::-1]),
        "lengthoflongestnonspecial": int(nonsp.max()) if nonsp.size else 0,
        "minseqlen": int(seqs.min()), "maxseqlen": int(seqs.max()),
        "equallength": int(seqs.min() == seqs.max() and not (enc == 254).any()),
        "characterdistribution": [int((enc == c).sum()) for c in range(sigma)] + [0] * (32 - sigma),
    }


def twobit_units(n):
    """2 + (n-1)/32 words, 2 if n < 32"""
    return 2 if n < 32 else 2 + (n - 1) // 32


def specialbits_units(n):
    return 1 + (n + 63) // 64


def twobit(enc, bitaccess, fill):
    """two bits per symbol, 32 symbols per word, the first symbol in the top bits;
    a special is stored as wildcard 0 / separator 1 (bitaccess) or as `fill`; the
    positions behind the sequence are 0"""
    n, units = int(enc.size), twobit_units(int(enc.size))
    codes = np.zeros(32 * units, dtype=np.uint64)
    codes[:n] = enc
    special = np.zeros(32 * units, dtype=bool)
    special[:n] = enc >= WILDCARD
    if bitaccess:
        codes[special] = (codes[special] == SEPARATOR).astype(np.uint64)
    else:
        codes[special] = np.uint64(fill)
    assert int(codes.max(initial=0)) < 4, "two bits hold the codes 0..3 only"
    shift = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)
    return np.bitwise_or.reduce(codes.reshape(units, 32) << shift, axis=1)


def specialbits(enc):
    """one bit per position, the first in the top bit of a word; set for every
    special and for the 64 positions behind the sequence"""
    n, units = int(enc.size), specialbits_units(int(enc.size))
    bits = np.zeros(64 * units, dtype=np.uint64)
    bits[:n] = enc >= WILDCARD
    bits[n:n + 64] = 1
    shift = np.uint64(63) - np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(bits.reshape(units, 64) << shift, axis=1)


def bytecompress(enc, sigma, bits):
    """`bits` per symbol, most significant bit first, one stream over all symbols:
    (bits*n+7)/8 bytes; wildcard = sigma, separator = sigma + 1"""
    v = enc.astype(np.uint64)
    v[enc == WILDCARD] = sigma
    v[enc == SEPARATOR] = sigma + 1
    assert int(v.max(initial=0)) < (1 << bits)
    place = np.uint64(bits - 1) - np.arange(bits, dtype=np.uint64)
    stream = ((v[:, None] >> place) & np.uint64(1)).astype(np.uint8).reshape(-1)
    out = np.packbits(stream)            # big end first, zero bits behind the last symbol
    assert out.size == (bits * int(enc.size) + 7) // 8
    return out


def _run_bounds(mask):
    m = np.concatenate([[False], mask, [False]]).astype(np.int8)
    d = np.diff(m)
    return np.flatnonzero(d == 1).astype(np.uint64), np.flatnonzero(d == -1).astype(np.uint64)


def wildcard_runs(enc):
    """(start, length) of every maximal run of wildcards, in order"""
    first, behind = _run_bounds(enc == WILDCARD)
    return first, behind - first


def separators(enc):
    return np.flatnonzero(enc == SEPARATOR).astype(np.uint64)


def first_empty_sequence(enc):
    """position of the first separator that stands at either end of the sequence
    or behind another separator; None if every sequence has a symbol"""
    n = int(enc.size)
    for i in np.flatnonzero(enc == SEPARATOR).tolist():
        if i == 0 or i + 1 == n or enc[i - 1] == SEPARATOR:
            return i
    return None
