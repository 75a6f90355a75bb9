"""Encoded sequences whose special runs and ends stand on the borders of the
device encoder's kernels (genometools_amd/csrc/esa_encode.hip): the case list
shared by tests/test_esq_sections_reference.py, tests/test_esq_sections_gpu.py
and the recipe tests/golden/make_golden_esq_edges.py.

The symbols are made by arithmetic, never by a random generator, so that the
recipe and the tests regenerate the same bytes on any numpy.

The borders, stated once:
  THREAD = 16    symbols per thread of k_run_summary / k_positions (EN_PER)
  TILE   = 4096  symbols per block of those kernels (EN_TILE = 256 * EN_PER)
  BLOCK  = 256   threads per block of k_empty_sequence and the pack kernels, which
                 handle 1 (empty sequence), 8 (bit packing), 32 (two-bit words) or
                 64 (special bits) symbols per thread
  256, 65536     the longest run one entry of an 8- / 16-bit range table holds

len(cases()) == 384: 133 DNA, 133 protein and 59 for each of the two alphabets
made with gtamd_encoder_create_map; the longest has 196613 symbols.
"""
import collections
import functools

import numpy as np

THREAD, TILE, BLOCK = 16, 4096, 256
W, S = 254, 255

# name -> (number of letters, bits per symbol of the bit packing)
ALPHABETS = collections.OrderedDict([("dna", (4, 3)), ("protein", (20, 5)),
                                     ("ab", (2, 2)), ("l28", (28, 5))])
STANDARD = ("dna", "protein")
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097,
           8191, 8192, 8193, 12288)
BIG = 3 * 65536 + 5

Case = collections.namedtuple("Case", "name alphabet sigma bits enc")


def letters(n, sigma):
    i = np.arange(n, dtype=np.uint64)
    return ((np.uint64(7) * i + i // np.uint64(13)) % np.uint64(sigma)).astype(np.uint8)


def _with(n, sigma, wild=(), sep=(), runs=()):
    enc = letters(n, sigma)
    for s, ln in runs:
        assert 0 <= s and ln > 0 and s + ln <= n
        enc[s:s + ln] = W
    for p in wild:
        enc[p] = W
    for p in sep:
        enc[p] = S
    return enc


def _contents(sigma, standard):
    """(name, symbols) of every content for an alphabet of sigma letters"""
    out = []

    def add(name, enc):
        out.append((name, enc))
    # (a) letters only: every tile takes the shortcut of k_run_summary
    for n in LENGTHS:
        add("a-letters-n%d" % n, letters(n, sigma))
    # (b) wildcards only: the "all members" case of thread, tile and whole input
    for n in (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8193, 12288):
        add("b-wildcards-n%d" % n, np.full(n, W, dtype=np.uint8))
    # (c) a wildcard at 0, at n-1, at both
    for n in (2, 16, 17, 32, 33, 64, 65, 256, 4096, 4097, 8192, 8193):
        add("c-both-n%d" % n, _with(n, sigma, wild=(0, n - 1)))
    for n in (33, 4097):
        add("c-first-n%d" % n, _with(n, sigma, wild=(0,)))
        add("c-last-n%d" % n, _with(n, sigma, wild=(n - 1,)))
    # (f) dense specials: 5 to 8 hits per thread for the tile scan of k_positions;
    # period 3 is letter, wildcard, separator (lengths that do not end in a separator)
    for n in (16, 17, 257, 4097, 8192):
        i = np.arange(n)
        enc = letters(n, sigma)
        enc[i % 3 == 1] = W
        enc[i % 3 == 2] = S
        assert enc[-1] != S
        add("f-period3-n%d" % n, enc)
    for n in (16, 17, 257, 4097, 8193):
        enc = letters(n, sigma)
        enc[1::2] = W
        add("f-period2-n%d" % n, enc)
    if not standard:
        return out
    # (d) one wildcard run [s, s+len) in three tiles
    n = 3 * TILE
    seen = set()
    for ln in (1, 16, 255, 256, 257, 4096, 8192):
        for s in (0, 15, 16, 17, 4095, 4096, 4097, 8192 - ln, n - ln):
            if s + ln > n or (s, ln) in seen:
                continue
            seen.add((s, ln))
            add("d-run-s%d-len%d" % (s, ln), _with(n, sigma, runs=[(s, ln)]))
    for ln in (65535, 65536, 65537):
        add("d-run%d" % ln, _with(BIG, sigma, runs=[(65536 - 3, ln)]))
    # (e) separators
    for n in (64, 4097):
        add("e-sep-1-and-n-2-n%d" % n, _with(n, sigma, sep=(1, n - 2)))
    add("e-sep-4095", _with(8193, sigma, sep=(4095,)))
    add("e-sep-4096", _with(8193, sigma, sep=(4096,)))
    add("e-sep-4095-4097", _with(8193, sigma, sep=(4095, 4097)))
    # the shortest sequence is [4095, 4097), the longest [4098, 12288): both
    # straddle a tile border
    add("e-short-and-long-straddle", _with(3 * TILE, sigma, sep=(2000, 4094, 4097)))
    # equal-length sets without wildcards: K sequences of L, K*(L+1)-1 >= 4097
    for L in (31, 32, 33):
        K = -(-(TILE + 2) // (L + 1))
        n = K * (L + 1) - 1
        assert n >= TILE + 1
        add("e-eqlen-L%d" % L, _with(n, sigma, sep=range(L, n, L + 1)))
    # (g) a tile of wildcards, and one of wildcard wildcard separator, between two
    # tiles of letters
    add("g-wildcard-tile", _with(3 * TILE, sigma, runs=[(TILE, TILE)]))
    enc = _with(3 * TILE, sigma, runs=[(TILE, TILE)])
    enc[TILE + 2:2 * TILE:3] = S
    assert enc[2 * TILE - 1] == W
    add("g-triplet-tile", enc)
    # (h) three run ends on one border: wildcards up to 4095, a separator at 4096,
    # a wildcard at 4097
    add("h-three-ends", _with(2 * TILE, sigma, runs=[(4000, 96)], sep=(4096,), wild=(4097,)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for alphabet, (sigma, bits) in ALPHABETS.items():
        for name, enc in _contents(sigma, alphabet in STANDARD):
            enc.setflags(write=False)
            out.append(Case("%s-%s" % (name, alphabet), alphabet, sigma, bits, enc))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ---- the subset the reference itself encoded (tests/golden/golden_esq_edges.json):
# no empty sequence, DNA and protein only
GOLDEN_CASES = ("d-run65535-dna", "d-run65536-dna", "d-run65537-dna", "d-run65536-protein",
                "c-both-n32-dna", "c-both-n64-dna", "c-both-n4096-protein", "c-both-n4097-dna",
                "a-letters-n4096-dna", "f-period3-n4097-dna", "f-period3-n257-protein",
                "e-eqlen-L32-dna", "e-sep-1-and-n-2-n4097-dna", "h-three-ends-dna")
DNA_LETTERS, PROTEIN_LETTERS = "acgt", "LVIFKREDAGSTNQYWPHMC"


def fasta_name(case):
    return case.name + (".faa" if case.alphabet == "protein" else ".fna")


def fasta_bytes(case):
    """the case as FASTA: 70 columns, one description per sequence"""
    assert case.alphabet in STANDARD
    table = np.zeros(256, dtype=np.uint8)
    text = DNA_LETTERS if case.alphabet == "dna" else PROTEIN_LETTERS
    table[:len(text)] = np.frombuffer(text.encode(), dtype=np.uint8)
    table[W] = ord("n" if case.alphabet == "dna" else "X")
    out = []
    bounds = [-1] + np.flatnonzero(case.enc == S).tolist() + [case.enc.size]
    for k in range(len(bounds) - 1):
        seq = table[case.enc[bounds[k] + 1:bounds[k + 1]]].tobytes()
        assert seq
        out.append(b">seq%d of %s\n" % (k, case.name.encode()))
        out.extend(seq[i:i + 70] + b"\n" for i in range(0, len(seq), 70))
    return b"".join(out)


def legal_access_types(case, equallength):
    if case.alphabet == "protein":
        return ["direct", "bytecompress"]
    return ["direct", "bit", "uchar", "ushort", "uint32"] + (["eqlen"] if equallength else [])
