"""The random inputs and switch draws of the differential fuzzer
(tools/fuzz_gpu.py), shared with the fixed-seed replay of
tests/test_switches_gpu.py.  Both take them in the same order -- sequence,
prefix length, MSD switches (not in a case of 64-bit positions), part switches
-- so case k of the replay has the switches of case k of
`fuzz_gpu.py --seed REPLAY_SEED`, up to its part build.  The writers of the
fuzzer's FASTA and FASTQ files and its packed-index options are here too: the
sanitized run of the checker (test_host_sanitized.py) takes them after the prefix
length."""
import numpy as np


def random_sequence(rng, sigma):
    n = int(rng.choice([1, 2, 3, 17, 64, 255, 256, 257, 1000, 4096, 4097, 9000, 20000]))
    if rng.integers(0, 25) == 0:          # several tiles of every kernel, now and then
        n = int(rng.choice([70000, 140000]))
    n = max(1, int(n * rng.uniform(0.5, 1.0)))
    kind = rng.integers(0, 4)
    if kind == 0:                       # low entropy: few letters
        enc = rng.integers(0, min(sigma, rng.integers(1, 3) + 1), size=n).astype(np.uint8)
    else:
        enc = rng.integers(0, sigma, size=n).astype(np.uint8)
    # copies of earlier stretches (long LCPs, big tie groups)
    for _ in range(int(rng.integers(0, 8))):
        if n < 8:
            break
        length = int(rng.integers(2, max(3, min(n // 2, 4000))))
        src = int(rng.integers(0, n - length + 1))
        dst = int(rng.integers(0, n - length + 1))
        enc[dst:dst + length] = enc[src:src + length].copy()
    # tandem repeats
    for _ in range(int(rng.integers(0, 4))):
        period = int(rng.integers(1, 7))
        length = int(rng.integers(period, max(period + 1, min(n, 3000))))
        at = int(rng.integers(0, max(1, n - length)))
        unit = rng.integers(0, sigma, size=period).astype(np.uint8)
        enc[at:at + length] = np.resize(unit, length)[:len(enc[at:at + length])]
    # wildcard runs and separators (never an empty sequence)
    for _ in range(int(rng.integers(0, 6))):
        length = int(rng.choice([1, 1, 2, 5, 40, 300, 700]))
        at = int(rng.integers(0, n))
        enc[at:at + length] = 254
    nsep = int(rng.integers(0, 6))
    for at in rng.integers(1, max(2, n - 1), size=nsep):
        at = int(at)
        if 0 < at < n - 1 and enc[at - 1] != 255 and enc[at + 1] != 255:
            enc[at] = 255
    if enc[0] == 255:
        enc[0] = 0
    if enc[-1] == 255:
        enc[-1] = 0
    return enc


def prefix_length(rng, sigma):
    """the prefix length of the fuzzer's first build (check_engine)"""
    return int(rng.integers(0, (8 if sigma == 4 else 3) + 1))


# pair chunks that differ from the default (16 at every size below 17.8 M pair
# records); 17 is rounded up to 32
PAIR_CHUNKS = [17, 32, 128, 1024]


def msd_switches(rng):
    """the switches of a whole-table build through the MSD first sort: a random
    depth of level C, a random limit of the one-workgroup path and, one case in
    four, the LDS radix fallback in every run; the rank table of the rounds in
    windows of a random size (one case in three the whole table), random chunks of
    the pair comparison, the pairs' table entries at random places of the flow, a
    random crowded-bin limit, one case in four without the pair path"""
    return {"GTAMD_MSD": "1", "GTAMD_MSD_CBITS": str(int(rng.integers(0, 9))),
            "GTAMD_MSD_BIG_MAX": str(int(rng.choice([4096, 8192, 524288]))),
            "GTAMD_MSD_RADIX": "1" if rng.integers(0, 4) == 0 else "0",
            "GTAMD_RANK_WINDOW_BITS": str(int(rng.choice([3, 4, 6, 9, 15]))),
            "GTAMD_RANK_ALL_WINDOWS": "1" if rng.integers(0, 3) == 0 else "0",
            "GTAMD_WIN_FILTER_LDS": "0" if rng.integers(0, 3) == 0 else "1",
            "GTAMD_PAIR_CHUNK": str(int(rng.choice(PAIR_CHUNKS))),
            "GTAMD_APPLY_EARLY": str(int(rng.integers(0, 3))),
            "GTAMD_MSD_BIN_LIMIT": str(int(rng.choice([2, 16, 128]))),
            "GTAMD_MSD_PACK": str(int(rng.integers(0, 2))),
            "GTAMD_MSD_PACK_CAP": str(int(rng.choice([1024, 2048, 4096]))),
            "GTAMD_ROUND_STRIDE": str(int(rng.choice([512, 1024, 1536, 2048]))),
            "GTAMD_NO_SMALL_GROUPS": "1" if rng.integers(0, 4) == 0 else "0",
            "GTAMD_NO_PAIRS": "1" if rng.integers(0, 4) == 0 else "0"}


def parts_switches(rng):
    """(number of parts, switches) of a part build"""
    parts = int(rng.integers(2, 6))
    env = {"GTAMD_WIN_FILTER_LDS": "0" if rng.integers(0, 3) == 0 else "1",
           "GTAMD_PAIR_CHUNK": str(int(rng.choice(PAIR_CHUNKS))),
           "GTAMD_NO_PAIRS": "1" if rng.integers(0, 5) == 0 else "0"}
    return parts, env


# line widths write_fasta draws from, one per sequence
LINE_WIDTHS = [1, 7, 60, 70, 4095, 4096, 100000]


def _alphabet_text(sigma):
    protein = sigma == 20
    return (b"LVIFKREDAGSTNQYWPHMC" if protein else b"ACGT",
            b"XUBZJO*-" if protein else b"NSYWRKVBDHM")


def write_fasta(rng, enc, sigma, path):
    """enc as a FASTA file: one record per sequence, a random wildcard letter for
    every wildcard, DNA in random case, a random line width per record, one file
    in four with CRLF line ends, a blank line after one line in twenty.  Returns
    what was drawn: {"crlf": bool, "widths": set}."""
    protein = sigma == 20
    letters, wild = _alphabet_text(sigma)
    eol = b"\r\n" if rng.integers(0, 4) == 0 else b"\n"
    widths = set()
    with open(path, "wb") as f:
        start = 0
        cuts = list(np.flatnonzero(enc == 255)) + [enc.size]
        for i, end in enumerate(cuts):
            f.write(b">seq%d some text\t%d" % (i, int(rng.integers(0, 1000))) + eol)
            seq = enc[start:end]
            txt = bytearray(len(seq))
            for j, c in enumerate(seq):
                ch = wild[int(rng.integers(0, len(wild)))] if c == 254 else letters[c]
                if not protein and rng.integers(0, 3) == 0:
                    ch = ord(chr(ch).lower())
                txt[j] = ch
            width = int(rng.choice(LINE_WIDTHS))
            widths.add(width)
            for a in range(0, len(txt), width):
                f.write(bytes(txt[a:a + width]) + eol)
                if rng.integers(0, 20) == 0:
                    f.write(eol)
            start = end + 1
    return {"crlf": eol == b"\r\n", "widths": widths}


def write_fastq(rng, enc, sigma, path):
    """the same sequences as four-line FASTQ records with random qualities, one
    record in five without a name, one in three with the name repeated behind
    the '+'.  Returns the number of records."""
    letters, wild = _alphabet_text(sigma)
    cuts = list(np.flatnonzero(enc == 255)) + [enc.size]
    with open(path, "wb") as f:
        start = 0
        for i, end in enumerate(cuts):
            seq = enc[start:end]
            txt = bytes(wild[int(rng.integers(0, len(wild)))] if c == 254 else letters[c] for c in seq)
            name = b"read%d x=%d" % (i, int(rng.integers(0, 99))) if rng.integers(0, 5) else b""
            qual = bytes(rng.integers(33, 127, size=len(txt), dtype=np.uint8))
            f.write(b"@" + name + b"\n" + txt + b"\n+" + (name if rng.integers(0, 3) == 0 else b"") + b"\n" +
                    qual + b"\n")
            start = end + 1
    return len(cuts)


def pck_options(rng, sigma):
    """options of one packed-index build: block size, blocks per bucket, locate
    interval and mode, both flavours, -sprank"""
    bmax = 10 if sigma == 4 else 3
    return dict(bsize=int(rng.integers(1, bmax + 1)),
                blbuck=int(rng.choice([1, 2, 3, 5, 8, 8, 8, 13, 64, 300])),
                locfreq=int(rng.choice([0, 1, 2, 3, 7, 16, 16, 32, 1000])),
                locbitmap=[None, True, False][int(rng.integers(0, 3))],
                mkindex=bool(rng.integers(0, 2)), sprank=bool(rng.integers(0, 2)))
