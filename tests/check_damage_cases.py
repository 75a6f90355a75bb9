"""Damaged LCP tables for the tests of the index checker's phase 5
(genometools_amd/csrc/esa_check.hip; the criterion: include/gtamd_check.h, 5),
made by arithmetic with fixed seeds, and a model on the CPU of which branch of
the kernel meets the mismatch of every case.  TEST INFRASTRUCTURE.

A case is (text, table index r, new claim).  The claim is written into the .lcp
byte when the old and the new claim are below 255, into the value of the row's
.llv pair when both are at least 255; a case never crosses 255, so criteria 1 to
4 hold for every case (asserted).  The expected tables are the CPU oracle's.

The model restates constants of esa_check.hip: first_bad16 compares PIECE = 16
symbols, with whole words when the count is at least WORD_MIN = 8 and both
sides stay FRONT = 3 symbols behind the start and BACK = 20 in front of the end
of the sequence; a range longer than LONG (check.geometry()) goes to the work
list, which a workgroup walks in steps of STEP = 16 * 256 symbols, 16 a lane.
A CHANGE OF THOSE CONSTANTS IN esa_check.hip MUST BE FOLLOWED HERE: the
coverage asserted below is a statement about that code.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle_util as ou
from check_criteria import claims, first_suf_failure
from genometools_amd import check

WILDCARD, SEPARATOR = 254, 255
PIECE, WORD_MIN, FRONT, BACK, LANES = 16, 8, 3, 20, 256
STEP = PIECE * LANES
TILE, LONG = check.geometry()
KS = (1, 2, 7, 8, 9, 16, 17, 100)          # new claim - true value, where (a) holds there

Case = namedtuple("Case", "text r claim true s len off p q below path branch byte piece_last ma mb "
                          "front back ends step lane past_n in_llv")
Text = namedtuple("Text", "name enc sigma ora true suf rank s pairs")


# ---- texts -----------------------------------------------------------------------

class _Builder:
    """pairs X ... Y planted between random letters.  Y stands behind a wildcard,
    so the range (b) of its position starts at 0; X is the smaller suffix, so Y is
    the position p of the row and X is q."""

    def __init__(self, seed, sigma):
        self.rng, self.sigma, self.parts, self.size, self.pairs = np.random.default_rng(seed), sigma, [], 0, []

    def letters(self, k):
        return self.rng.integers(0, self.sigma, k, dtype=np.uint8)

    def add(self, a):
        a = np.asarray(a, dtype=np.uint8)
        self.parts.append(a)
        self.size += a.size

    def pair(self, off, ends, length, extra=KS, lead=True, y_len=None, flip=False):
        """copies that agree for exactly `off` symbols and then meet `ends`: a
        differing "letter", equal "specials", a "special" on one side; they differ
        again at off + k for every k of `extra`, so that (a) holds for the claim
        off + k, and agree elsewhere.  The starts take the residues mod 4 in turn;
        lead = False: X starts where the text stands; flip: X is the larger suffix."""
        i = len(self.pairs)
        if lead:
            self.add([WILDCARD])
            self.add(self.letters((i % 4 - self.size) % 4))
        x = self.letters(length)
        y = x.copy()
        if ends == "letter":
            x[off] = self.rng.integers(0, self.sigma - 1)
            y[off] = self.rng.integers(x[off] + 1, self.sigma)
            if flip:
                x[off], y[off] = y[off], x[off]
        elif ends == "specials":
            x[off] = y[off] = WILDCARD
        else:
            y[off] = WILDCARD
        for k in extra:
            if off + k < length:
                y[off + k] = (x[off + k] + 1 + self.rng.integers(0, self.sigma - 1)) % self.sigma
        xs = self.size
        self.add(x)
        self.add(self.letters((i // 4 % 4 - (self.size + 1)) % 4))
        self.add([WILDCARD])
        self.pairs.append((self.size, xs, off, ends) if flip else (xs, self.size, off, ends))
        self.add(y if y_len is None else y[:y_len])

    def enc(self):
        return np.concatenate(self.parts)


def _text_a():
    """every offset 9 ... 58 of a mismatch (bytes 0 ... 15 of pieces 0 ... 3), all 16
    residues of the two starts, one X at position 1, the last Y at the end"""
    b = _Builder(1001, 4)
    b.add(b.letters(1))
    b.pair(12, "letter", 100, lead=False)
    for d in range(9, 59):
        b.pair(d, "letter", 100)
    for d in (12, 13, 14, 15, 16, 17, 31, 32, 33):
        b.pair(d, "specials", 100)
    for d in (14, 21, 40):
        b.pair(d, "special", 100)
    b.add([WILDCARD])
    b.add(b.letters(600))
    b.pair(20, "letter", 100)
    return b.enc(), 4, b.pairs


B_OFFS = sorted(set(range(512, 528)) | {511, 513, 527, 528, 529, 4094, 4095, 4096, 4097, 4111, 4112,
                                        8191, 8192, 8193})
B_SPECIALS, B_SPECIAL = (520, 4095, 8192), (515, 4111)


def _text_b():
    """long pairs: every byte of a piece behind the work list's threshold, the
    borders of its steps of 4096; more than 600 symbols follow each mismatch"""
    b = _Builder(1002, 4)
    b.add(b.letters(50))
    for off in B_OFFS:
        extra = KS + (600,) + tuple(c - off for c in (LONG, LONG + 1, LONG + 2) if c > off)
        b.pair(off, "specials" if off in B_SPECIALS else "special" if off in B_SPECIAL else "letter",
               off + 700, extra)
    b.add([WILDCARD])
    b.add(b.letters(50))
    return b.enc(), 4, b.pairs


def _text_c():
    """protein: letters up to code 19, separators and wildcard runs"""
    b = _Builder(1003, 20)
    b.add(b.letters(40))
    for d in (10, 11, 15, 16, 23, 24, 31, 37, 47, 48):
        b.pair(d, "letter", 100)
    b.add([SEPARATOR])
    b.add(b.letters(30))
    b.add([WILDCARD] * 5)
    for d in (12, 16, 33):
        b.pair(d, "specials", 100)
    b.add([SEPARATOR, SEPARATOR])
    for d in (13, 30):
        b.pair(d, "special", 100)
    b.add([WILDCARD] * 3)
    b.add(b.letters(25))
    return b.enc(), 20, b.pairs


E_TEXTS = [(d, BACK - 1) for d in range(7, 16)] + [(9, BACK), (15, BACK), (12, BACK + 1)]


def _text_e(d, m):
    """the borders of the sequence: a short pair whose X starts at position 0, 1 or
    2 (mismatch in byte d of the first piece), and a long pair whose Y is cut off by
    the end of the text m symbols behind the start of the piece that holds its
    mismatch (byte d of that piece): whole words are loaded from m = 20 on"""
    b = _Builder(3000 + 32 * m + d, 4)
    b.add(b.letters(d % 3))
    b.pair(d, "letter", 60, lead=False)
    b.add([WILDCARD])
    b.add(b.letters(200))
    off = LONG + PIECE + d
    b.pair(off, "letter", off + 40, y_len=off - d + m)
    return b.enc(), 4, b.pairs


def _text_f():
    """position 0 is the position p of a row: the text starts with the larger
    suffix of a pair.  Its range starts at 0 because nothing stands in front of it."""
    b = _Builder(1007, 4)
    b.pair(37, "letter", 100, lead=False, flip=True)
    b.add([WILDCARD])
    b.add(b.letters(300))
    return b.enc(), 4, b.pairs


D_BLOCK, D_COPIES = LONG + 1, 2100


def _text_d():
    """B w B w ... B w: every copy's start but the first has a range (b) of 513
    symbols, more positions than the work list's kernel has workgroups"""
    blk = np.append(np.random.default_rng(1004).integers(0, 4, D_BLOCK, dtype=np.uint8), WILDCARD)
    return np.tile(blk, D_COPIES).astype(np.uint8), 4, []


CASE_TEXTS = ["A", "B", "C"] + ["E:%d:%d" % dm for dm in E_TEXTS] + ["F"]


@functools.lru_cache(maxsize=None)
def text(name):
    """a text with the oracle's tables (shared, never written to), the true LCP
    values, the inverse of the suffix table and the start s of every row's range"""
    builder = {"A": _text_a, "B": _text_b, "C": _text_c, "D": _text_d, "F": _text_f}.get(name)
    if builder is None:
        kind, d, m = name.split(":")
        assert kind == "E", name
        builder = functools.partial(_text_e, int(d), int(m))
    enc, sigma, pairs = builder()
    ora = ou.esa(enc, sigma)
    for a in (enc, ora["suf"], ora["lcp"], ora["llv"], ora["bwt"], ora["lcpfull"]):
        a.setflags(write=False)
    n = enc.size
    suf = ora["suf"].astype(np.int64)
    true = ora["lcpfull"].astype(np.int64)
    rank = np.empty(n + 1, dtype=np.int64)
    rank[suf] = np.arange(n + 1)
    plcp = np.where(rank >= 1, true[rank], 0)
    s_of_pos = np.zeros(n + 1, dtype=np.int64)
    s_of_pos[1:] = np.maximum(plcp[:-1] - 1, 0)
    assert first_suf_failure(enc, ora["suf"])[0] == check.CRIT_NONE
    return Text(name, enc, sigma, ora, true, suf, rank, s_of_pos[suf], tuple(pairs))


def _sym(t, i):
    return int(t.enc[i]) if i < t.enc.size else 255


def _a_holds(t, p, q, claim):
    va, vb = _sym(t, p + claim), _sym(t, q + claim)
    return va != vb or va >= 254


def pair_rows(t):
    """the rows of the planted pairs: the row of the larger suffix (Y, unless the
    pair was flipped), with the smaller one in front of it"""
    rows = []
    for qs, ps, off, _ in t.pairs:
        r = int(t.rank[ps])
        assert r >= 1 and t.suf[r - 1] == qs and t.true[r] == off and t.s[r] == 0, (t.name, qs, ps, off)
        rows.append(r)
    return rows


def _model(t, r, claim):
    """which code of phase 5 meets the mismatch of (r, claim)"""
    n = t.enc.size
    p, q, true, s = int(t.suf[r]), int(t.suf[r - 1]), int(t.true[r]), int(t.s[r])
    assert s <= true
    ln, off = claim - s, true - s
    va, vb = _sym(t, p + true), _sym(t, q + true)
    ends = "end" if max(p, q) + true >= n else "specials" if va >= 254 and vb >= 254 else \
        "special" if max(va, vb) >= 254 else "letter"
    assert ends != "letter" or va != vb
    in_llv = true >= 255
    past_n = max(p, q) + claim > n
    if claim < true:                      # (a) fails: no symbol of (b) matters
        return Case(t.name, r, claim, true, s, ln, off, p, q, True, None, None, None, None, None, None,
                    None, None, ends, None, None, past_n, in_llv)
    assert _a_holds(t, p, q, claim)
    o = s + off // PIECE * PIECE                         # the piece that holds the mismatch
    cnt = min(PIECE, claim - o)
    front, back = min(p, q) + o < FRONT, max(p, q) + o + BACK > n
    word = cnt >= WORD_MIN and not front and not back
    return Case(t.name, r, claim, true, s, ln, off, p, q, False, "list" if ln > LONG else "lane",
                "word" if word else "byte", off % PIECE, o + PIECE >= claim, (p + o) % 4, (q + o) % 4,
                front, back, ends, off // STEP, off % STEP // PIECE, past_n, in_llv)


def _claims_for(t, r, ks):
    n = t.enc.size
    p, q, true = int(t.suf[r]), int(t.suf[r - 1]), int(t.true[r])
    out = []

    def admit(c):
        return 0 <= c <= n and c != true and (c < 255) == (true < 255) and c not in out
    for k in ks:
        if admit(true + k) and _a_holds(t, p, q, true + k):
            out.append(true + k)
    past = n - max(p, q) + 1              # the later suffix ends in front of the claim
    if past - true <= 1000 and past > true and admit(past):
        out.append(past)
    for c in (0, true // 2, true - 2):
        if c < true and admit(c):
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def cases(name):
    t = text(name)
    out = []
    for r in pair_rows(t):
        # (B: the claims LONG ... LONG + 2 where they lie above the true value, and 600 more)
        out += [_model(t, r, c) for c in _claims_for(t, r, KS + ((3, 600) if name == "B" else ()))]
    if name == "A":
        # a mismatch in bytes 0 ... 8 of the first piece under the word branch: planting
        # does not make such suffixes neighbours, the text's own rows do
        for off in range(9):
            for r in range(1, t.suf.size):
                ln = [c - int(t.s[r]) for c in _claims_for(t, r, range(WORD_MIN, 40)) if c > t.true[r]]
                if t.true[r] - t.s[r] == off and ln and min(t.suf[r], t.suf[r - 1]) >= FRONT and \
                        max(t.suf[r], t.suf[r - 1]) + 100 < t.enc.size:
                    out.append(_model(t, r, int(t.s[r]) + min(v for v in ln if v >= WORD_MIN)))
                    assert out[-1].branch == "word" and out[-1].off == off and out[-1].len >= WORD_MIN
                    break
            else:
                raise AssertionError("no row of text A with off = %d" % off)
    assert len({(c.r, c.claim) for c in out}) == len(out)
    return tuple(out)


def all_cases():
    return [c for name in CASE_TEXTS for c in cases(name)]


def damaged(case):
    """(lcp, llv) of the case's text with the claim written in, and criteria 1
    to 4 asserted (the suffix table is the oracle's: text())"""
    t = text(case.text)
    lcp, llv = t.ora["lcp"], t.ora["llv"]
    if case.in_llv:
        assert case.claim >= 255
        llv = llv.copy()
        j = int(np.searchsorted(llv[:, 0], case.r))
        assert llv[j, 0] == case.r and llv[j, 1] == case.true
        llv[j, 1] = case.claim
    else:
        assert case.claim < 255 and lcp[case.r] == case.true
        lcp = lcp.copy()
        lcp[case.r] = case.claim
    assert_structure(t.enc, lcp, llv)
    return lcp, llv


def assert_structure(enc, lcp, llv):
    """criterion 4 of include/gtamd_check.h"""
    n = enc.size
    idx, val = llv[:, 0].astype(np.int64), llv[:, 1].astype(np.int64)
    assert lcp[0] == 0 and lcp.size == n + 1
    assert (np.diff(idx) > 0).all() and (idx >= 1).all() and (idx <= n).all()
    assert (lcp[idx] == 255).all() and np.count_nonzero(lcp == 255) == idx.size
    assert (val >= 255).all() and (val <= n).all()


# ---- what the cases cover -------------------------------------------------------------

def coverage(cs):
    """the classes of the kernel's code the cases reach, each with its count"""
    seen = {}

    def add(*key):
        seen[key] = seen.get(key, 0) + 1
    for c in cs:
        add("table", "llv" if c.in_llv else "lcp")
        if c.below:
            add("below")
            continue
        add("branch", c.path, c.branch, c.byte)
        if c.branch == "word":
            add("align", c.ma, c.mb)
            add("ends", c.ends)
        if c.path == "list":
            add("step", c.step)
            add("lane", c.lane)
        if not c.piece_last:
            add("piece not last")
        if c.past_n:
            add("past n")
        if c.p == 0 and c.off >= 2:
            add("position 0")
        if c.front:
            add("front")
        if c.back:
            add("back")
    return seen


def required_classes():
    want = [("branch", path, branch, byte) for path in ("lane", "list") for branch in ("word", "byte")
            for byte in range(PIECE)]
    want += [("align", ma, mb) for ma in range(4) for mb in range(4)]
    want += [("ends", e) for e in ("letter", "specials", "special")]
    want += [("step", k) for k in range(3)] + [("lane", 0), ("lane", LANES - 1)]
    want += [("piece not last",), ("past n",), ("table", "lcp"), ("table", "llv"), ("below",),
             ("front",), ("back",), ("position 0",)]
    return want


def assert_coverage():
    """no class is waived: a text that cannot fill one has to change"""
    seen = coverage(all_cases())
    missing = [k for k in required_classes() if not seen.get(k)]
    assert not missing, missing
    t = text("C")
    assert any((t.enc[qs:qs + off] == t.sigma - 1).any() for qs, _, off, _ in t.pairs)   # code 19 compared
    return seen


# ---- more than one damage ---------------------------------------------------------------

def write_claims(t, damages):
    """(lcp, llv) with several (r, claim) written in; a claim may cross 255"""
    C = t.true.copy()
    for r, c in damages:
        C[r] = c
    lcp = np.minimum(C, 255).astype(np.uint8)
    idx = np.flatnonzero(C >= 255)
    llv = np.stack([idx, C[idx]], axis=1).astype(np.uint64).reshape(-1, 2)
    assert_structure(t.enc, lcp, llv)
    return lcp, llv


def double_damages():
    """tables of text A with two damaged rows: far apart; position p - 1 too large
    and p wrong; p - 1 too small and p too large"""
    t = text("A")
    rows = pair_rows(t)
    out = []
    up = {r: next(c for c in _claims_for(t, r, (16, 17, 8, 9)) if c > t.true[r]) for r in rows}
    for a, b in ((3, 40), (40, 3), (10, 11), (55, 20)):
        out.append(("far apart", [(rows[a], up[rows[a]]), (rows[b], up[rows[b]])]))
        out.append(("far apart, one too small", [(rows[a], int(t.true[rows[a]]) - 2), (rows[b], up[rows[b]])]))
    for i in (5, 17, 33, 50):
        r = rows[i]
        r1 = int(t.rank[t.suf[r] + 1])                     # the row of position p, p - 1 the planted Y
        assert r1 >= 1 and t.true[r1] == t.true[r] - 1
        out.append(("p - 1 too large, p too large", [(r, up[r]), (r1, int(t.true[r1]) + 1)]))
        out.append(("p - 1 too large, p too small", [(r, up[r]), (r1, int(t.true[r1]) - 2)]))
        out.append(("p - 1 too small, p too large", [(r, int(t.true[r]) - 2), (r1, int(t.true[r1]) + 8)]))
    return out


def listed_positions(t, lcp, llv):
    """how many positions phase 5 sends to the work list (long_claims): (a) holds
    and the range [s, C) is longer than LONG, by the claims"""
    n = t.enc.size
    C = claims(lcp, llv)
    has = t.rank >= 1
    row = np.maximum(t.rank, 1)
    Cp = np.where(has, C[row], 0)
    s = np.zeros(n + 1, dtype=np.int64)
    s[1:] = np.maximum(Cp[:-1] - 1, 0)
    sym = np.concatenate([t.enc, np.full(n + 2, 255, dtype=np.uint8)])
    p = np.arange(n + 1)
    va, vb = sym[p + Cp], sym[t.suf[row - 1] + Cp]
    return int(np.count_nonzero(has & ((va != vb) | (va >= 254)) & (Cp - s > LONG)))


def overflow_rows(count):
    """`count` rows of text A that can claim true + 600 with (a) holding there, no
    two at neighbouring positions (a large claim at p - 1 empties the range of p)"""
    t = text("A")
    n = t.enc.size
    taken, rows = set(), []
    for r in range(1, n + 1):
        p, q, c = int(t.suf[r]), int(t.suf[r - 1]), int(t.true[r]) + 600
        if c <= n and _a_holds(t, p, q, c) and not {p - 1, p, p + 1} & taken:
            taken.add(p)
            rows.append(r)
            if len(rows) == count:
                return rows
    raise AssertionError("text A has %d such rows, not %d" % (len(rows), count))


def list_overflow(rows):
    """(lcp, llv) of text A with those rows claiming true + 600: every one of
    their positions is sent to the work list, and the text has none of its own"""
    t = text("A")
    lcp, llv = write_claims(t, [(r, int(t.true[r]) + 600) for r in rows])
    assert listed_positions(t, t.ora["lcp"], t.ora["llv"]) == 0
    assert listed_positions(t, lcp, llv) == len(rows)
    return lcp, llv


def list_cap(t):
    """positions the work list of phase 5 holds (esa_check.hip, run_phases)"""
    return 2 * (t.enc.size + 1) // LONG + 1


# ---- text D ---------------------------------------------------------------------------------

D_CLAIM = 2 * D_BLOCK + 1        # both suffixes hold the wildcard of the next copy there, or the end


def d_rows():
    """(rows whose position is listed, index of each row's .llv pair)"""
    t = text("D")
    rows = np.flatnonzero((t.true == D_BLOCK) & (t.suf % (D_BLOCK + 1) == 0))
    assert rows.size == D_COPIES - 1 > 2048 and (t.s[rows] == 0).all()
    assert listed_positions(t, t.ora["lcp"], t.ora["llv"]) == rows.size
    assert (np.maximum(t.true[t.rank[1:]] - t.s[t.rank[1:]], 0)).sum() + t.true[t.rank[0]] <= 2 * (t.enc.size + 1)
    assert 2 * (t.enc.size + 1) // LONG + 1 > 2048
    llv = t.ora["llv"]
    entry = np.searchsorted(llv[:, 0], rows)
    assert (llv[entry, 0] == rows).all() and (llv[entry, 1] == D_BLOCK).all() and D_CLAIM <= t.enc.size
    for r in rows[[0, 1, -1]]:
        assert _a_holds(t, int(t.suf[r]), int(t.suf[r - 1]), D_CLAIM)
    return rows, entry


# ---- order damage ------------------------------------------------------------------------------

def order_text(name):
    """(enc, the oracle's suffix table) of the two 300-symbol texts"""
    if name == "specials:300":
        from test_check_gpu import _sequence as seq
        enc, sigma = seq(name)
    else:
        assert name == "protein:300"
        rng = np.random.default_rng(1005)
        enc, sigma = rng.integers(0, 20, 300, dtype=np.uint8), 20
        enc[[40, 41, 42, 150, 151]] = WILDCARD
        enc[[0, 99, 100, 222]] = SEPARATOR
    return enc, ou.esa(enc, sigma)["suf"]


@functools.lru_cache(maxsize=None)
def order_swaps(name):
    """(enc, suf, pairs of rows to swap): every pair of neighbours, 100 seeded
    pairs of distant rows"""
    enc, suf = order_text(name)
    N = suf.size
    rng = np.random.default_rng(1006)
    far = set()
    while len(far) < 100:
        i, j = sorted(int(v) for v in rng.integers(0, N, 2))
        if j - i > 1:
            far.add((i, j))
    enc.setflags(write=False)
    suf.setflags(write=False)
    return enc, suf, [(i - 1, i) for i in range(1, N)] + sorted(far)


def order_classes(names=("specials:300", "protein:300")):
    """what decides the order at the reported index, over all swaps"""
    seen = set()
    for name in names:
        enc, suf0, swaps = order_swaps(name)
        n = enc.size
        for i, j in swaps:
            suf = suf0.copy()
            suf[[i, j]] = suf0[[j, i]]
            crit, at = first_suf_failure(enc, suf)
            assert crit == check.CRIT_ORDER
            a, b = int(suf[at - 1]), int(suf[at])
            sa, sb = (int(enc[v]) if v < n else 255 for v in (a, b))
            if sa >= 254 and sb >= 254:
                seen.add("two specials")
            elif sa >= 254 or sb >= 254:
                seen.add("a letter against a special")
            elif sa == sb and n in (a + 1, b + 1):
                seen.add("decided at a + 1 = n")
            elif sa == sb:
                seen.add("decided by the ranks")
            else:
                seen.add("two letters")
    return seen
