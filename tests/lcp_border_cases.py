"""Texts that aim the tie paths of the engine (genometools_amd/csrc/esa_engine.hip) at
the borders of their arithmetic: DIRECT_MAX_LCP = 250, DIRECT_MAX_GROUP = 16,
direct_limit() = 4096, GTAMD_LCPOVERFLOW = 255, Key<2>::KNOWN = 20 / Key<5>::KNOWN = 8,
the window steps of lcp_extend (32 symbols, 11 for the 5-bit alphabets) and of
lcp_extend_long (4 x 32), its no-shift branches, the diagonal shortcut of
k_pair_resolve, the Kasai step of k_lcp_chunks and the chunk starts of both.

A text is a random BACKGROUND (checked here: no KNOWN-mer occurs twice in it) with
PROBES planted in it.  A probe is k copies of a random block; every copy has a chosen
start alignment mod 64, three symbols in front that spell the copy's number (so no two
copies match to the left for more than two symbols), a chosen length (a copy may be a
prefix of the block), a terminator (a letter, a wildcard, a separator or the end of
the text), optionally one substituted symbol or wildcard inside, and optionally a tail
behind the terminator.  What a probe is made of says, without looking at any table,
the LCP and the order of every two of its copies at every offset: by_construction().

The MODEL says which path of the engine settles which entry.  Its input is the
oracle's suffix table and LCP values (tests/oracle_util.py), never the engine's.

  Tie rule (k_tiebits; esa_msd.h msd_emit_quad for the MSD sort).  Entry i is tied
  with entry i - 1 when
    DNA, either first sort:  both suffixes have 20 letters in front of their first
        special and share them, which is  lcpfull[i] >= 20  (specials never match, so
        an LCP of 20 says both have 20 letters);
    5-bit alphabets, LSD sort (Key<5>: 10 symbols):  lcpfull[i] >= 10;
    5-bit alphabets, MSD sort (FMT 1: 8 symbols and the class s >> 1 of the ninth,
        "nine letters or more"):  lcpfull[i] >= 8, both ninth symbols are letters and
        their classes agree.
  A tie group is a maximal run of tied entries with the entry in front of it.

  Figures of the engine's "ties" line (count_left): tied = tied entries; pairs =
  groups of two; small groups = groups of three or four (none when their 3 or 6
  records each exceed an eighth of the table); entries settled = members of the small
  groups; left = members (heads included) of all other groups.  m0 of
  settle_few_ties / settle_few_left counts members, heads included.

  The direct path gives up on a list when a group has more than 16 members or a
  compared pair has LCP >= 250.  Insertion sort compares every two suffixes that end
  up next to each other, and an LCP of two members is the minimum of the entries
  between them: so it gives up exactly when some tied entry of the list has
  lcpfull >= 250.

  Record list of k_pair_resolve: (a, b) = (smaller, larger position) of every pair, then
  of the members (0,1) (0,2) (1,2) (0,3) (1,3) (2,3) of every small group in position
  order; sorted by a (stable).  A thread takes `chunk` consecutive records and keeps the
  last four: a record on the diagonal of one of them (b - b' = a - a' = d) with
  l' >= KNOWN + d takes l' - d; every other record is FRESH: lcp_extend_long from
  P = a + KNOWN, Q = b + KNOWN.  k_lcp_chunks: the tied entries of what the pair path
  left, sorted by position p, 32 per thread, every one compared with its predecessor q
  from KNOWN or from l' - (p - p') when that is more.

Helper module, not a conftest; no GPU."""
import itertools

import numpy as np

import oracle_util as ou

WILD, SEP, END = 254, 255, 256       # END: by_construction's code for "the text ends here"
KNOWN = {4: 20, 20: 8}
DIRECT_MAX_LCP, DIRECT_MAX_GROUP, DIRECT_LIMIT = 250, 16, 4096
LCPOVERFLOW, LCP_CHUNK, PR_LINE = 255, 32, 16

DNA_LENGTHS = (20, 21, 51, 52, 53, 83, 84, 85, 147, 148, 149, 249, 250, 251, 254, 255, 256,
               275, 276, 277, 1000)
# (beyond the issue's list: window 3 of the first step at offset 0, window 1 of a later step)
DNA_EXTRA_LENGTHS = (116, 180)
PROTEIN_LENGTHS = (8, 9, 18, 19, 20, 30, 249, 250, 254, 255, 256)
GROUP_SIZES = (2, 3, 4, 5, 6, 16, 17)


# ---------------------------------------------------------------------------------
# background
# ---------------------------------------------------------------------------------
def has_repeated_kmer(enc, k, sigma):
    """whether some k-mer of letters occurs twice in `enc` (letters only)"""
    enc = np.asarray(enc, dtype=np.uint64)
    if enc.size < k + 1:
        return False
    bits = 2 if sigma <= 4 else 5
    code = np.zeros(enc.size - k + 1, dtype=np.uint64)
    for j in range(k):
        code = (code << np.uint64(bits)) | enc[j:enc.size - k + 1 + j]
    return np.unique(code).size != code.size


def background(sigma, size, seed, letters=None):
    """uniform letters; the first seed from `seed` on whose text holds no KNOWN-mer
    twice (returns the text and the seed that passed)"""
    letters = sigma if letters is None else letters
    for s in range(seed, seed + 64):
        bg = np.random.default_rng(s).integers(0, letters, size, dtype=np.uint8)
        if not has_repeated_kmer(bg, KNOWN[sigma], sigma):
            return bg, s
    raise AssertionError("no seed without a repeated %d-mer" % KNOWN[sigma])


# ---------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------
class Copy:
    """one copy of a probe's block: `length` symbols of it (None: all), start at
    `align` mod 64 (None: wherever), terminator `term` (a letter, WILD, SEP or END), one
    symbol `sub` = (offset, symbol) replaced, `tail` symbols behind the terminator"""

    def __init__(self, term, length=None, align=None, sub=None, tail=()):
        self.term, self.length, self.align, self.sub, self.tail = term, length, align, sub, tuple(tail)
        self.start = None

    def described(self, block):
        """the symbols this copy is made of, terminator included"""
        s = np.append(block[:self.length].astype(np.int64), self.term)
        if self.sub is not None:
            s[self.sub[0]] = self.sub[1]
        return s


class Text:
    """background stream + probes -> encoded symbols"""

    def __init__(self, name, sigma, size, seed, letters=None, gap=28):
        self.name, self.sigma, self.gap = name, sigma, gap
        self.bg, self.seed = background(sigma, size, seed, letters)
        self.rng = np.random.default_rng(1000 + seed)
        self.used, self.out, self.n, self.probes, self.closed = 0, [], 0, [], False

    def _fill(self, k):
        assert self.used + k <= self.bg.size, "%s: background used up" % self.name
        self.out.append(self.bg[self.used:self.used + k])
        self.used += k
        self.n += k

    def block(self, length, letters=None):
        return self.rng.integers(0, self.sigma if letters is None else letters, length, dtype=np.uint8)

    def place(self, block, c, number, lead=0):
        """copy `c`, the number-th of its probe, behind `lead` + gap symbols of background
        (and what its alignment asks for)"""
        assert not self.closed
        lead += self.gap
        if c.align is not None:
            lead += (c.align - (self.n + lead + 3)) % 64
        self._fill(lead)
        # (the symbol right in front of the copy differs among sigma copies in a row)
        mark = [(number // self.sigma ** 2) % self.sigma, (number // self.sigma) % self.sigma,
                number % self.sigma]
        c.start = self.n + 3
        assert c.align is None or c.start % 64 == c.align
        syms = mark + [int(x) for x in c.described(block) if x != END] + list(c.tail)
        self.out.append(np.array(syms, dtype=np.uint8))
        self.n += len(syms)
        if c.term == END:
            assert not c.tail
            self.closed = True

    def probe(self, block, copies):
        block = np.asarray(block, dtype=np.uint8)
        for number, c in enumerate(copies):
            if c.start is None:
                self.place(block, c, number)
        self.probes.append((block, list(copies)))

    def finish(self, rest=None):
        """the rest of the background (or `rest` symbols of it) behind the last probe"""
        if not self.closed:
            self._fill(self.bg.size - self.used if rest is None else rest)
        self.enc = np.concatenate(self.out).astype(np.uint8)
        assert self.enc.size == self.n
        return self


def _pair_from_descriptions(sa, sb):
    """per offset o: (LCP of the two copies' suffixes at o, whether the first copy's is
    the smaller one), from what the copies are made of.  Specials never match, a special
    is larger than a letter, two specials (the end of the text is one) order by position,
    and the first copy stands first in the text."""
    m = min(sa.size, sb.size)
    a, b = sa[:m], sb[:m]
    brk = (a != b) | (a >= WILD) | (b >= WILD)
    assert brk.any(), "the two copies do not differ inside what describes them"
    idx = np.where(brk, np.arange(m), m)
    nxt = np.minimum.accumulate(idx[::-1])[::-1]          # first break at or behind o
    o = np.flatnonzero(nxt < m)
    t = nxt[o]
    xa, xb = a[t], b[t]
    first = np.where((xa >= WILD) & (xb >= WILD), True, np.where(xa >= WILD, False,
                                                                 np.where(xb >= WILD, True, xa < xb)))
    return o, t - o, first


def by_construction(text, min_lcp=None):
    """(a, b, lcp, a_smaller) arrays with a < b: every two copies of every probe at every
    offset where they share at least `min_lcp` (default: KNOWN) symbols"""
    min_lcp = KNOWN[text.sigma] if min_lcp is None else min_lcp
    A, B, L, F = [], [], [], []
    for block, copies in text.probes:
        desc = [c.described(block) for c in copies]
        for i, j in itertools.combinations(range(len(copies)), 2):
            o, l, first = _pair_from_descriptions(desc[i], desc[j])
            keep = l >= min_lcp
            A.append(copies[i].start + o[keep])
            B.append(copies[j].start + o[keep])
            L.append(l[keep])
            F.append(first[keep])
    return tuple(np.concatenate(x) for x in (A, B, L, F))


# ---------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------
class Rmq:
    """range minimum over a fixed array (sparse table)"""

    def __init__(self, v):
        self.lv = [np.asarray(v, dtype=np.int64)]
        k = 1
        while 2 * k <= self.lv[0].size:
            p = self.lv[-1]
            self.lv.append(np.minimum(p[:-k], p[k:]))
            k *= 2

    def query(self, lo, hi):
        """min v[lo .. hi] (inclusive), arrays"""
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        j = np.floor(np.log2(np.maximum(hi - lo + 1, 1))).astype(np.int64)
        out = np.empty(lo.shape, dtype=np.int64)
        for lev in np.unique(j):
            s = j == lev
            t = self.lv[lev]
            out[s] = np.minimum(t[lo[s]], t[hi[s] - (1 << lev) + 1])
        return out


def lcpfull_of(lcp, llv):
    """the full LCP values of a byte table and its .llv pairs"""
    full = np.asarray(lcp).astype(np.uint64)
    llv = np.asarray(llv).reshape(-1, 2)
    full[llv[:, 0].astype(np.int64)] = llv[:, 1]
    return full


class Tables:
    """rank and pairwise LCP from a suffix table and full LCP values"""

    def __init__(self, suf, lcpfull):
        self.suf = np.asarray(suf).astype(np.int64)
        self.lcpfull = np.asarray(lcpfull).astype(np.int64)
        self.rank = np.empty(self.suf.size, dtype=np.int64)
        self.rank[self.suf] = np.arange(self.suf.size)
        self.rmq = Rmq(self.lcpfull)

    def pair(self, a, b):
        """(LCP of suffixes a and b, whether a is the smaller suffix)"""
        ra, rb = self.rank[np.asarray(a)], self.rank[np.asarray(b)]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        return self.rmq.query(lo + 1, hi), ra < rb


def check_by_construction(text, suf, lcpfull):
    """every (a, b, LCP, order) the probes imply, in the given tables; every probe's
    copies (their starts) stand together in the table"""
    tab = Tables(suf, lcpfull)
    a, b, l, first = by_construction(text)
    got_l, got_first = tab.pair(a, b)
    bad = np.flatnonzero((got_l != l) | (got_first != first))
    assert bad.size == 0, "%s: suffixes %d and %d: LCP %d, first smaller %s; by construction %d, %s" % (
        text.name, a[bad[0]], b[bad[0]], got_l[bad[0]], got_first[bad[0]], l[bad[0]], first[bad[0]])
    for block, copies in text.probes:
        r = np.sort(tab.rank[[c.start for c in copies]])
        assert r[-1] - r[0] == len(copies) - 1, "%s: a foreign suffix among the copies at %d" % (
            text.name, copies[0].start)
    return a.size


# ---------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------
def tied_entries(enc, sigma, suf, lcpfull, msd=False):
    """bool per entry: tied with its predecessor after the first sort (rule: above)"""
    lcpfull = np.asarray(lcpfull).astype(np.int64)
    if sigma <= 4:
        t = lcpfull >= 20
    elif not msd:
        t = lcpfull >= 10
    else:
        suf = np.asarray(suf).astype(np.int64)
        ext = np.append(np.asarray(enc), [SEP] * 16)          # (the end of the text is a special)
        ninth = ext[np.minimum(suf + 8, ext.size - 1)]
        t = np.zeros(suf.size, dtype=bool)
        t[1:] = (lcpfull[1:] >= 8) & (ninth[1:] < WILD) & (ninth[:-1] < WILD) & \
                ((ninth[1:] >> 1) == (ninth[:-1] >> 1))
    t = t.copy()
    t[0] = False
    return t


def groups_of(t):
    """(head index, size) of every tie group"""
    t = np.asarray(t, dtype=bool)
    nxt = np.append(t[1:], False)
    heads = np.flatnonzero(~t & nxt)
    ends = np.flatnonzero(t & ~nxt)
    return heads, ends - heads + 1


def _gives_up(sizes, heads, lcpfull):
    """the direct path on a list of groups"""
    if sizes.size == 0:
        return False
    if sizes.max() > DIRECT_MAX_GROUP:
        return True
    return any(lcpfull[h + 1:h + g].max() >= DIRECT_MAX_LCP for h, g in zip(heads, sizes))


def predict(enc, sigma, ora, msd=False, no_pairs=False, no_small=False, pair_chunk=0, dist=False,
            slices=None):
    """what a build does with the ties of `enc`: see the module text.  Keys: direct (the
    list of direct_ties() calls as engine_paths reads them), ties (the five figures, None
    when the direct path settles the build), pair_resolve (records and chunk, None
    without a record), rounds (bool).
    dist: the part machinery (GTAMD_FORCE_WIDE, a build in parts): settle_few_left is
    skipped, what is left goes through the rounds.
    slices: (first entry, entries) of every part of a build in parts.  A tie group lies in
    one part (its members share the key the parts are cut by); the figures are summed
    over the parts, the small groups' limit of an eighth of the table holds part by part,
    records / chunk and the direct calls are per part and not predicted (direct: None)."""
    lcpfull = np.asarray(ora["lcpfull"]).astype(np.int64)
    t = tied_entries(enc, sigma, ora["suf"], lcpfull, msd)
    heads, sizes = groups_of(t)
    parts = slices is not None and len(slices) > 1
    dist = dist or parts
    slices = [(0, enc.size + 1)] if slices is None else sorted(slices)
    out = {"tied": int(t.sum()), "members": int(sizes.sum()), "direct": None if parts else [], "ties": None,
           "pair_resolve": None, "rounds": False, "heads": heads, "sizes": sizes}
    if heads.size == 0:
        return out
    part = np.searchsorted(np.array([off for off, _ in slices]), heads, side="right") - 1
    per_part = np.bincount(part, weights=sizes, minlength=len(slices))
    gaveup = True
    if per_part.max() <= DIRECT_LIMIT:                      # (every part's list is short: all try)
        gaveup = _gives_up(sizes, heads, lcpfull)
        if not parts:
            out["direct"].append({"call": "first", "tied": out["members"], "gaveup": int(gaveup)})
    if not gaveup:
        return out
    pair = (sizes == 2) & (not no_pairs)
    small = ((sizes == 3) | (sizes == 4)) & (not no_pairs) & (not no_small)
    nsrec = 0
    for r, (off, cnt) in enumerate(slices):
        mine = small & (part == r)
        rec = int(np.where(sizes[mine] == 3, 3, 6).sum())
        if rec > cnt // 8:                                  # (nsrec > NL / 8)
            small &= part != r
        else:
            nsrec += rec
    left = ~pair & ~small
    nrec = int(pair.sum()) + nsrec
    out["ties"] = {"tied": out["tied"], "pairs": int(pair.sum()), "small_groups": int(small.sum()),
                   "settled": int(sizes[small].sum()), "left": int(sizes[left].sum())}
    out["is_pair"], out["is_small"], out["is_left"] = pair, small, left
    if nrec > 0 and not parts:
        chunk = pair_chunk if pair_chunk > 0 else 16        # (nrec >> 20 < 16 at these sizes)
        out["pair_resolve"] = {"records": nrec, "chunk": (chunk + PR_LINE - 1) // PR_LINE * PR_LINE}
    nleft = out["ties"]["left"]
    if nleft > 0:
        gaveup = dist or nleft > DIRECT_LIMIT
        if not gaveup:
            gaveup = _gives_up(sizes[left], heads[left], lcpfull)
            out["direct"].append({"call": "left", "tied": nleft, "gaveup": int(gaveup)})
        out["rounds"] = bool(gaveup)
    return out


def _stored(enc):
    """the 2-bit codes of the packed text: a wildcard is stored as 0, a separator as 1,
    0 behind the text"""
    s = np.asarray(enc).astype(np.int64)
    s = np.where(s == WILD, 0, np.where(s == SEP, 1, s))
    return np.append(s, np.zeros(192, dtype=np.int64))


def _special(enc):
    s = np.asarray(enc) >= WILD
    return np.append(np.append(s, True), np.zeros(191, dtype=bool))    # (bit n: the end)


def _window_classes(kind, enc, stored, special, x, y, start, l, decides=True):
    """classes of one comparison lcp_extend_long(x, y, start) that ends with LCP l"""
    P, Q, rel = x + start, y + start, l - start
    cl = {"%s:P%%32%s" % (kind, "=0" if P % 32 == 0 else "!=0"), "%s:Q%%32%s" % (kind, "=0" if Q % 32 == 0 else "!=0"),
          "%s:P%%64%s" % (kind, "=0" if P % 64 == 0 else "!=0"), "%s:Q%%64%s" % (kind, "=0" if Q % 64 == 0 else "!=0"),
          "%s:window%d,%s" % (kind, rel % 128 // 32, "first step" if rel < 128 else "later step")}
    if rel % 32 in (0, 1, 31):
        cl.add("%s:offset%d" % (kind, rel % 32))
    if not decides:
        return cl
    n = np.asarray(enc).size
    sx, sy = bool(special[x + l]), bool(special[y + l])
    if y + l == n or x + l == n:
        cl.add("decides:end of text")
    elif sx and sy:
        cl.add("decides:specials on both sides")
    elif sx or sy:
        cl.add("decides:special on the %s side" % ("smaller-position" if sx == (x < y) else "other"))
        mine, other = (x, y) if sx else (y, x)
        if not special[other + l] and stored[mine + l] == stored[other + l]:
            cl.add("decides:%s against %s" % (("wildcard", "A") if enc[mine + l] == WILD else ("separator", "C")))
    else:
        cl.add("decides:two letters")
    if sx or sy:
        cl.add("decides:special in the %s half of the bitmap window" % ("odd" if rel % 128 // 32 & 1 else "even"))
    w0 = rel - rel % 32                                     # the deciding window, 32 symbols
    dx, dy = stored[x + start + w0:x + start + w0 + 32], stored[y + start + w0:y + start + w0 + 32]
    sp = special[x + start + w0:x + start + w0 + 32] | special[y + start + w0:y + start + w0 + 32]
    m = int(np.argmax(dx != dy)) if (dx != dy).any() else 32
    ds = int(np.argmax(sp)) if sp.any() else 32
    if m < ds < 32:
        cl.add("decides:m < ds")
    if ds < m < 32:
        cl.add("decides:ds < m")
    return cl


def resolve_model(enc, sigma, ora, pred):
    """the record list of k_pair_resolve and the verdict of every record: arrays a, b, l,
    fresh (bool), chunk_start (bool), refused (a record on a held diagonal that the
    shortcut may not take); and the classes of the fresh comparisons"""
    suf = np.asarray(ora["suf"]).astype(np.int64)
    tab = Tables(suf, ora["lcpfull"])
    heads, sizes = pred["heads"], pred["sizes"]
    ra, rb = [], []
    for h in heads[pred["is_pair"]]:
        p = np.sort(suf[h:h + 2])
        ra.append(p[0]); rb.append(p[1])
    for h, g in zip(heads[pred["is_small"]], sizes[pred["is_small"]]):
        m = np.sort(suf[h:h + g])
        for x, y in ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))[:3 if g == 3 else 6]:
            ra.append(m[x]); rb.append(m[y])
    a, b = np.array(ra, dtype=np.int64), np.array(rb, dtype=np.int64)
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    l, _ = tab.pair(a, b)
    chunk, kn = pred["pair_resolve"]["chunk"], KNOWN[sigma]
    fresh = np.ones(a.size, dtype=bool)
    refused = np.zeros(a.size, dtype=bool)
    weak = False          # a refusal that rl[k] >= d alone would not have made
    for s in range(a.size):
        for k in range(1, min(4, s % chunk) + 1):
            d = a[s] - a[s - k]
            if b[s] >= b[s - k] and b[s] - b[s - k] == d:
                if l[s - k] >= kn + d:
                    fresh[s] = False
                    break
                refused[s] = True
                weak |= l[s - k] >= d
    classes = set()
    stored, special = _stored(enc), _special(enc)
    for s in np.flatnonzero(fresh):
        if sigma <= 4:
            classes |= _window_classes("resolve", enc, stored, special, int(a[s]), int(b[s]), kn, int(l[s]))
        else:
            rel = int(l[s]) - kn
            classes.add("resolve5:%s" % ("one window" if rel < 11 else "more windows"))
            if rel % 11 in (0, 1, 10):
                classes.add("resolve5:offset%d" % (rel % 11))
        classes.add("resolve:fresh at a chunk start" if s % chunk == 0 else "resolve:fresh inside a chunk")
    if (~fresh).any():
        classes.add("resolve:shortcut taken")
    if refused.any():
        classes.add("resolve:diagonal held, shortcut refused")
    if weak:
        classes.add("resolve:diagonal held, rl[k] >= d, shortcut refused")
    return {"a": a, "b": b, "l": l, "fresh": fresh, "chunk_start": np.arange(a.size) % chunk == 0,
            "refused": refused, "classes": classes}


def chunks_model(enc, sigma, ora, pred, slices=None):
    """k_lcp_chunks over what the pair path left; slices: (first entry, entries) of every
    part of a build in parts -- a part walks the positions of its own entries only, so
    it sees some of the positions of a repeat and p - prevp > 1"""
    suf = np.asarray(ora["suf"]).astype(np.int64)
    lcpfull = np.asarray(ora["lcpfull"]).astype(np.int64)
    idx = np.concatenate([np.arange(h + 1, h + g) for h, g in
                          zip(pred["heads"][pred["is_left"]], pred["sizes"][pred["is_left"]])] or
                         [np.zeros(0, dtype=np.int64)])
    if slices is None:
        slices = [(0, suf.size)]
    out = {"p": [], "q": [], "l": [], "classes": set()}
    for off, cnt in slices:
        mine = idx[(idx >= off) & (idx < off + cnt)]
        mine = mine[np.argsort(suf[mine], kind="stable")]
        one = _chunks_of_a_part(enc, sigma, suf[mine], suf[mine - 1], lcpfull[mine])
        for k in ("p", "q", "l"):
            out[k].append(one[k])
        out["classes"] |= one["classes"]
    for k in ("p", "q", "l"):
        out[k] = np.concatenate(out[k])
    return out


def _chunks_of_a_part(enc, sigma, p, q, l):
    kn, classes = KNOWN[sigma], set()
    stored, special = _stored(enc), _special(enc)
    for s in range(p.size):
        start = kn
        if s % LCP_CHUNK:
            d = p[s] - p[s - 1]
            classes.add("chunks:p - prevp %s" % ("= 1" if d == 1 else "> 1"))
            if l[s - 1] > kn + d:
                start = l[s - 1] - d
                classes.add("chunks:from l - (p - prevp)")
            else:
                classes.add("chunks:from KNOWN behind a record")
        else:
            classes.add("chunks:from KNOWN at a chunk start")
        if sigma <= 4:
            classes |= _window_classes("chunks", enc, stored, special, int(q[s]), int(p[s]), int(start), int(l[s]),
                                       decides=False)
        for v in (254, 255, 256):
            if l[s] == v:
                classes.add("chunks:LCP %d" % v)
    return {"p": p, "q": q, "l": l, "classes": classes}


def direct_classes(pred, lcpfull):
    """group sizes and the largest LCP the direct path settles"""
    classes = set()
    lcpfull = np.asarray(lcpfull).astype(np.int64)
    for call in pred["direct"]:
        if call["gaveup"]:
            continue
        sel = pred["is_left"] if call["call"] == "left" else np.ones(pred["sizes"].size, dtype=bool)
        for h, g in zip(pred["heads"][sel], pred["sizes"][sel]):
            classes.add("direct:group of %d" % g)
            if lcpfull[h + 1:h + g].max() == DIRECT_MAX_LCP - 1:
                classes.add("direct:LCP 249")
    return classes


# ---------------------------------------------------------------------------------
# the texts
# ---------------------------------------------------------------------------------
# start alignments (first copy, second copy) mod 64: P = start + 20 a multiple of 64, of
# 32 only, of neither -- each on either side
_ALIGN = ((44, 44), (44, 12), (12, 44), (12, 45), (45, 12), (44, 7), (7, 44), (13, 50), (12, 12))
# terminators (first copy, second copy): letters in both orders, a special on either
# side, on both sides, and the special whose stored code is the letter opposite
_TERMS = ((0, 3), (3, 0), (WILD, 2), (2, WILD), (SEP, 2), (2, SEP), (WILD, WILD), (SEP, WILD),
          (WILD, 0), (0, WILD), (SEP, 1), (1, SEP), (2, 1), (1, 2))


def _shallow_probes(t):
    """groups of 2 .. 16 with LCP <= 249: what the direct path settles (one pair with
    LCP 249 exactly)"""
    t.probe(t.block(249), [Copy(1, align=44), Copy(2, align=12)])
    t.probe(t.block(100), [Copy(3), Copy(WILD), Copy(0)])
    t.probe(t.block(52), [Copy(SEP), Copy(2), Copy(0), Copy(WILD, align=44)])
    t.probe(t.block(84), [Copy(2), Copy(WILD), Copy(SEP), Copy(0), Copy(WILD)])
    t.probe(t.block(148), [Copy(WILD), Copy(3), Copy(1), Copy(SEP), Copy(0, length=100), Copy(2)])
    t.probe(t.block(30), [Copy((WILD, SEP)[k & 1] if k >= 4 else 3 - k) for k in range(16)])


def _text_direct():
    t = Text("direct", 4, 40_000, 11)
    _shallow_probes(t)
    return t.finish()


def _text_deep_250():
    t = Text("deep_250", 4, 40_000, 11)
    _shallow_probes(t)
    t.probe(t.block(250), [Copy(0, align=44), Copy(WILD, align=45)])
    return t.finish()


def _text_group_17():
    t = Text("group_17", 4, 40_000, 11)
    _shallow_probes(t)
    t.probe(t.block(22), [Copy((WILD, SEP)[k & 1] if k >= 4 else k) for k in range(17)])
    return t.finish()


def _text_direct_count(extra):
    """pairs only, all with LCP <= 249: 4096 members of tie groups; with `extra` the last
    probe gets a third copy: 4097"""
    t = Text("direct_count_%d" % (4096 + extra), 4, 40_000, 12)
    for k in range(8):
        t.probe(t.block(249), [Copy(k & 3), Copy(WILD)])               # 230 pairs each
    t.probe(t.block(226), [Copy(SEP), Copy(1)])                        # 207 pairs
    t.probe(t.block(20), [Copy(0), Copy(1)] + ([Copy(2)] if extra else []))
    return t.finish()


def _text_pairs():
    t = Text("pairs", 4, 40_000, 13)
    t.probe(t.block(300), [Copy(0), Copy(1)])                          # the driver: no direct path
    n = 0
    for sweep in range(3):
        for L in DNA_LENGTHS + DNA_EXTRA_LENGTHS:
            if L == 1000 and sweep:
                continue
            ta, tb = _TERMS[(n + 3 * sweep) % len(_TERMS)] if sweep else _TERMS[n % 2]
            al = _ALIGN[n % len(_ALIGN)]
            tail = (WILD,) if sweep == 0 and n % 3 == 0 else ()         # a special behind the letters that decide
            t.probe(t.block(L), [Copy(ta, align=al[0], tail=tail), Copy(tb, align=al[1])])
            n += 1
    # every terminator pair once more, at a length whose decision falls into the odd half of
    # a 64-bit bitmap window (20 + 32 + 5)
    for k, (ta, tb) in enumerate(_TERMS):
        al = _ALIGN[k % len(_ALIGN)]
        t.probe(t.block(57), [Copy(ta, align=al[0]), Copy(tb, align=al[1])])
    # two matches on one diagonal, one symbol apart: a substituted letter, a wildcard
    blk = t.block(120)
    t.probe(blk, [Copy(0), Copy(1, sub=(60, (int(blk[60]) + 1) & 3))])
    t.probe(t.block(120), [Copy(2), Copy(3, sub=(50, WILD))])
    t.probe(t.block(90), [Copy(1, sub=(45, SEP)), Copy(0)])
    # the end of the text decides
    t._fill(t.bg.size - t.used - 200)
    t.probe(t.block(85), [Copy(2, align=12), Copy(END, align=44)])
    return t.finish()


def _text_small():
    t = Text("small", 4, 55_000, 14)
    t.probe(t.block(300), [Copy(0), Copy(1)])
    for n, perm in enumerate(itertools.permutations(range(3))):
        t.probe(t.block(21 + n % 3), [Copy(perm[k]) for k in range(3)])
    for n, perm in enumerate(itertools.permutations(range(4))):
        t.probe(t.block(20 + n % 4), [Copy(perm[k], align=_ALIGN[n % 9][k & 1]) for k in range(4)])
    # pairwise LCPs that differ inside one group: prefix copies
    for Ls in ((None, 20, None), (254, None, None), (None, None, 255), (255, None, 254), (20, 254, None),
               (None, 255, None, 20), (254, None, 255, None)):
        blk = t.block(300)
        # (a prefix copy ends with a letter that is not the block's next one; the full copies
        # end with a letter, a wildcard, another letter, a separator)
        full = iter((0, WILD, 2, SEP))
        t.probe(blk, [Copy((int(blk[L]) + 1) & 3, length=L) if L else Copy(next(full)) for L in Ls])
    return t.finish()


def _text_rounds():
    t = Text("rounds", 4, 40_000, 15)
    kinds = (0, WILD, 2, SEP, 3, WILD)
    for n, (k, L) in enumerate(((5, 250), (6, 254), (5, 255), (6, 256), (5, 1000), (5, 275))):
        t.probe(t.block(L), [Copy(kinds[(c + n) % 6] if c else 1, align=(7 + 13 * c + n) % 64) for c in range(k)])
    return t.finish()


def _text_last_group():
    """no special anywhere; T occurs only in the first 40 symbols of a block of 300 whose
    second copy ends the text: the largest suffixes are pairs with LCP >= 260, so the last,
    partial group of 16 table entries holds bytes of 255"""
    t = Text("last_group", 4, 40_000, 16, letters=3)
    blk = np.concatenate([t.block(40) | 2, t.block(260, letters=3)]).astype(np.uint8)
    blk[0] = 3
    one, two = Copy(0), Copy(END)
    t.place(blk, one, 0)
    lead = t.bg.size - t.used - 100
    lead += (5 - (t.n + lead + t.gap + 3 + 300 + 1)) % 16              # n + 1 = 5 mod 16
    t.place(blk, two, 1, lead=lead)
    t.probe(blk, [one, two])
    t.finish()
    assert (t.n + 1) % 16 == 5
    return t


def _text_protein():
    t = Text("protein", 20, 25_000, 17)
    for n, L in enumerate(PROTEIN_LENGTHS):
        ta, tb = ((3, 11), (12, 2), (WILD, 5), (6, SEP), (WILD, WILD))[n % 5]
        t.probe(t.block(L), [Copy(ta), Copy(tb)])
    for n, L in enumerate((9, 19, 30, 250, 256)):
        t.probe(t.block(L), [Copy((7, WILD, 2)[(k + n) % 3] if k < 2 else 13 + k) for k in range(3)])
    for L in (9, 20, 255):
        t.probe(t.block(L), [Copy((4, SEP, 9, WILD, 16)[k]) for k in range(5)])
    return t.finish()


_BUILDERS = {
    "direct": _text_direct, "direct_count_4096": lambda: _text_direct_count(0),
    "direct_count_4097": lambda: _text_direct_count(1), "deep_250": _text_deep_250,
    "group_17": _text_group_17, "pairs": _text_pairs, "small": _text_small, "rounds": _text_rounds,
    "last_group": _text_last_group, "protein": _text_protein,
}
NAMES = tuple(_BUILDERS)
_cache = {}


def text(name):
    """the Text `name`, with .enc, .ora (the oracle's tables) -- built once"""
    if name not in _cache:
        t = _BUILDERS[name]()
        t.ora = ou.esa(t.enc, t.sigma)
        _cache[name] = t
    return _cache[name]


# what the issue's table says of every text: (the first direct call gives up, records in
# the pair list, a direct call on what is left and whether it gives up, rounds)
EXPECTED_PATH = {
    "direct": dict(first=0, pair_resolve=False, left=None, rounds=False),
    "direct_count_4096": dict(first=0, pair_resolve=False, left=None, rounds=False),
    "direct_count_4097": dict(first=None, pair_resolve=True, left=None, rounds=False),
    "deep_250": dict(first=1, pair_resolve=True, left=0, rounds=False),
    "group_17": dict(first=1, pair_resolve=True, left=1, rounds=True),
    "pairs": dict(first=None, pair_resolve=True, left=None, rounds=False),
    "small": dict(first=None, pair_resolve=True, left=None, rounds=False),
    "rounds": dict(first=None, pair_resolve=True, left=None, rounds=True),
    "last_group": dict(first=1, pair_resolve=True, left=None, rounds=False),
    "protein": dict(first=None, pair_resolve=True, left=1, rounds=True),
}


def path_of(pred):
    """a prediction in the terms of EXPECTED_PATH"""
    calls = {c["call"]: c["gaveup"] for c in pred["direct"]}
    return dict(first=calls.get("first"), pair_resolve=pred["pair_resolve"] is not None,
                left=calls.get("left"), rounds=pred["rounds"])


# ---------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------
def _required():
    req = set()
    for kind in ("resolve", "chunks"):
        for x in "PQ":
            for m in (32, 64):
                req |= {"%s:%s%%%d=0" % (kind, x, m), "%s:%s%%%d!=0" % (kind, x, m)}
        for k in range(4):
            req |= {"%s:window%d,first step" % (kind, k), "%s:window%d,later step" % (kind, k)}
        req |= {"%s:offset%d" % (kind, o) for o in (0, 1, 31)}
    req |= {"decides:two letters", "decides:special on the smaller-position side",
            "decides:special on the other side", "decides:specials on both sides", "decides:end of text",
            "decides:wildcard against A", "decides:separator against C", "decides:m < ds", "decides:ds < m",
            "decides:special in the odd half of the bitmap window",
            "decides:special in the even half of the bitmap window",
            "resolve:fresh at a chunk start", "resolve:fresh inside a chunk", "resolve:shortcut taken",
            "resolve:diagonal held, shortcut refused",
            "chunks:p - prevp = 1", "chunks:p - prevp > 1", "chunks:from l - (p - prevp)",
            "chunks:from KNOWN at a chunk start", "chunks:from KNOWN behind a record",
            "chunks:LCP 254", "chunks:LCP 255", "chunks:LCP 256", "direct:LCP 249",
            "resolve5:one window", "resolve5:more windows", "resolve5:offset0", "resolve5:offset1",
            "resolve5:offset10"}
    req |= {"direct:group of %d" % g for g in GROUP_SIZES if g <= DIRECT_MAX_GROUP}
    req |= {"gives up:group of 17", "gives up:LCP 250", "gives up:more than 4096 members"}
    return req


REQUIRED = _required()

# classes the issue names that no text can reach
UNREACHABLE = {
    "resolve:diagonal held, rl[k] >= d, shortcut refused":
        "rl[k] >= KNOWN + d cannot be false for a record of the list.  Two records on one "
        "diagonal, d apart, with d < rl[k]: the later one's suffixes share exactly rl[k] - d "
        "symbols, and as a record of the list they are tied, so rl[k] - d >= KNOWN.  With "
        "d >= rl[k] (the gapped copies: the match ends, one symbol differs, the next match "
        "begins) d is at least 1 + KNOWN, more than the held LCP of the last record of the first "
        "match, which is KNOWN, so rl[k] >= d fails as well.  d = rl[k] would make the later "
        "record start at the difference itself: not tied.  The refusal is reached only by "
        "records the weaker test rl[k] >= d refuses as well; mutation 1 is equivalent.",
}


def coverage(pair_chunk=0):
    """{text name: classes reached}"""
    out = {}
    for name in NAMES:
        t = text(name)
        pred = predict(t.enc, t.sigma, t.ora, pair_chunk=pair_chunk)
        cl = set()
        if pred["direct"] and pred["direct"][0]["gaveup"]:
            if pred["sizes"].max() > DIRECT_MAX_GROUP:
                cl.add("gives up:group of 17")
            lf = np.asarray(t.ora["lcpfull"]).astype(np.int64)
            if pred["sizes"].max() <= DIRECT_MAX_GROUP and lf[tied_entries(t.enc, t.sigma, t.ora["suf"], lf)].max() \
                    == DIRECT_MAX_LCP:
                cl.add("gives up:LCP 250")
        if not pred["direct"] and pred["members"] == DIRECT_LIMIT + 1:
            cl.add("gives up:more than 4096 members")
        if pred["ties"] is not None:
            cl |= direct_classes(pred, t.ora["lcpfull"])
            if pred["pair_resolve"] is not None:
                cl |= resolve_model(t.enc, t.sigma, t.ora, pred)["classes"]
            if pred["rounds"]:
                cl |= chunks_model(t.enc, t.sigma, t.ora, pred)["classes"]
        else:
            pred["is_left"] = np.zeros(pred["sizes"].size, dtype=bool)
            cl |= direct_classes(pred, t.ora["lcpfull"])
        out[name] = cl
    return out
