"""The k-mer correction of `gt readjoiner correct -k K -c C`, restated: the
sequential definition of include/gtamd_kcorrect.h in Python, slow and plain
(src/match/rdj-errfind.c, src/match/rdj-twobitenc-editor.c, the traversal
src/match/esa-bottomup-errfind.inc).  Test infrastructure only.

`tables(text)` sorts the suffixes of a text (letters 0..3, specials 254 and 255
after the letters, an LCP never spans a special); `records(...)` walks the
groups and children of the table and lists the records in table order;
`correct(...)` applies them one after the other.  RULES names the rules of the
header; `broken` switches one of them off, which some golden or generated set
must notice (tests/test_kcorrect_reference.py).  `original_sources` reads every
source from the text as it was; it is used only to construct sets on which the
live reading differs.  "All four letters trusted: nothing happens" is no rule of
its own here: no child of such a group has fewer than c entries, so breaking
it changes nothing that any set could notice.  Nor is "a group without an
interval of depth k - 1 is skipped": it is one k-mer, which has nothing to be
corrected from; the rule shows in the number of groups examined alone."""
import numpy as np

RULES = ("first_trusted", "invalid_ends_group", "live_source", "last_write_wins",
         "mirror_complement", "source_once_per_group")


def revcomp(r):
    r = np.asarray(r, dtype=np.uint8)[::-1]
    return np.where(r < 254, 3 - r, r).astype(np.uint8)


def joined(reads):
    parts = []
    for i, r in enumerate(reads):
        if i:
            parts.append(np.array([255], dtype=np.uint8))
        parts.append(np.asarray(r, dtype=np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def mirrored(enc):
    enc = np.asarray(enc, dtype=np.uint8)
    return np.concatenate([enc, np.array([255], dtype=np.uint8), revcomp(enc)])


def split(enc):
    """the reads of joined symbols"""
    out, cur = [], []
    for x in np.asarray(enc).tolist():
        if x == 255:
            out.append(np.array(cur, dtype=np.uint8))
            cur = []
        else:
            cur.append(x)
    out.append(np.array(cur, dtype=np.uint8))
    return out


def tables(text):
    """(suf, lcp) of the text, n + 1 entries each: the non-special suffixes in
    order, then the special ones and the empty one by position; lcp[i] is the
    common prefix of entries i - 1 and i, which ends in front of a special"""
    t = np.asarray(text, dtype=np.uint8).tolist()
    n = len(t)
    nxt, at = [n] * (n + 1), n
    for p in range(n - 1, -1, -1):
        if t[p] >= 254:
            at = p
        nxt[p] = at
    keys = [(bytes(t[p:nxt[p]]) + b"\xff", nxt[p]) for p in range(n) if t[p] < 254]      # a special is larger than a letter
    order = sorted(range(len(keys)), key=keys.__getitem__)
    letters = [p for p in range(n) if t[p] < 254]
    suf = [letters[i] for i in order] + [p for p in range(n) if t[p] >= 254] + [n]
    lcp = [0] * (n + 1)
    for i in range(1, len(order)):
        a, b = keys[order[i - 1]][0], keys[order[i]][0]
        m = 0
        while m < len(a) - 1 and m < len(b) - 1 and a[m] == b[m]:
            m += 1
        lcp[i] = m
    return np.array(suf, dtype=np.uint64), np.array(lcp, dtype=np.uint64)


def records(text, suf, lcp, k, c, broken=(), layout=None):
    """[(table entry, target position, source position, first record of the
    group)] in record order, the positions in the text as it stands, and the
    figures (groups examined, groups with an untrusted child).  layout: a list
    that gets (first entry, end, child heads, valid children, records) of every
    group examined"""
    t = np.asarray(text, dtype=np.uint8)
    n = t.size
    N = int((t < 254).sum())
    out, examined, untrusted_groups = [], 0, 0
    if k < 2:
        return out, examined, untrusted_groups
    lcp = [int(x) for x in lcp[:N]] + [0]
    suf = [int(x) for x in suf[:N]]

    def valid(e):
        p = suf[e] + k - 1
        return p < n and t[p] < 254

    i = 0
    while i < N:
        j = i + 1
        while j < N and lcp[j] >= k - 1:
            j += 1
        heads = [i] + [x for x in range(i + 1, j) if lcp[x] < k]
        if len(heads) > 1:
            examined += 1
            ends = heads[1:] + [j]
            children = []
            for h, e in zip(heads, ends):
                if not valid(h) and "invalid_ends_group" not in broken:
                    break                                   # (broken: a k-mer like the others)
                children.append((h, e - h))
            children = children[:4]
            counts = [w for _, w in children]
            all_trusted = len(children) == 4 and all(w >= c for w in counts)
            trusted = [x for x in children if x[1] >= c]
            if not all_trusted and trusted:
                if "first_trusted" in broken:
                    src = max(trusted, key=lambda x: x[1])[0]
                else:
                    src = trusted[0][0]
                first = len(out)
                for h, w in children:
                    if w < c:
                        for e in range(h, h + w):
                            out.append((e, suf[e] + k - 1, suf[src] + k - 1, first))
                untrusted_groups += len(out) > first
            if layout is not None:
                layout.append((i, j, heads, len(children), len(out) - first if not all_trusted and trusted else 0))
        i = j
    return out, examined, untrusted_groups


def correct(text, k, c, mirror, suf=None, lcp=None, broken=(), original_sources=False, layout=None):
    """the corrected unmirrored symbols of `text` (its first half if `mirror`),
    the triples (table entry, normalised position, letter written) in record
    order, and the figures of the info struct"""
    t = np.asarray(text, dtype=np.uint8)
    n = t.size
    if suf is None:
        suf, lcp = tables(t)
    recs, examined, untrusted_groups = records(t, suf, lcp, k, c, broken, layout)
    first_mirror = n >> 1 if mirror else n
    half = t[:first_mirror].copy()
    original = half.copy()

    def norm(p):
        flip = p >= first_mirror and "mirror_complement" not in broken
        return (n - 1 - p if p >= first_mirror else p), flip

    writer = {}                       # position -> the record that wrote it last
    letter, dep, triples = [], [], []
    live = not original_sources and "live_source" not in broken
    for r, (e, target, source, first) in enumerate(recs):
        tp, tflip = norm(target)
        sp, sflip = norm(source)
        if "source_once_per_group" in broken:
            first = r
        d = -1
        if sp in writer:
            # the last record in front of the group that wrote the source: the
            # reference reads the trusted letter once, before the group's edits
            cands = [w for w in writer[sp] if w < first]
            d = cands[-1] if cands else -1
        x = int(letter[d]) if (d >= 0 and live) else int(original[sp])
        if sflip:
            x = 3 - x
        if tflip:
            x = 3 - x
        dep.append(d if live else -1)
        letter.append(x)
        writer.setdefault(tp, []).append(r)
        triples.append((e, tp, x))
    for tp, ws in writer.items():
        if tp < first_mirror:                               # (the separator in the middle: only where a rule is broken)
            half[tp] = letter[ws[0 if "last_write_wins" in broken else -1]]
    # the rounds of a synchronous pointer doubling over the dependencies
    ptr, done, rounds = list(dep), [d < 0 for d in dep], 0
    while not all(done):
        rounds += 1
        nptr, ndone = list(ptr), list(done)
        for r in range(len(ptr)):
            if not done[r]:
                if done[ptr[r]]:
                    ndone[r] = True
                else:
                    nptr[r] = ptr[ptr[r]]
        ptr, done = nptr, ndone
    depth = [0] * len(dep)
    for r, d in enumerate(dep):
        depth[r] = depth[d] + 1 if d >= 0 else 0
    changed = np.flatnonzero(half != original)
    delta = [0, 0, 0, 0]
    for p in changed:
        if original[p] < 4:                                 # (a special: only where a rule is broken)
            delta[int(original[p])] -= 1
        delta[int(half[p])] += 1
    info = dict(table_entries=n + 1, groups=examined, untrusted_groups=untrusted_groups, records=len(recs),
                dependent=sum(d >= 0 for d in dep), rounds=rounds, changed=int(changed.size), delta=delta,
                chain=max(depth) if depth else 0,
                conflicts=sum(len({letter[w] for w in ws}) > 1 for ws in writer.values()))
    return half, triples, info


def correct_reads(reads, k, c, **kw):
    """the reads after one call of the tool: corrected on both strands"""
    out, triples, info = correct(mirrored(joined(reads)), k, c, True, **kw)
    return split(out), triples, info


# ---- generated sets ----------------------------------------------------------------
def coverage_reads(seed, length, count, errors=0.3, genome=None):
    """`count` reads of `length` letters drawn from a random genome of length +
    count / 2 letters, a share `errors` of them with one substituted letter"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, length + count // 2 if genome is None else genome, dtype=np.uint8)
    reads = []
    for _ in range(count):
        at = int(rng.integers(0, g.size - length + 1))
        r = g[at:at + length].copy()
        if rng.random() < 0.5:
            r = revcomp(r)
        if rng.random() < errors:
            p = int(rng.integers(0, length))
            r[p] = (r[p] + 1 + int(rng.integers(0, 3))) % 4
        reads.append(r)
    return reads


def search(want, length, count, k, c, seeds):
    """the first seed of `seeds` whose coverage set has the property `want`
    (info, info with sources from the original text, reads after, reads after
    with original sources) -> bool"""
    for seed in seeds:
        reads = coverage_reads(seed, length, count)
        a, _, ia = correct_reads(reads, k, c)
        b, _, ib = correct_reads(reads, k, c, original_sources=True)
        if want(ia, ib, a, b):
            return seed
    return None


def write_fasta(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, "".join("acgtn"[min(int(x), 4)] for x in r)))


def parse_fasta(path):
    reads, cur = [], None
    code = {"a": 0, "c": 1, "g": 2, "t": 3}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if cur is not None:
                    reads.append(np.array(cur, dtype=np.uint8))
                cur = []
            elif line:
                cur.extend(code.get(ch, 254) for ch in line.lower())
    if cur is not None:
        reads.append(np.array(cur, dtype=np.uint8))
    return reads


# ---- sets for the borders of the kernels (tests/test_kcorrect_core.py, test_kcorrect_gpu.py) ----
def _random(rng, length):
    return rng.integers(0, 4, length, dtype=np.uint8)


def width_reads(c=3, k=8, seed=5):
    """groups with children of c - 1, c and c + 1 entries; with all four letters
    trusted; with three trusted and one absent; whose only valid child is
    untrusted (the others end a read)"""
    rng = np.random.default_rng(seed)
    reads = []

    def group(counts, ends=0):
        ctx = _random(rng, k - 1)
        for letter, count in enumerate(counts):
            for _ in range(count):
                reads.append(np.concatenate([_random(rng, 6), ctx, [letter], _random(rng, 6)]).astype(np.uint8))
        for _ in range(ends):
            reads.append(np.concatenate([_random(rng, 7), ctx]).astype(np.uint8))

    group([c - 1, c, c + 1, 0])
    group([c, c, c, c])
    group([c, 0, c + 1, c])
    group([1, 0, 0, 0], ends=2)
    return reads, k, c


def invalid_tail_reads(tile, k=8, seed=6):
    """tile + 6 copies of one read, whose last k - 1 letters two reads go on
    from with one letter and a third with another: the group's valid children,
    then tile + 6 invalid ones"""
    rng = np.random.default_rng(seed)
    r = _random(rng, 20)
    ctx = r[-(k - 1):]
    a = np.concatenate([_random(rng, 5), ctx, [0], _random(rng, 5)]).astype(np.uint8)
    b = np.concatenate([_random(rng, 5), ctx, [2], _random(rng, 5)]).astype(np.uint8)
    return [r] * (tile + 6) + [a, a.copy(), b], k, 2


def long_reads(seed=7):
    """reads of 300 letters that share 259 letters and more: LCP bytes of 255,
    and a k-mer that differs in its 255th letter"""
    rng = np.random.default_rng(seed)
    base = _random(rng, 300)
    other = base.copy()
    other[259] = (other[259] + 1) % 4
    far = base.copy()
    far[290] = (far[290] + 2) % 4
    return [base, base.copy(), far, other, _random(rng, 300)]


def many_records_reads(seed=8, count=110, length=60):
    """k = 2 and a c near the median count of a 2-mer: four groups, the first at
    table entry 0 and the last up to the last non-special suffix, thousands of
    records, many positions written twice"""
    rng = np.random.default_rng(seed)
    reads = [_random(rng, length) for _ in range(count)]
    return reads, 2, 2 * count * length // 16


def chain_reads(seed=9, count=110, length=60):
    """k = 5: thousands of records, hundreds of them dependent, chains of three"""
    rng = np.random.default_rng(seed)
    return [_random(rng, length) for _ in range(count)], 5, 12


def mixed_reads(seed=10):
    """reads of several lengths and one with a wildcard, over a genome with errors"""
    rng = np.random.default_rng(seed)
    g = _random(rng, 60)
    reads = []
    for i in range(50):
        length = int(rng.integers(12, 31))
        at = int(rng.integers(0, g.size - length + 1))
        r = g[at:at + length].copy()
        if i % 3 == 0:
            p = int(rng.integers(0, length))
            r[p] = (r[p] + 1) % 4
        if i % 2:
            r = revcomp(r)
        reads.append(r)
    reads[7][5] = 254
    reads[20][0] = 254
    return reads, 6, 2


def tile_border(layout, tile, kind):
    """some group of the layout that gives records and (kind `head`) whose first
    entry is the last of a tile and its second child starts the next, or
    (`child`) one of whose valid children lies on both sides of a tile border"""
    for i, j, heads, valid, recs in layout:
        if not recs:
            continue
        if kind == "head" and i % tile == tile - 1 and heads[1] == i + 1:
            return True
        if kind == "child":
            ends = heads[1:] + [j]
            for h, e in list(zip(heads, ends))[:valid]:
                if h // tile != (e - 1) // tile:
                    return True
    return False
