"""Plain-Python restatement of the sequential traversal behind `gt readjoiner
assembly` with default options (include/gtamd_strgraph.h states the rules; the
reference: src/match/rdj-strgraph.c, rdj-contigpaths.c, rdj-contigs-writer.c and
src/extended/assembly_stats_calculator.c): the string graph of a list of
suffix-prefix matches, its unbranched paths in the order the reference visits
them with its elimination marks, the contigs they spell, X.contigs.fas and the
stdout.  tests/test_assembly_reference.py holds it to every golden call; from
there on it is the yardstick for generated shapes.

RULES names the rules of the header; `broken` switches one of them off, which
the mutation checks of the tests use.  Test infrastructure only."""
import numpy as np

from spmred_reference import PREFIX_DIRECT, SUFFIX_DIRECT, revcomp

DEPTHCUTOFF, LENGTHCUTOFF = 3, 100
WIDTH = 60
RULES = ("min_len", "self_match", "edge_cases", "edge_length", "insertion_order", "internal",
         "orientation", "hairpin_tie", "single_edge_marks", "cycle_start", "cycles_last", "strand", "depth",
         "cutoffs", "numbering")


def other(v):
    return v ^ 1


def edge_pair(sn, pn, flags):
    """the two edges (from, to) of a match, in the order they are inserted"""
    B, E = lambda r: 2 * r, lambda r: 2 * r + 1
    sd, pd = bool(flags & SUFFIX_DIRECT), bool(flags & PREFIX_DIRECT)
    if sd and pd:
        return (E(sn), E(pn)), (B(pn), B(sn))
    if sd:
        return (E(sn), B(pn)), (E(pn), B(sn))
    if pd:
        return (B(sn), E(pn)), (B(pn), E(sn))
    return (B(sn), B(pn)), (E(pn), E(sn))


def build_graph(lengths, records, min_len=0, broken=()):
    """adjacency lists [(to, edge length)] of the 2R vertices, in insertion order"""
    adj = [[] for _ in range(2 * len(lengths))]
    for sn, pn, k, f in np.asarray(records, dtype=np.int64).reshape(-1, 4).tolist():
        if k < min_len and "min_len" not in broken:
            continue
        if sn == pn and "self_match" not in broken:
            continue
        pair = edge_pair(sn, pn, f)
        if "edge_cases" in broken and not f & PREFIX_DIRECT:
            pair = ((pair[0][0], other(pair[0][1])), (pair[1][0] ^ 1, pair[1][1]))
        for a, b in pair:
            adj[a].append((b, lengths[(a if "edge_length" in broken else b) >> 1] - k))
    if "insertion_order" in broken:
        adj = [sorted(e, key=lambda x: x[1]) for e in adj]
    return adj


def is_internal(adj, v, broken=()):
    if "internal" in broken:
        return len(adj[v]) == 1
    return len(adj[v]) == 1 and len(adj[other(v)]) == 1


def traverse(adj, broken=()):
    """the paths as (first vertex, [(vertex, edge length), ...]) in the order the
    reference starts them (gt_strgraph_traverse with its marks)"""
    n = len(adj)
    gone = [False] * n
    paths = []
    internal = [is_internal(adj, v, broken) for v in range(n)]

    def simple_path(i, j):
        steps = []
        frm, to, k = i, adj[i][j][0], adj[i][j][1]
        while internal[to] and to != i and not gone[to]:
            steps.append((to, k))
            gone[to] = gone[other(to)] = True
            frm = to
            to, k = adj[frm][0]
        steps.append((to, k))
        paths.append((i, steps))

    def from_vertex(i):
        edges = range(len(adj[i]))
        for j in (reversed(edges) if "hairpin_tie" in broken else edges):
            to = adj[i][j][0]
            if gone[to] and (internal[to] or "single_edge_marks" not in broken):
                continue
            simple_path(i, j)

    def cycles():
        order = range(n)
        for i in (reversed(order) if "cycle_start" in broken else order):
            if internal[i] and not gone[i]:
                from_vertex(i)

    if "cycles_last" in broken:
        cycles()
    order = range(n)
    for i in (reversed(order) if "orientation" in broken else order):
        if gone[i]:
            continue
        if not adj[i]:
            gone[i] = True
        elif not internal[i]:
            from_vertex(i)
            gone[i] = True
    if "cycles_last" not in broken:
        cycles()
    return paths


def oriented(reads, v, broken=()):
    """the read of vertex v as a contig reads it: E direct, B reverse complement"""
    r = np.asarray(reads[v >> 1], dtype=np.uint8)
    return r if (v & 1) != ("strand" in broken) else revcomp(r)


def contigs(reads, records, min_len=0, depthcutoff=DEPTHCUTOFF, lengthcutoff=LENGTHCUTOFF, broken=()):
    """the kept contigs in order: [(symbols, depth, first vertex, last vertex)]"""
    lengths = [len(r) for r in reads]
    out = []
    for first, steps in traverse(build_graph(lengths, records, min_len, broken), broken):
        depth = 1 + len(steps) - ("depth" in broken)
        length = lengths[first >> 1] + sum(k for _, k in steps)
        if "cutoffs" in broken:
            if depth <= depthcutoff or length <= lengthcutoff:
                continue
        elif depth < depthcutoff or length < lengthcutoff:
            continue
        parts = [oriented(reads, first, broken)]
        for v, k in steps:
            parts.append(oriented(reads, v, broken)[lengths[v >> 1] - k:])
        out.append((np.concatenate(parts), depth, first, steps[-1][0]))
    if "numbering" in broken:
        out.sort(key=lambda c: -c[1])
    return out


def vertex_name(v):
    return "%d%s" % (v >> 1, "E" if v & 1 else "B")


def fasta(found):
    """X.contigs.fas of contigs()"""
    out = []
    for n, (sym, depth, first, last) in enumerate(found):
        path = vertex_name(first)
        if depth > 1:
            path += ("-->...-->" if depth > 2 else "-->") + vertex_name(last)
        out.append(">contig_%d length=%d depth=%d %s\n" % (n, sym.size, depth, path))
        text = "".join("acgt"[c] for c in sym.tolist())
        out.extend(text[a:a + WIDTH] + "\n" for a in range(0, len(text), WIDTH))
    return "".join(out).encode()


def statistics(lengths):
    """the lines of gt_assembly_stats_calculator_show for contig lengths (at least one)"""
    lengths = [int(x) for x in lengths]
    num, total = len(lengths), sum(lengths)
    mins = [int(np.float32(total) * (np.float32(v) / np.float32(100))) for v in (50, 80)]
    limits = (500, 1000, 10000, 100000, 1000000)
    larger = [0] * 5
    half = num >> 1
    fourth = half >> 1
    three = fourth + half
    q1 = median = q3 = 0
    nval, lval, done = [0, 0], [0, 0], [False, False]
    cur_len = cur_num = 0
    for key in sorted(set(lengths), reverse=True):
        value = lengths.count(key)
        cur_len += key * value
        cur_num += value
        for i in range(5):
            if key > limits[i]:
                larger[i] = cur_num
        if q3 == 0 and cur_num >= fourth:
            q3 = key
        if median == 0 and cur_num >= half:
            median = key
        if q1 == 0 and cur_num >= three:
            q1 = key
        for i in range(2):
            if not done[i] and cur_len >= mins[i]:
                done[i], nval[i], lval[i] = True, key, cur_num
    out = ["number of contigs:     %d" % num, "total contigs length:  %d" % total,
           "mean contig size:      %.2f" % (total / num), "contig size first quartile: %d" % q1,
           "median contig size:         %d" % median, "contig size third quartile: %d" % q3,
           "longest contig:             %d" % max(lengths), "shortest contig:            %d" % min(lengths)]
    for name, count in zip(("500 nt: ", "1K nt:  ", "10K nt: ", "100K nt:", "1M nt:  "), larger):
        out.append("contigs > %s          %d (%.2f %%)" % (name, count, count * 100 / num))
    for i, v in enumerate((50, 80)):
        for letter, x in (("N", nval[i]), ("L", lval[i])):
            out.append("%s%02d                %s" % (letter, v, x if nval[i] > 0 else "n.a."))
    return out


def stdout_of(reads, lengths):
    """what the tool prints for a set of `reads` reads and the lengths of its contigs"""
    lines = ["gt readjoiner assembly (version 1.2)", "number of reads in filtered readset = %d" % reads,
             "calculate edges space for each vertex", "build string graph", "save contig paths",
             "pump encseq through cache", "save contig sequences"]
    lines += statistics(lengths) if len(lengths) else ["no contigs respect the given cutoff parameters"]
    return "".join("# %s\n" % l for l in lines).encode()


def stdout(reads, found, quiet=False):
    """what the tool prints for a read set and its contigs()"""
    return b"" if quiet else stdout_of(len(reads), [c[0].size for c in found])


def canonical(found):
    """the contigs as a sorted multiset of min(sequence, reverse complement)"""
    return sorted(min(c[0].tobytes(), revcomp(c[0]).tobytes()) for c in found)


# ---- generated shapes: reads and the list worked out, not searched for ------------

def chain(count, length=20, step=7, seed=5, flip=True):
    """`count` reads of `length` letters every `step` letters of a random text,
    every other one reverse-complemented with `flip`, and the count - 1 matches of
    neighbours in the form `readjoiner overlap` keeps"""
    rng = np.random.default_rng(seed)
    text = rng.integers(0, 4, length + step * (count - 1), dtype=np.uint8)
    reads, direct = [], []
    for k in range(count):
        d = not (flip and k % 3 == 1)
        r = text[k * step:k * step + length]
        reads.append(r.copy() if d else revcomp(r))
        direct.append(d)
    records = [match(a, direct[a], a + 1, direct[a + 1], length - step) for a in range(count - 1)]
    return reads, np.array(records, dtype=np.uint64).reshape(-1, 4)


def match(a, a_direct, b, b_direct, k):
    """the record of: read a as it lies (direct or not) ends with the k letters
    read b as it lies starts with; in the one of the two forms with a direct side"""
    if not a_direct and not b_direct:
        return (b, a, k, SUFFIX_DIRECT | PREFIX_DIRECT)
    return (a, b, k, (SUFFIX_DIRECT if a_direct else 0) | (PREFIX_DIRECT if b_direct else 0))


def disjoint_chains(chains, count=3, length=20, step=7, seed=9):
    """`chains` chains of `count` reads, no match between two of them"""
    reads, records = [], []
    for c in range(chains):
        r, m = chain(count, length, step, seed + c, flip=c % 2 == 1)
        m = m.copy()
        m[:, :2] += len(reads)
        reads += r
        records.append(m)
    return reads, np.concatenate(records)


def circle(count, length=20, step=7, seed=21):
    """reads of a circular text of count * step letters, one every step letters:
    every read internal, one cycle"""
    rng = np.random.default_rng(seed)
    ring = rng.integers(0, 4, count * step, dtype=np.uint8)
    text = np.concatenate([ring, ring[:length]])
    reads, direct = [], []
    for k in range(count):
        d = k % 4 != 2
        r = text[k * step:k * step + length]
        reads.append(r.copy() if d else revcomp(r))
        direct.append(d)
    records = [match(a, direct[a], (a + 1) % count, direct[(a + 1) % count], length - step) for a in range(count)]
    return reads, np.array(records, dtype=np.uint64).reshape(-1, 4)


def join(*sets):
    """several (reads, records) as one, read numbers shifted"""
    reads, records = [], []
    for r, m in sets:
        m = np.array(m, dtype=np.uint64).reshape(-1, 4).copy()
        m[:, :2] += len(reads)
        reads += list(r)
        records.append(m)
    return reads, np.concatenate(records) if records else np.zeros((0, 4), dtype=np.uint64)


def hairpin(arm=4, length=20, step=7, seed=31):
    """the text S X revcomp(S) tiled by arm + 2 reads every `step` letters, the
    first and the last of which are one read on its two strands, given once: the
    path 0E -> 1E -> ... -> 0B and its mirror image both start at 0E"""
    rng = np.random.default_rng(seed)
    count = arm + 2
    total = length + step * (count - 1)
    assert total >= 2 * length
    stem = rng.integers(0, 4, length, dtype=np.uint8)
    text = np.concatenate([stem, rng.integers(0, 4, total - 2 * length, dtype=np.uint8), revcomp(stem)])
    reads = [text[k * step:k * step + length].copy() for k in range(count - 1)]
    records = [match(a, True, a + 1, True, length - step) for a in range(count - 2)]
    records.append(match(count - 2, True, 0, False, length - step))
    return reads, np.array(records, dtype=np.uint64).reshape(-1, 4)


def junction(branches=3, arm=3, length=20, step=7, seed=41):
    """a stem of `arm` reads whose last read has `branches` successors, each the
    first of an arm of `arm` reads: a vertex with `branches` out-edges"""
    rng = np.random.default_rng(seed)
    stem = rng.integers(0, 4, length + step * (arm - 1), dtype=np.uint8)
    reads = [stem[k * step:k * step + length].copy() for k in range(arm)]
    records = [match(a, True, a + 1, True, length - step) for a in range(arm - 1)]
    for b in range(branches):
        text = np.concatenate([stem[-length:], rng.integers(0, 4, step * arm, dtype=np.uint8)])
        first = len(reads)
        dirs = [(k + b) % 2 == 0 for k in range(arm)]
        for k in range(arm):
            r = text[(k + 1) * step:(k + 1) * step + length]
            reads.append(r.copy() if dirs[k] else revcomp(r))
        records.append(match(arm - 1, True, first, dirs[0], length - step))
        for k in range(arm - 1):
            records.append(match(first + k, dirs[k], first + k + 1, dirs[k + 1], length - step))
    return reads, np.array(records, dtype=np.uint64).reshape(-1, 4)


def check_records(reads, records):
    """every record of a worked-out list is a true suffix-prefix match (one of a
    read with itself is not looked at: it adds nothing, whatever it claims)"""
    for sn, pn, k, f in np.asarray(records, dtype=np.int64).tolist():
        if sn == pn:
            continue
        s = reads[sn] if f & SUFFIX_DIRECT else revcomp(reads[sn])
        p = reads[pn] if f & PREFIX_DIRECT else revcomp(reads[pn])
        assert 0 < k <= min(len(s), len(p)) and s[len(s) - k:].tobytes() == p[:k].tobytes(), (sn, pn, k, f)
