"""The reader of the packed index on the device (include/gtamd_pckidx.h,
genometools_amd/pck.py PackedIndexReader) and matstat / uniquesub through it
(mstat.MatchStats.set_index_packed).

Decode and rank: an image is built on the device and read back through the
reader; the decoded BWT equals .bwt on every row, rank(s, r) for every letter
and every row equals a cumulative count of .bwt in which specials count for
nobody, locate(r) equals .suf for every row of a letter suffix (every row for
-sprank images).  Search: ms(i) and mu(i) through a -dir rev packed index equal
those of MatchStats on the forward .suf at every position, and the witness is
n - (suf_rev[lo] + ms(i)) with lo from a backward search on the CPU."""
import functools
import os

import numpy as np
import pytest

import mstat_reference as mr
import oracle_util as ou
from genometools_amd import _lib, esa, mstat, pck

pytestmark = pytest.mark.gpu

WILDCARD, SEPARATOR = 254, 255
DNA = ["Atinsert.fna", "Duplicate.fna", "Random-Small.fna", "Random.fna", "Random159.fna",
       "Random160.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]
SUITE = dict(bsize=10, blbuck=8, locfreq=32, sprank=True, mkindex=True)    # gt_idxsearch_include.rb:67-68
LINE, CP, TILE = 192, 64, 16384      # rows of a 2-bit line, between two counter rows, of a decode tile


@pytest.fixture(scope="module")
def tools(gpu):
    with pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, pck.PackedIndexReader() as second, \
            mstat.MatchStats() as packed, mstat.MatchStats() as plain:
        yield dict(builder=builder, reader=reader, second=second, packed=packed, plain=plain)


def _letters(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8)


def _with_specials(n, sigma, seed):
    """specials next to each other, at positions 0 and n - 1 among them"""
    enc = _letters(n, sigma, seed)
    rng = np.random.default_rng(seed + 1)
    if n >= 8:
        at = rng.integers(0, n, max(2, n // 40))
        enc[at] = rng.choice([WILDCARD, SEPARATOR], at.size)
        enc[0], enc[n - 1] = WILDCARD, SEPARATOR
        enc[n // 2:n // 2 + 3] = [WILDCARD, SEPARATOR, WILDCARD]
    return enc


def _tables(eng, enc, readmode=0):
    eng.set_readmode(readmode)
    eng.set_sequence(enc)
    eng.run(esa.WANT_SUF | esa.WANT_BWT)
    return eng.table(esa.TAB_SUF), eng.table(esa.TAB_BWT)


def _check_reader(reader, bwt, suf, sigma, kw):
    """every row, every letter"""
    N = bwt.size
    info = reader.info()
    assert (info["rows"], info["numofchars"]) == (N, sigma)
    assert info["locate_interval"] == kw.get("locfreq", 16)
    assert info["two_bit"] == int(sigma <= 4) and info["line_rows"] == (LINE if sigma <= 4 else CP)
    assert np.array_equal(reader.bwt(), bwt)
    if N > 3:
        assert np.array_equal(reader.bwt(1, N - 3), bwt[1:N - 2])
    rows = np.arange(N + 1, dtype=np.uint64)
    for s in range(sigma):
        want = np.concatenate([[0], np.cumsum(bwt == s)]).astype(np.uint64)
        got = reader.rank(np.full(N + 1, s, dtype=np.uint8), rows)
        assert np.array_equal(got, want), (s, np.flatnonzero(got != want)[:5])
    special_rows = int((bwt >= 254).sum())
    assert info["special_rows"] == special_rows
    if not kw.get("locfreq", 16):
        with pytest.raises(_lib.EsaError, match="no locate information"):
            reader.locate(rows[:1])
        return
    upto = N if kw.get("sprank") else N - special_rows       # the rows of the letter suffixes
    got = reader.locate(rows[:upto])
    assert np.array_equal(got, suf[:upto]), np.flatnonzero(got != suf[:upto])[:5]
    assert info["rot0_row"] == int(np.flatnonzero(suf == 0)[0])


def _build_and_check(tools, enc, sigma, both=True, **kw):
    with esa.EsaEngine(enc.size, sigma) as eng:
        suf, bwt = _tables(eng, enc)
        tools["builder"].build_from_esa(eng, **kw)
        reader = tools["reader"].open_builder(tools["builder"])
        _check_reader(reader, bwt, suf, sigma, kw)
        if both:
            # the same image from host memory: the same decoded form
            second = tools["second"].open(tools["builder"].image())
            _check_reader(second, bwt, suf, sigma, kw)
            for part in pck.PackedIndexReader.PARTS:
                assert np.array_equal(reader.decoded(part), second.decoded(part)), part


FLAVOURS = [dict(), dict(locbitmap=True), dict(locfreq=0), SUITE, dict(locfreq=1, sprank=True),
            dict(locfreq=7, locbitmap=True, sprank=True), dict(bsize=5, blbuck=3, locfreq=7, mkindex=True),
            dict(bsize=1, blbuck=1, locfreq=32), dict(bsize=16, blbuck=8, locfreq=1, locbitmap=False),
            dict(bsize=8, blbuck=3, locfreq=32, locbitmap=True, mkindex=True)]


@pytest.mark.parametrize("name", DNA)
def test_the_nine_fixtures(tools, name):
    enc = ou.encode_fasta(ou.fixture_path(name))
    for kw in (SUITE, dict(), dict(locbitmap=True), dict(locfreq=0)):
        _build_and_check(tools, enc, 4, **kw)


@pytest.mark.parametrize("kw", FLAVOURS, ids=lambda kw: "-".join("%s%s" % (k[:3], int(v)) for k, v in kw.items()) or "defaults")
def test_bucket_borders(tools, kw):
    """n + 1 = L - 1, L, L + 1, 2 L and 257 buckets + 3, with specials next to each
    other and at both ends"""
    L = kw.get("bsize", 8) * kw.get("blbuck", 8)
    for N in (L - 1, L, L + 1, 2 * L, 257 * L + 3):
        if N >= 2:
            _build_and_check(tools, _with_specials(N - 1, 4, N), 4, both=N < 1000, **kw)


@pytest.mark.parametrize("N", [LINE - 1, LINE, LINE + 1, 2 * LINE - 1, 2 * LINE, 2 * LINE + 1,
                               32 * LINE - 1, 32 * LINE, 32 * LINE + 1,       # (32 lines: a word of the line flags)
                               TILE - 1, TILE, TILE + 1])
def test_line_and_tile_borders_two_bit(tools, N):
    for kw in (SUITE, dict(locbitmap=True)):
        _build_and_check(tools, _with_specials(N - 1, 4, N), 4, both=False, **kw)


@pytest.mark.parametrize("sigma,B", [(2, 16), (5, 8), (20, 5), (20, 1)])
def test_other_alphabets_and_their_borders(tools, sigma, B):
    """2 letters in the 2-bit lines, 5 and 20 in bytes: the borders of the counter rows"""
    for N in (CP - 1, CP, CP + 1, 2 * CP - 1, 2 * CP, 2 * CP + 1, TILE + 1, 40000):
        for kw in (dict(bsize=B, blbuck=3, locfreq=7), dict(bsize=B, blbuck=8, locfreq=32, sprank=True, mkindex=True)):
            _build_and_check(tools, _with_specials(N - 1, sigma, N + sigma), sigma, both=N < 1000, **kw)


def test_special_texts(tools):
    """one letter; 20 % wildcards in runs (RandomN-like); 300 separators"""
    _build_and_check(tools, np.zeros(1, dtype=np.uint8), 4)
    _build_and_check(tools, np.full(1, 3, dtype=np.uint8), 4, **SUITE)
    _build_and_check(tools, np.full(5000, 2, dtype=np.uint8), 4, **SUITE)
    rng = np.random.default_rng(5)
    enc = _letters(100000, 4, 6)
    for a in rng.integers(0, enc.size, 400):
        enc[a:a + 50] = WILDCARD
    assert 0.15 < (enc == WILDCARD).mean() < 0.25
    for kw in (SUITE, dict(), dict(locbitmap=True, mkindex=True)):
        _build_and_check(tools, enc, 4, **kw)
    enc = _letters(60000, 4, 7)
    enc[rng.choice(enc.size, 300, replace=False)] = SEPARATOR
    for kw in (SUITE, dict(locfreq=7)):
        _build_and_check(tools, enc, 4, **kw)


def test_both_ways_the_builder_writes(tools, monkeypatch):
    """GTAMD_PCK_DIRECT: the tiles of the builder write straight into the image"""
    enc = _with_specials(50000, 4, 8)
    for direct in (None, "1"):
        if direct is None:
            monkeypatch.delenv("GTAMD_PCK_DIRECT", raising=False)
        else:
            monkeypatch.setenv("GTAMD_PCK_DIRECT", direct)
        for kw in (SUITE, dict(locbitmap=True)):
            _build_and_check(tools, enc, 4, **kw)


def test_an_image_in_device_memory(tools):
    import torch
    enc = _with_specials(30000, 4, 9)
    with esa.EsaEngine(enc.size, 4) as eng:
        suf, bwt = _tables(eng, enc)
        tools["builder"].build_from_esa(eng, **SUITE)
        raw = tools["builder"].image()
        t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda:0")
        t[3:3 + raw.size] = torch.from_numpy(raw).to("cuda:0")          # (not aligned)
        torch.cuda.synchronize()
        reader = tools["reader"].open_device(t.data_ptr() + 3, raw.size)
        del t
        _check_reader(reader, bwt, suf, 4, SUITE)


def test_images_that_lie_are_refused(tools):
    enc = _with_specials(30000, 4, 10)
    with esa.EsaEngine(enc.size, 4) as eng:
        _tables(eng, enc)
        tools["builder"].build_from_esa(eng)
        raw = tools["builder"].image()
    info = tools["builder"].info()
    bad = raw.copy()
    bad[info["var_data_pos"] + 100:info["var_data_pos"] + 4000] ^= 0x5a
    with pytest.raises(_lib.EsaError, match="packed index reader: the image does not decode"):
        tools["reader"].open(bad)
    with pytest.raises(_lib.EsaError, match="packed index reader: "):
        tools["reader"].open(raw[:-1])
    with pytest.raises(_lib.EsaError, match="no image is open"):
        tools["reader"].info()
    reader = tools["reader"].open(raw)
    with pytest.raises(_lib.EsaError, match="outside the index"):
        reader.rank(np.array([4], dtype=np.uint8), np.array([0], dtype=np.uint64))
    with pytest.raises(_lib.EsaError, match="outside the index"):
        reader.locate(np.array([enc.size + 1], dtype=np.uint64))


# ---- search ---------------------------------------------------------------------

def _queries(enc, sigma, m, seed):
    """m positions: pieces cut from the text with substitutions and wildcards, and random ones"""
    rng = np.random.default_rng(seed)
    out = []
    letters = enc[enc < 254]
    while sum(p.size for p in out) < m - 200 and letters.size > 4:
        a = int(rng.integers(0, enc.size))
        piece = enc[a:a + int(rng.integers(5, 400))].copy()
        hit = rng.random(piece.size) < 0.04
        piece[hit] = rng.integers(0, sigma, int(hit.sum()))
        piece[rng.random(piece.size) < 0.004] = WILDCARD
        out += [piece, np.array([SEPARATOR], dtype=np.uint8)]
    out.append(_letters(max(0, m - sum(p.size for p in out)), sigma, seed + 1))
    return np.concatenate(out)[:m]


def _backward_search(bwt, sigma, query):
    """(ms, mu, lowest row of the last interval that was not empty) of every query
    position by the reference's loops, src/match/eis-bwtseq.c:225-364"""
    occ = [np.concatenate([[0], np.cumsum(bwt == s)]) for s in range(sigma)]
    count = np.concatenate([[0], np.cumsum([o[-1] for o in occ])])
    m = query.size
    ms, mu, low = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.int64)
    for i in range(m):
        c = query[i]
        if c >= sigma or count[c] == count[c + 1]:
            continue
        lo, hi, k = count[c], count[c + 1], 1
        low[i] = lo
        unique = 1 if lo + 1 == hi else 0
        while i + k < m:
            c = query[i + k]
            if c >= sigma:
                break
            lo, hi = count[c] + occ[c][lo], count[c] + occ[c][hi]
            if lo >= hi:
                break
            k += 1
            low[i] = lo
            if not unique and lo + 1 == hi:
                unique = k
        ms[i], mu[i] = k, unique
    return ms, mu, low


@functools.lru_cache(maxsize=None)
def _search_subject(N, sigma):
    enc = _with_specials(N - 1, sigma, 1000 + N)
    enc.setflags(write=False)
    return enc


def _search_case(tools, enc, sigma, m=5000, caps=(1, 5, 20), **kw):
    n = enc.size
    query = _queries(enc, sigma, m, n)
    with esa.EsaEngine(n, sigma) as eng:
        suf_rev, bwt_rev = _tables(eng, enc, readmode=1)
        tools["builder"].build_from_esa(eng, **kw)
        reader = tools["reader"].open_builder(tools["builder"])
        suf, _ = _tables(eng, enc, readmode=0)
    tools["packed"].set_index_packed(reader)
    tools["plain"].set_index(enc, suf, sigma)
    want_ms, _ = tools["plain"].matstat(query)
    want_mu = tools["plain"].uniquesub(query)
    ms, mu, low = _backward_search(bwt_rev, sigma, query)
    assert np.array_equal(ms, want_ms) and np.array_equal(mu, want_mu)     # (the CPU search, for the witness)
    got_mu = tools["packed"].uniquesub(query)
    assert np.array_equal(got_mu, want_mu), np.flatnonzero(got_mu != want_mu)[:5]
    if kw.get("locfreq", 16):
        got_ms, got_w = tools["packed"].matstat(query)
        witness = np.where(ms > 0, n - (suf_rev[low].astype(np.int64) + ms), 0)
        assert np.array_equal(got_w, witness.astype(np.uint64)), np.flatnonzero(got_w != witness)[:5]
        # (what the witness means: the match starts there in the subject)
        for i in np.flatnonzero(ms > 0)[:200]:
            assert np.array_equal(enc[got_w[i]:got_w[i] + ms[i]], query[i:i + ms[i]])
    else:
        with pytest.raises(_lib.EsaError, match="no locate information"):
            tools["packed"].matstat(query)
        got_ms = np.empty(query.size, dtype=np.uint32)
        import torch
        q = torch.from_numpy(query).to("cuda:0")
        out = torch.zeros(query.size, dtype=torch.int32, device="cuda:0")
        tools["packed"].matstat_device(q.data_ptr(), query.size, out.data_ptr())
        got_ms = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_ms, want_ms), np.flatnonzero(got_ms != want_ms)[:5]
    for cap in caps:
        if kw.get("locfreq", 16):
            length, pos = tools["packed"].matstat(query, cap)
            assert np.array_equal(length, mr.capped(ms, cap))
            exact = ms <= cap
            assert np.array_equal(pos[exact], got_w[exact])
        assert np.array_equal(tools["packed"].uniquesub(query, cap), mr.capped(mu, cap))
    info = tools["packed"].info()
    assert info["positions"] == query.size and info["reruns"] == 0 and info["symbols_compared"] > 0


@pytest.mark.parametrize("kw", [SUITE, dict(), dict(locbitmap=True, mkindex=True), dict(locfreq=0),
                                dict(bsize=5, blbuck=3, locfreq=7, sprank=True)],
                         ids=["suite", "defaults", "bitmap", "nolocate", "small"])
def test_search_at_the_bucket_borders(tools, kw):
    L = kw.get("bsize", 8) * kw.get("blbuck", 8)
    for N in (L - 1, L, L + 1, 2 * L, 257 * L + 3):
        if N >= 3:
            _search_case(tools, _search_subject(N, 4), 4, **kw)


@pytest.mark.parametrize("N", [LINE, LINE + 1, TILE - 1, TILE + 1, 100000])
def test_search_at_the_line_and_tile_borders(tools, N):
    _search_case(tools, _search_subject(N, 4), 4, **SUITE)


def test_search_other_alphabets(tools):
    for sigma, B in ((2, 16), (5, 8), (20, 5)):
        _search_case(tools, _search_subject(30000, sigma), sigma, bsize=B, blbuck=8, locfreq=32, sprank=True, mkindex=True)
    rng = np.random.default_rng(3)
    enc = _letters(60000, 4, 11)
    for a in rng.integers(0, enc.size, 240):
        enc[a:a + 50] = WILDCARD
    _search_case(tools, enc, 4, **SUITE)
    enc = _letters(40000, 4, 12)
    enc[rng.choice(enc.size, 300, replace=False)] = SEPARATOR
    _search_case(tools, enc, 4, **SUITE)


def test_queries_that_match_nothing(tools):
    enc = (_letters(5000, 2, 13) * 2).astype(np.uint8)          # letters 0 and 2 of four
    with esa.EsaEngine(enc.size, 4) as eng:
        _tables(eng, enc, readmode=1)
        tools["builder"].build_from_esa(eng, **SUITE)
        reader = tools["reader"].open_builder(tools["builder"])
    s = tools["packed"]
    s.set_index_packed(reader)
    for query in (np.full(40, WILDCARD, np.uint8), np.array([SEPARATOR, WILDCARD], np.uint8), np.zeros(0, np.uint8),
                  np.full(30, 1, np.uint8), np.full(30, 3, np.uint8), np.full(3, 7, np.uint8)):
        length, pos = s.matstat(query)
        assert not length.any() and not pos.any() and not s.uniquesub(query).any()
    # the searcher goes back to a suffix table, and forth
    suf = ou.esa(enc, 4)["suf"]
    query = enc[100:300].copy()
    s.set_index(enc, suf, 4)
    want = s.matstat(query)[0]
    s.set_index_packed(reader)
    assert np.array_equal(s.matstat(query)[0], want)
    with pytest.raises(_lib.EsaError, match="no image open|invalid argument"):
        with pck.PackedIndexReader() as closed:
            s.set_index_packed(closed)


def test_a_searcher_whose_reader_lost_its_image(tools):
    """a reader whose next open fails holds no image: the searcher that points to
    it refuses, and searches again after a good open"""
    enc = _with_specials(20000, 4, 16)
    with esa.EsaEngine(enc.size, 4) as eng:
        _tables(eng, enc, readmode=1)
        tools["builder"].build_from_esa(eng, **SUITE)
        raw = tools["builder"].image()
    query = enc[500:900].copy()
    with pck.PackedIndexReader() as reader, mstat.MatchStats() as s:
        s.set_index_packed(reader.open(raw))
        want = s.matstat(query)
        for bad in (raw[:-1], raw[:9000]):
            with pytest.raises(_lib.EsaError, match="packed index reader: "):
                reader.open(bad)
            with pytest.raises(_lib.EsaError, match="no image open any more"):
                s.matstat(query)
            with pytest.raises(_lib.EsaError, match="no image open any more"):
                s.uniquesub(query)
        reader.open(raw)
        got = s.matstat(query)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_size(tools):
    """2^25 symbols of uniform DNA, 10^6 query positions: lengths against MatchStats
    on .suf, witnesses by reading the subject.  More than one decode grid's worth of
    buckets for the row arithmetic, and the rank directory of the marks far from 0.
    All of it, the making of the text and the queries included, in under ten seconds."""
    import time
    import torch
    started = time.monotonic()
    n, m = 1 << 25, 1000000
    enc = _letters(n, 4, 14)
    rng = np.random.default_rng(15)
    pieces = []
    for a in rng.integers(0, n - 200, m // 100):
        p = enc[a:a + 100].copy()
        p[rng.integers(0, 100, 3)] = rng.integers(0, 4, 3)
        pieces.append(p)
    query = np.concatenate(pieces)
    q = torch.from_numpy(query).to("cuda:0")
    want = torch.zeros(m, dtype=torch.int32, device="cuda:0")
    got = torch.zeros(m, dtype=torch.int32, device="cuda:0")
    pos = torch.zeros(m, dtype=torch.int64, device="cuda:0")
    with esa.EsaEngine(n, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF)
        t = torch.from_numpy(enc).to("cuda:0")
        tools["plain"].set_index_engine(eng, t.data_ptr(), n)
        tools["plain"].matstat_device(q.data_ptr(), m, want.data_ptr())
        torch.cuda.synchronize()
        eng.set_readmode(1)
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        tools["builder"].build_from_esa(eng, **SUITE)
        reader = tools["reader"].open_builder(tools["builder"])
    info = reader.info()
    assert info["rows"] == n + 1 and info["marks"] >= n // 32
    tools["packed"].set_index_packed(reader)
    tools["packed"].matstat_device(q.data_ptr(), m, got.data_ptr(), pos.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # every witness: the subject reads as the query does, over the whole match
    length = got.to(torch.int64)
    for k in range(0, int(length.max().item())):
        live = length > k
        idx = torch.nonzero(live).flatten()
        assert torch.equal(t[pos[idx] + k], q[idx + k]), k
    assert time.monotonic() - started < 10.0
