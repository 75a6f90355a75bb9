"""Every alphabet size the engine accepts (2..28 letters, gtamd_esa_create) against
the CPU oracle.  Alphabets of 2 and 3 letters run through the 2-bit (DNA) kernels,
4 is DNA, 5..28 use the 5-bit keys; the MSD first sort takes 5-bit alphabets only
up to 20 letters.  The DNA and protein tests cover 4 and 20; the sizes between,
and the two ends, are here."""
import numpy as np
import pytest

import engine_paths
import oracle_util as ou
from genometools_amd import esa
from thread_comm import build_in_parts

pytestmark = pytest.mark.gpu

SIGMAS = list(range(2, 29))
FORCED_SIGMAS = [2, 3, 5, 12, 20, 21, 28]
WILD, SEP = 254, 255


def key_syms(sigma):
    """symbols of one sort key: the largest prefix length the engine takes"""
    return 20 if sigma <= 4 else 10


def _assert_same_as_oracle(enc, sigma, res, ora=None, what=""):
    ora = ou.esa(enc, sigma) if ora is None else ora
    assert np.array_equal(res.suf, ora["suf"]), ("suf", what)
    assert np.array_equal(res.bwt, ora["bwt"]), ("bwt", what)
    assert np.array_equal(res.lcp, ora["lcp"]), ("lcp", what)
    assert np.array_equal(res.llv, ora["llv"]), ("llv", what)
    st = ora["stats"]
    assert res.stats["longest"] == st["longest"], what
    assert res.stats["largelcpvalues"] == st["largelcpvalues"], what
    assert res.stats["maxbranchdepth"] == st["maxbranchdepth"], what
    assert res.stats["lcptabsum"] == int(st["lcptabsum"]), what
    assert res.stats["prefixlength"] == st["prefixlength"], what


def _with_specials(a, rng):
    """wildcard runs, isolated wildcards and separators laid over a text"""
    a = a.copy()
    n = a.size
    for _ in range(max(1, n // 2000)):
        p = int(rng.integers(0, n))
        a[p:p + int(rng.integers(2, 60))] = WILD
    a[rng.integers(0, n, max(1, n // 500))] = WILD
    a[rng.integers(0, n, max(1, n // 3000))] = SEP
    return a


def _texts(sigma):
    rng = np.random.default_rng(1000 + sigma)
    for n in (1, 2, 63, 64, 65, 4095, 4097, 70001):
        yield "iid_%d" % n, rng.integers(0, sigma, n, dtype=np.uint8)
    base = rng.integers(0, sigma, 70001, dtype=np.uint8)
    yield "specials", _with_specials(base, rng)
    yield "specials_at_ends", np.concatenate(
        [[WILD] * 5, base[:3000], [SEP], base[:3000], [WILD] * 9]).astype(np.uint8)
    # the largest letter sits next to the key's padding code
    yield "largest_letter", np.full(3000, sigma - 1, dtype=np.uint8)
    yield "largest_letter_runs", np.concatenate(
        [[sigma - 1] * 40, [WILD], [sigma - 1] * 30, [SEP], [sigma - 1] * 25,
         [WILD], [sigma - 1] * 70]).astype(np.uint8)
    yield "letter_0", np.zeros(3000, dtype=np.uint8)
    yield "period_2", np.tile(np.array([0, 1], dtype=np.uint8), 4000)
    yield "period_7", np.tile((np.array([0, sigma - 1, 1, sigma - 1, 0, 1, 1]) % sigma)
                              .astype(np.uint8), 1500)
    # a copied stretch longer than 255: .llv carries the large values
    b = rng.integers(0, sigma, 5000, dtype=np.uint8)
    yield "copied_stretch", np.concatenate([b, base[:100], b[1000:1700], base[:10],
                                            b[:400]]).astype(np.uint8)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_every_alphabet_size(gpu, sigma):
    texts = list(_texts(sigma))
    with esa.EsaEngine(max(t.size for _, t in texts), sigma) as eng:
        for name, enc in texts:
            eng.set_sequence(enc)
            eng.run()
            _assert_same_as_oracle(enc, sigma, eng.result(), what=name)


def _mixed(sigma, n, seed):
    """i.i.d. letters with specials, copied blocks (long and short, many copies of
    the short ones: tie groups of every size) and a tandem repeat"""
    rng = np.random.default_rng(seed)
    a = _with_specials(rng.integers(0, sigma, n, dtype=np.uint8), rng)
    for _ in range(max(1, n // 20000)):
        ln = int(rng.integers(300, 3000))
        src, dst = rng.integers(0, n - ln, 2)
        a[dst:dst + ln] = a[src:src + ln].copy()
    short = rng.integers(0, sigma, 40, dtype=np.uint8)
    for dst in rng.integers(0, n - 40, max(1, n // 5000)):
        a[dst:dst + 40] = short
    t0 = int(rng.integers(0, n - 2000))
    a[t0:t0 + 2000] = np.tile(rng.integers(0, sigma, 3, dtype=np.uint8), 700)[:2000]
    return a


@pytest.mark.parametrize("n", [300_000, 1_000_000])
@pytest.mark.parametrize("sigma", FORCED_SIGMAS)
def test_default_path_at_size(gpu, sigma, n):
    enc = _mixed(sigma, n, 77 + sigma)
    _assert_same_as_oracle(enc, sigma, esa.suffixerator_tables(enc, sigma))


@pytest.mark.parametrize("msd", ["1", "0"])
@pytest.mark.parametrize("sigma", FORCED_SIGMAS)
def test_msd_switch(gpu, monkeypatch, capfd, sigma, msd):
    """GTAMD_MSD=1 runs the MSD first sort for the alphabets it takes (2-bit keys,
    5-bit keys up to 20 letters at prefixlength <= 9); for 21..28 letters the
    switch has no effect: the LSD sort runs either way"""
    enc = _mixed(sigma, 300_000, 5 + sigma)
    monkeypatch.setenv("GTAMD_MSD", msd)
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    res = esa.suffixerator_tables(enc, sigma)
    err = capfd.readouterr().err
    ora = ou.esa(enc, sigma)
    _assert_same_as_oracle(enc, sigma, res, ora)
    takes_msd = sigma <= 4 or (sigma <= 20 and ora["stats"]["prefixlength"] <= 9)
    p = engine_paths.single(err)
    assert p["switches"]["msd"] == int(msd)
    assert p["run"]["first_sort"] == ("msd" if msd == "1" and takes_msd else "lsd"), err
    assert (p["msd"] is not None) == (msd == "1" and takes_msd), err


@pytest.mark.parametrize("switch", [("GTAMD_FORCE_WIDE", "1"), ("GTAMD_NO_PAIRS", "1"),
                                    ("GTAMD_RANK_WINDOW_BITS", "4")],
                         ids=lambda s: "%s=%s" % s)
@pytest.mark.parametrize("sigma", FORCED_SIGMAS)
def test_forced_paths(gpu, monkeypatch, capfd, sigma, switch):
    enc = _mixed(sigma, 300_000, 11 + sigma)
    monkeypatch.setenv(*switch)
    if switch[0] == "GTAMD_RANK_WINDOW_BITS":
        monkeypatch.setenv("GTAMD_NO_PAIRS", "1")   # (pairs would not need the table)
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    res = esa.suffixerator_tables(enc, sigma)
    p = engine_paths.single(capfd.readouterr().err)
    if switch[0] == "GTAMD_FORCE_WIDE":
        assert p["switches"]["force_wide"] == 1 and p["run"]["positions"] == 64
    elif switch[0] == "GTAMD_NO_PAIRS":
        assert p["switches"]["no_pairs"] == 1 and p["pair_resolve"] is None
        assert res.stats["pair_suffixes"] == 0
    else:
        assert p["switches"]["rank_window_bits"] == 4 and (p["rank_whole"] or p["rank_windows"])
    _assert_same_as_oracle(enc, sigma, res)


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("sigma", FORCED_SIGMAS)
def test_part_builds(gpu, sigma, parts):
    enc = _mixed(sigma, 300_000, 23 + sigma)
    tabs, stats, _ = build_in_parts(enc, sigma, parts)
    ora = ou.esa(enc, sigma)
    for name in ("suf", "bwt", "lcp", "llv"):
        assert np.array_equal(tabs[name], ora[name]), name
    st = ora["stats"]
    assert stats["longest"] == st["longest"]
    assert stats["largelcpvalues"] == st["largelcpvalues"]
    assert stats["maxbranchdepth"] == st["maxbranchdepth"]
    assert stats["lcptabsum"] == int(st["lcptabsum"])


@pytest.mark.parametrize("sigma", FORCED_SIGMAS)
def test_reverse_readmode(gpu, sigma):
    enc = _mixed(sigma, 300_000, 31 + sigma)
    enc[:7] = WILD          # the special prefix becomes a special suffix
    rev = enc[::-1].copy()
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_readmode(1)
        eng.set_sequence(enc)
        eng.run()
        _assert_same_as_oracle(rev, sigma, eng.result())


# ---------------------------------------------------------------------------
# bucket table
# ---------------------------------------------------------------------------
def _kmer_codes(enc, sigma, k):
    """padded k-code of every suffix that starts with a letter (bcktab.c: a prefix
    shorter than k letters is padded with the largest letter), as int64"""
    n = enc.size
    ext = np.concatenate([enc, np.full(k, WILD, dtype=np.uint8)]).astype(np.int64)
    code = np.zeros(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    for j in range(k):
        d = ext[j:j + n]
        live &= d < sigma
        code = code * sigma + np.where(live, d, sigma - 1)
    return code[enc < sigma]


def _largest_k(sigma, limit):
    k = 0
    while k < key_syms(sigma) and sigma ** (k + 1) <= limit:
        k += 1
    return k


def _bck_text(sigma):
    rng = np.random.default_rng(500 + sigma)
    a = _with_specials(rng.integers(0, sigma, 60_000, dtype=np.uint8), rng)
    a[100:160] = sigma - 1      # padded codes next to real runs of the largest letter
    a[160] = WILD
    return a


@pytest.mark.parametrize("sigma", SIGMAS)
def test_bucket_table_every_alphabet(gpu, sigma):
    """GTAMD_WANT_BCK at k = 0 (the recommended prefix length), 1, 2 and the
    largest k with at most 2^22 codes, against the oracle; the content check of
    test_bucket_table_matches_oracle"""
    enc = _bck_text(sigma)
    ks = [0, 1, 2, _largest_k(sigma, 1 << 22)]
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        for k in ks:
            eng.set_prefixlength(k)
            eng.run(esa.WANT_SUF | esa.WANT_BCK)
            kk = eng.stats()["prefixlength"]
            assert k in (0, kk)
            got = eng.bcktab()
            want = ou.bcktab(enc, sigma, kk)
            for name, g, w in zip(("leftborder", "countspecialcodes", "distpfxidx"), got, want):
                assert np.array_equal(g, w), (name, kk)
            suf = eng.table(esa.TAB_SUF)
            lb = got[0]
            codes = np.flatnonzero(np.diff(lb.astype(np.int64)))
            for code in codes[[0, len(codes) // 2, -1]] if codes.size else []:
                digits = [(int(code) // sigma ** (kk - 1 - j)) % sigma for j in range(kk)]
                for i in range(int(lb[code]), min(int(lb[code + 1]), int(lb[code]) + 50)):
                    p = int(suf[i])
                    seen = [int(x) for x in enc[p:p + kk]]
                    letters = next((j for j, x in enumerate(seen) if x >= sigma), len(seen))
                    assert seen[:letters] == digits[:letters], (code, p)
                    assert all(d == sigma - 1 for d in digits[letters:]), (code, p)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_bucket_table_at_the_code_limit(gpu, sigma):
    """the largest k with sigma^k <= 2^31 codes (capped at the key width): too large
    to copy, so sampled left borders are compared with counts of the suffixes'
    padded k-codes; one letter more is refused"""
    k = _largest_k(sigma, 1 << 31)
    enc = _bck_text(sigma)[:20_000]
    codes = np.sort(_kmer_codes(enc, sigma, k))
    ncodes = sigma ** k
    rng = np.random.default_rng(sigma)
    probe = np.unique(np.concatenate([
        codes[rng.integers(0, codes.size, 40)], codes[rng.integers(0, codes.size, 40)] + 1,
        rng.integers(0, ncodes, 40), [0, 1, ncodes - 1, ncodes]]))
    probe = probe[probe <= ncodes]
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.set_prefixlength(k)
        eng.run(esa.WANT_SUF | esa.WANT_BCK)
        assert eng.stats()["prefixlength"] == k
        for c in probe:
            got = int(eng.table(esa.TAB_BCK, int(c), 1)[0])
            assert got == int(np.searchsorted(codes, c, "left")), (k, int(c))
        if k < key_syms(sigma):
            eng.set_prefixlength(k + 1)
            with pytest.raises(esa.EsaError, match="is too large"):
                eng.run(esa.WANT_SUF | esa.WANT_BCK)


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0, 1, 29, 30, 255])
def test_alphabet_size_refused(gpu, sigma):
    with pytest.raises(esa.EsaError, match="alphabet size %d not supported" % sigma):
        esa.EsaEngine(100, sigma)


@pytest.mark.parametrize("sigma", [2, 3, 5, 28])
def test_complement_readmodes_refused(gpu, sigma):
    with esa.EsaEngine(100, sigma) as eng:
        for mode, name in ((2, "cpl"), (3, "rcl")):
            with pytest.raises(esa.EsaError, match="readmode %s is only defined for DNA" % name):
                eng.set_readmode(mode)
