"""The device checkers (tests/device_check.py) on the CPU: they accept the oracle's
tables and the reference's own, and reject every seeded mutation of the table each
of them checks -- an .lcp byte or .llv value off by one, a byte of 254 raised to
255 with an .llv entry, a dropped .llv entry, two neighbours of .suf swapped, a
duplicated .suf entry, a changed .bwt byte -- at table index 1, in the special
tail, at the entry of position n and at random indices.  The packed-index
checker accepts the oracle's INDEX.bdx images (oracle/pck_oracle.c) and rejects
a single flipped bit in each kind of field, naming the bucket.  The full-size GPU
tests rely on these checkers to be exact, not sampled."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

import device_check as dc
import oracle_util as ou
from genometools_amd import synth


def _special_heavy(seed, n):
    """uniform DNA with a third of its positions special: runs and single
    wildcards and separators, a run at both ends"""
    rng = np.random.default_rng(seed)
    enc = rng.integers(0, 4, n).astype(np.uint8)
    enc[rng.random(n) < 0.2] = 254
    for start in rng.integers(0, n - 40, n // 200):
        enc[start:start + rng.integers(1, 40)] = 254
    enc[rng.random(n) < 0.02] = 255
    enc[:7] = 254
    enc[-5:] = 255
    return enc


def _runs(n):
    """long homopolymer and period-3 runs between specials: LCPs up to
    thousands, every byte from 0 to 255 in .lcp"""
    parts = [np.zeros(6000, np.uint8), [254], np.tile(np.array([1, 2, 3], np.uint8), 3000), [255],
             np.zeros(2500, np.uint8), [254], synth.generate(synth.MODEL_UNIFORM_DNA, 5, n - 17503)]
    return np.concatenate([np.asarray(p, np.uint8) for p in parts])


def _text(name):
    """(encoded symbols, tables {suf, lcp, llv, bwt} as numpy)"""
    if name.startswith("fixture:"):
        fx = name.split(":", 1)[1]
        protein = ou.golden()[fx]["alphabet"] == "protein"
        enc = ou.encode_fasta(ou.fixture_path(fx), protein)
        t = {ext: ou.golden_table(fx, ext) for ext in ("suf", "lcp", "llv", "bwt")}
        t["llv"] = t["llv"].reshape(-1, 2)
        return enc, t
    model_of = {"uniform": synth.MODEL_UNIFORM_DNA, "humanlike": synth.MODEL_HUMANLIKE_DNA,
                "repeatheavy": synth.MODEL_REPEAT_HEAVY, "protein": synth.MODEL_PROTEIN}
    if name in model_of:
        enc = synth.generate(model_of[name], 43, 120_000)
        sigma = synth.numofchars(model_of[name])
    elif name == "specialheavy":
        enc, sigma = _special_heavy(32, 100_000), 4
    else:
        enc, sigma = _runs(60_000), 4
    return enc, ou.esa(enc, sigma)


@functools.lru_cache(maxsize=None)
def _case(name):
    enc, t = _text(name)
    return {"enc": torch.from_numpy(np.ascontiguousarray(enc)),
            "suf": torch.from_numpy(t["suf"].astype(np.int64)),
            "lcp": torch.from_numpy(np.array(t["lcp"])),
            "llv": torch.from_numpy(t["llv"].astype(np.int64).reshape(-1, 2)),
            "bwt": torch.from_numpy(np.array(t["bwt"])),
            "N": enc.size + 1, "specials": int(np.count_nonzero(enc >= 254))}


def _rng(name, what):
    return np.random.default_rng([sum(map(ord, name)), sum(map(ord, what))])


TEXTS = ["uniform", "humanlike", "repeatheavy", "protein", "specialheavy", "runs",
         "fixture:Atinsert.fna", "fixture:Duplicate.fna", "fixture:sw100K1.fsa"]
# the texts with LCPs of 254 and above (.llv entries)
LLV_TEXTS = ["humanlike", "repeatheavy", "runs", "fixture:Duplicate.fna"]


def _lcp_check(c, lcp=None, llv=None):
    llv = c["llv"] if llv is None else llv
    return dc.check_lcp_exact(c["suf"], c["enc"], c["lcp"] if lcp is None else lcp,
                              llv[:, 0].contiguous(), llv[:, 1].contiguous())


def _indices(c, rng, count):
    """table index 1, the first entry of the special tail and its last special,
    the entry of position n (N - 1), and `count` random indices >= 1"""
    N, sp = c["N"], c["specials"]
    edge = [1, N - 1] + ([N - 1 - sp, N - 2] if sp else [])
    return sorted(set(edge) | set(int(x) for x in rng.integers(1, N, count)))


@pytest.mark.parametrize("name", TEXTS)
def test_checkers_accept_the_tables(name):
    c = _case(name)
    rank, msg = dc.suffix_ranks(c["suf"])
    assert rank is not None, msg
    assert dc.check_suffix_array_exact(c["suf"], c["enc"], rank) == (True, "")
    assert dc.check_bwt_exact(c["suf"], c["enc"], c["bwt"]) == (True, "")
    idx, val = c["llv"][:, 0].contiguous(), c["llv"][:, 1].contiguous()
    assert dc.check_lcp_exact(c["suf"], c["enc"], c["lcp"], idx, val, rank) == (True, "")
    assert dc.check_llv_all(c["suf"], c["enc"], c["lcp"], idx, val) == (True, "")
    assert (c["llv"].shape[0] > 0) == (name in LLV_TEXTS)


@pytest.mark.parametrize("name", TEXTS)
def test_lcp_byte_off_by_one_is_rejected(name):
    c = _case(name)
    accepted, tried = [], 0
    for i in _indices(c, _rng(name, "lcp"), 40):
        b = int(c["lcp"][i])
        for d in (1, -1):
            if b == 255 or b + d < 0:
                continue
            lcp = c["lcp"].clone()
            lcp[i] = b + d
            tried += 1
            if _lcp_check(c, lcp=lcp)[0]:
                accepted.append((i, b, d))
    assert tried >= 40 and not accepted


@pytest.mark.parametrize("name", LLV_TEXTS)
def test_llv_value_off_by_one_is_rejected(name):
    c = _case(name)
    m = c["llv"].shape[0]
    accepted = []
    for k in sorted({0, m - 1} | set(int(x) for x in _rng(name, "llv").integers(0, m, 30))):
        for d in (1, -1):
            llv = c["llv"].clone()
            llv[k, 1] += d
            ok = _lcp_check(c, llv=llv)[0]
            ok_all = dc.check_llv_all(c["suf"], c["enc"], c["lcp"], llv[:, 0].contiguous(),
                                      llv[:, 1].contiguous())[0]
            if ok or ok_all:
                accepted.append((k, d, ok, ok_all))
    assert not accepted


@pytest.mark.parametrize("name", LLV_TEXTS)
def test_lcp_254_raised_with_an_llv_entry_is_rejected(name):
    c = _case(name)
    at = np.flatnonzero(c["lcp"].numpy() == 254)
    assert at.size > 0
    accepted = []
    for i in at[:20]:
        i = int(i)
        lcp = c["lcp"].clone()
        lcp[i] = 255
        k = int(torch.searchsorted(c["llv"][:, 0].contiguous(), torch.tensor(i)))
        llv = torch.cat([c["llv"][:k], torch.tensor([[i, 255]]), c["llv"][k:]])
        if _lcp_check(c, lcp=lcp, llv=llv)[0]:
            accepted.append(i)
    assert not accepted


@pytest.mark.parametrize("name", LLV_TEXTS)
def test_dropped_llv_entry_is_rejected(name):
    c = _case(name)
    m = c["llv"].shape[0]
    accepted = []
    for k in sorted({0, m - 1} | set(int(x) for x in _rng(name, "drop").integers(0, m, 10))):
        llv = torch.cat([c["llv"][:k], c["llv"][k + 1:]])
        if _lcp_check(c, llv=llv)[0]:
            accepted.append(k)
    assert not accepted


@pytest.mark.parametrize("name", TEXTS)
def test_swapped_suf_neighbours_are_rejected(name):
    c = _case(name)
    accepted = []
    for i in _indices(c, _rng(name, "swap"), 40):
        sa = c["suf"].clone()
        sa[i - 1], sa[i] = c["suf"][i], c["suf"][i - 1]
        if dc.check_suffix_array_exact(sa, c["enc"])[0]:
            accepted.append(i)
    assert not accepted


@pytest.mark.parametrize("name", TEXTS)
def test_duplicated_suf_entry_is_rejected(name):
    c = _case(name)
    accepted = []
    for i in _indices(c, _rng(name, "dup"), 20):
        for src in (i - 1, i):               # the entry before over this one, and back
            sa = c["suf"].clone()
            sa[2 * i - 1 - src] = c["suf"][src]
            if dc.check_suffix_array_exact(sa, c["enc"])[0]:
                accepted.append((i, src))
    assert not accepted


@pytest.mark.parametrize("name", TEXTS)
def test_changed_bwt_byte_is_rejected(name):
    c = _case(name)
    sigma = 20 if name in ("protein", "fixture:sw100K1.fsa") else 4
    accepted = []
    for i in [0] + _indices(c, _rng(name, "bwt"), 40):
        b = int(c["bwt"][i])
        for v in {(b + 1) % sigma if b < sigma else 0, 254 if b != 254 else 1}:
            bwt = c["bwt"].clone()
            bwt[i] = v
            if dc.check_bwt_exact(c["suf"], c["enc"], bwt)[0]:
                accepted.append((i, b, v))
    assert not accepted


# ---- check_esastats_exact: the .prj numbers at other alphabet sizes and prefix
# lengths, beyond the key width (20 symbols of the 2-bit keys) included
def _stats_text(sigma, seed):
    """letters with dense wildcard runs and separators (many suffixes with fewer
    letters than the prefix length in front of a special), long copies (.llv)"""
    rng = np.random.default_rng(seed)
    enc = rng.integers(0, sigma, 40_000).astype(np.uint8)
    enc[rng.random(enc.size) < 0.01] = 254
    for start in rng.integers(0, enc.size - 30, 60):
        enc[start:start + rng.integers(1, 30)] = 254
    enc[rng.random(enc.size) < 0.002] = 255
    enc[20_000:21_000] = enc[5_000:6_000]
    enc[30_000:30_600] = sigma - 1
    return enc


def _oracle_stats(enc, sigma, prefixlength):
    t = ou.esa(enc, sigma)
    st = ou.EsaStats()
    ou.lib().ora_esastats_compute(ou._p(enc), enc.size, ou._p(t["suf"]), ou._p(t["lcpfull"]),
                                  prefixlength, ctypes.byref(st))
    return t, {name: int(getattr(st, name)) for name, _ in st._fields_}


STATS_CASES = [(2, 0), (2, 1), (2, 20), (2, 21), (2, 40), (3, 14), (3, 21), (5, 9), (5, 11),
               (12, 4), (28, 5), (28, 12)]


@functools.lru_cache(maxsize=None)
def _stats_case(sigma, prefixlength):
    enc = _stats_text(sigma, 100 + sigma)
    t, st = _oracle_stats(enc, sigma, prefixlength)
    llv = torch.from_numpy(t["llv"].astype(np.int64).reshape(-1, 2))
    args = (torch.from_numpy(t["suf"].astype(np.int64)), torch.from_numpy(enc),
            torch.from_numpy(np.array(t["lcp"])), llv[:, 0].contiguous(), llv[:, 1].contiguous(),
            prefixlength)
    return args, st, t


@pytest.mark.parametrize("sigma,prefixlength", STATS_CASES)
def test_esastats_checker_accepts_the_oracle(sigma, prefixlength):
    args, st, t = _stats_case(sigma, prefixlength)
    assert st["largelcpvalues"] > 0
    assert dc.check_esastats_exact(*args, st) == (True, "")


@pytest.mark.parametrize("sigma,prefixlength", STATS_CASES)
def test_esastats_off_by_one_is_rejected(sigma, prefixlength):
    args, st, _ = _stats_case(sigma, prefixlength)
    for name in ("longest", "largelcpvalues", "maxbranchdepth", "lcptabsum"):
        for d in (1, -1):
            bad = dict(st)
            bad[name] += d
            ok, msg = dc.check_esastats_exact(*args, bad)
            assert not ok and msg.startswith(name), (name, d)


@pytest.mark.parametrize("sigma,prefixlength", [c for c in STATS_CASES if c[1] > 1])
def test_esastats_unmasked_sum_is_rejected(sigma, prefixlength):
    """a sum that also counts entries with fewer than prefixlength letters in
    front of a special -- all of them, or those one letter short (at prefix length
    1 the two agree: a suffix that starts with a special has LCP 0)"""
    args, st, t = _stats_case(sigma, prefixlength)
    for k in (0, prefixlength - 1):
        _, loose = _oracle_stats(args[1].numpy(), sigma, k)
        assert loose["lcptabsum"] > st["lcptabsum"], k
        ok, msg = dc.check_esastats_exact(*args, dict(st, lcptabsum=loose["lcptabsum"]))
        assert not ok and msg.startswith("lcptabsum"), k


# ---- check_packed_index_exact: INDEX.bdx images of the oracle (oracle/pck_oracle.c)
def _pck_alphabet_text(sigma, n, seed):
    """i.i.d. letters with wildcard runs, single wildcards and separators, a run
    at both ends"""
    rng = np.random.default_rng(seed)
    enc = rng.integers(0, sigma, n).astype(np.uint8)
    for start in rng.integers(0, n - 50, n // 500):
        enc[start:start + rng.integers(1, 50)] = 254
    enc[rng.random(n) < 0.01] = 254
    enc[rng.random(n) < 0.003] = 255
    enc[:3] = 254
    enc[-4:] = 254
    return enc


# name -> (encoded text, letters); N = n + 1 just below, at and just above a
# multiple of the default bucket length 64 for the special-heavy DNA texts
PCK_TEXTS = {
    "fixture:Atinsert.fna": None, "fixture:sw100K1.fsa": None,
    "special:64k-1": (lambda: _special_heavy(33, 64 * 1000 - 2), 4),
    "special:64k": (lambda: _special_heavy(34, 64 * 1000 - 1), 4),
    "special:64k+1": (lambda: _special_heavy(35, 64 * 1000), 4),
    "sigma20": (lambda: _pck_alphabet_text(20, 40_000, 36), 20),
    "sigma7": (lambda: _pck_alphabet_text(7, 50_001, 37), 7),
}
PCK_OPTIONS = [dict(), dict(locbitmap=True), dict(locfreq=0), dict(mkindex=True),
               dict(bsize=5, blbuck=3, locfreq=7),
               dict(bsize=16, blbuck=16, locfreq=32, locbitmap=True, mkindex=True)]


@functools.lru_cache(maxsize=None)
def _pck_tables(name):
    if name.startswith("fixture:"):
        fx = name.split(":", 1)[1]
        sigma = 20 if ou.golden()[fx]["alphabet"] == "protein" else 4
        enc = ou.encode_fasta(ou.fixture_path(fx), sigma == 20)
    else:
        make, sigma = PCK_TEXTS[name]
        enc = make()
    t = ou.esa(enc, sigma)
    return enc, sigma, t["suf"], np.array(t["bwt"])


@functools.lru_cache(maxsize=None)
def _pck_case(name, opts):
    enc, sigma, suf, bwt = _pck_tables(name)
    kw = dict(opts)
    img = ou.pck_bdx(enc, sigma, suf, bwt, **kw)
    return (torch.frombuffer(bytearray(img), dtype=torch.uint8), torch.from_numpy(bwt),
            torch.from_numpy(suf.astype(np.int64)), sigma, kw)


PCK_CHUNK = 1000          # table entries per step: every text takes several


def _pck_check(img, bwt, suf, sigma, kw, **extra):
    return dc.check_packed_index_exact(img, bwt, suf, sigma, chunk=PCK_CHUNK, **kw, **extra)


@pytest.mark.parametrize("opts", [tuple(sorted(o.items())) for o in PCK_OPTIONS],
                         ids=["-".join("%s=%s" % kv for kv in sorted(o.items())) or "default"
                              for o in PCK_OPTIONS])
@pytest.mark.parametrize("name", list(PCK_TEXTS))
def test_packed_index_checker_accepts_the_oracle(name, opts):
    img, bwt, suf, sigma, kw = _pck_case(name, opts)
    rep = {}
    assert _pck_check(img, bwt, suf, sigma, kw, report=rep) == (True, "")
    L = kw.get("bsize", 8) * kw.get("blbuck", 8)
    N = bwt.numel()
    assert rep["buckets"] == (N + L) // L
    assert rep["regions"] > 1
    # several chunks, the carries between them included
    assert N > 4 * PCK_CHUNK


def test_packed_index_checker_covers_the_bucket_borders():
    """the special-heavy texts end one entry before, on and one entry behind a
    multiple of the bucket length"""
    assert [(_pck_tables(n)[0].size + 1) % 64 for n in ("special:64k-1", "special:64k",
                                                       "special:64k+1")] == [63, 0, 1]


@pytest.mark.parametrize("sigma,B", [(4, 8), (4, 1), (2, 16), (5, 6), (20, 3), (28, 3)])
def test_block_ranks_invert_unrank(sigma, B):
    """every block of the geometry: unrank_block (gt_block2IndexPair inverted by
    enumeration) takes the ranks back to the block; the permutation index lies
    below the arrangements of the composition and takes bits(arrangements - 1) bits"""
    from math import comb
    codes = torch.arange(sigma ** B, dtype=torch.int64)
    blocks = torch.stack([(codes // sigma ** (B - 1 - i)) % sigma for i in range(B)], 1)
    comp, perm, pbits = dc.block_ranks(blocks, sigma)
    assert int(comp.min()) == 0 and int(comp.max()) == comb(B + sigma - 1, sigma - 1) - 1
    bad = []
    for blk, c, p, pb in zip(blocks.tolist(), comp.tolist(), perm.tolist(), pbits.tolist()):
        back, arrangements = dc.unrank_block(c, p, sigma, B)
        ways = arrangements([blk.count(s) for s in range(sigma)])
        if back != blk or p >= ways or pb != (ways - 1).bit_length():
            bad.append((blk, c, p, pb))
    assert not bad[:5]


def test_packed_index_checker_refuses_sprank():
    img, bwt, suf, sigma, kw = _pck_case("special:64k", ())
    with pytest.raises(ValueError, match="sprank"):
        dc.check_packed_index_exact(img, bwt, suf, sigma, sprank=True)


def _flip(img, bit):
    out = img.clone()
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return out


def _pck_fields(name, opts):
    """the oracle's image and the bit positions of one field of each kind"""
    img, bwt, suf, sigma, kw = _pck_case(name, opts)
    raw = img.numpy().tobytes()
    N = bwt.numel()
    letters = [int((bwt == s).sum()) for s in range(sigma)]
    ly = dc.pck_layout(N, sigma, letters, **kw)

    def rec(j):
        return 8 * ly["cw_data_pos"] + j * ly["cw_bits"]

    def var_at(j):
        return 8 * ly["var_data_pos"] + dc.read_bits(raw, rec(j) + ly["pre_var_idx"], ly["var_off_bits"])
    return img, bwt, suf, sigma, kw, raw, ly, rec, var_at


def _low(at, width):
    """the last (least significant) bit of a field"""
    return at + width - 1


PCK_REJECT = "special:64k+1"


def _expect_rejected(args, bit, words, bucket=None):
    img, bwt, suf, sigma, kw = args
    ok, msg = _pck_check(_flip(img, bit), bwt, suf, sigma, kw)
    assert not ok, (bit, words)
    assert words in msg, msg
    if bucket is not None:
        assert msg.startswith("bucket %d:" % bucket), msg


def test_packed_index_flipped_counters_are_rejected():
    img, bwt, suf, sigma, kw, raw, ly, rec, _ = _pck_fields(PCK_REJECT, ())
    args = (img, bwt, suf, sigma, kw)
    nb = ly["nb"]
    for j, s in ((0, 0), (0, 3), (nb - 1, 1), (nb - 1, 2), (nb // 2, 0)):
        _expect_rejected(args, _low(rec(j) + ly["sym_off"][s], ly["sym_bits"][s]),
                         "occurrence counter of letter %d" % s, j)
    # the top bit of a counter
    _expect_rejected(args, rec(nb - 1) + ly["sym_off"][3], "occurrence counter of letter 3", nb - 1)


def test_packed_index_flipped_bucket_fields_are_rejected():
    img, bwt, suf, sigma, kw, raw, ly, rec, var_at = _pck_fields(PCK_REJECT, ())
    args = (img, bwt, suf, sigma, kw)
    nb = ly["nb"]
    for j in (1, nb // 3, nb - 1):
        _expect_rejected(args, _low(rec(j) + ly["pre_var_idx"], ly["var_off_bits"]), "var offset", j)
        _expect_rejected(args, _low(rec(j) + ly["pre_cb_off"], ly["cb_off_bits"]),
                         "bits of the permutation indices", j)
    for j, b in ((0, 0), (nb // 2, 7), (nb - 1, 0)):
        _expect_rejected(args, _low(rec(j) + ly["pre_comp_idx"] + b * ly["comp_idx_bits"],
                                    ly["comp_idx_bits"]), "composition index of block %d" % b, j)
    # a permutation bit: the first block with a permutation index of a bucket
    for j in (0, nb // 2, nb - 2):
        blocks = bwt[j * 64:(j + 1) * 64].to(torch.int64).view(8, 8)
        _, _, pbits = dc.block_ranks(torch.where(blocks >= 254, 0, blocks), sigma)
        b = int(torch.nonzero(pbits).flatten()[0])
        at = var_at(j) + int(pbits[:b].sum())
        for bit in (at, at + int(pbits[b]) - 1):
            _expect_rejected(args, bit, "permutation index of block %d" % b, j)


def test_packed_index_flipped_marks_are_rejected():
    img, bwt, suf, sigma, kw, raw, ly, rec, var_at = _pck_fields(PCK_REJECT, ())
    args = (img, bwt, suf, sigma, kw)
    assert ly["count"]
    nb = ly["nb"]
    for j in (0, nb // 2, nb - 2):
        at = var_at(j) + dc.read_bits(raw, rec(j) + ly["pre_cb_off"], ly["cb_off_bits"])
        nm = dc.read_bits(raw, at, 7)
        assert nm > 1
        _expect_rejected(args, _low(at, 7), "mark count", j)
        row = at + 7
        _expect_rejected(args, _low(row, 6), "row of mark 0", j)
        _expect_rejected(args, _low(row + 6, ly["bits_orig_pos"]), "text position of mark 0", j)
        last = row + (nm - 1) * (6 + ly["bits_orig_pos"])
        _expect_rejected(args, last, "row of mark %d" % (nm - 1), j)
        _expect_rejected(args, last + 6, "text position of mark %d" % (nm - 1), j)


def test_packed_index_flipped_bitmap_bits_are_rejected():
    opts = (("locbitmap", True),)
    img, bwt, suf, sigma, kw, raw, ly, rec, var_at = _pck_fields(PCK_REJECT, opts)
    args = (img, bwt, suf, sigma, kw)
    assert ly["bitmap"]
    nb = ly["nb"]
    N = bwt.numel()
    for j, i in ((0, 0), (nb // 2, 17), (nb - 1, N - 1 - (nb - 1) * 64)):
        _expect_rejected(args, rec(j) + ly["pre_cw_ext"] + i, "locate bit of row %d" % i, j)
    # a text position in the var part
    j = nb // 2
    at = var_at(j) + dc.read_bits(raw, rec(j) + ly["pre_cb_off"], ly["cb_off_bits"])
    _expect_rejected(args, _low(at, ly["bits_orig_pos"]), "text position of mark 0", j)


def test_packed_index_flipped_regions_header_and_size_are_rejected():
    img, bwt, suf, sigma, kw, raw, ly, rec, var_at = _pck_fields(PCK_REJECT, ())
    args = (img, bwt, suf, sigma, kw)
    roff = struct.unpack_from("<Q", raw, 40)[0]
    nr = struct.unpack_from("<Q", raw, roff)[0]
    assert nr > 100
    for r in (0, nr // 2, nr - 1):
        base = 8 * (roff + 8 + 16 * r)
        for bit in (base + 3, base + 64, base + 127):     # start, symbol, length
            _expect_rejected(args, bit, "region record %d" % r)
    _expect_rejected(args, 8 * roff + 7, "region list")
    # header: block size, sequence length, var offset bits, a counter width, the
    # locate interval, the padding
    for at, what in ((12 * 8 + 7, "block size"), (52 * 8 + 7, "sequence length"),
                     (72 * 8 + 7, "var offset bits"), (84 * 8 + 7, "counter bits of letter 0"),
                     (8 * (ly["header_len"] + 16) + 7, "locate interval"),
                     (8 * (ly["cw_data_pos"] - 1), "byte %d before the first record" % (ly["cw_data_pos"] - 1))):
        _expect_rejected(args, at, "header: " + what)
    ok, msg = _pck_check(img[:-1], bwt, suf, sigma, kw)
    assert not ok and msg.startswith("image is"), msg
    ok, msg = _pck_check(torch.cat([img, torch.zeros(1, dtype=torch.uint8)]), bwt, suf, sigma, kw)
    assert not ok and msg.startswith("image is"), msg
