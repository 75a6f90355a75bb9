"""BASELINE.json sizes, checked through size-independent properties (the CPU
oracle's comparison sort cannot run at these sizes):

* configs[1], 256 Mbp uniform DNA: the suffix array passes the linear-time
  checker (permutation + sortedness, oracle/esa_oracle.c ora_check_suffix_array)
  and LCP/BWT equal the tables the oracle derives from that suffix array
  (Kasai).  Together that is bit-exactness of all three tables.
* configs[2], 3 Gbp human-like DNA (the bench workload), and the repeat-heavy
  model at 3 Gbp: every table EXACTLY on the device (tests/device_check.py) --
  the suffix table as a permutation whose every neighbour pair is ordered by
  (first symbol, rank of the successor), .lcp with .llv by Kasai's inheritance
  argument, .bwt entry by entry --, every .llv entry probed once more, the tail
  layout (specials in text order, then n) and the .prj statistics.
* configs[4], 10^9 protein residues: the same exact checks on the 5-bit path.
* the position range of configs[3] (n >= 2^32; the 24 Gbp input itself needs
  the 8 GPUs it is defined on): 2^32 + 4 M bases of uniform DNA built in two
  parts on the one GPU, 64-bit positions and ranks; both slices put together
  and checked exactly.
* the largest single build, SINGLE_LIMIT - 1 entries (k_win_filter's window
  bitmap in global memory), exactly; one entry more is refused.
* the packed index (INDEX.bdx) of 10^9 and 3 * 10^9 human-like bases, of 10^9
  protein residues in the largest block size the builder takes for 20 letters,
  in a non-default geometry, and of made-up tables past 2^32 entries whose
  counters and var offsets pass 2^32: every field of every bucket, the header
  and the region list exact on the device (check_packed_index_exact).
"""
import numpy as np
import pytest
import torch

import engine_paths
import oracle_util as ou
from genometools_amd import _lib, esa, synth

pytestmark = pytest.mark.gpu


def _device_sequence(model, seed, n):
    lib = _lib.load()
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, model, seed, n, buf.data_ptr()))
    torch.cuda.synchronize()
    return buf


class _Wrap:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr,
                                         "data": (ptr, False), "version": 2}


def test_config1_256mbp_uniform_bit_exact(gpu):
    n = 256 * 1000 * 1000
    buf = _device_sequence(synth.MODEL_UNIFORM_DNA, 42, n)
    with esa.EsaEngine(n, 4) as eng:
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run()
        res = eng.result()
    enc = buf.cpu().numpy()
    del buf
    rc, where = ou.check_suffix_array(enc, res.suf)
    assert rc == 0, (rc, where)
    t = ou.tables_given_sa(enc, res.suf)
    assert np.array_equal(res.lcp, t["lcp"])
    assert np.array_equal(res.llv, t["llv"])
    assert np.array_equal(res.bwt, t["bwt"])
    assert res.stats["maxbranchdepth"] == int(t["lcpfull"].max())
    assert res.stats["largelcpvalues"] == len(t["llv"])
    # the device generator and the numpy definition of the model agree
    assert np.array_equal(enc[:1 << 20], synth.generate(synth.MODEL_UNIFORM_DNA, 42, n, 0, 1 << 20))


def _check_tables(sa, enc, lcp, bwt, llv_idx, llv_val):
    """the four exact checks of tests/device_check.py, one rank table for two of them"""
    import device_check as dc
    rank, msg = dc.suffix_ranks(sa)
    assert rank is not None, msg
    ok, msg = dc.check_suffix_array_exact(sa, enc, rank)
    assert ok, msg
    ok, msg = dc.check_lcp_exact(sa, enc, lcp, llv_idx, llv_val, rank)
    assert ok, msg
    del rank
    ok, msg = dc.check_bwt_exact(sa, enc, bwt)
    assert ok, msg
    ok, msg = dc.check_llv_all(sa, enc, lcp, llv_idx, llv_val)
    assert ok, msg
    torch.cuda.empty_cache()        # (the next engine allocates outside torch)


def _check_tail_and_prj(sa, enc, lcp, llv_val, st):
    """the special tail (every suffix that starts with a special, in text order,
    then n) and the statistics of .prj that follow from the tables"""
    import device_check as dc
    N = sa.numel()
    n = N - 1
    assert int(sa[st["longest"]].item()) == 0
    specials = int((enc >= 254).sum().item())
    tail = sa[N - 1 - specials:]
    assert int(tail[-1].item()) == n
    assert bool((enc[tail[:-1]] >= 254).all()) and bool((tail[1:] > tail[:-1]).all())
    assert int(enc[sa[N - 2 - specials]].item()) < 254
    assert bool((lcp[N - specials:] == 0).all())
    nl = llv_val.numel()
    assert nl == st["largelcpvalues"] == dc.count_lcp_overflows(lcp)
    assert nl == 0 or int(llv_val.max().item()) == st["maxbranchdepth"]


def _device_tables(eng, N):
    import device_check as dc
    nl = eng.entries(esa.TAB_LLV)
    llv = (dc.as_tensor(eng.device_pointer(esa.TAB_LLV), 2 * nl, "<i8") if nl else
           torch.empty(0, dtype=torch.int64, device="cuda:0")).view(-1, 2)
    return (dc.as_tensor(eng.device_pointer(esa.TAB_SUF), N, "<i8"),
            dc.as_tensor(eng.device_pointer(esa.TAB_LCP), N, "|u1"),
            dc.as_tensor(eng.device_pointer(esa.TAB_BWT), N, "|u1"),
            llv[:, 0].contiguous(), llv[:, 1].contiguous())


def _tables_to_host(engines):
    """the slices of .suf, .lcp, .bwt and .llv of `engines` (the parts of one
    build, or one whole build) in host memory, so that the engines can be closed
    before the tables return to the device for the checks: the engine's workspace
    and the checks' rank table do not fit the device together at these sizes"""
    return [(eng.table_offset(), eng.table(esa.TAB_SUF).view(np.int64), eng.table(esa.TAB_LCP),
             eng.table(esa.TAB_BWT), eng.table(esa.TAB_LLV).view(np.int64)) for eng in engines]


def _tables_to_device(slices, N):
    """whole-table device tensors (sa, lcp, bwt, llv_idx, llv_val) from the
    slices of _tables_to_host; .llv indices count from the start of the whole
    table (k_llv_emit adds the slice's table offset)"""
    dev = "cuda:0"
    sa = torch.empty(N, dtype=torch.int64, device=dev)
    lcp = torch.empty(N, dtype=torch.uint8, device=dev)
    bwt = torch.empty(N, dtype=torch.uint8, device=dev)
    for off, suf, lc, bw, _ in slices:
        sa[off:off + suf.size].copy_(torch.from_numpy(suf))
        lcp[off:off + suf.size].copy_(torch.from_numpy(lc))
        bwt[off:off + suf.size].copy_(torch.from_numpy(bw))
    llv = torch.from_numpy(np.concatenate([sl[4] for sl in slices])).to(dev)
    return sa, lcp, bwt, llv[:, 0].contiguous(), llv[:, 1].contiguous()


def test_config2_3gbp_humanlike_exact(gpu):
    """BASELINE.json configs[2], the bench workload, with the switches the bench
    runs with (none).  Every table EXACTLY, on the device (tests/device_check.py):
    the suffix table by the reference's lightweight check restated -- a
    permutation whose every neighbour pair is ordered by (first symbol, rank of the
    successor) is the sorted table --, .lcp and .llv by Kasai's inheritance
    argument turned into a check, .bwt for every entry, and every one of the 117 M
    .llv entries once more (mismatch right behind its value, agreement at its last
    and at 16 random offsets); the tail; the statistics of .prj from the tables."""
    n = 3 * 1000 * 1000 * 1000
    N = n + 1
    buf = _device_sequence(synth.MODEL_HUMANLIKE_DNA, 43, n)
    with esa.EsaEngine(n, 4) as eng:
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run()
        st = eng.stats()
        assert st["msd_big_entries"] > 0 and st["pair_suffixes"] > 3e8 and st["refine_rounds"] >= 9
        sa, lcp, bwt, llv_idx, llv_val = _device_tables(eng, N)
        assert llv_idx.numel() > 10 ** 8
        _check_tables(sa, buf, lcp, bwt, llv_idx, llv_val)
        _check_tail_and_prj(sa, buf, lcp, llv_val, st)


def test_repeatheavy_3gbp_exact(gpu):
    """MODEL_REPEAT_HEAVY at 3 Gbp: the hard case of prefix doubling (14 rounds,
    393 M .llv entries, LCPs up to 255 865), every table exact"""
    n = 3 * 1000 * 1000 * 1000
    N = n + 1
    buf = _device_sequence(synth.MODEL_REPEAT_HEAVY, 43, n)
    with esa.EsaEngine(n, 4) as eng:
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run()
        st = eng.stats()
        assert st["refine_rounds"] >= 12
        sa, lcp, bwt, llv_idx, llv_val = _device_tables(eng, N)
        assert llv_idx.numel() > 3 * 10 ** 8 and st["maxbranchdepth"] > 10 ** 5
        _check_tables(sa, buf, lcp, bwt, llv_idx, llv_val)
        _check_tail_and_prj(sa, buf, lcp, llv_val, st)


def _sampled_neighbours(eng, enc_of, n, lo, hi, rng, samples, index_offset=0, wildcard_ok=True):
    """order, LCP byte and BWT byte of `samples` neighbour pairs of the table
    slice held by `eng`, re-derived on the CPU; enc_of(a, b) delivers the
    encoded symbols [a, b)"""
    bad = 0
    for i in np.sort(rng.integers(lo, hi, samples)):
        i = int(i)
        p, q = (int(x) for x in eng.table(esa.TAB_SUF, i - 1, 2))
        lcpb = int(eng.table(esa.TAB_LCP, i, 1)[0])
        bwtb = int(eng.table(esa.TAB_BWT, i, 1)[0])
        span = 64
        while True:
            a, b = enc_of(p, min(n, p + span)), enc_of(q, min(n, q + span))
            m = min(len(a), len(b))
            neq = np.nonzero((a[:m] != b[:m]) | (a[:m] >= 254))[0]
            if len(neq) or m < span:
                l = int(neq[0]) if len(neq) else m
                break
            span *= 8
        ca = a[l] if l < len(a) else 255
        cb = b[l] if l < len(b) else 255
        ka = 256 + p + l if ca >= 254 else int(ca)
        kb = 256 + q + l if cb >= 254 else int(cb)
        bw = 254 if q == 0 else int(enc_of(q - 1, q)[0])
        bad += not (ka < kb and lcpb == min(l, 255) and bwtb == bw)
    return bad


def test_config4_protein_1g_exact(gpu):
    """BASELINE.json configs[4]: 10^9 residues over the 20-letter alphabet
    (src/core/alphabet.c:488-503), -suf -lcp (+ -bwt): the 5-bit symbol path at
    full size (7 sort passes, N/12 word indexing), every table exact on the device"""
    n = 1000 * 1000 * 1000
    N = n + 1
    buf = _device_sequence(synth.MODEL_PROTEIN, 44, n)
    with esa.EsaEngine(n, 20) as eng:
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run()
        st = eng.stats()
        assert st["prefixlength"] == 5
        sa, lcp, bwt, llv_idx, llv_val = _device_tables(eng, N)
        _check_tables(sa, buf, lcp, bwt, llv_idx, llv_val)
        assert int(sa[st["longest"]].item()) == 0
        del sa
        enc = buf.cpu().numpy()
        del buf
        torch.cuda.empty_cache()
        specials = int(np.count_nonzero(enc >= 254))
        assert specials > 2_000_000          # ~3 M sequence borders + X
        # tail: separators and X in text order, then n
        tail = eng.table(esa.TAB_SUF, N - 1 - specials, specials + 1)
        assert tail[-1] == n
        assert np.all(enc[tail[:-1].astype(np.int64)] >= 254)
        assert np.all(np.diff(tail[:-1].astype(np.int64)) > 0)
        before_tail = eng.table(esa.TAB_SUF, N - 2 - specials, 1)[0]
        assert enc[int(before_tail)] < 254
        # i.i.d. residues: no LCP near the byte limit
        assert st["largelcpvalues"] == 0 and st["maxbranchdepth"] < 64
        lcp = eng.table(esa.TAB_LCP)
        assert int(lcp.max()) == st["maxbranchdepth"]
        assert np.all(lcp[N - 1 - specials + 1:] == 0)
        # averagelcp of .prj: entries with >= prefixlength letters;
        # an upper bound here, the exact mask is checked at oracle sizes
        assert 0 < st["lcptabsum"] <= int(lcp.sum(dtype=np.uint64))


def test_positions_beyond_2p32_in_two_parts(gpu):
    """n just above 2^32 (the position range BASELINE.json configs[3], 24 Gbp
    on 8 GPUs, needs): two parts as threads on the one GPU, 64-bit positions
    and ranks; the slices of both parts checked on the device and by samples,
    then put together and every table checked exactly"""
    import threading
    from thread_comm import ThreadComm
    n = (1 << 32) + (1 << 22) + 12345
    N = n + 1
    seed = 45
    buf = _device_sequence(synth.MODEL_UNIFORM_DNA, seed, n)
    shared = ThreadComm(2, 0)
    engines = [esa.EsaEngine(n, 4) for _ in range(2)]
    errors = []

    def worker(r):
        try:
            eng = engines[r]
            eng.set_sequence_device(buf.data_ptr(), n)
            eng.set_part(r, 2, shared.view(r))
            eng.run()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))
            shared.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors
        del buf
        torch.cuda.empty_cache()

        def enc_of(a, b):
            return synth.generate(synth.MODEL_UNIFORM_DNA, seed, n, a, b)

        total, sq, top = 0, 0, 0
        offs = []
        rng = np.random.default_rng(7)
        for r, eng in enumerate(engines):
            cnt, off = eng.entries(esa.TAB_SUF), eng.table_offset()
            offs.append((off, cnt))
            st = eng.stats()
            sa = torch.as_tensor(_Wrap(eng.device_pointer(esa.TAB_SUF), cnt, "<i8"), device="cuda:0")
            total += int(sa.sum().item())            # (below 2^63 for each slice?  no: mod 2^64)
            sq += int((sa * sa).sum().item())
            top = max(top, int(sa.max().item()))
            del sa
            assert st["tied_suffixes"] > 0           # random 20-mers collide at this size
            assert _sampled_neighbours(eng, enc_of, n, 1, cnt - (1 if r == 1 else 0), rng, 1500) == 0
        assert offs[0][0] == 0 and offs[1][0] == offs[0][1] and offs[1][0] + offs[1][1] == N
        assert abs(offs[0][1] - offs[1][1]) < N // 50          # even ranges
        assert total % (1 << 64) == (N * (N - 1) // 2) % (1 << 64)
        assert sq % (1 << 64) == ((N - 1) * N * (2 * N - 1) // 6) % (1 << 64)
        assert top == n                               # the virtual end, a position >= 2^32
        # the border between the slices is in order too
        p = int(engines[0].table(esa.TAB_SUF, offs[0][1] - 1, 1)[0])
        q = int(engines[1].table(esa.TAB_SUF, 0, 1)[0])
        a, b = enc_of(p, min(n, p + 64)), enc_of(q, min(n, q + 64))
        m = min(len(a), len(b))
        d = int(np.nonzero(a[:m] != b[:m])[0][0])
        assert a[d] < b[d]
        assert int(engines[1].table(esa.TAB_LCP, 0, 1)[0]) == d
        # every entry: both slices as one table, checked once the engines are closed
        slices = _tables_to_host(engines)
        for eng in engines:
            eng.close()
        tables = _tables_to_device(slices, N)
        del slices
        buf = _device_sequence(synth.MODEL_UNIFORM_DNA, seed, n)
        _check_tables(tables[0], buf, *tables[1:])
    finally:
        for eng in engines:
            eng.close()


SINGLE_LIMIT = (1 << 32) - 4096     # table entries of a single build (esa_engine.hip)


def test_single_build_at_the_32bit_limit(gpu):
    """the largest single build, N = SINGLE_LIMIT - 1 entries of human-like DNA:
    32-bit ranks and compact positions at their largest, and the window bitmap
    of k_win_filter too large for the LDS, read from global memory.  Every table
    exact.  One symbol more is refused with the advice to build in parts."""
    import device_check as dc
    n = SINGLE_LIMIT - 2
    N = n + 1
    with esa.EsaEngine(n + 1, 4) as eng:
        buf = _device_sequence(synth.MODEL_HUMANLIKE_DNA, 46, n + 1)
        eng.set_sequence_device(buf.data_ptr(), n + 1)
        with pytest.raises(esa.EsaError, match="build it in parts"):
            eng.run()
        del buf
        torch.cuda.empty_cache()
        buf = _device_sequence(synth.MODEL_HUMANLIKE_DNA, 46, n)
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run()
        st = eng.stats()
        free, total = torch.cuda.mem_get_info()
        print("after the build: %.1f of %.1f GB free" % (free / 1e9, total / 1e9))
        assert eng.table_offset() == 0 and eng.entries(esa.TAB_SUF) == N
        # k_win_filter keeps the bitmap of the selected rank windows (2^13
        # positions each) in LDS while (words + 4) * 5 <= 60 KB; this build is past
        # that, and it built only the selected windows, so the filter ran on the
        # bitmap in global memory
        words = -(-N // (1 << 13)) // 32 + 2
        assert (words + 4) * 5 > 60 * 1024
        assert 0 < st["rank_entries_built"] < N
        slices = _tables_to_host([eng])
    tables = _tables_to_device(slices, N)
    del slices
    _check_tables(tables[0], buf, *tables[1:])
    _check_tail_and_prj(tables[0], buf, tables[1], tables[4], st)
    assert tables[4].numel() > 10 ** 7


# ---- the packed index at sizes the oracle cannot reach: every field of every bucket
def _check_packed_index(builder, bwt, suf, sigma, what, **kw):
    """check_packed_index_exact (tests/device_check.py) of the builder's image,
    on the device, against the tables it was built from: header, every bucket's
    counters, var offset, index bits, composition and permutation indices and
    locate marks, the region list, the size.  Prints what it checked and the
    time the check took."""
    import time
    import device_check as dc
    inf = builder.info()
    img = dc.as_tensor(builder.device_pointer(), inf["file_bytes"], "|u1")
    rep = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ok, msg = dc.check_packed_index_exact(img, bwt, suf, sigma, report=rep, **kw)
    torch.cuda.synchronize()
    print("%s: %d buckets checked in %.1f s; largest counter %d, largest var offset %d bits; "
          "%d regions; image %.2f GB built in %.1f ms" % (
              what, rep.get("buckets", -1), time.perf_counter() - t0, rep.get("max_counter", -1),
              rep.get("max_var_offset", -1), rep.get("regions", -1), inf["file_bytes"] / 1e9,
              inf["build_ms"]))
    assert ok, msg
    assert rep["buckets"] == inf["num_buckets"] and rep["regions"] == inf["num_regions"]
    assert rep["var_bits"] == inf["var_bits"]
    torch.cuda.empty_cache()
    return rep


def _esa_bwt_suf(eng, N):
    import device_check as dc
    return (dc.as_tensor(eng.device_pointer(esa.TAB_BWT), N, "|u1"),
            dc.as_tensor(eng.device_pointer(esa.TAB_SUF), N, "<i8"))


def _packed_index_of(model, seed, n, sigma, what, **kw):
    """INDEX.bdx of n symbols of a model, built from the resident tables and
    checked exactly; returns the check's report"""
    from genometools_amd import pck
    buf = _device_sequence(model, seed, n)
    with esa.EsaEngine(n, sigma) as eng, pck.PackedIndex() as builder:
        eng.set_sequence_device(buf.data_ptr(), n)
        del buf
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        builder.build_from_esa(eng, **kw)
        return _check_packed_index(builder, *_esa_bwt_suf(eng, n + 1), sigma, what, **kw)


def test_packed_index_of_a_1gbp_sequence_decodes_to_the_bwt(gpu):
    """INDEX.bdx of 10^9 bases (human-like model: wildcard runs, separators) with
    the default options, built from the resident tables: every one of the 15.6 M
    buckets decodes -- occurrence counters, var offset, composition and
    permutation index of every block, locate marks -- to the .bwt and .suf tables
    the image was made from; the region list is the list of the runs of specials
    in the BWT; sizes add up"""
    rep = _packed_index_of(synth.MODEL_HUMANLIKE_DNA, 43, 10 ** 9, 4, "1 Gbp human-like")
    assert rep["buckets"] == (10 ** 9 + 2 + 63) // 64
    assert rep["regions"] > 1000 and rep["max_counter"] > 2 * 10 ** 8


def test_packed_index_of_a_1gbp_sequence_in_another_geometry(gpu):
    """the same 10^9 bases in blocks of 16 (too many for the block table: the
    indices computed per block), 16 blocks per bucket, a mark every 32 positions
    as a bitmap, with sequence statistics (mkindex: counters as wide as each
    letter's total), every field exact"""
    rep = _packed_index_of(synth.MODEL_HUMANLIKE_DNA, 43, 10 ** 9, 4, "1 Gbp human-like, 16x16/32 bitmap mkindex",
                           bsize=16, blbuck=16, locfreq=32, locbitmap=True, mkindex=True)
    assert rep["buckets"] == (10 ** 9 + 2 + 255) // 256


def test_packed_index_of_config2_3gbp_exact(gpu):
    """BASELINE.json configs[2], the 3 Gbp human-like sequence of the bench, with
    the default options: every field of the 47 M buckets exact"""
    rep = _packed_index_of(synth.MODEL_HUMANLIKE_DNA, 43, 3 * 10 ** 9, 4, "3 Gbp human-like")
    assert rep["max_var_offset"] > 1 << 32


def test_packed_index_of_config4_protein_1g_exact(gpu):
    """BASELINE.json configs[4], 10^9 residues over 20 letters, in blocks of 6: the
    largest block size whose composition indices (C(25, 19) = 177 100 of them) fit
    the builder's 18 bits -- 7 letters per block is refused --, indices computed
    per block (20^6 blocks are too many for the table); every field exact"""
    from genometools_amd import pck
    n = 10 ** 9
    buf = _device_sequence(synth.MODEL_PROTEIN, 44, n)
    with esa.EsaEngine(n, 20) as eng, pck.PackedIndex() as builder:
        eng.set_sequence_device(buf.data_ptr(), n)
        del buf
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        with pytest.raises(esa.EsaError, match="needs wider indices"):
            builder.build_from_esa(eng, bsize=7)
        builder.build_from_esa(eng, bsize=6)
        rep = _check_packed_index(builder, *_esa_bwt_suf(eng, n + 1), 20, "1 G protein, blocks of 6",
                                  bsize=6)
    assert rep["buckets"] == (n + 2 + 47) // 48 and rep["regions"] > 10 ** 6


def test_packed_index_beyond_2p32_positions(gpu):
    """more than 2^32 table entries: tables made up on the device (the builder
    takes any .bwt / .suf pair) with 97 % of the BWT letter 0, so that letter's
    33-bit counters pass 2^32 in the last sixth of the buckets, and var offsets
    beyond 2^32 bits; every field of the image exact"""
    from genometools_amd import pck
    N = 5 * (1 << 30) + 7
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    bwt = torch.empty(N, dtype=torch.uint8, device=dev)
    suf = torch.empty(N, dtype=torch.int64, device=dev)
    step = 1 << 28
    for o in range(0, N, step):
        m = min(step, N - o)
        x = torch.randint(1, 4, (m,), dtype=torch.uint8, device=dev, generator=g)
        u = torch.rand(m, device=dev, generator=g)
        x[u < 0.97] = 0
        x[u >= 0.99] = 254
        x[u >= 0.998] = 255
        bwt[o:o + m] = x
        i = torch.arange(o, o + m, dtype=torch.int64, device=dev)
        suf[o:o + m] = (i * 11400714819 + 12345) % N          # any values below N do
        del x, u, i
    with pck.PackedIndex() as builder:
        builder.build(bwt.data_ptr(), suf.data_ptr(), N, 4, 5)
        rep = _check_packed_index(builder, bwt, suf, 4, "2^32 + made-up tables", longest=5)
    assert rep["max_counter"] >= 1 << 32 and rep["max_var_offset"] >= 1 << 32
    assert rep["var_bits"] > 1 << 32


# ---------------------------------------------------------------------------
# alphabets other than DNA and protein at the sizes where the prefix length, and
# with it the path, changes: 2 and 3 letters through the DNA kernels, 5 letters on
# either side of the 5-bit MSD sort's limit (prefixlength 9), 28 letters (largest
# codes, LSD sort), and 2 and 5 letters on either side of the key width (20 and 10
# symbols): beyond it lcptabsum and .bck read the text past the key
# ---------------------------------------------------------------------------
def _alphabet_text(sigma, n, seed, copies=False):
    """i.i.d. letters (numpy, fixed seed) with wildcard runs, single wildcards and
    separators; `copies`: 5 kb blocks copied elsewhere, ties far past the key"""
    rng = np.random.default_rng(seed)
    enc = rng.integers(0, sigma, n, dtype=np.uint8)
    for p in rng.integers(0, n - 1000, n // 100_000):
        enc[p:p + int(rng.integers(1, 1000))] = 254
    enc[rng.integers(0, n, n // 50_000)] = 254
    enc[rng.integers(0, n, n // 200_000)] = 255
    if copies:
        for src, dst in rng.integers(0, n - 5000, (400, 2)):
            enc[dst:dst + 5000] = enc[src:src + 5000]
    return torch.from_numpy(enc).to("cuda:0")


ALPHABET_SIZES = [(2, 67_108_847, 20, True), (2, 67_108_848, 21, True), (3, 1 << 28, 14, False),
                  (5, 195_312_495, 9, False), (5, 195_312_496, 10, False),
                  (5, 976_562_496, 11, False), (28, 300_000_000, 5, False)]


@pytest.mark.parametrize("sigma,n,prefixlength,copies", ALPHABET_SIZES,
                         ids=["sigma%d_n%d" % (c[0], c[1]) for c in ALPHABET_SIZES])
def test_alphabet_at_size_exact(gpu, monkeypatch, capfd, sigma, n, prefixlength, copies):
    """every table and the .prj statistics exact on the device, the prefix length
    the reference recommends, the first sort the size selects"""
    import device_check as dc
    assert ou.lib().ora_recommended_prefixlength(sigma, n) == prefixlength
    N = n + 1
    buf = _alphabet_text(sigma, n, 60 + sigma, copies)
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    with esa.EsaEngine(n, sigma) as eng:
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run()
        st = eng.stats()
        p = engine_paths.single(capfd.readouterr().err)
        msd = p["run"]["first_sort"] == "msd"
        assert msd == (p["msd"] is not None)
        assert st["prefixlength"] == prefixlength
        # the 5-bit MSD sort tells the prefix length from nine symbols' codes
        assert msd == (sigma <= 4 or (sigma <= 20 and prefixlength <= 9))
        sa, lcp, bwt, llv_idx, llv_val = _device_tables(eng, N)
        if copies:
            assert llv_idx.numel() > 0 and st["maxbranchdepth"] >= 5000
        _check_tables(sa, buf, lcp, bwt, llv_idx, llv_val)
        _check_tail_and_prj(sa, buf, lcp, llv_val, st)
        ok, msg = dc.check_esastats_exact(sa, buf, lcp, llv_idx, llv_val, prefixlength, st)
        assert ok, msg


@pytest.mark.parametrize("sigma,n,k", [(2, 67_108_847, 20), (2, 67_108_848, 21),
                                       (5, 976_562_496, 11)])
def test_alphabet_bucket_table_at_size(gpu, sigma, n, k):
    """-bck at the recommended prefix length on either side of the 2-bit key width
    (20 symbols) and past the 5-bit one (10): base-sigma codes with clamped
    padding, digits past the key from the text; left borders against counts of
    the suffixes' padded k-codes on the device; the LSD sort's suffix table
    (WANT_BCK turns the MSD sort off) exact"""
    import device_check as dc
    buf = _alphabet_text(sigma, n, 62, sigma == 2)
    with esa.EsaEngine(n, sigma) as eng:
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run(esa.WANT_SUF | esa.WANT_BCK)
        assert eng.stats()["prefixlength"] == k
        leftborder = torch.from_numpy(eng.bcktab()[0].astype(np.int64)).to("cuda:0")
        sa = dc.as_tensor(eng.device_pointer(esa.TAB_SUF), n + 1, "<i8")
        rank, msg = dc.suffix_ranks(sa)
        assert rank is not None, msg
        ok, msg = dc.check_suffix_array_exact(sa, buf, rank)
        assert ok, msg
        del rank
    # padded k-code of every suffix that starts with a letter
    code = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    live = torch.ones(n, dtype=torch.bool, device="cuda:0")
    for j in range(k):
        d = torch.full((n,), 254, dtype=torch.uint8, device="cuda:0")
        d[:n - j] = buf[j:]
        live &= d < sigma
        code = code * sigma + torch.where(live, d.to(torch.int64), torch.full_like(code, sigma - 1))
    counts = torch.bincount(code[buf < sigma], minlength=sigma ** k)
    want = torch.zeros(sigma ** k + 1, dtype=torch.int64, device="cuda:0")
    want[1:] = torch.cumsum(counts, 0)
    assert leftborder.numel() == want.numel()
    assert bool((leftborder == want).all())
