"""What the four consumers that hold an index -- matching statistics (mstat.py),
maximal pairs (maxpairs.py), query matches (qmatch.py), suffix-prefix matches
(spm.py) -- say when they refuse one, word for word, and that the three ways of
setting one (host memory, device pointers, a live engine) give the same records.

The refusals are decided on the arguments alone: the device addresses here are
made up and nothing is read from them.  The expected texts are the format
strings of the C sources with the arguments of each call filled in; the holder
of the index and its checks are one piece of code for the four
(csrc/esa_index.h), and this file keeps their wording apart where it differs:
a missing .lcp table is an invalid argument to the maximal pairs and a sentence
of its own to the suffix-prefix matches.

The real index has 300 symbols: one tile of every kernel and one piece of the
upload, so that only the three entry paths differ between the runs."""
import functools

import numpy as np
import pytest

from genometools_amd import _lib, esa, maxpairs, mstat, qmatch, spm

pytestmark = pytest.mark.gpu

ENC, SUF, LCP, LLV = 1 << 20, 1 << 21, 1 << 22, 1 << 23      # addresses of nothing
LIMIT = 2 ** 32 - 4096
MIN_LEN = 10


class Kind:
    """one consumer: how its wrapper is called"""

    def __init__(self, name, cls, feature, with_lcp):
        self.name, self.cls, self.feature, self.with_lcp = name, cls, feature, with_lcp

    def __repr__(self):
        return self.name

    def set_device(self, obj, enc, n, suf, suf_bytes, lcp=LCP, llv=None, llv_pairs=0):
        if self.name == "mstat":
            obj.set_index_device(enc, n, suf, suf_bytes, 4)
        elif self.with_lcp:
            obj.set_index_device(enc, n, suf, suf_bytes, lcp, llv, llv_pairs)
        else:
            obj.set_index_device(enc, n, suf, suf_bytes)

    def set_host(self, obj, enc, suf, lcp, llv):
        if self.name == "mstat":
            obj.set_index(enc, suf, 4)
        elif self.with_lcp:
            obj.set_index(enc, suf, lcp, llv)
        else:
            obj.set_index(enc, suf)

    def first_call(self, obj, query):
        """the call that needs an index: a prepare, or the search itself"""
        if self.name == "mstat":
            return obj.matstat(query)
        if self.name == "qmatch":
            return obj.prepare(query, MIN_LEN)
        return obj.prepare(MIN_LEN)

    def emit(self, obj):
        """the call that needs a prepare; None: there is none"""
        if self.name == "mstat":
            return None
        return list(getattr(obj, {"maxpairs": "pairs", "qmatch": "emit", "spm": "matches"}[self.name])())

    def records(self, obj, query):
        """everything the consumer finds, as one tuple of arrays"""
        if self.name == "mstat":
            return obj.matstat(query) + (obj.uniquesub(query),)
        if self.name == "qmatch":
            return (obj.all_matches(query, MIN_LEN),)
        if self.name == "maxpairs":
            obj.prepare(MIN_LEN)
            return (obj.all_pairs(),)
        return (obj.all_matches(MIN_LEN),)


KINDS = [Kind("mstat", mstat.MatchStats, "matching statistics", False),
         Kind("maxpairs", maxpairs.MaxPairs, "maximal pairs", True),
         Kind("qmatch", qmatch.QueryMatches, "query matches", False),
         Kind("spm", spm.SuffixPrefixMatches, "suffix-prefix matches", True)]
everyone = pytest.mark.parametrize("kind", KINDS, ids=repr)


def _refused(call, *args, **kw):
    with pytest.raises(_lib.EsaError) as e:
        call(*args, **kw)
    return str(e.value)


@functools.lru_cache(maxsize=None)
def _reads():
    """300 symbols: six reads of 49 or 50 letters, each starting with the last 20
    of the one before, joined by separators; and a query cut from them.  Shared,
    never written to."""
    rng = np.random.default_rng(11)
    reads = [rng.integers(0, 4, 50, dtype=np.uint8)]
    for _ in range(5):
        reads.append(np.concatenate([reads[-1][-20:], rng.integers(0, 4, 29, dtype=np.uint8)]))
    parts = []
    for r in reads:
        parts += [r, np.array([255], dtype=np.uint8)]
    enc = np.concatenate(parts[:-1])
    assert enc.size == 300
    query = np.concatenate([enc[30:90], rng.integers(0, 4, 15, dtype=np.uint8), enc[200:240]])
    for a in (enc, query):
        a.setflags(write=False)
    return enc, query


def _device_copy(a):
    import torch
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


@everyone
def test_refusals_on_the_arguments_alone(gpu, kind):
    f, api = kind.feature, "gtamd_" + kind.name
    query = _reads()[1]
    no_index = "%s: no index is set (%s_set_index)" % (f, api)
    with kind.cls() as obj:
        assert _refused(kind.first_call, obj, query) == no_index
        if kind.name != "mstat":
            assert _refused(kind.emit, obj) == "%s: nothing is prepared (%s_prepare)" % (f, api)
        assert _refused(kind.set_device, obj, ENC, 100, SUF, 3) == \
            "%s: .suf entries of 3 bytes, 4 or 8 expected" % f
        assert _refused(kind.set_device, obj, ENC, LIMIT, SUF, 8) == \
            "%s: sequence of %d symbols is beyond the limit of a single build (%d table entries); " \
            "the slices of a build in parts are not searched" % (f, LIMIT, LIMIT)
        if kind.with_lcp:
            assert _refused(kind.set_device, obj, ENC, 100, SUF, 8, LCP, LLV, 101) == \
                "%s: 101 .llv pairs for 100 symbols" % f
            assert _refused(kind.set_device, obj, ENC, 100, SUF, 8, None) == {
                "maxpairs": "invalid argument to gtamd_maxpairs_set_index",
                "spm": "suffix-prefix matches: no .lcp table is given: the matches are found from .suf and "
                       ".lcp together"}[kind.name]
            # (a violation of two rules: the one that is tested first)
            assert _refused(kind.set_device, obj, ENC, LIMIT, SUF, 3, LCP, LLV, LIMIT + 1) == \
                "%s: .suf entries of 3 bytes, 4 or 8 expected" % f
        # a refused index is none
        assert _refused(kind.first_call, obj, query) == no_index


@everyone
def test_an_engine_without_the_tables_is_refused(gpu, kind):
    enc, query = _reads()
    d_enc = _device_copy(enc)
    with kind.cls() as obj, esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_LCP)
        assert _refused(obj.set_index_engine, eng, d_enc.data_ptr(), enc.size) == \
            "%s: the last run did not produce the %s" % (
                kind.feature, ".suf and .lcp tables" if kind.with_lcp else ".suf table")
        assert _refused(kind.first_call, obj, query) == \
            "%s: no index is set (gtamd_%s_set_index)" % (kind.feature, kind.name)


@everyone
def test_three_ways_of_setting_one_index(gpu, kind):
    enc, query = _reads()
    with kind.cls() as obj, esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        suf, lcp, llv = eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV)
        assert suf.size == 301 and suf.dtype == np.uint64 and llv.size == 0

        kind.set_host(obj, enc, suf, lcp, llv)
        if kind.name != "mstat":
            # an index and no prepare
            assert _refused(kind.emit, obj) == "%s: nothing is prepared (gtamd_%s_prepare)" % (kind.feature, kind.name)
        from_host = kind.records(obj, query)
        assert all(a.size > 0 for a in from_host) and from_host[0].any()

        kind.set_host(obj, enc, suf.astype(np.uint32), lcp, llv)
        from_host32 = kind.records(obj, query)

        d_enc, d_suf, d_lcp = _device_copy(enc), _device_copy(suf), _device_copy(lcp)
        kind.set_device(obj, d_enc.data_ptr(), enc.size, d_suf.data_ptr(), 8, d_lcp.data_ptr())
        from_device = kind.records(obj, query)

        obj.set_index_engine(eng, d_enc.data_ptr(), enc.size)
        from_engine = kind.records(obj, query)

        for other in (from_host32, from_device, from_engine):
            assert len(other) == len(from_host)
            for a, b in zip(from_host, other):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
