"""Host-side mirror of `gt repfind -l L -ii INDEX` over the C ABI: the maximal
exact repeats of the indexed sequences, enumerated from the suffix table and the
LCP table together (gt_enumeratemaxpairs, src/match/esa-maxpairs.c).

`MaxPairs.prepare(min_len)` counts, `MaxPairs.pairs()` yields the records
(pos1, pos2, len) in table order, in chunks, so that a result larger than
memory is streamed.  The index is the encoded sequence with its .suf, .lcp and
.llv tables: in host memory, in device memory or resident in an `EsaEngine`
(include/gtamd_maxpairs.h states the semantics, the order and what the fields
of the info mean).

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import numpy as np

from ._consumer import Consumer, host_tables, ptr, record_chunks
from ._lib import MaxPairsInfo

DEFAULT_CAPACITY = 1 << 20        # records of one chunk (24 bytes each)


class MaxPairs(Consumer):
    """enumerator over one index on one device"""
    NAME, INFO = "maxpairs", MaxPairsInfo

    # -- the index: each call replaces the one before -------------------------
    def set_index(self, enc, suf, lcp, llv=None):
        """tables in host memory (numpy): enc uint8, n symbols; suf uint32 or
        uint64, n + 1 entries; lcp uint8, n + 1 bytes; llv uint64 pairs
        (table index, value), any shape of 2 * pairs numbers, or None"""
        enc, suf, lcp, llv = host_tables(enc, suf, lcp, llv)
        self._call("set_index_host", ptr(enc), enc.size, ptr(suf), suf.dtype.itemsize, ptr(lcp),
                   ptr(llv) if llv.size else None, llv.size // 2)

    def set_index_device(self, enc_ptr, n, suf_ptr, suf_bytes, lcp_ptr, llv_ptr=None, llv_pairs=0):
        """the same for raw device pointers, which must outlive the calls"""
        self._call("set_index", enc_ptr, n, suf_ptr, suf_bytes, lcp_ptr, llv_ptr, llv_pairs)

    def set_index_engine(self, engine, enc_device_ptr, n):
        """the tables an EsaEngine holds after run() with esa.WANT_SUF |
        esa.WANT_LCP (forward read mode); enc_device_ptr: the n symbols, on the
        device.  The engine must outlive the calls."""
        self._call("set_index_esa", engine._ctx, enc_device_ptr, n)

    # -- the enumeration ------------------------------------------------------
    def prepare(self, min_len):
        """count the maximal pairs of at least min_len letters; the info as a dict"""
        return self._call_info("prepare", min_len)

    def info(self):
        """gtamd_maxpairs_info of the last prepare, as a dict"""
        return self._call_info("get_info")

    def pairs(self, capacity=None, device=False, cursor=0):
        """the records of the last prepare in table order, in chunks of whole
        suffixes and at most `capacity` records (default: DEFAULT_CAPACITY, or
        what one suffix needs if that is more): numpy uint64 arrays of shape
        (records, 3) -- pos1, pos2, len -- or, with device=True, torch int64
        tensors of that shape on the device, which the next chunk overwrites.
        cursor: the suffix in a run to start from, in table order, 0 to
        info()["run_suffixes"] (or a uint64 array of one element that every call
        advances: _consumer.record_chunks)"""
        if capacity is None:
            capacity = max(DEFAULT_CAPACITY, self.info()["max_pairs_of_one_suffix"])
        yield from record_chunks(self._fn("emit"), self._p, capacity, device, self._device, cursor)

    def all_pairs(self, capacity=None):
        """every record as one numpy array of shape (pairs, 3)"""
        chunks = list(self.pairs(capacity))
        return np.concatenate(chunks) if chunks else np.zeros((0, 3), dtype=np.uint64)
