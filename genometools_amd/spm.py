"""Host-side mirror of `gt encseq2spm -l L -ii READS -spm show|count` over the C
ABI: all suffix-prefix matches of a sequence set, the overlap phase of a
string-graph assembler, from the suffix table and the LCP table together
(src/match/esa-spmsk.c).

`SuffixPrefixMatches.prepare(min_len)` counts, `SuffixPrefixMatches.matches()`
yields the records (suffix_seq, prefix_seq, len) in table order, in chunks, so
that a result larger than memory is streamed; `all_matches` does both.  The
index is the encoded sequence set with its .suf, .lcp and .llv tables: in host
memory, in device memory or resident in an `EsaEngine`.  The library never
mirrors: `mirrored(enc)` makes the set `gt encseq2spm` works on, both strands
(include/gtamd_spm.h states the semantics, the order and what the fields of the
info mean).

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, host_tables, ptr, record_chunks
from ._lib import SpmInfo

DEFAULT_CAPACITY = 1 << 20        # records of one emit call (24 bytes each)


def geometry():
    """(terminal suffixes of one workgroup, smallest capacity of an emit call);
    needs no device"""
    tile, least = ctypes.c_uint32(), ctypes.c_uint64()
    _lib.load().gtamd_spm_geometry(ctypes.byref(tile), ctypes.byref(least))
    return tile.value, least.value


def mirrored(enc):
    """the encoded DNA sequence set followed by a separator and its reverse
    complement, 2n + 1 symbols (gtamd_mirror): R sequences become 2R, number
    R + j the reverse complement of number R - 1 - j; specials stay as they are"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    back = enc[::-1]
    return np.concatenate([enc, np.array([255], dtype=np.uint8),
                           np.where(back < 254, 3 - back, back).astype(np.uint8)])


class SuffixPrefixMatches(Consumer):
    """matcher over one index on one device"""
    NAME, INFO = "spm", SpmInfo

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
        """count the suffix-prefix matches of at least min_len letters; the info as a dict"""
        return self._call_info("prepare", min_len)

    def info(self):
        """gtamd_spm_info of the last prepare, as a dict"""
        return self._call_info("get_info")

    def matches(self, capacity=DEFAULT_CAPACITY, device=False, cursor=0):
        """the records of the last prepare in order, one array per emit call of
        at most `capacity` records: numpy uint64 arrays of shape (records, 3) --
        suffix_seq, prefix_seq, len -- or, with device=True, torch int64 tensors
        of that shape on the device, which the next call overwrites.  cursor:
        the record number to start from, 0 to info()["matches"] (or a uint64 array
        of one element that every call advances: _consumer.record_chunks)"""
        yield from record_chunks(self._fn("emit"), self._p, capacity, device, self._device, cursor)

    def all_matches(self, min_len, capacity=DEFAULT_CAPACITY):
        """every record of minimum length min_len as one numpy array of shape (matches, 3)"""
        self.prepare(min_len)
        chunks = list(self.matches(capacity))
        return np.concatenate(chunks) if chunks else np.zeros((0, 3), dtype=np.uint64)
