"""Host-side mirror of `gt readjoiner overlap -readset X -l L` over the C ABI:
the irreducible suffix-prefix matches of a read set, the overlaps a string graph
keeps, decided pair by pair on the device while they are found
(src/match/rdj-spmfind.c).

`IrreducibleMatches.prepare(min_len, elimtrans, mirrored)` decides and counts,
`IrreducibleMatches.matches()` yields the kept records (suffix_read,
prefix_read, len, flags) in table order, in chunks; `all_matches` does both.
The index is that of `spm.SuffixPrefixMatches`; with `mirrored` it is the set
`spm.mirrored(enc)` makes, and the records carry read numbers and directions
(flags: SUFFIX_DIRECT | PREFIX_DIRECT).  include/gtamd_spmred.h states the
definition, the filter, the order and what the fields of the info mean;
`closing_figures` turns the info into the three figures the tool prints.

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, host_tables, ptr, record_chunks
from ._lib import SpmredInfo

DEFAULT_CAPACITY = 1 << 20        # records of one emit call (32 bytes each)
ELIMTRANS, MIRRORED = 1, 2        # GTAMD_SPMRED_ELIMTRANS, GTAMD_SPMRED_MIRRORED
PREFIX_DIRECT, SUFFIX_DIRECT = 1, 2


def geometry():
    """(pairs of one launch of the decision, smallest capacity of an emit call);
    needs no device"""
    chunk, least = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.load().gtamd_spmred_geometry(ctypes.byref(chunk), ctypes.byref(least))
    return chunk.value, least.value


def closing_figures(info, reads):
    """(irreducible, transitive, irreducible per read) as `gt readjoiner overlap`
    closes its output: the transitive pairs of two different reads are counted
    once for their two mirror images"""
    return (info["kept"], info["transitive_same_read"] + (info["transitive_other"] >> 1),
            "%.2f" % (np.float32(info["kept"]) / np.float32(reads)))


class IrreducibleMatches(Consumer):
    """matcher over one index on one device"""
    NAME, INFO = "spmred", SpmredInfo

    # -- the index: each call replaces the one before -------------------------
    def set_index(self, enc, suf, lcp, llv=None):
        """tables in host memory (numpy), as spm.SuffixPrefixMatches.set_index"""
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
    def prepare(self, min_len, elimtrans=True, mirrored=True):
        """decide every suffix-prefix match of at least min_len letters; the info
        as a dict.  elimtrans: keep the irreducible ones only; mirrored: the set
        is the reads and their reverse complements, one of the two mirror images
        of an overlap is kept, records carry read numbers and directions"""
        return self._call_info("prepare", min_len, (ELIMTRANS if elimtrans else 0) | (MIRRORED if mirrored else 0))

    def info(self):
        """gtamd_spmred_info of the last prepare, as a dict"""
        return self._call_info("get_info")

    def matches(self, capacity=DEFAULT_CAPACITY, device=False, cursor=0):
        """the kept records of the last prepare in order, one array per emit call
        of at most `capacity` records: numpy uint64 arrays of shape (records, 4)
        -- suffix_read, prefix_read, len, flags -- or, with device=True, torch
        int64 tensors of that shape on the device, which the next call
        overwrites.  cursor: the kept record to start from, 0 to info()["kept"]
        (or a uint64 array of one element that every call advances:
        _consumer.record_chunks)"""
        yield from record_chunks(self._fn("emit"), self._p, capacity, device, self._device, cursor, columns=4)

    def all_matches(self, min_len, elimtrans=True, mirrored=True, capacity=DEFAULT_CAPACITY):
        """every kept record as one numpy array of shape (kept, 4)"""
        self.prepare(min_len, elimtrans, mirrored)
        chunks = list(self.matches(capacity))
        return np.concatenate(chunks) if chunks else np.zeros((0, 4), dtype=np.uint64)
