"""Host-side mirror of `gt dev idxlocali -th T -esa INDEX -q FILES` over the C
ABI: every local alignment of a query of any length against an indexed
sequence whose score reaches a threshold, under match / mismatch / gap scores
and without a seed (gt_indexbasedlocali, src/match/idx-limdfs.c, with the
column of src/match/idxlocalidp.c).

`LocalAlignments.prepare(queries, T)` walks every (query, group of the table)
once and counts its matches, `LocalAlignments.records()` yields the records
(query, dbstart, dblen | score << 32, qstart | qlen << 32) in the order of
include/gtamd_locali.h -- query, table index -- in pieces, so that a result
larger than memory is streamed.  The index is the encoded sequence with its
.suf table: in host memory, in device memory or resident in an `EsaEngine`; or
a `pck.PackedIndexReader` (`gt dev idxlocali -pck`, include/gtamd_pcklocali.h).

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, SufIndexSetters, gathered, pack_sequences, ptr, record_chunks
from ._lib import LocaliInfo

DEFAULT_CAPACITY = 1 << 20        # records of one emit call (32 bytes each)
AUTO = 0xffffffff
WILDCARD = 254


def geometry():
    """(waves of one workgroup, smallest capacity of an emit call, letters a
    query may have, smallest stack of set_limits in words); needs no device"""
    waves, least, longest, stack = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    _lib.load().gtamd_locali_geometry(ctypes.byref(waves), ctypes.byref(least), ctypes.byref(longest),
                                      ctypes.byref(stack))
    return waves.value, least.value, longest.value, stack.value


pack_queries = pack_sequences


def unpack(records):
    """the columns (query, dbstart, dblen, score, qstart, qlen) of an array of records"""
    records = np.asarray(records, dtype=np.uint64).reshape(-1, 4)
    low, high = np.uint64(0xffffffff), np.uint64(32)
    return (records[:, 0], records[:, 1], records[:, 2] & low, records[:, 2] >> high,
            records[:, 3] & low, records[:, 3] >> high)


class LocalAlignments(SufIndexSetters, Consumer):
    """aligner over one index on one device"""
    NAME, INFO = "locali", LocaliInfo

    # -- the index: each call replaces the one before -------------------------
    def set_index_packed(self, reader):
        """a `pck.PackedIndexReader` with an open image
        (include/gtamd_pcklocali.h): the matches are those of the text the index
        was built from read backwards -- an index of the reversed subject answers
        for the subject -- in the order of that header, which inside one query
        is not the order of the suffix table.  The reader must outlive the
        calls."""
        self._call("set_index_pckidx", reader._p)

    def set_limits(self, stack_words=0, cut_depth=AUTO):
        """what the next prepare sizes itself by: the words of one wave's stack
        (0: chosen from the longest query) and the depth q of the cut of the
        table into groups (AUTO: chosen from the number of queries)"""
        self._call("set_limits", stack_words, cut_depth)

    # -- the enumeration ------------------------------------------------------
    def prepare(self, queries, T, match=1, mismatch=-1, gapextend=-1):
        """counts the local alignments of score >= T of a list of encoded
        queries (arrays of letters, 254 for a wildcard) in host memory; the
        info as a dict"""
        symbols, offsets = pack_queries(queries)
        return self._call_info("prepare", ptr(symbols) if len(queries) else None,
                               ptr(offsets) if len(queries) else None, len(queries), 0, match, mismatch, gapextend, T)

    def prepare_device(self, symbols_ptr, offsets_ptr, Q, T, match=1, mismatch=-1, gapextend=-1):
        """the same for Q queries whose symbols and Q + 1 uint64 offsets are in
        device memory, which must outlive the emit calls"""
        return self._call_info("prepare", symbols_ptr, offsets_ptr, Q, 1, match, mismatch, gapextend, T)

    def info(self):
        """gtamd_locali_info of the last prepare and the emit calls since, as a dict"""
        return self._call_info("get_info")

    def records(self, capacity=DEFAULT_CAPACITY, device=False, cursor=0):
        """the records of the last prepare in order, one array per emit call of
        at most `capacity` records: numpy uint64 arrays of shape (records, 4) --
        query, dbstart, dblen | score << 32, qstart | qlen << 32 -- or, with
        device=True, torch int64 tensors of that shape on the device, which the
        next call overwrites.  cursor: the record number to start from, 0 to
        info()["matches"] (or a uint64 array of one element that every call
        advances: _consumer.record_chunks)"""
        yield from record_chunks(self._fn("emit"), self._p, capacity, device, self._device, cursor, columns=4)

    def all_records(self, queries, T, match=1, mismatch=-1, gapextend=-1, capacity=DEFAULT_CAPACITY):
        """every record of `queries` as one numpy array of shape (matches, 4)"""
        self.prepare(queries, T, match, mismatch, gapextend)
        return gathered(self.records(capacity), columns=4)
