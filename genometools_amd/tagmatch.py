"""Host-side mirror of `gt tagerator -e K -esa INDEX -q TAGS` over the C ABI:
the approximate matches of short tags (reads, probes, primers) against an
indexed sequence, from the suffix table and the sequence
(gt_indexbasedapproxpatternmatching, src/match/idx-limdfs.c, with the column of
src/match/apmeoveridx.c).

`TagMatches.prepare(tags, K)` walks every (tag, strand) once and counts its
matches, `TagMatches.records()` yields the records (tag, dbstart, lendist) in
the order of include/gtamd_tagmatch.h -- tag, strand, table index -- in pieces,
so that a result larger than memory is streamed.  The index is the encoded
sequence with its .suf table: in host memory, in device memory or resident in
an `EsaEngine`; or a `pck.PackedIndexReader` (`gt tagerator -pck`,
include/gtamd_pcktag.h).

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, SufIndexSetters, gathered, pack_sequences, ptr, record_chunks
from ._lib import TagmatchInfo

DEFAULT_CAPACITY = 1 << 20        # records of one emit call (24 bytes each)
FORWARD, REVCOMP, BEST, WITH_WILDCARDS = 1, 2, 4, 8
NO_K = 0xffffffff
MAX_TAG = 64


def geometry():
    """(jobs of one workgroup, smallest capacity of an emit call, levels of a
    walk); needs no device"""
    waves, least, levels = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
    _lib.load().gtamd_tagmatch_geometry(ctypes.byref(waves), ctypes.byref(least), ctypes.byref(levels))
    return waves.value, least.value, levels.value


pack_tags = pack_sequences


def unpack(records):
    """the columns (tagnumber, reverse complement?, dbstart, len, dist) of an
    array of records"""
    records = np.asarray(records, dtype=np.uint64).reshape(-1, 3)
    return (records[:, 0] >> np.uint64(1), (records[:, 0] & np.uint64(1)).astype(bool), records[:, 1],
            records[:, 2] & np.uint64(0xffffffff), records[:, 2] >> np.uint64(32))


class TagMatches(SufIndexSetters, Consumer):
    """matcher over one index on one device"""
    NAME, INFO = "tagmatch", TagmatchInfo

    # -- the index: each call replaces the one before -------------------------
    def set_index_packed(self, reader):
        """a `pck.PackedIndexReader` with an open image (include/gtamd_pcktag.h):
        the matches are those of the text the index was built from read
        backwards -- an index of the reversed subject answers for the subject --
        in the order of that header, which inside one (tag, strand) is not the
        order of the suffix table; WITH_WILDCARDS is refused.  The reader must
        outlive the calls."""
        self._call("set_index_pckidx", reader._p)

    # -- the enumeration ------------------------------------------------------
    def prepare(self, tags, K, flags=FORWARD | REVCOMP):
        """counts the matches with up to K differences of a list of encoded tags
        (arrays of letters) in host memory; flags: an OR of FORWARD, REVCOMP,
        BEST and WITH_WILDCARDS; the info as a dict"""
        symbols, offsets = pack_tags(tags)
        self._tags = len(tags)
        return self._call_info("prepare", ptr(symbols) if len(tags) else None, ptr(offsets) if len(tags) else None,
                               len(tags), 0, K, flags)

    def prepare_device(self, symbols_ptr, offsets_ptr, T, K, flags=FORWARD | REVCOMP):
        """the same for T tags whose symbols and T + 1 uint64 offsets are in
        device memory, which must outlive the emit calls"""
        self._tags = T
        return self._call_info("prepare", symbols_ptr, offsets_ptr, T, 1, K, flags)

    def info(self):
        """gtamd_tagmatch_info of the last prepare and the emit calls since, as a dict"""
        return self._call_info("get_info")

    def best_k(self):
        """K' of every tag of the last prepare (uint32, NO_K for a tag without a
        match): with BEST the smallest k that gives the tag a match, else K"""
        k = np.zeros(self._tags, dtype=np.uint32)
        self._call("best_k", ptr(k) if k.size else None, k.size)
        return k

    def records(self, capacity=DEFAULT_CAPACITY, device=False, cursor=0):
        """the records of the last prepare in order, one array per emit call of
        at most `capacity` records: numpy uint64 arrays of shape (records, 3) --
        tag, dbstart, lendist -- or, with device=True, torch int64 tensors of
        that shape on the device, which the next call overwrites.  cursor: the
        record number to start from, 0 to info()["matches"] (or a uint64 array of
        one element that every call advances: _consumer.record_chunks)"""
        yield from record_chunks(self._fn("emit"), self._p, capacity, device, self._device, cursor)

    def all_records(self, tags, K, flags=FORWARD | REVCOMP, capacity=DEFAULT_CAPACITY):
        """every record of `tags` as one numpy array of shape (matches, 3)"""
        self.prepare(tags, K, flags)
        return gathered(self.records(capacity))
