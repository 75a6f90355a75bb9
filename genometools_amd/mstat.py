"""Host-side mirror of `gt matstat -esa` and `gt uniquesub -esa` over the C ABI.

For every position of a query, `MatchStats.matstat` gives the longest prefix
that occurs in the subject and where (gt_suffixarraymstats,
src/match/esa-minunique.c:68-105), `MatchStats.uniquesub` the shortest prefix
that occurs exactly once (gt_suffixarrayuniqueforward, :26-66).  The subject is
an index: its encoded sequence and its suffix table, in host memory, in device
memory or resident in an `EsaEngine` (include/gtamd_mstat.h states the
semantics and what the fields of `info()` mean).

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, host_tables, ptr
from ._lib import MstatInfo


def geometry():
    """(query positions one workgroup takes, symbols of one wide comparison,
    number of symbols from which the wide comparison is used); needs no device"""
    tile, word, word_min = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _lib.load().gtamd_mstat_geometry(ctypes.byref(tile), ctypes.byref(word), ctypes.byref(word_min))
    return tile.value, word.value, word_min.value


class MatchStats(Consumer):
    """searcher over one index on one device; TILE, WORD and WORD_MIN: geometry()"""
    NAME, INFO = "mstat", MstatInfo

    def __init__(self, device=0):
        self.TILE, self.WORD, self.WORD_MIN = geometry()
        super().__init__(device)

    # -- the index: each call replaces the one before -------------------------
    def set_index(self, enc, suf, numofchars):
        """tables in host memory (numpy): enc uint8, n symbols; suf uint32 or
        uint64, n + 1 entries"""
        enc, suf = host_tables(enc, suf, suf_only="suf has %(given)d entries, %(n)d symbols need %(entries)d")
        self._call("set_index_host", ptr(enc), enc.size, ptr(suf), suf.dtype.itemsize, numofchars)

    def set_index_device(self, enc_ptr, n, suf_ptr, suf_bytes, numofchars):
        """the same for raw device pointers, which must outlive the searches"""
        self._call("set_index", enc_ptr, n, suf_ptr, suf_bytes, numofchars)

    def set_index_engine(self, engine, enc_device_ptr, n):
        """the .suf table an EsaEngine holds after run() with esa.WANT_SUF;
        enc_device_ptr: the n symbols the table describes (as the engine's read
        mode reads them), on the device.  The engine must outlive the searches."""
        self._call("set_index_esa", engine._ctx, enc_device_ptr, n, engine.numofchars)

    def set_index_packed(self, reader):
        """a `pck.PackedIndexReader` with an open image (include/gtamd_pckidx.h):
        lengths are those of the text the index was built from read backwards --
        an index of the reversed subject answers for the subject -- and
        subjectpos is the reference's witness.  The reader must outlive the
        searches."""
        self._call("set_index_pckidx", reader._p)

    # -- the questions --------------------------------------------------------
    def matstat(self, query, max_len=0):
        """(length, subjectpos) for every position of the encoded query (numpy
        uint8): uint32 and uint64; subjectpos is 0 where length is 0"""
        query = np.ascontiguousarray(query, dtype=np.uint8)
        length = np.empty(query.size, dtype=np.uint32)
        pos = np.empty(query.size, dtype=np.uint64)
        self._call("matstat", ptr(query), query.size, 0, max_len, ptr(length), ptr(pos), 0)
        return length, pos

    def uniquesub(self, query, max_len=0):
        """length of the minimum unique prefix for every position, 0: none"""
        query = np.ascontiguousarray(query, dtype=np.uint8)
        length = np.empty(query.size, dtype=np.uint32)
        self._call("uniquesub", ptr(query), query.size, 0, max_len, ptr(length), 0)
        return length

    def matstat_device(self, query_ptr, m, length_ptr, subjectpos_ptr=None, max_len=0):
        """query and outputs (uint32[m], uint64[m] or None) in device memory"""
        self._call("matstat", query_ptr, m, 1, max_len, length_ptr, subjectpos_ptr, 1)

    def uniquesub_device(self, query_ptr, m, length_ptr, max_len=0):
        self._call("uniquesub", query_ptr, m, 1, max_len, length_ptr, 1)

    def info(self):
        """gtamd_mstat_info of the last call, as a dict"""
        return self._call_info("get_info")
