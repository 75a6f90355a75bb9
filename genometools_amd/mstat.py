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
from ._lib import MstatInfo, check


def geometry():
    """(query positions one workgroup takes, symbols of one wide comparison,
    number of symbols from which the wide comparison is used); needs no device"""
    tile, word, word_min = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _lib.load().gtamd_mstat_geometry(ctypes.byref(tile), ctypes.byref(word), ctypes.byref(word_min))
    return tile.value, word.value, word_min.value


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class MatchStats:
    """searcher over one index on one device; TILE, WORD and WORD_MIN: geometry()"""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self.TILE, self.WORD, self.WORD_MIN = geometry()
        self._p = self._lib.gtamd_mstat_create(device)
        if not self._p:
            raise _lib.EsaError(self._lib.gtamd_esa_last_error().decode())

    def close(self):
        if self._p:
            self._lib.gtamd_mstat_destroy(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the index: each call replaces the one before -------------------------
    def set_index(self, enc, suf, numofchars):
        """tables in host memory (numpy): enc uint8, n symbols; suf uint32 or
        uint64, n + 1 entries"""
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        suf = np.ascontiguousarray(suf)
        if suf.dtype not in (np.dtype(np.uint32), np.dtype(np.uint64)):
            raise TypeError("suf must be uint32 or uint64, not %s" % suf.dtype)
        if suf.size != enc.size + 1:
            raise ValueError("suf has %d entries, %d symbols need %d" % (suf.size, enc.size, enc.size + 1))
        check(self._lib.gtamd_mstat_set_index_host(self._p, _ptr(enc), enc.size, _ptr(suf),
                                                   suf.dtype.itemsize, numofchars))

    def set_index_device(self, enc_ptr, n, suf_ptr, suf_bytes, numofchars):
        """the same for raw device pointers, which must outlive the searches"""
        check(self._lib.gtamd_mstat_set_index(self._p, enc_ptr, n, suf_ptr, suf_bytes, numofchars))

    def set_index_engine(self, engine, enc_device_ptr, n):
        """the .suf table an EsaEngine holds after run() with esa.WANT_SUF;
        enc_device_ptr: the n symbols the table describes (as the engine's read
        mode reads them), on the device.  The engine must outlive the searches."""
        check(self._lib.gtamd_mstat_set_index_esa(self._p, engine._ctx, enc_device_ptr, n,
                                                  engine.numofchars))

    # -- the questions --------------------------------------------------------
    def matstat(self, query, max_len=0):
        """(length, subjectpos) for every position of the encoded query (numpy
        uint8): uint32 and uint64; subjectpos is 0 where length is 0"""
        query = np.ascontiguousarray(query, dtype=np.uint8)
        length = np.empty(query.size, dtype=np.uint32)
        pos = np.empty(query.size, dtype=np.uint64)
        check(self._lib.gtamd_mstat_matstat(self._p, _ptr(query), query.size, 0, max_len, _ptr(length),
                                            _ptr(pos), 0))
        return length, pos

    def uniquesub(self, query, max_len=0):
        """length of the minimum unique prefix for every position, 0: none"""
        query = np.ascontiguousarray(query, dtype=np.uint8)
        length = np.empty(query.size, dtype=np.uint32)
        check(self._lib.gtamd_mstat_uniquesub(self._p, _ptr(query), query.size, 0, max_len,
                                              _ptr(length), 0))
        return length

    def matstat_device(self, query_ptr, m, length_ptr, subjectpos_ptr=None, max_len=0):
        """query and outputs (uint32[m], uint64[m] or None) in device memory"""
        check(self._lib.gtamd_mstat_matstat(self._p, query_ptr, m, 1, max_len, length_ptr,
                                            subjectpos_ptr, 1))

    def uniquesub_device(self, query_ptr, m, length_ptr, max_len=0):
        check(self._lib.gtamd_mstat_uniquesub(self._p, query_ptr, m, 1, max_len, length_ptr, 1))

    def info(self):
        """gtamd_mstat_info of the last call, as a dict"""
        info = MstatInfo()
        check(self._lib.gtamd_mstat_get_info(self._p, ctypes.byref(info)))
        return {name: getattr(info, name) for name, _ in info._fields_}
