"""Host-side mirror of `gt repfind -q FILE`, `-r` and `-p` over the C ABI: the
maximal exact matches of a query against an indexed sequence, from the suffix
table and the sequence (GtQuerysubstringmatchiterator,
src/match/esa-mmsearch.c).

`QueryMatches.prepare(query, min_len)` finds the interval of every query
position and counts the candidates, `QueryMatches.emit()` yields the records
(dbpos, qpos, len) in the reference's order -- ascending query position, then
table index -- in chunks, so that a result larger than memory is streamed.
`all_matches` does both, for the query read forward, reversed or
reverse-complemented sequence by sequence.  The index is the encoded sequence
with its .suf table: in host memory, in device memory or resident in an
`EsaEngine` (include/gtamd_qmatch.h states the semantics, the order and what
the fields of the info mean).

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, gathered, host_tables, ptr, record_chunks
from ._lib import QmatchInfo

DEFAULT_CAPACITY = 1 << 20        # records of one emit call (24 bytes each)
READMODES = ("fwd", "rev", "rcl")


def geometry():
    """(query positions of one workgroup, smallest capacity of an emit call);
    needs no device"""
    tile, least = ctypes.c_uint32(), ctypes.c_uint64()
    _lib.load().gtamd_qmatch_geometry(ctypes.byref(tile), ctypes.byref(least))
    return tile.value, least.value


def transformed(query, readmode):
    """the encoded query (sequences joined by separators 255) as a match of
    `readmode` reads it (gt_mmsearch_accessquery): "rev" reverses every
    sequence on its own, "rcl" also turns the letters c into 3 - c; specials
    stay as they are"""
    if readmode not in READMODES:
        raise ValueError("readmode %r, one of %s expected" % (readmode, ", ".join(READMODES)))
    query = np.ascontiguousarray(query, dtype=np.uint8)
    if readmode == "fwd":
        return query
    out = query.copy()
    cuts = np.flatnonzero(query == 255)
    for start, end in zip(np.concatenate([[0], cuts + 1]).tolist(), np.concatenate([cuts, [query.size]]).tolist()):
        out[start:end] = query[start:end][::-1]
    if readmode == "rcl":
        out = np.where(out < 254, 3 - out, out).astype(np.uint8)
    return out


class QueryMatches(Consumer):
    """matcher over one index on one device"""
    NAME, INFO = "qmatch", QmatchInfo

    # -- the index: each call replaces the one before -------------------------
    def set_index(self, enc, suf):
        """tables in host memory (numpy): enc uint8, n symbols; suf uint32 or
        uint64, n + 1 entries"""
        enc, suf = host_tables(enc, suf)
        self._call("set_index_host", ptr(enc), enc.size, ptr(suf), suf.dtype.itemsize)

    def set_index_device(self, enc_ptr, n, suf_ptr, suf_bytes):
        """the same for raw device pointers, which must outlive the calls"""
        self._call("set_index", enc_ptr, n, suf_ptr, suf_bytes)

    def set_index_engine(self, engine, enc_device_ptr, n):
        """the .suf table an EsaEngine holds after run() with esa.WANT_SUF
        (forward read mode); enc_device_ptr: the n symbols, on the device.  The
        engine must outlive the calls."""
        self._call("set_index_esa", engine._ctx, enc_device_ptr, n)

    # -- the enumeration ------------------------------------------------------
    def prepare(self, query, min_len):
        """the intervals and the candidate count of an encoded query in host
        memory (sequences joined by separators) for matches of at least min_len
        letters; the info as a dict"""
        query = np.ascontiguousarray(query, dtype=np.uint8)
        return self._call_info("prepare", ptr(query) if query.size else None, query.size, 0, min_len)

    def prepare_device(self, query_ptr, m, min_len):
        """the same for m symbols in device memory, which must outlive the emit calls"""
        return self._call_info("prepare", query_ptr, m, 1, min_len)

    def info(self):
        """gtamd_qmatch_info of the last prepare and the emit calls since, as a dict"""
        return self._call_info("get_info")

    def emit(self, capacity=DEFAULT_CAPACITY, device=False, cursor=0):
        """the records of the last prepare in order, one array per emit call of
        at most `capacity` records: numpy uint64 arrays of shape (records, 3) --
        dbpos, qpos, len -- or, with device=True, torch int64 tensors of that
        shape on the device, which the next call overwrites.  cursor: the
        candidate number to start from, 0 to info()["candidates"] (or a uint64
        array of one element that every call advances: _consumer.record_chunks)"""
        yield from record_chunks(self._fn("emit"), self._p, capacity, device, self._device, cursor)

    def all_matches(self, query, min_len, readmode="fwd", capacity=DEFAULT_CAPACITY):
        """every record of `query` read in `readmode` ("fwd", "rev": every
        sequence reversed, "rcl": reversed and complemented) as one numpy array
        of shape (matches, 3), in the coordinates of the transformed query"""
        self.prepare(transformed(query, readmode), min_len)
        return gathered(self.emit(capacity))
