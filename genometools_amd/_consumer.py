"""What the wrappers of the index consumers share (check.py, mstat.py,
maxpairs.py, qmatch.py, spm.py, spmred.py, tagmatch.py, locali.py, and the
reader and the builder of pck.py): the life of the object behind the C ABI, its
info struct as a dict, the checks of tables in host memory, the setters of an
index of .suf with its alphabet, the sequences of a job walker, and the
generator over the records of an enumeration with their gathering."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def as_dict(struct):
    return {name: getattr(struct, name) for name, _ in struct._fields_}


class Consumer:
    """one object of the library on one device.  NAME: gtamd_NAME_create, ... are
    its entry points; INFO: the ctypes struct of gtamd_NAME_get_info"""
    NAME = None
    INFO = None

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._device = device
        self._p = self._fn("create")(device)
        if not self._p:
            raise _lib.EsaError(self._lib.gtamd_esa_last_error().decode())

    def _fn(self, what):
        return getattr(self._lib, "gtamd_%s_%s" % (self.NAME, what))

    def _call(self, what, *args):
        check(self._fn(what)(self._p, *args))

    def _call_info(self, what, *args):
        """a call whose last argument is the info struct, which comes back as a dict"""
        info = self.INFO()
        self._call(what, *(args + (ctypes.byref(info),)))
        return as_dict(info)

    def close(self):
        if self._p:
            self._fn("destroy")(self._p)
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


def host_tables(enc, suf, lcp=None, llv=None,
                suf_only="%(n)d symbols need %(entries)d entries of suf (%(given)d given)"):
    """(enc, suf) or (enc, suf, lcp, llv) as contiguous arrays of the types the
    library reads, llv flat; suf_only words a suf of the wrong size where there
    is no lcp"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    suf = np.ascontiguousarray(suf)
    if lcp is not None:
        lcp = np.ascontiguousarray(lcp, dtype=np.uint8)
        llv = np.zeros(0, dtype=np.uint64) if llv is None else np.ascontiguousarray(llv, dtype=np.uint64).reshape(-1)
    if suf.dtype not in (np.dtype(np.uint32), np.dtype(np.uint64)):
        raise TypeError("suf must be uint32 or uint64, not %s" % suf.dtype)
    if lcp is None:
        if suf.size != enc.size + 1:
            raise ValueError(suf_only % dict(n=enc.size, entries=enc.size + 1, given=suf.size))
        return enc, suf
    if suf.size != enc.size + 1 or lcp.size != enc.size + 1 or llv.size % 2:
        raise ValueError("%d symbols need %d entries of suf and lcp (%d, %d given) and whole pairs of llv"
                         % (enc.size, enc.size + 1, suf.size, lcp.size))
    return enc, suf, lcp, llv


class SufIndexSetters:
    """the index of a Consumer that reads the sequence and .suf and is told the
    letters of the alphabet (tagmatch.py, locali.py): each call replaces the
    index before.  Their set_index_packed is their own: what a packed index
    answers differs."""

    def set_index(self, enc, suf, numofchars=4):
        """tables in host memory (numpy): enc uint8, n symbols; suf uint32 or
        uint64, n + 1 entries; numofchars: letters of the alphabet"""
        enc, suf = host_tables(enc, suf)
        self._call("set_index_host", ptr(enc), enc.size, ptr(suf), suf.dtype.itemsize, numofchars)

    def set_index_device(self, enc_ptr, n, suf_ptr, suf_bytes, numofchars=4):
        """the same for raw device pointers, which must outlive the calls"""
        self._call("set_index", enc_ptr, n, suf_ptr, suf_bytes, numofchars)

    def set_index_engine(self, engine, enc_device_ptr, n, numofchars=4):
        """the .suf table an EsaEngine holds after run() with esa.WANT_SUF
        (forward read mode); enc_device_ptr: the n symbols, on the device.  The
        engine must outlive the calls."""
        self._call("set_index_esa", engine._ctx, enc_device_ptr, n, numofchars)


def pack_sequences(sequences):
    """(symbols, offsets) of a list of encoded sequences (tags, queries): one
    uint8 array and the len(sequences) + 1 uint64 offsets into it"""
    sequences = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1) for s in sequences]
    offsets = np.zeros(len(sequences) + 1, dtype=np.uint64)
    if sequences:
        offsets[1:] = np.cumsum([s.size for s in sequences])
    symbols = np.concatenate(sequences) if sequences else np.zeros(0, dtype=np.uint8)
    return symbols, offsets


def gathered(chunks, columns=3):
    """the arrays of record_chunks as one numpy array of shape (records, columns)"""
    chunks = list(chunks)
    return np.concatenate(chunks) if chunks else np.zeros((0, columns), dtype=np.uint64)


def record_chunks(emit_fn, handle, capacity, device, device_index, cursor=0, columns=3):
    """the records of an enumeration, one array of shape (records, columns) per
    call of emit_fn (gtamd_*_emit) with at most `capacity` records, until a call
    gives none: numpy uint64 copies, or, with `device`, torch int64 views of one
    buffer on cuda:device_index, which the next call overwrites.  cursor: where
    the enumeration starts, in the unit the consumer's header states for its
    cursor, 0 to its total; a value beyond is refused by the first call.  An
    int, or a numpy uint64 array of one element, which every call advances in
    place: what a caller that stops early passes again to resume"""
    if isinstance(cursor, np.ndarray):
        if cursor.dtype != np.uint64 or cursor.size != 1 or not cursor.flags.writeable:
            raise TypeError("a cursor array must be one writable uint64")
        cursor = ctypes.c_uint64.from_buffer(cursor)
    else:
        cursor = ctypes.c_uint64(cursor)
    written = ctypes.c_uint64(0)
    if device:
        import torch
        buf = torch.empty((max(capacity, 1), columns), dtype=torch.int64, device="cuda:%d" % device_index)
        address = buf.data_ptr()
    else:
        buf = np.empty((max(capacity, 1), columns), dtype=np.uint64)
        address = buf.ctypes.data
    while True:
        check(emit_fn(handle, ctypes.byref(cursor), address, capacity, int(device), ctypes.byref(written)))
        if written.value == 0:
            return
        yield buf[:written.value] if device else buf[:written.value].copy()
