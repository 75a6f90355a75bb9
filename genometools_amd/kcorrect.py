"""Host-side mirror of the k-mer correction of `gt readjoiner correct -k K -c C`
over the C ABI: which letters of a read set are rewritten from trusted k-mers,
and the read set with them rewritten, decided and applied on the device
(src/match/rdj-errfind.c).

`KmerCorrection.decide(k, c)` finds the records and the letter each writes,
`records()` hands them out, `corrected(enc)` the reads with the final letters.
The index is .suf and .lcp of the reads or, as the tool uses it, of their
MIRRORED set (`spm.mirrored(enc)`, `ContainedReads.mirrored_device`).
`correct(enc, k, c)` does all of it for an encoded read set: the set mirrored,
the tables built by an `EsaEngine`, the decision and the application, the
symbols on the device from the first step to the last.
include/gtamd_kcorrect.h states the definition and the order rules.

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, as_dict, host_tables, ptr
from ._lib import KcorrectInfo
from .contained import _on_device

MAX_K = 255


def geometry():
    """table entries, children or records of one workgroup; needs no device"""
    tile = ctypes.c_uint32()
    _lib.load().gtamd_kcorrect_geometry(ctypes.byref(tile))
    return tile.value


class KmerCorrection(Consumer):
    """k-mer correction over one index on one device"""
    NAME, INFO = "kcorrect", KcorrectInfo

    # -- the index: each call replaces the one before ------------------------------
    def set_index(self, enc, suf, lcp, mirrored=True):
        """tables in host memory (numpy): enc uint8, n symbols; suf uint32 or
        uint64 and lcp uint8, n + 1 entries; mirrored: enc is a mirrored set"""
        enc, suf, lcp, _ = host_tables(enc, suf, lcp)
        self._call("set_index_host", ptr(enc), enc.size, ptr(suf), suf.dtype.itemsize, ptr(lcp), int(mirrored))

    def set_index_device(self, enc_ptr, n, suf_ptr, suf_bytes, lcp_ptr, mirrored=True):
        """the same for raw device pointers, which must outlive the calls"""
        self._call("set_index", enc_ptr, n, suf_ptr, suf_bytes, lcp_ptr, int(mirrored))

    def set_index_engine(self, engine, enc_device_ptr, n, mirrored=True):
        """the tables an EsaEngine holds after run() with esa.WANT_SUF |
        esa.WANT_LCP (forward read mode); enc_device_ptr: the n symbols, on the
        device.  The engine must outlive the calls."""
        self._call("set_index_esa", engine._ctx, enc_device_ptr, n, int(mirrored))

    # -- the decision --------------------------------------------------------------
    @staticmethod
    def _dict(info):
        out = as_dict(info)
        out["delta"] = list(info.delta)
        return out

    def decide(self, k=31, c=3):
        """the records of the index for k-mers of k letters trusted from c
        occurrences on; the info as a dict"""
        info = KcorrectInfo()
        self._call("decide", k, c, ctypes.byref(info))
        return self._dict(info)

    def info(self):
        """gtamd_kcorrect_info of the last decide, as a dict"""
        info = KcorrectInfo()
        self._call("get_info", ctypes.byref(info))
        return self._dict(info)

    def records(self, device=False):
        """the records of the last decide in record order, shape (records, 3):
        table entry, normalised position, letter written; a numpy uint64 array
        or, with device=True, a torch int64 tensor on the device"""
        count = self.info()["records"]
        if device:
            import torch
            out = torch.empty((count, 3), dtype=torch.int64, device="cuda:%d" % self._device)
            self._call("records", out.data_ptr() if count else None, 1)
            return out
        out = np.empty((count, 3), dtype=np.uint64)
        self._call("records", ptr(out) if count else None, 0)
        return out

    def corrected(self, enc=None, device=False):
        """the unmirrored symbols with the final letters of the last decide: a
        numpy uint8 array or, with device=True, a torch tensor.  enc: the
        symbols of the unmirrored reads, numpy or a torch tensor on the device;
        None: those of the index"""
        keep, address, n = None, None, 0
        if enc is not None:
            keep, address = _on_device(enc, self._device)      # (keep: alive until the call is over)
            n = keep.numel()
        out, count = ctypes.c_void_p(), ctypes.c_uint64()
        self._call("apply", address, n, ctypes.byref(out), ctypes.byref(count))
        count = count.value
        if device:
            import torch
            res = torch.empty(count, dtype=torch.uint8, device="cuda:%d" % self._device)
            self._call("result", res.data_ptr() if count else None, 1)
            return res
        res = np.empty(count, dtype=np.uint8)
        self._call("result", ptr(res) if count else None, 0)
        return res


def correct(enc, k=31, c=3, device=0):
    """(corrected symbols, records, info) of the encoded read set enc, corrected
    on both strands as the tool does"""
    from . import esa
    from .contained import ContainedReads
    with KmerCorrection(device) as kc, ContainedReads(device) as ct:
        both = ct.mirrored_device(enc)
        with esa.EsaEngine(both.numel(), 4) as eng:
            eng.set_sequence_device(both.data_ptr(), both.numel())
            eng.run(esa.WANT_SUF | esa.WANT_LCP)
            kc.set_index_engine(eng, both.data_ptr(), both.numel(), mirrored=True)
            info = kc.decide(k, c)
            return kc.corrected(), kc.records(), info
