"""Host-side mirror of the decision of `gt readjoiner prefilter` over the C ABI:
which reads of a set are duplicates of, or stand whole inside, another read on
either strand, and the read set without them, decided and compacted on the
device (src/match/rdj-contfinder.c).

`ContainedReads.decide()` gives every read its verdict (KEPT, DUPLICATE, AFFIX,
INTERNAL, SELF_COMPLEMENTARY) and counts them, `verdicts()` hands them out,
`filtered(enc, strict)` the reads that are left.  The index is that of the
MIRRORED set, `spm.mirrored(enc)` or `ContainedReads.mirrored_device`, as
`spm.SuffixPrefixMatches` takes it.  `prefilter(enc, strict)` does all of it for
an encoded read set: the reads with a wildcard dropped, the set mirrored, the
tables built by an `EsaEngine`, the decision and the compaction, the symbols on
the device from the first step to the last.  include/gtamd_contained.h states
the definition, the tie rule, what `strict` adds and where the reference
departs from the definition.

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, as_dict, host_tables, ptr
from ._lib import ContainedInfo

KEPT, DUPLICATE, AFFIX, INTERNAL, SELF_COMPLEMENTARY = range(5)
NAMES = ("kept", "duplicates", "affixes", "internal", "self_complementary")
MASK_DEFAULT = 1 << DUPLICATE | 1 << AFFIX
MASK_STRICT = MASK_DEFAULT | 1 << INTERNAL | 1 << SELF_COMPLEMENTARY


def geometry():
    """reads, sequences or symbols of one workgroup; needs no device"""
    tile = ctypes.c_uint32()
    _lib.load().gtamd_contained_geometry(ctypes.byref(tile))
    return tile.value


def _on_device(a, device):
    """(tensor, address) of the symbols a, a numpy array or a torch tensor, on cuda:device"""
    import torch
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy())
    if a.dtype != torch.uint8:
        raise TypeError("symbols must be uint8, not %s" % a.dtype)
    a = a.to("cuda:%d" % device).contiguous()
    return a, a.data_ptr()


class ContainedReads(Consumer):
    """finder of contained reads over one index on one device"""
    NAME, INFO = "contained", ContainedInfo

    # -- the index of the mirrored set: each call replaces the one before -------
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
        esa.WANT_LCP (forward read mode); enc_device_ptr: the n symbols of the
        mirrored set, on the device.  The engine must outlive the calls."""
        self._call("set_index_esa", engine._ctx, enc_device_ptr, n)

    # -- the decision ------------------------------------------------------------
    @staticmethod
    def _dict(info):
        out = as_dict(info)
        out["count"] = list(info.count)
        out.update(zip(NAMES, out["count"]))
        return out

    def decide(self):
        """the verdict of every read; the info as a dict, with the reads of every
        verdict under `count` and under their names (NAMES)"""
        info = ContainedInfo()
        self._call("decide", ctypes.byref(info))
        return self._dict(info)

    def info(self):
        """gtamd_contained_info of the last decide, as a dict"""
        info = ContainedInfo()
        self._call("get_info", ctypes.byref(info))
        return self._dict(info)

    def verdicts(self, device=False):
        """the verdicts of the last decide, one a read: a numpy uint8 array or,
        with device=True, a torch uint8 tensor on the device"""
        reads = self.info()["reads"]
        if device:
            import torch
            out = torch.empty(reads, dtype=torch.uint8, device="cuda:%d" % self._device)
            self._call("verdicts", out.data_ptr() if reads else None, 1)
            return out
        out = np.empty(reads, dtype=np.uint8)
        self._call("verdicts", ptr(out) if reads else None, 0)
        return out

    def _result(self, count, device):
        """a copy of the `count` symbols of the last compaction"""
        if device:
            import torch
            out = torch.empty(count, dtype=torch.uint8, device="cuda:%d" % self._device)
            self._call("result", out.data_ptr() if count else None, 1)
            return out
        out = np.empty(count, dtype=np.uint8)
        self._call("result", ptr(out) if count else None, 0)
        return out

    def filtered(self, enc=None, strict=False, device=False):
        """the reads that are left after the last decide, in input order, a
        separator between two: a numpy uint8 array or, with device=True, a torch
        tensor.  enc: the symbols of the unmirrored reads, numpy or a torch
        tensor on the device; None: the first half of the index.  strict: the
        reads that stand inside another and those equal to their own reverse
        complement go as well"""
        info = self.info()
        keep, address, n = None, None, (info["table_entries"] - 2) // 2 if info["sequences"] else 0
        if enc is not None:
            keep, address = _on_device(enc, self._device)      # (keep: alive until the call is over)
            n = keep.numel()
        out, count = ctypes.c_void_p(), ctypes.c_uint64()
        self._call("compact", MASK_STRICT if strict else MASK_DEFAULT, address, n, ctypes.byref(out), ctypes.byref(count))
        return self._result(count.value, device)

    # -- what needs no index -----------------------------------------------------
    def mirrored_device(self, enc):
        """spm.mirrored(enc) as a torch tensor on the device, made there"""
        import torch
        keep, address = _on_device(enc, self._device)
        out = torch.empty(2 * keep.numel() + 1, dtype=torch.uint8, device="cuda:%d" % self._device)
        self._call("mirror", address if keep.numel() else None, keep.numel(), out.data_ptr())
        return out

    def without_wildcards(self, enc, separators=None, device=False):
        """(the reads of enc that hold no wildcard, the number of those that do):
        separators: their ascending positions where the caller has them (the
        encoder's), else they are looked for here"""
        if separators is None:
            host = enc if isinstance(enc, np.ndarray) else enc.cpu().numpy()
            separators = np.flatnonzero(host == 255)
        keep, address = _on_device(enc, self._device)
        seps = np.ascontiguousarray(separators, dtype=np.uint64)
        out, count, dropped = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._call("drop_wildcards", address if keep.numel() else None, keep.numel(), ptr(seps) if seps.size else None,
                   seps.size, ctypes.byref(out), ctypes.byref(count), ctypes.byref(dropped))
        return self._result(count.value, device), dropped.value


def prefilter(enc, strict=False, device=0):
    """(kept symbols, verdicts, info) of the encoded read set enc: the reads
    with a wildcard go first (info["wildcard_reads"]), the verdicts are those of
    the reads that are left, numbered in input order"""
    from . import esa
    with ContainedReads(device) as ct:
        reads, dropped = ct.without_wildcards(enc, device=True)
        if reads.numel() == 0:
            info = dict(ContainedReads._dict(ContainedInfo()), wildcard_reads=dropped)
            return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), info
        both = ct.mirrored_device(reads)
        with esa.EsaEngine(both.numel(), 4) as eng:
            eng.set_sequence_device(both.data_ptr(), both.numel())
            eng.run(esa.WANT_SUF | esa.WANT_LCP)
            ct.set_index_engine(eng, both.data_ptr(), both.numel())
            info = ct.decide()
            info["wildcard_reads"] = dropped
            return ct.filtered(strict=strict), ct.verdicts(), info
