"""Host-side mirror of the reference's index checker over the C ABI.

`gt dev sfxmap -suf -lcp -bwt -esa INDEX` (src/tools/gt_sfxmap.c) answers
whether the tables of an index are those of its sequence, with
gt_suftab_lightweightcheck (src/match/sfx-lwcheck.c:181-337) and
gt_lcptab_lightweightcheck (src/match/sfx-linlcp.c:548).  `EsaChecker` does the
same for tables in host memory, in device memory or resident in an `EsaEngine`
(include/gtamd_check.h states the criteria and what a report's fields mean).

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._consumer import Consumer, ptr
from ._lib import CheckReport, check

SUF, LCP, LLV, BWT = 1, 2, 4, 8                  # CheckResult.table
CRIT_NONE, CRIT_RANGE, CRIT_PERM, CRIT_ORDER, CRIT_BWT, CRIT_LCP0, CRIT_LLV_ENTRY, \
    CRIT_LLV_MISSING, CRIT_LCP_SMALL, CRIT_LCP_LARGE = range(10)   # CheckResult.criterion
NONE = (1 << 64) - 1                             # a field without a value


def geometry():
    """(table entries one workgroup takes, length from which a range of symbols
    to compare goes to the work list); needs no device"""
    tile, long_claim = ctypes.c_uint32(), ctypes.c_uint32()
    _lib.load().gtamd_check_geometry(ctypes.byref(tile), ctypes.byref(long_claim))
    return tile.value, long_claim.value


@dataclass
class CheckResult:
    """gtamd_check_report, and its text"""
    ok: bool
    table: int
    criterion: int
    checked: int
    index: int
    llv_entry: int
    pos_a: int
    pos_b: int
    claimed: int
    found: int
    longest: int
    largelcpvalues: int
    maxbranchdepth: int
    long_claims: int
    check_ms: float
    phase_ms: tuple
    message: str

    def __bool__(self):
        return self.ok


class EsaChecker(Consumer):
    """checker of index tables on one device; TILE and LONG_CLAIM: geometry()"""
    NAME = "check"

    def __init__(self, device=0):
        self.TILE, self.LONG_CLAIM = geometry()
        super().__init__(device)

    def _result(self, rep):
        buf = ctypes.create_string_buffer(512)
        self._lib.gtamd_check_message(ctypes.byref(rep), buf, len(buf))
        fields = {name: getattr(rep, name) for name, _ in rep._fields_}
        fields["ok"] = bool(rep.ok)
        fields["phase_ms"] = tuple(rep.phase_ms)
        return CheckResult(message=buf.value.decode(), **fields)

    def check(self, enc, suf, lcp=None, llv=None, bwt=None):
        """tables in host memory (numpy): enc uint8, n symbols; suf uint32 or
        uint64, n + 1 entries; lcp and bwt uint8, n + 1 entries; llv uint64,
        pairs (table index, value)"""
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        suf = np.ascontiguousarray(suf)
        if suf.dtype not in (np.dtype(np.uint32), np.dtype(np.uint64)):
            raise TypeError("suf must be uint32 or uint64, not %s" % suf.dtype)
        if suf.size != enc.size + 1:
            raise ValueError("suf has %d entries, %d symbols need %d" % (suf.size, enc.size, enc.size + 1))
        lcp = None if lcp is None else np.ascontiguousarray(lcp, dtype=np.uint8)
        bwt = None if bwt is None else np.ascontiguousarray(bwt, dtype=np.uint8)
        for name, tab in (("lcp", lcp), ("bwt", bwt)):
            if tab is not None and tab.size != suf.size:
                raise ValueError("%s has %d entries, not %d" % (name, tab.size, suf.size))
        llv = np.zeros(0, dtype=np.uint64) if llv is None else np.ascontiguousarray(llv, dtype=np.uint64)
        if llv.size % 2 or (llv.size and lcp is None):
            raise ValueError("llv holds pairs and goes with lcp")
        rep = CheckReport()
        check(self._lib.gtamd_check_tables_host(
            self._p, ptr(enc), enc.size, ptr(suf), suf.dtype.itemsize, ptr(lcp),
            ptr(llv) if llv.size else None, llv.size // 2, ptr(bwt), ctypes.byref(rep)))
        return self._result(rep)

    def check_device(self, enc_ptr, n, suf_ptr, suf_bytes=8, lcp_ptr=None, llv_ptr=None, llv_pairs=0,
                     bwt_ptr=None):
        """the same for raw device pointers"""
        rep = CheckReport()
        check(self._lib.gtamd_check_tables(self._p, enc_ptr, n, suf_ptr, suf_bytes, lcp_ptr, llv_ptr,
                                           llv_pairs, bwt_ptr, ctypes.byref(rep)))
        return self._result(rep)

    def check_engine(self, engine, enc_device_ptr, n, want):
        """the tables an EsaEngine holds after run(): want = esa.WANT_SUF, with
        WANT_LCP / WANT_BWT for the tables the run produced; enc_device_ptr: the n
        symbols the tables describe (as the engine's read mode reads them), on
        the device"""
        rep = CheckReport()
        check(self._lib.gtamd_check_esa(self._p, engine._ctx, enc_device_ptr, n, want,
                                        ctypes.byref(rep)))
        return self._result(rep)
