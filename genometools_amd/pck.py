"""Host-side mirror of the reference's packed-index construction over the C ABI.

`gt packedindex trsuftab INDEX` (src/tools/gt_packedindex_trsuftab.c:44-79)
builds INDEX.bdx from the tables of a suffix-array project through
gt_trSuftab2BWTSeq (src/match/eis-bwtseq-construct.c:64-92).  `PackedIndex`
does the same from tables resident on the device (include/gtamd_pck.h); the
option names are the tool's (-bsize, -blbuck, -locfreq, -locbitmap).

`PackedIndexReader` opens such an image again (include/gtamd_pckidx.h): it
decodes it once on the device and answers, for batches, what the reference's
BWTSeq answers on the host -- the BWT symbol of a row, the occurrences of a
letter before a row (BWTSeqTransformedOcc), the text position of a row
(gt_BWTSeqLocateMatch).  `mstat.MatchStats.set_index_packed` searches through it.

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, ptr
from ._lib import PckidxInfo, PckInfo, PckParams, check

LOCATE_BITMAP, LOCATE_COUNT, REVERSIBLY_SORTED = 1, 2, 4


def default_toggles(bsize=8, blbuck=8, locfreq=16, locbitmap=None, sprank=False):
    """the feature toggles gt_computePackedIndexDefaults derives
    (src/match/eis-bwtseq-param.c:89-103); locbitmap None = option not given"""
    return _lib.load().gtamd_pck_default_toggles(
        bsize, blbuck, locfreq, -1 if locbitmap is None else int(bool(locbitmap))) | \
        (REVERSIBLY_SORTED if sprank else 0)


class PackedIndex:
    """builder of INDEX.bdx images on one device"""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._p = self._lib.gtamd_pck_create(device)
        if not self._p:
            raise _lib.EsaError(self._lib.gtamd_esa_last_error().decode())

    def close(self):
        if self._p:
            self._lib.gtamd_pck_destroy(self._p)
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

    @staticmethod
    def _params(bsize, blbuck, locfreq, locbitmap, mkindex, sprank):
        return PckParams(bsize, blbuck, locfreq,
                         default_toggles(bsize, blbuck, locfreq, locbitmap, sprank),
                         int(bool(mkindex)))

    def build_from_esa(self, engine, bsize=8, blbuck=8, locfreq=16, locbitmap=None,
                       mkindex=False, sprank=False):
        """from an EsaEngine whose last run produced .suf and .bwt; mkindex: the
        file of `gt packedindex mkindex` (with sequence statistics) instead of
        the one of `gt packedindex trsuftab`"""
        pp = self._params(bsize, blbuck, locfreq, locbitmap, mkindex, sprank)
        check(self._lib.gtamd_pck_build_from_esa(self._p, engine._ctx, ctypes.byref(pp)))

    def build(self, bwt_ptr, suf_ptr, total_len, numofchars, longest, bsize=8, blbuck=8,
              locfreq=16, locbitmap=None, mkindex=False, sprank=False):
        """from raw device pointers of the .bwt and .suf tables"""
        pp = self._params(bsize, blbuck, locfreq, locbitmap, mkindex, sprank)
        check(self._lib.gtamd_pck_build(self._p, bwt_ptr, suf_ptr, total_len, numofchars,
                                        longest, ctypes.byref(pp)))

    def context_map_from_esa(self, engine, ilog=-1):
        """INDEX.<ilog>cxm (-ctxilog; -1: the automatic interval) from the engine's
        suffix array: (interval log used, bytes of the file)"""
        used = ctypes.c_int()
        check(self._lib.gtamd_pck_ctxmap_build_from_esa(self._p, engine._ctx, ilog,
                                                        ctypes.byref(used)))
        n = self._lib.gtamd_pck_ctxmap_bytes(self._p)
        out = np.empty(n, dtype=np.uint8)
        check(self._lib.gtamd_pck_ctxmap_copy(self._p, out.ctypes.data_as(ctypes.c_void_p), 0, n))
        return used.value, out

    def info(self):
        inf = PckInfo()
        check(self._lib.gtamd_pck_get_info(self._p, ctypes.byref(inf)))
        return {name: getattr(inf, name) for name, _ in inf._fields_}

    def device_pointer(self):
        return self._lib.gtamd_pck_image_device(self._p)

    def image(self, offset=0, count=None):
        """bytes [offset, offset + count) of INDEX.bdx"""
        total = self.info()["file_bytes"]
        count = total - offset if count is None else count
        out = np.empty(count, dtype=np.uint8)
        if count:
            check(self._lib.gtamd_pck_image_copy(self._p, out.ctypes.data_as(ctypes.c_void_p),
                                                 offset, count))
        return out


def check_image(image):
    """the checks every open makes before a kernel runs, on the bytes of an
    INDEX.bdx in host memory; raises EsaError with the refusal.  Needs no device."""
    image = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray))
                                 else image, dtype=np.uint8)
    check(_lib.load().gtamd_pckidx_check_image(ptr(image), image.size))


class PackedIndexReader(Consumer):
    """an INDEX.bdx image, decoded on one device"""
    NAME, INFO = "pckidx", PckidxInfo
    PARTS = ("rows", "aux", "marks", "marks_before", "stored", "special_ranks", "region_starts", "count")

    # -- the image: each call replaces the one before -------------------------
    def open(self, image):
        """the bytes of a file (bytes or numpy uint8) this project or GenomeTools wrote"""
        image = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray))
                                     else image, dtype=np.uint8)
        self._call("open_host", ptr(image), image.size)
        return self

    def open_device(self, image_ptr, size):
        """an image in device memory, which is only read during the call"""
        self._call("open_device", image_ptr, size)
        return self

    def open_builder(self, builder):
        """the image a `PackedIndex` still holds after a build: nothing leaves the device"""
        self._call("open_builder", builder._p)
        return self

    def info(self):
        """gtamd_pckidx_info as a dict"""
        return self._call_info("get_info")

    def decoded(self, part):
        """one part of the decoded form (PARTS) as bytes"""
        size = ctypes.c_uint64()
        idx = self.PARTS.index(part)
        self._call("decoded_copy", idx, None, 0, ctypes.byref(size))
        out = np.empty(size.value, dtype=np.uint8)
        self._call("decoded_copy", idx, ptr(out), out.size, ctypes.byref(size))
        return out

    # -- the batch calls --------------------------------------------------------
    def bwt(self, row0=0, count=None):
        """BWT symbols of rows [row0, row0 + count): letters, 254, 255"""
        count = self.info()["rows"] - row0 if count is None else count
        out = np.empty(count, dtype=np.uint8)
        self._call("bwt", row0, count, ptr(out), 0)
        return out

    def rank(self, symbols, rows):
        """occurrences of letter symbols[i] in rows [0, rows[i]); specials count for nobody"""
        symbols = np.ascontiguousarray(symbols, dtype=np.uint8)
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        if symbols.size != rows.size:
            raise ValueError("%d symbols for %d rows" % (symbols.size, rows.size))
        out = np.empty(rows.size, dtype=np.uint64)
        self._call("rank", ptr(symbols), ptr(rows), rows.size, ptr(out), 0)
        return out

    def locate(self, rows):
        """text position of the suffix of every row"""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.empty(rows.size, dtype=np.uint64)
        self._call("locate", ptr(rows), rows.size, ptr(out), 0)
        return out

    def bwt_device(self, row0, count, out_ptr):
        self._call("bwt", row0, count, out_ptr, 1)

    def rank_device(self, symbols_ptr, rows_ptr, count, out_ptr):
        self._call("rank", symbols_ptr, rows_ptr, count, out_ptr, 1)

    def locate_device(self, rows_ptr, count, out_ptr):
        self._call("locate", rows_ptr, count, out_ptr, 1)
