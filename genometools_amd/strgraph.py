"""Host-side mirror of `gt readjoiner assembly -readset X` with default options
over the C ABI: the string graph of a list of irreducible suffix-prefix matches,
its unbranched paths and the contigs they spell, on the device
(src/match/rdj-strgraph.c, rdj-contigpaths.c).

`StringGraph.set_reads(enc)` takes the read set (unmirrored, a separator
between two reads), `set_matches(records)` the list -- numpy arrays, or torch
tensors on the device, as `IrreducibleMatches.matches(device=True)` hands them
out -- `prepare(min_len, depthcutoff, lengthcutoff)` builds, ranks and selects,
`contigs()` yields the records (length, depth, first vertex, last vertex,
offset), `symbols()` the letters of all kept contigs side by side;
`all_contigs` does all of it.  `assemble(reads, min_len)` chains
`contained.prefilter` (strict), `IrreducibleMatches` and `StringGraph` on the
device: reads to contigs without a table or the list leaving it.
include/gtamd_strgraph.h states the graph, the order of the paths and what the
fields of the info mean; `fasta` and `vertex_name` give the text of
X.contigs.fas.

Everything here goes through genometools_amd/libgtamd_esa.so (HIP); there is
no CPU implementation in this package.
"""
import ctypes

import numpy as np

from . import _lib
from ._consumer import Consumer, gathered, ptr, record_chunks
from ._lib import StrgraphInfo, check

DEFAULT_CAPACITY = 1 << 20        # contig records (40 bytes each) or symbols of one emit call
DEPTHCUTOFF, LENGTHCUTOFF = 3, 100      # GTAMD_STRGRAPH_DEPTHCUTOFF, GTAMD_STRGRAPH_LENGTHCUTOFF
WIDTH = 60                        # letters of a line of X.contigs.fas


def geometry():
    """(lanes of one workgroup, symbols of one workgroup of the separator
    search, smallest capacity of an emit call); needs no device"""
    tile, sep, least = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    _lib.load().gtamd_strgraph_geometry(ctypes.byref(tile), ctypes.byref(sep), ctypes.byref(least))
    return tile.value, sep.value, least.value


def vertex_name(v):
    """`12E`, `7B`: the read and the end of it, as the reference's contig lines name a vertex"""
    return "%d%s" % (int(v) >> 1, "E" if int(v) & 1 else "B")


def fasta(records, symbols):
    """the bytes of X.contigs.fas for the contig records and their symbols"""
    out = []
    for number, (length, depth, first, last, offset) in enumerate(np.asarray(records).tolist()):
        path = vertex_name(first)
        if depth > 1:
            path += ("-->...-->" if depth > 2 else "-->") + vertex_name(last)
        out.append(b">contig_%d length=%d depth=%d %s\n" % (number, length, depth, path.encode()))
        text = np.frombuffer(b"acgt", dtype=np.uint8)[symbols[offset:offset + length]].tobytes()
        out.extend(text[a:a + WIDTH] + b"\n" for a in range(0, len(text), WIDTH))
    return b"".join(out)


def _is_tensor(a):
    return hasattr(a, "data_ptr")


class StringGraph(Consumer):
    """string graph of one read set and one list of matches on one device"""
    NAME, INFO = "strgraph", StrgraphInfo

    def __init__(self, device=0):
        super().__init__(device)
        self._keep = {}                   # device tensors the library reads: alive as long as it may

    # -- the inputs: each call replaces what was set before -------------------
    def set_reads(self, enc):
        """the read set: uint8 symbols, letters 0..3, a separator (255) between
        two reads, unmirrored; a numpy array, or a torch tensor on the device"""
        if _is_tensor(enc):
            import torch
            if enc.dtype != torch.uint8 or enc.dim() != 1:
                raise TypeError("symbols on the device must be a uint8 tensor of one dimension, not %s %s"
                                % (enc.dtype, tuple(enc.shape)))
            enc = enc.contiguous()
            self._keep["reads"] = enc
            self._call("set_reads", enc.data_ptr() if enc.numel() else None, enc.numel(), 1)
        else:
            enc = np.ascontiguousarray(enc, dtype=np.uint8)
            self._keep.pop("reads", None)
            self._call("set_reads", ptr(enc) if enc.size else None, enc.size, 0)

    def set_matches(self, records):
        """the list: records (suffix_read, prefix_read, len, flags) of shape
        (matches, 4), a numpy uint64 array or a torch int64 tensor on the device"""
        if _is_tensor(records):
            import torch
            if records.dtype != torch.int64 or records.dim() != 2 or records.shape[1] != 4:
                raise TypeError("records on the device must be an int64 tensor of shape (matches, 4), not %s %s"
                                % (records.dtype, tuple(records.shape)))
            records = records.contiguous()
            self._keep["matches"] = records
            self._call("set_matches", records.data_ptr() if records.numel() else None, records.numel() // 4, 1)
        else:
            records = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 4)
            self._keep.pop("matches", None)
            self._call("set_matches", ptr(records) if records.size else None, records.shape[0], 0)

    # -- the contigs ------------------------------------------------------------
    def prepare(self, min_len=0, depthcutoff=DEPTHCUTOFF, lengthcutoff=LENGTHCUTOFF):
        """build the graph of the records of at least min_len letters, rank its
        paths, keep those of at least depthcutoff vertices and lengthcutoff
        letters; the info as a dict"""
        return self._call_info("prepare", min_len, depthcutoff, lengthcutoff)

    def info(self):
        """gtamd_strgraph_info of the last prepare, as a dict"""
        return self._call_info("get_info")

    def contigs(self, capacity=DEFAULT_CAPACITY, device=False, cursor=0):
        """the records of the kept contigs in order, one array per emit call:
        numpy uint64 arrays of shape (contigs, 5) -- length, depth, first vertex,
        last vertex, offset -- or torch int64 tensors on the device"""
        yield from record_chunks(self._fn("emit"), self._p, capacity, device, self._device, cursor, columns=5)

    def symbols(self, capacity=DEFAULT_CAPACITY, device=False, cursor=0):
        """the symbols of the kept contigs side by side, one array of at most
        `capacity` per emit call: numpy uint8 arrays, or torch uint8 tensors on
        the device, which the next call overwrites"""
        cursor, written = ctypes.c_uint64(cursor), ctypes.c_uint64(0)
        if device:
            import torch
            buf = torch.empty(max(capacity, 1), dtype=torch.uint8, device="cuda:%d" % self._device)
            address = buf.data_ptr()
        else:
            buf = np.empty(max(capacity, 1), dtype=np.uint8)
            address = buf.ctypes.data
        while True:
            check(self._fn("emit_symbols")(self._p, ctypes.byref(cursor), address, capacity, int(device),
                                           ctypes.byref(written)))
            if written.value == 0:
                return
            yield buf[:written.value] if device else buf[:written.value].copy()

    def all_contigs(self, min_len=0, depthcutoff=DEPTHCUTOFF, lengthcutoff=LENGTHCUTOFF, capacity=DEFAULT_CAPACITY):
        """(records of shape (contigs, 5), all symbols, info) as numpy arrays"""
        info = self.prepare(min_len, depthcutoff, lengthcutoff)
        records = gathered(self.contigs(capacity), columns=5)
        chunks = list(self.symbols(capacity))
        return records, (np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)), info


def assemble(reads, min_len, depthcutoff=DEPTHCUTOFF, lengthcutoff=LENGTHCUTOFF, device=0):
    """(contig records, symbols, info) of the encoded read set `reads`: the
    reads without wildcards, duplicates and contained reads (contained.prefilter,
    strict), their irreducible suffix-prefix matches of at least min_len letters
    on both strands (spmred.IrreducibleMatches) and the contigs of the string
    graph of these, every step on the device.  info: that of the string graph,
    with the prefilter's under "prefilter" and the matcher's under "overlap" """
    import torch
    from . import esa
    from .contained import ContainedReads
    from .spmred import IrreducibleMatches
    with ContainedReads(device) as ct:
        clean, dropped = ct.without_wildcards(reads, device=True)
        kept = clean
        pre = {"wildcard_reads": dropped}
        if clean.numel():
            both = ct.mirrored_device(clean)
            with esa.EsaEngine(both.numel(), 4) as eng:
                eng.set_sequence_device(both.data_ptr(), both.numel())
                eng.run(esa.WANT_SUF | esa.WANT_LCP)
                ct.set_index_engine(eng, both.data_ptr(), both.numel())
                pre.update(ct.decide())
                kept = ct.filtered(strict=True, device=True)
        with StringGraph(device) as graph:
            graph.set_reads(kept)
            records = torch.zeros((0, 4), dtype=torch.int64, device="cuda:%d" % device)
            over = {}
            if kept.numel():
                both = ct.mirrored_device(kept)
                with esa.EsaEngine(both.numel(), 4) as eng, IrreducibleMatches(device) as im:
                    eng.set_sequence_device(both.data_ptr(), both.numel())
                    eng.run(esa.WANT_SUF | esa.WANT_LCP)
                    im.set_index_engine(eng, both.data_ptr(), both.numel())
                    over = im.prepare(min_len)
                    chunks = [c.clone() for c in im.matches(device=True)]
                    if chunks:
                        records = torch.cat(chunks)
            graph.set_matches(records)
            found, symbols, info = graph.all_contigs(0, depthcutoff, lengthcutoff)
            info["prefilter"], info["overlap"] = pre, over
            return found, symbols, info
