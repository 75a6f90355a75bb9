"""Build and load the HIP engine (libgtamd_esa.so) through its C ABI.

The library is built in-tree (next to this file) so that it travels to the GPU
box with the repository snapshot.  There is no fallback: if it cannot be
loaded, everything that needs it raises.
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "libgtamd_esa.so")
SOURCES = [os.path.join(HERE, "csrc", f) for f in
           ("esa_prims.hip", "esa_engine.hip", "esa_synth.hip", "esa_encode.hip",
            "esa_pck.hip", "esa_comm.hip", "esa_check.hip", "esa_mstat.hip",
            "esa_maxpairs.hip", "esa_qmatch.hip", "esa_spm.hip", "esa_tagmatch.hip",
            "esa_locali.hip", "esa_pckidx.hip", "esa_spmred.hip", "esa_contained.hip",
            "esa_strgraph.hip", "esa_kcorrect.hip")]
HEADERS = [os.path.join(HERE, "csrc", f) for f in ("esa_common.h", "esa_own.h", "esa_index.h", "esa_prims.h", "esa_devutil.h", "esa_msd.h", "esa_msd_blocks.h",
                                                     "esa_jobs.h", "esa_ivwalk.h",
                                                     "esa_pck_replay.h", "esa_mstat_search.h",
                                                     "esa_maxpairs_walk.h", "esa_qmatch_core.h",
                                                     "esa_spm_core.h", "esa_tagmatch_core.h",
                                                     "esa_locali_core.h", "esa_pckidx_core.h",
                                                     "esa_pckidx.h", "esa_pckidx_dec.h",
                                                     "esa_spm_state.h", "esa_spmred_core.h",
                                                     "esa_contained_core.h", "esa_strgraph_core.h",
                                                     "esa_kcorrect_core.h")] + \
          [os.path.join(ROOT, "include", h) for h in ("gtamd_esa.h", "gtamd_encode.h", "gtamd_pck.h",
                                                       "gtamd_check.h", "gtamd_mstat.h",
                                                       "gtamd_maxpairs.h", "gtamd_qmatch.h",
                                                       "gtamd_spm.h", "gtamd_tagmatch.h",
                                                       "gtamd_locali.h", "gtamd_pckidx.h",
                                                       "gtamd_pcktag.h", "gtamd_pcklocali.h",
                                                       "gtamd_spmred.h", "gtamd_contained.h",
                                                       "gtamd_strgraph.h", "gtamd_kcorrect.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in SOURCES + HEADERS)


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 ... -> genometools_amd/libgtamd_esa.so"""
    if not force and not needs_build():
        return LIB_PATH
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           "-shared", "-Wall", "-Wno-unused-function", "-o", LIB_PATH] + SOURCES
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


class EsaStats(ctypes.Structure):
    _fields_ = [("totallength", ctypes.c_uint64),
                ("numberofallsortedsuffixes", ctypes.c_uint64),
                ("longest", ctypes.c_uint64),
                ("largelcpvalues", ctypes.c_uint64),
                ("maxbranchdepth", ctypes.c_uint64),
                ("lcptabsum", ctypes.c_uint64),
                ("prefixlength", ctypes.c_uint32),
                ("refine_rounds", ctypes.c_uint32),
                ("tied_suffixes", ctypes.c_uint64),
                ("pair_suffixes", ctypes.c_uint64),
                ("device_bytes", ctypes.c_uint64),
                ("msd_big_entries", ctypes.c_uint64),
                ("msd_crowded_entries", ctypes.c_uint64),
                ("rank_entries_built", ctypes.c_uint64)]


class EsaTiming(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_float),
                ("keygen_ms", ctypes.c_float),
                ("sort_ms", ctypes.c_float),
                ("finalize_ms", ctypes.c_float),
                ("refine_ms", ctypes.c_float),
                ("tie_fix_ms", ctypes.c_float),
                ("scatter_ms", ctypes.c_float),
                ("scatter_launches", ctypes.c_uint32),
                ("scatter_items", ctypes.c_uint64),
                ("comm_ms", ctypes.c_float),
                ("comm_calls", ctypes.c_uint32),
                ("comm_bytes", ctypes.c_uint64),
                ("alloc_ms", ctypes.c_float),
                ("dominant_kernel", ctypes.c_uint32),
                ("scatter_read_items", ctypes.c_uint64),
                ("scatter_written_items", ctypes.c_uint64)]


class EncodeSummary(ctypes.Structure):     # gtamd_encode_summary, include/gtamd_encode.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("totallength", "numofsequences", "specialcharacters",
                 "realspecialranges")] + \
               [("specialrangestab", ctypes.c_uint64 * 3)] + \
               [(name, ctypes.c_uint64) for name in
                ("lengthofspecialprefix", "lengthofspecialsuffix", "wildcards",
                 "realwildcardranges")] + \
               [("wildcardrangestab", ctypes.c_uint64 * 3)] + \
               [(name, ctypes.c_uint64) for name in
                ("lengthofwildcardprefix", "lengthofwildcardsuffix",
                 "lengthoflongestnonspecial", "minseqlen", "maxseqlen",
                 "equallength")] + \
               [("characterdistribution", ctypes.c_uint64 * 32),
                ("originaldistribution", ctypes.c_uint64 * 256)]


class PckParams(ctypes.Structure):       # gtamd_pck_params, include/gtamd_pck.h
    _fields_ = [("block_size", ctypes.c_uint32), ("bucket_blocks", ctypes.c_uint32),
                ("locate_interval", ctypes.c_uint32), ("feature_toggles", ctypes.c_int32),
                ("with_statistics", ctypes.c_int32)]


class PckInfo(ctypes.Structure):         # gtamd_pck_info
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("file_bytes", "cw_data_pos", "var_data_pos", "range_enc_pos",
                 "num_buckets", "num_regions", "var_bits")] + \
               [("cw_bits", ctypes.c_uint32), ("build_ms", ctypes.c_float)]


class CheckReport(ctypes.Structure):     # gtamd_check_report, include/gtamd_check.h
    _fields_ = [("ok", ctypes.c_int32), ("table", ctypes.c_uint32),
                ("criterion", ctypes.c_uint32), ("checked", ctypes.c_uint32)] + \
               [(name, ctypes.c_uint64) for name in
                ("index", "llv_entry", "pos_a", "pos_b", "claimed", "found", "longest",
                 "largelcpvalues", "maxbranchdepth", "long_claims")] + \
               [("check_ms", ctypes.c_float), ("phase_ms", ctypes.c_float * 5)]


class MstatInfo(ctypes.Structure):       # gtamd_mstat_info, include/gtamd_mstat.h
    _fields_ = [("device_ms", ctypes.c_float), ("reruns", ctypes.c_uint32)] + \
               [(name, ctypes.c_uint64) for name in
                ("positions", "symbols_compared", "device_bytes")]


class MaxPairsInfo(ctypes.Structure):    # gtamd_maxpairs_info, include/gtamd_maxpairs.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("pairs", "run_suffixes", "runs", "segments", "max_pairs_of_one_suffix", "max_len",
                 "walk_steps", "device_bytes")] + [("device_ms", ctypes.c_float)]


class QmatchInfo(ctypes.Structure):      # gtamd_qmatch_info, include/gtamd_qmatch.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("positions", "seeds", "candidates", "max_width", "matches", "search_symbols",
                 "extension_symbols", "device_bytes")] + [("device_ms", ctypes.c_float)]


class SpmInfo(ctypes.Structure):         # gtamd_spm_info, include/gtamd_spm.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("table_entries", "terminal_suffixes", "read_starts", "matches", "max_width",
                 "max_matches_of_one_suffix", "search_symbols", "device_bytes")] + [("device_ms", ctypes.c_float)]


class SpmredInfo(ctypes.Structure):      # gtamd_spmred_info, include/gtamd_spmred.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("table_entries", "terminal_suffixes", "read_starts", "matches", "max_width",
                 "max_matches_of_one_suffix", "search_symbols", "kept", "transitive_same_read",
                 "transitive_other", "contained_sequences", "candidates_examined",
                 "max_candidates_of_one_pair", "letters_compared", "device_bytes")] + \
               [(name, ctypes.c_float) for name in ("device_ms", "spm_ms", "decide_ms")]


class ContainedInfo(ctypes.Structure):   # gtamd_contained_info, include/gtamd_contained.h
    _fields_ = [(name, ctypes.c_uint64) for name in ("table_entries", "sequences", "reads")] + \
               [("count", ctypes.c_uint64 * 5), ("device_bytes", ctypes.c_uint64)] + \
               [(name, ctypes.c_float) for name in ("device_ms", "lists_ms")]


class KcorrectInfo(ctypes.Structure):    # gtamd_kcorrect_info, include/gtamd_kcorrect.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("table_entries", "suffixes", "groups", "untrusted_groups", "records", "dependent", "rounds", "changed")] + \
               [("delta", ctypes.c_int64 * 4), ("device_bytes", ctypes.c_uint64), ("device_ms", ctypes.c_float),
                ("k", ctypes.c_uint32), ("c", ctypes.c_uint32)]


class StrgraphInfo(ctypes.Structure):    # gtamd_strgraph_info, include/gtamd_strgraph.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("reads", "vertices", "matches", "edges", "internal_vertices", "junctions", "paths", "cycles",
                 "cycle_vertices", "contigs", "elements", "total_length", "longest_contig", "device_bytes")] + \
               [(name, ctypes.c_uint32) for name in ("doubling_rounds", "cycle_rounds")] + \
               [(name, ctypes.c_float) for name in ("device_ms", "build_ms", "rank_ms", "select_ms", "scatter_ms", "spell_ms")]


class TagmatchInfo(ctypes.Structure):    # gtamd_tagmatch_info, include/gtamd_tagmatch.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("jobs", "matches", "max_matches_of_one_job", "levels_pushed", "children_examined",
                 "single_walks", "emitted", "device_bytes")] + [("device_ms", ctypes.c_float)]


class LocaliInfo(ctypes.Structure):      # gtamd_locali_info, include/gtamd_locali.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("jobs", "matches", "max_matches_of_one_job", "levels_pushed", "children_examined",
                 "single_walks", "jobs_finished_alone", "emitted", "device_bytes", "groups")] + \
               [("cut_depth", ctypes.c_uint32), ("stack_words", ctypes.c_uint32), ("device_ms", ctypes.c_float)]


# every symbol include/gtamd_esa.h, gtamd_encode.h and gtamd_pck.h declare:
# (restype, argtypes)
_P = ctypes.c_void_p
_U64 = ctypes.c_uint64
_U32 = ctypes.c_uint32
_INT = ctypes.c_int
ABI = {
    "gtamd_device_count": (_INT, []),
    "gtamd_esa_last_error": (ctypes.c_char_p, []),
    "gtamd_recommended_prefixlength": (_U32, [_U32, _U64]),
    "gtamd_abi_selftest": (_INT, [_U64]),
    "gtamd_esa_create": (_P, [_INT, _U64, _U32]),
    "gtamd_esa_destroy": (None, [_P]),
    "gtamd_esa_set_part": (_INT, [_P, _U32, _U32]),
    "gtamd_esa_set_prefixlength": (_INT, [_P, _U32]),
    "gtamd_esa_set_readmode": (_INT, [_P, _INT]),
    "gtamd_esa_set_comm": (_INT, [_P, _P, _P, _P]),
    "gtamd_comm_threads_create": (_P, [_U32]),
    "gtamd_comm_rccl_unique_id": (_INT, [_P]),
    "gtamd_comm_rccl_create": (_P, [_P, _U32, _U32, _INT]),
    "gtamd_comm_attach": (_INT, [_P, _U32, _P, _INT]),
    "gtamd_comm_abort": (None, [_P]),
    "gtamd_esa_set_comm_abort": (_INT, [_P, _P, _P]),
    "gtamd_comm_destroy": (None, [_P]),
    "gtamd_esa_set_sequence_bytes": (_INT, [_P, _P, _U64, _INT]),
    "gtamd_esa_set_sequence_packed": (_INT, [_P, _P, _P, _U64]),
    "gtamd_esa_run": (_INT, [_P, _U32]),
    "gtamd_esa_table_entries": (_U64, [_P, _INT]),
    "gtamd_esa_table_offset": (_U64, [_P]),
    "gtamd_esa_bck_layout": (_INT, [_P, ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                                    ctypes.POINTER(_U64)]),
    "gtamd_esa_table_device": (_P, [_P, _INT]),
    "gtamd_esa_table_copy": (_INT, [_P, _INT, _P, _U64, _U64]),
    "gtamd_esa_get_stats": (_INT, [_P, ctypes.POINTER(EsaStats)]),
    "gtamd_esa_get_timing": (_INT, [_P, ctypes.POINTER(EsaTiming)]),
    "gtamd_esa_build": (_INT, [_P, _U64, _U32, _U32, _P, _P, _P, _P, _U64,
                               ctypes.POINTER(_U64), ctypes.POINTER(EsaStats)]),
    "gtamd_synth_bytes": (_INT, [_INT, _INT, _U64, _U64, _P]),
    # include/gtamd_encode.h
    "gtamd_encoder_create": (_P, [_INT, _INT]),
    "gtamd_encoder_create_map": (_P, [_INT, _P, _U32, ctypes.c_uint]),
    "gtamd_encoder_destroy": (None, [_P]),
    "gtamd_encoder_add_file": (_INT, [_P, ctypes.c_char_p, _P, _U64]),
    "gtamd_encoder_finish": (_INT, [_P]),
    "gtamd_encoder_declined": (_INT, [_P]),
    "gtamd_encoder_num_fastq_records": (_U64, [_P]),
    "gtamd_encoder_get_fastq_records": (_INT, [_P, _P, _P, _P, _U64]),
    "gtamd_encoder_set_symbols": (_INT, [_P, _P, _U64]),
    "gtamd_encoder_length": (_U64, [_P]),
    "gtamd_encoder_device_symbols": (_P, [_P]),
    "gtamd_encoder_copy_symbols": (_INT, [_P, _P, _U64, _U64]),
    "gtamd_encoder_get_summary": (_INT, [_P, ctypes.POINTER(EncodeSummary)]),
    "gtamd_encoder_file_lengths": (_INT, [_P, ctypes.c_size_t, ctypes.POINTER(_U64),
                                          ctypes.POINTER(_U64)]),
    "gtamd_encoder_num_descriptions": (_U64, [_P]),
    "gtamd_encoder_get_descriptions": (_INT, [_P, _P, _P, _P, _U64]),
    "gtamd_encoder_pack_twobit": (_INT, [_P, _INT, ctypes.c_uint, _P, _U64]),
    "gtamd_encoder_pack_specialbits": (_INT, [_P, _P, _U64]),
    "gtamd_encoder_pack_bytecompress": (_INT, [_P, _P, _U64]),
    "gtamd_encoder_get_wildcard_runs": (_INT, [_P, _P, _P, _U64]),
    "gtamd_encoder_get_separators": (_INT, [_P, _P, _U64]),
    "gtamd_encoder_get_timing": (_INT, [_P, ctypes.POINTER(ctypes.c_float),
                                        ctypes.POINTER(ctypes.c_float),
                                        ctypes.POINTER(ctypes.c_float),
                                        ctypes.POINTER(_U64)]),
    # include/gtamd_pck.h
    "gtamd_pck_default_toggles": (_INT, [_U32, _U32, _U32, _INT]),
    "gtamd_pck_create": (_P, [_INT]),
    "gtamd_pck_destroy": (None, [_P]),
    "gtamd_pck_build": (_INT, [_P, _P, _P, _U64, _U32, _U64, ctypes.POINTER(PckParams)]),
    "gtamd_pck_build_host": (_INT, [_P, _P, _P, _U64, _U32, _U64, ctypes.POINTER(PckParams)]),
    "gtamd_pck_build_from_esa": (_INT, [_P, _P, ctypes.POINTER(PckParams)]),
    "gtamd_pck_get_info": (_INT, [_P, ctypes.POINTER(PckInfo)]),
    "gtamd_pck_image_device": (_P, [_P]),
    "gtamd_pck_image_copy": (_INT, [_P, _P, _U64, _U64]),
    "gtamd_pck_ctxmap_build": (_INT, [_P, _P, _U64, _INT, ctypes.POINTER(_INT)]),
    "gtamd_pck_ctxmap_build_from_esa": (_INT, [_P, _P, _INT, ctypes.POINTER(_INT)]),
    "gtamd_pck_ctxmap_build_host": (_INT, [_P, _P, _U64, _INT, ctypes.POINTER(_INT)]),
    "gtamd_pck_ctxmap_bytes": (_U64, [_P]),
    "gtamd_pck_ctxmap_copy": (_INT, [_P, _P, _U64, _U64]),
}

# every symbol include/gtamd_check.h declares.  (A table of its own: ABI is, entry
# for entry, what the three headers above declare.)
CHECK_ABI = {
    "gtamd_check_create": (_P, [_INT]),
    "gtamd_check_destroy": (None, [_P]),
    "gtamd_check_geometry": (None, [ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    "gtamd_check_tables": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64, _P,
                                  ctypes.POINTER(CheckReport)]),
    "gtamd_check_tables_host": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64, _P,
                                       ctypes.POINTER(CheckReport)]),
    "gtamd_check_esa": (_INT, [_P, _P, _P, _U64, _U32, ctypes.POINTER(CheckReport)]),
    "gtamd_check_message": (_INT, [ctypes.POINTER(CheckReport), ctypes.c_char_p,
                                   ctypes.c_size_t]),
}

# every symbol include/gtamd_mstat.h declares
MSTAT_ABI = {
    "gtamd_mstat_create": (_P, [_INT]),
    "gtamd_mstat_destroy": (None, [_P]),
    "gtamd_mstat_geometry": (None, [ctypes.POINTER(_U32), ctypes.POINTER(_U32),
                                    ctypes.POINTER(_U32)]),
    "gtamd_mstat_set_index": (_INT, [_P, _P, _U64, _P, _U32, _U32]),
    "gtamd_mstat_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _U32]),
    "gtamd_mstat_set_index_esa": (_INT, [_P, _P, _P, _U64, _U32]),
    "gtamd_mstat_matstat": (_INT, [_P, _P, _U64, _INT, _U32, _P, _P, _INT]),
    "gtamd_mstat_uniquesub": (_INT, [_P, _P, _U64, _INT, _U32, _P, _INT]),
    "gtamd_mstat_get_info": (_INT, [_P, ctypes.POINTER(MstatInfo)]),
}

# every symbol include/gtamd_maxpairs.h declares
MAXPAIRS_ABI = {
    "gtamd_maxpairs_create": (_P, [_INT]),
    "gtamd_maxpairs_destroy": (None, [_P]),
    "gtamd_maxpairs_set_index": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_maxpairs_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_maxpairs_set_index_esa": (_INT, [_P, _P, _P, _U64]),
    "gtamd_maxpairs_prepare": (_INT, [_P, _U32, ctypes.POINTER(MaxPairsInfo)]),
    "gtamd_maxpairs_emit": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_maxpairs_get_info": (_INT, [_P, ctypes.POINTER(MaxPairsInfo)]),
}

# every symbol include/gtamd_qmatch.h declares
QMATCH_ABI = {
    "gtamd_qmatch_create": (_P, [_INT]),
    "gtamd_qmatch_destroy": (None, [_P]),
    "gtamd_qmatch_geometry": (None, [ctypes.POINTER(_U32), ctypes.POINTER(_U64)]),
    "gtamd_qmatch_set_index": (_INT, [_P, _P, _U64, _P, _U32]),
    "gtamd_qmatch_set_index_host": (_INT, [_P, _P, _U64, _P, _U32]),
    "gtamd_qmatch_set_index_esa": (_INT, [_P, _P, _P, _U64]),
    "gtamd_qmatch_prepare": (_INT, [_P, _P, _U64, _INT, _U32, ctypes.POINTER(QmatchInfo)]),
    "gtamd_qmatch_emit": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_qmatch_get_info": (_INT, [_P, ctypes.POINTER(QmatchInfo)]),
}

# every symbol include/gtamd_spm.h declares
SPM_ABI = {
    "gtamd_spm_create": (_P, [_INT]),
    "gtamd_spm_destroy": (None, [_P]),
    "gtamd_spm_geometry": (None, [ctypes.POINTER(_U32), ctypes.POINTER(_U64)]),
    "gtamd_spm_set_index": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_spm_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_spm_set_index_esa": (_INT, [_P, _P, _P, _U64]),
    "gtamd_spm_prepare": (_INT, [_P, _U32, ctypes.POINTER(SpmInfo)]),
    "gtamd_spm_emit": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_spm_get_info": (_INT, [_P, ctypes.POINTER(SpmInfo)]),
}

# every symbol include/gtamd_tagmatch.h declares
TAGMATCH_ABI = {
    "gtamd_tagmatch_create": (_P, [_INT]),
    "gtamd_tagmatch_destroy": (None, [_P]),
    "gtamd_tagmatch_geometry": (None, [ctypes.POINTER(_U32), ctypes.POINTER(_U64), ctypes.POINTER(_U32)]),
    "gtamd_tagmatch_set_index": (_INT, [_P, _P, _U64, _P, _U32, _U32]),
    "gtamd_tagmatch_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _U32]),
    "gtamd_tagmatch_set_index_esa": (_INT, [_P, _P, _P, _U64, _U32]),
    "gtamd_tagmatch_prepare": (_INT, [_P, _P, _P, _U64, _INT, _U32, _U32, ctypes.POINTER(TagmatchInfo)]),
    "gtamd_tagmatch_emit": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_tagmatch_best_k": (_INT, [_P, _P, _U64]),
    "gtamd_tagmatch_get_info": (_INT, [_P, ctypes.POINTER(TagmatchInfo)]),
}

# every symbol include/gtamd_locali.h declares
LOCALI_ABI = {
    "gtamd_locali_create": (_P, [_INT]),
    "gtamd_locali_destroy": (None, [_P]),
    "gtamd_locali_geometry": (None, [ctypes.POINTER(_U32), ctypes.POINTER(_U64), ctypes.POINTER(_U32),
                                     ctypes.POINTER(_U32)]),
    "gtamd_locali_set_index": (_INT, [_P, _P, _U64, _P, _U32, _U32]),
    "gtamd_locali_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _U32]),
    "gtamd_locali_set_index_esa": (_INT, [_P, _P, _P, _U64, _U32]),
    "gtamd_locali_set_limits": (_INT, [_P, _U32, _U32]),
    "gtamd_locali_prepare": (_INT, [_P, _P, _P, _U64, _INT, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _U32,
                                    ctypes.POINTER(LocaliInfo)]),
    "gtamd_locali_emit": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_locali_get_info": (_INT, [_P, ctypes.POINTER(LocaliInfo)]),
}

class PckidxInfo(ctypes.Structure):      # gtamd_pckidx_info, include/gtamd_pckidx.h
    _fields_ = [(name, ctypes.c_uint64) for name in
                ("rows", "buckets", "regions", "special_rows", "marks", "rot0_row", "image_bytes",
                 "decoded_bytes")] + \
               [(name, ctypes.c_uint32) for name in
                ("numofchars", "block_size", "bucket_blocks", "locate_interval", "feature_toggles",
                 "two_bit")] + [("decode_ms", ctypes.c_float), ("line_rows", ctypes.c_uint32)]


# every symbol include/gtamd_pckidx.h declares
PCKIDX_ABI = {
    "gtamd_pckidx_check_image": (_INT, [_P, _U64]),
    "gtamd_pckidx_create": (_P, [_INT]),
    "gtamd_pckidx_destroy": (None, [_P]),
    "gtamd_pckidx_open_host": (_INT, [_P, _P, _U64]),
    "gtamd_pckidx_open_device": (_INT, [_P, _P, _U64]),
    "gtamd_pckidx_open_builder": (_INT, [_P, _P]),
    "gtamd_pckidx_get_info": (_INT, [_P, ctypes.POINTER(PckidxInfo)]),
    "gtamd_pckidx_decoded_copy": (_INT, [_P, _U32, _P, _U64, ctypes.POINTER(_U64)]),
    "gtamd_pckidx_bwt": (_INT, [_P, _U64, _U64, _P, _INT]),
    "gtamd_pckidx_rank": (_INT, [_P, _P, _P, _U64, _P, _INT]),
    "gtamd_pckidx_locate": (_INT, [_P, _P, _U64, _P, _INT]),
    "gtamd_mstat_set_index_pckidx": (_INT, [_P, _P]),
}

# every symbol include/gtamd_pcktag.h declares
PCKTAG_ABI = {
    "gtamd_tagmatch_set_index_pckidx": (_INT, [_P, _P]),
}

# every symbol include/gtamd_pcklocali.h declares
PCKLOCALI_ABI = {
    "gtamd_locali_set_index_pckidx": (_INT, [_P, _P]),
}

# every symbol include/gtamd_spmred.h declares
SPMRED_ABI = {
    "gtamd_spmred_create": (_P, [_INT]),
    "gtamd_spmred_destroy": (None, [_P]),
    "gtamd_spmred_geometry": (None, [ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "gtamd_spmred_set_index": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_spmred_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_spmred_set_index_esa": (_INT, [_P, _P, _P, _U64]),
    "gtamd_spmred_prepare": (_INT, [_P, _U32, _U32, ctypes.POINTER(SpmredInfo)]),
    "gtamd_spmred_emit": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_spmred_get_info": (_INT, [_P, ctypes.POINTER(SpmredInfo)]),
}

# every symbol include/gtamd_contained.h declares
CONTAINED_ABI = {
    "gtamd_contained_create": (_P, [_INT]),
    "gtamd_contained_destroy": (None, [_P]),
    "gtamd_contained_geometry": (None, [ctypes.POINTER(_U32)]),
    "gtamd_contained_set_index": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_contained_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _P, _P, _U64]),
    "gtamd_contained_set_index_esa": (_INT, [_P, _P, _P, _U64]),
    "gtamd_contained_decide": (_INT, [_P, ctypes.POINTER(ContainedInfo)]),
    "gtamd_contained_verdicts": (_INT, [_P, _P, _INT]),
    "gtamd_contained_compact": (_INT, [_P, _U32, _P, _U64, ctypes.POINTER(_P), ctypes.POINTER(_U64)]),
    "gtamd_contained_result": (_INT, [_P, _P, _INT]),
    "gtamd_contained_get_info": (_INT, [_P, ctypes.POINTER(ContainedInfo)]),
    "gtamd_contained_mirror": (_INT, [_P, _P, _U64, _P]),
    "gtamd_contained_wildcard_flags": (_INT, [_P, _P, _INT]),
    "gtamd_contained_mirror_result": (_INT, [_P, ctypes.POINTER(_P), ctypes.POINTER(_U64)]),
    "gtamd_contained_drop_wildcards": (_INT, [_P, _P, _U64, _P, _U64, ctypes.POINTER(_P), ctypes.POINTER(_U64),
                                              ctypes.POINTER(_U64)]),
}

# every symbol include/gtamd_strgraph.h declares
STRGRAPH_ABI = {
    "gtamd_strgraph_create": (_P, [_INT]),
    "gtamd_strgraph_destroy": (None, [_P]),
    "gtamd_strgraph_geometry": (None, [ctypes.POINTER(_U32), ctypes.POINTER(_U32), ctypes.POINTER(_U64)]),
    "gtamd_strgraph_set_reads": (_INT, [_P, _P, _U64, _INT]),
    "gtamd_strgraph_set_matches": (_INT, [_P, _P, _U64, _INT]),
    "gtamd_strgraph_prepare": (_INT, [_P, _U32, _U32, _U32, ctypes.POINTER(StrgraphInfo)]),
    "gtamd_strgraph_emit": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_strgraph_emit_symbols": (_INT, [_P, ctypes.POINTER(_U64), _P, _U64, _INT, ctypes.POINTER(_U64)]),
    "gtamd_strgraph_get_info": (_INT, [_P, ctypes.POINTER(StrgraphInfo)]),
}

# every symbol include/gtamd_kcorrect.h declares
KCORRECT_ABI = {
    "gtamd_kcorrect_create": (_P, [_INT]),
    "gtamd_kcorrect_destroy": (None, [_P]),
    "gtamd_kcorrect_geometry": (None, [ctypes.POINTER(_U32)]),
    "gtamd_kcorrect_set_index": (_INT, [_P, _P, _U64, _P, _U32, _P, _INT]),
    "gtamd_kcorrect_set_index_host": (_INT, [_P, _P, _U64, _P, _U32, _P, _INT]),
    "gtamd_kcorrect_set_index_esa": (_INT, [_P, _P, _P, _U64, _INT]),
    "gtamd_kcorrect_decide": (_INT, [_P, _U32, _U32, ctypes.POINTER(KcorrectInfo)]),
    "gtamd_kcorrect_records": (_INT, [_P, _P, _INT]),
    "gtamd_kcorrect_apply": (_INT, [_P, _P, _U64, ctypes.POINTER(_P), ctypes.POINTER(_U64)]),
    "gtamd_kcorrect_result": (_INT, [_P, _P, _INT]),
    "gtamd_kcorrect_get_info": (_INT, [_P, ctypes.POINTER(KcorrectInfo)]),
}

_lib = None


def load():
    """ctypes handle with typed entry points; raises if the library is absent"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (needs hipcc); there is no CPU fallback" % LIB_PATH)
        # PyTorch-ROCm bundles its own HIP/HSA runtime next to the system one
        # this library links.  Both work in one process only when torch's
        # copy is mapped first (measured on the MI355X box: the other order
        # leaves torch with "No HIP GPUs are available"), so a Python process
        # that may use torch for device buffers or torch.distributed gets
        # torch imported here, before the library.  C callers are unaffected.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(ABI.items()) + list(CHECK_ABI.items()) + list(MSTAT_ABI.items()) + \
                list(MAXPAIRS_ABI.items()) + list(QMATCH_ABI.items()) + list(SPM_ABI.items()) + list(TAGMATCH_ABI.items()) + \
                list(LOCALI_ABI.items()) + list(PCKIDX_ABI.items()) + list(PCKTAG_ABI.items()) + \
                list(PCKLOCALI_ABI.items()) + list(SPMRED_ABI.items()) + list(CONTAINED_ABI.items()) + \
                list(STRGRAPH_ABI.items()) + list(KCORRECT_ABI.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class EsaError(RuntimeError):
    """mirrors a GtError message: 'gt suffixerator: error: <message>'"""


def check(rc):
    if rc != 0:
        raise EsaError(load().gtamd_esa_last_error().decode())
