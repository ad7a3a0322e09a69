"""ctypes binding of libcropsr_hip.so (C ABI: include/cropsr_hip.h).

The library is the only compute path of this package: if it is missing, or no
HIP device can be opened, the callers raise -- nothing falls back to the CPU.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CROPSR_HIP_LIB: load another build of the same library (kernel A/B experiments)
LIB_PATH = os.environ.get("CROPSR_HIP_LIB") or os.path.join(_HERE, "libcropsr_hip.so")

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
f64p = ctypes.POINTER(ctypes.c_double)
i32p = ctypes.POINTER(ctypes.c_int)


class RowSegment(ctypes.Structure):
    """crp_row_segment (include/cropsr_hip.h): consecutive rows of one contig with their columns, as crp_write_segments takes them."""
    _fields_ = [("contig_text", ctypes.c_void_p), ("contig_len", ctypes.c_uint64), ("chrom", ctypes.c_void_p), ("chrom_len", ctypes.c_uint64),
                ("pos", ctypes.c_void_p), ("minus", ctypes.c_void_p), ("score", ctypes.c_void_p), ("ids", ctypes.c_void_p),
                ("n_rows", ctypes.c_uint64), ("feat_blob", ctypes.c_void_p), ("feat_off", ctypes.c_void_p), ("feat_idx", ctypes.c_void_p),
                ("offtarget", ctypes.c_void_p)]



class RowExtra(ctypes.Structure):
    """crp_row_extra (include/cropsr_hip.h): the CSV join's columns of one segment, as crp_write_segments_cols takes them."""
    _fields_ = [("self_counts", ctypes.c_void_p), ("n_counts", ctypes.c_int), ("self_hit_sum", ctypes.c_void_p)]


class SelectParams(ctypes.Structure):
    """crp_select_params (include/cropsr_hip.h): the thresholds and K of one crp_select_run."""
    _fields_ = [("min_score", ctypes.c_double), ("max_hit_sum", ctypes.c_uint64), ("max_mm0", ctypes.c_uint32), ("k", ctypes.c_int32),
                ("require_cds", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SelectSelfParams(ctypes.Structure):
    """crp_select_self_params (include/cropsr_hip.h): the thresholds, the cut offset and K of one crp_select_run_self."""
    _fields_ = [("max_hit_sum", ctypes.c_uint64), ("max_mm0", ctypes.c_uint32), ("k", ctypes.c_int32), ("cut_offset", ctypes.c_int32),
                ("require_cds", ctypes.c_int32), ("gc_min", ctypes.c_uint32), ("gc_max", ctypes.c_uint32), ("max_t_run", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class SelectPropertyLimits(ctypes.Structure):
    """crp_select_property_limits (include/cropsr_hip.h): the bounds a selection puts on the guide properties."""
    _fields_ = [("gc_min", ctypes.c_uint32), ("gc_max", ctypes.c_uint32), ("max_run", ctypes.c_uint32), ("max_t_run", ctypes.c_uint32),
                ("max_stem", ctypes.c_uint32)]


class SelectRepairLimits(ctypes.Structure):
    """crp_select_repair_limits (include/cropsr_hip.h): the bounds a selection puts on the repair scores."""
    _fields_ = [("min_mh", ctypes.c_uint32), ("min_oof_pct", ctypes.c_uint32)]


class SelectVariantLimits(ctypes.Structure):
    """crp_select_variant_limits (include/cropsr_hip.h): the bounds a selection puts on the variant counts."""
    _fields_ = [("max_site", ctypes.c_uint32), ("max_guide", ctypes.c_uint32), ("max_seed", ctypes.c_uint32), ("max_pam", ctypes.c_uint32)]


class SelectCodingLimits(ctypes.Structure):
    """crp_select_coding_limits (include/cropsr_hip.h): the bounds a selection puts on the coding position of the cut."""
    _fields_ = [("min_pct", ctypes.c_uint32), ("max_pct", ctypes.c_uint32), ("min_transcripts_pct", ctypes.c_uint32)]


class SelectFamilyLimits(ctypes.Structure):
    """crp_select_family_limits (include/cropsr_hip.h): the bounds a selection puts on what a guide hits outside its gene's
    family and on the members it covers; min_members SELECT_ALL_MEMBERS: the family's size."""
    _fields_ = [("max_hit_sum_outside", ctypes.c_uint64), ("max_mm0_outside", ctypes.c_uint32), ("min_members", ctypes.c_uint32)]


class SelectEditWindow(ctypes.Structure):
    """crp_select_edit_window (include/cropsr_hip.h): the base editor's window, protospacer positions from the PAM-distal end."""
    _fields_ = [("lo", ctypes.c_uint32), ("hi", ctypes.c_uint32)]


class SelectEditLimits(ctypes.Structure):
    """crp_select_edit_limits (include/cropsr_hip.h): the bounds a selection puts on the stop codon a base editor writes."""
    _fields_ = [("min_pct", ctypes.c_uint32), ("max_pct", ctypes.c_uint32), ("max_targets", ctypes.c_uint32)]


class SelectSpliceLimits(ctypes.Structure):
    """crp_select_splice_limits (include/cropsr_hip.h): the bounds a selection puts on the splice site a base editor destroys;
    kinds: CRP_SPLICE_DONOR (1) | CRP_SPLICE_ACCEPTOR (2)."""
    _fields_ = [("min_pct", ctypes.c_uint32), ("max_pct", ctypes.c_uint32), ("max_targets", ctypes.c_uint32), ("kinds", ctypes.c_uint32)]


class SelectPairParams(ctypes.Structure):
    """crp_select_pair_params (include/cropsr_hip.h): KP, the distance window, the orientation mask and frameshift of one
    crp_select_run_pairs."""
    _fields_ = [("k", ctypes.c_int32), ("dmin", ctypes.c_uint32), ("dmax", ctypes.c_uint32), ("orientation_mask", ctypes.c_uint32),
                ("frameshift", ctypes.c_int32)]


voidpp = ctypes.POINTER(ctypes.c_void_p)

# every symbol include/cropsr_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "crp_abi_version": (ctypes.c_int, []),
    "crp_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "crp_init": (ctypes.c_int, [ctypes.c_int, voidpp]),
    "crp_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "crp_device_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_int), u64p]),
    "crp_arena_words_for": (ctypes.c_uint64, [ctypes.c_uint64]),
    "crp_arena_words_total": (ctypes.c_uint64, [ctypes.c_uint64]),
    "crp_arena_max_words": (ctypes.c_uint64, []),
    "crp_pack_ascii": (ctypes.c_int, [u8p, ctypes.c_uint64, u64p, u64p, u64p, u64p, ctypes.c_int]),
    "crp_arena_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, voidpp]),
    "crp_arena_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_arena_add_contig_ascii": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_uint64, u64p]),
    "crp_arena_add_contigs_ascii": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), u64p, ctypes.c_uint64, u64p]),
    "crp_arena_add_contig_packed": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p, u64p, u64p,
                                                   ctypes.c_uint64, u64p]),
    "crp_arena_seal": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_arena_tiles": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), u64p, u64p]),
    "crp_arena_stats": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p, u64p]),
    "crp_arena_composition": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p]),
    "crp_scan_score": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, u64p, u64p]),
    "crp_fetch_hits": (ctypes.c_int, [ctypes.c_void_p, u32p, f64p, f64p, u32p, f64p, f64p]),
    "crp_hits_counts": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p]),
    "crp_hits_device": (ctypes.c_int, [ctypes.c_void_p, voidpp, voidpp, voidpp, voidpp]),
    "crp_score_30mers": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_uint64, ctypes.c_int, f64p, f64p]),
    "crp_format_rows": (ctypes.c_int, [u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, ctypes.c_int, u32p, u8p, f64p,
                                       u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, u64p, ctypes.c_int]),
    "crp_write_rows": (ctypes.c_int, [ctypes.c_int, u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, ctypes.c_int, u32p, u8p,
                                      f64p, u8p, ctypes.c_uint64, u64p, ctypes.c_int]),
    "crp_legacy_ids": (ctypes.c_int, [u32p, ctypes.POINTER(ctypes.c_int32), u8p, ctypes.c_uint64, ctypes.c_int]),
    "crp_fasta_table": (ctypes.c_int, [u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, u64p, ctypes.c_uint64, u64p, u64p,
                                       ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "crp_write_rows_ex": (ctypes.c_int, [ctypes.c_int, u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, ctypes.c_int, u32p, u8p,
                                         f64p, u8p, ctypes.c_uint64, u8p, u64p, u32p, u32p, u64p, ctypes.c_int]),
    "crp_write_segments": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, u64p, ctypes.c_int]),
    "crp_write_segments_cols": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, u64p, ctypes.c_int]),
    "crp_write_segments_props": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, u64p,
                                                ctypes.c_int]),
    "crp_comm_unique_id": (ctypes.c_int, [u8p]),
    "crp_comm_init": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_int, ctypes.c_int]),
    "crp_comm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_comm_barrier": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_comm_allreduce_f64": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int, ctypes.c_int]),
    "crp_gather_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, u64p]),
    "crp_gathered_fetch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u32p, f64p, u32p, u32p, f64p, u32p]),
    "crp_gathered_fetch_features": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u32p, u32p]),
    "crp_scan_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_uint64, u32p, f64p, ctypes.c_uint64, u32p, f64p, ctypes.c_uint64, u64p, u64p, u64p, f64p]),
    "crp_scan_stream_prepare": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "crp_host_alloc": (ctypes.c_int, [ctypes.c_uint64, voidpp]),
    "crp_host_free": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_plan_shares": (ctypes.c_int, [u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, u64p, ctypes.c_uint64, u64p]),
    "crp_node_init": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), voidpp]),
    "crp_node_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_node_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "crp_node_size": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_node_ctx": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "crp_node_arena": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "crp_node_arenas": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "crp_node_arena_at": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "crp_node_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "crp_node_transport_note": (ctypes.c_char_p, [ctypes.c_void_p]),
    "crp_node_comm_stuck": (ctypes.c_int, []),
    "crp_node_load": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), u64p, ctypes.c_uint64]),
    "crp_node_plan": (ctypes.c_int, [ctypes.c_void_p, u64p, ctypes.c_uint64, u64p]),
    "crp_node_scan_score": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, u64p, u64p]),
    "crp_node_offtarget": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u64p]),
    "crp_node_annotate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u64p, ctypes.c_int]),
    "crp_node_fetch_offtarget": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p]),
    "crp_node_fetch_features": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p]),
    "crp_node_gather": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "crp_node_counts": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p, u64p]),
    "crp_node_count_scored": (ctypes.c_int, [ctypes.c_void_p, u64p]),
    "crp_node_fetch": (ctypes.c_int, [ctypes.c_void_p, u32p, f64p, u32p, f64p]),
    "crp_node_tables_device": (ctypes.c_int, [ctypes.c_void_p, voidpp, voidpp, voidpp, voidpp]),
    "crp_node_gather_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, f64p, u64p, ctypes.POINTER(ctypes.c_int)]),
    "crp_annotation_build": (ctypes.c_int, [u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, voidpp]),
    "crp_annotation_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_annotation_stats": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p, u64p, u64p, u64p]),
    "crp_annotation_strings": (ctypes.c_int, [ctypes.c_void_p, u8p, u64p]),
    "crp_annotation_seqid": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, voidpp, u64p, voidpp, voidpp, u64p]),
    "crp_annotation_track": (ctypes.c_int, [ctypes.c_void_p, u64p, ctypes.c_uint64, ctypes.c_int, u32p, u32p, ctypes.c_uint64,
                                            u64p]),
    "crp_annotate_set_track": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, ctypes.c_uint64]),
    "crp_annotate_lookup": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p]),
    "crp_offtarget_hist_get": (ctypes.c_int, [ctypes.c_void_p, u32p]),
    "crp_offtarget_hist_set": (ctypes.c_int, [ctypes.c_void_p, u32p]),
    "crp_offtarget_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_offtarget_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u64p, ctypes.c_uint64, u64p]),
    "crp_offtarget_reduce": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_offtarget_solve": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_offtarget_counts": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p]),
    "crp_offtarget_seeds": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p]),
    "crp_search_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, voidpp]),
    "crp_search_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_search_set_budget": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "crp_search_set_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "crp_search_candidates": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p]),
    "crp_search_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, u32p, u64p]),
    "crp_search_fetch": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u8p, u8p, ctypes.c_uint64]),
    "crp_search_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_search_run_bulge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u8p,
                                             ctypes.c_int, ctypes.c_uint64, u32p, u64p]),
    "crp_search_fetch_bulge": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u8p, u8p, u8p, ctypes.c_uint64]),
    "crp_search_set_scheme": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int, ctypes.c_int, f64p]),
    "crp_search_run_scored": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, u32p, u64p,
                                              u64p]),
    "crp_search_set_pair_scheme": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int, ctypes.c_int, i32p, ctypes.c_int, f64p]),
    "crp_search_self_set_pair_scheme": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int, i32p, ctypes.c_int, f64p]),
    "crp_search_self_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_uint64, u64p, voidpp]),
    "crp_search_self_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_search_self_set_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "crp_search_self_set_scheme": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int, f64p]),
    "crp_search_self_sizes": (ctypes.c_int, [ctypes.c_void_p, u64p, u64p, u64p]),
    "crp_search_self_order": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "crp_search_self_compare": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "crp_search_self_fetch": (ctypes.c_int, [ctypes.c_void_p, u32p, u8p, u32p, u32p, u32p, u64p, ctypes.c_uint64]),
    "crp_search_self_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_search_self_set_model": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, f64p, f64p, f64p, ctypes.c_int]),
    "crp_search_self_run_model": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_search_self_fetch_model": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_uint64]),
    "crp_search_self_model_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_search_self_join_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u32p, u64p, u32p, u64p]),
    "crp_search_self_join_device": (ctypes.c_int, [ctypes.c_void_p, voidpp, voidpp, voidpp, voidpp]),
    "crp_search_self_set_families": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u32p, u32p, ctypes.c_uint64, ctypes.c_int]),
    "crp_search_self_family_set_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]),
    "crp_search_self_family_assign": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_search_self_family_compare": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "crp_search_self_family_fetch": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u32p, u64p, u64p, ctypes.c_uint64]),
    "crp_search_self_family_join_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u32p, u64p, u64p, u32p, u32p, u64p, u64p, u32p]),
    "crp_search_self_family_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_annotation_genes": (ctypes.c_int, [ctypes.c_void_p, u64p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), u8p, u64p,
                                            u64p]),
    "crp_annotation_gene_layout": (ctypes.c_int, [ctypes.c_void_p, u64p, ctypes.c_uint64, ctypes.c_int, u32p, u32p, u64p, ctypes.c_uint64,
                                                  u64p]),
    "crp_annotation_cds_flags": (ctypes.c_int, [ctypes.c_void_p, u8p]),
    "crp_select_create": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, ctypes.c_uint64, voidpp]),
    "crp_select_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_select_set_flags": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_uint64]),
    "crp_select_set_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "crp_select_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "crp_select_fetch": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u32p]),
    "crp_select_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_property_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "crp_guide_properties": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p]),
    "crp_guide_properties_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_repair_scores": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u64p, u64p]),
    "crp_repair_scores_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_repair_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "crp_variants_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint64, ctypes.c_int, voidpp]),
    "crp_variants_add_bytes": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_uint64]),
    "crp_variants_finish": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_variants_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "crp_variants_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "crp_variants_stats": (ctypes.c_int, [ctypes.c_void_p, u64p, ctypes.c_int]),
    "crp_variants_chrom": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, voidpp, u64p]),
    "crp_variants_track": (ctypes.c_int, [ctypes.c_void_p, u64p, ctypes.c_uint64, ctypes.c_int, u32p, u32p, ctypes.c_uint64, u64p]),
    "crp_variant_set_track": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, ctypes.c_uint64]),
    "crp_variant_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u32p, u32p]),
    "crp_variant_counts_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_variant_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "crp_sites_set_enzymes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_char_p), u32p, u32p, u32p, ctypes.c_uint64]),
    "crp_site_columns": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, u64p, u64p]),
    "crp_site_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_site_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),
    "crp_select_set_pair_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "crp_select_run_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "crp_select_fetch_pairs": (ctypes.c_int, [ctypes.c_void_p, u32p, u64p, u32p]),
    "crp_select_pairs_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_run_pairs_distinct": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "crp_select_fetch_pairs_distinct": (ctypes.c_int, [ctypes.c_void_p, u32p, u64p, u32p, u32p]),
    "crp_select_pairs_distinct_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_pair_distinct_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "crp_select_run_spaced": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "crp_select_fetch_spaced": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u32p]),
    "crp_select_spaced_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_run_self": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "crp_select_set_self_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "crp_select_fetch_self": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u32p, u32p, u8p, u32p, u32p, u32p, u64p]),
    "crp_select_self_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_self_model": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    "crp_select_fetch_self_model": (ctypes.c_int, [ctypes.c_void_p, f64p]),
    "crp_annotation_gene_coding": (ctypes.c_int, [ctypes.c_void_p, u8p, u32p, u32p]),
    "crp_annotation_coding_layout": (ctypes.c_int, [ctypes.c_void_p, u64p, ctypes.c_uint64, ctypes.c_int, u32p, u32p, u64p, ctypes.c_uint64, u64p,
                                                    u32p, u32p, u32p, ctypes.c_uint64, u64p]),
    "crp_select_set_coding": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, u64p, ctypes.c_uint64, u32p, u32p, u32p, ctypes.c_uint64]),
    "crp_select_set_coding_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "crp_select_coding_eval": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, ctypes.c_uint64, u32p, u32p]),
    "crp_select_set_family": (ctypes.c_int, [ctypes.c_void_p, u32p, u32p, ctypes.c_uint64]),
    "crp_select_set_family_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "crp_select_family_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u32p, u32p, ctypes.c_uint64, u32p, u64p, u32p, u32p, u64p]),
    "crp_select_family_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_family_members": (ctypes.c_int, [ctypes.c_void_p, u32p, ctypes.c_uint64]),
    "crp_select_family_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, u64p, ctypes.c_uint64, ctypes.c_void_p]),
    "crp_select_family_step_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_coding_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_edit_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "crp_select_edit_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u32p, u32p, ctypes.c_uint64, u32p, u32p]),
    "crp_select_edit_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_select_set_splice_limits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "crp_select_splice_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, u32p, u32p, ctypes.c_uint64, u32p, u32p]),
    "crp_select_splice_stats": (ctypes.c_int, [ctypes.c_void_p, f64p, ctypes.c_int]),
    "crp_configure": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "crp_query": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    "crp_build_id": (ctypes.c_char_p, []),
    "crp_profile_read_kind": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, f64p, u64p, ctypes.c_int]),
    "crp_count_scored": (ctypes.c_int, [ctypes.c_void_p, u64p]),
    "crp_profile_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "crp_profile_read": (ctypes.c_int, [ctypes.c_void_p, f64p, u64p, ctypes.c_int]),
    "crp_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
}

CRP_OK = 0
ORDER_BODY4, ORDER_TAIL2, ORDER_DOT1 = 0, 1, 2
OPT_TWO_PASS, OPT_CHAIN_TIMEOUT_US, OPT_TILE_GEOMETRY, OPT_PREFETCH_TILES = 1, 2, 3, 4
GEOMETRIES = {"auto": 0, "large": 1, "small": 2}
Q_CHAIN_TIMEOUTS, Q_TWO_PASS_ACTIVE, Q_COMM_WORLD, Q_COMM_RANK, Q_HBM_FREE, Q_HBM_TOTAL, Q_GATHER_BYTES = 1, 2, 3, 4, 5, 6, 7
KINDS = ("count", "tile_scan", "emit_score", "ot_seed", "ot_ball", "ot_lookup", "gatherv", "ot_reduce",
         "annotate", "properties")  # CRP_K_*
REDUCE_SUM, REDUCE_MAX = 0, 1
COMM_ID_BYTES = 128
GATHER_OFFTARGET, GATHER_PRE, GATHER_FEATURES, GATHER_POS16 = 1, 2, 4, 8
NODE_PEER_COPY, NODE_HOST_GATHER = 16, 32
NODE_OPT_ARENA_WORDS, NODE_OPT_COMM_INIT_TIMEOUT_MS, NODE_OPT_COLLECTIVE_TIMEOUT_MS = 1, 2, 3
TRANSPORTS = {0: "none (one device)", 1: "RCCL (in-library, one process)", 2: "device-to-device copies",
              3: "none: every device's rows over its own PCIe link to the host"}
HALO = 128
NO_FEATURE = 0xFFFFFFFF
SCAN_PRE, SCAN_SEEDS = 1, 2
OT_SEEDS = 1 << 24
OT_NOT_A_SITE, OT_NOT_OWNED = 0xFFFFFFFF, 0xFFFFFFFE
ABI_VERSION = 6
SEARCH_BULGE_DNA, SEARCH_BULGE_RNA = 1, 2
SEARCH_PAM_3PRIME, SEARCH_PAM_5PRIME = 0, 1
SEARCH_SHAPE_DOUBLES = 288
SEARCH_SELF_MAX_MM = 4
SEARCH_PAIR_MAX_PAM = 3
FAMILY_SET_MAX_STEPS = 64  # CRP_FAMILY_SET_MAX_STEPS
# crp_family_step_best (include/cropsr_hip.h): one proposal of crp_select_family_step
FAMILY_STEP_BEST_DTYPE = [("key", "<u8"), ("cover", "<u8"), ("gain", "<u4"), ("tie", "<u4"), ("row", "<u4"), ("gene", "<u4")]
SELECT_ALL_MEMBERS = 0xFFFFFFFF  # crp_select_family_limits.min_members: the size of the gene's family
SELF_UNJOINED_COUNT, SELF_UNJOINED_SUM = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF  # crp_search_self_join_hits: a hit without a guide site's row
SELECT_MAX_K, SELECT_DEFAULT_SLICE_ROWS, SELECT_MIN_SLICE_ROWS, SELECT_NONE = 64, 65536, 64, 0xFFFFFFFF
SELECT_PAIRS_MAX_K, SELECT_PAIRS_MAX_DISTANCE, SELECT_DEFAULT_PAIR_SLICE_ROWS, SELECT_MIN_PAIR_SLICE_ROWS = 64, 65535, 1024, 64
SELECT_MAX_SPACING = 0x7FFFFFFF  # crp_select_run_spaced's largest minimum distance: cut sites lie below 2^31
CRP_ERR_INVALID = -1
CRP_ERR_NO_DEVICE = -2
CRP_ERR_UNSUPPORTED = -7
CRP_ERR_CAPACITY = -6
CRP_ERR_IO = -8
CRP_ERR_COMM = -9
CRP_ERR_NOMEM, CRP_ERR_STATE, CRP_ERR_PEER = -4, -5, -10
# what crp_gather_hits returns on EVERY rank together (agreed on before the exchange starts)
AGREED_GATHER_ERRORS = (CRP_ERR_NOMEM, CRP_ERR_STATE, CRP_ERR_PEER)

_lib = None


class CropsrHipError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        msg = "%s failed: %s" % (what, lib().crp_strerror(status).decode())
        if detail:
            msg += " [%s]" % detail
        super().__init__(msg)


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C cropsr_amd/csrc`).  cropsr_amd has no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH, use_errno=True)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.crp_abi_version() != ABI_VERSION:
            raise ImportError("libcropsr_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(status, what, ctx=None):
    if status != CRP_OK:
        detail = lib().crp_last_error(ctx).decode() if ctx else ""
        raise CropsrHipError(status, what, detail)
