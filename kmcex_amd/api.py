"""Python mirror of the reference's KModel interface (kmodel.hpp) over the C ABI of libkmx.so.

Names follow the reference / its README: ``get_model``, ``init`` (``init_KModel``), ``kmer_to_occ``,
``save`` (``save_model``), ``load`` (``load_model``).  All compute happens in the HIP library; this module
only marshals pointers.  It raises ``KmxError`` (there is no CPU fallback) when the library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

_PKG = os.path.dirname(os.path.abspath(__file__))


class KmxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"kmx error {code}: {msg}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [("n_total", C.c_uint64), ("n_km", C.c_uint64), ("n_bf", C.c_uint64 * 3),
                ("attempts", C.c_uint64), ("successes", C.c_uint64), ("rest_entries", C.c_uint64),
                ("km_byte_size", C.c_uint64), ("byte_km_back", C.c_uint64),
                ("byte_bf", C.c_uint64 * 3), ("byte_bf_back", C.c_uint64 * 3),
                ("fast_commits", C.c_uint64), ("contended", C.c_uint64), ("finisher_iters", C.c_uint64),
                ("blocks", C.c_uint64), ("rounds", C.c_uint64),
                ("k", C.c_int32), ("ci", C.c_int32), ("cs", C.c_int32), ("nh", C.c_int32), ("nb", C.c_int32),
                ("bf_num", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32), ("rest_bytes", C.c_uint64),
                ("piped_attempts", C.c_uint64), ("piped_commits", C.c_uint64),
                ("piped_gathers", C.c_uint64), ("piped_atomics", C.c_uint64),
                ("query_neighbour_calls", C.c_uint64), ("query_accounted", C.c_uint64)]


# every symbol include/kmx.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = [
    "kmx_last_error", "kmx_device_count", "kmx_create", "kmx_destroy", "kmx_set_stream", "kmx_build_from_kmc",
    "kmx_begin", "kmx_insert_batch", "kmx_insert_batch_dev", "kmx_finish", "kmx_build_dev", "kmx_build_host",
    "kmx_query_packed", "kmx_query_packed_dev", "kmx_query_ascii", "kmx_query_strings", "kmx_save", "kmx_load", "kmx_get_stats",
    "kmx_download", "kmx_debug_hash", "kmx_debug_min_kmer", "kmx_occubin", "kmx_microbench", "kmx_last_build_seconds",
    "kmx_set_profile", "kmx_get_kernel_times", "kmx_kmc_info", "kmx_kmc_read", "kmx_debug_mod",
    "kmx_count_classes_dev", "kmx_shard_begin", "kmx_shard_classify_dev", "kmx_ring_msg_bytes", "kmx_ring_round_dev",
    "kmx_ring_stale_dup_dev", "kmx_shard_local", "kmx_shard_complete", "kmx_dev_view", "kmx_or_words_dev",
    "kmx_debug_pack_strings", "kmx_kernel_classes", "kmx_abi_version", "kmx_get_stats_n",
    "kmx_create_on", "kmx_build_from_kmc_multi", "kmx_build_from_kmc_multi_ex", "kmx_range_begin", "kmx_range_buffers", "kmx_range_emit_dev", "kmx_range_verdict_dev", "kmx_range_resolve_dev", "kmx_range_commit_dev", "kmx_range_flush_dev", "kmx_range_inband", "kmx_range_verdict_inband_dev", "kmx_range_commit_inband_dev",
    "kmx_query_seqs", "kmx_query_seqs_dev", "kmx_summarise_seqs", "kmx_summarise_seqs_dev",
    "kmx_correct_seqs", "kmx_correct_seqs_dev",
    "kmx_edit_seqs", "kmx_edit_seqs_dev", "kmx_apply_edits", "kmx_apply_edits_dev", "kmx_polish_seqs", "kmx_polish_seqs_dev",
    "kmx_extend_seqs", "kmx_extend_seqs_dev",
    "kmx_count_begin", "kmx_count_seqs", "kmx_count_seqs_dev", "kmx_count_finish", "kmx_count_listing", "kmx_build_from_reads",
    "kmx_unitigs", "kmx_unitigs_dev", "kmx_count_unitigs", "kmx_count_unitigs_dev", "kmx_unitigs_last_phases",
    "kmx_unitig_graph", "kmx_unitig_graph_dev", "kmx_count_unitig_graph", "kmx_count_unitig_graph_dev", "kmx_unitig_graph_last_phases",
    "kmx_unitig_graph_clean", "kmx_unitig_graph_clean_dev", "kmx_count_unitig_graph_clean", "kmx_count_unitig_graph_clean_dev", "kmx_unitig_clean_last_phases",
    "kmx_unitig_map_begin", "kmx_unitig_map_begin_dev", "kmx_count_unitig_map_begin", "kmx_count_unitig_map_begin_dev", "kmx_unitig_map_seqs", "kmx_unitig_map_seqs_dev", "kmx_unitig_map_end",
    "kmx_unitig_walk_segs", "kmx_unitig_walk_segs_dev",
    "kmx_unitig_contigs", "kmx_unitig_contigs_dev", "kmx_unitig_contigs_last_phases",
    "kmx_unitig_walk_through", "kmx_unitig_walk_through_dev",
    "kmx_unitig_resolve", "kmx_unitig_resolve_dev", "kmx_unitig_resolve_last_phases",
    "kmx_unitig_pair_walks", "kmx_unitig_pair_walks_dev",
    "kmx_unitig_scaffold", "kmx_unitig_scaffold_dev", "kmx_unitig_scaffold_last_phases",
    "kmx_unitig_pair_paths", "kmx_unitig_pair_paths_dev", "kmx_unitig_pair_paths_last_phases",
    "kmx_unitig_pair_reduce", "kmx_unitig_pair_reduce_dev", "kmx_unitig_pair_reduce_last_phases",
    "kmx_unitig_pair_lift", "kmx_unitig_pair_lift_dev", "kmx_unitig_pair_lift_fold_variant", "kmx_unitig_pair_lift_last_phases",
    "kmx_unitig_scaffold_fill", "kmx_unitig_scaffold_fill_dev", "kmx_unitig_scaffold_fill_last_phases",
]


class SeqSummary(C.Structure):
    """kmx_seq_summary of include/kmx.h: one per sequence, 64 bytes"""
    _fields_ = [("n_windows", C.c_uint64), ("sum", C.c_uint64), ("min", C.c_int32), ("max", C.c_int32),
                ("n_ge", C.c_uint64 * 3), ("first_below", C.c_uint64), ("last_below", C.c_uint64)]


# the same record as a NumPy structured dtype (what KModel.seq_summary_flat returns)
SEQ_SUMMARY_DTYPE = np.dtype([("n_windows", "<u8"), ("sum", "<u8"), ("min", "<i4"), ("max", "<i4"), ("n_ge", "<u8", (3,)),
                              ("first_below", "<u8"), ("last_below", "<u8")])
SEQ_THRESHOLDS = 3
# kmx_seq_correction of include/kmx.h (what KModel.seq_correct_flat returns beside the corrected bases): 8 x uint64
SEQ_CORRECTION_DTYPE = np.dtype([(f, "<u8") for f in ("n_windows", "n_weak", "n_runs", "n_sites", "n_corrected", "n_ambiguous", "n_unfixable", "reserved")])
# kmx_seq_edits of include/kmx.h (what KModel.seq_edit_flat returns beside the edit list): 10 x uint64
SEQ_EDITS_DTYPE = np.dtype([(f, "<u8") for f in ("n_windows", "n_weak", "n_runs", "n_sites", "n_sub", "n_del", "n_ins", "n_ambiguous", "n_unfixable", "out_len")])
EDIT_OPS_SUB, EDIT_OPS_DEL, EDIT_OPS_INS = 1, 2, 4
# kmx_seq_polish of include/kmx.h (what KModel.seq_polish_flat returns beside the reads): 12 x uint64
SEQ_POLISH_DTYPE = np.dtype([(f, "<u8") for f in ("n_passes", "converged", "n_sub", "n_del", "n_ins", "out_len",
                                                   "n_windows", "n_weak", "n_runs", "n_sites", "n_ambiguous", "n_unfixable")])
POLISH_MAX_PASSES = 16
EDIT_SUB, EDIT_DEL, EDIT_INS = 1, 2, 3
# kmx_seq_extension of include/kmx.h (what KModel.seq_extend_flat returns beside the rows of appended bases): 32 bytes
SEQ_EXTENSION_DTYPE = np.dtype([("n_ext", "<u4"), ("stop", "<u4"), ("seed_occ", "<i4"), ("min_occ", "<i4"), ("max_occ", "<i4"), ("n_lookahead", "<u4"), ("sum_occ", "<u8")])
SEQ_EXTENSION_STOPS = {1: "DEAD_END", 2: "BRANCH", 3: "JOIN", 4: "CYCLE", 5: "MAX_EXT", 6: "BAD_SEED"}
_REVCOMP = np.arange(256, dtype=np.uint8)
_REVCOMP[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)


class Unitig(C.Structure):
    """kmx_unitig of include/kmx.h: one per unitig, 40 bytes"""
    _fields_ = [("n_kmers", C.c_uint64), ("sum_count", C.c_uint64), ("min_count", C.c_uint32), ("max_count", C.c_uint32),
                ("first_node", C.c_uint64), ("circular", C.c_uint8), ("n_pred", C.c_uint8), ("n_succ", C.c_uint8),
                ("first_fwd", C.c_uint8), ("reserved", C.c_uint8 * 4)]


# the same record as a NumPy structured dtype (what KModel.unitigs / count_unitigs return beside the strings)
UNITIG_DTYPE = np.dtype([("n_kmers", "<u8"), ("sum_count", "<u8"), ("min_count", "<u4"), ("max_count", "<u4"), ("first_node", "<u8"),
                         ("circular", "u1"), ("n_pred", "u1"), ("n_succ", "u1"), ("first_fwd", "u1"), ("reserved", "u1", (4,))])
UNITIG_PHASES = ["adjacency", "links", "ranking", "emit"]
UNITIG_GRAPH_PHASES = UNITIG_PHASES + ["unitig_links"]
UNITIG_CLEAN_PHASES = UNITIG_GRAPH_PHASES + ["clean"]
CLEAN_TIPS, CLEAN_ISLANDS, CLEAN_BUBBLES = 1, 2, 4
CLEAN_MAX_ROUNDS = 64


class CleanParams(C.Structure):
    """kmx_clean_params of include/kmx.h: 16 bytes"""
    _fields_ = [("ops", C.c_uint32), ("max_tip", C.c_uint32), ("max_bubble", C.c_uint32), ("max_rounds", C.c_uint32)]


class CleanStats(C.Structure):
    """kmx_clean_stats of include/kmx.h: 64 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("rounds_run", "converged", "n_tips", "n_islands", "n_bubbles", "n_kmers_removed", "n_unitigs_before", "n_links_before")]


class MapSegment(C.Structure):
    """kmx_map_segment of include/kmx.h: a run of a read's windows along one oriented unitig, 24 bytes"""
    _fields_ = [("pos", C.c_uint64), ("n_windows", C.c_uint32), ("o", C.c_uint32), ("off", C.c_uint32), ("reserved", C.c_uint32)]


class SeqMap(C.Structure):
    """kmx_seq_map of include/kmx.h: one per read, 64 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_windows", "n_mapped", "n_segments", "n_gaps", "first_mapped", "last_mapped", "longest", "reserved")]


# the same two as NumPy structured dtypes (what KModel.seq_to_unitigs returns)
SEQ_SEGMENT_DTYPE = np.dtype([("pos", "<u8"), ("n_windows", "<u4"), ("o", "<u4"), ("off", "<u4"), ("reserved", "<u4")])
SEQ_MAP_DTYPE = np.dtype([(f, "<u8") for f in ("n_windows", "n_mapped", "n_segments", "n_gaps", "first_mapped", "last_mapped", "longest", "reserved")])


class WalkParams(C.Structure):
    """kmx_walk_params of include/kmx.h: 16 bytes"""
    _fields_ = [("max_gap", C.c_uint32), ("max_indel", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class Walk(C.Structure):
    """kmx_walk of include/kmx.h: a maximal chain of joined segments of one read, 80 bytes"""
    _fields_ = ([(f, C.c_uint64) for f in ("pos", "n_span", "n_mapped", "n_covered", "first_seg", "first_step")] +
                [(f, C.c_uint32) for f in ("n_segs", "n_steps", "off_first", "off_last", "n_inside", "n_across")] + [("indel", C.c_int32), ("reserved", C.c_uint32)])


class WalkStats(C.Structure):
    """kmx_walk_stats of include/kmx.h: 64 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_walks", "n_steps", "n_edge", "n_inside", "n_across", "n_unlinked", "n_breaks", "reserved")]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_walk as a NumPy structured dtype (what KModel.unitig_walks_flat returns)
WALK_DTYPE = np.dtype([(f, "<u8") for f in ("pos", "n_span", "n_mapped", "n_covered", "first_seg", "first_step")] +
                      [(f, "<u4") for f in ("n_segs", "n_steps", "off_first", "off_last", "n_inside", "n_across")] + [("indel", "<i4"), ("reserved", "<u4")])


class ContigParams(C.Structure):
    """kmx_contig_params of include/kmx.h: 16 bytes"""
    _fields_ = [("min_reads", C.c_uint64), ("ratio", C.c_uint32), ("reserved", C.c_uint32)]


class ContigStats(C.Structure):
    """kmx_contig_stats of include/kmx.h: 64 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_links", "n_kept", "n_below_min", "n_below_ratio", "n_chain", "n_contigs", "n_circular", "n_multi")]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_contig and kmx_contig_place as NumPy structured dtypes (what KModel.unitig_contigs_flat returns): 64 and 8 bytes
CONTIG_DTYPE = np.dtype([("n_kmers", "<u8"), ("sum_count", "<u8"), ("min_count", "<u4"), ("max_count", "<u4"), ("first_step", "<u8"), ("n_steps", "<u4"),
                         ("circular", "u1"), ("n_pred", "u1"), ("n_succ", "u1"), ("reserved", "u1"), ("min_support", "<u8"), ("sum_support", "<u8"), ("reserved2", "<u8")])
CONTIG_PLACE_DTYPE = np.dtype([("oc", "<u4"), ("off", "<u4")])


class ThroughStats(C.Structure):
    """kmx_through_stats of include/kmx.h: 64 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_walks", "n_steps", "n_interior", "n_added", "n_missing")] + [("reserved", C.c_uint64 * 3)]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_ if f != "reserved"}


class ResolveParams(C.Structure):
    """kmx_resolve_params of include/kmx.h: 16 bytes"""
    _fields_ = [("min_reads", C.c_uint64), ("max_cross", C.c_uint64)]


class ResolveStats(C.Structure):
    """kmx_resolve_stats of include/kmx.h: 64 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_candidates", "n_resolved", "n_crossed", "n_unsupported", "n_ambiguous", "n_copies_added", "n_unitigs_out", "reserved")]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_resolve_place as a NumPy structured dtype (what KModel.unitig_resolve_flat returns): 8 bytes
RESOLVE_PLACE_DTYPE = np.dtype([("first", "<u4"), ("n_copies", "<u4")])


class PairParams(C.Structure):
    """kmx_pair_params of include/kmx.h: 16 bytes"""
    _fields_ = [(f, C.c_uint32) for f in ("min_mapped", "max_dist", "bin_width", "n_bins")]


class Pair(C.Structure):
    """kmx_pair of include/kmx.h: where the two mates of a pair lie, 64 bytes"""
    _fields_ = ([("walk_a", C.c_uint64), ("walk_b", C.c_uint64)] + [(f, C.c_uint32) for f in ("cls", "edge", "oa", "xa", "ob", "xb")] +
                [("d", C.c_int64), ("frag", C.c_int64), ("reserved", C.c_uint64)])


class PairLink(C.Structure):
    """kmx_pair_link of include/kmx.h: the pairs between two oriented unitigs, 32 bytes"""
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("n_pairs", C.c_uint64), ("sum_dist", C.c_uint64), ("min_dist", C.c_uint32), ("max_dist", C.c_uint32)]


class PairStats(C.Structure):
    """kmx_pair_stats of include/kmx.h: 80 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_pairs", "n_none", "n_single", "n_same", "n_negative", "n_inverted", "n_link", "n_adjacent", "n_far", "reserved")]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_pair and kmx_pair_link as NumPy structured dtypes (what KModel.unitig_pairs_flat returns): 64 and 32 bytes
PAIR_DTYPE = np.dtype([("walk_a", "<u8"), ("walk_b", "<u8")] + [(f, "<u4") for f in ("cls", "edge", "oa", "xa", "ob", "xb")] + [("d", "<i8"), ("frag", "<i8"), ("reserved", "<u8")])
PAIR_LINK_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("n_pairs", "<u8"), ("sum_dist", "<u8"), ("min_dist", "<u4"), ("max_dist", "<u4")])
PAIR_CLASSES = {0: "NONE", 1: "SINGLE", 2: "SAME", 3: "INVERTED", 4: "LINK", 5: "FAR"}


class ScaffoldParams(C.Structure):
    """kmx_scaffold_params of include/kmx.h: 32 bytes"""
    _fields_ = [("min_pairs", C.c_uint64), ("ratio", C.c_uint32), ("inner", C.c_uint32), ("min_n", C.c_uint32), ("max_n", C.c_uint32), ("reserved", C.c_uint64)]


class ScaffoldStats(C.Structure):
    """kmx_scaffold_stats of include/kmx.h: 80 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_entries", "n_links", "n_ignored", "n_below_min", "n_below_ratio", "n_kept", "n_chain", "n_scaffolds", "n_circular", "n_multi")]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_scaffold, kmx_scaffold_step and kmx_scaffold_place as NumPy structured dtypes (what KModel.unitig_scaffold_flat returns): 64,
# 16 and 16 bytes.  n_steps carries SCAFFOLD_CIRCULAR above the count: scaffold_n_steps and scaffold_circular take it apart.
SCAFFOLD_DTYPE = np.dtype([("n_bases", "<u8"), ("n_kmers", "<u8"), ("sum_count", "<u8"), ("min_count", "<u4"), ("max_count", "<u4"), ("first_step", "<u4"), ("n_steps", "<u4"),
                           ("n_gap_bases", "<u8"), ("min_pairs", "<u8"), ("sum_pairs", "<u8")])
SCAFFOLD_STEP_DTYPE = np.dtype([("o", "<u4"), ("n_gap", "<u4"), ("est", "<i8")])
SCAFFOLD_PLACE_DTYPE = np.dtype([("os", "<u4"), ("step", "<u4"), ("off", "<u8")])
SCAFFOLD_CIRCULAR = 0x80000000


def scaffold_n_steps(srec) -> np.ndarray:
    return np.asarray(srec["n_steps"]) & np.uint32(SCAFFOLD_CIRCULAR - 1)


def scaffold_circular(srec) -> np.ndarray:
    return (np.asarray(srec["n_steps"]) >> np.uint32(31)).astype(np.uint8)


class PairPathParams(C.Structure):
    """kmx_pair_path_params of include/kmx.h: 32 bytes"""
    _fields_ = [("min_pairs", C.c_uint64), ("inner", C.c_uint32), ("tol", C.c_uint32), ("max_steps", C.c_uint32), ("max_visits", C.c_uint32), ("reserved", C.c_uint64)]


class PairPathStats(C.Structure):
    """kmx_pair_path_stats of include/kmx.h: 80 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_entries", "n_ignored", "n_below_min", "n_no_path", "n_adjacent", "n_path", "n_ambiguous", "n_complex", "n_added", "n_missing")]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_pair_path as a NumPy structured dtype (what KModel.unitig_pair_paths_flat returns): 32 bytes
PAIR_PATH_DTYPE = np.dtype([("verdict", "<u4"), ("n_steps", "<u4"), ("first_step", "<u8"), ("windows", "<u8"), ("n_hits", "<u4"), ("n_visited", "<u4")])
PAIR_PATH_VERDICTS = {0: "IGNORED", 1: "BELOW_MIN", 2: "NO_PATH", 3: "ADJACENT", 4: "PATH", 5: "AMBIGUOUS", 6: "COMPLEX"}
PAIR_PATH_MAX_STEPS = 16


class FillParams(C.Structure):
    """kmx_fill_params of include/kmx.h: 8 bytes"""
    _fields_ = [("kinds", C.c_uint32), ("reserved", C.c_uint32)]


class FillStats(C.Structure):
    """kmx_fill_stats of include/kmx.h: 80 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_head", "n_path", "n_adjacent", "n_n", "n_no_entry", "n_mirror", "n_removed", "n_filled")] + [("reserved", C.c_uint64 * 2)]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_[:8]}


# kmx_scaffold_fill and kmx_fill_step as NumPy structured dtypes (what KModel.unitig_scaffold_fill_flat returns): 64 and 32 bytes
SCAFFOLD_FILL_DTYPE = np.dtype([(f, "<u8") for f in ("n_bases", "n_gap_bases", "n_fill_bases", "n_path_links", "n_adjacent_links", "n_n_links", "n_pieces", "first_piece")])
FILL_STEP_DTYPE = np.dtype([("o", "<u4"), ("kind", "<u4"), ("entry", "<u4"), ("n_pieces", "<u4"), ("off", "<u8"), ("n_front", "<u8")])
FILL_KINDS = {0: "HEAD", 1: "N", 2: "ADJACENT", 3: "PATH"}
FILL_NO_ENTRY = 0xFFFFFFFF


class PairReduceParams(C.Structure):
    """kmx_pair_reduce_params of include/kmx.h: 24 bytes"""
    _fields_ = [("min_pairs", C.c_uint64), ("inner", C.c_uint32), ("tol", C.c_uint32), ("max_row", C.c_uint32), ("reserved", C.c_uint32)]


class PairReduceStats(C.Structure):
    """kmx_pair_reduce_stats of include/kmx.h: 80 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_entries", "n_ignored", "n_below_min", "n_kept", "n_transitive", "n_complex", "n_out", "n_rows", "n_examined", "reserved")]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_pair_reduce as a NumPy structured dtype (what KModel.unitig_pair_reduce_flat returns): 32 bytes
PAIR_REDUCE_DTYPE = np.dtype([("verdict", "<u4"), ("via", "<u4"), ("n_via", "<u4"), ("side", "<u4"), ("g", "<i8"), ("delta", "<i8")])
PAIR_REDUCE_VERDICTS = {0: "IGNORED", 1: "BELOW_MIN", 2: "KEPT", 3: "TRANSITIVE", 4: "COMPLEX"}
PAIR_REDUCE_NO_VIA = 0xFFFFFFFF


class PairLiftParams(C.Structure):
    """kmx_pair_lift_params of include/kmx.h: 8 bytes"""
    _fields_ = [("max_dist", C.c_uint32), ("reserved", C.c_uint32)]


class PairLiftStats(C.Structure):
    """kmx_pair_lift_stats of include/kmx.h: 128 bytes"""
    _fields_ = [(f, C.c_uint64) for f in ("n_entries", "n_ignored", "n_same", "n_inverted", "n_link", "n_far", "n_same_back", "n_out", "pairs_ignored", "pairs_same", "pairs_inverted",
                                          "pairs_link", "pairs_far", "pairs_same_back")] + [("sum_same_d", C.c_int64), ("reserved", C.c_uint64)]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


# kmx_pair_lift as a NumPy structured dtype (what KModel.unitig_pair_lift_flat returns): 32 bytes
PAIR_LIFT_DTYPE = np.dtype([("cls", "<u4"), ("out", "<u4"), ("A", "<u4"), ("B", "<u4"), ("shift", "<i8"), ("flipped", "<u4"), ("reserved", "<u4")])
PAIR_LIFT_CLASSES = {0: "IGNORED", 1: "SAME", 2: "INVERTED", 3: "LINK", 4: "FAR"}
PAIR_LIFT_NO_OUT = 0xFFFFFFFF
PAIR_LIFT_FOLDS = {"wave": 0, "plain": 1}


class RingList(C.Structure):
    """kmx_ring_list of include/kmx.h"""
    _fields_ = [("list", C.c_int32), ("n_host", C.c_int32), ("src_kmers", C.c_void_p), ("src_counts", C.c_void_p),
                ("src_msg", C.c_void_p), ("dst_msg", C.c_void_p)]

_lib = None


def lib_path() -> str:
    return _build.LIB


def load_library():
    """dlopen libkmx.so (building it first if hipcc is available and the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    # a specially built variant (tools/stress_small_tables.py): a test hook like the library's own, honoured only with KMX_TEST_HOOKS=1
    path = os.environ.get("KMX_LIBRARY") if os.environ.get("KMX_TEST_HOOKS") == "1" else None
    if os.environ.get("KMX_LIBRARY") and path is None:
        # results must not be taken for the variant's: refuse instead of silently running the stock library
        raise KmxError(-2, "KMX_LIBRARY is set but KMX_TEST_HOOKS=1 is not: the variant library would be ignored")
    if path:
        if not os.path.exists(path):
            raise KmxError(-2, f"KMX_LIBRARY={path} does not exist")
    else:
        path = _build.LIB
    if path == _build.LIB and (not os.path.exists(path) or _build.stale()):
        try:
            _build.build_lib()
        except Exception as e:  # noqa: BLE001
            # never run against a library older than the sources: the numbers would describe code that is not in the tree
            what = "is missing" if not os.path.exists(path) else "is older than its sources"
            raise KmxError(-2, f"libkmx.so {what} and could not be built ({e}); there is no CPU fallback")
    # A process that also uses PyTorch-ROCm must end up with ONE HIP runtime: torch bundles its own libamdhip64
    # (same SONAME as /opt/rocm's).  Importing torch first makes libkmx.so bind to the copy torch already loaded;
    # the other order leaves torch unable to see the GPU ("No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.kmx_last_error.restype = C.c_char_p
    L.kmx_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.kmx_destroy.argtypes = [vp]
    L.kmx_set_stream.argtypes = [vp, vp]
    L.kmx_build_from_kmc.argtypes = [vp, C.c_char_p]
    L.kmx_begin.argtypes = [vp, i32, C.POINTER(u64), u64]
    L.kmx_insert_batch.argtypes = [vp, vp, vp, u64]
    L.kmx_insert_batch_dev.argtypes = [vp, vp, vp, u64]
    L.kmx_finish.argtypes = [vp]
    L.kmx_build_dev.argtypes = [vp, i32, vp, vp, u64]
    L.kmx_build_host.argtypes = [vp, i32, vp, vp, u64]
    L.kmx_query_packed.argtypes = [vp, vp, u64, vp]
    L.kmx_query_packed_dev.argtypes = [vp, vp, u64, vp]
    L.kmx_query_ascii.argtypes = [vp, C.c_char_p, i32, i32, u64, vp]
    L.kmx_query_strings.argtypes = [vp, C.POINTER(C.c_char_p), i32, u64, vp]
    L.kmx_save.argtypes = [vp, C.c_char_p]
    L.kmx_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.kmx_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.kmx_download.argtypes = [vp, i32, i32, vp, u64, C.POINTER(u64)]
    L.kmx_debug_hash.argtypes = [i32, vp, u64, vp, i32, i32, vp]
    L.kmx_debug_min_kmer.argtypes = [i32, vp, u64, vp]
    L.kmx_occubin.argtypes = [i32, i32, vp, vp]
    L.kmx_debug_mod.argtypes = [vp, u64, u64, vp]
    L.kmx_microbench.argtypes = [i32, u64, u64, i32, C.POINTER(C.c_double)]
    L.kmx_last_build_seconds.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.kmx_kmc_info.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(u64)]
    L.kmx_kmc_read.argtypes = [C.c_char_p, vp, vp, u64, C.POINTER(u64)]
    L.kmx_count_classes_dev.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.kmx_shard_begin.argtypes = [vp, i32, C.POINTER(u64), u64, i32, i32]
    L.kmx_shard_classify_dev.argtypes = [vp, vp, vp, u64, vp, vp, C.POINTER(u64)]
    L.kmx_ring_msg_bytes.restype = u64
    L.kmx_ring_msg_bytes.argtypes = [i32]
    L.kmx_ring_round_dev.argtypes = [vp, i32, C.POINTER(RingList), i32]
    L.kmx_ring_stale_dup_dev.argtypes = [vp, i32]
    L.kmx_shard_local.argtypes = [vp, C.POINTER(Stats), C.POINTER(vp), C.POINTER(vp)]
    L.kmx_shard_complete.argtypes = [vp, vp, vp, u64, C.POINTER(Stats)]
    L.kmx_dev_view.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(u64)]
    _sig(L, "kmx_create_on", [i32, i32, i32, i32, i32, C.POINTER(vp)])
    _sig(L, "kmx_build_from_kmc_multi", [C.POINTER(vp), i32, C.c_char_p])
    _sig(L, "kmx_build_from_kmc_multi_ex", [C.POINTER(vp), i32, C.c_char_p, i32])
    _sig(L, "kmx_range_begin", [vp, i32, C.POINTER(u64), u64, i32, i32])
    _sig(L, "kmx_range_buffers", [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_range_emit_dev", [vp, i32, C.POINTER(RingList), i32, C.POINTER(u64)])
    _sig(L, "kmx_range_verdict_dev", [vp, i32, vp, C.POINTER(u64), C.POINTER(u64), i32, vp])
    _sig(L, "kmx_range_resolve_dev", [vp, i32, vp])
    _sig(L, "kmx_range_commit_dev", [vp, vp, u64])
    _sig(L, "kmx_range_flush_dev", [vp, C.POINTER(u64)])
    _sig(L, "kmx_range_inband", [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_range_verdict_inband_dev", [vp, i32, vp, i32, vp])
    _sig(L, "kmx_range_commit_inband_dev", [vp, vp, i32])
    L.kmx_or_words_dev.argtypes = [vp, vp, vp, u64]
    _sig(L, "kmx_debug_pack_strings", [vp, vp, i32, i32, u64, vp, C.POINTER(i32)])
    _sig(L, "kmx_kernel_classes", [])
    _sig(L, "kmx_abi_version", [])
    _sig(L, "kmx_get_stats_n", [vp, vp, u64])
    _sig(L, "kmx_query_seqs", [vp, vp, vp, u64, vp])
    _sig(L, "kmx_query_seqs_dev", [vp, vp, vp, u64, u64, vp])
    _sig(L, "kmx_summarise_seqs", [vp, vp, vp, u64, vp, i32, vp])
    _sig(L, "kmx_summarise_seqs_dev", [vp, vp, vp, u64, u64, vp, i32, vp])
    _sig(L, "kmx_correct_seqs", [vp, vp, vp, u64, i32, i32, vp, vp])
    _sig(L, "kmx_correct_seqs_dev", [vp, vp, vp, u64, u64, i32, i32, vp, vp])
    _sig(L, "kmx_edit_seqs", [vp, vp, vp, u64, i32, i32, i32, vp, u64, vp, vp])
    _sig(L, "kmx_edit_seqs_dev", [vp, vp, vp, u64, u64, i32, i32, i32, vp, u64, vp, vp])
    _sig(L, "kmx_apply_edits", [vp, vp, u64, vp, u64, vp, u64, vp])
    _sig(L, "kmx_apply_edits_dev", [vp, vp, vp, u64, u64, vp, u64, vp, u64, vp])
    _sig(L, "kmx_polish_seqs", [vp, vp, vp, u64, i32, i32, i32, i32, vp, u64, vp, vp, vp])
    _sig(L, "kmx_polish_seqs_dev", [vp, vp, vp, u64, u64, i32, i32, i32, i32, vp, u64, vp, vp, vp])
    _sig(L, "kmx_extend_seqs", [vp, vp, vp, u64, i32, i32, i32, vp, vp])
    _sig(L, "kmx_extend_seqs_dev", [vp, vp, vp, u64, u64, i32, i32, i32, vp, vp])
    _sig(L, "kmx_count_begin", [vp, i32])
    _sig(L, "kmx_count_seqs", [vp, vp, vp, u64])
    _sig(L, "kmx_count_seqs_dev", [vp, vp, vp, u64, u64])
    _sig(L, "kmx_count_finish", [vp, C.POINTER(u64)])
    _sig(L, "kmx_count_listing", [vp, vp, vp, u64, C.POINTER(u64)])
    _sig(L, "kmx_build_from_reads", [vp, i32, C.c_char_p])
    u32 = C.c_uint32
    _sig(L, "kmx_unitigs", [vp, i32, vp, vp, u64, u32, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_unitigs_dev", [vp, i32, vp, vp, u64, u32, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_count_unitigs", [vp, u32, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_count_unitigs_dev", [vp, u32, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_unitigs_last_phases", [vp, C.POINTER(C.c_double), C.POINTER(u64)])
    _sig(L, "kmx_unitig_graph", [vp, i32, vp, vp, u64, u32, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_unitig_graph_dev", [vp, i32, vp, vp, u64, u32, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_count_unitig_graph", [vp, u32, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_count_unitig_graph_dev", [vp, u32, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)])
    _sig(L, "kmx_unitig_graph_last_phases", [vp, C.POINTER(C.c_double), C.POINTER(u64)])
    _sig(L, "kmx_unitig_graph_clean", [vp, i32, vp, vp, u64, u32, vp, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, vp])
    _sig(L, "kmx_unitig_graph_clean_dev", [vp, i32, vp, vp, u64, u32, vp, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, vp])
    _sig(L, "kmx_count_unitig_graph_clean", [vp, u32, vp, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, vp])
    _sig(L, "kmx_count_unitig_graph_clean_dev", [vp, u32, vp, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, vp])
    _sig(L, "kmx_unitig_clean_last_phases", [vp, C.POINTER(C.c_double), C.POINTER(u64)])
    _sig(L, "kmx_unitig_map_begin", [vp, i32, vp, u64, vp, vp, u64])
    _sig(L, "kmx_unitig_map_begin_dev", [vp, i32, vp, u64, vp, vp, u64, u64])
    _sig(L, "kmx_count_unitig_map_begin", [vp, vp, vp, u64])
    _sig(L, "kmx_count_unitig_map_begin_dev", [vp, vp, vp, u64, u64])
    _sig(L, "kmx_unitig_map_seqs", [vp, vp, vp, u64, vp, u64, C.POINTER(u64), vp, vp, vp])
    _sig(L, "kmx_unitig_map_seqs_dev", [vp, vp, vp, u64, u64, vp, u64, C.POINTER(u64), vp, vp, vp])
    _sig(L, "kmx_unitig_map_end", [vp])
    _sig(L, "kmx_unitig_walk_segs", [vp, vp, u64, vp, u64, vp, vp, u64, C.POINTER(WalkParams), vp, u64, vp, vp, u64, vp, C.POINTER(WalkStats)])
    _sig(L, "kmx_unitig_walk_segs_dev", [vp, vp, u64, vp, u64, vp, vp, u64, C.POINTER(WalkParams), vp, u64, vp, vp, u64, vp, C.POINTER(WalkStats)])
    p64 = C.POINTER(C.c_uint64)
    _sig(L, "kmx_unitig_contigs", [vp, C.c_int, vp, vp, u64, vp, vp, vp, u64, vp, C.POINTER(ContigParams), vp, vp, vp, vp, vp, vp, vp, vp, p64, p64, p64, C.POINTER(ContigStats)])
    _sig(L, "kmx_unitig_contigs_dev", [vp, C.c_int, vp, vp, u64, u64, vp, vp, vp, u64, vp, C.POINTER(ContigParams), vp, vp, vp, vp, vp, vp, vp, vp, p64, p64, p64, C.POINTER(ContigStats)])
    _sig(L, "kmx_unitig_contigs_last_phases", [vp, C.POINTER(C.c_double), p64])
    _sig(L, "kmx_unitig_walk_through", [vp, vp, u64, vp, u64, vp, vp, u64, u64, vp, C.POINTER(ThroughStats)])
    _sig(L, "kmx_unitig_walk_through_dev", [vp, vp, u64, vp, u64, vp, vp, u64, u64, vp, C.POINTER(ThroughStats)])
    _sig(L, "kmx_unitig_pair_walks", [vp, vp, u64, vp, u64, vp, u64, vp, vp, u64, C.POINTER(PairParams), vp, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(PairStats)])
    _sig(L, "kmx_unitig_pair_walks_dev", [vp, vp, u64, vp, u64, vp, u64, vp, vp, u64, C.POINTER(PairParams), vp, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(PairStats)])
    _sig(L, "kmx_unitig_scaffold", [vp, C.c_int, vp, vp, u64, vp, vp, u64, C.POINTER(ScaffoldParams), vp, u64, vp, vp, vp, vp, p64, p64, C.POINTER(ScaffoldStats)])
    _sig(L, "kmx_unitig_scaffold_dev", [vp, C.c_int, vp, vp, u64, u64, vp, vp, u64, C.POINTER(ScaffoldParams), vp, u64, vp, vp, vp, vp, p64, p64, C.POINTER(ScaffoldStats)])
    _sig(L, "kmx_unitig_scaffold_last_phases", [vp, C.POINTER(C.c_double), p64])
    _sig(L, "kmx_unitig_pair_paths", [vp, C.c_int, vp, u64, vp, vp, u64, vp, u64, C.POINTER(PairPathParams), vp, vp, u64, p64, vp, vp, C.POINTER(PairPathStats)])
    _sig(L, "kmx_unitig_pair_paths_dev", [vp, C.c_int, vp, u64, vp, vp, u64, vp, u64, C.POINTER(PairPathParams), vp, vp, u64, p64, vp, vp, C.POINTER(PairPathStats)])
    _sig(L, "kmx_unitig_pair_paths_last_phases", [vp, C.POINTER(C.c_double)])
    _sig(L, "kmx_unitig_pair_reduce", [vp, C.c_int, vp, u64, vp, u64, C.POINTER(PairReduceParams), vp, vp, vp, u64, p64, C.POINTER(PairReduceStats)])
    _sig(L, "kmx_unitig_pair_reduce_dev", [vp, C.c_int, vp, u64, u64, vp, u64, C.POINTER(PairReduceParams), vp, vp, vp, u64, p64, C.POINTER(PairReduceStats)])
    _sig(L, "kmx_unitig_pair_reduce_last_phases", [vp, C.POINTER(C.c_double)])
    _sig(L, "kmx_unitig_pair_lift", [vp, C.c_int, vp, u64, vp, vp, u64, vp, u64, C.POINTER(PairLiftParams), vp, vp, u64, p64, C.POINTER(PairLiftStats)])
    _sig(L, "kmx_unitig_pair_lift_dev", [vp, C.c_int, vp, u64, u64, vp, vp, u64, vp, u64, C.POINTER(PairLiftParams), vp, vp, u64, p64, C.POINTER(PairLiftStats)])
    _sig(L, "kmx_unitig_pair_lift_fold_variant", [vp, C.c_int])
    _sig(L, "kmx_unitig_pair_lift_last_phases", [vp, C.POINTER(C.c_double)])
    _sig(L, "kmx_unitig_scaffold_fill", [vp, C.c_int, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(FillParams), vp, u64, vp, vp, vp, vp, u64, p64, p64, C.POINTER(FillStats)])
    _sig(L, "kmx_unitig_scaffold_fill_dev", [vp, C.c_int, vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, vp, u64, C.POINTER(FillParams), vp, u64, vp, vp, vp, vp, u64, p64, p64, C.POINTER(FillStats)])
    _sig(L, "kmx_unitig_scaffold_fill_last_phases", [vp, C.POINTER(C.c_double)])
    _sig(L, "kmx_unitig_resolve", [vp, C.c_int, vp, vp, u64, vp, vp, vp, u64, vp, vp, C.POINTER(ResolveParams), vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, p64, p64, C.POINTER(ResolveStats)])
    _sig(L, "kmx_unitig_resolve_dev", [vp, C.c_int, vp, vp, u64, u64, vp, vp, vp, u64, vp, vp, C.POINTER(ResolveParams), vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, p64, p64, C.POINTER(ResolveStats)])
    _sig(L, "kmx_unitig_resolve_last_phases", [vp, C.POINTER(C.c_double)])
    L.kmx_set_profile.argtypes = [vp, i32]
    L.kmx_get_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64), i32]
    _lib = L
    return L


def _sig(L, name, argtypes):
    """argtypes of an entry point a variant library (KMX_LIBRARY: an earlier round's build, for same-box comparisons) may lack"""
    f = getattr(L, name, None)
    if f is not None:
        f.argtypes = argtypes


def _chk(rc: int):
    if rc != 0:
        raise KmxError(rc, load_library().kmx_last_error().decode(errors="replace"))


def device_count() -> int:
    return load_library().kmx_device_count()


def occubin(cs: int, nh: int):
    b = np.zeros(cs + 1, dtype=np.uint32)
    m = np.zeros(1 << nh, dtype=np.uint32)
    _chk(load_library().kmx_occubin(cs, nh, b.ctypes.data, m.ctypes.data))
    return b, m


def debug_hash(k: int, kmers: np.ndarray, seeds, whole: bool = True) -> np.ndarray:
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    n = kmers.size // ((k + 31) // 32)
    out = np.zeros((n, len(seeds)), dtype=np.uint64)
    _chk(load_library().kmx_debug_hash(k, kmers.ctypes.data, n, seeds.ctypes.data, len(seeds), int(whole), out.ctypes.data))
    return out


def debug_min_kmer(k: int, kmers: np.ndarray) -> np.ndarray:
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    n = kmers.size // ((k + 31) // 32)
    out = np.zeros_like(kmers)
    _chk(load_library().kmx_debug_min_kmer(k, kmers.ctypes.data, n, out.ctypes.data))
    return out


def debug_mod(h: np.ndarray, d: int) -> np.ndarray:
    h = np.ascontiguousarray(h, dtype=np.uint64)
    out = np.zeros_like(h)
    _chk(load_library().kmx_debug_mod(h.ctypes.data, len(h), d, out.ctypes.data))
    return out


def pack_strings(flat: np.ndarray, separate: bool = False):
    """Host half of the vector<string> front door on its own (strpack.cpp): uint8[n, stride >= len] rows -> (packed u64[n * W], clean).
    `separate`: hand the rows over as n pointers (what a vector<string> holds) instead of one buffer."""
    L = load_library()
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    n, stride = flat.shape
    return _pack(L, flat, n, stride, stride, separate)


def _pack(L, flat, n, ln, stride, separate):
    out = np.zeros(n * ((ln + 31) // 32), dtype=np.uint64)
    clean = C.c_int32(-1)
    if separate:
        ptrs = (flat.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(stride)).astype(np.uint64)
        _chk(L.kmx_debug_pack_strings(ptrs.ctypes.data, None, ln, ln, n, out.ctypes.data, C.byref(clean)))
    else:
        _chk(L.kmx_debug_pack_strings(None, flat.ctypes.data, ln, stride, n, out.ctypes.data, C.byref(clean)))
    return out, bool(clean.value)


def pack_strings_len(flat: np.ndarray, ln: int, separate: bool = False):
    """as pack_strings, for rows that hold `ln` characters followed by padding"""
    L = load_library()
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    return _pack(L, flat, flat.shape[0], ln, flat.shape[1], separate)


def kmc_list(db_prefix: str):
    """(k, total_kmers, kmers, counts) of a KMC database in listing order; host only."""
    L = load_library()
    k, total = C.c_int(0), C.c_uint64(0)
    _chk(L.kmx_kmc_info(db_prefix.encode(), C.byref(k), C.byref(total)))
    W = (k.value + 31) // 32
    km = np.zeros(max(total.value, 1) * W, dtype=np.uint64)
    cnt = np.zeros(max(total.value, 1), dtype=np.uint32)
    n = C.c_uint64(0)
    _chk(L.kmx_kmc_read(db_prefix.encode(), km.ctypes.data, cnt.ctypes.data, total.value, C.byref(n)))
    km = km[: n.value * W]
    return k.value, total.value, (km if W == 1 else km.reshape(-1, W)), cnt[: n.value]


def microbench(mode: int, nbytes: int, touches: int, iters: int = 3) -> float:
    s = C.c_double(0)
    _chk(load_library().kmx_microbench(mode, nbytes, touches, iters, C.byref(s)))
    return s.value


def _flat_seqs(buf, offsets):
    """(bases, offsets) as the C calls take them: flat contiguous uint8 and uint64 [n_seqs + 1], the offsets ending inside the bases"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if offsets.size == 0:
        raise KmxError(-1, "offsets must hold n_seqs + 1 entries")
    if int(offsets[-1]) > buf.size:
        raise KmxError(-1, f"offsets end at {int(offsets[-1])}, past the {buf.size} bases given")
    return buf, offsets


def _join_seqs(seqs):
    """a str / bytes sequence (single) or a list of them -> (single, the bytes of each, their uint8 bases joined end to end, uint64 offsets)"""
    single = isinstance(seqs, (str, bytes))
    raw = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in ([seqs] if single else list(seqs))]
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    return single, raw, np.frombuffer(b"".join(raw), dtype=np.uint8), offsets


def _split_seqs(buf, offsets):
    """the bytes of every sequence of (bases, offsets)"""
    return [buf[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(offsets.size - 1)]


def apply_edits(buf: np.ndarray, offsets: np.ndarray, edits: np.ndarray):
    """kmx_apply_edits (host only, needs no GPU): an edit list applied to the bases it was found on -> (uint8 edited bases,
    uint64 offsets_out [n_seqs + 1])"""
    L = load_library()
    buf, offsets = _flat_seqs(buf, offsets)
    edits = np.ascontiguousarray(edits, dtype=np.uint64).reshape(-1)
    out = np.empty(int(offsets[-1]) + edits.size, dtype=np.uint8)
    off = np.zeros(offsets.size, dtype=np.uint64)
    _chk(L.kmx_apply_edits(buf.ctypes.data, offsets.ctypes.data, offsets.size - 1, edits.ctypes.data, edits.size, out.ctypes.data, out.size, off.ctypes.data))
    return out[:int(off[-1])].copy(), off


class KModel:
    """Handle on one model resident in HBM.  Mirrors reference class KModel (kmodel.hpp:39-672)."""

    DL = {"bf": 0, "bf_back": 1, "km_back": 2, "value": 3, "tag": 4, "claims": 5}

    def __init__(self, ci: int = 1, cs: int = 1023, num_hash: int = 7, num_bit: int = 5, _handle=None, device=None):
        """device: the HIP device of the handle (kmx_create_on); None = the calling thread's current device (kmx_create)"""
        self.L = load_library()
        if _handle is None:
            h = C.c_void_p()
            if device is None:
                _chk(self.L.kmx_create(ci, cs, num_hash, num_bit, C.byref(h)))
            else:
                _chk(self.L.kmx_create_on(int(device), ci, cs, num_hash, num_bit, C.byref(h)))
            _handle = h
        self.h = _handle

    # ---- build
    def init(self, db_file: str) -> None:                      # kmodel.hpp:57
        _chk(self.L.kmx_build_from_kmc(self.h, db_file.encode()))

    init_KModel = init                                         # README.md:76

    def build_packed(self, k: int, kmers: np.ndarray, counts: np.ndarray) -> None:
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        _chk(self.L.kmx_build_host(self.h, k, kmers.ctypes.data, counts.ctypes.data, len(counts)))

    def build_dev(self, k: int, d_kmers_ptr: int, d_counts_ptr: int, n: int) -> None:
        _chk(self.L.kmx_build_dev(self.h, k, d_kmers_ptr, d_counts_ptr, n))

    def begin(self, k: int, n_bf, n_total: int) -> None:
        arr = (C.c_uint64 * 3)(*[int(x) for x in list(n_bf) + [0, 0, 0]][:3])
        _chk(self.L.kmx_begin(self.h, k, arr, n_total))

    def insert_batch(self, kmers: np.ndarray, counts: np.ndarray) -> None:
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        _chk(self.L.kmx_insert_batch(self.h, kmers.ctypes.data, counts.ctypes.data, len(counts)))

    def insert_batch_dev(self, d_kmers_ptr: int, d_counts_ptr: int, n: int) -> None:
        _chk(self.L.kmx_insert_batch_dev(self.h, d_kmers_ptr, d_counts_ptr, n))

    def finish(self) -> None:
        _chk(self.L.kmx_finish(self.h))

    def set_stream(self, stream_ptr: int) -> None:
        _chk(self.L.kmx_set_stream(self.h, stream_ptr))

    # ---- one model, several GPUs: this rank's share (include/kmx.h, "ONE model built by several GPUs"; driven by dist.py)
    def count_classes_dev(self, d_counts_ptr: int, n: int):
        arr = (C.c_uint64 * 3)()
        _chk(self.L.kmx_count_classes_dev(self.h, d_counts_ptr, n, arr))
        return [int(x) for x in arr]

    def shard_begin(self, k: int, n_bf, n_total: int, rank: int, world: int) -> None:
        arr = (C.c_uint64 * 3)(*[int(x) for x in list(n_bf) + [0, 0, 0]][:3])
        _chk(self.L.kmx_shard_begin(self.h, k, arr, n_total, rank, world))

    def shard_classify_dev(self, d_kmers_ptr: int, d_counts_ptr: int, n: int, d_out_kmers_ptr: int, d_out_counts_ptr: int) -> int:
        n_out = C.c_uint64(0)
        _chk(self.L.kmx_shard_classify_dev(self.h, d_kmers_ptr, d_counts_ptr, n, d_out_kmers_ptr, d_out_counts_ptr, C.byref(n_out)))
        return int(n_out.value)

    def ring_msg_bytes(self, k: int) -> int:
        return int(self.L.kmx_ring_msg_bytes(k))

    def ring_round_dev(self, t: int, lists) -> None:
        """lists: (list, n_host, src_kmers_ptr, src_counts_ptr, src_msg_ptr, dst_msg_ptr) tuples, 0 for null pointers"""
        arr = (RingList * max(len(lists), 1))()
        for e, (i, n_host, sk, sc, sm, dm) in enumerate(lists):
            arr[e] = RingList(i, n_host, sk or None, sc or None, sm or None, dm or None)
        _chk(self.L.kmx_ring_round_dev(self.h, t, arr, len(lists)))

    def ring_stale_dup_dev(self, first_unused_row: int) -> None:
        _chk(self.L.kmx_ring_stale_dup_dev(self.h, first_unused_row))

    def shard_local(self):
        st, pk, pc = Stats(), C.c_void_p(), C.c_void_p()
        _chk(self.L.kmx_shard_local(self.h, C.byref(st), C.byref(pk), C.byref(pc)))
        return st, pk.value or 0, pc.value or 0

    def shard_complete(self, d_rest_kmers_ptr: int, d_rest_counts_ptr: int, n_rest: int, totals: Stats) -> None:
        _chk(self.L.kmx_shard_complete(self.h, d_rest_kmers_ptr or None, d_rest_counts_ptr or None, n_rest, C.byref(totals)))

    # ---- position-range partition (include/kmx.h, kmx_range_*)
    def range_begin(self, k: int, n_bf, n_total: int, rank: int, world: int) -> None:
        arr = (C.c_uint64 * 3)(*[int(x) for x in list(n_bf) + [0, 0, 0]][:3])
        _chk(self.L.kmx_range_begin(self.h, k, arr, n_total, rank, world))
        self._range_world = world

    def range_buffers(self):
        p, cap = C.c_void_p(), C.c_uint64()
        lo = (C.c_uint64 * (self._range_world + 1))()
        _chk(self.L.kmx_range_buffers(self.h, C.byref(p), C.byref(cap), lo))
        return p.value or 0, int(cap.value), [int(x) for x in lo]

    def range_emit_dev(self, t: int, lists):
        """-> (words per destination rank, commit words among them): the headers of the regions"""
        arr = (RingList * max(len(lists), 1))()
        for j, (i, n, pk, pc) in enumerate(lists):
            arr[j] = RingList(i, n, pk or None, pc or None, None, None)
        w = self._range_world
        counts = (C.c_uint64 * (2 * w))()
        _chk(self.L.kmx_range_emit_dev(self.h, t, arr, len(lists), counts))
        return [int(x) for x in counts[:w]], [int(x) for x in counts[w:]]

    def range_inband(self):
        """fixed-size messages: -> (device pointer of the regions, 64-bit words per region incl. its header, capx)"""
        p, rw, cx = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _chk(self.L.kmx_range_inband(self.h, C.byref(p), C.byref(rw), C.byref(cx)))
        return p.value or 0, int(rw.value), int(cx.value)

    def range_emit_nowait_dev(self, t: int, lists) -> None:
        arr = (RingList * max(len(lists), 1))()
        for j, (i, n, pk, pc) in enumerate(lists):
            arr[j] = RingList(i, n, pk or None, pc or None, None, None)
        _chk(self.L.kmx_range_emit_dev(self.h, t, arr, len(lists), None))

    def range_flush_nowait_dev(self) -> None:
        _chk(self.L.kmx_range_flush_dev(self.h, None))

    def range_verdict_inband_dev(self, t: int, d_recv_ptr: int, n_src: int, d_verdict_ptr: int) -> None:
        _chk(self.L.kmx_range_verdict_inband_dev(self.h, t, d_recv_ptr, n_src, d_verdict_ptr))

    def range_commit_inband_dev(self, d_recv_ptr: int, n_src: int) -> None:
        _chk(self.L.kmx_range_commit_inband_dev(self.h, d_recv_ptr, n_src))

    def range_verdict_dev(self, t: int, d_words_ptr: int, totals, commits, d_verdict_ptr: int) -> None:
        n = len(totals)
        _chk(self.L.kmx_range_verdict_dev(self.h, t, d_words_ptr or None, (C.c_uint64 * n)(*totals), (C.c_uint64 * n)(*commits), n, d_verdict_ptr or None))

    def range_resolve_dev(self, t: int, d_verdict_ptr: int) -> None:
        _chk(self.L.kmx_range_resolve_dev(self.h, t, d_verdict_ptr or None))

    def range_commit_dev(self, d_commits_ptr: int, n: int) -> None:
        _chk(self.L.kmx_range_commit_dev(self.h, d_commits_ptr, n))

    def range_flush_dev(self):
        w = self._range_world
        counts = (C.c_uint64 * (2 * w))()
        _chk(self.L.kmx_range_flush_dev(self.h, counts))
        return [int(x) for x in counts[:w]]

    def dev_view(self, which: str, index: int = 0):
        """(device pointer, bytes) of a filter ("bf", "bf_back", "km_back") or of the cells of coupled array `index` ("cells")"""
        sel = {"bf": 0, "bf_back": 1, "km_back": 2, "cells": 3}[which]
        p, n = C.c_void_p(), C.c_uint64(0)
        _chk(self.L.kmx_dev_view(self.h, sel, index, C.byref(p), C.byref(n)))
        return p.value or 0, int(n.value)

    def or_words_dev(self, d_dst_ptr: int, d_src_ptr: int, n_words: int) -> None:
        _chk(self.L.kmx_or_words_dev(self.h, d_dst_ptr, d_src_ptr, n_words))

    # ---- query
    def kmer_to_occ(self, kmers, t_num: int = 4):             # kmodel.hpp:90,100 (t_num kept for signature parity)
        single = isinstance(kmers, str)
        strs = [kmers] if single else list(kmers)
        if not strs:
            return []
        out = np.zeros(len(strs), dtype=np.int32)
        by_len = {}
        for i, s in enumerate(strs):                           # the reference answers every string on its own
            by_len.setdefault(len(s), []).append(i)
        for ln, idx in by_len.items():
            part = np.zeros(len(idx), dtype=np.int32)
            _chk(self.L.kmx_query_ascii(self.h, "".join(strs[i] for i in idx).encode("latin-1"), ln, ln, len(idx), part.ctypes.data))
            out[idx] = part
        return int(out[0]) if single else out.tolist()

    def kmer_to_occ_rows(self, rows: np.ndarray, ln: int, separate: bool = True) -> np.ndarray:
        """kmer_to_occ over uint8[n, stride >= ln] rows holding one string each -- as n separate strings (kmx_query_strings:
        what the reference's vector<string> is, kmodel.hpp:90-98) or as one buffer (kmx_query_ascii)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n, stride = rows.shape
        out = np.zeros(n, dtype=np.int32)
        if separate:
            ptrs = (rows.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(stride)).astype(np.uint64)
            _chk(self.L.kmx_query_strings(self.h, C.cast(ptrs.ctypes.data, C.POINTER(C.c_char_p)), ln, n, out.ctypes.data))
        else:
            _chk(self.L.kmx_query_ascii(self.h, C.cast(rows.ctypes.data, C.c_char_p), ln, stride, n, out.ctypes.data))
        return out

    def kmer_to_occ_packed(self, kmers: np.ndarray) -> np.ndarray:
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        k = self.stats().k
        if k == 0:
            raise KmxError(-4, "query before the model is built or loaded")
        n = kmers.size // ((k + 31) // 32)
        out = np.zeros(n, dtype=np.int32)
        _chk(self.L.kmx_query_packed(self.h, kmers.ctypes.data, n, out.ctypes.data))
        return out

    def kmer_to_occ_dev(self, d_kmers_ptr: int, n: int, d_out_ptr: int) -> None:
        _chk(self.L.kmx_query_packed_dev(self.h, d_kmers_ptr, n, d_out_ptr))

    def seq_to_occ_flat(self, buf: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """kmx_query_seqs: uint8 bases of sequences stored back to back, uint64 offsets[n_seqs + 1] -> int32[n_bases], aligned
        to the bases; -1 where no k-mer starts (the last k - 1 positions of each sequence)."""
        buf, offsets = _flat_seqs(buf, offsets)
        n_bases = int(offsets[-1])
        out = np.empty(n_bases, dtype=np.int32)
        _chk(self.L.kmx_query_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, offsets.size - 1, out.ctypes.data))
        return out

    def seq_to_occ(self, seqs):
        """kmer_to_occ of every overlapping k-mer of each sequence (str or bytes; one sequence or a list): one int32 array of
        max(len - k + 1, 0) answers per sequence (a list of them for a list)."""
        single, raw, flat, offsets = _join_seqs(seqs)
        k = self.stats().k
        if k == 0:
            raise KmxError(-4, "query before the model is built or loaded")
        occ = self.seq_to_occ_flat(flat, offsets) if raw else np.zeros(0, np.int32)
        res = [occ[int(offsets[i]):int(offsets[i]) + max(len(r) - k + 1, 0)] for i, r in enumerate(raw)]
        return res[0] if single else res

    def seq_to_occ_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int, d_out_ptr: int) -> None:
        """kmx_query_seqs_dev: device buffers, enqueued on the model's stream (no wait)"""
        _chk(self.L.kmx_query_seqs_dev(self.h, d_seq_ptr, d_offsets_ptr, n_seqs, n_bases, d_out_ptr))

    def seq_summary_flat(self, buf: np.ndarray, offsets: np.ndarray, thr=()) -> np.ndarray:
        """kmx_summarise_seqs: the answers of seq_to_occ_flat reduced per sequence on the device -> a structured array of
        n_seqs records (SEQ_SUMMARY_DTYPE: n_windows, sum, min, max, n_ge[3], first_below, last_below); thr: up to 3 int32
        thresholds, thr[0] also defines first_below / last_below."""
        buf, offsets = _flat_seqs(buf, offsets)
        t = np.ascontiguousarray(thr, dtype=np.int32).reshape(-1)
        out = np.zeros(offsets.size - 1, dtype=SEQ_SUMMARY_DTYPE)
        _chk(self.L.kmx_summarise_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, offsets.size - 1,
                                       t.ctypes.data if t.size else None, t.size, out.ctypes.data))
        return out

    def seq_summary(self, seqs, thr=()):
        """seq_summary_flat for a str / bytes sequence (-> one record) or a list of them (-> a structured array)"""
        single, _, buf, offsets = _join_seqs(seqs)
        res = self.seq_summary_flat(buf, offsets, thr)
        return res[0] if single else res

    def seq_summary_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int, thr, d_out_ptr: int) -> None:
        """kmx_summarise_seqs_dev: device buffers (d_out: n_seqs records of 64 bytes), enqueued on the model's stream (no
        wait); thr is a host sequence, read during the call"""
        t = np.ascontiguousarray(thr, dtype=np.int32).reshape(-1)
        _chk(self.L.kmx_summarise_seqs_dev(self.h, d_seq_ptr, d_offsets_ptr, n_seqs, n_bases, t.ctypes.data if t.size else None, t.size, d_out_ptr))

    def seq_correct_flat(self, buf: np.ndarray, offsets: np.ndarray, thr: int, min_support: int = 1):
        """kmx_correct_seqs: substitution errors corrected from the k-mer spectrum (the rule: include/kmx.h) -> (uint8 corrected
        bases [n_bases], SEQ_CORRECTION_DTYPE records [n_seqs]); a window is weak when its answer is below thr, a site is tried
        when at least min_support windows verify it."""
        buf, offsets = _flat_seqs(buf, offsets)
        n_bases = int(offsets[-1])
        out = np.empty(n_bases, dtype=np.uint8)
        rec = np.zeros(offsets.size - 1, dtype=SEQ_CORRECTION_DTYPE)
        _chk(self.L.kmx_correct_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, offsets.size - 1, int(thr), int(min_support),
                                     out.ctypes.data, rec.ctypes.data))
        return out, rec

    def seq_correct(self, seqs, thr: int, min_support: int = 1):
        """seq_correct_flat for a str / bytes sequence (-> (bytes, record)) or a list of them (-> (list of bytes, records))"""
        single, _, buf, offsets = _join_seqs(seqs)
        out, rec = self.seq_correct_flat(buf, offsets, thr, min_support)
        fixed = _split_seqs(out, offsets)
        return (fixed[0], rec[0]) if single else (fixed, rec)

    def seq_correct_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int, thr: int, min_support: int,
                        d_seq_out_ptr: int, d_rec_ptr: int = 0) -> None:
        """kmx_correct_seqs_dev: device buffers (d_seq_out: n_bases bytes, not overlapping d_seq; d_rec: n_seqs records of 64
        bytes, or 0), enqueued on the model's stream (no wait)"""
        _chk(self.L.kmx_correct_seqs_dev(self.h, d_seq_ptr, d_offsets_ptr, n_seqs, n_bases, int(thr), int(min_support),
                                         d_seq_out_ptr, d_rec_ptr or None))

    def seq_edit_flat(self, buf: np.ndarray, offsets: np.ndarray, thr: int, min_support: int = 1, ops: int = 7):
        """kmx_edit_seqs: substitutions and single-base insertions / deletions found from the k-mer spectrum (the rule:
        include/kmx.h) -> (uint64 edits, ascending: pos << 8 | op << 4 | code; SEQ_EDITS_DTYPE records [n_seqs]).  ops is a subset
        of EDIT_OPS_SUB | EDIT_OPS_DEL | EDIT_OPS_INS; apply_edits turns the list into the edited bases."""
        buf, offsets = _flat_seqs(buf, offsets)
        n_bases = int(offsets[-1])
        rec = np.zeros(offsets.size - 1, dtype=SEQ_EDITS_DTYPE)
        edits = np.empty(n_bases // 3 + 1, dtype=np.uint64)        # always enough (include/kmx.h)
        n = C.c_uint64(0)
        _chk(self.L.kmx_edit_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, offsets.size - 1, int(thr), int(min_support), int(ops),
                                  edits.ctypes.data, edits.size, C.addressof(n), rec.ctypes.data))
        return edits[:n.value].copy(), rec

    def seq_edit(self, seqs, thr: int, min_support: int = 1, ops: int = 7):
        """seq_edit_flat and apply_edits for a str / bytes sequence (-> (edited bytes, record, edits)) or a list of them
        (-> (list of edited bytes, records, edits)); the positions of the edits are those of the reads joined end to end"""
        single, _, buf, offsets = _join_seqs(seqs)
        edits, rec = self.seq_edit_flat(buf, offsets, thr, min_support, ops)
        fixed = _split_seqs(*apply_edits(buf, offsets, edits))
        return (fixed[0], rec[0], edits) if single else (fixed, rec, edits)

    def seq_edit_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int, thr: int, min_support: int, ops: int,
                     d_edits_ptr: int, capacity: int, d_rec_ptr: int = 0) -> int:
        """kmx_edit_seqs_dev: device buffers (d_edits: capacity uint64, d_rec: n_seqs records of 80 bytes, or 0) -> the number of
        edits found; KmxError -5 (KMX_E_RANGE) with .needed = that number when it exceeds capacity.  Waits once, for the count."""
        n = C.c_uint64(0)
        rc = self.L.kmx_edit_seqs_dev(self.h, d_seq_ptr, d_offsets_ptr, n_seqs, n_bases, int(thr), int(min_support), int(ops),
                                      d_edits_ptr or None, capacity, C.addressof(n), d_rec_ptr or None)
        try:
            _chk(rc)
        except KmxError as e:
            e.needed = n.value
            raise
        return n.value

    def apply_edits_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int, d_edits_ptr: int, n_edits: int,
                        d_seq_out_ptr: int, out_capacity: int, d_offsets_out_ptr: int) -> None:
        """kmx_apply_edits_dev: the (sorted) device list applied to the device bases it was found on; d_offsets_out: n_seqs + 1"""
        _chk(self.L.kmx_apply_edits_dev(self.h, d_seq_ptr, d_offsets_ptr, n_seqs, n_bases, d_edits_ptr or None, n_edits,
                                        d_seq_out_ptr or None, out_capacity, d_offsets_out_ptr))

    def seq_polish_flat(self, buf: np.ndarray, offsets: np.ndarray, thr: int, min_support: int = 1, ops: int = 7, max_passes: int = 8):
        """kmx_polish_seqs: kmx_edit_seqs' rule iterated per read until a pass finds nothing in it, or max_passes passes ran
        (the rule: include/kmx.h) -> (uint8 polished bases, uint64 offsets_out [n_seqs + 1], SEQ_POLISH_DTYPE records [n_seqs],
        passes run).  The output's length is not known beforehand: the call is repeated with the exact room when the first
        guess (the input's length and a sixteenth) is too small."""
        buf, offsets = _flat_seqs(buf, offsets)
        n_bases = int(offsets[-1])
        n_seqs = offsets.size - 1
        rec = np.zeros(n_seqs, dtype=SEQ_POLISH_DTYPE)
        off = np.zeros(n_seqs + 1, dtype=np.uint64)
        passes = C.c_uint64(0)
        cap = n_bases + n_bases // 16 + 64
        while True:
            out = np.empty(cap, dtype=np.uint8)
            rc = self.L.kmx_polish_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, n_seqs, int(thr), int(min_support), int(ops), int(max_passes),
                                        out.ctypes.data, out.size, off.ctypes.data, rec.ctypes.data, C.addressof(passes))
            if rc == -5 and int(off[-1]) > cap:                      # KMX_E_RANGE: offsets_out is complete
                cap = int(off[-1])
                continue
            _chk(rc)
            return out[:int(off[-1])].copy(), off, rec, int(passes.value)

    def seq_polish(self, seqs, thr: int, min_support: int = 1, ops: int = 7, max_passes: int = 8):
        """seq_polish_flat for a str / bytes sequence (-> (polished bytes, record)) or a list of them (-> (list of polished
        bytes, records))"""
        single, _, buf, offsets = _join_seqs(seqs)
        out, off, rec, _ = self.seq_polish_flat(buf, offsets, thr, min_support, ops, max_passes)
        fixed = _split_seqs(out, off)
        return (fixed[0], rec[0]) if single else (fixed, rec)

    def seq_polish_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int, thr: int, min_support: int, ops: int, max_passes: int,
                       d_seq_out_ptr: int, out_capacity: int, d_offsets_out_ptr: int, d_rec_ptr: int = 0) -> int:
        """kmx_polish_seqs_dev: device buffers (d_seq_out: out_capacity bytes, not overlapping d_seq; d_offsets_out: n_seqs + 1
        uint64; d_rec: n_seqs records of 96 bytes, or 0) -> the passes run.  KmxError -5 (KMX_E_RANGE) with .passes_run when
        the reads need more than out_capacity bytes: d_offsets_out[n_seqs] says how many.  Waits once per pass and once for the
        final length; returns with the gather enqueued."""
        passes = C.c_uint64(0)
        rc = self.L.kmx_polish_seqs_dev(self.h, d_seq_ptr or None, d_offsets_ptr or None, n_seqs, n_bases, int(thr), int(min_support), int(ops), int(max_passes),
                                        d_seq_out_ptr or None, out_capacity, d_offsets_out_ptr or None, d_rec_ptr or None, C.addressof(passes))
        try:
            _chk(rc)
        except KmxError as e:
            e.passes_run = int(passes.value)
            raise
        return int(passes.value)

    def seq_extend_flat(self, buf: np.ndarray, offsets: np.ndarray, thr: int, max_ext: int, depth: int = 2):
        """kmx_extend_seqs: every seed walked to the right along the unique path of k-mers answered >= thr (the rule:
        include/kmx.h) -> (uint8 appended bases [n_seqs, max_ext], 0 behind the n_ext of a row; SEQ_EXTENSION_DTYPE records
        [n_seqs]).  depth 0 ... 3 is the lookahead that breaks the ties the model's false positives cause."""
        buf, offsets = _flat_seqs(buf, offsets)
        n_seqs = offsets.size - 1
        rows = int(max_ext) if 1 <= int(max_ext) <= 65536 else 1               # (an invalid max_ext is the library's to refuse)
        ext = np.empty((n_seqs, rows), dtype=np.uint8)
        rec = np.zeros(n_seqs, dtype=SEQ_EXTENSION_DTYPE)
        _chk(self.L.kmx_extend_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, n_seqs, int(thr), int(max_ext), int(depth),
                                    ext.ctypes.data, rec.ctypes.data))
        return ext, rec

    def seq_extend(self, seqs, thr: int, max_ext: int, depth: int = 2, left: bool = False):
        """seq_extend_flat for a str / bytes seed (-> (bytes, record)) or a list of them (-> (list of bytes, records)): the
        appended bases of every seed.  left=True extends to the left instead: the walk of the seed's reverse complement,
        returned reverse-complemented again, so the result reads in the seed's direction and ends where the seed begins
        (for k > 32 the two strands of a k-mer need not get the same answer: include/kmx.h)."""
        single, raw, buf, offsets = _join_seqs(seqs)
        if left:
            _, raw, buf, offsets = _join_seqs([_REVCOMP[np.frombuffer(r, dtype=np.uint8)[::-1]].tobytes() for r in raw])
        ext, rec = self.seq_extend_flat(buf, offsets, thr, max_ext, depth)
        out = [ext[i, :int(rec["n_ext"][i])] for i in range(len(raw))]
        out = [(_REVCOMP[e[::-1]] if left else e).tobytes() for e in out]
        return (out[0], rec[0]) if single else (out, rec)

    def seq_extend_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int, thr: int, max_ext: int, depth: int,
                       d_ext_ptr: int, d_rec_ptr: int = 0) -> None:
        """kmx_extend_seqs_dev: device buffers (d_ext: n_seqs * max_ext bytes; d_rec: n_seqs records of 32 bytes, or 0),
        enqueued on the model's stream (no wait)"""
        _chk(self.L.kmx_extend_seqs_dev(self.h, d_seq_ptr, d_offsets_ptr, n_seqs, n_bases, int(thr), int(max_ext), int(depth),
                                        d_ext_ptr, d_rec_ptr or None))

    # ---- k-mer counting on the device (KMC's step, then init on its listing: main.cpp:137-146)
    def init_reads(self, path: str, k: int) -> None:
        """kmx_build_from_reads: count the k-mers of a FASTQ / FASTA file (plain or gzip) or "@list" and build the model"""
        _chk(self.L.kmx_build_from_reads(self.h, k, path.encode()))
        self._count_k = k

    def count_begin(self, k: int) -> None:
        _chk(self.L.kmx_count_begin(self.h, k))
        self._count_k = k

    def count_seqs(self, seqs, offsets=None) -> None:
        """kmx_count_seqs: a str / bytes sequence or a list of them, or (uint8 buf, uint64 offsets[n_seqs + 1])"""
        if offsets is None:
            _, _, seqs, offsets = _join_seqs(seqs)
        buf, offsets = _flat_seqs(seqs, offsets)
        _chk(self.L.kmx_count_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, offsets.size - 1))

    def count_seqs_dev(self, d_seq_ptr: int, d_offsets_ptr: int, n_seqs: int, n_bases: int) -> None:
        """kmx_count_seqs_dev: device buffers, enqueued on the model's stream"""
        _chk(self.L.kmx_count_seqs_dev(self.h, d_seq_ptr, d_offsets_ptr, n_seqs, n_bases))

    def count_finish(self) -> int:
        """filter + cap, then the build; returns the number of k-mers listed"""
        n = C.c_uint64()
        _chk(self.L.kmx_count_finish(self.h, C.byref(n)))
        return n.value

    def count_listing(self):
        """(kmers uint64[n, W] squeezed to [n] when W = 1, counts uint32[n]) the last count_finish built from"""
        n = C.c_uint64()
        _chk(self.L.kmx_count_listing(self.h, None, None, 0, C.byref(n)))
        W = ((getattr(self, "_count_k", 0) or self.stats().k) + 31) // 32
        kmers = np.zeros((n.value, W), dtype=np.uint64)
        counts = np.zeros(n.value, dtype=np.uint32)
        _chk(self.L.kmx_count_listing(self.h, kmers.ctypes.data, counts.ctypes.data, n.value, C.byref(n)))
        return (kmers[:, 0].copy() if W == 1 else kmers), counts

    # ---- unitigs: the compacted de Bruijn graph of a counted listing (the rule: include/kmx.h)
    def _unitig_call(self, call, dev: bool, links: bool = False, n=None):
        """the sizing call, then the call with exact room, of any of the twelve unitig entry points: call takes what follows thr
        (and params) in the C prototype.  -> (uint8 bases, uint64 offsets [n_unitigs + 1], UNITIG_DTYPE records [n_unitigs]); with
        links + (uint64 link_offsets [2 n_unitigs + 1], uint32 links [n_links]); with n, the listing's size (the cleaning calls),
        + (uint8 removed [n], stats dict).  dev: torch tensors on the model's device instead (int64 offsets and link_offsets, uint8
        records [n_unitigs, 40], int32 links: the bits of the uint32 targets).  Both calls rank the whole graph, so this costs the
        construction twice; tools/bench_unitigs.py times the bare C call."""
        clean = n is not None
        ctr = [C.c_uint64(0) for _ in range(3 if links else 2)]
        tail = [C.byref(c) for c in ctr] + ([None, None] if clean else [])
        _chk(call(None, 0, None, None, 0, *([None, None, 0] if links else []), *tail))
        nu, nb, nl = ctr[0].value, ctr[1].value, ctr[2].value if links else 0
        if dev:
            import torch
            where = torch.device("cuda", self.stats().device)
            u8, w64, w32, rec_shape = torch.uint8, torch.int64, torch.int32, ((nu, C.sizeof(Unitig)), torch.uint8)

            def new(shape, dtype):
                return torch.zeros(shape, dtype=dtype, device=where)

            def ptr(a):
                return a.data_ptr()
        else:
            u8, w64, w32, rec_shape, new = np.uint8, np.uint64, np.uint32, (nu, UNITIG_DTYPE), np.zeros

            def ptr(a):
                return a.ctypes.data
        buf, off, rec = new(max(nb, 1), u8), new(nu + 1, w64), new(*rec_shape)
        out, args = [buf[:nb], off, rec], [ptr(buf), nb, ptr(off), ptr(rec), nu]
        if links:
            loff, lk = new(2 * nu + 1, w64), new(max(nl, 1), w32)
            out += [loff, lk[:nl]]
            args += [ptr(loff), ptr(lk), nl]
        if clean:
            removed, st = new(max(n, 1), u8), CleanStats()
            tail[-2:] = [ptr(removed), C.addressof(st)]
        _chk(call(*args, *tail))
        if clean:
            out += [removed[:n], {f: int(getattr(st, f)) for f, _ in CleanStats._fields_}]
        return tuple(out)

    @staticmethod
    def _host_listing(kmers, counts, k):
        """a caller's listing as the host routes take it -> (contiguous uint64 words, uint32 counts, n)"""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if kmers.size != counts.size * ((int(k) + 31) // 32):
            raise KmxError(-1, f"{kmers.size} words for {counts.size} counts at k = {k}")
        return kmers, counts, counts.size

    @staticmethod
    def _dev_listing(d_kmers, d_counts, k):
        """a caller's listing as the _dev routes take it (int64 / uint64 words, int32 / uint32 counts) -> (contiguous words, counts, n)"""
        n = d_counts.numel()
        if d_kmers.numel() != n * ((int(k) + 31) // 32) or d_kmers.element_size() != 8 or d_counts.element_size() != 4:
            raise KmxError(-1, f"{d_kmers.numel()} words for {n} counts at k = {k}")
        return d_kmers.contiguous(), d_counts.contiguous(), n

    def unitigs(self, kmers: np.ndarray, counts: np.ndarray, k: int, thr: int = 1):
        """kmx_unitigs: the unitigs of a listing (packed canonical k-mers, strictly ascending; uint32 counts; odd k in [5, 63])
        whose nodes are the k-mers with count >= thr -> (buf, offsets, rec) in seq_to_occ_flat's layout.  Needs no built model."""
        kmers, counts, n = self._host_listing(kmers, counts, k)
        return self._unitig_call(lambda *a: self.L.kmx_unitigs(self.h, int(k), kmers.ctypes.data, counts.ctypes.data, n, int(thr), *a), False)

    def unitigs_dev(self, d_kmers, d_counts, k: int, thr: int = 1):
        """kmx_unitigs_dev on torch tensors of the model's device (int64 / uint64 words, int32 / uint32 counts) -> torch tensors"""
        d_kmers, d_counts, n = self._dev_listing(d_kmers, d_counts, k)
        return self._unitig_call(lambda *a: self.L.kmx_unitigs_dev(self.h, int(k), d_kmers.data_ptr(), d_counts.data_ptr(), n, int(thr), *a), True)

    def count_unitigs(self, thr: int = 1):
        """kmx_count_unitigs: the unitigs of the listing the last count_finish / init_reads kept, read where it lies"""
        return self._unitig_call(lambda *a: self.L.kmx_count_unitigs(self.h, int(thr), *a), False)

    def count_unitigs_dev(self, thr: int = 1):
        """kmx_count_unitigs_dev: the same, the output as torch tensors on the model's device"""
        return self._unitig_call(lambda *a: self.L.kmx_count_unitigs_dev(self.h, int(thr), *a), True)

    def _unitig_phases(self, call, names) -> dict:
        sec, rounds = (C.c_double * len(names))(), C.c_uint64(0)
        _chk(call(self.h, sec, C.byref(rounds)))
        return {**{n: sec[i] for i, n in enumerate(names)}, "rounds": int(rounds.value)}

    def unitigs_phases(self) -> dict:
        """kmx_unitigs_last_phases: seconds per phase of the last unitig call (measured under set_profile(1)) and its rounds"""
        return self._unitig_phases(self.L.kmx_unitigs_last_phases, UNITIG_PHASES)

    # ---- the unitig graph: the unitigs and the edges between them as CSR over the 2 U oriented unitigs (the rule: include/kmx.h)
    def unitig_graph(self, kmers: np.ndarray, counts: np.ndarray, k: int, thr: int = 1):
        """kmx_unitig_graph: unitigs() and the edges between the oriented unitigs o = 2 u + d (d = 1: the reverse complement) ->
        (buf, offsets, rec, link_offsets, links); the edges of o are links[link_offsets[o]:link_offsets[o + 1]]"""
        kmers, counts, n = self._host_listing(kmers, counts, k)
        return self._unitig_call(lambda *a: self.L.kmx_unitig_graph(self.h, int(k), kmers.ctypes.data, counts.ctypes.data, n, int(thr), *a), False, links=True)

    def unitig_graph_dev(self, d_kmers, d_counts, k: int, thr: int = 1):
        """kmx_unitig_graph_dev on torch tensors of the model's device (as unitigs_dev) -> torch tensors"""
        d_kmers, d_counts, n = self._dev_listing(d_kmers, d_counts, k)
        return self._unitig_call(lambda *a: self.L.kmx_unitig_graph_dev(self.h, int(k), d_kmers.data_ptr(), d_counts.data_ptr(), n, int(thr), *a), True, links=True)

    def count_unitig_graph(self, thr: int = 1):
        """kmx_count_unitig_graph: the unitig graph of the listing the last count_finish / init_reads kept"""
        return self._unitig_call(lambda *a: self.L.kmx_count_unitig_graph(self.h, int(thr), *a), False, links=True)

    def count_unitig_graph_dev(self, thr: int = 1):
        """kmx_count_unitig_graph_dev: the same, the output as torch tensors on the model's device"""
        return self._unitig_call(lambda *a: self.L.kmx_count_unitig_graph_dev(self.h, int(thr), *a), True, links=True)

    def unitig_graph_phases(self) -> dict:
        """kmx_unitig_graph_last_phases: unitigs_phases() plus "unitig_links", the seconds spent on the edges between unitigs"""
        return self._unitig_phases(self.L.kmx_unitig_graph_last_phases, UNITIG_GRAPH_PHASES)

    # ---- cleaning the unitig graph: tips, islands and bubbles removed round by round (the rule: include/kmx.h)
    @staticmethod
    def _clean_params(k, ops, max_tip, max_bubble, max_rounds):
        return CleanParams(int(ops), int(2 * k if max_tip is None else max_tip), int(2 * k if max_bubble is None else max_bubble), int(max_rounds))

    def unitig_graph_clean(self, kmers: np.ndarray, counts: np.ndarray, k: int, thr: int = 1, ops: int = 7, max_tip=None, max_bubble=None, max_rounds: int = 16):
        """kmx_unitig_graph_clean: unitig_graph() after tips (CLEAN_TIPS), islands (CLEAN_ISLANDS) and bubbles (CLEAN_BUBBLES) of at
        most max_tip / max_bubble k-mers (2 k when None) have been removed round by round -> (buf, offsets, rec, link_offsets,
        links, removed, stats): removed[i] is the round that removed listing entry i (0: it stays), stats a dict of kmx_clean_stats"""
        kmers, counts, n = self._host_listing(kmers, counts, k)
        P = self._clean_params(int(k), ops, max_tip, max_bubble, max_rounds)
        return self._unitig_call(lambda *a: self.L.kmx_unitig_graph_clean(self.h, int(k), kmers.ctypes.data, counts.ctypes.data, n, int(thr), C.addressof(P), *a), False, links=True, n=n)

    def unitig_graph_clean_dev(self, d_kmers, d_counts, k: int, thr: int = 1, ops: int = 7, max_tip=None, max_bubble=None, max_rounds: int = 16):
        """kmx_unitig_graph_clean_dev on torch tensors of the model's device (as unitigs_dev) -> torch tensors and the stats dict"""
        d_kmers, d_counts, n = self._dev_listing(d_kmers, d_counts, k)
        P = self._clean_params(int(k), ops, max_tip, max_bubble, max_rounds)
        return self._unitig_call(lambda *a: self.L.kmx_unitig_graph_clean_dev(self.h, int(k), d_kmers.data_ptr(), d_counts.data_ptr(), n, int(thr), C.addressof(P), *a), True, links=True, n=n)

    def _count_listing_size(self):
        n = C.c_uint64(0)
        _chk(self.L.kmx_count_listing(self.h, None, None, 0, C.byref(n)))
        return int(n.value)

    def count_unitig_graph_clean(self, thr: int = 1, ops: int = 7, max_tip=None, max_bubble=None, max_rounds: int = 16):
        """kmx_count_unitig_graph_clean: the cleaned unitig graph of the listing the last count_finish / init_reads kept"""
        P = self._clean_params(getattr(self, "_count_k", 0) or self.stats().k, ops, max_tip, max_bubble, max_rounds)
        return self._unitig_call(lambda *a: self.L.kmx_count_unitig_graph_clean(self.h, int(thr), C.addressof(P), *a), False, links=True, n=self._count_listing_size())

    def count_unitig_graph_clean_dev(self, thr: int = 1, ops: int = 7, max_tip=None, max_bubble=None, max_rounds: int = 16):
        """kmx_count_unitig_graph_clean_dev: the same, the output as torch tensors on the model's device"""
        P = self._clean_params(getattr(self, "_count_k", 0) or self.stats().k, ops, max_tip, max_bubble, max_rounds)
        return self._unitig_call(lambda *a: self.L.kmx_count_unitig_graph_clean_dev(self.h, int(thr), C.addressof(P), *a), True, links=True, n=self._count_listing_size())

    def unitig_clean_phases(self) -> dict:
        """kmx_unitig_clean_last_phases: unitig_graph_phases() summed over the rounds of the last cleaning call, plus "clean", the
        seconds spent on the decisions and the removal"""
        return self._unitig_phases(self.L.kmx_unitig_clean_last_phases, UNITIG_CLEAN_PHASES)

    # ---- persistence
    # ---- mapping reads onto the unitigs (the rule: include/kmx.h): a session on the handle, begin .. seq_to_unitigs .. end
    def unitig_map_begin(self, kmers: np.ndarray, k: int, ubuf: np.ndarray, uoffsets: np.ndarray) -> None:
        """kmx_unitig_map_begin: the index of a listing (packed canonical k-mers, strictly ascending, odd k in [5, 63]) and a
        unitig set (ubuf, uoffsets) in seq_to_occ_flat's layout, as any of the unitig calls returns it.  Needs no built model."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        W = (int(k) + 31) // 32
        if kmers.size % W:
            raise KmxError(-1, f"{kmers.size} words are no whole k-mers at k = {k}")
        ubuf, uoffsets = _flat_seqs(ubuf, uoffsets)
        _chk(self.L.kmx_unitig_map_begin(self.h, int(k), kmers.ctypes.data, kmers.size // W, ubuf.ctypes.data, uoffsets.ctypes.data, uoffsets.size - 1))
        self._map_units = uoffsets.size - 1

    def unitig_map_begin_dev(self, d_kmers, k: int, d_ubuf, d_uoffsets) -> None:
        """kmx_unitig_map_begin_dev on torch tensors of the model's device; d_kmers is borrowed until unitig_map_end (keep it alive)"""
        n = d_kmers.numel() // ((int(k) + 31) // 32)
        _chk(self.L.kmx_unitig_map_begin_dev(self.h, int(k), d_kmers.data_ptr(), n, d_ubuf.data_ptr(), d_uoffsets.data_ptr(), d_uoffsets.numel() - 1, d_ubuf.numel()))
        self._map_units = d_uoffsets.numel() - 1
        self._map_listing = d_kmers

    def count_unitig_map_begin(self, ubuf: np.ndarray, uoffsets: np.ndarray) -> None:
        """kmx_count_unitig_map_begin: the same on the listing the last count_finish / init_reads kept, read where it lies"""
        ubuf, uoffsets = _flat_seqs(ubuf, uoffsets)
        _chk(self.L.kmx_count_unitig_map_begin(self.h, ubuf.ctypes.data, uoffsets.ctypes.data, uoffsets.size - 1))
        self._map_units = uoffsets.size - 1

    def count_unitig_map_begin_dev(self, d_ubuf, d_uoffsets) -> None:
        """kmx_count_unitig_map_begin_dev: the unitig set as torch tensors on the model's device"""
        _chk(self.L.kmx_count_unitig_map_begin_dev(self.h, d_ubuf.data_ptr(), d_uoffsets.data_ptr(), d_uoffsets.numel() - 1, d_ubuf.numel()))
        self._map_units = d_uoffsets.numel() - 1

    def unitig_map_end(self) -> None:
        _chk(self.L.kmx_unitig_map_end(self.h))
        self._map_listing = None

    def seq_to_unitigs_flat(self, buf: np.ndarray, offsets: np.ndarray, capacity=None, records: bool = True, hits=None):
        """kmx_unitig_map_seqs on (uint8 bases, uint64 offsets [n_seqs + 1]) -> (SEQ_SEGMENT_DTYPE segments, uint64 seg_offsets
        [n_seqs + 1], SEQ_MAP_DTYPE records [n_seqs] or None).  hits (uint64 [n_unitigs], optional) is ADDED to.  capacity None:
        room for every window, so the call never comes back short; a number: that many segments (KmxError KMX_E_RANGE when short)."""
        buf, offsets = _flat_seqs(buf, offsets)
        n_seqs = offsets.size - 1
        cap = int(offsets[-1]) if capacity is None else int(capacity)
        segs = np.zeros(cap, dtype=SEQ_SEGMENT_DTYPE)
        so = np.zeros(n_seqs + 1, dtype=np.uint64)
        rec = np.zeros(n_seqs, dtype=SEQ_MAP_DTYPE) if records else None
        if hits is not None and (hits.dtype != np.uint64 or not hits.flags.c_contiguous or hits.size < getattr(self, "_map_units", 0)):
            raise KmxError(-1, "hits must be a contiguous uint64 array with one entry per unitig")
        ns = C.c_uint64(0)
        _chk(self.L.kmx_unitig_map_seqs(self.h, buf.ctypes.data, offsets.ctypes.data, n_seqs, segs.ctypes.data, cap, C.byref(ns), so.ctypes.data,
                                        rec.ctypes.data if records else None, hits.ctypes.data if hits is not None else None))
        return segs[:ns.value].copy(), so, rec

    def seq_to_unitigs(self, seqs, hits=None):
        """the same for a str / bytes read or a list of them -> (segments, seg_offsets, records)"""
        _, _, buf, offsets = _join_seqs(seqs)
        return self.seq_to_unitigs_flat(buf, offsets, hits=hits)

    def seq_to_unitigs_dev(self, d_seq, d_offsets, d_segs=None, d_seg_offsets=None, d_rec=None, d_hits=None):
        """kmx_unitig_map_seqs_dev on torch tensors of the model's device: d_seq uint8 [n_bases], d_offsets int64 [n_seqs + 1];
        d_segs uint8 [capacity, 24] (None: the sizing call), d_seg_offsets int64 [n_seqs + 1] (None: allocated), d_rec uint8
        [n_seqs, 64] or None, d_hits int64 [n_unitigs] or None (added to) -> (the number of segments, d_seg_offsets)."""
        import torch
        n_seqs = d_offsets.numel() - 1
        if d_seg_offsets is None:
            d_seg_offsets = torch.zeros(n_seqs + 1, dtype=torch.int64, device=d_seq.device)
        ns = C.c_uint64(0)
        _chk(self.L.kmx_unitig_map_seqs_dev(self.h, d_seq.data_ptr(), d_offsets.data_ptr(), n_seqs, d_seq.numel(),
                                            d_segs.data_ptr() if d_segs is not None else None, d_segs.shape[0] if d_segs is not None else 0, C.byref(ns),
                                            d_seg_offsets.data_ptr(), d_rec.data_ptr() if d_rec is not None else None, d_hits.data_ptr() if d_hits is not None else None))
        return ns.value, d_seg_offsets

    # ---- walks: the segments of a batch threaded through the unitig graph (the rule: include/kmx.h), inside the map session
    def unitig_walks_flat(self, segs: np.ndarray, seg_offsets: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, max_gap: int, max_indel: int = 1,
                          walk_capacity=None, step_capacity=None, link_hits=None):
        """kmx_unitig_walk_segs on what seq_to_unitigs_flat returned and the CSR of the graph the session's unitigs came from ->
        (WALK_DTYPE walks, uint64 walk_offsets [n_seqs + 1], uint32 steps, stats as a dict).  link_hits (uint64 [n_links], optional)
        is ADDED to.  Capacities None: room for every segment, so the call never comes back short."""
        segs = np.ascontiguousarray(segs, dtype=SEQ_SEGMENT_DTYPE)
        seg_offsets = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
        link_offsets = np.ascontiguousarray(link_offsets, dtype=np.uint64)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        n_seqs = seg_offsets.size - 1
        wcap = segs.size if walk_capacity is None else int(walk_capacity)
        scap = segs.size if step_capacity is None else int(step_capacity)
        walks = np.zeros(wcap, dtype=WALK_DTYPE)
        steps = np.zeros(scap, dtype=np.uint32)
        wo = np.zeros(n_seqs + 1, dtype=np.uint64)
        if link_hits is not None and (link_hits.dtype != np.uint64 or not link_hits.flags.c_contiguous or link_hits.size < links.size):
            raise KmxError(-1, "link_hits must be a contiguous uint64 array with one entry per link")
        par, st = WalkParams(int(max_gap), int(max_indel)), WalkStats()
        _chk(self.L.kmx_unitig_walk_segs(self.h, segs.ctypes.data, segs.size, seg_offsets.ctypes.data, n_seqs, link_offsets.ctypes.data, links.ctypes.data, links.size, C.byref(par),
                                         walks.ctypes.data, wcap, wo.ctypes.data, steps.ctypes.data, scap, link_hits.ctypes.data if link_hits is not None else None, C.byref(st)))
        return walks[:st.n_walks].copy(), wo, steps[:st.n_steps].copy(), st.as_dict()

    def unitig_walks_dev(self, d_segs, n_segs: int, d_seg_offsets, d_link_offsets, d_links, max_gap: int, max_indel: int = 1, d_walks=None, d_steps=None, d_walk_offsets=None,
                         d_link_hits=None):
        """kmx_unitig_walk_segs_dev on torch tensors of the model's device, read where seq_to_unitigs_dev and the graph call left
        them: d_segs uint8 [capacity, 24] holding n_segs segments, d_seg_offsets int64 [n_seqs + 1], d_link_offsets int64
        [2 U + 1], d_links int32 [n_links]; d_walks uint8 [walk_capacity, 80] (None: the sizing call) with d_steps int32
        [step_capacity], d_walk_offsets int64 [n_seqs + 1] (None: allocated), d_link_hits int64 [n_links] or None (added to)
        -> (stats as a dict, d_walk_offsets)."""
        import torch
        n_seqs = d_seg_offsets.numel() - 1
        if d_walk_offsets is None:
            d_walk_offsets = torch.zeros(n_seqs + 1, dtype=torch.int64, device=d_seg_offsets.device)
        par, st = WalkParams(int(max_gap), int(max_indel)), WalkStats()
        _chk(self.L.kmx_unitig_walk_segs_dev(self.h, d_segs.data_ptr() if d_segs is not None else None, int(n_segs), d_seg_offsets.data_ptr(), n_seqs, d_link_offsets.data_ptr(),
                                             d_links.data_ptr(), d_links.numel(), C.byref(par), d_walks.data_ptr() if d_walks is not None else None,
                                             d_walks.shape[0] if d_walks is not None else 0, d_walk_offsets.data_ptr(), d_steps.data_ptr() if d_steps is not None else None,
                                             d_steps.numel() if d_steps is not None else 0, d_link_hits.data_ptr() if d_link_hits is not None else None, C.byref(st)))
        return st.as_dict(), d_walk_offsets

    def seq_to_walks(self, reads, link_offsets: np.ndarray, links: np.ndarray, max_gap: int, max_indel: int = 1, link_hits=None):
        """seq_to_unitigs, then unitig_walks_flat on its segments -> (walks, walk_offsets, steps, stats, segments, seg_offsets)"""
        segs, so, _ = self.seq_to_unitigs(reads)
        walks, wo, steps, st = self.unitig_walks_flat(segs, so, link_offsets, links, max_gap, max_indel, link_hits=link_hits)
        return walks, wo, steps, st, segs, so

    # ---- read pairs: the two mates of every pair placed in the graph (the rule: include/kmx.h), inside the map session
    def unitig_pairs_flat(self, walks: np.ndarray, walk_offsets: np.ndarray, steps: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, max_dist: int, min_mapped: int = 1,
                          bin_width: int = 10, n_bins: int = 200, plinks=None, capacity=None, hist=None, pair_hits=None, records: bool = True):
        """kmx_unitig_pair_walks on what unitig_walks_flat returned for a batch of interleaved mates and the CSR of the session's
        graph -> (PAIR_DTYPE records [n_pairs] or None, PAIR_LINK_DTYPE list, stats as a dict).  plinks: the list earlier batches
        left (None: empty; False: no list is built and None comes back); the merged list is returned, the argument is not
        changed.  capacity None: room for every entry, so the call never comes back short; a number: that many entries (KmxError
        KMX_E_RANGE when short, its `needed` the number needed).  hist (uint64 [n_bins]) and pair_hits (uint64 [n_links]), both
        optional, are ADDED to."""
        walks = np.ascontiguousarray(walks, dtype=WALK_DTYPE)
        walk_offsets = np.ascontiguousarray(walk_offsets, dtype=np.uint64)
        steps = np.ascontiguousarray(steps, dtype=np.uint32)
        link_offsets = np.ascontiguousarray(link_offsets, dtype=np.uint64)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        n_seqs = walk_offsets.size - 1
        if hist is not None and (hist.dtype != np.uint64 or not hist.flags.c_contiguous or hist.size < int(n_bins)):
            raise KmxError(-1, "hist must be a contiguous uint64 array with one entry per bin")
        if pair_hits is not None and (pair_hits.dtype != np.uint64 or not pair_hits.flags.c_contiguous or pair_hits.size < links.size):
            raise KmxError(-1, "pair_hits must be a contiguous uint64 array with one entry per link")
        rec = np.zeros(n_seqs // 2, dtype=PAIR_DTYPE) if records else None
        par, st, n = PairParams(int(min_mapped), int(max_dist), int(bin_width), int(n_bins)), PairStats(), C.c_uint64(0)
        lst = None
        if plinks is not False:
            old = np.zeros(0, dtype=PAIR_LINK_DTYPE) if plinks is None else np.ascontiguousarray(plinks, dtype=PAIR_LINK_DTYPE)
            cap = old.size + n_seqs // 2 if capacity is None else int(capacity)
            lst = np.zeros(max(cap, old.size), dtype=PAIR_LINK_DTYPE)
            lst[:old.size] = old
            n.value = old.size
        try:
            _chk(self.L.kmx_unitig_pair_walks(self.h, walks.ctypes.data, walks.size, walk_offsets.ctypes.data, n_seqs, steps.ctypes.data, steps.size, link_offsets.ctypes.data, links.ctypes.data,
                                              links.size, C.byref(par), rec.ctypes.data if records else None, hist.ctypes.data if hist is not None else None,
                                              pair_hits.ctypes.data if pair_hits is not None else None, lst.ctypes.data if lst is not None else None, cap if lst is not None else 0, C.byref(n),
                                              C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            raise
        return rec, (lst[:n.value].copy() if lst is not None else None), st.as_dict()

    def unitig_pairs_dev(self, d_walks, n_walks: int, d_walk_offsets, d_steps, n_steps: int, d_link_offsets, d_links, max_dist: int, min_mapped: int = 1, bin_width: int = 10,
                         n_bins: int = 200, d_pairs=None, d_hist=None, d_pair_hits=None, d_plinks=None, n_plinks: int = 0):
        """kmx_unitig_pair_walks_dev on torch tensors of the model's device, read where unitig_walks_dev and the graph call left
        them: d_walks uint8 [walk_capacity, 80] holding n_walks walks, d_walk_offsets int64 [n_seqs + 1], d_steps int32 holding
        n_steps steps, d_link_offsets int64 [2 U + 1], d_links int32 [n_links]; d_pairs uint8 [n_pairs, 64] or None, d_hist int64
        [n_bins] and d_pair_hits int64 [n_links] or None (added to), d_plinks uint8 [capacity, 32] holding n_plinks entries or
        None -> (stats as a dict, the entries the list now holds).  KmxError KMX_E_RANGE carries the number needed in `needed`."""
        n_seqs = d_walk_offsets.numel() - 1
        par, st, n = PairParams(int(min_mapped), int(max_dist), int(bin_width), int(n_bins)), PairStats(), C.c_uint64(int(n_plinks))
        ptr = lambda t: t.data_ptr() if t is not None else None
        try:
            _chk(self.L.kmx_unitig_pair_walks_dev(self.h, d_walks.data_ptr() if n_walks else None, int(n_walks), d_walk_offsets.data_ptr(), n_seqs, d_steps.data_ptr() if n_steps else None,
                                                  int(n_steps), d_link_offsets.data_ptr(), d_links.data_ptr() if d_links.numel() else None, d_links.numel(), C.byref(par), ptr(d_pairs), ptr(d_hist),
                                                  ptr(d_pair_hits), ptr(d_plinks), d_plinks.shape[0] if d_plinks is not None else 0, C.byref(n), C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            raise
        return st.as_dict(), int(n.value)

    def seq_to_pairs(self, reads, link_offsets: np.ndarray, links: np.ndarray, max_dist: int, max_gap: int, max_indel: int = 1, min_mapped: int = 1, bin_width: int = 10, n_bins: int = 200,
                     plinks=None, hist=None, pair_hits=None, link_hits=None):
        """inside a map session, on interleaved reads (2 p and 2 p + 1 are the mates of pair p): seq_to_walks, then
        unitig_pairs_flat on its walks -> (pair records, the merged list, pair stats, walks, walk_offsets, steps)"""
        walks, wo, steps, _, _, _ = self.seq_to_walks(reads, link_offsets, links, max_gap, max_indel, link_hits=link_hits)
        rec, lst, st = self.unitig_pairs_flat(walks, wo, steps, link_offsets, links, max_dist, min_mapped, bin_width, n_bins, plinks=plinks, hist=hist, pair_hits=pair_hits)
        return rec, lst, st, walks, wo, steps

    # ---- scaffolds: unitigs or contigs joined along the pair links, with runs of N (the rule: include/kmx.h); no model, no session
    def unitig_scaffold_flat(self, k: int, ubuf: np.ndarray, uoffsets: np.ndarray, plinks: np.ndarray, inner: int, min_pairs: int = 2, ratio: int = 0, min_n: int = 10, max_n: int = 1000,
                             urec=None, capacity=None):
        """kmx_unitig_scaffold on a unitig set (uint8 bases, uint64 offsets [U + 1], optionally its UNITIG_DTYPE records) and the
        PAIR_LINK_DTYPE list unitig_pairs_flat left -> (uint8 scaffold bases, uint64 soffsets [S + 1], SCAFFOLD_DTYPE records [S],
        SCAFFOLD_STEP_DTYPE steps [U], SCAFFOLD_PLACE_DTYPE place [U], stats as a dict).  capacity None: n_ubases + (U - 1) * max_n,
        which always suffices; a number: that many bytes, 0 being the sizing call (KmxError KMX_E_RANGE when short: its `needed`
        the bytes needed, its `result` everything but the bases)."""
        ubuf = np.ascontiguousarray(ubuf, dtype=np.uint8)
        uoffsets = np.ascontiguousarray(uoffsets, dtype=np.uint64)
        plinks = np.ascontiguousarray(plinks, dtype=PAIR_LINK_DTYPE)
        nu = uoffsets.size - 1
        if urec is not None:
            urec = np.ascontiguousarray(urec, dtype=UNITIG_DTYPE)
            if urec.size != nu:
                raise KmxError(-1, "urec holds one record per unitig")
        cap = ubuf.size + max(nu - 1, 0) * int(max_n) if capacity is None else int(capacity)
        sseq = np.zeros(cap, dtype=np.uint8) if cap else None
        soffs = np.zeros(nu + 1, dtype=np.uint64)
        srec = np.zeros(max(nu, 1), dtype=SCAFFOLD_DTYPE)
        steps = np.zeros(max(nu, 1), dtype=SCAFFOLD_STEP_DTYPE)
        place = np.zeros(max(nu, 1), dtype=SCAFFOLD_PLACE_DTYPE)
        par, st = ScaffoldParams(int(min_pairs), int(ratio), int(inner), int(min_n), int(max_n), 0), ScaffoldStats()
        ns, nb = C.c_uint64(0), C.c_uint64(0)
        try:
            _chk(self.L.kmx_unitig_scaffold(self.h, int(k), ubuf.ctypes.data, uoffsets.ctypes.data, nu, urec.ctypes.data if urec is not None else None, plinks.ctypes.data if plinks.size else None,
                                            plinks.size, C.byref(par), sseq.ctypes.data if cap else None, cap, soffs.ctypes.data, srec.ctypes.data, steps.ctypes.data, place.ctypes.data,
                                            C.byref(ns), C.byref(nb), C.byref(st)))
        except KmxError as e:
            e.needed = int(nb.value)
            e.result = (soffs[:ns.value + 1].copy(), srec[:ns.value].copy(), steps[:nu].copy(), place[:nu].copy(), st.as_dict())
            raise
        s, b = ns.value, nb.value
        return (sseq[:b].copy() if cap else np.zeros(0, dtype=np.uint8)), soffs[:s + 1].copy(), srec[:s].copy(), steps[:nu].copy(), place[:nu].copy(), st.as_dict()

    def unitig_scaffold_dev(self, k: int, d_ubuf, d_uoffsets, d_plinks, n_plinks: int, inner: int, min_pairs: int = 2, ratio: int = 0, min_n: int = 10, max_n: int = 1000, d_urec=None,
                            capacity=None, out=None):
        """kmx_unitig_scaffold_dev on torch tensors of the model's device, read where the graph, contig and pair calls left them:
        d_ubuf uint8 [n_ubases], d_uoffsets int64 [U + 1], d_plinks uint8 [capacity, 32] holding n_plinks entries (or None),
        d_urec uint8 [U, 40] or None.  out: the five output tensors (d_sseq uint8 [capacity] or None for the sizing call, d_soffsets
        int64 [U + 1], d_srec uint8 [U, 64], d_steps uint8 [U, 16], d_place uint8 [U, 16]), allocated when None with `capacity`
        bytes (None: n_ubases + (U - 1) * max_n) -> (out, (n_scaffolds, n_sbases), stats as a dict).  KmxError KMX_E_RANGE carries the
        bytes needed in `needed` and everything else in `result`."""
        import torch
        nu, nb, dev = d_uoffsets.numel() - 1, d_ubuf.numel(), d_uoffsets.device
        if out is None:
            cap = nb + max(nu - 1, 0) * int(max_n) if capacity is None else int(capacity)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            out = (z(cap, torch.uint8) if cap else None, z(nu + 1, torch.int64), z((max(nu, 1), 64), torch.uint8), z((max(nu, 1), 16), torch.uint8), z((max(nu, 1), 16), torch.uint8))
        par, st = ScaffoldParams(int(min_pairs), int(ratio), int(inner), int(min_n), int(max_n), 0), ScaffoldStats()
        ns, nsb = C.c_uint64(0), C.c_uint64(0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        try:
            _chk(self.L.kmx_unitig_scaffold_dev(self.h, int(k), d_ubuf.data_ptr(), d_uoffsets.data_ptr(), nu, nb, ptr(d_urec), ptr(d_plinks) if n_plinks else None, int(n_plinks), C.byref(par),
                                                ptr(out[0]), out[0].numel() if out[0] is not None else 0, *[t.data_ptr() for t in out[1:]], C.byref(ns), C.byref(nsb), C.byref(st)))
        except KmxError as e:
            e.needed = int(nsb.value)
            e.result = (out, (ns.value, nsb.value), st.as_dict())
            raise
        return out, (ns.value, nsb.value), st.as_dict()

    def scaffolds_from_pairs(self, k: int, strs, plinks: np.ndarray, inner: int, min_pairs: int = 2, ratio: int = 0, min_n: int = 10, max_n: int = 1000):
        """unitig_scaffold_flat on a list of unitig or contig strings and a pair list -> (the scaffold strings as str, SCAFFOLD_DTYPE
        records, SCAFFOLD_STEP_DTYPE steps, SCAFFOLD_PLACE_DTYPE place, stats as a dict)"""
        _, _, ubuf, uoffs = _join_seqs(list(strs))
        sseq, soffs, srec, steps, place, st = self.unitig_scaffold_flat(k, ubuf, uoffs, plinks, inner, min_pairs, ratio, min_n, max_n)
        return [b.decode("latin-1") for b in _split_seqs(sseq, soffs)], srec, steps, place, st

    def unitig_scaffold_phases(self) -> dict:
        """kmx_unitig_scaffold_last_phases: seconds per phase of the last scaffold call (under set_profile(1)) and its doubling rounds"""
        sec, rounds = (C.c_double * 5)(), C.c_uint64(0)
        _chk(self.L.kmx_unitig_scaffold_last_phases(self.h, sec, C.byref(rounds)))
        return dict(zip(("verdicts", "ranking", "marks", "records", "bytes"), (float(x) for x in sec)), rounds=int(rounds.value))

    # ---- pair paths: the graph path every entry of a pair list stands for (the rule: include/kmx.h); no model, no session
    def unitig_pair_paths_flat(self, k: int, uoffsets: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, plinks: np.ndarray, inner: int, tol: int, min_pairs: int = 2, max_steps: int = 8,
                               max_visits: int = 4096, through=None, path_hits=None, capacity=None, steps: bool = True):
        """kmx_unitig_pair_paths on the offsets of a unitig set (uint64 [U + 1]), the CSR of its graph and the PAIR_LINK_DTYPE list
        unitig_pairs_flat left -> (PAIR_PATH_DTYPE records [n_plinks], uint32 psteps or None, stats as a dict).  through (uint64
        [16 U]) and path_hits (uint64 [n_links]), both optional, are ADDED to.  capacity None: n_plinks * max_steps, which always
        suffices; a number: that many steps (KmxError KMX_E_RANGE when short: its `needed` the steps needed, its `result` the
        records and the stats).  steps False: no list is built."""
        uoffsets = np.ascontiguousarray(uoffsets, dtype=np.uint64)
        link_offsets = np.ascontiguousarray(link_offsets, dtype=np.uint64)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        plinks = np.ascontiguousarray(plinks, dtype=PAIR_LINK_DTYPE)
        nu = uoffsets.size - 1
        if link_offsets.size != 2 * nu + 1:
            raise KmxError(-1, "link_offsets holds 2 U + 1 entries")
        if through is not None and (through.dtype != np.uint64 or not through.flags.c_contiguous or through.size < 16 * nu):
            raise KmxError(-1, "through must be a contiguous uint64 array with 16 entries per unitig")
        if path_hits is not None and (path_hits.dtype != np.uint64 or not path_hits.flags.c_contiguous or path_hits.size < links.size):
            raise KmxError(-1, "path_hits must be a contiguous uint64 array with one entry per link")
        cap = plinks.size * int(max_steps) if capacity is None else int(capacity)
        rec = np.zeros(max(plinks.size, 1), dtype=PAIR_PATH_DTYPE)
        pst = np.zeros(max(cap, 1), dtype=np.uint32) if steps else None
        par, st, n = PairPathParams(int(min_pairs), int(inner), int(tol), int(max_steps), int(max_visits), 0), PairPathStats(), C.c_uint64(0)
        try:
            _chk(self.L.kmx_unitig_pair_paths(self.h, int(k), uoffsets.ctypes.data, nu, link_offsets.ctypes.data, links.ctypes.data if links.size else None, links.size,
                                              plinks.ctypes.data if plinks.size else None, plinks.size, C.byref(par), rec.ctypes.data, pst.ctypes.data if steps else None, cap if steps else 0,
                                              C.byref(n), through.ctypes.data if through is not None else None, path_hits.ctypes.data if path_hits is not None else None, C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            e.result = (rec[:plinks.size].copy(), st.as_dict())
            raise
        return rec[:plinks.size].copy(), (pst[:n.value].copy() if steps else None), st.as_dict()

    def unitig_pair_paths_dev(self, k: int, d_uoffsets, d_link_offsets, d_links, d_plinks, n_plinks: int, inner: int, tol: int, min_pairs: int = 2, max_steps: int = 8, max_visits: int = 4096,
                              d_through=None, d_path_hits=None, capacity=None, out=None):
        """kmx_unitig_pair_paths_dev on torch tensors of the model's device, read where the graph and pair calls left them:
        d_uoffsets int64 [U + 1], d_link_offsets int64 [2 U + 1], d_links int32 [n_links], d_plinks uint8 [capacity, 32] holding
        n_plinks entries; d_through int64 [16 U] and d_path_hits int64 [n_links] or None (added to).  out: (d_precs uint8
        [n_plinks, 32], d_psteps int32 [capacity] or None for no list), allocated when None with `capacity` steps (None: n_plinks *
        max_steps) -> (out, the steps the list holds, stats as a dict).  KmxError KMX_E_RANGE carries the steps needed in `needed`."""
        import torch
        nu, dev = d_uoffsets.numel() - 1, d_uoffsets.device
        if out is None:
            cap = int(n_plinks) * int(max_steps) if capacity is None else int(capacity)
            out = (torch.zeros((max(int(n_plinks), 1), 32), dtype=torch.uint8, device=dev), torch.zeros(max(cap, 1), dtype=torch.int32, device=dev))
        else:
            cap = out[1].numel() if out[1] is not None and capacity is None else int(capacity or 0)
        par, st, n = PairPathParams(int(min_pairs), int(inner), int(tol), int(max_steps), int(max_visits), 0), PairPathStats(), C.c_uint64(0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        try:
            _chk(self.L.kmx_unitig_pair_paths_dev(self.h, int(k), d_uoffsets.data_ptr(), nu, d_link_offsets.data_ptr(), d_links.data_ptr() if d_links.numel() else None, d_links.numel(),
                                                  ptr(d_plinks) if n_plinks else None, int(n_plinks), C.byref(par), out[0].data_ptr(), ptr(out[1]), cap if out[1] is not None else 0, C.byref(n),
                                                  ptr(d_through), ptr(d_path_hits), C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            raise
        return out, int(n.value), st.as_dict()

    def unitig_pair_paths_phases(self) -> dict:
        """kmx_unitig_pair_paths_last_phases: seconds per phase of the last pair path call (under set_profile(1))"""
        sec = (C.c_double * 3)()
        _chk(self.L.kmx_unitig_pair_paths_last_phases(self.h, sec))
        return dict(zip(("search", "scan", "apply"), (float(x) for x in sec)))

    # ---- reduced pair lists: a pair list without the entries that skip a unitig (the rule: include/kmx.h); no model, no session
    def unitig_pair_reduce_flat(self, k: int, uoffsets: np.ndarray, plinks: np.ndarray, inner: int, tol: int, min_pairs: int = 2, max_row: int = 64, capacity=None, lists: bool = True):
        """kmx_unitig_pair_reduce on the offsets of a unitig set (uint64 [U + 1]) and the PAIR_LINK_DTYPE list unitig_pairs_flat left
        -> (PAIR_REDUCE_DTYPE records [n_plinks], the PAIR_LINK_DTYPE list that stays or None, uint32 origin or None, stats as a
        dict).  capacity None: n_plinks, which always suffices; a number: that many entries (KmxError KMX_E_RANGE when short: its
        `needed` the entries needed, its `result` the records and the stats).  lists False: the verdicts only."""
        uoffsets = np.ascontiguousarray(uoffsets, dtype=np.uint64)
        plinks = np.ascontiguousarray(plinks, dtype=PAIR_LINK_DTYPE)
        nu, np_ = uoffsets.size - 1, plinks.size
        cap = np_ if capacity is None else int(capacity)
        rec = np.zeros(max(np_, 1), dtype=PAIR_REDUCE_DTYPE)
        lout = np.zeros(max(cap, 1), dtype=PAIR_LINK_DTYPE) if lists else None
        org = np.zeros(max(cap, 1), dtype=np.uint32) if lists else None
        par, st, n = PairReduceParams(int(min_pairs), int(inner), int(tol), int(max_row), 0), PairReduceStats(), C.c_uint64(0)
        try:
            _chk(self.L.kmx_unitig_pair_reduce(self.h, int(k), uoffsets.ctypes.data, nu, plinks.ctypes.data if np_ else None, np_, C.byref(par), rec.ctypes.data,
                                               lout.ctypes.data if lists else None, org.ctypes.data if lists else None, cap if lists else 0, C.byref(n), C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            e.result = (rec[:np_].copy(), st.as_dict())
            raise
        return rec[:np_].copy(), (lout[:n.value].copy() if lists else None), (org[:n.value].copy() if lists else None), st.as_dict()

    def unitig_pair_reduce_dev(self, k: int, d_uoffsets, n_ubases: int, d_plinks, n_plinks: int, inner: int, tol: int, min_pairs: int = 2, max_row: int = 64, capacity=None, out=None):
        """kmx_unitig_pair_reduce_dev on torch tensors of the model's device, read where the pair call left them: d_uoffsets int64
        [U + 1], d_plinks uint8 [>= n_plinks, 32].  out: (d_rrecs uint8 [n_plinks, 32], d_lout uint8 [capacity, 32] or None, d_origin
        int32 [capacity] or None; both None: the verdicts only), allocated when None with `capacity` entries (None: n_plinks) ->
        (out, the entries that stay, stats as a dict).  KmxError KMX_E_RANGE carries the entries needed in `needed` and the stats
        in `result`."""
        import torch
        nu, dev = d_uoffsets.numel() - 1, d_uoffsets.device
        if out is None:
            cap = int(n_plinks) if capacity is None else int(capacity)
            out = (torch.zeros((max(int(n_plinks), 1), 32), dtype=torch.uint8, device=dev), torch.zeros((max(cap, 1), 32), dtype=torch.uint8, device=dev),
                   torch.zeros(max(cap, 1), dtype=torch.int32, device=dev))
        else:
            cap = min(t.shape[0] for t in out[1:] if t is not None) if capacity is None and (out[1] is not None or out[2] is not None) else int(capacity or 0)
        par, st, n = PairReduceParams(int(min_pairs), int(inner), int(tol), int(max_row), 0), PairReduceStats(), C.c_uint64(0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        try:
            _chk(self.L.kmx_unitig_pair_reduce_dev(self.h, int(k), d_uoffsets.data_ptr(), nu, int(n_ubases), ptr(d_plinks) if n_plinks else None, int(n_plinks), C.byref(par), out[0].data_ptr(),
                                                   ptr(out[1]), ptr(out[2]), cap, C.byref(n), C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            e.result = st.as_dict()
            raise
        return out, int(n.value), st.as_dict()

    def unitig_pair_reduce_phases(self) -> dict:
        """kmx_unitig_pair_reduce_last_phases: seconds per phase of the last reduce call (under set_profile(1))"""
        sec = (C.c_double * 4)()
        _chk(self.L.kmx_unitig_pair_reduce_last_phases(self.h, sec))
        return dict(zip(("rows", "sort", "verdicts", "compact"), (float(x) for x in sec)))

    def reduced_scaffolds_from_pairs(self, k: int, strs, plinks: np.ndarray, inner: int, min_pairs: int = 2, ratio: int = 0, min_n: int = 10, max_n: int = 1000, tol=None, max_row: int = 64):
        """on a list of unitig or contig strings and a pair list: unitig_pair_reduce_flat at min_pairs and inner with tol (None: k),
        then scaffolds_from_pairs on the list that stays -> (what scaffolds_from_pairs returns, then the reduce records, the
        reduced list and the reduce stats)"""
        _, _, _, uoffs = _join_seqs(list(strs))
        rec, lout, _, rst = self.unitig_pair_reduce_flat(k, uoffs, plinks, inner, int(k) if tol is None else int(tol), min_pairs, max_row)
        return self.scaffolds_from_pairs(k, strs, lout, inner, min_pairs, ratio, min_n, max_n) + (rec, lout, rst)

    # ---- lifted pair lists: a unitig-level pair list in contig coordinates (the rule: include/kmx.h); no model, no session
    def unitig_pair_lift_flat(self, k: int, uoffsets: np.ndarray, place: np.ndarray, crec: np.ndarray, plinks: np.ndarray, max_dist: int, capacity=None, lists: bool = True):
        """kmx_unitig_pair_lift on the offsets of a unitig set (uint64 [U + 1]), the CONTIG_PLACE_DTYPE place [U] and CONTIG_DTYPE
        records [C] unitig_contigs_flat returned for it, and the PAIR_LINK_DTYPE list unitig_pairs_flat left on the unitigs ->
        (PAIR_LIFT_DTYPE records [n_plinks], the PAIR_LINK_DTYPE list in contig coordinates or None, stats as a dict).  capacity
        None: n_plinks, which always suffices; a number: that many entries (KmxError KMX_E_RANGE when short: its `needed` the
        entries needed, its `result` the records and the stats).  lists False: the sizing call."""
        uoffsets = np.ascontiguousarray(uoffsets, dtype=np.uint64)
        place = np.ascontiguousarray(place, dtype=CONTIG_PLACE_DTYPE)
        crec = np.ascontiguousarray(crec, dtype=CONTIG_DTYPE)
        plinks = np.ascontiguousarray(plinks, dtype=PAIR_LINK_DTYPE)
        nu, nc, np_ = uoffsets.size - 1, crec.size, plinks.size
        if place.size != nu:
            raise KmxError(-1, "place holds one entry per unitig")
        cap = np_ if capacity is None else int(capacity)
        rec = np.zeros(max(np_, 1), dtype=PAIR_LIFT_DTYPE)
        lout = np.zeros(max(cap, 1), dtype=PAIR_LINK_DTYPE) if lists else None
        par, st, n = PairLiftParams(int(max_dist), 0), PairLiftStats(), C.c_uint64(0)
        try:
            _chk(self.L.kmx_unitig_pair_lift(self.h, int(k), uoffsets.ctypes.data, nu, place.ctypes.data if nu else None, crec.ctypes.data if nc else None, nc,
                                             plinks.ctypes.data if np_ else None, np_, C.byref(par), rec.ctypes.data, lout.ctypes.data if lists else None, cap if lists else 0, C.byref(n),
                                             C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            e.result = (rec[:np_].copy(), st.as_dict())
            raise
        return rec[:np_].copy(), (lout[:n.value].copy() if lists else None), st.as_dict()

    def unitig_pair_lift_dev(self, k: int, d_uoffsets, n_ubases: int, d_place, d_crec, n_contigs: int, d_plinks, n_plinks: int, max_dist: int, capacity=None, out=None):
        """kmx_unitig_pair_lift_dev on torch tensors of the model's device, read where the contig and pair calls left them:
        d_uoffsets int64 [U + 1], d_place int32 [U, 2], d_crec uint8 [>= n_contigs, 64], d_plinks uint8 [>= n_plinks, 32].  out:
        (d_lrec uint8 [n_plinks, 32], d_lout uint8 [capacity, 32] or None for the sizing call), allocated when None with
        `capacity` entries (None: n_plinks) -> (out, the entries of the lifted list, stats as a dict).  KmxError KMX_E_RANGE
        carries the entries needed in `needed` and the stats in `result`."""
        import torch
        nu, dev = d_uoffsets.numel() - 1, d_uoffsets.device
        if out is None:
            cap = int(n_plinks) if capacity is None else int(capacity)
            out = (torch.zeros((max(int(n_plinks), 1), 32), dtype=torch.uint8, device=dev), torch.zeros((max(cap, 1), 32), dtype=torch.uint8, device=dev))
        else:
            cap = (out[1].shape[0] if out[1] is not None else 0) if capacity is None else int(capacity)
        par, st, n = PairLiftParams(int(max_dist), 0), PairLiftStats(), C.c_uint64(0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        try:
            _chk(self.L.kmx_unitig_pair_lift_dev(self.h, int(k), d_uoffsets.data_ptr(), nu, int(n_ubases), ptr(d_place) if nu else None, ptr(d_crec) if n_contigs else None, int(n_contigs),
                                                 ptr(d_plinks) if n_plinks else None, int(n_plinks), C.byref(par), out[0].data_ptr(), ptr(out[1]), cap, C.byref(n), C.byref(st)))
        except KmxError as e:
            e.needed = int(n.value)
            e.result = st.as_dict()
            raise
        return out, int(n.value), st.as_dict()

    def unitig_pair_lift_fold(self, variant) -> None:
        """kmx_unitig_pair_lift_fold_variant: "wave" or "plain" (or its number), the fold kernel of the next lift calls; for measuring"""
        _chk(self.L.kmx_unitig_pair_lift_fold_variant(self.h, int(PAIR_LIFT_FOLDS.get(variant, variant))))

    def unitig_pair_lift_phases(self) -> dict:
        """kmx_unitig_pair_lift_last_phases: seconds per phase of the last lift call (under set_profile(1))"""
        sec = (C.c_double * 4)()
        _chk(self.L.kmx_unitig_pair_lift_last_phases(self.h, sec))
        return dict(zip(("classify", "sort", "fold", "store"), (float(x) for x in sec)))

    def lifted_scaffolds_from_pairs(self, k: int, ustrs, place: np.ndarray, crec: np.ndarray, cstrs, plinks: np.ndarray, inner: int, max_dist: int, min_pairs: int = 2, ratio: int = 0,
                                    min_n: int = 10, max_n: int = 1000):
        """on the unitig strings a pair list was built on, the place and records unitig_contigs_flat returned for them and the contig
        strings: unitig_pair_lift_flat at max_dist, then scaffolds_from_pairs of the contigs on the lifted list -> (what
        scaffolds_from_pairs returns, then the lift records, the lifted list and the lift stats)"""
        _, _, _, uoffs = _join_seqs(list(ustrs))
        rec, lout, lst = self.unitig_pair_lift_flat(k, uoffs, place, crec, plinks, max_dist)
        return self.scaffolds_from_pairs(k, cstrs, lout, inner, min_pairs, ratio, min_n, max_n) + (rec, lout, lst)

    # ---- filled scaffolds: the scaffolds spelled again with the graph's bases in the gaps the pair paths cross (the rule:
    # include/kmx.h); no model, no session, no CSR
    def unitig_scaffold_fill_flat(self, k: int, ubuf: np.ndarray, uoffsets: np.ndarray, srec: np.ndarray, steps: np.ndarray, plinks: np.ndarray, precs: np.ndarray, psteps, kinds: int = 3,
                                  capacity=None, piece_capacity=None, pieces: bool = True):
        """kmx_unitig_scaffold_fill on the unitig set the scaffold call was given, the SCAFFOLD_DTYPE records [S] and
        SCAFFOLD_STEP_DTYPE steps [U] it returned, the PAIR_LINK_DTYPE list, and the PAIR_PATH_DTYPE records and uint32 steps
        unitig_pair_paths_flat returned on it -> (uint8 bases, uint64 foffsets [S + 1], SCAFFOLD_FILL_DTYPE records [S],
        FILL_STEP_DTYPE steps [U], uint32 pieces or None, stats as a dict).  capacity None: a sizing call first, then the bytes it
        asked for; a number: that many bytes, 0 being the sizing call.  piece_capacity None: the
        size of psteps.  KmxError KMX_E_RANGE when either is short: its `needed` the bytes needed, its `needed_pieces` the
        pieces, its `result` everything but the bases.  pieces False: no list is built."""
        ubuf = np.ascontiguousarray(ubuf, dtype=np.uint8)
        uoffsets = np.ascontiguousarray(uoffsets, dtype=np.uint64)
        srec = np.ascontiguousarray(srec, dtype=SCAFFOLD_DTYPE)
        steps = np.ascontiguousarray(steps, dtype=SCAFFOLD_STEP_DTYPE)
        plinks = np.ascontiguousarray(plinks, dtype=PAIR_LINK_DTYPE)
        precs = np.ascontiguousarray(precs, dtype=PAIR_PATH_DTYPE)
        psteps = np.zeros(0, dtype=np.uint32) if psteps is None else np.ascontiguousarray(psteps, dtype=np.uint32)
        nu, ns = uoffsets.size - 1, srec.size
        if steps.size != nu or precs.size != plinks.size:
            raise KmxError(-1, "steps holds one entry per unitig and precs one per pair link")
        if capacity is None:                                      # the sizing call says what is needed
            try:
                return self.unitig_scaffold_fill_flat(k, ubuf, uoffsets, srec, steps, plinks, precs, psteps, kinds, 0, piece_capacity, pieces)
            except KmxError as e:
                if e.code != -5 or not getattr(e, "needed", 0):
                    raise
                capacity = e.needed
        cap = int(capacity)
        pcap = (psteps.size if piece_capacity is None else int(piece_capacity)) if pieces else 0
        fseq = np.zeros(cap, dtype=np.uint8) if cap else None
        foffs = np.zeros(ns + 1, dtype=np.uint64)
        frec = np.zeros(max(ns, 1), dtype=SCAFFOLD_FILL_DTYPE)
        fst = np.zeros(max(nu, 1), dtype=FILL_STEP_DTYPE)
        pcs = np.zeros(max(pcap, 1), dtype=np.uint32) if pieces else None
        par, st, nb, npc = FillParams(int(kinds), 0), FillStats(), C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        try:
            _chk(self.L.kmx_unitig_scaffold_fill(self.h, int(k), ubuf.ctypes.data, uoffsets.ctypes.data, nu, ptr(srec), ns, ptr(steps), ptr(plinks), plinks.size, ptr(precs), ptr(psteps), psteps.size,
                                                 C.byref(par), ptr(fseq), cap, foffs.ctypes.data, frec.ctypes.data, fst.ctypes.data, pcs.ctypes.data if pieces else None, pcap, C.byref(nb),
                                                 C.byref(npc), C.byref(st)))
        except KmxError as e:
            e.needed, e.needed_pieces = int(nb.value), int(npc.value)
            e.result = (foffs.copy(), frec[:ns].copy(), fst[:nu].copy(), (pcs[:min(npc.value, pcap)].copy() if pieces else None), st.as_dict())
            raise
        return ((fseq[:nb.value].copy() if cap else np.zeros(0, dtype=np.uint8)), foffs.copy(), frec[:ns].copy(), fst[:nu].copy(), (pcs[:npc.value].copy() if pieces else None), st.as_dict())

    def unitig_scaffold_fill_dev(self, k: int, d_ubuf, d_uoffsets, d_srec, n_scaffolds: int, d_steps, d_plinks, n_plinks: int, d_precs, d_psteps, n_psteps: int, kinds: int = 3, capacity: int = 0,
                                 piece_capacity: int = 0, out=None):
        """kmx_unitig_scaffold_fill_dev on torch tensors of the model's device, read where the scaffold and pair-path calls left
        them: d_ubuf uint8 [n_ubases], d_uoffsets int64 [U + 1], d_srec uint8 [>= S, 64], d_steps uint8 [U, 16], d_plinks uint8
        [>= n_plinks, 32], d_precs uint8 [>= n_plinks, 32], d_psteps int32 [>= n_psteps].  out: the five output tensors (d_fseq
        uint8 [capacity] or None for the sizing call, d_foffsets int64 [S + 1], d_frec uint8 [S, 64], d_fsteps uint8 [U, 32],
        d_pieces int32 [piece_capacity] or None for no list), allocated when None from `capacity` and `piece_capacity` ->
        (out, (n_fbases, n_pieces), stats as a dict).  KmxError KMX_E_RANGE carries the bytes needed in `needed`, the pieces in
        `needed_pieces` and everything else in `result`."""
        import torch
        nu, nb, dev, ns = d_uoffsets.numel() - 1, d_ubuf.numel(), d_uoffsets.device, int(n_scaffolds)
        if out is None:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            out = (z(int(capacity), torch.uint8) if capacity else None, z(ns + 1, torch.int64), z((max(ns, 1), 64), torch.uint8), z((max(nu, 1), 32), torch.uint8),
                   z(int(piece_capacity), torch.int32) if piece_capacity else None)
        par, st, nf, npc = FillParams(int(kinds), 0), FillStats(), C.c_uint64(0), C.c_uint64(0)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        try:
            _chk(self.L.kmx_unitig_scaffold_fill_dev(self.h, int(k), d_ubuf.data_ptr(), d_uoffsets.data_ptr(), nu, nb, ptr(d_srec) if ns else None, ns, ptr(d_steps) if nu else None,
                                                     ptr(d_plinks) if n_plinks else None, int(n_plinks), ptr(d_precs) if n_plinks else None, ptr(d_psteps) if n_psteps else None, int(n_psteps),
                                                     C.byref(par), ptr(out[0]), out[0].numel() if out[0] is not None else 0, out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), ptr(out[4]),
                                                     out[4].numel() if out[4] is not None else 0, C.byref(nf), C.byref(npc), C.byref(st)))
        except KmxError as e:
            e.needed, e.needed_pieces = int(nf.value), int(npc.value)
            e.result = (out, (nf.value, npc.value), st.as_dict())
            raise
        return out, (nf.value, npc.value), st.as_dict()

    def filled_scaffolds_from_pairs(self, k: int, strs, link_offsets: np.ndarray, links: np.ndarray, plinks: np.ndarray, inner: int, min_pairs: int = 2, ratio: int = 0, min_n: int = 10,
                                    max_n: int = 1000, tol=None, max_steps: int = 8, max_visits: int = 4096, kinds: int = 3):
        """on a list of unitig strings, the CSR of their graph and a pair list: unitig_scaffold_flat, unitig_pair_paths_flat at the
        same min_pairs and inner and tol (None: k), then unitig_scaffold_fill_flat -> (the filled scaffold strings as str,
        SCAFFOLD_FILL_DTYPE records, FILL_STEP_DTYPE steps, uint32 pieces, fill stats as a dict, what unitig_scaffold_flat
        returned, what unitig_pair_paths_flat returned)"""
        _, _, ubuf, uoffs = _join_seqs(list(strs))
        scf = self.unitig_scaffold_flat(k, ubuf, uoffs, plinks, inner, min_pairs, ratio, min_n, max_n)
        pth = self.unitig_pair_paths_flat(k, uoffs, link_offsets, links, plinks, inner, int(k) if tol is None else int(tol), min_pairs, max_steps, max_visits)
        fseq, foffs, frec, fst, pcs, st = self.unitig_scaffold_fill_flat(k, ubuf, uoffs, scf[2], scf[3], plinks, pth[0], pth[1], kinds)
        return [b.decode("latin-1") for b in _split_seqs(fseq, foffs)], frec, fst, pcs, st, scf, pth

    def unitig_scaffold_fill_phases(self) -> dict:
        """kmx_unitig_scaffold_fill_last_phases: seconds per phase of the last fill call (under set_profile(1))"""
        sec = (C.c_double * 4)()
        _chk(self.L.kmx_unitig_scaffold_fill_last_phases(self.h, sec))
        return dict(zip(("kinds", "scan", "records", "bytes"), (float(x) for x in sec)))

    def resolved_contigs_from_pairs(self, k: int, ubuf: np.ndarray, uoffsets: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, reads, max_dist: int, tol=None, max_gap=None,
                                    max_indel: int = 1, min_reads: int = 2, max_cross: int = 0, contig_min_reads: int = 1, ratio: int = 0, max_steps: int = 8, max_visits: int = 4096,
                                    pair_paths: bool = True):
        """inside a map session on these unitigs, on interleaved reads: seq_to_walks (the link hits), unitig_through_flat (the
        through hits), unitig_pairs_flat (the list, the pair hits and inner: the floor of the mean d of the SAME pairs with frag >= 0), then
        unitig_pair_paths_flat at min_pairs = min_reads and tol (None: k), whose through and path_hits are added to the walks'
        arrays, unitig_resolve_flat and unitig_contigs_flat on the resolved graph -> (the contig strings as str, the resolve
        stats, the pair path stats or None, the pair path records or None).  pair_paths False: the same chain without the new
        call."""
        link_offsets = np.ascontiguousarray(link_offsets, dtype=np.uint64)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        hits = np.zeros(links.size, dtype=np.uint64)
        walks, wo, steps, _, _, _ = self.seq_to_walks(reads, link_offsets, links, int(k) if max_gap is None else int(max_gap), max_indel, link_hits=hits)
        through, _ = self.unitig_through_flat(walks, steps, link_offsets, links)
        rec, lst, _ = self.unitig_pairs_flat(walks, wo, steps, link_offsets, links, max_dist, pair_hits=hits)
        pst = prec = None
        if pair_paths:
            d = rec["d"][(rec["cls"] == 2) & (rec["frag"] >= 0)]
            inner = int(d.sum()) // d.size if d.size and int(d.sum()) > 0 else 0
            prec, _, pst = self.unitig_pair_paths_flat(k, uoffsets, link_offsets, links, lst, inner, int(k) if tol is None else int(tol), min_reads, max_steps, max_visits, through=through,
                                                       path_hits=hits)
        r = self.unitig_resolve_flat(k, ubuf, uoffsets, link_offsets, links, through, min_reads, max_cross, link_hits=hits)
        c = self.unitig_contigs_flat(k, r[0], r[1], r[5], r[6], r[8], contig_min_reads, ratio)
        return [b.decode("latin-1") for b in _split_seqs(c[0], c[1])], r[9], pst, prec

    # ---- contigs: the unitigs merged along the edges the reads support (the rule: include/kmx.h); no model, no session
    def unitig_contigs_flat(self, k: int, ubuf: np.ndarray, uoffsets: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, link_hits: np.ndarray, min_reads: int = 1, ratio: int = 0,
                            urec=None):
        """kmx_unitig_contigs on what a graph call returned (uint8 bases, uint64 offsets [U + 1], optionally its UNITIG_DTYPE
        records, uint64 link_offsets [2 U + 1], uint32 links) and the uint64 link_hits [n_links] the walks accumulated ->
        (uint8 contig bases, uint64 coffsets [C + 1], CONTIG_DTYPE records [C], uint32 steps [U], CONTIG_PLACE_DTYPE place [U],
        uint64 clink_offsets [2 C + 1], uint32 clinks, uint64 csupport, stats as a dict)."""
        ubuf = np.ascontiguousarray(ubuf, dtype=np.uint8)
        uoffsets = np.ascontiguousarray(uoffsets, dtype=np.uint64)
        link_offsets = np.ascontiguousarray(link_offsets, dtype=np.uint64)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        link_hits = np.ascontiguousarray(link_hits, dtype=np.uint64)
        nu = uoffsets.size - 1
        if link_offsets.size != 2 * nu + 1 or link_hits.size != links.size:
            raise KmxError(-1, "link_offsets holds 2 U + 1 entries and link_hits one per link")
        if urec is not None:
            urec = np.ascontiguousarray(urec, dtype=UNITIG_DTYPE)
            if urec.size != nu:
                raise KmxError(-1, "urec holds one record per unitig")
        cseq = np.zeros(max(ubuf.size, 1), dtype=np.uint8)
        coffs = np.zeros(nu + 1, dtype=np.uint64)
        crec = np.zeros(max(nu, 1), dtype=CONTIG_DTYPE)
        steps = np.zeros(max(nu, 1), dtype=np.uint32)
        place = np.zeros(max(nu, 1), dtype=CONTIG_PLACE_DTYPE)
        cloffs = np.zeros(2 * nu + 1, dtype=np.uint64)
        clinks = np.zeros(max(links.size, 1), dtype=np.uint32)
        csup = np.zeros(max(links.size, 1), dtype=np.uint64)
        par, st = ContigParams(int(min_reads), int(ratio), 0), ContigStats()
        nc, nb, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _chk(self.L.kmx_unitig_contigs(self.h, int(k), ubuf.ctypes.data, uoffsets.ctypes.data, nu, urec.ctypes.data if urec is not None else None, link_offsets.ctypes.data, links.ctypes.data,
                                       links.size, link_hits.ctypes.data, C.byref(par), cseq.ctypes.data, coffs.ctypes.data, crec.ctypes.data, steps.ctypes.data, place.ctypes.data,
                                       cloffs.ctypes.data, clinks.ctypes.data, csup.ctypes.data, C.byref(nc), C.byref(nb), C.byref(nl), C.byref(st)))
        c, b, l = nc.value, nb.value, nl.value
        return cseq[:b].copy(), coffs[:c + 1].copy(), crec[:c].copy(), steps[:nu].copy(), place[:nu].copy(), cloffs[:2 * c + 1].copy(), clinks[:l].copy(), csup[:l].copy(), st.as_dict()

    def unitig_contigs_dev(self, k: int, d_ubuf, d_uoffsets, d_link_offsets, d_links, d_link_hits, min_reads: int = 1, ratio: int = 0, d_urec=None, out=None):
        """kmx_unitig_contigs_dev on torch tensors of the model's device, read where the graph and walk calls left them: d_ubuf
        uint8 [n_ubases], d_uoffsets int64 [U + 1], d_link_offsets int64 [2 U + 1], d_links int32 [n_links], d_link_hits int64
        [n_links], d_urec uint8 [U, 40] or None.  out: the eight output tensors (d_cseq uint8 [n_ubases], d_coffsets int64 [U + 1],
        d_crec uint8 [U, 64], d_steps int32 [U], d_place int32 [U, 2], d_clink_offsets int64 [2 U + 1], d_clinks int32 [n_links],
        d_csupport int64 [n_links]), allocated when None -> (out, (n_contigs, n_cbases, n_clinks), stats as a dict)."""
        import torch
        nu, nb, nl, dev = d_uoffsets.numel() - 1, d_ubuf.numel(), d_links.numel(), d_uoffsets.device
        if out is None:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            out = (z(max(nb, 1), torch.uint8), z(nu + 1, torch.int64), z((max(nu, 1), 64), torch.uint8), z(max(nu, 1), torch.int32), z((max(nu, 1), 2), torch.int32),
                   z(2 * nu + 1, torch.int64), z(max(nl, 1), torch.int32), z(max(nl, 1), torch.int64))
        par, st = ContigParams(int(min_reads), int(ratio), 0), ContigStats()
        nc, ncb, ncl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _chk(self.L.kmx_unitig_contigs_dev(self.h, int(k), d_ubuf.data_ptr(), d_uoffsets.data_ptr(), nu, nb, d_urec.data_ptr() if d_urec is not None else None, d_link_offsets.data_ptr(),
                                           d_links.data_ptr(), nl, d_link_hits.data_ptr(), C.byref(par), *[t.data_ptr() for t in out], C.byref(nc), C.byref(ncb), C.byref(ncl), C.byref(st)))
        return out, (nc.value, ncb.value, ncl.value), st.as_dict()

    def contigs_from_walks(self, k: int, ubuf: np.ndarray, uoffsets: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, reads, max_gap=None, max_indel: int = 1, min_reads: int = 1,
                           ratio: int = 0, urec=None):
        """inside a map session on these unitigs: seq_to_walks on the reads, then unitig_contigs_flat on the link hits they leave
        -> what unitig_contigs_flat returns, with the link hits behind it"""
        hits = np.zeros(np.asarray(links).size, dtype=np.uint64)
        self.seq_to_walks(reads, link_offsets, links, int(k) if max_gap is None else int(max_gap), max_indel, link_hits=hits)
        return self.unitig_contigs_flat(k, ubuf, uoffsets, link_offsets, links, hits, min_reads, ratio, urec) + (hits,)

    def unitig_contigs_phases(self) -> dict:
        """kmx_unitig_contigs_last_phases: seconds per phase of the last contig call (under set_profile(1)) and its doubling rounds"""
        sec, rounds = (C.c_double * 5)(), C.c_uint64(0)
        _chk(self.L.kmx_unitig_contigs_last_phases(self.h, sec, C.byref(rounds)))
        return dict(zip(("support", "ranking", "marks", "records", "bytes"), (float(x) for x in sec)), rounds=int(rounds.value))

    # ---- through hits: the reads per (way in, way out) of every unitig (the rule: include/kmx.h); no model, no session
    def unitig_through_flat(self, walks: np.ndarray, steps: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, through=None):
        """kmx_unitig_walk_through on what unitig_walks_flat returned (WALK_DTYPE walks, uint32 steps) and the CSR those walks were
        made with -> (uint64 through [16 U], stats as a dict).  through (uint64 [16 U], optional) is ADDED to and returned; None: a
        zeroed one."""
        walks = np.ascontiguousarray(walks, dtype=WALK_DTYPE)
        steps = np.ascontiguousarray(steps, dtype=np.uint32)
        link_offsets = np.ascontiguousarray(link_offsets, dtype=np.uint64)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        nu = (link_offsets.size - 1) // 2
        if through is None:
            through = np.zeros(16 * nu, dtype=np.uint64)
        if through.dtype != np.uint64 or not through.flags.c_contiguous or through.size < 16 * nu:
            raise KmxError(-1, "through must be a contiguous uint64 array with 16 entries per unitig")
        st = ThroughStats()
        _chk(self.L.kmx_unitig_walk_through(self.h, walks.ctypes.data, walks.size, steps.ctypes.data, steps.size, link_offsets.ctypes.data, links.ctypes.data, links.size, nu,
                                            through.ctypes.data, C.byref(st)))
        return through, st.as_dict()

    def unitig_through_dev(self, d_walks, n_walks: int, d_steps, n_steps: int, d_link_offsets, d_links, d_through=None):
        """kmx_unitig_walk_through_dev on torch tensors of the model's device, read where unitig_walks_dev and the graph call left
        them: d_walks uint8 [walk_capacity, 80] holding n_walks walks, d_steps int32 [step_capacity] holding n_steps steps,
        d_link_offsets int64 [2 U + 1], d_links int32 [n_links]; d_through int64 [16 U] is ADDED to (None: a zeroed one is
        allocated) -> (d_through, stats as a dict)."""
        import torch
        nu = (d_link_offsets.numel() - 1) // 2
        if d_through is None:
            d_through = torch.zeros(16 * nu, dtype=torch.int64, device=d_link_offsets.device)
        st = ThroughStats()
        _chk(self.L.kmx_unitig_walk_through_dev(self.h, d_walks.data_ptr() if n_walks else None, int(n_walks), d_steps.data_ptr() if n_steps else None, int(n_steps), d_link_offsets.data_ptr(),
                                                d_links.data_ptr(), d_links.numel(), nu, d_through.data_ptr(), C.byref(st)))
        return d_through, st.as_dict()

    def through_from_walks(self, reads, link_offsets: np.ndarray, links: np.ndarray, max_gap: int, max_indel: int = 1, link_hits=None, through=None):
        """inside a map session: seq_to_walks on the reads (link_hits, optional, is added to), then unitig_through_flat on the walks
        they leave -> (through, stats as a dict)"""
        walks, _, steps, _, _, _ = self.seq_to_walks(reads, link_offsets, links, max_gap, max_indel, link_hits=link_hits)
        return self.unitig_through_flat(walks, steps, link_offsets, links, through)

    # ---- resolution: the unitigs whose through hits pair their ways in with their ways out are split (the rule: include/kmx.h)
    def unitig_resolve_flat(self, k: int, ubuf: np.ndarray, uoffsets: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, through: np.ndarray, min_reads: int = 2, max_cross: int = 0,
                            urec=None, link_hits=None, capacity=None):
        """kmx_unitig_resolve on what a graph call returned, the through hits and optionally the records and the link hits ->
        (uint8 bases, uint64 roffsets [U' + 1], UNITIG_DTYPE records [U'] or None, uint32 origin [U'], RESOLVE_PLACE_DTYPE rplace [U],
        uint64 rlink_offsets [2 U' + 1], uint32 rlinks, uint64 link_origin, uint64 rlink_hits or None, stats as a dict).  capacity None:
        a sizing call first; (rec_capacity, seq_capacity): those (KmxError KMX_E_RANGE when short)."""
        ubuf = np.ascontiguousarray(ubuf, dtype=np.uint8)
        uoffsets = np.ascontiguousarray(uoffsets, dtype=np.uint64)
        link_offsets = np.ascontiguousarray(link_offsets, dtype=np.uint64)
        links = np.ascontiguousarray(links, dtype=np.uint32)
        through = np.ascontiguousarray(through, dtype=np.uint64)
        nu, nl = uoffsets.size - 1, links.size
        if link_offsets.size != 2 * nu + 1 or through.size != 16 * nu or (link_hits is not None and np.asarray(link_hits).size != nl):
            raise KmxError(-1, "link_offsets holds 2 U + 1 entries, through 16 per unitig and link_hits one per link")
        if urec is not None:
            urec = np.ascontiguousarray(urec, dtype=UNITIG_DTYPE)
        if link_hits is not None:
            link_hits = np.ascontiguousarray(link_hits, dtype=np.uint64)
        par, st = ResolveParams(int(min_reads), int(max_cross)), ResolveStats()
        n_out, b_out = C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if a is not None else None
        head = (self.h, int(k), ubuf.ctypes.data, uoffsets.ctypes.data, nu, ptr(urec), link_offsets.ctypes.data, links.ctypes.data, nl, ptr(link_hits), through.ctypes.data, C.byref(par))
        if capacity is None:
            _chk(self.L.kmx_unitig_resolve(*head, None, 0, None, 0, None, None, None, None, None, None, None, C.byref(n_out), C.byref(b_out), C.byref(st)))
            capacity = (n_out.value, b_out.value)
        rcap, scap = int(capacity[0]), int(capacity[1])
        rseq = np.zeros(max(scap, 1), dtype=np.uint8)
        roffs = np.zeros(rcap + 1, dtype=np.uint64)
        rrec = np.zeros(max(rcap, 1), dtype=UNITIG_DTYPE) if urec is not None else None
        origin = np.zeros(max(rcap, 1), dtype=np.uint32)
        rplace = np.zeros(max(nu, 1), dtype=RESOLVE_PLACE_DTYPE)
        rloffs = np.zeros(2 * rcap + 1, dtype=np.uint64)
        rlinks = np.zeros(max(nl, 1), dtype=np.uint32)
        lorigin = np.zeros(max(nl, 1), dtype=np.uint64)
        rhits = np.zeros(max(nl, 1), dtype=np.uint64) if link_hits is not None else None
        _chk(self.L.kmx_unitig_resolve(*head, rseq.ctypes.data, scap, roffs.ctypes.data, rcap, ptr(rrec), origin.ctypes.data, rplace.ctypes.data, rloffs.ctypes.data, rlinks.ctypes.data,
                                       lorigin.ctypes.data, ptr(rhits), C.byref(n_out), C.byref(b_out), C.byref(st)))
        n, b = n_out.value, b_out.value
        return (rseq[:b].copy(), roffs[:n + 1].copy(), rrec[:n].copy() if rrec is not None else None, origin[:n].copy(), rplace[:nu].copy(), rloffs[:2 * n + 1].copy(), rlinks[:nl].copy(),
                lorigin[:nl].copy(), rhits[:nl].copy() if rhits is not None else None, st.as_dict())

    def unitig_resolve_dev(self, k: int, d_ubuf, d_uoffsets, d_link_offsets, d_links, d_through, min_reads: int = 2, max_cross: int = 0, d_urec=None, d_link_hits=None, capacity=None, out=None):
        """kmx_unitig_resolve_dev on torch tensors of the model's device: d_ubuf uint8 [n_ubases], d_uoffsets int64 [U + 1],
        d_link_offsets int64 [2 U + 1], d_links int32 [n_links], d_through int64 [16 U], d_urec uint8 [U, 40] or None, d_link_hits int64
        [n_links] or None.  capacity None: a sizing call first; (rec_capacity, seq_capacity): those.  out: the nine output tensors
        (d_rseq uint8, d_roffsets int64 [rec_capacity + 1], d_rrec uint8 [rec_capacity, 40] or None, d_origin int32, d_rplace int32 [U, 2],
        d_rlink_offsets int64 [2 rec_capacity + 1], d_rlinks int32, d_link_origin int64, d_rlink_hits int64 or None), allocated when None
        -> (out, (n_unitigs_out, n_bases_out), stats as a dict); the outputs are complete once the model's stream has drained."""
        import torch
        nu, nb, nl, dev = d_uoffsets.numel() - 1, d_ubuf.numel(), d_links.numel(), d_uoffsets.device
        par, st = ResolveParams(int(min_reads), int(max_cross)), ResolveStats()
        n_out, b_out = C.c_uint64(0), C.c_uint64(0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        head = (self.h, int(k), d_ubuf.data_ptr(), d_uoffsets.data_ptr(), nu, nb, ptr(d_urec), d_link_offsets.data_ptr(), d_links.data_ptr(), nl, ptr(d_link_hits), d_through.data_ptr(), C.byref(par))
        if capacity is None and out is None:
            _chk(self.L.kmx_unitig_resolve_dev(*head, None, 0, None, 0, None, None, None, None, None, None, None, C.byref(n_out), C.byref(b_out), C.byref(st)))
            capacity = (n_out.value, b_out.value)
        if out is None:
            rcap, scap = int(capacity[0]), int(capacity[1])
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            out = (z(max(scap, 1), torch.uint8), z(rcap + 1, torch.int64), z((max(rcap, 1), 40), torch.uint8) if d_urec is not None else None, z(max(rcap, 1), torch.int32),
                   z((max(nu, 1), 2), torch.int32), z(2 * rcap + 1, torch.int64), z(max(nl, 1), torch.int32), z(max(nl, 1), torch.int64), z(max(nl, 1), torch.int64) if d_link_hits is not None else None)
        else:
            rcap, scap = (out[1].numel() - 1, out[0].numel()) if capacity is None else (int(capacity[0]), int(capacity[1]))
        _chk(self.L.kmx_unitig_resolve_dev(*head, out[0].data_ptr(), scap, out[1].data_ptr(), rcap, ptr(out[2]), out[3].data_ptr(), out[4].data_ptr(), out[5].data_ptr(), out[6].data_ptr(),
                                           out[7].data_ptr(), ptr(out[8]), C.byref(n_out), C.byref(b_out), C.byref(st)))
        return out, (n_out.value, b_out.value), st.as_dict()

    def resolved_contigs_from_walks(self, k: int, ubuf: np.ndarray, uoffsets: np.ndarray, link_offsets: np.ndarray, links: np.ndarray, reads, max_gap=None, max_indel: int = 1,
                                    resolve_min_reads: int = 2, max_cross: int = 0, min_reads: int = 1, ratio: int = 0, urec=None):
        """inside a map session on these unitigs: map -> walks with link_hits -> through -> resolve -> contigs on the resolved graph
        -> (what unitig_contigs_flat returns on the resolved graph, what unitig_resolve_flat returned, the through hits)"""
        hits = np.zeros(np.asarray(links).size, dtype=np.uint64)
        through, _ = self.through_from_walks(reads, link_offsets, links, int(k) if max_gap is None else int(max_gap), max_indel, link_hits=hits)
        res = self.unitig_resolve_flat(k, ubuf, uoffsets, link_offsets, links, through, resolve_min_reads, max_cross, urec, hits)
        return self.unitig_contigs_flat(k, res[0], res[1], res[5], res[6], res[8], min_reads, ratio, res[2]), res, through

    def unitig_resolve_phases(self) -> dict:
        """kmx_unitig_resolve_last_phases: seconds per phase of the last resolve call (under set_profile(1))"""
        sec = (C.c_double * 4)()
        _chk(self.L.kmx_unitig_resolve_last_phases(self.h, sec))
        return dict(zip(("verdicts", "records", "links", "bytes"), (float(x) for x in sec)))

    def save(self, save_dir: str) -> None:                    # kmodel.hpp:173
        _chk(self.L.kmx_save(self.h, save_dir.encode()))

    save_model = save                                          # README.md:78

    @classmethod
    def load(cls, save_dir: str) -> "KModel":                  # kmodel.hpp:680-696 + :209
        L = load_library()
        h = C.c_void_p()
        _chk(L.kmx_load(save_dir.encode(), C.byref(h)))
        return cls(_handle=h)

    load_model = load

    # ---- introspection
    def stats(self) -> Stats:
        st = Stats()
        _chk(self.L.kmx_get_stats(self.h, C.byref(st)))
        return st

    def download(self, which: str, index: int = 0) -> np.ndarray:
        st = self.stats()
        cap = max(int(st.km_byte_size), int(st.byte_km_back), max(st.byte_bf), max(st.byte_bf_back), 1)
        buf = np.zeros(cap, dtype=np.uint8)
        w = C.c_uint64(0)
        _chk(self.L.kmx_download(self.h, self.DL[which], index, buf.ctypes.data, cap, C.byref(w)))
        return buf[:w.value].copy()

    KERNEL_CLASSES = ["classify", "check", "commit", "slow_path", "reorder", "rest_table", "query", "detect", "commit_check", "file"]

    def set_profile(self, on) -> None:
        """True / 1: time the kernel classes; 2: the next builds run the fused launches' accounting variant (stats().piped_*)"""
        _chk(self.L.kmx_set_profile(self.h, int(on)))

    def kernel_times(self, reset: bool = True) -> dict:
        sec = (C.c_double * len(self.KERNEL_CLASSES))()
        cnt = (C.c_uint64 * len(self.KERNEL_CLASSES))()
        _chk(self.L.kmx_get_kernel_times(self.h, sec, cnt, int(reset)))
        return {n: {"seconds": sec[i], "launches": int(cnt[i])} for i, n in enumerate(self.KERNEL_CLASSES)}

    def build_seconds(self) -> float:
        a, b = C.c_double(0), C.c_double(0)
        _chk(self.L.kmx_last_build_seconds(self.h, C.byref(a), C.byref(b)))
        return b.value

    def close(self) -> None:
        if getattr(self, "h", None):
            self.L.kmx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


PARTITIONS = {"ring": 0, "range": 1, "range-rccl": 2}                                # KMX_PARTITION_* of include/kmx.h


def init_multi(models, db_file: str, partition: str = "ring") -> None:
    """KModel::init(db_file) (kmodel.hpp:57-86) by several handles together, from inside libkmx.so (kmx_build_from_kmc_multi_ex:
    one host thread per handle).  partition "ring": arrays owned whole, hipMemcpyPeerAsync hand-offs; "range": every array cut
    by position range, the words of a round written into the owners' inboxes through peer mappings, no host wait in a round.
    Every handle ends with the whole model."""
    L = load_library()
    arr = (C.c_void_p * len(models))(*[m.h for m in models])
    _chk(L.kmx_build_from_kmc_multi_ex(arr, len(models), db_file.encode(), PARTITIONS[partition]))


def get_model(ci_or_dir=1, cs: int = 1023, num_hash: int = 7, num_bit: int = 5) -> KModel:
    """Both reference factories (kmodel.hpp:674-677 and :680-696)."""
    if isinstance(ci_or_dir, (str, os.PathLike)):
        return KModel.load(os.fspath(ci_or_dir))
    return KModel(int(ci_or_dir), cs, num_hash, num_bit)
