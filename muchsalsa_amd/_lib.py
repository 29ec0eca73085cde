"""ctypes binding of include/msgpu.h (muchsalsa_amd/libmsgpu.so).

There is no fallback: if the HIP library is missing or no GPU is present the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSGPU_LIB") or os.path.join(_HERE, "libmsgpu.so")  # MSGPU_LIB: another build of the same ABI

ROW_DTYPE = np.dtype([("anchor_id", "<u4"), ("read_id", "<u4"), ("read_len", "<i4"), ("i_lo", "<i4"),
                      ("i_hi", "<i4"), ("n_lo", "<i4"), ("n_hi", "<i4"), ("score", "<u4"), ("line", "<u4"),
                      ("flags", "<u4")])
EDGE_DTYPE = np.dtype([("v1", "<u4"), ("v2", "<u4"), ("em_off", "<u8"), ("order_off", "<u8"), ("em_cnt", "<u4"),
                       ("order_cnt", "<u2"), ("shadow", "u1"), ("pad", "u1")])
EM_DTYPE = np.dtype([("ov_lo", "<i4"), ("ov_hi", "<i4"), ("score", "<f8"), ("anchor_id", "<u4"), ("line", "<u4"),
                     ("flags", "<u4"), ("edge_idx", "<u4")])
ORDER_DTYPE = np.dtype([("edge_idx", "<u4"), ("flags", "<u4"), ("left_offset", "<f8"), ("right_offset", "<f8"),
                        ("score", "<u8"), ("ids_off", "<u8"), ("ids_cnt", "<u4"), ("start", "<u4"), ("end", "<u4"),
                        ("base", "<u4"), ("pad", "<u4", (2,))])
COPY_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("len", "<u4"), ("flags", "<u4")])
assert (ROW_DTYPE.itemsize, EDGE_DTYPE.itemsize, EM_DTYPE.itemsize, ORDER_DTYPE.itemsize) == (40, 32, 32, 64)
assert COPY_DTYPE.itemsize == 24
COPY_ILLUMINA, COPY_REVCOMP = 1, 2
PATH_READ_DTYPE = np.dtype([("read_id", "<u4"), ("direction", "<u4"), ("nanopore_length", "<u8")])
PATH_ORDER_DTYPE = np.dtype([("score", "<u8"), ("base_read", "<u4"), ("ids_off", "<u4"), ("ids_cnt", "<u4"),
                             ("pad", "<u4")])
PATH_EM_DTYPE = np.dtype([("anchor_id", "<u4"), ("ov_lo", "<i4"), ("ov_hi", "<i4")])
PATH_CONTAIN_DTYPE = np.dtype([("host_read", "<u4"), ("nano", "<u4"), ("direction", "<u4"), ("anchors_off", "<u4"),
                               ("anchors_cnt", "<u4")])
PATH_INFO_DTYPE = np.dtype([("target_len", "<u8"), ("target_raw_off", "<u8"), ("query_begin", "<u4"),
                            ("query_end", "<u4"), ("n_anchors", "<u4"), ("n_anchor_edges", "<u4"),
                            ("border_lo", "<i4"), ("border_hi", "<i4"), ("asm_idx", "<i4"), ("pad", "<u4")])
QUERY_INFO_DTYPE = np.dtype([("len", "<u8"), ("raw_off", "<u8"), ("lb", "<i8"), ("rb", "<i8"), ("kind", "<u4"),
                             ("path", "<u4")])
FASTA_RECORD_DTYPE = np.dtype([("raw_off", "<u8"), ("text_off", "<u8"), ("len", "<u4"), ("header_off", "<u4"),
                               ("header_len", "<u4"), ("pad", "<u4")])
assert (PATH_READ_DTYPE.itemsize, PATH_ORDER_DTYPE.itemsize, PATH_EM_DTYPE.itemsize, PATH_CONTAIN_DTYPE.itemsize,
        PATH_INFO_DTYPE.itemsize, QUERY_INFO_DTYPE.itemsize, FASTA_RECORD_DTYPE.itemsize) == (16, 24, 12, 20, 48, 40, 32)
ALIGN_PAIR_DTYPE = np.dtype([("a_off", "<u8"), ("b_off", "<u8"), ("a_len", "<u4"), ("b_len", "<u4")])
assert ALIGN_PAIR_DTYPE.itemsize == 24

OK = 0
E_IO, E_FORMAT, E_NUMBER, E_NOMEM, E_ARG, E_HIP, E_STATE, E_IDS, E_NODEVICE = -1, -2, -3, -4, -5, -6, -7, -8, -9
E_LAYOUT = -10
E_TIMEOUT = -11

ORD_START_V1, ORD_CONTAINED, ORD_DIR, ORD_PRIMARY = 1, 2, 4, 8
BATCH_RESIDENT, BATCH_NO_EDGEMATCHES, BATCH_ROWS_ON_DEVICE, BATCH_ROWS_PACKED = 1, 2, 4, 8


class Params(C.Structure):
    _fields_ = [("min_matches", C.c_uint32), ("th_length", C.c_uint32), ("th_matches", C.c_uint32),
                ("th_overlap", C.c_uint32), ("wiggle_room", C.c_uint64), ("ratio_pct", C.c_double),
                ("alt_frac", C.c_double)]


class PackedRows(C.Structure):  # msgpu_packed_rows: the row table's 28-byte form for the host link
    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_uint64), ("read_len", C.c_void_p), ("n_reads", C.c_uint32),
                ("n_runs", C.c_uint32), ("run_start", C.c_void_p), ("run_delta", C.c_void_p), ("owner", C.c_void_p)]


class HostTables(C.Structure):  # msgpu_host_tables
    _fields_ = [("edges", C.c_void_p), ("ems", C.c_void_p), ("orders", C.c_void_p), ("ids", C.c_void_p),
                ("read_len", C.c_void_p), ("read_first_line", C.c_void_p), ("n_edges", C.c_uint64),
                ("n_ems", C.c_uint64), ("n_orders", C.c_uint64), ("n_ids", C.c_uint64), ("n_reads", C.c_uint32),
                ("n_anchors", C.c_uint32), ("n_batches", C.c_uint32), ("pad", C.c_uint32), ("wall_ms", C.c_float),
                ("load_ms", C.c_float), ("first_batch_ms", C.c_float), ("compute_done_ms", C.c_float)]


class PathInput(C.Structure):
    _fields_ = [("reads", C.c_void_p), ("n_reads", C.c_uint32), ("asm_idx", C.c_int32), ("order_off", C.c_void_p),
                ("orders", C.c_void_p), ("ids", C.c_void_p), ("em_off", C.c_void_p), ("ems", C.c_void_p),
                ("rows", C.c_void_p), ("n_rows", C.c_size_t), ("contains", C.c_void_p), ("n_contains", C.c_uint32),
                ("pad", C.c_uint32), ("contain_anchors", C.c_void_p)]


class GraphStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_vertices_in", "n_edges_in", "n_contraction_edges", "n_deleted_vertices",
                                          "n_contain_elements", "n_decycled_edges", "n_vertices", "n_edges",
                                          "n_components", "n_paths", "n_path_reads")]


class Counts(C.Structure):
    _fields_ = [("n_rows_in", C.c_uint64), ("n_rows_alive", C.c_uint64), ("n_reads", C.c_uint32),
                ("n_anchors", C.c_uint32), ("n_edges", C.c_uint64), ("n_ems", C.c_uint64), ("n_orders", C.c_uint64),
                ("n_ids", C.c_uint64), ("n_pairs_scanned", C.c_uint64), ("n_edges_fastpath", C.c_uint64),
                ("n_lost_publications", C.c_uint64), ("index_path", C.c_uint64)]


class GroupTables(C.Structure):
    _fields_ = [("edges", C.c_void_p), ("orders", C.c_void_p), ("ids", C.c_void_p), ("read_len", C.c_void_p),
                ("read_first_line", C.c_void_p), ("n_edges", C.c_uint64), ("n_orders", C.c_uint64), ("n_ids", C.c_uint64),
                ("n_ems", C.c_uint64), ("n_reads", C.c_uint32), ("n_anchors", C.c_uint32), ("n_members", C.c_uint32),
                ("id_bytes", C.c_uint32), ("slab_bytes", C.c_uint64), ("wall_ms", C.c_float), ("compute_ms", C.c_float),
                ("exchange_ms", C.c_float), ("rows_sliced", C.c_uint32)]


INDEX_BIN, INDEX_ATOMIC, INDEX_TWO_PASS, INDEX_GENERIC = 0, 1, 2, 4


class Timings(C.Structure):
    _fields_ = [("index_ms", C.c_float), ("candidates_ms", C.c_float), ("chain_ms", C.c_float),
                ("compact_ms", C.c_float), ("chain_kernel_ms", C.c_float), ("chain_kernel_launches", C.c_uint32),
                ("pad", C.c_uint32)]


class UfTables(C.Structure):  # msgpu_uf_tables
    _fields_ = [("n_lines", C.c_uint64), ("n_blocks", C.c_uint32), ("n_unitigs", C.c_uint32), ("n_reads", C.c_uint32),
                ("pad", C.c_uint32)] + [(n, C.POINTER(C.c_uint32)) for n in (
                    "line_block", "line_qs", "line_qe", "line_read", "block_first", "block_n", "block_qlen",
                    "block_unitig", "unitig_last_block")]


class UfStats(C.Structure):  # msgpu_uf_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_lines", "n_blocks", "n_ids", "n_outliers", "n_rescued", "n_fragments",
                                           "n_records", "bases", "text_bytes")] +
                [(n, C.c_uint32) for n in ("n_wave", "n_group", "n_giant", "pad")] +
                [(n, C.c_double) for n in ("q1", "q3", "upper")] +
                [(n, C.c_float) for n in ("load_ms", "upload_ms", "pass1_ms", "pass2_ms", "plan_ms", "gather_ms",
                                          "format_ms", "copy_ms", "wall_ms", "pad2")])


UF_PACKED = 1


class ScrubTables(C.Structure):  # msgpu_scrub_tables
    _fields_ = ([(n, C.c_uint64) for n in ("n_anchor_lines", "n_ava_lines", "n_hits", "n_ava")] +
                [(n, C.c_uint32) for n in ("n_nodes", "n_anchors", "n_chunks", "pad")] +
                [("node_length", C.POINTER(C.c_int32)), ("node_line", C.POINTER(C.c_uint32))] +
                [(n, C.POINTER(C.c_uint32)) for n in ("hit_node", "hit_anchor", "hit_line")] +
                [(n, C.POINTER(C.c_int32)) for n in ("hit_s", "hit_e")] +
                [(n, C.POINTER(C.c_uint32)) for n in ("chunk_first", "chunk_n", "ava_a", "ava_b", "ava_strand",
                                                      "ava_line")] +
                [(n, C.POINTER(C.c_int32)) for n in ("ava_sa", "ava_ea", "ava_sb", "ava_eb")])


class ScrubPlanTables(C.Structure):  # msgpu_scrub_plan_tables
    _fields_ = [("n_batches", C.c_uint32), ("pad", C.c_uint32), ("subset_off", C.POINTER(C.c_uint64)),
                ("centre_off", C.POINTER(C.c_uint64)), ("subset", C.POINTER(C.c_uint32)),
                ("centre", C.POINTER(C.c_uint32)), ("start", C.POINTER(C.c_uint32))]


class ScrubStats(C.Structure):  # msgpu_scrub_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_nodes", "n_hits", "n_pairs", "n_edges", "n_ava", "n_batches",
                                           "n_subset_total", "n_intervals", "n_records", "bases", "text_bytes")] +
                [(n, C.c_float) for n in ("load_ms", "graph_ms", "batch_ms", "fold_ms", "union_ms", "plan_ms",
                                          "gather_ms", "format_ms", "copy_ms", "wall_ms")])


SCRUB_SUBSET = 60000


class KfStats(C.Structure):  # msgpu_kf_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_pairs", "n_pairs_out", "n_windows", "n_distinct", "n_candidates",
                                           "n_abundant", "n_hist_rows", "largest_partition")] +
                [("bytes_in", C.c_uint64 * 2), ("bytes_out", C.c_uint64 * 2)] +
                [(n, C.c_int64) for n in ("q1", "q3", "upper")] + [("k", C.c_uint32), ("n_partitions", C.c_uint32)] +
                [(n, C.c_float) for n in ("load_ms", "records_ms", "bins_ms", "extract_ms", "sort_ms", "runs_ms",
                                          "hist_ms", "select_ms", "verdict_ms", "output_ms", "copy_ms", "wall_ms")])


KF_TEXT_OUT_A, KF_TEXT_OUT_B, KF_TEXT_REPORT, KF_TEXT_HISTO, KF_TEXT_KMERS = 0, 1, 2, 3, 4


class UgParams(C.Structure):  # msgpu_ug_params
    _fields_ = [("k", C.c_int32), ("min_count", C.c_uint32), ("trim", C.c_int32), ("min_length", C.c_uint32)]


class UgStats(C.Structure):  # msgpu_ug_stats
    _fields_ = ([("n_records", C.c_uint64 * 2)] +
                [(n, C.c_uint64) for n in ("n_windows", "n_distinct", "n_solid", "n_solid_trimmed", "n_unitigs",
                                           "n_unitigs_kept", "n_cycles", "longest_chain", "largest_partition",
                                           "n_lost_publications")] +
                [("bytes_in", C.c_uint64 * 2), ("bytes_out", C.c_uint64 * 2)] +
                [(n, C.c_uint32) for n in ("k", "min_count", "trim", "min_length", "n_tip_rounds", "doubling_rounds",
                                           "n_partitions", "reserved")] +
                [(n, C.c_float) for n in ("load_ms", "records_ms", "bins_ms", "extract_ms", "sort_ms", "runs_ms", "select_ms",
                                          "adjacency_ms", "tips_ms", "next_ms", "doubling_ms", "order_ms", "write_ms",
                                          "copy_ms", "host_ms", "wall_ms")])


class UgRound(C.Structure):  # msgpu_ug_round
    _fields_ = [("limit", C.c_uint32), ("reserved", C.c_uint32), ("removed", C.c_uint64), ("tips_ms", C.c_float),
                ("adjacency_ms", C.c_float)]


class UgUnitig(C.Structure):  # msgpu_ug_unitig
    _fields_ = [(n, C.c_uint64) for n in ("length", "coverage", "first_hi", "first_lo", "offset")] + [
        ("cyclic", C.c_uint32), ("reserved", C.c_uint32)]


class UgBubbleStats(C.Structure):  # msgpu_ug_bubble_stats
    _fields_ = ([(n, C.c_uint32) for n in ("bubble", "n_phases", "n_rounds", "reserved")] +
                [(n, C.c_uint64) for n in ("n_bubbles", "n_branches_removed", "n_kmers_removed", "max_forks")] +
                [(n, C.c_float) for n in ("forks_ms", "walk_ms", "adjacency_ms", "reserved2")])


class UgBubbleRound(C.Structure):  # msgpu_ug_bubble_round
    _fields_ = ([("after_tip_rounds", C.c_uint32), ("reserved", C.c_uint32)] +
                [(n, C.c_uint64) for n in ("forks", "bubbles", "branches_removed", "removed")] +
                [("forks_ms", C.c_float), ("walk_ms", C.c_float)])


class UgLink(C.Structure):  # msgpu_ug_link
    _fields_ = [("from", C.c_uint32), ("to", C.c_uint32), ("from_rev", C.c_uint8), ("to_rev", C.c_uint8), ("reserved", C.c_uint16)]


class UgGraphStats(C.Structure):  # msgpu_ug_graph_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_links", "n_adjacencies", "n_self_mirror", "n_dead_ends", "gfa_bytes")] +
                [(n, C.c_float) for n in ("links_ms", "sort_ms", "text_ms", "reserved")])


UG_TEXT_ALL, UG_TEXT_CUT, UG_TEXT_GFA = 0, 1, 2


class MapParams(C.Structure):  # msgpu_map_params
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("max_occ", C.c_uint32)] + [
        (n, C.c_int32) for n in ("max_gap", "bandwidth", "max_pred", "min_score", "min_count", "exact", "band", "ava", "cigar")]


class MapChain(C.Structure):  # msgpu_map_chain
    _fields_ = [("query", C.c_uint32), ("target", C.c_uint32), ("strand", C.c_uint32), ("n_anchors", C.c_uint32),
                ("score", C.c_int32)] + [(n, C.c_uint32) for n in ("nm", "q_start", "q_end", "t_start", "t_end", "matches",
                                                                   "block")]


class MapStats(C.Structure):  # msgpu_map_stats
    _fields_ = ([("n_records", C.c_uint64 * 2), ("n_bases", C.c_uint64 * 2), ("n_minimizers", C.c_uint64 * 2)] +
                [(n, C.c_uint64) for n in ("n_keys", "n_index_entries", "n_keys_dropped", "n_entries_dropped", "n_anchors",
                                           "n_groups", "n_groups_kept", "n_groups_small", "n_groups_large", "largest_group",
                                           "n_chains", "n_chains_below_score", "n_chains_below_count", "n_chains_cut", "n_pairs",
                                           "n_pairs_capped", "n_lost_publications", "bytes_out")] +
                [("group_hist", C.c_uint64 * 16), ("params", MapParams)] +
                [(n, C.c_float) for n in ("load_ms", "sketch_ms", "sort_ms", "table_ms", "anchors_ms", "group_ms", "chain_ms",
                                          "backtrack_ms", "pairs_ms", "distance_ms", "copy_ms", "host_ms", "wall_ms")] +
                [("reserved", C.c_uint32)])


class MapIndexStats(C.Structure):  # msgpu_map_istats
    _fields_ = ([(n, C.c_uint64) for n in ("n_records", "n_bases", "n_minimizers", "n_keys", "n_index_entries")] +
                [("k", C.c_int32), ("w", C.c_int32)] +
                [(n, C.c_float) for n in ("load_ms", "sketch_ms", "sort_ms", "table_ms", "wall_ms")] + [("reserved", C.c_uint32)])


class MapAlignStats(C.Structure):  # msgpu_map_astats
    _fields_ = ([(n, C.c_uint64) for n in ("n_pairs_d0", "n_pairs_lds", "n_pairs_slab", "n_pairs_capped", "max_d", "x_columns",
                                           "i_columns", "d_columns", "script_words", "n_runs", "n_inconsistent")] +
                [("slots", C.c_uint32), ("lds_max_d", C.c_uint32), ("align_ms", C.c_float), ("cigar_host_ms", C.c_float)])


class ExtEnd(C.Structure):  # msgpu_ext_end
    _fields_ = [("e", C.c_uint32), ("k", C.c_int32), ("x", C.c_uint32), ("y", C.c_uint32), ("score", C.c_int32), ("rows", C.c_uint32)]


class MapExtStats(C.Structure):  # msgpu_map_xstats
    _fields_ = ([("extend", C.c_uint32), ("reserved", C.c_uint32)] +
                [(n, C.c_uint64) for n in ("n_ends", "n_ends_extended", "n_ends_at_sequence_end", "t_bases", "q_bases", "x_columns",
                                           "i_columns", "d_columns", "max_e", "rows", "n_inconsistent")] +
                [("extend_ms", C.c_float)])


MAP_EXTEND_MAX = 65535   # MSGPU_MAP_EXTEND_MAX
MAP_EXTEND_PENALTY = 8   # MSGPU_MAP_EXTEND_PENALTY
EXT_END_DTYPE = np.dtype([("e", "<u4"), ("k", "<i4"), ("x", "<u4"), ("y", "<u4"), ("score", "<i4"), ("rows", "<u4")])


class MapRank(C.Structure):  # msgpu_map_rank
    _fields_ = [("parent", C.c_uint32), ("sub", C.c_int32), ("n_secondary", C.c_uint32), ("mapq", C.c_uint32)]


class MapRankStats(C.Structure):  # msgpu_map_rstats
    _fields_ = ([("ranking", C.c_uint32), ("lds_primaries", C.c_uint32)] +
                [(n, C.c_uint64) for n in ("n_segments", "n_primaries", "n_secondaries", "n_mapq0", "largest_segment",
                                           "n_segments_single", "n_segments_wave", "n_segments_list", "n_segments_spilled")] +
                [("rank_ms", C.c_float), ("reserved2", C.c_float)])


MAP_RANK_LDS = 512   # MSGPU_MAP_RANK_LDS
MAP_CHAIN_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4"), ("strand", "<u4"), ("n_anchors", "<u4"), ("score", "<i4"), ("nm", "<u4"),
                            ("q_start", "<u4"), ("q_end", "<u4"), ("t_start", "<u4"), ("t_end", "<u4"), ("matches", "<u4"),
                            ("block", "<u4")])
MAP_RANK_DTYPE = np.dtype([("parent", "<u4"), ("sub", "<i4"), ("n_secondary", "<u4"), ("mapq", "<u4")])


class MapMate(C.Structure):  # msgpu_map_mate
    _fields_ = [("mate", C.c_uint32), ("tlen", C.c_uint32), ("cls", C.c_uint32), ("n_best", C.c_uint32)]


class MapMateStats(C.Structure):  # msgpu_map_mstats
    _fields_ = ([("mates", C.c_uint32), ("max_insert", C.c_uint32)] +
                [(n, C.c_uint64) for n in ("n_pairs", "n_proper", "n_ambiguous", "n_discordant", "n_single", "n_unmapped",
                                           "n_pairs_settled", "n_pairs_lanes16", "n_pairs_lanes64", "n_pairs_list", "largest_pair",
                                           "tlen_sum", "tlen_min", "tlen_max")] +
                [("mate_ms", C.c_float), ("reserved2", C.c_float)])


MAP_MATE_DTYPE = np.dtype([("mate", "<u4"), ("tlen", "<u4"), ("cls", "<u4"), ("n_best", "<u4")])
MAP_MATES_ANCHOR_BYTES = 60          # MSGPU_MAP_MATES_ANCHOR_BYTES
MAP_MATES_FIXED_BYTES = 12 * 256     # MSGPU_MAP_MATES_FIXED_BYTES
MAP_MAX_INSERT_DEFAULT = 1000        # MSGPU_MAP_MAX_INSERT_DEFAULT


class MapBatch(C.Structure):  # msgpu_map_batch
    _fields_ = [("first_query", C.c_uint32), ("n_queries", C.c_uint32)] + [
        (n, C.c_uint64) for n in ("n_anchors", "n_query_bases", "n_groups", "n_chains", "n_pairs", "bytes_bound", "bytes_peak")]


class PlParams(C.Structure):  # msgpu_pl_params
    _fields_ = [("min_depth", C.c_int32), ("min_identity", C.c_int32)]


class PlStats(C.Structure):  # msgpu_pl_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_records", "n_bases", "n_reads", "n_read_bases", "n_chains", "n_runs", "n_voters",
                                           "n_ignored", "cols_eq", "cols_x", "cols_d", "cols_i", "pos_verbatim", "pos_unchanged",
                                           "pos_substituted", "pos_deleted", "ins_usable", "ins_unusable", "ins_at_ends",
                                           "ins_applied", "bases_inserted", "max_depth", "n_lost_publications", "bytes_out",
                                           "bytes_peak")] +
                [("params", PlParams)] +
                [(n, C.c_float) for n in ("load_ms", "validate_ms", "offsets_ms", "voters_ms", "pileup_ms", "insertions_ms", "call_ms",
                                          "output_ms", "format_ms", "copy_ms", "wall_ms")] +
                [("reserved", C.c_uint32)])


class PlRecord(C.Structure):  # msgpu_pl_record
    _fields_ = [(n, C.c_uint64) for n in ("len_in", "len_out", "n_substituted", "n_deleted", "n_inserted", "depth_x100")]


class PlVariant(C.Structure):  # msgpu_pl_variant
    _fields_ = [(n, C.c_uint32) for n in ("record", "a", "ref_len", "alt_len", "dp", "ao", "type", "anchor")] + [
        ("offset", C.c_uint64), ("length", C.c_uint64)]


class PlVcfStats(C.Structure):  # msgpu_pl_vcf_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_variants", "n_snp", "n_mnp", "n_ins", "n_del", "n_complex", "n_whole_deleted", "n_short",
                                           "n_long", "ref_bases", "alt_bases", "header_bytes", "text_bytes", "bytes_peak")] +
                [("vcf_ms", C.c_float), ("reserved", C.c_uint32)])


PL_VARIANT_DTYPE = np.dtype([(n, "<u4") for n in ("record", "a", "ref_len", "alt_len", "dp", "ao", "type", "anchor")] +
                            [("offset", "<u8"), ("length", "<u8")])
PL_VCF = 1                   # MSGPU_PL_VCF
VCF_SHORT_BYTES = 512        # MSGPU_VCF_SHORT_BYTES
VCF_LINE_FIXED = 96          # MSGPU_VCF_LINE_FIXED
VCF_TYPES = ("snp", "mnp", "ins", "del", "complex")  # MSGPU_VCF_SNP .. MSGPU_VCF_COMPLEX


class SamParams(C.Structure):  # msgpu_sam_params
    _fields_ = [("eqx", C.c_int32), ("md", C.c_int32), ("unmapped", C.c_int32), ("reserved", C.c_int32)]


class SamLine(C.Structure):  # msgpu_sam_line
    _fields_ = [("chain", C.c_uint32), ("query", C.c_uint32), ("flag", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64)]


SAM_LINE_DTYPE = np.dtype([("chain", "<u4"), ("query", "<u4"), ("flag", "<u4"), ("reserved", "<u4"), ("offset", "<u8")])
SAM_UNMAPPED = 0xffffffff    # MSGPU_SAM_UNMAPPED
SAM_LINE_FIXED = 1024        # MSGPU_SAM_LINE_FIXED
SAM_SHORT_BYTES = 2048       # MSGPU_SAM_SHORT_BYTES


class SamBatch(C.Structure):  # msgpu_sam_batch
    _fields_ = [("first_query", C.c_uint32), ("n_queries", C.c_uint32)] + [
        (n, C.c_uint64) for n in ("n_lines", "text_bound", "n_short", "n_long", "text_bytes", "bytes_bound", "bytes_peak")]


class SamStats(C.Structure):  # msgpu_sam_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_targets", "n_queries", "n_chains", "n_runs", "n_lines", "n_representative",
                                           "n_supplementary", "n_secondary", "n_unmapped", "n_short", "n_long", "n_batches",
                                           "budget_bytes", "header_bytes", "bytes_out", "bytes_peak", "n_lost_publications")] +
                [("params", SamParams)] +
                [(n, C.c_float) for n in ("load_ms", "validate_ms", "scan_ms", "roles_ms", "format_ms", "copy_ms", "wall_ms")] +
                [("reserved", C.c_uint32)])


class EvParams(C.Structure):  # msgpu_ev_params
    _fields_ = [("k", C.c_int32), ("min_count", C.c_uint32), ("intervals", C.c_uint32), ("reserved", C.c_uint32)]


class EvTableStats(C.Structure):  # msgpu_ev_tstats
    _fields_ = ([("n_records", C.c_uint64 * 2), ("bytes_in", C.c_uint64 * 2)] +
                [(n, C.c_uint64) for n in ("n_windows", "n_distinct", "largest_partition", "bytes_resident")] +
                [("k", C.c_uint32), ("n_partitions", C.c_uint32)] +
                [(n, C.c_float) for n in ("load_ms", "records_ms", "bins_ms", "extract_ms", "sort_ms", "runs_ms", "select_ms",
                                          "table_ms", "wall_ms")] + [("reserved", C.c_uint32)])


class EvRecord(C.Structure):  # msgpu_ev_record
    _fields_ = [(n, C.c_uint64) for n in ("length", "windows", "missing")]


class EvInterval(C.Structure):  # msgpu_ev_interval
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("record", C.c_uint32), ("reserved", C.c_uint32)]


class EvStats(C.Structure):  # msgpu_ev_stats
    _fields_ = ([(n, C.c_uint64) for n in ("n_records", "n_bases", "n_windows", "n_missing", "n_missing_distinct", "n_intervals",
                                           "solid", "found", "n_lost_publications", "bytes_peak")] +
                [("k", C.c_uint32), ("min_count", C.c_uint32)] +
                [(n, C.c_float) for n in ("load_ms", "window_ms", "reduce_ms", "missing_ms", "spectrum_ms", "intervals_ms", "copy_ms",
                                          "host_ms", "wall_ms")] + [("reserved", C.c_uint32)])


EV_CLASSES, EV_ROWS = 5, 10002  # MSGPU_EV_CLASSES, MSGPU_EV_ROWS
EV_TEXT_HEAD, EV_TEXT_REPORT, EV_TEXT_SPECTRUM, EV_TEXT_BED = 0, 1, 2, 3


# every symbol include/msgpu.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("msgpu_default_params", None, [C.POINTER(Params)]),
    ("msgpu_strerror", C.c_char_p, [C.c_int]),
    ("msgpu_create", C.c_int, [C.c_int, C.POINTER(Params), C.POINTER(C.c_void_p)]),
    ("msgpu_destroy", None, [C.c_void_p]),
    ("msgpu_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("msgpu_get_stream", C.c_void_p, [C.c_void_p]),
    ("msgpu_stream_wait", C.c_int, [C.c_void_p, C.c_void_p]),
    ("msgpu_stream_release", C.c_int, [C.c_void_p, C.c_void_p]),
    ("msgpu_set_shard", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    ("msgpu_set_id_space", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    ("msgpu_parse_paf", C.c_int, [C.c_char_p, C.POINTER(Params), C.POINTER(C.c_void_p)]),
    ("msgpu_paf_free", None, [C.c_void_p]),
    ("msgpu_paf_rows", C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    ("msgpu_paf_line_count", C.c_size_t, [C.c_void_p]),
    ("msgpu_paf_read_count", C.c_uint32, [C.c_void_p]),
    ("msgpu_paf_anchor_count", C.c_uint32, [C.c_void_p]),
    ("msgpu_paf_read_name", C.c_char_p, [C.c_void_p, C.c_uint32]),
    ("msgpu_paf_anchor_name", C.c_char_p, [C.c_void_p, C.c_uint32]),
    ("msgpu_paf_register_sequences", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("msgpu_load_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("msgpu_load_rows_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("msgpu_calculate_edges", C.c_int, [C.c_void_p]),
    ("msgpu_chaining_and_overlaps", C.c_int, [C.c_void_p]),
    ("msgpu_get_counts", C.c_int, [C.c_void_p, C.POINTER(Counts)]),
    ("msgpu_get_timings", C.c_int, [C.c_void_p, C.POINTER(Timings)]),
    ("msgpu_get_chain_band_counts", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("msgpu_chain_band_width", C.c_int, []),
    ("msgpu_cand_wide", C.c_int, [C.c_uint32]),
    ("msgpu_order_finish", C.c_int, [C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32,
                                     C.c_uint32, C.c_void_p]),
    ("msgpu_set_stage_events", C.c_int, [C.c_void_p, C.c_int]),
    ("msgpu_copy_tables", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("msgpu_copy_tables_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("msgpu_copy_reads", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("msgpu_merge_gathered", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                       C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("msgpu_merge_gathered_ex", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                          C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    ("msgpu_wire_edges_bytes", C.c_uint64, [C.c_uint64]),
    ("msgpu_wire_orders_bytes", C.c_uint64, [C.c_uint64]),
    ("msgpu_wire_ids_bytes", C.c_uint64, [C.c_uint64, C.c_uint32]),
    ("msgpu_pack_wire", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("msgpu_merge_wire", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("msgpu_chain_launches", C.c_uint64, [C.c_void_p]),
    ("msgpu_wait_chain_launch", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32]),
    ("msgpu_unpack_wire_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("msgpu_find_contraction_edges", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                               C.c_void_p]),
    ("msgpu_pack_rows", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(PackedRows)]),
    ("msgpu_packed_rows_free", None, [C.POINTER(PackedRows)]),
    ("msgpu_load_rows_packed", C.c_int, [C.c_void_p, C.POINTER(PackedRows)]),
    ("msgpu_synchronize", C.c_int, [C.c_void_p]),
    ("msgpu_set_deadline", C.c_int, [C.c_void_p, C.c_uint32]),
    ("msgpu_debug_buffers", C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("msgpu_seq_parse", C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_seq_free", None, [C.c_void_p]),
    ("msgpu_seq_count", C.c_uint32, [C.c_void_p]),
    ("msgpu_seq_name", C.c_char_p, [C.c_void_p, C.c_uint32]),
    ("msgpu_seq_length", C.c_uint64, [C.c_void_p, C.c_uint32]),
    ("msgpu_seq_bases", C.c_void_p, [C.c_void_p, C.c_uint32]),
    ("msgpu_seq_buffer", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_str_slice", C.c_uint64, [C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]),
    ("msgpu_seq_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_seq_destroy", None, [C.c_void_p]),
    ("msgpu_seq_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_seq_upload", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("msgpu_seq_upload_device", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_uint32]),
    ("msgpu_seq_pack", C.c_int, [C.c_void_p]),
    ("msgpu_seq_pack_store", C.c_int, [C.c_void_p, C.c_int]),
    ("msgpu_seq_upload_bases", C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    ("msgpu_seq_parse_upload", C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_seq_offset", C.c_uint64, [C.c_void_p, C.c_uint32]),
    ("msgpu_seq_set_ids", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("msgpu_seq_resolve", C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_int32, C.c_int32, C.c_int, C.c_void_p]),
    ("msgpu_seg_anchor", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p,
                                   C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("msgpu_seg_left_of_anchor", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int,
                                           C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("msgpu_seg_right_of_anchor", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int,
                                            C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("msgpu_seg_between_anchors", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int, C.c_void_p, C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    ("msgpu_consensus_new", C.c_void_p, []),
    ("msgpu_consensus_free", None, [C.c_void_p]),
    ("msgpu_consensus_update", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32]),
    ("msgpu_consensus_borders", C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_uint64)]),
    ("msgpu_consensus_pieces", C.c_size_t, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t]),
    ("msgpu_consensus_clone", C.c_void_p, [C.c_void_p]),
    ("msgpu_assembly_create", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("msgpu_assembly_free", None, [C.c_void_p]),
    ("msgpu_assembly_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_assembly_set_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("msgpu_assembly_borrow_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("msgpu_assembly_add_path", C.c_int, [C.c_void_p, C.POINTER(PathInput)]),
    ("msgpu_assembly_add_paths", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    ("msgpu_assembly_add_graph_paths", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("msgpu_assembly_path_count", C.c_uint32, [C.c_void_p]),
    ("msgpu_assembly_query_count", C.c_uint32, [C.c_void_p]),
    ("msgpu_assembly_path_info", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("msgpu_assembly_query_info", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("msgpu_assembly_pieces", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("msgpu_assembly_raw_bytes", C.c_uint64, [C.c_void_p]),
    ("msgpu_assembly_finish", C.c_int, [C.c_void_p, C.c_void_p]),
    ("msgpu_assembly_validate", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_assembly_text", C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    ("msgpu_fasta_text_bytes", C.c_uint64, [C.c_uint32, C.c_uint64]),
    ("msgpu_fasta_format", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                     C.c_void_p, C.c_uint64, C.c_void_p]),
    ("msgpu_graph_create", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("msgpu_graph_create_borrowed", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                              C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.POINTER(C.c_void_p)]),
    ("msgpu_graph_path_edges", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("msgpu_graph_set_path_edgematches", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("msgpu_graph_free", None, [C.c_void_p]),
    ("msgpu_graph_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_graph_clean_up", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("msgpu_graph_set_threads", C.c_int, [C.c_void_p, C.c_uint32]),
    ("msgpu_graph_linearize", C.c_int, [C.c_void_p]),
    ("msgpu_graph_get_stats", C.c_int, [C.c_void_p, C.POINTER(GraphStats)]),
    ("msgpu_graph_path_count", C.c_uint32, [C.c_void_p]),
    ("msgpu_graph_path_input", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(PathInput)]),
    ("msgpu_graph_state", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("msgpu_graph_max_span_tree", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.c_void_p]),
    ("msgpu_graph_bookkeeping", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("msgpu_graph_connected_components", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                   C.c_void_p, C.POINTER(C.c_uint32)]),
    ("msgpu_graph_shortest_path", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("msgpu_graph_sort_topologically", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.POINTER(C.c_uint32)]),
    ("msgpu_group_create", C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(Params), C.POINTER(C.c_void_p)]),
    ("msgpu_group_destroy", None, [C.c_void_p]),
    ("msgpu_group_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_group_size", C.c_int, [C.c_void_p]),
    ("msgpu_group_ctx", C.c_void_p, [C.c_void_p, C.c_int]),
    ("msgpu_group_overlap", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(GroupTables)]),
    ("msgpu_group_set_timeout", C.c_int, [C.c_void_p, C.c_uint32]),
    ("msgpu_group_device_tables", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p)]),
    ("msgpu_overlap_batched", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(HostTables)]),
    ("msgpu_overlap_batched_ex", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                           C.POINTER(HostTables)]),
    ("msgpu_get_edgematches", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("msgpu_pinned_alloc", C.c_void_p, [C.c_size_t]),
    ("msgpu_pinned_free", None, [C.c_void_p]),
    ("msgpu_index_lines", C.c_int, [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("msgpu_registry_new", C.c_void_p, []),
    ("msgpu_registry_free", None, [C.c_void_p]),
    ("msgpu_registry_id", C.c_uint32, [C.c_void_p, C.c_char_p]),
    ("msgpu_registry_size", C.c_uint32, [C.c_void_p]),
    ("msgpu_registry_clear", None, [C.c_void_p]),
    ("msgpu_toggle_mul", C.c_int, [C.c_int, C.c_int]),
    ("msgpu_gather_plan_create", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("msgpu_gather_plan_free", None, [C.c_void_p]),
    ("msgpu_uf_parse", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    ("msgpu_uf_free", None, [C.c_void_p]),
    ("msgpu_uf_get_tables", C.c_int, [C.c_void_p, C.POINTER(UfTables)]),
    ("msgpu_uf_unitig_name", C.c_char_p, [C.c_void_p, C.c_uint32]),
    ("msgpu_uf_read_name", C.c_char_p, [C.c_void_p, C.c_uint32]),
    ("msgpu_uf_unitig_id", C.c_uint32, [C.c_void_p, C.c_char_p]),
    ("msgpu_uf_quartiles", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double)]),
    ("msgpu_uf_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_uf_destroy", None, [C.c_void_p]),
    ("msgpu_uf_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_uf_error_line", C.c_uint64, [C.c_void_p]),
    ("msgpu_uf_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("msgpu_uf_result_stats", C.c_int, [C.c_void_p, C.POINTER(UfStats)]),
    ("msgpu_uf_result_text", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_uf_result_free", None, [C.c_void_p]),
    ("msgpu_scrub_parse", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_int)]),
    ("msgpu_scrub_free", None, [C.c_void_p]),
    ("msgpu_scrub_get_tables", C.c_int, [C.c_void_p, C.POINTER(ScrubTables)]),
    ("msgpu_scrub_node_name", C.c_char_p, [C.c_void_p, C.c_uint32]),
    ("msgpu_scrub_node_id", C.c_uint32, [C.c_void_p, C.c_char_p]),
    ("msgpu_scrub_name_order", C.c_int, [C.c_void_p, C.c_void_p]),
    ("msgpu_scrub_plan_create", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]),
    ("msgpu_scrub_plan_get", C.c_int, [C.c_void_p, C.POINTER(ScrubPlanTables)]),
    ("msgpu_scrub_plan_free", None, [C.c_void_p]),
    ("msgpu_scrub_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_scrub_destroy", None, [C.c_void_p]),
    ("msgpu_scrub_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_scrub_error_line", C.c_uint64, [C.c_void_p]),
    ("msgpu_scrub_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("msgpu_scrub_result_stats", C.c_int, [C.c_void_p, C.POINTER(ScrubStats)]),
    ("msgpu_scrub_result_text", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_scrub_result_graph", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)),
                                           C.POINTER(C.POINTER(C.c_uint32))]),
    ("msgpu_scrub_result_free", None, [C.c_void_p]),
    ("msgpu_kf_threshold", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64)]),
    ("msgpu_kf_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_kf_destroy", None, [C.c_void_p]),
    ("msgpu_kf_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_kf_error_line", C.c_uint64, [C.c_void_p]),
    ("msgpu_kf_error_file", C.c_int, [C.c_void_p]),
    ("msgpu_kf_run", C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint64,
                               C.POINTER(C.c_void_p)]),
    ("msgpu_kf_open_pair", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    ("msgpu_pair_close", None, [C.c_void_p]),
    ("msgpu_kf_run_pair", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("msgpu_kf_result_stats", C.c_int, [C.c_void_p, C.POINTER(KfStats)]),
    ("msgpu_kf_result_histogram", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)),
                                            C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]),
    ("msgpu_kf_result_abundant", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint64)),
                                           C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint64)]),
    ("msgpu_kf_result_verdicts", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]),
    ("msgpu_kf_result_text", C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    ("msgpu_kf_result_free", None, [C.c_void_p]),
    ("msgpu_ug_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_ug_destroy", None, [C.c_void_p]),
    ("msgpu_ug_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_ug_error_line", C.c_uint64, [C.c_void_p]),
    ("msgpu_ug_error_file", C.c_int, [C.c_void_p]),
    ("msgpu_ug_run", C.c_int, [C.c_void_p, C.POINTER(UgParams), C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint64,
                               C.POINTER(C.c_void_p)]),
    ("msgpu_ug_run_pair", C.c_int, [C.c_void_p, C.POINTER(UgParams), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64,
                                    C.POINTER(C.c_void_p)]),
    ("msgpu_ug_result_stats", C.c_int, [C.c_void_p, C.POINTER(UgStats)]),
    ("msgpu_ug_result_rounds", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(UgRound)), C.POINTER(C.c_uint64)]),
    ("msgpu_ug_result_unitigs", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(UgUnitig)), C.POINTER(C.c_uint64)]),
    ("msgpu_ug_set_bubbles", C.c_int, [C.c_void_p, C.c_uint32]),
    ("msgpu_ug_result_bubbles", C.c_int, [C.c_void_p, C.POINTER(UgBubbleStats), C.POINTER(C.POINTER(UgBubbleRound)),
                                          C.POINTER(C.c_uint64)]),
    ("msgpu_ug_set_graph", C.c_int, [C.c_void_p, C.c_int]),
    ("msgpu_ug_set_wide", C.c_int, [C.c_void_p, C.c_int]),
    ("msgpu_ug_result_peak_bytes", C.c_uint64, [C.c_void_p]),
    ("msgpu_ug_result_first_kmers", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_uint64)]),
    ("msgpu_ug_result_links", C.c_int, [C.c_void_p, C.POINTER(UgGraphStats), C.POINTER(C.POINTER(UgLink)), C.POINTER(C.c_uint64)]),
    ("msgpu_ug_result_text", C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    ("msgpu_ug_result_free", None, [C.c_void_p]),
    ("msgpu_map_default_params", None, [C.POINTER(MapParams)]),
    ("msgpu_map_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_map_destroy", None, [C.c_void_p]),
    ("msgpu_map_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_map_run", C.c_int, [C.c_void_p, C.POINTER(MapParams), C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint64,
                                C.POINTER(C.c_void_p)]),
    ("msgpu_map_index_create", C.c_int, [C.c_void_p, C.POINTER(MapParams), C.c_char_p, C.POINTER(C.c_void_p)]),
    ("msgpu_map_index_free", None, [C.c_void_p]),
    ("msgpu_map_index_stats", C.c_int, [C.c_void_p, C.POINTER(MapIndexStats)]),
    ("msgpu_map_run_index", C.c_int, [C.c_void_p, C.POINTER(MapParams), C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint64,
                                      C.POINTER(C.c_void_p)]),
    ("msgpu_map_result_stats", C.c_int, [C.c_void_p, C.POINTER(MapStats)]),
    ("msgpu_map_result_chains", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(MapChain)), C.POINTER(C.c_uint64)]),
    ("msgpu_map_result_batches", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(MapBatch)), C.POINTER(C.c_uint64)]),
    ("msgpu_map_result_budget", C.c_uint64, [C.c_void_p]),
    ("msgpu_map_batch_bytes", C.c_uint64, [C.POINTER(MapParams), C.c_uint64, C.c_uint64]),
    ("msgpu_map_result_text", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_map_result_cigars", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint64)),
                                          C.POINTER(C.c_uint64)]),
    ("msgpu_map_result_align_stats", C.c_int, [C.c_void_p, C.POINTER(MapAlignStats)]),
    ("msgpu_map_set_extension", C.c_int, [C.c_void_p, C.c_uint32]),
    ("msgpu_map_result_ext_stats", C.c_int, [C.c_void_p, C.POINTER(MapExtStats)]),
    ("msgpu_map_result_ext_ends", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(ExtEnd)), C.POINTER(C.c_uint64)]),
    ("msgpu_map_batch_bytes_ext", C.c_uint64, [C.POINTER(MapParams), C.c_uint32, C.c_uint64, C.c_uint64]),
    ("msgpu_map_set_ranking", C.c_int, [C.c_void_p, C.c_int]),
    ("msgpu_map_result_ranks", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(MapRank)), C.POINTER(C.c_uint64)]),
    ("msgpu_map_result_rank_stats", C.c_int, [C.c_void_p, C.POINTER(MapRankStats)]),
    ("msgpu_map_batch_bytes_rank", C.c_uint64, [C.POINTER(MapParams), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]),
    ("msgpu_map_rank_tables", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("msgpu_map_rank_tables_stats", C.c_int, [C.c_void_p, C.POINTER(MapRankStats)]),
    ("msgpu_map_set_mates", C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    ("msgpu_map_result_mates", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(MapMate)), C.POINTER(C.c_uint64)]),
    ("msgpu_map_result_mate_stats", C.c_int, [C.c_void_p, C.POINTER(MapMateStats)]),
    ("msgpu_map_batch_bytes_mates", C.c_uint64, [C.POINTER(MapParams), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]),
    ("msgpu_map_mate_tables", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("msgpu_map_mate_tables_stats", C.c_int, [C.c_void_p, C.POINTER(MapMateStats)]),
    ("msgpu_map_result_free", None, [C.c_void_p]),
    ("msgpu_pl_default_params", None, [C.POINTER(PlParams)]),
    ("msgpu_pl_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_pl_destroy", None, [C.c_void_p]),
    ("msgpu_pl_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_pl_run", C.c_int, [C.c_void_p, C.POINTER(PlParams), C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p,
                               C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("msgpu_pl_run_mates", C.c_int, [C.c_void_p, C.POINTER(PlParams), C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("msgpu_pl_run_ranked", C.c_int, [C.c_void_p, C.POINTER(PlParams), C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("msgpu_pl_result_text", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_pl_result_stats", C.c_int, [C.c_void_p, C.POINTER(PlStats)]),
    ("msgpu_pl_result_records", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(PlRecord)), C.POINTER(C.c_uint64)]),
    ("msgpu_pl_result_vcf", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_pl_result_variants", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(PlVariant)), C.POINTER(C.c_uint64)]),
    ("msgpu_pl_result_vcf_stats", C.c_int, [C.c_void_p, C.POINTER(PlVcfStats)]),
    ("msgpu_pl_result_free", None, [C.c_void_p]),
    ("msgpu_sam_default_params", None, [C.POINTER(SamParams)]),
    ("msgpu_sam_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_sam_destroy", None, [C.c_void_p]),
    ("msgpu_sam_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_sam_batch_bytes", C.c_uint64, [C.POINTER(SamParams), C.c_uint64, C.c_uint64]),
    ("msgpu_sam_run", C.c_int, [C.c_void_p, C.POINTER(SamParams), C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("msgpu_sam_result_text", C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("msgpu_sam_result_stats", C.c_int, [C.c_void_p, C.POINTER(SamStats)]),
    ("msgpu_sam_result_lines", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SamLine)), C.POINTER(C.c_uint64)]),
    ("msgpu_sam_result_batches", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SamBatch)), C.POINTER(C.c_uint64)]),
    ("msgpu_sam_result_free", None, [C.c_void_p]),
    ("msgpu_ev_default_params", None, [C.POINTER(EvParams)]),
    ("msgpu_ev_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("msgpu_ev_destroy", None, [C.c_void_p]),
    ("msgpu_ev_last_error", C.c_char_p, [C.c_void_p]),
    ("msgpu_ev_error_line", C.c_uint64, [C.c_void_p]),
    ("msgpu_ev_error_file", C.c_int, [C.c_void_p]),
    ("msgpu_ev_qv", C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
    ("msgpu_ev_table_open", C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("msgpu_ev_table_open_pair", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("msgpu_ev_table_stats", C.c_int, [C.c_void_p, C.POINTER(EvTableStats)]),
    ("msgpu_ev_table_free", None, [C.c_void_p]),
    ("msgpu_ev_run_table", C.c_int, [C.c_void_p, C.POINTER(EvParams), C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("msgpu_ev_run", C.c_int, [C.c_void_p, C.POINTER(EvParams), C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint64,
                               C.POINTER(C.c_void_p)]),
    ("msgpu_ev_result_stats", C.c_int, [C.c_void_p, C.POINTER(EvStats)]),
    ("msgpu_ev_result_records", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(EvRecord)), C.POINTER(C.POINTER(EvRecord)),
                                          C.POINTER(C.c_uint64)]),
    ("msgpu_ev_result_spectrum", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64))]),
    ("msgpu_ev_result_intervals", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(EvInterval)), C.POINTER(C.c_uint64)]),
    ("msgpu_ev_result_text", C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    ("msgpu_ev_result_free", None, [C.c_void_p]),
    ("msgpu_gather_plan_out_bytes", C.c_uint64, [C.c_void_p]),
    ("msgpu_gather_plan_bases", C.c_uint64, [C.c_void_p]),
    ("msgpu_gather_run", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("msgpu_seq_synchronize", C.c_int, [C.c_void_p]),
    ("msgpu_edit_distance", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                      C.c_void_p]),
    ("msgpu_edit_script", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("msgpu_extend_ends", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
]

_lib = None
PRELOAD_TORCH = True  # the command-line driver turns this off: it never imports torch, so there is nothing to reconcile


def lib():
    """Load libmsgpu.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "muchsalsa_amd/libmsgpu.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C muchsalsa_amd/csrc`). There is no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own HIP/HSA runtime.  Two HIP runtimes in one process do not share the
        # device: whichever is initialised second sees "no GPU".  Importing torch first (when it is installed) makes
        # libmsgpu's libamdhip64.so.7 dependency resolve to the copy torch already loaded, so load order stops mattering.
        import sys
        if PRELOAD_TORCH or "torch" in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        handle = C.CDLL(LIB_PATH)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(handle, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib
