"""ctypes binding of libhylight_mi.so (include/hylight_mi.h) - the product's only route to the
hot path.  There is no CPU fallback: a missing library or a missing GPU raises."""
from __future__ import annotations

import ctypes as C
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhylight_mi.so")


class HlmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libhylight_mi error {code}: {msg}")
        self.code = code


class AvaOpts(C.Structure):
    _fields_ = [("k", C.c_int), ("w", C.c_int), ("hpc", C.c_int), ("min_chain_score", C.c_int),
                ("max_gap", C.c_int), ("bandwidth", C.c_int), ("min_cnt", C.c_int),
                ("min_mid_occ", C.c_int), ("mid_occ_frac", C.c_double),
                ("match", C.c_int), ("mismatch", C.c_int), ("gap_open", C.c_int), ("gap_ext", C.c_int),
                ("ambi", C.c_int), ("min_dp_score", C.c_int), ("end_bonus", C.c_int), ("pair_once", C.c_int),
                ("gap_open2", C.c_int), ("gap_ext2", C.c_int), ("stub_oh", C.c_int), ("zdrop", C.c_int)]


class VqOverlap(C.Structure):
    _fields_ = [("id1", C.c_uint64), ("id2", C.c_uint64), ("pos1", C.c_uint32), ("pos2", C.c_uint32),
                ("perc1", C.c_uint32), ("perc2", C.c_uint32), ("len1", C.c_uint32), ("len2", C.c_uint32),
                ("ord", C.c_char), ("ori1", C.c_char), ("ori2", C.c_char), ("type1", C.c_char), ("type2", C.c_char),
                ("pad", C.c_char * 3)]


class VqGraphOpts(C.Structure):
    _fields_ = [("min_overlap_len", C.c_uint32), ("min_overlap_perc", C.c_uint32), ("min_read_len", C.c_uint32),
                ("max_tip_len", C.c_uint32), ("remove_trans", C.c_uint32), ("edge_threshold", C.c_double),
                ("ov_threshold", C.c_double), ("merge_contigs", C.c_double), ("mismatch", C.c_double),
                ("ignore_inclusions", C.c_int), ("remove_tips", C.c_int), ("remove_branches", C.c_int),
                ("remove_backedges", C.c_int), ("max_overlaps", C.c_uint64)]


VQ_GRAPH_STATS = ("vertices", "candidates", "duplicates", "inclusions", "edges_built", "conflicts", "moved", "transitive",
                  "tip_edges", "tip_reads", "branch_edges", "backedges", "edges_final")


class VqGraphStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VQ_GRAPH_STATS]


class VqMergeOpts(C.Structure):
    _fields_ = [("first_it", C.c_int), ("keep_singletons", C.c_uint32), ("store_tips_separately", C.c_int),
                ("min_clique_size", C.c_uint32)]


VQ_MERGE_STATS = ("pairs", "merged", "dropped_empty", "dropped_n", "trivial", "trivial_reverse", "short_reads", "n_reads",
                  "inclusion_reads", "tip_reads", "bases_in", "bytes_out")
VQ_MERGE_MS = ("ms_merge",)


class VqMergeStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VQ_MERGE_STATS] + [(k, C.c_double) for k in VQ_MERGE_MS]


class VqCliqueOpts(C.Structure):
    _fields_ = [("min_clique_size", C.c_uint32), ("error_correction", C.c_int), ("first_it", C.c_int),
                ("keep_singletons", C.c_uint32)]


VQ_CLIQUE_STATS = ("cliques_read", "singletons", "below_min", "taken", "filtered", "superreads", "dropped_empty", "dropped_n",
                   "dropped_support", "trivial", "trivial_reverse", "short_reads", "n_reads", "columns", "columns_host",
                   "bases_in", "bytes_out")
VQ_CLIQUE_MS = ("ms_cliques",)


class VqCliqueStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VQ_CLIQUE_STATS] + [(k, C.c_double) for k in VQ_CLIQUE_MS]


class VqNextOpts(C.Structure):
    _fields_ = [("no_inclusion_overlaps", C.c_int)]


VQ_NEXT_STATS = ("src_graph", "src_branching", "src_nonedge", "nonedge_skipped", "src_induced", "copied", "u2sr", "v2sr", "sr2sr",
                 "claims_failed", "lines")
VQ_NEXT_MS = ("ms_next",)


class VqNextStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VQ_NEXT_STATS] + [(k, C.c_double) for k in VQ_NEXT_MS]


VQ_CLIQUE_NEXT_STATS = VQ_NEXT_STATS + ("candidates", "max_list", "in_several")


class VqCliqueNextStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VQ_CLIQUE_NEXT_STATS] + [(k, C.c_double) for k in VQ_NEXT_MS]


class VqBranchOpts(C.Structure):
    _fields_ = [("se_count", C.c_uint32), ("pe_count", C.c_uint32), ("careful", C.c_int)]


VQ_BRANCH_STATS = ("in_branches", "out_branches", "pairs", "diff_positions", "work_items", "evidence_ids", "missing_edges",
                   "false_branches", "inclusion_pairs", "components", "components_kept", "dist_too_large", "scheduled", "edges_removed")
VQ_BRANCH_MS = ("ms_diff", "ms_evidence", "ms_branch")


class VqBranchStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VQ_BRANCH_STATS] + [(k, C.c_double) for k in VQ_BRANCH_MS]


class ClusterOpts(C.Structure):
    _fields_ = [("size", C.c_int64), ("threads", C.c_int32), ("pad", C.c_int32), ("window_bytes", C.c_uint64)]


CLUSTER_STATS = ("names", "rows", "chunks", "sessions", "windows", "survivors", "strict_rejects", "unions", "clusters_ge20",
                 "reads_sliced", "files")
CLUSTER_MS = ("ms_fastq", "ms_paf", "ms_prefilter", "ms_union", "ms_refresh", "ms_group", "ms_demux", "ms_write", "ms_total")


class ClusterStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in CLUSTER_STATS] + [(k, C.c_double) for k in CLUSTER_MS]


class PolishOpts(C.Structure):
    _fields_ = [("min_len", C.c_int), ("min_iden", C.c_double), ("min_cov", C.c_int), ("include_unpolished", C.c_int)]


POLISH_STATS = ("rows", "rows_selected", "contigs", "contigs_polished", "substituted", "deleted", "inserted_bases", "slots_opened",
                "ins_long", "ins_edge")
POLISH_MS = ("ms_device", "ms_total")


class PolishStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in POLISH_STATS] + [(k, C.c_double) for k in POLISH_MS]


class PolishQOpts(C.Structure):
    _fields_ = PolishOpts._fields_ + [("qual_weight", C.c_int), ("min_avg_qual", C.c_double)]


POLISH_QSTATS = ("reads_with_qual", "rows_low_qual")


class PolishQStats(C.Structure):
    _fields_ = [("base", PolishStats)] + [(k, C.c_uint64) for k in POLISH_QSTATS]


POLISH_PSTATS = ("pairs_listed", "pairs_unknown", "rows_not_listed")


class PolishPStats(C.Structure):
    _fields_ = [("q", PolishQStats)] + [(k, C.c_uint64) for k in POLISH_PSTATS]


class DepthOpts(C.Structure):
    _fields_ = [("min_len", C.c_int), ("min_iden", C.c_double)]


DEPTH_STATS = ("rows", "rows_selected", "contigs", "contigs_covered", "positions", "covered", "bases", "runs", "pairs_listed",
               "pairs_unknown", "rows_not_listed")


class DepthStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in DEPTH_STATS] + [(k, C.c_double) for k in POLISH_MS]


class VariantOpts(C.Structure):
    _fields_ = [("min_len", C.c_int), ("min_iden", C.c_double), ("min_cov", C.c_int), ("min_alt", C.c_int), ("min_frac", C.c_double)]


VARIANT_STATS = ("rows", "rows_selected", "contigs", "contigs_covered", "positions", "callable", "ref_other", "sites", "sites_base",
                 "sites_del", "pairs_listed", "pairs_unknown", "rows_not_listed")


class VariantStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VARIANT_STATS] + [(k, C.c_double) for k in POLISH_MS]


VARIANT_INS_STATS = VARIANT_STATS + ("slots_callable", "ins_sites", "ins_long", "ins_edge")


class VariantInsStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VARIANT_INS_STATS] + [(k, C.c_double) for k in POLISH_MS]


class VariantQOpts(C.Structure):
    _fields_ = list(VariantOpts._fields_) + [("min_base_qual", C.c_int), ("min_avg_qual", C.c_double)]


VARIANT_QCOUNTS = ("reads_with_qual", "rows_low_qual", "columns_low_qual")


class VariantQCounts(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in VARIANT_QCOUNTS]


class PhaseOpts(C.Structure):
    _fields_ = list(VariantOpts._fields_) + [("min_link", C.c_int), ("min_agree", C.c_double)]


PHASE_STATS = VARIANT_STATS + ("links", "links_phased", "blocks", "blocks_multi", "sites_phased", "alleles", "read_records", "reads_a",
                               "reads_b", "reads_tie")


class PhaseStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in PHASE_STATS] + [(k, C.c_double) for k in POLISH_MS]


PHASE_REACH_MAX = 8      # include/hylight_mi.h: HLMI_PHASE_REACH_MAX
PHASE_REACH_STATS = ("links_far", "links_far_phased", "joins_far", "sites_bridged", "links_conflict")


class PhaseReachStats(C.Structure):
    _fields_ = [("base", PhaseStats)] + [(k, C.c_uint64) for k in PHASE_REACH_STATS]


PHASE_INS_STATS = ("slots_callable", "ins_sites", "ins_long", "ins_edge", "ins_sites_phasing", "ins_sites_left_out", "ins_sites_phased")


class PhaseInsStats(C.Structure):
    _fields_ = [("reach", PhaseReachStats)] + [(k, C.c_uint64) for k in PHASE_INS_STATS]


class HaplotigOpts(C.Structure):
    _fields_ = list(PhaseOpts._fields_) + [("min_side", C.c_int), ("include_unpolished", C.c_int)]


HAPLOTIG_STATS = ("blocks_split", "contigs_split", "positions_split", "diff_positions", "records", "substituted", "deleted",
                  "inserted_bases", "slots_opened", "ins_long", "ins_edge")


class HaplotigStats(C.Structure):
    _fields_ = [("phase", PhaseStats)] + [(k, C.c_uint64) for k in HAPLOTIG_STATS] + [(k, C.c_double) for k in POLISH_MS]


HAPLOTIG_INS_STATS = PHASE_INS_STATS + ("diff_slots",)


class HaplotigInsStats(C.Structure):
    _fields_ = [("base", HaplotigStats)] + [(k, C.c_uint64) for k in HAPLOTIG_INS_STATS]


ABI_VERSION = 7          # include/hylight_mi.h: HLMI_ABI_VERSION

# every symbol include/hylight_mi.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "hlmi_abi_version": (C.c_int, []),
    "hlmi_init": (C.c_int, [C.c_int, C.c_int]),
    "hlmi_shutdown": (None, []),
    "hlmi_last_error": (C.c_char_p, []),
    "hlmi_version": (C.c_char_p, []),
    "hlmi_split_reads2": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                    C.c_int, C.c_double, C.c_int]),
    "hlmi_split_reads2_shard": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int,
                                          C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int]),
    "hlmi_merge_scored_paf": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_char_p]),
    "hlmi_filter_chunk": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                    C.c_int]),
    "hlmi_paf_window_filter": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_char_p, C.c_char_p]),
    "hlmi_filter_ovlp_inline": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_double]),
    "hlmi_minimap22sfo": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_double]),
    "hlmi_filter_non_atcg": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int]),
    "hlmi_gfa2fa": (C.c_int, [C.c_char_p, C.c_char_p]),
    "hlmi_pick_up": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "hlmi_ava_opts_long": (None, [C.POINTER(AvaOpts)]),
    "hlmi_ava_opts_short": (None, [C.POINTER(AvaOpts)]),
    "hlmi_ava": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.c_char_p]),
    "hlmi_miniasm": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]),
    "hlmi_sfo2overlaps": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int]),
    "hlmi_sr_overlaps": (C.c_int, [C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_char_p, C.POINTER(C.c_uint64)]),
    "hlmi_vq_parse_overlaps": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(VqOverlap),
                                         C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hlmi_vq_transitive_edges": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]),
    "hlmi_vq_overlap_scores": (C.c_int, [C.c_char_p, C.POINTER(VqOverlap), C.c_uint64, C.c_double, C.c_uint32, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "hlmi_vq_graph_opts_stageb": (None, [C.POINTER(VqGraphOpts)]),
    "hlmi_vq_graph": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.c_char_p, C.POINTER(VqGraphStats)]),
    "hlmi_vq_merge_opts_stageb": (None, [C.POINTER(VqMergeOpts)]),
    "hlmi_vq_merge": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqMergeOpts), C.c_char_p,
                                C.POINTER(VqGraphStats), C.POINTER(VqMergeStats)]),
    "hlmi_vq_clique_opts_polyte": (None, [C.POINTER(VqCliqueOpts), C.c_int]),
    "hlmi_vq_cliques_of_graph": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]),
    "hlmi_vq_cliques": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqCliqueOpts), C.c_char_p,
                                  C.POINTER(VqGraphStats), C.POINTER(VqCliqueStats)]),
    "hlmi_vq_next_opts_stageb": (None, [C.POINTER(VqNextOpts)]),
    "hlmi_vq_iteration": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqMergeOpts),
                                    C.POINTER(VqNextOpts), C.c_char_p, C.POINTER(VqGraphStats), C.POINTER(VqMergeStats),
                                    C.POINTER(VqNextStats)]),
    "hlmi_vq_clique_iteration": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqCliqueOpts),
                                           C.POINTER(VqNextOpts), C.c_char_p, C.POINTER(VqGraphStats), C.POINTER(VqCliqueStats),
                                           C.POINTER(VqCliqueNextStats)]),
    "hlmi_vq_branch_opts_polyte": (None, [C.POINTER(VqBranchOpts)]),
    "hlmi_vq_branch_graph": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts),
                                       C.POINTER(VqBranchOpts), C.c_char_p, C.POINTER(VqGraphStats), C.POINTER(VqBranchStats)]),
    "hlmi_vq_branch_iteration": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts),
                                           C.POINTER(VqBranchOpts), C.POINTER(VqCliqueOpts), C.POINTER(VqNextOpts), C.c_char_p,
                                           C.POINTER(VqGraphStats), C.POINTER(VqBranchStats), C.POINTER(VqCliqueStats),
                                           C.POINTER(VqCliqueNextStats)]),
    "hlmi_vq_consensus_pair": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    # the same calls with --min_qual: the sibling's signature with one double in front of out_dir (consensus_pair: of out_seq)
    "hlmi_vq_consensus_pair_mq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_double, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    "hlmi_vq_merge_mq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqMergeOpts), C.c_double,
                                   C.c_char_p, C.POINTER(VqGraphStats), C.POINTER(VqMergeStats)]),
    "hlmi_vq_cliques_mq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqCliqueOpts), C.c_double,
                                     C.c_char_p, C.POINTER(VqGraphStats), C.POINTER(VqCliqueStats)]),
    "hlmi_vq_iteration_mq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqMergeOpts),
                                       C.POINTER(VqNextOpts), C.c_double, C.c_char_p, C.POINTER(VqGraphStats),
                                       C.POINTER(VqMergeStats), C.POINTER(VqNextStats)]),
    "hlmi_vq_clique_iteration_mq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts), C.POINTER(VqCliqueOpts),
                                              C.POINTER(VqNextOpts), C.c_double, C.c_char_p, C.POINTER(VqGraphStats),
                                              C.POINTER(VqCliqueStats), C.POINTER(VqCliqueNextStats)]),
    "hlmi_vq_branch_iteration_mq": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VqGraphOpts),
                                              C.POINTER(VqBranchOpts), C.POINTER(VqCliqueOpts), C.POINTER(VqNextOpts), C.c_double,
                                              C.c_char_p, C.POINTER(VqGraphStats), C.POINTER(VqBranchStats),
                                              C.POINTER(VqCliqueStats), C.POINTER(VqCliqueNextStats)]),
    "hlmi_cluster_opts_default": (None, [C.POINTER(ClusterOpts)]),
    "hlmi_cluster_short": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(ClusterOpts), C.c_char_p, C.POINTER(ClusterStats)]),
    "hlmi_polish_opts_default": (None, [C.POINTER(PolishOpts)]),
    "hlmi_polish": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PolishOpts), C.c_char_p, C.POINTER(PolishStats)]),
    "hlmi_polish_reads": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(PolishOpts), C.c_char_p,
                                    C.POINTER(PolishStats)]),
    # the same two calls with base qualities: weighted votes and the read-quality floor
    "hlmi_polish_qopts_default": (None, [C.POINTER(PolishQOpts)]),
    "hlmi_polish_q": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PolishQOpts), C.c_char_p, C.POINTER(PolishQStats)]),
    "hlmi_polish_reads_q": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(PolishQOpts), C.c_char_p,
                                      C.POINTER(PolishQStats)]),
    "hlmi_polish_pairs": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PolishQOpts), C.c_char_p, C.c_char_p,
                                    C.POINTER(PolishPStats)]),
    "hlmi_polish_reads_pairs": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(PolishQOpts), C.c_char_p, C.c_char_p,
                                          C.POINTER(PolishPStats)]),
    # read depth and abundance per contig
    "hlmi_depth_opts_default": (None, [C.POINTER(DepthOpts)]),
    "hlmi_depth": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(DepthOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                             C.POINTER(DepthStats)]),
    "hlmi_depth_reads": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(DepthOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                                   C.POINTER(DepthStats)]),
    # variant sites per contig
    "hlmi_variant_opts_default": (None, [C.POINTER(VariantOpts)]),
    "hlmi_variants": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VariantOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                                C.POINTER(VariantStats)]),
    "hlmi_variants_reads": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(VariantOpts), C.c_char_p, C.c_char_p,
                                      C.c_char_p, C.POINTER(VariantStats)]),
    # ... with insertion sites
    "hlmi_variants_ins": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VariantOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                                    C.c_char_p, C.POINTER(VariantInsStats)]),
    "hlmi_variants_reads_ins": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(VariantOpts), C.c_char_p, C.c_char_p,
                                          C.c_char_p, C.c_char_p, C.POINTER(VariantInsStats)]),
    # ... with base qualities: a per-base floor and a read floor
    "hlmi_variant_qopts_default": (None, [C.POINTER(VariantQOpts)]),
    "hlmi_variants_q": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VariantQOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                                  C.POINTER(VariantStats), C.POINTER(VariantQCounts)]),
    "hlmi_variants_reads_q": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(VariantQOpts), C.c_char_p, C.c_char_p,
                                        C.c_char_p, C.POINTER(VariantStats), C.POINTER(VariantQCounts)]),
    "hlmi_variants_ins_q": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(VariantQOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                                      C.c_char_p, C.POINTER(VariantInsStats), C.POINTER(VariantQCounts)]),
    "hlmi_variants_reads_ins_q": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(VariantQOpts), C.c_char_p, C.c_char_p,
                                            C.c_char_p, C.c_char_p, C.POINTER(VariantInsStats), C.POINTER(VariantQCounts)]),
    # phased variant sites
    "hlmi_phase_opts_default": (None, [C.POINTER(PhaseOpts)]),
    "hlmi_phase": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PhaseOpts), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                             C.POINTER(PhaseStats)]),
    "hlmi_phase_reads": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(PhaseOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                                   C.c_char_p, C.POINTER(PhaseStats)]),
    "hlmi_phase_reach": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PhaseOpts), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p,
                                   C.c_char_p, C.POINTER(PhaseReachStats)]),
    "hlmi_phase_reads_reach": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(PhaseOpts), C.c_int, C.c_char_p, C.c_char_p,
                                         C.c_char_p, C.c_char_p, C.POINTER(PhaseReachStats)]),
    "hlmi_phase_ins": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PhaseOpts), C.c_int, C.c_char_p, C.c_char_p, C.c_char_p,
                                 C.c_char_p, C.POINTER(PhaseInsStats)]),
    "hlmi_phase_reads_ins": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(PhaseOpts), C.c_int, C.c_char_p, C.c_char_p,
                                       C.c_char_p, C.c_char_p, C.POINTER(PhaseInsStats)]),
    # haplotigs
    "hlmi_haplotig_opts_default": (None, [C.POINTER(HaplotigOpts)]),
    "hlmi_haplotigs": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(HaplotigOpts), C.c_char_p, C.c_char_p, C.c_char_p,
                                 C.POINTER(HaplotigStats)]),
    "hlmi_haplotigs_reads": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(HaplotigOpts), C.c_char_p, C.c_char_p,
                                       C.c_char_p, C.POINTER(HaplotigStats)]),
    "hlmi_haplotigs_reach": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(HaplotigOpts), C.c_int, C.c_char_p, C.c_char_p,
                                       C.c_char_p, C.POINTER(HaplotigStats)]),
    "hlmi_haplotigs_reads_reach": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(HaplotigOpts), C.c_int, C.c_char_p,
                                             C.c_char_p, C.c_char_p, C.POINTER(HaplotigStats)]),
    "hlmi_haplotigs_ins": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(HaplotigOpts), C.c_int, C.c_char_p, C.c_char_p,
                                     C.c_char_p, C.POINTER(HaplotigInsStats)]),
    "hlmi_haplotigs_reads_ins": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(AvaOpts), C.POINTER(HaplotigOpts), C.c_int, C.c_char_p,
                                           C.c_char_p, C.c_char_p, C.POINTER(HaplotigInsStats)]),
    "hlmi_job_open": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_int, C.c_int]),
    "hlmi_job_close": (None, [C.c_void_p]),
    "hlmi_job_num_queries": (C.c_int64, [C.c_void_p]),
    "hlmi_job_num_chunks": (C.c_int64, [C.c_void_p]),
    "hlmi_job_sketch_bound": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int64]),
    "hlmi_job_sketch": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.POINTER(C.c_int64)]),
    "hlmi_job_sketch_own": (C.c_int, [C.c_void_p]),
    "hlmi_job_set_query_sketch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "hlmi_job_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_char_p]),
    "hlmi_last_stats_json": (C.c_int, [C.c_char_p, C.c_int64]),
}

_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as
    /opt/rocm's); if both get loaded, whichever initialises second finds no device.  Loading torch's
    copy first makes the dynamic loader bind libhylight_mi.so's NEEDED libamdhip64.so.7 to it, so the
    library, torch's allocator and RCCL share one runtime whatever the import order."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    """Load the shared library (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -m hylight_amd.build` "
                              "(there is no CPU fallback)")
        _preload_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.hlmi_abi_version() != ABI_VERSION:          # (AvaOpts above mirrors the header's hlmi_ava_opts of that version)
            raise ImportError(f"{LIB_PATH}: ABI version {lib.hlmi_abi_version()}, this binding is written for {ABI_VERSION}")
        _lib = lib
    return _lib


def _b(s):
    return None if s is None else os.fspath(s).encode()


def _check(rc):
    if rc != 0:
        raise HlmiError(rc, load().hlmi_last_error().decode(errors="replace"))


def init(device=-1, host_threads=0):
    _check(load().hlmi_init(device, host_threads))


def shutdown():
    load().hlmi_shutdown()


def version():
    return load().hlmi_version().decode()


def last_stats():
    buf = C.create_string_buffer(1 << 16)
    _check(load().hlmi_last_stats_json(buf, len(buf)))
    return json.loads(buf.value.decode())


def filter_chunk(paf_in, out_paf, len_over, mc, iden, thre=0.0025, min_o=4, long_mode=True):
    _check(load().hlmi_filter_chunk(_b(paf_in), _b(out_paf), len_over, mc, iden, thre, min_o, int(long_mode)))


def paf_window_filter(variant, in_paf, out_path, min_len=60, min_iden=-1.0, min_o=0, sfo=False):
    _check(load().hlmi_paf_window_filter(variant, min_len, min_iden, min_o, int(sfo), _b(in_paf), _b(out_path)))


def filter_ovlp_inline(in_paf, out_paf, min_ovlp_len, min_identity, o=1000, r=0.8):
    _check(load().hlmi_filter_ovlp_inline(_b(in_paf), _b(out_paf), min_ovlp_len, min_identity, o, r))


def minimap22sfo(in_paf, out_sfo, min_overlap_len=0, min_pident=0.0):
    _check(load().hlmi_minimap22sfo(_b(in_paf), _b(out_sfo), min_overlap_len, min_pident))


def filter_non_atcg(fastx, out_fa, model):
    """utils.filter_non_atcg with an explicit output path; model = "fastq" | "fasta" (script/utils.py:81)."""
    _check(load().hlmi_filter_non_atcg(_b(fastx), _b(out_fa), int(model == "fastq")))
    return out_fa


def gfa2fa(gfa, fa):
    _check(load().hlmi_gfa2fa(_b(gfa), _b(fa)))


def pick_up(ovlap_paf, fastx, out_fastx, mode):
    """HyLight.pick_up with an explicit output path; mode = "fastq" | "fasta" (script/HyLight.py:347)."""
    _check(load().hlmi_pick_up(_b(ovlap_paf), _b(fastx), _b(out_fastx), int(mode == "fastq")))
    return out_fastx


def split_reads2(reads_fa, ref_fa, nsplit, out_dir, out_paf, threads=30, len_over=3000, mc=2, iden=0.95,
                 long=False, rank=0, world=1):
    _check(load().hlmi_split_reads2_shard(_b(reads_fa), _b(ref_fa), nsplit, _b(out_dir), _b(out_paf), threads,
                                          len_over, mc, iden, int(long), rank, world))
    return out_paf


def merge_scored_paf(in_pafs, out_paf):
    arr = (C.c_char_p * len(in_pafs))(*[_b(p) for p in in_pafs])
    _check(load().hlmi_merge_scored_paf(arr, len(in_pafs), _b(out_paf)))


def ava_opts_long():
    o = AvaOpts()
    load().hlmi_ava_opts_long(C.byref(o))
    return o


def ava_opts_short():
    o = AvaOpts()
    load().hlmi_ava_opts_short(C.byref(o))
    return o


def ava(target_fa, query_fa, out_paf, opts=None):
    _check(load().hlmi_ava(_b(target_fa), _b(query_fa), C.byref(opts) if opts is not None else None, _b(out_paf)))


def miniasm(paf, reads_fa, out_path, bub_dist=10000, n_rounds_arg=1, max_ext=1, min_dp=1, outfmt="ug"):
    _check(load().hlmi_miniasm(_b(paf), _b(reads_fa), bub_dist, n_rounds_arg, max_ext, min_dp, _b(outfmt),
                               _b(out_path)))


def sfo2overlaps(in_sfo, out_savage, num_singles, num_pairs=0):
    _check(load().hlmi_sfo2overlaps(_b(in_sfo), _b(out_savage), num_singles, num_pairs))


def sr_overlaps(reads, out_overlaps, min_ovlp_len, min_identity=0.98, o=1, r=0.8):
    """hlmi_sr_overlaps: the self-overlaps of `reads` (FASTQ / FASTA, names 0, 1, 2, ..) as a SAVAGE overlaps file - POLYTE's
    run_sfo chain (ava with driver.contig_ava_opts() -> filter_ovlp_inline -> minimap22sfo(0, 0) -> sfo2overlaps) in one call,
    no intermediate files.  -> the number of lines written."""
    n = C.c_uint64(0)
    _check(load().hlmi_sr_overlaps(_b(reads), min_ovlp_len, min_identity, o, r, _b(out_overlaps), C.byref(n)))
    return n.value


def vq_parse_overlaps(savage_path, min_len=150, min_perc=0, relax_pe=False, max_overlaps=100000000):
    """edge candidates of a 13-column overlaps file -> (list of dicts, n_nonedge, n_skipped)."""
    n, ne, sk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(load().hlmi_vq_parse_overlaps(_b(savage_path), min_len, min_perc, int(relax_pe), max_overlaps, None, 0,
                                         C.byref(n), C.byref(ne), C.byref(sk)))
    buf = (VqOverlap * max(n.value, 1))()
    _check(load().hlmi_vq_parse_overlaps(_b(savage_path), min_len, min_perc, int(relax_pe), max_overlaps, buf, n.value,
                                         C.byref(n), C.byref(ne), C.byref(sk)))
    rows = []
    for o in buf[:n.value]:
        rows.append(dict(id1=o.id1, id2=o.id2, pos1=o.pos1, pos2=o.pos2, ord=o.ord.decode(), ori1=o.ori1.decode(),
                         ori2=o.ori2.decode(), perc1=o.perc1, perc2=o.perc2, len1=o.len1, len2=o.len2,
                         type1=o.type1.decode(), type2=o.type2.decode()))
    return rows, ne.value, sk.value


def vq_overlap_scores(fastq_singles, overlaps, mismatch=0.0, min_read_len=0):
    """EdgeCalculator::overlap_score for single-single overlaps (dicts as vq_parse_overlaps returns them) ->
    list of (score, mismatch_rate, pos3)."""
    n = len(overlaps)
    buf = (VqOverlap * max(n, 1))()
    for k, o in enumerate(overlaps):
        b = buf[k]
        b.id1, b.id2, b.pos1, b.pos2 = o["id1"], o["id2"], o["pos1"], o.get("pos2", 0)
        b.perc1, b.perc2, b.len1, b.len2 = o.get("perc1", 0), o.get("perc2", 0), o.get("len1", 0), o.get("len2", 0)
        b.ord, b.ori1, b.ori2 = o.get("ord", "-").encode(), o["ori1"].encode(), o["ori2"].encode()
        b.type1, b.type2 = o.get("type1", "s").encode(), o.get("type2", "s").encode()
    sc, mr, p3 = (C.c_double * max(n, 1))(), (C.c_double * max(n, 1))(), (C.c_int64 * max(n, 1))()
    _check(load().hlmi_vq_overlap_scores(_b(fastq_singles), buf, n, mismatch, min_read_len, sc, mr, p3))
    return [(sc[k], mr[k], p3[k]) for k in range(n)]


def vq_transitive_edges(n_vertices, src, dst, ovlen=None, remove_trans=1):
    """-> (flags per edge as bytes: bit 0 transitive in the last round, bit 1 scheduled by the branch reduction; count)."""
    n = len(src)
    a32 = lambda v: (C.c_uint32 * max(n, 1))(*v)
    flags = (C.c_uint8 * max(n, 1))()
    cnt = C.c_uint64(0)
    _check(load().hlmi_vq_transitive_edges(n_vertices, n, a32(src), a32(dst), a32(ovlen) if ovlen is not None else None,
                                           remove_trans, flags, C.byref(cnt)))
    return list(flags[:n]), cnt.value


def _set_opts(caller, structs, opts):
    """Each keyword goes into the first of the option structs that has a field of its name (a bool as an int)."""
    for k, v in opts.items():
        target = next((t for t in structs if k in dict(type(t)._fields_)), None)
        if target is None:
            raise TypeError(f"{caller}: unknown option {k!r}")
        setattr(target, k, int(v) if isinstance(v, bool) else v)


def _stats(st, names):
    return {k: getattr(st, k) for k in names}


def _mq(name, min_qual, head, tail):
    """The call `name` over head + tail; with a min_qual its `_mq` sibling, the value between the two."""
    if min_qual is None:
        return getattr(load(), name)(*head, *tail)
    return getattr(load(), name + "_mq")(*head, float(min_qual), *tail)


def vq_graph_opts_stageb():
    """hlmi_vq_graph_opts_stageb: the options of HyLight's first stage-b iteration, as a dict."""
    o = VqGraphOpts()
    load().hlmi_vq_graph_opts_stageb(C.byref(o))
    return {k: getattr(o, k) for k, _ in VqGraphOpts._fields_}


def vq_graph(singles_fastq, overlaps, out_dir, **opts):
    """ViralQuasispecies --graph_only: the oriented, reduced overlap graph of `overlaps` over the reads
    of `singles_fastq`, written into out_dir (created if missing).  Options: the fields of hlmi_vq_graph_opts, the
    stage-b values by default.  -> dict of the stats (hlmi_vq_graph_stats)."""
    o = VqGraphOpts()
    load().hlmi_vq_graph_opts_stageb(C.byref(o))
    _set_opts("vq_graph", (o,), opts)
    os.makedirs(out_dir, exist_ok=True)
    st = VqGraphStats()
    _check(load().hlmi_vq_graph(_b(singles_fastq), _b(overlaps), C.byref(o), _b(out_dir), C.byref(st)))
    return _stats(st, VQ_GRAPH_STATS)


def vq_merge_opts_stageb():
    """hlmi_vq_merge_opts_stageb: the SRBuilder options of HyLight's first stage-b iteration, as a dict."""
    o = VqMergeOpts()
    load().hlmi_vq_merge_opts_stageb(C.byref(o))
    return {k: getattr(o, k) for k, _ in VqMergeOpts._fields_}


def vq_merge(singles_fastq, overlaps, out_dir, subreads_in=None, min_qual=None, **opts):
    """hlmi_vq_merge: the graph of vq_graph (same files) and then SRBuilder::mergeAlongEdges - singles.fastq, subreads.txt,
    removed_tip_sequences.fastq (appended to) and superread_map.txt in out_dir (created if missing).  Options: the fields
    of hlmi_vq_graph_opts and of hlmi_vq_merge_opts, the stage-b values by default; subreads_in: the previous iteration's
    subreads.txt when first_it is off; min_qual: --min_qual, 0 .. 1 (None: SRBuilder's default 0.9 through hlmi_vq_merge itself,
    a number: hlmi_vq_merge_mq).  -> (graph stats, merge stats) as dicts."""
    go, mo = VqGraphOpts(), VqMergeOpts()
    load().hlmi_vq_graph_opts_stageb(C.byref(go))
    load().hlmi_vq_merge_opts_stageb(C.byref(mo))
    _set_opts("vq_merge", (go, mo), opts)
    os.makedirs(out_dir, exist_ok=True)
    gst, mst = VqGraphStats(), VqMergeStats()
    _check(_mq("hlmi_vq_merge", min_qual, (_b(singles_fastq), _b(overlaps), _b(subreads_in), C.byref(go), C.byref(mo)),
               (_b(out_dir), C.byref(gst), C.byref(mst))))
    return _stats(gst, VQ_GRAPH_STATS), _stats(mst, VQ_MERGE_STATS + VQ_MERGE_MS)


def vq_clique_opts_polyte(error_correction=False):
    """hlmi_vq_clique_opts_polyte: the SRBuilder options POLYTE passes with --cliques=true, as a dict.  POLYTE also passes
    --min_qual=0, which is no field of the struct: give min_qual=0 to vq_cliques / vq_clique_iteration / vq_branch_iteration.
    Without it they keep minQual 0.9, so disagreeing columns become N (see the header)."""
    o = VqCliqueOpts()
    load().hlmi_vq_clique_opts_polyte(C.byref(o), int(bool(error_correction)))
    return {k: getattr(o, k) for k, _ in VqCliqueOpts._fields_}


def vq_cliques_of_graph(graph_txt, cliques_out):
    """hlmi_vq_cliques_of_graph: the maximal cliques of a graph.txt, written as the reference's enumerator prints them (its
    two text lines, then one clique per line).  Host code: needs no GPU.  -> the number of cliques."""
    n = C.c_uint64(0)
    _check(load().hlmi_vq_cliques_of_graph(_b(graph_txt), _b(cliques_out), C.byref(n)))
    return n.value


def vq_cliques(singles_fastq, overlaps, out_dir, subreads_in=None, min_qual=None, **opts):
    """hlmi_vq_cliques: the graph of vq_graph (same files) and then ViralQuasispecies' --cliques=true step for single-end reads -
    cliques.txt, singles.fastq, subreads.txt and clique_map.txt in out_dir (created if missing).  Options: the fields of
    hlmi_vq_graph_opts (the stage-b values by default; what POLYTE passes beside them is written down in the header) and of
    hlmi_vq_clique_opts (hlmi_vq_clique_opts_polyte for the error_correction given); min_qual as for vq_merge (POLYTE: 0).
    -> (graph stats, clique stats)."""
    go, co = VqGraphOpts(), VqCliqueOpts()
    load().hlmi_vq_graph_opts_stageb(C.byref(go))
    load().hlmi_vq_clique_opts_polyte(C.byref(co), int(bool(opts.get("error_correction", False))))
    _set_opts("vq_cliques", (go, co), opts)
    os.makedirs(out_dir, exist_ok=True)
    gst, cst = VqGraphStats(), VqCliqueStats()
    _check(_mq("hlmi_vq_cliques", min_qual, (_b(singles_fastq), _b(overlaps), _b(subreads_in), C.byref(go), C.byref(co)),
               (_b(out_dir), C.byref(gst), C.byref(cst))))
    return _stats(gst, VQ_GRAPH_STATS), _stats(cst, VQ_CLIQUE_STATS + VQ_CLIQUE_MS)


def vq_iteration(singles_fastq, overlaps, out_dir, subreads_in=None, min_qual=None, **opts):
    """hlmi_vq_iteration: one stage-b iteration - the files of vq_merge, then overlaps.txt (SRBuilder::findNextOverlaps) and one
    line appended to stats.txt, in out_dir (created if missing).  The inputs may lie in out_dir under the names written: they
    are read first.  Options: the fields of hlmi_vq_graph_opts, hlmi_vq_merge_opts and hlmi_vq_next_opts, the stage-b values
    by default; min_qual as for vq_merge.  -> (graph stats, merge stats, next stats) as dicts."""
    go, mo, no = VqGraphOpts(), VqMergeOpts(), VqNextOpts()
    load().hlmi_vq_graph_opts_stageb(C.byref(go))
    load().hlmi_vq_merge_opts_stageb(C.byref(mo))
    load().hlmi_vq_next_opts_stageb(C.byref(no))
    _set_opts("vq_iteration", (go, mo, no), opts)
    os.makedirs(out_dir, exist_ok=True)
    gst, mst, nst = VqGraphStats(), VqMergeStats(), VqNextStats()
    _check(_mq("hlmi_vq_iteration", min_qual, (_b(singles_fastq), _b(overlaps), _b(subreads_in), C.byref(go), C.byref(mo), C.byref(no)),
               (_b(out_dir), C.byref(gst), C.byref(mst), C.byref(nst))))
    return _stats(gst, VQ_GRAPH_STATS), _stats(mst, VQ_MERGE_STATS + VQ_MERGE_MS), _stats(nst, VQ_NEXT_STATS + VQ_NEXT_MS)


def vq_clique_iteration(singles_fastq, overlaps, out_dir, subreads_in=None, min_qual=None, **opts):
    """hlmi_vq_clique_iteration: one clique iteration - the files of vq_cliques, then overlaps.txt (SRBuilder::findNextOverlaps
    over the super-read lists of the vertices) and one line appended to stats.txt, in out_dir (created if missing).  The inputs
    may lie in out_dir under the names written: they are read first.  Options: the fields of hlmi_vq_graph_opts,
    hlmi_vq_clique_opts and hlmi_vq_next_opts, with the defaults of vq_cliques and vq_iteration; min_qual as there.  -> (graph stats, clique
    stats, next stats) as dicts; the next stats add candidates, max_list and in_several to those of vq_iteration."""
    go, co, no = VqGraphOpts(), VqCliqueOpts(), VqNextOpts()
    load().hlmi_vq_graph_opts_stageb(C.byref(go))
    load().hlmi_vq_clique_opts_polyte(C.byref(co), int(bool(opts.get("error_correction", False))))
    load().hlmi_vq_next_opts_stageb(C.byref(no))
    _set_opts("vq_clique_iteration", (go, co, no), opts)
    os.makedirs(out_dir, exist_ok=True)
    gst, cst, nst = VqGraphStats(), VqCliqueStats(), VqCliqueNextStats()
    _check(_mq("hlmi_vq_clique_iteration", min_qual,
               (_b(singles_fastq), _b(overlaps), _b(subreads_in), C.byref(go), C.byref(co), C.byref(no)),
               (_b(out_dir), C.byref(gst), C.byref(cst), C.byref(nst))))
    return (_stats(gst, VQ_GRAPH_STATS), _stats(cst, VQ_CLIQUE_STATS + VQ_CLIQUE_MS),
            _stats(nst, VQ_CLIQUE_NEXT_STATS + VQ_NEXT_MS))


def vq_branch_opts_polyte():
    """hlmi_vq_branch_opts_polyte: careful on, the counts 0, as a dict."""
    o = VqBranchOpts()
    load().hlmi_vq_branch_opts_polyte(C.byref(o))
    return {k: getattr(o, k) for k, _ in VqBranchOpts._fields_}


def _branch_graph_opts(caller, structs, opts):
    """The graph options of a branch-reduction run: the stage-b values with remove_branches off (the reduction takes its place)."""
    load().hlmi_vq_graph_opts_stageb(C.byref(structs[0]))
    structs[0].remove_branches = 0
    load().hlmi_vq_branch_opts_polyte(C.byref(structs[1]))
    _set_opts(caller, structs, opts)


def vq_branch_graph(singles_fastq, overlaps, original_fastq, threshold_table, out_dir, subreads_in=None, **opts):
    """hlmi_vq_branch_graph: ViralQuasispecies --graph_only with --branch_reduction=true - the files of vq_graph plus
    branch_components.txt in out_dir (created if missing).  Options: the fields of hlmi_vq_graph_opts (stage-b values,
    remove_branches off) and of hlmi_vq_branch_opts (se_count, pe_count, careful).  subreads_in None: every read is its own
    original.  -> (graph stats, branch stats) as dicts."""
    go, bo = VqGraphOpts(), VqBranchOpts()
    _branch_graph_opts("vq_branch_graph", (go, bo), opts)
    os.makedirs(out_dir, exist_ok=True)
    gst, bst = VqGraphStats(), VqBranchStats()
    _check(load().hlmi_vq_branch_graph(_b(singles_fastq), _b(overlaps), _b(subreads_in), _b(original_fastq), _b(threshold_table),
                                       C.byref(go), C.byref(bo), _b(out_dir), C.byref(gst), C.byref(bst)))
    return _stats(gst, VQ_GRAPH_STATS), _stats(bst, VQ_BRANCH_STATS + VQ_BRANCH_MS)


def vq_branch_iteration(singles_fastq, overlaps, original_fastq, threshold_table, out_dir, subreads_in=None, min_qual=None, **opts):
    """hlmi_vq_branch_iteration: the graph of vq_branch_graph, then everything vq_clique_iteration does behind its graph.
    Options: those of vq_branch_graph and of vq_clique_iteration, its min_qual among them.  -> (graph, branch, clique, next stats)
    as dicts."""
    go, bo, co, no = VqGraphOpts(), VqBranchOpts(), VqCliqueOpts(), VqNextOpts()
    load().hlmi_vq_clique_opts_polyte(C.byref(co), int(bool(opts.get("error_correction", False))))
    load().hlmi_vq_next_opts_stageb(C.byref(no))
    _branch_graph_opts("vq_branch_iteration", (go, bo, co, no), opts)
    os.makedirs(out_dir, exist_ok=True)
    gst, bst, cst, nst = VqGraphStats(), VqBranchStats(), VqCliqueStats(), VqCliqueNextStats()
    _check(_mq("hlmi_vq_branch_iteration", min_qual,
               (_b(singles_fastq), _b(overlaps), _b(subreads_in), _b(original_fastq), _b(threshold_table), C.byref(go), C.byref(bo),
                C.byref(co), C.byref(no)), (_b(out_dir), C.byref(gst), C.byref(bst), C.byref(cst), C.byref(nst))))
    return (_stats(gst, VQ_GRAPH_STATS), _stats(bst, VQ_BRANCH_STATS + VQ_BRANCH_MS), _stats(cst, VQ_CLIQUE_STATS + VQ_CLIQUE_MS),
            _stats(nst, VQ_CLIQUE_NEXT_STATS + VQ_NEXT_MS))


def vq_consensus_pair(seq1, qual1, seq2, qual2, pos, min_qual=None):
    """hlmi_vq_consensus_pair: SRBuilder::consensus of two oriented sequences (str or bytes), the second `pos` bases behind
    the first -> (sequence, qualities) as str; ("", "") where the reference returns an empty consensus.  min_qual as for
    vq_merge (a number: hlmi_vq_consensus_pair_mq)."""
    if pos < 0 or pos >= 1 << 30:
        raise ValueError(f"vq_consensus_pair: pos {pos} is outside 0 .. 2^30")
    s1, q1, s2, q2 = (x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in (seq1, qual1, seq2, qual2))
    cap = max(len(s1), pos + len(s2), 1)
    out_s, out_q = C.create_string_buffer(cap), C.create_string_buffer(cap)
    n = C.c_uint32(0)
    _check(_mq("hlmi_vq_consensus_pair", min_qual, (s1, q1, len(s1), len(q1), s2, q2, len(s2), len(q2), pos), (out_s, out_q, C.byref(n))))
    return out_s.raw[:n.value].decode("latin-1"), out_q.raw[:n.value].decode("latin-1")


def cluster_short(paf, fastq, out_dir, size=15000, threads=20, **opts):
    """HyLight's short-read clustering (HyLight.py:215-226): readnames.txt, HiStrain_max<size>_final_clusters_grouped.json
    and fq_<size>/<cid>/<cid>.{1,2}.fq in out_dir (created if missing), byte for byte as the reference scripts leave them.
    `size`, `threads`: HyLight --size and -t.  Options: window_bytes (PAF bytes per upload; 1 = one session per window).
    -> dict of the stats (hlmi_cluster_stats)."""
    o = ClusterOpts()
    load().hlmi_cluster_opts_default(C.byref(o))
    o.size, o.threads = int(size), int(threads)
    for k, v in opts.items():
        if k != "window_bytes":
            raise TypeError(f"cluster_short: unknown option {k!r}")
        o.window_bytes = int(v)
    os.makedirs(out_dir, exist_ok=True)
    st = ClusterStats()
    _check(load().hlmi_cluster_short(_b(paf), _b(fastq), C.byref(o), _b(out_dir), C.byref(st)))
    return {k: getattr(st, k) for k in CLUSTER_STATS + CLUSTER_MS}


def polish(contigs, reads, paf, out_fa, pairs=None, **opts):
    """hlmi_polish: the pile-up consensus of `contigs` (FASTA / FASTQ) under the rows of `paf` (cg:Z: CIGARs in = X I D, as
    api.ava writes them) of `reads`, written to out_fa - the native stand-in for `racon --no-trimming -u` (a function of
    this project's own: include/hylight_mi.h states it, tests/polish_model.py is its contract).  Options: the fields of
    hlmi_polish_opts (min_len 0, min_iden 0.0, min_cov 3, include_unpolished 1).  -> dict of the stats (hlmi_polish_stats).
    With qual_weight= or min_avg_qual= the call is hlmi_polish_q (votes weighted by the reads' base qualities, rows of reads
    whose mean Phred is below min_avg_qual dropped; the one not given is off: 0 / 0.0; tests/polish_qual_model.py is the
    contract) and the dict also holds reads_with_qual and rows_low_qual.
    pairs=path: hlmi_polish_pairs - only rows whose (read, contig) pair is named by a row of that PAF-like list vote (fields 1
    and 6, either order; tests/polish_pairs_model.py is the contract); the dict also holds the quality stats and pairs_listed,
    pairs_unknown and rows_not_listed."""
    if pairs is not None:
        o, st = _polish_qopts("polish", opts), PolishPStats()
        _check(load().hlmi_polish_pairs(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_fa), C.byref(st)))
        return _polish_pstats(st)
    if _wants_qual(opts):
        o, st = _polish_qopts("polish", opts), PolishQStats()
        _check(load().hlmi_polish_q(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(out_fa), C.byref(st)))
        return _polish_qstats(st)
    o = _polish_opts("polish", opts)
    st = PolishStats()
    _check(load().hlmi_polish(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(out_fa), C.byref(st)))
    return {k: getattr(st, k) for k in POLISH_STATS + POLISH_MS}


def _polish_opts(who, opts):
    o = PolishOpts()
    load().hlmi_polish_opts_default(C.byref(o))
    for k, v in opts.items():
        if k not in dict(PolishOpts._fields_):
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, int(v) if isinstance(v, bool) else v)
    return o


def _wants_qual(opts):
    return "qual_weight" in opts or "min_avg_qual" in opts


def _polish_qopts(who, opts):
    """hlmi_polish_qopts: the base fields at hlmi_polish's defaults, the two quality options off unless given"""
    o = PolishQOpts()
    load().hlmi_polish_qopts_default(C.byref(o))
    o.qual_weight, o.min_avg_qual = 0, 0.0
    for k, v in opts.items():
        if k not in dict(PolishQOpts._fields_):
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, int(v) if isinstance(v, bool) else v)
    return o


def _polish_qstats(st):
    d = {k: getattr(st.base, k) for k in POLISH_STATS + POLISH_MS}
    d.update({k: getattr(st, k) for k in POLISH_QSTATS})
    return d


def _polish_pstats(st):
    d = _polish_qstats(st.q)
    d.update({k: getattr(st, k) for k in POLISH_PSTATS})
    return d


def polish_reads(contigs, reads, out_fa, ava_opts=None, pairs=None, **polish_opts):
    """hlmi_polish_reads: `ava(contigs, reads, P, ava_opts)` and `polish(contigs, reads, P, out_fa, **polish_opts)` in one
    call without the PAF P - the same file and the same integer stats, the overlapper's rows never leaving the device.
    ava_opts None: the long constants.  Refused (HlmiError, code -1) besides what polish refuses: a name twice among the reads
    or among the contigs, ava_opts.stub_oh >= 0.  -> dict of the stats (hlmi_polish_stats).  qual_weight= / min_avg_qual=: as
    for polish (hlmi_polish_reads_q).  pairs=path: as for polish (hlmi_polish_reads_pairs; the list is parsed on the device)."""
    if pairs is not None:
        o, st = _polish_qopts("polish_reads", polish_opts), PolishPStats()
        _check(load().hlmi_polish_reads_pairs(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                              _b(pairs), _b(out_fa), C.byref(st)))
        return _polish_pstats(st)
    if _wants_qual(polish_opts):
        o, st = _polish_qopts("polish_reads", polish_opts), PolishQStats()
        _check(load().hlmi_polish_reads_q(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                          _b(out_fa), C.byref(st)))
        return _polish_qstats(st)
    o = _polish_opts("polish_reads", polish_opts)
    st = PolishStats()
    _check(load().hlmi_polish_reads(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                    _b(out_fa), C.byref(st)))
    return {k: getattr(st, k) for k in POLISH_STATS + POLISH_MS}


def _depth_opts(who, opts):
    o = DepthOpts()
    load().hlmi_depth_opts_default(C.byref(o))
    for k, v in opts.items():
        if k not in dict(DepthOpts._fields_):
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, v)
    return o


def depth(contigs, reads, paf, out_tsv, out_bedgraph=None, pairs=None, **opts):
    """hlmi_depth: read depth and relative abundance of every contig of `contigs` under the rows of `paf` (as api.polish reads
    them; one row per read, api.polish's selection with pairs=, without a quality floor).  Writes the table out_tsv (contig,
    length, reads, bases, covered, mean_depth, median_depth, abundance) and, when given, the runs of equal depth as the
    bedGraph out_bedgraph.  Options: min_len 0, min_iden 0.0.  A function of this project's own: include/hylight_mi.h states
    it, tests/depth_model.py is its contract.  -> dict of the stats (hlmi_depth_stats)."""
    o, st = _depth_opts("depth", opts), DepthStats()
    _check(load().hlmi_depth(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_tsv), _b(out_bedgraph), C.byref(st)))
    return {k: getattr(st, k) for k in DEPTH_STATS + POLISH_MS}


def depth_reads(contigs, reads, out_tsv, out_bedgraph=None, ava_opts=None, pairs=None, **opts):
    """hlmi_depth_reads: `ava(contigs, reads, P, ava_opts)` and `depth(contigs, reads, P, ...)` in one call without the PAF P:
    the same files and the same integer stats.  ava_opts None: the long constants.  Refused besides what depth refuses:
    ava_opts.stub_oh >= 0.  -> dict of the stats (hlmi_depth_stats)."""
    o, st = _depth_opts("depth_reads", opts), DepthStats()
    _check(load().hlmi_depth_reads(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o), _b(pairs),
                                   _b(out_tsv), _b(out_bedgraph), C.byref(st)))
    return {k: getattr(st, k) for k in DEPTH_STATS + POLISH_MS}


def _variant_opts(who, opts):
    o = VariantOpts()
    load().hlmi_variant_opts_default(C.byref(o))
    for k, v in opts.items():
        if k not in dict(VariantOpts._fields_):
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, v)
    return o


def variants(contigs, reads, paf, out_sites, out_summary=None, pairs=None, **opts):
    """hlmi_variants: the variant sites of every contig of `contigs` under the rows of `paf` (selected as api.depth selects them,
    pairs= included; voted as api.polish votes positions, unweighted): a position is a site when the symbol other than the
    contig's own base with the most votes has min_alt votes and min_frac of the position's votes.  Writes the sites out_sites
    (contig, pos, ref, depth, A, C, G, T, del, alt, alt_count, alt_frac) and, when given, one line per contig out_summary
    (contig, length, reads, callable, sites, site_rate).  Options: min_len 0, min_iden 0.0, min_cov 3, min_alt 2, min_frac 0.2.
    A function of this project's own: include/hylight_mi.h states it, tests/variants_model.py is its contract.
    -> dict of the stats (hlmi_variant_stats)."""
    o, st = _variant_opts("variants", opts), VariantStats()
    _check(load().hlmi_variants(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_sites), _b(out_summary), C.byref(st)))
    return {k: getattr(st, k) for k in VARIANT_STATS + POLISH_MS}


def variants_reads(contigs, reads, out_sites, out_summary=None, ava_opts=None, pairs=None, **opts):
    """hlmi_variants_reads: `ava(contigs, reads, P, ava_opts)` and `variants(contigs, reads, P, ...)` in one call without the PAF
    P: the same files and the same integer stats.  ava_opts None: the long constants.  Refused besides what variants refuses:
    ava_opts.stub_oh >= 0.  -> dict of the stats (hlmi_variant_stats)."""
    o, st = _variant_opts("variants_reads", opts), VariantStats()
    _check(load().hlmi_variants_reads(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o), _b(pairs),
                                      _b(out_sites), _b(out_summary), C.byref(st)))
    return {k: getattr(st, k) for k in VARIANT_STATS + POLISH_MS}


def variants_ins(contigs, reads, paf, out_sites, out_ins, out_summary=None, pairs=None, **opts):
    """hlmi_variants_ins: api.variants with the insertion sites beside it.  out_sites is the file api.variants writes.  A slot (the
    gap in front of a contig position, as api.polish defines it) that min_cov selected rows span is an insertion site when the rows
    that insert there - 1..16 bases, or more (long rows) - number min_alt and make min_frac of the spanning rows, whether or not
    api.polish would open it.  Writes out_ins (contig, pos, ref, span, ins, ins_long, ins_frac, len, len_count, seq: the most
    frequent length among the inserting rows and the most frequent base per index among the rows of that length, '*' when only
    long rows insert) and, when given, out_summary with three columns more (slots, ins_sites, ins_rate).  Options: api.variants's.
    A function of this project's own: include/hylight_mi.h states it, tests/variants_ins_model.py is its contract.
    -> dict of the stats (hlmi_variant_ins_stats)."""
    o, st = _variant_opts("variants_ins", opts), VariantInsStats()
    _check(load().hlmi_variants_ins(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_sites), _b(out_summary), _b(out_ins),
                                    C.byref(st)))
    return {k: getattr(st, k) for k in VARIANT_INS_STATS + POLISH_MS}


def variants_ins_reads(contigs, reads, out_sites, out_ins, out_summary=None, ava_opts=None, pairs=None, **opts):
    """hlmi_variants_reads_ins: `ava(contigs, reads, P, ava_opts)` and `variants_ins(contigs, reads, P, ...)` in one call without
    the PAF P: the same files and the same integer stats.  ava_opts None: the long constants.  Refused besides what variants_ins
    refuses: ava_opts.stub_oh >= 0.  -> dict of the stats (hlmi_variant_ins_stats)."""
    o, st = _variant_opts("variants_ins_reads", opts), VariantInsStats()
    _check(load().hlmi_variants_reads_ins(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                          _b(pairs), _b(out_sites), _b(out_summary), _b(out_ins), C.byref(st)))
    return {k: getattr(st, k) for k in VARIANT_INS_STATS + POLISH_MS}


def _variant_qopts(who, opts):
    o = VariantQOpts()
    load().hlmi_variant_qopts_default(C.byref(o))
    for k, v in opts.items():
        if k not in dict(VariantQOpts._fields_):
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, v)
    return o


def _variant_qstats(st, qc, keys):
    return {**{k: getattr(st, k) for k in keys + POLISH_MS}, **{k: getattr(qc, k) for k in VARIANT_QCOUNTS}}


def variants_q(contigs, reads, paf, out_sites, out_summary=None, pairs=None, **opts):
    """hlmi_variants_q: api.variants with base qualities - a column whose Phred is below min_base_qual (default 10; 0: off) casts no
    vote, as an N column casts none, and the rows of a read whose mean Phred is below min_avg_qual (default 10.0; 0.0: off) are
    dropped as api.polish_q drops them.  The counts stay counts of reads.  FASTA records pass every floor; both floors 0 give
    api.variants's files.  include/hylight_mi.h states it, tests/variants_qual_model.py is its contract.
    -> dict of the stats (hlmi_variant_stats) with reads_with_qual, rows_low_qual and columns_low_qual (hlmi_variant_qcounts)."""
    o, st, qc = _variant_qopts("variants_q", opts), VariantStats(), VariantQCounts()
    _check(load().hlmi_variants_q(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_sites), _b(out_summary), C.byref(st),
                                  C.byref(qc)))
    return _variant_qstats(st, qc, VARIANT_STATS)


def variants_reads_q(contigs, reads, out_sites, out_summary=None, ava_opts=None, pairs=None, **opts):
    """hlmi_variants_reads_q: `ava(contigs, reads, P, ava_opts)` and `variants_q(contigs, reads, P, ...)` in one call without the
    PAF P: the same files and the same integer stats.  -> as variants_q."""
    o, st, qc = _variant_qopts("variants_reads_q", opts), VariantStats(), VariantQCounts()
    _check(load().hlmi_variants_reads_q(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                        _b(pairs), _b(out_sites), _b(out_summary), C.byref(st), C.byref(qc)))
    return _variant_qstats(st, qc, VARIANT_STATS)


def variants_ins_q(contigs, reads, paf, out_sites, out_ins, out_summary=None, pairs=None, **opts):
    """hlmi_variants_ins_q: api.variants_ins with the floors of variants_q.  out_sites is the file variants_q writes; a column
    below the base floor still spans its slot, and the slots' own counts take no quality into account: out_ins differs from
    api.variants_ins's only through rows the read floor dropped.  -> dict of the stats (hlmi_variant_ins_stats) with the three
    counters of hlmi_variant_qcounts."""
    o, st, qc = _variant_qopts("variants_ins_q", opts), VariantInsStats(), VariantQCounts()
    _check(load().hlmi_variants_ins_q(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_sites), _b(out_summary),
                                      _b(out_ins), C.byref(st), C.byref(qc)))
    return _variant_qstats(st, qc, VARIANT_INS_STATS)


def variants_ins_reads_q(contigs, reads, out_sites, out_ins, out_summary=None, ava_opts=None, pairs=None, **opts):
    """hlmi_variants_reads_ins_q: `ava(contigs, reads, P, ava_opts)` and `variants_ins_q(contigs, reads, P, ...)` in one call
    without the PAF P: the same files and the same integer stats.  -> as variants_ins_q."""
    o, st, qc = _variant_qopts("variants_ins_reads_q", opts), VariantInsStats(), VariantQCounts()
    _check(load().hlmi_variants_reads_ins_q(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                            _b(pairs), _b(out_sites), _b(out_summary), _b(out_ins), C.byref(st), C.byref(qc)))
    return _variant_qstats(st, qc, VARIANT_INS_STATS)


def _phase_opts(who, opts):
    o = PhaseOpts()
    load().hlmi_phase_opts_default(C.byref(o))
    for k, v in opts.items():
        if k not in dict(PhaseOpts._fields_):
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, v)
    return o


def phase(contigs, reads, paf, out_sites, out_links=None, out_reads=None, pairs=None, **opts):
    """hlmi_phase: the variant sites of api.variants (same selection, pairs= included, same votes, same site rule) phased from the
    reads.  Every selected row reads one allele at every site it spans (0 own, 1 alt, 2 another symbol, none); a link between two
    consecutive sites of a contig counts the rows with 0 or 1 at both (n00 n01 n10 n11) and is phased when min_link of them are
    informative and min_agree of those lie on its majority side (cis or trans); phased links chain sites into blocks with a phase
    bit per site, and every row gets hap_a / hap_b / other counts per block.  Writes out_sites (contig, pos, ref, alt, depth,
    ref_count, alt_count, block, phase) and, when given, out_links (contig, pos1, pos2, n00, n01, n10, n11, informative, agree,
    phased) and out_reads (read, contig, block, spanned, hap_a, hap_b, other, hap).  Options: those of api.variants, min_link 3,
    min_agree 0.8.  A function of this project's own: include/hylight_mi.h states it, tests/phase_model.py is its contract.
    -> dict of the stats (hlmi_phase_stats)."""
    o, st = _phase_opts("phase", opts), PhaseStats()
    _check(load().hlmi_phase(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_sites), _b(out_links), _b(out_reads),
                             C.byref(st)))
    return {k: getattr(st, k) for k in PHASE_STATS + POLISH_MS}


def phase_reads(contigs, reads, out_sites, out_links=None, out_reads=None, ava_opts=None, pairs=None, **opts):
    """hlmi_phase_reads: `ava(contigs, reads, P, ava_opts)` and `phase(contigs, reads, P, ...)` in one call without the PAF P: the
    same files and the same integer stats.  ava_opts None: the long constants.  Refused besides what phase refuses:
    ava_opts.stub_oh >= 0.  -> dict of the stats (hlmi_phase_stats)."""
    o, st = _phase_opts("phase_reads", opts), PhaseStats()
    _check(load().hlmi_phase_reads(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o), _b(pairs),
                                   _b(out_sites), _b(out_links), _b(out_reads), C.byref(st)))
    return {k: getattr(st, k) for k in PHASE_STATS + POLISH_MS}


def _phase_reach_stats(st):
    out = {k: getattr(st.base, k) for k in PHASE_STATS + POLISH_MS}
    out.update({k: getattr(st, k) for k in PHASE_REACH_STATS})
    return out


def phase_reach(contigs, reads, paf, out_sites, out_links=None, out_reads=None, pairs=None, reach=1, **opts):
    """hlmi_phase_reach: api.phase with links between sites up to `reach` (1 .. PHASE_REACH_MAX) apart, so that one noisy site does
    not cut a block.  Sites, selection and alleles are api.phase's; every pair of sites (i, i + d), d <= reach, of a contig has a
    link under api.phase's link rule; a site joins the block in front of it through the nearest member within reach that has a
    phased link to it; a site inside a block that did not join is bridged: its block's id, phase ".", counted in a record's
    spanned alone.  out_links has one line per link of any distance.  With reach 1 the files and the shared stats are
    api.phase's.  include/hylight_mi.h states it, tests/phase_reach_model.py is its contract.
    -> dict of the stats (hlmi_phase_reach_stats: api.phase's keys, links_far, links_far_phased, joins_far, sites_bridged,
    links_conflict)."""
    o, st = _phase_opts("phase_reach", opts), PhaseReachStats()
    _check(load().hlmi_phase_reach(_b(contigs), _b(reads), _b(paf), C.byref(o), int(reach), _b(pairs), _b(out_sites), _b(out_links),
                                   _b(out_reads), C.byref(st)))
    return _phase_reach_stats(st)


def phase_reads_reach(contigs, reads, out_sites, out_links=None, out_reads=None, ava_opts=None, pairs=None, reach=1, **opts):
    """hlmi_phase_reads_reach: `ava(contigs, reads, P, ava_opts)` and `phase_reach(contigs, reads, P, ...)` in one call without the
    PAF P, as phase_reads is for phase.  -> dict of the stats (hlmi_phase_reach_stats)."""
    o, st = _phase_opts("phase_reads_reach", opts), PhaseReachStats()
    _check(load().hlmi_phase_reads_reach(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o), int(reach),
                                         _b(pairs), _b(out_sites), _b(out_links), _b(out_reads), C.byref(st)))
    return _phase_reach_stats(st)


def _phase_ins_stats(st):
    out = _phase_reach_stats(st.reach)
    out.update({k: getattr(st, k) for k in PHASE_INS_STATS})
    return out


def phase_ins(contigs, reads, paf, out_sites, out_links=None, out_reads=None, pairs=None, reach=1, **opts):
    """hlmi_phase_ins: api.phase_reach over the merged list of api.variants's position sites and the insertion sites of
    api.variants_ins that take part (len >= 1 and len_count >= min_alt); slot p sorts directly in front of position p.  At an
    insertion site a row that spans the slot reads 0 if it inserts nothing there, 1 if it inserts the site's called length (by
    length alone), 2 for any other length.  Links, blocks, bridged sites and read records are api.phase_reach's over the merged
    list.  An insertion site's line has pos = p, the base in front of the slot, alt "+" and the called bases; a slot endpoint of a
    link, and the id of a block that starts at an insertion site, carry a trailing "+".  Where no insertion site takes part the
    files and the shared stats are api.phase_reach's.  include/hylight_mi.h states it, tests/phase_ins_model.py is its contract.
    -> dict of the stats (hlmi_phase_ins_stats: api.phase_reach's keys, slots_callable, ins_sites, ins_long, ins_edge,
    ins_sites_phasing, ins_sites_left_out, ins_sites_phased)."""
    o, st = _phase_opts("phase_ins", opts), PhaseInsStats()
    _check(load().hlmi_phase_ins(_b(contigs), _b(reads), _b(paf), C.byref(o), int(reach), _b(pairs), _b(out_sites), _b(out_links),
                                 _b(out_reads), C.byref(st)))
    return _phase_ins_stats(st)


def phase_reads_ins(contigs, reads, out_sites, out_links=None, out_reads=None, ava_opts=None, pairs=None, reach=1, **opts):
    """hlmi_phase_reads_ins: `ava(contigs, reads, P, ava_opts)` and `phase_ins(contigs, reads, P, ...)` in one call without the PAF
    P, as phase_reads_reach is for phase_reach.  -> dict of the stats (hlmi_phase_ins_stats)."""
    o, st = _phase_opts("phase_reads_ins", opts), PhaseInsStats()
    _check(load().hlmi_phase_reads_ins(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o), int(reach),
                                       _b(pairs), _b(out_sites), _b(out_links), _b(out_reads), C.byref(st)))
    return _phase_ins_stats(st)


def _haplotig_opts(who, opts):
    o = HaplotigOpts()
    load().hlmi_haplotig_opts_default(C.byref(o))
    for k, v in opts.items():
        if k not in dict(HaplotigOpts._fields_):
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, v)
    return o


def _haplotig_stats(st):
    out = {k: getattr(st.phase, k) for k in PHASE_STATS}
    out.update({k: getattr(st, k) for k in HAPLOTIG_STATS + POLISH_MS})
    return out


def haplotigs(contigs, reads, paf, out_fa, out_blocks=None, pairs=None, **opts):
    """hlmi_haplotigs: the contigs polished as api.polish polishes them, once per side of every phased block the reads split.  The
    phasing is api.phase's (same selection, pairs= included, sites, links, blocks, every row's side per block).  A block of two or
    more sites is split when min_side of its rows read side A and min_side side B; inside its extent [first site, last site] a row
    votes only on its own side, everywhere else on both.  A contig with a split block gives two records (name_hapA, name_hapB with
    HB:i: split blocks and HP:i: positions inside them), every other contig api.polish's record byte for byte.  Writes out_fa and,
    when given, out_blocks (contig, block, start, end, sites, rows_a, rows_b, split, diff_positions).  Options: those of api.phase,
    min_side 3, include_unpolished 1.  A function of this project's own: include/hylight_mi.h states it, tests/haplotigs_model.py
    is its contract.  -> dict of the stats (hlmi_haplotig_stats, the phasing's integer stats among them)."""
    o, st = _haplotig_opts("haplotigs", opts), HaplotigStats()
    _check(load().hlmi_haplotigs(_b(contigs), _b(reads), _b(paf), C.byref(o), _b(pairs), _b(out_fa), _b(out_blocks), C.byref(st)))
    return _haplotig_stats(st)


def haplotigs_reads(contigs, reads, out_fa, out_blocks=None, ava_opts=None, pairs=None, **opts):
    """hlmi_haplotigs_reads: `ava(contigs, reads, P, ava_opts)` and `haplotigs(contigs, reads, P, ...)` in one call without the PAF
    P: the same files and the same integer stats.  ava_opts None: the long constants.  Refused besides what haplotigs refuses:
    ava_opts.stub_oh >= 0.  -> dict of the stats (hlmi_haplotig_stats)."""
    o, st = _haplotig_opts("haplotigs_reads", opts), HaplotigStats()
    _check(load().hlmi_haplotigs_reads(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o), _b(pairs),
                                       _b(out_fa), _b(out_blocks), C.byref(st)))
    return _haplotig_stats(st)


def haplotigs_reach(contigs, reads, paf, out_fa, out_blocks=None, pairs=None, reach=1, **opts):
    """hlmi_haplotigs_reach: api.haplotigs over the blocks of api.phase_reach (reach 1 .. PHASE_REACH_MAX): a block's extent runs
    from its first to its last site, bridged sites included; a row's side comes from its record.  With reach 1 it is
    api.haplotigs byte for byte.  tests/haplotigs_reach_model.py is its contract.  -> dict of the stats (hlmi_haplotig_stats)."""
    o, st = _haplotig_opts("haplotigs_reach", opts), HaplotigStats()
    _check(load().hlmi_haplotigs_reach(_b(contigs), _b(reads), _b(paf), C.byref(o), int(reach), _b(pairs), _b(out_fa), _b(out_blocks),
                                       C.byref(st)))
    return _haplotig_stats(st)


def haplotigs_reads_reach(contigs, reads, out_fa, out_blocks=None, ava_opts=None, pairs=None, reach=1, **opts):
    """hlmi_haplotigs_reads_reach: `ava(contigs, reads, P, ava_opts)` and `haplotigs_reach(contigs, reads, P, ...)` in one call
    without the PAF P.  -> dict of the stats (hlmi_haplotig_stats)."""
    o, st = _haplotig_opts("haplotigs_reads_reach", opts), HaplotigStats()
    _check(load().hlmi_haplotigs_reads_reach(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                             int(reach), _b(pairs), _b(out_fa), _b(out_blocks), C.byref(st)))
    return _haplotig_stats(st)


def _haplotig_ins_stats(st):
    out = _haplotig_stats(st.base)
    out.update({k: getattr(st, k) for k in HAPLOTIG_INS_STATS})        # ins_long and ins_edge: the same values as base's
    return out


def haplotigs_ins(contigs, reads, paf, out_fa, out_blocks=None, pairs=None, reach=1, **opts):
    """hlmi_haplotigs_ins: api.haplotigs_reach over the blocks of api.phase_ins, whose first or last site may be an insertion site.
    A block's extent lies in key space (slot p: 2 p, position p: 2 p + 1) and runs from the key of its first site to the key of its
    last: one that starts at an insertion site shuts the other side's rows out of that slot too, one that ends at slot p shuts them
    out of slot p and not out of position p.  An insertion site inside a split block is decided per side: two strains that differ
    by insertions alone give name_hapA and name_hapB.  out_blocks has a tenth column, diff_slots (slots inside the extent whose
    opened length differs between the sides); block, start and end carry a trailing "+" at an insertion site.  Where no insertion
    site takes part out_fa and the shared stats are api.haplotigs_reach's.  include/hylight_mi.h states it,
    tests/haplotigs_ins_model.py is its contract.  -> dict of the stats (hlmi_haplotig_ins_stats: api.haplotigs_reach's keys, the
    seven insertion counters of api.phase_ins, diff_slots)."""
    o, st = _haplotig_opts("haplotigs_ins", opts), HaplotigInsStats()
    _check(load().hlmi_haplotigs_ins(_b(contigs), _b(reads), _b(paf), C.byref(o), int(reach), _b(pairs), _b(out_fa), _b(out_blocks),
                                     C.byref(st)))
    return _haplotig_ins_stats(st)


def haplotigs_reads_ins(contigs, reads, out_fa, out_blocks=None, ava_opts=None, pairs=None, reach=1, **opts):
    """hlmi_haplotigs_reads_ins: `ava(contigs, reads, P, ava_opts)` and `haplotigs_ins(contigs, reads, P, ...)` in one call without
    the PAF P.  -> dict of the stats (hlmi_haplotig_ins_stats)."""
    o, st = _haplotig_opts("haplotigs_reads_ins", opts), HaplotigInsStats()
    _check(load().hlmi_haplotigs_reads_ins(_b(contigs), _b(reads), C.byref(ava_opts) if ava_opts is not None else None, C.byref(o),
                                           int(reach), _b(pairs), _b(out_fa), _b(out_blocks), C.byref(st)))
    return _haplotig_ins_stats(st)


DEVICE = "cuda"          # where the buffers that cross the C ABI live (stage.py allocates them with torch)


class Job:
    """Staged stage run for the multi-GPU path (sketch shard -> all-gather -> run)."""

    def __init__(self, reads_fa, ref_fa, nsplit, long_mode=True):
        self._h = load().hlmi_job_open(_b(reads_fa), _b(ref_fa), nsplit, int(long_mode))
        if not self._h:
            raise HlmiError(-1, load().hlmi_last_error().decode(errors="replace"))

    def close(self):
        if self._h and _lib is not None:
            _lib.hlmi_job_close(self._h)
        self._h = None

    def __del__(self):          # at interpreter shutdown module globals may already be gone
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_queries(self):
        return load().hlmi_job_num_queries(self._h)

    @property
    def num_chunks(self):
        return load().hlmi_job_num_chunks(self._h)

    def sketch_bound(self, lo, hi):
        return load().hlmi_job_sketch_bound(self._h, lo, hi)

    def sketch(self, lo, hi, dev_mz_ptr, cap, dev_counts_ptr):
        n = C.c_int64(0)
        _check(load().hlmi_job_sketch(self._h, lo, hi, dev_mz_ptr, cap, dev_counts_ptr, C.byref(n)))
        return n.value

    def sketch_own(self):
        _check(load().hlmi_job_sketch_own(self._h))

    def set_query_sketch(self, dev_mz_ptr, n, dev_counts_ptr):
        _check(load().hlmi_job_set_query_sketch(self._h, dev_mz_ptr, n, dev_counts_ptr))

    def run(self, rank, world, len_over, mc, iden, out_paf):
        _check(load().hlmi_job_run(self._h, rank, world, len_over, mc, iden, _b(out_paf)))
