"""MI355X-native REO pair-comparison engine behind RankCompV3's identify_degs().

The directory name carries a dot, so import it through `__graft_entry__.load_pkg()`
(or add an alias with importlib); see INTEGRATION.md.
"""
from . import _ffi, dist, synth  # noqa: F401
from ._ffi import Context, DimensionMismatch, LibraryMissing, PairList, PairSupport, PermNull, ReoError, SampleCalls, SampleCounts, SampleScores, SampleTests, TopPairs, TopPairsLoo, TopPairsNull, TopPartners, TopPartnersNull, build_library, permuted_labels, permuted_sides, threshold  # noqa: F401
from .hotpath import (HEADER, CellsDegRun, DegRun, cells_partition, encode_groups, identify_degs, identify_degs_cells,  # noqa: F401
                      label_genes, parse_contrasts, run_identify_degs, write_pair_support_tsv, write_pairs_tsv, write_perm_null_tsv, write_perm_summary_tsv, write_sample_calls_tsv, write_sample_scores_tsv, write_top_pairs_cv_tsv, write_top_pairs_loo_tsv, write_top_pairs_null_tsv, write_top_pairs_tsv, write_top_partners_null_tsv, write_top_partners_tsv)
from .reoa import ArgumentError, reoa  # noqa: F401

__all__ = ["Context", "DimensionMismatch", "LibraryMissing", "ReoError", "build_library", "threshold", "HEADER",
           "DegRun", "CellsDegRun", "cells_partition", "identify_degs_cells", "encode_groups", "identify_degs", "label_genes", "run_identify_degs", "synth", "dist", "reoa", "ArgumentError", "PairList", "write_pairs_tsv", "SampleCounts", "SampleScores", "write_sample_scores_tsv", "PairSupport", "write_pair_support_tsv", "parse_contrasts", "SampleTests", "write_sample_calls_tsv", "SampleCalls", "PermNull", "permuted_labels", "write_perm_null_tsv", "write_perm_summary_tsv", "TopPairs", "write_top_pairs_tsv", "TopPairsNull", "permuted_sides", "write_top_pairs_null_tsv", "TopPairsLoo", "write_top_pairs_cv_tsv", "write_top_pairs_loo_tsv", "TopPartners", "write_top_partners_tsv", "TopPartnersNull", "write_top_partners_null_tsv"]
