"""ViralQuasispecies --branch_reduction=true for single-end reads: the overlap graph of a SAVAGE overlaps
file with its branches reduced by read evidence (BranchReduction::readBasedBranchReduction), built by libhylight_mi.so
(hlmi_vq_branch_graph) - the iteration POLYTE runs after every merge round (polyte.tune_params.py:641-645).

    python -m hylight_amd.vq_branches --singles singles.fastq --overlaps overlaps.txt --out DIR --branch_reduction true
        --original_fastq original.fastq --branch_SE_c N --branch_PE_c M --thresholds evidence_threshold_table.tsv
        [--careful_diploid true] [--subreads subreads.txt --first_it false] [--iteration [clique options, --min_qual X]]

Writes what python -m hylight_amd.vq_graph writes, and branch_components.txt.  The flags carry the reference's names;
--thresholds names the table the reference reads from its working directory.  The defaults are POLYTE's for this iteration:
remove_trans 1, remove_branches false, tips and inclusions kept, the cliques without error correction.  With --iteration the run
goes on through the clique step to the end of ViralQuasispecies' main (hlmi_vq_branch_iteration); --min_qual 0 there is what
POLYTE passes (not passed by default: minQual 0.9).  Not built, and said so: --diploid (the typical-double-branch resolution), paired-end vertices.  POLYTE's loop is
python -m hylight_amd.polyte, its threshold table hylight_amd/min_ev.py.  Prints {"graph": ..., "branches": ...} - with --iteration also "cliques" and "next" - as one JSON line.
Exit status 0 on success, 4 (EXIT_REFUSED) for what is refused as not built (a paired-end row, --remove_trans other than 1,
--remove_branches true, --branch_reduction false, --diploid true), 2 (EXIT_INVALID) for a malformed input: counts that do not
match --original_fastq, a table that cannot be read, an original the FASTQ does not hold.
"""
from __future__ import annotations

import json
import sys

from . import api
from .vq_cliques import EXIT_INVALID, build_parser as cliques_parser
from .vq_graph import EXIT_REFUSED, _bool, exit_status


def build_parser():
    p = cliques_parser()
    p.prog = "python -m hylight_amd.vq_branches"
    p.description = __doc__.split("\n\n")[0]
    p.set_defaults(remove_trans=1, remove_branches=False, branch_reduction=True)
    p.add_argument("--original_fastq", required=True, help="the original reads the subreads name, looked up by id")
    p.add_argument("--branch_SE_c", type=int, required=True, help="original single-end reads")
    p.add_argument("--branch_PE_c", type=int, default=0, help="original read pairs (ids: singles, /1 mates, /2 mates)")
    p.add_argument("--thresholds", required=True, help="evidence_threshold_table.tsv: column 1 distance, column 3 minimum evidence")
    p.add_argument("--careful_diploid", type=_bool, default=True, help="remove a component next to a kept one")
    p.add_argument("--diploid", type=_bool, default=False, help="refused when true")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    refused = [msg for bad, msg in ((a.add_duplicates, "--add_duplicates true"), (not a.resolve_orientations, "--resolve_orientations false"),
                                    (not a.branch_reduction, "--branch_reduction false (python -m hylight_amd.vq_cliques runs without it)"),
                                    (a.remove_trans != 1, "--remove_trans other than 1"), (a.remove_branches, "--remove_branches true"),
                                    (a.diploid, "--diploid true")) if bad]
    if refused:
        sys.stderr.write(f"hylight_amd.vq_branches: {', '.join(refused)} is not built\n")
        return EXIT_REFUSED
    if a.branch_SE_c < 0 or a.branch_PE_c < 0 or max(a.branch_SE_c, a.branch_PE_c) >= 1 << 32:
        sys.stderr.write("hylight_amd.vq_branches: --branch_SE_c / --branch_PE_c out of range\n")
        return EXIT_INVALID
    ec = bool(a.error_correction)
    polyte = api.vq_clique_opts_polyte(ec)
    opts = dict(subreads_in=None if a.first_it else a.subreads, min_overlap_len=a.min_overlap_len,
                min_overlap_perc=a.min_overlap_perc, min_read_len=a.min_read_len, edge_threshold=a.edge_threshold,
                ov_threshold=a.ov_threshold, merge_contigs=a.merge_contigs, mismatch=a.mismatch, max_tip_len=a.max_tip_len,
                remove_trans=1, remove_branches=False, remove_tips=a.remove_tips, ignore_inclusions=a.ignore_inclusions,
                remove_backedges=not ec, max_overlaps=a.max_ov, se_count=a.branch_SE_c, pe_count=a.branch_PE_c,
                careful=a.careful_diploid)
    if a.min_qual is not None and not a.iteration:
        sys.stderr.write("hylight_amd.vq_branches: --min_qual belongs to the clique step: it needs --iteration\n")
        return EXIT_INVALID
    if not a.first_it and a.subreads is None:
        sys.stderr.write("hylight_amd.vq_branches: --first_it false needs --subreads\n")
        return EXIT_INVALID
    try:
        if a.iteration:
            gst, bst, cst, nst = api.vq_branch_iteration(
                a.singles, a.overlaps, a.original_fastq, a.thresholds, a.out, no_inclusion_overlaps=a.no_inclusion_overlaps,
                error_correction=ec, first_it=a.first_it, min_clique_size=a.min_clique_size,
                keep_singletons=polyte["keep_singletons"] if a.keep_singletons is None else a.keep_singletons,
                min_qual=a.min_qual, **opts)
            result = {"graph": gst, "branches": bst, "cliques": cst, "next": nst}
        else:
            gst, bst = api.vq_branch_graph(a.singles, a.overlaps, a.original_fastq, a.thresholds, a.out, **opts)
            result = {"graph": gst, "branches": bst}
    except api.HlmiError as e:
        return exit_status("vq_branches", e, invalid=EXIT_INVALID)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
