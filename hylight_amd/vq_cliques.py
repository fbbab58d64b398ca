"""ViralQuasispecies --cliques=true for single-end reads: the overlap graph of a SAVAGE overlaps
file, its maximal cliques and one super-read per clique, built by libhylight_mi.so (hlmi_vq_cliques) - the step POLYTE runs in
the first iteration of every cluster.

    python -m hylight_amd.vq_cliques --singles singles.fastq --overlaps overlaps.txt --out DIR [--error_correction true]
        [--min_clique_size N] [--edge_threshold X] [--min_overlap_len N] [--keep_singletons N] [--subreads F]
        [--min_qual X] [--iteration [--no_inclusion_overlaps true]]

Writes what python -m hylight_amd.vq_graph writes, and cliques.txt (as the reference's enumerator prints it), singles.fastq,
subreads.txt and clique_map.txt.  The defaults are what POLYTE's run_viralquasispecies passes (polyte.tune_params.py:684-738):
with --error_correction true remove_trans 2, the back edges kept, keep_singletons 1000; without it remove_trans 1,
remove_branches true, keep_singletons 0; tips and inclusions stay either way.  One of its options is not a default here:
--min_qual 0 ("never insert N's", :737).  Without the flag minQual stays at ViralQuasispecies' own default 0.9, and a column
whose best base is less than 90 % sure becomes N; with `--min_qual 0 --iteration` the run is a POLYTE first-iteration call.  The
loop around such calls is python -m hylight_amd.polyte.  With --iteration the run goes on to the end of
ViralQuasispecies' main (hlmi_vq_clique_iteration, --FNO=1): overlaps.txt and one line appended to stats.txt, so that another
iteration can follow; the inputs may then lie in DIR under the names written.  Prints {"graph": ..., "cliques": ...} - with
--iteration also "next": ... - as one JSON line.  Exit status 0 on success, 4 (EXIT_REFUSED) for what vq_graph refuses (a
paired-end row among them), 2 (EXIT_INVALID) for a malformed input or a --min_clique_size outside 1 .. 21.
"""
from __future__ import annotations

import json
import sys

from . import api
from .vq_graph import EXIT_REFUSED, _bool, build_parser as graph_parser, exit_status, not_built

EXIT_INVALID = 2


def build_parser():
    p = graph_parser()
    p.prog = "python -m hylight_amd.vq_cliques"
    p.description = __doc__.split("\n\n")[0]
    p.set_defaults(remove_trans=None, remove_branches=None, remove_tips=False, ignore_inclusions=False)
    p.add_argument("--subreads", default=None, help="subreads.txt of the previous iteration (with --first_it false)")
    p.add_argument("--first_it", type=_bool, default=True)
    p.add_argument("--keep_singletons", type=int, default=None, help="default: 1000 with --error_correction true, else 0")
    p.add_argument("--min_clique_size", type=int, default=2)
    p.add_argument("--min_qual", type=float, default=None, help="0 .. 1; POLYTE passes 0 (default: not passed, minQual 0.9)")
    p.add_argument("--iteration", action="store_true", help="go on to findNextOverlaps: overlaps.txt and the stats.txt line")
    p.add_argument("--no_inclusion_overlaps", type=_bool, default=False, help="with --iteration: leave out the lines with percentage 100")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    if not_built("vq_cliques", a, tail="is not built"):
        return EXIT_REFUSED
    ec = bool(a.error_correction)
    polyte = api.vq_clique_opts_polyte(ec)
    opts = dict(subreads_in=a.subreads, min_overlap_len=a.min_overlap_len,
                min_overlap_perc=a.min_overlap_perc, min_read_len=a.min_read_len,
                edge_threshold=a.edge_threshold, ov_threshold=a.ov_threshold, merge_contigs=a.merge_contigs,
                mismatch=a.mismatch, max_tip_len=a.max_tip_len,
                remove_trans=(2 if ec else 1) if a.remove_trans is None else a.remove_trans,
                remove_branches=(not ec) if a.remove_branches is None else a.remove_branches,
                remove_tips=a.remove_tips, ignore_inclusions=a.ignore_inclusions, remove_backedges=not ec,
                max_overlaps=a.max_ov, error_correction=ec, first_it=a.first_it,
                keep_singletons=polyte["keep_singletons"] if a.keep_singletons is None else a.keep_singletons,
                min_clique_size=a.min_clique_size, min_qual=a.min_qual)
    try:
        if a.iteration:
            gst, cst, nst = api.vq_clique_iteration(a.singles, a.overlaps, a.out, no_inclusion_overlaps=a.no_inclusion_overlaps, **opts)
            result = {"graph": gst, "cliques": cst, "next": nst}
        else:
            gst, cst = api.vq_cliques(a.singles, a.overlaps, a.out, **opts)
            result = {"graph": gst, "cliques": cst}
    except api.HlmiError as e:
        return exit_status("vq_cliques", e, invalid=EXIT_INVALID)   # HLMI_EINVAL: malformed input, min_clique_size
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
