"""ViralQuasispecies --cliques=false for HyLight's stage b: the overlap graph of a SAVAGE
overlaps file and the super-reads merged along its edges, built by libhylight_mi.so (hlmi_vq_merge).

    python -m hylight_amd.vq_merge --singles singles.fastq --overlaps sfoverlap.out.savage --out DIR [options]

Writes what python -m hylight_amd.vq_graph writes, and singles.fastq, subreads.txt, removed_tip_sequences.fastq (appended
to, as the reference does) and superread_map.txt.  Options keep the reference's names (ViralQuasispecies.cpp:55-100); the
defaults are what HyLight's first stage-b iteration passes (pipeline_per_stage.py:170-203).  With --first_it false,
--subreads names the previous iteration's subreads.txt.  --min_qual X (0 .. 1) is the reference's flag of that name; it is not
passed by default, which leaves minQual at 0.9.  Prints {"graph": ..., "merge": ...} as one JSON line.  Exit status 0
on success, 4 (EXIT_REFUSED) for what vq_graph refuses and for --cliques true, --error_correction true.
"""
from __future__ import annotations

import json
import sys

from . import api
from .vq_graph import EXIT_REFUSED, _bool, build_parser as graph_parser, exit_status, not_built


def build_parser():
    p = graph_parser()
    p.prog = "python -m hylight_amd.vq_merge"
    p.description = __doc__.split("\n\n")[0]
    p.add_argument("--subreads", default=None, help="subreads.txt of the previous iteration (with --first_it false)")
    p.add_argument("--first_it", type=_bool, default=True)
    p.add_argument("--keep_singletons", type=int, default=300)
    p.add_argument("--separate_tips", type=_bool, default=True)
    p.add_argument("--min_clique_size", type=int, default=2)
    p.add_argument("--min_qual", type=float, default=None, help="0 .. 1 (default: not passed, minQual 0.9)")
    p.add_argument("--cliques", type=_bool, default=False, help="refused when true")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    if not_built("vq_merge", a, more=((a.cliques, "--cliques true"), (a.error_correction, "--error_correction true"))):
        return EXIT_REFUSED
    try:
        gst, mst = api.vq_merge(a.singles, a.overlaps, a.out, subreads_in=a.subreads, min_overlap_len=a.min_overlap_len,
                                min_overlap_perc=a.min_overlap_perc, min_read_len=a.min_read_len,
                                edge_threshold=a.edge_threshold, ov_threshold=a.ov_threshold,
                                merge_contigs=a.merge_contigs, mismatch=a.mismatch, max_tip_len=a.max_tip_len,
                                remove_trans=a.remove_trans, remove_branches=a.remove_branches,
                                remove_tips=a.remove_tips, ignore_inclusions=a.ignore_inclusions, remove_backedges=True,
                                max_overlaps=a.max_ov, first_it=a.first_it, keep_singletons=a.keep_singletons,
                                store_tips_separately=a.separate_tips, min_clique_size=a.min_clique_size,
                                min_qual=a.min_qual)
    except api.HlmiError as e:
        return exit_status("vq_merge", e)
    print(json.dumps({"graph": gst, "merge": mst}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
