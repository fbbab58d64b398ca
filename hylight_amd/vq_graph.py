"""ViralQuasispecies --graph_only=true for HyLight's stage b: the oriented, reduced overlap
graph of a SAVAGE overlaps file, built by libhylight_mi.so (hlmi_vq_graph).

    python -m hylight_amd.vq_graph --singles singles.fastq --overlaps sfoverlap.out.savage --out DIR [options]

Options keep the reference's names (ViralQuasispecies.cpp:55-100); the defaults are what HyLight's first stage-b iteration
passes (HyLight.py:320-324 -> pipeline_per_stage.py:170-200).  Booleans take true / false (also 1 / 0, yes / no, on / off).
Prints the stats as one JSON line.  Exit status 0 on success, 4 (EXIT_REFUSED) for a setting that is not on HyLight's path
and that this implementation refuses: --add_duplicates true, --resolve_orientations false, --branch_reduction true,
--remove_branches true with --remove_trans other than 1, and an overlaps file whose edge candidates involve paired-end
reads.
"""
from __future__ import annotations

import argparse
import json
import sys

from . import api

EXIT_REFUSED = 4


def _bool(s):
    v = str(s).strip().lower()
    if v in ("1", "true", "yes", "on"):
        return True
    if v in ("0", "false", "no", "off"):
        return False
    raise argparse.ArgumentTypeError(f"not a boolean: {s!r}")


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.vq_graph", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--singles", "-s", required=True, help="single-end reads (FASTQ); vertex = position in the file")
    p.add_argument("--overlaps", required=True, help="13-column SAVAGE overlaps file")
    p.add_argument("--out", "--output", "-O", dest="out", required=True, help="output directory")
    p.add_argument("--min_overlap_len", type=int, default=300)
    p.add_argument("--min_overlap_perc", type=int, default=0)
    p.add_argument("--min_read_len", type=int, default=0)
    p.add_argument("--edge_threshold", type=float, default=1.0)
    p.add_argument("--ov_threshold", type=float, default=0.9)
    p.add_argument("--merge_contigs", type=float, default=0.0)
    p.add_argument("--mismatch", type=float, default=0.0)
    p.add_argument("--max_tip_len", type=int, default=1000)
    p.add_argument("--remove_trans", type=int, default=1, choices=[0, 1, 2, 3])
    p.add_argument("--remove_branches", type=_bool, default=True)
    p.add_argument("--remove_tips", type=_bool, default=True)
    p.add_argument("--ignore_inclusions", type=_bool, default=True)
    p.add_argument("--error_correction", type=_bool, default=False, help="true: keep the back edges of the cycle search")
    p.add_argument("--max_ov", type=int, default=100000000, help="maximum number of overlap lines read")
    p.add_argument("--add_duplicates", type=_bool, default=False, help="refused when true")
    p.add_argument("--resolve_orientations", type=_bool, default=True, help="refused when false")
    p.add_argument("--branch_reduction", type=_bool, default=False, help="refused when true")
    return p


def not_built(prog, a, more=(), tail="is not on HyLight's path and is not built"):
    """Names the refused settings of the arguments `a` (`more`: a step's own (set, name) pairs) on stderr -> True if any."""
    refused = [msg for bad, msg in ((a.add_duplicates, "--add_duplicates true"), (not a.resolve_orientations, "--resolve_orientations false"),
                                    (a.branch_reduction, "--branch_reduction true"), *more) if bad]
    if refused:
        sys.stderr.write(f"hylight_amd.{prog}: {', '.join(refused)} {tail}\n")
    return bool(refused)


def exit_status(prog, e, invalid=None):
    """api.HlmiError -> EXIT_REFUSED for HLMI_ESTATE (-6: not on HyLight's path), `invalid` (if given) for HLMI_EINVAL (-1),
    with the message on stderr; anything else is raised again."""
    if e.code != -6 and (e.code != -1 or invalid is None):
        raise e
    sys.stderr.write(f"hylight_amd.{prog}: {e}\n")
    return EXIT_REFUSED if e.code == -6 else invalid


def main(argv=None):
    a = build_parser().parse_args(argv)
    if not_built("vq_graph", a):
        return EXIT_REFUSED
    try:
        st = api.vq_graph(a.singles, a.overlaps, a.out, min_overlap_len=a.min_overlap_len,
                          min_overlap_perc=a.min_overlap_perc, min_read_len=a.min_read_len,
                          edge_threshold=a.edge_threshold, ov_threshold=a.ov_threshold, merge_contigs=a.merge_contigs,
                          mismatch=a.mismatch, max_tip_len=a.max_tip_len, remove_trans=a.remove_trans,
                          remove_branches=a.remove_branches, remove_tips=a.remove_tips,
                          ignore_inclusions=a.ignore_inclusions, remove_backedges=not a.error_correction,
                          max_overlaps=a.max_ov)
    except api.HlmiError as e:
        return exit_status("vq_graph", e)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
