"""Read depth and relative abundance per contig on the GPU (hlmi_depth): how many reads lie over every position of the contigs
and each contig's share of the sample.  A function of the project's own (include/hylight_mi.h states the rules,
tests/depth_model.py is their contract); the reads are selected as the polisher selects them, one row per read.

    python -m hylight_amd.depth --contigs contigs.fa --reads reads.fa --paf rows.paf --out depth.tsv [--bedgraph depth.bedgraph]
    python -m hylight_amd.depth --contigs contigs.fa --reads reads.fa --out depth.tsv [--short] [options]

--paf holds rows with a cg:Z: CIGAR in = X I D as the last field, reads against contigs, as `api.ava(contigs, reads, paf)`
writes them.  Without --paf the reads are aligned to the contigs in the same call (hlmi_depth_reads: the overlapper's long
constants, --short: its short-read ones; every pair, pair_once = 0) and no PAF exists.
--pairs FILE lets only the rows count whose (read, contig) pair a row of FILE names (a PAF-like list, fields 1 and 6, either
order - with the overlap stage's filtered rows a read counts only on the contig the SNP filter paired it with).
--out: the table (contig, length, reads, bases, covered, mean_depth, median_depth, abundance); --bedgraph: the runs of equal
depth.  Prints the stats as one JSON line.  Exit status 0 on success.
"""
from __future__ import annotations

import argparse
import json
import sys

from . import api
from .polish import read_ava_opts


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.depth", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--contigs", required=True, help="FASTA / FASTQ of the contigs")
    p.add_argument("--reads", required=True, help="FASTA / FASTQ of the reads")
    p.add_argument("--paf", default=None,
                   help="rows of reads (query) against contigs (target) with cg:Z: CIGARs; not given: align here, write none")
    p.add_argument("--pairs", default=None, metavar="FILE",
                   help="PAF-like list (fields 1 and 6): only rows of a listed (read, contig) pair count (not given: every row may)")
    p.add_argument("--out", required=True, help="the table, one line per contig (TSV)")
    p.add_argument("--bedgraph", default=None, help="the runs of equal depth (bedGraph; not given: not written)")
    p.add_argument("--short", action="store_true", help="without --paf: the overlapper's short-read constants")
    p.add_argument("--min_len", type=int, default=0, help="drop rows that cover fewer contig bases")
    p.add_argument("--min_iden", type=float, default=0.0, help="drop rows with a smaller share of '=' columns")
    return p


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    opts = dict(min_len=a.min_len, min_iden=a.min_iden)
    if a.paf is not None:
        if a.short:
            parser.error("--short chooses the alignment of a call without --paf")
        st = api.depth(a.contigs, a.reads, a.paf, a.out, a.bedgraph, pairs=a.pairs, **opts)
    else:
        st = api.depth_reads(a.contigs, a.reads, a.out, a.bedgraph, read_ava_opts(a.short), pairs=a.pairs, **opts)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
