"""Pile-up consensus polishing of contigs on the GPU (hlmi_polish): the native stand-in for the `racon --no-trimming -u`
calls of HyLight.py:152,182,203.  Not racon's function - a column vote over the CIGARs of the project's own overlapper
(include/hylight_mi.h states the rules, tests/polish_model.py is their contract).

    python -m hylight_amd.polish --contigs contigs.fa --reads reads.fa --paf rows.paf --out polished.fa [options]

--paf holds rows with a cg:Z: CIGAR in = X I D as the last field, reads against contigs, as `api.ava(contigs, reads, paf)`
writes them.  Prints the stats as one JSON line.  Exit status 0 on success.
"""
from __future__ import annotations

import argparse
import json
import sys

from . import api


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.polish", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--contigs", required=True, help="FASTA / FASTQ of the contigs to polish")
    p.add_argument("--reads", required=True, help="FASTA / FASTQ of the reads the rows name")
    p.add_argument("--paf", required=True, help="rows of reads (query) against contigs (target) with cg:Z: CIGARs")
    p.add_argument("--out", required=True, help="polished contigs (FASTA, two lines per record)")
    p.add_argument("--min_len", type=int, default=0, help="drop rows that cover fewer contig bases")
    p.add_argument("--min_iden", type=float, default=0.0, help="drop rows with a smaller share of '=' columns")
    p.add_argument("--min_cov", type=int, default=3, help="votes a position needs, rows a slot needs")
    p.add_argument("--drop_unpolished", action="store_true", help="leave out contigs no row was selected on")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    st = api.polish(a.contigs, a.reads, a.paf, a.out, min_len=a.min_len, min_iden=a.min_iden, min_cov=a.min_cov,
                    include_unpolished=not a.drop_unpolished)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
