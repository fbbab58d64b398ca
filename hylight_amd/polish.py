"""Pile-up consensus polishing of contigs on the GPU (hlmi_polish): the native stand-in for the `racon --no-trimming -u`
calls of HyLight.py:152,182,203.  Not racon's function - a column vote over the CIGARs of the project's own overlapper
(include/hylight_mi.h states the rules, tests/polish_model.py is their contract).

    python -m hylight_amd.polish --contigs contigs.fa --reads reads.fa --paf rows.paf --out polished.fa [options]
    python -m hylight_amd.polish --contigs contigs.fa --reads reads.fa --out polished.fa [--short] [options]

--paf holds rows with a cg:Z: CIGAR in = X I D as the last field, reads against contigs, as `api.ava(contigs, reads, paf)`
writes them.  Without --paf the reads are aligned to the contigs in the same call (hlmi_polish_reads: the overlapper's long
constants, --short: its short-read ones; every pair, pair_once = 0, as the driver's polishing sites do) and no PAF exists.
--qual_weight weighs every vote by the read base's Phred quality and --min_avg_qual Q drops the rows of reads whose mean quality
is below Q (hlmi_polish_q / hlmi_polish_reads_q; FASTQ reads - a FASTA read's bases weigh 1 and it is never dropped).
--pairs FILE lets only the rows vote whose (read, contig) pair a row of FILE names (hlmi_polish_pairs / hlmi_polish_reads_pairs:
a PAF-like list, fields 1 and 6, either order - the overlap stage's filtered rows make the polisher strain-aware).
Prints the stats as one JSON line.  Exit status 0 on success.
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
    p.add_argument("--paf", default=None,
                   help="rows of reads (query) against contigs (target) with cg:Z: CIGARs; not given: align here, write none")
    p.add_argument("--short", action="store_true", help="without --paf: the overlapper's short-read constants")
    p.add_argument("--out", required=True, help="polished contigs (FASTA, two lines per record)")
    p.add_argument("--min_len", type=int, default=0, help="drop rows that cover fewer contig bases")
    p.add_argument("--min_iden", type=float, default=0.0, help="drop rows with a smaller share of '=' columns")
    p.add_argument("--min_cov", type=int, default=3, help="votes a position needs, rows a slot needs")
    p.add_argument("--drop_unpolished", action="store_true", help="leave out contigs no row was selected on")
    p.add_argument("--qual_weight", action="store_true", help="weigh votes by the reads' base qualities (FASTQ reads)")
    p.add_argument("--min_avg_qual", type=float, default=None, metavar="Q",
                   help="drop rows of reads whose mean Phred quality is below Q (racon -q; not given: no such test)")
    p.add_argument("--pairs", default=None, metavar="FILE",
                   help="PAF-like list (fields 1 and 6): only rows of a listed (read, contig) pair vote (not given: every row may)")
    return p


def read_ava_opts(short=False):
    """The overlapper's options of a polishing site: long or short constants, every pair (driver.polish_native)."""
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    return o


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    opts = dict(min_len=a.min_len, min_iden=a.min_iden, min_cov=a.min_cov, include_unpolished=not a.drop_unpolished)
    if a.qual_weight:
        opts["qual_weight"] = 1
    if a.min_avg_qual is not None:
        opts["min_avg_qual"] = a.min_avg_qual
    if a.pairs is not None:
        opts["pairs"] = a.pairs
    if a.paf is not None:
        if a.short:
            parser.error("--short chooses the alignment of a call without --paf")
        st = api.polish(a.contigs, a.reads, a.paf, a.out, **opts)
    else:
        st = api.polish_reads(a.contigs, a.reads, a.out, read_ava_opts(a.short), **opts)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
