"""Haplotigs on the GPU (hlmi_haplotigs): the contigs polished once per side of every phased block the reads split - two consensus
sequences where `python -m hylight_amd.phase` proves two sides, `python -m hylight_amd.polish`'s bytes everywhere else.  A function
of the project's own (include/hylight_mi.h states the rules, tests/haplotigs_model.py is their contract); selection, sites and
phasing are hlmi_phase's, votes and decisions hlmi_polish's.

    python -m hylight_amd.haplotigs --contigs contigs.fa --reads reads.fa --paf rows.paf --out haplotigs.fa [--blocks F]
    python -m hylight_amd.haplotigs --contigs contigs.fa --reads reads.fa --out haplotigs.fa [--short] [options]

--paf holds rows with a cg:Z: CIGAR in = X I D as the last field, reads against contigs, as `api.ava(contigs, reads, paf)`
writes them.  Without --paf the reads are aligned to the contigs in the same call (hlmi_haplotigs_reads: the overlapper's long
constants, --short: its short-read ones; every pair, pair_once = 0) and no PAF exists.
--pairs FILE lets only the rows vote whose (read, contig) pair a row of FILE names, as for the phase module.
--out: FASTA - a contig with a split block as name_hapA and name_hapB (HB:i: split blocks, HP:i: positions inside them; the sides
of different blocks are independent of each other), every other contig as the polish module writes it; --blocks: one line per
block of two or more sites (contig, block, start, end, sites, rows_a, rows_b, split, diff_positions).  Prints the stats as one
JSON line.  Exit status 0 on success.
--reach K (2 .. 8; hlmi_haplotigs_reach): the blocks of `python -m hylight_amd.phase --reach K`, whose extents cover their bridged
sites.  The default 1 is the call without it.
--ins (hlmi_haplotigs_ins; honours --reach): the blocks of `python -m hylight_amd.phase --ins`, in which insertion sites are
phasing evidence: a block may begin or end at an insertion site (block, start, end then carry a trailing +), a slot inside a
split block is opened on the side whose rows insert, and --blocks has a tenth column, diff_slots.
"""
from __future__ import annotations

import argparse
import json
import sys

from . import api
from .polish import read_ava_opts


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.haplotigs", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--contigs", required=True, help="FASTA / FASTQ of the contigs")
    p.add_argument("--reads", required=True, help="FASTA / FASTQ of the reads")
    p.add_argument("--paf", default=None,
                   help="rows of reads (query) against contigs (target) with cg:Z: CIGARs; not given: align here, write none")
    p.add_argument("--pairs", default=None, metavar="FILE",
                   help="PAF-like list (fields 1 and 6): only rows of a listed (read, contig) pair vote (not given: every row may)")
    p.add_argument("--out", required=True, help="the haplotigs and the other contigs (FASTA)")
    p.add_argument("--blocks", default=None, metavar="F", help="one line per block of two or more sites (TSV; not given: not written)")
    p.add_argument("--short", action="store_true", help="without --paf: the overlapper's short-read constants")
    p.add_argument("--min_len", type=int, default=0, help="drop rows that cover fewer contig bases")
    p.add_argument("--min_iden", type=float, default=0.0, help="drop rows with a smaller share of '=' columns")
    p.add_argument("--min_cov", type=int, default=3, help="votes a position needs to be decided, and to be callable")
    p.add_argument("--min_alt", type=int, default=2, help="votes the alternative symbol needs")
    p.add_argument("--min_frac", type=float, default=0.2, help="share of the position's votes the alternative symbol needs")
    p.add_argument("--min_link", type=int, default=3, help="informative rows a link needs")
    p.add_argument("--min_agree", type=float, default=0.8, help="share of the informative rows on the link's majority side")
    p.add_argument("--min_side", type=int, default=3, help="rows a block needs on either side to be split")
    p.add_argument("--include_unpolished", type=int, default=1, choices=(0, 1), help="write contigs without a selected row as they are")
    p.add_argument("--reach", type=int, default=1, metavar="K", help="link sites up to K sites apart (1: neighbours alone; at most 8)")
    p.add_argument("--ins", action="store_true", help="insertion sites take part in the phasing and are decided per side")
    return p


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    opts = dict(min_len=a.min_len, min_iden=a.min_iden, min_cov=a.min_cov, min_alt=a.min_alt, min_frac=a.min_frac, min_link=a.min_link,
                min_agree=a.min_agree, min_side=a.min_side, include_unpolished=a.include_unpolished)
    if a.paf is not None:
        if a.short:
            parser.error("--short chooses the alignment of a call without --paf")
        if a.ins:
            st = api.haplotigs_ins(a.contigs, a.reads, a.paf, a.out, a.blocks, pairs=a.pairs, reach=a.reach, **opts)
        elif a.reach != 1:
            st = api.haplotigs_reach(a.contigs, a.reads, a.paf, a.out, a.blocks, pairs=a.pairs, reach=a.reach, **opts)
        else:
            st = api.haplotigs(a.contigs, a.reads, a.paf, a.out, a.blocks, pairs=a.pairs, **opts)
    elif a.ins:
        st = api.haplotigs_reads_ins(a.contigs, a.reads, a.out, a.blocks, read_ava_opts(a.short), pairs=a.pairs, reach=a.reach, **opts)
    elif a.reach != 1:
        st = api.haplotigs_reads_reach(a.contigs, a.reads, a.out, a.blocks, read_ava_opts(a.short), pairs=a.pairs, reach=a.reach, **opts)
    else:
        st = api.haplotigs_reads(a.contigs, a.reads, a.out, a.blocks, read_ava_opts(a.short), pairs=a.pairs, **opts)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
