"""Phased variant sites on the GPU (hlmi_phase): the variant sites of `python -m hylight_amd.variants` with what the reads say about
their neighbours - links between consecutive sites (do the minor alleles ride on the same reads?), blocks of sites chained by
phased links with a phase bit each, and for every read the side it reads per block.  A function of the project's own
(include/hylight_mi.h states the rules, tests/phase_model.py is their contract); sites, selection and votes are hlmi_variants's.

    python -m hylight_amd.phase --contigs contigs.fa --reads reads.fa --paf rows.paf --out sites.tsv [--links F] [--read-haps F]
    python -m hylight_amd.phase --contigs contigs.fa --reads reads.fa --out sites.tsv [--short] [options]

--paf holds rows with a cg:Z: CIGAR in = X I D as the last field, reads against contigs, as `api.ava(contigs, reads, paf)`
writes them.  Without --paf the reads are aligned to the contigs in the same call (hlmi_phase_reads: the overlapper's long
constants, --short: its short-read ones; every pair, pair_once = 0) and no PAF exists.
--pairs FILE lets only the rows vote whose (read, contig) pair a row of FILE names, as for the variants module.
--out: the sites (contig, pos, ref, alt, depth, ref_count, alt_count, block, phase); --links: one line per pair of consecutive
sites (contig, pos1, pos2, n00, n01, n10, n11, informative, agree, phased); --read-haps: one line per read and block (read, contig,
block, spanned, hap_a, hap_b, other, hap).  Prints the stats as one JSON line.  Exit status 0 on success.
--reach K (2 .. 8; hlmi_phase_reach) also links sites up to K sites apart, so that one noisy site does not cut a block: a site
inside a block that joined nothing is bridged (its block's id, phase "."), --links has one line per link of any distance.  The
default 1 is the call without it.
--ins (hlmi_phase_ins, with --reach K as well) adds the insertion sites of `python -m hylight_amd.variants --ins` whose called length
has --min_alt rows as phasing evidence: a site line with pos of the base in front, alt "+" and the called bases; a slot endpoint of
a link and the id of a block that starts at an insertion site carry a trailing "+".  Without --ins the module calls what it called.
"""
from __future__ import annotations

import argparse
import json
import sys

from . import api
from .polish import read_ava_opts


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.phase", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--contigs", required=True, help="FASTA / FASTQ of the contigs")
    p.add_argument("--reads", required=True, help="FASTA / FASTQ of the reads")
    p.add_argument("--paf", default=None,
                   help="rows of reads (query) against contigs (target) with cg:Z: CIGARs; not given: align here, write none")
    p.add_argument("--pairs", default=None, metavar="FILE",
                   help="PAF-like list (fields 1 and 6): only rows of a listed (read, contig) pair vote (not given: every row may)")
    p.add_argument("--out", required=True, help="the sites with their block and phase, one line each (TSV)")
    p.add_argument("--links", default=None, metavar="F", help="one line per pair of consecutive sites (TSV; not given: not written)")
    p.add_argument("--read-haps", dest="read_haps", default=None, metavar="F",
                   help="one line per read and block (TSV; not given: not written)")
    p.add_argument("--short", action="store_true", help="without --paf: the overlapper's short-read constants")
    p.add_argument("--min_len", type=int, default=0, help="drop rows that cover fewer contig bases")
    p.add_argument("--min_iden", type=float, default=0.0, help="drop rows with a smaller share of '=' columns")
    p.add_argument("--min_cov", type=int, default=3, help="votes a position needs to be callable")
    p.add_argument("--min_alt", type=int, default=2, help="votes the alternative symbol needs")
    p.add_argument("--min_frac", type=float, default=0.2, help="share of the position's votes the alternative symbol needs")
    p.add_argument("--min_link", type=int, default=3, help="informative rows a link needs")
    p.add_argument("--min_agree", type=float, default=0.8, help="share of the informative rows on the link's majority side")
    p.add_argument("--reach", type=int, default=1, metavar="K", help="link sites up to K sites apart (1: neighbours alone; at most 8)")
    p.add_argument("--ins", action="store_true", help="insertion sites as phasing evidence (hlmi_phase_ins; --reach applies)")
    return p


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    opts = dict(min_len=a.min_len, min_iden=a.min_iden, min_cov=a.min_cov, min_alt=a.min_alt, min_frac=a.min_frac, min_link=a.min_link,
                min_agree=a.min_agree)
    if a.paf is not None:
        if a.short:
            parser.error("--short chooses the alignment of a call without --paf")
        if a.ins:
            st = api.phase_ins(a.contigs, a.reads, a.paf, a.out, a.links, a.read_haps, pairs=a.pairs, reach=a.reach, **opts)
        elif a.reach != 1:
            st = api.phase_reach(a.contigs, a.reads, a.paf, a.out, a.links, a.read_haps, pairs=a.pairs, reach=a.reach, **opts)
        else:
            st = api.phase(a.contigs, a.reads, a.paf, a.out, a.links, a.read_haps, pairs=a.pairs, **opts)
    elif a.ins:
        st = api.phase_reads_ins(a.contigs, a.reads, a.out, a.links, a.read_haps, read_ava_opts(a.short), pairs=a.pairs, reach=a.reach, **opts)
    elif a.reach != 1:
        st = api.phase_reads_reach(a.contigs, a.reads, a.out, a.links, a.read_haps, read_ava_opts(a.short), pairs=a.pairs, reach=a.reach, **opts)
    else:
        st = api.phase_reads(a.contigs, a.reads, a.out, a.links, a.read_haps, read_ava_opts(a.short), pairs=a.pairs, **opts)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
