"""Variant sites per contig on the GPU (hlmi_variants): the positions of the contigs where a second symbol has real support among
the reads aligned to them - a collapsed strain, a mis-join or a polishing error - and how many each contig has.  A function of
the project's own (include/hylight_mi.h states the rules, tests/variants_model.py is their contract); the reads are selected as
the polisher selects them, one row per read, and vote as its position votes do, unweighted.

    python -m hylight_amd.variants --contigs contigs.fa --reads reads.fa --paf rows.paf --out sites.tsv [--summary contigs.tsv]
    python -m hylight_amd.variants --contigs contigs.fa --reads reads.fa --out sites.tsv [--short] [options]

--paf holds rows with a cg:Z: CIGAR in = X I D as the last field, reads against contigs, as `api.ava(contigs, reads, paf)`
writes them.  Without --paf the reads are aligned to the contigs in the same call (hlmi_variants_reads: the overlapper's long
constants, --short: its short-read ones; every pair, pair_once = 0) and no PAF exists.
--pairs FILE lets only the rows vote whose (read, contig) pair a row of FILE names (a PAF-like list, fields 1 and 6, either
order - with the overlap stage's filtered rows a read votes only on the contig the SNP filter paired it with, and the sister
strain's alleles no longer show as sites).
--out: the sites (contig, pos, ref, depth, A, C, G, T, del, alt, alt_count, alt_frac); --summary: one line per contig (contig,
length, reads, callable, sites, site_rate).  Prints the stats as one JSON line.  Exit status 0 on success.
--ins FILE: the insertion sites too (hlmi_variants_ins / hlmi_variants_reads_ins) - the slots where rows that insert bases the
contig lacks number --min_alt and make --min_frac of the --min_cov or more rows that span the slot (contig, pos, ref, span, ins,
ins_long, ins_frac, len, len_count, seq); --out stays the same file, --summary gains slots, ins_sites and ins_rate.
--min_base_qual N / --min_avg_qual X: base qualities take part (hlmi_variants_q and its _reads and _ins forms) - a column whose
Phred is below N casts no vote, as an N column casts none, and the rows of a read whose mean Phred is below X are dropped; the
counts stay counts of reads.  Giving either selects the _q call; without both the calls above are made.  FASTA records pass.
"""
from __future__ import annotations

import argparse
import json
import sys

from . import api
from .polish import read_ava_opts


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.variants", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--contigs", required=True, help="FASTA / FASTQ of the contigs")
    p.add_argument("--reads", required=True, help="FASTA / FASTQ of the reads")
    p.add_argument("--paf", default=None,
                   help="rows of reads (query) against contigs (target) with cg:Z: CIGARs; not given: align here, write none")
    p.add_argument("--pairs", default=None, metavar="FILE",
                   help="PAF-like list (fields 1 and 6): only rows of a listed (read, contig) pair vote (not given: every row may)")
    p.add_argument("--out", required=True, help="the sites, one line each (TSV)")
    p.add_argument("--summary", default=None, help="one line per contig (TSV; not given: not written)")
    p.add_argument("--ins", default=None, metavar="FILE",
                   help="also the insertion sites, one line each (TSV; hlmi_variants_ins; not given: insertions take no part)")
    p.add_argument("--short", action="store_true", help="without --paf: the overlapper's short-read constants")
    p.add_argument("--min_len", type=int, default=0, help="drop rows that cover fewer contig bases")
    p.add_argument("--min_iden", type=float, default=0.0, help="drop rows with a smaller share of '=' columns")
    p.add_argument("--min_cov", type=int, default=3, help="votes a position needs to be callable")
    p.add_argument("--min_alt", type=int, default=2, help="votes the alternative symbol needs")
    p.add_argument("--min_frac", type=float, default=0.2, help="share of the position's votes the alternative symbol needs")
    p.add_argument("--min_base_qual", type=int, default=None, metavar="N",
                   help="a column whose Phred is below N (0..93) casts no vote (hlmi_variants_q and its forms; 0: off; given alone, "
                        "--min_avg_qual is 0; neither given: base qualities take no part)")
    p.add_argument("--min_avg_qual", type=float, default=None, metavar="X",
                   help="drop the rows of a read whose mean Phred is below X, as the polisher's --min_avg_qual does (0: off; given "
                        "alone, --min_base_qual is 0)")
    return p


def main(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    opts = dict(min_len=a.min_len, min_iden=a.min_iden, min_cov=a.min_cov, min_alt=a.min_alt, min_frac=a.min_frac)
    if a.paf is not None and a.short:
        parser.error("--short chooses the alignment of a call without --paf")
    if a.min_base_qual is not None or a.min_avg_qual is not None:       # either selects the _q call, with or without --ins
        opts.update(min_base_qual=a.min_base_qual or 0, min_avg_qual=a.min_avg_qual or 0.0)
        if a.ins is not None and a.paf is not None:
            st = api.variants_ins_q(a.contigs, a.reads, a.paf, a.out, a.ins, a.summary, pairs=a.pairs, **opts)
        elif a.ins is not None:
            st = api.variants_ins_reads_q(a.contigs, a.reads, a.out, a.ins, a.summary, read_ava_opts(a.short), pairs=a.pairs, **opts)
        elif a.paf is not None:
            st = api.variants_q(a.contigs, a.reads, a.paf, a.out, a.summary, pairs=a.pairs, **opts)
        else:
            st = api.variants_reads_q(a.contigs, a.reads, a.out, a.summary, read_ava_opts(a.short), pairs=a.pairs, **opts)
    elif a.ins is not None:
        if a.paf is not None:
            st = api.variants_ins(a.contigs, a.reads, a.paf, a.out, a.ins, a.summary, pairs=a.pairs, **opts)
        else:
            st = api.variants_ins_reads(a.contigs, a.reads, a.out, a.ins, a.summary, read_ava_opts(a.short), pairs=a.pairs, **opts)
    elif a.paf is not None:
        st = api.variants(a.contigs, a.reads, a.paf, a.out, a.summary, pairs=a.pairs, **opts)
    else:
        st = api.variants_reads(a.contigs, a.reads, a.out, a.summary, read_ava_opts(a.short), pairs=a.pairs, **opts)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
