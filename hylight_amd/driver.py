"""Counterpart of the reference driver for the long-read path.

Keeps script/HyLight.py's CLI flags and defaults (HyLight.py:25-52), stage order and output tree
(OUT/1.split_fastx/s1.fa, OUT/2.overlap/s1_s1.paf, OUT/tmp/contigs1.{gfa,fa}, OUT/tmp/ov_long_ref.paf,
...), and calls libhylight_mi.so at the two boundaries the path owns: B1 = split_reads2 and
B3 = miniasm.  External tools the reference shells out to (bfc, ropebwt2, fmlrc2, racon) are still
external (`--polish_native` replaces racon with the library's own pile-up consensus, hlmi_polish, and `--polish_direct` does
the same without the PAF between overlapper and polisher, hlmi_polish_reads); unlike the reference (whose `execute()` swallows most failures) a missing or
failing tool stops the run with a message.  The two short-read overlap calls of the path (HyLight.py:200,207)
run in the library's short mode.  `extend_con` (HyLight.py:282-326) is wired up to the SAVAGE overlap file: contigs ->
contigs_b.fastq -> self-overlaps (the `minimap2 --sr -X ... -r 0` call as hlmi_ava) -> v3 window filter with -sfo ->
sfo2overlaps; the stage-b contig merge (pipeline_per_stage.py / ViralQuasispecies) that reads that file is opt-in (`--stageb_native`): without
`--stageb_cmd` the run says so on stderr and, because the contractual output final_contigs.fa was not written, exits
with EXIT_NO_FINAL (3) and everything up to tmp/stageb/sfoverlap.out.savage in place (`--stop_after savage` declares
that partial run and exits 0).  The text passes (filter_non_atcg, gfa2fa, pick_up) are the library's native ones.

The short-read branch (HyLight.py:211-275) is opt-in: `--stop_after clusters` runs the clustering of HyLight.py:215-226
(hlmi_cluster_short: readnames.txt, the grouped JSON and fq_<size>/ in tmp/) and exits 0; `--polyte_cmd PREFIX`, without
`--short_contigs`, also runs POLYTE per cluster through PREFIX (the reference's polyte.tune_params.py, external), collects
tmp/all.contigs_<size>.fasta, extends it into short_stageb.fa (with `--stageb_cmd`) and builds all_contigs.fa from it and
long_con_polished.fa.  Without these flags the run is the same as before.  `--polyte_native` takes the place of `--polyte_cmd`
with the library's own POLYTE (hylight_amd.polyte: the loop of polyte.tune_params.py, its threshold table, every iteration and
every overlap computation a library call; HyLight's copy of the script treats the mates as single reads, so no paired-end
vertices are needed), one cluster after the other in this process; `--polyte_cmd` itself is untouched, and both together are an
error.  `--polyte_workers W` (extension) deals the clusters out, largest first, to W processes per GPU (this one and W - 1 fresh
interpreters, hylight_amd/polyte_pool.py) and, under `--gpus N`, to the N ranks as well (StagePool.polyte): the reference's
`xargs -i -P threads` over cmd_polyte.sh (HyLight.py:245).  A cluster's files do not depend on who ran it.
`--stageb_native` keeps minQual 0.9: pipeline_per_stage.py does not pass the flag.

`--gpus N` (extension): every split_reads2 call is sharded over N GPUs of the node, chunk i -> rank i % N, the way the
reference fans its chunks out with `xargs -P` (script/utils.py:44-69).  The process starts N - 1 further copies of
itself before it touches the GPU (hylight_amd/launch.py); rank 0 runs the pipeline (text passes, graph builds, external
tools, merges), the other ranks only take part in the stage calls (stage.py:StagePool).  Started under torchrun
(RANK / WORLD_SIZE in the environment) it uses the ranks it was given.
"""
from __future__ import annotations

import argparse
import os
import shutil
import subprocess
import sys
import time

from . import api, launch
from .stage import StagePool

__version__ = "1.0.1-mi355x"
MAX_GPU_PROCESSES = 16   # --gpus x --polyte_workers: shared machines allow this many processes with a GPU open
EXIT_NO_FINAL = 3        # everything this implementation covers ran, but final_contigs.fa (the stage-b merge) was not written


def fq_or_fa(path):
    """toolkits.fq_or_fa (script/toolkits.py:7-18): first character decides."""
    with open(path) as f:
        c = f.read(1)
    if c == "@":
        return "fastq"
    if c == ">":
        return "fasta"
    raise SystemExit(f"{path}: neither FASTQ nor FASTA")


def filter_non_atcg(fq, out_dir, model):
    """utils.filter_non_atcg (script/utils.py:81-114): upper-case, [^ATGCN] -> N, header cut at the first
    space; 4-line FASTQ / 2-line FASTA records.  The pass itself is hlmi_filter_non_atcg."""
    new_dir = os.path.join(out_dir, "1.split_fastx")
    os.makedirs(new_dir, exist_ok=True)
    return api.filter_non_atcg(fq, os.path.join(new_dir, "s1.fa"), model)


def gfa2fa(gfa, fa):
    """HyLight.gfa2fa (script/HyLight.py:328-337): S lines only (hlmi_gfa2fa)."""
    api.gfa2fa(gfa, fa)


def pick_up(ovlap, outdir, fq):
    """HyLight.pick_up (script/HyLight.py:347-378): reads whose name (up to the first '/') appears in
    neither column 1 nor column 6 of the PAF (hlmi_pick_up); the output name follows the reference.  When every
    read overlaps, the reference leaves no file behind - callers get the path either way."""
    out = os.path.join(outdir, "sub" + str(time.time())[-3:] + "_remain.fq")
    return api.pick_up(ovlap, fq, out, fq_or_fa(fq))


def _tool(name):
    p = shutil.which(name)
    if not p:
        raise SystemExit(f"external tool `{name}` (README.md:14-19 of the reference) is not on PATH")
    return p


def _run(cmd, cwd=None):
    r = subprocess.run(cmd, shell=True, cwd=cwd, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print(f"Error executing the command: {cmd}\n{r.stderr}", file=sys.stderr)
        raise SystemExit(1)


def contig_ava_opts():
    """minimap2 -t T --sr -X -c -k 21 -w 11 -s 60 -m 30 -n 2 -r 0 -A 4 -B 2 --end-bonus=100 (HyLight.py:309-310): the
    short-read constants, each pair once and never a contig against itself (-X), chaining bandwidth 0 (-r 0)."""
    o = api.ava_opts_short()
    o.pair_once = 1
    o.bandwidth = 0
    return o


def extend_con(input_con, outdir1, out_file, threads=30, len_c=50000000, stageb_cmd=None, stageb_graph=False, stageb_merge=False,
               stageb_native=False):
    """HyLight.extend_con (script/HyLight.py:282-326) up to the SAVAGE overlap file.  Returns the number of contigs
    written to contigs_b.fastq.  `stageb_cmd`: command prefix of the reference's stage-b script
    (`python .../pipeline_per_stage.py`) for installations that have it; without it the merge itself is skipped.
    `stageb_graph`: also build the overlap graph of the first stage-b iteration (ViralQuasispecies --graph_only,
    hlmi_vq_graph with the stage-b options) into outdir1/stageb/ - graph.gfa, graph.txt, graph_trimmed.gfa,
    digraph.txt, cycles.txt, tips.txt, nonedge_overlaps.txt.  `stageb_merge`: that graph and the super-reads merged along
    its edges (ViralQuasispecies --cliques=false up to findNextOverlaps, hlmi_vq_merge with the stage-b options) -
    singles.fastq, subreads.txt, removed_tip_sequences.fastq, superread_map.txt in outdir1/stageb/.  `stageb_native`: the
    whole stage-b loop in outdir1/stageb/ (hylight_amd.vq_stageb) and out_file from its last singles.fastq."""
    conb = os.path.join(outdir1, "contigs_b.fastq")
    if os.path.exists(conb):
        os.remove(conb)
    n = 0
    if os.path.exists(input_con):                              # HyLight.py:289-305: every sequence LINE longer than 150
        with open(input_con) as f, open(conb, "a") as w:
            for line in f:
                line = line.strip()
                if line.startswith(">"):
                    continue
                if len(line) > 150:
                    n += 1
                    w.write(f"@{n}\n{line}\n+\n{'=' * len(line)}\n")
    sb = os.path.join(outdir1, "stageb")
    os.makedirs(os.path.join(sb, "fastq"), exist_ok=True)
    raw, sfo, savage = os.path.join(sb, "contigs_ava.paf"), os.path.join(sb, "sfoverlaps.out"), os.path.join(sb, "sfoverlap.out.savage")
    if n:
        api.ava(conb, conb, raw, contig_ava_opts())
        api.paf_window_filter(3, raw, sfo, min_len=90, min_iden=0.99, min_o=2, sfo=True)      # HyLight.py:310-311
        api.sfo2overlaps(sfo, savage, num_singles=n, num_pairs=0)                              # HyLight.py:315-317
        shutil.copyfile(conb, os.path.join(sb, "fastq", "singles.fastq"))
    else:
        for p in (raw, sfo, savage):
            open(p, "w").close()
    if stageb_merge and n:
        api.vq_merge(os.path.join(sb, "fastq", "singles.fastq"), savage, sb)
    elif stageb_graph and n:
        api.vq_graph(os.path.join(sb, "fastq", "singles.fastq"), savage, sb)
    if stageb_native and n:                                    # HyLight.py:320-324 with the library's own stage b
        from . import vq_stageb
        vq_stageb.run(os.path.join(sb, "fastq"), savage, sb)
        merged = os.path.join(sb, "singles.fastq")             # absent when no two contigs overlap: they are the result
        vq_stageb.fastq2fasta(merged if os.path.exists(merged) else os.path.join(sb, "fastq", "singles.fastq"), out_file)
        return n
    if stageb_cmd and n:                                       # HyLight.py:320-324
        _run(f"{stageb_cmd} --no_error_correction --remove_branches true --stage b --min_overlap_len 300 "
             f"--min_overlap_perc 0 --edge_threshold 1 --overlaps ./sfoverlap.out.savage --fastq ./fastq --max_tip_len 1000 "
             f"--len_c {len_c} --num_threads {threads}", cwd=sb)
        singles = os.path.join(sb, "singles.fastq")
        with open(singles) as f, open(out_file, "w") as o:     # fastq2fasta.py
            for k, line in enumerate(f):
                if k % 4 == 0:
                    o.write(">" + line[1:])
                elif k % 4 == 1:
                    o.write(line)
    return n


def polish_native(k, reads, contigs, out_fa, tmp, min_len, iden, short=False, append=False, direct=False, qual=None, pairs=None):
    """One racon site with the library's own polisher (`--polish_native`): the reads are aligned to the contigs once more
    (hlmi_ava, every pair: the stage's scored PAF carries no CIGAR) into tmp/polish_<k>.paf, and hlmi_polish votes over those
    rows.  `direct` (`--polish_direct`): both in one call (hlmi_polish_reads) with the same options - the same file, and no
    tmp/polish_<k>.paf.  `append`: out_fa grows, as the `>>` of HyLight.py:182 does.  `qual` (`--polish_qual`): the read floor Q -
    votes weighted by base quality and rows of reads below mean quality Q dropped (hlmi_polish_q / hlmi_polish_reads_q).  `pairs`
    (`--polish_strain`): the stage's filtered PAF of this site - only its (read, contig) pairs vote (hlmi_polish_pairs /
    hlmi_polish_reads_pairs), as racon only ever sees those rows in the reference."""
    popts = dict(min_len=min_len, min_iden=iden)
    if qual is not None:
        popts.update(qual_weight=1, min_avg_qual=qual)
    if pairs is not None:
        popts.update(pairs=pairs)
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    part = out_fa + ".part" if append else out_fa
    if direct:
        st = api.polish_reads(contigs, reads, part, o, **popts)
    else:
        paf = os.path.join(tmp, f"polish_{k}.paf")
        api.ava(contigs, reads, paf, o)
        st = api.polish(contigs, reads, paf, part, **popts)
    if append:
        with open(part, "rb") as f, open(out_fa, "ab") as w:
            shutil.copyfileobj(f, w)
        os.remove(part)
    return st


def depth_tables(final, long_reads, short_reads, outdir, device=None):
    """`--depth`: read depth and relative abundance of the final contigs (hlmi_depth_reads: the reads are aligned to the contigs
    in the call, every pair, one row per read).  The long reads - the filtered ones the overlap stage read - with the
    overlapper's long constants give outdir/final_contigs.long.depth.tsv and .bedgraph; short reads, when there are any, with
    the short constants give final_contigs.short.depth.tsv and .bedgraph.  `device`: the GPU to initialise the library on
    (None: the caller has done so).  -> {"long": stats, "short": stats}."""
    if device is not None:
        api.init(device)
    out = {}
    for kind, reads in (("long", long_reads), ("short", short_reads)):
        if not reads:
            continue
        o = api.ava_opts_short() if kind == "short" else api.ava_opts_long()
        o.pair_once = 0
        stem = os.path.join(outdir, f"final_contigs.{kind}.depth")
        out[kind] = api.depth_reads(final, reads, stem + ".tsv", stem + ".bedgraph", o)
    return out


def variant_tables(final, long_reads, short_reads, outdir, device=None, long_pairs=None, short_pairs=None, ins=False, qual=None):
    """`--variants`: the variant sites of the final contigs (hlmi_variants_reads: the reads are aligned to the contigs in the
    call, every pair, one row per read) - is each contig one strain?  The long reads - the filtered ones the overlap stage read -
    with the overlapper's long constants give outdir/final_contigs.long.variants.tsv and .long.variants.summary.tsv; short reads,
    when there are any, with the short constants give the .short. pair.  long_pairs / short_pairs (`--polish_strain`: the run's
    ov_long_ref.paf / shortr1.paf): only the (read, contig) pairs the list names vote; a list row whose names this call does not
    know counts in pairs_unknown.  `device`: the GPU to initialise the library on (None: the caller has done so).
    ins (`--variants_ins`): hlmi_variants_reads_ins takes the call's place - the same two files (the summary with three columns
    more) and the insertion sites in .variants.ins.tsv beside them; still one call per read set.
    qual (`--variants_qual`): dict(min_base_qual=, min_avg_qual=) - the _q form of either call takes its place, the file names
    stay; FASTA reads pass every floor (the identity), FASTQ reads are where it bites.
    -> {"long": stats, "short": stats}."""
    if device is not None:
        api.init(device)
    out = {}
    for kind, reads, pairs in (("long", long_reads, long_pairs), ("short", short_reads, short_pairs)):
        if not reads:
            continue
        o = api.ava_opts_short() if kind == "short" else api.ava_opts_long()
        o.pair_once = 0
        stem = os.path.join(outdir, f"final_contigs.{kind}.variants")
        if qual is not None and ins:
            out[kind] = api.variants_ins_reads_q(final, reads, stem + ".tsv", stem + ".ins.tsv", stem + ".summary.tsv", o, pairs=pairs, **qual)
        elif qual is not None:
            out[kind] = api.variants_reads_q(final, reads, stem + ".tsv", stem + ".summary.tsv", o, pairs=pairs, **qual)
        elif ins:
            out[kind] = api.variants_ins_reads(final, reads, stem + ".tsv", stem + ".ins.tsv", stem + ".summary.tsv", o, pairs=pairs)
        else:
            out[kind] = api.variants_reads(final, reads, stem + ".tsv", stem + ".summary.tsv", o, pairs=pairs)
    return out


def variants_qual_args(args):
    """`--variants_qual` as variant_tables takes it (nothing without the flag: the calls made before it existed are made)"""
    if not args.variants_qual:
        return {}
    return {"qual": dict(min_base_qual=args.variants_min_base_qual, min_avg_qual=args.variants_min_avg_qual)}


def phase_tables(final, long_reads, short_reads, outdir, device=None, long_pairs=None, short_pairs=None, reach=1, ins=False):
    """`--phase`: the variant sites of the final contigs phased from the reads (hlmi_phase_reads: the reads are aligned to the
    contigs in the call, every pair, one row per read).  The long reads with the overlapper's long constants give
    outdir/final_contigs.long.phase.sites.tsv, .links.tsv and .reads.tsv; short reads, when there are any, with the short
    constants give the .short. triple.  long_pairs / short_pairs: as for variant_tables.  `device`: the GPU to initialise the
    library on (None: the caller has done so).  reach (`--phase_reach`) above 1: hlmi_phase_reads_reach, links between sites up to
    `reach` apart.  ins (`--phase_ins`): hlmi_phase_reads_ins takes the call's place at any reach - the same three files with the
    insertion sites that take part among the sites.  -> {"long": stats, "short": stats}."""
    if device is not None:
        api.init(device)
    out = {}
    for kind, reads, pairs in (("long", long_reads, long_pairs), ("short", short_reads, short_pairs)):
        if not reads:
            continue
        o = api.ava_opts_short() if kind == "short" else api.ava_opts_long()
        o.pair_once = 0
        stem = os.path.join(outdir, f"final_contigs.{kind}.phase")
        files = (stem + ".sites.tsv", stem + ".links.tsv", stem + ".reads.tsv")
        out[kind] = (api.phase_reads_ins(final, reads, *files, o, pairs=pairs, reach=reach) if ins else
                     api.phase_reads(final, reads, *files, o, pairs=pairs) if reach == 1 else
                     api.phase_reads_reach(final, reads, *files, o, pairs=pairs, reach=reach))
    return out


def haplotig_files(final, long_reads, short_reads, outdir, device=None, long_pairs=None, short_pairs=None, reach=1, ins=False):
    """`--haplotigs`: the final contigs polished once per side of every phased block the reads split (hlmi_haplotigs_reads: the
    reads are aligned to the contigs in the call, every pair, one row per read).  The long reads with the overlapper's long
    constants give outdir/final_contigs.long.haplotigs.fa and .long.haplotigs.blocks.tsv; short reads, when there are any, with
    the short constants give the .short. pair.  long_pairs / short_pairs: as for phase_tables.  `device`: the GPU to initialise
    the library on (None: the caller has done so).  reach (`--phase_reach`) above 1: hlmi_haplotigs_reads_reach.  ins
    (`--haplotigs_ins`): hlmi_haplotigs_reads_ins takes the call's place at any reach - the same two files over the blocks of
    `--phase_ins`, the blocks file with its tenth column.  -> {"long": stats, "short": stats}."""
    if device is not None:
        api.init(device)
    out = {}
    for kind, reads, pairs in (("long", long_reads, long_pairs), ("short", short_reads, short_pairs)):
        if not reads:
            continue
        o = api.ava_opts_short() if kind == "short" else api.ava_opts_long()
        o.pair_once = 0
        stem = os.path.join(outdir, f"final_contigs.{kind}.haplotigs")
        out[kind] = (api.haplotigs_reads_ins(final, reads, stem + ".fa", stem + ".blocks.tsv", o, pairs=pairs, reach=reach) if ins else
                     api.haplotigs_reads(final, reads, stem + ".fa", stem + ".blocks.tsv", o, pairs=pairs) if reach == 1 else
                     api.haplotigs_reads_reach(final, reads, stem + ".fa", stem + ".blocks.tsv", o, pairs=pairs, reach=reach))
    return out


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.driver",
                                description="Haplotype-aware de novo assembly of metagenome from hybrid sequencing data "
                                            "(long reads, short reads) - MI355X long-read path",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("-s", "--short_reads", dest="short_reads", type=str, required=False)
    p.add_argument("-l", "--long_reads", dest="long_reads", type=str, required=True)
    p.add_argument("-o", "--outdir", dest="outdir", type=str, default="./")
    p.add_argument("-t", "--threads", dest="threads", type=int, default=20)
    p.add_argument("--corrected", dest="corrected", action="store_true")
    p.add_argument("--low_q", dest="low_quality", action="store_true")
    p.add_argument("--nsplit", dest="nsplit", type=int, default=60)
    p.add_argument("--min_identity", dest="min_identity", type=float, default=0.95)
    p.add_argument("--min_ovlp_len", dest="min_ovlp_len", type=int, default=3000)
    p.add_argument("--size", dest="size", default=15000, type=int)
    p.add_argument("--max_tip_len", dest="max_tip_len", type=int, default=10000)
    p.add_argument("--insert_size", dest="insert_size", default=450, type=int)
    p.add_argument("--average_read_len", dest="average_read_len", default=250, type=int)
    p.add_argument("--version", "-v", action="version", version="%(prog)s version: " + __version__)
    p.add_argument("--stop_after", choices=["overlap", "contigs1", "polish", "clusters", "savage", "stageb_graph", "stageb_merge"],
                   default=None,
                   help="(extension) stop after the named stage (clusters: the short-read clustering into tmp/ - "
                        "readnames.txt, the grouped JSON, fq_<size>/; savage: the contig overlap file of extend_con; "
                        "stageb_graph: also the overlap graph of the stage-b merge in tmp/stageb/ - graph.gfa, "
                        "graph.txt, graph_trimmed.gfa, digraph.txt, cycles.txt, tips.txt - then exit status 3; stageb_merge: "
                        "that graph and the super-reads merged along its edges - singles.fastq, subreads.txt, "
                        "removed_tip_sequences.fastq, superread_map.txt in tmp/stageb/ - then exit status 3)")
    p.add_argument("--device", type=int, default=0, help="(extension) GPU index of a single-GPU run")
    p.add_argument("--gpus", type=int, default=1,
                   help="(extension) shard every overlap stage over this many GPUs of the node (one process per GPU)")
    p.add_argument("--short_contigs", default=None,
                   help="(extension) contigs of the short-read branch (POLYTE, run elsewhere) to merge with the long-read contigs")
    p.add_argument("--polyte_cmd", default=None,
                   help="(extension) command prefix of the reference's polyte.tune_params.py, if installed: without "
                        "--short_contigs, cluster the short reads and run it per cluster (HyLight.py:215-275)")
    p.add_argument("--polyte_native", action="store_true",
                   help="(extension) the same with the library's own POLYTE (hylight_amd.polyte: the clique, merge and branch "
                        "iterations and the overlaps between them on the GPU), cluster after cluster in this process "
                        "(--polyte_workers: in several); not together with --polyte_cmd")
    p.add_argument("--polyte_workers", type=int, default=1,
                   help="(extension) processes per GPU during the --polyte_native step: the clusters are dealt out to them by "
                        "size, every cluster's files are the same whichever process ran it; --gpus times this is at most 16")
    p.add_argument("--stageb_cmd", default=None,
                   help="(extension) command prefix of the reference's pipeline_per_stage.py, if installed")
    p.add_argument("--stageb_native", action="store_true",
                   help="(extension) run stage b with the library (hylight_amd.vq_stageb: ViralQuasispecies' merge iterations on "
                        "the GPU) and write final_contigs.fa - the contigs themselves when no two of them overlap")
    p.add_argument("--polish_native", action="store_true",
                   help="(extension) polish with the library (hlmi_polish: a pile-up consensus over the overlapper's own CIGARs, "
                        "tmp/polish_<k>.paf) in place of the three racon calls; racon is then not needed")
    p.add_argument("--polish_direct", action="store_true",
                   help="(extension) the same polisher with the alignment inside the call (hlmi_polish_reads): the same contigs, "
                        "no tmp/polish_<k>.paf; not together with --polish_native")
    p.add_argument("--polish_qual", action="store_true",
                   help="(extension) with --polish_native or --polish_direct: weigh the polisher's votes by the reads' base "
                        "qualities and drop reads of low mean quality (hlmi_polish_q; the short-read FASTQ of the third site "
                        "carries qualities, the long-read FASTA of the first two does not)")
    p.add_argument("--polish_strain", action="store_true",
                   help="(extension) with --polish_native or --polish_direct: only the (read, contig) pairs the overlap stage's "
                        "SNP filter kept vote at the three polishing sites (hlmi_polish_pairs with ov_long_ref.paf, the round's "
                        "ov_long_ref2.paf and shortr1.paf), as the reference's racon calls see only those rows")
    p.add_argument("--polish_min_avg_qual", type=float, default=10.0, metavar="Q",
                   help="with --polish_qual: reads whose mean Phred quality is below Q do not vote (racon's -q)")
    p.add_argument("--depth", action="store_true",
                   help="(extension) when final_contigs.fa is written: read depth and relative abundance of its contigs "
                        "(hlmi_depth_reads) into final_contigs.long.depth.tsv and .bedgraph, and with -s also "
                        "final_contigs.short.depth.tsv and .bedgraph")
    p.add_argument("--variants", action="store_true",
                   help="(extension) when final_contigs.fa is written: the variant sites of its contigs and a summary per contig "
                        "(hlmi_variants_reads) into final_contigs.long.variants.tsv and .long.variants.summary.tsv, and with -s "
                        "also the .short. pair; with --polish_strain only the pairs of ov_long_ref.paf / shortr1.paf vote")
    p.add_argument("--variants_ins", action="store_true",
                   help="(extension) as --variants, with the insertion sites of the contigs beside the two files "
                        "(hlmi_variants_reads_ins) in final_contigs.long.variants.ins.tsv, and with -s also the .short. one; the "
                        "summary gains slots, ins_sites and ins_rate; with --variants too, still one call per read set")
    p.add_argument("--variants_qual", action="store_true",
                   help="(extension) with --variants / --variants_ins: base qualities take part (hlmi_variants_reads_q, "
                        "hlmi_variants_reads_ins_q) - a column below --variants_min_base_qual casts no vote, the rows of a read whose "
                        "mean quality is below --variants_min_avg_qual are dropped; the same file names; FASTA reads pass every "
                        "floor, so it is the short-read FASTQ where this bites; refused without --variants or --variants_ins")
    p.add_argument("--variants_min_base_qual", type=int, default=10, metavar="Q",
                   help="with --variants_qual: the per-base floor, a Phred of 0..93 (0: off); no real data stands behind the default")
    p.add_argument("--variants_min_avg_qual", type=float, default=10.0, metavar="Q",
                   help="with --variants_qual: the read floor, --polish_min_avg_qual's rule and default (0: off)")
    p.add_argument("--phase", action="store_true",
                   help="(extension) when final_contigs.fa is written: its variant sites phased from the reads (hlmi_phase_reads) "
                        "into final_contigs.long.phase.sites.tsv, .links.tsv and .reads.tsv, and with -s also the .short. triple; "
                        "independent of --variants; with --polish_strain only the pairs of ov_long_ref.paf / shortr1.paf vote")
    p.add_argument("--phase_ins", action="store_true",
                   help="(extension) with --phase: insertion sites as phasing evidence - the same three files from "
                        "hlmi_phase_reads_ins, whose sites are the variant sites and the insertion sites with a supported length; "
                        "honours --phase_reach; refused without --phase")
    p.add_argument("--haplotigs", action="store_true",
                   help="(extension) when final_contigs.fa is written: its contigs polished once per side of every phased block "
                        "the reads split (hlmi_haplotigs_reads) into final_contigs.long.haplotigs.fa and "
                        ".long.haplotigs.blocks.tsv, and with -s also the .short. pair; independent of --phase; with "
                        "--polish_strain only the pairs of ov_long_ref.paf / shortr1.paf vote")
    p.add_argument("--haplotigs_ins", action="store_true",
                   help="(extension) with --haplotigs: the blocks of --phase_ins - insertion sites are phasing evidence and are "
                        "decided per side - the same two files from hlmi_haplotigs_reads_ins, the blocks file with a tenth column "
                        "diff_slots; honours --phase_reach and --polish_strain; refused without --haplotigs")
    p.add_argument("--phase_reach", type=int, default=1, metavar="K",
                   help="(extension) with --phase and --haplotigs: link variant sites up to K sites apart (hlmi_phase_reads_reach, "
                        "hlmi_haplotigs_reads_reach; 1: neighbours alone, at most 8), so that one noisy site does not cut a block")
    return p


def polyte_lines(tmp, size, polyte_cmd, insert_size, average_read_len):
    """HyLight.py:228-242: one POLYTE command per cluster directory of tmp/fq_<size>/, `polyte_cmd` in place of
    `python <bin>/polyte.tune_params.py`."""
    outdir2 = os.path.join(tmp, f"fq_{size}")
    lines = []
    for i in sorted(os.listdir(outdir2)):
        fq1, fq2, folder = f"{outdir2}/{i}/{i}.1.fq", f"{outdir2}/{i}/{i}.2.fq", f"{outdir2}/{i}"
        lines.append(f"cd {folder}; {polyte_cmd} -p1 {fq1} -p2 {fq2}  -m 50 -m_EC 60 -t 1 --hap_cov 10 --insert_size  "
                     f"{insert_size} --stddev 27  --mismatch_rate 0 --min_clique_size 2 --average_read_len "
                     f"{average_read_len} --edge1 0.93 --edge2 1.0 --no_EC > log.txt 2>&1")
    return lines


def polyte_native(tmp, size, insert_size, average_read_len, workers=1, device=0, host_threads=20, pool=None):
    """HyLight.py:228-242 with the library's own POLYTE (`--polyte_native`): hylight_amd.polyte.run in every cluster directory
    of tmp/fq_<size>/ with the options of polyte_lines; each cluster's output goes to its log.txt.  A cluster that fails leaves
    no contigs.fasta and is named by the caller's warning, as in the reference.  With one worker and no pool of ranks: one
    cluster after the other in this process.  `workers` > 1 (`--polyte_workers`): that many processes on GPU `device`, this one
    among them, with `host_threads` shared out (polyte_pool.run); `pool`: the StagePool of the run, which knows its own device
    and threads - under `--gpus N` every rank takes its share of the clusters with `workers` processes on its own GPU.  The
    files are the same in every case."""
    from . import polyte_pool
    if pool is not None:
        return pool.polyte(tmp, size, insert_size, average_read_len, workers)
    polyte_pool.run(polyte_pool.cluster_folders(tmp, size), workers, device, host_threads, insert_size, average_read_len)


def _short_branch(args, tmp, outdir, long_con3, pool=None):
    """HyLight.py:228-275 after the clustering: POLYTE per cluster (external with `--polyte_cmd`, the library's with
    `--polyte_native`), the cluster contigs, their stage-b extension (short_stageb.fa) and all_contigs.fa; then the final
    extend_con as on the other path."""
    from concurrent.futures import ThreadPoolExecutor

    size = args.size
    if args.polyte_native:
        polyte_native(tmp, size, args.insert_size, args.average_read_len, workers=args.polyte_workers, device=args.device,
                      host_threads=args.threads, pool=pool)
    else:
        lines = polyte_lines(tmp, size, args.polyte_cmd, args.insert_size, args.average_read_len)
        with open(os.path.join(tmp, "cmd_polyte.sh"), "w") as f:
            f.writelines(line + "\n" for line in lines)
        with ThreadPoolExecutor(max_workers=max(1, args.threads)) as ex:    # `xargs -i -P threads bash -c "{}"`
            list(ex.map(lambda line: subprocess.run(["bash", "-c", line]), lines))
    outdir2 = os.path.join(tmp, f"fq_{size}")
    ids = sorted(os.listdir(outdir2))
    for i in ids:                                               # HyLight.py:248-256
        folder = f"{outdir2}/{i}/"
        if not os.path.isfile(folder + "contigs.fasta"):
            print(f"You need to rerun polyte in {folder} or decrease the size of cluster and rerun the whole steps")
    fname = os.path.join(tmp, f"all.contigs_{size}.fasta")
    with open(fname, "wb") as o:                                # `cat fq_<size>/*/contigs.fasta` (C-locale glob order)
        for i in ids:
            p = f"{outdir2}/{i}/contigs.fasta"
            if os.path.isfile(p):
                with open(p, "rb") as f:
                    shutil.copyfileobj(f, o)
    short_con = os.path.join(outdir, "short_stageb.fa")
    extend_con(fname, tmp, short_con, threads=30, len_c=500000, stageb_cmd=args.stageb_cmd, stageb_native=args.stageb_native)
    all_con = os.path.join(outdir, "all_contigs.fa")
    first = short_con if os.path.exists(short_con) and os.path.getsize(short_con) else fname     # HyLight.py:266-275
    with open(all_con, "wb") as o:
        for p in (first, long_con3):
            with open(p, "rb") as f:
                shutil.copyfileobj(f, o)
    final = os.path.join(outdir, "final_contigs.fa")
    n_con = extend_con(all_con, tmp, final, threads=30, stageb_cmd=args.stageb_cmd, stageb_native=args.stageb_native)
    if not os.path.exists(final):
        sys.stderr.write(f"hylight-mi: {n_con} contigs, their overlaps are in tmp/stageb/sfoverlap.out.savage; the stage-b merge "
                         "(pipeline_per_stage.py / ViralQuasispecies, HyLight.py:320-324) was not asked for, so final_contigs.fa "
                         "was not written (pass --stageb_native to run the library's, or --stageb_cmd for the reference's): "
                         f"exit status {EXIT_NO_FINAL}\n")
        return EXIT_NO_FINAL
    return 0


def _rank_device(args, world, local):
    """The index of this rank's GPU."""
    import torch
    n_dev = torch.cuda.device_count()                         # (counting devices does not initialise the GPU)
    return args.device if world == 1 else local % max(n_dev, 1)


def _init_rank(args, world, local):
    """This rank's GPU, the library on it, the process group of the run (RCCL)."""
    import torch
    dev = _rank_device(args, world, local)
    torch.cuda.set_device(dev)
    api.init(dev, args.threads)
    launch.init_process_group(dev)


def refuse_polyte_workers(args):
    """`--polyte_workers` against the flags it goes with; before anything is created."""
    w = args.polyte_workers
    if w < 1:
        raise SystemExit(f"--polyte_workers {w}: at least one process runs the POLYTE step")
    if w > 1 and not args.polyte_native:
        raise SystemExit("--polyte_workers is about the library's own POLYTE: give --polyte_native with it (--polyte_cmd runs "
                         "its lines with -t workers)")
    if args.gpus * w > MAX_GPU_PROCESSES:
        raise SystemExit(f"--gpus {args.gpus} with --polyte_workers {w} is {args.gpus * w} processes with a GPU open; shared "
                         f"machines allow {MAX_GPU_PROCESSES} at a time")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if args.variants_qual and not (args.variants or args.variants_ins):
        raise SystemExit("--variants_qual puts quality floors into the calls of --variants / --variants_ins: give one of them as well")
    if args.phase_ins and not args.phase:
        raise SystemExit("--phase_ins adds insertion sites to the files of --phase: give --phase as well")
    if args.haplotigs_ins and not args.haplotigs:
        raise SystemExit("--haplotigs_ins adds insertion sites to the blocks of --haplotigs: give --haplotigs as well")
    if args.polyte_native and args.polyte_cmd:
        raise SystemExit("--polyte_native and --polyte_cmd are two ways to run the same step: give one of them")
    if args.polish_qual and not (args.polish_native or args.polish_direct):
        raise SystemExit("--polish_qual is an option of the library's polisher: give --polish_native or --polish_direct with it")
    if args.polish_strain and not (args.polish_native or args.polish_direct):
        raise SystemExit("--polish_strain is an option of the library's polisher: give --polish_native or --polish_direct with it")
    if args.polish_native and args.polish_direct:
        raise SystemExit("--polish_native and --polish_direct are two ways to run the same step: give one of them")
    refuse_polyte_workers(args)
    if args.gpus > 1 and not launch.launched():
        # one process per GPU, started before this one has made any GPU call; this process only waits for them
        return launch.spawn_ranks(args.gpus, [sys.executable, "-m", "hylight_amd.driver", *argv])
    rank, world, local = launch.rank_env()
    if launch.launched() and args.gpus not in (1, world):
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    _init_rank(args, world, local)
    pool = StagePool(rank, world, device_index=_rank_device(args, world, local), host_threads=args.threads)
    try:
        if rank != 0:
            pool.serve()
            return 0
        return _pipeline(args, pool)
    finally:
        pool.shutdown()
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()


def _pipeline(args, pool):
    """The run itself (rank 0).  `pool.stage` = utils.split_reads2 on every rank."""
    def stage(fa, ref, nsplit, out_file, len_over, mc, iden, long=True):
        return pool.stage(fa, ref, nsplit, out_file, len_over, mc, iden, long)

    outdir, nsplit, iden = args.outdir, args.nsplit, args.min_identity
    len_over, max_tip = args.min_ovlp_len, args.max_tip_len
    long_reads = os.path.abspath(args.long_reads)
    os.makedirs(outdir, exist_ok=True)
    tmp = os.path.join(outdir, "tmp") + "/"
    os.makedirs(tmp, exist_ok=True)

    if args.corrected:
        infile = long_reads
    else:                                                       # HyLight.py:85-112
        if not args.short_reads:
            raise SystemExit("read correction needs --short_reads (or pass --corrected)")
        short_reads = os.path.abspath(args.short_reads)
        bfc, rope, conv, fml = _tool("bfc"), _tool("ropebwt2"), _tool("fmlrc2-convert"), _tool("fmlrc2")
        cor = os.path.join(tmp, "cor_short_reads.fq")
        _run(f"{bfc} -s 3g -t{args.threads} {short_reads} 2>/dev/null | awk 'NR%4==1{{print $1; next}} {{print}}' > {cor}")
        _run(f"cat {cor} | awk 'NR % 4 == 2' | sort | tr NT TN | {rope} -LR | tr NT TN | {conv} {tmp}/comp_msbwt.npy")
        _run(f"{fml} -t 30 -m 2 comp_msbwt.npy {long_reads} fmlrc1.fasta && {fml} -t 30 -m 2 comp_msbwt.npy fmlrc1.fasta "
             f"fmlrc2.fasta && {fml} -t 30 -m 2 comp_msbwt.npy fmlrc2.fasta fmlrc3.fasta && rm fmlrc1.fasta fmlrc2.fasta", cwd=tmp)
        infile = os.path.join(tmp, "fmlrc3.fasta")

    infile = filter_non_atcg(infile, outdir, fq_or_fa(infile))  # HyLight.py:116-118
    ovl_dir = os.path.join(outdir, "2.overlap")
    shutil.rmtree(ovl_dir, ignore_errors=True)
    os.makedirs(ovl_dir)
    # main all-vs-all: len_over is hard-coded to 6000 here in the reference (HyLight.py:130)
    overlap = stage(infile, infile, nsplit, os.path.join(ovl_dir, "s1_s1.paf"), 6000, 2, iden)
    if args.stop_after == "overlap":
        return 0
    gfa, long_con = tmp + "contigs1.gfa", tmp + "contigs1.fa"
    n_arg, c_arg = (3, 3) if args.low_quality else (1, 1)       # HyLight.py:137,140
    api.miniasm(overlap, infile, gfa, bub_dist=max_tip, n_rounds_arg=n_arg, max_ext=1, min_dp=c_arg)
    gfa2fa(gfa, long_con)
    if args.stop_after == "contigs1":
        return 0

    ov_long_ref = stage(infile, long_con, nsplit, tmp + "ov_long_ref.paf", len_over, 2, iden)   # HyLight.py:149
    native = args.polish_native or args.polish_direct
    pqual = args.polish_min_avg_qual if args.polish_qual else None      # (sites 1 and 2 read s1.fa: no qualities, all weights 1)
    racon = None if native else _tool("racon")
    p1, p2 = tmp + "polish1.fa", tmp + "polish2.fa"
    if native:
        polish_native(1, infile, long_con, p1, tmp, len_over, iden, direct=args.polish_direct, qual=pqual,
                      pairs=ov_long_ref if args.polish_strain else None)      # (as it is now: it grows below)
    else:
        _run(f"{racon} --no-trimming -u -t 30 {infile} {ov_long_ref} {long_con} > {p1}", cwd=tmp)
    ti = 0
    while ti < 2 and not args.low_quality:                      # HyLight.py:158-190
        remain = pick_up(ov_long_ref, tmp, infile)
        if not os.path.exists(remain) or os.path.getsize(remain) == 0:    # every read overlapped: nothing left to assemble
            break
        ov_remain = stage(remain, remain, nsplit, tmp + "ov_long_remain.paf", len_over, 2, iden)
        remain_gfa = tmp + "remain.gfa"
        api.miniasm(ov_remain, infile, remain_gfa, bub_dist=max_tip, n_rounds_arg=1, max_ext=1, min_dp=1)
        if os.path.getsize(remain_gfa) == 0:                    # HyLight.py:173
            break
        remain_con = tmp + "remain_con.fa"
        gfa2fa(remain_gfa, remain_con)
        ov2 = stage(infile, remain_con, nsplit, tmp + "ov_long_ref2.paf", len_over, 2, iden)
        if native:
            polish_native(2 if ti == 0 else f"2_{ti}", infile, remain_con, p2, tmp, len_over, iden, append=True, direct=args.polish_direct,
                          qual=pqual, pairs=ov2 if args.polish_strain else None)
            with open(ov2, "rb") as f, open(ov_long_ref, "ab") as w:
                shutil.copyfileobj(f, w)
        else:
            _run(f"{racon} --no-trimming -u -t 30 {infile} {ov2} {remain_con} >> {p2}; cat {ov2} >> {ov_long_ref}", cwd=tmp)
        ti += 1
    long_con2 = tmp + "long_con_polished.fa"
    with open(long_con2, "w") as o:                             # HyLight.py:192-201
        num = 0
        for p in (p1, p2):
            if not os.path.exists(p):
                continue
            for line in open(p):
                o.write(line if num % 2 == 1 else f">longr_con_{num // 2}\n")
                num += 1
    if args.stop_after == "polish":
        return 0
    if not args.short_reads:
        sys.stderr.write("hylight-mi: long-read path finished (tmp/long_con_polished.fa); no --short_reads given\n")
        return 0
    short_reads = os.path.abspath(args.short_reads) if args.corrected else os.path.join(tmp, "cor_short_reads.fq")
    # the two short-read calls of the same path (HyLight.py:200,207: len_over 70, mc 3, short mode)
    ov_short = stage(short_reads, long_con2, nsplit, tmp + "shortr1.paf", 70, 3, iden, long=False)
    long_con3 = os.path.join(outdir, "long_con_polished.fa")
    if native:
        polish_native(3, short_reads, long_con2, long_con3, tmp, 70, iden, short=True, direct=args.polish_direct, qual=pqual,
                      pairs=ov_short if args.polish_strain else None)
    else:
        _run(f"{racon} --no-trimming -u -t 30 {short_reads} {ov_short} {long_con2} > {long_con3}", cwd=outdir)
    remain_short = pick_up(ov_short, tmp, short_reads)
    shortr2 = os.devnull                                       # no reads remain: the clustering sees no rows
    if os.path.exists(remain_short) and os.path.getsize(remain_short):
        shortr2 = stage(short_reads, remain_short, nsplit, tmp + "shortr2.paf", 70, 3, iden, long=False)
    if args.stop_after == "clusters" or ((args.polyte_cmd or args.polyte_native) and not args.short_contigs):
        st = api.cluster_short(shortr2, short_reads, tmp, size=args.size, threads=args.threads)    # HyLight.py:215-226
        sys.stderr.write(f"hylight-mi: {st['files'] // 2} short-read clusters in tmp/fq_{args.size}/\n")
        if args.stop_after == "clusters":
            return 0
        rc = _short_branch(args, tmp, outdir, long_con3, pool)
        if rc == 0 and args.depth:
            depth_tables(os.path.join(outdir, "final_contigs.fa"), infile, short_reads, outdir)
        if rc == 0 and (args.variants or args.variants_ins):
            variant_tables(os.path.join(outdir, "final_contigs.fa"), infile, short_reads, outdir,
                           long_pairs=ov_long_ref if args.polish_strain else None, short_pairs=ov_short if args.polish_strain else None,
                           **({"ins": True} if args.variants_ins else {}), **variants_qual_args(args))
        if rc == 0 and args.phase:
            phase_tables(os.path.join(outdir, "final_contigs.fa"), infile, short_reads, outdir,
                         long_pairs=ov_long_ref if args.polish_strain else None, short_pairs=ov_short if args.polish_strain else None,
                         **({"reach": args.phase_reach} if args.phase_reach != 1 else {}), **({"ins": True} if args.phase_ins else {}))
        if rc == 0 and args.haplotigs:
            haplotig_files(os.path.join(outdir, "final_contigs.fa"), infile, short_reads, outdir,
                           long_pairs=ov_long_ref if args.polish_strain else None, short_pairs=ov_short if args.polish_strain else None,
                           **({"reach": args.phase_reach} if args.phase_reach != 1 else {}), **({"ins": True} if args.haplotigs_ins else {}))
        return rc
    # HyLight.py:211-262 (read clustering, POLYTE per cluster) is the short-read branch: not part of this path.  Its
    # contigs can be handed in; the contig-overlap half of extend_con runs either way (HyLight.py:264-280).
    sys.stderr.write("hylight-mi: short-read clustering and POLYTE (HyLight.py:211-262) are outside this implementation"
                     + (": using --short_contigs\n" if args.short_contigs else "; continuing with the long-read contigs only\n"))
    all_con = os.path.join(outdir, "all_contigs.fa")
    with open(all_con, "w") as o:
        for p in ([args.short_contigs] if args.short_contigs else []) + [long_con3]:
            with open(p) as f:
                shutil.copyfileobj(f, o)
    final = os.path.join(outdir, "final_contigs.fa")
    if args.stop_after == "stageb_graph":
        n_con = extend_con(all_con, tmp, final, threads=30, stageb_graph=True)
        sys.stderr.write(f"hylight-mi: {n_con} contigs; the overlap graph of the stage-b merge is in tmp/stageb/ (graph.gfa, "
                         "graph.txt, graph_trimmed.gfa, digraph.txt, cycles.txt, tips.txt); the run stops there as asked, so "
                         f"final_contigs.fa was not written (--stageb_native runs all of stage b): exit status {EXIT_NO_FINAL}\n")
        return EXIT_NO_FINAL
    if args.stop_after == "stageb_merge":
        n_con = extend_con(all_con, tmp, final, threads=30, stageb_merge=True)
        sys.stderr.write(f"hylight-mi: {n_con} contigs; the super-reads of the first stage-b iteration are in tmp/stageb/ "
                         "(singles.fastq, subreads.txt, superread_map.txt, removed_tip_sequences.fastq); the run stops there as "
                         "asked, so final_contigs.fa was not written (--stageb_native runs all of stage b): "
                         f"exit status {EXIT_NO_FINAL}\n")
        return EXIT_NO_FINAL
    n_con = extend_con(all_con, tmp, final, threads=30, stageb_cmd=None if args.stop_after == "savage" else args.stageb_cmd,
                       stageb_native=args.stageb_native and args.stop_after != "savage")
    if args.stop_after == "savage":
        return 0
    if not os.path.exists(final):
        sys.stderr.write(f"hylight-mi: {n_con} contigs, their overlaps are in tmp/stageb/sfoverlap.out.savage; the stage-b merge "
                         "(pipeline_per_stage.py / ViralQuasispecies, HyLight.py:320-324) was not asked for, so final_contigs.fa "
                         "was not written (pass --stageb_native to run the library's, or --stageb_cmd for the reference's): "
                         f"exit status {EXIT_NO_FINAL}\n")
        return EXIT_NO_FINAL
    if args.depth:
        depth_tables(final, infile, short_reads, outdir)
    if args.variants or args.variants_ins:
        variant_tables(final, infile, short_reads, outdir, long_pairs=ov_long_ref if args.polish_strain else None,
                       short_pairs=ov_short if args.polish_strain else None, **({"ins": True} if args.variants_ins else {}),
                       **variants_qual_args(args))
    if args.phase:
        phase_tables(final, infile, short_reads, outdir, long_pairs=ov_long_ref if args.polish_strain else None,
                     short_pairs=ov_short if args.polish_strain else None, **({"reach": args.phase_reach} if args.phase_reach != 1 else {}),
                     **({"ins": True} if args.phase_ins else {}))
    if args.haplotigs:
        haplotig_files(final, infile, short_reads, outdir, long_pairs=ov_long_ref if args.polish_strain else None,
                       short_pairs=ov_short if args.polish_strain else None, **({"reach": args.phase_reach} if args.phase_reach != 1 else {}),
                       **({"ins": True} if args.haplotigs_ins else {}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
