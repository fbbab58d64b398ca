"""Stage b of SAVAGE as HyLight runs it (script/pipeline_per_stage.py:94-160, :170-275, :347-372 with --stage b
--no_error_correction --remove_branches true): a first iteration on fastq_dir/singles.fastq, then merge iterations in place
on the singles.fastq / overlaps.txt / subreads.txt of out_dir, each one call of libhylight_mi.so (hlmi_vq_iteration).  With
--remove_branches true the loop holds merge iterations only: no cliques, no BranchReduction.

    python -m hylight_amd.vq_stageb --fastq DIR --overlaps sfoverlap.out.savage --out DIR [options]

The reference's len_c only sizes a histogram and is not an option here.
"""
import argparse
import os
import sys

from . import api


def count_records(path):
    """analyze_fastq's read count: FASTQ records of `path` (0 when it is missing)."""
    if not os.path.isfile(path):
        return 0
    with open(path, "rb") as f:
        return f.read().count(b"\n") // 4


def count_lines(path):
    """analyze_overlaps: lines of `path` (0 when it is missing, :368-371)."""
    if not os.path.isfile(path):
        return 0
    with open(path, "rb") as f:
        return f.read().count(b"\n")


def edge_count(out_dir):
    """get_edge_count (:347-354): the lines of graph.txt less its two header lines; -2 without the file."""
    p = os.path.join(out_dir, "graph.txt")
    return count_lines(p) - 2 if os.path.isfile(p) else -2


def loop(step):
    """The stage-b loop (:141-160) over step(k) -> (reads, overlaps, edges) after iteration k = 0, 1, ..: it goes on while the
    last overlaps.txt has lines, the last graph.txt has more than two lines, and the read count has stayed unchanged fewer
    than two times in a row.  -> (reads, overlaps, edges) per iteration run."""
    reads, ovs, edges = [], [], []

    def run(k):
        r, o, e = step(k)
        reads.append(r); ovs.append(o); edges.append(e)

    run(0)                                                    # run_first_it_merge
    const_read_its = 0
    while ovs[-1] > 0 and edges[-1] > 0 and const_read_its < 2:
        run(len(reads))                                       # run_merging_it
        const_read_its = const_read_its + 1 if reads[-1] == reads[-2] else 0
    return reads, ovs, edges


def run(fastq_dir, overlaps, out_dir, edge_threshold=1.0, min_overlap_perc=0, min_overlap_len=300, merge_contigs=0.0,
        min_read_len=0, max_tip_len=1000, verbose=False, min_qual=None):
    """-> dict(iterations, reads, overlaps, edges): the counts pipeline_per_stage.py prints, `overlaps` led by the input's.
    min_qual: --min_qual for every iteration (None, as pipeline_per_stage.py leaves it: minQual 0.9)."""
    os.makedirs(out_dir, exist_ok=True)
    p = lambda name: os.path.join(out_dir, name)
    for name in ("stats.txt", "removed_tip_sequences.fastq"):                  # :127-132
        open(p(name), "w").close()
    common = dict(edge_threshold=edge_threshold, min_overlap_perc=min_overlap_perc, min_overlap_len=min_overlap_len,
                  keep_singletons=max(min_overlap_len, min_read_len), min_read_len=min_read_len, max_tip_len=max_tip_len,
                  min_qual=min_qual)

    def step(k):
        if k == 0:
            api.vq_iteration(os.path.join(fastq_dir, "singles.fastq"), overlaps, out_dir, first_it=1, merge_contigs=merge_contigs,
                             **common)
        else:
            api.vq_iteration(p("singles.fastq"), p("overlaps.txt"), out_dir, subreads_in=p("subreads.txt"), first_it=0,
                             merge_contigs=0, **common)
        counts = count_records(p("singles.fastq")), count_lines(p("overlaps.txt")), edge_count(out_dir)
        if verbose:
            print(f"iteration {k + 1}: {counts[0]} reads, {counts[1]} overlaps, {counts[2]} edges", flush=True)
        return counts

    reads, ovs, edges = loop(step)
    return dict(iterations=len(reads), reads=reads, overlaps=[count_lines(overlaps)] + ovs, edges=edges)


def fastq2fasta(fastq, fasta):
    """fastq2fasta.py: line 1 of every record with '>' for '@', then line 2."""
    with open(fastq) as f, open(fasta, "w") as o:
        for k, line in enumerate(f):
            if k % 4 == 0:
                o.write(">" + line[1:])
            elif k % 4 == 1:
                o.write(line)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.vq_stageb", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--fastq", required=True, help="directory that holds singles.fastq")
    p.add_argument("--overlaps", required=True)
    p.add_argument("--out", required=True)
    p.add_argument("--edge_threshold", type=float, default=1.0)
    p.add_argument("--min_overlap_perc", type=int, default=0)
    p.add_argument("--min_overlap_len", type=int, default=300)
    p.add_argument("--merge_contigs", type=float, default=0.0)
    p.add_argument("--min_read_len", type=int, default=0)
    p.add_argument("--max_tip_len", type=int, default=1000)
    p.add_argument("--min_qual", type=float, default=None, help="0 .. 1, passed to every iteration (default: not passed, minQual 0.9)")
    p.add_argument("--verbose", action="store_true")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    try:
        r = run(a.fastq, a.overlaps, a.out, a.edge_threshold, a.min_overlap_perc, a.min_overlap_len, a.merge_contigs, a.min_read_len,
                a.max_tip_len, a.verbose, a.min_qual)
    except api.HlmiError as e:
        sys.stderr.write(f"hylight_amd.vq_stageb: {e}\n")
        return 1
    print(f"Stage b done in {r['iterations']} iterations")
    print("Number of contigs per iteration: \t", r["reads"])
    print("Number of overlaps per iteration: \t", r["overlaps"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
