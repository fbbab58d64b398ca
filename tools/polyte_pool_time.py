"""Time the native POLYTE step with 1, 2, 4 and 8 worker processes on one GPU (not part of the test suite; needs the GPU).

    python tools/polyte_pool_time.py [--clusters 32] [--runs 3] [--workers 1,2,4,8] [--out DIR]

The clusters: `--clusters` directories under DIR/fq_60/, each with 500-3000 read pairs (drawn once, fixed seed) of 2 x 150 bases
from two haplotypes of 20 kb at 1 % divergence, insert N(450, 27), every cluster with haplotypes and reads of its own seeds.
One warm-up of every worker count, then `--runs` rounds in which the worker counts take turns, so that drift hits all alike; a
run is polyte_pool.run over all clusters, children's start-up included (that is what a user waits for).  One worker is the
step as it was before there were workers: the same code in this process.  After every run all contigs.fasta are compared with
those of the first one-worker run.  Prints one JSON line: every run's wall seconds, the medians, the spread ((max - min) /
median) and the speed-up of the medians over one worker.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hylight_amd import api, polyte_pool, simulate as S  # noqa: E402

READ_LEN, GENOME, SIZE, HOST_THREADS = 150, 20000, 60, 16


def contigs(folders):
    out = []
    for f in folders:
        p = os.path.join(f, "contigs.fasta")
        out.append(open(p, "rb").read() if os.path.exists(p) else None)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--clusters", type=int, default=32)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--workers", default="1,2,4,8")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    counts = [int(w) for w in a.workers.split(",")]
    if counts[0] != 1:
        raise SystemExit("--workers starts with 1: the one-worker run is what the others are compared with")
    d = a.out or tempfile.mkdtemp(prefix="polyte_pool_time_")
    pairs = [int(n) for n in np.random.default_rng(11).integers(500, 3001, size=a.clusters)]
    for k, n in enumerate(pairs):
        c = os.path.join(d, f"fq_{SIZE}", str(k))
        os.makedirs(c, exist_ok=True)
        strains = S.make_strains(np.random.default_rng(1000 + k), 2, GENOME, 0.01)
        reads = S.simulate_short_pairs(2000 + k, strains, n, read_len=READ_LEN)
        S.write_fastq(reads[0::2], os.path.join(c, f"{k}.1.fq"))
        S.write_fastq(reads[1::2], os.path.join(c, f"{k}.2.fq"))
    folders = polyte_pool.cluster_folders(d, SIZE)
    api.init(0, HOST_THREADS)

    def timed(w):
        t0 = time.perf_counter()
        polyte_pool.run(folders, w, 0, HOST_THREADS, 450, READ_LEN)
        return time.perf_counter() - t0

    warm, want, equal = {}, None, True
    for w in counts:                                             # warm-up: code objects, the allocator's pool, the page cache
        warm[w] = round(timed(w), 3)
        if w == 1:
            want = contigs(folders)
        equal = equal and contigs(folders) == want
    times = {w: [] for w in counts}
    for _ in range(a.runs):
        for w in counts:
            times[w].append(timed(w))
            equal = equal and contigs(folders) == want
    med = {w: statistics.median(t) for w, t in times.items()}
    print(json.dumps({
        "version": api.version(), "clusters": a.clusters, "pairs": pairs, "host_threads": HOST_THREADS,
        "with_contigs": sum(bool(c) for c in want), "equal": equal, "warmup_s": warm,
        "runs_s": {w: [round(x, 3) for x in t] for w, t in times.items()},
        "median_s": {w: round(m, 3) for w, m in med.items()},
        "spread": {w: round((max(t) - min(t)) / med[w], 3) for w, t in times.items()},
        "speedup": {w: round(med[1] / m, 2) for w, m in med.items()}}))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
