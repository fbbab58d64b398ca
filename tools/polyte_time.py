"""Time the native POLYTE loop and hlmi_sr_overlaps on one simulated cluster (not part of the test suite).

    python tools/polyte_time.py [--pairs 3000] [--runs 5] [--out DIR]

The cluster: two haplotypes of 20 kb at 1 % divergence, `--pairs` error-free read pairs of 2 x 150 bases, insert N(450, 27).
Prints one JSON line:
  "ab": hlmi_sr_overlaps against the four calls it fuses (ava with driver.contig_ava_opts -> filter_ovlp_inline ->
        minimap22sfo -> sfo2overlaps: entry points this library shares unchanged with its parent commit) on the renumbered
        reads, `--runs` alternating runs after one warm-up of each, wall seconds per run, the medians, and whether the two
        files are equal;
  "loop": hylight_amd.polyte.run on the same cluster - the wall seconds of the whole run and of its phases (preprocessing,
        input overlaps, threshold table, the iterations by kind, the overlap computations between them).
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hylight_amd import api, driver, polyte, simulate as S  # noqa: E402

READ_LEN, GENOME = 150, 20000


def chain(fq, d, n, min_len):
    fa, paf, flt, sfo, sav = (os.path.join(d, "chain." + e) for e in ("fa", "paf", "flt", "sfo", "savage"))
    polyte.fastq2fasta(fq, fa)
    api.ava(fa, fa, paf, driver.contig_ava_opts())
    api.filter_ovlp_inline(paf, flt, min_len, 0.98, 1, 0.8)
    api.minimap22sfo(flt, sfo, 0, 0.0)
    api.sfo2overlaps(sfo, sav, num_singles=n, num_pairs=0)
    return sav


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--pairs", type=int, default=3000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="polyte_time_")
    os.makedirs(d, exist_ok=True)
    api.init(0, 0)
    strains = S.make_strains(np.random.default_rng(7), 2, GENOME, 0.01)
    reads = S.simulate_short_pairs(8, strains, a.pairs, read_len=READ_LEN, err_sub=0.0)
    p1, p2 = os.path.join(d, "c.1.fq"), os.path.join(d, "c.2.fq")
    S.write_fastq(reads[0::2], p1)
    S.write_fastq(reads[1::2], p2)
    fq = os.path.join(d, "s_p1_p2.fastq")
    n = polyte.preprocess(p1, p2, fq)
    fused = os.path.join(d, "fused.txt")

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    run_fused = lambda: api.sr_overlaps(fq, fused, 60, 0.98, 1, 0.8)
    run_chain = lambda: chain(fq, d, n, 60)
    run_chain(); run_fused()                                   # warm-up: code objects, the allocator's pool, the page cache
    t_chain, t_fused = [], []
    for _ in range(a.runs):                                    # alternating, so that drift hits both alike
        t_chain.append(timed(run_chain)[0])
        t_fused.append(timed(run_fused)[0])
    stats = api.last_stats()
    ab = {"reads": n, "lines": open(fused, "rb").read().count(b"\n"), "raw_rows": int(stats.get("sr_rows_raw", 0)),
          "equal": open(fused, "rb").read() == open(os.path.join(d, "chain.savage"), "rb").read(),
          "chain_s": [round(t, 4) for t in t_chain], "fused_s": [round(t, 4) for t in t_fused],
          "chain_median_s": round(statistics.median(t_chain), 4), "fused_median_s": round(statistics.median(t_fused), 4),
          "kernel_ms_sr_overlaps": stats.get("kernel_ms.sr_overlaps")}

    # the loop, its phases timed by wrapping what it calls
    phases = {}

    def wrap(mod, name, label):
        real = getattr(mod, name)

        def fn(*pos, **kw):
            t, r = timed(lambda: real(*pos, **kw))
            phases[label] = phases.get(label, 0.0) + t
            phases[label + "_calls"] = phases.get(label + "_calls", 0) + 1
            return r
        setattr(mod, name, fn)

    wrap(api, "vq_clique_iteration", "clique_iteration")
    wrap(api, "vq_iteration", "merge_iteration")
    wrap(api, "vq_branch_iteration", "branch_iteration")
    wrap(api, "sr_overlaps", "sr_overlaps")
    wrap(polyte, "preprocess", "preprocess")
    wrap(polyte.min_ev, "write", "threshold_table")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            t_loop, r = timed(lambda: polyte.run(p1, p2, 50, 60, 10, 450, 27, READ_LEN, 2, 0.93, 1.0))
    finally:
        os.chdir(cwd)
    loop = {"wall_s": round(t_loop, 3), "kinds": r["kinds"], "reads": r["reads"], "overlaps": r["overlaps"],
            "phases_s": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in sorted(phases.items())}}
    print(json.dumps({"version": api.version(), "pairs": a.pairs, "ab": ab, "loop": loop}))


if __name__ == "__main__":
    main()
