"""Time hlmi_variants_reads beside hlmi_depth_reads and hlmi_polish_reads on one input (not part of the test suite).

    python tools/variants_time.py [--genome 400000] [--reads 3000] [--runs 5] [--out DIR]

The long input of tools/depth_time.py (one simulated genome cut into four contigs with planted errors, `--reads` long reads).
One warm-up of each call, then `--runs` alternating runs in this process; `ms_device` of the three, the kernel timers of the
variants call's last run and the share of tiles its second pass revisited.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from hylight_amd import api, simulate as S  # noqa: E402
from polish_time import with_errors  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--genome", type=int, default=400000)
    p.add_argument("--reads", type=int, default=3000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="variants_time_")
    os.makedirs(d, exist_ok=True)
    api.init(0, 0)
    reads, strains = S.simulate_reads(seed=4301, n_strains=1, genome_len=a.genome, n_reads=a.reads, mean_len=8000, min_len=4000,
                                      max_len=14000)
    truth = strains[0].tobytes()
    rng = np.random.default_rng(4302)
    cfa, lfa = (os.path.join(d, n) for n in ("contigs.fa", "long.fa"))
    q = len(truth) // 4
    with open(cfa, "wb") as f:
        for k in range(4):
            f.write(b">contig%d\n" % k + with_errors(rng, truth[k * q:(k + 1) * q if k < 3 else len(truth)]) + b"\n")
    S.write_fasta(reads, lfa)
    o = api.ava_opts_long()
    o.pair_once = 0
    opts = dict(min_len=3000, min_iden=0.95)
    fa, tsv, sites, summ = (os.path.join(d, n) for n in ("polished.fa", "depth.tsv", "sites.tsv", "summary.tsv"))

    def run_polish():
        return api.polish_reads(cfa, lfa, fa, o, **opts)

    def run_depth():
        return api.depth_reads(cfa, lfa, tsv, None, o, **opts)

    def run_variants():
        st = api.variants_reads(cfa, lfa, sites, summ, o, **opts)
        return st, api.last_stats()

    run_polish(); run_depth(); run_variants()                  # warm-up: code objects, the allocator's pool, the page cache
    ms_p, ms_d, ms_v = [], [], []
    for _ in range(a.runs):                                    # alternating, so that drift hits all alike
        ms_p.append(run_polish()["ms_device"])
        ms_d.append(run_depth()["ms_device"])
        st_v, stats = run_variants()
        ms_v.append(st_v["ms_device"])
    kernels = {k[len("kernel_ms."):]: round(v, 4) for k, v in stats.items() if k.startswith("kernel_ms.")}
    print(json.dumps({"version": api.version(), "genome": a.genome, "long_reads": a.reads, "runs": a.runs, "rows": st_v["rows"],
                      "rows_selected": st_v["rows_selected"], "positions": st_v["positions"], "callable": st_v["callable"],
                      "sites": st_v["sites"], "sites_base": st_v["sites_base"], "sites_del": st_v["sites_del"],
                      "tiles": stats.get("variants_tiles"), "tiles_revisited": stats.get("variants_tiles_revisited"),
                      "ms_device_polish": [round(t, 3) for t in ms_p], "ms_device_depth": [round(t, 3) for t in ms_d],
                      "ms_device_variants": [round(t, 3) for t in ms_v],
                      "ms_device_polish_median": round(statistics.median(ms_p), 3), "ms_device_depth_median": round(statistics.median(ms_d), 3),
                      "ms_device_variants_median": round(statistics.median(ms_v), 3), "kernel_ms": kernels}))


if __name__ == "__main__":
    main()
