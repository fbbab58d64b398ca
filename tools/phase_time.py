"""Time hlmi_phase_reads beside hlmi_variants_reads on one input (not part of the test suite).

    python tools/phase_time.py [--genome 400000] [--reads 3000] [--runs 5] [--out DIR]

The long input of tools/variants_time.py (one simulated genome cut into four contigs with planted errors, `--reads` long reads).
One warm-up of each call, then `--runs` alternating runs in this process; `ms_device` of both and the kernel timers of the phase
call's last run.  Prints one JSON line.
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
    d = a.out or tempfile.mkdtemp(prefix="phase_time_")
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
    vsites, summ, sites, links, haps = (os.path.join(d, n) for n in ("variants.tsv", "summary.tsv", "phase.sites.tsv", "phase.links.tsv",
                                                                     "phase.reads.tsv"))

    def run_variants():
        return api.variants_reads(cfa, lfa, vsites, summ, o, **opts)

    def run_phase():
        st = api.phase_reads(cfa, lfa, sites, links, haps, o, **opts)
        return st, api.last_stats()

    run_variants(); run_phase()                                # warm-up: code objects, the allocator's pool, the page cache
    ms_v, ms_p = [], []
    for _ in range(a.runs):                                    # alternating, so that drift hits both alike
        ms_v.append(run_variants()["ms_device"])
        st_p, stats = run_phase()
        ms_p.append(st_p["ms_device"])
    kernels = {k[len("kernel_ms."):]: round(v, 4) for k, v in stats.items() if k.startswith("kernel_ms.")}
    print(json.dumps({"version": api.version(), "genome": a.genome, "long_reads": a.reads, "runs": a.runs, "rows": st_p["rows"],
                      "rows_selected": st_p["rows_selected"], "positions": st_p["positions"], "sites": st_p["sites"],
                      "links": st_p["links"], "links_phased": st_p["links_phased"], "blocks": st_p["blocks"], "alleles": st_p["alleles"],
                      "read_records": st_p["read_records"],
                      "ms_device_variants": [round(t, 3) for t in ms_v], "ms_device_phase": [round(t, 3) for t in ms_p],
                      "ms_device_variants_median": round(statistics.median(ms_v), 3),
                      "ms_device_phase_median": round(statistics.median(ms_p), 3), "kernel_ms": kernels}))


if __name__ == "__main__":
    main()
