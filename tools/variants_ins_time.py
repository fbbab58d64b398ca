"""Time hlmi_variants_reads_ins beside hlmi_variants_reads on one input (not part of the test suite).

    python tools/variants_ins_time.py [--genome 400000] [--reads 3000] [--runs 5] [--out DIR]

The long input of tools/variants_time.py (one simulated genome cut into four contigs with planted errors, `--reads` long reads).
One warm-up of each call, then `--runs` alternating runs in this process; `ms_device` of both and the kernel timers of each
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
    d = a.out or tempfile.mkdtemp(prefix="variants_ins_time_")
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
    vsites, vsumm, isites, ins, isumm = (os.path.join(d, n) for n in ("variants.tsv", "summary.tsv", "ins.sites.tsv", "ins.tsv",
                                                                       "ins.summary.tsv"))

    def run_variants():
        return api.variants_reads(cfa, lfa, vsites, vsumm, o, **opts), api.last_stats()

    def run_ins():
        return api.variants_ins_reads(cfa, lfa, isites, ins, isumm, o, **opts), api.last_stats()

    run_variants(); run_ins()                                  # warm-up: code objects, the allocator's pool, the page cache
    ms_v, ms_i = [], []
    for _ in range(a.runs):                                    # alternating, so that drift hits both alike
        st_v, stats_v = run_variants()
        ms_v.append(st_v["ms_device"])
        st_i, stats_i = run_ins()
        ms_i.append(st_i["ms_device"])

    def kernels(stats):
        return {k[len("kernel_ms."):]: round(v, 4) for k, v in stats.items() if k.startswith("kernel_ms.")}
    with open(vsites, "rb") as f1, open(isites, "rb") as f2:
        same_sites = f1.read() == f2.read()
    print(json.dumps({"version": api.version(), "genome": a.genome, "long_reads": a.reads, "runs": a.runs, "rows": st_i["rows"],
                      "rows_selected": st_i["rows_selected"], "positions": st_i["positions"], "sites": st_i["sites"],
                      "slots_callable": st_i["slots_callable"], "ins_sites": st_i["ins_sites"], "ins_long": st_i["ins_long"],
                      "slot_sites": stats_i.get("variants_ins_slot_sites"), "tiles": stats_i.get("variants_tiles"),
                      "tiles_revisited_variants": stats_v.get("variants_tiles_revisited"),
                      "tiles_revisited_ins": stats_i.get("variants_tiles_revisited"), "same_sites_file": same_sites,
                      "ms_device_variants": [round(t, 3) for t in ms_v], "ms_device_ins": [round(t, 3) for t in ms_i],
                      "ms_device_variants_median": round(statistics.median(ms_v), 3),
                      "ms_device_ins_median": round(statistics.median(ms_i), 3),
                      "kernel_ms_variants": kernels(stats_v), "kernel_ms_ins": kernels(stats_i)}))


if __name__ == "__main__":
    main()
