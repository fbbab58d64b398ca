"""Time hlmi_polish_reads_pairs beside hlmi_polish_reads_q on one input (not part of the test suite).

    python tools/polish_pairs_time.py [--genome 400000] [--reads 3000] [--runs 5] [--out DIR]

The long input of tools/polish_time.py (one simulated genome cut into four contigs with planted errors, `--reads` long reads).
The list is what the overlap stage writes for these reads against these contigs (the driver's ov_long_ref.paf: len_over 3000,
mc 2, iden 0.95); `--true_contigs`: against the contigs as they were before the errors were planted, under the same names.  One warm-up of each call, then `--runs` alternating runs in this process; `ms_device` of both, the list's
rows, the share of alignment rows the list drops.  Prints one JSON line.
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
from hylight_amd import api, simulate as S, stage  # noqa: E402
from polish_time import with_errors  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--genome", type=int, default=400000)
    p.add_argument("--reads", type=int, default=3000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--true_contigs", action="store_true", help="the list from the contigs without their planted errors")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="polish_pairs_time_")
    os.makedirs(d, exist_ok=True)
    api.init(0, 0)
    reads, strains = S.simulate_reads(seed=4301, n_strains=1, genome_len=a.genome, n_reads=a.reads, mean_len=8000, min_len=4000,
                                      max_len=14000)
    truth = strains[0].tobytes()
    rng = np.random.default_rng(4302)
    cfa, lfa, lst = (os.path.join(d, n) for n in ("contigs.fa", "long.fa", "ov_long_ref.paf"))
    q = len(truth) // 4
    with open(cfa, "wb") as f:
        for k in range(4):
            f.write(b">contig%d\n" % k + with_errors(rng, truth[k * q:(k + 1) * q if k < 3 else len(truth)]) + b"\n")
    tfa = os.path.join(d, "contigs_true.fa")
    with open(tfa, "wb") as f:
        for k in range(4):
            f.write(b">contig%d\n" % k + truth[k * q:(k + 1) * q if k < 3 else len(truth)] + b"\n")
    S.write_fasta(reads, lfa)
    stage.split_reads2(lfa, tfa if a.true_contigs else cfa, 3, d, lst, len_over=3000, mc=2, iden=0.95, long=True)
    with open(lst, "rb") as f:
        list_rows = f.read().count(b"\n")
    o = api.ava_opts_long()
    o.pair_once = 0
    opts = dict(min_len=3000, min_iden=0.95, qual_weight=0, min_avg_qual=0.0)
    fa_q, fa_p = os.path.join(d, "q.fa"), os.path.join(d, "pairs.fa")

    def run_q():
        return api.polish_reads(cfa, lfa, fa_q, o, **opts)

    def run_p():
        return api.polish_reads(cfa, lfa, fa_p, o, pairs=lst, **opts)

    run_q(); run_p()                                           # warm-up: code objects, the allocator's pool, the page cache
    ms_q, ms_p = [], []
    for _ in range(a.runs):                                    # alternating, so that drift hits both alike
        st_q = run_q()
        st_p = run_p()
        ms_q.append(st_q["ms_device"])
        ms_p.append(st_p["ms_device"])
    stats = api.last_stats()
    print(json.dumps({"version": api.version(), "genome": a.genome, "long_reads": a.reads, "runs": a.runs, "list_rows": list_rows,
                      "list_bytes": os.path.getsize(lst), "rows": st_p["rows"], "rows_not_listed": st_p["rows_not_listed"],
                      "share_dropped": round(st_p["rows_not_listed"] / max(st_p["rows"], 1), 4),
                      "pairs_listed": st_p["pairs_listed"], "pairs_unknown": st_p["pairs_unknown"],
                      "rows_selected_q": st_q["rows_selected"], "rows_selected_pairs": st_p["rows_selected"],
                      "ms_device_q": [round(t, 3) for t in ms_q], "ms_device_pairs": [round(t, 3) for t in ms_p],
                      "ms_device_q_median": round(statistics.median(ms_q), 3), "ms_device_pairs_median": round(statistics.median(ms_p), 3),
                      "kernel_ms_polish_pairs": stats.get("kernel_ms.polish_pairs"), "kernel_ms_polish_rows": stats.get("kernel_ms.polish_rows")}))


if __name__ == "__main__":
    main()
