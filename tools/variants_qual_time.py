"""Time hlmi_variants_reads_q at both floors 0 and at 10 / 10.0 beside hlmi_variants_reads on one input (not part of the test suite).

    python tools/variants_qual_time.py [--genome 400000] [--reads 3000] [--runs 5] [--out DIR] [--plain_only]

The long input of tools/variants_time.py (one simulated genome cut into four contigs with planted errors, `--reads` long reads),
the reads written as FASTQ with the simulator's qualities, so that the base floor withholds votes.  One warm-up of each call, then
`--runs` alternating runs in this process; `ms_device` of each and the kernel timers of each call's last run.  Prints one JSON
line.  --plain_only times hlmi_variants_reads alone and touches no newer symbol: run with another build's package first on the
module path (an older commit's), it gives that build's figure for the same files.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(HERE))              # behind what the caller put on the path: see --plain_only
sys.path.insert(0, HERE)
from hylight_amd import api, simulate as S  # noqa: E402
from polish_time import with_errors  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--genome", type=int, default=400000)
    p.add_argument("--reads", type=int, default=3000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--plain_only", action="store_true")
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="variants_qual_time_")
    os.makedirs(d, exist_ok=True)
    api.init(0, 0)
    reads, strains = S.simulate_reads(seed=4301, n_strains=1, genome_len=a.genome, n_reads=a.reads, mean_len=8000, min_len=4000,
                                      max_len=14000)
    truth = strains[0].tobytes()
    rng = np.random.default_rng(4302)
    cfa, lfq = (os.path.join(d, n) for n in ("contigs.fa", "long.fq"))
    q = len(truth) // 4
    with open(cfa, "wb") as f:
        for k in range(4):
            f.write(b">contig%d\n" % k + with_errors(rng, truth[k * q:(k + 1) * q if k < 3 else len(truth)]) + b"\n")
    with open(lfq, "wb") as f:                                 # one base in twenty at Q2 - Q9, the others at Q12 - Q40
        for r in reads:
            qual = np.where(rng.random(len(r.seq)) < 0.05, rng.integers(2, 10, size=len(r.seq)), rng.integers(12, 41, size=len(r.seq)))
            f.write(b"@" + r.name.encode() + b"\n" + r.seq.tobytes() + b"\n+\n" + (qual + 33).astype(np.uint8).tobytes() + b"\n")
    o = api.ava_opts_long()
    o.pair_once = 0
    opts = dict(min_len=3000, min_iden=0.95)
    calls = {"plain": lambda out: api.variants_reads(cfa, lfq, out, None, o, **opts)}
    if not a.plain_only:
        calls["q_off"] = lambda out: api.variants_reads_q(cfa, lfq, out, None, o, min_base_qual=0, min_avg_qual=0.0, **opts)
        calls["q_10"] = lambda out: api.variants_reads_q(cfa, lfq, out, None, o, min_base_qual=10, min_avg_qual=10.0, **opts)
    files = {k: os.path.join(d, k + ".sites.tsv") for k in calls}
    for k, call in calls.items():                              # warm-up: code objects, the allocator's pool, the page cache
        call(files[k])
    ms, st, kern = {k: [] for k in calls}, {}, {}
    for _ in range(a.runs):                                    # alternating, so that drift hits all alike
        for k, call in calls.items():
            st[k] = call(files[k])
            ms[k].append(st[k]["ms_device"])
            kern[k] = {n[len("kernel_ms."):]: round(v, 4) for n, v in api.last_stats().items() if n.startswith("kernel_ms.")}
    out = {"version": api.version(), "library": api.LIB_PATH, "genome": a.genome, "long_reads": a.reads, "runs": a.runs,
           "rows": st["plain"]["rows"], "rows_selected": {k: v["rows_selected"] for k, v in st.items()},
           "sites": {k: v["sites"] for k, v in st.items()}, "callable": {k: v["callable"] for k, v in st.items()},
           "ms_device": {k: [round(t, 3) for t in v] for k, v in ms.items()},
           "ms_device_median": {k: round(statistics.median(v), 3) for k, v in ms.items()}, "kernel_ms": kern}
    if not a.plain_only:
        with open(files["plain"], "rb") as f1, open(files["q_off"], "rb") as f2:
            out["q_off_same_sites_file"] = f1.read() == f2.read()
        out["qcounts"] = {k: {n: st[k][n] for n in api.VARIANT_QCOUNTS} for k in ("q_off", "q_10")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
