"""Time hlmi_polish_reads against the chain it stands for, hlmi_ava + hlmi_polish (not part of the test suite).

    python tools/polish_time.py [--genome 400000] [--reads 3000] [--pairs 20000] [--runs 5] [--out DIR]

One simulated genome (`--genome` bases, one strain).  The contigs are the genome cut in four, each with a substitution, a
missing base or one to three bases too many about every 100 bases.  Two inputs against them:
  "long":  `--reads` long reads (mean 8 kb, the simulator's corrected-read error rates), the overlapper's long constants,
           min_len 3000, min_iden 0.95 - the driver's first two polishing sites;
  "short": `--pairs` pairs of 2 x 150 bases (0.1 % substitutions), the short constants, min_len 70 - its third.
For each: one warm-up of each side, then `--runs` alternating runs of the chain (api.ava + api.polish, entry points this
library shares unchanged with its parent commit) and of api.polish_reads; wall seconds per call, the medians, both spreads
(min - max), whether the two files and the integer stats are equal, and the PAF's size.  Prints one JSON line.
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
from hylight_amd import api, simulate as S  # noqa: E402


def with_errors(rng, truth, every=100):
    at = np.sort(rng.choice(np.arange(50, len(truth) - 50), size=len(truth) // every, replace=False))
    out, prev = bytearray(), 0
    for p in at:
        out += truth[prev:p]
        k = int(rng.integers(3))
        if k == 0:
            out.append(b"ACGT"[(b"ACGT".find(truth[p:p + 1]) + 1 + int(rng.integers(3))) % 4])
        elif k == 2:
            out += bytes(b"ACGT"[j] for j in rng.integers(0, 4, size=int(rng.integers(1, 4))))
            out.append(truth[p])
        prev = p + 1                                           # (k == 1: the base is missing)
    return bytes(out + truth[prev:])


def ab(name, contigs, reads, ava_opts, d, runs, **opts):
    paf, chain_fa, direct_fa = (os.path.join(d, f"{name}.{e}") for e in ("paf", "chain.fa", "direct.fa"))

    def run_chain():
        api.ava(contigs, reads, paf, ava_opts)
        return api.polish(contigs, reads, paf, chain_fa, **opts)

    def run_direct():
        return api.polish_reads(contigs, reads, direct_fa, ava_opts, **opts)

    def timed(fn):
        t0 = time.perf_counter()                               # (both sides end in a download and a file: the device is drained)
        r = fn()
        return time.perf_counter() - t0, r

    run_chain(); run_direct()                                  # warm-up: code objects, the allocator's pool, the page cache
    t_chain, t_direct = [], []
    for _ in range(runs):                                      # alternating, so that drift hits both alike
        tc, st_c = timed(run_chain)
        td, st_d = timed(run_direct)
        t_chain.append(tc)
        t_direct.append(td)
    stats = api.last_stats()
    return {"rows": st_c["rows"], "rows_selected": st_c["rows_selected"], "slots_opened": st_c["slots_opened"],
            "paf_bytes": os.path.getsize(paf),
            "equal": open(chain_fa, "rb").read() == open(direct_fa, "rb").read()
            and all(st_c[k] == st_d[k] for k in api.POLISH_STATS),
            "chain_s": [round(t, 4) for t in t_chain], "direct_s": [round(t, 4) for t in t_direct],
            "chain_median_s": round(statistics.median(t_chain), 4), "direct_median_s": round(statistics.median(t_direct), 4),
            "chain_spread_s": [round(min(t_chain), 4), round(max(t_chain), 4)],
            "direct_spread_s": [round(min(t_direct), 4), round(max(t_direct), 4)],
            "kernel_ms_polish_rows": stats.get("kernel_ms.polish_rows"), "kernel_ms_polish_count": stats.get("kernel_ms.polish_count")}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--genome", type=int, default=400000)
    p.add_argument("--reads", type=int, default=3000)
    p.add_argument("--pairs", type=int, default=20000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="polish_time_")
    os.makedirs(d, exist_ok=True)
    api.init(0, 0)
    reads, strains = S.simulate_reads(seed=4301, n_strains=1, genome_len=a.genome, n_reads=a.reads, mean_len=8000, min_len=4000,
                                      max_len=14000)
    truth = strains[0].tobytes()
    rng = np.random.default_rng(4302)
    cfa, lfa, sfa = (os.path.join(d, n) for n in ("contigs.fa", "long.fa", "short.fa"))
    q = len(truth) // 4
    with open(cfa, "wb") as f:
        for k in range(4):
            f.write(b">contig%d\n" % k + with_errors(rng, truth[k * q:(k + 1) * q if k < 3 else len(truth)]) + b"\n")
    S.write_fasta(reads, lfa)
    S.write_fasta(S.simulate_short_pairs(4303, strains, a.pairs, read_len=150), sfa)
    lo, so = api.ava_opts_long(), api.ava_opts_short()
    lo.pair_once = so.pair_once = 0
    out = {"version": api.version(), "genome": a.genome, "long_reads": a.reads, "short_reads": 2 * a.pairs, "runs": a.runs,
           "long": ab("long", cfa, lfa, lo, d, a.runs, min_len=3000, min_iden=0.95),
           "short": ab("short", cfa, sfa, so, d, a.runs, min_len=70, min_iden=0.95)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
