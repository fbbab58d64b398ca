"""Time hlmi_cluster_short (the short-read clustering, HyLight.py:215-226) on a C4-like input generated with
tests/cluster_inputs.py: 5 M read pairs and 5e7 score-sorted PAF rows by default.  Prints one JSON line: PAF rows per
second end to end without the file writes, the per-phase milliseconds of the stats and the host union pass's share.

    python tools/cluster_time.py [--pairs 5000000] [--rows 50000000] [--size 15000] [-t 20] [--dir DIR] [--keep]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cluster_inputs as CI  # noqa: E402
from hylight_amd import api  # noqa: E402

BLOCK = 1_000_000


def generate(d, pairs, rows, seed=7, group=40):
    fq_path, paf_path = os.path.join(d, "reads.fq"), os.path.join(d, "shortr2.paf")
    fq, _ = CI.make_case(seed, pairs, 0, group=group, name_fmt=CI.LONG_NAMES, read_len=150)
    with open(fq_path, "wb") as f:
        f.write(fq)
    del fq
    names = [(CI.LONG_NAMES % i).encode() for i in range(pairs)]
    rng = np.random.default_rng(seed + 1)
    with open(paf_path, "wb") as f:
        for b0 in range(0, rows, BLOCK):
            m = min(BLOCK, rows - b0)
            score = 1.0 - (b0 + np.arange(m)) / rows                         # one descending score over all blocks
            f.write(CI.paf_rows(rng, names, m, group=group, descending=score))
    return fq_path, paf_path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--size", type=int, default=15000)
    ap.add_argument("-t", "--threads", type=int, default=20)
    ap.add_argument("--dir", default=None, help="work directory (default: a temporary one, removed at exit)")
    ap.add_argument("--keep", action="store_true", help="keep the generated inputs")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="hlmi_cluster_time_")
    os.makedirs(d, exist_ok=True)
    try:
        t = time.time()
        fq, paf = generate(d, a.pairs, a.rows)
        gen_s = time.time() - t
        out = os.path.join(d, "tmp")
        shutil.rmtree(out, ignore_errors=True)
        st = api.cluster_short(paf, fq, out, size=a.size, threads=a.threads)
        compute_ms = st["ms_total"] - st["ms_write"]
        rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
        print(json.dumps({"bench": "cluster_short", "rev": rev, "lib": api.version(), "pairs": a.pairs, "rows": st["rows"],
                          "size": a.size, "threads": a.threads, "paf_bytes": os.path.getsize(paf),
                          "rows_per_s": st["rows"] / (compute_ms / 1e3), "host_union_share": st["ms_union"] / compute_ms,
                          "gen_s": round(gen_s, 1), **st}))
    finally:
        if not a.keep and not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
