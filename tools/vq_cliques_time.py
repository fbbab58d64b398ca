"""Time hlmi_vq_cliques after the graph on a simulated cluster set (not part of the test suite).

    python tools/vq_cliques_time.py [--clusters 250] [--reads 400] [--min_clique_size 3] [--no_ec] [--min_qual X] [--iteration] [--out DIR]

Makes `--clusters` clusters of the kind tests/test_gpu_vq_cliques.py uses - 3 haplotypes of 2 kb at 1 % divergence, `--reads`
reads of 150 bases with 1 % substitutions and qualities that know about them - into one singles.fastq, with the overlaps
the coordinates give inside every cluster; runs the command line (hylight_amd.vq_cliques.main) once and prints one JSON
line: the stats, ms_cliques and its phases (enumerator, placement, device with its copies, the rest), the kernel's time
from the library's own timer and the share of columns the host redid.  250 x 400 is the 1e5-read set of DESIGN.md 4.3f.
--min_qual X is passed on as it stands (POLYTE: 0); without it the run is the one at minQual 0.9.
With --iteration the run goes on to findNextOverlaps (hlmi_vq_clique_iteration) and the line also holds "next": ms_next,
candidates, max_list and the rest of its stats, and "next_kernel_ms": the library's timers of the count, expand, claim sort,
eval and order passes.  No reference time exists beside any of these: ViralQuasispecies needs Boost and is not built here.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hylight_amd import api, simulate as S, vq_cliques  # noqa: E402

READ_LEN, GENOME, MIN_OVL = 150, 2000, 60


def make(d, clusters, n_reads, seed=5):
    fq, ov = os.path.join(d, "singles.fastq"), os.path.join(d, "overlaps.txt")
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rows = 0
    with open(fq, "w") as f, open(ov, "w") as o:
        for c in range(clusters):
            rng = np.random.default_rng(seed + c)
            strains = S.make_strains(rng, 3, GENOME, 0.01)
            starts = np.sort(rng.integers(0, GENOME - READ_LEN + 1, n_reads))
            hap = rng.integers(0, 3, n_reads)
            first = c * n_reads
            for k in range(n_reads):
                s = np.array(strains[hap[k]][starts[k]:starts[k] + READ_LEN], dtype=np.uint8)
                wrong = rng.random(READ_LEN) < 0.01
                code = np.searchsorted(acgt, s)                               # (ACGT is ascending)
                s[wrong] = acgt[(code[wrong] + rng.integers(1, 4, int(wrong.sum()))) % 4]
                q = np.where(rng.random(READ_LEN) < 0.9, rng.integers(30, 41, READ_LEN), rng.integers(12, 30, READ_LEN))
                q[wrong] = np.where(rng.random(int(wrong.sum())) < 0.8, rng.integers(8, 21, int(wrong.sum())), q[wrong])
                f.write(f"@{first + k}\n{s.tobytes().decode()}\n+\n{(q + 33).astype(np.uint8).tobytes().decode()}\n")
            for i in range(n_reads):
                for j in range(i + 1, n_reads):
                    n = int(starts[i]) + READ_LEN - int(starts[j])
                    if n < MIN_OVL:
                        break
                    o.write(f"{first + i}\t{first + j}\t{int(starts[j] - starts[i])}\t-\t-\t+\t+\t{100 * n // READ_LEN}\t-\t{n}\t-\ts\ts\n")
                    rows += 1
    return fq, ov, rows


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--clusters", type=int, default=250)
    p.add_argument("--reads", type=int, default=400)
    p.add_argument("--min_clique_size", type=int, default=3)
    p.add_argument("--no_ec", action="store_true")
    p.add_argument("--min_qual", type=float, default=None, help="--min_qual of the run (default: not passed, minQual 0.9)")
    p.add_argument("--iteration", action="store_true", help="go on to findNextOverlaps and report its stats and kernel timers")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="vq_cliques_time_")
    os.makedirs(d, exist_ok=True)
    fq, ov, rows = make(d, a.clusters, a.reads)
    argv = ["--singles", fq, "--overlaps", ov, "--out", os.path.join(d, "out"), "--min_overlap_len", str(MIN_OVL),
            "--edge_threshold", "0.97", "--min_clique_size", str(a.min_clique_size),
            "--error_correction", "false" if a.no_ec else "true"] + (["--iteration"] if a.iteration else [])
    if a.min_qual is not None:
        argv += ["--min_qual", repr(a.min_qual)]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        rc = vq_cliques.main(argv)
    if rc:
        sys.exit(rc)
    st = json.loads(text.getvalue().strip().split("\n")[-1])
    stats = api.last_stats()
    cst = st["cliques"]
    out = {"version": api.version(), "min_qual": a.min_qual, "reads": a.clusters * a.reads, "overlap_rows": rows, "graph": st["graph"], "cliques": cst,
           "phases_ms": {k[len("vq_clique_ms_"):]: round(v, 2) for k, v in stats.items() if k.startswith("vq_clique_ms_")},
           "piles": int(stats.get("vq_clique_piles", 0)),
           "kernel_ms": stats.get("kernel_ms.vq_clique_piles"),
           "columns_host_share": cst["columns_host"] / cst["columns"] if cst["columns"] else None}
    if a.iteration:
        out["next"] = st["next"]
        out["next_kernel_ms"] = {k: stats.get("kernel_ms.vq_next_" + k) for k in ("count", "expand", "claim_sort", "eval", "order")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
