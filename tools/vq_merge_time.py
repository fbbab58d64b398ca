"""Time hlmi_vq_merge after the graph on a synthetic stage-b input (not part of the test suite).

    python tools/vq_merge_time.py [--contigs 100000] [--length 2000] [--min_qual X] [--iteration] [--out DIR]

Makes `--contigs` contigs of `--length` bases tiling a seeded genome with 300-base overlaps, half of them stored
reverse-complemented, and their exact SAVAGE rows; runs api.vq_merge with the stage-b options and prints one JSON line:
the stats, ms_merge (the step after the graph), the kernel times of the library's own timers, and the HBM traffic model
2 x input bases + output bytes over the kernels' time.  For per-kernel shares run it under
`rocprofv3 --kernel-trace --stats -- python tools/vq_merge_time.py`.  With --iteration the call is api.vq_iteration (a
warm-up call first, so that ms_next holds no module load) and the line also holds "next": its stats with ms_next.
--min_qual X goes to the call as it stands (default: not passed, minQual 0.9); the tiling reads agree, so it changes the tables
the kernels read and not the output.
"""
import argparse
import json
import os
import random
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hylight_amd import api  # noqa: E402

COMP = str.maketrans("ACGT", "TGCA")


def make(d, n, length, seed=1):
    rng = random.Random(seed)
    step = length - 300
    g = "".join(rng.choices("ACGT", k=step * n + 300))
    fq, ov = os.path.join(d, "singles.fastq"), os.path.join(d, "overlaps.savage")
    fwd = [rng.random() < 0.5 for _ in range(n)]
    with open(fq, "w") as f:
        for k in range(n):
            s = g[k * step:k * step + length]
            if not fwd[k]:
                s = s.translate(COMP)[::-1]
            f.write(f"@{k + 1}\n{s}\n+\n{'I' * length}\n")
    with open(ov, "w") as f:
        for k in range(n - 1):
            f.write(f"{k + 1}\t{k + 2}\t{step}\t-\t-\t{'+' if fwd[k] else '-'}\t{'+' if fwd[k + 1] else '-'}\t99\t-\t300\t-\ts\ts\n")
    return fq, ov


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--contigs", type=int, default=100000)
    p.add_argument("--length", type=int, default=2000)
    p.add_argument("--min_qual", type=float, default=None, help="--min_qual of the call (default: not passed, minQual 0.9)")
    p.add_argument("--iteration", action="store_true", help="time api.vq_iteration and report ms_next as well")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="vq_merge_time_")
    os.makedirs(d, exist_ok=True)
    fq, ov = make(d, a.contigs, a.length)
    api.init(0)
    nst = None
    if a.iteration:
        api.vq_iteration(fq, ov, os.path.join(d, "warm"), min_qual=a.min_qual)
        gst, mst, nst = api.vq_iteration(fq, ov, os.path.join(d, "out"), min_qual=a.min_qual)
    else:
        gst, mst = api.vq_merge(fq, ov, os.path.join(d, "out"), min_qual=a.min_qual)
    stats = api.last_stats()
    kernels = {k.split(".", 1)[1]: v for k, v in stats.items() if k.startswith("kernel_ms.vq_")}
    traffic = 2 * mst["bases_in"] + mst["bytes_out"]
    kms = sum(kernels.values())
    print(json.dumps({"version": api.version(), "min_qual": a.min_qual, "contigs": a.contigs, "length": a.length, "graph": gst, "merge": mst,
                      **({"next": nst} if nst else {}), "kernel_ms": kernels, "traffic_bytes": traffic,
                      "gb_per_s_over_kernels": traffic / kms / 1e6 if kms else None}))


if __name__ == "__main__":
    main()
