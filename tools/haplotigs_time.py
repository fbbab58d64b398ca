"""Time hlmi_haplotigs_reads beside hlmi_phase_reads followed by hlmi_polish_reads on one input (not part of the test suite).

    python tools/haplotigs_time.py [--genome 400000] [--reads 3000] [--runs 5] [--out DIR]

An input of tools/phase_time.py's size with two strains: two simulated genomes that differ at about 1 % of their bases, the first
cut into four contigs, `--reads` long reads of both.  One warm-up of each call, then `--runs` alternating runs in this process;
`ms_device` of the haplotig call and of the pair of older calls, and the kernel timers of the haplotig call's last run.  Prints
one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from hylight_amd import api, simulate as S  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--genome", type=int, default=400000)
    p.add_argument("--reads", type=int, default=3000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="haplotigs_time_")
    os.makedirs(d, exist_ok=True)
    api.init(0, 0)
    reads, strains = S.simulate_reads(seed=4401, n_strains=2, genome_len=a.genome, n_reads=a.reads, mean_len=8000, min_len=4000,
                                      max_len=14000, snp_rate=0.01)
    first = strains[0].tobytes()
    cfa, lfa = (os.path.join(d, n) for n in ("contigs.fa", "long.fa"))
    q = len(first) // 4
    with open(cfa, "wb") as f:
        for k in range(4):
            f.write(b">contig%d\n" % k + first[k * q:(k + 1) * q if k < 3 else len(first)] + b"\n")
    S.write_fasta(reads, lfa)
    o = api.ava_opts_long()
    o.pair_once = 0
    sel = dict(min_len=3000, min_iden=0.95)
    hfa, blocks, sites, pfa = (os.path.join(d, n) for n in ("haplotigs.fa", "haplotigs.blocks.tsv", "phase.sites.tsv", "polished.fa"))

    def run_haplotigs():
        st = api.haplotigs_reads(cfa, lfa, hfa, blocks, o, **sel)
        return st, api.last_stats()

    def run_phase_then_polish():
        st = api.phase_reads(cfa, lfa, sites, None, None, o, **sel)
        polish_count = api.last_stats().get("kernel_ms.polish_count", 0.0)      # (the phase call runs none)
        pst = api.polish_reads(cfa, lfa, pfa, o, **sel)
        return st["ms_device"], pst["ms_device"], polish_count + api.last_stats().get("kernel_ms.polish_count", 0.0)

    run_phase_then_polish(); run_haplotigs()                   # warm-up: code objects, the allocator's pool, the page cache
    ms_h, ms_ph, ms_po, k_po = [], [], [], []
    for _ in range(a.runs):                                    # alternating, so that drift hits both alike
        x, y, z = run_phase_then_polish()
        ms_ph.append(x); ms_po.append(y); k_po.append(z)
        st, stats = run_haplotigs()
        ms_h.append(st["ms_device"])
    kernels = {k[len("kernel_ms."):]: round(v, 4) for k, v in stats.items() if k.startswith("kernel_ms.")}
    print(json.dumps({"version": api.version(), "genome": a.genome, "long_reads": a.reads, "runs": a.runs, "rows": st["rows"],
                      "rows_selected": st["rows_selected"], "positions": st["positions"], "sites": st["sites"], "blocks": st["blocks"],
                      "blocks_split": st["blocks_split"], "contigs_split": st["contigs_split"], "positions_split": st["positions_split"],
                      "diff_positions": st["diff_positions"], "slots_opened": st["slots_opened"],
                      "ms_device_haplotigs": [round(t, 3) for t in ms_h], "ms_device_phase": [round(t, 3) for t in ms_ph],
                      "ms_device_polish": [round(t, 3) for t in ms_po],
                      "ms_device_haplotigs_median": round(statistics.median(ms_h), 3),
                      "ms_device_phase_plus_polish_median": round(statistics.median([x + y for x, y in zip(ms_ph, ms_po)]), 3),
                      "kernel_ms_polish_count_of_polish_reads_median": round(statistics.median(k_po), 4), "kernel_ms": kernels}))


if __name__ == "__main__":
    main()
