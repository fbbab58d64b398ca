"""Pin the short-read clustering to the reference itself: run HyLight's four scripts, unmodified, on seeded inputs from
tests/cluster_inputs.py, the way HyLight.py:215-226 does (cwd = a fresh tmp/, then its cmd_rm), and write one manifest per
case: tests/golden/fxH_cluster_<case>.json with the generator parameters, the sha256 of both inputs, the
{relative path: [bytes, sha256]} of every output file (null for a directory), and the stats of tests/cluster_model.py,
which must give the same tree (the maker stops otherwise).

    python tests/golden/make_goldens_cluster.py --reference HYLIGHT_CHECKOUT [--case NAME]

Needs only Python with numpy and pandas (the reference scripts' imports); no GPU.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)

import cluster_inputs as CI  # noqa: E402
import cluster_model as CM  # noqa: E402

# name -> (make_case parameters, size, threads)
CASES = {
    # every header oddity; size 5 keeps every cluster under 20 (an empty tree), size 30 gives one
    "hand_s5": (dict(seed=1, n_pairs=40, n_rows=200, odd=True), 5, 1),
    "hand_s30": (dict(seed=1, n_pairs=40, n_rows=200, odd=True), 30, 1),
    # ~3000 pairs, a slicing remainder (K % threads != 0)
    "mid": (dict(seed=2, n_pairs=3000, n_rows=20000, name_fmt=CI.LONG_NAMES), 40, 4),
    # >= 5 chunks of 2.6 MB with 2 per session: the last session is short; seed chosen for strict_rejects >= 1
    "multi": (dict(seed=3, n_pairs=20000, n_rows=95000, name_fmt=CI.LONG_NAMES), 40, 2),
    # threads 64: slices 60 .. 63 are dropped
    "t64": (dict(seed=4, n_pairs=3000, n_rows=20000, name_fmt=CI.LONG_NAMES), 40, 64),
    # fewer kept nodes than threads: {} and an empty fq_<size>/
    "few": (dict(seed=5, n_pairs=30, n_rows=300), 25, 50),
}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def run_reference(ref, fq_path, paf_path, size, threads, tmp):
    """HyLight.py:215-226 with outdir1 = tmp"""
    script = os.path.join(ref, "script")
    py = sys.executable
    cmds = [
        [py, os.path.join(script, "get_readnames.py"), fq_path, os.path.join(tmp, "readnames.txt")],
        [py, os.path.join(script, "bin_pointer_limited_filechunks_shortpath2.py"), paf_path, "readnames.txt", str(size),
         CM.RUN_ID, str(threads)],
        [py, os.path.join(script, "getclusters.py"), f"{CM.RUN_ID}_max{size}_final", str(threads)],
        [py, os.path.join(script, "get_fq_cluster.py"), f"{CM.RUN_ID}_max{size}_final_clusters_grouped.json", fq_path,
         f"{tmp}//fq_{size}"],
    ]
    for c in cmds:
        subprocess.run(c, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for f in os.listdir(tmp):                                            # cmd_rm
        if f.startswith("Chunkfile") or f in (f"{CM.RUN_ID}_max{size}_final_clustersizes.json",
                                              f"{CM.RUN_ID}_max{size}_final_clusters_unchained.json",
                                              f"{CM.RUN_ID}_max{size}_final_clusters.json"):
            os.remove(os.path.join(tmp, f))


def make(name, ref):
    params, size, threads = CASES[name]
    fq, paf = CI.make_case(**params)
    work = tempfile.mkdtemp(prefix="hlmi_cluster_golden_")
    try:
        fq_path, paf_path = os.path.join(work, "reads.fq"), os.path.join(work, "shortr2.paf")
        open(fq_path, "wb").write(fq)
        open(paf_path, "wb").write(paf)
        tmp = os.path.join(work, "tmp")
        os.makedirs(tmp)
        run_reference(ref, fq_path, paf_path, size, threads, tmp)
        got = CM.tree(tmp)
    finally:
        shutil.rmtree(work)
    files, st = CM.run(paf, fq, size, threads)
    if CM.manifest_of(files) != CM.manifest_of(got):
        diff = sorted(set(CM.manifest_of(files).items()) ^ set((k, None if v is None else tuple(v))
                                                              for k, v in CM.manifest_of(got).items()))
        raise SystemExit(f"{name}: cluster_model.py differs from the reference: {str(diff)[:2000]}")
    man = {"case": name, "params": params, "size": size, "threads": threads,
           "inputs": {"fastq": [len(fq), sha(fq)], "paf": [len(paf), sha(paf)]},
           "outputs": CM.manifest_of(got), "model_stats": st}
    out = os.path.join(HERE, f"fxH_cluster_{name}.json")
    with open(out, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    print(name, st, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="HyLight checkout (holds script/)")
    ap.add_argument("--case", action="append", help="only these cases (default: all)")
    a = ap.parse_args()
    for name in a.case or CASES:
        make(name, a.reference)


if __name__ == "__main__":
    main()
