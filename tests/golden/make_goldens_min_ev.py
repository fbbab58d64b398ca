#!/usr/bin/env python3
"""Golden threshold tables for hylight_amd/min_ev.py, made by RUNNING the reference's own min_ev_table.py (it needs scipy) the
way polyte.tune_params.py:832-838 calls it.  Only its outputs are committed.

Usage: python tests/golden/make_goldens_min_ev.py <the reference's script directory>
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (readlen, insert_size, stddev, hcov); intseg = insert_size - 2 * readlen (polyte.tune_params.py:333-336)
CASES = {
    "hylight": (150.0, 450.0, 27.0, 10.0),          # HyLight.py:236-239 with 150-base reads
    "len250": (250.0, 450.0, 27.0, 10.0),           # HyLight's default --average_read_len: a negative intseg of -50
    "len148_7": (148.7, 450.0, 27.0, 10.0),         # an average that is no integer
    "negseg": (150.0, 250.0, 27.0, 10.0),           # mates that overlap
    "hcov3": (150.0, 450.0, 27.0, 3.0),             # a short table
}


def main():
    script = os.path.join(sys.argv[1], "min_ev_table.py")
    for name, (readlen, insert, stddev, hcov) in CASES.items():
        intseg = insert - 2 * readlen
        out = os.path.join(HERE, f"min_ev_{name}.tsv")
        subprocess.check_call(f"{sys.executable} {script} -l {readlen} -i {intseg} --stddev {stddev} --hcov {hcov} -o {out}",
                              shell=True, stdout=subprocess.DEVNULL)
        print(out)


if __name__ == "__main__":
    main()
