"""HyLight's short-read clustering (script/HyLight.py:215-226: get_readnames.py, bin_pointer_limited_filechunks_shortpath2.py,
getclusters.py, get_fq_cluster.py) in one call of libhylight_mi.so (hlmi_cluster_short).

    python -m hylight_amd.cluster_short shortr2.paf short_reads.fq -o tmp/ [--size 15000] [-t 20]

Writes readnames.txt, HiStrain_max<size>_final_clusters_grouped.json and fq_<size>/<cid>/<cid>.{1,2}.fq into the output
directory, byte for byte as the reference scripts leave them (cwd = tmp/, after HyLight's cmd_rm).  Prints the stats as
one JSON line.  Exit status 0 on success, 4 (EXIT_REFUSED) for an input the implementation refuses (HLMI_EINVAL: see
include/hylight_mi.h).
"""
from __future__ import annotations

import argparse
import json
import sys

from . import api

EXIT_REFUSED = 4


def build_parser():
    p = argparse.ArgumentParser(prog="python -m hylight_amd.cluster_short", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("paf", help="scored 14-column PAF of the short reads (shortr2.paf)")
    p.add_argument("fastq", help="the short reads (paired FASTQ, /1 and /2 headers)")
    p.add_argument("-o", "--out", dest="out", required=True, help="output directory (HyLight's tmp/)")
    p.add_argument("--size", type=int, default=15000, help="cluster size cap (HyLight --size)")
    p.add_argument("-t", "--threads", type=int, default=20, help="HyLight -t: chunks per session and getclusters' slices")
    p.add_argument("--window_bytes", type=int, default=0, help="PAF bytes per upload (0: the library's default)")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    try:
        st = api.cluster_short(a.paf, a.fastq, a.out, size=a.size, threads=a.threads, window_bytes=a.window_bytes)
    except api.HlmiError as e:
        if e.code == -1:                      # HLMI_EINVAL: refused input
            sys.stderr.write(f"hylight_amd.cluster_short: {e}\n")
            return EXIT_REFUSED
        raise
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
