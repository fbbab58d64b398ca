"""POLYTE's evidence threshold table (script/min_ev_table.py, called from polyte.tune_params.py:813-839): for every variation
distance the evidence a haplotype of coverage `hcov` is expected to give, and the smallest evidence count that sequencing errors
alone reach with probability below 10^-3.  hlmi_vq_branch_* reads the file as evidence_threshold_table.tsv.

    python -m hylight_amd.min_ev -l READLEN -i INTSEG --stddev S --hcov C [-o FILE]

The reference takes the normal CDF from scipy; this module has it from math.erf / math.erfc with the case split of cephes'
ndtr, which scipy evaluates (DESIGN.md section 4.3 states how far the two agree).
"""
from __future__ import annotations

import argparse
import math
import os
import sys

SEQ_ERR = 0.01           # min_ev_table.py:55-56
ACCURACY = 1e-3
FILENAME = "evidence_threshold_table.tsv"


def ndtr(a):
    """The standard normal CDF as cephes' ndtr computes it: erf near zero, erfc in the tails."""
    x = a * math.sqrt(0.5)
    z = abs(x)
    if z < math.sqrt(0.5):
        return 0.5 + 0.5 * math.erf(x)
    y = 0.5 * math.erfc(z)
    return 1.0 - y if x > 0 else y


def choose(n, k):
    """min_ev_table.py:145-151 - exact integers."""
    return math.comb(n, min(k, n - k))


def find_min_ev(c, m1, seq_err=SEQ_ERR, accuracy=ACCURACY):
    """findMinEv (:132-143): the smallest m1 whose error tail over range(m1, c) - m = c is left out, as there - is at most
    `accuracy`."""
    def tail(lo):
        p = 0
        for m in range(lo, c):
            p += choose(c, m) * seq_err ** m * (1 - seq_err) ** (c - m)
        return p

    p1 = tail(m1)
    while p1 > accuracy:
        m1 += 1
        p1 = tail(m1)
    return m1


def table(readlen, intseg, stddev, hcov):
    """-> [(dist, exp_ev, min_ev)] for dist = 1, 2, ..: the rows of min_ev_table.py:76-111.  The last row is the first with
    exp_ev == 0, or the last distance not above fragsize + 2 * stddev."""
    fragsize = intseg + 2 * readlen
    if not fragsize > 0:
        raise ValueError(f"min_ev.table: fragment size {fragsize} is not positive")
    cdf = {}

    def norm_cdf(v):
        if v not in cdf:
            cdf[v] = ndtr((v - intseg) / stddev)
        return cdf[v]

    exp_evs = []
    dist = 1
    while True:
        exp_ev = 0
        exp_ev += hcov * max(0, readlen - dist) / readlen                  # single-end evidence (:79)
        p_l = []
        for x in range(0, int(math.floor(readlen))):                       # paired-end evidence (:81-85, prob :117-130)
            p1 = norm_cdf(dist - 2 * readlen + x + 1)
            p2 = norm_cdf(dist - readlen + x)
            p_l.append(p2 - p1)
        exp_ev += hcov * sum(p_l) / readlen
        exp_ev = int(math.floor(exp_ev))
        exp_evs.append(exp_ev)
        if exp_ev == 0:
            break
        dist += 1
        if dist > fragsize + 2 * stddev:
            break
    threshold = {}
    min_ev = 1
    for ev in sorted(set(exp_evs)):                                        # thresholds in increasing order (:99-104)
        min_ev = find_min_ev(ev, min_ev)
        threshold[ev] = min_ev
    return [(i + 1, ev, threshold[ev]) for i, ev in enumerate(exp_evs)]


def text(readlen, intseg, stddev, hcov):
    """The file as min_ev_table.py:58-111 writes it."""
    head = ("# INPUT:\n# readlen {}\n# intseg {}\n# stddev {}\n# hcov {}\n# OUTPUT:\n# dist\texp_ev\tmin_ev\n"
            .format(readlen, intseg, stddev, hcov))
    return head + "".join(f"{d}\t{e}\t{m}\n" for d, e, m in table(readlen, intseg, stddev, hcov))


def header_params(path):
    """The `# name value` lines of an existing table (build_threshold_table, polyte.tune_params.py:817-825)."""
    params = {}
    with open(path) as f:
        for line in f:
            if line[0] != "#":
                continue
            parts = line.rstrip("\n").split()
            if len(parts) != 3:
                continue
            params[parts[1]] = float(parts[2])
    return params


def write(path, readlen, intseg, stddev, hcov):
    """build_threshold_table (:813-839): an existing file whose four header values are the ones asked for is kept as it is.
    The values are floats, as argparse hands them to the reference.  -> True when the file was (re)built."""
    readlen, intseg, stddev, hcov = float(readlen), float(intseg), float(stddev), float(hcov)
    if os.path.isfile(path):
        p = header_params(path)
        if (readlen, intseg, stddev, hcov) == tuple(p.get(k) for k in ("readlen", "intseg", "stddev", "hcov")):
            return False
    with open(path, "w") as f:
        f.write(text(readlen, intseg, stddev, hcov))
    return True


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m hylight_amd.min_ev", description=__doc__.split("\n\n")[0])
    p.add_argument("-l", dest="readlen", type=float, required=True)
    p.add_argument("-i", dest="intseg", type=float, required=True)
    p.add_argument("-s", "--stddev", dest="stddev", type=float, required=True)
    p.add_argument("-c", "--hcov", dest="hcov", type=float, required=True)
    p.add_argument("-o", dest="outfile", default="exp_ev_table.tsv")
    a = p.parse_args(argv)
    with open(a.outfile, "w") as f:
        f.write(text(a.readlen, a.intseg, a.stddev, a.hcov))
    return 0


if __name__ == "__main__":
    sys.exit(main())
