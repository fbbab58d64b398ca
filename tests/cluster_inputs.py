"""Seeded inputs for the short-read clustering step (script/HyLight.py:211-262): paired FASTQ and a score-sorted
14-column PAF in the layout the library writes (shortr2.paf).  Plain numpy, so the GPU tests, the golden maker and
tools/cluster_time.py regenerate the same bytes from the same parameters.

    fastq, paf = make_case(seed, n_pairs, n_rows, group=40, odd=False)

PAF rows only name reads that have a /1 header (the reference truncates a chunk silently on any other name).  Reads come
in groups of `group` consecutive pairs; most rows join two reads of one group, the rest two reads anywhere, so clusters
grow to the size cap the way strains do.
"""
from __future__ import annotations

import numpy as np

LONG_NAMES = "HiStrain.sim.short.%08d"
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)

# names of the odd pairs - the header oddities of get_readnames.py / get_fq_cluster.py: a '/' inside the name
# (demux looks up its last part, another read's name), '@' inside the name, an empty name, a blank inside the name.
# make_case(odd=True) adds single records on top: "@x/1y/2" ('/1' not at the end: a readnames entry "x/1y" whose record
# is a mate 2 and whose demux name is "1y"), a /2-only record and a header without '/'.
ODD = [b"a/b", b"b", b"c@d", b"d", b"", b"e f"]     # "a/b" demuxes as "b", "c@d" as "d"; "@/1" is the empty name


def _seq(rng, n, L):
    return BASES[rng.integers(0, 4, size=(n, L))]


def _fastq_records(names, mates, seqs, quals):
    out = []
    for nm, m, s, q in zip(names, mates, seqs, quals):
        out.append(b"@" + nm + m + b"\n" + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return out


def make_case(seed, n_pairs, n_rows, group=40, odd=False, read_len=20, cross=0.05, name_fmt="r%d"):
    """-> (fastq bytes, paf bytes).  n_pairs regular pairs r<i>/1, r<i>/2; with odd=True the ODD names and a few odd
    records (a /2-only record, a header without '/', a header '@x/1y/2') join in.  n_rows PAF rows, sorted by a
    descending score in column 13.  name_fmt LONG_NAMES gives rows of ~125 bytes, as real ones are."""
    rng = np.random.default_rng(seed)
    names = [(name_fmt % i).encode() for i in range(n_pairs)]
    if odd:
        names += ODD
    n_paired = len(names)
    recs = []
    seqs = _seq(rng, 2 * n_paired, read_len)
    quals = np.full((2 * n_paired, read_len), ord("I"), dtype=np.uint8)
    for i, nm in enumerate(names):
        recs.append((nm, b"/1", 2 * i))
        recs.append((nm, b"/2", 2 * i + 1))
    fq_parts = []
    for nm, m, k in recs:
        fq_parts += _fastq_records([nm], [m], [seqs[k]], [quals[k]])
    if odd:
        extra_s = _seq(rng, 4, read_len)
        q = np.full(read_len, ord("#"), dtype=np.uint8)
        fq_parts.insert(7, _fastq_records([b"only2"], [b"/2"], [extra_s[0]], [q])[0])      # /2-only record
        fq_parts.insert(3, _fastq_records([b"noslash"], [b""], [extra_s[1]], [q])[0])      # header without '/'
        fq_parts.append(_fastq_records([b"r1"], [b"/2"], [extra_s[2]], [q])[0])           # a second mate-2 record of r1
        fq_parts.insert(11, _fastq_records([b"x/1y"], [b"/2"], [extra_s[3]], [q])[0])     # '/1' not at the end
        names.insert(5, b"x/1y")
    fastq = b"".join(fq_parts)
    return fastq, paf_rows(rng, names, n_rows, group, cross)


def paf_rows(rng, names, n_rows, group=40, cross=0.05, descending=None):
    """n_rows PAF rows over `names` (the readnames keys, each row's names get a /1 or /2 suffix), score-sorted"""
    n = len(names)
    # endpoints mostly inside one group of consecutive reads
    g = max(1, min(group, n))
    a = rng.integers(0, n, size=n_rows)
    same = rng.random(n_rows) >= cross
    base = (a // g) * g
    b_in = np.minimum(base + rng.integers(0, g, size=n_rows), n - 1)
    b_any = rng.integers(0, n, size=n_rows)
    b = np.where(same, b_in, b_any)
    score = np.sort(rng.random(n_rows))[::-1] if descending is None else descending
    ql = rng.integers(100, 300, size=n_rows)
    qs = rng.integers(0, 50, size=n_rows)
    ma = rng.integers(60, 99, size=n_rows)
    strand = rng.integers(0, 2, size=n_rows)
    m1 = rng.integers(1, 3, size=n_rows)
    m2 = rng.integers(1, 3, size=n_rows)
    lines = []
    for i in range(n_rows):
        q = names[a[i]] + b"/%d" % m1[i]
        t = names[b[i]] + b"/%d" % m2[i]
        L, s = int(ql[i]), int(qs[i])
        e = min(L, s + int(ma[i]) + 40)
        lines.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t\n" % (
            q, L, s, e, b"-" if strand[i] else b"+", t, L + 7, s + 3, e + 3, int(ma[i]), e - s,
            score[i], 0.9 + 0.1 * score[i], 0.95 + 0.05 * score[i]))
    return b"".join(lines)


def write_case(dirpath, seed, n_pairs, n_rows, **kw):
    """make_case into dirpath/reads.fq and dirpath/shortr2.paf -> (fastq path, paf path)."""
    import os
    fq, paf = make_case(seed, n_pairs, n_rows, **kw)
    fp, pp = os.path.join(dirpath, "reads.fq"), os.path.join(dirpath, "shortr2.paf")
    with open(fp, "wb") as f:
        f.write(fq)
    with open(pp, "wb") as f:
        f.write(paf)
    return fp, pp
