"""Inputs of tests/test_gpu_polish_reads.py (hlmi_polish_reads against the chain hlmi_ava + hlmi_polish): small contigs cut
from one random genome with errors put in, error-free reads of that genome, and what a test needs to know of the chain's PAF.
Everything comes from seeds; nothing is read from a file.

-> Input(contigs [(name, bases)], reads [(name, bases)], short, opts): `short` chooses the overlapper's constants (every pair,
pair_once = 0, as at the driver's polishing sites), `opts` are hlmi_polish_opts fields."""
import collections
import re

import numpy as np

Input = collections.namedtuple("Input", "contigs reads short opts")
_RC = bytes.maketrans(b"ACGTacgtNR", b"TGCAtgcaNY")


def revcomp(b):
    return b.translate(_RC)[::-1]


def genome(rng, n):
    return bytes(b"ACGT"[k] for k in rng.integers(0, 4, size=n))


def with_errors(rng, seg, every=75):
    """seg with a substitution, a one-base deletion or a one-base insertion (in turn) about every `every` bases, as many
    deletions as insertions: the length stays."""
    out, p, kind = bytearray(), int(rng.integers(20, 40)), 0
    prev = 0
    n_kinds = [0, 0, 0]
    while p < len(seg) - 20:
        out += seg[prev:p]
        k = kind % 3
        if k == 0:
            out.append(b"ACGT"[(b"ACGT".find(seg[p:p + 1]) + 1 + int(rng.integers(3))) % 4])
        elif k == 2:
            out += bytes([b"ACGT"[int(rng.integers(4))], seg[p]])
        n_kinds[k] += 1                                        # (k == 1: the base is missing)
        prev = p + 1
        kind += 1
        p += every + int(rng.integers(-15, 16))
    out += seg[prev:]
    if n_kinds[1] > n_kinds[2]:                                # one deletion more than insertions: give the base back at the end
        out += b"A"
    return bytes(out)


def sample_reads(rng, g, n, lo, hi, prefix="r", span=None):
    """n error-free reads of lo..hi bases from g[span], every third one reverse-complemented, in shuffled order"""
    a, b = span or (0, len(g))
    reads = []
    for k in range(n):
        L = int(rng.integers(lo, hi + 1))
        s = int(rng.integers(a, b - L + 1))
        seq = g[s:s + L]
        reads.append((f"{prefix}{k}", revcomp(seq) if k % 3 == 2 else seq))
    order = rng.permutation(n)
    return [reads[i] for i in order]


def every_kind_long():
    """three contigs of 1 500, 2 500 and 900 bases (rows cross the 1024-position tile edge), ~60 reads of 600 - 1 200 bases"""
    rng = np.random.default_rng(9101)
    g = genome(rng, 4900)
    cuts = [(0, 1500), (1500, 4000), (4000, 4900)]
    contigs = [(f"c{k}", with_errors(rng, g[a:b])) for k, (a, b) in enumerate(cuts)]
    assert [len(s) for _, s in contigs] == [1500, 2500, 900]
    return Input(contigs, sample_reads(rng, g, 60, 600, 1200), False, dict(min_len=300, min_iden=0.9))


def every_kind_short():
    """one contig of 2 500 bases, 150-base reads, the short constants, min_len 70"""
    rng = np.random.default_rng(9102)
    g = genome(rng, 2500)
    return Input([("c0", with_errors(rng, g))], sample_reads(rng, g, 220, 150, 150, prefix="s"), True, dict(min_len=70))


def tie_between_contigs():
    """two contigs around one identical 800-base segment, reads wholly inside it: two rows of equal te - ts per read"""
    rng = np.random.default_rng(9103)
    x = genome(rng, 800)
    contigs = [("cA", genome(rng, 600) + x + genome(rng, 500)), ("cB", genome(rng, 400) + x + genome(rng, 700))]
    return Input(contigs, sample_reads(rng, x, 12, 500, 700), False, dict(min_len=300))


def non_voting_and_case():
    """one contig of 1 200 bases, lower case on [300, 500) and [1000, 1100); reads cover [0, 950) densely and [950, 1200) with
    one read (below min_cov 3); the reads hold N, R, U and lower-case bases"""
    rng = np.random.default_rng(9104)
    g = genome(rng, 1200)
    c = bytearray(with_errors(rng, g))
    for a, b in ((300, 500), (1000, 1100)):
        c[a:b] = bytes(c[a:b]).lower()
    reads = sample_reads(rng, g, 36, 400, 700, span=(0, 950)) + [("tail", g[700:1200])]
    out = []
    for k, (name, seq) in enumerate(reads):
        s = bytearray(seq)
        for j, p in enumerate(rng.choice(len(s), size=12, replace=False)):
            p = int(p)
            if j < 3:
                s[p] = ord("N")
            elif j < 6:
                s[p] = ord("R")
            elif j < 8:
                s[p] = ord("U") if k % 2 else ord("u")
            else:
                s[p] |= 0x20
        out.append((name, bytes(s)))
    return Input([("c0", bytes(c))], out, False, dict(min_len=200))


def contig_without_rows(include_unpolished):
    """c1 is random sequence no read matches"""
    rng = np.random.default_rng(9105)
    g = genome(rng, 2400)
    contigs = [("c0", with_errors(rng, g[:1200])), ("c1", genome(rng, 700)), ("c2", with_errors(rng, g[1200:]))]
    return Input(contigs, sample_reads(rng, g, 40, 500, 900), False, dict(min_len=300, include_unpolished=include_unpolished))


def no_read_matches():
    rng = np.random.default_rng(9106)
    contigs = [("c0", genome(rng, 1100)), ("c1", genome(rng, 600))]
    return Input(contigs, sample_reads(rng, genome(rng, 3000), 20, 500, 900), False, {})


def fasta(recs):
    return b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs)


# ---- the chain's PAF, as far as a test asks it something -----------------------------------------------------------------
def paf_rows(data):
    """-> [dict(q, t, ts, te, n_eq, n_all)] in line order; n_eq / n_all from the cg:Z: tag, as hlmi_polish counts them"""
    rows = []
    for line in data.split(b"\n"):
        if not line:
            continue
        f = line.split(b"\t")
        assert f[-1].startswith(b"cg:Z:")
        ops = [(int(n), o) for n, o in re.findall(rb"(\d+)([=XID])", f[-1][5:])]
        rows.append(dict(q=f[0], t=f[5], ts=int(f[7]), te=int(f[8]), n_eq=sum(n for n, o in ops if o == b"="),
                         n_all=sum(n for n, _ in ops)))
    return rows


def expect_selected(rows, min_len, min_iden):
    """reads with at least one row the selection keeps (include/hylight_mi.h: hlmi_polish, row selection)"""
    return len({r["q"] for r in rows if r["q"] != r["t"] and r["te"] > r["ts"] and r["te"] - r["ts"] >= min_len
                and r["n_eq"] / r["n_all"] >= min_iden})
