"""Seeded low-complexity and repeat-rich inputs for the overlapper tests.  Plain numpy, deterministic: the CPU tests
(tests/test_structured_inputs.py: the oracle alone) and the GPU tests (tests/test_gpu_ava_structured.py: HIP against the
oracle) regenerate the same bytes from the same seeds.  Every other input of the suite is uniform random sequence
(hylight_amd/simulate.py), where the optimal alignment of two reads is essentially unique; here gaps can sit in many
places at equal score, blocks match themselves under a shift, and a query has several chains on one target.

    g, ann = genome(rng, length)                      # genome + annotation [(start, end, kind, period)]
    st = strains(rng, g, ann, n)                      # [Strain(seq, ann)]: substitutions, repeat-unit slippage, 24-36-base indels
    rd = reads(rng, st, n, lo, hi, err_sub, err_ins, err_del)      # [simulate.Read] on both strands, gpos = strain coordinate
    rd = micro_cases(rng)                             # read pairs around one short repeat: the classifier's boundaries

long_set / short_set / contig_set / micro_set are the fixed sets the two test files share.
"""
from __future__ import annotations

import itertools

import numpy as np

from hylight_amd import simulate as S

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
N = ord("N")
_CODE = np.zeros(256, dtype=np.int64)
for _i, _b in enumerate(b"ACGT"):
    _CODE[_b] = _i

SHORT_PERIOD_KINDS = ("homopolymer", "str")          # the kinds with period 1..6: a one-unit indel inside has no unique place
KINDS = ("homopolymer", "long_homopolymer", "str", "str_partial", "tandem", "dispersed+", "dispersed-", "N")


def _uniform(rng, n):
    return BASES[rng.integers(0, 4, size=int(n))]


def _other_base(rng, seq):
    """seq with every base replaced by a different one (ambiguous bases stay)"""
    out = BASES[(_CODE[seq] + rng.integers(1, 4, size=len(seq))) % 4]
    return np.where(seq == N, seq, out).astype(np.uint8)


def _unit(rng, period):
    """a random unit of `period` bases that is not a repeat of a shorter one"""
    while True:
        u = _uniform(rng, period)
        if all(period % d or not (u == np.tile(u[:d], period // d)).all() for d in range(1, period)):
            return u


def genome(rng, length, n_dispersed=4, n_ambiguous=8, p_tandem=0.02):
    """-> (uint8 array of about `length` bases, annotation).  Uniform stretches of 20-200 bases alternate with features:
    homopolymers of 8-60 bases (kind "homopolymer", period 1) and one of 256-400 and one of 401-520 bases
    ("long_homopolymer": beyond the 8-bit span field of a homopolymer-compressed minimizer), short tandem repeats of period
    2-6 and 8-60 bases ("str": whole units, "str_partial": a partial last unit), tandem duplications of period 30-400 with 2-5
    copies ("tandem"), copies of 300-1500 earlier bases of the same genome ("dispersed+", or reverse-complemented
    "dispersed-"; period 0) and single ambiguous bases inside and at the edges of repeats ("N").  Annotation entries are
    (start, end, kind, period), sorted by start; the N entries come last."""
    parts, ann = [], []
    n = 0

    def add(seq, kind=None, period=0):
        nonlocal n
        if kind:
            ann.append((n, n + len(seq), kind, period))
        parts.append(np.ascontiguousarray(seq, dtype=np.uint8))
        n += len(seq)

    long_homo = [(0.2 * length, int(rng.integers(256, 401))), (0.65 * length, int(rng.integers(401, 521)))]
    disp_at = [length * (0.35 + 0.55 * k / max(1, n_dispersed - 1)) for k in range(n_dispersed)]
    n_disp = 0
    while n < length:
        add(_uniform(rng, rng.integers(20, 201)))
        if long_homo and n >= long_homo[0][0]:
            add(np.full(long_homo.pop(0)[1], BASES[rng.integers(0, 4)], dtype=np.uint8), "long_homopolymer", 1)
            continue
        if n_disp < n_dispersed and n >= disp_at[n_disp]:
            ln = int(rng.integers(300, 1501))
            sofar = np.concatenate(parts)
            s = int(rng.integers(0, len(sofar) - ln + 1))
            copy = sofar[s:s + ln]
            add(S.revcomp(copy) if n_disp & 1 else copy.copy(), "dispersed-" if n_disp & 1 else "dispersed+", 0)
            n_disp += 1
            continue
        u = rng.random()
        if u < p_tandem:
            period, copies = int(rng.integers(30, 401)), int(rng.integers(2, 6))
            add(np.tile(_uniform(rng, period), copies), "tandem", period)
        elif u < p_tandem + (1 - p_tandem) / 2:
            add(np.full(int(rng.integers(8, 61)), BASES[rng.integers(0, 4)], dtype=np.uint8), "homopolymer", 1)
        else:
            period = int(rng.integers(2, 7))
            total = int(rng.integers(max(8, 2 * period), 61))
            partial = bool(rng.random() < 0.5)
            if partial and total % period == 0:
                total += -1 if total == 60 else 1
            if not partial:
                total += -total % period                   # (60 is a multiple of every period)
            add(np.tile(_unit(rng, period), total // period + 1)[:total], "str_partial" if total % period else "str", period)
    add(_uniform(rng, rng.integers(20, 201)))
    g = np.concatenate(parts)
    # ambiguous bases: at the first / last base of a repeat and inside one, in turn
    feats = [a for a in ann if a[2] in ("homopolymer", "str", "str_partial", "tandem")]
    pick = rng.choice(len(feats), size=min(n_ambiguous, len(feats)), replace=False)
    amb = []
    for k, f in enumerate(sorted(pick.tolist())):
        s, e = feats[f][0], feats[f][1]
        pos = (s, e - 1, int(rng.integers(s + 1, e - 1)))[k % 3]
        g[pos] = N
        amb.append((pos, pos + 1, "N", 0))
    return g, ann + amb


class Strain:
    __slots__ = ("seq", "ann")

    def __init__(self, seq, ann):
        self.seq = seq        # np.uint8 array
        self.ann = ann        # the genome's annotation in this strain's coordinates


def _apply_edits(seq, ann, edits):
    """edits: [(pos, n_deleted, inserted bases)]; the ones that touch an earlier one are dropped.  -> (sequence, annotation
    carried over: a position inside a deleted range maps to the first base behind the edit)"""
    kept, last_end = [], -1
    for pos, dlen, ins in sorted(edits, key=lambda e: e[0]):
        if pos > last_end and pos + dlen <= len(seq):
            kept.append((pos, dlen, ins))
            last_end = pos + dlen
    out, at = [], 0
    for pos, dlen, ins in kept:
        out += [seq[at:pos], ins]
        at = pos + dlen
    out.append(seq[at:])
    epos = np.array([e[0] for e in kept], dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum([len(e[2]) - e[1] for e in kept])]).astype(np.int64)

    def f(x):
        i = int(np.searchsorted(epos, x, side="left"))            # edits that start before x
        if i and x < kept[i - 1][0] + kept[i - 1][1]:
            return int(kept[i - 1][0] + cum[i - 1] + len(kept[i - 1][2]))
        return int(x + cum[i])
    new_ann = [(f(s), f(e), kind, period) for s, e, kind, period in ann]
    return np.concatenate(out).astype(np.uint8), [a for a in new_ann if a[1] > a[0]]


def strains(rng, g, ann, n=2, sub_rate=0.005, slip_frac=0.5, long_indel_every=4000):
    """-> [Strain]; strain 0 is the genome itself.  Every other strain has substitutions at `sub_rate`, one repeat unit
    gained or lost in a fraction `slip_frac` of the period-1..6 repeats (the slippage indel: every place inside the repeat
    spells the same sequence) and an inserted or deleted stretch of 24-36 bases about every `long_indel_every` bases."""
    out = [Strain(g.copy(), list(ann))]
    for _ in range(1, n):
        s = g.copy()
        pos = np.nonzero((rng.random(len(s)) < sub_rate) & (s != N))[0]
        s[pos] = _other_base(rng, s[pos])
        edits = []
        for a, e, kind, period in ann:
            if 1 <= period <= 6 and e - a >= 3 * period and rng.random() < slip_frac:
                if rng.random() < 0.5:
                    edits.append((a, period, np.zeros(0, dtype=np.uint8)))            # one unit lost
                else:
                    edits.append((a, 0, g[a:a + period].copy()))                      # one unit gained
        for k in range(max(1, len(s) // long_indel_every)):
            p = int(rng.integers(100, len(s) - 100))
            ln = int(rng.integers(24, 37))
            edits.append((p, ln, np.zeros(0, dtype=np.uint8)) if k & 1 else (p, 0, _uniform(rng, ln)))
        out.append(Strain(*_apply_edits(s, ann, edits)))
    return out


def reads(rng, strain_list, n, lo, hi, err_sub=0.004, err_ins=0.002, err_del=0.002, name="s"):
    """n reads of lo..hi strain bases (uniform), strain and strand drawn evenly, per-base substitution / insertion / deletion
    errors; an inserted base repeats its left neighbour half of the time.  -> [simulate.Read], gpos = strain coordinate
    of every base (-1: inserted)."""
    out = []
    for i in range(n):
        st = int(rng.integers(0, len(strain_list)))
        g = strain_list[st].seq
        ln = int(min(rng.integers(lo, hi + 1), len(g)))
        s = int(rng.integers(0, len(g) - ln + 1))
        frag = g[s:s + ln].copy()
        u = rng.random(ln)
        is_del = u < err_del
        is_sub = (u >= err_del) & (u < err_del + err_sub) & (frag != N)
        frag[is_sub] = _other_base(rng, frag[is_sub])
        keep = ~is_del
        keep[0] = keep[-1] = True
        base = frag[keep]
        gp = np.arange(s, s + ln, dtype=np.int64)[keep]
        n_ins = int(rng.binomial(len(base), err_ins))
        if n_ins:
            ipos = np.sort(rng.integers(1, len(base), size=n_ins))
            rand = _uniform(rng, n_ins)
            ibase = np.where(rng.random(n_ins) < 0.5, base[ipos - 1], rand)
            base = np.insert(base, ipos, ibase)
            gp = np.insert(gp, ipos, -1)
        rev = bool(rng.random() < 0.5)
        if rev:
            base, gp = S.revcomp(base), gp[::-1]
        out.append(S.Read(f"{name}{i:04d}", np.ascontiguousarray(base), np.ascontiguousarray(gp), st, s, s + ln, rev))
    return out


MICRO_PERIODS = (1, 2, 3, 4, 6)
MICRO_COPIES = (5, 12)
MICRO_DELTAS = ("0", "p1", "m1", "pu", "mu")          # nothing / one base more / one base less / one unit more / one unit less
MICRO_SITES = ("first", "middle", "last", "outside")
MICRO_FLANK = 350


def micro_cases(rng, periods=MICRO_PERIODS, copies=MICRO_COPIES, deltas=MICRO_DELTAS, flank=MICRO_FLANK):
    """Pairs of reads `<case>_a`, `<case>_b` that share two unique random flanks around a core of `copies` units of a random
    `period`-base unit.  Read b differs from read a by the case's delta in the core (a base or a unit gained or lost at a unit
    boundary a third into the core) and by substitutions at every subset of four sites: the first base of the core, a base
    two thirds into it, its last base, the second flank base behind it; b is given on both strands.  The case is spelled
    in the name: p<period>c<copies>_<delta>_<one digit per site>_<f|r>.  A second family, end<period of the repeat the reads
    end in, 0: none>_k<substitutions>_d<distance of the last one from the end>_<f|r>, has its differences inside the end
    extension.  -> [simulate.Read] (a, b, a, b, ...)"""
    out = []
    for period, cop, delta in itertools.product(periods, copies, deltas):
        if period == 1 and delta in ("pu", "mu"):
            continue                                   # (the unit is the base)
        for mask in range(16):
            for strand in "fr":
                unit = _unit(rng, period)
                left, right = _uniform(rng, flank), _uniform(rng, flank)
                # the flanks must not continue the repeat
                while left[-1] == unit[-1]:
                    left[-1] = BASES[rng.integers(0, 4)]
                while right[0] == unit[0]:
                    right[0] = BASES[rng.integers(0, 4)]
                core = np.tile(unit, cop)
                a = np.concatenate([left, core, right])
                b = a.copy()
                c0, cl = flank, len(core)
                sites = (c0, c0 + (2 * cl) // 3, c0 + cl - 1, c0 + cl + 1)
                for k in range(4):
                    if mask >> k & 1:
                        b[sites[k]:sites[k] + 1] = _other_base(rng, b[sites[k]:sites[k] + 1])
                at = c0 + max(1, (cl // 3) // period) * period        # a unit boundary (left of the "middle" site)
                if delta == "p1":
                    b = np.insert(b, at, b[at - 1])
                elif delta == "m1":
                    b = np.delete(b, at)
                elif delta == "pu":
                    b = np.insert(b, at, unit)
                elif delta == "mu":
                    b = np.delete(b, np.arange(at, at + period))
                if strand == "r":
                    b = S.revcomp(b)
                case = f"p{period}c{cop:02d}_{delta}_{mask:04b}_{strand}"
                out.append(S.Read(case + "_a", np.ascontiguousarray(a), None, 0, 0, len(a), False))
                out.append(S.Read(case + "_b", np.ascontiguousarray(b), None, 0, 0, len(a), strand == "r"))
    # the end extensions: k substitutions close to the right end of b, the last one d bases before the end (with one
    # substitution the extension stops before it or runs to the end, depending on d), the reads ending in uniform sequence
    # or inside a repeat of period 1, 2 or 3
    for tail, k, d, strand in itertools.product((0, 1, 2, 3), (1, 2, 3), range(1, 9), "fr"):
        a = _uniform(rng, 2 * flank)
        if tail:
            a[-24:] = np.tile(_unit(rng, tail), 24)[:24]
        b = a.copy()
        for off in (0, 3, 7)[:k]:
            at = len(b) - d - off
            b[at:at + 1] = _other_base(rng, b[at:at + 1])
        if strand == "r":
            b = S.revcomp(b)
        case = f"end{tail}_k{k}_d{d}_{strand}"
        out.append(S.Read(case + "_a", np.ascontiguousarray(a), None, 0, 0, len(a), False))
        out.append(S.Read(case + "_b", np.ascontiguousarray(b), None, 0, 0, len(a), strand == "r"))
    return out


# ---- the fixed sets of the two test files -------------------------------------------------------------------------------

LONG_SEEDS = (8101, 8102)
SHORT_SEED = 8201
CONTIG_SEED = 8301
MICRO_SEED = 8401


def population(seed, length=45_000, n_strains=2):
    rng = np.random.default_rng(seed)
    g, ann = genome(rng, length)
    return rng, strains(rng, g, ann, n_strains)


def long_set(seed):
    """150 reads of 3-9 kb, 0.4 % / 0.2 % / 0.2 % errors, two strains of a 45 kb genome -> (reads, strains)"""
    rng, st = population(seed)
    return reads(rng, st, 150, 3000, 9000), st


def short_set(seed=SHORT_SEED):
    """1500 reads of 150-250 bases of the same kind of population -> (reads, strains)"""
    rng, st = population(seed)
    return reads(rng, st, 1500, 150, 250), st


def contig_set(seed=CONTIG_SEED):
    """50 error-free "contigs" of 2-8 kb cut from the strains (the input of the bandwidth-0 call) -> (reads, strains)"""
    rng, st = population(seed)
    return reads(rng, st, 50, 2000, 8000, 0.0, 0.0, 0.0, name="c"), st


def micro_set(seed=MICRO_SEED):
    return micro_cases(np.random.default_rng(seed))


def repeat_mask(strain):
    """bool per strain base: inside an annotated period-1..6 repeat"""
    m = np.zeros(len(strain.seq), dtype=bool)
    for s, e, kind, period in strain.ann:
        if 1 <= period <= 6:
            m[s:e] = True
    return m
