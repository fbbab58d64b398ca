"""CPU: the structured-sequence generator (tests/structured_inputs.py) and the oracle on its output.  The GPU tests of
tests/test_gpu_ava_structured.py hold the HIP overlapper equal to the oracle on these inputs, byte for byte; here the
oracle's own rows are checked to be true alignments (so that the parity is not agreement on nonsense) and the inputs to
contain what they are for: several rows per read pair, gaps inside short-period repeats, long gaps - counted on the
oracle's output alone."""
import collections
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import structured_inputs as SI  # noqa: E402
from hylight_amd import simulate as S  # noqa: E402
from oracle import ava as OA  # noqa: E402

OPS = re.compile(r"(\d+)([=XID])")


def _fasta_bytes(reads):
    return b"".join(b">" + r.name.encode() + b"\n" + r.seq.tobytes() + b"\n" for r in reads)


def _oracle_rows(tmp_path, reads, opts=None, tag="o"):
    fa = tmp_path / f"{tag}.fa"
    S.write_fasta(reads, fa)
    OA.ava(fa, fa, tmp_path / f"{tag}.paf", opts)
    return [l.split("\t") for l in open(tmp_path / f"{tag}.paf").read().split("\n")[:-1]]


def check_true_alignments(rows, reads, on_gap=None):
    """Every row's cg:Z: string spells the two reads: '=' columns are equal bases, 'X' columns differ, the op lengths add
    up to the coordinates, columns 10 / 11 are the column sums.  on_gap(query read, target read, op, index of the gap's
    first base in the query read's own orientation / in the target read, length) sees every I / D op."""
    by = {r.name: r for r in reads}
    for c in rows:
        assert c[-1].startswith("cg:Z:"), c[:12]
        ops = [(int(k), o) for k, o in OPS.findall(c[-1][5:])]
        assert "".join(f"{k}{o}" for k, o in ops) == c[-1][5:]
        q, t = by[c[0]], by[c[5]]
        assert int(c[1]) == len(q.seq) and int(c[6]) == len(t.seq)
        assert sum(k for k, o in ops if o in "=XI") == int(c[3]) - int(c[2])
        assert sum(k for k, o in ops if o in "=XD") == int(c[8]) - int(c[7])
        assert sum(k for k, o in ops if o == "=") == int(c[9]) and sum(k for k, o in ops) == int(c[10])
        rev = c[4] == "-"
        qs = S.revcomp(q.seq) if rev else q.seq
        qpos = len(qs) - int(c[3]) if rev else int(c[2])
        ts, tpos = t.seq, int(c[7])
        for k, o in ops:
            if o == "=":
                assert (qs[qpos:qpos + k] == ts[tpos:tpos + k]).all(), (c[0], c[5], qpos, tpos)
            elif o == "X":
                assert (qs[qpos:qpos + k] != ts[tpos:tpos + k]).all(), (c[0], c[5], qpos, tpos)
            elif on_gap is not None:
                on_gap(q, t, o, len(qs) - qpos - k if rev else qpos, tpos, k)
            if o in "=XI":
                qpos += k
            if o in "=XD":
                tpos += k


def test_generator_is_deterministic():
    for make in (lambda: SI.long_set(SI.LONG_SEEDS[0])[0], lambda: SI.short_set()[0], lambda: SI.contig_set()[0], SI.micro_set):
        assert _fasta_bytes(make()) == _fasta_bytes(make())
    assert _fasta_bytes(SI.long_set(SI.LONG_SEEDS[0])[0]) != _fasta_bytes(SI.long_set(SI.LONG_SEEDS[1])[0])
    a, b = SI.long_set(SI.LONG_SEEDS[0])[0], SI.long_set(SI.LONG_SEEDS[0])[0]
    assert all((x.gpos == y.gpos).all() for x, y in zip(a, b))


@pytest.mark.parametrize("seed", SI.LONG_SEEDS + (SI.SHORT_SEED, SI.CONTIG_SEED))
def test_genome_census(seed):
    rng = np.random.default_rng(seed)
    g, ann = SI.genome(rng, 45_000)
    kinds = collections.Counter(a[2] for a in ann)
    assert all(kinds[k] >= 1 for k in SI.KINDS), kinds
    covered = np.zeros(len(g), dtype=bool)
    for s, e, kind, period in ann:
        assert 0 <= s < e <= len(g)
        if kind != "N":
            covered[s:e] = True
        seg = g[s:e][g[s:e] != SI.N]
        if kind in ("homopolymer", "long_homopolymer"):
            assert len(set(seg.tolist())) == 1
            assert 8 <= e - s <= 60 or kind == "long_homopolymer"
        elif kind in ("str", "str_partial"):
            assert 2 <= period <= 6 and 8 <= e - s <= 60 and ((e - s) % period != 0) == (kind == "str_partial")
            u = g[s:e]
            assert ((u[period:] == u[:-period]) | (u[period:] == SI.N) | (u[:-period] == SI.N)).all()
        elif kind == "tandem":
            assert 30 <= period <= 400 and 2 <= (e - s) // period <= 5 and (e - s) % period == 0
        elif kind.startswith("dispersed"):
            assert 300 <= e - s <= 1500
        elif kind == "N":
            assert g[s] == SI.N
    lh = sorted(e - s for s, e, kind, _ in ann if kind == "long_homopolymer")
    assert len(lh) >= 2 and lh[0] > 255 and lh[-1] > 400
    assert 0.20 <= covered.mean() <= 0.50, covered.mean()
    assert int((g == SI.N).sum()) == kinds["N"] >= 4
    # a dispersed copy is a copy: it is found elsewhere in the genome, on its strand
    text = g.tobytes()
    for s, e, kind, _ in ann:
        if kind.startswith("dispersed"):
            probe = g[s + 40:s + 100]
            if (probe == SI.N).any():
                continue
            probe = (S.revcomp(probe) if kind.endswith("-") else probe).tobytes()
            assert text.count(probe) >= (1 if kind.endswith("-") else 2)
    # strains: the annotation is carried over (a homopolymer of the genome is one in the strain, a unit more or less)
    st = SI.strains(rng, g, ann, 2)
    assert (st[0].seq == g).all() and len(st[1].seq) != len(g)
    lens0 = collections.Counter(e - s for s, e, kind, _ in st[0].ann if kind == "homopolymer")
    lens1 = collections.Counter(e - s for s, e, kind, _ in st[1].ann if kind == "homopolymer")
    assert lens0 != lens1 and sum(lens0.values()) == sum(lens1.values())
    pure = 0
    hp = [(s, e) for s, e, kind, _ in st[1].ann if kind == "homopolymer"]
    for s, e in hp:
        seg = st[1].seq[s:e]
        pure += int((seg != np.bincount(seg).argmax()).sum() <= 1)
    assert pure >= 0.9 * len(hp)


def test_reads_carry_strain_coordinates():
    reads, st = SI.long_set(SI.LONG_SEEDS[0])
    assert {r.rev for r in reads} == {True, False} and {r.strain for r in reads} == {0, 1}
    n_ins = 0
    for r in reads:
        g = st[r.strain].seq
        seq = S.revcomp(r.seq) if r.rev else r.seq
        gp = r.gpos[::-1] if r.rev else r.gpos
        ok = gp >= 0
        n_ins += int((~ok).sum())
        assert gp[0] == r.start and gp[-1] == r.end - 1 and (np.diff(gp[ok]) > 0).all()
        assert (seq[ok] == g[gp[ok]]).mean() > 0.98            # (substitution errors: 0.4 %)
    assert n_ins > 500


def test_micro_cases_cover_the_grid():
    reads = SI.micro_set()
    names = [r.name for r in reads]
    assert len(set(names)) == len(names) and 2 * 300 <= len(names) <= 2 * 3000
    cases = {n[:-2] for n in names}
    for period in SI.MICRO_PERIODS:
        for cop in SI.MICRO_COPIES:
            for delta in SI.MICRO_DELTAS:
                if period == 1 and delta in ("pu", "mu"):
                    continue
                for mask in range(16):
                    for strand in "fr":
                        assert f"p{period}c{cop:02d}_{delta}_{mask:04b}_{strand}" in cases
    ends = {f"end{tail}_k{k}_d{d}_{strand}" for tail in range(4) for k in (1, 2, 3) for d in range(1, 9) for strand in "fr"}
    assert ends <= cases
    by = {r.name: r for r in reads}
    a, b = by["end2_k3_d5_f_a"].seq, by["end2_k3_d5_f_b"].seq
    assert (np.nonzero(a != b)[0] == len(a) - 5 - np.array([7, 3, 0])).all() and (a[-24:-2] == a[-22:]).all()
    a, b = by["p3c12_mu_0000_f_a"].seq, by["p3c12_mu_0000_f_b"].seq
    assert len(a) == 2 * SI.MICRO_FLANK + 36 and len(b) == len(a) - 3
    assert (a[:SI.MICRO_FLANK] == b[:SI.MICRO_FLANK]).all() and (a[-SI.MICRO_FLANK:] == b[-SI.MICRO_FLANK:]).all()
    a, b = by["p2c05_0_1111_r_a"].seq, S.revcomp(by["p2c05_0_1111_r_b"].seq)
    assert len(a) == len(b) and int((a != b).sum()) == 4


@pytest.mark.parametrize("seed", SI.LONG_SEEDS)
def test_oracle_on_the_long_set(tmp_path, seed):
    reads, st = SI.long_set(seed)
    rows = _oracle_rows(tmp_path, reads)
    masks = [SI.repeat_mask(s) for s in st]
    count = collections.Counter()

    def on_gap(q, t, op, qi, ti, k):
        count["long_gaps"] += k > 20
        if op == "D":
            pos, strain = int(t.gpos[ti]), t.strain
        else:
            pos, strain = int(q.gpos[qi]), q.strain
            for j in range(qi + 1, min(qi + k + 2, len(q.gpos))):      # an inserted error base: its neighbour's place
                if pos >= 0:
                    break
                pos = int(q.gpos[j])
        count["gaps"] += 1
        count["gaps_in_short_period_repeats"] += pos >= 0 and bool(masks[strain][pos])

    check_true_alignments(rows, reads, on_gap)
    per_pair = collections.Counter((c[0], c[5]) for c in rows)
    several = sum(1 for v in per_pair.values() if v > 1)
    print(f"long set {seed}: rows {len(rows)}, pairs {len(per_pair)}, with several rows {several}, max {max(per_pair.values())}, "
          f"{dict(count)}")
    assert len(rows) >= 3000
    assert several >= 0.20 * len(per_pair)
    assert count["gaps_in_short_period_repeats"] >= 1000
    assert count["long_gaps"] >= 30


def test_oracle_on_the_short_set(tmp_path):
    reads, _ = SI.short_set()
    rows = _oracle_rows(tmp_path, reads, OA.opts_short())
    count = collections.Counter()
    check_true_alignments(rows, reads, lambda q, t, op, qi, ti, k: count.update(gaps=1))
    print(f"short set: rows {len(rows)}, {dict(count)}")
    assert len(rows) >= 20_000
    assert count["gaps"] >= 20_000


def test_oracle_on_the_contigs_without_gaps(tmp_path):
    reads, _ = SI.contig_set()
    assert 40 <= len(reads) <= 60 and all(2000 <= len(r.seq) <= 8000 for r in reads)
    o = OA.opts_short()
    o.pair_once, o.bandwidth = 1, 0
    rows = _oracle_rows(tmp_path, reads, o)
    check_true_alignments(rows, reads, lambda *a: pytest.fail("a gap at bandwidth 0"))
    print(f"contigs: rows {len(rows)}")
    assert len(rows) >= 100


@pytest.mark.parametrize("mode", ["long", "short"])
def test_oracle_on_the_micro_cases(tmp_path, mode):
    reads = SI.micro_set()
    rows = _oracle_rows(tmp_path, reads, OA.opts_short() if mode == "short" else None)
    check_true_alignments(rows, reads)
    cases = {r.name[:-2] for r in reads}
    hit = {c[0][:-2] for c in rows if c[0][:-2] == c[5][:-2]}
    gapped = sum(1 for c in rows if "I" in c[-1] or "D" in c[-1])
    print(f"micro cases ({mode}): pairs {len(cases)}, with a row {len(hit)}, rows {len(rows)}, gapped rows {gapped}")
    assert len(hit) >= 0.80 * len(cases)
    assert gapped >= 0.25 * len(rows)
