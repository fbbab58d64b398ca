"""Deterministic inputs for the optimality checks of the alignment side (tests/test_align_optimal.py,
tests/test_gpu_align_optimal.py): uniform random sequence with PLANTED differences, so that what an optimal alignment has to
do is known by construction - unlike tests/structured_inputs.py, whose repeats are there to make alignments tie.

Every set is a dict name -> bases (str), at most 40 reads of at most 3 kb; reads come in pairs (A, B), unrelated between
pairs, so the overlapper reports about one row per pair and direction.

  planted_set     B = A with isolated edits >= 150 bases apart: substitution runs of 1-3 bases, insertions and deletions of
                  INDELS bases (the narrow / wide switch at |shift| 5 / 6, the second gap piece from 21 bases on, the largest
                  shift of one block, 39); a few pairs with B reverse-complemented
  long_block_set  the same, and stretches of STRETCHES bases with a substitution every 9 bases (no k-mer survives: one block
                  spans the stretch) with an indel of SHIFTS bases in their middle: blocks around the 256-row switch to LONG
                  blocks, and LONG blocks on either side of |shift| 7 / 8 (32 / 64 diagonals)
  paired_set      an insertion and a deletion of 3 - 5 bases 14 bases apart, in one block: the path uses the band's padding
  chimera_set     A = X + U, B = X + V (or U + X, V + X) with U, V unrelated: the homology ends inside both reads, the end
                  extension has to stop; edits within 40 bases of the boundary.  Returns the boundaries too
  short_set       250-base reads, edits of at most 10 bases, for the short-mode constants
  raw_planted_set planted_set with its edits wherever they fall, next to homopolymer runs too (_clean_site): claim 0 only
  split_set       planted indels of 40 and 41 bases: the shift bound of one block (39) splits the row
  noisy_set       the simulator's reads at the error rates of tests/test_gpu_ava.py::test_ava_noisy_reads, seed 71, the first
                  30 reads cut to 3 kb
"""
import numpy as np

from hylight_amd import simulate as S

INDELS = (1, 2, 3, 5, 6, 7, 8, 12, 19, 20, 21, 22, 30, 39)
STRETCHES = (200, 228, 250, 256, 257, 300, 520)      # 200, 228: blocks that stay within 256 rows with the same content
SHIFTS = (0, 5, 7, 8, 20, 39)
MAX_READ = 3000
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _random(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, size=n))


def _other(rng, *avoid):
    """a base that is none of `avoid`"""
    left = [c for c in "ACGT" if c not in avoid]
    return left[int(rng.integers(0, len(left)))]


def _clean_site(a, pos, kind, n, step=1):
    """The first position from pos on (step -1: backwards) where an edit of this kind leaves every homopolymer run of both reads as long as it was: the
    bases on either side of the cut differ from each other and from what the edit puts or leaves next to them.  The long mode
    seeds on homopolymer-compressed k-mers; next to an edit that lengthens or shortens a run, two k-mers can be equal in
    compressed form and end on different offsets, and a fixed point there forces a gap on every alignment (DESIGN.md section 5,
    deviations; raw_planted_set keeps such sites on purpose)."""
    while True:
        end = pos if kind == "ins" else pos + n
        ok = a[pos - 1] != a[pos] and a[end - 1] != a[end]
        if kind == "del":
            ok = ok and a[pos - 1] != a[end] and a[pos] != a[end] and a[end - 1] != a[pos - 1]
        if ok:
            return pos
        pos += step


def _apply(rng, a, edits, clean=True):
    """edits: [(pos, kind, n)] ascending and apart, kind sub / ins / del, positions on a (moved to the next clean site) -> b"""
    out, at = [], 0
    for pos, kind, n in edits:
        if clean:
            pos = _clean_site(a, pos, kind, n)
        if pos < at and kind == "sub":          # moved into the edit before it (long_block_set: a substitution next to the indel)
            continue
        assert pos >= at
        out.append(a[at:pos])
        if kind == "sub":
            new = [_other(rng, a[p]) for p in range(pos, pos + n)]
            new[0] = _other(rng, a[pos], a[pos - 1], *(a[pos + 1],) * (n == 1))
            if n > 1:
                new[-1] = _other(rng, a[pos + n - 1], a[pos + n])
            out.append("".join(new))
            at = pos + n
        elif kind == "del":
            at = pos + n
        else:
            ins = _random(rng, n)
            while clean and (ins[0] in a[pos - 1:pos + 1] or ins[-1] in a[pos - 1:pos + 1]):
                ins = _random(rng, n)
            out.append(ins)
            at = pos
    out.append(a[at:])
    return "".join(out)


def _edit_kinds(indels=INDELS):
    return [("sub", n) for n in (1, 2, 3)] + [(k, n) for n in indels for k in ("ins", "del")]


def _sites(rng, lo, hi):
    """edit positions lo <= p < hi, 150 - 190 apart"""
    out, p = [], lo
    while p < hi:
        out.append(p)
        p += int(rng.integers(150, 191))
    return out


def planted_set(seed=4101, n_pairs=20, rc_every=6, clean=True):
    rng = np.random.default_rng(seed)
    kinds = _edit_kinds()
    seqs, turn = {}, 0
    for p in range(n_pairs):
        a = _random(rng, int(rng.integers(2400, 2900)))
        edits = []
        for pos in _sites(rng, 100, len(a) - 140):
            kind, n = kinds[turn % len(kinds)]
            turn += 1
            edits.append((pos, kind, n))
        b = _apply(rng, a, edits, clean)
        assert len(b) <= MAX_READ
        seqs[f"p{p:02d}a"] = a
        seqs[f"p{p:02d}b"] = revcomp(b) if p % rc_every == rc_every - 1 else b
    return seqs


def raw_planted_set():
    """planted_set without the choice of clean sites: some fixed points bind here (claim 0 only; the measured loss: DESIGN.md
    section 5)"""
    return planted_set(seed=4106, clean=False)


def paired_set(seed=4107, n_pairs=6):
    """Two opposite indels of 3 - 5 bases 14 bases apart: no k-mer fits between them, so one block of shift 0 holds both
    and its best path leaves the corner diagonals by the indel's length - the padding of the 16-diagonal band (5)."""
    rng = np.random.default_rng(seed)
    seqs = {}
    for p in range(n_pairs):
        a = _random(rng, 2000)
        edits = []
        for x, pos in enumerate(range(150, 1850, 200)):
            n, first = 3 + (x + p) % 3, ("del", "ins")[(x + p // 3) % 2]
            pos = _clean_site(a, pos, first, n)
            edits += [(pos, first, n), (pos + (n if first == "del" else 0) + 14, "ins" if first == "del" else "del", n)]
        seqs[f"d{p:02d}a"] = a
        seqs[f"d{p:02d}b"] = _apply(rng, a, edits)
    return seqs


def long_block_set(seed=4102):
    rng = np.random.default_rng(seed)
    stretches = [(r, d, k) for k in ("ins", "del") for r in STRETCHES for d in SHIFTS]
    kinds = _edit_kinds(tuple(n for n in INDELS if n < 20))
    seqs, turn, p = {}, 0, 0
    while stretches:
        full = _random(rng, 2800)
        edits, at = [], 120
        while stretches and at + stretches[0][0] + 200 <= 2700:
            r, d, k = stretches.pop(0)
            subs = list(range(at + 4, at + r, 9))
            mid = _clean_site(full, subs[len(subs) // 2] + 4, k, d) if d else 0
            cut = (mid, mid + d) if k == "del" else (mid, mid)
            edits += [(s, "sub", 1) for s in subs if not cut[0] - 9 <= s <= cut[1] + 1]
            if d:
                edits.append((mid, k, d))
            at += r + 170
            kind, n = kinds[turn % len(kinds)]          # an ordinary edit between two stretches
            turn += 1
            edits.append((at - 85, kind, n))
        a = full[:at + 60]
        b = _apply(rng, a, sorted(edits))
        assert len(a) <= MAX_READ and len(b) <= MAX_READ
        seqs[f"L{p:02d}a"] = a
        seqs[f"L{p:02d}b"] = revcomp(b) if p % 5 == 4 else b
        p += 1
    assert len(seqs) <= 40
    return seqs


def chimera_set(seed=4103, n_pairs=18):
    """-> (seqs, bounds): bounds[name] = (p, shared_is_left): the shared part of the read is [0, p) or [p, len)"""
    rng = np.random.default_rng(seed)
    near = [None, ("sub", 1, 6), ("sub", 2, 20), ("ins", 1, 12), ("del", 2, 5), ("del", 5, 6), ("ins", 3, 30), ("del", 3, 38),
            ("ins", 5, 25), ("sub", 1, 2)]
    seqs, bounds = {}, {}
    for p in range(n_pairs):
        x = _random(rng, int(rng.integers(1000, 1400)))
        u, v = _random(rng, int(rng.integers(600, 900))), _random(rng, int(rng.integers(600, 900)))
        while len({u[0], v[0], x[-1]}) < 3 or len({u[-1], v[-1], x[0]}) < 3:      # the homology ends exactly at the boundary
            u, v = _random(rng, len(u)), _random(rng, len(v))
        left = p % 2 == 0                               # X + U / X + V, else U + X / V + X
        edits = [(400, "del", 2), (700, "sub", 1)]
        e = near[p % len(near)]
        if e is not None:
            kind, n, dist = e
            edits.append((_clean_site(x, len(x) - dist - n, kind, n, -1), kind, n) if left else (dist, kind, n))
        y = _apply(rng, x, sorted(edits))
        a, b = (x + u, y + v) if left else (u + x, v + y)
        pa, pb = (len(x), len(y)) if left else (len(u), len(v))
        la, lb = left, left
        if p % 5 == 3:
            b, pb, lb = revcomp(b), len(b) - pb, not lb
        seqs[f"c{p:02d}a"], seqs[f"c{p:02d}b"] = a, b
        bounds[f"c{p:02d}a"], bounds[f"c{p:02d}b"] = (pa, la), (pb, lb)
        assert len(a) <= MAX_READ and len(b) <= MAX_READ
    return seqs, bounds


def short_set(seed=4104, n_pairs=20):
    rng = np.random.default_rng(seed)
    kinds = [("sub", 1), ("sub", 2), ("sub", 3)] + [(k, n) for n in (1, 2, 3, 5, 8, 10) for k in ("ins", "del")]
    seqs = {}
    for p in range(n_pairs):
        a = _random(rng, 250)
        edits = [(int(rng.integers(60, 90)),) + kinds[(2 * p) % len(kinds)], (int(rng.integers(160, 185)),) + kinds[(2 * p + 1) % len(kinds)]]
        b = _apply(rng, a, edits)
        seqs[f"s{p:02d}a"] = a
        seqs[f"s{p:02d}b"] = revcomp(b) if p % 4 == 3 else b
    return seqs


def split_set(seed=4105, n_pairs=6):
    rng = np.random.default_rng(seed)
    seqs = {}
    for p in range(n_pairs):
        a = _random(rng, 2400)
        edits = [(600, "ins" if p % 2 else "del", 40 + p % 2), (1200, "del" if p % 2 else "ins", 41 - p % 2), (1800, "sub", 2)]
        seqs[f"x{p:02d}a"] = a
        seqs[f"x{p:02d}b"] = _apply(rng, a, edits)
    return seqs


def noisy_set():
    reads, _ = S.simulate_reads(seed=71, n_reads=36, n_strains=2, genome_len=12000, mean_len=4000, min_len=1500, max_len=8000,
                                err_sub=0.06, err_ins=0.03, err_del=0.03)
    return {r.name: r.seq.tobytes().decode()[:MAX_READ] for r in reads[:30]}


def write_fasta(seqs, path):
    with open(path, "w") as f:
        for name, s in seqs.items():
            f.write(f">{name}\n{s}\n")
    return path


# name -> (builder, constants, claims asserted (tests/align_score.py), tail rule of claim C, least number of judged rows)
SETS = {
    "planted": (planted_set, "long", "0ABC", True, 20),
    "long_block": (long_block_set, "long", "0AC", True, 15),
    "chimera": (chimera_set, "long", "0BC", True, 18),
    "short": (short_set, "short", "0AC", True, 40),
    "paired": (paired_set, "long", "0A", True, 6),
    "split": (split_set, "long", "0BC", True, 12),
    "noisy": (noisy_set, "long", "0", False, 20),       # claim C on it: the tests' own test_noisy_rows_begin_and_end_on_a_match
    "raw_planted": (raw_planted_set, "long", "0", False, 20),
}
