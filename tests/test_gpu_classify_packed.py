"""The classifier on 2-bit packed bases (classify_kernel<1>, <2>: 32 bases per load) against the CPU oracle and against
the same call on the byte array (HLMI_CLASSIFY_BYTES).  Every case is compared three ways: the packed rows with the
oracle's, byte for byte with CIGARs; the byte-path rows with the oracle's; and the classifier statistics of the two GPU
runs with each other - the packed path has to certify exactly the tasks the byte path certifies, not merely end at the
same rows.

The inputs are the smallest ones where a 32-base piece can go wrong: a substitution (an indel) that visits every offset
of a piece, read sets whose lengths leave the arrays at every position of a packed byte, overlaps that reach the first
and the last base of a file on both strands, and ambiguous bases, which the 2-bit array cannot hold (their granules
are flagged and their tasks take the byte loops)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import structured_inputs as SI  # noqa: E402
from hylight_amd import api  # noqa: E402
from hylight_amd import simulate as S  # noqa: E402
from oracle import ava as OA  # noqa: E402

pytestmark = pytest.mark.gpu

BYTES = "HLMI_CLASSIFY_BYTES"
CLASS_STATS = ("align_tasks_fast", "align_tasks_dp", "align_tasks_narrow", "align_tasks_wide", "align_tasks_long",
               "align_tasks_wide_one_piece")
PACKED = "align_tasks_packed"
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
N = ord("N")


def _first_difference(got, want):
    if got == want:
        return None
    g, w = got.split("\n"), want.split("\n")
    for k in range(max(len(g), len(w))):
        a, b = (g[k] if k < len(g) else "<end of file>"), (w[k] if k < len(w) else "<end of file>")
        if a != b:
            return f"row {k} of {len(w) - 1}:\n  got  {a[:400]}\n  want {b[:400]}"


def _read(name, seq):
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    return S.Read(name, seq, None, 0, 0, len(seq), False)


def _uniform(rng, n):
    return BASES[rng.integers(0, 4, size=n)]


def _sub(seq, *positions):
    """seq with another base at every position"""
    out = seq.copy()
    for p in positions:
        out[p] = BASES[(int(np.where(BASES == seq[p])[0][0]) + 1 + p % 3) % 4]
    return out


def _rc(seq):
    """reverse complement; N stays N"""
    return np.where(seq[::-1] == N, N, S.revcomp(np.where(seq == N, BASES[0], seq))).astype(np.uint8)


class Runner:
    """one directory, numbered files; gpu(): rows + statistics of one hlmi_ava call with the given hooks set"""

    def __init__(self, d, monkeypatch):
        self.d, self.mp, self.n = d, monkeypatch, 0

    def fasta(self, reads):
        self.n += 1
        p = self.d / f"in{self.n}.fa"
        S.write_fasta(reads, p)
        return p

    def oracle(self, tfa, qfa, mode="long"):
        self.n += 1
        p = self.d / f"oracle{self.n}.paf"
        OA.ava(tfa, qfa, p, OA.opts_short() if mode == "short" else OA.opts_long())
        return open(p).read()

    def gpu(self, tfa, qfa, hooks=(), mode="long"):
        self.n += 1
        p = self.d / f"gpu{self.n}.paf"
        with self.mp.context() as m:
            m.delenv(BYTES, raising=False)
            for h in hooks:
                m.setenv(h, "1")
            api.ava(tfa, qfa, p, api.ava_opts_short() if mode == "short" else api.ava_opts_long())
        return open(p).read(), dict(api.last_stats())

    def three_ways(self, tfa, qfa, min_rows, hooks=(), mode="long", want=None):
        """-> statistics of the packed run, after the three comparisons"""
        want = want if want is not None else self.oracle(tfa, qfa, mode)
        assert want.count("\n") >= min_rows, want.count("\n")
        packed, st_p = self.gpu(tfa, qfa, hooks, mode)
        plain, st_b = self.gpu(tfa, qfa, tuple(hooks) + (BYTES,), mode)
        diff = _first_difference(packed, want)
        assert diff is None, "packed: " + diff
        diff = _first_difference(plain, want)
        assert diff is None, "bytes: " + diff
        cls_p, cls_b = {k: st_p[k] for k in CLASS_STATS}, {k: st_b[k] for k in CLASS_STATS}
        print("packed", cls_p, "bytes", cls_b, "compared from the 2-bit arrays", st_p[PACKED], st_b[PACKED])
        assert cls_p == cls_b
        assert cls_p["align_tasks_fast"] > 0
        # the two runs really took the two forms: align_tasks_packed counts the tasks the classifier compared from the 2-bit arrays
        assert st_p[PACKED] > 0 and st_b[PACKED] == 0
        return st_p


@pytest.fixture()
def run(tmp_path, monkeypatch):
    return Runner(tmp_path, monkeypatch)


def _both_strands(queries):
    return queries + [_read(r.name + "_rc", _rc(r.seq)) for r in queries]


def test_substitution_sweep(run):
    """One substitution at 64 consecutive offsets, two substitutions 1..40 bases apart: the substitution is every base of
    a 32-base piece of whatever block holds it, the base behind a block included (fourth certificate)."""
    rng = np.random.default_rng(5101)
    t = _uniform(rng, 3000)
    q = [_read(f"one{j}", _sub(t, 200 + j)) for j in range(64)]
    q += [_read(f"two{d}", _sub(t, 1500 + d, 1500 + 2 * d)) for d in range(1, 41)]
    q = _both_strands(q)
    run.three_ways(run.fasta([_read("zt", t)]), run.fasta(q), len(q))


def test_indel_sweep(run):
    """One- and two-base insertions and deletions at 64 consecutive offsets: the scans of the second pass from both ends
    of a block with m != n (second, fifth, seventh certificate), with a substitution 1..64 bases away for the fifth and
    seventh."""
    rng = np.random.default_rng(5102)
    t = _uniform(rng, 3000)
    q = []
    for j in range(64):
        p = 700 + j
        for gap in (1, 2):
            q.append(_read(f"del{gap}_{j}", np.concatenate([t[:p], t[p + gap:]])))
            q.append(_read(f"ins{gap}_{j}", np.concatenate([t[:p], _uniform(rng, gap), t[p:]])))
        near = _sub(t, 700 - j - 1)
        q.append(_read(f"del1sub_{j}", np.concatenate([near[:700], near[701:]])))
        both = _sub(t, 700 - j - 1, 702 + j // 2)
        q.append(_read(f"del1sub2_{j}", np.concatenate([both[:700], both[701:]])))
    q = _both_strands(q)
    st = run.three_ways(run.fasta([_read("zt", t)]), run.fasta(q), len(q))
    assert st["align_tasks_dp"] > 0


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("rest", [1, 2, 3])
def test_array_edges(run, rest, flip):
    """Target and query arrays of a length that is `rest` modulo 4, reads of fewer than 32 bases in between (no rows, but
    every later offset moves), overlaps that reach the first base of the first read and the last base of the last read of
    both files - forward at both ends, or (flip) the query on the reverse strand there."""
    rng = np.random.default_rng(5103 + rest)
    g = _uniform(rng, 5500)
    tiny_t, tiny_q = 17 + (rest - (3000 + 17 + 3000)) % 4, 11 + (rest - (2000 + 11 + 3000 + 29 + 2000)) % 4
    targets = [_read("t_first", g[:3000]), _read("t_tiny", _uniform(rng, tiny_t)), _read("t_last", g[2500:])]
    first, last = _read("q_first", g[:2000]), _read("q_last", g[3500:])
    if flip:
        first, last = _read("q_first", _rc(g[3500:])), _read("q_last", _rc(g[:2000]))
    queries = [first, _read("q_tiny", _uniform(rng, tiny_q)), _read("q_mid", _rc(g[1000:4000]) if not flip else g[1000:4000]),
               _read("q_tiny2", _uniform(rng, 29)), last]
    assert sum(len(r.seq) for r in targets) % 4 == rest and sum(len(r.seq) for r in queries) % 4 == rest
    tfa, qfa = run.fasta(targets), run.fasta(queries)
    want = run.oracle(tfa, qfa)
    rows = [l.split("\t") for l in want.split("\n")[:-1]]
    # (columns: query, length, start, end, strand, target, length, start, end)
    assert any(r[0] == "q_first" and r[5] == ("t_last" if flip else "t_first") and r[2] == "0" and (r[8] == r[6] if flip else r[7] == "0") for r in rows), rows
    assert any(r[0] == "q_last" and r[5] == ("t_first" if flip else "t_last") and r[3] == r[1] and (r[7] == "0" if flip else r[8] == r[6]) for r in rows), rows
    run.three_ways(tfa, qfa, 4, want=want)


def _ambiguous_sets(rng):
    """-> (targets, queries, the same without the ambiguous bases)"""
    t = _uniform(rng, 3000)
    t_n = t.copy()
    t_n[0] = t_n[-1] = N
    t_n[1200:1207] = N
    # the query file: the position of every base in its array is known, so a run can be laid across a granule boundary
    q_clean, q_amb = [], []

    def add(name, seq, positions):
        q_clean.append(_read(name, seq))
        amb = seq.copy()
        amb[list(positions)] = N
        q_amb.append(_read(name, amb))

    sub = _sub(t, 2000)                                  # (the queries differ from the target in one base: names apart)
    add("n_first", sub, [0])
    add("n_last", sub, [len(sub) - 1])
    for j in range(40):                                  # inside an identical block, behind one, at every offset of a granule
        add(f"n_in{j}", sub, [900 + j])
    used = sum(len(r.seq) for r in q_clean)
    start = 1500 + (28 - (used + 1500)) % 32             # bases 28 .. 35 of a granule pair
    add("n_run", sub, range(start, start + 8))
    n = len(q_clean)
    for k in range(n):
        q_clean.append(_read(q_clean[k].name + "_rc", _rc(q_clean[k].seq)))
        q_amb.append(_read(q_amb[k].name + "_rc", _rc(q_amb[k].seq)))
    return [_read("t", t), _read("t_n", t_n)], q_amb, [_read("t", t), _read("t_n2", t)], q_clean


def test_ambiguous_bases(run):
    """N at a read's first and last base, inside and behind an otherwise identical block, as a run across a granule
    boundary, in the target and in the queries, on both strands.  The tasks that touch one take the byte loops: fewer
    tasks are compared from the 2-bit arrays, and fewer finish in the classifier, than on the same reads without N."""
    t_amb, q_amb, t_clean, q_clean = _ambiguous_sets(np.random.default_rng(5104))
    st_amb = run.three_ways(run.fasta(t_amb), run.fasta(q_amb), len(q_amb))
    _, st_clean = run.gpu(run.fasta(t_clean), run.fasta(q_clean))
    print("fast with N", st_amb["align_tasks_fast"], "without", st_clean["align_tasks_fast"])
    assert st_amb["align_tasks_fast"] < st_clean["align_tasks_fast"]
    print("packed with N", st_amb[PACKED], "without", st_clean[PACKED])
    assert 0 < st_amb[PACKED] < st_clean[PACKED]


@pytest.fixture(scope="module")
def structured(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed_structured")
    fa = {}
    for name, rd in (("long0", SI.long_set(SI.LONG_SEEDS[0])[0]), ("micro", SI.micro_set())):
        fa[name] = d / f"{name}.fa"
        S.write_fasta(rd, fa[name])
    want = {}
    for name in fa:
        OA.ava(fa[name], fa[name], d / f"{name}.paf")
        want[name] = open(d / f"{name}.paf").read()
    return fa, want


@pytest.mark.parametrize("name", ["micro", "long0"])
def test_structured_sets(run, structured, name):
    """The low-complexity sets of tests/structured_inputs.py (ties, repeats, ambiguous bases inside repeats)."""
    fa, want = structured
    run.three_ways(fa[name], fa[name], 1000, want=want[name])


# the existing certificate switches on the packed path -> the statistic each must lower (None: rows only)
HOOKS = {"HLMI_NO_SHIFT_CERT": "align_tasks_fast", "HLMI_NO_GAP1_CERT": "align_tasks_fast", "HLMI_NO_GAP2_CERT": "align_tasks_fast",
         "HLMI_NO_EXT_CERT": "align_ext_certified", "HLMI_NO_SUFFIX_TRIM": None}


@pytest.fixture(scope="module")
def micro_default(structured, tmp_path_factory):
    fa, _ = structured
    p = tmp_path_factory.mktemp("packed_micro") / "default.paf"
    saved = os.environ.pop(BYTES, None)
    try:
        api.ava(fa["micro"], fa["micro"], p, api.ava_opts_long())
    finally:
        if saved is not None:
            os.environ[BYTES] = saved
    return dict(api.last_stats())


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_certificate_hooks_still_switch(run, structured, micro_default, hook):
    fa, want = structured
    st = run.three_ways(fa["micro"], fa["micro"], 1000, hooks=(hook,), want=want["micro"])
    key = HOOKS[hook]
    if key:
        print(hook, key, micro_default[key], "->", st[key])
        assert st[key] < micro_default[key]
