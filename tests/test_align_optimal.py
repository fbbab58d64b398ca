"""CPU: the rows of the overlapper's oracle held to a plain two-piece affine DP (tests/capi/align_ref_check.cpp).

Every GPU test of the alignment side compares the kernels byte for byte with `band_dp` of oracle/ava_oracle.c; this module
holds band_dp's rows to the scoring rules of DESIGN.md section 5 themselves: a row is an OPTIMAL alignment of its two
substrings (claim A), its end extensions stopped where nothing more was to gain (claim B) and on a match, without a tail
that gains nothing (claim C) - tests/align_score.py states the claims, tests/align_inputs.py the inputs.  The reference is
held to hand-worked literals and to the enumeration of all alignments of short strings first, and the checker to rows
spoiled by hand.  tests/test_gpu_align_optimal.py asserts the same claims on the GPU's own rows."""
import os
import random
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import align_inputs as AI  # noqa: E402
import align_score as AS  # noqa: E402
from oracle import ava as OA  # noqa: E402

LONG = (2, 4, 1, 4, 2, 24, 1)            # match, mismatch, ambi, o1, e1, o2, e2 of the long mode
SHORT = (4, 2, 1, 12, 2, 32, 1)
ONES = (1, 1, 1, 1, 1, 0, 0)
CROSS = (2, 3, 1, 1, 3, 4, 1)            # the second piece is the cheaper one from 2 bases on: it decides 6 x 6 cases


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_ref")
    return AS.compile_reference(d), d


def test_reference_literals(ref):
    exe, d = ref
    a = "ACGTTGCAAGGCTATCGGATCCATGCAAGT"                     # 30 bases
    g20, g21 = "TCTCAGAGTCTCAGAGTCTC", "TCTCAGAGTCTCAGAGTCTCA"
    wide = (-40, 40)
    tasks = [
        AS.global_task(a, a[:15] + g20 + a[15:], LONG, *wide),       # 60 - (4 + 2 * 20) = 60 - 44
        AS.global_task(a, a[:15] + g21 + a[15:], LONG, *wide),       # 60 - (24 + 21) = 60 - 45
        AS.global_task(a[:15] + g21 + a[15:], a, LONG, *wide),       # the same gap on the other side
        AS.global_task("-", g20, LONG, *wide), AS.global_task(g21, "-", LONG, *wide),
        AS.global_task(a, a[:15] + g21 + a[15:], LONG[:5] + (0, 0), *wide),     # one piece: 4 + 2 * 21 = 46
        # I next to D is two gaps: ACGT+AAAA+ACGT against ACGT+CC+ACGT under all-ones: mismatches 8 - 2 - (1 + 2) = 3 beats
        # 8 - (1 + 4) - (1 + 2) = 0; with mismatch 9 the two gaps win, and one gap of 6 bases (8 - 7 = 1) is not what they cost
        AS.global_task("ACGTAAAAACGT", "ACGTCCACGT", ONES, *wide),
        AS.global_task("ACGTAAAAACGT", "ACGTCCACGT", (1, 9, 1, 1, 1, 0, 0), *wide),
        AS.global_task("NN", "NN", LONG, 0, 0), AS.global_task("ACNGT", "ACNGT", LONG, 0, 0), AS.global_task("ACNGT", "ACAGT", LONG, 0, 0),
        AS.global_task("acgu", "ACGT", LONG, 0, 0),
        # the corridor: the end cell lies on diagonal 2; no alignment with dhi < n - m
        AS.global_task("ACGT", "ACGTGG", LONG, -1, 2), AS.global_task("ACGT", "ACGTGG", LONG, -1, 1),
        # extensions: nothing but mismatches -> 0; 5 matches then junk -> 10; a mismatch repaid by 3 matches -> +2 more;
        # 4 matches, mismatch, 2 matches: the tail gains nothing (-4 + 4): 8; rows / cols / band cut the rectangle
        AS.extend_task("AAAAAAAA", "CCCCCCCC", LONG), AS.extend_task("ACGTAGGGGG", "ACGTACCCCC", LONG),
        AS.extend_task("ACGTAGTCA", "ACGTATTCA", LONG), AS.extend_task("ACGTGAC", "ACGTCAC", LONG),
        AS.extend_task("ACGTACGTAC", "ACGTACGTAC", LONG, rows=4), AS.extend_task("ACGTACGTAC", "ACGTACGTAC", LONG, cols=3),
        AS.extend_task("ACGTACGTAC", "GGGGGGGGGGACGTACGTAC", LONG, band=8), AS.extend_task("-", "ACGT", LONG),
        AS.extend_task("ACGTACGTACGTACGTACGT", "ACGTACGTAC" + "GG" + "GTACGTACGT", LONG, band=2),   # 20 - 8 + 20: the gap fits the band
        AS.extend_task("ACGTACGTACGTACGTACGT", "ACGTACGTAC" + "GG" + "GTACGTACGT", LONG, band=1),   # 11 matches: it does not
    ]
    want = [60 - 44, 60 - 45, 60 - 45, -44, -45, 60 - 46,
            3, 0, -2, 7, 7, 8, 8 - 8, None,
            0, 10, 12, 8, 8, 6, 0, 0, 32, 22]
    assert AS.run_reference(exe, tasks, d, name="literals") == want
    # the scorer agrees on the same cases
    assert AS.gap_cost(LONG, 20) == 44 and AS.gap_cost(LONG, 21) == 45 and AS.gap_cost(LONG[:5] + (0, 0), 21) == 46
    assert AS.score_alignment("4=4I2D4=", "ACGTAAAAACGT", "ACGTCCACGT", ONES).score == 0
    assert AS.score_alignment("2=", "NN", "NN", LONG).score == -2
    sc = AS.score_alignment("15=21D10=2I5=", a[:25] + "GG" + a[25:], a[:15] + g21 + a[15:], LONG)
    assert (sc.score, sc.dlo, sc.dhi, sc.first_ok, sc.last_ok) == (60 - 45 - 8, 0, 21, True, True)
    with pytest.raises(AssertionError):
        AS.score_alignment("4=", "ACGT", "ACGA", LONG)


def _enumerate(a, b, c, band):
    """All alignments of prefixes of a and b, column by column -> (best global score, best score of any prefix pair inside
    |j - i| <= band, the empty one included).  A path is a string of =/X, I and D columns; a run of equal gap columns is one
    gap."""
    best = {"global": None, "extend": 0}

    def walk(i, j, done, op, run):
        total = done - (AS.gap_cost(c, run) if run else 0)
        if i == len(a) and j == len(b) and (best["global"] is None or total > best["global"]):
            best["global"] = total
        if abs(j - i) <= band and total > best["extend"]:
            best["extend"] = total
        if i < len(a) and j < len(b):
            walk(i + 1, j + 1, total + AS.column_score(c, a[i], b[j]), "M", 0)
        if i < len(a):
            walk(i + 1, j, done if op == "I" else total, "I", run + 1 if op == "I" else 1)
        if j < len(b):
            walk(i, j + 1, done if op == "D" else total, "D", run + 1 if op == "D" else 1)

    walk(0, 0, 0, "M", 0)
    return best["global"], best["extend"]


def test_reference_against_enumeration(ref):
    """Every alignment of random strings up to 6 x 6 (8 989 global paths at 6 x 6), four constant sets; the corridor and the
    band hold every cell here (the literals have the cases where they bind)."""
    exe, d = ref
    rnd = random.Random(20251)
    tasks, want = [], []
    for c in (LONG, SHORT, ONES, CROSS):
        for n in range(36):
            la, lb = (6, 6) if n < 6 else (rnd.randint(0, 6), rnd.randint(0, 6))
            alphabet = "ACGTN" if n % 4 == 0 else "AC" if n % 4 == 1 else "ACGT"
            a, b = ("".join(rnd.choice(alphabet) for _ in range(l)) for l in (la, lb))
            g, e = _enumerate(a, b, c, 6)
            tasks += [AS.global_task(a, b, c, -6, 6), AS.extend_task(a, b, c, band=6)]
            want += [g, e]
    got = AS.run_reference(exe, tasks, d, name="enumeration")
    bad = [(t, g, w) for t, g, w in zip(tasks, got, want) if g != w]
    assert not bad, bad[:5]
    assert len({w for w in want}) > 20


def _spoiled_cases():
    rnd = random.Random(77)
    x = "".join(rnd.choice("ACGT") for _ in range(300))
    ins = "GTC" if x[149] != "C" else "GTA"
    u = "".join(rnd.choice("AC") for _ in range(250))
    v = "".join(rnd.choice("GT") for _ in range(250))
    q, t = x + u, x[:150] + ins + x[150:] + v                  # homology: x, with 3 bases more in t; nothing in common behind it
    seqs = {"q": q, "t": t}

    def row(qs, qe, ts, te, cg):
        return AS.paf_line("q", len(q), qs, qe, "t", len(t), ts, te, cg)
    return seqs, {
        "true": row(0, 300, 0, 303, "150=3D150="),
        "gap_slid_into_a_mismatch": row(0, 300, 0, 303, "149=3D1X150="),
        "cut_short_by_10_matches": row(0, 290, 0, 293, "150=3D140="),
        "lengthened_by_one_mismatch": row(0, 301, 0, 304, "150=3D150=1X"),
    }


def test_checker_flags_spoiled_rows(ref):
    """Each hand-spoiled row is flagged by the claim written for its fault, and the true row by none."""
    exe, d = ref
    seqs, rows = _spoiled_cases()
    o = OA.opts_long()
    flagged = {}
    for name, line in rows.items():
        _, bad = AS.check_set(exe, line + "\n", seqs, o, d, "0ABC", name="spoiled")
        flagged[name] = sorted(bad)
    assert flagged == {"true": [], "gap_slid_into_a_mismatch": ["A"], "cut_short_by_10_matches": ["B"],
                       "lengthened_by_one_mismatch": ["C"]}, flagged
    # a row that claims more than the reference finds: an `=` that is none is refused by the scorer itself
    with pytest.raises(AssertionError):
        AS.check_set(exe, rows["true"].replace("150=3D150=", "149=3D151="), seqs, o, d, "0")


class OracleRows:
    """the sets, their FASTA files and the oracle's rows on them, each computed once"""

    def __init__(self, d):
        self.d, self._got = d, {}

    def get(self, name):
        if name not in self._got:
            build, mode, claims, ties, least = AI.SETS[name]
            seqs = build()
            bounds = None
            if isinstance(seqs, tuple):
                seqs, bounds = seqs
            fa = AI.write_fasta(seqs, self.d / f"{name}.fa")
            o = OA.opts_short() if mode == "short" else OA.opts_long()
            OA.ava(fa, fa, self.d / f"{name}.paf", o)
            self._got[name] = (seqs, bounds, o, open(self.d / f"{name}.paf").read())
        return self._got[name]


@pytest.fixture(scope="module")
def oracle_rows(tmp_path_factory):
    return OracleRows(tmp_path_factory.mktemp("align_sets"))


@pytest.mark.parametrize("name", sorted(AI.SETS))
def test_oracle_rows_are_optimal(ref, oracle_rows, name):
    exe, d = ref
    _, _, claims, ties, least = AI.SETS[name]
    seqs, bounds, o, text = oracle_rows.get(name)
    reps, bad = AS.check_set(exe, text, seqs, o, d, claims, ties=ties, bounds=bounds, name=name)
    rows, lossy, mean, worst = AS.loss_figures(reps)
    print(f"{name}: {rows} rows judged, claims {claims}; S < S* on {lossy} rows, mean loss {mean:.3f}, largest {worst}")
    assert rows >= least, (name, rows)
    assert not bad, AS.failure_text(exe, bad, o, d)


def test_noisy_rows_begin_and_end_on_a_match(ref, oracle_rows):
    """The noisy set asserts claim 0 alone (test_oracle_rows_are_optimal[noisy]); claim C is MEASURED on it and the part of
    it that the first fixed point does not decide is asserted.  Measured: 5 of the oracle's 66 rows begin with a gap or a
    mismatch (`1D12=`, `1X2=2D`, `1I3=`, `2D1X12=`, `2I10=`); every row ends on a match.  A piece's first fixed point is the
    start of its first anchor, taken `span` bases before the anchor's end in BOTH reads with the query's span (DESIGN.md
    section 5 item 5, and the deviations table); anchors are homopolymer-compressed k-mers, and where a run of the k-mer is
    longer in one read the two starts are not homologous: the anchor's own block opens with a gap or a mismatch, and a left
    extension that gains nothing leaves it as the row's first column.  Asserted: every row ENDS on a match of two ACGT
    bases (a piece ends on a run's last base in both reads); a row that does not begin on one has a left extension with
    nothing to gain (claim B at that end: the rule, not the extension, put the start there)."""
    exe, d = ref
    seqs, _, o, text = oracle_rows.get("noisy")
    reps, bad = AS.check_set(exe, text, seqs, o, d, "C", ties=False, name="noisy_c")
    print(f"noisy: claim C fails on {len(bad.get('C', []))} of {len(reps)} rows: " + ", ".join(r.row.cg[:12] for r in bad.get("C", [])))
    AS.assert_first_fixed_point_alone(reps, bad.get("C", []))


def test_sets_hold_what_they_are_for(oracle_rows):
    """The planted differences show in the oracle's rows: every indel length as an I and as a D op, the split rows, both
    strands - and the sets keep the sizes the reference's running time was planned for."""
    for name in AI.SETS:
        seqs = oracle_rows.get(name)[0]
        assert len(seqs) <= 40 and max(map(len, seqs.values())) <= AI.MAX_READ, name
    ops = {op for l in oracle_rows.get("planted")[3].split("\n")[:-1] for op in re.findall(r"\d+[ID]", l.split("cg:Z:")[1])}
    assert {f"{n}{k}" for n in AI.INDELS for k in "ID"} <= ops
    assert {l.split("\t")[4] for l in oracle_rows.get("planted")[3].split("\n")[:-1]} == {"+", "-"}
    ops = {op for l in oracle_rows.get("long_block")[3].split("\n")[:-1] for op in re.findall(r"\d+[ID]", l.split("cg:Z:")[1])}
    assert {f"{n}{k}" for n in AI.SHIFTS if n for k in "ID"} <= ops
    split = oracle_rows.get("split")
    assert len(split[3].split("\n")) - 1 == 3 * (len(split[0]) // 2)          # two planted 40 / 41-base indels: three rows a pair
    assert not re.findall(r"(?:40|41)[ID]", split[3])


def test_reference_under_sanitizers(ref, oracle_rows, tmp_path):
    """The stand-alone program once more with -fsanitize=address,undefined, on the job file of the short set and on the
    literals' kinds of task (empty strings, corridors that bind, --path)."""
    exe, d = ref
    san = AS.compile_reference(tmp_path, sanitize=True)
    seqs, _, o, text = oracle_rows.get("short")
    c = AS.constants(o)
    tasks = []
    for r in AS.read_rows(text, seqs)[:12]:
        tasks += [AS.global_task(r.a, r.b, c, -20, 20), AS.extend_task(r.qa[r.qe:], r.t[r.te:], c)]
    tasks += [AS.global_task("-", "-", c, 0, 0), AS.global_task("-", "ACG", c, -1, 1), AS.global_task("ACGT", "A", c, -5, -3),
              AS.extend_task("-", "-", c), AS.extend_task("ACGT", "ACGT", c, rows=0, cols=0, band=0)]
    for path in (False, True):
        assert AS.run_reference(san, tasks, tmp_path, path=path, name="san") == AS.run_reference(exe, tasks, tmp_path, path=path, name="plain")
    r = subprocess.run([san, str(tmp_path / "missing.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot read" in r.stderr
