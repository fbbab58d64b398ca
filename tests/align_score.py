"""Scores PAF rows of the overlapper from their cg:Z: string and the two sequences, and holds them to the plain reference
(tests/capi/align_ref_check.cpp).  Nothing here reads the oracle's or the library's code: the scores are DESIGN.md section 5
restated - a column of two ACGT bases +match / -mismatch, any other byte -ambi; a gap of L bases min(o1 + e1 L, o2 + e2 L);
every I or D op of the string is one gap.

The claims (tests/test_align_optimal.py, tests/test_gpu_align_optimal.py), with S the row's score and S* the reference's
global score over the row's two substrings inside a corridor of CORRIDOR diagonals around the row's own path:
  0  S <= S*                        (holds for any true alignment: guards the scorer and the reference)
  A  S == S*                        (the row is an optimal alignment of its two substrings)
  B  `extend` from either end of the row outward (EXT_ROWS x EXT_COLS, |diagonal| <= EXT_B) finds nothing above 0
  C  the first and the last column are matches of two ACGT bases; `ties`: beyond the outermost run of >= k `=` columns (the
     last anchor at the latest) no prefix / suffix of the row scores <= 0 - an extension takes the smallest i + j among
     equal best cells, so it never carries a tail that gains nothing.
"""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "capi", "align_ref_check.cpp")

CORRIDOR = 64                 # diagonals on either side of the row's path: the widest band of any task
EXT_ROWS, EXT_COLS, EXT_B = 200, 264, 8

_CODE = {c: i for i, c in enumerate("ACGT")}
_CODE.update({c.lower(): i for c, i in list(_CODE.items())})
_CODE.update({"U": 3, "u": 3})
_COMP = str.maketrans("ACGTUacgtu", "TGCAAtgcaa")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def constants(o):
    """(match, mismatch, ambi, o1, e1, o2, e2) of an option set (oracle.ava.Opts or api.AvaOpts)"""
    return (o.match, o.mismatch, o.ambi, o.gap_open, o.gap_ext, max(o.gap_open2, 0), o.gap_ext2)


def gap_cost(c, L):
    _, _, _, o1, e1, o2, e2 = c
    return min(o1 + e1 * L, o2 + e2 * L) if o2 > 0 else o1 + e1 * L


def column_score(c, a, b):
    x, y = _CODE.get(a), _CODE.get(b)
    if x is None or y is None:
        return -c[2]
    return c[0] if x == y else -c[1]


class Scored:
    """score: S; dlo, dhi: lowest / highest diagonal j - i the path visits, (0, 0) the row's start; units: (op, score) per
    =/X column and per gap, in row order; n_cols, n_match: columns and `=` columns; first_ok / last_ok: that column is a match
    of two ACGT bases"""
    __slots__ = ("score", "dlo", "dhi", "units", "n_cols", "n_match", "first_ok", "last_ok")


def parse_cigar(cg):
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cg)]
    assert "".join(f"{n}{op}" for n, op in ops) == cg and all(n > 0 for n, _ in ops), cg
    return ops


def score_alignment(cg, a, b, c):
    """Scores the alignment `cg` (=/X/I/D; I consumes a, D consumes b) of the strings a and b under the constants c.  Raises
    AssertionError where the string is no alignment of the two: lengths, `=` on unequal bases, `X` on equal ones."""
    r = Scored()
    i = j = 0
    r.score, r.dlo, r.dhi, r.units, r.n_cols, r.n_match = 0, 0, 0, [], 0, 0
    for n, op in parse_cigar(cg):
        r.n_cols += n
        if op in "=X":
            r.n_match += n if op == "=" else 0
            for _ in range(n):
                x, y = _CODE.get(a[i], 4), _CODE.get(b[j], 4)          # two bytes outside ACGT print as `=`
                assert (x == y) == (op == "="), (cg, i, j, a[i], b[j], op)
                s = column_score(c, a[i], b[j])
                r.score += s
                r.units.append((op, s))
                i += 1
                j += 1
        else:
            s = -gap_cost(c, n)
            r.score += s
            r.units.append((op, s))
            if op == "I":
                i += n
            else:
                j += n
            r.dlo, r.dhi = min(r.dlo, j - i), max(r.dhi, j - i)
    assert i == len(a) and j == len(b), (cg, i, len(a), j, len(b))

    r.first_ok = bool(r.units) and r.units[0][0] == "=" and a[0] in _CODE and b[0] in _CODE
    r.last_ok = bool(r.units) and r.units[-1][0] == "=" and a[-1] in _CODE and b[-1] in _CODE
    return r


class PafRow:
    """One row with its sequences in aligned orientation: qa the whole query (reverse complement on '-'), the row covers
    qa[qs:qe] and t[ts:te]."""

    def __init__(self, line, seqs):
        f = line.split("\t")
        self.line = line
        self.qname, self.tname, self.strand = f[0], f[5], f[4]
        ql, qs, qe = int(f[1]), int(f[2]), int(f[3])
        self.ts, self.te = int(f[7]), int(f[8])
        self.qs, self.qe = (ql - qe, ql - qs) if self.strand == "-" else (qs, qe)
        self.qa = revcomp(seqs[self.qname]) if self.strand == "-" else seqs[self.qname]
        self.t = seqs[self.tname]
        assert len(self.qa) == ql and len(self.t) == int(f[6])
        cg = [x for x in f[12:] if x.startswith("cg:Z:")]
        self.cg = cg[0][5:] if cg else "*"
        self.bare = self.cg == "*"
        self.nm = int([x for x in f[12:] if x.startswith("NM:i:")][0][5:])
        self.n_match, self.n_cols = int(f[9]), int(f[10])

    @property
    def a(self):
        return self.qa[self.qs:self.qe]

    @property
    def b(self):
        return self.t[self.ts:self.te]


def read_rows(text, seqs):
    return [PafRow(l, seqs) for l in text.split("\n") if l]


# ---- the reference program ---------------------------------------------------------------------------------------------

def compile_reference(outdir, sanitize=False):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler on PATH"
    exe = os.path.join(str(outdir), "align_ref_check" + ("_san" if sanitize else ""))
    flags = ["-std=c++17"] + (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"])
    subprocess.run([cxx, *flags, REF_SRC, "-o", exe], check=True)
    return exe


def global_task(a, b, c, dlo, dhi):
    return "global %s %s %s %d %d" % (a or "-", b or "-", " ".join(map(str, c)), dlo, dhi)


def extend_task(a, b, c, rows=EXT_ROWS, cols=EXT_COLS, band=EXT_B):
    return "extend %s %s %s %d %d %d" % (a[:rows] or "-", b[:cols] or "-", " ".join(map(str, c)), rows, cols, band)


def run_reference(exe, tasks, workdir, path=False, name="tasks"):
    """-> one answer per task: the score (None: no alignment inside the corridor), with path=True (score, CIGAR)"""
    job = os.path.join(str(workdir), name + ".txt")
    with open(job, "w") as f:
        f.write("".join(t + "\n" for t in tasks))
    r = subprocess.run([exe] + (["--path"] if path else []) + [job], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(tasks), (len(out), len(tasks))

    def one(l):
        f = l.split(" ")
        s = None if f[0] == "none" else int(f[0])
        return (s, f[1] if len(f) > 1 else None) if path else s
    return [one(l) for l in out]


# ---- the claims --------------------------------------------------------------------------------------------------------

class RowReport:
    __slots__ = ("row", "scored", "best", "ext_left", "ext_right", "tie_left", "tie_right")

    @property
    def loss(self):
        return self.best - self.scored.score


def _tail_gains_nothing(units, k):
    """True when, after the last run of >= k `=` columns, some suffix of the row scores <= 0"""
    run, cut = 0, None
    for x, (op, _) in enumerate(units):
        run = run + 1 if op == "=" else 0
        if run >= k:
            cut = x + 1
    if cut is None:
        return False
    s = 0
    for _, v in reversed(units[cut:]):
        s += v
        if s <= 0:
            return True
    return False


def judge(exe, rows, c, workdir, k, name="rows"):
    """Scores every row that is not bare and asks the reference for S* and for the two outward extensions -> [RowReport]"""
    reps, tasks = [], []
    for r in rows:
        if r.bare:
            continue
        rep = RowReport()
        rep.row, rep.scored = r, score_alignment(r.cg, r.a, r.b, c)
        sc = rep.scored
        assert (r.n_cols, r.n_match, r.nm) == (sc.n_cols, sc.n_match, sc.n_cols - sc.n_match), r.line[:200]
        tasks.append(global_task(r.a, r.b, c, sc.dlo - CORRIDOR, sc.dhi + CORRIDOR))
        tasks.append(extend_task(r.qa[:r.qs][::-1], r.t[:r.ts][::-1], c))
        tasks.append(extend_task(r.qa[r.qe:], r.t[r.te:], c))
        rep.tie_right = _tail_gains_nothing(sc.units, k)
        rep.tie_left = _tail_gains_nothing(sc.units[::-1], k)
        reps.append(rep)
    ans = run_reference(exe, tasks, workdir, name=name)
    for x, rep in enumerate(reps):
        rep.best, rep.ext_left, rep.ext_right = ans[3 * x], ans[3 * x + 1], ans[3 * x + 2]
    return reps


def describe(exe, rep, c, workdir):
    """a failing row next to one optimal path of the reference (diagnosis)"""
    r, sc = rep.row, rep.scored
    (best, cg), = run_reference(exe, [global_task(r.a, r.b, c, sc.dlo - CORRIDOR, sc.dhi + CORRIDOR)], workdir, path=True, name="path")
    return (f"{r.qname} {r.strand} {r.tname} q[{r.qs},{r.qe}) t[{r.ts},{r.te}): S {sc.score} S* {best} ext {rep.ext_left}/{rep.ext_right}\n"
            f"  row {r.cg}\n  ref {cg}")


def claim0(reps):
    return [rep for rep in reps if rep.best is None or rep.scored.score > rep.best]


def claimA(reps):
    return [rep for rep in reps if rep.best is None or rep.scored.score != rep.best]


def claimB(reps):
    return [rep for rep in reps if rep.ext_left != 0 or rep.ext_right != 0]


def claimC(reps, ties=False, end_bonus=0):
    """ties: also the tail rule (sets whose anchors are exact matches); with an end bonus an end that reaches the query's
    end is exempt from it: the bonus ranks such a cell above a better-scoring one."""
    bad = []
    for rep in reps:
        r, sc = rep.row, rep.scored
        ok = sc.first_ok and sc.last_ok
        if ties:
            if rep.tie_left and not (end_bonus > 0 and r.qs == 0):
                ok = False
            if rep.tie_right and not (end_bonus > 0 and r.qe == len(r.qa)):
                ok = False
        if not ok:
            bad.append(rep)
    return bad


def assert_first_fixed_point_alone(reps, bad):
    """Rows of reads with errors that miss claim C (`bad`) miss it for the first fixed point's sake alone: all rows end on a
    match; a row that begins on none gains nothing to its left (claim B at that end)."""
    assert not [r.row.line[:200] for r in reps if not r.scored.last_ok]
    for rep in bad:
        assert not rep.scored.first_ok, rep.row.line[:200]
        assert rep.ext_left == 0, rep.row.line[:200]


def loss_figures(reps):
    """(rows, rows with S < S*, mean loss over all rows, largest loss)"""
    losses = [rep.loss for rep in reps]
    return len(losses), sum(l > 0 for l in losses), (sum(losses) / len(losses) if losses else 0.0), max(losses, default=0)


def paf_line(qname, ql, qs, qe, tname, tl, ts, te, cg, strand="+"):
    """a row as the overlapper writes it, for hand-made alignments"""
    ops = parse_cigar(cg)
    cols, match = sum(n for n, _ in ops), sum(n for n, op in ops if op == "=")
    return f"{qname}\t{ql}\t{qs}\t{qe}\t{strand}\t{tname}\t{tl}\t{ts}\t{te}\t{match}\t{cols}\t0\tNM:i:{cols - match}\ttp:A:S\tcg:Z:{cg}"


def misses_boundary(rep, bounds, slack=30):
    """chimera rows: the row's end on the side where the homology ends inside both reads lies within `slack` bases of the
    boundary, in the query and in the target"""
    r = rep.row
    (pq, q_left), (pt, t_left) = bounds[r.qname], bounds[r.tname]
    if r.strand == "-":
        pq, q_left = len(r.qa) - pq, not q_left
    assert q_left == t_left, r.line[:120]
    q_end, t_end = (r.qe, r.te) if t_left else (r.qs, r.ts)
    return abs(q_end - pq) > slack or abs(t_end - pt) > slack


def check_set(exe, text, seqs, opts, workdir, claims, ties=True, bounds=None, name="rows"):
    """Judges the rows of `text` and returns (reports, {claim: [failing reports]}) for the claims named in `claims` (a string
    of 0, A, B, C; chimera sets: `bounds`)."""
    c = constants(opts)
    reps = judge(exe, read_rows(text, seqs), c, workdir, opts.k, name=name)
    bad = {}
    if "0" in claims:
        bad["0"] = claim0(reps)
    if "A" in claims:
        bad["A"] = claimA(reps)
    if "B" in claims:
        bad["B"] = claimB(reps)
    if "C" in claims:
        bad["C"] = claimC(reps, ties=ties, end_bonus=opts.end_bonus)
    if bounds is not None:
        bad["boundary"] = [rep for rep in reps if misses_boundary(rep, bounds)]
    return reps, {k: v for k, v in bad.items() if v}


def failure_text(exe, bad, opts, workdir, limit=4):
    c = constants(opts)
    return "\n".join(f"claim {k}: {len(v)} rows\n" + "\n".join(describe(exe, rep, c, workdir) for rep in v[:limit]) for k, v in bad.items())
