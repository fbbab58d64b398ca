"""CPU: the model of ViralQuasispecies --graph_only (tests/vq_graph_model.py) on hand-made graphs whose answers are worked
out by hand, and its libstdc++ pieces against the compiler's own.  PARITY UNPINNED (the reference needs Boost)."""
import random
import shutil
import subprocess

import pytest

import vq_graph_model as M  # noqa: E402  (tests/ is on sys.path under pytest's rootdir-relative import)


def _case(tmp_path, lens, rows, **opts):
    """Reads 1..n of the given lengths (vertex = id - 1), one overlap row per edge: (id1, id2, pos1, ori1, ori2) plus
    optional len, perc, score, mr, pos2.  Scores are given, not computed: pos3 follows the read lengths."""
    rng = random.Random(len(lens))
    fq = tmp_path / "singles.fastq"
    fq.write_text("".join(f"@{k + 1}\n{''.join(rng.choice('ACGT') for _ in range(n))}\n+\n{'=' * n}\n"
                          for k, n in enumerate(lens)))
    ov = tmp_path / "ov.savage"
    lines, scores = [], []
    for r in rows:
        a, b, pos1, o1, o2 = r[:5]
        x = r[5] if len(r) > 5 else {}
        ln = x.get("len", min(lens[a - 1] - pos1, lens[b - 1]))
        pos2 = x.get("pos2", "-")
        lines.append(f"{a}\t{b}\t{pos1}\t{pos2}\t-\t{o1}\t{o2}\t{x.get('perc', 99)}\t-\t{ln}\t-\ts\ts")
        scores.append((x.get("score", 0.99), x.get("mr", 0.0), lens[a - 1] - pos1 - lens[b - 1]))
    ov.write_text("\n".join(lines) + "\n")
    o = dict(min_overlap_len=1, edge_threshold=0.5, remove_trans=0, remove_tips=False, remove_branches=False, ignore_inclusions=False)
    o.update(opts)
    return str(fq), str(ov), scores, o


def _run(tmp_path, lens, rows, **opts):
    fq, ov, scores, o = _case(tmp_path, lens, rows, **opts)
    out = tmp_path / "out"
    st = M.graph(fq, ov, str(out), scores=scores, **o)
    files = {n: (out / n).read_text() for n in M.OUTPUTS if (out / n).exists()}
    return st, files


def _digraph(files):
    return [tuple(map(int, l.split("\t"))) for l in files["digraph.txt"].splitlines()]


def test_odd_cycle_of_flipping_edges_deletes_one_conflict(tmp_path):
    # three edges that each ask for different labels at their ends: no labelling satisfies all three
    st, files = _run(tmp_path, [500] * 3, [(1, 2, 100, "+", "-"), (2, 3, 100, "+", "-"), (1, 3, 200, "+", "-")])
    assert st["edges_built"] == 3 and st["conflicts"] == 1 and len(_digraph(files)) == 2


def test_flipped_edge_moves_to_the_other_list(tmp_path):
    # 1 -> 2 read '-' '-': the labels are both '+', so the edge flips; pos3 = 500 - 100 - 500 < 0 turns it into 2 -> 1
    st, files = _run(tmp_path, [500, 500], [(1, 2, 100, "-", "-")])
    assert st["moved"] == 1 and st["conflicts"] == 0 and _digraph(files) == [(1, 0)]
    # the same with pos3 >= 0 flips in place and stays 1 -> 2
    st, files = _run(tmp_path, [500, 300], [(1, 2, 100, "-", "-")])
    assert st["moved"] == 0 and _digraph(files) == [(0, 1)]


@pytest.mark.parametrize("first,second,winner", [
    (dict(score=0.98), dict(score=0.99), 1),                  # score
    (dict(score=0.99), dict(score=0.98), 0),
    (dict(len=300), dict(len=310), 1),                        # equal score: the longer overlap
    (dict(len=310), dict(len=300), 0),
    (dict(mr=0.01), dict(mr=0.0), 1),                         # then the lower mismatch rate
    (dict(mr=0.0), dict(mr=0.01), 0),
    (dict(pos2=7), dict(pos2=3), 1),                          # ... the smaller pos2
    (dict(pos2=3), dict(pos2=7), 0),
    (dict(), dict(), 1),                                      # fully equal: the later candidate replaces
])
def test_duplicate_tie_break(tmp_path, first, second, winner):
    lens = [600, 600, 600]
    rows = [(1, 2, 100, "+", "+", dict(first, len=first.get("len", 300))),
            (1, 3, 50, "+", "+"),
            (1, 2, 100, "+", "+", dict(second, len=second.get("len", 300)))]
    fq, ov, scores, o = _case(tmp_path, lens, rows)
    m, _, st = M.build(fq, ov, scores=scores, **o)
    assert st["duplicates"] == 1 and st["edges_built"] == 2
    kept = [e for e in m.adj[0] if e["v2"] == 1][0]
    assert kept["k"] == (0 if winner == 0 else 2)
    # a replacement is appended: the later winner ends the list
    assert [e["v2"] for e in m.adj[0]] == ([1, 2] if winner == 0 else [2, 1])


@pytest.mark.parametrize("first,second,winner", [
    ((1, 2, 100, "+", "+"), (2, 1, 100, "+", "+"), 0),        # vertex(1): the smaller source stays
    ((2, 1, 100, "+", "+"), (1, 2, 100, "+", "+"), 1),
    ((1, 2, 100, "+", "+"), (1, 2, 100, "-", "-"), 0),        # ori1: '+' stays
    ((1, 2, 100, "-", "-"), (1, 2, 100, "+", "+"), 1),
    ((1, 2, 100, "+", "+"), (1, 2, 120, "+", "+"), 0),        # pos1: the smaller stays
    ((1, 2, 120, "+", "+"), (1, 2, 100, "+", "+"), 1),
])
def test_duplicate_tie_break_direction_and_orientation(tmp_path, first, second, winner):
    rows = [first + (dict(len=300),), second + (dict(len=300),)]
    fq, ov, scores, o = _case(tmp_path, [600, 600], rows)
    m, _, st = M.build(fq, ov, scores=scores, **o)
    edges = m.adj[0] + m.adj[1]
    assert len(edges) == 1 and edges[0]["k"] == winner and st["duplicates"] == 1


def test_ori2_rung(tmp_path):
    # same vertex(1) and ori1, different ori2 needs ori1 != ori2 on one and == on the other: two keys, no duplicate; with
    # ori1 equal the class differs, so the ori2 rung is only reached through two candidates of one class and direction
    rows = [(1, 2, 100, "-", "+", dict(len=300)), (2, 1, 100, "-", "+", dict(len=300))]
    fq, ov, scores, o = _case(tmp_path, [600, 600], rows)
    _, _, st = M.build(fq, ov, scores=scores, **o)
    assert st["duplicates"] == 1


def test_inclusion_only_from_the_first_candidate(tmp_path):
    lens = [600, 300, 600]
    # 1 contains 2 (pos3 = 600 - 100 - 300 > 0: vertex 2 is included); the first candidate of the key has perc 99, the
    # later, better one perc 100: it replaces the edge but marks nothing
    rows = [(1, 2, 100, "+", "+", dict(perc=99, score=0.98)), (1, 2, 100, "+", "+", dict(perc=100, score=0.99))]
    fq, ov, scores, o = _case(tmp_path, lens, rows, ignore_inclusions=True)
    m, incl, st = M.build(fq, ov, scores=scores, **o)
    assert incl == [0, 0, 0] and st["inclusions"] == 1 and m.adj[0][0]["k"] == 1
    rows.reverse()                                            # now the first candidate marks it
    fq, ov, scores, o = _case(tmp_path, lens, rows, ignore_inclusions=True)
    m, incl, st = M.build(fq, ov, scores=scores, **o)
    assert incl == [0, 1, 0] and m.adj[0][0]["k"] == 0
    st, files = _run(tmp_path, lens, rows + [(2, 3, 50, "+", "+")], ignore_inclusions=True)
    assert files["graph.txt"].splitlines()[:2] == ["3", "0"] and _digraph(files) == []


def test_transitive_removal_both_branches_agree(tmp_path):
    # a chain 1 -> 2 -> 3 -> 4 -> 5 with every shortcut: 6 of 10 edges are transitive (> 50 %); a second, sparse graph
    # (one shortcut among 5 edges) takes the other branch by itself
    lens = [1000] * 5
    rows = [(a, b, 100 * (b - a), "+", "+") for a in range(1, 6) for b in range(a + 1, 6)]
    fq, ov, scores, o = _case(tmp_path, lens, rows)
    res = []
    for branch in (True, False):
        m, _, st = M.build(fq, ov, scores=scores, **o)
        m.sort_edges()
        M.label_vertices(m, st)
        M.remove_transitive(m, 1, st, branch)
        res.append([[e["v2"] for e in l] for l in m.adj])
    assert res[0] == res[1] == [[1], [2], [3], [4], []] and st["transitive"] == 6
    st, files = _run(tmp_path, lens, rows, remove_trans=1)
    assert _digraph(files) == [(0, 1), (1, 2), (2, 3), (3, 4)] and st["transitive"] == 6
    st, files = _run(tmp_path, lens, rows, remove_trans=2)       # double transitive: 1 -> 5 only (through 1 -> 3 -> 5)
    assert st["transitive"] == 1 and len(_digraph(files)) == 9 and (0, 4) not in _digraph(files)


def test_tips(tmp_path):
    # out-tip: 1 -> 2 (2 has no out-edge, extends 1 by 100 < max_tip_len) next to 1 -> 3 -> 4: 1 -> 2 goes, read 2 is a tip
    lens = [500, 500, 500, 500]
    rows = [(1, 2, 100, "+", "+"), (1, 3, 50, "+", "+"), (3, 4, 100, "+", "+")]
    st, files = _run(tmp_path, lens, rows, remove_tips=True)
    assert _digraph(files) == [(0, 2), (2, 3)] and files["tips.txt"] == "1\n" and st["tip_edges"] == 1
    # all out-neighbours tips: nothing goes
    st, files = _run(tmp_path, lens[:3], rows[:2], remove_tips=True)
    assert len(_digraph(files)) == 2 and files["tips.txt"] == "" and st["tip_reads"] == 0
    # ... except an inclusion tip (ext_len 0: read 2 ends inside read 1)
    st, files = _run(tmp_path, [500, 300, 500], [(1, 2, 100, "+", "+", dict(len=300)), (1, 3, 50, "+", "+")],
                     remove_tips=True)
    assert _digraph(files) == [(0, 2)] and files["tips.txt"] == "1\n"
    # in-tip: 2 -> 4 with 2 without in-edges (pos1 50 < max_tip_len) next to 1 -> 3 -> 4
    rows = [(1, 3, 100, "+", "+"), (3, 4, 100, "+", "+"), (2, 4, 50, "+", "+")]
    st, files = _run(tmp_path, lens, rows, remove_tips=True)
    assert (1, 3) not in _digraph(files) and files["tips.txt"] == "1\n"
    st, files = _run(tmp_path, lens, rows, remove_tips=True, max_tip_len=50)      # not shorter than max_tip_len
    assert (1, 3) in _digraph(files) and files["tips.txt"] == ""


def test_branches_y_split_and_one_sided_lists(tmp_path):
    lens = [500] * 5
    # Y: 1 -> 3, 2 -> 3, 3 -> 4: 3's in-list is cleared, so 1 and 2 are components of their own
    st, files = _run(tmp_path, lens[:4], [(1, 3, 100, "+", "+"), (2, 3, 150, "+", "+"), (3, 4, 100, "+", "+")],
                     remove_trans=1, remove_branches=True)
    assert _digraph(files) == [(2, 3)] and st["branch_edges"] == 2
    # 1 -> 2, 1 -> 3, 3 -> 4: 1's out-list is cleared while 2's and 3's in-lists still hold 1 - an edge joins only when
    # both lists hold it, so 1 stays alone and both of its edges go
    st, files = _run(tmp_path, lens[:4], [(1, 2, 100, "+", "+"), (1, 3, 150, "+", "+"), (3, 4, 100, "+", "+")],
                     remove_trans=1, remove_branches=True)
    assert _digraph(files) == [(2, 3)] and st["branch_edges"] == 2


def test_three_cycle_back_edge(tmp_path):
    st, files = _run(tmp_path, [500] * 3, [(1, 2, 100, "+", "+"), (2, 3, 100, "+", "+"), (3, 1, 100, "+", "+")],
                     remove_trans=1, remove_branches=True, remove_tips=True)
    assert files["cycles.txt"] == "2\t0\n" and st["backedges"] == 1 and _digraph(files) == [(0, 1), (1, 2)]
    head = files["graph.txt"].splitlines()
    assert head[0] == "3" and int(head[1]) == len(head) - 2 == 4
    st, files = _run(tmp_path, [500] * 3, [(1, 2, 100, "+", "+"), (2, 3, 100, "+", "+")])
    assert "cycles.txt" not in files and st["backedges"] == 0


def test_no_edges_writes_only_nonedges(tmp_path):
    st, files = _run(tmp_path, [500, 500], [(1, 2, 100, "+", "+", dict(score=0.95, mr=0.5))], edge_threshold=0.99)
    assert st["edges_built"] == 0 and set(files) == {"nonedge_overlaps.txt"}
    assert files["nonedge_overlaps.txt"] == "1\t2\t100\t0\t-\t+\t+\t99\t0\t400\t0\ts\ts\n"


_SHUFFLE_CPP = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
int main() {
    for (unsigned seed = 1; seed <= 120; ++seed)
        for (int n = 0; n <= 64; ++n) {
            std::vector<int> v(n);
            for (int i = 0; i < n; ++i) v[i] = i;
            std::srand(seed);
            std::random_shuffle(v.begin(), v.end());
            for (int x : v) printf("%d ", x);
            printf("\n");
        }
}
"""

_SORT_CPP = r"""
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>
int main() {
    int n, k;
    while (scanf("%d", &n) == 1) {
        std::vector<std::pair<int, int>> v(n);
        for (int i = 0; i < n; ++i) { scanf("%d", &k); v[i] = {k, i}; }
        std::sort(v.begin(), v.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
        for (auto &p : v) printf("%d ", p.second);
        printf("\n");
    }
}
"""


def _compile(tmp_path, name, src):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / (name + ".cpp")).write_text(src)
    exe = tmp_path / name
    subprocess.check_call([gxx, "-O1", "-w", "-o", str(exe), str(tmp_path / (name + ".cpp"))])
    return str(exe)


def test_shuffle_matches_std_random_shuffle(tmp_path):
    exe = _compile(tmp_path, "shuffle", _SHUFFLE_CPP)
    want = subprocess.check_output([exe], text=True).splitlines()
    got = [" ".join(map(str, M.random_shuffle(list(range(n)), seed))) + (" " if n else "")
           for seed in range(1, 121) for n in range(65)]
    assert got == want


def test_std_sort_matches_libstdcxx(tmp_path):
    # few distinct keys: the order among equal keys is std::sort's own, for lengths through the insertion-sort cut-off and
    # the partitioning
    exe = _compile(tmp_path, "sort", _SORT_CPP)
    rng = random.Random(3)
    cases = [[rng.randrange(kk) for _ in range(n)] for n in list(range(0, 40)) + [100, 257, 1000] for kk in (1, 2, 5)]
    cases.append([0] * 300)
    cases.append(list(range(200, 0, -1)) * 2)
    inp = "".join(f"{len(c)} " + " ".join(map(str, c)) + "\n" for c in cases)
    want = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
    got = []
    for c in cases:
        pairs = [(k, i) for i, k in enumerate(c)]
        M.std_sort(pairs, lambda a, b: a[0] < b[0])
        got.append(" ".join(str(i) for _, i in pairs) + (" " if c else ""))
    assert got == want


def test_cli_refuses_what_is_not_on_the_path(tmp_path):
    from hylight_amd import vq_graph as CLI
    base = ["--singles", str(tmp_path / "s.fq"), "--overlaps", str(tmp_path / "o"), "--out", str(tmp_path / "d")]
    for extra in (["--add_duplicates", "true"], ["--resolve_orientations", "false"], ["--branch_reduction", "1"]):
        assert CLI.main(base + extra) == CLI.EXIT_REFUSED
    assert not (tmp_path / "d").exists()
