"""tests/vq_branch_model.py held to hand-worked cases, one per oddity of BranchReduction.cpp it restates (the expected values are
worked out by hand in each test's docstring), its unordered_map order held to the compiler's own container, the table parser,
the CLI's refusals and the new symbols.  No GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_branch_model as B  # noqa: E402
import vq_graph_model as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model(seqs, edges):
    """edges: (u, v, pos1, len[, ori1, ori2]) in list order."""
    m = G.Model(list(seqs))
    for k, e in enumerate(edges):
        u, v, pos1, ln = e[:4]
        o1, o2 = (e[4], e[5]) if len(e) > 4 else (True, True)
        m.adj[u].append(dict(v1=u, v2=v, pos1=pos1, pos2=0, pos3=0, pos4=0, ori1=o1, ori2=o2, len=ln, perc=50, score=2.0, mr=0.0, k=k))
    return m


def reduction(seqs, edges, orient=None, originals=None, oseq=None, se=None, pe=0, table=None, careful=True, mol=0):
    m = model(seqs, edges)
    originals = originals if originals is not None else [{v: (True, 0, len(s))} for v, s in enumerate(seqs)]
    oseq = oseq if oseq is not None else dict(enumerate(seqs))
    se = len(oseq) if se is None else se
    return B.Reduction(m, orient or [True] * len(seqs), originals, oseq, se, pe, table or {}, careful, mol, 0.97)


# ---- the difference lists ------------------------------------------------------------------------------------------------
def test_neighbours_are_oriented_by_the_branching_vertex():
    """0 -> 1 and 0 -> 2, both at 5.  Forward: AAAAAC / AAAAAG differ at 5 -> 5 + 5 = 10.  Vertex 0 labelled reverse, 1 and 2
    forward: the neighbours are reverse-complemented all the same, GTTTTT / CTTTTT differ at 0 -> 0 + 5 = 5."""
    seqs, edges = ["A" * 10, "AAAAAC", "AAAAAG"], [(0, 1, 5, 5), (0, 2, 5, 5)]
    assert reduction(seqs, edges).diff_list(0, [1, 2], True)[:2] == ([10], 10)
    assert reduction(seqs, edges, orient=[False, True, True]).diff_list(0, [1, 2], True)[:2] == ([5], 5)


def test_in_branch_startpos_reversal_and_report():
    """1 -> 0 at 3, 2 -> 0 at 5: max_pos 5, startpos 2 and 0.  pos_i 2 > pos_j 0: relative_pos 2, len min(8 - 2, 6) = 6, CCATTT
    against GGCCGTTT[2:] = CCGTTT; reversed TTTACC / TTTGCC differ at 3, reported 6 - 3 + 2 = 5.  distance: overlap_len =
    min(6 - 3, 8 - 5) = 3, 3 + |read 0| 10 - 3 = 10."""
    r = reduction(["TTTAAAAAAA", "CCATTT", "GGCCGTTT"], [(1, 0, 3, 3), (2, 0, 5, 3)])
    diff, dist, _, start, _ = r.diff_list(0, [1, 2], False)
    assert (diff, dist, start) == ([5], 10, [2, 0])


def test_find_diff_pos_stops_at_100():
    assert B.find_diff_pos("A" * 150, "C" * 150) == list(range(100))
    assert B.find_diff_pos("A" * 99 + "C" + "A" * 50, "C" * 99 + "C" + "C" * 50) == list(range(99)) + [100]


def test_distance_takes_the_first_neighbours_pairs_only_and_truncates():
    """Three neighbours at 0.  1 / 2 differ at 4, 1 / 3 at 4, 2 / 3 at 9 only: distance_vec = [4, 4] (i == 0), dist 4; with the
    pair (2, 3) it would be int(0.5 * (4 + 9)) = 6.  Then 1 / 2 at 3 and 1 / 3 at 8: int(0.5 * 11) = 5."""
    edges = [(0, 1, 0, 10), (0, 2, 0, 10), (0, 3, 0, 10)]
    r = reduction(["A" * 10, "A" * 10, "AAAACAAAAA", "AAAACAAAAG"], edges)
    assert r.diff_list(0, [1, 2, 3], True)[:2] == ([4, 9], 4)
    r = reduction(["A" * 10, "A" * 10, "AAACAAAAAA", "AAAAAAAACA"], edges)
    assert r.diff_list(0, [1, 2, 3], True)[:2] == ([3, 8], 5)


def test_inclusion_test_and_its_unsigned_subtraction():
    """min_overlap_len 5.  0 -> 1 at 2, 0 -> 2 at 8, |1| = 10: relative_pos 6 > int(10 - 5).  At 7 instead: 5 > 5 is false, the
    pair is compared over min(10 - 5, 4) = 4 bases.  |1| = 4 < 5 at equal positions: 4 - 5 wraps in size_t and int() brings -1
    back, 0 > -1: an inclusion of the second-named vertex (the else branch names node_j first)."""
    r = reduction(["A" * 12, "A" * 10, "AAAA"], [(0, 1, 2, 10), (0, 2, 8, 4)], mol=5)
    assert r.diff_list(0, [1, 2], True)[4] == [(1, 2)] and r.stats["pairs"] == 0
    r = reduction(["A" * 12, "A" * 10, "AAAC"], [(0, 1, 2, 10), (0, 2, 7, 4)], mol=5)
    assert r.diff_list(0, [1, 2], True)[0] == [3 + 7] and r.stats["pairs"] == 1
    # pos_i == pos_j takes the else branch: relative_pos > int(|seq_j| - 5) = 5 is false for j = 2 (10 bases) ...
    assert reduction(["A" * 12, "AAAA", "A" * 10], [(0, 1, 3, 4), (0, 2, 3, 9)], mol=5).diff_list(0, [1, 2], True)[4] == []
    # ... and true for j of 4 bases: 0 > int(4 - 5) = -1, named (node_j, node_i)
    assert reduction(["A" * 12, "A" * 10, "AAAA"], [(0, 1, 3, 9), (0, 2, 3, 4)], mol=5).diff_list(0, [1, 2], True)[4] == [(2, 1)]


def test_inclusion_in_a_two_branch_clears_it_and_in_a_three_branch_drops_the_neighbour():
    """Two neighbours: final_branch is cleared, nothing is stored.  Three, at 2, 3 and 8 with 10, 12 and 4 bases: the pair (1, 3) has
    relative_pos 6 > int(10 - 5), so 1 leaves final_branch and its evidence is not stored; (2, 3) has 5 > int(12 - 5) false and is
    compared; 2 and 3 stay."""
    r = reduction(["A" * 12, "A" * 10, "AAAA"], [(0, 1, 2, 10), (0, 2, 8, 4)], mol=5)
    assert r.branch_evidence(0, [1, 2], True)[0] == [] and r.evidence == {}
    r = reduction(["A" * 14, "A" * 10, "C" + "A" * 11, "AAAC"], [(0, 1, 2, 10), (0, 2, 3, 11), (0, 3, 8, 4)], mol=5)
    final, _ = r.branch_evidence(0, [1, 2, 3], True)
    assert final == [0, 2, 3] and sorted(r.evidence) == [(0, 2), (0, 3)]


def test_identical_overlap_makes_a_missing_edge_and_a_false_branch():
    """0 -> 1 at 4 (ori2 '-'), 0 -> 2 at 2 (ori2 '+'), both all A: pos_i 4 > pos_j 2, relative_pos 2, len min(10 - 2, 6) = 6,
    no difference.  Vertex order: pos_i < pos_j fails, so node_j = 2 first: 2 -> 1, pos1 2, pos2 0, ord '-', ori '+' '-', score =
    edge_threshold, perc floor(100 * 6 / 6) = 100.  The component of a false branch loses every edge."""
    r = reduction(["A" * 12, "A" * 6, "A" * 10], [(0, 1, 4, 6, True, False), (0, 2, 2, 10, True, True)], table={k: 0 for k in range(400)})
    missing, removed = r.run()
    e = missing[0]
    assert len(missing) == 1 and (e["v1"], e["v2"], e["pos1"], e["pos2"], e["ord"], e["ori1"], e["ori2"], e["len"], e["perc"], e["score"]) == \
        (2, 1, 2, 0, "-", True, False, 6, 100, 0.97)
    assert r.false_out == {0} and removed == [(0, 1), (0, 2)] and r.components == [] and r.stats["false_branches"] == 1
    # equal positions: the smaller vertex first
    r = reduction(["A" * 12, "A" * 6, "A" * 10], [(0, 2, 3, 9), (0, 1, 3, 6)])
    r.diff_list(0, [1, 2], True)
    assert (r.missing[0]["v1"], r.missing[0]["v2"], r.missing[0]["perc"]) == (1, 2, 100)


# ---- the evidence ------------------------------------------------------------------------------------------------------------
def test_check_read_evidence():
    """Contig ACGTACGT at 10, read at 10 + index.  True only with one listed position covered by both and none disagreeing."""
    c = "ACGTACGT"
    assert not B.check_read_evidence(c, 10, "ACGT", 0, [14, 20])            # covers none of the listed positions
    assert B.check_read_evidence(c, 10, "ACGT", 0, [11, 13, 17])            # agrees at 11 and 13; 17 is not covered by the read
    assert not B.check_read_evidence(c, 10, "ACGA", 0, [11, 13])            # disagrees at the last covered one
    assert B.check_read_evidence(c, 10, "TTAC", -2, [9, 10, 11])            # index -2: 9 is not on the contig, 10 and 11 agree
    assert not B.check_read_evidence(c, 10, "ACGT", 8, [18, 19])            # the read starts behind the contig's end
    assert not B.check_read_evidence(c, 10, "ACGT", 0, [])


def test_mate_branch_reads_the_subread_itself_and_records_the_joint_id():
    """se 1, pe 2: ids 0 | 1 2 | 3 4, original_readcount 5.  The branching vertex holds original 1; neighbour 1 holds original 3
    (>= se + pe: its /1 mate is 3 - 2 = 1) at index 0 and agrees with read 3's own sequence at the listed position 5 + 5 = 10;
    neighbour 2 holds original 2 (>= se: mate 2 + 2 = 4, absent) and 1 (present, but its read disagrees).  Evidence: [5 + min(3, 1)]
    = [6] and []."""
    seqs = ["A" * 10, "AAAAAC", "AAAAAG"]
    originals = [{1: (True, 0, 10)}, {3: (True, 0, 6)}, {2: (True, 0, 6), 1: (True, 0, 6)}]
    oseq = {0: "T", 1: "AAAAAT", 2: "AAAAAG", 3: "AAAAAC", 4: "T"}
    r = reduction(seqs, [(0, 1, 5, 5), (0, 2, 5, 5)], originals=originals, oseq=oseq, se=1, pe=2)
    r.branch_evidence(0, [1, 2], True)
    assert r.evidence == {(0, 1): [6], (0, 2): []} and r.stats["work_items"] == 3


def test_a_reverse_original_is_reverse_complemented():
    """Neighbour 1 = AAAAAC holds original 1 reverse at index 0: read 1 is GTTTTT, its reverse complement AAAAAC agrees at 10."""
    originals = [{1: (True, 0, 10), 2: (True, 0, 10)}, {1: (False, 0, 6)}, {2: (True, 0, 6)}]
    r = reduction(["A" * 10, "AAAAAC", "AAAAAG"], [(0, 1, 5, 5), (0, 2, 5, 5)], originals=originals,
                  oseq={0: "T", 1: "GTTTTT", 2: "AAAAAG"}, se=3)
    r.branch_evidence(0, [1, 2], True)
    assert r.evidence == {(0, 1): [1], (0, 2): [2]}


def test_second_visit_intersects_in_the_existing_lists_order():
    r = reduction(["A" * 10, "AAAAAC", "AAAAAG"], [(0, 1, 5, 5), (0, 2, 5, 5)])
    r.evidence[(0, 1)] = [9, 3, 7]                                        # (as a first visit left it)
    r.originals = [{3: (True, 0, 10), 7: (True, 0, 10), 8: (True, 0, 10)}, {3: (True, 0, 6), 7: (True, 0, 6), 8: (True, 0, 6)}, {}]
    r.oseq = {3: "AAAAAC", 7: "AAAAAC", 8: "AAAAAC"}
    r.se = 100
    r.branch_evidence(0, [1, 2], True)
    assert r.evidence[(0, 1)] == [3, 7] and r.evidence[(0, 2)] == []


# ---- the components ----------------------------------------------------------------------------------------------------------
SEQ120 = ["A" * 120] * 6


def test_double_branch_component_and_dist_clamps():
    """0 -> 2, 0 -> 3, 1 -> 2, 1 -> 3, every overlap 80 (< 100) at 40.  In-branches 2 and 3, out-branches 0 and 1.  The in-map
    {2, 3} iterates 3, 2 (head insertion).  From 3: its in-edges, then the out-branch of 0 (its edges, then the in-branch of 2 with
    its edges, then the out-branch of 1), one component of the four edges.  dist_node_pair is the LAST out-branch the loop of
    extendComponentOut entered at the top level - vertex 0 only (1 was visited inside the recursion) - so outnode 0, dist2 =
    the out-branch's 7.  dist1 = 3: clamped to len2 - 80 + 100 = 140; dist2 7 -> 140; dist = 140 + 140 - 240 + 80 = 120."""
    edges = [(0, 2, 40, 80), (0, 3, 40, 80), (1, 2, 40, 80), (1, 3, 40, 80)]
    r = reduction(SEQ120[:4], edges)
    fin, fout, rm = [([], 0)] * 4, [([], 0)] * 4, []
    fin[2], fin[3] = ([2, 0, 1], 5), ([3, 0, 1], 3)
    fout[0], fout[1] = ([0, 2, 3], 7), ([1, 2, 3], 9)
    r.find_components(fin, fout, rm)
    assert r.components == [([(0, 2), (0, 3), (1, 2), (1, 3)], 120)] and rm == []
    # overlaps of 100: dist1 = max(3, 120), dist2 = max(7, 120): 120 + 120 - 240 + 100 = 100
    r = reduction(SEQ120[:4], [(u, v, 20, 100) for u, v, _, _ in edges])
    r.find_components(fin, fout, rm)
    assert r.components[0][1] == 100


def test_trivial_out_branch_component():
    """Out-branch 0 -> 1, 0 -> 2 (overlap 100 at 20, reads of 120): dist1 = max(150, 120) = 150, dist2 = len2 = 120, dist = 150 + 120
    - 240 + 100 = 130."""
    r = reduction(SEQ120[:3], [(0, 1, 20, 100), (0, 2, 20, 100)])
    fout, rm = [([], 0)] * 3, []
    fout[0] = ([0, 1, 2], 150)
    r.find_components([([], 0)] * 3, fout, rm)
    assert r.components == [([(0, 1), (0, 2)], 130)]


def _two_components(careful):
    """Out-branch 0 -> {1, 2} and out-branch 2 -> {3, 4} share vertex 2; both have distance 100 + 120 - 240 + 120... = the table's
    key.  Map order of {0, 2}: 2, 0 (head insertion), so the component of 2 is component 0.  Evidence: every edge two unique ids."""
    edges = [(0, 1, 20, 100), (0, 2, 20, 100), (2, 3, 20, 100), (2, 4, 20, 100)]
    r = reduction(SEQ120[:5], edges, table={100: 2}, careful=careful)
    fout, rm = [([], 0)] * 5, []
    fout[0], fout[2] = ([0, 1, 2], 0), ([2, 3, 4], 0)
    r.find_components([([], 0)] * 5, fout, rm)
    assert [c for c, _ in r.components] == [[(2, 3), (2, 4)], [(0, 1), (0, 2)]] and {d for _, d in r.components} == {100}
    r.evidence = {(0, 1): [1, 2], (0, 2): [3, 4], (2, 3): [5, 6], (2, 4): [7, 8]}
    return r


def test_careful_removes_the_component_next_to_a_kept_one():
    """What run() does behind find_components, restated on the two components: with careful the second (vertex 2 is in both) is
    removed because the first was kept; without, both are kept."""
    for careful, want in ((True, [(0, 1), (0, 2)]), (False, [])):
        r = _two_components(careful)
        comps, r.components = r.components, []
        m = r.m
        r2 = B.Reduction(m, [True] * 5, r.originals, r.oseq, 5, 0, {100: 2}, careful, 0, 0.97)
        # run() from the components on: feed them through a subclass hook
        r2.find_components = lambda fi, fo, rm: r2.components.extend(comps)
        r2.branch_evidence = lambda *a: ([], 0)
        r2.evidence = r.evidence
        missing, removed = r2.run()
        assert removed == want and r2.stats["components_kept"] == (1 if careful else 2)
        assert r2.report[0] == "100\t2\t1\t2>3:2\t2>4:2\n"
        assert r2.report[1] == ("100\t2\t0\t0>1:-1\t0>2:-1\n" if careful else "100\t2\t1\t0>1:2\t0>2:2\n")


def test_a_distance_missing_from_the_table_removes_the_component():
    r = _two_components(False)
    comps = r.components
    r2 = B.Reduction(r.m, [True] * 5, r.originals, r.oseq, 5, 0, {99: 0}, False, 0, 0.97)
    r2.find_components = lambda fi, fo, rm: r2.components.extend(comps)
    r2.branch_evidence = lambda *a: ([], 0)
    r2.evidence = r.evidence
    _, removed = r2.run()
    assert removed == [(0, 1), (0, 2), (2, 3), (2, 4)] and r2.stats["dist_too_large"] == 2 and r2.report[0] == "100\t-1\t0\t2>3:-1\t2>4:-1\n"


def test_count_unique_evidence_counts_strictly_unique_minima():
    """Fronts 1 1 2: 1 is shared, dropped from both; then 2 (a), 2 (c): shared again...  a = [1, 2, 5], b = [1, 3], c = [2, 4]:
    turn 1 min 1 twice -> dropped; fronts 2 3 2 -> 2 twice, dropped; fronts 5 3 4 -> 3 unique (b); 5 4 -> 4 unique (c); 5 unique (a).
    Counts a 1, b 1, c 1; with min_evidence 1 all stay.  With 2 all go and the component is not kept."""
    comp = [(0, 1), (0, 2), (0, 3)]
    r = reduction(SEQ120[:4], [(0, 1, 20, 100), (0, 2, 20, 100), (0, 3, 20, 100)])
    r.evidence = {(0, 1): [1, 2, 5], (0, 2): [1, 3], (0, 3): [2, 4]}
    rm = []
    assert r.count_unique(comp, 1, rm) == (True, [1, 1, 1]) and rm == []
    r.evidence = {(0, 1): [1, 2, 5], (0, 2): [1, 3], (0, 3): [2, 4]}
    assert r.count_unique(comp, 2, rm) == (False, [1, 1, 1]) and rm == comp


def test_edges_to_remove_are_sorted_and_uniqued_behind_the_missing_edges():
    """A false out-branch 3 -> {1, 2} and a supported-by-nothing out-branch 0 -> {4, 5}: the false branch's edges enter
    edges_to_remove first, the list is sorted before removal: (0, 4), (0, 5), (3, 1), (3, 2); the missing edge comes in front."""
    seqs = ["A" * 12, "A" * 6, "A" * 6, "A" * 12, "AAAAAC", "AAAAAG"]
    r = reduction(seqs, [(0, 4, 6, 6), (0, 5, 6, 6), (3, 1, 6, 6), (3, 2, 6, 6)], table={k: 1 for k in range(300)},
                  originals=[{v: (True, 0, 6)} for v in range(6)])
    missing, removed = r.run()
    assert [(e["v1"], e["v2"]) for e in missing] == [(1, 2)] and removed == [(0, 4), (0, 5), (3, 1), (3, 2)]
    assert r.stats["components"] == 1 and r.stats["components_kept"] == 0 and r.stats["missing_edges"] == 1


# ---- the 3-clique rule -------------------------------------------------------------------------------------------------------
def test_transitive_removal_schedules_short_branches_in_both_removal_branches():
    """0 -> 1 -> 2 with 0 -> 2 transitive (length 50).  Scheduled: the out-edges of 0 and the in-edges of 2 no longer than 50 -
    0 -> 3 (40), 4 -> 2 (50), and 0 -> 2 itself; 0 -> 1 (60), 1 -> 2 (70), 5 -> 2 (51) stay."""
    edges = [(0, 1, 1, 60), (0, 2, 2, 50), (0, 3, 3, 40), (1, 2, 1, 70), (4, 2, 1, 50), (5, 2, 1, 51)]
    for branch in (True, False):
        m, stats, n = model(["A" * 80] * 6, edges), {}, []
        B.remove_transitive_scheduling(m, 1, stats, branch, n)
        assert [(u, e["v2"]) for u in range(6) for e in m.adj[u]] == [(0, 1), (1, 2), (5, 2)]
        assert stats["transitive"] == 1 and n == [3]


# ---- the container order -------------------------------------------------------------------------------------------------------
def test_unordered_map_order_by_hand():
    """13 buckets from the first insert.  0, 1, 2: each into an empty bucket, at the head: 2 1 0.  Then 13 shares bucket 0 with 0:
    head of that bucket's run: 2 1 13 0."""
    assert B.umap_order([0, 1, 2]) == [2, 1, 0] and B.umap_order([0, 1, 2, 13]) == [2, 1, 13, 0]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_unordered_map_order_against_the_compiler(tmp_path):
    src = tmp_path / "order.cpp"
    src.write_text("#include <cstdio>\n#include <cstdlib>\n#include <unordered_map>\n"
                   "int main(int argc, char **argv) { std::unordered_map<unsigned, int> m;\n"
                   "  for (int k = 1; k < argc; ++k) m.insert(std::make_pair((unsigned)strtoul(argv[k], 0, 10), 0));\n"
                   "  for (auto &p : m) printf(\"%u \", p.first); printf(\"\\n%zu\\n\", m.bucket_count()); }\n")
    exe = tmp_path / "order"
    subprocess.run(["g++", "-O1", "-o", str(exe), str(src)], check=True)
    import random
    rng = random.Random(5)
    key_sets = [list(range(n)) for n in (1, 13, 14, 29, 30, 59, 60, 127, 128)]          # across 13 -> 29 -> 59 -> 127 -> 257
    key_sets += [sorted(rng.sample(range(5000), n)) for n in (12, 14, 31, 61, 200)]     # ascending, as the reference inserts
    key_sets += [rng.sample(range(100000), 70), [13 * k for k in range(40)], [29 * k + 3 for k in range(35)]]
    for keys in key_sets:
        out = subprocess.run([str(exe)] + [str(k) for k in keys], check=True, capture_output=True, text=True).stdout.split("\n")
        assert [int(x) for x in out[0].split()] == B.umap_order(keys), keys


# ---- the table, the CLI, the symbols ---------------------------------------------------------------------------------------
def test_table_parsing(tmp_path):
    p = tmp_path / "t.tsv"
    p.write_text("# dist\tx\tmin_ev\n\n100\t0.5\t3\n 200\tq\t+4 trailing\n300\t1\t-1\n100\t9\t7\n")
    assert B.read_table(str(p)) == {100: 7, 200: 4, 300: -1}
    # one stringstream for all lines: "extra" behind the third tab goes in front of the next line, std::stoi("extra100") throws
    p.write_text("300\t1\t-1\textra\n100\t9\t7\n")
    with pytest.raises(ValueError):
        B.read_table(str(p))
    # ... and "5<TAB>6" makes the next line "5", "6100", "9", with "7" carried on to a comment-skipped line's successor
    p.write_text("300\t1\t-1\t5\t6\n100\t9\t7\n# skipped\n0\t1\t2\n")
    assert B.read_table(str(p)) == {300: -1, 5: 9, 70: 2}
    p.write_text("300\t1\t2\t\n100\t9\t7\n")                    # a trailing tab leaves nothing behind
    assert B.read_table(str(p)) == {300: 2, 100: 7}
    p.write_text("100\t1\tx\n")
    with pytest.raises(ValueError):
        B.read_table(str(p))
    p.write_text("100\n")                               # getline at the end of the stream keeps the last column read
    assert B.read_table(str(p)) == {100: 100}


def test_cli_refusals(tmp_path):
    base = [sys.executable, "-m", "hylight_amd.vq_branches", "--singles", "s", "--overlaps", "o", "--out", str(tmp_path), "--original_fastq",
            "f", "--branch_SE_c", "1", "--thresholds", "t"]
    for extra in (["--branch_reduction", "false"], ["--remove_trans", "2"], ["--remove_branches", "true"], ["--diploid", "true"],
                  ["--add_duplicates", "true"]):
        r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 4 and "is not built" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--first_it", "false"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "--subreads" in r.stderr
    r = subprocess.run(base[:-4], cwd=ROOT, capture_output=True, text=True)      # no --branch_SE_c, no --thresholds
    assert r.returncode == 2 and "required" in r.stderr
    # vq_graph and vq_cliques refuse the flag as before
    for mod in ("vq_graph", "vq_cliques"):
        r = subprocess.run([sys.executable, "-m", "hylight_amd." + mod, "--singles", "s", "--overlaps", "o", "--out", str(tmp_path),
                            "--branch_reduction", "true"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 4 and "--branch_reduction true" in r.stderr


def test_symbols_and_abi_version():
    from hylight_amd import api
    assert api.ABI_VERSION == 7
    assert len(api.SYMBOLS["hlmi_vq_branch_graph"][1]) == 10 and len(api.SYMBOLS["hlmi_vq_branch_iteration"][1]) == 14
    assert api.SYMBOLS["hlmi_vq_branch_opts_polyte"] == (None, [ctypes.POINTER(api.VqBranchOpts)])
    assert ctypes.sizeof(api.VqBranchOpts) == 12 and ctypes.sizeof(api.VqBranchStats) == 8 * 17
    assert api.VQ_BRANCH_STATS == B.STATS and callable(api.vq_branch_graph) and callable(api.vq_branch_iteration)
    header = open(os.path.join(ROOT, "include", "hylight_mi.h")).read()
    assert "#define HLMI_ABI_VERSION 7" in header
    for text in ("int hlmi_vq_branch_graph(", "int hlmi_vq_branch_iteration(", "void hlmi_vq_branch_opts_polyte(", "} hlmi_vq_branch_opts;",
                 "} hlmi_vq_branch_stats;"):
        assert text in header, text
    lib = os.path.join(ROOT, "hylight_amd", "libhylight_mi.so")
    if os.path.exists(lib):
        so = ctypes.CDLL(lib)
        for name in ("hlmi_vq_branch_graph", "hlmi_vq_branch_iteration", "hlmi_vq_branch_opts_polyte"):
            assert hasattr(so, name)
