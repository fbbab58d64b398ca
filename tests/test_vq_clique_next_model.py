"""CPU: tests/vq_clique_next_model.py held to lines worked out by hand from the reference's text (tools/HaploConduct/src/
FindNextOverlaps.cpp, cited per case), to vq_next_model.Next where every list holds one entry at the most, and the parts of
the new interface that need no GPU.

The tables of every case.  New reads: super-reads 0 (300 bases), 1 (200), 2 (250); copied reads 5 (100 bases) and 6 (120).
Vertices: 0 unvisited, copied as 5;  1 in super-reads 0 at index 50, 1 at 0 and 2 at -10;  2 in 0 at 10 and 1 at 0;  3 in 1 at
40 and 2 at 5;  4 in 1 at 0;  5 unvisited, copied as 6;  7 in 1 at 190;  8 in 1 at 0;  9 in 2 at -15 (it starts 15 columns in
front of trim_pos);  10 visited with an empty list (too short / N rate, SRBuilder.cpp:1149-1160);  6 likewise."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vq_next_model as T  # noqa: E402
import vq_clique_next_model as CN  # noqa: E402
import vq_next_model as N  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = [[(5, 0)], [(0, 50), (1, 0), (2, -10)], [(0, 10), (1, 0)], [(1, 40), (2, 5)], [(1, 0)], [(6, 0)], [], [(1, 190)], [(1, 0)],
         [(2, -15)], []]
COPIED = [True, False, False, False, False, True, False, False, False, False, False]
LENGTH = {0: 300, 1: 200, 2: 250, 5: 100, 6: 120}
ORIENT = [1] * 11
TAIL = "\t0\t-\t+\t+\t"
_edge = T._edge


def _next(**k):
    return CN.CliqueNext(LISTS, COPIED, LENGTH, ORIENT, **k)


def _lines(nx):
    return nx.image().split("\n")[:-1]


def _line(a, b, pos, perc, ol):
    return f"{a}\t{b}\t{pos}{TAIL}{perc}\t0\t{ol}\t0\ts\ts"


# edge 0 -> 1 at 20, u unvisited (:73-150), one turn per super-read of vertex 1 in ascending id:
#   0: 20 + 0 - 50 = -30 -> the super-read first at 30, len 300; min(270, 100, 300) = 100; max(100/100, 100/300) -> 100
#   1: 20 + 0 - 0 = 20, len 100; min(80, 100, 200) = 80; max(80/100, 80/200) = 0.8f, 0.8f * 100 = 80.000001.. -> 80
#   2: 20 + 0 - (-10) = 30, len 100; min(70, 100, 250) = 70; max(0.7f, 0.28f) * 100 rounds to 70.0f -> 70
THREE = [_line(0, 5, 30, 100, 100), _line(5, 1, 20, 80, 80), _line(5, 2, 30, 70, 70)]


def test_one_vertex_in_three_superreads_against_an_unvisited_neighbour():
    nx = _next()
    nx.update(_edge(0, 1, 20))
    assert _lines(nx) == sorted(THREE)
    assert (nx.stats["u2sr"], nx.stats["candidates"], nx.max_turns, nx.min_idx) == (3, 3, 3, -10)
    assert nx.found == {(0, 5), (1, 5), (2, 5)} and nx.stats["max_list"] == 3 and nx.stats["in_several"] == 3
    # the same vertex on the other side (:151-228): 1 -> 5 at 20, the list of u; 20 + 50 = 70 of 300: min(230, 300, 120) = 120
    # -> 100; 20 + 0 = 20 of 200: min(180, 200, 120) = 120 -> 100; 20 - 10 = 10 of 250: 120 -> 100
    nx = _next()
    nx.update(_edge(1, 5, 20))
    assert _lines(nx) == sorted([_line(0, 6, 70, 100, 120), _line(1, 6, 20, 100, 120), _line(2, 6, 10, 100, 120)])
    assert nx.stats["v2sr"] == 3


def test_shared_superread_is_skipped_before_the_claim():
    """:229-326, edge 2 -> 3 at 30: u's list outer, v's inner: (0, 1), (0, 2), (1, 1) skipped at :255, (1, 2).
    (0, 1): 30 + 10 - 40 = 0, len 300; min(300, 300, 200) = 200; max(200/300, 200/200) -> 100
    (0, 2): 30 + 10 - 5 = 35; min(265, 300, 250) = 250 -> 100
    (1, 2): 30 + 0 - 5 = 25, len 200; min(175, 200, 250) = 175; max(0.875, 0.7) -> 87"""
    nx = _next()
    nx.update(_edge(2, 3, 30))
    assert _lines(nx) == [_line(0, 1, 0, 100, 200), _line(0, 2, 35, 100, 250), _line(1, 2, 25, 87, 175)]
    assert nx.found == {(0, 1), (0, 2), (1, 2)} and nx.stats["candidates"] == 3 and nx.stats["sr2sr"] == 3
    assert nx.wide_sr2sr == 3 and nx.max_turns == 4 and nx.late_owners == 2


def test_a_later_turn_meets_a_key_an_earlier_edge_owns():
    """Edge 0 -> 4 at 10 claims (1, 5): 10 of 100, min(90, 100, 200) = 90, 0.9f * 100 rounds to 90.0f -> 90.  The second turn
    of edge 0 -> 1 then finds the key taken (:90-92); its first and third turn own theirs."""
    nx = _next()
    nx.update(_edge(0, 4, 10))
    nx.update(_edge(0, 1, 20))
    assert _lines(nx) == sorted([THREE[0], THREE[2], _line(5, 1, 10, 90, 90)])
    assert nx.stats["u2sr"] == 3 and nx.stats["candidates"] == 4 and nx.late_owners == 1


def test_failed_owner_blocks_a_turn_that_would_succeed():
    """:162-175 in front of :193-196: 7 -> 0 at 20 claims (1, 5) and fails, 20 + 190 - 0 = 210 >= 200; 8 -> 0 at 10 would give
    10 + 0 - 0 = 10 of 200, but the key is taken: no line.  Alone it does."""
    nx = _next()
    nx.update(_edge(7, 0, 20))
    nx.update(_edge(8, 0, 10))
    assert _lines(nx) == [] and nx.stats["claims_failed"] == 1 and nx.stats["v2sr"] == 0 and nx.stats["candidates"] == 2
    nx = _next()
    nx.update(_edge(8, 0, 10))
    assert _lines(nx) == [_line(1, 5, 10, 100, 100)]             # min(190, 200, 100) = 100 -> 100


def test_negative_index_under_error_correction():
    """findCliqueIndex = index1 - startpos1 = 0 - 15 for a read that starts in front of trim_pos (:337): 9 -> 0 at 5 gives
    5 + (-15) - 0 = -10 -> the copied read first at 10, len 100; min(90, 250, 100) = 90; max(90/250, 90/100) -> 90.  An
    unsigned index would have made it 2^32 - 10."""
    nx = _next()
    nx.update(_edge(9, 0, 5))
    assert _lines(nx) == [_line(5, 2, 10, 90, 90)] and nx.stats["v2sr"] == 1 and nx.min_idx == -15


def test_an_empty_list_on_one_side():
    """SRBuilder.cpp:1149-1160 marks the vertex visited, nodes_to_SR holds nothing for it: every branch loops over nothing."""
    nx = _next()
    for e in (_edge(0, 10, 10), _edge(10, 0, 10), _edge(1, 10, 10), _edge(10, 1, 10), _edge(6, 10, 10)):
        nx.update(e)
    assert _lines(nx) == [] and not nx.found and nx.stats["candidates"] == 0


def test_percentage_100_and_no_inclusion_overlaps():
    nx = _next(no_inclusion_overlaps=1)
    nx.update(_edge(0, 1, 20))
    nx.update(_edge(0, 5, 3, perc=100))
    assert _lines(nx) == sorted(THREE[1:]) and nx.stats["u2sr"] == 2 and nx.stats["copied"] == 0 and nx.stats["candidates"] == 3


def test_lists_of_one_entry_are_vq_next_model():
    """With lists of at most one entry the model is vq_next_model.Next, line for line and stat for stat, on that model's own
    tables and source edges (tests/test_vq_next_model.py), in both orders and with the inclusion option."""
    e = T._edge
    edges = [e(0, 1, 10), e(0, 2, 20), e(2, 1, 200), e(2, 3, 100), e(8, 2, 30), e(2, 1, 250), e(4, 3, 120), e(2, 8, 140, score=0),
             e(4, 8, 160, score=1.0), e(2, 4, 10), e(0, 5, 10), e(5, 0, 10), e(2, 5, 10), e(5, 2, 10),
             e(0, 1, 10, score=0, ori1=False, ori2=True), e(2, 3, 100, score=0), e(0, 1, 10, perc=100), e(6, 7, 5), e(7, 8, 390),
             e(3, 6, 199), e(3, 6, 200)]
    for order in (edges, edges[::-1], edges[7:] + edges[:7]):
        for opt in (0, 1):
            a = N.Next(T.ENT, T.IN_SR, T.OFF, T.LENGTH, T.ORIENT, no_inclusion_overlaps=opt)
            b = CN.from_next_tables(T.ENT, T.IN_SR, T.OFF, T.LENGTH, T.ORIENT, no_inclusion_overlaps=opt)
            for x in order:
                a.update(x)
                b.update(x)
            assert a.image() == b.image() and a.lines
            assert {k: b.stats[k] for k in N.STATS} == a.stats and a.found == b.found
            assert b.stats["max_list"] == 1 and b.stats["in_several"] == 0 and b.late_owners == 0


def test_tables_from_clique_map():
    """clique_map.txt -> the lists, in ascending super-read id; the vertices in none: copied from the super-read count on,
    unless too short (keep_singletons) or failing the N rate."""
    seqs = ["A" * 100, "A" * 100, "A" * 100, "A" * 40, "N" * 100, "A" * 100]
    text = "0\t7\t0:-7:+\t1:3:+\n1\t0\t1:0:+\t2:12:-\n"
    lists, copied, count = CN.tables(text, seqs, 50)
    assert lists == [[(0, -7)], [(0, 3), (1, 0)], [(1, 12)], [], [], [(2, 0)]]
    assert copied == [False, False, False, False, False, True] and count == 3


def test_symbols_and_abi():
    from hylight_amd import api
    assert api.ABI_VERSION == 7
    assert len(api.SYMBOLS["hlmi_vq_clique_iteration"][1]) == 10 and len(api.SYMBOLS["hlmi_vq_iteration"][1]) == 10
    assert api.VQ_CLIQUE_NEXT_STATS == api.VQ_NEXT_STATS + ("candidates", "max_list", "in_several")
    import ctypes
    assert ctypes.sizeof(api.VqCliqueNextStats) == 8 * 15 and callable(api.vq_clique_iteration)
    header = open(os.path.join(ROOT, "include", "hylight_mi.h")).read()
    assert re.search(r"#define\s+HLMI_ABI_VERSION\s+7\b", header)
    assert "int hlmi_vq_clique_iteration(" in header and "} hlmi_vq_clique_next_stats;" in header


def test_cli_has_the_iteration_switch():
    from hylight_amd import vq_cliques
    p = vq_cliques.build_parser()
    base = ["--singles", "s", "--overlaps", "o", "--out", "d"]
    assert p.parse_args(base).iteration is False and p.parse_args(base + ["--iteration"]).iteration is True
