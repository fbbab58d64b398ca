"""CPU: tests/vq_next_model.py held to lines worked out by hand from the reference's text (tools/HaploConduct/src/
FindNextOverlaps.cpp, cited per case), and the parts of the new interface that need no GPU: the bound symbols, the driver's
flag and the stopping rule of the stage-b loop (script/pipeline_per_stage.py:145-152).

The tables of every case: vertices 0, 1 unvisited (new ids 5 and 6, 100 and 120 bases), 2 in super-read 0 (300 bases) at
offset 50, 3 in super-read 1 (200 bases) at offset 0, 4 in super-read 0 at offset 0, 5 visited without a super-read (too
short / N rate / inclusion / tip, SRBuilder.cpp:1286-1311), 6 unvisited (new id 9) and 7 (new id 10), 8 in super-read 1 at
offset 20."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_next_model as N  # noqa: E402

ENT = [5, 6, 0, 1, 0, None, 9, 10, 1]
IN_SR = [False, False, True, True, True, False, False, False, True]
OFF = [0, 0, 50, 0, 0, 0, 0, 0, 20]
LENGTH = {0: 300, 1: 200, 5: 100, 6: 120, 9: 400, 10: 400}
ORIENT = [1, 1, 1, 0, 1, 1, 1, 1, 1]


def _next(**k):
    return N.Next(ENT, IN_SR, OFF, LENGTH, ORIENT, **k)


def _edge(u, v, pos1, score=2.0, **k):
    e = dict(v1=u, v2=v, pos1=pos1, pos2=0, ori1=True, ori2=True, ord="-", perc=80, len1=90, len2=0, score=score)
    e.update(k)
    return e


def _lines(nx):
    return nx.image().split("\n")[:-1]


def test_copied():
    """:47-72: both unvisited - the edge's own numbers under the new ids."""
    nx = _next()
    nx.update(_edge(0, 1, 10))
    assert _lines(nx) == ["5\t6\t10\t0\t-\t+\t+\t80\t0\t90\t0\ts\ts"] and nx.stats["copied"] == 1


def test_u_to_superread_negative_position():
    """:73-149 with :360-368: new_pos1 = 20 + 0 - 50 = -30 -> the super-read comes first at 30, len = 300; overlap
    min(270, 100, 300) = 100; max(100/100, 100/300) * 100 = 100."""
    nx = _next()
    nx.update(_edge(0, 2, 20))
    assert _lines(nx) == ["0\t5\t30\t0\t-\t+\t+\t100\t0\t100\t0\ts\ts"] and nx.stats["u2sr"] == 1


def test_superread_to_v_positive_position():
    """:151-227: new_pos1 = 200 + 50 - 0 = 250, len = 300; overlap min(50, 300, 120) = 50; max(50/300, 50/120) = 0.41666 -> 41."""
    nx = _next()
    nx.update(_edge(2, 1, 200))
    assert _lines(nx) == ["0\t6\t250\t0\t-\t+\t+\t41\t0\t50\t0\ts\ts"] and nx.stats["v2sr"] == 1


def test_superread_to_superread_and_zero_position():
    """:229-326: 100 + 50 - 0 = 150; min(150, 300, 200) = 150; max(0.5, 0.75) -> 75.  Then position zero: 30 + 20 - 50 = 0
    from super-read 1 (vertex 8) to super-read 0 (vertex 2): ord1 '1', min(200, 200, 300) = 200 -> 100 - but the key (0, 1)
    is taken (:261-273), so a fresh table shows it."""
    nx = _next()
    nx.update(_edge(2, 3, 100))
    assert _lines(nx) == ["0\t1\t150\t0\t-\t+\t+\t75\t0\t150\t0\ts\ts"] and nx.stats["sr2sr"] == 1
    nx.update(_edge(8, 2, 30))
    assert len(_lines(nx)) == 1
    nx = _next()
    nx.update(_edge(8, 2, 30))
    assert _lines(nx) == ["1\t0\t0\t0\t-\t+\t+\t100\t0\t200\t0\ts\ts"]
    assert N.overlap_data(30, 20, 50, 200, 300) == ("1", 0, 200, 100)


def test_last_position_and_failure():
    """:373-384: new_pos1 == len - 1 leaves one base; new_pos1 == len fails."""
    assert N.overlap_data(249, 50, 0, 300, 120) == ("1", 299, 1, 0)
    assert N.overlap_data(250, 50, 0, 300, 120) is None
    assert N.overlap_data(0, 0, 119, 100, 120) == ("2", 119, 1, 1)
    assert N.overlap_data(0, 0, 120, 100, 120) is None


def test_failed_owner_blocks_the_key():
    """:84-97 in front of :115-118: the first claimant fails, a later one that would succeed is dropped - no line."""
    nx = _next()
    nx.update(_edge(2, 1, 250))          # 250 + 50 = 300 >= 300: failure, key (0, 6) taken
    nx.update(_edge(2, 1, 200))
    assert _lines(nx) == [] and nx.stats["claims_failed"] == 1 and nx.stats["v2sr"] == 0


def test_first_source_owns_the_key():
    """One key from four source edges with different positions: the first wins (:612-629, then :697, then :878)."""
    sources = [_edge(2, 3, 100), _edge(4, 3, 120), _edge(2, 8, 140, score=0), _edge(4, 8, 160, score=1.0)]
    want = ["0\t1\t150\t0\t-\t+\t+\t75\t0\t150\t0\ts\ts", "0\t1\t120\t0\t-\t+\t+\t90\t0\t180\t0\ts\ts",
            "0\t1\t170\t0\t-\t+\t+\t65\t0\t130\t0\ts\ts", "0\t1\t140\t0\t-\t+\t+\t80\t0\t160\t0\ts\ts"]
    for k in range(4):
        nx = _next()
        for e in sources[k:]:
            nx.update(e)
        assert _lines(nx) == [want[k]], k


def test_same_superread_is_skipped_before_the_claim():
    """:255: vertices 2 and 4 are both in super-read 0."""
    nx = _next()
    nx.update(_edge(2, 4, 10))
    assert _lines(nx) == [] and not nx.found


def test_visited_without_superread():
    """SRBuilder.cpp:1286-1311 marks vertex 5 visited; nodes_to_SR.at(5) is empty, so no loop turn and no claim."""
    nx = _next()
    for e in (_edge(0, 5, 10), _edge(5, 0, 10), _edge(2, 5, 10), _edge(5, 2, 10)):
        nx.update(e)
    assert _lines(nx) == [] and not nx.found


def test_minus_orientation_on_a_nonedge_row():
    """:34-37: score 0 - '+' where the row's orientation equals the label; vertex 3 is labelled reverse."""
    nx = _next()
    nx.update(_edge(0, 1, 10, score=0, ori1=False, ori2=True))
    nx.update(_edge(2, 3, 100, score=0, ori1=True, ori2=True))
    assert _lines(nx) == ["0\t1\t150\t0\t-\t+\t-\t75\t0\t150\t0\ts\ts", "5\t6\t10\t0\t-\t-\t+\t80\t0\t90\t0\ts\ts"]
    nx = _next()
    nx.update(_edge(2, 3, 100, score=2.0, ori1=False, ori2=True))          # an edge: '+' whatever it holds (:38-41)
    assert _lines(nx)[0].split("\t")[5:7] == ["+", "+"]


def test_percentage_100_and_no_inclusion_overlaps():
    """:68, :145: left out only with the option."""
    for opt, n in ((0, 2), (1, 0)):
        nx = _next(no_inclusion_overlaps=opt)
        nx.update(_edge(0, 1, 10, perc=100))
        nx.update(_edge(0, 2, 20))
        assert len(_lines(nx)) == n


def test_line_order_is_byte_order():
    """std::set<std::string>: TAB < digit, so 1<TAB> < 10<TAB> < 9<TAB>, and 99 / 100 likewise."""
    ent = [1, 9, 10, 99, 100, 2]
    nx = N.Next(ent, [False] * 6, [0] * 6, {}, [1] * 6)
    for u in range(5):
        nx.update(_edge(u, 5, 10))
    assert [l.split("\t")[0] for l in _lines(nx)] == ["1", "10", "100", "9", "99"]


def test_two_sources_one_line():
    nx = _next()
    nx.update(_edge(0, 1, 10))
    nx.update(_edge(0, 1, 10))
    assert len(_lines(nx)) == 1 and nx.stats["copied"] == 2 and nx.stats["lines"] == 1


def test_percentage_is_single_precision():
    """:375: float division, float product, floor - numpy.float32 step by step; 29 of 100 is 28 in exact-then-rounded
    double arithmetic only if the product were not rounded to float first."""
    for ol, ln in ((29, 100), (57, 100), (1, 3), (599, 600), (7, 25)):
        f = np.float32(ol) / np.float32(ln)
        assert N.overlap_data(0, 0, 0, ln, ol)[3] == 100
        assert N.overlap_data(ln - ol, 0, 0, ln, 10 ** 6)[3] == int(np.floor(f * np.float32(100)))


def test_induced_edges():
    """:841-875: out-edge 1 -> 2 and in-edge 0 -> 1 of included vertex 1 chain to 0 -> 2; len = min(|r0| - pos1, |r2|),
    perc = 100 * len / min(|r0|, |r2|) in integers."""
    seqs = ["A" * 500, "A" * 100, "A" * 300]
    lst = [_edge(1, 2, 40), _edge(0, 1, 250)]
    got = N.induced_edges([lst], seqs, 1.0)
    assert len(got) == 1 and (got[0]["v1"], got[0]["v2"], got[0]["pos1"], got[0]["len1"], got[0]["perc"]) == (0, 2, 250, 250, 83)
    assert N.induced_edges([[_edge(1, 2, 40), _edge(1, 3, 40)]], seqs + ["A"], 1.0) == []      # :841 same source


def test_symbols_and_abi():
    from hylight_amd import api
    assert api.ABI_VERSION == 7
    assert "hlmi_vq_iteration" in api.SYMBOLS and "hlmi_vq_next_opts_stageb" in api.SYMBOLS
    assert len(api.SYMBOLS["hlmi_vq_iteration"][1]) == 10


def test_driver_accepts_stageb_native():
    from hylight_amd import driver
    p = driver.build_parser()
    assert p.parse_args(["-l", "x.fq", "--stageb_native"]).stageb_native is True
    assert p.parse_args(["-l", "x.fq"]).stageb_native is False


@pytest.mark.parametrize("counts,runs", [
    ([(10, 5, 3), (8, 4, 2), (8, 4, 2), (8, 4, 2), (7, 1, 1)], 4),      # unchanged twice in a row: stop after the fourth
    ([(10, 0, 3), (8, 4, 2)], 1),                                       # no overlap line
    ([(10, 5, 0), (8, 4, 2)], 1),                                       # graph.txt holds its two header lines only
    ([(10, 5, -2), (8, 4, 2)], 1),                                      # no graph.txt
    ([(10, 5, 3), (10, 5, 3), (9, 5, 3), (9, 5, 3), (9, 0, 3)], 5),     # a change resets the count
])
def test_stopping_rule(counts, runs):
    from hylight_amd import vq_stageb
    reads, ovs, edges = vq_stageb.loop(lambda k: counts[k])
    assert len(reads) == runs and list(zip(reads, ovs, edges)) == counts[:runs]
