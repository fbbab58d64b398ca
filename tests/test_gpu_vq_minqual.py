"""GPU: --min_qual through the hlmi_vq_*_mq calls against the models of tests/vq_*_model.py with their MIN_QUAL set
(tests/vq_minqual_helper.py), byte for byte; tests/test_vq_minqual_model.py holds the model at minQual 0 to hand-worked answers.
What an input has to reach is asserted from the model, never from the library."""
import math
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_branch_model as B  # noqa: E402
import vq_clique_cases as K  # noqa: E402
import vq_clique_model as CM  # noqa: E402
import vq_clique_next_model as CN  # noqa: E402
import vq_graph_model as M  # noqa: E402
import vq_merge_model as MM  # noqa: E402
import vq_minqual_helper as H  # noqa: E402
import test_gpu_vq_branch as TB  # noqa: E402
import test_gpu_vq_clique_next as TN  # noqa: E402
from test_gpu_vq_merge import _all_cases, _kernel_constants  # noqa: E402

pytestmark = pytest.mark.gpu
cluster = TN.cluster                             # the smallest simulated cluster of the clique-iteration tests (a fixture)
generated = TB.generated                         # ... of the branch-iteration test
BAD = (-0.1, 1.1, math.nan)


def _files(d, names):
    return {n: open(os.path.join(d, n), "rb").read() for n in names if os.path.exists(os.path.join(d, n))}


def _same_files(lib_dir, model_dir, names):
    got, want = _files(lib_dir, names), _files(model_dir, names)
    assert sorted(got) == sorted(want)
    for n in want:
        assert got[n] == want[n], n
    return got


# ---- 1: the pair ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def all_pairs():
    """Every (base1, q1, base2, q2) as two sequences of 220 900 positions, and the model's answers at minQual 0, once."""
    s1, q1, s2, q2 = _all_cases()
    with H.model_min_qual(0.0):
        want = {pos: MM.consensus_pair(s1, q1, s2, q2, pos) for pos in (0, 1000)}
    return (s1, q1, s2, q2), want


@pytest.mark.parametrize("pos", [0, 1000])
def test_pair_every_base_and_quality_at_0(all_pairs, pos):
    from hylight_amd import api
    (s1, q1, s2, q2), want = all_pairs
    got = api.vq_consensus_pair(s1, q1, s2, q2, pos, min_qual=0.0)
    assert len(got[0]) == 220900 + pos and got == want[pos]
    if pos == 0:
        two = [k for k in range(220900) if s1[k] != "N" and s2[k] != "N"]
        assert not any(got[0][k] == "N" for k in two)             # never an N where two bases were read
        # a base that was not read: two different bases in the four cells of Q0 / Q1 (12 ordered pairs each), twice one base
        # at Q0 against anything and at Q1 against Q1 (188 cells, 4 bases each) - tests/test_vq_minqual_model.py
        assert sum(got[0][k] not in (s1[k], s2[k]) for k in two) == 12 * 4 + 4 * 188


def test_pair_ties_at_the_layout_borders():
    """The overlap holds nothing but two different bases of equal quality - code 3 on every lane, the last lane of a wave and the
    first of the next among them - and is 63 / 64 / 65, 255 / 256 / 257, span - 1 / span / span + 1 positions long, from output
    position 0 and from 10."""
    from hylight_amd import api
    Kc = _kernel_constants()
    rng = random.Random(5)
    pairs = [(a, b) for a in "ACGT" for b in "ACGT" if a != b]
    with H.model_min_qual(0.0):
        for n in (Kc["WAVE"] - 1, Kc["WAVE"], Kc["WAVE"] + 1, Kc["WG"] - 1, Kc["WG"], Kc["WG"] + 1, Kc["SPAN"] - 1, Kc["SPAN"], Kc["SPAN"] + 1):
            for pos in (0, 10):
                ov = [pairs[(k + n) % 12] for k in range(n)]
                q = "".join(chr(33 + rng.choice((2, 20, 40, 93))) for _ in range(n))
                head = "".join(rng.choice("ACGT") for _ in range(pos))
                s1, q1 = head + "".join(a for a, _ in ov), "I" * pos + q
                s2, q2 = "".join(b for _, b in ov) + "ACGTA", q + "IIIII"
                got = api.vq_consensus_pair(s1, q1, s2, q2, pos, min_qual=0.0)
                assert got == MM.consensus_pair(s1, q1, s2, q2, pos), (n, pos)
                assert got[0][pos:pos + n] == "".join(min(p, key=H.ATCG.index) for p in ov), (n, pos)


# ---- 2: 0.9 through the new symbols is the old path --------------------------------------------------------------------------------
def test_the_default_through_the_new_symbols(tmp_path):
    from hylight_amd import api
    s1, q1, s2, q2 = _all_cases()
    for pos in (0, 1000):
        assert api.vq_consensus_pair(s1, q1, s2, q2, pos, min_qual=0.9) == api.vq_consensus_pair(s1, q1, s2, q2, pos)
    fq, ov, _ = K.write_files(tmp_path, K.case_pairs())
    opts = dict(K.HAND_GRAPH, first_it=True, keep_singletons=0, store_tips_separately=False, min_clique_size=2)
    old = api.vq_merge(fq, ov, str(tmp_path / "old"), **opts)
    new = api.vq_merge(fq, ov, str(tmp_path / "new"), min_qual=0.9, **opts)
    names = M.OUTPUTS + MM.OUTPUTS
    assert _files(str(tmp_path / "old"), names) == _files(str(tmp_path / "new"), names) and "singles.fastq" in _files(str(tmp_path / "new"), names)
    assert old[0] == new[0] and {k: old[1][k] for k in MM.STATS} == {k: new[1][k] for k in MM.STATS}
    assert new[1]["dropped_n"] == 1 and new[1]["merged"] == 3


# ---- 3: the merge ------------------------------------------------------------------------------------------------------------------
def disagreeing_pairs():
    """Three disjoint edges; one column in seven of every overlap (more than 5 % of the super-read) holds two different bases at
    equal quality.  1 -> 0 is stored from the higher vertex, 3 is stored reverse-complemented."""
    rng = random.Random(21)
    g = ["".join(rng.choices("ACGT", k=260)) for _ in range(3)]

    def other(s, lo, hi):
        s = list(s)
        for c in range(lo, hi, 7):
            s[c] = "ACGT"[("ACGT".index(s[c]) + 1 + c % 3) % 4]
        return "".join(s)

    reads = [(g[0][60:260], K.Q * 200, True), (other(g[0][0:170], 60, 170), K.Q * 170, True),
             (g[1][0:160], K.Q * 160, True), (K.rc(other(g[1][50:230], 0, 110)), K.Q * 180, False),
             (g[2][0:150], K.Q * 150, True), (other(g[2][40:200], 0, 110), K.Q * 160, True)]
    return dict(reads=reads, edges=[(1, 0, 60), (2, 3, 50), (4, 5, 40)], opts=dict(min_clique_size=2))


def test_merge_keeps_what_the_default_drops(tmp_path):
    from hylight_amd import api
    fq, ov, _ = K.write_files(tmp_path, disagreeing_pairs())
    opts = dict(K.HAND_GRAPH, first_it=True, keep_singletons=0, store_tips_separately=False, min_clique_size=2)
    ggot, mgot = api.vq_merge(fq, ov, str(tmp_path / "lib"), min_qual=0.0, **opts)
    with H.model_min_qual(0.0):
        gwant, mwant = MM.merge(fq, ov, str(tmp_path / "model"), **opts)
    files = _same_files(str(tmp_path / "lib"), str(tmp_path / "model"), M.OUTPUTS + MM.OUTPUTS)
    assert ggot == gwant and {k: mgot[k] for k in MM.STATS} == mwant
    assert mwant["pairs"] == mwant["merged"] == 3 and mgot["dropped_n"] == 0 and b"N" not in files["singles.fastq"]
    _, dropped = api.vq_merge(fq, ov, str(tmp_path / "default"), **opts)
    assert dropped["dropped_n"] == 3 and dropped["merged"] == 0           # the same input at 0.9: the input has not gone stale


# ---- 4: the cliques -----------------------------------------------------------------------------------------------------------------
def pile_case():
    """Four reads of 150 bases at 0, 40, 100 and 110 of one genome, every pair an edge: 260 columns, the tile border at 64 inside.
    Read 1 is stored reverse-complemented.  Depth 2 in [40, 100) and [190, 250), 3 in [100, 110) and [150, 190), 4 in [110, 150).
      63, 64   read 1 differs from read 0, both Q40: a two-read tie on the last lane of a tile and the first of the next
      105      reads 0 and 1 agree at Q10, read 2 differs at Q20: 0.9 * 0.9 * 0.01 / 3 against (0.1 / 3)^2 * 0.99 - the best
               base is 71 % sure: N at 0.9, the base at 0
      120      reads 0, 1 against reads 2, 3, all Q40: a tie of two bases in a column of four (the chain in decide())
      130      all four N
      160      reads 1, 2 agree at Q10, read 3 differs at Q20 (the same vote in the part error correction writes)"""
    rng = random.Random(9)
    g = "".join(rng.choices("ACGT", k=260))
    off = [0, 40, 100, 110]
    seq = [list(g[o:o + 150]) for o in off]
    qual = [list(K.Q * 150) for _ in off]
    nxt = lambda b, k=1: "ACGT"[("ACGT".index(b) + k) % 4]
    for c in (63, 64):
        seq[1][c - 40] = nxt(g[c])
    for c, agree, differ in ((105, (0, 1), 2), (160, (1, 2), 3)):
        for r in agree:
            qual[r][c - off[r]] = "+"
        seq[differ][c - off[differ]] = nxt(g[c], 2)
        qual[differ][c - off[differ]] = "5"
    for r in (2, 3):
        seq[r][120 - off[r]] = nxt(g[120], 3)
    for r in range(4):
        seq[r][130 - off[r]] = "N"
    reads = [("".join(seq[r]), "".join(qual[r]), True) for r in range(4)]
    reads[1] = (K.rc(reads[1][0]), reads[1][1][::-1], False)
    edges = [(i, j, off[j] - off[i]) for i in range(4) for j in range(i + 1, 4)]
    return dict(reads=reads, edges=edges, offsets=off, opts={})


POLYTE = dict(min_overlap_len=30, edge_threshold=0.9, remove_tips=False, ignore_inclusions=False, merge_contigs=1.0)
PILE_RUNS = dict(ec=dict(POLYTE, error_correction=True, min_clique_size=3, remove_trans=2, remove_branches=False, remove_backedges=False,
                         keep_singletons=0),
                 no_ec=dict(POLYTE, error_correction=False, min_clique_size=2, remove_trans=1, remove_branches=True, remove_backedges=True,
                            keep_singletons=0),
                 whole=dict(K.HAND_GRAPH, error_correction=False, min_clique_size=2, keep_singletons=0))


def test_pile_case_stays_under_the_host_cap():
    """On the CPU, with the margins of decide() in Python's libm: of the 130 columns of three reads and more only the all-N
    column is handed back, at either minQual - far under half."""
    cols = H.pile_columns(pile_case())
    assert len(cols) == 260 and [len(cols[c][0]) for c in (39, 40, 63, 64, 99, 100, 110, 149, 150, 189, 190, 250)] == [1, 2, 2, 2, 2, 3, 4, 4, 3, 3, 2, 1]
    deep = [c for c in range(260) if len(cols[c][0]) >= 3]
    for mq in (0.0, 0.9):
        back = [c for c in deep if H.goes_to_host(*cols[c], mq)]
        assert back == [130], (mq, back)
    assert len(deep) == 90
    with H.model_min_qual(0.0):
        at0 = [MM.consensus_pos(*cols[c])[0] for c in (63, 64, 105, 120, 130, 160)]
    at9 = [MM.consensus_pos(*cols[c])[0] for c in (63, 64, 105, 120, 130, 160)]
    assert at9 == ["N"] * 6 and "N" not in at0[:4] and at0[4] == "N" and at0[5] != "N"
    assert at0[3] == min(set(cols[120][0]), key=H.ATCG.index)


@pytest.mark.parametrize("name", sorted(PILE_RUNS))
def test_hand_built_piles(tmp_path, name):
    """ec: POLYTE's options with error correction (min_clique_size 3, remove_trans 2); no_ec: without (min_clique_size 2,
    remove_trans 1); whole: the graph as the rows give it, the four reads one pile of 260 columns without error correction."""
    from hylight_amd import api
    opts = PILE_RUNS[name]
    fq, ov, _ = K.write_files(tmp_path, pile_case())
    lib_dir, model_dir = str(tmp_path / "lib"), str(tmp_path / "model")
    ggot, cgot = api.vq_cliques(fq, ov, lib_dir, min_qual=0.0, **opts)
    with H.model_min_qual(0.0):
        gwant, cwant = CM.cliques(fq, ov, model_dir, api.vq_cliques_of_graph, **opts)
    _same_files(lib_dir, model_dir, M.OUTPUTS + CM.OUTPUTS)
    print(name, cgot, cwant)
    assert ggot == gwant and {k: cgot[k] for k in CM.STATS} == {k: cwant[k] for k in CM.STATS}
    assert cwant["superreads"] >= 1 and cwant["dropped_n"] == 0
    assert 2 * cgot["columns_host"] < cgot["columns"]                  # a kernel that hands everything back cannot pass
    records = open(os.path.join(model_dir, "singles.fastq")).read().split("\n")[1::4]
    if name == "whole":                                                # what the input is for, from the model's own output
        assert cwant["deep"] == 90 and len(records[0]) == 260 and records[0].count("N") == 1 and records[0][130] == "N"
    if name == "ec":
        assert cwant["deep"] > 0
    api.vq_cliques(fq, ov, str(tmp_path / "default"), **opts)           # the same input at 0.9 writes more N: it has not gone stale
    assert open(tmp_path / "default" / "singles.fastq").read().count("N") > open(tmp_path / "lib" / "singles.fastq").read().count("N")


# ---- 5: the iterations ---------------------------------------------------------------------------------------------------------------
def test_clique_iteration_at_0(tmp_path, cluster):
    from hylight_amd import api
    fq, ov, scores = cluster
    assert "N" not in "".join(open(fq).read().split("\n")[1::4])
    lib_dir, model_dir = str(tmp_path / "lib"), str(tmp_path / "model")
    got = api.vq_clique_iteration(fq, ov, lib_dir, min_qual=0.0, **TN.NO_EC)
    with H.model_min_qual(0.0):
        want = CN.clique_iteration(fq, ov, model_dir, api.vq_cliques_of_graph, scores=scores, **TN.NO_EC)
    TN._same(lib_dir, model_dir, got, want)
    assert got[1]["superreads"] > 0 and got[1]["dropped_n"] == 0 and got[2]["lines"] > 0
    assert "N" not in "".join(open(os.path.join(lib_dir, "singles.fastq")).read().split("\n")[1::4])


def test_branch_iteration_at_0(tmp_path, generated):
    from hylight_amd import api
    fq, ov, sub, ofq, tab, n, scores = generated
    assert "N" not in "".join(open(fq).read().split("\n")[1::4])
    lib_dir, model_dir = str(tmp_path / "lib"), str(tmp_path / "model")
    with H.model_min_qual(0.0):
        with B.Hook(ofq, n, 0, tab, True, False, sub, TB.GEN["min_overlap_len"], TB.GEN["edge_threshold"]) as h:
            want = CN.clique_iteration(fq, ov, model_dir, api.vq_cliques_of_graph, subreads_in=sub, scores=scores, **TB.GEN, **TB.CLIQUE)
    with open(os.path.join(model_dir, "branch_components.txt"), "w", newline="") as f:
        f.write("".join(h.report))
    got = api.vq_branch_iteration(fq, ov, ofq, tab, lib_dir, subreads_in=sub, se_count=n, pe_count=0, careful=True, min_qual=0.0,
                                  **TB.GEN, **TB.CLIQUE)
    _same_files(lib_dir, model_dir, TB.NAMES + CM.OUTPUTS + ("overlaps.txt", "stats.txt"))
    assert got[0] == want[0] and {k: got[1][k] for k in B.STATS} == h.stats
    assert {k: got[2][k] for k in CM.STATS} == {k: want[1][k] for k in CM.STATS} and {k: got[3][k] for k in CN.STATS} == want[2]
    assert got[2]["superreads"] > 0 and got[2]["dropped_n"] == 0
    assert "N" not in "".join(open(os.path.join(lib_dir, "singles.fastq")).read().split("\n")[1::4])


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", BAD, ids=["below", "above", "nan"])
def test_a_bad_min_qual_is_refused_before_any_output(tmp_path, bad):
    from hylight_amd import api
    fq, ov, _ = K.write_files(tmp_path, K.case_pairs())
    reads, rows = TB.out_branch(70, [10])
    bfq, bov, bofq, _, btab = TB.write_case(str(tmp_path / "in"), reads, rows, table={100: 0})
    out = str(tmp_path / "out")
    calls = (lambda: api.vq_merge(fq, ov, out, min_qual=bad, **K.HAND_GRAPH),
             lambda: api.vq_iteration(fq, ov, out, min_qual=bad, **K.HAND_GRAPH),
             lambda: api.vq_cliques(fq, ov, out, min_qual=bad, **K.HAND_GRAPH),
             lambda: api.vq_clique_iteration(fq, ov, out, min_qual=bad, **K.HAND_GRAPH),
             lambda: api.vq_branch_iteration(bfq, bov, bofq, btab, out, se_count=3, pe_count=0, min_qual=bad, **TB.HAND),
             lambda: api.vq_consensus_pair("ACGT", "IIII", "CGTA", "IIII", 1, min_qual=bad))
    for call in calls:
        with pytest.raises(api.HlmiError) as e:
            call()
        assert e.value.code == -1 and os.listdir(out) == [], e.value
    api.vq_cliques(fq, ov, out, min_qual=0.0, **K.HAND_GRAPH)
    assert "singles.fastq" in os.listdir(out)
