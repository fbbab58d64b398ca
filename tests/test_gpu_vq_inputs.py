"""GPU: what hlmi_vq_graph / hlmi_vq_merge / hlmi_vq_iteration make of their two input files at the seams between the stage-b
sources: which reads are refused and when (singles.fastq is parsed once and handed on), what the C entry point of the
overlaps parser writes into a short buffer, and a vertex with enough out-edges for trans_big_kernel on its way through the
graph.  The models are tests/vq_graph_model.py and oracle/vq.py."""
import ctypes as C
import os
import random

import pytest

import vq_graph_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1
GRAPH = dict(min_overlap_len=1, merge_contigs=1.0)          # every row is a candidate and every candidate an edge


def _fastq(path, lens, seed, qual=None):
    """Reads 1 .. len(lens) of random bases; qual: {read id: quality line} for the ones that are not all '='."""
    rng = random.Random(seed)
    qual = qual or {}
    path.write_text("".join(f"@{k + 1}\n{''.join(rng.choice('ACGT') for _ in range(n))}\n+\n{qual.get(k + 1, '=' * n)}\n"
                            for k, n in enumerate(lens)))
    return str(path)


def _row(id1, id2, pos1, length, perc=99):
    return f"{id1}\t{id2}\t{pos1}\t-\t-\t+\t+\t{perc}\t-\t{length}\t-\ts\ts\n"


def _refused(call, out):
    from hylight_amd import api
    with pytest.raises(api.HlmiError) as e:
        call(str(out))
    assert e.value.code == EINVAL
    assert os.listdir(out) == []


@pytest.mark.parametrize("bad", ["=" * 399, "=" * 200 + "\x1f" + "=" * 199], ids=["short", "below_bang"])
def test_bad_quality_of_an_unnamed_read(tmp_path, bad):
    """(a), (b): read 3 is named by no row; its quality line is refused all the same, before a file is written."""
    from hylight_amd import api
    fq = _fastq(tmp_path / "singles.fastq", [400] * 3, 1, {3: bad})
    ov = tmp_path / "ov.savage"
    ov.write_text(_row(1, 2, 100, 300))
    _refused(lambda out: api.vq_graph(fq, str(ov), out, **GRAPH), tmp_path / "o")


def test_bad_quality_without_a_candidate(tmp_path):
    """(c), (d): without a candidate nothing is scored and the graph call does not look at the qualities; the merge and the
    iteration do (vq_merge_check_reads), before a file is written."""
    from hylight_amd import api
    fq = _fastq(tmp_path / "singles.fastq", [400] * 3, 1, {3: "=" * 399})
    ov = tmp_path / "ov.savage"
    ov.write_text(_row(1, 2, 100, 300))
    out = tmp_path / "g"
    st = api.vq_graph(fq, str(ov), str(out), min_overlap_len=301, merge_contigs=1.0)
    assert st["edges_built"] == 0 and st["vertices"] == 3
    assert os.listdir(out) == ["nonedge_overlaps.txt"]
    assert (out / "nonedge_overlaps.txt").read_text() == "1\t2\t100\t0\t-\t+\t+\t99\t0\t300\t0\ts\ts\n"   # get_overlap_line
    _refused(lambda o: api.vq_merge(fq, str(ov), o, min_overlap_len=301, merge_contigs=1.0), tmp_path / "m")
    _refused(lambda o: api.vq_iteration(fq, str(ov), o, min_overlap_len=301, merge_contigs=1.0), tmp_path / "i")


def test_candidate_names_a_missing_read(tmp_path):
    """(e)"""
    from hylight_amd import api
    fq = _fastq(tmp_path / "singles.fastq", [400] * 3, 1)
    ov = tmp_path / "ov.savage"
    ov.write_text(_row(1, 2, 100, 300) + _row(2, 7, 100, 300))
    _refused(lambda out: api.vq_graph(fq, str(ov), out, **GRAPH), tmp_path / "o")


def test_parser_wrapper(tmp_path):
    """5 candidates, 2 rows too short for an edge, a row of 12 columns and a self-overlap; then the C entry point with room for
    two rows: the count is the whole file's, and the third slot is left alone."""
    from hylight_amd import api
    cand = [_row(1, 2, 10 * k, 300 + k) for k in range(5)]
    short = [_row(3, 4, 5, 100), _row(4, 5, 6, 120)]
    bad = "\t".join(_row(5, 6, 7, 300).split("\t")[:12]) + "\n"
    lines = [cand[0], bad, short[0], cand[1], _row(6, 6, 0, 300), cand[2], short[1], cand[3], cand[4]]
    ov = tmp_path / "ov.savage"
    ov.write_text("".join(lines))
    rows, n_nonedge, n_skipped = api.vq_parse_overlaps(str(ov), 150)
    assert (n_nonedge, n_skipped) == (2, 2)
    assert [(r["id1"], r["id2"], r["pos1"], r["len1"]) for r in rows] == [(1, 2, 10 * k, 300 + k) for k in range(5)]
    rows, n_nonedge, n_skipped = api.vq_parse_overlaps(str(ov), 150, max_overlaps=3)      # the first three LINES
    assert ([r["pos1"] for r in rows], n_nonedge, n_skipped) == ([0], 1, 1)

    buf = (api.VqOverlap * 3)()
    C.memset(buf, 0xa5, C.sizeof(buf))
    n, ne, sk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = api.load().hlmi_vq_parse_overlaps(str(ov).encode(), 150, 0, 0, 100000000, buf, 2, C.byref(n), C.byref(ne), C.byref(sk))
    assert rc == 0 and (n.value, ne.value, sk.value) == (5, 2, 2)
    assert [(o.id1, o.id2, o.pos1, o.len1) for o in buf[:2]] == [(1, 2, 0, 300), (1, 2, 10, 301)]
    assert bytes(buf)[2 * C.sizeof(api.VqOverlap):] == b"\xa5" * C.sizeof(api.VqOverlap)


N_BIG = 1027                     # reads; read 1 overlaps reads 2 .. 1026: vqk::SET_CAP / 2 + 1 = 1025 out-edges


def _big_vertex(tmp_path):
    """Read k lies at P(k) of one layout, so every row i -> j (pos1 = P(j) - P(i) > 0) is a consistent overlap.  Reads 1 .. 6
    overlap each other in all pairs: 1 -> k is transitive through 2 for k = 3 .. 6, and among those transitive edges
    1 -> 5 is transitive again (through 3), so remove_trans 2 finds edges too."""
    lens = [320 + k % 7 for k in range(N_BIG)]
    P = lambda k: 10 * (k - 1) if k <= 6 else 60 + k % 200
    pairs = [(1, k) for k in range(2, N_BIG)] + [(a, b) for a in range(2, 7) for b in range(a + 1, 7)]
    random.Random(4).shuffle(pairs)
    fq = _fastq(tmp_path / "big.fastq", lens, 4)
    ov = tmp_path / "big.savage"
    ov.write_text("".join(_row(a, b, P(b) - P(a), min(lens[a - 1] - (P(b) - P(a)), lens[b - 1])) for a, b in pairs))
    return fq, str(ov), pairs


@pytest.mark.parametrize("remove_trans", [1, 2])
def test_big_vertex_through_the_graph(tmp_path, remove_trans):
    from hylight_amd import api
    from test_gpu_vq_graph import _same
    fq, ov, pairs = _big_vertex(tmp_path)
    assert sum(a == 1 for a, _ in pairs) == 1025
    o = dict(GRAPH, remove_branches=False, remove_tips=False, remove_trans=remove_trans)
    model_dir, lib_dir = str(tmp_path / "model"), str(tmp_path / "lib")
    want = M.graph(fq, ov, model_dir, **o)                    # the model alone, its own scores
    assert want["transitive"] > 0 and want["edges_built"] == len(pairs) and want["conflicts"] == 0 and want["moved"] == 0
    got = api.vq_graph(fq, ov, lib_dir, **o)
    _same(lib_dir, model_dir, got, want)
    assert got["transitive"] > 0
    # no edge was dropped or turned before removeTransitiveEdges, so it saw the rows' edges: the public entry point agrees
    _, n = api.vq_transitive_edges(N_BIG, [a - 1 for a, _ in pairs], [b - 1 for _, b in pairs], None, remove_trans)
    assert n == got["transitive"]
