"""GPU: hlmi_vq_clique_iteration against tests/vq_clique_next_model.py - every file of out_dir byte for byte (the graph's, the
clique step's, overlaps.txt, stats.txt) and every counter.  What an input has to reach - vertices in several super-reads,
products of two lists, owners that are not the first turn of their edge, negative indices, lists longer than a wave and
products larger than a workgroup - is asserted from the model, never from the library."""
import json
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_clique_cases as K  # noqa: E402
import vq_clique_inputs as I  # noqa: E402
import vq_clique_model as CM  # noqa: E402
import vq_clique_next_model as CN  # noqa: E402
import vq_graph_model as M  # noqa: E402
import vq_next_model as NX  # noqa: E402
from test_gpu_vq_graph import _lib_scores  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLYTE = dict(min_overlap_len=60, edge_threshold=0.97, remove_tips=False, ignore_inclusions=False)
EC = dict(POLYTE, error_correction=True, min_clique_size=3, remove_trans=2, remove_branches=False, remove_backedges=False,
          keep_singletons=1000)
NO_EC = dict(POLYTE, error_correction=False, min_clique_size=2, remove_trans=1, remove_branches=True, remove_backedges=True,
             keep_singletons=0)
NAMES = M.OUTPUTS + CM.OUTPUTS + ("overlaps.txt", "stats.txt")


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in NAMES if os.path.exists(os.path.join(d, n))}


def _same(lib_dir, model_dir, got, want):
    a, b = _files(lib_dir), _files(model_dir)
    assert sorted(a) == sorted(b)
    for n in b:
        assert a[n] == b[n], n
    ggot, cgot, ngot = got
    gwant, cwant, nwant, _ = want
    assert ggot == gwant
    assert {k: cgot[k] for k in CM.STATS} == {k: cwant[k] for k in CM.STATS}
    print("next stats", ngot, nwant)
    assert {k: ngot[k] for k in CN.STATS} == nwant and ngot["ms_next"] >= 0


def _compare(tmp_path, fq, ov, name, scores=None, subreads_in=None, **opts):
    from hylight_amd import api
    lib_dir, model_dir = str(tmp_path / (name + "_lib")), str(tmp_path / (name + "_model"))
    got = api.vq_clique_iteration(fq, ov, lib_dir, subreads_in=subreads_in, **opts)
    want = CN.clique_iteration(fq, ov, model_dir, api.vq_cliques_of_graph, subreads_in=subreads_in, scores=scores, **opts)
    _same(lib_dir, model_dir, got, want)
    assert "overlaps.txt" in _files(lib_dir) and _files(lib_dir)["stats.txt"].count(b"\n") == 1
    return got[2], want[3]


@pytest.fixture(scope="module")
def cluster(tmp_path_factory):
    """3 haplotypes of 2 kb at 1 % divergence, 400 reads of 150 bases with 1 % substitutions; the scores once."""
    from hylight_amd import api
    d = tmp_path_factory.mktemp("cluster")
    fq, ov = str(d / "singles.fastq"), str(d / "overlaps.txt")
    assert I.write_inputs(I.haplotype_reads(), fq, ov) > 5000
    return fq, ov, _lib_scores(api, fq, ov, min_overlap_len=60)


@pytest.fixture(scope="module")
def ec_run(tmp_path_factory, cluster):
    fq, ov, scores = cluster
    return _compare(tmp_path_factory.mktemp("ec"), fq, ov, "ec", scores=scores, **EC)


def test_simulated_cluster_error_correction(ec_run):
    """Error correction, min_clique_size 3, remove_trans 2, keep_singletons 1000: the input reaches what the lists are about."""
    st, nx = ec_run
    print("ec reaches", nx.stats, nx.late_owners, nx.wide_sr2sr, nx.min_idx, nx.max_turns)
    assert nx.stats["in_several"] > 0 and nx.stats["max_list"] >= 2
    assert nx.wide_sr2sr > 0                                 # sr2sr turns with both lists of two entries and more
    assert nx.late_owners > 0                                # an owner that is not the first claiming turn of its edge
    assert nx.min_idx < 0                                    # a read in front of trim_pos
    assert st["sr2sr"] > 0 and st["lines"] > 0 and st["candidates"] > st["sr2sr"]


def test_simulated_cluster_without_error_correction(tmp_path, cluster):
    """--no_EC, min_clique_size 2, remove_trans 1, remove_branches 1: removeBranches leaves this graph few cliques, mostly pairs
    (the model of tests/test_gpu_vq_cliques.py), so the copied reads, all four cases and the branching edges carry this run;
    without error correction trim_pos is 0 and no index is negative."""
    fq, ov, scores = cluster
    st, nx = _compare(tmp_path, fq, ov, "no_ec", scores=scores, **NO_EC)
    print("no_ec reaches", nx.stats, nx.late_owners, nx.wide_sr2sr, nx.min_idx, nx.max_turns)
    assert nx.min_idx == 0 and st["src_branching"] > 0 and st["lines"] > 0
    assert min(st["copied"], st["u2sr"], st["v2sr"], st["sr2sr"]) > 0


def test_no_inclusion_overlaps(tmp_path, cluster, ec_run):
    fq, ov, scores = cluster
    plain, _ = ec_run
    st, _ = _compare(tmp_path, fq, ov, "noincl", scores=scores, no_inclusion_overlaps=True, **EC)
    lines = open(tmp_path / "noincl_lib" / "overlaps.txt").read().split("\n")[:-1]
    assert lines and all(l.split("\t")[7] != "100" for l in lines)
    assert st["lines"] < plain["lines"] and st["candidates"] == plain["candidates"]
    assert sum(st[k] for k in ("copied", "u2sr", "v2sr", "sr2sr")) < sum(plain[k] for k in ("copied", "u2sr", "v2sr", "sr2sr"))


def tiling(n=131, length=130, seed=11):
    """Reads of one genome at step 1: with a minimum overlap of 65 the reads k .. k + 65 are a maximal clique for every k."""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(n + length))
    return [(k, 0, g[k:k + length], "I" * length) for k in range(n)]


def test_dense_tiling(tmp_path):
    """131 identical-genome reads at step 1, every overlap of 65 bases and more an edge, no transitive reduction
    (remove_trans 0), so the 66 windows of 66 reads survive as cliques and read 65 lies in all of them.  The model reaches:
    max_list 66 (a list crossing a wave), 4290 turns of one source edge (a product crossing a workgroup), 8 435 570
    candidates in all, 2145 lines.  A smaller tiling cannot reach a list of 65: that needs 65 windows of 65 reads."""
    from hylight_amd import api
    fq, ov = str(tmp_path / "singles.fastq"), str(tmp_path / "overlaps.txt")
    assert I.write_inputs(tiling(), fq, ov, min_ovl=65) == 6370
    opts = dict(NO_EC, min_overlap_len=65, remove_trans=0, remove_branches=False)
    st, nx = _compare(tmp_path, fq, ov, "tiling", scores=_lib_scores(api, fq, ov, min_overlap_len=65), **opts)
    print("tiling reaches", nx.stats, nx.max_turns)
    assert nx.stats["max_list"] > 64 and nx.max_turns > 256
    assert (nx.stats["max_list"], nx.max_turns) == (66, 4290)


G600 = "".join(random.Random(3).choice("ACGT") for _ in range(600))


def _reads(*spans):
    return [(G600[p:p + n], K.Q * n, True) for p, n in spans]


def case_hub():
    """min_clique_size 3.  h = 0 at 100; triangles {a_k, h, b_k}, k = 0 .. 2, and {h, w, b_0}: h lies in four super-reads, b_0
    in two, one of them shared with h (:255).  x1 (left) and x2 (right) touch h alone: cliques of two are below the minimum, so
    both are copied and meet the whole list of h (:73, :151)."""
    spans = [(100, 100)] + [(60 + 10 * k, 100) for k in range(3)] + [(120 + 10 * k, 100) for k in range(3)] + [(130, 100), (50, 80), (170, 80)]
    h, a, b, w, x1, x2 = 0, [1, 2, 3], [4, 5, 6], 7, 8, 9
    pos = [p for p, _ in spans]
    pairs = [(a[k], h) for k in range(3)] + [(h, b[k]) for k in range(3)] + [(a[k], b[k]) for k in range(3)] + [(h, w), (b[0], w), (x1, h), (h, x2)]
    return dict(reads=_reads(*spans), edges=[(u, v, pos[v] - pos[u]) for u, v in pairs], opts=dict(min_clique_size=3))


def case_trimmed():
    """Error correction, min_clique_size 4.  m0 .. m3 (vertices 1 .. 4) at 40, 45, 50, 55, 60 bases each: trim_pos 15, indices
    -15, -10, -5, 0, a consensus of 45 bases.  x (vertex 0, 40 bases at 10) ends in front of the super-read: x -> m0 at 30 owns
    the pair and fails, 30 + 15 = 45 >= 40; the row m3 -> x at 5 - its position is the file's, not the genome's - would give
    5 + 0 = 5 of 45 and is dropped: no line (:84-97 in front of :115).  y (vertex 5) hangs behind m1 at 5: 5 - 10 = -5, y
    first."""
    spans = [(10, 40), (40, 60), (45, 60), (50, 60), (55, 60), (50, 60)]
    edges = [(1, 2, 5), (1, 3, 10), (1, 4, 15), (2, 3, 5), (2, 4, 10), (3, 4, 5), (0, 1, 30), (4, 0, 5), (2, 5, 5)]
    return dict(reads=_reads(*spans), edges=edges, opts=dict(min_clique_size=4, error_correction=True, keep_singletons=0))


def case_empty_list():
    """min_clique_size 3, keep_singletons 50: z (30 bases) touches a of the triangle {a, b, c} and the lone read t; it is in
    no clique of three, unvisited and too short: visited with an empty list (SRBuilder.cpp:1149-1154).  a -> z and z -> t give
    nothing; t -> u between two copied reads is copied."""
    spans = [(0, 100), (10, 100), (20, 100), (80, 30), (90, 100), (120, 100)]
    edges = [(0, 1, 10), (0, 2, 20), (1, 2, 10), (0, 3, 80), (3, 4, 10), (4, 5, 30)]
    return dict(reads=_reads(*spans), edges=edges, opts=dict(min_clique_size=3, keep_singletons=50))


HAND = dict(K.CASES, hub=case_hub, trimmed=case_trimmed, empty_list=case_empty_list)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_through_the_library(tmp_path, name):
    """The graph is the case's rows as they are (merge_contigs 1, no reduction, the back edges kept).  n_rate: a clique dropped
    for its N rate leaves its members to the copied reads."""
    case = HAND[name]()
    fq, ov, sub = K.write_files(tmp_path, case)
    st, nx = _compare(tmp_path, fq, ov, name, subreads_in=sub, remove_backedges=False, **K.HAND_GRAPH, **dict(CM.CLIQUE, **case["opts"]))
    print(name, "reaches", nx.stats, nx.late_owners, nx.wide_sr2sr, nx.min_idx, nx.max_turns)
    if name == "hub":
        assert nx.stats["max_list"] == 4 and nx.stats["in_several"] == 2 and nx.wide_sr2sr > 0 and nx.late_owners > 0
        assert st["u2sr"] == 4 and st["v2sr"] == 4 and st["copied"] == 0
    if name == "trimmed":
        assert nx.min_idx == -15 and st["claims_failed"] == 1 and st["u2sr"] == 0 and st["v2sr"] == 1
    if name == "empty_list":
        assert st["copied"] == 1 and st["lines"] == 1 and st["candidates"] == 0
    if name == "n_rate":
        assert nx.stats["max_list"] == 0


def test_in_place_after_a_merge_iteration(tmp_path, cluster):
    """hlmi_vq_iteration into a directory, then hlmi_vq_clique_iteration over that directory's own singles.fastq, overlaps.txt
    and subreads.txt (first_it 0) into the same directory; the models are chained the same way."""
    from hylight_amd import api
    fq, ov, scores = cluster
    lib_dir, model_dir = str(tmp_path / "lib"), str(tmp_path / "model")
    first = dict(POLYTE, remove_trans=1, remove_branches=True, keep_singletons=0, first_it=True)
    api.vq_iteration(fq, ov, lib_dir, **first)
    NX.iteration(fq, ov, model_dir, scores=scores, **first)
    p = lambda d, n: os.path.join(d, n)
    for n in ("singles.fastq", "overlaps.txt", "subreads.txt"):
        assert open(p(lib_dir, n), "rb").read() == open(p(model_dir, n), "rb").read(), n
    scores2 = _lib_scores(api, p(lib_dir, "singles.fastq"), p(lib_dir, "overlaps.txt"), min_overlap_len=60)
    second = dict(EC, first_it=False, keep_singletons=0, min_clique_size=2)
    got = api.vq_clique_iteration(p(lib_dir, "singles.fastq"), p(lib_dir, "overlaps.txt"), lib_dir, subreads_in=p(lib_dir, "subreads.txt"), **second)
    want = CN.clique_iteration(p(model_dir, "singles.fastq"), p(model_dir, "overlaps.txt"), model_dir, api.vq_cliques_of_graph,
                               subreads_in=p(model_dir, "subreads.txt"), scores=scores2, **second)
    _same(lib_dir, model_dir, got, want)
    assert got[1]["superreads"] > 0 and got[2]["lines"] > 0
    assert open(p(lib_dir, "stats.txt")).read().count("\n") == 2


def test_cli_iteration(tmp_path, cluster):
    fq, ov, _ = cluster
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "hylight_amd.vq_cliques", "--singles", fq, "--overlaps", ov, "--out", out, "--min_overlap_len", "60",
           "--edge_threshold", "0.97", "--error_correction", "true", "--min_clique_size", "3"]
    r = subprocess.run(cmd + ["--iteration"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().split("\n")[-1])
    assert st["next"]["lines"] > 0 and st["next"]["lines"] == open(os.path.join(out, "overlaps.txt")).read().count("\n")
