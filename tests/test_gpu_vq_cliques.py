"""GPU: hlmi_vq_cliques against tests/vq_clique_model.py - cliques.txt, singles.fastq, subreads.txt and clique_map.txt byte
for byte, the counters equal (columns_host and the wall time are the library's own: the model has no margin).  The clique file
itself is pinned to the reference by tests/test_vq_cliques_host.py."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_clique_cases as K  # noqa: E402
import vq_clique_inputs as I  # noqa: E402
import vq_clique_model as CM  # noqa: E402
import vq_graph_model as M  # noqa: E402
from test_gpu_vq_graph import _lib_scores  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLYTE = dict(min_overlap_len=60, edge_threshold=0.97, remove_tips=False, ignore_inclusions=False)
EC = dict(POLYTE, error_correction=True, remove_trans=2, remove_branches=False, remove_backedges=False, keep_singletons=1000)
NO_EC = dict(POLYTE, error_correction=False, remove_trans=1, remove_branches=True, remove_backedges=True, keep_singletons=0)


def _files(d, names):
    return {n: open(os.path.join(d, n), "rb").read() for n in names if os.path.exists(os.path.join(d, n))}


def _compare(tmp_path, fq, ov, name, scores=None, subreads_in=None, **opts):
    from hylight_amd import api
    lib_dir, model_dir = str(tmp_path / (name + "_lib")), str(tmp_path / (name + "_model"))
    ggot, cgot = api.vq_cliques(fq, ov, lib_dir, subreads_in=subreads_in, **opts)
    gwant, cwant = CM.cliques(fq, ov, model_dir, api.vq_cliques_of_graph, subreads_in=subreads_in, scores=scores, **opts)
    names = M.OUTPUTS + CM.OUTPUTS
    got, want = _files(lib_dir, names), _files(model_dir, names)
    assert sorted(got) == sorted(want)
    for n in want:
        assert got[n] == want[n], n
    assert ggot == gwant
    print(name, cgot, cwant)
    assert {k: cgot[k] for k in CM.STATS} == {k: cwant[k] for k in CM.STATS}
    assert cgot["ms_cliques"] >= 0 and cgot["columns_host"] <= cgot["columns"]
    return cgot, cwant


@pytest.fixture(scope="module")
def cluster(tmp_path_factory):
    """(a): 3 haplotypes of 2 kb at 1 % divergence, 400 reads of 150 bases with 1 % substitutions; the scores once."""
    from hylight_amd import api
    d = tmp_path_factory.mktemp("cluster")
    fq, ov = str(d / "singles.fastq"), str(d / "overlaps.txt")
    assert I.write_inputs(I.haplotype_reads(), fq, ov) > 5000
    return fq, ov, _lib_scores(api, fq, ov, min_overlap_len=60)


@pytest.mark.parametrize("name,opts", [("ec3", dict(EC, min_clique_size=3)), ("ec4", dict(EC, min_clique_size=4)),
                                       ("no_ec", dict(NO_EC, min_clique_size=2))])
def test_simulated_cluster(tmp_path, cluster, name, opts):
    fq, ov, scores = cluster
    got, want = _compare(tmp_path, fq, ov, name, scores=scores, **opts)
    assert got["superreads"] > 20
    if opts["error_correction"]:
        # (d) not a vacuous comparison: the columns of three bases and more were decided on the device, not all sent back
        assert want["deep"] > 2000 and 2 * got["columns_host"] <= want["deep"]
    else:
        # remove_branches leaves this graph's vertices one edge in and one out: its maximal cliques are pairs (the model: 31
        # cliques taken, no column of three bases), so this run covers the two-base tables, ids and trivial reads, and the
        # deep columns without error correction are those of the hand cases and of (c)
        assert want["deep"] < 100 and got["columns_host"] <= want["deep"]


_write_case = K.write_files


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_hand_cases_through_the_library(tmp_path, name):
    """(b) The graph is built from the case's edges as they are: every row an edge (merge_contigs 1), no reduction."""
    case = K.CASES[name]()
    fq, ov, sub = _write_case(tmp_path, case)
    got, _ = _compare(tmp_path, fq, ov, name, subreads_in=sub, min_overlap_len=1, merge_contigs=1.0, remove_trans=0,
                      remove_branches=False, remove_tips=False, ignore_inclusions=False, **dict(CM.CLIQUE, **case["opts"]))
    assert got["taken"] == 1
    if name == "size7":
        assert got["filtered"] == 1
    if name in ("vote", "ec3", "reverse"):                   # what the model's own test works out by hand
        want = CM.superreads(K.state(case), K.clique_text(case), str(tmp_path / "hand"), **case["opts"])
        lib = _files(str(tmp_path / (name + "_lib")), ("singles.fastq", "subreads.txt"))
        assert lib["singles.fastq"] == open(tmp_path / "hand" / "singles.fastq", "rb").read() and want["superreads"] == 1


_HAND = K.HAND_GRAPH
# vqc::MARGIN, X_SLOPE, X_FLOOR of hylight_amd/csrc/vq_internal.h
MARGIN, X_SLOPE, X_FLOOR = 2.0 ** -44, 4.35, 2.0 ** -36


def _three_reads(tmp_path, seqs, quals):
    case = dict(reads=[(seqs[k], quals[k], True) for k in range(3)], edges=[(0, 1, 0), (0, 2, 0), (1, 2, 0)], opts=dict(min_clique_size=2))
    fq, ov, _ = _write_case(tmp_path, case)
    return _compare(tmp_path, fq, ov, "c", **_HAND, **dict(CM.CLIQUE, **case["opts"]))


def test_columns_without_a_base_go_to_the_host(tmp_path):
    """Three reads with an N each in three columns: max_score == 0, which the device always hands back."""
    got, want = _three_reads(tmp_path, ["ACGTACGTAC" + "NNN" + "ACGTACGTAC" * 6] * 3, ["I" * 73] * 3)
    assert want["deep"] == 73 and got["columns_host"] == 3


def test_columns_on_a_rounding_boundary(tmp_path):
    """(c) Three-base columns on a rounding boundary of the phred and nothing else: of all quality triples of A, A, C whose
    best base is at least 90 % sure (the others are N before anything is rounded) the 60 whose x = -10 log10(p_incorrect)
    comes closest to a half-integer, found with the same arithmetic on the CPU.  d is that distance, m = X_SLOPE * MARGIN / p
    + X_FLOOR the margin the device applies.  MARGIN is the derived bound of |p_dev - p_host| 23 times over,
    so the device's x lies within m / 23 of the host's: a column with d < 0.9 m must go back to the host, one with d > 1.1 m
    must not.  The distances start at 4.6e-7; the margin grows as 1 / p, which puts 10 of the 60 inside it (d / m from 0.11
    to 0.87; the next one stands at 1.08) and none between the two bands.  On an MI355X: columns_host 10, output identical."""
    import math
    near = []
    for q1 in range(2, 94):
        for q2 in range(q1, 94):
            for q3 in range(2, 94):
                p = [10 ** (-q / 10.0) for q in (q1, q2, q3)]
                a = math.log10(1 - p[0]) + math.log10(1 - p[1]) + math.log10(p[2] / 3)
                c = math.log10(p[0] / 3) + math.log10(p[1] / 3) + math.log10(1 - p[2])
                o = math.log10(p[0] / 3) + math.log10(p[1] / 3) + math.log10(p[2] / 3)
                tot = 10 ** a + 10 ** c + 2 * 10 ** o
                pi = 1 - 10 ** max(a, c) / tot
                if 5.1e-10 < pi < 0.0999:       # clear of the two other thresholds, 10^-9.3 and 1 - minQual
                    x = -10 * math.log10(pi)
                    near.append((abs(x - math.floor(x) - 0.5), q1, q2, q3, pi))
    near.sort()
    cols = near[:60]
    ratio = [d / (X_SLOPE * MARGIN / pi + X_FLOOR) for d, _, _, _, pi in cols]
    must, may = sum(r < 0.9 for r in ratio), sum(r < 1.1 for r in ratio)
    print("nearest rounding boundaries (distance, q1, q2, q3, p_incorrect):", cols[:5], "inside the margin:", must, may)
    assert must > 0
    got, want = _three_reads(tmp_path, ["A" * 60, "A" * 60, "C" * 60], ["".join(chr(33 + c[k + 1]) for c in cols) for k in range(3)])
    assert want["deep"] == 60 and got["superreads"] == 1
    assert got["columns_host"] > 0 and must <= got["columns_host"] <= may


def test_a_pair_is_a_clique_of_two(tmp_path):
    """The GPU half of tests/test_vq_clique_model.py::test_a_pair_is_a_clique_of_two: hlmi_vq_merge (merge_kernel) and
    hlmi_vq_cliques (the two-base tables of pile_kernel) over the one placement, each byte for byte its model, write the same
    records."""
    from test_gpu_vq_merge import _compare as compare_merge
    case = K.case_pairs()
    fq, ov, _ = _write_case(tmp_path, case)
    _, mst = compare_merge(tmp_path, fq, ov, "m", **_HAND, first_it=True, keep_singletons=0, store_tips_separately=False, min_clique_size=2)
    cst, _ = _compare(tmp_path, fq, ov, "c", **_HAND, **dict(CM.CLIQUE, keep_singletons=0, **case["opts"]))
    assert K.records(str(tmp_path / "m_lib")) == K.records(str(tmp_path / "c_lib"))
    for k in ("dropped_empty", "dropped_n", "trivial", "trivial_reverse"):
        assert mst[k] == cst[k], k
    assert (mst["pairs"], mst["merged"], cst["taken"], cst["superreads"], cst["dropped_n"], cst["trivial"]) == (4, 3, 4, 3, 1, 2)


def test_cli_and_refusals(tmp_path, cluster):
    """(e)"""
    fq, ov, _ = cluster
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "hylight_amd.vq_cliques", "--singles", fq, "--overlaps", ov, "--out", out, "--min_overlap_len", "60",
           "--edge_threshold", "0.97"]
    r = subprocess.run(cmd + ["--error_correction", "true", "--min_clique_size", "3"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().split("\n")[-1])
    assert st["cliques"]["superreads"] > 20 and st["cliques"]["short_reads"] > 0          # keep_singletons 1000 with EC
    assert all(os.path.exists(os.path.join(out, n)) for n in CM.OUTPUTS)
    r = subprocess.run(cmd + ["--min_clique_size", "22"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "min_clique_size" in r.stderr
    r = subprocess.run(cmd + ["--min_clique_size", "0"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2
    paired = str(tmp_path / "paired.txt")
    open(paired, "w").write(open(ov).read() + "0\t1\t10\t20\t1\t+\t+\t90\t90\t100\t100\tp\tp\n")
    r = subprocess.run(cmd[:6] + [paired] + cmd[7:], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 4, r.stderr
