"""GPU: hlmi_vq_iteration (SRBuilder::findNextOverlaps behind the merge) and hylight_amd.vq_stageb against the model in
tests/vq_next_model.py: every output file byte for byte, every integer stat field for field.  PARITY UNPINNED: the
reference needs Boost and cannot be built here; tests/test_vq_next_model.py holds the model to hand-worked lines.

The ids of overlaps.txt are the NEW reads' ids, counted from 0, so a line's width cannot be driven through `@<id>` lines;
the width cases reach it through the numeric columns of a copied non-edge row (a numeric column 4: pos2 and len2 are kept)."""
import os
import re
import shutil

import pytest

import vq_graph_model as M  # noqa: E402
import vq_merge_model as MM  # noqa: E402
import vq_next_model as N  # noqa: E402
from test_gpu_vq_graph import _lib_scores  # noqa: E402
from test_gpu_vq_merge import _synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = M.OUTPUTS + MM.OUTPUTS + ("overlaps.txt", "stats.txt")


def _width():
    src = open(os.path.join(ROOT, "hylight_amd", "csrc", "vq_internal.h")).read()
    return int(re.search(r"constexpr uint32_t LINE_WIDTH = (\d+);", src).group(1))


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in NAMES if os.path.exists(os.path.join(d, n))}


def _check(got, want, lib_dir, model_dir):
    a, b = _files(lib_dir), _files(model_dir)
    assert sorted(a) == sorted(b)
    for n in b:
        assert a[n] == b[n], n
    assert got[0] == want[0]
    assert {k: got[1][k] for k in MM.STATS} == want[1]
    assert {k: got[2][k] for k in N.STATS} == want[2] and got[2]["ms_next"] >= 0


def _compare(tmp_path, fq, ov, name, subreads_in=None, **opts):
    from hylight_amd import api
    lib_dir, model_dir = str(tmp_path / (name + "_lib")), str(tmp_path / (name + "_model"))
    gopts = {k: v for k, v in opts.items() if k in M.STAGEB}
    scores = _lib_scores(api, fq, ov, **gopts)
    got = api.vq_iteration(fq, ov, lib_dir, subreads_in=subreads_in, **opts)
    want = N.iteration(fq, ov, model_dir, subreads_in=subreads_in, scores=scores, **opts)
    _check(got, want, lib_dir, model_dir)
    return got


def _reads(tmp_path, seqs, name="singles.fastq"):
    fq = tmp_path / name
    fq.write_text("".join(f"@{k + 1}\n{s}\n+\n{'I' * len(s)}\n" for k, s in enumerate(seqs)))
    return str(fq)


def _genome(n, seed=3):
    import random
    return "".join(random.Random(seed).choices("ACGT", k=n))


def _tiling(tmp_path, n, length=400, step=150, extra_rows=()):
    """n reads of `length` bases every `step` bases of one genome, rows between neighbours and next-but-one neighbours."""
    g = _genome(step * n + length)
    fq = _reads(tmp_path, [g[k * step:k * step + length] for k in range(n)])
    rows = []
    for k in range(n):
        for d in (1, 2):
            if k + d < n and d * step < length:
                ol = length - d * step
                rows.append(f"{k + 1}\t{k + 1 + d}\t{d * step}\t-\t-\t+\t+\t{100 * ol // length}\t-\t{ol}\t-\ts\ts")
    ov = tmp_path / "rows.savage"
    ov.write_text("\n".join(rows + list(extra_rows)) + "\n")
    return fq, str(ov)


@pytest.mark.parametrize("n", [2, 3, 7, 300])
def test_tiling_every_case(tmp_path, n):
    """A chain of overlapping reads, min_overlap_len 200: the next-but-one rows (100 bases) are non-edge rows, the greedy
    merge pairs (0, 1), (2, 3), .. (250-base edges; 100-base rows to the next but one): with an odd count the last read stays a copy (u2sr / v2sr), pairs meet pairs (sr2sr),
    and 300 reads put a key's claimants (graph edge and non-edge rows) across 256-thread blocks."""
    fq, ov = _tiling(tmp_path, n)
    g = _compare(tmp_path, fq, ov, "t", min_overlap_len=200, keep_singletons=200)
    if n >= 7:
        assert g[2]["sr2sr"] > 0 and g[2]["src_nonedge"] > 0
    if n % 2:                                                 # the last read has no partner left
        assert g[2]["u2sr"] + g[2]["v2sr"] > 0
    if n == 3:
        assert g[2]["lines"] == 1


def test_no_source_edge_and_one(tmp_path):
    """One edge, both reads merged: its only source edge joins a super-read with itself (:255) - an empty overlaps.txt and a
    stats.txt line with 0.  No edge at all: the call stops where hlmi_vq_merge stops."""
    from hylight_amd import api
    fq, ov = _tiling(tmp_path, 2)
    g = _compare(tmp_path, fq, ov, "one", min_overlap_len=100)
    assert g[2]["src_graph"] == 1 and g[2]["lines"] == 0
    assert open(tmp_path / "one_lib" / "overlaps.txt", "rb").read() == b""
    assert open(tmp_path / "one_lib" / "stats.txt").read() == "2\t1\t0\n"
    out = tmp_path / "none"
    g = api.vq_iteration(fq, ov, str(out), min_overlap_len=500)
    assert g[0]["edges_built"] == 0 and not os.path.exists(out / "overlaps.txt") and not os.path.exists(out / "stats.txt")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_line_width(tmp_path, delta):
    """The longest line at LINE_WIDTH - 1, LINE_WIDTH (device order) and LINE_WIDTH + 1 (host order): a non-edge row between
    two reads that stay unmerged copies, its columns filled to the width; further rows keep the order non-trivial."""
    W = _width()
    g = _genome(20000, 5)
    # 120 lone reads in front: the super-read of reads 121 / 122 is new read 0, the lone reads 1 .. 120, so the reads of the
    # wide row get three-digit ids
    seqs = [g[100 * k:100 * k + 100] for k in range(120)] + [g[13000:13400], g[13250:13650], g[15000:15400], g[16000:16400],
                                                             g[17000:17400]]
    fq = _reads(tmp_path, seqs)
    # The parser holds a row to Overlap.h:59-72: a percentage is at most 100 and a single-end row carries ord '-'; a numeric
    # column 4 still keeps pos2 and len2.  So the width comes from pos1, pos2, len2 (ten digits each), perc 100 and len1 -
    # which stays below a min_overlap_len of 1e8, so that the row is a non-edge row; the one edge's row claims 2e8.
    fixed = 3 + 3 + len("-++0ss") + 12                                          # two ids, six single characters, twelve tabs
    big = "1111111111"                                                          # ten digits, below 2^31
    len1 = "1" * (W + delta - fixed - 3 * len(big) - len("100"))
    assert 1 <= len(len1) <= 8
    rows = ["121\t122\t250\t-\t-\t+\t+\t37\t-\t200000000\t-\ts\ts",
            f"123\t124\t{big}\t{big}\t-\t+\t+\t100\t0\t{len1}\t{big}\ts\ts",
            "124\t125\t9\t-\t-\t-\t+\t50\t-\t50\t-\ts\ts", "123\t125\t9\t-\t-\t+\t+\t50\t-\t50\t-\ts\ts"]
    ov = tmp_path / "w.savage"
    ov.write_text("\n".join(rows) + "\n")
    got = _compare(tmp_path, fq, str(ov), "w", min_overlap_len=100000000, keep_singletons=100)
    lines = open(tmp_path / "w_lib" / "overlaps.txt").read().split("\n")[:-1]
    assert max(len(l) for l in lines) == W + delta and got[2]["copied"] == 3


def test_refusals(tmp_path):
    from hylight_amd import api
    fq, ov = _tiling(tmp_path, 3, extra_rows=["1\t3\t1\t2\t1\t+\t+\t90\t90\t40\t40\tp\tp"])
    out = tmp_path / "o"
    with pytest.raises(api.HlmiError) as e:
        api.vq_iteration(fq, ov, str(out), min_overlap_len=200)
    assert e.value.code == -6 and not os.path.exists(out / "nonedge_overlaps.txt")
    with pytest.raises(api.HlmiError):
        api.vq_iteration(fq, ov, str(out), first_it=False)
    with pytest.raises(TypeError):
        api.vq_iteration(fq, ov, str(out), add_duplicates=True)


def test_synthetic_two_iterations_in_place(tmp_path):
    """The read set of test_gpu_vq_merge.py's synthetic case; the second iteration runs in place on the first one's
    singles.fastq / overlaps.txt / subreads.txt, for the library and for the model each in its own directory, and equals the
    same iteration run from copies into another directory."""
    from hylight_amd import api
    fq, ov, _ = _synthetic(tmp_path, 7, 2000, 200000)
    o = dict(min_overlap_len=100, merge_contigs=1.0)
    g1 = _compare(tmp_path, fq, ov, "s", **o)
    assert g1[2]["lines"] > 0 and g1[2]["sr2sr"] > 0 and g1[2]["copied"] + g1[2]["u2sr"] + g1[2]["v2sr"] > 0
    print("ms_next iteration 1:", g1[2]["ms_next"])
    lib, model, copy = str(tmp_path / "s_lib"), str(tmp_path / "s_model"), tmp_path / "copy"
    copy.mkdir()
    for n in ("singles.fastq", "overlaps.txt", "subreads.txt"):
        shutil.copyfile(os.path.join(lib, n), copy / n)
    p = lambda d, n: os.path.join(d, n)
    o2 = dict(o, first_it=False, merge_contigs=0)
    scores = _lib_scores(api, p(lib, "singles.fastq"), p(lib, "overlaps.txt"), min_overlap_len=100)
    got = api.vq_iteration(p(lib, "singles.fastq"), p(lib, "overlaps.txt"), lib, subreads_in=p(lib, "subreads.txt"), **o2)
    want = N.iteration(p(model, "singles.fastq"), p(model, "overlaps.txt"), model, subreads_in=p(model, "subreads.txt"),
                       scores=scores, **o2)
    _check(got, want, lib, model)
    print("ms_next iteration 2:", got[2]["ms_next"])
    assert open(p(lib, "stats.txt")).read().count("\n") == 2
    away = str(tmp_path / "away")
    api.vq_iteration(str(copy / "singles.fastq"), str(copy / "overlaps.txt"), away, subreads_in=str(copy / "subreads.txt"), **o2)
    for n in ("singles.fastq", "overlaps.txt", "subreads.txt", "superread_map.txt", "graph.txt"):
        assert open(p(away, n), "rb").read() == open(p(lib, n), "rb").read(), n


def test_stageb_to_its_end(tmp_path):
    """vq_stageb.run against the model's loop: the final files and the counts per iteration."""
    from hylight_amd import vq_stageb
    fq, ov = _tiling(tmp_path, 9, length=700, step=300)
    fdir = tmp_path / "fastq"
    fdir.mkdir()
    shutil.move(fq, fdir / "singles.fastq")
    lib, model = str(tmp_path / "lib"), str(tmp_path / "model")
    got = vq_stageb.run(str(fdir), ov, lib)
    want = N.stageb(str(fdir), ov, model)
    assert got == want and got["iterations"] >= 2
    for n in ("singles.fastq", "subreads.txt", "overlaps.txt", "stats.txt", "removed_tip_sequences.fastq"):
        assert open(os.path.join(lib, n), "rb").read() == open(os.path.join(model, n), "rb").read(), n
    vq_stageb.fastq2fasta(os.path.join(lib, "singles.fastq"), str(tmp_path / "a.fa"))
    N.fastq2fasta(os.path.join(model, "singles.fastq"), str(tmp_path / "b.fa"))
    assert open(tmp_path / "a.fa").read() == open(tmp_path / "b.fa").read() != ""
