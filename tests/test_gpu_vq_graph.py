"""GPU: hlmi_vq_graph (ViralQuasispecies --graph_only for HyLight's stage b) against the model in tests/vq_graph_model.py,
byte for byte on every output file and field for field on the stats.  PARITY UNPINNED: the reference needs Boost and
cannot be built here; tests/test_vq_graph_model.py holds the model to hand-worked answers."""
import json
import os
import random
import subprocess
import sys

import pytest

import vq_graph_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
COMP = str.maketrans("ACGT", "TGCA")


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in M.OUTPUTS if os.path.exists(os.path.join(d, n))}


def _same(got_dir, want_dir, got_stats, want_stats):
    got, want = _files(got_dir), _files(want_dir)
    assert sorted(got) == sorted(want)
    for n in want:
        assert got[n] == want[n], n
    assert got_stats == want_stats


def _lib_scores(api, fq, ov, **o):
    """The library's own scores for the model (oracle/vq.py's Python scoring is too slow for these sizes; the score is
    held to the oracle by tests/test_vq_front.py)."""
    opts = dict(M.STAGEB)
    opts.update(o)
    cands, _, _ = api.vq_parse_overlaps(ov, opts["min_overlap_len"], opts["min_overlap_perc"], False, opts["max_overlaps"])
    return api.vq_overlap_scores(fq, cands, opts["mismatch"], opts["min_read_len"]) if cands else []


def _compare(tmp_path, fq, ov, name, scores=None, **opts):
    from hylight_amd import api
    lib_dir, model_dir = str(tmp_path / (name + "_lib")), str(tmp_path / (name + "_model"))
    got = api.vq_graph(fq, ov, lib_dir, **opts)
    if scores == "lib":
        scores = _lib_scores(api, fq, ov, **opts)
    want = M.graph(fq, ov, model_dir, scores=scores, **opts)
    _same(lib_dir, model_dir, got, want)
    return got


def _random_reads(path, ids, length, seed):
    rng = random.Random(seed)
    with open(path, "w") as f:
        for i in ids:
            n = length + rng.randrange(200)
            q = "".join(chr(33 + rng.randint(20, 41)) for _ in range(n)) if i % 2 else "=" * n
            f.write(f"@{i}\n{''.join(rng.choice('ACGT') for _ in range(n))}\n+\n{q}\n")


def test_golden_savage_file(tmp_path):
    """(a) the path's own SAVAGE file; reads synthesized for its ids.  They are random, so merge_contigs 1 lets every
    candidate through (mismatch rate <= 1): a dense graph."""
    ov = os.path.join(GOLD, "fxC_v3.savage")
    ids = sorted({int(l.split("\t")[k]) for l in open(ov) for k in (0, 1)})
    fq = str(tmp_path / "singles.fastq")
    _random_reads(fq, ids, 4000, 1)
    from hylight_amd import api
    scores = _lib_scores(api, fq, ov, merge_contigs=1.0)
    seqs, quals, index = M.read_singles(fq)
    cands, _, _ = api.vq_parse_overlaps(ov, 300, 0)
    for k in range(0, len(cands), 97):                        # a spot check of the scores against the oracle
        c = cands[k]
        a, b = index[c["id1"]], index[c["id2"]]
        assert scores[k] == M.OV.single_single_edge(seqs[a], quals[a], seqs[b], quals[b], c["pos1"], c["ori1"] == "+",
                                                    c["ori2"] == "+")
    st = _compare(tmp_path, fq, ov, "a", scores=scores, merge_contigs=1.0)
    assert st["edges_built"] > 1000 and st["duplicates"] > 0
    # one row in ten with its second orientation flipped: labels that no try satisfies - all 100 labelling tries, the
    # start labels carried from try to try, in-place flips piling up
    rng = random.Random(2)
    rows = [l.split("\t") for l in open(ov).read().split("\n")[:-1]]
    for r in rows:
        if rng.random() < 0.1:
            r[6] = "-" if r[6] == "+" else "+"
    ov2 = str(tmp_path / "flipped.savage")
    with open(ov2, "w") as f:
        f.write("".join("\t".join(r) + "\n" for r in rows))
    st = _compare(tmp_path, fq, ov2, "a2", scores="lib", merge_contigs=1.0)
    assert st["conflicts"] > 0 and st["moved"] > 0
    st = _compare(tmp_path, fq, ov, "a0", scores="lib")      # stage-b options as they are: random reads make no edge
    assert st["edges_built"] == 0


HAND = [  # (read lengths, rows (id1, id2, pos1, ori1, ori2[, len]), options) - tests/test_vq_graph_model.py's shapes
    ([500] * 3, [(1, 2, 100, "+", "-"), (2, 3, 100, "+", "-"), (1, 3, 200, "+", "-")], dict(remove_trans=0, remove_branches=False)),
    ([500, 500], [(1, 2, 100, "-", "-")], dict()),
    ([600, 600, 600], [(1, 2, 100, "+", "+", 300), (1, 3, 50, "+", "+"), (1, 2, 100, "+", "+", 310), (2, 1, 100, "+", "+", 310)], dict()),
    ([600, 300, 600], [(1, 2, 100, "+", "+"), (1, 2, 100, "+", "+"), (2, 3, 50, "+", "+")], dict()),
    ([1000] * 5, [(a, b, 100 * (b - a), "+", "+") for a in range(1, 6) for b in range(a + 1, 6)], dict()),
    ([500, 500, 500, 500], [(1, 2, 100, "+", "+"), (1, 3, 50, "+", "+"), (3, 4, 100, "+", "+")], dict(remove_branches=False)),
    ([500, 300, 500], [(1, 2, 100, "+", "+", 300), (1, 3, 50, "+", "+")], dict()),
    ([500] * 4, [(1, 3, 100, "+", "+"), (3, 4, 100, "+", "+"), (2, 4, 50, "+", "+")], dict(remove_branches=False)),
    ([500] * 4, [(1, 3, 100, "+", "+"), (2, 3, 150, "+", "+"), (3, 4, 100, "+", "+")], dict(remove_tips=False)),
    ([500] * 4, [(1, 2, 100, "+", "+"), (1, 3, 150, "+", "+"), (3, 4, 100, "+", "+")], dict(remove_tips=False)),
    ([500] * 3, [(1, 2, 100, "+", "+"), (2, 3, 100, "+", "+"), (3, 1, 100, "+", "+")], dict()),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_made_cases(tmp_path, case):
    """(b) the model tests' hand-made graphs on random reads (merge_contigs 1: every candidate is an edge)."""
    lens, rows, opts = HAND[case]
    rng = random.Random(case)
    fq = tmp_path / "singles.fastq"
    fq.write_text("".join(f"@{k + 1}\n{''.join(rng.choice('ACGT') for _ in range(n))}\n+\n{'=' * n}\n" for k, n in enumerate(lens)))
    ov = tmp_path / "ov.savage"
    ov.write_text("".join(f"{r[0]}\t{r[1]}\t{r[2]}\t-\t-\t{r[3]}\t{r[4]}\t{100 if len(r) > 5 and r[5] == lens[r[1] - 1] else 99}"
                          f"\t-\t{r[5] if len(r) > 5 else min(lens[r[0] - 1] - r[2], lens[r[1] - 1])}\t-\ts\ts\n" for r in rows))
    o = dict(min_overlap_len=1, merge_contigs=1.0)
    o.update(opts)
    _compare(tmp_path, str(fq), str(ov), "h", **o)


def _synthetic(tmp_path, seed, n_strains, genome_len, step, name):
    """Reads cut in random orientation from random strain genomes (a start every ~`step` bases), exact SAVAGE rows for
    every true overlap of >= 100 bases, each also from the other end (a duplicate of the same key), a share of rows one
    base off, and one substitution in some reads.  Half of the reads carry Q40 qualities: their exact overlaps pass
    edge_threshold 0.999; the others' ('=', Q28) only pass through merge_contigs."""
    rng = random.Random(seed)
    reads = []                                                  # (strain, start, len, fwd)
    for s in range(n_strains):
        g = "".join(rng.choice("ACGT") for _ in range(genome_len))
        pos = 0
        while pos < genome_len - 400:
            L = min(rng.randint(400, 900), genome_len - pos)
            reads.append((s, pos, L, rng.random() < 0.5, g[pos:pos + L]))
            pos += rng.randint(step // 2, step * 3 // 2)
    rng.shuffle(reads)
    fq = tmp_path / f"{name}.fastq"
    with open(fq, "w") as f:
        for k, (s, st, L, fwd, seq) in enumerate(reads):
            if k % 23 == 0:
                i = rng.randrange(L)
                seq = seq[:i] + "ACGT"[("ACGT".index(seq[i]) + 1) % 4] + seq[i + 1:]
            if not fwd:
                seq = seq.translate(COMP)[::-1]
            q = "I" * L if k % 2 else "=" * L
            f.write(f"@{k + 1}\n{seq}\n+\n{q}\n")
    rows = []
    by_strain = {}
    for k, r in enumerate(reads):
        by_strain.setdefault(r[0], []).append((r[1], k))
    sign = lambda b: "+" if b else "-"
    for s, lst in by_strain.items():
        lst.sort()
        for x in range(len(lst)):
            si, i = lst[x]
            Li, fi = reads[i][2], reads[i][3]
            for y in range(x + 1, len(lst)):
                sj, j = lst[y]
                if sj >= si + Li - 100:
                    break
                Lj, fj = reads[j][2], reads[j][3]
                ov = min(si + Li, sj + Lj) - sj
                perc = 100 if sj + Lj <= si + Li else 99
                rows.append(f"{i + 1}\t{j + 1}\t{sj - si}\t-\t-\t{sign(fi)}\t{sign(fj)}\t{perc}\t-\t{ov}\t-\ts\ts")
                if sj + Lj > si + Li and rng.random() < 0.3:       # the same overlap read from the other end
                    rows.append(f"{j + 1}\t{i + 1}\t{sj + Lj - si - Li}\t-\t-\t{sign(not fj)}\t{sign(not fi)}\t{perc}\t-\t{ov}\t-\ts\ts")
                if rng.random() < 0.05 and sj - si > 1:           # one base off
                    rows.append(f"{i + 1}\t{j + 1}\t{sj - si - 1}\t-\t-\t{sign(fi)}\t{sign(fj)}\t{perc}\t-\t{ov}\t-\ts\ts")
    rng.shuffle(rows)
    ovf = tmp_path / f"{name}.savage"
    ovf.write_text("\n".join(rows) + "\n")
    return str(fq), str(ovf), len(rows)


def test_synthetic_1e5_edges(tmp_path):
    """(c) >= 1e5 edges; edge_threshold 0.999 and merge_contigs 0.004 make both edge rules fire."""
    fq, ov, n_rows = _synthetic(tmp_path, 5, 4, 60000, 30, "c")
    assert n_rows > 100000
    st = _compare(tmp_path, fq, ov, "c", scores="lib", min_overlap_len=100, edge_threshold=0.999, merge_contigs=0.004)
    assert st["edges_built"] >= 100000 and st["duplicates"] > 1000 and st["transitive"] > 0 and st["inclusions"] > 0
    d = str(tmp_path / "c_lib")
    assert st["edges_final"] == open(os.path.join(d, "digraph.txt")).read().count("\n")
    g = open(os.path.join(d, "graph.txt")).read().split("\n")[:-1]
    assert int(g[1]) == len(g) - 2
    from hylight_amd import api
    cands, _, _ = api.vq_parse_overlaps(ov, 100, 0)
    sc = _lib_scores(api, fq, ov, min_overlap_len=100)
    assert sum(s > 0.999 for s, _, _ in sc) > 1000 and sum(s <= 0.999 and 0 < mr <= 0.004 for s, mr, _ in sc) > 100


@pytest.mark.parametrize("remove_trans", [2, 3])
def test_synthetic_double_and_triple_transitive(tmp_path, remove_trans):
    """(d) --remove_trans 2 / 3 (no branch removal)."""
    fq, ov, _ = _synthetic(tmp_path, 9, 2, 15000, 40, "d")
    st = _compare(tmp_path, fq, ov, "d", scores="lib", min_overlap_len=100, edge_threshold=0.999, merge_contigs=0.004,
                  remove_trans=remove_trans, remove_branches=False)
    assert st["transitive"] > 0


def test_stageb_through_driver_and_cli(tmp_path):
    """(e) the stage-b defaults: driver.extend_con(..., stageb_graph=True) on a small contigs FASTA, then the CLI on the
    same files; both against the model."""
    from hylight_amd import driver, simulate as S
    rng = random.Random(3)
    _, strains = S.simulate_reads(seed=3, n_strains=2, genome_len=30000, n_reads=1, snp_rate=0.003)
    recs = []
    for k in range(12):
        g = strains[k % 2].tobytes().decode()
        a = rng.randrange(0, 30000 - 6000)
        seq = g[a:a + rng.randint(3000, 6000)]
        if k % 3 == 0:
            seq = seq.translate(COMP)[::-1]
        recs.append(f">c{k}\n{seq}\n")
    fa = tmp_path / "all_contigs.fa"
    fa.write_text("".join(recs))
    tmp = tmp_path / "tmp"
    tmp.mkdir()
    n = driver.extend_con(str(fa), str(tmp), str(tmp_path / "final_contigs.fa"), stageb_graph=True)
    assert n == 12 and not (tmp_path / "final_contigs.fa").exists()
    sb = tmp / "stageb"
    fq, ov = str(sb / "fastq" / "singles.fastq"), str(sb / "sfoverlap.out.savage")
    want = M.graph(fq, ov, str(tmp_path / "model"))
    got_files, want_files = _files(str(sb)), _files(str(tmp_path / "model"))
    assert got_files == want_files and want["edges_built"] > 0
    r = subprocess.run([sys.executable, "-m", "hylight_amd.vq_graph", "--singles", fq, "--overlaps", ov, "--out",
                        str(tmp_path / "cli")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().split("\n")[-1]) == want
    assert _files(str(tmp_path / "cli")) == want_files


def test_refusals(tmp_path):
    from hylight_amd import api
    fq = tmp_path / "singles.fastq"
    fq.write_text("@1\nACGTACGTAC\n+\n==========\n@2\nACGTACGTAC\n+\n==========\n")
    ov = tmp_path / "ov.savage"
    ov.write_text("1\t2\t1\t2\t1\t+\t+\t90\t90\t400\t400\tp\tp\n")
    with pytest.raises(api.HlmiError) as e:
        api.vq_graph(str(fq), str(ov), str(tmp_path / "o"))
    assert e.value.code == -6
    ov.write_text("1\t2\t1\t-\t-\t+\t+\t90\t-\t400\t-\ts\ts\n")
    with pytest.raises(api.HlmiError) as e:
        api.vq_graph(str(fq), str(ov), str(tmp_path / "o"), remove_trans=2)
    assert e.value.code == -6
