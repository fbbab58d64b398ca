"""GPU: the parts of hlmi_vq_iteration that a clean tiling never reaches, each against tests/vq_next_model.py in every file
and stat: the hand cases of tests/test_vq_next_model.py as rows of a real read set, graphs with inclusions, tips, branches,
back edges, non-edge rows over existing edges and failing owners, inclusion lists of every size the pair kernel treats
differently, every (overlap_len, len) of the single-precision percentage, and the driver with and without --stageb_native.

merge_contigs 1.0 makes every scored candidate an edge (its mismatch rate is known and <= 1, EdgeCalculator.cpp:389-419),
so a graph's shape is the rows' alone; reads are random, overlaps are 40 of 1 000 bases so that a merged pair's N stay
under 5 %."""
import os
import random

import numpy as np
import pytest

import vq_next_model as N  # noqa: E402
from test_gpu_vq_next import _compare, _genome, _reads  # noqa: E402

pytestmark = pytest.mark.gpu


def _row(a, b, pos1, length, perc=50, o1="+", o2="+"):
    return f"{a}\t{b}\t{pos1}\t-\t-\t{o1}\t{o2}\t{perc}\t-\t{length}\t-\ts\ts"


def _lines(tmp_path, name):
    return open(tmp_path / (name + "_lib") / "overlaps.txt").read().split("\n")[:-1]


def test_hand_cases_as_rows(tmp_path):
    """The tables of tests/test_vq_next_model.py from real reads (read ids = vertex + 1): reads 5 -> 3 (vertices 4, 2) merge
    into super-read 1 of 300 bases with vertex 2 at offset 50, reads 4 -> 9 (vertices 3, 8) - the merge list's first pair -
    into super-read 0 of 200 bases with vertex 8 at offset 20; vertex 5 is too short to keep (visited, no super-read); the others stay copies, new ids 2
    (vertex 0, 100 bases), 3 (vertex 1, 120 bases), 4, 5.  Every hand case is then a non-edge row, in this file order -
    the lines are those of the CPU tests with these ids."""
    g, h, r = _genome(300, 1), _genome(200, 2), _genome(2000, 3)
    seqs = [r[0:100], r[100:220], g[50:300], h[0:200], g[0:200], r[300:350], r[400:800], r[900:1300], h[20:120]]
    fq = _reads(tmp_path, seqs)
    rows = [_row(5, 3, 50, 150), _row(4, 9, 20, 100),
            _row(1, 2, 10, 90, perc=80),                 # copied (:47-72)
            _row(1, 3, 20, 9),                           # u -> super-read, -30: "1 2 30 .. 100 .. 100"
            _row(3, 2, 200, 9),                          # super-read -> v, 250: "1 3 250 .. 41 .. 50"
            _row(3, 4, 100, 9, o1="-"),                  # both, 150: "1 0 150 .. 75 .. 150"; '-' against the label
            _row(9, 3, 30, 9),                           # the same key later, position zero: dropped (:261-273)
            _row(3, 5, 10, 9),                           # over the edge 5 -> 3: checkEdge > 0, left out (:694)
            _row(1, 6, 10, 9), _row(6, 1, 10, 9), _row(3, 6, 10, 9),          # visited without a super-read
            _row(7, 3, 450, 9), _row(7, 5, 10, 9),       # the owner of (1, 4) fails: 450 - 50 >= 400; the later row is dropped
            _row(8, 3, 449, 9),                          # new_pos1 == len - 1: one base
            _row(1, 2, 10, 90, perc=80),                 # the same line twice
            _row(7, 8, 5, 9, perc=100)]                  # percentage 100, copied
    ov = tmp_path / "rows.savage"
    ov.write_text("\n".join(rows) + "\n")
    o = dict(min_overlap_len=100, keep_singletons=100)
    got = _compare(tmp_path, fq, str(ov), "h", **o)
    lines = _lines(tmp_path, "h")
    assert got[1]["merged"] == 2 and got[1]["short_reads"] == 1
    for want in ("2\t3\t10\t0\t-\t+\t+\t80\t0\t90\t0\ts\ts", "1\t2\t30\t0\t-\t+\t+\t100\t0\t100\t0\ts\ts",
                 "1\t3\t250\t0\t-\t+\t+\t41\t0\t50\t0\ts\ts", "1\t0\t150\t0\t-\t-\t+\t75\t0\t150\t0\ts\ts",
                 "5\t1\t399\t0\t-\t+\t+\t0\t0\t1\t0\ts\ts", "4\t5\t5\t0\t-\t+\t+\t100\t0\t9\t0\ts\ts"):
        assert want in lines, want
    assert got[2]["claims_failed"] == 1 and not any(l.startswith(("1\t4\t", "4\t1\t")) for l in lines)
    assert got[2]["nonedge_skipped"] == 1
    assert got[2]["copied"] == 3 and got[2]["lines"] == len(lines) == 6
    got = _compare(tmp_path, fq, str(ov), "hn", no_inclusion_overlaps=1, **o)
    assert got[2]["lines"] == 4 and not any(l.split("\t")[7] == "100" for l in _lines(tmp_path, "hn"))


def _tangle(tmp_path, seed, n=70):
    """A chain with side branches, dead ends, backward rows, rows at positions behind the read (score 0, still an edge),
    contained copies with in- and out-neighbours, and short rows over and beside the edges, some behind the read's end."""
    rng = random.Random(seed)
    g = _genome(1000 * n + 1000, seed)
    seqs = [g[1000 * k:1000 * k + 1000] for k in range(n)]
    rows = []
    for k in range(n - 1):
        if k % 9 != 8:
            rows.append(_row(k + 1, k + 2, 960, 40))
    for _ in range(n // 2):
        a, b = rng.sample(range(1, n + 1), 2)
        kind = rng.random()
        if kind < 0.5:
            rows.append(_row(a, b, rng.randint(940, 990), 45, o2=rng.choice("+++-")))
        elif kind < 0.7:
            rows.append(_row(a, b, 1000 + rng.randint(0, 50), 45))                   # behind read 1: score 0
        else:
            rows.append(_row(a, b, rng.randint(0, 1100), rng.randint(1, 29)))        # a non-edge row
    edges = [r.split("\t")[:2] for r in rows if int(r.split("\t")[9]) >= 30]
    for a, b in rng.sample(edges, len(edges) // 3):                                   # non-edge rows over existing edges
        rows.append(_row(*rng.choice([(a, b), (b, a)]), rng.randint(0, 1100), rng.randint(1, 29), o1=rng.choice("+-")))
    for c in range(4):                                                                # contained copies
        parent = rng.randint(1, n)
        seqs.append(seqs[parent - 1][300:700])
        cid = len(seqs)
        rows.append(_row(parent, cid, 300, 400, perc=100))
        for _ in range(rng.randint(1, 4)):
            rows.append(_row(rng.randint(1, n), cid, rng.randint(600, 960), 40))
        for _ in range(rng.randint(1, 4)):
            rows.append(_row(cid, rng.randint(1, n), rng.randint(360, 390), 35))
    rng.shuffle(rows)
    ov = tmp_path / "tangle.savage"
    ov.write_text("\n".join(rows) + "\n")
    return _reads(tmp_path, seqs), str(ov)


def test_every_source_and_every_check(tmp_path):
    """Three seeded tangles; together every origin, both checkEdge tests in both outcomes and a failing owner occur."""
    total = dict.fromkeys(N.STATS, 0)
    tips = branches = back = 0
    for seed in (1, 2, 3):
        fq, ov = _tangle(tmp_path, seed)
        g = _compare(tmp_path, fq, ov, f"t{seed}", min_overlap_len=30, keep_singletons=300, merge_contigs=1.0)
        for k in N.STATS:
            total[k] += g[2][k]
        tips, branches, back = tips + g[0]["tip_edges"], branches + g[0]["branch_edges"], back + g[0]["backedges"]
    assert all(total[k] > 0 for k in N.STATS), total
    assert tips > 0 and branches > 0 and back > 0
    assert total["src_branching"] == tips + branches + back


@pytest.mark.parametrize("size", [0, 1, 2, 3, 64, 65, 300])
def test_inclusion_list_sizes(tmp_path, size):
    """One included read with `size` edges: the inclusion edge, then in- and out-neighbours in turn.  Size 0: the
    inclusion edge is marked by a first candidate and the pair's later, better candidate replaces it in the other
    direction's orientation class - no: with no other edge the list holds one edge, so size 0 is a read set without an
    included read (no list at all), the kernel's no-pair path."""
    n_in, n_out = (max(size - 1, 0) + 1) // 2, max(size - 1, 0) // 2
    g = _genome(1000 * (n_in + n_out + 2), 9)
    seqs = [g[0:1000]] + ([g[300:700]] if size else [g[1000:1400]])
    rows = [_row(1, 2, 300, 400, perc=100 if size else 50)]
    for k in range(n_in + n_out):
        seqs.append(g[1000 * (k + 1):1000 * (k + 2)])
        rows.append(_row(k + 3, 2, 960, 40) if k < n_in else _row(2, k + 3, 360, 40))
    ov = tmp_path / "incl.savage"
    ov.write_text("\n".join(rows) + "\n")
    got = _compare(tmp_path, _reads(tmp_path, seqs), str(ov), "i", min_overlap_len=30, keep_singletons=300, merge_contigs=1.0)
    assert got[2]["src_induced"] == (n_in + 1) * n_out if size else got[2]["src_induced"] == 0
    assert got[0]["inclusions"] == (1 if size else 0)


def test_percentage_every_overlap_and_length(tmp_path):
    """One call: reads u_L of L = 1 .. 600 bases stay copies, 600 pairs merge into super-reads of 620 bases; the non-edge
    row (u_L, first read of super-read k) at position L - k gives overlap k of length L, k = 1 .. L - 180 300 lines, each
    percentage (int)floor(k / float(L) * 100) since the super-read is the longer.  Checked against numpy.float32 line by line
    (the model's parsers need half a minute for these rows; its percentage is the same three numpy.float32 steps)."""
    from hylight_amd import api
    K = 600
    g = _genome(640 * K + 310 * K, 4)
    seqs, rows = [], []
    for k in range(K):
        seqs += [g[640 * k:640 * k + 320], g[640 * k + 320:640 * k + 640]]
        rows.append(_row(2 * k + 1, 2 * k + 2, 300, 20))
    base = 640 * K
    for L in range(1, K + 1):
        seqs.append(g[base:base + L])
        base += L
        rows += [_row(2 * K + L, 2 * k - 1, L - k, 1) for k in range(1, L + 1)]
    ov = tmp_path / "perc.savage"
    ov.write_text("\n".join(rows) + "\n")
    got = api.vq_iteration(_reads(tmp_path, seqs), str(ov), str(tmp_path / "p_lib"), min_overlap_len=20, keep_singletons=1,
                           merge_contigs=1.0)
    assert got[1]["merged"] == K and got[2]["u2sr"] == got[2]["lines"] == K * (K + 1) // 2
    seen = set()
    for l in _lines(tmp_path, "p"):
        f = l.split("\t")
        L, k = int(f[0]) - K + 1, int(f[9])                   # u_L is new read K + L - 1
        assert 0 <= int(f[1]) < K and f[3:7] == ["0", "-", "+", "+"] and f[8:] == ["0", str(k), "0", "s", "s"], l
        assert int(f[2]) == L - k and int(f[7]) == int(np.floor(np.float32(k) / np.float32(L) * np.float32(100))), l
        seen.add((k, L))
    assert len(seen) == K * (K + 1) // 2


def _driver_inputs(tmp_path, monkeypatch):
    from hylight_amd import simulate as S
    reads, strains = S.simulate_reads(seed=83, n_strains=2, genome_len=30000, n_reads=90, mean_len=9000, min_len=7000,
                                      max_len=14000)
    lfq, sfq = tmp_path / "long.fq", tmp_path / "short.fq"
    S.write_fastq(reads, lfq)
    S.write_fastq(S.simulate_short_pairs(84, strains, 2500, read_len=150), sfq)
    bin_dir = tmp_path / "bin"
    bin_dir.mkdir()
    racon = bin_dir / "racon"                                  # external: a stub that leaves the contigs unchanged
    racon.write_text('#!/bin/sh\ncat "$7"\n')
    racon.chmod(0o755)
    monkeypatch.setenv("PATH", f"{bin_dir}:{os.environ['PATH']}")
    return ["-l", str(lfq), "-s", str(sfq), "-o", str(tmp_path / "OUT"), "--corrected", "--nsplit", "3", "-t", "4"]


def _want_final(sb, tmp_path):
    """The model's loop on the driver's own stage-b inputs -> (the text of final_contigs.fa, the loop's counts)."""
    want = N.stageb(str(sb / "fastq"), str(sb / "sfoverlap.out.savage"), str(tmp_path / "model"))
    merged = tmp_path / "model" / "singles.fastq"              # absent when the first graph has no edge
    N.fastq2fasta(str(merged if merged.exists() else sb / "fastq" / "singles.fastq"), str(tmp_path / "want.fa"))
    return open(tmp_path / "want.fa").read(), want


def test_driver_stageb_native(tmp_path, monkeypatch):
    """The whole driver with the flag: exit status 0 and final_contigs.fa equal to the model's."""
    from hylight_amd import driver
    args = _driver_inputs(tmp_path, monkeypatch)
    assert driver.main(args + ["--stageb_native"]) == 0
    text, _ = _want_final(tmp_path / "OUT" / "tmp" / "stageb", tmp_path)
    final = open(tmp_path / "OUT" / "final_contigs.fa").read()
    assert final == text and final.startswith(">")


def test_extend_con_stageb_native_merges(tmp_path):
    """extend_con on contigs that do overlap (the set of test_gpu_vq_merge.py's driver test): the loop runs, and
    final_contigs.fa and the stage-b files equal the model's."""
    from hylight_amd import driver, simulate as S
    rng = random.Random(3)
    _, strains = S.simulate_reads(seed=3, n_strains=2, genome_len=30000, n_reads=1, snp_rate=0.003)
    recs = []
    for k in range(12):
        g = strains[k % 2].tobytes().decode()
        a = rng.randrange(0, 30000 - 6000)
        seq = g[a:a + rng.randint(3000, 6000)]
        if k % 3 == 0:
            seq = seq.translate(str.maketrans("ACGT", "TGCA"))[::-1]
        recs.append(f">c{k}\n{seq}\n")
    fa = tmp_path / "all_contigs.fa"
    fa.write_text("".join(recs))
    tmp = tmp_path / "tmp"
    tmp.mkdir()
    assert driver.extend_con(str(fa), str(tmp), str(tmp_path / "final_contigs.fa"), stageb_native=True) == 12
    sb = tmp / "stageb"
    text, want = _want_final(sb, tmp_path)
    assert open(tmp_path / "final_contigs.fa").read() == text and want["edges"][0] > 0 and want["reads"][0] < 12
    for n in ("singles.fastq", "subreads.txt", "overlaps.txt", "stats.txt", "removed_tip_sequences.fastq"):
        assert open(sb / n, "rb").read() == open(tmp_path / "model" / n, "rb").read(), n


def test_driver_without_the_flag(tmp_path, monkeypatch):
    from hylight_amd import driver
    args = _driver_inputs(tmp_path, monkeypatch)
    assert driver.main(args) == driver.EXIT_NO_FINAL == 3
    assert not (tmp_path / "OUT" / "final_contigs.fa").exists()
    sb = tmp_path / "OUT" / "tmp" / "stageb"
    assert (sb / "sfoverlap.out.savage").exists() and not (sb / "overlaps.txt").exists()      # stage b was reached, not run
