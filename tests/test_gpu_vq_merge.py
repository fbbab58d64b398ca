"""GPU: hlmi_vq_merge and hlmi_vq_consensus_pair (SRBuilder::mergeAlongEdges for HyLight's stage b) against the model in
tests/vq_merge_model.py, byte for byte on every output file and field for field on the stats.  PARITY UNPINNED: the
reference needs Boost and cannot be built here; tests/test_vq_merge_model.py holds the model to hand-worked answers.

pos == len1 joins the two reads: read 2 turns active (SRBuilder.cpp:455-459) at the very position read 1 has just left
(:487-492); pos == len1 + 1 is the first position that leaves a gap and gives an empty consensus (:498-501).  Both are
asserted here, against the model and by hand."""
import json
import os
import random
import re
import subprocess
import sys

import pytest

import vq_graph_model as M  # noqa: E402
import vq_merge_model as MM  # noqa: E402
import test_vq_merge_model as T  # noqa: E402
from test_gpu_vq_graph import HAND, _lib_scores, _random_reads  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
COMP = str.maketrans("ACGT", "TGCA")
INT_STATS = MM.STATS


def _kernel_constants():
    src = open(os.path.join(ROOT, "hylight_amd", "csrc", "vq_internal.h")).read()
    body = src[src.index("namespace vqm {"):]
    return {k: int(re.search(rf"constexpr int {k} = (\d+);", body).group(1)) for k in ("WG", "WAVE", "SPAN")}


def _files(d, names):
    return {n: open(os.path.join(d, n), "rb").read() for n in names if os.path.exists(os.path.join(d, n))}


def _compare(tmp_path, fq, ov, name, scores=None, subreads_in=None, **opts):
    """vq_merge against the model (and its graph files against vq_graph's own) -> (graph stats, merge stats)."""
    from hylight_amd import api
    lib_dir, model_dir, graph_dir = (str(tmp_path / (name + s)) for s in ("_lib", "_model", "_graph"))
    gopts = {k: v for k, v in opts.items() if k not in MM.MERGE}
    ggot, mgot = api.vq_merge(fq, ov, lib_dir, subreads_in=subreads_in, **opts)
    if scores == "lib":
        scores = _lib_scores(api, fq, ov, **gopts)
    gwant, mwant = MM.merge(fq, ov, model_dir, subreads_in=subreads_in, scores=scores, **opts)
    names = M.OUTPUTS + MM.OUTPUTS
    got, want = _files(lib_dir, names), _files(model_dir, names)
    assert sorted(got) == sorted(want)
    for n in want:
        assert got[n] == want[n], n
    assert ggot == gwant
    assert {k: mgot[k] for k in INT_STATS} == mwant and mgot["ms_merge"] >= 0
    assert api.vq_graph(fq, ov, graph_dir, **gopts) == ggot                   # the graph files: hlmi_vq_graph's, unchanged
    assert _files(graph_dir, M.OUTPUTS) == _files(lib_dir, M.OUTPUTS)
    return ggot, mgot


def _all_cases():
    """Every (base1, q1, base2, q2) as two sequences of 220 900 positions."""
    s1, q1, s2, q2 = [], [], [], []
    Q = [chr(33 + q) for q in range(94)]
    for b1 in "ACGTN":
        for b2 in "ACGTN":
            for a in Q:
                s1.append(b1 * 94); q1.append(a * 94); s2.append(b2 * 94); q2.append("".join(Q))
    return "".join(s1), "".join(q1), "".join(s2), "".join(q2)


@pytest.fixture(scope="module")
def all_cases():
    return _all_cases()


@pytest.mark.parametrize("pos", [0, 1000])
def test_consensus_pair_every_base_and_quality(all_cases, pos):
    """pos 0: every case against its partner; pos 1000: the same sequences shifted, so the cases straddle the kernel's
    spans differently and the ends are single bases."""
    from hylight_amd import api
    s1, q1, s2, q2 = all_cases
    assert len(s1) == 220900 and len({(a, b, c, d) for a, b, c, d in zip(s1, q1, s2, q2)}) == 220900
    got = api.vq_consensus_pair(s1, q1, s2, q2, pos)
    want = MM.consensus_pair(s1, q1, s2, q2, pos)
    assert len(got[0]) == 220900 + pos
    assert got == want


def _rand_read(rng, n):
    return ("".join(rng.choice("ACGTN" if rng.random() < 0.1 else "ACGT") for _ in range(n)),
            "".join(chr(33 + rng.choice((0, 1, 2, 20, 31, 40, 93))) for _ in range(n)))


def test_consensus_pair_borders():
    from hylight_amd import api
    K = _kernel_constants()
    assert K["SPAN"] % K["WG"] == 0 and K["WG"] % K["WAVE"] == 0
    rng = random.Random(11)
    cases = []
    for e in (K["WAVE"] - 1, K["WAVE"], K["WAVE"] + 1, K["WG"] - 1, K["WG"], K["WG"] + 1, K["SPAN"] - 1, K["SPAN"], K["SPAN"] + 1,
              2 * K["SPAN"] - 1, 2 * K["SPAN"], 2 * K["SPAN"] + 1):
        cases.append((e + 5, 10, e))                 # the first overlapping base at e
        cases.append((e + 1, e + 20, 3))             # the last overlapping base at e (read 1 ends there)
        cases.append((e + 30, e - 2, 3))             # ... read 2 ends there (contained)
    cases += [(50, 20, 49), (50, 20, 50), (1, 1, 0), (1, 1, 1), (K["SPAN"], K["SPAN"], K["SPAN"] - 1), (K["SPAN"], 1, K["SPAN"])]
    for len1, len2, pos in cases:
        (s1, q1), (s2, q2) = _rand_read(rng, len1), _rand_read(rng, len2)
        got = api.vq_consensus_pair(s1, q1, s2, q2, pos)
        assert got == MM.consensus_pair(s1, q1, s2, q2, pos), (len1, len2, pos)
        assert len(got[0]) == max(len1, pos + len2)
    (s1, q1), (s2, q2) = _rand_read(rng, 50), _rand_read(rng, 20)
    assert len(api.vq_consensus_pair(s1, q1, s2, q2, 50)[0]) == 70        # pos == len1: joined (the module's note)
    assert api.vq_consensus_pair(s1, q1, s2, q2, 51) == ("", "")          # pos == len1 + 1: a position without a base
    assert api.vq_consensus_pair(s1, q1[:49], s2, q2, 10) == ("", "")      # a quality string shorter than its sequence
    assert api.vq_consensus_pair(s1, q1, s2, q2[:19], 10) == ("", "")
    assert api.vq_consensus_pair(s1, q1, "", "", 10) == ("", "")
    assert api.vq_consensus_pair("", "", s2, q2, 0) == ("", "")
    with pytest.raises(api.HlmiError):
        api.vq_consensus_pair("ACGR", "IIII", "AC", "II", 1)
    with pytest.raises(api.HlmiError):
        api.vq_consensus_pair("ACGT", "II I", "AC", "II", 1)


def test_golden_savage_file(tmp_path):
    """The path's own SAVAGE file on reads synthesized for its ids (merge_contigs 1: every candidate is an edge; random
    reads disagree, so most pairs fail the N rate and come back unmerged), and with one row in ten flipped: labelling
    conflicts, reverse vertices."""
    from hylight_amd import api
    ov = os.path.join(GOLD, "fxC_v3.savage")
    ids = sorted({int(l.split("\t")[k]) for l in open(ov) for k in (0, 1)})
    fq = str(tmp_path / "singles.fastq")
    _random_reads(fq, ids, 4000, 1)
    g, m = _compare(tmp_path, fq, ov, "a", scores="lib", merge_contigs=1.0)
    assert m["pairs"] > 0 and m["pairs"] == m["merged"] + m["dropped_n"] + m["dropped_empty"]
    rng = random.Random(2)
    rows = [l.split("\t") for l in open(ov).read().split("\n")[:-1]]
    for r in rows:
        if rng.random() < 0.1:
            r[6] = "-" if r[6] == "+" else "+"
    ov2 = str(tmp_path / "flipped.savage")
    with open(ov2, "w") as f:
        f.write("".join("\t".join(r) + "\n" for r in rows))
    g, m = _compare(tmp_path, fq, ov2, "a2", scores="lib", merge_contigs=1.0, keep_singletons=1)
    assert g["conflicts"] > 0 and m["trivial_reverse"] > 0


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_made_graphs(tmp_path, case):
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


RUN_CASES = [(n, ()) for n in ("test_overlap_of_one", "test_overlap_of_300", "test_contained_read", "test_base_is_read_2_of_the_edge",
                               "test_five_percent_n", "test_keep_singletons_299_300", "test_dropped_pair_returns_as_two_trivials",
                               "test_inclusion_and_tip_go_to_the_tip_file", "test_second_iteration_with_a_reverse_vertex")]
RUN_CASES += [("test_four_orientations", tuple(a)) for a in T.test_four_orientations.pytestmark[0].args[1]]


@pytest.mark.parametrize("name,args", RUN_CASES, ids=[f"{n}{'_' + a[0] + a[1] if a else ''}" for n, a in RUN_CASES])
def test_model_hand_cases_on_the_library(tmp_path, monkeypatch, name, args):
    """The hand-made cases of tests/test_vq_merge_model.py: every run of theirs also goes through the library, whose files
    and stats must equal the model's, and their written-out bytes are then asserted on what the LIBRARY wrote."""
    from hylight_amd import api
    model_run = T._run
    calls = []

    def both(tp, reads, rows, sub=None, **o):
        g, m, f = model_run(tp, reads, rows, sub=sub, **o)
        opts = dict(min_overlap_len=1, merge_contigs=1.0, keep_singletons=1)
        opts.update(o)
        lg, lm = api.vq_merge(str(tp / "s.fastq"), str(tp / "o.savage"), str(tp / "out_lib"),
                              subreads_in=str(tp / "sub.txt") if sub is not None else None, **opts)
        lf = {n: open(os.path.join(tp / "out_lib", n)).read() for n in MM.OUTPUTS if os.path.exists(os.path.join(tp / "out_lib", n))}
        lm = {k: lm[k] for k in INT_STATS}
        assert lf == f and lg == g and lm == m
        assert _files(str(tp / "out_lib"), M.OUTPUTS) == _files(str(tp / "out"), M.OUTPUTS)
        calls.append(1)
        return lg, lm, lf

    monkeypatch.setattr(T, "_run", both)
    getattr(T, name)(tmp_path, *args)
    assert calls


def _synthetic(tmp_path, seed, n_small, big=200000):
    """n_small contigs of 151 .. 3000 bases tiling one seeded genome with overlaps of 100 .. 150 bases, three of `big` bases
    tiling another (each starts a quarter of its length behind the one before), about half stored reverse-complemented;
    every twentieth small contig carries an N run of 4 % or 6 % of its length.  Rows: the exact overlaps of neighbours.
    -> (fastq, overlaps, reads by id: (genome, start, length, stored forward))."""
    rng = random.Random(seed)
    reads = []                                                     # (sequence, start, length, genome)
    g = "".join(rng.choices("ACGT", k=big + big // 2))
    for a in (0, big // 4, big // 2):
        reads.append((g[a:a + big], a, big, 0))
    start, small, glen = 0, [], 0
    for k in range(n_small):
        L = rng.randint(151, 3000)
        small.append((start, L))
        glen = max(glen, start + L)
        start += L - rng.randint(100, min(150, L - 1))
    g2 = "".join(rng.choices("ACGT", k=glen))
    for k, (a, L) in enumerate(small):
        s = g2[a:a + L]
        if k % 20 == 7:
            n = int(L * (0.04 if k % 40 == 7 else 0.06))
            s = s[:L // 2] + "N" * n + s[L // 2 + n:]
        reads.append((s, a, L, 1))
    order = list(range(len(reads)))
    rng.shuffle(order)
    vid = {r: k + 1 for k, r in enumerate(order)}
    fwd = {r: rng.random() < 0.5 for r in order}
    fq = tmp_path / "syn.fastq"
    with open(fq, "w") as f:
        for r in order:
            s = reads[r][0] if fwd[r] else reads[r][0].translate(COMP)[::-1]
            q = "".join(rng.choices("I5=", k=len(s)))
            f.write(f"@{vid[r]}\n{s}\n+\n{q}\n")
    rows = _rows([(vid[r], reads[r][3], reads[r][1], reads[r][2], fwd[r]) for r in range(len(reads))], rng)
    ov = tmp_path / "syn.savage"
    ov.write_text("\n".join(rows) + "\n")
    return str(fq), str(ov), {vid[r]: (reads[r][3], reads[r][1], reads[r][2], fwd[r]) for r in range(len(reads))}


def _rows(items, rng, reach=2):
    """SAVAGE rows for the true overlaps of (id, genome, start, length, forward) with their next `reach` neighbours."""
    items = sorted(items, key=lambda t: (t[1], t[2], t[0]))
    sign = lambda b: "+" if b else "-"
    rows = []
    for i in range(len(items)):
        for j in range(i + 1, min(i + 1 + reach, len(items))):
            (ii, gi, ai, Li, fi), (ij, gj, aj, Lj, fj) = items[i], items[j]
            if gi != gj or aj >= ai + Li:
                continue
            ovl = min(ai + Li, aj + Lj) - aj
            rows.append(f"{ii}\t{ij}\t{aj - ai}\t-\t-\t{sign(fi)}\t{sign(fj)}\t{100 if aj + Lj <= ai + Li else 99}\t-\t{ovl}\t-\ts\ts")
    rng.shuffle(rows)
    return rows


def _second_iteration_rows(out_dir, coords, min_len=100):
    """Where the super-reads of an iteration lie on the genomes - from superread_map.txt and the first reads' own
    coordinates - and the true overlaps between them.  FindNextOverlaps is not built; the test stands in for it."""
    lines = open(os.path.join(out_dir, "singles.fastq")).read().split("\n")
    lens = [len(lines[k + 1]) for k in range(0, len(lines) - 1, 4)]
    ids = sorted(coords)                                           # vertex = position in the file = rank of the id
    place = {}
    for l in open(os.path.join(out_dir, "superread_map.txt")).read().split("\n")[:-1]:
        v, new, off, ori = l.split("\t")
        if new == "-1":
            continue
        genome, a, L, stored_fwd = coords[ids[int(v)]]
        new, off = int(new), int(off)
        forward = stored_fwd == (ori == "+")                       # the super-read shows the genome's own strand
        start = a - off if forward else a + L + off - lens[new]
        assert place.setdefault(new, (genome, start, forward)) == (genome, start, forward)
    items = [(new, g, a, lens[new], f) for new, (g, a, f) in place.items()]
    rows = [r for r in _rows(items, random.Random(1), reach=1) if int(r.split("\t")[9]) >= min_len]
    return rows, {new: (g, a, lens[new], f) for new, (g, a, f) in place.items()}


def _two_iterations(tmp_path, n_small, big, scores):
    fq, ov, coords = _synthetic(tmp_path, 7, n_small, big)
    g, m = _compare(tmp_path, fq, ov, "s1", scores=scores, min_overlap_len=100, merge_contigs=1.0)
    assert m["merged"] > n_small // 6 and m["trivial_reverse"] > 0 and m["dropped_n"] + m["n_reads"] > 0
    lib = str(tmp_path / "s1_lib")
    smap = [l.split("\t") for l in open(os.path.join(lib, "superread_map.txt")).read().split("\n")[:-1]]
    assert sum(r[3] == "-" for r in smap) > len(smap) // 4
    rows, place = _second_iteration_rows(lib, coords)
    # One labelling gives a whole component one strand, so the super-reads of a component all come out alike.  To meet
    # reverse vertices in the second iteration, every third super-read is stored reverse-complemented here, its originals
    # mirrored as a reverse copy's are (SRBuilder.cpp:1357-1363) and its row signs turned.
    lines = open(os.path.join(lib, "singles.fastq")).read().split("\n")
    subs = open(os.path.join(lib, "subreads.txt")).read().split("\n")[:-1]
    flipped = {k for k in place if k % 3 == 1}
    with open(tmp_path / "it2.fastq", "w") as f, open(tmp_path / "it2_subreads.txt", "w") as fs:
        for k in range(len(subs)):
            seq, qual, fields = lines[4 * k + 1], lines[4 * k + 3], subs[k].split("\t")
            if k in flipped:
                seq, qual = seq.translate(COMP)[::-1], qual[::-1]
                for x in range(1, len(fields)):
                    oid, ori, idx, ln = fields[x].split(":")
                    fields[x] = f"{oid}:{'-' if ori == '+' else '+'}:{len(seq) - (int(idx) + int(ln))}:{ln}"
            f.write(f"@{k}\n{seq}\n+\n{qual}\n")
            fs.write("\t".join(fields) + "\n")
    turn = lambda i, sg: ("-" if sg == "+" else "+") if int(i) in flipped else sg
    rows = ["\t".join(r[:5] + [turn(r[0], r[5]), turn(r[1], r[6])] + r[7:]) for r in (x.split("\t") for x in rows)]
    ov2 = tmp_path / "it2.savage"
    ov2.write_text("\n".join(rows) + "\n")
    g, m = _compare(tmp_path, str(tmp_path / "it2.fastq"), str(ov2), "s2", scores=scores,
                    subreads_in=str(tmp_path / "it2_subreads.txt"), first_it=False, min_overlap_len=100, merge_contigs=1.0)
    assert m["merged"] > n_small // 20                              # true overlaps: the non-first_it merged branch runs
    smap = [l.split("\t") for l in open(os.path.join(tmp_path / "s2_lib", "superread_map.txt")).read().split("\n")[:-1]]
    shared = {}
    for r in smap:
        shared.setdefault(r[1], []).append(r[3])
    assert any(k != "-1" and len(v) == 2 and "-" in v for k, v in shared.items())      # a reverse vertex inside a merged pair
    sub2 = open(os.path.join(tmp_path / "s2_lib", "subreads.txt")).read()
    assert max(l.count("\t") for l in sub2.split("\n")) >= 4       # originals carried through two merges


def test_synthetic_two_iterations(tmp_path):
    """About 2 000 contigs of 151 .. 3 000 bases and three of 200 kb; then a second iteration on the first one's super-reads
    and subreads.txt with their true overlaps."""
    _two_iterations(tmp_path, 2000, 200000, "lib")


def test_refusals(tmp_path):
    from hylight_amd import api
    fq = tmp_path / "singles.fastq"
    fq.write_text("@1\nACGTACGTAC\n+\n==========\n@2\nACGTACGTAC\n+\n==========\n")
    ov = tmp_path / "ov.savage"
    ov.write_text("1\t2\t1\t2\t1\t+\t+\t90\t90\t400\t400\tp\tp\n")
    with pytest.raises(api.HlmiError) as e:
        api.vq_merge(str(fq), str(ov), str(tmp_path / "o"))
    assert e.value.code == -6
    ov.write_text("1\t2\t1\t-\t-\t+\t+\t90\t-\t9\t-\ts\ts\n")              # too short for an edge: no graph, no merge
    g, m = api.vq_merge(str(fq), str(ov), str(tmp_path / "o2"))
    assert g["edges_built"] == 0 and m["pairs"] == 0
    assert not any(os.path.exists(tmp_path / "o2" / n) for n in MM.OUTPUTS)
    with pytest.raises(api.HlmiError):                                    # first_it off without a subreads file
        api.vq_merge(str(fq), str(ov), str(tmp_path / "o3"), first_it=False)


def test_driver_and_cli(tmp_path):
    """--stop_after stageb_merge on a small read set: exit status 3 and the four files in tmp/stageb/; then the CLI on
    the same files equals the API and the model."""
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
    n = driver.extend_con(str(fa), str(tmp), str(tmp_path / "final_contigs.fa"), stageb_merge=True)
    assert n == 12 and not (tmp_path / "final_contigs.fa").exists()
    sb = tmp / "stageb"
    fq, ov = str(sb / "fastq" / "singles.fastq"), str(sb / "sfoverlap.out.savage")
    gwant, mwant = MM.merge(fq, ov, str(tmp_path / "model"))
    names = M.OUTPUTS + MM.OUTPUTS
    want_files = _files(str(tmp_path / "model"), names)
    assert _files(str(sb), names) == want_files and gwant["edges_built"] > 0
    assert all(n in want_files for n in ("singles.fastq", "subreads.txt", "superread_map.txt"))
    r = subprocess.run([sys.executable, "-m", "hylight_amd.vq_merge", "--singles", fq, "--overlaps", ov, "--out",
                        str(tmp_path / "cli")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().split("\n")[-1])
    assert out["graph"] == gwant and {k: out["merge"][k] for k in INT_STATS} == mwant
    assert _files(str(tmp_path / "cli"), names) == want_files


def test_driver_stop_after_stageb_merge(tmp_path, monkeypatch):
    """The whole driver on the small hybrid set of tests/test_gpu_cluster_driver.py (racon is external: a stub that
    leaves the contigs unchanged stands in for it, as there): exit status 3 (EXIT_NO_FINAL), no final_contigs.fa, and
    tmp/stageb/ holds what the model writes from the driver's own stage-b inputs."""
    from hylight_amd import driver, simulate as S
    reads, strains = S.simulate_reads(seed=83, n_strains=2, genome_len=30000, n_reads=90, mean_len=9000, min_len=7000,
                                      max_len=14000)
    lfq, sfq = tmp_path / "long.fq", tmp_path / "short.fq"
    S.write_fastq(reads, lfq)
    S.write_fastq(S.simulate_short_pairs(84, strains, 2500, read_len=150), sfq)
    bin_dir = tmp_path / "bin"
    bin_dir.mkdir()
    racon = bin_dir / "racon"
    racon.write_text('#!/bin/sh\ncat "$7"\n')
    racon.chmod(0o755)
    monkeypatch.setenv("PATH", f"{bin_dir}:{os.environ['PATH']}")
    out = tmp_path / "OUT"
    assert driver.main(["-l", str(lfq), "-s", str(sfq), "-o", str(out), "--corrected", "--nsplit", "3", "-t", "4",
                        "--stop_after", "stageb_merge"]) == driver.EXIT_NO_FINAL == 3
    assert not (out / "final_contigs.fa").exists()
    sb = out / "tmp" / "stageb"
    names = M.OUTPUTS + MM.OUTPUTS
    MM.merge(str(sb / "fastq" / "singles.fastq"), str(sb / "sfoverlap.out.savage"), str(tmp_path / "model"))
    assert (sb / "sfoverlap.out.savage").exists()
    assert _files(str(sb), names) == _files(str(tmp_path / "model"), names)
