"""GPU: hlmi_vq_branch_graph / hlmi_vq_branch_iteration against tests/vq_branch_model.py - every file of out_dir byte for byte,
branch_components.txt among them, and every counter.  The inputs are built here, at the smallest shapes where the two kernels can
go wrong; what an input has to reach is asserted from the model, never from the library."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_branch_model as B  # noqa: E402
import vq_clique_inputs as I  # noqa: E402
import vq_clique_model as CM  # noqa: E402
import vq_clique_next_model as CN  # noqa: E402
import vq_graph_model as M  # noqa: E402
from test_gpu_vq_graph import _lib_scores  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = M.OUTPUTS + ("branch_components.txt",)
# every row an edge (merge_contigs 1), nothing reduced but what the branch reduction needs
HAND = dict(min_overlap_len=1, merge_contigs=1.0, remove_trans=1, remove_branches=False, remove_tips=False, ignore_inclusions=False)
RNG = random.Random(17)
GENOME = "".join(RNG.choice("ACGT") for _ in range(4000))
COMP = str.maketrans("ACGT", "TGCA")
Q = "I"


def rc(s):
    return s.translate(COMP)[::-1]


def mutate(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def write_case(d, reads, rows, oreads=None, subreads=None, table=None):
    """reads: sequences (id = position); rows: (u, v, pos1[, ori1, ori2]); oreads: the original FASTQ's sequences (default: the
    reads themselves, first_it); subreads: {read: [(original, forward, index, len)]}; table: {dist: min evidence}."""
    os.makedirs(d, exist_ok=True)
    p = lambda n: os.path.join(d, n)
    with open(p("singles.fastq"), "w") as f:
        f.write("".join(f"@{k}\n{s}\n+\n{Q * len(s)}\n" for k, s in enumerate(reads)))
    with open(p("overlaps.txt"), "w") as f:
        for r in rows:
            u, v, pos = r[:3]
            o1, o2 = (r[3], r[4]) if len(r) > 3 else ("+", "+")
            n = min(len(reads[u]) - pos, len(reads[v]))
            f.write(f"{u}\t{v}\t{pos}\t-\t-\t{o1}\t{o2}\t{100 * n // min(len(reads[u]), len(reads[v]))}\t-\t{n}\t-\ts\ts\n")
    with open(p("original.fastq"), "w") as f:
        f.write("".join(f"@{k}\n{s}\n+\n{Q * len(s)}\n" for k, s in enumerate(oreads if oreads is not None else reads)))
    sub = None
    if subreads is not None:
        sub = p("subreads_in.txt")
        with open(sub, "w") as f:
            for v in range(len(reads)):
                f.write(str(v) + "".join(f"\t{o}:{'+' if fw else '-'}:{idx}:{ln}" for o, fw, idx, ln in sorted(subreads[v])) + "\n")
    with open(p("table.tsv"), "w") as f:
        f.write("# dist\tfraction\tmin_evidence\n" + "".join(f"{k}\t0\t{v}\n" for k, v in sorted((table or {}).items())))
    return p("singles.fastq"), p("overlaps.txt"), p("original.fastq"), sub, p("table.tsv")


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in NAMES if os.path.exists(os.path.join(d, n))}


def compare(tmp_path, reads, rows, oreads=None, subreads=None, table=None, se=None, pe=0, careful=True, **opts):
    from hylight_amd import api
    fq, ov, ofq, sub, tab = write_case(str(tmp_path / "in"), reads, rows, oreads, subreads, table)
    se = (len(oreads) if oreads is not None else len(reads)) - 2 * pe if se is None else se
    o = dict(HAND, **opts)
    lib_dir, model_dir = str(tmp_path / "lib"), str(tmp_path / "model")
    scores = _lib_scores(api, fq, ov, min_overlap_len=o["min_overlap_len"])
    gwant, bwant = B.branch_graph(fq, ov, sub, ofq, tab, model_dir, se, pe, careful, first_it=sub is None, scores=scores, **o)
    ggot, bgot = api.vq_branch_graph(fq, ov, ofq, tab, lib_dir, subreads_in=sub, se_count=se, pe_count=pe, careful=careful, **o)
    a, b = _files(lib_dir), _files(model_dir)
    print("branch stats", bgot, bwant)
    assert sorted(a) == sorted(b) and "branch_components.txt" in a
    for n in b:
        assert a[n] == b[n], n
    assert ggot == gwant and {k: bgot[k] for k in B.STATS} == bwant
    return bwant, b["branch_components.txt"].decode()


def out_branch(n, diffs, lead=20, third=None):
    """Vertex 0 and two (three) neighbours behind `lead` bases of it, sharing a stretch of n bases that differs at `diffs`."""
    g = GENOME[:lead + n]
    reads = [g, g[lead:], mutate(g[lead:], diffs)]
    rows = [(0, 1, lead), (0, 2, lead)]
    if third is not None:
        reads.append(mutate(g[lead:], third))
        rows.append((0, 3, lead))
    return reads, rows


def in_branch(n, diffs, tail=20):
    """Two neighbours that end in vertex 0: each n bases, the last of them shared with 0's first; compared reversed."""
    g = GENOME[100:100 + n + tail]
    reads = [g[n - 1:], g[:n], mutate(g[:n], diffs)]
    return reads, [(1, 0, n - 1), (2, 0, n - 1)]


def in_branch_one_base():
    """An in-branch whose common stretch is one base.  A one-base in-neighbour can only lie at position 0, and a row at position
    0 runs from the smaller vertex, so the branching vertex is the largest: 0 (50 bases) -> 2 at 30, 1 (one base) -> 2 at 0.
    startpos 0 and 30, relative_pos 30, len min(50 - 30, 1) = 1: base 30 of read 0 against the base of read 1, which differs."""
    g = GENOME[300:400]
    return [g[:50], mutate(g[30], [0]), g[30:90]], [(0, 2, 30), (1, 2, 0)]


@pytest.mark.parametrize("kind,n", [(k, n) for k in ("out", "in") for n in (1, 63, 64, 65, 129)])
def test_common_stretch_lengths(tmp_path, n, kind):
    """One mismatch in the last compared base of a stretch of n: the end of a step, one step and one base, two steps and one."""
    if kind == "in" and n == 1:
        reads, rows = in_branch_one_base()
    else:
        reads, rows = out_branch(n, [n - 1]) if kind == "out" else in_branch(n, [0])
    st, _ = compare(tmp_path, reads, rows, table={k: 0 for k in range(600)})
    assert st["pairs"] == 1 and st["diff_positions"] == 1 and st[kind + "_branches"] == 1 and st["missing_edges"] == 0


@pytest.mark.parametrize("lane", [0, 63])
@pytest.mark.parametrize("kind", ["out", "in"])
def test_hundredth_mismatch_at_a_lane_with_one_behind_it(tmp_path, kind, lane):
    """99 mismatches in the first two steps, the 100th at `lane` of the third step (compare position 128 + lane) and a 101st
    behind it: 100 positions are kept."""
    n = 260
    at = list(range(0, 99)) + [128 + lane, 128 + lane + 1 if lane == 0 else 250]
    if kind == "out":
        reads, rows = out_branch(n, at)
    else:
        reads, rows = in_branch(n, [n - 1 - p for p in at])
    st, _ = compare(tmp_path, reads, rows, table={k: 0 for k in range(800)})
    assert st["diff_positions"] == 100 and st["pairs"] == 1


def test_no_mismatch_missing_edge_false_branch(tmp_path):
    for kind, (reads, rows) in (("out", out_branch(70, [])), ("in", in_branch(70, []))):
        st, _ = compare(tmp_path / kind, reads, rows, table={k: 0 for k in range(600)})
        assert st["missing_edges"] == 1 and st["false_branches"] == 1 and st["components"] == 0 and st["edges_removed"] == 2


def test_three_neighbours_and_a_reverse_branching_vertex(tmp_path):
    """s -> u with '+' '-' labels u reverse, and its neighbours through '-' '-' rows with it: the sequences are compared reverse-
    complemented.  Three neighbours: three pairs."""
    reads, rows = out_branch(100, [30], third=[60])
    reads = [GENOME[500:560] + reads[0][:40]] + reads
    rows = [(0, 1, 60, "+", "-")] + [(u + 1, v + 1, p, "-", "-") for u, v, p in rows]
    st, _ = compare(tmp_path, reads, rows, table={k: 0 for k in range(600)})
    assert st["pairs"] == 3 and st["out_branches"] == 1 and st["diff_positions"] == 4


@pytest.mark.parametrize("neighbours", [2, 3])
def test_inclusion_pairs(tmp_path, neighbours):
    """min_overlap_len 30: a neighbour of 100 bases at 10 and one of 40 bases at 90 (relative_pos 80 > 100 - 30)."""
    g = GENOME[:200]
    reads, rows = [g[:130], g[10:110], g[90:130]], [(0, 1, 10), (0, 2, 90)]
    if neighbours == 3:
        reads.append(mutate(g[15:130], [50]))
        rows.append((0, 3, 15))
    st, _ = compare(tmp_path, reads, rows, table={k: 0 for k in range(600)}, min_overlap_len=30)
    assert st["inclusion_pairs"] == 1 and st["pairs"] == (0 if neighbours == 2 else 2)


def evidence_case(n_first=65, n_second=64):
    """Out-branch 0 -> {1, 2, 3}; the three differ in the first 12 bases.  se 10, pe 40: ids 0..9 single, 10..49 /1, 50..89 /2.
    Vertex 1 holds n_first originals, 2 holds n_second, 3 holds one; they are cut from the neighbour itself (agree), from another
    neighbour (disagree), forward or reverse-complemented, at negative indices, behind the contig's end, and short ones that
    cover no listed position.  The listed positions are 3, 6, 9 and 11 of the contigs; every read of 30 bases at index <= 8 covers
    11 as its last one, and kind 4 disagrees there and nowhere else.  Vertex 0 holds the ids that are no multiple of 3: an id
    and its mate (+- 40) never agree modulo 3 both ways, so hits without a mate hit and mate hits without a hit occur on both
    sides of se + pe (test_evidence_kernel_cases counts them from the inputs)."""
    rng = random.Random(23)
    lead, n = 40, 120
    g = GENOME[1000:1000 + lead + n]
    base = g[lead:]
    contigs = [base, mutate(base, [3, 9]), mutate(base, [6, 11])]
    reads = [g] + contigs
    rows = [(0, 1, lead), (0, 2, lead), (0, 3, lead)]
    oreads = [None] * 90
    subreads = {0: [], 1: [], 2: [], 3: []}
    ids = list(range(90))
    rng.shuffle(ids)
    counts = {1: n_first, 2: n_second, 3: 1}
    k = 0
    for v in (1, 2, 3):
        for t in range(counts[v]):
            oid = ids[k]; k += 1
            kind = t % 6
            src = contigs[v - 1] if kind != 1 else contigs[v % 3]             # kind 1: a read of another neighbour
            idx = rng.choice([-5, -1, 0, 2, 8]) if kind != 2 else 60          # kind 2: covers no listed position
            if kind == 3:
                idx = 125                                                     # starts behind the contig's end
            ln = 30
            padded = GENOME[2000:2010] + src + GENOME[2100:2140]
            seq = padded[10 + idx:10 + idx + ln]
            if kind == 4 and v == 1:
                seq = mutate(seq, [11 - idx])                                 # disagrees at the last covered listed position only
            fw = kind != 5
            oreads[oid] = seq if fw else rc(seq)
            subreads[v].append((oid, fw, idx, ln))
    for oid in range(90):
        if oreads[oid] is None:
            oreads[oid] = GENOME[3000 + oid:3030 + oid]
        if oid % 3 != 0:
            subreads[0].append((oid, True, 0, 30))
    return reads, rows, oreads, subreads


def hit_kinds(subreads, se, pe):
    """From the inputs alone: how many originals of the neighbours are found by id only / by mate only, below and above se + pe."""
    own = {o for o, _, _, _ in subreads[0]}
    n = dict(id_only_low=0, mate_only_low=0, id_only_high=0, mate_only_high=0, both=0, none=0)
    for v in subreads:
        for o, _, _, _ in subreads[v] if v else ():
            mate = o - pe if o >= se + pe else o + pe if o >= se else None
            hit, mhit = o in own, mate is not None and mate in own
            side = "high" if o >= se + pe else "low"
            n["both" if hit and mhit else "none" if not (hit or mhit) else ("id_only_" if hit else "mate_only_") + side] += 1
    return n


@pytest.mark.parametrize("sizes", [(65, 24), (64, 25), (1, 1)])
def test_evidence_kernel_cases(tmp_path, sizes):
    reads, rows, oreads, subreads = evidence_case(*sizes)
    st, _ = compare(tmp_path, reads, rows, oreads=oreads, subreads=subreads, table={k: 1 for k in range(600)}, se=10, pe=40)
    assert st["work_items"] == sizes[0] + sizes[1] + 1
    if sizes[0] > 1:
        kinds = hit_kinds(subreads, 10, 40)
        print("hit kinds", kinds)
        assert min(kinds.values()) > 0                       # every way of being found, separately, on both sides of se + pe
        assert 0 < st["evidence_ids"] < st["work_items"]


def targeted_evidence(flip):
    """Out-branch 0 -> {1, 2} at 40; contig 2 differs from contig 1 at 3, 9 and 20: the list is 43, 49, 60.  se 4, pe 5: ids 0..3
    single, 4..8 /1, 9..13 /2, original_readcount 14.  Vertex 0 holds 0 2 3 4 6 8 10 12 13.  The originals of vertex 1, all cut from
    contig 1 (30 bases at index 0 unless said):
      0   single, held                                            -> 0
      1   single, not held by vertex 0                            -> nothing
      2   single, held; 15 bases: covers 3 and 9, and with `flip` disagrees at 9, its LAST covered position, only
                                                                  -> nothing (without flip: 2)
      3   single, held; the same 15 bases, untouched              -> 3
      4   /1, held, mate 9 not; 5 bases at index 8: covers 9 alone -> 4
      5   /1, not held, mate 10 held                              -> 14 + 5 = 19
      11  /2, not held, mate 6 held                               -> 14 + 6 = 20
      12  /2, held, mate 7 not                                    -> 12
      13  /2, held, mate 8 held                                   -> 13 and 14 + 8 = 22
    Vertex 2 holds 0 and 3: their reads are contig 1's and disagree with contig 2 at 3 -> nothing.  So edge 0 -> 1 has 0 3 4 12
    13 19 20 22 (and 2 without flip), edge 0 -> 2 has nothing: 8 (9) evidence ids, unique counts 8 (9) and 0."""
    lead = 40
    g = GENOME[2600:2600 + lead + 100]
    c1 = g[lead:]
    c2 = mutate(c1, [3, 9, 20])
    reads, rows = [g, c1, c2], [(0, 1, lead), (0, 2, lead)]
    oreads = [GENOME[3500 + 7 * k:3530 + 7 * k] for k in range(14)]
    sub = {0: [(o, True, 0, 30) for o in (0, 2, 3, 4, 6, 8, 10, 12, 13)], 1: [], 2: []}
    for o, idx, ln in ((0, 0, 30), (1, 0, 30), (2, 0, 15), (3, 0, 15), (4, 8, 5), (5, 0, 30), (11, 0, 30), (12, 0, 30), (13, 0, 30)):
        oreads[o] = c1[idx:idx + ln]
        sub[1].append((o, True, idx, ln))
    if flip:
        oreads[2] = mutate(oreads[2], [9])
    sub[2] = [(0, True, 0, 30), (3, True, 0, 15)]
    return reads, rows, oreads, sub


def test_evidence_targeted(tmp_path):
    """The look-up paths one by one and the disagreement at the last covered position: expected values worked out in
    targeted_evidence's text.  Original 2 alone makes the difference between the two runs."""
    for flip, n1, ids in ((True, 8, 8), (False, 9, 9)):
        reads, rows, oreads, sub = targeted_evidence(flip)
        st, report = compare(tmp_path / str(flip), reads, rows, oreads=oreads, subreads=sub, table={k: 1 for k in range(600)}, se=4, pe=5)
        assert st["work_items"] == 11 and st["evidence_ids"] == ids, st
        assert report.rstrip("\n").split("\t")[3:] == [f"0>1:{n1}", "0>2:0"], report


def test_double_branch_and_missing_distance(tmp_path):
    """0, 1 -> 2, 3: a 2 x 2 double branch, every edge visited from its in-branch and from its out-branch.  Reads of the two
    haplotypes support their own edges; the table holds the distance in one run and not in the other."""
    g = GENOME[1500:1800]
    h = mutate(g, [60, 150])
    reads = [g[:120], h[:120], g[40:200], h[40:200]]
    rows = [(0, 2, 40), (0, 3, 40), (1, 2, 40), (1, 3, 40)]
    oreads, subreads = [], {0: [], 1: [], 2: [], 3: []}
    for k in range(12):
        src, a, b = (g, 0, 2) if k % 2 == 0 else (h, 1, 3)
        start = 30 + 3 * k
        oreads.append(src[start:start + 140])
        subreads[a].append((k, True, start, 140))
        subreads[b].append((k, True, start - 40, 140))
    st, report = compare(tmp_path / "a", reads, rows, oreads=oreads, subreads=subreads, table={k: 2 for k in range(100, 400)})
    assert st["in_branches"] == 2 and st["out_branches"] == 2 and st["components"] == 1 and report.count(">") == 4
    st2, _ = compare(tmp_path / "b", reads, rows, oreads=oreads, subreads=subreads, table={5: 2})
    assert st2["dist_too_large"] == 1 and st2["edges_removed"] == 4


@pytest.mark.parametrize("careful", [True, False])
def test_neighbouring_components(tmp_path, careful):
    """Out-branch 0 -> {1, 2} and out-branch 2 -> {3, 4} share vertex 2; every read is its own original and supports nothing, so
    min evidence 0 keeps a component: with careful the second one is removed for standing next to the first."""
    g = GENOME[2200:2600]
    reads = [g[:100], mutate(g[40:140], [70]), g[40:140], mutate(g[80:180], [75]), g[80:180]]
    rows = [(0, 1, 40), (0, 2, 40), (2, 3, 40), (2, 4, 40)]
    st, _ = compare(tmp_path, reads, rows, table={k: 0 for k in range(600)}, careful=careful)
    assert st["components"] == 2 and st["components_kept"] == (1 if careful else 2) and st["edges_removed"] == (2 if careful else 0)


# ---- a generated cluster through the whole iteration ---------------------------------------------------------------------------
POLYTE = dict(min_overlap_len=60, edge_threshold=0.97, remove_tips=False, ignore_inclusions=False)
FIRST = dict(POLYTE, error_correction=True, min_clique_size=3, remove_trans=2, remove_branches=False, remove_backedges=False,
             keep_singletons=0)
GEN = dict(POLYTE, remove_trans=1, remove_branches=False)
CLIQUE = dict(error_correction=False, min_clique_size=2, keep_singletons=0, remove_backedges=True, first_it=False)
GEN_SEED = 5        # with the model alone (no library): 14 components, 3 of them kept, 11 removed, 4 evidence ids, 3 inclusion pairs


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """300 reads of two strains (hylight_amd.simulate through vq_clique_inputs) and POLYTE's first iteration over them - the
    cliques with error correction, whose super-reads share original reads - by the model: the input of the branch iteration."""
    from hylight_amd import api
    d = tmp_path_factory.mktemp("generated")
    fq, ov, tab = str(d / "original.fastq"), str(d / "overlaps0.txt"), str(d / "table.tsv")
    reads = I.haplotype_reads(seed=GEN_SEED, n_strains=2, genome_len=1500, n_reads=300)
    I.write_inputs(reads, fq, ov)
    with open(tab, "w") as f:
        f.write("".join(f"{k}\t0\t1\n" for k in range(100, 400)))
    first = str(d / "first")
    CN.clique_iteration(fq, ov, first, api.vq_cliques_of_graph, scores=_lib_scores(api, fq, ov, min_overlap_len=60), **FIRST)
    p = lambda n: os.path.join(first, n)
    scores = _lib_scores(api, p("singles.fastq"), p("overlaps.txt"), min_overlap_len=60)
    return p("singles.fastq"), p("overlaps.txt"), p("subreads.txt"), fq, tab, len(reads), scores


def test_generated_cluster_iteration(tmp_path, generated):
    """hlmi_vq_branch_iteration over the first iteration's super-reads against the branch model inside the clique-next model."""
    from hylight_amd import api
    fq, ov, sub, ofq, tab, n, scores = generated
    lib_dir, model_dir = str(tmp_path / "lib"), str(tmp_path / "model")
    with B.Hook(ofq, n, 0, tab, True, False, sub, GEN["min_overlap_len"], GEN["edge_threshold"]) as h:
        want = CN.clique_iteration(fq, ov, model_dir, api.vq_cliques_of_graph, subreads_in=sub, scores=scores, **GEN, **CLIQUE)
    with open(os.path.join(model_dir, "branch_components.txt"), "w", newline="") as f:
        f.write("".join(h.report))
    got = api.vq_branch_iteration(fq, ov, ofq, tab, lib_dir, subreads_in=sub, se_count=n, pe_count=0, careful=True, **GEN, **CLIQUE)
    for name in NAMES + CM.OUTPUTS + ("overlaps.txt", "stats.txt"):
        a, b = os.path.join(lib_dir, name), os.path.join(model_dir, name)
        assert os.path.exists(a) == os.path.exists(b), name
        if os.path.exists(b):
            assert open(a, "rb").read() == open(b, "rb").read(), name
    print("generated", got[1], h.stats, {k: v for k, v in api.last_stats().items() if "vq_branch" in k})
    assert got[0] == want[0] and {k: got[1][k] for k in B.STATS} == h.stats
    assert {k: got[2][k] for k in CM.STATS} == {k: want[1][k] for k in CM.STATS}
    assert {k: got[3][k] for k in CN.STATS} == want[2]
    kept = sum(line.split("\t")[2] == "1" for line in h.report)
    assert kept >= 1 and len(h.report) - kept >= 1, "the input has to hold a kept and a removed component"
    assert h.stats["pairs"] > 0 and h.stats["evidence_ids"] > 0 and want[2]["src_branching"] > 0


def test_clique_iteration_is_unchanged(tmp_path, generated):
    """hlmi_vq_clique_iteration on the same input: the new parameter is absent there, the call equals its model as before."""
    from hylight_amd import api
    fq, ov, sub, _, _, _, scores = generated
    opts = dict(GEN, remove_branches=True, **CLIQUE)
    got = api.vq_clique_iteration(fq, ov, str(tmp_path / "lib"), subreads_in=sub, **opts)
    want = CN.clique_iteration(fq, ov, str(tmp_path / "model"), api.vq_cliques_of_graph, subreads_in=sub, scores=scores, **opts)
    for name in M.OUTPUTS + CM.OUTPUTS + ("overlaps.txt", "stats.txt"):
        a, b = tmp_path / "lib" / name, tmp_path / "model" / name
        assert a.exists() == b.exists() and (not b.exists() or a.read_bytes() == b.read_bytes()), name
    assert not (tmp_path / "lib" / "branch_components.txt").exists()
    assert got[0] == want[0] and {k: got[2][k] for k in CN.STATS} == want[2]


def test_refusals_come_before_any_output(tmp_path):
    """HLMI_EINVAL (-1), and out_dir stays empty: counts that do not match the original FASTQ, a table that cannot be opened or
    holds a line std::stoi rejects, an original id the FASTQ does not hold, remove_trans != 1, remove_branches set."""
    from hylight_amd import api
    reads, rows = out_branch(70, [10])
    fq, ov, ofq, _, tab = write_case(str(tmp_path / "in"), reads, rows, table={100: 0})
    bad_tab, sub = str(tmp_path / "bad.tsv"), str(tmp_path / "sub.txt")
    open(bad_tab, "w").write("100\t0\tx\n")
    carried = str(tmp_path / "carried.tsv")               # a fourth column goes in front of the next line: stoi("extra100")
    open(carried, "w").write("300\t1\t2\textra\n100\t0\t0\n")
    open(sub, "w").write("0\t0:+:0:90\n1\t1:+:0:70\n2\t7:+:0:70\n")
    out = str(tmp_path / "out")
    ok = dict(HAND, se_count=3, pe_count=0)
    for kw, table, subreads in ((dict(ok, se_count=2), tab, None), (dict(ok, se_count=1, pe_count=2), tab, None),
                                (ok, str(tmp_path / "none.tsv"), None), (ok, bad_tab, None), (ok, carried, None), (ok, tab, sub),
                                (dict(ok, remove_trans=2), tab, None), (dict(ok, remove_branches=True), tab, None)):
        with pytest.raises(api.HlmiError) as e:
            api.vq_branch_graph(fq, ov, ofq, table, out, subreads_in=subreads, **kw)
        assert e.value.code == -1 and os.listdir(out) == [], (kw, e.value)
    api.vq_branch_graph(fq, ov, ofq, tab, out, **ok)
    assert "branch_components.txt" in os.listdir(out)
