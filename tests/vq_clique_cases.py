"""Hand-made cases of the clique step, shared by tests/test_vq_clique_model.py (the model against values worked out by hand)
and tests/test_gpu_vq_cliques.py (the library against the model, through files).  TEST INFRASTRUCTURE ONLY.

A case is reads (sequence, qualities, forward label), edges (v1, v2, pos1: v2 starts pos1 behind v1) and options.  Read k has
id 10 + k.  `write_files` writes singles.fastq and an overlaps file whose graph is exactly these edges with these labels;
`state` is the same as the model's graph state.
"""
import collections
import os
import random

G = "ACGTTGCAAGCTTAGGCATCGATTACAGGCTA"           # 32 bases without a repeat of length 4
COMP = str.maketrans("ACGT", "TGCA")
Q = "I"                                          # phred 40


def rc(s):
    return s.translate(COMP)[::-1]


def _chain(offsets, length, genome=G):
    """Reads of `length` bases of the genome at the given offsets, every pair an edge."""
    reads = [(genome[o:o + length], Q * length, True) for o in offsets]
    edges = [(i, j, offsets[j] - offsets[i]) for i in range(len(offsets)) for j in range(i + 1, len(offsets))]
    return reads, edges


def case_vote():
    """Three reads on top of each other, one of them with a C in column 2."""
    reads = [("AAAAA", Q * 5, True), ("AAAAA", Q * 5, True), ("AACAA", Q * 5, True)]
    return dict(reads=reads, edges=[(0, 1, 0), (0, 2, 0), (1, 2, 0)], opts=dict(min_clique_size=2))


def case_ec3():
    reads, edges = _chain([0, 2, 4], 10)
    return dict(reads=reads, edges=edges, opts=dict(min_clique_size=3, error_correction=True))


def case_ends_before_trim():
    """Read 1 (three bases) lies two columns in front of the base and ends where the third entry starts: the offsets are 0
    (read 1), 2 (read 0), 3 (read 2), trim_pos = 3 and read 1 is over by then."""
    reads = [(G[2:12], Q * 10, True), (G[0:3], Q * 3, True), (G[3:13], Q * 10, True)]
    return dict(reads=reads, edges=[(1, 0, 2), (0, 2, 1), (1, 2, 1)], opts=dict(min_clique_size=3, error_correction=True))


def case_size(n):
    """n reads of 24 bases at offsets 0 .. n - 1; reads 2, 3, 4 carry a T in column 5 where the genome has a G."""
    genome = G[:5] + "G" + G[6:]
    reads, edges = _chain(list(range(n)), 24, genome)
    for k in (2, 3, 4):
        s = reads[k][0]
        reads[k] = (s[:5 - k] + "T" + s[6 - k:], reads[k][1], True)
    return dict(reads=reads, edges=edges, opts=dict(min_clique_size=2))


def case_reverse():
    reads, edges = _chain([0, 3], 10)
    reads[1] = (rc(reads[1][0]), reads[1][1], False)
    return dict(reads=reads, edges=edges, opts=dict(min_clique_size=2))


def case_n_rate():
    reads = [("AAAAAAAAAA", Q * 10, True), ("AAAAACCCCC", Q * 10, True)]
    return dict(reads=reads, edges=[(0, 1, 0)], opts=dict(min_clique_size=2))


def case_not_first():
    reads, edges = _chain([0, 2], 10)
    reads[1] = (rc(reads[1][0]), reads[1][1], False)
    return dict(reads=reads, edges=edges, opts=dict(min_clique_size=2, first_it=False),
                subreads="10\t100:+:3:5\n11\t101:-:2:4\n")


CASES = dict(vote=case_vote, ec3=case_ec3, ends_before_trim=case_ends_before_trim, size6=lambda: case_size(6),
             size7=lambda: case_size(7), reverse=case_reverse, n_rate=case_n_rate, not_first=case_not_first)


def case_pairs():
    """Eight reads of 150 to 200 bases whose graph is four disjoint edges - what the merge and the clique step (min_clique_size
    2, no error correction) must both turn into the same records.  Not one of CASES: its cliques are four.
      0, 1  the edge is stored from the higher vertex: 1 -> 0 at 60
      2, 3  3 is stored reverse-complemented and labelled reverse
      4, 5  16 of the 110 shared columns disagree at equal quality: 16 N in 200 columns, above the 5 % of test_N_rate
      6, 7  pos1 = 0: both start in the same column"""
    rng = random.Random(11)
    g = ["".join(rng.choices("ACGT", k=260)) for _ in range(4)]
    qual = lambda n: "".join(chr(33 + rng.randint(20, 40)) for _ in range(n))
    other = g[2][40:200]
    for c in range(3, 110, 7):                   # 16 columns of the overlap
        other = other[:c] + "ACGT"[("ACGT".index(other[c]) + 1) % 4] + other[c + 1:]
    reads = [(g[0][60:260], qual(200), True), (g[0][0:170], qual(170), True),
             (g[1][0:160], qual(160), True), (rc(g[1][50:230]), qual(180), False),
             (g[2][0:150], Q * 150, True), (other, Q * 160, True),
             (g[3][0:150], qual(150), True), (g[3][0:190], qual(190), True)]
    return dict(reads=reads, edges=[(1, 0, 60), (2, 3, 50), (4, 5, 40), (6, 7, 0)], opts=dict(min_clique_size=2))


def state(case):
    reads, edges = case["reads"], case["edges"]
    adj = [[] for _ in reads]
    for v1, v2, pos1 in edges:
        adj[v1].append(dict(v1=v1, v2=v2, pos1=pos1))
    return dict(seqs=[r[0] for r in reads], quals=[r[1] for r in reads], ids=[10 + k for k in range(len(reads))],
                orient=[r[2] for r in reads], adj=adj)


def clique_text(case):
    """Every vertex of a case is in one clique: the file the enumerator writes for a complete graph."""
    return "NOTE: Quick Cliques v2.0beta.\nReading .edges file format. \n" + "".join(f"{k} " for k in range(len(case["reads"]))) + "\n"


def write_files(tmp_path, case):
    """-> (singles.fastq, overlaps file, subreads file or None) of a case, in tmp_path."""
    fq, ov = str(tmp_path / "singles.fastq"), str(tmp_path / "overlaps.txt")
    reads = case["reads"]
    with open(fq, "w") as f:
        f.write("".join(f"@{10 + k}\n{s}\n+\n{q}\n" for k, (s, q, _) in enumerate(reads)))
    with open(ov, "w") as f:
        for v1, v2, pos1 in case["edges"]:
            n = min(len(reads[v1][0]) - pos1, len(reads[v2][0]))
            f.write(f"{10 + v1}\t{10 + v2}\t{pos1}\t-\t-\t{'+' if reads[v1][2] else '-'}\t{'+' if reads[v2][2] else '-'}\t99\t-\t{n}\t-\ts\ts\n")
    sub = None
    if "subreads" in case:
        sub = str(tmp_path / "subreads_in.txt")
        open(sub, "w").write(case["subreads"])
    return fq, ov, sub


# every row an edge (merge_contigs 1), no reduction: the graph is the case's edges as they are
HAND_GRAPH = dict(min_overlap_len=1, merge_contigs=1.0, remove_trans=0, remove_branches=False, remove_tips=False, ignore_inclusions=False)


def records(out_dir):
    """The records of a step's singles.fastq without their ids: a Counter of (sequence, quality line, the originals of the
    record's subreads.txt line)."""
    fq = open(os.path.join(out_dir, "singles.fastq")).read().split("\n")[:-1]
    sub = dict(line.split("\t", 1) for line in open(os.path.join(out_dir, "subreads.txt")).read().split("\n")[:-1])
    assert len(fq) % 4 == 0 and len(sub) == len(fq) // 4
    return collections.Counter((fq[k + 1], fq[k + 3], sub[fq[k][1:]]) for k in range(0, len(fq), 4))
