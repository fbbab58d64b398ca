"""CPU: tests/vq_merge_model.py (the yardstick of hlmi_vq_merge and hlmi_vq_consensus_pair) held to hand-worked cases whose
expected bytes are written out here.  PARITY UNPINNED: the reference needs Boost and cannot be built here.

Worked from SRBuilder::consensus_pos (SRBuilder.cpp:297-402), minQual 0.9:
  - two equal bases of Q40: the three others score 1e-4 / 3 each, so p_incorrect is about 1e-8 / 9 ... quality 'v' (Q85);
    Q40 with Q20: 'b' (Q65); twice Q93: '~'; twice Q0: every score is -inf, total_prob 0 -> 'N', '$'
  - two different bases of equal quality: each has probability 1/2 < minQual -> 'N', '$' (the A, T, C, G tie order of
    :390-393 can therefore only decide where ONE read is active: a single base of Q0 scores -inf and the three others
    log10(1/3) each, so A becomes T and C, G, T become A, with quality '#' = round(-10 log10(2/3)))
  - Q40 against Q20: the Q40 base with probability 0.99 -> kept, quality '5' (Q20); Q40 against Q31 ('@'): 0.888 < 0.9 -> N
  - a base against N: N adds nothing, the base comes back with its own quality; N against N: max_score == 0 -> 'N', '$'
"""
import os

import pytest

import vq_merge_model as MM


def _run(tmp_path, reads, rows, sub=None, **o):
    fq, ov = tmp_path / "s.fastq", tmp_path / "o.savage"
    fq.write_text("".join(f"@{i}\n{s}\n+\n{q}\n" for i, s, q in reads))
    ov.write_text("".join(f"{a}\t{b}\t{p}\t-\t-\t{o1}\t{o2}\t{perc}\t-\t{ln}\t-\ts\ts\n" for a, b, p, o1, o2, perc, ln in rows))
    opts = dict(min_overlap_len=1, merge_contigs=1.0, keep_singletons=1)       # every row is an edge
    opts.update(o)
    if sub is not None:
        (tmp_path / "sub.txt").write_text(sub)
        opts["subreads_in"] = str(tmp_path / "sub.txt")
    out = str(tmp_path / "out")
    g, m = MM.merge(str(fq), str(ov), out, **opts)
    return g, m, {n: open(os.path.join(out, n)).read() for n in MM.OUTPUTS if os.path.exists(os.path.join(out, n))}


def test_overlap_of_one(tmp_path):
    _, st, f = _run(tmp_path, [(1, "ACGTA", "IIIII"), (2, "AGGCC", "IIIII")], [(1, 2, 4, "+", "+", 99, 1)])
    assert f == {"singles.fastq": "@0\nACGTAGGCC\n+\nIIIIvIIII\n", "subreads.txt": "0\t1:+:0:5\t2:+:4:5\n",
                 "superread_map.txt": "0\t0\t0\t+\n1\t0\t4\t+\n"}
    assert st["pairs"] == st["merged"] == 1 and st["bases_in"] == 10 and st["bytes_out"] == 25


def test_overlap_of_300(tmp_path):
    a, b = "ACGT" * 100, "ACGT" * 75 + "GGCC" * 25                    # b starts 100 behind a: 300 shared bases
    _, st, f = _run(tmp_path, [(1, a, "I" * 400), (2, b, "5" * 400)], [(1, 2, 100, "+", "+", 99, 300)])
    assert f["singles.fastq"] == "@0\n" + a + "GGCC" * 25 + "\n+\n" + "I" * 100 + "b" * 300 + "5" * 100 + "\n"
    assert f["subreads.txt"] == "0\t1:+:0:400\t2:+:100:400\n"


def test_contained_read(tmp_path):
    _, _, f = _run(tmp_path, [(1, "ACGTACGTAC", "I" * 10), (2, "GTAC", "5555")], [(1, 2, 2, "+", "+", 99, 4)])
    assert f["singles.fastq"] == "@0\nACGTACGTAC\n+\nIIbbbbIIII\n" and f["subreads.txt"] == "0\t1:+:0:10\t2:+:2:4\n"


def test_base_is_read_2_of_the_edge(tmp_path):
    """The edge runs 2 -> 1; vertex 0 (read 1) is the base and lies 4 behind."""
    _, _, f = _run(tmp_path, [(1, "GGCCA", "IIIII"), (2, "ACGTG", "IIIII")], [(2, 1, 4, "+", "+", 99, 1)])
    assert f == {"singles.fastq": "@0\nACGTGGCCA\n+\nIIIIvIIII\n", "subreads.txt": "0\t1:+:4:5\t2:+:0:5\n",
                 "superread_map.txt": "0\t0\t4\t+\n1\t0\t0\t+\n"}


@pytest.mark.parametrize("o1,o2,fastq,sub,smap", [
    ("+", "+", "@0\nAACCGTTT\n+\nIIIbbIII\n", "0\t1:+:0:5\t2:+:3:5\n", "0\t0\t0\t+\n1\t0\t3\t+\n"),
    ("+", "-", "@0\nAACCGTTT\n+\nIIIbbIII\n", "0\t1:+:0:5\t2:-:3:5\n", "0\t0\t0\t+\n1\t0\t3\t-\n"),
    # read 1 is stored reversed and vertex 0 keeps the label forward: the edge is flipped and moved (2 -> 1), and the
    # super-read is the reverse complement of the two above
    ("-", "+", "@0\nAAACGGTT\n+\nIIIbbIII\n", "0\t1:+:3:5\t2:-:0:5\n", "0\t0\t3\t+\n1\t0\t0\t-\n"),
    ("-", "-", "@0\nAAACGGTT\n+\nIIIbbIII\n", "0\t1:+:3:5\t2:+:0:5\n", "0\t0\t3\t+\n1\t0\t0\t+\n")])
def test_four_orientations(tmp_path, o1, o2, fastq, sub, smap):
    a, b = "AACCG", "CGTTT"
    r1 = (1, a if o1 == "+" else MM.revcomp(a), "IIII5" if o1 == "+" else "5IIII")
    r2 = (2, b if o2 == "+" else MM.revcomp(b), "5IIII" if o2 == "+" else "IIII5")
    _, _, f = _run(tmp_path, [r1, r2], [(1, 2, 3, o1, o2, 99, 2)])
    assert f == {"singles.fastq": fastq, "subreads.txt": sub, "superread_map.txt": smap}


def test_per_position_rules():
    # position 3 T/Q40 against G/Q20 (kept, '5'); 4 A against G, both Q40 (N); 5 C/Q40 against T/Q31 (below minQual: N);
    # 6 G against N (G with its quality); 7 T/Q0 against C/Q40 (C); 8 twice A/Q93 ('~'); 9 twice A/Q0 (N)
    assert MM.consensus_pair("ACGTACGTAA", "IIIIIII!~!", "GGTNCAAAGG", "5I@II~!III", 3) == ("ACGTNNGCANAGG", "III5$$IK~$III")
    assert MM.pair_base("N", "I", "N", "I") == ("N", "$")
    assert MM.pair_base("C", "I", "G", "I") == ("N", "$") and MM.pair_base("T", "5", "A", "5") == ("N", "$")
    assert MM.pair_base("C", "I", "G", "5") == ("C", "5") and MM.pair_base("G", "5", "C", "I") == ("C", "5")
    assert MM.pair_base("C", "I", "G", "@") == ("N", "$")
    assert MM.pair_base("A", "~", "A", "~") == ("A", "~") and MM.pair_base("A", "!", "A", "!") == ("N", "$")
    # one active base: itself from Q2 on; Q0 / Q1 give the first other base in A, T, C, G; N gets '$'
    assert [MM.one_base(b, "!") for b in "ACGT"] == [("T", "#"), ("A", "#"), ("A", "#"), ("A", "#")]
    assert [MM.one_base(b, '"') for b in "ACGT"] == [("T", '"'), ("A", '"'), ("A", '"'), ("A", '"')]
    assert all(MM.one_base(b, chr(33 + q)) == (b, chr(33 + q)) for b in "ACGT" for q in range(2, 94))
    assert all(MM.one_base("N", chr(33 + q)) == ("N", "$") for q in range(94))


def test_empty_consensus():
    assert MM.consensus_pair("ACGT", "IIII", "GG", "II", 4) == ("ACGTGG", "IIIIII")     # pos == len1: read 2 follows at once
    assert MM.consensus_pair("ACGT", "IIII", "GG", "II", 5) == ("", "")                 # a position without a base
    assert MM.consensus_pair("ACGT", "III", "GG", "II", 2) == ("", "")                  # qualities end first
    assert MM.consensus_pair("ACGT", "IIII", "GG", "I", 3) == ("", "")
    assert MM.consensus_pair("ACGT", "IIII", "", "", 0) == ("", "")                     # an empty sequence, active at 0
    assert MM.consensus_pair("ACGT", "IIII", "GG", "II", 3) == ("ACGNG", "III$I")


def test_stretch_form_equals_the_loop():
    import random
    rng = random.Random(5)
    for _ in range(300):
        l1, l2 = rng.randint(1, 40), rng.randint(1, 40)
        pos = rng.randint(0, l1)
        s1, s2 = ("".join(rng.choice("ACGTN") for _ in range(n)) for n in (l1, l2))
        q1, q2 = ("".join(chr(33 + rng.choice((0, 1, 2, 20, 31, 40, 93))) for _ in range(n)) for n in (l1, l2))
        assert MM.consensus_pair(s1, q1, s2, q2, pos) == MM.consensus_pair_loop(s1, q1, s2, q2, pos)


def test_two_base_function_over_every_input():
    """The answer for two bases by class - same base / different bases / with N, the form the kernel keeps in LDS - equals
    consensus_pos evaluated directly for all 5 x 5 x 94 x 94 inputs."""
    Q = [chr(33 + q) for q in range(94)]
    rank = "ATCG"
    n = 0
    for q1 in Q:
        for q2 in Q:
            same = MM.consensus_pos("AA", q1 + q2)
            diff = MM.consensus_pos("AC", q1 + q2)                 # -> N / first / second
            for b1 in "ACGTN":
                for b2 in "ACGTN":
                    got = MM.consensus_pos(b1 + b2, q1 + q2)
                    n += 1
                    if b1 == "N" and b2 == "N":
                        want = ("N", "$")
                    elif b2 == "N":
                        want = MM.consensus_pos(b1 + "N", q1 + "!")
                    elif b1 == "N":
                        want = MM.consensus_pos(b2 + "N", q2 + "!")
                    elif b1 == b2:
                        want = (b1 if same[0] == "A" else "N", same[1])
                    else:
                        want = ({"N": "N", "A": b1, "C": b2}[diff[0]], diff[1])
                        if q1 == q2 and diff[0] != "N":              # equal scores: the earlier of A, T, C, G
                            want = (min(b1, b2, key=rank.index), diff[1])
                    assert got == want, (b1, q1, b2, q2)
    assert n == 220900


def test_five_percent_n(tmp_path):
    s1, s2 = "ACGTACGTACGTACGTACGN", "N" + "T" * 20                   # 40 bases merged; N against N stays N
    _, st, f = _run(tmp_path, [(1, s1, "I" * 20), (2, s2, "I" * 21)], [(1, 2, 19, "+", "+", 99, 1)])
    assert st["merged"] == 1 and f["singles.fastq"] == "@0\n" + s1 + "T" * 20 + "\n+\n" + "I" * 19 + "$" + "I" * 20 + "\n"
    # one N more: 2 of 40 is not below 5 %: dropped; read 1 (1 of 20) fails too, read 2 (1 of 21) comes back as it is
    (tmp_path / "b").mkdir()
    _, st, f = _run(tmp_path / "b", [(1, "N" + s1[1:], "I" * 20), (2, s2, "I" * 21)], [(1, 2, 19, "+", "+", 99, 1)])
    assert (st["dropped_n"], st["merged"], st["n_reads"], st["trivial"]) == (1, 0, 1, 1)
    assert f == {"singles.fastq": "@0\n" + s2 + "\n+\n" + "I" * 21 + "\n", "subreads.txt": "0\t2:+:0:21\n",
                 "superread_map.txt": "0\t-1\t0\t+\n1\t0\t0\t+\n"}


def test_keep_singletons_299_300(tmp_path):
    _, st, f = _run(tmp_path, [(1, "ACGTA", "IIIII"), (2, "AGGCC", "IIIII"), (3, "A" * 299, "I" * 299), (4, "C" * 300, "5" * 300)],
                    [(1, 2, 4, "+", "+", 99, 1)], keep_singletons=300)
    assert st["short_reads"] == 1 and st["trivial"] == 1
    assert f["singles.fastq"] == "@0\nACGTAGGCC\n+\nIIIIvIIII\n@1\n" + "C" * 300 + "\n+\n" + "5" * 300 + "\n"
    assert f["subreads.txt"] == "0\t1:+:0:5\t2:+:4:5\n1\t4:+:0:300\n"
    assert f["superread_map.txt"] == "0\t0\t0\t+\n1\t0\t4\t+\n2\t-1\t0\t+\n3\t1\t0\t+\n"


def test_dropped_pair_returns_as_two_trivials(tmp_path):
    """The overlapping bases disagree at equal quality: 2 N in 8 bases, the pair is dropped and both reads are written."""
    _, st, f = _run(tmp_path, [(1, "AACCG", "IIIII"), (2, "GCTTT", "IIIII")], [(1, 2, 3, "+", "+", 99, 2)])
    assert (st["pairs"], st["dropped_n"], st["merged"], st["trivial"]) == (1, 1, 0, 2)
    assert f["singles.fastq"] == "@0\nAACCG\n+\nIIIII\n@1\nGCTTT\n+\nIIIII\n"
    assert f["superread_map.txt"] == "0\t0\t0\t+\n1\t1\t0\t+\n"


def test_inclusion_and_tip_go_to_the_tip_file(tmp_path):
    g3 = "ACGGTCATTGCAAGCTTAGC" * 3
    # read 2 is included in read 1 (perc 100, no mismatch): its edges go, read 1 and read 3 merge, read 2 is set aside
    reads = [(1, g3[:40], "I" * 40), (2, g3[10:30], "I" * 20), (3, g3[20:60], "I" * 40)]
    gs, st, f = _run(tmp_path, reads, [(1, 2, 10, "+", "+", 100, 20), (1, 3, 20, "+", "+", 99, 20)])
    assert st["inclusion_reads"] == 1 and st["merged"] == 1
    assert f["removed_tip_sequences.fastq"] == "@0\n" + g3[10:30] + "\n+\n" + "I" * 20 + "\n"
    assert f["singles.fastq"] == "@0\n" + g3 + "\n+\n" + "I" * 20 + "v" * 20 + "I" * 20 + "\n"
    # a tip: read 1 has two out-neighbours, read 3 ends where read 1 ends (extension 0) and has no out-edge
    (tmp_path / "t").mkdir()
    reads = [(1, g3[:40], "I" * 40), (2, g3[10:60], "I" * 50), (3, g3[20:40], "I" * 20)]
    gs, st, f = _run(tmp_path / "t", reads, [(1, 2, 10, "+", "+", 99, 30), (1, 3, 20, "+", "+", 99, 20)], ignore_inclusions=False)
    assert gs["tip_reads"] == 1 and st["tip_reads"] == 1 and st["merged"] == 1
    assert f["removed_tip_sequences.fastq"] == "@0\n" + g3[20:40] + "\n+\n" + "I" * 20 + "\n"
    # the reference appends to the file: a second run leaves two records
    _run(tmp_path / "t", reads, [(1, 2, 10, "+", "+", 99, 30), (1, 3, 20, "+", "+", 99, 20)], ignore_inclusions=False)
    assert open(tmp_path / "t" / "out" / "removed_tip_sequences.fastq").read().count("@0\n") == 2
    gs, st, f = _run(tmp_path / "t", reads, [(1, 2, 10, "+", "+", 99, 30), (1, 3, 20, "+", "+", 99, 20)], ignore_inclusions=False,
                     store_tips_separately=False)
    assert st["tip_reads"] == 0 and st["trivial"] == 1


def test_second_iteration_with_a_reverse_vertex(tmp_path):
    """Read 2 is stored reversed (vertex 1 gets the label reverse) and holds the originals 7 (forward, at 1, 3 long) and 9
    (reverse, at 0, 2 long); read 1 holds 7 too - the base vertex's entry wins - and 8."""
    a, b = "AACCG", "CGTTT"
    sub = "1\t7:+:0:5\t8:-:2:3\n2\t9:-:0:2\t7:+:1:3\n3\t5:+:0:4\n"
    reads = [(1, a, "IIII5"), (2, MM.revcomp(b), "IIII5"), (3, "ACGT", "IIII")]
    _, st, f = _run(tmp_path, reads, [(1, 2, 3, "+", "-", 99, 2)], sub=sub, first_it=False)
    # read 2, reverse, 5 long, lies at 3: 9 -> forward flips to '+', index 5 + 3 - (2 + 0) = 6; 7 is already there
    assert f["singles.fastq"] == "@0\nAACCGTTT\n+\nIIIbbIII\n@1\nACGT\n+\nIIII\n"
    assert f["subreads.txt"] == "0\t7:+:0:5\t8:-:2:3\t9:+:6:2\n1\t5:+:0:4\n"
    # unmerged (a mismatching overlap): read 2 is written reversed, its originals mirrored: 7 -> '-', 5 - (1 + 3) = 1;
    # 9 -> '+', 5 - (0 + 2) = 3
    (tmp_path / "u").mkdir()
    reads[1] = (2, MM.revcomp("GCTTT"), "IIIII")
    reads[0] = (1, a, "IIIII")
    _, st, f = _run(tmp_path / "u", reads, [(1, 2, 3, "+", "-", 99, 2)], sub=sub, first_it=False)
    assert st["trivial_reverse"] == 1
    assert f["singles.fastq"] == "@0\nAACCG\n+\nIIIII\n@1\nGCTTT\n+\nIIIII\n@2\nACGT\n+\nIIII\n"
    assert f["subreads.txt"] == "0\t7:+:0:5\t8:-:2:3\n1\t7:-:1:3\t9:+:3:2\n2\t5:+:0:4\n"
