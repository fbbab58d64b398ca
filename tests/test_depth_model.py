"""CPU: tests/depth_model.py held to literals worked by hand from the rules of include/hylight_mi.h (hlmi_depth)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_model as DM  # noqa: E402
import polish_inputs as PI  # noqa: E402
import polish_model as PM  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import polish_pairs_model as XM  # noqa: E402

HEAD = DM.TSV_HEAD


def span_case(contigs, spans):
    """contigs: [(name, length)]; spans: [(contig name, ts, te)] - one read per span, every column '='"""
    c = PI.Case([(n, (b"ACGT" * (L // 4 + 1))[:L]) for n, L in contigs])
    seqs = dict(c.contigs)
    for t, a, b in spans:
        c.add(a, f"{b - a}=", seqs[t.encode()][a:b], target=t)
    return c


def run(c, **kw):
    return DM.depth(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), **kw)


def test_three_rows_on_ten_bases():
    c = span_case([("c", 10)], [("c", 0, 4), ("c", 2, 10), ("c", 2, 6)])
    assert DM.depths_of(10, [(0, 4), (2, 10), (2, 6)]) == [1, 1, 3, 3, 2, 2, 1, 1, 1, 1]
    tsv, bed, st = run(c)
    assert tsv == HEAD + b"c\t10\t3\t16\t10\t1.600000\t1\t1.000000\n"
    assert bed == b"c\t0\t2\t1\nc\t2\t4\t3\nc\t4\t6\t2\nc\t6\t10\t1\n"
    assert st == dict(rows=3, rows_selected=3, contigs=1, contigs_covered=1, positions=10, covered=10, bases=16, runs=4,
                      pairs_listed=0, pairs_unknown=0, rows_not_listed=0)
    tsv2, bed2, st2 = run(c, bedgraph=False)
    assert tsv2 == tsv and bed2 is None and st2 == dict(st, runs=0)


def test_abundance_of_two_contigs_and_a_contig_without_rows():
    # a: 8 of 8 positions once and 4 twice: mean 1.5; b: 5 of 10 once: mean 0.5; n: nothing.  Sum 2.0.
    c = span_case([("a", 8), ("n", 6), ("b", 10)], [("a", 0, 8), ("a", 2, 6), ("b", 5, 10)])
    tsv, bed, st = run(c)
    assert tsv == (HEAD + b"a\t8\t2\t12\t8\t1.500000\t1\t0.750000\n" + b"n\t6\t0\t0\t0\t0.000000\t0\t0.000000\n"
                   + b"b\t10\t1\t5\t5\t0.500000\t0\t0.250000\n")
    assert bed == b"a\t0\t2\t1\na\t2\t6\t2\na\t6\t8\t1\nn\t0\t6\t0\nb\t0\t5\t0\nb\t5\t10\t1\n"
    assert (st["contigs"], st["contigs_covered"], st["positions"], st["covered"], st["bases"], st["runs"]) == (3, 2, 24, 13, 17, 6)


def test_median_zero_on_a_half_covered_contig():
    # depths 0 0 0 0 0 1 1 1 1 1: element (10 - 1) // 2 = 4 of the sorted depths is 0
    tsv, _, _ = run(span_case([("c", 10)], [("c", 5, 10)]))
    assert tsv == HEAD + b"c\t10\t1\t5\t5\t0.500000\t0\t1.000000\n"
    # one more covered position: sorted 0 0 0 0 1 ...: element 4 is 1
    tsv, _, _ = run(span_case([("c", 10)], [("c", 4, 10)]))
    assert tsv.split(b"\n")[1].split(b"\t")[6] == b"1"


def test_even_length_takes_the_lower_middle():
    # depths 1 1 2 2 on four bases: the two middle elements of 1 1 2 2 are 1 and 2; element (4 - 1) // 2 = 1 is 1
    tsv, bed, _ = run(span_case([("c", 4)], [("c", 0, 4), ("c", 2, 4)]))
    assert tsv == HEAD + b"c\t4\t2\t6\t4\t1.500000\t1\t1.000000\n"
    assert bed == b"c\t0\t2\t1\nc\t2\t4\t2\n"


def test_one_row_per_read_over_two_contigs():
    ca, cb = b"ACGTACGTAC", b"TTGACCATGGAACC"
    # r0: 6 columns on a, then 8 on b: the longer span wins.  r1: 5 on b, then 5 on a: the earlier line on a tie
    c = PI.Case([("a", ca), ("b", cb)])
    c.add(0, "6=", ca[:6], target="a", name="r0", right=cb[:8])
    c.add(0, "8=", cb[:8], target="b", read="r0")
    c.add(2, "5=", cb[2:7], target="b", name="r1")
    c.add(3, "5X", cb[2:7], target="a", read="r1")
    tsv, bed, st = run(c)
    assert tsv == HEAD + b"a\t10\t0\t0\t0\t0.000000\t0\t0.000000\n" + b"b\t14\t2\t13\t8\t0.928571\t1\t1.000000\n"
    assert bed == b"a\t0\t10\t0\nb\t0\t2\t1\nb\t2\t7\t2\nb\t7\t8\t1\nb\t8\t14\t0\n"
    assert (st["rows"], st["rows_selected"]) == (4, 2)
    # min_len 6 leaves r0's rows only
    assert run(c, min_len=6)[2]["rows_selected"] == 1


def test_zero_length_contig_and_zero_sum():
    data = b">e\n>c\nACGT\n"
    tsv, bed, st = DM.depth(data, b">r\nAC\n", b"")
    assert tsv == HEAD + b"e\t0\t0\t0\t0\t0.000000\t0\t0.000000\n" + b"c\t4\t0\t0\t0\t0.000000\t0\t0.000000\n"
    assert bed == b"c\t0\t4\t0\n" and st["runs"] == 1 and st["positions"] == 4


def test_pair_list_and_duplicate_names():
    c = span_case([("c", 10)], [("c", 0, 4), ("c", 2, 10), ("c", 2, 6)])
    tsv, bed, st = run(c, pairs=XI.row(b"c", b"r1", 14))
    assert tsv == HEAD + b"c\t10\t1\t8\t8\t0.800000\t1\t1.000000\n" and bed == b"c\t0\t2\t0\nc\t2\t10\t1\n"
    assert (st["pairs_listed"], st["pairs_unknown"], st["rows_not_listed"], st["rows_selected"]) == (1, 0, 2, 1)
    tsv, bed, st = run(c, pairs=b"")
    assert tsv == HEAD + b"c\t10\t0\t0\t0\t0.000000\t0\t0.000000\n" and st["rows_not_listed"] == 3 and st["rows_selected"] == 0
    with pytest.raises(XM.ListRefused) as e:
        run(c, pairs=XI.row(b"c", b"r1") + XI.row(b"c", b"r0", 5))
    assert e.value.line == 2
    with pytest.raises(PM.Refused):
        DM.depth(b">c\nACGT\n>c\nACGT\n", c.reads_bytes(), b"")
    with pytest.raises(PM.Refused):
        DM.depth(c.contigs_bytes(), b">r\nAC\n>r\nAC\n", b"")
