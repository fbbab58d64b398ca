"""GPU: hlmi_depth against its model (tests/depth_model.py) - the TSV and the bedGraph byte for byte and every integer stat.  The
shapes of tests/depth_inputs.py (tile borders, the clip, contig lengths around the tile, a cbase that is no multiple of the
tile, a deep pile on one span, runs at tile borders and contig junctions), each with and without a pair list and with an empty
one; the refusals, with nothing written; out_bedgraph = NULL."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_inputs as DI  # noqa: E402
import depth_model as DM  # noqa: E402
import polish_inputs as PI  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = DI.shapes()


def ints(st):
    return {k: st[k] for k in DM.STAT_KEYS}


def run_and_compare(c, d, pairs=None, bedgraph=True, **opts):
    """-> the model's (tsv, bed, stats), after the library's files and stats were found equal to them"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = DM.depth(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, bedgraph=bedgraph, **opts)
    tsv, bed = os.path.join(d, "depth.tsv"), os.path.join(d, "depth.bedgraph")
    st = api.depth(cfa, rfa, paf, tsv, bed if bedgraph else None, pairs=lst, **opts)
    assert ints(st) == want[2]
    with open(tsv, "rb") as f:
        assert f.read() == want[0]
    if bedgraph:
        with open(bed, "rb") as f:
            assert f.read() == want[1]
    else:
        assert not os.path.exists(bed) and st["runs"] == 0
    return want


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape(name, tmp_path):
    s = SHAPES[name]
    s.where(*DM.depth(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes()))
    tsv, bed, st = run_and_compare(s.case, tmp_path / "plain")
    assert st["pairs_listed"] == st["rows_not_listed"] == 0
    # every other read listed, in either order
    reads = [n for n, _ in s.case.reads]
    target = {r.split(b"\t")[0]: r.split(b"\t")[5] for r in s.case.rows}
    lst = b"".join(XI.row(q, target[q], 14) if i % 4 else XI.row(target[q], q) for i, q in enumerate(reads) if i % 2 == 0)
    _, _, st2 = run_and_compare(s.case, tmp_path / "listed", pairs=lst)
    assert st2["rows_selected"] == (len(reads) + 1) // 2 and st2["rows_not_listed"] == len(reads) // 2
    # an empty list: no row counts, every contig a row of zeros
    tsv0, bed0, st0 = run_and_compare(s.case, tmp_path / "empty", pairs=b"")
    assert st0["rows_selected"] == st0["covered"] == st0["bases"] == 0 and st0["rows_not_listed"] == len(reads)
    assert all(line.split(b"\t")[2:] == [b"0", b"0", b"0", b"0.000000", b"0", b"0.000000"] for line in tsv0.split(b"\n")[1:-1])
    # no bedGraph asked for
    run_and_compare(s.case, tmp_path / "nobed", bedgraph=False)


def test_selection_options_and_one_row_per_read(tmp_path):
    """min_len, min_iden and the tie between two contigs, through the library"""
    ca, cb = DI._seq(40), DI._seq(60, 3)
    c = PI.Case([("a", ca), ("b", cb)])
    c.add(0, "6=", ca[:6], target="a", name="r0", right=cb[:8])
    c.add(0, "8=", cb[:8], target="b", read="r0")
    c.add(2, "5=", cb[2:7], target="b", name="r1")
    c.add(3, "5X", cb[2:7], target="a", read="r1")
    c.add(10, "10=10X", ca[10:30], target="a", name="r2")
    _, _, st = run_and_compare(c, tmp_path / "all")
    assert st["rows_selected"] == 3
    assert run_and_compare(c, tmp_path / "len", min_len=6)[2]["rows_selected"] == 2
    assert run_and_compare(c, tmp_path / "iden", min_iden=0.75)[2]["rows_selected"] == 2


def refused(call, word, outs):
    with pytest.raises(api.HlmiError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)
    for p in outs:
        assert not os.path.exists(p)


REFUSALS = PI.refusal_cases()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_row_refusals(name, tmp_path):
    c, line = REFUSALS[name]
    cfa, rfa, paf = c.write(tmp_path)
    tsv, bed = str(tmp_path / "d.tsv"), str(tmp_path / "d.bedgraph")
    with pytest.raises(Exception):
        DM.depth(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    refused(lambda: api.depth(cfa, rfa, paf, tsv, bed), f"rows.paf:{line}:", (tsv, bed))
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "reads.fa", "rows.paf"]


def test_list_and_name_refusals(tmp_path):
    s = SHAPES["equal_depth_at_a_contig_junction"]
    cfa, rfa, paf = s.case.write(tmp_path)
    tsv, bed, lst = str(tmp_path / "d.tsv"), str(tmp_path / "d.bedgraph"), str(tmp_path / "pairs.paf")
    with open(lst, "wb") as f:
        f.write(XI.row(b"r0", b"a") + XI.row(b"r1", b"b", 5))
    refused(lambda: api.depth(cfa, rfa, paf, tsv, bed, pairs=lst), "pairs.paf:2:", (tsv, bed))
    # a row refusal comes in front of the list's
    bad = str(tmp_path / "bad.paf")
    with open(bad, "wb") as f:
        f.write(s.case.paf_bytes().replace(b"cg:Z:100=", b"cg:Z:99=", 1))
    refused(lambda: api.depth(cfa, rfa, bad, tsv, bed, pairs=lst), "bad.paf:1:", (tsv, bed))
    # a missing list cannot be read
    with pytest.raises(api.HlmiError):
        api.depth(cfa, rfa, paf, tsv, bed, pairs=str(tmp_path / "none.paf"))
    assert not os.path.exists(tsv) and not os.path.exists(bed)
    # two records of one name, among the contigs and among the reads
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(s.case.contigs_bytes() + b">a\nACGT\n")
    refused(lambda: api.depth(twice, rfa, paf, tsv, bed), "two records are named a", (tsv, bed))
    with open(twice, "wb") as f:
        f.write(s.case.reads_bytes() + b">r1\nACGT\n")
    refused(lambda: api.depth(cfa, twice, paf, tsv, bed), "two records are named r1", (tsv, bed))
    with pytest.raises(TypeError):
        api.depth(cfa, rfa, paf, tsv, bed, min_cov=3)
