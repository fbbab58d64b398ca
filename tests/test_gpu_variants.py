"""GPU: hlmi_variants against its model (tests/variants_model.py) - the sites and the summary byte for byte and every integer stat.
The hand cases of tests/variants_inputs.py (ties, the own base in the minority, N and lower case, every threshold one below and
exactly at its border, a contig of no bases) and its shapes (contig lengths around the tile, sites on tile borders and contig
junctions, a tile without a site between two with sites, a tile of sites, the lane / wave switch in CIGARs of 63 to 513 ops, a D
run across a tile border, a cbase that is no multiple of the tile, 4 097 rows on one position), each with a pair list and with an
empty one; the call without a site, whose second pass is not launched; the refusals, with nothing written; the two-strain case
whose list removes every site."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import variants_inputs as VI  # noqa: E402
import variants_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = VI.hand_cases()
SHAPES = VI.shapes()


def ints(st):
    return {k: st[k] for k in VM.STAT_KEYS}


def run_and_compare(c, d, pairs=None, summary=True, **opts):
    """-> the model's (sites, summary, stats), after the library's files and stats were found equal to them"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = VM.variants(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, **opts)
    sites, summ = os.path.join(d, "sites.tsv"), os.path.join(d, "summary.tsv")
    st = api.variants(cfa, rfa, paf, sites, summ if summary else None, pairs=lst, **opts)
    assert ints(st) == want[2]
    with open(sites, "rb") as f:
        assert f.read() == want[0]
    if summary:
        with open(summ, "rb") as f:
            assert f.read() == want[1]
    else:
        assert not os.path.exists(summ)
    return want


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    h = HAND[name]
    sites, summary, st = run_and_compare(h.case, tmp_path, **h.opts)
    assert sites == VM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert summary == VM.SUMMARY_HEAD + b"".join(line + b"\n" for line in h.summary)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape(name, tmp_path):
    s = SHAPES[name]
    s.where(*VM.variants(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(), **s.opts))
    sites, _, st = run_and_compare(s.case, tmp_path / "plain", **s.opts)
    last = api.last_stats()
    assert last["variants_tiles"] >= 1 and 1 <= last["variants_tiles_revisited"] <= last["variants_tiles"]
    assert st["pairs_listed"] == st["rows_not_listed"] == 0
    # every other read listed, in either order
    reads = [n for n, _ in s.case.reads]
    target = {r.split(b"\t")[0]: r.split(b"\t")[5] for r in s.case.rows}
    lst = b"".join(XI.row(q, target[q], 14) if i % 4 else XI.row(target[q], q) for i, q in enumerate(reads) if i % 2 == 0)
    _, _, st2 = run_and_compare(s.case, tmp_path / "listed", pairs=lst, **s.opts)
    assert st2["rows_selected"] == (len(reads) + 1) // 2 and st2["rows_not_listed"] == len(reads) // 2
    # an empty list: no row votes, the header line alone and a summary of zeros
    sites0, summ0, st0 = run_and_compare(s.case, tmp_path / "empty", pairs=b"", **s.opts)
    assert sites0 == VM.SITES_HEAD and st0["rows_selected"] == st0["callable"] == st0["sites"] == 0 and st0["rows_not_listed"] == len(reads)
    assert all(line.split(b"\t")[2:] == [b"0", b"0", b"0", b"0.000000"] for line in summ0.split(b"\n")[1:-1])
    # no summary asked for
    run_and_compare(s.case, tmp_path / "nosummary", summary=False, **s.opts)


def test_only_the_tiles_with_a_site_are_revisited(tmp_path):
    s = SHAPES["tile_borders_and_a_tile_without_a_site"]
    run_and_compare(s.case, tmp_path, **s.opts)
    last = api.last_stats()
    assert (last["variants_tiles"], last["variants_tiles_revisited"]) == (5, 4)


def test_no_site_second_pass_not_launched(tmp_path):
    T = VI.T
    ref = VI._seq(2 * T + 7, 4)
    c = VI.add_pile(PI.Case([("c", ref)]), ref, T, [None] * 4, strands="+-")
    sites, summary, st = run_and_compare(c, tmp_path)
    assert sites == VM.SITES_HEAD and st["sites"] == 0 and st["callable"] == 2 * T + 7
    last = api.last_stats()
    assert last["variants_tiles"] == 3 and last["variants_tiles_revisited"] == 0
    assert last.get("kernel_ms.variants_tile", 0) > 0 and last.get("kernel_ms.variants_sites", 0) == 0


def test_selection_options_and_one_row_per_read(tmp_path):
    """min_len, min_iden and the tie between two contigs, through the library"""
    ca, cb = VI._seq(40), VI._seq(60, 3)
    c = PI.Case([("a", ca), ("b", cb)])
    c.add(0, "6=", ca[:6], target="a", name="r0", right=cb[:8])
    c.add(0, "8=", cb[:8], target="b", read="r0")
    c.add(2, "5=", cb[2:7], target="b", name="r1")
    c.add(3, "5X", cb[2:7], target="a", read="r1")
    c.add(10, "10=10X", ca[10:20] + bytes(VI.other_base(b)[0] for b in ca[20:30]), target="a", name="r2")
    opts = dict(min_cov=1, min_alt=1, min_frac=0.5)
    sites, _, st = run_and_compare(c, tmp_path / "all", **opts)
    assert st["rows_selected"] == 3 and [p for n, p, _ in VI.site_rows(sites) if n == b"a"] == list(range(20, 30))      # r2's ten X
    assert run_and_compare(c, tmp_path / "len", min_len=6, **opts)[2]["rows_selected"] == 2
    assert run_and_compare(c, tmp_path / "iden", min_iden=0.75, **opts)[2]["rows_selected"] == 2


def test_two_strains_the_list_removes_every_site(tmp_path):
    s = XI.two_strains()
    sites, _, st = run_and_compare(s.case, tmp_path / "all")
    assert [p for _, p, _ in VI.site_rows(sites)] == sorted(s.snps) and st["sites"] >= 20
    sites1, _, st1 = run_and_compare(s.case, tmp_path / "listed", pairs=s.same_strain_list)
    assert sites1 == VM.SITES_HEAD and st1["sites"] == 0 and st1["rows_selected"] == 15 and st1["callable"] == 3000


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
    sites, summ = str(tmp_path / "s.tsv"), str(tmp_path / "t.tsv")
    with pytest.raises(Exception):
        VM.variants(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    refused(lambda: api.variants(cfa, rfa, paf, sites, summ), f"rows.paf:{line}:", (sites, summ))
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "reads.fa", "rows.paf"]


def test_option_list_and_name_refusals(tmp_path):
    h = HAND["min_alt_at"]
    cfa, rfa, paf = h.case.write(tmp_path)
    sites, summ, lst = str(tmp_path / "s.tsv"), str(tmp_path / "t.tsv"), str(tmp_path / "pairs.paf")
    for bad, word in ((dict(min_cov=0), "min_cov"), (dict(min_alt=0), "min_alt"), (dict(min_frac=-0.5), "min_frac"),
                      (dict(min_frac=1.5), "min_frac"), (dict(min_frac=float("nan")), "min_frac")):
        with pytest.raises(VM.PM.Refused):
            VM.variants(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), **bad)
        refused(lambda: api.variants(cfa, rfa, paf, sites, summ, **bad), word, (sites, summ))
    with open(lst, "wb") as f:
        f.write(XI.row(b"r0", b"c") + XI.row(b"r1", b"c", 5))
    refused(lambda: api.variants(cfa, rfa, paf, sites, summ, pairs=lst), "pairs.paf:2:", (sites, summ))
    # a row refusal comes in front of the list's
    bad = str(tmp_path / "bad.paf")
    with open(bad, "wb") as f:
        f.write(h.case.paf_bytes().replace(b"cg:Z:4=1X5=", b"cg:Z:4=1X4=", 1))
    refused(lambda: api.variants(cfa, rfa, bad, sites, summ, pairs=lst), "bad.paf:1:", (sites, summ))
    # a missing list cannot be read
    with pytest.raises(api.HlmiError):
        api.variants(cfa, rfa, paf, sites, summ, pairs=str(tmp_path / "none.paf"))
    assert not os.path.exists(sites) and not os.path.exists(summ)
    # two records of one name, among the contigs and among the reads
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(h.case.contigs_bytes() + b">c\nACGT\n")
    refused(lambda: api.variants(twice, rfa, paf, sites, summ), "two records are named c", (sites, summ))
    with open(twice, "wb") as f:
        f.write(h.case.reads_bytes() + b">r1\nACGT\n")
    refused(lambda: api.variants(cfa, twice, paf, sites, summ), "two records are named r1", (sites, summ))
    with pytest.raises(TypeError):
        api.variants(cfa, rfa, paf, sites, summ, qual_weight=1)
