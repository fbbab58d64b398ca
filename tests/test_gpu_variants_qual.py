"""GPU: hlmi_variants_q against its model (tests/variants_qual_model.py) - the sites and the summary byte for byte and every integer
field, columns_low_qual among them - over the PAF path with ASCII reads.  The cases of tests/variants_qual_inputs.py (a column at
the floor and one below, a vanishing site, a position that leaves callable, strand '-', the D op's flanks, D and X runs at the lane
/ wave switch, failing columns around the tile border and in ops 63 to 65, a FASTA record among FASTQ records, a deep pile, the read
floor), a tile that is revisited for its site (its failing columns are not counted twice), a pair list with the floor, the
refusals, and the three identities on every older input of tests/variants_inputs.py."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_pairs_inputs as XI  # noqa: E402
import polish_qual_inputs as QI  # noqa: E402
import variants_inputs as VI  # noqa: E402
import variants_model as VM  # noqa: E402
import variants_qual_inputs as VQI  # noqa: E402
import variants_qual_model as VQ  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = VQI.cases()
OLDER = {**{f"hand_{k}": (v.case, v.opts) for k, v in VI.hand_cases().items()},
         **{f"shape_{k}": (v.case, v.opts) for k, v in VI.shapes().items()}}
OFF = dict(min_base_qual=0, min_avg_qual=0.0)


def run_and_compare(c, d, pairs=None, **opts):
    """-> the model's (sites, summary, stats), after the library's files and integer fields were found equal to them"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = VQ.variants_q(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, **opts)
    sites, summ = os.path.join(d, "sites.tsv"), os.path.join(d, "summary.tsv")
    st = api.variants_q(cfa, rfa, paf, sites, summ, pairs=lst, **opts)
    assert {k: st[k] for k in VQ.STAT_KEYS} == want[2]
    with open(sites, "rb") as f:
        assert f.read() == want[0]
    with open(summ, "rb") as f:
        assert f.read() == want[1]
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(name, tmp_path):
    s = CASES[name]
    sites, summary, st = run_and_compare(s.case, tmp_path, **s.opts)
    if s.sites is not None:
        assert sites == VM.SITES_HEAD + b"".join(line + b"\n" for line in s.sites)
    s.where(sites, summary, st)
    assert {k: st[k] for k in s.stats} == s.stats


def test_a_revisited_tile_counts_its_failing_columns_once(tmp_path):
    s = CASES["failing_columns_around_the_tile_border"]
    _, _, st = run_and_compare(s.case, tmp_path, **s.opts)
    last = api.last_stats()
    assert last["variants_tiles"] == 2 and last["variants_tiles_revisited"] == 2 and st["columns_low_qual"] == 6


def test_pair_list_with_the_floor(tmp_path):
    s = CASES["read_floor_drops_the_row_that_made_the_site"]
    lst = b"".join(XI.row(n, b"c") for n, _ in s.case.reads[2:])
    _, _, st = run_and_compare(s.case, tmp_path / "read_floor", pairs=lst, **s.opts)
    assert (st["rows_low_qual"], st["rows_not_listed"], st["rows_selected"]) == (1, 1, 3)
    s = CASES["deep_pile_half_below_the_floor"]
    reads = [n for n, _ in s.case.reads]
    lst = b"".join(XI.row(q, b"c", 14) if i % 4 else XI.row(b"c", q) for i, q in enumerate(reads) if i % 3)
    _, _, st = run_and_compare(s.case, tmp_path / "base_floor", pairs=lst, **s.opts)
    assert st["rows_selected"] == 200 and st["rows_not_listed"] == 100 and st["columns_low_qual"] == 100


@pytest.mark.parametrize("name", sorted(OLDER))
def test_identities_on_the_older_inputs(name, tmp_path):
    c, opts = OLDER[name]
    want = VM.variants(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), **opts)

    def same(got):
        assert got[:2] == want[:2] and {k: got[2][k] for k in VM.STAT_KEYS} == want[2]
        assert got[2]["columns_low_qual"] == got[2]["rows_low_qual"] == 0
    same(run_and_compare(c, tmp_path / "off", **opts, **OFF))
    same(run_and_compare(c, tmp_path / "fasta", **opts, min_base_qual=93, min_avg_qual=90.0))
    q = QI.with_quals(c, 5, choices=(10, 11, 40, 93))
    same(run_and_compare(q, tmp_path / "passing", **opts, min_base_qual=10, min_avg_qual=10.0))


def test_refusals_and_their_order(tmp_path):
    s = CASES["site_vanishes"]
    cfa, rfa, paf = s.case.write(tmp_path)
    sites, summ = str(tmp_path / "s.tsv"), str(tmp_path / "t.tsv")

    def refused(word, *a, **k):
        with pytest.raises(api.HlmiError) as e:
            api.variants_q(*a, **k)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
        assert not os.path.exists(sites) and not os.path.exists(summ)
    for bad, word in ((dict(min_base_qual=-1), "min_base_qual"), (dict(min_base_qual=94), "min_base_qual"),
                      (dict(min_avg_qual=-0.5), "min_avg_qual"), (dict(min_avg_qual=float("nan")), "min_avg_qual")):
        # in front of the older call's option refusals and of anything that is read
        refused(word, str(tmp_path / "none.fa"), rfa, paf, sites, summ, min_cov=0, **bad)
    refused("min_cov", cfa, rfa, paf, sites, summ, min_cov=0)
    refused("min_frac", cfa, rfa, paf, sites, summ, min_frac=1.5)
    bad = str(tmp_path / "bad.fq")
    with open(bad, "wb") as f:
        f.write(s.case.reads_bytes().replace(b"+\n" + QI.Q(40) * 4, b"+\n" + QI.Q(40) * 3, 1))
    refused("r0", cfa, bad, paf, sites, summ)
    api.variants_q(cfa, rfa, paf, sites, summ, min_base_qual=93)              # the highest floor is a floor
    with pytest.raises(TypeError):
        api.variants_q(cfa, rfa, paf, sites, summ, qual_weight=1)
