"""GPU: hlmi_phase_ins against its model (tests/phase_ins_model.py) - the three files byte for byte and every integer stat.  The
hand cases of tests/phase_ins_inputs.py; on every older phasing input in which no insertion site takes part, the equality with
hlmi_phase_reach at reach 1 and 2; the shapes (an I op as op 63, 64 and 65, slots at ts + 1 and te - 1 and edge I ops at ts and te,
rows over slots only and over a single slot, an = op over SHORT_RUN and SHORT_RUN + 1 sites of both kinds, both kinds around
PHASE_REACH_TILE, a slot behind a contig junction and a contig without rows, 4 097 rows on a link between a slot and a position),
each with a pair list, with an empty one and with the optional files left out; two strains that differ by insertions alone; the
kernel timers; the refusals, with nothing written."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phase_inputs as HI  # noqa: E402
import phase_ins_inputs as II  # noqa: E402
import phase_ins_model as IM  # noqa: E402
import phase_model as HM  # noqa: E402
import phase_reach_inputs as RI  # noqa: E402
import phase_reach_model as RM  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402

pytestmark = pytest.mark.gpu
HAND, SHAPES = II.hand_cases(), II.shapes()
OLD = {**{n: (h.case, h.opts) for n, h in HI.hand_cases().items()}, **{n: (s.case, s.opts) for n, s in HI.shapes().items()},
       **{n: (h.case, h.opts) for n, h in RI.hand_cases().items()}}
NAMES = ("phase.sites.tsv", "phase.links.tsv", "phase.reads.tsv")
LAST = {}


def ints(st):
    return {k: st[k] for k in IM.STAT_KEYS}


def run_and_compare(c, d, reach, pairs=None, optional=True, **opts):
    """-> the model's (sites, links, reads, stats), after the library's files and stats were found equal to them"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = IM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, reach, **opts)
    out = [os.path.join(d, n) for n in NAMES]
    st = api.phase_ins(cfa, rfa, paf, out[0], out[1] if optional else None, out[2] if optional else None, pairs=lst, reach=reach, **opts)
    LAST.clear()
    LAST.update(api.last_stats())
    assert ints(st) == want[3]
    for path, data in zip(out, want[:3]):
        if optional or path == out[0]:
            with open(path, "rb") as f:
                assert f.read() == data, path
        else:
            assert not os.path.exists(path)
    return want


def three_ways(c, d, reach, **opts):
    """with a pair list (every second read), with an empty one, with the optional files left out"""
    reads = [n for n, _ in c.reads]
    target = {r.split(b"\t")[0]: r.split(b"\t")[5] for r in c.rows}
    lst = b"".join(XI.row(q, target[q], 14) if i % 4 else XI.row(target[q], q) for i, q in enumerate(reads) if i % 2 == 0)
    _, _, _, st = run_and_compare(c, d / "listed", reach, pairs=lst, **opts)
    assert st["rows_selected"] == (len(reads) + 1) // 2 and st["rows_not_listed"] == len(reads) // 2
    sites0, links0, reads0, st0 = run_and_compare(c, d / "empty", reach, pairs=b"", **opts)
    assert (sites0, links0, reads0) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD)
    assert st0["rows_selected"] == st0["sites"] == st0["alleles"] == st0["blocks"] == st0["ins_sites"] == 0 and st0["rows_not_listed"] == len(reads)
    run_and_compare(c, d / "sites_only", reach, optional=False, **opts)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    h = HAND[name]
    sites, links, reads, st = run_and_compare(h.case, tmp_path / "all", h.reach, **h.opts)
    assert sites == HM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert links == HM.LINKS_HEAD + b"".join(line + b"\n" for line in h.links)
    assert reads == HM.READS_HEAD + b"".join(line + b"\n" for line in h.reads)
    assert {k: v for k, v in st.items() if v} == h.stats
    three_ways(h.case, tmp_path, h.reach, **h.opts)


@pytest.mark.parametrize("name", sorted(OLD))
def test_without_a_taking_part_insertion_site_it_is_hlmi_phase_reach(name, tmp_path):
    c, opts = OLD[name]
    for reach in (1, 2):
        want = run_and_compare(c, tmp_path / f"ins{reach}", reach, **opts)
        if want[3]["ins_sites_phasing"]:
            assert "cigar_of" in name, name                        # the only older inputs whose I ops have support
            continue
        cfa, rfa, paf = c.write(str(tmp_path / f"reach{reach}"))
        out = [str(tmp_path / f"reach{reach}" / n) for n in NAMES]
        st = api.phase_reach(cfa, rfa, paf, *out, reach=reach, **opts)
        assert {k: st[k] for k in RM.STAT_KEYS} == {k: want[3][k] for k in RM.STAT_KEYS}
        for path, data in zip(out, want[:3]):
            with open(path, "rb") as f:
                assert f.read() == data, path


@pytest.mark.parametrize("name,reach", [(n, r) for n in sorted(SHAPES) for r in SHAPES[n].reaches])
def test_shape(name, reach, tmp_path):
    s = SHAPES[name]
    s.where(reach, *run_and_compare(s.case, tmp_path, reach, **s.opts))
    assert all(LAST.get(f"kernel_ms.phase_{k}", 0) > 0 for k in ("allele_ins", "link_reach", "assign"))
    assert LAST.get("kernel_ms.phase_allele", 0) == 0 and LAST.get("kernel_ms.phase_link", 0) == 0


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_with_a_list_an_empty_one_and_sites_only(name, tmp_path):
    s = SHAPES[name]
    three_ways(s.case, tmp_path, s.reaches[-1], **s.opts)


def test_strains_that_differ_by_insertions_alone_are_one_block(tmp_path):
    s = II.insertion_strains()
    cfa, rfa, paf = s.case.write(str(tmp_path / "reach"))
    st = api.phase_reach(cfa, rfa, paf, str(tmp_path / "reach" / "s.tsv"), reach=1)
    assert st["sites"] == st["blocks_multi"] == st["sites_phased"] == 0
    sites, _, reads, st = run_and_compare(s.case, tmp_path / "ins", 1)
    assert (st["blocks"], st["blocks_multi"], st["sites_phased"], st["ins_sites_phased"]) == (1, 1, 3, 3)
    assert [(p, a, b) for _, p, a, b, _ in II.site_rows(sites)] == [(300, b"+G", b"300+"), (600, b"+TGA", b"300+"), (900, b"+" + II.S16, b"300+")]
    rr = II.read_rows(reads)
    assert len(rr) == 16 and all(hap == (b"B" if read.startswith(s.minor) else b"A") for read, _, _, _, _, _, _, hap in rr)
    assert LAST.get("kernel_ms.phase_allele_ins", 0) > 0 and LAST.get("kernel_ms.phase_link_reach", 0) > 0
    assert LAST.get("kernel_ms.phase_allele", 0) == 0 and LAST.get("kernel_ms.phase_link", 0) == 0


def test_no_site_phase_kernels_not_launched(tmp_path):
    ref = HI._seq(300, 4)
    sites, links, reads, st = run_and_compare(HI.pile(ref, [{}] * 4, strands="+-"), tmp_path, 3)
    assert (sites, links, reads) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD) and st["sites"] == st["ins_sites"] == 0
    assert LAST.get("kernel_ms.variants_tile", 0) > 0
    assert all(LAST.get(f"kernel_ms.phase_{k}", 0) == 0 for k in ("allele", "allele_ins", "link", "link_reach", "assign"))


def refused(call, word, outs):
    with pytest.raises(api.HlmiError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)
    for p in outs:
        assert not os.path.exists(p)


def test_refusals(tmp_path):
    h = HAND["insertion_and_snp_cis"]
    cfa, rfa, paf = h.case.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("s.tsv", "l.tsv", "r.tsv")]
    for reach in (0, RI.REACH_MAX + 1, -1):
        with pytest.raises(IM.PM.Refused):
            IM.phase(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), reach=reach)
        refused(lambda: api.phase_ins(cfa, rfa, paf, *outs, reach=reach), "hlmi_phase_ins: reach ", outs)
        refused(lambda: api.phase_reads_ins(cfa, rfa, *outs, reach=reach), "hlmi_phase_reads_ins: reach ", outs)
    # hlmi_phase_reach's order: the options, then reach, then the rows
    refused(lambda: api.phase_ins(cfa, rfa, paf, *outs, min_cov=0, min_link=0), "hlmi_phase_ins: min_cov", outs)
    refused(lambda: api.phase_ins(cfa, rfa, paf, *outs, min_link=0, min_agree=0.5), "hlmi_phase_ins: min_link", outs)
    refused(lambda: api.phase_ins(cfa, rfa, paf, *outs, reach=0, min_agree=0.5), "min_agree", outs)
    broken = str(tmp_path / "bad.paf")
    with open(broken, "wb") as f:
        f.write(h.case.paf_bytes().replace(b"cg:Z:5=2I5=1X9=", b"cg:Z:5=2I5=1X8=", 1))
    assert open(broken, "rb").read() != h.case.paf_bytes()
    refused(lambda: api.phase_ins(cfa, rfa, broken, *outs, reach=9), "reach 9", outs)
    refused(lambda: api.phase_ins(cfa, rfa, broken, *outs, reach=2), "bad.paf:1:", outs)
    assert sorted(os.listdir(tmp_path)) == ["bad.paf", "contigs.fa", "reads.fa", "rows.paf"]
