"""GPU: hlmi_phase_reach against its model (tests/phase_reach_model.py) - the three files byte for byte and every integer stat.
reach = 1 on every hand case and shape of tests/phase_inputs.py, equal to hlmi_phase on the same input and run by the new link
kernel; the hand cases of tests/phase_reach_inputs.py; its shapes at reach 2, 3 and 8 (left sites around PHASE_REACH_TILE with
their partners in the next tile, rows over 63 / 64 / 65 / 129 sites and over fewer than d + 1, a row that ends inside a tile, a
contig junction and a contig without rows, 4 097 rows on one far link), each with a pair list, with an empty one and with the
optional files left out; the two-strain pile with one and two noisy sites; the call without a site; hlmi_phase_reads_reach
against the chain hlmi_ava -> hlmi_phase_reach; the refusals, with nothing written."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phase_inputs as HI  # noqa: E402
import phase_model as HM  # noqa: E402
import phase_reach_inputs as RI  # noqa: E402
import phase_reach_model as RM  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import polish_reads_inputs as PR  # noqa: E402
import test_gpu_variants_reads as VR  # noqa: E402

pytestmark = pytest.mark.gpu
OLD_HAND, OLD_SHAPES = HI.hand_cases(), HI.shapes()
OLD = {**{n: (h.case, h.opts) for n, h in OLD_HAND.items()}, **{n: (s.case, s.opts) for n, s in OLD_SHAPES.items()}}
HAND, SHAPES = RI.hand_cases(), RI.shapes()
NAMES = ("phase.sites.tsv", "phase.links.tsv", "phase.reads.tsv")
LAST = {}


def ints(st):
    return {k: st[k] for k in RM.STAT_KEYS}


def run_and_compare(c, d, reach, pairs=None, optional=True, **opts):
    """-> the model's (sites, links, reads, stats), after the library's files and stats were found equal to them"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = RM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, reach, **opts)
    out = [os.path.join(d, n) for n in NAMES]
    st = api.phase_reach(cfa, rfa, paf, out[0], out[1] if optional else None, out[2] if optional else None, pairs=lst, reach=reach, **opts)
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


@pytest.mark.parametrize("name", sorted(OLD))
def test_reach_1_is_hlmi_phase_by_the_new_kernel(name, tmp_path):
    c, opts = OLD[name]
    want = run_and_compare(c, tmp_path / "reach", 1, **opts)
    assert LAST.get("kernel_ms.phase_link_reach", 0) > 0 and LAST.get("kernel_ms.phase_link", 0) == 0
    assert all(want[3][k] == 0 for k in RM.FAR_KEYS)
    cfa, rfa, paf = c.write(str(tmp_path / "plain"))
    out = [str(tmp_path / "plain" / n) for n in NAMES]
    st = api.phase(cfa, rfa, paf, *out, **opts)
    assert {k: st[k] for k in HM.STAT_KEYS} == {k: want[3][k] for k in HM.STAT_KEYS}
    for path, data in zip(out, want[:3]):
        with open(path, "rb") as f:
            assert f.read() == data, path


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    h = HAND[name]
    sites, links, reads, st = run_and_compare(h.case, tmp_path, h.reach, **h.opts)
    assert sites == HM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert links == HM.LINKS_HEAD + b"".join(line + b"\n" for line in h.links)
    assert reads == HM.READS_HEAD + b"".join(line + b"\n" for line in h.reads)
    assert {k: v for k, v in st.items() if v} == h.stats


@pytest.mark.parametrize("name,reach", [(n, r) for n in sorted(SHAPES) for r in SHAPES[n].reaches])
def test_shape(name, reach, tmp_path):
    s = SHAPES[name]
    s.where(reach, *run_and_compare(s.case, tmp_path, reach, **s.opts))
    assert all(LAST.get(f"kernel_ms.phase_{k}", 0) > 0 for k in ("allele", "link_reach", "assign")) and LAST.get("kernel_ms.phase_link", 0) == 0


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_with_a_list_an_empty_one_and_sites_only(name, tmp_path):
    s = SHAPES[name]
    reach = s.reaches[-1]
    reads = [n for n, _ in s.case.reads]
    target = {r.split(b"\t")[0]: r.split(b"\t")[5] for r in s.case.rows}
    lst = b"".join(XI.row(q, target[q], 14) if i % 4 else XI.row(target[q], q) for i, q in enumerate(reads) if i % 2 == 0)
    _, _, _, st = run_and_compare(s.case, tmp_path / "listed", reach, pairs=lst, **s.opts)
    assert st["rows_selected"] == (len(reads) + 1) // 2 and st["rows_not_listed"] == len(reads) // 2
    sites0, links0, reads0, st0 = run_and_compare(s.case, tmp_path / "empty", reach, pairs=b"", **s.opts)
    assert (sites0, links0, reads0) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD)
    assert st0["rows_selected"] == st0["sites"] == st0["alleles"] == st0["blocks"] == 0 and st0["rows_not_listed"] == len(reads)
    run_and_compare(s.case, tmp_path / "sites_only", reach, optional=False, **s.opts)


def test_no_site_phase_kernels_not_launched(tmp_path):
    ref = HI._seq(2 * HI.T + 7, 4)
    sites, links, reads, st = run_and_compare(HI.pile(ref, [{}] * 4, strands="+-"), tmp_path, 3)
    assert (sites, links, reads) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD) and st["sites"] == 0
    assert LAST.get("kernel_ms.variants_tile", 0) > 0
    assert all(LAST.get(f"kernel_ms.phase_{k}", 0) == 0 for k in ("allele", "link", "link_reach", "assign"))


def test_one_noisy_site_cuts_at_reach_1_and_is_bridged_at_reach_2(tmp_path):
    s = RI.noisy_two_strains(1)
    sites, _, _, st = run_and_compare(s.case, tmp_path / "one", 1)
    blocks = [b for _, _, _, b, _ in HI.site_rows(sites)]
    assert (st["blocks"], st["blocks_multi"]) == (3, 2) and blocks.count(s.noise[0] + 1) == 1
    sites, _, reads, st = run_and_compare(s.case, tmp_path / "two", 2)
    assert (st["blocks"], st["sites_bridged"], st["joins_far"]) == (1, 1, 1)
    assert (st["read_records"], st["reads_a"], st["reads_b"], st["reads_tie"]) == (90, 15, 75, 0)
    assert [p for _, p, _, _, ph in HI.site_rows(sites) if ph == b"."] == s.noise
    for read, _, _, _, a, b, _, hap in HI.read_rows(reads):
        assert (hap, b) == (b"A", 0) if read.startswith(b"min_") else (hap, a) == (b"B", 0), read


def test_two_noisy_sites_cut_at_reach_2_and_are_bridged_at_reach_3(tmp_path):
    s = RI.noisy_two_strains(2)
    _, _, _, st = run_and_compare(s.case, tmp_path / "two", 2)
    assert st["blocks"] >= 3 and st["sites_bridged"] == 0
    sites, _, _, st = run_and_compare(s.case, tmp_path / "three", 3)
    assert (st["blocks"], st["sites_bridged"], st["joins_far"], st["read_records"]) == (1, 2, 1, 90)
    assert [p for _, p, _, _, ph in HI.site_rows(sites) if ph == b"."] == s.noise


def test_phase_reads_reach_is_the_chain(tmp_path):
    contigs, reads, _, _ = VR.two_strain_set(False)
    d = str(tmp_path)
    cfa, rfa, paf = (os.path.join(d, n) for n in ("contigs.fa", "reads.fa", "chain.paf"))
    with open(cfa, "wb") as f:
        f.write(PR.fasta(contigs))
    with open(rfa, "wb") as f:
        f.write(PR.fasta(reads))
    api.ava(cfa, rfa, paf, VR.ava_opts(False))
    with open(paf, "rb") as f:
        paf_bytes = f.read()
    opts = dict(min_len=300, min_iden=0.9, min_cov=1, min_alt=1, min_frac=0.0, min_link=1, min_agree=0.6)     # every column that differs
    want = RM.phase(PR.fasta(contigs), PR.fasta(reads), paf_bytes, None, 3, **opts)
    assert want[3]["sites"] >= 3 and want[3]["links_far"] >= 1
    for who in ("chain", "direct"):
        out = [os.path.join(d, f"{who}.{e}") for e in NAMES]
        st = (api.phase_reach(cfa, rfa, paf, *out, reach=3, **opts) if who == "chain" else
              api.phase_reads_reach(cfa, rfa, *out, VR.ava_opts(False), reach=3, **opts))
        assert ints(st) == want[3], who
        for p, data in zip(out, want[:3]):
            with open(p, "rb") as f:
                assert f.read() == data, (who, p)


def refused(call, word, outs):
    with pytest.raises(api.HlmiError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)
    for p in outs:
        assert not os.path.exists(p)


def test_refusals(tmp_path):
    h = OLD_HAND["cis"]
    cfa, rfa, paf = h.case.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("s.tsv", "l.tsv", "r.tsv")]
    for reach in (0, RI.REACH_MAX + 1, -1):
        with pytest.raises(RM.PM.Refused):
            RM.phase(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), reach=reach)
        refused(lambda: api.phase_reach(cfa, rfa, paf, *outs, reach=reach), "hlmi_phase_reach: reach ", outs)
        refused(lambda: api.phase_reads_reach(cfa, rfa, *outs, reach=reach), "hlmi_phase_reads_reach: reach ", outs)
    # behind min_agree's refusal, in front of a row's
    refused(lambda: api.phase_reach(cfa, rfa, paf, *outs, reach=0, min_agree=0.5), "min_agree", outs)
    broken = str(tmp_path / "bad.paf")
    with open(broken, "wb") as f:
        f.write(h.case.paf_bytes().replace(b"cg:Z:2=1X3=1X13=", b"cg:Z:2=1X3=1X12=", 1))
    refused(lambda: api.phase_reach(cfa, rfa, broken, *outs, reach=9), "reach 9", outs)
    refused(lambda: api.phase_reach(cfa, rfa, broken, *outs, reach=2), "bad.paf:1:", outs)
    assert sorted(os.listdir(tmp_path)) == ["bad.paf", "contigs.fa", "reads.fa", "rows.paf"]
