"""GPU: hlmi_phase_reads_ins against the chain hlmi_ava -> PAF -> hlmi_phase_ins: the three files byte for byte and every integer
stat, and the chain's against the model (tests/phase_ins_model.py) on the PAF hlmi_ava wrote.  The two-strain set of
tests/test_gpu_variants_ins_reads.py (simulated reads of two strains with SNPs, three bases cut out of the first strain's contig
and twenty out of the second's, so that the reads carry indels against their contigs): the fused call reads the overlapper's
resident read codes (phase_allele_ins_kernel<READS_CODES>), the chain the reads' ASCII.  With the same-strain list the first
contig's insertion site of three bases takes part and sits in a block with SNPs; with and without the list, with an empty one,
at reach 1 and 3; driver.phase_tables with ins=True writes the same three files."""
import os
import sys

import pytest

from hylight_amd import api, driver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phase_ins_inputs as II  # noqa: E402
import phase_ins_model as IM  # noqa: E402
import phase_model as HM  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import test_gpu_variants_ins_reads as VR  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("sites.tsv", "links.tsv", "reads.tsv")


def ints(st):
    return {k: st[k] for k in IM.STAT_KEYS}


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    return VR.Chain(False, tmp_path_factory.mktemp("phase_ins_long"))


def check(c, lst, reach, optional=True, **more):
    """model == chain == fused call -> the model's (sites, links, reads, stats)"""
    c.n += 1
    opts = {**c.opts, **more}
    path = None
    if lst is not None:
        path = os.path.join(c.d, f"list{c.n}.paf")
        with open(path, "wb") as f:
            f.write(lst)
    want = IM.phase(RI.fasta(c.contigs), RI.fasta(c.reads), c.paf_bytes, lst, reach, **opts)
    for who in ("chain", "direct"):
        out = [os.path.join(c.d, f"{who}{c.n}.{e}") for e in NAMES]
        given = out if optional else [out[0], None, None]
        st = (api.phase_ins(c.cfa, c.rfa, c.paf, *given, pairs=path, reach=reach, **opts) if who == "chain" else
              api.phase_reads_ins(c.cfa, c.rfa, *given, VR.ava_opts(False), pairs=path, reach=reach, **opts))
        assert ints(st) == want[3], who
        for p, data in zip(out, want[:3]):
            if optional or p == out[0]:
                assert VR.read(p) == data, (who, p)
            else:
                assert not os.path.exists(p)
    return want


def test_the_fused_call_is_the_chain(chain):
    _, _, _, st = check(chain, None, 1)
    assert st["rows_selected"] >= 40 and st["contigs_covered"] == 2 and st["sites"] >= 3
    check(chain, None, 3, min_cov=1, min_alt=1, min_frac=0.0, min_link=1, min_agree=0.6)      # every column and slot that differs
    check(chain, None, 2, optional=False)


def test_with_the_same_strain_list_the_insertion_takes_part(chain):
    sites, _, _, st = check(chain, chain.same_strain, 2, min_link=2)
    assert st["rows_not_listed"] >= 10 and st["pairs_listed"] == 60 and st["ins_sites_phasing"] >= 1 and st["ins_long"] >= 3
    three = [r for r in II.site_rows(sites) if r[0] == b"s0" and r[2].startswith(b"+") and abs(r[1] - VR.CUTS[0][0]) <= 12]
    assert any(len(r[2]) == 4 for r in three)                                   # the bases the contig lacks: + and three of them
    sites0, links0, reads0, st0 = check(chain, b"", 2)
    assert (sites0, links0, reads0) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD)
    assert st0["rows_selected"] == st0["alleles"] == st0["ins_sites"] == st0["ins_sites_left_out"] == 0


def test_driver_phase_tables_with_insertions(chain, tmp_path):
    c = chain
    out = tmp_path / "out"
    out.mkdir()
    lst = str(tmp_path / "ov_long_ref.paf")
    with open(lst, "wb") as f:
        f.write(c.same_strain)
    st = driver.phase_tables(c.cfa, c.rfa, None, str(out), 0, long_pairs=lst, reach=2, ins=True)
    assert sorted(os.listdir(out)) == [f"final_contigs.long.phase.{e}" for e in ("links.tsv", "reads.tsv", "sites.tsv")]
    want = IM.phase(RI.fasta(c.contigs), RI.fasta(c.reads), c.paf_bytes, c.same_strain, 2)
    for e, data in zip(NAMES, want[:3]):
        assert (out / f"final_contigs.long.phase.{e}").read_bytes() == data, e
    assert ints(st["long"]) == want[3]
