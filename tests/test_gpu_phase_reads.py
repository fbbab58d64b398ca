"""GPU: hlmi_phase_reads against the chain hlmi_ava -> PAF -> hlmi_phase: the three files byte for byte and every integer stat, and
the chain's against the model (tests/phase_model.py) on the PAF hlmi_ava wrote.  The two-strain sets of
tests/test_gpu_variants_reads.py - two strains of 3 kb, each strain's genome a contig, long reads with the overlapper's long
constants and 150-base reads with its short ones - with and without the same-strain list; stub_oh >= 0 is refused under the entry
point's name; driver.phase_tables writes its three files and they equal the model's."""
import os
import sys

import pytest

from hylight_amd import api, driver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phase_inputs as HI  # noqa: E402
import phase_model as HM  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import test_gpu_variants_reads as VR  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("sites.tsv", "links.tsv", "reads.tsv")


def ints(st):
    return {k: st[k] for k in HM.STAT_KEYS}


class Chain:
    """a set's files and the PAF hlmi_ava writes for them"""

    def __init__(self, short, d):
        self.short, self.d = short, str(d)
        self.contigs, self.reads, self.same_strain, self.snps = VR.two_strain_set(short)
        self.cfa, self.rfa, self.paf = (os.path.join(self.d, n) for n in ("contigs.fa", "reads.fa", "chain.paf"))
        with open(self.cfa, "wb") as f:
            f.write(RI.fasta(self.contigs))
        with open(self.rfa, "wb") as f:
            f.write(RI.fasta(self.reads))
        api.ava(self.cfa, self.rfa, self.paf, VR.ava_opts(short))
        with open(self.paf, "rb") as f:
            self.paf_bytes = f.read()
        self.opts = dict(min_len=70) if short else dict(min_len=300, min_iden=0.9)
        self.n = 0

    def check(self, lst, optional=True, **more):
        """model == chain == fused call -> the model's (sites, links, reads, stats)"""
        self.n += 1
        opts = {**self.opts, **more}
        path = None
        if lst is not None:
            path = os.path.join(self.d, f"list{self.n}.paf")
            with open(path, "wb") as f:
                f.write(lst)
        want = HM.phase(RI.fasta(self.contigs), RI.fasta(self.reads), self.paf_bytes, lst, **opts)
        for who in ("chain", "direct"):
            out = [os.path.join(self.d, f"{who}{self.n}.{e}") for e in NAMES]
            given = out if optional else [out[0], None, None]
            st = (api.phase(self.cfa, self.rfa, self.paf, *given, pairs=path, **opts) if who == "chain" else
                  api.phase_reads(self.cfa, self.rfa, *given, VR.ava_opts(self.short), pairs=path, **opts))
            assert ints(st) == want[3], who
            for p, g, data in zip(out, given, want[:3]):
                if g is None:
                    assert not os.path.exists(p)
                    continue
                with open(p, "rb") as f:
                    assert f.read() == data, (who, p)
        return want


@pytest.fixture(scope="module")
def long_chain(tmp_path_factory):
    return Chain(False, tmp_path_factory.mktemp("phase_long"))


def test_long_reads(long_chain):
    c = long_chain
    sites, links, reads, st = c.check(None)
    assert st["rows_selected"] >= 40 and st["contigs_covered"] == 2 and st["sites"] >= 1
    assert st["alleles"] >= st["read_records"] >= 2 and st["reads_b"] + st["reads_tie"] >= 1      # a site has two alt votes at least
    c.check(None, optional=False)
    c.check(None, min_cov=1, min_alt=1, min_frac=0.0, min_link=1, min_agree=0.6)      # every column that differs anywhere


def test_long_reads_with_the_same_strain_list(long_chain):
    c = long_chain
    _, _, _, st0 = c.check(None)
    sites, _, reads, st = c.check(c.same_strain)
    assert st["rows_not_listed"] >= 10 and st["pairs_listed"] == 60
    assert not {p for _, p, _, _, _ in HI.site_rows(sites)} & set(c.snps) and st0["sites"] >= 1
    sites0, links0, reads0, st_empty = c.check(b"")
    assert (sites0, links0, reads0) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD) and st_empty["rows_selected"] == 0


def test_short_reads(tmp_path):
    c = Chain(True, tmp_path)
    _, _, _, st0 = c.check(None)
    assert st0["rows_selected"] >= 200 and st0["sites"] >= 1 and st0["read_records"] >= 1
    sites, _, _, st = c.check(c.same_strain)
    assert st["rows_not_listed"] >= 50 and not {p for _, p, _, _, _ in HI.site_rows(sites)} & set(c.snps)


def test_refusals(long_chain, tmp_path):
    c = long_chain
    outs = [str(tmp_path / n) for n in NAMES]
    o = VR.ava_opts()
    o.stub_oh = 0
    with pytest.raises(api.HlmiError) as e:
        api.phase_reads(c.cfa, c.rfa, *outs, o)
    assert e.value.code == -1 and "stub_oh" in str(e.value) and "hlmi_phase_reads" in str(e.value)
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(RI.fasta(c.reads) + b">r3\nACGTACGT\n")
    with pytest.raises(api.HlmiError) as e:
        api.phase_reads(c.cfa, twice, *outs, VR.ava_opts())
    assert e.value.code == -1 and "two records are named r3" in str(e.value)
    with pytest.raises(api.HlmiError) as e:
        api.phase_reads(c.cfa, c.rfa, *outs, VR.ava_opts(), min_agree=0.4)
    assert e.value.code == -1 and "min_agree" in str(e.value) and "hlmi_phase_reads" in str(e.value)
    assert not any(os.path.exists(p) for p in outs)


def test_driver_phase_tables(long_chain, tmp_path):
    c = long_chain
    out = tmp_path / "out"
    out.mkdir()
    lst = str(tmp_path / "ov_long_ref.paf")
    with open(lst, "wb") as f:
        f.write(c.same_strain)
    st = driver.phase_tables(c.cfa, c.rfa, None, str(out), 0, long_pairs=lst)
    assert sorted(os.listdir(out)) == [f"final_contigs.long.phase.{e}" for e in ("links.tsv", "reads.tsv", "sites.tsv")]
    want = HM.phase(RI.fasta(c.contigs), RI.fasta(c.reads), c.paf_bytes, c.same_strain)
    for e, data in zip(NAMES, want[:3]):
        assert (out / f"final_contigs.long.phase.{e}").read_bytes() == data
    assert ints(st["long"]) == want[3]
