"""GPU: hlmi_variants_reads against the chain hlmi_ava -> PAF -> hlmi_variants: both files byte for byte and every integer stat,
and the chain's against the model (tests/variants_model.py) on the PAF hlmi_ava wrote.  A small two-strain set of
hylight_amd/simulate.py - two strains of 3 kb that differ at about 1 % of their bases, each strain's genome a contig, tens of
reads of both - with the overlapper's long constants and, cut into 150-base reads, with its short ones; with and without the
same-strain list.  Without the list the sister strain's alleles show as sites; stub_oh >= 0 and a name twice are refused;
driver.variant_tables writes its files and they equal the model's."""
import os
import sys

import numpy as np
import pytest

from hylight_amd import api, driver, simulate as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_pairs_inputs as XI  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import variants_inputs as VI  # noqa: E402
import variants_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu


def ava_opts(short=False):
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    return o


def ints(st):
    return {k: st[k] for k in VM.STAT_KEYS}


def two_strain_set(short):
    """-> (contigs [(name, bases)], reads [(name, bases)], same-strain list bytes, positions where the strains differ)"""
    reads, strains = S.simulate_reads(seed=7301, n_strains=2, genome_len=3000, n_reads=60, mean_len=1000, min_len=600, max_len=1500,
                                      snp_rate=0.01)
    contigs = [(f"s{k}", g.tobytes()) for k, g in enumerate(strains)]
    snps = [p for p in range(3000) if contigs[0][1][p] != contigs[1][1][p]]
    if not short:
        rr = [(r.name, r.seq.tobytes(), r.strain) for r in reads]
    else:
        rng = np.random.default_rng(7302)
        rr = [(n, s, k) for k, (_, g) in enumerate(contigs) for n, s in RI.sample_reads(rng, g, 160, 150, 150, prefix=f"q{k}_")]
    lst = b"".join(XI.row(n.encode(), contigs[k][0].encode(), 14) for n, _, k in rr)
    return contigs, [(n, s) for n, s, _ in rr], lst, snps


class Chain:
    """a set's files and the PAF hlmi_ava writes for them"""

    def __init__(self, short, d):
        self.short, self.d = short, str(d)
        self.contigs, self.reads, self.same_strain, self.snps = two_strain_set(short)
        self.cfa, self.rfa, self.paf = (os.path.join(self.d, n) for n in ("contigs.fa", "reads.fa", "chain.paf"))
        with open(self.cfa, "wb") as f:
            f.write(RI.fasta(self.contigs))
        with open(self.rfa, "wb") as f:
            f.write(RI.fasta(self.reads))
        api.ava(self.cfa, self.rfa, self.paf, ava_opts(short))
        with open(self.paf, "rb") as f:
            self.paf_bytes = f.read()
        self.opts = dict(min_len=70) if short else dict(min_len=300, min_iden=0.9)
        self.n = 0

    def check(self, lst, summary=True, **more):
        """model == chain == fused call -> the model's (sites, summary, stats)"""
        self.n += 1
        opts = {**self.opts, **more}
        path = None
        if lst is not None:
            path = os.path.join(self.d, f"list{self.n}.paf")
            with open(path, "wb") as f:
                f.write(lst)
        want = VM.variants(RI.fasta(self.contigs), RI.fasta(self.reads), self.paf_bytes, lst, **opts)
        for who in ("chain", "direct"):
            sites, summ = (os.path.join(self.d, f"{who}{self.n}.{e}") for e in ("sites.tsv", "summary.tsv"))
            b = summ if summary else None
            st = (api.variants(self.cfa, self.rfa, self.paf, sites, b, pairs=path, **opts) if who == "chain" else
                  api.variants_reads(self.cfa, self.rfa, sites, b, ava_opts(self.short), pairs=path, **opts))
            assert ints(st) == want[2], who
            with open(sites, "rb") as f:
                assert f.read() == want[0], who
            if summary:
                with open(summ, "rb") as f:
                    assert f.read() == want[1], who
            else:
                assert not os.path.exists(summ)
        return want


@pytest.fixture(scope="module")
def long_chain(tmp_path_factory):
    return Chain(False, tmp_path_factory.mktemp("variants_long"))


def test_long_reads(long_chain):
    c = long_chain
    assert 15 <= len(c.snps) <= 60
    sites, summary, st = c.check(None)
    assert st["rows_selected"] >= 40 and st["contigs_covered"] == 2 and st["sites"] >= 1
    assert {p for _, p, _ in VI.site_rows(sites)} & set(c.snps)                 # the sister strain's alleles show
    c.check(None, summary=False)
    c.check(None, min_cov=1, min_alt=1, min_frac=0.0)                           # every column that differs anywhere


def test_long_reads_with_the_same_strain_list(long_chain):
    c = long_chain
    sites0, _, st0 = c.check(None)
    sites, _, st = c.check(c.same_strain)
    assert st["rows_not_listed"] >= 10 and st["rows_selected"] >= 40 and st["pairs_listed"] == 60
    at_snps = lambda s: sum(1 for _, p, _ in VI.site_rows(s) if p in set(c.snps))     # noqa: E731
    assert at_snps(sites0) >= 1 and at_snps(sites) == 0                          # with the list they vanish
    _, _, st_empty = c.check(b"")
    assert st_empty["rows_selected"] == 0 and st_empty["sites"] == 0 and st_empty["rows_not_listed"] > 0


def test_short_reads(tmp_path):
    c = Chain(True, tmp_path)
    sites0, _, st0 = c.check(None)
    assert st0["rows_selected"] >= 200 and st0["sites"] >= 1
    sites, _, st = c.check(c.same_strain)
    assert st["rows_not_listed"] >= 50 and not {p for _, p, _ in VI.site_rows(sites)} & set(c.snps)


def test_refusals(long_chain, tmp_path):
    c = long_chain
    sites, summ = str(tmp_path / "s.tsv"), str(tmp_path / "t.tsv")
    o = ava_opts()
    o.stub_oh = 0
    with pytest.raises(api.HlmiError) as e:
        api.variants_reads(c.cfa, c.rfa, sites, summ, o)
    assert e.value.code == -1 and "stub_oh" in str(e.value) and "hlmi_variants_reads" in str(e.value)
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(RI.fasta(c.reads) + b">r3\nACGTACGT\n")
    with pytest.raises(api.HlmiError) as e:
        api.variants_reads(c.cfa, twice, sites, summ, ava_opts())
    assert e.value.code == -1 and "two records are named r3" in str(e.value)
    lst = str(tmp_path / "pairs.paf")
    with open(lst, "wb") as f:
        f.write(XI.row(b"r1", b"s0") + XI.row(b"r2", b"s0", 4))
    with pytest.raises(api.HlmiError) as e:
        api.variants_reads(c.cfa, c.rfa, sites, summ, ava_opts(), pairs=lst)
    assert e.value.code == -1 and "pairs.paf:2:" in str(e.value)
    with pytest.raises(api.HlmiError) as e:
        api.variants_reads(c.cfa, c.rfa, sites, summ, ava_opts(), min_frac=2.0)
    assert e.value.code == -1 and "min_frac" in str(e.value)
    assert not os.path.exists(sites) and not os.path.exists(summ)


def test_driver_variant_tables(long_chain, tmp_path):
    c = long_chain
    out = tmp_path / "out"
    out.mkdir()
    lst = str(tmp_path / "ov_long_ref.paf")
    with open(lst, "wb") as f:
        f.write(c.same_strain)
    st = driver.variant_tables(c.cfa, c.rfa, None, str(out), 0, long_pairs=lst)
    assert sorted(os.listdir(out)) == ["final_contigs.long.variants.summary.tsv", "final_contigs.long.variants.tsv"]
    want = VM.variants(RI.fasta(c.contigs), RI.fasta(c.reads), c.paf_bytes, c.same_strain)
    assert (out / "final_contigs.long.variants.tsv").read_bytes() == want[0]
    assert (out / "final_contigs.long.variants.summary.tsv").read_bytes() == want[1]
    assert ints(st["long"]) == want[2]
