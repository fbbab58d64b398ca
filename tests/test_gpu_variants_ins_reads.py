"""GPU: hlmi_variants_reads_ins against the chain hlmi_ava -> PAF -> hlmi_variants_ins: the three files byte for byte and every
integer stat, and the chain's against the model (tests/variants_ins_model.py) on the PAF hlmi_ava wrote.  The two-strain set of
tests/test_gpu_variants_reads.py (hylight_amd/simulate.py: two strains of 3 kb, tens of reads of both) with three bases cut out
of the first strain's contig and twenty out of the second's: the reads carry them, so with the same-strain list - every read on
its own strain's contig - the first contig has an insertion site with a length and bases, the second one whose evidence is long
rows.  With the overlapper's long constants and, cut into 150-base reads, with its short ones; with and without the list and
with an empty one; the refusals; driver.variant_tables with ins=True writes its three files and they equal the model's."""
import os
import sys

import numpy as np
import pytest

from hylight_amd import api, driver, simulate as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_pairs_inputs as XI  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import variants_ins_model as IM  # noqa: E402

pytestmark = pytest.mark.gpu
CUTS = ((1200, 3), (2000, 20))                  # (position, bases) cut out of contig 0 and contig 1


def ava_opts(short=False):
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    return o


def ints(st):
    return {k: st[k] for k in IM.STAT_KEYS}


def read(p):
    with open(p, "rb") as f:
        return f.read()


def two_strain_set(short):
    """-> (contigs [(name, bases)], reads [(name, bases)], same-strain list bytes)"""
    reads, strains = S.simulate_reads(seed=7301, n_strains=2, genome_len=3000, n_reads=60, mean_len=1000, min_len=600, max_len=1500,
                                      snp_rate=0.01)
    genomes = [g.tobytes() for g in strains]
    contigs = [(f"s{k}", g[:at] + g[at + n:]) for k, (g, (at, n)) in enumerate(zip(genomes, CUTS))]
    if not short:
        rr = [(r.name, r.seq.tobytes(), r.strain) for r in reads]
    else:
        rng = np.random.default_rng(7302)
        rr = [(n, s, k) for k, g in enumerate(genomes) for n, s in RI.sample_reads(rng, g, 160, 150, 150, prefix=f"q{k}_")]
    lst = b"".join(XI.row(n.encode(), contigs[k][0].encode(), 14) for n, _, k in rr)
    return contigs, [(n, s) for n, s, _ in rr], lst


class Chain:
    """a set's files and the PAF hlmi_ava writes for them"""

    def __init__(self, short, d):
        self.short, self.d = short, str(d)
        self.contigs, self.reads, self.same_strain = two_strain_set(short)
        self.cfa, self.rfa, self.paf = (os.path.join(self.d, n) for n in ("contigs.fa", "reads.fa", "chain.paf"))
        with open(self.cfa, "wb") as f:
            f.write(RI.fasta(self.contigs))
        with open(self.rfa, "wb") as f:
            f.write(RI.fasta(self.reads))
        api.ava(self.cfa, self.rfa, self.paf, ava_opts(short))
        self.paf_bytes = read(self.paf)
        self.opts = dict(min_len=70) if short else dict(min_len=300, min_iden=0.9)
        self.n = 0

    def check(self, lst, summary=True, **more):
        """model == chain == fused call -> the model's (sites, ins, summary, stats)"""
        self.n += 1
        opts = {**self.opts, **more}
        path = None
        if lst is not None:
            path = os.path.join(self.d, f"list{self.n}.paf")
            with open(path, "wb") as f:
                f.write(lst)
        want = IM.variants_ins(RI.fasta(self.contigs), RI.fasta(self.reads), self.paf_bytes, lst, **opts)
        for who in ("chain", "direct"):
            sites, ins, summ = (os.path.join(self.d, f"{who}{self.n}.{e}") for e in ("sites.tsv", "ins.tsv", "summary.tsv"))
            b = summ if summary else None
            st = (api.variants_ins(self.cfa, self.rfa, self.paf, sites, ins, b, pairs=path, **opts) if who == "chain" else
                  api.variants_ins_reads(self.cfa, self.rfa, sites, ins, b, ava_opts(self.short), pairs=path, **opts))
            print(who, ints(st))
            assert ints(st) == want[3], who
            assert read(sites) == want[0], who
            assert read(ins) == want[1], who
            if summary:
                assert read(summ) == want[2], who
            else:
                assert not os.path.exists(summ)
        return want


@pytest.fixture(scope="module")
def long_chain(tmp_path_factory):
    return Chain(False, tmp_path_factory.mktemp("variants_ins_long"))


def near(rows, contig, at, width=12):
    return [r for r in rows if r[0] == contig and abs(r[1] - at) <= width]


def test_long_reads(long_chain):
    c = long_chain
    sites, ins, summary, st = c.check(None)
    # (a read's one row is its longest: across a cut that is the row on the OTHER strain's contig, which has those bases - what
    # the sites are without a list is the model's to say; with the list, below, every read votes on its own strain's contig)
    assert st["rows_selected"] >= 40 and st["contigs_covered"] == 2
    c.check(None, summary=False)
    c.check(None, min_cov=1, min_alt=1, min_frac=0.0)                           # every slot any row inserts at
    # out_sites is the older call's file
    old = os.path.join(c.d, "old.sites.tsv")
    api.variants_reads(c.cfa, c.rfa, old, None, ava_opts(), **c.opts)
    assert read(old) == sites


def test_long_reads_with_the_same_strain_list(long_chain):
    c = long_chain
    _, ins, _, st = c.check(c.same_strain)
    assert st["rows_not_listed"] >= 10 and st["rows_selected"] >= 40 and st["pairs_listed"] == 60
    rows = IM.ins_rows(ins)
    three = near(rows, b"s0", CUTS[0][0])
    assert three and max(three, key=lambda r: r[3])[5] == 3                     # the bases the contig lacks: a length of three
    twenty = near(rows, b"s1", CUTS[1][0], 24)
    assert twenty and max(twenty, key=lambda r: r[4])[4] >= 3 and st["ins_long"] >= 3       # long rows: more than 16 bases
    _, ins0, _, st0 = c.check(b"")
    assert ins0 == IM.INS_HEAD and st0["rows_selected"] == st0["slots_callable"] == st0["ins_sites"] == st0["ins_long"] == 0


def test_short_reads(tmp_path):
    c = Chain(True, tmp_path)
    _, _, _, st = c.check(None)
    assert st["rows_selected"] >= 200
    _, ins, _, st = c.check(c.same_strain)
    assert st["rows_not_listed"] >= 50 and near(IM.ins_rows(ins), b"s0", CUTS[0][0])


def test_refusals(long_chain, tmp_path):
    c = long_chain
    sites, ins, summ = str(tmp_path / "s.tsv"), str(tmp_path / "i.tsv"), str(tmp_path / "t.tsv")
    o = ava_opts()
    o.stub_oh = 0
    with pytest.raises(api.HlmiError) as e:
        api.variants_ins_reads(c.cfa, c.rfa, sites, None, summ, o)              # out_ins NULL comes first
    assert e.value.code == -1 and "out_ins" in str(e.value) and "hlmi_variants_reads_ins" in str(e.value)
    with pytest.raises(api.HlmiError) as e:
        api.variants_ins_reads(c.cfa, c.rfa, sites, ins, summ, o)
    assert e.value.code == -1 and "stub_oh" in str(e.value) and "hlmi_variants_reads_ins" in str(e.value)
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(RI.fasta(c.reads) + b">r3\nACGTACGT\n")
    with pytest.raises(api.HlmiError) as e:
        api.variants_ins_reads(c.cfa, twice, sites, ins, summ, ava_opts())
    assert e.value.code == -1 and "two records are named r3" in str(e.value)
    lst = str(tmp_path / "pairs.paf")
    with open(lst, "wb") as f:
        f.write(XI.row(b"r1", b"s0") + XI.row(b"r2", b"s0", 4))
    with pytest.raises(api.HlmiError) as e:
        api.variants_ins_reads(c.cfa, c.rfa, sites, ins, summ, ava_opts(), pairs=lst)
    assert e.value.code == -1 and "pairs.paf:2:" in str(e.value)
    with pytest.raises(api.HlmiError) as e:
        api.variants_ins_reads(c.cfa, c.rfa, sites, ins, summ, ava_opts(), min_frac=2.0)
    assert e.value.code == -1 and "min_frac" in str(e.value)
    assert not os.path.exists(sites) and not os.path.exists(ins) and not os.path.exists(summ)


def test_driver_variant_tables_with_insertions(long_chain, tmp_path):
    c = long_chain
    out = tmp_path / "out"
    out.mkdir()
    lst = str(tmp_path / "ov_long_ref.paf")
    with open(lst, "wb") as f:
        f.write(c.same_strain)
    st = driver.variant_tables(c.cfa, c.rfa, None, str(out), 0, long_pairs=lst, ins=True)
    assert sorted(os.listdir(out)) == ["final_contigs.long.variants.ins.tsv", "final_contigs.long.variants.summary.tsv",
                                       "final_contigs.long.variants.tsv"]
    want = IM.variants_ins(RI.fasta(c.contigs), RI.fasta(c.reads), c.paf_bytes, c.same_strain)
    assert (out / "final_contigs.long.variants.tsv").read_bytes() == want[0]
    assert (out / "final_contigs.long.variants.ins.tsv").read_bytes() == want[1]
    assert (out / "final_contigs.long.variants.summary.tsv").read_bytes() == want[2]
    assert ints(st["long"]) == want[3]
