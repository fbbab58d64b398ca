"""GPU: hlmi_depth_reads against the chain hlmi_ava -> PAF -> hlmi_depth: both files byte for byte and every integer stat, and the
chain's against the model (tests/depth_model.py) on the PAF hlmi_ava wrote.  The long and the short input of
tests/polish_reads_inputs.py, with and without a pair list; the tie between two contigs; stub_oh >= 0 and a name twice are
refused; driver.depth_tables writes its four files and the tables equal the model's."""
import os
import sys

import numpy as np
import pytest

from hylight_amd import api, driver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_model as DM  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402

pytestmark = pytest.mark.gpu


def ava_opts(short=False):
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    return o


def ints(st):
    return {k: st[k] for k in DM.STAT_KEYS}


class Chain:
    """an input's files and the PAF hlmi_ava writes for them"""

    def __init__(self, inp, d):
        self.inp, self.d = inp, str(d)
        self.cfa, self.rfa, self.paf = (os.path.join(self.d, n) for n in ("contigs.fa", "reads.fa", "chain.paf"))
        with open(self.cfa, "wb") as f:
            f.write(RI.fasta(inp.contigs))
        with open(self.rfa, "wb") as f:
            f.write(RI.fasta(inp.reads))
        api.ava(self.cfa, self.rfa, self.paf, ava_opts(inp.short))
        with open(self.paf, "rb") as f:
            self.paf_bytes = f.read()
        self.pairs = list(dict.fromkeys((r["q"], r["t"]) for r in RI.paf_rows(self.paf_bytes)))
        self.opts = {k: v for k, v in inp.opts.items() if k in ("min_len", "min_iden")}
        self.n = 0

    def check(self, lst, bedgraph=True):
        """model == chain == fused call -> the model's (tsv, bed, stats)"""
        self.n += 1
        path = None
        if lst is not None:
            path = os.path.join(self.d, f"list{self.n}.paf")
            with open(path, "wb") as f:
                f.write(lst)
        want = DM.depth(RI.fasta(self.inp.contigs), RI.fasta(self.inp.reads), self.paf_bytes, lst, bedgraph=bedgraph, **self.opts)
        for who in ("chain", "direct"):
            tsv, bed = (os.path.join(self.d, f"{who}{self.n}.{e}") for e in ("tsv", "bedgraph"))
            b = bed if bedgraph else None
            st = (api.depth(self.cfa, self.rfa, self.paf, tsv, b, pairs=path, **self.opts) if who == "chain" else
                  api.depth_reads(self.cfa, self.rfa, tsv, b, ava_opts(self.inp.short), pairs=path, **self.opts))
            assert ints(st) == want[2], who
            with open(tsv, "rb") as f:
                assert f.read() == want[0], who
            if bedgraph:
                with open(bed, "rb") as f:
                    assert f.read() == want[1], who
            else:
                assert not os.path.exists(bed)
        return want


@pytest.fixture(scope="module")
def long_chain(tmp_path_factory):
    return Chain(RI.every_kind_long(), tmp_path_factory.mktemp("depth_long"))


def test_long_reads(long_chain):
    c = long_chain
    tsv, bed, st = c.check(None)
    assert st["rows_selected"] >= 40 and st["contigs_covered"] == 3 and st["runs"] > 20
    assert abs(sum(float(line.split(b"\t")[7]) for line in tsv.split(b"\n")[1:-1]) - 1.0) < 1e-5
    _, _, st1 = c.check(None, bedgraph=False)
    assert st1["runs"] == 0


def test_long_reads_with_a_list(long_chain):
    c = long_chain
    lst = b"".join(XI.row(q, t, 14) if i % 4 else XI.row(t, q) for i, (q, t) in enumerate(c.pairs) if i % 2 == 0)
    lst += XI.row(b"r1", b"remain_1", 14)
    _, _, st = c.check(lst)
    assert st["rows_not_listed"] >= 10 and st["rows_selected"] >= 10 and st["pairs_unknown"] == 1
    _, _, st0 = c.check(b"")
    assert st0["rows_selected"] == 0 and st0["bases"] == 0 and st0["rows_not_listed"] > 0


def test_short_reads(tmp_path):
    c = Chain(RI.every_kind_short(), tmp_path)
    _, _, st = c.check(None)
    assert st["rows_selected"] >= 150
    c.check(b"".join(XI.row(q, t) for q, t in c.pairs[::3]))


def test_tie_between_two_contigs(tmp_path):
    c = Chain(RI.tie_between_contigs(), tmp_path)
    both = sorted({q for q, t in c.pairs if t == b"cA"} & {q for q, t in c.pairs if t == b"cB"})
    assert len(both) >= 6
    tsv, _, st = c.check(None)
    _, _, st2 = c.check(b"".join(XI.row(q, b"cB") for q in both))
    assert st2["rows_selected"] == len(both) and st2["contigs_covered"] == 1


def test_refusals(long_chain, tmp_path):
    c = long_chain
    tsv, bed = str(tmp_path / "d.tsv"), str(tmp_path / "d.bedgraph")
    o = ava_opts()
    o.stub_oh = 0
    with pytest.raises(api.HlmiError) as e:
        api.depth_reads(c.cfa, c.rfa, tsv, bed, o)
    assert e.value.code == -1 and "stub_oh" in str(e.value) and "hlmi_depth_reads" in str(e.value)
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(RI.fasta(c.inp.reads) + b">r3\nACGTACGT\n")
    with pytest.raises(api.HlmiError) as e:
        api.depth_reads(c.cfa, twice, tsv, bed, ava_opts())
    assert e.value.code == -1 and "two records are named r3" in str(e.value)
    lst = str(tmp_path / "pairs.paf")
    with open(lst, "wb") as f:
        f.write(XI.row(b"r1", b"c0") + XI.row(b"r2", b"c0", 4))
    with pytest.raises(api.HlmiError) as e:
        api.depth_reads(c.cfa, c.rfa, tsv, bed, ava_opts(), pairs=lst)
    assert e.value.code == -1 and "pairs.paf:2:" in str(e.value)
    assert not os.path.exists(tsv) and not os.path.exists(bed)


def test_driver_depth_tables(long_chain, tmp_path):
    c = long_chain
    rng = np.random.default_rng(9201)
    short = [r for k, (_, s) in enumerate(c.inp.contigs) for r in RI.sample_reads(rng, s, 40, 150, 150, prefix=f"s{k}_")]
    sfa = str(tmp_path / "short.fa")
    with open(sfa, "wb") as f:
        f.write(RI.fasta(short))
    out = tmp_path / "out"
    out.mkdir()
    st = driver.depth_tables(c.cfa, c.rfa, sfa, str(out), 0)
    assert sorted(os.listdir(out)) == ["final_contigs.long.depth.bedgraph", "final_contigs.long.depth.tsv",
                                       "final_contigs.short.depth.bedgraph", "final_contigs.short.depth.tsv"]
    want = DM.depth(RI.fasta(c.inp.contigs), RI.fasta(c.inp.reads), c.paf_bytes)
    assert (out / "final_contigs.long.depth.tsv").read_bytes() == want[0]
    assert (out / "final_contigs.long.depth.bedgraph").read_bytes() == want[1]
    assert ints(st["long"]) == want[2] and st["short"]["rows_selected"] >= 60
    spaf = str(tmp_path / "short.paf")
    api.ava(c.cfa, sfa, spaf, ava_opts(True))
    with open(spaf, "rb") as f:
        want_s = DM.depth(RI.fasta(c.inp.contigs), RI.fasta(short), f.read())
    assert (out / "final_contigs.short.depth.tsv").read_bytes() == want_s[0]
    # without short reads: the long pair alone
    out2 = tmp_path / "out2"
    out2.mkdir()
    driver.depth_tables(c.cfa, c.rfa, None, str(out2), 0)
    assert sorted(os.listdir(out2)) == ["final_contigs.long.depth.bedgraph", "final_contigs.long.depth.tsv"]
