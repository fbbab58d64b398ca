"""GPU: hlmi_haplotigs_reads against the chain hlmi_ava -> PAF -> hlmi_haplotigs: both files byte for byte and every integer stat,
and the chain's against the model (tests/haplotigs_model.py) on the PAF hlmi_ava wrote.  One contig of 20 kb that is strain 1; strain
2 has another base about every 400 bases, one base more, two bases fewer and three bases more in its middle; 20 reads of 3 kb of
each strain, tiled alike, with a few substitution errors - and without any: there each haplotig equals its strain over the split
extents.  Long and short constants, one run with a pair list; driver.haplotig_files writes its two files."""
import os
import sys

import numpy as np
import pytest

from hylight_amd import api, driver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import haplotigs_inputs as GI  # noqa: E402
import haplotigs_model as GM  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402

pytestmark = pytest.mark.gpu
N, READ, PER_STRAIN = 20000, 3000, 20
OPTS = dict(min_len=300, min_iden=0.9, min_cov=2, min_side=2)


def ava_opts(short=False):
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    return o


def strain_two(s1, lo, hi, subs, ins, dels):
    """s1[lo:hi + 1] as strain 2 has it: subs {p: base}, ins {p: bases in front of p} (lo < p), dels positions"""
    out = bytearray()
    for p in range(lo, hi + 1):
        if p in ins and p > lo:
            out += ins[p]
        if p not in dels:
            out += subs.get(p, s1[p:p + 1])
    return bytes(out)


def two_strain_set(error_rate):
    rng = np.random.default_rng(8801)
    s1 = bytes(b"ACGT"[k] for k in rng.integers(0, 4, size=N))
    at = [int(p) for p in np.arange(200, N - 200, 400) + rng.integers(-20, 20, size=len(np.arange(200, N - 200, 400)))]
    subs = {p: GI.other_base(s1[p], 1 + p % 3) for p in at}
    ins = {9050: GI.other_base(s1[9050], 1), 11050: b"GCA"}
    if ins[11050][:1] == s1[11050:11051]:
        ins[11050] = b"TCA" if s1[11050:11051] != b"T" else b"CCA"
    dels = {10050, 10051}
    edits = (subs, ins, dels)
    reads = []
    for k in range(2):
        for i in range(PER_STRAIN):
            a = i * (N - READ) // (PER_STRAIN - 1)
            seq = bytearray(s1[a:a + READ] if k == 0 else strain_two(s1, a, a + READ - 1, *edits))
            for p in np.flatnonzero(rng.random(len(seq)) < error_rate):
                seq[p] = GI.other_base(seq[p], 2)[0]
            seq = bytes(seq)
            reads.append((f"s{k + 1}_{i}", seq if i % 2 == 0 else GI.PI.revcomp(seq)))
    return [("contig", s1)], reads, s1, edits


class Chain:
    def __init__(self, d, error_rate):
        self.d = str(d)
        self.contigs, self.reads, self.s1, self.edits = two_strain_set(error_rate)
        self.cfa, self.rfa = (os.path.join(self.d, n) for n in ("contigs.fa", "reads.fa"))
        with open(self.cfa, "wb") as f:
            f.write(RI.fasta(self.contigs))
        with open(self.rfa, "wb") as f:
            f.write(RI.fasta(self.reads))
        self.n = 0

    def check(self, short=False, lst=None, **more):
        """model == chain == fused call -> the model's (fasta, blocks, stats)"""
        self.n += 1
        opts = {**OPTS, **more}
        paf = os.path.join(self.d, f"chain{self.n}.paf")
        api.ava(self.cfa, self.rfa, paf, ava_opts(short))
        with open(paf, "rb") as f:
            paf_bytes = f.read()
        path = None
        if lst is not None:
            path = os.path.join(self.d, f"list{self.n}.paf")
            with open(path, "wb") as f:
                f.write(lst)
        want = GM.haplotigs(RI.fasta(self.contigs), RI.fasta(self.reads), paf_bytes, lst, **opts)
        for who in ("chain", "direct"):
            out = [os.path.join(self.d, f"{who}{self.n}.{e}") for e in ("fa", "blocks.tsv")]
            st = (api.haplotigs(self.cfa, self.rfa, paf, *out, pairs=path, **opts) if who == "chain" else
                  api.haplotigs_reads(self.cfa, self.rfa, *out, ava_opts(short), pairs=path, **opts))
            assert {k: st[k] for k in GM.STAT_KEYS} == want[2], who
            for p, data in zip(out, want[:2]):
                with open(p, "rb") as f:
                    assert f.read() == data, (who, p)
        return want


@pytest.fixture(scope="module")
def noisy(tmp_path_factory):
    return Chain(tmp_path_factory.mktemp("haplotigs_noisy"), 0.002)


def test_long_constants(noisy):
    fa, blocks, st = noisy.check()
    assert st["rows_selected"] == 2 * PER_STRAIN and st["blocks_split"] >= 1 and st["records"] == 2 and st["diff_positions"] >= 20


def test_short_constants(noisy):
    fa, blocks, st = noisy.check(short=True)
    assert st["rows_selected"] >= PER_STRAIN and st["records"] >= 1


def test_with_a_pair_list(noisy):
    # strain 2's reads alone: no second side, the polisher's single record
    lst = b"".join(XI.row(n.encode(), b"contig", 14) for n, _ in noisy.reads if n.startswith("s2_"))
    fa, blocks, st = noisy.check(lst=lst)
    assert st["rows_selected"] == PER_STRAIN and st["rows_not_listed"] >= PER_STRAIN and st["blocks_split"] == 0 and st["records"] == 1


def test_error_free_reads_give_each_strain_over_the_split_extents(tmp_path):
    c = Chain(tmp_path, 0.0)
    fa, blocks, st = c.check()
    extents = [(r[1], r[2]) for r in GI.block_rows(blocks) if r[6]]
    assert 1 <= len(extents) == st["blocks_split"]
    subs, ins, dels = c.edits
    for p in list(ins) + list(dels):                           # the three indels lie inside a split extent, their slots too
        assert any(first < p <= last for first, last in extents), p
    assert sum(1 for p in subs if any(first <= p <= last for first, last in extents)) >= 40
    (na, _, a), (nb, _, b) = GI.records(fa)
    assert (na, nb) == (b"contig_hapA", b"contig_hapB")
    want, prev = bytearray(), 0                                # strain 2 inside every extent, the contig between them
    for first, last in extents:
        want += c.s1[prev:first] + strain_two(c.s1, first, last, *c.edits)
        prev = last + 1
    assert a == c.s1 and b == bytes(want + c.s1[prev:])


def test_refusals_and_driver(noisy, tmp_path):
    o = ava_opts()
    o.stub_oh = 0
    outs = [str(tmp_path / n) for n in ("h.fa", "b.tsv")]
    with pytest.raises(api.HlmiError) as e:
        api.haplotigs_reads(noisy.cfa, noisy.rfa, *outs, o)
    assert e.value.code == -1 and "stub_oh" in str(e.value) and "hlmi_haplotigs_reads" in str(e.value)
    with pytest.raises(api.HlmiError) as e:
        api.haplotigs_reads(noisy.cfa, noisy.rfa, *outs, ava_opts(), min_side=0)
    assert e.value.code == -1 and "hlmi_haplotigs_reads: min_side" in str(e.value)
    assert not any(os.path.exists(p) for p in outs)
    out = tmp_path / "out"
    out.mkdir()
    st = driver.haplotig_files(noisy.cfa, noisy.rfa, None, str(out), 0)
    assert sorted(os.listdir(out)) == ["final_contigs.long.haplotigs.blocks.tsv", "final_contigs.long.haplotigs.fa"]
    assert st["long"]["rows_selected"] == 2 * PER_STRAIN
