"""GPU: hlmi_variants_reads_q against the chain hlmi_ava -> PAF -> hlmi_variants_q: both files byte for byte and every integer
field, and the chain's against the model (tests/variants_qual_model.py) on the PAF hlmi_ava wrote.  The reads of
polish_qual_inputs.overlap_input - wrong bases at Q2 - Q5, the same wrong base at Q2 in most reads on one position in a hundred, a
low 3' tail, some reads Q4 throughout, some FASTA records - with the overlapper's long constants and with its short ones: the
fused call votes from the overlapper's resident codes (the READS_CODES instantiations of var_tile_kernel<QF>), its quality bytes
lie at the codes' offsets."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_qual_inputs as QI  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import variants_model as VM  # noqa: E402
import variants_qual_model as VQ  # noqa: E402

pytestmark = pytest.mark.gpu


def ava_opts(short):
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    return o


def chain_and_direct(inp, quals, d, **opts):
    """model == chain == fused call -> (the model's (sites, summary, stats), the PAF's bytes)"""
    os.makedirs(d, exist_ok=True)
    cfa, rfa, paf = (os.path.join(d, n) for n in ("contigs.fa", "reads.fq", "chain.paf"))
    contigs, reads = RI.fasta(inp.contigs), QI.fastq(inp.reads, quals)
    with open(cfa, "wb") as f:
        f.write(contigs)
    with open(rfa, "wb") as f:
        f.write(reads)
    api.ava(cfa, rfa, paf, ava_opts(inp.short))
    with open(paf, "rb") as f:
        paf_bytes = f.read()
    opts = {**inp.opts, **opts}
    want = VQ.variants_q(contigs, reads, paf_bytes, **opts)
    for who in ("chain", "direct"):
        sites, summ = (os.path.join(d, f"{who}.{e}") for e in ("sites.tsv", "summary.tsv"))
        st = (api.variants_q(cfa, rfa, paf, sites, summ, **opts) if who == "chain" else
              api.variants_reads_q(cfa, rfa, sites, summ, ava_opts(inp.short), **opts))
        assert {k: st[k] for k in VQ.STAT_KEYS} == want[2], who
        with open(sites, "rb") as f:
            assert f.read() == want[0], who
        with open(summ, "rb") as f:
            assert f.read() == want[1], who
    return want, (contigs, reads, paf_bytes)


@pytest.mark.parametrize("short", [0, 1])
def test_fused_call_equals_the_chain(short, tmp_path):
    inp, quals = QI.overlap_input(short, n_low=0 if short else 3, fasta_every=7)
    (sites, _, st), (contigs, reads, paf) = chain_and_direct(inp, quals, str(tmp_path / "on"), min_base_qual=10, min_avg_qual=10.0)
    assert 0 < st["reads_with_qual"] < len(inp.reads) and st["columns_low_qual"] > 0 and st["rows_selected"] > 20
    assert st["rows_low_qual"] >= (0 if short else 3)
    # the floor matters on this input: the systematic Q2 bases are sites by count and none under the floor
    plain = VM.variants(contigs, reads, paf, **inp.opts)
    assert plain[2]["sites"] > st["sites"] and plain[0] != sites
    # both floors off: hlmi_variants's answer through both entry points
    (sites0, summ0, st0), _ = chain_and_direct(inp, quals, str(tmp_path / "off"), min_base_qual=0, min_avg_qual=0.0)
    assert (sites0, summ0) == plain[:2] and {k: st0[k] for k in VM.STAT_KEYS} == plain[2] and st0["columns_low_qual"] == 0


def test_refusals_of_the_fused_call(tmp_path):
    inp, quals = QI.overlap_input(1)
    cfa, rfa = tmp_path / "contigs.fa", tmp_path / "reads.fq"
    cfa.write_bytes(RI.fasta(inp.contigs))
    rfa.write_bytes(QI.fastq(inp.reads, quals))
    sites = str(tmp_path / "s.tsv")
    o = ava_opts(1)
    o.stub_oh = 0
    for kw, word in ((dict(min_base_qual=94), "min_base_qual"), (dict(min_avg_qual=-1.0), "min_avg_qual"), ({}, "stub_oh")):
        with pytest.raises(api.HlmiError) as e:
            api.variants_reads_q(str(cfa), str(rfa), sites, None, o, **kw)
        assert e.value.code == -1 and word in str(e.value) and "hlmi_variants_reads_q" in str(e.value)
    assert not os.path.exists(sites)
