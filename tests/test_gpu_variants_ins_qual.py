"""GPU: hlmi_variants_ins_q and hlmi_variants_reads_ins_q against their model (tests/variants_qual_model.py: variants_ins_q) - the
three files byte for byte and every integer field.  A failing column still spans its slot (span unchanged, depth drops); out_sites
is the _q call's; with the base floor alone out_ins is hlmi_variants_ins's; the read floor takes rows out of the slots; the
identities on the inputs of tests/variants_ins_inputs.py; one fused call against its chain."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_qual_inputs as QI  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402
import variants_ins_inputs as II  # noqa: E402
import variants_ins_model as IM  # noqa: E402
import variants_qual_model as VQ  # noqa: E402

pytestmark = pytest.mark.gpu
OFF = dict(min_base_qual=0, min_avg_qual=0.0)
OLDER = {**{f"hand_{k}": (v.case, v.opts) for k, v in II.hand_cases().items()},
         **{f"shape_{k}": (v.case, v.opts) for k, v in II.shapes().items()}}


def run_and_compare(c, d, **opts):
    d = str(d)
    cfa, rfa, paf = c.write(d)
    want = VQ.variants_ins_q(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), **opts)
    sites, ins, summ = (os.path.join(d, n) for n in ("sites.tsv", "ins.tsv", "summary.tsv"))
    st = api.variants_ins_q(cfa, rfa, paf, sites, ins, summ, **opts)
    assert {k: st[k] for k in VQ.INS_STAT_KEYS} == want[3]
    for path, data in ((sites, want[0]), (ins, want[1]), (summ, want[2])):
        with open(path, "rb") as f:
            assert f.read() == data, path
    return want


def spanning_case():
    """slot 5 of a 12-base contig: two rows insert T, every column of theirs at Q3; three plain rows at Q40.  Slot 9: two other
    rows insert GG with a C at Q3 on position 9 - the slot is a site, and position 9 would be one without the floor"""
    ref = b"ACGTACGTACGT"
    c = QI.QCase([("c", ref)])
    for s in "+-":
        c.addq(0, "5=1I7=", ref[:5] + b"T" + ref[5:], QI._col(13, 3), strand=s, left=b"GA")
    for s in "+-":
        c.addq(0, "9=2I1X2=", ref[:9] + b"GG" + b"A" + ref[10:], QI._col(14, 40, c11=3), strand=s)
    for _ in range(3):
        c.addq(0, "12=", ref, QI._col(12, 40))
    return c


def test_a_failing_column_still_spans(tmp_path):
    c = spanning_case()
    on = dict(min_base_qual=10, min_avg_qual=0.0)
    sites, ins, summary, st = run_and_compare(c, tmp_path / "on", **on)
    args = (c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    plain = IM.variants_ins(*args)
    # the slots are hlmi_variants_ins's: span 7 on both, though position 5 has five votes and position 9 five
    assert ins == plain[1] == IM.INS_HEAD + b"c\t5\tA\t7\t2\t0\t0.285714\t1\t2\tT\nc\t9\tA\t7\t2\t0\t0.285714\t2\t2\tGG\n"
    assert st["slots_callable"] == plain[3]["slots_callable"] == 11 and st["columns_low_qual"] == 2 * 12 + 2
    assert plain[0] != sites == IM.VM.SITES_HEAD and plain[3]["sites"] == 1 and st["sites"] == 0
    # out_sites is the _q call's, byte for byte
    d = tmp_path / "q"
    d.mkdir()
    cfa, rfa, paf = c.write(str(tmp_path / "on"))
    stq = api.variants_q(cfa, rfa, paf, str(d / "sites.tsv"), None, **on)
    assert (d / "sites.tsv").read_bytes() == sites and stq["columns_low_qual"] == st["columns_low_qual"]
    # the read floor: the two rows of Q3 leave the slots too
    _, ins2, _, st2 = run_and_compare(c, tmp_path / "read_floor", min_base_qual=0, min_avg_qual=10.0)
    assert st2["rows_low_qual"] == 2 and ins2 == IM.INS_HEAD + b"c\t9\tA\t5\t2\t0\t0.400000\t2\t2\tGG\n"


@pytest.mark.parametrize("name", sorted(OLDER))
def test_identities_on_the_older_inputs(name, tmp_path):
    c, opts = OLDER[name]
    want = IM.variants_ins(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), **opts)

    def same(got):
        assert got[:3] == want[:3] and {k: got[3][k] for k in IM.STAT_KEYS} == want[3] and got[3]["columns_low_qual"] == 0
    same(run_and_compare(c, tmp_path / "off", **opts, **OFF))
    same(run_and_compare(c, tmp_path / "fasta", **opts, min_base_qual=40, min_avg_qual=30.0))
    q = QI.with_quals(c, 6, choices=(10, 30, 93))
    same(run_and_compare(q, tmp_path / "passing", **opts, min_base_qual=10, min_avg_qual=10.0))


def test_refusals(tmp_path):
    c = spanning_case()
    cfa, rfa, paf = c.write(str(tmp_path))
    sites, ins = str(tmp_path / "s.tsv"), str(tmp_path / "i.tsv")
    for args, kw, word in (((cfa, rfa, paf, sites, None), dict(min_base_qual=94), "min_base_qual"),      # the floor, then out_ins
                           ((cfa, rfa, paf, sites, None), {}, "out_ins"),
                           ((cfa, rfa, paf, sites, None), dict(min_cov=0), "out_ins"),
                           ((cfa, rfa, paf, sites, ins), dict(min_cov=0), "min_cov")):
        with pytest.raises(api.HlmiError) as e:
            api.variants_ins_q(*args, **kw)
        assert e.value.code == -1 and word in str(e.value) and "hlmi_variants_ins_q" in str(e.value)
    assert not os.path.exists(sites) and not os.path.exists(ins)


def test_fused_call_equals_the_chain(tmp_path):
    inp, quals = QI.overlap_input(0, n_low=3, fasta_every=7)
    cfa, rfa, paf = (str(tmp_path / n) for n in ("contigs.fa", "reads.fq", "chain.paf"))
    contigs, reads = RI.fasta(inp.contigs), QI.fastq(inp.reads, quals)
    with open(cfa, "wb") as f:
        f.write(contigs)
    with open(rfa, "wb") as f:
        f.write(reads)
    o = api.ava_opts_long()
    o.pair_once = 0
    api.ava(cfa, rfa, paf, o)
    with open(paf, "rb") as f:
        want = VQ.variants_ins_q(contigs, reads, f.read(), **inp.opts)
    assert want[3]["columns_low_qual"] > 0 and want[3]["rows_low_qual"] >= 3 and want[3]["slots_callable"] > 0
    for who in ("chain", "direct"):
        sites, ins, summ = (str(tmp_path / f"{who}.{e}") for e in ("sites.tsv", "ins.tsv", "summary.tsv"))
        st = (api.variants_ins_q(cfa, rfa, paf, sites, ins, summ, **inp.opts) if who == "chain" else
              api.variants_ins_reads_q(cfa, rfa, sites, ins, summ, o, **inp.opts))
        assert {k: st[k] for k in VQ.INS_STAT_KEYS} == want[3], who
        for path, data in ((sites, want[0]), (ins, want[1]), (summ, want[2])):
            with open(path, "rb") as f:
                assert f.read() == data, (who, path)
