"""GPU: hlmi_haplotigs_ins against its model (tests/haplotigs_ins_model.py) - both files byte for byte and every integer stat - on
the cases of tests/haplotigs_ins_inputs.py (each first asserts on the model that it sits where it claims to), on two strains that
differ by insertions alone (hlmi_haplotigs_reach's model writes one record there), and on every older haplotig input at reach 1
and 2: where the model says that no insertion site takes part, out_fa is hlmi_haplotigs_reach's, the blocks file is its file with
a tenth column and the shared stats agree.  The refusals in their order - options, reach, then rows, list, names and files under
the new names - with nothing written; no kernel of haplotigs.hip runs where no block is split."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import haplotigs_inputs as GI  # noqa: E402
import haplotigs_ins_inputs as KI  # noqa: E402
import haplotigs_ins_model as KM  # noqa: E402
import haplotigs_reach_model as GR  # noqa: E402
import phase_ins_model as IM  # noqa: E402
import phase_reach_inputs as RI  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = KI.cases()
OLD = {**{n: (h.case, h.opts) for n, h in GI.hand_cases().items()}, **{n: (s.case, s.opts) for n, s in GI.shapes().items()},
       "noisy_two_strains": (RI.noisy_two_strains(1).case, {})}
NAMES = ("haplotigs.fa", "haplotigs.blocks.tsv")
HAP_TIMERS = ("kernel_ms.hap_intervals", "kernel_ms.hap_count", "kernel_ms.hap_slots")


def ints(st):
    return {k: st[k] for k in KM.STAT_KEYS}


def run_and_compare(c, d, reach, where=None, **opts):
    """-> the model's (fasta, blocks, stats), after the library's files and stats were found equal to them"""
    cfa, rfa, paf = c.write(str(d))
    want = KM.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, reach, **opts)
    if where:
        where(reach, *want)
    out = [os.path.join(str(d), n) for n in NAMES]
    st = api.haplotigs_ins(cfa, rfa, paf, *out, reach=reach, **opts)
    assert ints(st) == want[2]
    for path, data in zip(out, want[:2]):
        with open(path, "rb") as f:
            assert f.read() == data, path
    split = want[2]["blocks_split"] > 0
    last = api.last_stats()
    assert all((last.get(t, 0) > 0) == split for t in HAP_TIMERS[:2]) and (split or last.get(HAP_TIMERS[2], 0) == 0)
    return want


@pytest.mark.parametrize("name,reach", [(n, r) for n in sorted(CASES) for r in CASES[n].reaches])
def test_cases_against_the_model(name, reach, tmp_path):
    k = CASES[name]
    run_and_compare(k.case, tmp_path, reach, k.where, **k.opts)


def test_insertion_strains_only(tmp_path):
    """The test that fails without the feature: a minority strain that differs by three insertions of 1, 3 and 16 bases alone"""
    s = KI.insertion_strains_only()
    c = s.case
    fa1, blocks1, st1 = GR.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, 1)
    assert len(GI.records(fa1)) == 1 and st1["blocks_split"] == 0 and blocks1 == GR.GM.BLOCKS_HEAD     # hlmi_haplotigs_reach: one record
    fa, blocks, st = run_and_compare(c, tmp_path, 1)
    (na, _, a), (nb, _, b) = GI.records(fa)
    contig = c.contigs[0][1]
    strain, shift = bytearray(contig), 0
    for p, ins in zip(s.slots, (b"G", b"TGA", KI.II.S16)):
        strain[p + shift:p + shift] = ins
        shift += len(ins)
    assert (na, nb) == (b"major_contig_hapA", b"major_contig_hapB") and a == contig and b == bytes(strain)
    (row,) = KI.block_rows(blocks)
    assert row[1:4] == (b"%d+" % s.slots[0],) * 2 + (b"%d+" % s.slots[-1],) and row[7:] == (1, 0, 3)
    assert st["diff_positions"] == 0 and st["diff_slots"] == 3 and st["slots_opened"] == 3 and st["inserted_bases"] == 20


@pytest.mark.parametrize("reach", (1, 2))
@pytest.mark.parametrize("name", sorted(OLD))
def test_older_inputs(name, reach, tmp_path):
    c, opts = OLD[name]
    want = run_and_compare(c, tmp_path / "ins", reach, **opts)
    popts = {k: v for k, v in opts.items() if k not in ("min_side", "include_unpolished")}
    if KM.takes_part(IM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, reach, **popts)[0]):
        return                                                     # an insertion site takes part: the model alone
    cfa, rfa, paf = c.write(str(tmp_path / "reach"))
    out = [str(tmp_path / "reach" / n) for n in NAMES]
    st = api.haplotigs_reach(cfa, rfa, paf, *out, reach=reach, **opts)
    assert {k: st[k] for k in GR.STAT_KEYS} == {k: want[2][k] for k in GR.STAT_KEYS}
    with open(out[0], "rb") as f:
        assert f.read() == want[0]
    with open(out[1], "rb") as f:
        assert f.read() == b"".join(line.rsplit(b"\t", 1)[0] + b"\n" for line in want[1].split(b"\n")[:-1])


def test_refusals(tmp_path):
    c, opts = OLD["min_side_at"]
    cfa, rfa, paf = c.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("h.fa", "b.tsv")]
    for call, who in ((lambda **k: api.haplotigs_ins(cfa, rfa, paf, *outs, **k), "hlmi_haplotigs_ins"),
                      (lambda **k: api.haplotigs_reads_ins(cfa, rfa, *outs, **k), "hlmi_haplotigs_reads_ins")):
        for reach in (0, RI.REACH_MAX + 1):
            with pytest.raises(api.HlmiError) as e:
                call(reach=reach)
            assert e.value.code == -1 and f"{who}: reach {reach} " in str(e.value)
        with pytest.raises(api.HlmiError) as e:                   # behind min_side's refusal
            call(reach=0, min_side=0)
        assert f"{who}: min_side " in str(e.value)
        with pytest.raises(api.HlmiError) as e:                   # ... which is behind the phase options'
            call(reach=0, min_side=0, min_link=0)
        assert f"{who}: min_link " in str(e.value)
    with pytest.raises(KM.PM.Refused):
        KM.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), reach=9)
    assert not any(os.path.exists(p) for p in outs)


def test_file_row_and_list_refusals(tmp_path):
    """behind the options, hlmi_haplotigs_reach's refusals under the new names: a row, the list, a name twice, a missing file"""
    c, _ = OLD["min_side_at"]
    cfa, rfa, paf = c.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("h.fa", "b.tsv")]
    broken, lst, twice = (str(tmp_path / n) for n in ("bad.paf", "pairs.paf", "twice.fa"))
    with open(broken, "wb") as f:
        f.write(c.paf_bytes().replace(b"cg:Z:2=1X3=1X13=", b"cg:Z:2=1X3=1X12=", 1))
    with open(lst, "wb") as f:
        f.write(XI.row(b"r0", b"c") + XI.row(b"r1", b"c", 5))
    with open(twice, "wb") as f:
        f.write(c.contigs_bytes() + b">c\nACGT\n")
    stub = api.ava_opts_long()
    stub.stub_oh = 0
    for call, code, words in (
            (lambda: api.haplotigs_ins(cfa, rfa, broken, *outs, reach=2), -1, ("bad.paf:1:",)),
            (lambda: api.haplotigs_ins(cfa, rfa, broken, *outs, reach=0), -1, ("hlmi_haplotigs_ins: reach 0 ",)),          # the option first
            (lambda: api.haplotigs_ins(cfa, rfa, broken, *outs, pairs=lst), -1, ("bad.paf:1:",)),                          # a row's before the list's
            (lambda: api.haplotigs_ins(cfa, rfa, paf, *outs, pairs=lst), -1, ("hlmi_haplotigs_ins: ", "pairs.paf:2:")),
            (lambda: api.haplotigs_ins(twice, rfa, paf, *outs), -1, ("hlmi_haplotigs_ins: ", "two records are named c")),
            (lambda: api.haplotigs_ins(cfa, rfa, str(tmp_path / "none.paf"), *outs), -2, ("none.paf",)),
            (lambda: api.haplotigs_reads_ins(cfa, rfa, *outs, stub), -1, ("hlmi_haplotigs_reads_ins: stub_oh 0",)),
            (lambda: api.haplotigs_reads_ins(twice, rfa, *outs), -1, ("hlmi_haplotigs_reads_ins: ", "two records are named c")),
            (lambda: api.haplotigs_reads_ins(cfa, rfa, *outs, pairs=lst), -1, ("hlmi_haplotigs_reads_ins: ", "pairs.paf:2:"))):
        with pytest.raises(api.HlmiError) as e:
            call()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
        assert not any(os.path.exists(p) for p in outs)
