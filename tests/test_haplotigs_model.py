"""CPU: the haplotig model (tests/haplotigs_model.py, the contract of hlmi_haplotigs / hlmi_haplotigs_reads) held to answers worked
by hand from the header's rules - two strains with substitutions, two insertions and a deletion, where the polisher's model keeps
the contig; no split block: the polisher's bytes; min_side at its border; a tied row on both sides; the extent's edges for
positions and for slots; a side below min_cov - and the shapes' claims about where they sit."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import haplotigs_inputs as GI  # noqa: E402
import haplotigs_model as GM  # noqa: E402
import phase_model as HM  # noqa: E402
import polish_model as PM  # noqa: E402

HAND = GI.hand_cases()
SHAPES = GI.shapes()
POLISH_OPTS = ("min_len", "min_iden", "min_cov", "include_unpolished")


def args(c):
    return c.contigs_bytes(), c.reads_bytes(), c.paf_bytes()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    h = HAND[name]
    fa, blocks, st = GM.haplotigs(*args(h.case), **h.opts)
    assert fa == h.fasta
    assert blocks == GM.BLOCKS_HEAD + b"".join(line + b"\n" for line in h.blocks)
    assert {k: st[k] for k in GM.OWN_KEYS} == {**dict.fromkeys(GM.OWN_KEYS, 0), **h.stats}
    phase = HM.phase(*args(h.case), **{k: v for k, v in h.opts.items() if k not in ("min_side", "include_unpolished")})[3]
    assert {k: st[k] for k in HM.STAT_KEYS} == phase


def test_the_polisher_recovers_neither_indel_of_the_second_strain():
    h = HAND["two_strains"]
    fa, st = PM.polish(*args(h.case))
    ref = h.case.contigs[0][1]
    assert fa == GI.head(b"c", 40, 8, b"1.000000") + ref + b"\n" and st["slots_opened"] == st["deleted"] == st["substituted"] == 0
    (_, _, a), (_, _, b) = GI.records(GM.haplotigs(*args(h.case))[0])
    assert a == ref and len(b) == 42 and b != ref


@pytest.mark.parametrize("name", ["no_multi_site_block", "min_side_above"])
def test_without_a_split_block_the_output_is_the_polishers(name):
    h = HAND[name]
    fa, _, st = GM.haplotigs(*args(h.case), **h.opts)
    want, pst = PM.polish(*args(h.case))
    assert fa == want and st["blocks_split"] == 0
    assert {k: st[k] for k in ("substituted", "deleted", "inserted_bases", "slots_opened", "ins_long", "ins_edge")} == \
           {k: pst[k] for k in ("substituted", "deleted", "inserted_bases", "slots_opened", "ins_long", "ins_edge")}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_min_side_above_the_rows_gives_the_polishers_bytes(name):
    s = SHAPES[name]
    opts = {**s.opts, "min_side": len(s.case.rows) + 1}
    fa, _, st = GM.haplotigs(*args(s.case), **opts)
    assert fa == PM.polish(*args(s.case), **{k: v for k, v in opts.items() if k in POLISH_OPTS})[0] and st["contigs_split"] == 0


def test_inside_rules():
    assert [GM.position_inside([(6, 14)], p) for p in (5, 6, 14, 15)] == [False, True, True, False]
    assert [GM.slot_inside([(6, 14)], p) for p in (6, 7, 14, 15)] == [False, True, True, False]
    ext = [(6, 14, 7), (20, 30, 21)]
    assert GM.shut_out(ext, {7: b"A", 21: b"B"}, b"A") == [(20, 30)] and GM.shut_out(ext, {7: b"A", 21: b"B"}, b"B") == [(6, 14)]
    assert GM.shut_out(ext, {7: b"-"}, b"A") == [] == GM.shut_out(ext, {}, b"B")


def test_option_refusals():
    a = args(HAND["min_side_at"].case)
    for bad in (dict(min_cov=0), dict(min_link=0), dict(min_agree=0.5), dict(min_side=0), dict(min_side=0, min_agree=0.4)):
        with pytest.raises(PM.Refused) as e:
            GM.haplotigs(*a, **bad)
        assert e.value.line == 0
    with pytest.raises(PM.Refused) as e:                      # the phase call's refusal comes first
        GM.haplotigs(*a, min_side=0, min_agree=0.4)
    assert "min_agree" in str(e.value)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_sit_where_they_claim(name):
    s = SHAPES[name]
    s.where(*GM.haplotigs(*args(s.case), **s.opts))
