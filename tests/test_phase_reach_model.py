"""CPU: the model of hlmi_phase_reach (tests/phase_reach_model.py) held to what it rests on.  With reach = 1 it gives
tests/phase_model.py's three files and shared stats on every hand case and shape of tests/phase_inputs.py; the hand cases of
tests/phase_reach_inputs.py match their hand-written lines; the shapes sit where they claim to; the block rule alone on literal
link calls (a pending run of exactly reach and of reach + 1 sites); tests/haplotigs_reach_model.py with reach = 1 gives
tests/haplotigs_model.py's files on the haplotig inputs."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import haplotigs_inputs as GI  # noqa: E402
import haplotigs_model as GM  # noqa: E402
import haplotigs_reach_model as GR  # noqa: E402
import phase_inputs as HI  # noqa: E402
import phase_model as HM  # noqa: E402
import phase_reach_inputs as RI  # noqa: E402
import phase_reach_model as RM  # noqa: E402

OLD_HAND, OLD_SHAPES = HI.hand_cases(), HI.shapes()
HAND, SHAPES = RI.hand_cases(), RI.shapes()
OLD = {**{n: (h.case, h.opts) for n, h in OLD_HAND.items()}, **{n: (s.case, s.opts) for n, s in OLD_SHAPES.items()}}


@pytest.mark.parametrize("name", sorted(OLD))
def test_reach_1_is_the_phase_model(name):
    c, opts = OLD[name]
    args = (c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    want, got = HM.phase(*args, **opts), RM.phase(*args, reach=1, **opts)
    assert got[:3] == want[:3]
    assert {k: got[3][k] for k in HM.STAT_KEYS} == want[3] and {k: got[3][k] for k in RM.FAR_KEYS} == dict.fromkeys(RM.FAR_KEYS, 0)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    h = HAND[name]
    sites, links, reads, st = RM.phase(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), reach=h.reach, **h.opts)
    assert sites == HM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert links == HM.LINKS_HEAD + b"".join(line + b"\n" for line in h.links)
    assert reads == HM.READS_HEAD + b"".join(line + b"\n" for line in h.reads)
    assert {k: v for k, v in st.items() if v} == h.stats


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_sit_where_they_claim(name):
    s = SHAPES[name]
    for reach in s.reaches:
        s.where(reach, *RM.phase(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(), reach=reach, **s.opts))


def test_the_block_rule_on_literal_calls():
    def blocks(n, reach, phased):
        return RM.build_blocks(n, reach, lambda j, i: phased.get((j, i), b"-"))
    X = RM.BRIDGED
    # reach 2: the pending run behind site 0 is sites 1 and 2 - exactly reach sites, site 2 joins; with site 3 instead (reach + 1
    # sites) no link of that distance exists and the block ends
    assert blocks(4, 2, {(0, 2): b"cis"}) == ([0, 0, 0, 3], [0, X, 0, 0], 1, 0)
    assert blocks(4, 2, {(0, 3): b"cis"}) == ([0, 1, 2, 3], [0, 0, 0, 0], 0, 0)
    assert blocks(4, 3, {(0, 3): b"trans"}) == ([0, 0, 0, 0], [0, X, X, 1], 1, 0)
    # the pending sites that stay outside start blocks of their own, and may join each other
    assert blocks(5, 2, {(1, 2): b"trans", (2, 4): b"trans"}) == ([0, 1, 1, 1, 1], [0, 0, 1, X, 0], 1, 0)
    # the nearest member decides; the farther link that says otherwise is a conflict
    assert blocks(3, 2, {(0, 1): b"cis", (1, 2): b"cis", (0, 2): b"trans"}) == ([0, 0, 0], [0, 0, 0], 0, 1)
    assert blocks(3, 2, {(0, 1): b"cis", (0, 2): b"trans"}) == ([0, 0, 0], [0, 0, 1], 1, 0)
    # a bridged site is no member: its phased link to a later site joins nothing
    assert blocks(4, 2, {(0, 2): b"cis", (1, 3): b"cis"}) == ([0, 0, 0, 3], [0, X, 0, 0], 1, 0)
    assert blocks(0, 3, {}) == ([], [], 0, 0) and blocks(1, 8, {}) == ([0], [0], 0, 0)


def test_noisy_two_strains_cut_and_joined():
    one, two = RI.noisy_two_strains(1), RI.noisy_two_strains(2)
    args = (one.case.contigs_bytes(), one.case.reads_bytes(), one.case.paf_bytes())
    _, _, _, st1 = RM.phase(*args, reach=1)
    assert st1["sites"] == len(one.snps) + 1 and (st1["blocks"], st1["blocks_multi"]) == (3, 2)
    sites, _, reads, st2 = RM.phase(*args, reach=2)
    assert (st2["blocks"], st2["sites_bridged"], st2["joins_far"], st2["read_records"]) == (1, 1, 1, 90)
    assert [p for _, p, _, _, ph in HI.site_rows(sites) if ph == b"."] == one.noise
    args = (two.case.contigs_bytes(), two.case.reads_bytes(), two.case.paf_bytes())
    assert RM.phase(*args, reach=2)[3]["blocks"] >= 3
    st3 = RM.phase(*args, reach=3)[3]
    assert (st3["blocks"], st3["sites_bridged"], st3["joins_far"]) == (1, 2, 1)


@pytest.mark.parametrize("name", sorted(GI.hand_cases()))
def test_haplotigs_reach_1_is_the_haplotigs_model(name):
    h = GI.hand_cases()[name]
    args = (h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes())
    assert GR.haplotigs(*args, reach=1, **h.opts) == GM.haplotigs(*args, **h.opts)
