"""CPU: the phasing model (tests/phase_model.py, the contract of hlmi_phase / hlmi_phase_reads) held to answers worked by hand from
the header's rules - cis, trans, a chain, a tie, min_link and min_agree one below and exactly at their borders, a third base and a
read N, del from one D run, the own base in the minority, strand '-', a row over two blocks, a row that says nothing, hap ties -
the shapes' claims about where they sit, and the case that states what the pass is for: two strains collapsed into one contig,
every link phased, one block, every read on its strain's side; with the same-strain list no site and no record."""
import math
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phase_inputs as HI  # noqa: E402
import phase_model as HM  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import variants_model as VM  # noqa: E402

HAND = HI.hand_cases()
SHAPES = HI.shapes()


def args(c):
    return c.contigs_bytes(), c.reads_bytes(), c.paf_bytes()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    h = HAND[name]
    sites, links, reads, st = HM.phase(*args(h.case), **h.opts)
    assert sites == HM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert links == HM.LINKS_HEAD + b"".join(line + b"\n" for line in h.links)
    assert reads == HM.READS_HEAD + b"".join(line + b"\n" for line in h.reads)
    assert st == {**dict.fromkeys(HM.STAT_KEYS, 0), **h.stats}
    assert st["read_records"] == st["reads_a"] + st["reads_b"] + st["reads_tie"]


def test_the_sites_are_the_variant_models(name="third_base_and_read_n"):
    h = HAND[name]
    vsites, _, vst = VM.variants(*args(h.case))
    sites, _, _, st = HM.phase(*args(h.case))
    v = [f.split(b"\t") for f in vsites.split(b"\n")[1:-1]]
    p = [f.split(b"\t") for f in sites.split(b"\n")[1:-1]]
    assert [(f[0], f[1], f[2], f[9], f[3], f[10]) for f in v] == [(f[0], f[1], f[2], f[3], f[4], f[6]) for f in p]
    assert {k: st[k] for k in VM.STAT_KEYS} == vst


def test_link_rule_literals():
    assert HM.link_call([3, 0, 0, 3], 3, 0.8) == (6, 1.0, b"cis")
    assert HM.link_call([0, 3, 3, 0], 3, 0.8) == (6, 1.0, b"trans")
    assert HM.link_call([1, 1, 1, 1], 3, 0.8) == (4, 0.5, b"-")
    assert HM.link_call([2, 0, 1, 2], 3, 0.8) == (5, 0.8, b"cis")
    assert HM.link_call([2, 0, 1, 2], 3, math.nextafter(0.8, 1.0))[2] == b"-"
    assert HM.link_call([1, 0, 0, 1], 3, 0.8) == (2, 1.0, b"-") and HM.link_call([1, 0, 0, 1], 2, 0.8)[2] == b"cis"
    assert HM.link_call([0, 0, 0, 0], 1, 0.8) == (0, 0.0, b"-")
    assert HM.hap_of(2, 1) == b"A" and HM.hap_of(1, 2) == b"B" and HM.hap_of(1, 1) == HM.hap_of(0, 0) == b"-"
    assert HM.allele({4: 2}, 4, 2, 3) == 0 and HM.allele({4: 3}, 4, 2, 3) == 1 and HM.allele({4: 4}, 4, 2, 3) == 2
    assert HM.allele({4: 2}, 5, 2, 3) is HM.NONE


def test_option_refusals():
    a = args(HAND["cis"].case)
    for bad in (dict(min_cov=0), dict(min_alt=0), dict(min_frac=1.5), dict(min_link=0), dict(min_agree=0.5), dict(min_agree=1.01),
                dict(min_agree=float("nan"))):
        with pytest.raises(HM.PM.Refused) as e:
            HM.phase(*a, **bad)
        assert e.value.line == 0
    HM.phase(*a, min_agree=1.0, min_link=1)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_sit_where_they_claim(name):
    s = SHAPES[name]
    s.where(*HM.phase(*args(s.case), **s.opts))


def test_two_strains_every_link_phased_and_every_read_on_its_side():
    s = XI.two_strains()
    sites, links, reads, st = HM.phase(*args(s.case))
    assert [p for _, p, _, _, _ in HI.site_rows(sites)] == sorted(s.snps) and len(s.snps) >= 20
    assert st["links"] == st["links_phased"] == len(s.snps) - 1 and all(call == b"cis" for *_, call in HI.link_rows(links))
    assert st["blocks"] == st["blocks_multi"] == 1 and st["sites_phased"] == len(s.snps)
    rows = HI.read_rows(reads)
    assert len(rows) == st["read_records"] == 90 and st["reads_a"] == 15 and st["reads_b"] == 75 and st["reads_tie"] == 0
    for read, _, block, spanned, a, b, other, hap in rows:                     # the contig is the minor strain's: its reads are hap A
        assert block == min(s.snps) + 1 and other == 0 and spanned == a + b
        assert (hap, b) == (b"A", 0) if read.startswith(b"min_") else (hap, a) == (b"B", 0), read
    sites1, links1, reads1, st1 = HM.phase(*args(s.case), pairs=s.same_strain_list)
    assert (sites1, links1, reads1) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD)
    assert st1["sites"] == st1["read_records"] == st1["alleles"] == 0 and st1["rows_selected"] == 15
