"""CPU: the variant-site model (tests/variants_model.py, the contract of hlmi_variants / hlmi_variants_reads) held to answers
worked by hand from the header's rules - ties between two alternatives, the own base in the minority, N and lower case, every
threshold one below and exactly at its border, a contig of no bases, no site at all - and the case that states what the pair list
is for: two strains, the minor one's contig, five reads of the major strain for every read of the minor one."""
import math
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_pairs_inputs as XI  # noqa: E402
import variants_inputs as VI  # noqa: E402
import variants_model as VM  # noqa: E402

HAND = VI.hand_cases()
SHAPES = VI.shapes()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    h = HAND[name]
    sites, summary, st = VM.variants(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), **h.opts)
    assert sites == VM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert summary == VM.SUMMARY_HEAD + b"".join(line + b"\n" for line in h.summary)
    assert st == {**dict.fromkeys(VM.STAT_KEYS, 0), **h.stats}
    assert st["sites"] == st["sites_base"] + st["sites_del"]


def test_site_rule_literals():
    assert VM.site_at([2, 2, 1, 0, 0], ord("G"), 3, 2, 0.2) == ("site", 0)
    assert VM.site_at([1, 0, 0, 2, 2], ord("a"), 3, 2, 0.2) == ("site", 3)
    assert VM.site_at([0, 0, 0, 0, 0], ord("A"), 1, 1, 0.0) == ("none", None)
    assert VM.site_at([5, 0, 0, 0, 0], ord("A"), 3, 1, 0.0) == ("callable", 1)           # no alternative has a vote: C, with none
    assert VM.site_at([0, 3, 0, 0, 0], ord("N"), 3, 1, 0.0) == ("other", None)
    assert VM.site_at([4, 1, 0, 0, 0], ord("A"), 3, 1, 0.2)[0] == "site"
    assert VM.site_at([4, 1, 0, 0, 0], ord("A"), 3, 1, math.nextafter(0.2, 1.0))[0] == "callable"


def test_option_refusals():
    h = HAND["no_site"]
    args = (h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes())
    for bad in (dict(min_cov=0), dict(min_alt=0), dict(min_frac=-0.01), dict(min_frac=1.01), dict(min_frac=float("nan"))):
        with pytest.raises(VM.PM.Refused) as e:
            VM.variants(*args, **bad)
        assert e.value.line == 0


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_sit_where_they_claim(name):
    s = SHAPES[name]
    s.where(*VM.variants(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(), **s.opts))


def test_two_strains_the_list_removes_the_sister_strains_alleles():
    s = XI.two_strains()
    args = (s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes())
    sites, summary, st = VM.variants(*args)
    rows = VI.site_rows(sites)
    assert [p for _, p, _ in rows] == sorted(s.snps) and len(rows) >= 20
    assert all(alt == s.major[p:p + 1] != s.minor[p:p + 1] for _, p, alt in rows)       # every SNP, with the major allele
    assert st["rows_selected"] == 90 and st["sites"] == st["sites_base"] == len(s.snps) and st["callable"] == 3000
    assert all(f[10:] == [b"%d" % (int(f[3]) * 5 // 6), b"0.833333"] for f in (x.split(b"\t") for x in sites.split(b"\n")[1:-1]))
    sites1, summary1, st1 = VM.variants(*args, pairs=s.same_strain_list)
    assert sites1 == VM.SITES_HEAD and st1["sites"] == 0 and st1["callable"] == 3000
    assert st1["rows_selected"] == st1["pairs_listed"] == 15 and st1["rows_not_listed"] == 75
    assert summary1 == VM.SUMMARY_HEAD + b"%s\t3000\t15\t3000\t0\t0.000000\n" % s.case.contigs[0][0]
