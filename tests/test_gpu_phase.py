"""GPU: hlmi_phase against its model (tests/phase_model.py) - the three files byte for byte and every integer stat.  The hand
cases of tests/phase_inputs.py and its shapes (sites at a row's ends, rows over no and one site, links around PHASE_TILE, a contig
junction, a contig without rows, CIGARs of 63 to 513 ops with I ops in front of sites, ops of SHORT_RUN and one more sites, a D run
across the position-tile border, 4 097 rows on one link), each with a pair list, with an empty one and with the optional files left
out; every run also against hlmi_variants on the same input; the call without a site, whose phase kernels are not launched; the
two-strain case; the refusals, with nothing written."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phase_inputs as HI  # noqa: E402
import phase_model as HM  # noqa: E402
import polish_inputs as PI  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import variants_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = HI.hand_cases()
SHAPES = HI.shapes()
VARIANT_OPTS = ("min_len", "min_iden", "min_cov", "min_alt", "min_frac")
LAST = {}


def ints(st):
    return {k: st[k] for k in HM.STAT_KEYS}


def run_and_compare(c, d, pairs=None, optional=True, **opts):
    """-> the model's (sites, links, reads, stats), after the library's files and stats were found equal to them and the sites and
    the shared stats equal to hlmi_variants's on the same input"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = HM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, **opts)
    out = [os.path.join(d, n) for n in ("phase.sites.tsv", "phase.links.tsv", "phase.reads.tsv")]
    st = api.phase(cfa, rfa, paf, out[0], out[1] if optional else None, out[2] if optional else None, pairs=lst, **opts)
    LAST.clear()
    LAST.update(api.last_stats())               # of the phase call: the variants call below starts its own
    assert ints(st) == want[3]
    for path, data in zip(out, want[:3]):
        if optional or path == out[0]:
            with open(path, "rb") as f:
                assert f.read() == data, path
        else:
            assert not os.path.exists(path)
    vsites = os.path.join(d, "variants.tsv")
    vst = api.variants(cfa, rfa, paf, vsites, None, pairs=lst, **{k: v for k, v in opts.items() if k in VARIANT_OPTS})
    assert {k: st[k] for k in VM.STAT_KEYS} == {k: vst[k] for k in VM.STAT_KEYS}
    with open(vsites, "rb") as f:
        v = [line.split(b"\t") for line in f.read().split(b"\n")[1:-1]]
    p = [line.split(b"\t") for line in want[0].split(b"\n")[1:-1]]
    assert [(f[0], f[1], f[2], f[9], f[3], f[10]) for f in v] == [(f[0], f[1], f[2], f[3], f[4], f[6]) for f in p]
    return want


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    h = HAND[name]
    sites, links, reads, st = run_and_compare(h.case, tmp_path, **h.opts)
    assert sites == HM.SITES_HEAD + b"".join(line + b"\n" for line in h.sites)
    assert links == HM.LINKS_HEAD + b"".join(line + b"\n" for line in h.links)
    assert reads == HM.READS_HEAD + b"".join(line + b"\n" for line in h.reads)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape(name, tmp_path):
    s = SHAPES[name]
    s.where(*HM.phase(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(), **s.opts))
    _, _, _, st = run_and_compare(s.case, tmp_path / "plain", **s.opts)
    assert all(LAST.get(f"kernel_ms.phase_{k}", 0) > 0 for k in ("allele", "link", "assign"))
    assert st["pairs_listed"] == st["rows_not_listed"] == 0 and st["sites"] >= 2
    # every other read listed, in either order
    reads = [n for n, _ in s.case.reads]
    target = {r.split(b"\t")[0]: r.split(b"\t")[5] for r in s.case.rows}
    lst = b"".join(XI.row(q, target[q], 14) if i % 4 else XI.row(target[q], q) for i, q in enumerate(reads) if i % 2 == 0)
    _, _, _, st2 = run_and_compare(s.case, tmp_path / "listed", pairs=lst, **s.opts)
    assert st2["rows_selected"] == (len(reads) + 1) // 2 and st2["rows_not_listed"] == len(reads) // 2
    # an empty list: no row votes, three header lines
    sites0, links0, reads0, st0 = run_and_compare(s.case, tmp_path / "empty", pairs=b"", **s.opts)
    assert (sites0, links0, reads0) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD)
    assert st0["rows_selected"] == st0["sites"] == st0["alleles"] == st0["blocks"] == 0 and st0["rows_not_listed"] == len(reads)
    # neither optional file asked for
    run_and_compare(s.case, tmp_path / "sites_only", optional=False, **s.opts)


def test_no_site_phase_kernels_not_launched(tmp_path):
    T = HI.T
    ref = HI._seq(2 * T + 7, 4)
    c = HI.pile(ref, [{}] * 4, strands="+-")
    sites, links, reads, st = run_and_compare(c, tmp_path)
    assert (sites, links, reads) == (HM.SITES_HEAD, HM.LINKS_HEAD, HM.READS_HEAD) and st["sites"] == 0 and st["callable"] == 2 * T + 7
    assert LAST.get("kernel_ms.variants_tile", 0) > 0 and LAST.get("kernel_ms.variants_sites", 0) == 0
    assert all(LAST.get(f"kernel_ms.phase_{k}", 0) == 0 for k in ("allele", "link", "assign"))


def test_two_strains(tmp_path):
    s = XI.two_strains()
    sites, links, reads, st = run_and_compare(s.case, tmp_path / "all")
    assert st["links_phased"] == st["links"] == len(s.snps) - 1 and st["blocks"] == 1
    assert (st["read_records"], st["reads_a"], st["reads_b"], st["reads_tie"]) == (90, 15, 75, 0)
    for read, _, _, _, a, b, _, hap in HI.read_rows(reads):
        assert (hap, b) == (b"A", 0) if read.startswith(b"min_") else (hap, a) == (b"B", 0), read
    sites1, _, reads1, st1 = run_and_compare(s.case, tmp_path / "listed", pairs=s.same_strain_list)
    assert sites1 == HM.SITES_HEAD and reads1 == HM.READS_HEAD and st1["sites"] == st1["read_records"] == 0 and st1["rows_selected"] == 15


def refused(call, word, outs):
    with pytest.raises(api.HlmiError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)
    for p in outs:
        assert not os.path.exists(p)


REFUSALS = PI.refusal_cases()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_row_refusals(name, tmp_path):
    c, line = REFUSALS[name]
    cfa, rfa, paf = c.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("s.tsv", "l.tsv", "r.tsv")]
    with pytest.raises(Exception):
        HM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    refused(lambda: api.phase(cfa, rfa, paf, *outs), f"rows.paf:{line}:", outs)
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "reads.fa", "rows.paf"]


def test_option_list_and_name_refusals(tmp_path):
    h = HAND["cis"]
    cfa, rfa, paf = h.case.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("s.tsv", "l.tsv", "r.tsv")]
    lst = str(tmp_path / "pairs.paf")
    # the five option refusals, in order: every later option is bad too
    later = dict(min_cov=0, min_alt=0, min_frac=-0.5, min_link=0, min_agree=0.5)
    for k, word in enumerate(("min_cov", "min_alt", "min_frac", "min_link", "min_agree")):
        bad = {n: v for n, v in list(later.items())[k:]}
        with pytest.raises(HM.PM.Refused):
            HM.phase(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), **bad)
        refused(lambda: api.phase(cfa, rfa, paf, *outs, **bad), word + " ", outs)
    for bad in (dict(min_agree=1.5), dict(min_agree=float("nan")), dict(min_frac=float("nan"))):
        refused(lambda: api.phase(cfa, rfa, paf, *outs, **bad), next(iter(bad)), outs)
    # an option refusal comes in front of a row's
    broken = str(tmp_path / "bad.paf")
    with open(broken, "wb") as f:
        f.write(h.case.paf_bytes().replace(b"cg:Z:2=1X3=1X13=", b"cg:Z:2=1X3=1X12=", 1))
    refused(lambda: api.phase(cfa, rfa, broken, *outs, min_link=0), "min_link", outs)
    with open(lst, "wb") as f:
        f.write(XI.row(b"r0", b"c") + XI.row(b"r1", b"c", 5))
    refused(lambda: api.phase(cfa, rfa, paf, *outs, pairs=lst), "pairs.paf:2:", outs)
    # a row refusal comes in front of the list's
    refused(lambda: api.phase(cfa, rfa, broken, *outs, pairs=lst), "bad.paf:1:", outs)
    # a missing list cannot be read
    with pytest.raises(api.HlmiError):
        api.phase(cfa, rfa, paf, *outs, pairs=str(tmp_path / "none.paf"))
    assert not any(os.path.exists(p) for p in outs)
    # two records of one name, among the contigs and among the reads
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(h.case.contigs_bytes() + b">c\nACGT\n")
    refused(lambda: api.phase(twice, rfa, paf, *outs), "two records are named c", outs)
    with open(twice, "wb") as f:
        f.write(h.case.reads_bytes() + b">r1\nACGT\n")
    refused(lambda: api.phase(cfa, twice, paf, *outs), "two records are named r1", outs)
    with pytest.raises(TypeError):
        api.phase(cfa, rfa, paf, *outs, qual_weight=1)
