"""GPU: hlmi_variants_ins against its model (tests/variants_ins_model.py) - the sites, the insertion sites and the summary byte
for byte and every integer stat, and out_sites against the file hlmi_variants writes for the same arguments.  The hand cases of
tests/variants_ins_inputs.py (the spanning rules, edge insertions, the cap at 16 and 17, long rows alone, merged I ops, the ties,
strand and case, every threshold one below and exactly at its border) and its shapes (the first and last slot of contigs around
the tile, no slot on position 0 of the next contig, slots on the tile borders, a cbase that is no multiple of the tile, tiles
with one kind of site and with none, the lane / wave switch in CIGARs of 63 to 513 ops, 4 097 rows on one slot), each with a
pair list and with an empty one; the tiles revisited are the union of both kinds; the call without a site launches neither the
second pass nor the slot passes; the two-strain case the polisher leaves shut; the refusals, with nothing written."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402
import variants_inputs as VI  # noqa: E402
import variants_ins_inputs as II  # noqa: E402
import variants_ins_model as IM  # noqa: E402
import variants_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = II.hand_cases()
SHAPES = II.shapes()
LAST = {}                                       # api.last_stats() of run_and_compare's hlmi_variants_ins call


def ints(st):
    return {k: st[k] for k in IM.STAT_KEYS}


def read(p):
    with open(p, "rb") as f:
        return f.read()


def run_and_compare(c, d, pairs=None, summary=True, identity=False, **opts):
    """-> the model's (sites, ins, summary, stats), after the library's files and stats were found equal to them"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = IM.variants_ins(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, **opts)
    sites, ins, summ = (os.path.join(d, n) for n in ("sites.tsv", "ins.tsv", "summary.tsv"))
    st = api.variants_ins(cfa, rfa, paf, sites, ins, summ if summary else None, pairs=lst, **opts)
    LAST.clear()
    LAST.update(api.last_stats())               # of this call: the older call below resets them
    print(name_of(c), ints(st))
    assert ints(st) == want[3]
    assert read(sites) == want[0]
    assert read(ins) == want[1]
    if summary:
        assert read(summ) == want[2]
    else:
        assert not os.path.exists(summ)
    if identity:                                # out_sites is the file the older call writes, its stats the older call's
        old = os.path.join(d, "sites_old.tsv")
        st_old = api.variants(cfa, rfa, paf, old, pairs=lst, **opts)
        assert read(old) == read(sites) and {k: st_old[k] for k in VM.STAT_KEYS} == {k: st[k] for k in VM.STAT_KEYS}
    return want


def name_of(c):
    return b",".join(n for n, _ in c.contigs).decode()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    h = HAND[name]
    sites, ins, summary, st = run_and_compare(h.case, tmp_path, **h.opts)
    assert ins == IM.INS_HEAD + b"".join(line + b"\n" for line in h.ins)
    assert summary == IM.SUMMARY_HEAD + b"".join(line + b"\n" for line in h.summary)
    assert st == {**dict.fromkeys(IM.STAT_KEYS, 0), **h.stats}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape(name, tmp_path):
    s = SHAPES[name]
    s.where(*IM.variants_ins(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(), **s.opts))
    _, ins, _, st = run_and_compare(s.case, tmp_path / "plain", identity=True, **s.opts)
    last = dict(LAST)
    assert last["variants_tiles"] >= 1 and 1 <= last["variants_tiles_revisited"] <= last["variants_tiles"]
    assert last["variants_ins_slot_sites"] == sum(1 for r in IM.ins_rows(ins) if r[3] >= 1) >= 1
    assert last.get("kernel_ms.variants_slots", 0) > 0
    assert st["pairs_listed"] == st["rows_not_listed"] == 0
    # every other read listed, in either order
    reads = [n for n, _ in s.case.reads]
    target = {r.split(b"\t")[0]: r.split(b"\t")[5] for r in s.case.rows}
    lst = b"".join(XI.row(q, target[q], 14) if i % 4 else XI.row(target[q], q) for i, q in enumerate(reads) if i % 2 == 0)
    _, _, _, st2 = run_and_compare(s.case, tmp_path / "listed", pairs=lst, identity=True, **s.opts)
    assert st2["rows_selected"] == (len(reads) + 1) // 2 and st2["rows_not_listed"] == len(reads) // 2
    # an empty list: no row votes, spans or inserts - header lines alone and zeros
    sites0, ins0, summ0, st0 = run_and_compare(s.case, tmp_path / "empty", pairs=b"", **s.opts)
    assert sites0 == VM.SITES_HEAD and ins0 == IM.INS_HEAD and st0["rows_not_listed"] == len(reads)
    assert all(st0[k] == 0 for k in ("rows_selected", "callable", "sites", "slots_callable", "ins_sites", "ins_long", "ins_edge"))
    assert all(line.split(b"\t")[2:] == [b"0", b"0", b"0", b"0.000000", b"0", b"0", b"0.000000"] for line in summ0.split(b"\n")[1:-1])
    # no summary asked for
    run_and_compare(s.case, tmp_path / "nosummary", summary=False, **s.opts)


def test_the_tiles_revisited_are_the_union_of_both_kinds(tmp_path):
    s = SHAPES["tiles_with_one_kind_of_site"]
    run_and_compare(s.case, tmp_path / "ins", **s.opts)
    last = api.last_stats()
    assert (last["variants_tiles"], last["variants_tiles_revisited"], last["variants_ins_slot_sites"]) == (5, 3, 2)
    cfa, rfa, paf = s.case.write(tmp_path / "old")
    api.variants(cfa, rfa, paf, str(tmp_path / "old.tsv"), **s.opts)          # the older call sees the base site's tile alone
    last = api.last_stats()
    assert (last["variants_tiles"], last["variants_tiles_revisited"]) == (5, 1) and "variants_ins_slot_sites" not in last


def test_no_site_no_second_pass_and_no_slot_pass(tmp_path):
    T = II.T
    ref = VI._seq(2 * T + 7, 4)
    c = II.pile(PI.Case([("c", ref)]), ref, T, [None] * 4, strands="+-")
    sites, ins, summary, st = run_and_compare(c, tmp_path)
    assert sites == VM.SITES_HEAD and ins == IM.INS_HEAD and st["sites"] == st["ins_sites"] == 0
    assert st["callable"] == 2 * T + 7 and st["slots_callable"] == 2 * T + 6
    last = api.last_stats()
    assert last["variants_tiles"] == 3 and last["variants_tiles_revisited"] == 0 and last["variants_ins_slot_sites"] == 0
    assert last.get("kernel_ms.variants_tile", 0) > 0
    assert last.get("kernel_ms.variants_sites", 0) == 0 and last.get("kernel_ms.variants_slots", 0) == 0


def test_long_rows_alone_run_no_slot_vote(tmp_path):
    h = HAND["long_rows_alone"]
    run_and_compare(h.case, tmp_path, **h.opts)
    last = api.last_stats()
    assert last["variants_tiles_revisited"] == 1 and last["variants_ins_slot_sites"] == 0


def test_two_strains_a_site_the_polisher_leaves_shut(tmp_path):
    s = II.two_strains()
    _, ins, _, st = run_and_compare(s.case, tmp_path / "all", identity=True, **s.opts)
    assert IM.ins_rows(ins) == [(b"major_contig", s.slot, 36, 6, 0, 3, 6, s.bases)] and st["ins_sites"] == 1
    cfa, rfa, paf = s.case.write(tmp_path / "polish")
    pst = api.polish(cfa, rfa, paf, str(tmp_path / "polished.fa"))
    assert pst["slots_opened"] == 0 and pst["inserted_bases"] == 0                # 2 i <= s: the majority strain wins
    _, ins1, _, st1 = run_and_compare(s.case, tmp_path / "listed", pairs=s.same_strain_list, **s.opts)
    assert ins1 == IM.INS_HEAD and st1["ins_sites"] == 0 and st1["rows_selected"] == 75 and st1["rows_not_listed"] == 15


def refused(call, word, outs):
    with pytest.raises(api.HlmiError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)
    for p in outs:
        assert not os.path.exists(p)


def test_refusals_write_nothing(tmp_path):
    h = HAND["min_alt_at"]
    cfa, rfa, paf = h.case.write(tmp_path)
    sites, ins, summ, lst = (str(tmp_path / n) for n in ("s.tsv", "i.tsv", "t.tsv", "pairs.paf"))
    outs = (sites, ins, summ)
    # out_ins NULL comes first: in front of an option refusal, in front of a file that cannot be read
    refused(lambda: api.variants_ins(cfa, rfa, paf, sites, None, summ), "out_ins", outs)
    refused(lambda: api.variants_ins(cfa, rfa, paf, sites, None, summ, min_cov=0), "out_ins", outs)
    refused(lambda: api.variants_ins(str(tmp_path / "none.fa"), rfa, paf, sites, None, summ), "out_ins", outs)
    for bad, word in ((dict(min_cov=0), "min_cov"), (dict(min_alt=0), "min_alt"), (dict(min_frac=-0.5), "min_frac"),
                      (dict(min_frac=1.5), "min_frac"), (dict(min_frac=float("nan")), "min_frac"),
                      (dict(min_cov=0, min_alt=0), "min_cov"), (dict(min_alt=0, min_frac=2.0), "min_alt")):
        with pytest.raises(VM.PM.Refused):
            IM.variants_ins(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), **bad)
        refused(lambda: api.variants_ins(cfa, rfa, paf, sites, ins, summ, **bad), word, outs)
    with open(lst, "wb") as f:
        f.write(XI.row(b"r0", b"c") + XI.row(b"r1", b"c", 5))
    refused(lambda: api.variants_ins(cfa, rfa, paf, sites, ins, summ, pairs=lst), "pairs.paf:2:", outs)
    # a row refusal comes in front of the list's, an option refusal in front of both
    bad = str(tmp_path / "bad.paf")
    with open(bad, "wb") as f:
        f.write(h.case.paf_bytes().replace(b"cg:Z:4=1I6=", b"cg:Z:4=1I5=", 1))
    refused(lambda: api.variants_ins(cfa, rfa, bad, sites, ins, summ, pairs=lst), "bad.paf:1:", outs)
    refused(lambda: api.variants_ins(cfa, rfa, bad, sites, ins, summ, pairs=lst, min_alt=0), "min_alt", outs)
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(h.case.contigs_bytes() + b">c\nACGT\n")
    refused(lambda: api.variants_ins(twice, rfa, paf, sites, ins, summ), "two records are named c", outs)
    assert sorted(os.listdir(tmp_path)) == ["bad.paf", "contigs.fa", "pairs.paf", "reads.fa", "rows.paf", "twice.fa"]
