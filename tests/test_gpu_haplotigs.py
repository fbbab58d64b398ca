"""GPU: hlmi_haplotigs against its model (tests/haplotigs_model.py) - both files byte for byte and every integer stat.  The hand
cases of tests/haplotigs_inputs.py and its shapes (an extent across the count tile's border with an insertion on it, extents that
end and start on the border, D and = runs longer than SHORT_RUN across an extent's edges, two long rows over 300 split blocks,
rows on the '-' strand, CIGARs of 63 / 64 / 65 ops, split blocks on both sides of a contig junction, a contig with rows and no
site, a contig without rows with include_unpolished 0 and 1), each with a pair list, with an empty one and without out_blocks;
the call without a split block against hlmi_polish, with none of the new kernels run; the unsplit contig of a call with a split
one; the phase part of the stats against hlmi_phase; the refusals, with nothing written."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import haplotigs_inputs as GI  # noqa: E402
import haplotigs_model as GM  # noqa: E402
import phase_model as HM  # noqa: E402
import polish_inputs as PI  # noqa: E402
import polish_pairs_inputs as XI  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = GI.hand_cases()
SHAPES = GI.shapes()
NEW_TIMERS = ("hap_intervals", "hap_count", "hap_slots")
PHASE_OPTS = ("min_len", "min_iden", "min_cov", "min_alt", "min_frac", "min_link", "min_agree")
POLISH_OPTS = ("min_len", "min_iden", "min_cov", "include_unpolished")
LAST = {}


def ints(st):
    return {k: st[k] for k in GM.STAT_KEYS}


def run_and_compare(c, d, pairs=None, blocks=True, **opts):
    """-> the model's (fasta, blocks, stats), after the library's files and stats were found equal to them"""
    d = str(d)
    cfa, rfa, paf = c.write(d)
    lst = None
    if pairs is not None:
        lst = os.path.join(d, "pairs.paf")
        with open(lst, "wb") as f:
            f.write(pairs)
    want = GM.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, **opts)
    out = [os.path.join(d, n) for n in ("haplotigs.fa", "haplotigs.blocks.tsv")]
    st = api.haplotigs(cfa, rfa, paf, out[0], out[1] if blocks else None, pairs=lst, **opts)
    LAST.clear()
    LAST.update(api.last_stats())
    assert ints(st) == want[2]
    with open(out[0], "rb") as f:
        assert f.read() == want[0]
    if blocks:
        with open(out[1], "rb") as f:
            assert f.read() == want[1]
    else:
        assert not os.path.exists(out[1])
    return want


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    h = HAND[name]
    fa, blocks, st = run_and_compare(h.case, tmp_path, **h.opts)
    assert fa == h.fasta and blocks == GM.BLOCKS_HEAD + b"".join(line + b"\n" for line in h.blocks)
    assert [LAST.get(f"kernel_ms.{k}", 0) > 0 for k in ("hap_intervals", "hap_count")] == [st["blocks_split"] > 0] * 2


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape(name, tmp_path):
    s = SHAPES[name]
    s.where(*GM.haplotigs(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(), **s.opts))
    _, _, st = run_and_compare(s.case, tmp_path / "plain", **s.opts)
    assert LAST.get("kernel_ms.hap_intervals", 0) > 0 and LAST.get("kernel_ms.hap_count", 0) > 0 and st["blocks_split"] >= 1
    # every other read listed, in either order
    reads = [n for n, _ in s.case.reads]
    target = {r.split(b"\t")[0]: r.split(b"\t")[5] for r in s.case.rows}
    lst = b"".join(XI.row(q, target[q], 14) if i % 4 else XI.row(target[q], q) for i, q in enumerate(reads) if i % 2 == 0)
    _, _, st2 = run_and_compare(s.case, tmp_path / "listed", pairs=lst, **s.opts)
    assert st2["rows_selected"] == (len(reads) + 1) // 2 and st2["rows_not_listed"] == len(reads) // 2
    # an empty list: no row votes, every contig comes back as it is (or not at all)
    fa0, blocks0, st0 = run_and_compare(s.case, tmp_path / "empty", pairs=b"", **s.opts)
    assert blocks0 == GM.BLOCKS_HEAD and st0["rows_selected"] == st0["sites"] == st0["blocks_split"] == 0
    assert fa0 == (s.case.contigs_bytes() if s.opts.get("include_unpolished", 1) else b"")
    run_and_compare(s.case, tmp_path / "no_blocks", blocks=False, **s.opts)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_no_split_block_is_the_polishers_file_and_runs_no_new_kernel(name, tmp_path):
    s = SHAPES[name]
    opts = {**s.opts, "min_side": len(s.case.rows) + 1}
    fa, _, st = run_and_compare(s.case, tmp_path / "hap", **opts)
    assert st["blocks_split"] == 0 and all(LAST.get(f"kernel_ms.{k}", 0) == 0 for k in NEW_TIMERS) and LAST.get("kernel_ms.polish_count", 0) > 0
    cfa, rfa, paf = s.case.write(tmp_path / "polish")
    out = str(tmp_path / "polished.fa")
    pst = api.polish(cfa, rfa, paf, out, **{k: v for k, v in opts.items() if k in POLISH_OPTS})
    with open(out, "rb") as f:
        assert f.read() == fa
    assert all(st[k] == pst[k] for k in ("substituted", "deleted", "inserted_bases", "slots_opened", "ins_long", "ins_edge"))


def test_the_unsplit_contig_of_a_split_call_is_the_polishers_record(tmp_path):
    s = SHAPES["junction_and_plain_contigs_unpolished_1"]
    fa, _, st = run_and_compare(s.case, tmp_path / "hap", **s.opts)
    cfa, rfa, paf = s.case.write(tmp_path / "polish")
    out = str(tmp_path / "polished.fa")
    api.polish(cfa, rfa, paf, out)
    with open(out, "rb") as f:
        polished = {n: (t, b) for n, t, b in GI.records(f.read())}
    mine = {n: (t, b) for n, t, b in GI.records(fa)}
    assert st["contigs_split"] == 2 and mine[b"z"] == polished[b"z"] and mine[b"m"] == polished[b"m"] and b"a" not in mine


@pytest.mark.parametrize("name", ["two_strains", "one_long_row_over_300_split_blocks"])
def test_the_phase_part_of_the_stats_is_hlmi_phases(name, tmp_path):
    c, opts = (HAND[name].case, HAND[name].opts) if name in HAND else (SHAPES[name].case, SHAPES[name].opts)
    cfa, rfa, paf = c.write(tmp_path)
    st = api.haplotigs(cfa, rfa, paf, str(tmp_path / "h.fa"), **opts)
    pst = api.phase(cfa, rfa, paf, str(tmp_path / "sites.tsv"), **{k: v for k, v in opts.items() if k in PHASE_OPTS})
    assert {k: st[k] for k in HM.STAT_KEYS} == {k: pst[k] for k in HM.STAT_KEYS}


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
    outs = [str(tmp_path / n) for n in ("h.fa", "b.tsv")]
    with pytest.raises(Exception):
        GM.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    refused(lambda: api.haplotigs(cfa, rfa, paf, *outs), f"rows.paf:{line}:", outs)
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "reads.fa", "rows.paf"]


def test_option_list_and_name_refusals(tmp_path):
    h = HAND["min_side_at"]
    cfa, rfa, paf = h.case.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("h.fa", "b.tsv")]
    lst = str(tmp_path / "pairs.paf")
    # the six option refusals, in order: every later option is bad too
    later = dict(min_cov=0, min_alt=0, min_frac=-0.5, min_link=0, min_agree=0.5, min_side=0)
    for k, word in enumerate(("min_cov", "min_alt", "min_frac", "min_link", "min_agree", "min_side")):
        bad = {n: v for n, v in list(later.items())[k:]}
        with pytest.raises(GM.PM.Refused):
            GM.haplotigs(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), **bad)
        refused(lambda: api.haplotigs(cfa, rfa, paf, *outs, **bad), "hlmi_haplotigs: " + word + " ", outs)
    # an option refusal comes in front of a row's, a row's in front of the list's
    broken = str(tmp_path / "bad.paf")
    with open(broken, "wb") as f:
        f.write(h.case.paf_bytes().replace(b"cg:Z:2=1X3=1X13=", b"cg:Z:2=1X3=1X12=", 1))
    refused(lambda: api.haplotigs(cfa, rfa, broken, *outs, min_side=0), "min_side", outs)
    with open(lst, "wb") as f:
        f.write(XI.row(b"r0", b"c") + XI.row(b"r1", b"c", 5))
    refused(lambda: api.haplotigs(cfa, rfa, paf, *outs, pairs=lst), "pairs.paf:2:", outs)
    refused(lambda: api.haplotigs(cfa, rfa, broken, *outs, pairs=lst), "bad.paf:1:", outs)
    with pytest.raises(api.HlmiError):
        api.haplotigs(cfa, rfa, paf, *outs, pairs=str(tmp_path / "none.paf"))
    assert not any(os.path.exists(p) for p in outs)
    twice = str(tmp_path / "twice.fa")
    with open(twice, "wb") as f:
        f.write(h.case.contigs_bytes() + b">c\nACGT\n")
    refused(lambda: api.haplotigs(twice, rfa, paf, *outs), "two records are named c", outs)
    with pytest.raises(TypeError):
        api.haplotigs(cfa, rfa, paf, *outs, qual_weight=1)
