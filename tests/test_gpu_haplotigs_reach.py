"""GPU: hlmi_haplotigs_reach against its model (tests/haplotigs_reach_model.py) - both files byte for byte and every integer stat.
reach = 1 on the hand cases and shapes of tests/haplotigs_inputs.py equals hlmi_haplotigs on the same input; the two-strain pile
with one noisy site, cut in three blocks at reach 1, is one split block at reach 2 whose extent covers the bridged site; the
refusals of reach 0 and 9 by both entry points, behind min_side's, with nothing written."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import haplotigs_inputs as GI  # noqa: E402
import haplotigs_reach_model as GR  # noqa: E402
import phase_reach_inputs as RI  # noqa: E402

pytestmark = pytest.mark.gpu
OLD = {**{n: (h.case, h.opts) for n, h in GI.hand_cases().items()}, **{n: (s.case, s.opts) for n, s in GI.shapes().items()}}
NAMES = ("haplotigs.fa", "haplotigs.blocks.tsv")


def ints(st):
    return {k: st[k] for k in GR.STAT_KEYS}


def run_and_compare(c, d, reach, **opts):
    """-> the model's (fasta, blocks, stats), after the library's files and stats were found equal to them"""
    cfa, rfa, paf = c.write(str(d))
    want = GR.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, reach, **opts)
    out = [os.path.join(str(d), n) for n in NAMES]
    st = api.haplotigs_reach(cfa, rfa, paf, *out, reach=reach, **opts)
    assert ints(st) == want[2]
    for path, data in zip(out, want[:2]):
        with open(path, "rb") as f:
            assert f.read() == data, path
    return want


@pytest.mark.parametrize("name", sorted(OLD))
def test_reach_1_is_hlmi_haplotigs(name, tmp_path):
    c, opts = OLD[name]
    want = run_and_compare(c, tmp_path / "reach", 1, **opts)
    last = api.last_stats()
    assert last.get("kernel_ms.phase_link", 0) == 0
    assert (last.get("kernel_ms.phase_link_reach", 0) > 0) == (want[2]["sites"] >= 2 and want[2]["alleles"] > 0)
    cfa, rfa, paf = c.write(str(tmp_path / "plain"))
    out = [str(tmp_path / "plain" / n) for n in NAMES]
    st = api.haplotigs(cfa, rfa, paf, *out, **opts)
    assert ints(st) == want[2]
    for path, data in zip(out, want[:2]):
        with open(path, "rb") as f:
            assert f.read() == data, path


def test_a_noisy_site_inside_one_split_block(tmp_path):
    s = RI.noisy_two_strains(1)
    _, blocks1, st1 = run_and_compare(s.case, tmp_path / "one", 1)
    assert st1["blocks"] == 3 and len(blocks1.split(b"\n")) - 2 == 2                 # the block of one site has no line
    fa, blocks, st = run_and_compare(s.case, tmp_path / "two", 2)
    lines = [line.split(b"\t") for line in blocks.split(b"\n")[1:-1]]
    assert len(lines) == 1 and st["blocks"] == st["blocks_split"] == st["contigs_split"] == 1
    name, block, start, end, n_sites, rows_a, rows_b, split, _ = lines[0]
    assert (int(block), int(start), int(end)) == (s.snps[0] + 1, s.snps[0] + 1, s.snps[-1] + 1) and int(start) <= s.noise[0] + 1 <= int(end)
    assert int(n_sites) == len(s.snps) + 1 and (int(rows_a), int(rows_b), split) == (15, 75, b"1")
    assert [h.split(b" ")[0] for h in fa.split(b"\n") if h.startswith(b">")] == [b">minor_contig_hapA", b">minor_contig_hapB"]
    assert st["positions_split"] == s.snps[-1] - s.snps[0] + 1 and st["diff_positions"] >= len(s.snps)


def test_refusals(tmp_path):
    c, opts = OLD["min_side_at"]
    cfa, rfa, paf = c.write(tmp_path)
    outs = [str(tmp_path / n) for n in ("h.fa", "b.tsv")]
    for call, who in ((lambda **k: api.haplotigs_reach(cfa, rfa, paf, *outs, **k), "hlmi_haplotigs_reach"),
                      (lambda **k: api.haplotigs_reads_reach(cfa, rfa, *outs, **k), "hlmi_haplotigs_reads_reach")):
        for reach in (0, RI.REACH_MAX + 1):
            with pytest.raises(api.HlmiError) as e:
                call(reach=reach)
            assert e.value.code == -1 and f"{who}: reach {reach} " in str(e.value)
        with pytest.raises(api.HlmiError) as e:                   # behind min_side's refusal
            call(reach=0, min_side=0)
        assert f"{who}: min_side " in str(e.value)
    with pytest.raises(GR.PM.Refused):
        GR.haplotigs(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), reach=9)
    assert not any(os.path.exists(p) for p in outs)
