"""GPU: hlmi_polish against its model (tests/polish_model.py) - the file byte for byte and every stat - on the hand cases,
on piles around the count kernel's tile (contigs of T - 1 .. 2T + 1 positions, rows and opened slots on the border), on
rows of 1, 63, 64, 65 and 513 CIGAR ops (the walk takes 64 at a time), with contigs that get no row, on the quality
case's inputs, and every refusal (HLMI_EINVAL naming the line, no file written).  The kernel's counters are all 32 bits
wide, so there is no narrow-counter limit to stand around; one pile of 65 537 rows on one position shows it."""
import os
import sys

import pytest

from hylight_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = PI.hand_cases()
TILES = PI.tile_cases()
REFUSED = PI.refusal_cases()


def check(case, tmp_path):
    cfa, rfa, paf = case.write(tmp_path)
    want, want_st = PM.polish(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes(), **case.opts)
    out = tmp_path / "polished.fa"
    st = api.polish(cfa, rfa, paf, out, **case.opts)
    assert {k: st[k] for k in PM.STAT_KEYS} == want_st
    assert out.read_bytes() == want
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "polished.fa", "reads.fa", "rows.paf"]     # no temporary left
    assert st["ms_total"] >= st["ms_device"] >= 0
    return st


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    check(HAND[name], tmp_path)
    assert (tmp_path / "polished.fa").read_bytes() == HAND[name].want[0]


@pytest.mark.parametrize("name", sorted(TILES, key=lambda s: int(s.split("_")[1])))
def test_tile_edges(name, tmp_path):
    st = check(TILES[name], tmp_path)
    assert st["slots_opened"] >= 1 and st["deleted"] + st["substituted"] >= 1            # (the pile is not a plain copy)


@pytest.mark.parametrize("n_ops", [1, 63, 64, 65, 513])
def test_cigar_batches(n_ops, tmp_path):
    st = check(PI.ops_case(n_ops), tmp_path)
    assert st["substituted"] == (n_ops // 2 + 2) // 3 and st["slots_opened"] == (n_ops // 2) // 3


@pytest.mark.parametrize("include_unpolished", [0, 1])
def test_middle_contig_without_rows(include_unpolished, tmp_path):
    st = check(PI.three_contigs_case(include_unpolished), tmp_path)
    assert st["contigs"] == 3 and st["contigs_polished"] == 2
    names = [l.split()[0] for l in (tmp_path / "polished.fa").read_text().splitlines()[::2]]
    assert names == ([">c0", ">c1", ">c2"] if include_unpolished else [">c0", ">c2"])


def test_no_usable_row(tmp_path):
    st = check(PI.no_usable_row_case(), tmp_path)
    assert st["rows"] > 0 and st["rows_selected"] == 0 and st["contigs_polished"] == 0


def test_deep_pile_on_one_position(tmp_path):
    """65 537 identical rows of seven columns: one more than a 16-bit counter holds, all voting T on position 20 and
    opening the slot in front of position 23."""
    ref = PI.random_contig(__import__("numpy").random.default_rng(5), 40, lower=0, n_frac=0)
    alt = b"T" if ref[20:21] != b"T" else b"G"
    c = PI.Case([("c", ref)])
    for _ in range(65537):
        c.add(18, "2=1X2=2I2=", ref[18:20] + alt + ref[21:23] + b"CA" + ref[23:25])
    st = check(c, tmp_path)
    assert st["rows_selected"] == 65537 and st["substituted"] == 1 and st["inserted_bases"] == 2
    assert (tmp_path / "polished.fa").read_bytes().split(b"\n")[1] == ref[:20] + alt + ref[21:23] + b"CA" + ref[23:]


def test_quality_case_inputs(tmp_path):
    from oracle import ava as OA
    q = PI.quality_case()
    cfa, rfa, paf, out = tmp_path / "contig.fa", tmp_path / "reads.fa", tmp_path / "rows.paf", tmp_path / "polished.fa"
    cfa.write_bytes(b">contig\n" + q["contig"] + b"\n")
    rfa.write_bytes(q["reads_fa"])
    o = OA.opts_long()
    o.pair_once = 0
    OA.ava(cfa, rfa, paf, o)
    want, want_st = PM.polish(cfa.read_bytes(), q["reads_fa"], paf.read_bytes(), min_len=1000, min_iden=0.9)
    st = api.polish(cfa, rfa, paf, out, min_len=1000, min_iden=0.9)
    print(f"quality case: ms_device {st['ms_device']:.2f}, ms_total {st['ms_total']:.2f}")
    assert {k: st[k] for k in PM.STAT_KEYS} == want_st and want_st["slots_opened"] > 50
    assert out.read_bytes() == want


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusal_leaves_no_file(name, tmp_path):
    case, line = REFUSED[name]
    cfa, rfa, paf = case.write(tmp_path)
    with pytest.raises(api.HlmiError) as e:
        api.polish(cfa, rfa, paf, tmp_path / "polished.fa", **case.opts)
    assert e.value.code == -1 and f"rows.paf:{line}:" in str(e.value)
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "reads.fa", "rows.paf"]


def test_min_cov_below_one_is_refused(tmp_path):
    cfa, rfa, paf = HAND["del_wins"].write(tmp_path)
    with pytest.raises(api.HlmiError) as e:
        api.polish(cfa, rfa, paf, tmp_path / "polished.fa", min_cov=0)
    assert e.value.code == -1 and not (tmp_path / "polished.fa").exists()
    with pytest.raises(TypeError):
        api.polish(cfa, rfa, paf, tmp_path / "polished.fa", window=500)


def test_command_line_module(tmp_path, capsys):
    import json
    from hylight_amd import polish
    case = HAND["reverse_strand"]
    cfa, rfa, paf = case.write(tmp_path)
    assert polish.main(["--contigs", cfa, "--reads", rfa, "--paf", paf, "--out", str(tmp_path / "o.fa")]) == 0
    st = json.loads(capsys.readouterr().out)
    assert (tmp_path / "o.fa").read_bytes() == case.want[0] and st["slots_opened"] == 1
