"""GPU: hlmi_polish_reads against the chain it stands for - hlmi_ava into a PAF, then hlmi_polish over that PAF: the
output file byte for byte and every integer stat, on small inputs (tests/polish_reads_inputs.py).  Every case first asserts
on the chain's own PAF and stats that it exercises what it is there for: votes of every kind with the long and the short
constants, rows over the count kernel's tile edge, a tie between two contigs (the earlier line wins), the two thresholds
at their edges, bytes that do not vote and lower case that stays, contigs without rows, the refusals, and the driver's
`--polish_direct` beside `--polish_native`."""
import math
import os
import sys

import pytest

from hylight_amd import api, driver, simulate as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_reads_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu
INT_STATS = api.POLISH_STATS


def ava_opts(inp, **fields):
    o = api.ava_opts_short() if inp.short else api.ava_opts_long()
    o.pair_once = 0
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def write(inp, d):
    os.makedirs(d, exist_ok=True)
    cfa, rfa = os.path.join(d, "contigs.fa"), os.path.join(d, "reads.fa")
    with open(cfa, "wb") as f:
        f.write(I.fasta(inp.contigs))
    with open(rfa, "wb") as f:
        f.write(I.fasta(inp.reads))
    return cfa, rfa


def chain(inp, d, **over):
    """hlmi_ava + hlmi_polish -> (PAF rows, output bytes, stats)"""
    cfa, rfa = write(inp, d)
    paf, out = os.path.join(d, "chain.paf"), os.path.join(d, "chain.fa")
    api.ava(cfa, rfa, paf, ava_opts(inp))
    st = api.polish(cfa, rfa, paf, out, **{**inp.opts, **over})
    with open(paf, "rb") as f:
        rows = I.paf_rows(f.read())
    with open(out, "rb") as f:
        return rows, f.read(), st


def direct(inp, d, **over):
    cfa, rfa = write(inp, d)
    out = os.path.join(d, "direct.fa")
    st = api.polish_reads(cfa, rfa, out, ava_opts(inp), **{**inp.opts, **over})
    assert not [n for n in os.listdir(d) if n not in ("contigs.fa", "reads.fa", "chain.paf", "chain.fa", "direct.fa")]
    with open(out, "rb") as f:
        return f.read(), st


def same(inp, d, **over):
    rows, want, want_st = chain(inp, d, **over)
    got, st = direct(inp, d, **over)
    print({k: want_st[k] for k in INT_STATS})
    assert {k: st[k] for k in INT_STATS} == {k: want_st[k] for k in INT_STATS}
    assert got == want
    assert st["ms_total"] >= st["ms_device"] >= 0
    return rows, want, want_st


@pytest.fixture(scope="module")
def long_case(tmp_path_factory):
    inp = I.every_kind_long()
    rows, want, st = chain(inp, str(tmp_path_factory.mktemp("long")))
    return inp, rows, want, st


def test_votes_of_every_kind_long(long_case, tmp_path):
    inp, rows, _, st = long_case
    tile = PI.kernel_constants()["tile"]
    assert st["substituted"] > 0 and st["deleted"] > 0 and st["inserted_bases"] > 0 and st["contigs_polished"] == 3
    assert any(r["ts"] < tile < r["te"] for r in rows) and any(r["ts"] < 2 * tile < r["te"] for r in rows)
    assert st["rows"] == len(rows) > st["rows_selected"] >= 50                # (some reads have a row on two contigs)
    same(inp, tmp_path)


def test_votes_of_every_kind_short(tmp_path):
    inp = I.every_kind_short()
    assert inp.short and inp.opts["min_len"] == 70 and all(len(s) == 150 for _, s in inp.reads)
    _, _, st = same(inp, tmp_path)
    assert st["substituted"] > 0 and st["deleted"] > 0 and st["inserted_bases"] > 0 and st["rows_selected"] >= 150


def test_tie_between_two_contigs(tmp_path):
    rows, want, st = same(I.tie_between_contigs(), tmp_path)
    spans = {}
    for r in rows:
        spans.setdefault(r["q"], []).append((r["t"], r["te"] - r["ts"]))
    tied = [v for v in spans.values() if len(v) == 2 and v[0][0] != v[1][0] and v[0][1] == v[1][1]]
    assert tied and st["rows_selected"] == len(spans)
    # every read's earlier line is on one contig: that one is polished, the other comes back as it is
    assert st["contigs_polished"] == 1 and len({v[0][0] for v in tied}) == 1
    heads = want.split(b"\n")[0::2]
    assert sum(b"RC:i:" in h for h in heads) == 1


def test_thresholds_at_their_edges(long_case, tmp_path):
    inp, rows, _, _ = long_case
    # a row that is its read's only one: the read is selected exactly when the row is kept
    per_read = {}
    for r in rows:
        per_read.setdefault(r["q"], []).append(r)
    alone = sorted((v[0] for v in per_read.values() if len(v) == 1), key=lambda r: r["te"] - r["ts"])
    row = alone[len(alone) // 2]
    span, quot = row["te"] - row["ts"], row["n_eq"] / row["n_all"]          # the same double division as the library's
    up = math.nextafter(quot, math.inf)
    assert 0.9 < quot < 1.0 and up > quot
    n = []
    for k, over in enumerate((dict(min_len=span, min_iden=0.0), dict(min_len=span + 1, min_iden=0.0),
                              dict(min_len=0, min_iden=quot), dict(min_len=0, min_iden=up))):
        _, _, st = same(inp, tmp_path / str(k), **over)
        assert st["rows_selected"] == I.expect_selected(rows, over["min_len"], over["min_iden"])
        n.append(st["rows_selected"])
    # kept at the lower value of each threshold, dropped at the upper one - with the other reads whose only chance sits there
    assert n[0] - n[1] == sum(max(r["te"] - r["ts"] for r in v) == span for v in per_read.values()) >= 1
    assert n[2] - n[3] == sum(max(r["n_eq"] / r["n_all"] for r in v) == quot for v in per_read.values()) >= 1


def test_bytes_that_do_not_vote_and_case(tmp_path):
    inp = I.non_voting_and_case()
    reads = b"".join(s for _, s in inp.reads)
    assert all(c in reads for c in b"NRUu") and any(c in reads for c in b"acgt")
    _, want, st = same(inp, tmp_path)
    seq = want.split(b"\n")[1]
    assert st["rows_selected"] >= 30 and st["substituted"] + st["deleted"] > 0
    assert sum(97 <= c <= 122 for c in seq) >= 50                          # the stretch below min_cov keeps its lower case
    assert b" XC:f:0." in want.split(b"\n")[0]


@pytest.mark.parametrize("include_unpolished", [1, 0])
def test_contig_without_rows(include_unpolished, tmp_path):
    _, want, st = same(I.contig_without_rows(include_unpolished), tmp_path)
    assert st["contigs"] == 3 and st["contigs_polished"] == 2
    names = [h.split()[0] for h in want.split(b"\n")[0:-1:2]]
    assert names == ([b">c0", b">c1", b">c2"] if include_unpolished else [b">c0", b">c2"])


def test_no_read_matches_anything(tmp_path):
    inp = I.no_read_matches()
    _, want, st = same(inp, tmp_path)
    assert st["rows"] == 0 and st["contigs_polished"] == 0 and want == I.fasta(inp.contigs)


def _refused(inp, d, o, **opts):
    cfa, rfa = write(inp, d)
    out = os.path.join(d, "direct.fa")
    with pytest.raises(api.HlmiError) as e:
        api.polish_reads(cfa, rfa, out, o, **{**inp.opts, **opts})
    assert e.value.code == -1                                                   # HLMI_EINVAL
    assert sorted(os.listdir(d)) == ["contigs.fa", "reads.fa"]
    return str(e.value)


def test_refusals_leave_no_file(tmp_path):
    inp = I.contig_without_rows(1)
    twice = inp._replace(reads=inp.reads + [(inp.reads[3][0], inp.reads[5][1])])
    assert inp.reads[3][0] in _refused(twice, str(tmp_path / "read"), ava_opts(inp))
    twice = inp._replace(contigs=inp.contigs + [("c1", inp.contigs[0][1])])
    assert "c1" in _refused(twice, str(tmp_path / "contig"), ava_opts(inp))
    assert "stub_oh" in _refused(inp, str(tmp_path / "stub"), ava_opts(inp, stub_oh=3))
    assert "min_cov" in _refused(inp, str(tmp_path / "cov"), ava_opts(inp), min_cov=0)
    with pytest.raises(TypeError):
        api.polish_reads("c.fa", "r.fa", "o.fa", None, window=500)


def test_driver_polish_direct(tmp_path):
    reads, _ = S.simulate_reads(seed=83, n_strains=2, genome_len=30000, n_reads=90, mean_len=9000, min_len=7000, max_len=14000)
    lfq = tmp_path / "long.fq"
    S.write_fastq(reads, lfq)
    outs = {}
    for flag in ("--polish_native", "--polish_direct"):
        out = tmp_path / flag.strip("-")
        argv = ["-l", str(lfq), "-o", str(out), "--corrected", "--nsplit", "3", "-t", "4", "--stop_after", "polish", flag]
        assert driver.main(argv) == 0
        outs[flag] = out / "tmp"
    want = (outs["--polish_native"] / "long_con_polished.fa").read_bytes()
    assert want.count(b">") >= 1 and (outs["--polish_native"] / "polish_1.paf").stat().st_size > 0
    assert (outs["--polish_direct"] / "long_con_polished.fa").read_bytes() == want
    assert (outs["--polish_direct"] / "polish1.fa").read_bytes() == (outs["--polish_native"] / "polish1.fa").read_bytes()
    assert not [n for n in os.listdir(outs["--polish_direct"]) if n.startswith("polish_") and n.endswith(".paf")]
    with pytest.raises(SystemExit) as e:
        driver.main(["-l", str(lfq), "-o", str(tmp_path / "both"), "--polish_native", "--polish_direct"])
    assert "--polish_direct" in str(e.value)
