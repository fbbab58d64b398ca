"""CPU: the model of the polisher (tests/polish_model.py, the contract of hlmi_polish) on hand-worked cases whose answers
are written out in tests/polish_inputs.py, every refusal, the parser and symbol checks, and the quality case: on a
simulated 30 kb contig with ~300 planted errors under ~30x corrected reads, the polished contig lies closer to the truth
than the unpolished one (NM of oracle.ava against the true segment: 397 before, 23 after - DESIGN.md section 7)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_model as PM  # noqa: E402

HAND = PI.hand_cases()
REFUSED = PI.refusal_cases()


def run_model(case):
    return PM.polish(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes(), **case.opts)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    case = HAND[name]
    out, st = run_model(case)
    want_out, want_st = case.want
    assert out == want_out
    assert st == {**dict.fromkeys(PM.STAT_KEYS, 0), **want_st}


def test_hand_cases_cover_the_issue_list():
    assert set(HAND) >= {"tie_own_among", "tie_own_not_among", "del_wins", "coverage_edge", "slot_majority",
                         "slot_length_and_base_ties", "insertion_cap", "two_insertions_around_a_deletion",
                         "insertion_at_cigar_ends", "reverse_strand", "n_and_lower_case", "one_row_per_read",
                         "slots_on_the_tile_border"}
    assert PM.CAP == PI.kernel_constants()["cap"] == 16


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusal(name):
    case, line = REFUSED[name]
    with pytest.raises(PM.Refused) as e:
        run_model(case)
    assert e.value.line == line


def test_min_cov_below_one_is_refused():
    with pytest.raises(PM.Refused):
        PM.polish(b">c\nACGT\n", b"", b"", min_cov=0)


def test_unpolished_contigs_and_fastq_input():
    contigs = b"@c0 some comment\nACGT\nAC\n+\nIIIIII\n>c1\n\n>c2\nGG\n"
    out, st = PM.polish(contigs, b"", b"")
    assert out == b">c0\nACGTAC\n>c2\nGG\n" and st["contigs"] == 3 and st["contigs_polished"] == 0
    assert PM.polish(contigs, b"", b"", include_unpolished=0)[0] == b""


def test_generated_piles_are_valid_and_open_slots_at_the_tile_border():
    T = PI.kernel_constants()["tile"]
    case = PI.tile_cases()[f"contig_{2 * T + 1}"]
    out, st = run_model(case)
    assert st["rows_selected"] == len(case.rows) and st["slots_opened"] >= 2 and st["deleted"] >= 1 and st["substituted"] >= 1
    for c in PI.tile_cases().values():
        st = run_model(c)[1]
        assert st["slots_opened"] >= 1 and st["deleted"] + st["substituted"] >= 1
    for n in (1, 63, 64, 65, 513):
        c = PI.ops_case(n)
        assert all(len(PI.cigar_ops(r.split(b"\t")[-1][5:].decode())) == n for r in c.rows[:4])
        st = run_model(c)[1]
        assert st["rows_selected"] == 5 and st["substituted"] == (n // 2 + 2) // 3 and st["deleted"] == (n // 2 + 1) // 3


def test_parser_and_symbols():
    from hylight_amd import api, driver, polish
    a = driver.build_parser().parse_args(["-l", "x.fq", "--polish_native"])
    assert a.polish_native and not driver.build_parser().parse_args(["-l", "x.fq"]).polish_native
    assert "hlmi_polish" in api.SYMBOLS and "hlmi_polish_opts_default" in api.SYMBOLS
    assert api.ABI_VERSION == 7
    assert [k for k, _ in api.PolishOpts._fields_] == ["min_len", "min_iden", "min_cov", "include_unpolished"]
    assert tuple(k for k, _ in api.PolishStats._fields_) == PM.STAT_KEYS + ("ms_device", "ms_total")
    b = polish.build_parser().parse_args(["--contigs", "c", "--reads", "r", "--paf", "p", "--out", "o", "--min_cov", "5"])
    assert (b.min_len, b.min_iden, b.min_cov) == (0, 0.0, 5)


def _nm_against_truth(tmp_path, tag, truth, contig):
    from oracle import ava as OA
    t, q, paf = tmp_path / f"truth_{tag}.fa", tmp_path / f"{tag}.fa", tmp_path / f"{tag}.paf"
    t.write_bytes(b">truth\n" + truth + b"\n")
    q.write_bytes(b">" + tag.encode() + b"\n" + contig + b"\n")
    o = OA.opts_long()
    o.pair_once = 0
    OA.ava(t, q, paf, o)
    rows = [l.split("\t") for l in paf.read_text().splitlines()]
    best = max(rows, key=lambda f: int(f[8]) - int(f[7]))
    assert int(best[8]) - int(best[7]) > 0.99 * len(truth), "the alignment must span the segment for NM to mean anything"
    return int(next(x for x in best[12:] if x.startswith("NM:i:"))[5:])


def test_quality_polished_contig_is_closer_to_the_truth(tmp_path):
    from oracle import ava as OA
    q = PI.quality_case()
    cfa, rfa, paf = tmp_path / "contig.fa", tmp_path / "reads.fa", tmp_path / "rows.paf"
    cfa.write_bytes(b">contig\n" + q["contig"] + b"\n")
    rfa.write_bytes(q["reads_fa"])
    o = OA.opts_long()
    o.pair_once = 0
    OA.ava(cfa, rfa, paf, o)
    out, st = PM.polish(cfa.read_bytes(), q["reads_fa"], paf.read_bytes(), min_len=1000, min_iden=0.9)
    polished = out.split(b"\n")[1]
    before = _nm_against_truth(tmp_path, "before", q["truth"], q["contig"])
    after = _nm_against_truth(tmp_path, "after", q["truth"], polished)
    print(f"quality case: planted {q['planted']}, rows selected {st['rows_selected']}, NM before {before}, after {after}, stats {st}")
    assert st["rows_selected"] >= 100
    assert after < before
