"""CPU: tests/variants_qual_model.py (the contract of hlmi_variants_q and its forms) held to literal answers worked by hand from the
header's rules - the cases of tests/variants_qual_inputs.py: a column at the floor and one below, a site that vanishes, a position
that leaves callable, strand '-', the D op's flanks, a FASTA record among FASTQ records, the read floor - its three identities with
tests/variants_model.py on every input of tests/variants_inputs.py, the refusals' order, and the two-strain statement: with the
floor the model reports exactly the planted sites, without it also the sequencing errors'."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_model as PM  # noqa: E402
import polish_qual_inputs as QI  # noqa: E402
import polish_qual_model as QM  # noqa: E402
import variants_ins_inputs as II  # noqa: E402
import variants_ins_model as IM  # noqa: E402
import variants_inputs as VI  # noqa: E402
import variants_model as VM  # noqa: E402
import variants_qual_inputs as VQI  # noqa: E402
import variants_qual_model as VQ  # noqa: E402

CASES = VQI.cases()
HAND, SHAPES = VI.hand_cases(), VI.shapes()
OLDER = {**{f"hand_{k}": (v.case, v.opts) for k, v in HAND.items()}, **{f"shape_{k}": (v.case, v.opts) for k, v in SHAPES.items()}}
OFF = dict(min_base_qual=0, min_avg_qual=0.0)


def model(c, pairs=None, **opts):
    return VQ.variants_q(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, **opts)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_case(name):
    s = CASES[name]
    sites, summary, st = model(s.case, **s.opts)
    if s.sites is not None:
        assert sites == VM.SITES_HEAD + b"".join(line + b"\n" for line in s.sites)
    s.where(sites, summary, st)
    assert {k: st[k] for k in s.stats} == s.stats
    assert st["sites"] == st["sites_base"] + st["sites_del"] == len(VI.site_rows(sites))
    # the floors off: the older model's answer on the same bytes, no counter but reads_with_qual
    off = model(s.case, **{**s.opts, **OFF})
    plain = VM.variants(s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes(),
                        **{k: v for k, v in s.opts.items() if k not in OFF})
    assert off[:2] == plain[:2] and {k: off[2][k] for k in VM.STAT_KEYS} == plain[2]
    assert off[2]["columns_low_qual"] == off[2]["rows_low_qual"] == 0


def test_every_case_bites():
    """each case but the passing-flanks one differs from the call without floors: the floor is what the answer hangs on"""
    for name, s in CASES.items():
        on, off = model(s.case, **s.opts), model(s.case, **{**s.opts, **OFF})
        assert (on[0] != off[0] or on[2]["callable"] != off[2]["callable"]) == (name != "deletion_flanks_at_the_floor"), name


def test_row_votes_literals():
    """row_votes_q on one row, written out: 2= 1D 1= 1D 2= 1I 2= over positions 3.., Phred 30 30 5 30 30 12 9 30"""
    read = b"ACGTAGGT"
    r = dict(ts=3, te=12, qs=0, qe=8, rev=False, ops=PM.parse_paf(b"r\t8\t0\t8\t+\tc\t20\t3\t12\t7\t10\t60\tcg:Z:2=1D1=1D2=1I2=\n")[0]["ops"])
    votes, failed = VQ.row_votes_q(r, read, QI.Q(30, 30, 5, 30, 30, 12, 9, 30), 10)
    # columns: 0 A(3) 1 C(4) | D(5): flanks 1, 2 -> 5 fails | 2 G(6) Q5 fails | D(7): flanks 2, 3 -> fails | 3 T(8) 4 A(9) | I: 5 |
    # 6 G(10) Q9 fails, 7 T(11)
    assert votes == [(3, 0), (4, 1), (8, 3), (9, 0), (11, 3)] and failed == [5, 6, 7, 10]
    votes, failed = VQ.row_votes_q(r, read, QI.Q(30, 30, 5, 30, 30, 12, 9, 30), 5)
    assert failed == [] and (5, PM.DEL) in votes and (7, PM.DEL) in votes and len(votes) == 9
    # strand '-': the quality string is the read's, reversed with the bases - the same columns fail
    votes, failed = VQ.row_votes_q(dict(r, rev=True), PI.revcomp(read), QI.Q(30, 30, 5, 30, 30, 12, 9, 30)[::-1], 10)
    assert votes == [(3, 0), (4, 1), (8, 3), (9, 0), (11, 3)] and failed == [5, 6, 7, 10]
    # a FASTA record: nothing fails; an N votes nothing and fails nothing, whatever its quality
    assert VQ.row_votes_q(r, read, None, 93)[1] == []
    votes, failed = VQ.row_votes_q(r, b"NCGTAGGT", QI.Q(0, 30, 30, 30, 30, 30, 30, 30), 10)
    assert failed == [] and (3, 0) not in votes and len(votes) == 8


def test_ins_model_slots_take_no_quality():
    """a failing column still spans: span unchanged, depth drops; out_sites is the _q call's; with the base floor alone out_ins is
    hlmi_variants_ins's"""
    ref = b"ACGTACGTACGT"
    c = QI.QCase([("c", ref)])
    for _ in range(2):
        c.addq(0, "5=1I7=", ref[:5] + b"T" + ref[5:], QI._col(13, 3))          # every column below the floor
    for _ in range(3):
        c.addq(0, "12=", ref, QI._col(12, 40))
    args = (c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    sites, ins, summary, st = VQ.variants_ins_q(*args, min_base_qual=10, min_avg_qual=0.0)
    plain = IM.variants_ins(*args)
    assert ins == plain[1] == IM.INS_HEAD + b"c\t5\tA\t5\t2\t0\t0.400000\t1\t2\tT\n"
    assert st["columns_low_qual"] == 24 and st["slots_callable"] == plain[3]["slots_callable"] == 11 and st["callable"] == 12
    assert sites == VQ.variants_q(*args, min_base_qual=10, min_avg_qual=0.0)[0]
    assert summary.split(b"\n")[1] == b"c\t12\t5\t12\t0\t0.000000\t11\t1\t0.090909"
    # the read floor drops the two inserting rows: three rows span, none inserts
    sites, ins, summary, st = VQ.variants_ins_q(*args, min_base_qual=0, min_avg_qual=10.0)
    assert ins == IM.INS_HEAD and st["rows_low_qual"] == 2 and st["rows_selected"] == 3 and st["ins_sites"] == 0


@pytest.mark.parametrize("name", sorted(OLDER))
def test_identities_on_the_older_inputs(name):
    c, opts = OLDER[name]
    args = (c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    want = VM.variants(*args, **opts)

    def same(got):
        assert got[:2] == want[:2] and {k: got[2][k] for k in VM.STAT_KEYS} == want[2] and got[2]["columns_low_qual"] == 0
        assert got[2]["rows_low_qual"] == 0
    same(VQ.variants_q(*args, **opts, **OFF))                                       # both floors off
    same(VQ.variants_q(*args, **opts, min_base_qual=93, min_avg_qual=90.0))         # a FASTA file at any floors
    q = QI.with_quals(c, 5, choices=(10, 11, 40, 93))                               # a FASTQ whose bytes all pass
    got = VQ.variants_q(q.contigs_bytes(), q.reads_bytes(), q.paf_bytes(), **opts, min_base_qual=10, min_avg_qual=10.0)
    same(got)
    assert got[2]["reads_with_qual"] == len(c.reads)


def test_ins_identities():
    for name, h in sorted(II.hand_cases().items()):
        case, opts = h.case, h.opts
        args = (case.contigs_bytes(), case.reads_bytes(), case.paf_bytes())
        want = IM.variants_ins(*args, **opts)
        got = VQ.variants_ins_q(*args, **opts, **OFF)
        assert got[:3] == want[:3] and {k: got[3][k] for k in IM.STAT_KEYS} == want[3], name


def test_refusals_and_their_order():
    c = CASES["site_vanishes"].case
    args = (c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    for bad in (dict(min_base_qual=-1), dict(min_base_qual=94), dict(min_avg_qual=-0.5), dict(min_avg_qual=float("nan"))):
        with pytest.raises(PM.Refused) as e:
            VQ.variants_q(*args, min_cov=0, **bad)                                  # the floors come in front of min_cov
        assert "min_base_qual" in str(e.value) or "min_avg_qual" in str(e.value)
    with pytest.raises(PM.Refused) as e:
        VQ.variants_q(*args, min_cov=0)
    assert "min_cov" in str(e.value)
    VQ.variants_q(*args, min_base_qual=93, min_avg_qual=0.0)
    # a quality string of another length, a byte outside 33..126: refused as hlmi_polish_q refuses them
    bad = args[1].replace(b"+\n" + QI.Q(40) * 4, b"+\n" + QI.Q(40) * 3, 1)
    with pytest.raises(QM.RefusedRecord):
        VQ.variants_q(args[0], bad, args[2])
    with pytest.raises(QM.RefusedRecord):
        VQ.variants_q(args[0], args[1].replace(QI.Q(40) * 4, b" " + QI.Q(40) * 3, 1), args[2])


def test_read_floor_sits_in_front_of_the_pair_list():
    """a low read's row counts in rows_low_qual, not in rows_not_listed, and claims nothing"""
    import polish_pairs_inputs as XI
    s = CASES["read_floor_drops_the_row_that_made_the_site"]
    lst = b"".join(XI.row(n, b"c") for n, _ in s.case.reads[2:])                     # r0 and `low` are not listed
    _, _, st = model(s.case, pairs=lst, **s.opts)
    assert (st["rows_low_qual"], st["rows_not_listed"], st["rows_selected"], st["pairs_listed"]) == (1, 1, 3, 3)


def test_two_strains_the_floor_leaves_exactly_the_planted_sites():
    t = VQI.two_strains()
    args = (t.case.contigs_bytes(), t.case.reads_bytes(), t.case.paf_bytes())
    plain = [p for _, p, _ in VI.site_rows(VQ.variants_q(*args, **OFF)[0])]
    floor, _, st = VQ.variants_q(*args, min_base_qual=10, min_avg_qual=10.0)
    assert [p for _, p, _ in VI.site_rows(floor)] == t.planted                       # exactly the planted ones
    assert set(t.planted) <= set(plain) and len(plain) > len(t.planted)             # without: planted plus error sites
    assert all(any(p == e for e, _ in t.errors) for p in set(plain) - set(t.planted))
    assert st["rows_low_qual"] == 0 and st["columns_low_qual"] > 0
