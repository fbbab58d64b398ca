"""CPU: the model of hlmi_polish_q (tests/polish_qual_model.py) on hand-worked piles whose answers are written out as literals
(tests/polish_qual_inputs.py: hand_cases), the identities with tests/polish_model.py the header states, the quality refusals,
and a simulated pile whose low-quality read tails carry systematic wrong bases."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_model as PM  # noqa: E402
import polish_qual_inputs as QI  # noqa: E402
import polish_qual_model as QM  # noqa: E402

HAND = QI.hand_cases()


def run(case, **over):
    return QM.polish_q(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes(), **{**case.opts, **over})


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    case = HAND[name]
    out, st = run(case)
    assert out == case.want[0]
    assert {k: v for k, v in st.items() if v} == case.want[1]
    if case.plain is not None:                               # what the count model gives for the same rows
        plain, _ = PM.polish(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes())
        assert plain == case.plain


def test_hand_cases_cover_what_they_are_for():
    differ = [n for n, c in HAND.items() if c.plain is not None and c.plain != c.want[0]]
    assert {"q2_pair_against_q40", "tie_own_among", "del_lower_flank", "del_first_and_last_op", "reverse_strand_low_end",
            "slot_length_by_weight", "slot_base_votes_and_all_n"} <= set(differ)
    assert HAND["q2_pair_against_q40"].want[0].split(b"\n")[1] == b"ACGTACGTAC"
    assert HAND["q2_pair_against_q40"].plain.split(b"\n")[1] == b"ACGTGCGTAC"


def _identity_cases():
    cases = dict(PI.hand_cases())
    cases.update(PI.tile_cases())
    cases["ops_65"] = PI.ops_case(65)
    cases["three_contigs"] = PI.three_contigs_case(1)
    return cases


@pytest.mark.parametrize("name", sorted(_identity_cases()))
def test_identities_with_the_count_model(name):
    case = _identity_cases()[name]
    want, want_st = PM.polish(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes(), **case.opts)
    # FASTA reads: weights on or off, every vote weighs 1 and no read can be low
    for qw, floor in ((0, 0.0), (1, 0.0), (1, 10.0)):
        out, st = QM.polish_q(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes(), qual_weight=qw, min_avg_qual=floor, **case.opts)
        assert out == want and {k: st[k] for k in PM.STAT_KEYS} == want_st
        assert st["reads_with_qual"] == 0 and st["rows_low_qual"] == 0
    # FASTQ with every quality '"' (Q1): every weight is 1; and any qualities with the weights off
    q1 = QI.with_quals(case, 1, choices=(1,))
    out, st = QM.polish_q(q1.contigs_bytes(), q1.reads_bytes(), q1.paf_bytes(), **{**case.opts, "qual_weight": 1, "min_avg_qual": 0.0})
    assert out == want and {k: st[k] for k in PM.STAT_KEYS} == want_st and st["reads_with_qual"] == len(case.reads)
    assert b'\n+\n"' in q1.reads_bytes() or not case.reads
    anyq = QI.with_quals(case, 2)
    out, st = QM.polish_q(anyq.contigs_bytes(), anyq.reads_bytes(), anyq.paf_bytes(), **{**case.opts, "qual_weight": 0, "min_avg_qual": 0.0})
    assert out == want and {k: st[k] for k in PM.STAT_KEYS} == want_st


def test_quality_refusals():
    case = HAND["q2_pair_against_q40"]
    reads = case.reads_bytes()
    lines = reads.split(b"\n")
    assert lines[4][:1] == b"@" and len(lines[7]) == 10          # the second record's quality line
    for edit, who in ((lines[:7] + [lines[7][:-1]] + lines[8:], b"r1"),             # a truncated quality string
                      (lines[:7] + [b" " + lines[7][1:]] + lines[8:], b"r1"),       # byte 32
                      (lines[:7] + [lines[7][:-1] + b"\x7f"] + lines[8:], b"r1")):  # byte 127
        with pytest.raises(QM.RefusedRecord) as e:
            QM.polish_q(case.contigs_bytes(), b"\n".join(edit), case.paf_bytes(), **case.opts)
        assert e.value.record == who and e.value.line == 0
    # the refusal does not depend on the two options
    with pytest.raises(QM.RefusedRecord):
        QM.polish_q(case.contigs_bytes(), b"\n".join(lines[:7] + [lines[7][:-1]] + lines[8:]), case.paf_bytes(), qual_weight=0, min_avg_qual=0.0)
    with pytest.raises(PM.Refused):
        run(case, min_cov=0)
    with pytest.raises(PM.Refused):
        run(case, min_avg_qual=-1.0)


def test_parser_keeps_qualities():
    recs = QM.parse_seqs_qual(b"@r1 x\r\nACGT\r\nAC\r\n+r1\r\nIIII\r\n5I\r\n>f\nAC\n@r2\nGG\n+\n@>\n")
    assert recs == [(b"r1", b"ACGTAC", b"IIII5I"), (b"f", b"AC", None), (b"r2", b"GG", b"@>")]
    assert [(n, s) for n, s, _ in recs] == PM.parse_seqs(b"@r1 x\r\nACGT\r\nAC\r\n+r1\r\nIIII\r\n5I\r\n>f\nAC\n@r2\nGG\n+\n@>\n")


def test_low_quality_tails_with_systematic_errors():
    """A contig with planted substitutions; 300-base reads of the truth whose last 150 columns are Q2 and carry, on every third
    position, one wrong base that is the same in every read.  Where tails pile up they outvote the good columns by count;
    by weight they cannot."""
    rng = np.random.default_rng(20260)
    n = 3000
    truth = PI.random_contig(rng, n, lower=0, n_frac=0)
    contig = bytearray(truth)
    planted = rng.choice(np.arange(10, n - 10), size=60, replace=False)
    for p in planted:
        contig[p] = b"ACGT"[(b"ACGT".find(truth[p:p + 1]) + 1 + int(rng.integers(3))) % 4]
    contig = bytes(contig)
    wrong = bytes(b"ACGT"[(b"ACGT".find(truth[p:p + 1]) + 1 + p % 3) % 4] for p in range(n))
    c = QI.QCase([("c", contig)], dict(qual_weight=1, min_avg_qual=0.0))
    for k in range(140):
        a = int(rng.integers(0, n - 300))
        fwd = k % 2 == 0                                     # the tail is the read's 3' end: the row's right end on '+', its left on '-'
        tail = range(a + 150, a + 300) if fwd else range(a, a + 150)
        aligned = bytearray(truth[a:a + 300])
        qual = bytearray(QI.Q(40) * 300)
        for p in tail:
            qual[p - a] = 33 + 2
            if p % 3 == 0:
                aligned[p - a] = wrong[p]
        ops = []
        for j in range(300):
            o = "=" if aligned[j] == contig[a + j] else "X"
            if ops and ops[-1][1] == o:
                ops[-1][0] += 1
            else:
                ops.append([1, o])
        c.addq(a, "".join(f"{m}{o}" for m, o in ops), bytes(aligned), bytes(qual), strand="+" if fwd else "-")
    weighted, st = run(c)
    plain, _ = PM.polish(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes())
    errors = lambda out: sum(x != y for x, y in zip(out.split(b"\n")[1], truth))                 # noqa: E731
    e_in, e_w, e_p = sum(x != y for x, y in zip(contig, truth)), errors(weighted), errors(plain)
    assert len(weighted.split(b"\n")[1]) == len(plain.split(b"\n")[1]) == n and st["reads_with_qual"] == 140
    print(f"positions that differ from the truth: contig {e_in}, count model {e_p}, weighted model {e_w}; "
          f"restored: count model {e_in - e_p}, weighted model {e_in - e_w}")
    assert e_in - e_w > e_in - e_p
