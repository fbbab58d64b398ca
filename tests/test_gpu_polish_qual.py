"""GPU: hlmi_polish_q and hlmi_polish_reads_q against their model (tests/polish_qual_model.py) - the file byte for byte and
every integer stat.  The hand cases of tests/test_polish_qual_model.py; piles around the count kernel's tile border (weighted
substitutions and opened slots on T - 1, T, T + 1, a D op across the border); runs of 16, 17 and 70 columns on both strands
with a quality per column; CIGARs of 1 .. 513 ops; insertions of 1, 16 and 17 bases with the lowest quality first and last;
705 and 706 rows of Q93 on one position; the header's identities against api.polish / api.polish_reads; the refusals; the
read floor on both entry points; the driver with --polish_qual.  For the fused call the model runs on the PAF hlmi_ava writes
for the same inputs, as in tests/test_gpu_polish_reads.py."""
import os
import sys

import pytest

from hylight_amd import api, driver, simulate as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_model as PM  # noqa: E402
import polish_qual_inputs as QI  # noqa: E402
import polish_qual_model as QM  # noqa: E402
import polish_reads_inputs as RI  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = QI.hand_cases()
INT_STATS = QM.STAT_KEYS


def check(case, tmp_path, **over):
    """hlmi_polish_q on a case's files == the model"""
    cfa, rfa, paf = case.write(tmp_path)
    opts = {**case.opts, **over}
    want, want_st = QM.polish_q(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes(), **opts)
    out = tmp_path / "polished.fa"
    st = api.polish(cfa, rfa, paf, out, **opts)
    assert {k: st[k] for k in INT_STATS} == want_st
    assert out.read_bytes() == want
    assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "polished.fa", "reads.fa", "rows.paf"]     # no temporary left
    assert st["ms_total"] >= st["ms_device"] >= 0
    return want, st


def differs_from_count_model(case, want):
    plain, _ = PM.polish(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes(),
                         **{k: v for k, v in case.opts.items() if k not in ("qual_weight", "min_avg_qual")})
    return plain != want


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name, tmp_path):
    want, _ = check(HAND[name], tmp_path)
    assert want == HAND[name].want[0]


@pytest.mark.parametrize("kind", ["sub_and_slot", "del_across"])
def test_tile_border(kind, tmp_path):
    case = QI.tile_case(kind)
    T = PI.kernel_constants()["tile"]
    want, st = check(case, tmp_path)
    assert differs_from_count_model(case, want)              # the weights decide somewhere
    ops = [PI.cigar_ops(r.split(b"\t")[-1][5:].decode()) for r in case.rows]
    starts = [int(r.split(b"\t")[7]) for r in case.rows]

    def op_over(code, lo, hi):                               # a row has an op `code` that covers target positions lo .. hi - 1
        for ts, row in zip(starts, ops):
            p = ts
            for n, o in row:
                if o == code and p <= lo and p + n >= hi:
                    return True
                p += n if o != "I" else 0
        return False
    plain, plain_st = PM.polish(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes())
    if kind == "del_across":                                 # by count all three positions go, by weight the one between Q40 flanks
        assert op_over("D", T - 1, T + 1) and st["deleted"] == 1 and plain_st["deleted"] == 3
    else:                                                    # by count three substitutions, by weight none; the slots open either way
        assert all(op_over("X", p, p + 1) for p in (T - 1, T, T + 1)) and st["slots_opened"] == 3
        assert st["substituted"] == 0 and plain_st["substituted"] == 3 and st["inserted_bases"] == 4 and plain_st["inserted_bases"] == 5


def test_runs_of_16_17_and_70_columns(tmp_path):
    case = QI.runs_case()
    want, st = check(case, tmp_path)
    assert differs_from_count_model(case, want) and st["rows_selected"] == 13


@pytest.mark.parametrize("n_ops", [1, 63, 64, 65, 513])
def test_cigar_batches(n_ops, tmp_path):
    case = QI.with_quals(PI.ops_case(n_ops), 700 + n_ops)
    _, st = check(case, tmp_path)
    assert st["rows_selected"] == 5 and st["reads_with_qual"] == 5


def test_insertions_of_1_16_and_17_bases(tmp_path):
    case = QI.insertion_case()
    want, st = check(case, tmp_path)
    assert st["ins_long"] == 1 and st["slots_opened"] == 1 and st["inserted_bases"] == 1
    assert want.split(b"\n")[1] == b"ACGTA" + b"T" + b"CGTACGT"
    plain, _ = PM.polish(case.contigs_bytes(), case.reads_bytes(), case.paf_bytes())
    assert len(plain.split(b"\n")[1]) == 12 + PI.kernel_constants()["cap"]        # by count the 16 bases win


@pytest.mark.parametrize("n_rows", [705, 706])
def test_weight_sums_past_16_bits(n_rows, tmp_path):
    case, seq = QI.deep_case(n_rows)
    want, st = check(case, tmp_path)
    assert n_rows * 93 > 1 << 16 and st["rows_selected"] == n_rows + 1
    assert want.split(b"\n")[1] == seq and st["substituted"] == 1 and st["inserted_bases"] == 2


# ---- the fused call and its chain ------------------------------------------------------------------------------------------
def ava_opts(short):
    o = api.ava_opts_short() if short else api.ava_opts_long()
    o.pair_once = 0
    return o


def chain_and_direct(inp, quals, d, **qopts):
    """hlmi_ava's PAF -> the model; hlmi_polish_q over that PAF and hlmi_polish_reads_q must both give it"""
    os.makedirs(d, exist_ok=True)
    cfa, rfa, paf = (os.path.join(d, n) for n in ("contigs.fa", "reads.fq", "chain.paf"))
    with open(cfa, "wb") as f:
        f.write(RI.fasta(inp.contigs))
    with open(rfa, "wb") as f:
        f.write(QI.fastq(inp.reads, quals))
    api.ava(cfa, rfa, paf, ava_opts(inp.short))
    opts = {**inp.opts, **qopts}
    with open(paf, "rb") as f:
        want, want_st = QM.polish_q(RI.fasta(inp.contigs), QI.fastq(inp.reads, quals), f.read(), **opts)
    got = {}
    for who in ("chain", "direct"):
        out = os.path.join(d, who + ".fa")
        st = api.polish(cfa, rfa, paf, out, **opts) if who == "chain" else api.polish_reads(cfa, rfa, out, ava_opts(inp.short), **opts)
        assert {k: st[k] for k in INT_STATS} == want_st, who
        with open(out, "rb") as f:
            assert f.read() == want, who
        got[who] = st
    assert sorted(os.listdir(d)) == ["chain.fa", "chain.paf", "contigs.fa", "direct.fa", "reads.fq"]
    return want, want_st, (cfa, rfa, paf)


@pytest.mark.parametrize("short", [0, 1])
def test_both_entry_points_equal_the_model(short, tmp_path):
    inp, quals = QI.overlap_input(short, fasta_every=7)
    want, st, (cfa, rfa, paf) = chain_and_direct(inp, quals, str(tmp_path / "w"), qual_weight=1, min_avg_qual=0.0)
    assert st["substituted"] > 0 and st["deleted"] > 0 and st["inserted_bases"] > 0
    assert 0 < st["reads_with_qual"] < len(inp.reads) and st["rows_low_qual"] == 0
    # the weights matter on this input: the count model gives another file for the same rows
    with open(paf, "rb") as f:
        plain, _ = PM.polish(RI.fasta(inp.contigs), QI.fastq(inp.reads, quals), f.read(), **inp.opts)
    assert plain != want


def test_read_floor_on_both_entry_points(tmp_path):
    inp, quals = QI.overlap_input(0, n_low=3)
    low = [n for n, q in quals.items() if q is not None and set(q) == {33 + 4}]
    assert len(low) == 3 and "long" in low and len(dict(inp.reads)["long"]) == max(len(s) for _, s in inp.reads)
    _, off, _ = chain_and_direct(inp, quals, str(tmp_path / "off"), qual_weight=1, min_avg_qual=0.0)
    _, on, _ = chain_and_direct(inp, quals, str(tmp_path / "on"), qual_weight=1, min_avg_qual=10.0)
    assert off["rows_low_qual"] == 0 and on["rows_low_qual"] >= 3
    assert on["rows_selected"] == off["rows_selected"] - 3


# ---- identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["slot_length_and_base_ties", "reverse_strand", "n_and_lower_case", "slots_on_the_tile_border"])
def test_identities_of_hlmi_polish_q(name, tmp_path):
    case = PI.hand_cases()[name]
    cfa, rfa, paf = case.write(tmp_path / "plain")
    st0 = api.polish(cfa, rfa, paf, tmp_path / "plain.fa", **case.opts)
    want = (tmp_path / "plain.fa").read_bytes()
    assert want == case.want[0]
    variants = {"fasta_off": (case, dict(qual_weight=0, min_avg_qual=0.0)), "fasta_on": (case, dict(qual_weight=1)),
                "q1_on": (QI.with_quals(case, 1, choices=(1,)), dict(qual_weight=1, min_avg_qual=0.0)),
                "any_off": (QI.with_quals(case, 2), dict(qual_weight=0, min_avg_qual=0.0))}
    for who, (c, q) in variants.items():
        cfa, rfa, paf = c.write(tmp_path / who)
        st = api.polish(cfa, rfa, paf, tmp_path / (who + ".fa"), **{**case.opts, **q})
        assert (tmp_path / (who + ".fa")).read_bytes() == want, who
        assert {k: st[k] for k in PM.STAT_KEYS} == {k: st0[k] for k in PM.STAT_KEYS}, who
        assert st["reads_with_qual"] == (len(c.reads) if who in ("q1_on", "any_off") else 0) and st["rows_low_qual"] == 0


def test_identities_of_hlmi_polish_reads_q(tmp_path):
    inp, quals = QI.overlap_input(0)
    cfa, rfa = tmp_path / "contigs.fa", tmp_path / "reads.fa"
    cfa.write_bytes(RI.fasta(inp.contigs))
    rfa.write_bytes(RI.fasta(inp.reads))
    st0 = api.polish_reads(cfa, rfa, tmp_path / "plain.fa", ava_opts(0), **inp.opts)
    want = (tmp_path / "plain.fa").read_bytes()
    assert st0["substituted"] > 0 and st0["inserted_bases"] > 0
    q1 = {n: QI.Q(1) * len(s) for n, s in inp.reads}
    files = {"fasta_off": (RI.fasta(inp.reads), dict(qual_weight=0, min_avg_qual=0.0)), "fasta_on": (RI.fasta(inp.reads), dict(qual_weight=1)),
             "q1_on": (QI.fastq(inp.reads, q1), dict(qual_weight=1, min_avg_qual=0.0)),
             "any_off": (QI.fastq(inp.reads, quals), dict(qual_weight=0, min_avg_qual=0.0))}
    for who, (data, q) in files.items():
        rq = tmp_path / (who + ".fq")
        rq.write_bytes(data)
        st = api.polish_reads(cfa, rq, tmp_path / (who + ".fa"), ava_opts(0), **{**inp.opts, **q})
        assert (tmp_path / (who + ".fa")).read_bytes() == want, who
        assert {k: st[k] for k in PM.STAT_KEYS} == {k: st0[k] for k in PM.STAT_KEYS}, who


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["truncated", "byte_32", "min_cov"])
def test_refusals_leave_no_file(what, tmp_path):
    case = HAND["q2_pair_against_q40"]
    cfa, rfa, paf = case.write(tmp_path)
    lines = case.reads_bytes().split(b"\n")
    opts = dict(case.opts)
    if what == "truncated":
        lines[7] = lines[7][:-1]
    elif what == "byte_32":
        lines[7] = lines[7][:3] + b" " + lines[7][4:]
    else:
        opts["min_cov"] = 0
    with open(rfa, "wb") as f:
        f.write(b"\n".join(lines))
    for call in (lambda: api.polish(cfa, rfa, paf, tmp_path / "polished.fa", **opts),
                 lambda: api.polish_reads(cfa, rfa, tmp_path / "polished.fa", None, **opts)):
        with pytest.raises(api.HlmiError) as e:
            call()
        assert e.value.code == -1                                               # HLMI_EINVAL
        assert ("min_cov" if what == "min_cov" else "r1") in str(e.value)
        assert sorted(os.listdir(tmp_path)) == ["contigs.fa", "reads.fa", "rows.paf"]
    with pytest.raises(PM.Refused):
        QM.polish_q(case.contigs_bytes(), b"\n".join(lines), case.paf_bytes(), **opts)


# ---- the driver -------------------------------------------------------------------------------------------------------------
def test_driver_polish_qual(tmp_path):
    reads, _ = S.simulate_reads(seed=83, n_strains=2, genome_len=30000, n_reads=90, mean_len=9000, min_len=7000, max_len=14000)
    lfq = tmp_path / "long.fq"
    S.write_fastq(reads, lfq)
    outs = {}
    for name, flags in (("native", ["--polish_native"]), ("native_q", ["--polish_native", "--polish_qual"]),
                        ("direct_q", ["--polish_direct", "--polish_qual"])):
        out = tmp_path / name
        argv = ["-l", str(lfq), "-o", str(out), "--corrected", "--nsplit", "3", "-t", "4", "--stop_after", "polish"] + flags
        assert driver.main(argv) == 0
        outs[name] = (out / "tmp" / "long_con_polished.fa").read_bytes()
    assert outs["native"].count(b">") >= 1
    assert outs["direct_q"] == outs["native_q"]
    # without --polish_qual the run is what it was; and with it these two sites give the same bytes still, through the weighted
    # kernels: they read s1.fa, which has no qualities, so every weight is 1 and no read is low
    assert outs["native_q"] == outs["native"]
