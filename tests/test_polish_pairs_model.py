"""CPU: the pair-list model (tests/polish_pairs_model.py, the contract of hlmi_polish_pairs / hlmi_polish_reads_pairs) held to
answers worked by hand from the header's rules, and the case that states what the list is for: two strains, the minor one's
contig, five reads of the major strain for every read of the minor one."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_pairs_inputs as XI  # noqa: E402
import polish_pairs_model as XM  # noqa: E402
import polish_qual_model as QM  # noqa: E402

HAND = XI.hand_cases()


def run(h, pairs):
    return XM.polish_pairs(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), pairs, **h.case.opts)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    h = HAND[name]
    if h.refused_line:
        with pytest.raises(XM.ListRefused) as e:
            run(h, h.pairs)
        assert e.value.line == h.refused_line
        return
    out, st = run(h, h.pairs)
    assert out == h.want
    assert st == {**dict.fromkeys(XM.STAT_KEYS, 0), **h.stats}


def test_no_list_is_polish_q_and_every_pair_is_the_unlisted_answer():
    h = HAND["every_pair"]
    plain, plain_st = QM.polish_q(h.case.contigs_bytes(), h.case.reads_bytes(), h.case.paf_bytes(), **h.case.opts)
    out, st = run(h, None)
    assert out == plain and st == {**plain_st, "pairs_listed": 0, "pairs_unknown": 0, "rows_not_listed": 0}
    out, st = run(h, h.pairs)
    assert out == plain and {k: st[k] for k in QM.STAT_KEYS} == plain_st
    assert QM.select_rows_q.__module__ == "polish_qual_model"              # the model put the selection back


def test_the_rows_are_refused_before_the_list():
    h = HAND["five_fields_on_line_2"]
    paf = h.case.paf_bytes().replace(b"\tc\t", b"\tnot_a_contig\t", 1)
    with pytest.raises(XM.PM.Refused) as e:
        XM.polish_pairs(h.case.contigs_bytes(), h.case.reads_bytes(), paf, h.pairs, **h.case.opts)
    assert not isinstance(e.value, XM.ListRefused) and e.value.line == 1


def test_two_strains_the_list_keeps_the_minor_contig():
    s = XI.two_strains()
    assert len(s.minor) == 3000 and len(s.snps) >= 20
    # the minor strain covers every SNP at least min_cov times, from the reads' coordinates
    for p in s.snps:
        assert sum(s.per_start for a in s.starts if a <= p < a + 1000) >= s.case.opts["min_cov"] == 3
    args = (s.case.contigs_bytes(), s.case.reads_bytes(), s.case.paf_bytes())
    with_list, st = XM.polish_pairs(*args, s.same_strain_list, **s.case.opts)
    assert with_list.split(b"\n")[1] == s.minor                             # byte-identical to the input contig
    assert st["rows_selected"] == st["pairs_listed"] == 15 and st["rows_not_listed"] == 75 and st["substituted"] == 0
    without, st0 = XM.polish_pairs(*args, None, **s.case.opts)
    got = without.split(b"\n")[1]
    assert len(got) == 3000 and all(got[p] == s.major[p] != s.minor[p] for p in s.snps)     # every SNP carries the major allele
    assert st0["substituted"] == len(s.snps) and st0["rows_selected"] == 90
    assert all(got[p] == s.minor[p] for p in range(3000) if p not in set(s.snps))


def test_two_strains_with_the_oracle_overlappers_rows(tmp_path):
    """the same reads and contig through the overlapper's CPU oracle (oracle/ava_oracle.c, every pair as at the polishing
    sites): rows with real ends and both strains aligned to the minor contig give the model the same two answers - what
    tests/test_gpu_polish_pairs.py then asks of the library on hlmi_ava's rows"""
    from oracle import ava as OA
    s = XI.two_strains()
    cfa, rfa, paf = tmp_path / "contigs.fa", tmp_path / "reads.fa", tmp_path / "oracle.paf"
    cfa.write_bytes(s.case.contigs_bytes())
    rfa.write_bytes(s.case.reads_bytes())
    o = OA.opts_long()
    o.pair_once = 0
    OA.ava(cfa, rfa, paf, o)
    rows = paf.read_bytes()
    aligned = {l.split(b"\t")[0] for l in rows.splitlines()}
    assert aligned == {n for n, _ in s.case.reads}                          # the major strain's reads align to the minor contig too
    args = (s.case.contigs_bytes(), s.case.reads_bytes(), rows)
    with_list, st = XM.polish_pairs(*args, s.same_strain_list, **s.case.opts)
    assert with_list.split(b"\n")[1] == s.minor                             # byte-identical to the input contig
    assert st["rows_selected"] == st["pairs_listed"] == 15 and st["rows_not_listed"] >= 75 and st["substituted"] == 0
    without, st0 = XM.polish_pairs(*args, None, **s.case.opts)
    got = without.split(b"\n")[1]
    assert len(got) == 3000 and st0["deleted"] == st0["inserted_bases"] == 0
    assert all(got[p] == s.major[p] for p in s.snps) and st0["substituted"] == len(s.snps)      # every SNP carries the major allele
