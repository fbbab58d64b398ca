"""CPU: tests/variants_ins_model.py, the contract of hlmi_variants_ins.  The model gives the hand-worked answers of
tests/variants_ins_inputs.py and puts every shape where it claims to be; its sites and the first six summary columns are
tests/variants_model.py's on every case of tests/variants_inputs.py and of its own; and against tests/polish_model.py: at
min_alt 1 and min_frac 0 every slot hlmi_polish opens is listed, and the len / seq listed for a slot with 2 i > s are the bases
the polished contig carries there."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import polish_inputs as PI  # noqa: E402
import polish_model as PM  # noqa: E402
import variants_inputs as VI  # noqa: E402
import variants_ins_inputs as II  # noqa: E402
import variants_ins_model as IM  # noqa: E402
import variants_model as VM  # noqa: E402

HAND = II.hand_cases()
SHAPES = II.shapes()
OLD = {**{"hand_" + k: (v.case, v.opts) for k, v in VI.hand_cases().items()}, **{"shape_" + k: (v.case, v.opts) for k, v in VI.shapes().items()}}
MINE = {**{"hand_" + k: (v.case, v.opts) for k, v in HAND.items()}, **{"shape_" + k: (v.case, v.opts) for k, v in SHAPES.items()}}


def run(c, pairs=None, **opts):
    return IM.variants_ins(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), pairs, **opts)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    h = HAND[name]
    sites, ins, summary, st = run(h.case, **h.opts)
    assert ins == IM.INS_HEAD + b"".join(line + b"\n" for line in h.ins)
    assert summary == IM.SUMMARY_HEAD + b"".join(line + b"\n" for line in h.summary)
    assert sites == VM.SITES_HEAD
    assert st == {**dict.fromkeys(IM.STAT_KEYS, 0), **h.stats}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_sits_where_it_claims(name):
    s = SHAPES[name]
    s.where(*run(s.case, **s.opts))


@pytest.mark.parametrize("name", sorted(OLD) + sorted(MINE))
def test_sites_and_six_columns_are_the_variant_models(name):
    c, opts = (OLD if name in OLD else MINE)[name]
    sites, ins, summary, st = run(c, **opts)
    want = VM.variants(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), **opts)
    assert sites == want[0]
    assert [b"\t".join(line.split(b"\t")[:6]) for line in summary.split(b"\n")] == want[1].split(b"\n")
    assert {k: st[k] for k in VM.STAT_KEYS} == want[2]
    assert IM.STAT_KEYS[:13] == VM.STAT_KEYS and len(IM.STAT_KEYS) == 17


def _opts(c):
    return {k: v for k, v in c.opts.items() if k in ("min_len", "min_iden", "min_cov")}


def polish_cases():
    """the polisher's hand cases and this call's: those both models accept (the variant call refuses a name twice)"""
    out = {"polish_" + k: c for k, c in PI.hand_cases().items()}
    out.update({"ins_" + k: v.case for k, v in HAND.items()})
    ok = {}
    for k, c in out.items():
        try:
            PM.polish(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), **_opts(c))
            IM.variants_ins(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), min_alt=1, min_frac=0.0, **_opts(c))
        except Exception:
            continue
        ok[k] = c
    assert len(ok) >= 30 and any(k.startswith("polish_") for k in ok)
    return ok


POLISH = polish_cases()


@pytest.mark.parametrize("name", sorted(POLISH))
def test_opened_slots_of_the_polisher_are_listed_with_its_bases(name):
    """one contig per case: the polished contig is rebuilt from the model's decisions, slot by slot"""
    c = POLISH[name]
    opts = _opts(c)
    min_cov = opts.get("min_cov", 3)
    contigs, reads, paf = c.contigs_bytes(), c.reads_bytes(), c.paf_bytes()
    _, pst = PM.polish(contigs, reads, paf, **opts)
    _, ins, _, st = IM.variants_ins(contigs, reads, paf, min_alt=1, min_frac=0.0, **opts)
    listed = {(n, p): (s, i, ln, seq) for n, p, s, i, _, ln, _, seq in IM.ins_rows(ins)}
    assert (st["ins_long"], st["ins_edge"]) == (pst["ins_long"], pst["ins_edge"])
    # the polisher's own slot decisions, from its model's pieces
    rdict = dict(PM.parse_seqs(reads))
    rows = PM.select_rows(PM.parse_paf(paf), opts.get("min_len", 0), opts.get("min_iden", 0.0))
    opened = inserted = 0
    for name_, seq in PM.parse_seqs(contigs):
        mine = [r for r in rows if r["t"] == name_]
        for p in range(1, len(seq)):
            span = sum(1 for r in mine if r["ts"] < p < r["te"])
            inserts = [b for r in mine for q, b in PM.row_votes(r, rdict[r["q"]])[1].items() if q == p]
            add = PM.decide_slot(span, inserts, min_cov)
            if add:
                opened += 1
                inserted += len(add)
                s, i, ln, got = listed[(name_, p)]              # listed, and with the bases the polished contig carries
                assert (s, i) == (span, len(inserts)) and 2 * i > s and (ln, got) == (len(add), add)
            elif (name_, p) in listed:
                s, i, _, _ = listed[(name_, p)]
                assert 2 * i <= s                               # a site the polisher leaves shut
    assert (opened, inserted) == (pst["slots_opened"], pst["inserted_bases"])
