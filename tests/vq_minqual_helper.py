"""What tests/test_vq_minqual_model.py and tests/test_gpu_vq_minqual.py share.  TEST INFRASTRUCTURE ONLY.

tests/vq_merge_model.py reads its MIN_QUAL when consensus_pos is called, and the clique, clique-next and branch models reach
consensus_pos through that module alone (vq_clique_model.column -> MM.consensus_pos).  What they captured is not the value but
answers: vq_merge_model._PAIR and vq_clique_model._COL remember a column's answer by its bases and qualities, whatever MIN_QUAL
was.  `model_min_qual` sets the value and forgets those answers on the way in and on the way out, so neither value sees the
other's; the models themselves stay as they are.
"""
import contextlib
import math

import pytest

import vq_clique_model as CM
import vq_merge_model as MM

ATCG = "ATCG"                                    # the chain of SRBuilder.cpp:390-393
# vqc::MARGIN, X_SLOPE, X_FLOOR, MIN_PROB of hylight_amd/csrc/vq_internal.h
MARGIN, X_SLOPE, X_FLOOR, MIN_PROB = 2.0 ** -44, 4.35, 2.0 ** -36, 1e-290


def _forget():
    MM._PAIR.clear()
    CM._COL.clear()


@contextlib.contextmanager
def model_min_qual(value):
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(MM, "MIN_QUAL", value)
        _forget()
        try:
            yield
        finally:
            _forget()


def table_cell(q1, q2, same=False):
    """The build rule of the two-base tables (vq_superread.cpp, build_consensus_tables) restated over the model's consensus_pos
    at the MIN_QUAL in force: all ordered pairs of different bases (same: twice one base) at phreds q1, q2 -> (act, quality
    character); raises AssertionError where the build fails.  act: 0 N, 1 the first base, 2 the second, 3 the one of the two
    that comes first in A, T, C, G, 4 the first of A, T, C, G that is neither."""
    acts, quals, chain = set(), set(), True
    for b1 in "ACGT":
        for b2 in "ACGT":
            if (b1 == b2) != same:
                continue
            b, q = MM.consensus_pos(b1 + b2, chr(33 + q1) + chr(33 + q2))
            other = next(x for x in ATCG if x not in (b1, b2))
            act = 0 if b == "N" else 1 if b == b1 else 2 if b == b2 else 4 if b == other else -1
            assert act >= 0, (b1, q1, b2, q2, b)
            acts.add(act)
            quals.add(q)
            if not same and act != (1 if ATCG.index(b1) < ATCG.index(b2) else 2):
                chain = False
    assert len(quals) == 1, ("the quality byte depends on the bases", q1, q2, quals)
    if len(acts) == 1:
        return acts.pop(), quals.pop()
    assert not same and chain, ("the answer depends on the bases' identity", q1, q2, acts)
    return 3, quals.pop()


def goes_to_host(nuc, qual, min_qual):
    """decide() of vq_clique.hip for a column of three bases and more, with Python's libm in place of the device's: True where
    the column lies inside a margin and is handed to the host.  The device's own pow / log10 differ from these in the last bits,
    which is what the margins are for: a column may fall on the other side only when it lies at a margin's edge."""
    s = dict.fromkeys("ACGT", 0.0)
    for n, q in zip(nuc, qual):
        p = math.pow(10, -(ord(q) - 33) / 10.0)
        if n in s:
            for b in s:
                s[b] += MM._log10(1 - p) if b == n else MM._log10(p / 3.0)
    mx = max(s.values())
    max_prob = math.pow(10.0, mx)
    total = sum(math.pow(10.0, s[b]) for b in ATCG)
    if mx == 0 or total == 0.0 or max_prob < MIN_PROB:
        return True
    p_inc = 1 - max_prob / total
    if not abs((1 - p_inc) - min_qual) > MARGIN:
        return True
    if (1 - p_inc) < min_qual:
        return False
    p93 = math.pow(10.0, -9.3)
    if not abs(p_inc - p93) > MARGIN:
        return True
    if p_inc >= p93:
        x = -10 * math.log10(p_inc)
        return not abs(x - (math.floor(x) + 0.5)) > X_SLOPE * MARGIN / p_inc + X_FLOOR
    return False


def pile_columns(case):
    """The columns of a hand case's one pile-up, every read a member: [(bases, qualities)] in list order per column, reverse
    reads oriented.  Offsets: read k at case['offsets'][k]."""
    cols = []
    reads = [(s, q) if fw else (MM.revcomp(s), q[::-1]) for s, q, fw in case["reads"]]
    order = sorted(range(len(reads)), key=lambda k: case["offsets"][k])
    total = max(case["offsets"][k] + len(reads[k][0]) for k in order)
    for c in range(total):
        nuc = qu = ""
        for k in order:
            i = c - case["offsets"][k]
            if 0 <= i < len(reads[k][0]):
                nuc += reads[k][0][i]
                qu += reads[k][1][i]
        cols.append((nuc, qu))
    return cols
