"""Inputs of the tests of hlmi_variants_q and its forms (tests/variants_qual_model.py), built with polish_qual_inputs.QCase: piles
whose reads are FASTQ records, a quality per alignment column.

cases(): the smallest piles at which var_tile_kernel<QF> can go wrong, each with its answer worked by hand from the header's rules
- the site lines (None: judged by `where` alone), the stats that matter, and a function of the model's output.  The tile and the
lane / wave switch are the kernel's (polish_inputs.kernel_constants(), SHORT_RUN below is polish_walk.h's and checked against it).
two_strains(seed): the two-strain statement's input.
"""
import collections
import os
import re

import numpy as np

import polish_inputs as PI
import polish_qual_inputs as QI
import variants_inputs as VI

T = VI.T
REF = VI.REF
Q = QI.Q
other_base = VI.other_base
Spec = collections.namedtuple("Spec", "case opts sites stats where")


def short_run():
    text = open(os.path.join(PI.ROOT, "hylight_amd", "csrc", "polish_walk.h")).read()
    m = re.findall(r"constexpr uint32_t SHORT_RUN = (\d+);", text)
    assert len(m) == 1
    return int(m[0])


SHORT_RUN = short_run()


def qpile(c, ref, pos, votes, ts=0, te=None, strands="+", default=40, lefts=(b"",)):
    """one read over ref[ts:te) per entry (vote, phred) of votes: a base at `pos` (None: the contig's own) whose column has that
    Phred (None: a FASTA record); every other column has `default`"""
    te = len(ref) if te is None else te
    for i, (v, q) in enumerate(votes):
        seg, a = ref[ts:te].upper(), pos - ts
        own = v is None or v.upper() == seg[a:a + 1]
        cigar = "".join(f"{n}{o}" for n, o in ((a, "="), (1, "=" if own else "X"), (te - pos - 1, "=")) if n)
        aligned = seg[:a] + (seg[a:a + 1] if v is None else v) + seg[a + 1:]
        qual = None if q is None else QI._col(len(aligned), default, **{f"c{a}": q})
        c.addq(ts, cigar, aligned, qual, strand=strands[i % len(strands)], left=lefts[i % len(lefts)])
    return c


def _line(pos, ref, v, alt):
    c = sum(v)
    k = b"ACGT*".index(alt)
    return b"c\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%s" % (pos + 1, ref, c, v[0], v[1], v[2], v[3], v[4], alt, v[k],
                                                            b"%.6f" % (v[k] / c))


def cases():
    S = {}
    on = dict(min_base_qual=10, min_avg_qual=0.0)

    def add(name, c, opts, lines, where=None, /, **stats):
        S[name] = Spec(c, {**on, **opts}, lines, stats, where or (lambda sites, summary, st: None))

    # own A on position 4: C at Q10 passes, C at Q9 fails.  Four votes, one C: a site at min_alt 1 (0.25 >= 0.2)
    c = qpile(QI.QCase([("c", REF)]), REF, 4, [(b"C", 10), (b"C", 9), (None, 40), (None, 40), (None, 40)])
    add("at_the_floor_and_one_below", c, dict(min_alt=1), [_line(4, b"A", (3, 1, 0, 0, 0), b"C")], columns_low_qual=1, callable=10, sites=1,
        reads_with_qual=5)
    # both C below the floor: the site is gone, the position still has its three votes
    c = qpile(QI.QCase([("c", REF)]), REF, 4, [(b"C", 5), (b"C", 5), (None, 40), (None, 40), (None, 40)])
    add("site_vanishes", c, {}, [], columns_low_qual=2, callable=10, sites=0)
    # three rows, one column below the floor: two votes are left, the position is not callable
    c = qpile(QI.QCase([("c", REF)]), REF, 4, [(b"C", 5), (None, 40), (None, 40)])
    add("position_leaves_callable", c, {}, [], columns_low_qual=1, callable=9, sites=0)
    # strand '-', flanks of different lengths: column 4 (G, Q2) is read[qe - 1 - 4]; read the other way round it is column 5's Q40
    c = qpile(QI.QCase([("c", REF)]), REF, 4, [(b"G", 2), (b"G", 2), (None, 40)], strands="--+", lefts=(b"GG", b"T", b""))
    add("reverse_strand_asymmetric", c, {}, [], columns_low_qual=2, callable=9, sites=0)

    # D ops: 4= 1D 5= - the flanks are query columns 3 and 4
    for name, low in (("left", 3), ("right", 4)):
        c = QI.QCase([("c", REF)])
        for s in "+-":
            c.addq(0, "4=1D5=", REF[:4] + REF[5:], QI._col(9, 40, **{f"c{low}": 2}), strand=s, left=b"AC")
        qpile(c, REF, 4, [(None, 40)] * 3)
        add(f"deletion_low_flank_{name}", c, {}, [], columns_low_qual=4, callable=10, sites=0)
    # ... and both flanks at the floor: the op passes
    c = QI.QCase([("c", REF)])
    for s in "+-":
        c.addq(0, "4=1D5=", REF[:4] + REF[5:], QI._col(9, 40, c3=10, c4=10), strand=s)
    qpile(c, REF, 4, [(None, 40)] * 3)
    add("deletion_flanks_at_the_floor", c, {}, [_line(4, b"A", (3, 0, 0, 0, 2), b"*")], columns_low_qual=0, sites=1)
    # a D as the row's last op: query column qn - 1 alone flanks it (9= 1D), Q2 in two rows and Q40 in two
    c = QI.QCase([("c", REF)])
    for s, q in (("+", 2), ("-", 2), ("+", 40), ("-", 40)):
        c.addq(0, "9=1D", REF[:9], QI._col(9, 40, c8=q), strand=s)
    qpile(c, REF, 9, [(None, 40)])
    add("deletion_at_the_last_query_column", c, {}, [_line(9, b"C", (0, 1, 0, 0, 2), b"*")], columns_low_qual=4, sites=1)
    # a D as the first op: query column 0 alone (1D 9=)
    c = QI.QCase([("c", REF)])
    for s, q in (("+", 2), ("-", 2), ("+", 40), ("-", 40)):
        c.addq(0, "1D9=", REF[1:], QI._col(9, 40, c0=q), strand=s)
    qpile(c, REF, 0, [(None, 40)])
    add("deletion_at_the_first_query_column", c, {}, [_line(0, b"A", (1, 0, 0, 0, 2), b"*")], columns_low_qual=4, sites=1)

    # D runs of SHORT_RUN and SHORT_RUN + 1 columns (the lane votes the first itself, the wave the second): two rows whose runs
    # fail (a flank at Q2), one whose runs pass, two plain rows: del has one vote of three on all 2 SHORT_RUN + 1 columns
    n1, n2 = SHORT_RUN, SHORT_RUN + 1
    ln = 30 + n1 + n2
    ref = VI._seq(ln, 2)
    cig = f"10={n1}D10={n2}D10="
    aligned = ref[:10] + ref[10 + n1:20 + n1] + ref[20 + n1 + n2:]
    c = QI.QCase([("c", ref)])
    c.addq(0, cig, aligned, QI._col(30, 40, c9=2, c20=2)).addq(0, cig, aligned, QI._col(30, 40, c10=2, c19=2), strand="-")
    c.addq(0, cig, aligned, QI._col(30, 40), strand="-")
    c.addq(0, f"{ln}=", ref, Q(40) * ln).addq(0, f"{ln}=", ref, Q(40) * ln, strand="-")
    dels = list(range(10, 10 + n1)) + list(range(20 + n1, 20 + n1 + n2))
    add("deletion_runs_at_the_lane_wave_switch", c, dict(min_alt=1),
        [_line(p, bytes([ref[p]]), tuple(2 if b"ACGT"[k] == ref[p] else 0 for k in range(4)) + (1,), b"*") for p in dels],
        columns_low_qual=2 * (n1 + n2) + 4, sites=n1 + n2, sites_del=n1 + n2)

    # an X run of SHORT_RUN + 1 columns, its middle column below the floor in both rows that carry it: that position keeps one
    # vote and leaves callable, the other SHORT_RUN are sites
    n = SHORT_RUN + 1
    ref = VI._seq(n + 8, 3)
    alt = bytes(other_base(b)[0] for b in ref[4:4 + n])
    c = QI.QCase([("c", ref)])
    for s in "+-":
        c.addq(4, f"{n}X", alt, QI._col(n, 40, **{f"c{n // 2}": 3}), strand=s, left=b"ACG")
    c.addq(0, f"{n + 8}=", ref, Q(40) * (n + 8))

    def where(sites, summary, st, n=n):
        assert [p for _, p, _ in VI.site_rows(sites)] == [p for p in range(4, 4 + n) if p != 4 + n // 2]
    add("long_run_with_a_failing_column_in_the_middle", c, {}, None, where, columns_low_qual=2, callable=n - 1, sites=n - 1)

    # one X op of 400 columns across the tile's end (the second tile sees it clipped: quality index qc0 + (p - tp0)), positions
    # T - 1, T and T + 1 below the floor in both rows that carry it; a plain row beside them
    ref = VI._seq(2 * T + 1, 4)
    a, b = T - 200, T + 200
    alt = bytes(other_base(x)[0] for x in ref[a:b])
    c = QI.QCase([("c", ref)])
    for k, s in enumerate("+-"):
        c.addq(a, "400X", alt, QI.quals_by_target("400X", a, lambda p: 2 if T - 1 <= p <= T + 1 else 40), strand=s, left=b"AC"[:k + 1])
    c.addq(a, "400=", ref[a:b], Q(40) * 400)

    def where(sites, summary, st, a=a, b=b):
        assert [p for _, p, _ in VI.site_rows(sites)] == [p for p in range(a, b) if not T - 1 <= p <= T + 1]
    add("failing_columns_around_the_tile_border", c, {}, None, where, columns_low_qual=6, callable=397, sites=397)

    # 70 ops (2= 1X 2= 1X ...): the columns of ops 63 (X), 64 (=, its first column) and 65 (X) below the floor - the walk takes 64
    # ops a step.  Two such rows and a plain one at min_cov 2: the three positions keep one vote
    ops = [(2, "=") if k % 2 == 0 else (1, "X") for k in range(70)]
    ln = sum(n for n, _ in ops) + 6
    ref = VI._seq(ln, 6)
    aligned, qual, p, xs, low_at = bytearray(), bytearray(), 3, [], []
    for k, (n, o) in enumerate(ops):
        aligned += other_base(ref[p]) if o == "X" else ref[p:p + n]
        qual += Q(2 if k in (63, 65) else 40) * n
        if k == 64:
            qual[-n] = 33 + 2
        if k in (63, 64, 65):
            low_at.append(p)
        elif o == "X":
            xs.append(p)
        p += n
    cig = "".join(f"{n}{o}" for n, o in ops)
    c = QI.QCase([("c", ref)])
    c.addq(3, cig, bytes(aligned), bytes(qual)).addq(3, cig, bytes(aligned), bytes(qual), strand="-", left=b"T")
    c.addq(0, f"{ln}=", ref, Q(40) * ln)

    def where(sites, summary, st, xs=tuple(xs)):
        assert [p for _, p, _ in VI.site_rows(sites)] == list(xs)
    add("failing_columns_in_ops_63_64_65", c, dict(min_cov=2), None, where, columns_low_qual=6, callable=ln - 6 - 3, sites=len(xs))

    # a FASTA record among FASTQ records: its C votes whatever the floor; the C at Q5 does not
    c = qpile(QI.QCase([("c", REF)]), REF, 4, [(b"C", None), (b"C", 5), (b"C", 40), (None, 40), (None, 40)])
    add("fasta_record_among_fastq", c, dict(min_base_qual=93, min_avg_qual=10.0), None, columns_low_qual=4 * 10, reads_with_qual=4, sites=0,
        callable=0)
    add("fasta_record_among_fastq_floor_10", c, {}, [_line(4, b"A", (2, 2, 0, 0, 0), b"C")], columns_low_qual=1, reads_with_qual=4, sites=1)

    # 300 rows on one position: every second carries another base, and half of each kind lies below the floor
    ref = VI._seq(120, 1)
    c = qpile(QI.QCase([("c", ref)]), ref, 60, [(other_base(ref[60]) if i % 2 == 0 else None, 3 if i % 4 < 2 else 30) for i in range(300)],
              ts=40, te=80, strands="+-")
    v = [0, 0, 0, 0, 0]
    v[b"ACGT".index(ref[60:61])], v[b"ACGT".index(other_base(ref[60]))] = 75, 75
    add("deep_pile_half_below_the_floor", c, {}, [_line(60, ref[60:61], tuple(v), other_base(ref[60]))], columns_low_qual=150, callable=40,
        sites=1, rows_selected=300)

    # the read floor: the one read whose C would make the site is Q4 throughout (its mean 4 < 10): its row is dropped
    c = QI.QCase([("c", REF)])
    qpile(c, REF, 4, [(b"C", 40)])
    c.addq(0, "4=1X5=", REF[:4] + b"C" + REF[5:], Q(4) * 10, name="low")
    qpile(c, REF, 4, [(None, 40)] * 3)
    add("read_floor_drops_the_row_that_made_the_site", c, dict(min_base_qual=0, min_avg_qual=10.0), [], rows_low_qual=1, rows_selected=4,
        columns_low_qual=0, sites=0, callable=10)
    return S


TwoStrains = collections.namedtuple("TwoStrains", "case planted errors")


def two_strains(seed=11, length=600, n_snps=8, depth=10, error_rate=0.04):
    """A contig (strain A) and a sister strain B that differs at n_snps planted positions; depth / 2 whole-length reads of each,
    every base at Q12 - Q40; sequencing errors - another base at Q2 - Q5 - at error_rate per base.  -> TwoStrains(case, the planted
    positions, the (position, base) pairs that errors put into at least one read)"""
    rng = np.random.default_rng(seed)
    a = PI.random_contig(rng, length, lower=0, n_frac=0)
    planted = sorted(int(p) for p in rng.choice(np.arange(5, length - 5), size=n_snps, replace=False))
    b = bytearray(a)
    for p in planted:
        b[p] = other_base(a[p], 1 + int(rng.integers(3)))[0]
    c = QI.QCase([("c", a)])
    errors = set()
    for k in range(depth):
        s = bytearray(a if k % 2 == 0 else b)
        q = bytearray(33 + int(v) for v in rng.choice((12, 20, 30, 40), size=length))
        for p in np.flatnonzero(rng.random(length) < error_rate):
            p = int(p)
            s[p] = other_base(s[p], 1 + int(rng.integers(3)))[0]
            q[p] = 33 + int(rng.integers(2, 6))
            errors.add((p, bytes([s[p]])))
        ops = []
        for p in range(length):
            o = "=" if s[p] == a[p] else "X"
            if ops and ops[-1][1] == o:
                ops[-1][0] += 1
            else:
                ops.append([1, o])
        c.addq(0, "".join(f"{n}{o}" for n, o in ops), bytes(s), bytes(q), strand="+-"[k % 2])
    return TwoStrains(c, planted, errors)
