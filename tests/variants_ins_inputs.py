"""Inputs of the insertion-site tests (hlmi_variants_ins against tests/variants_ins_model.py), built with polish_inputs.Case.

hand_cases(): small piles on a 10-base contig with the answers written out by hand from the header's rules - the spanning
rules, the cap, merged I ops, the ties, strand and case, every threshold one below and exactly at its border.
shapes(): piles at the smallest sizes where the kernels can go wrong - the tile is read from the kernel's header as
polish_inputs.kernel_constants() reads it.  Each shape comes with `where`, a function of the model's output that asserts the
case sits where it claims to (the test calls it before the library runs).
two_strains(): a contig under reads of its own strain and, one in six, of a strain with three bases more.

-> {name: Hand(case, opts, ins lines, summary lines, non-zero stats)}, {name: Shape(case, opts, where)}"""
import collections
import math

import polish_inputs as PI
import polish_pairs_inputs as XI
import variants_inputs as VI
import variants_ins_model as IM

T = PI.kernel_constants()["tile"]
CAP = PI.kernel_constants()["cap"]
REF = b"ACGTACGTAC"
Hand = collections.namedtuple("Hand", "case opts ins summary stats")
Shape = collections.namedtuple("Shape", "case opts where")
Strains = collections.namedtuple("Strains", "case opts slot bases same_strain_list")
_seq = VI._seq


def ins_row(c, ref, at=None, ts=0, te=None, strand="+", target=None, lower=False, sub=None):
    """one read over ref[ts:te) that inserts at[p] in front of position p (ts < p < te for a slot) and carries sub[p] on position p"""
    te = len(ref) if te is None else te
    at, sub = dict(at or {}), dict(sub or {})
    ops, aligned, run = [], bytearray(), 0
    for p in range(ts, te + 1):
        if p in at:
            if run:
                ops.append(f"{run}=")
                run = 0
            ops.append(f"{len(at[p])}I")
            aligned += at[p]
        if p == te:
            break
        if p in sub:
            if run:
                ops.append(f"{run}=")
                run = 0
            ops.append("1X")
            aligned += sub[p]
        else:
            run += 1
            aligned += ref[p:p + 1].upper()
    if run:
        ops.append(f"{run}=")
    aligned = bytes(aligned)
    c.add(ts, "".join(ops), aligned.lower() if lower else aligned, strand=strand, target=target)
    return c


def pile(c, ref, p, inserts, ts=0, te=None, target=None, strands="+"):
    """one read per entry of inserts: the bases it inserts at slot p, None for none"""
    for k, b in enumerate(inserts):
        ins_row(c, ref, {p: b} if b else None, ts, te, strands[k % len(strands)], target)
    return c


def hand_cases():
    H = {}

    def one(name, c, opts, ins, slots, callable_=10, length=10, **stats):
        n = len(c.rows)
        rate = b"%.6f" % (len(ins) / slots if slots else 0.0)
        summary = [b"c\t%d\t%d\t%d\t0\t0.000000\t%d\t%d\t%s" % (length, n, callable_, slots, len(ins), rate)]
        H[name] = Hand(c, opts, ins, summary, dict(rows=n, rows_selected=n, contigs=1, contigs_covered=1, positions=length,
                                                   callable=callable_, slots_callable=slots, ins_sites=len(ins), **stats))

    def case(p, inserts, ref=REF, **kw):
        return pile(PI.Case([("c", ref)]), ref, p, inserts, **kw)

    # slot 4 (in front of the second A; the base in front of it is T): two rows insert GG, two T, one nothing - lengths 1 and 2 tie
    one("length_tie_takes_the_smallest", case(4, [b"GG", b"GG", b"T", b"T", None]), {}, [b"c\t4\tT\t5\t4\t0\t0.800000\t1\t2\tT"], 9)
    # index 0: G and C tie - C comes first; index 1: every row inserts N
    one("base_tie_and_all_n", case(4, [b"GN", b"CN", b"GN", b"CN", None]), {}, [b"c\t4\tT\t5\t4\t0\t0.800000\t2\t4\tCN"], 9)
    # 16 bases insert, 17 are a long row
    s16 = b"ACGTTGCAACGTTGCA"
    one("cap_16_and_17", case(4, [s16, s16, s16 + b"A", s16 + b"C", None]), {},
        [b"c\t4\tT\t5\t2\t2\t0.800000\t16\t2\t" + s16], 9, ins_long=2)
    # long rows alone: a site without a length
    one("long_rows_alone", case(4, [s16 + b"A", s16 + b"A", None, None, None]), {}, [b"c\t4\tT\t5\t0\t2\t0.400000\t0\t0\t*"], 9, ins_long=2)
    # the first and the last slot of the contig
    c = PI.Case([("c", REF)])
    for _ in range(2):
        ins_row(c, REF, {1: b"T", 9: b"GA"})
    ins_row(c, REF)
    one("first_and_last_slot", c, {}, [b"c\t1\tA\t3\t2\t0\t0.666667\t1\t2\tT", b"c\t9\tA\t3\t2\t0\t0.666667\t2\t2\tGA"], 9)
    # I ops at ts and at te belong to no slot: three rows over [2, 8) with two bases in front and one behind
    c = PI.Case([("c", REF)])
    for _ in range(3):
        c.add(2, "2I6=1I", b"TT" + REF[2:8] + b"G")
    one("edge_insertions_are_no_slot", c, {}, [], 5, callable_=6, ins_edge=6)
    # a row that starts exactly on position 4 does not span slot 4: s is 3, not 5
    c = pile(PI.Case([("c", REF)]), REF, 4, [b"G", b"G", None])
    pile(c, REF, 4, [None, None], ts=4)
    one("a_row_starting_at_p_does_not_span", c, {}, [b"c\t4\tT\t3\t2\t0\t0.666667\t1\t2\tG"], 9)
    one("a_row_starting_at_p_does_not_span_min_cov_4", c, dict(min_cov=4), [], 5, callable_=6)      # slots 5..9 have five rows, 1..4 three
    # a row whose column on position 4 is an N votes nothing there and still spans: s = 3 makes min_cov
    c = pile(PI.Case([("c", REF)]), REF, 4, [b"G", b"G"])
    ins_row(c, REF, sub={4: b"N"})
    H["a_column_of_n_spans"] = Hand(c, {}, [b"c\t4\tT\t3\t2\t0\t0.666667\t1\t2\tG"], [b"c\t10\t3\t9\t0\t0.000000\t9\t1\t0.111111"],
                                    dict(rows=3, rows_selected=3, contigs=1, contigs_covered=1, positions=10, callable=9, slots_callable=9,
                                         ins_sites=1))
    # two neighbouring I ops, and I - op of no length - I, are one insertion of two bases
    c = PI.Case([("c", REF)])
    c.add(0, "4=1I1I6=", REF[:4] + b"AG" + REF[4:]).add(0, "4=1I0D1I6=", REF[:4] + b"AG" + REF[4:]).add(0, "10=", REF)
    one("merged_i_ops", c, {}, [b"c\t4\tT\t3\t2\t0\t0.666667\t2\t2\tAG"], 9)
    # strand '-' rows insert the reverse complement of what the read holds; lower-case read bases
    c = PI.Case([("c", REF)])
    ins_row(c, REF, {4: b"AG"}, strand="-").add(0, "4=2I6=", (REF[:4] + b"AG" + REF[4:]).lower(), strand="-")
    ins_row(c, REF, {4: b"ag"}, lower=True).add(0, "10=", REF)
    one("strand_and_lower_case", c, {}, [b"c\t4\tT\t4\t3\t0\t0.750000\t2\t3\tAG"], 9)
    # the contig's own bytes play no part: an N in front of the slot prints as N, one behind it changes nothing (the reads carry N
    # on both columns: no vote, positions 3 and 4 are not callable - and the slot between them is, by its three spanning rows)
    ref_n = b"ACGNNCGTAC"
    one("slot_between_n", case(4, [b"G", b"G", None], ref=ref_n), {}, [b"c\t4\tN\t3\t2\t0\t0.666667\t1\t2\tG"], 9, callable_=8)
    # thresholds: s = 5, i = 2
    two5 = [b"G", b"G", None, None, None]
    line = [b"c\t4\tT\t5\t2\t0\t0.400000\t1\t2\tG"]
    one("min_cov_at", case(4, two5), dict(min_cov=5), line, 9)
    one("min_cov_below", case(4, two5), dict(min_cov=6), [], 0, callable_=0)
    one("min_alt_at", case(4, two5), dict(min_alt=2), line, 9)
    one("min_alt_below", case(4, two5), dict(min_alt=3), [], 9)
    one("min_alt_counts_long_rows", case(4, [b"G", s16 + b"AA", None, None, None]), dict(min_alt=2),
        [b"c\t4\tT\t5\t1\t1\t0.400000\t1\t1\tG"], 9, ins_long=1)
    one("min_frac_just_below_04", case(4, two5), dict(min_frac=math.nextafter(0.4, 0.0)), line, 9)
    one("min_frac_at_04", case(4, two5), dict(min_frac=0.4), line, 9)
    one("min_frac_just_above_04", case(4, two5), dict(min_frac=math.nextafter(0.4, 1.0)), [], 9)
    one5 = [b"G", None, None, None, None]
    one("min_frac_zero", case(4, one5), dict(min_alt=1, min_frac=0.0), [b"c\t4\tT\t5\t1\t0\t0.200000\t1\t1\tG"], 9)
    one("min_frac_one_all_rows", case(4, [b"G"] * 5), dict(min_frac=1.0), [b"c\t4\tT\t5\t5\t0\t1.000000\t1\t5\tG"], 9)
    one("min_frac_one_a_row_short", case(4, [b"G"] * 4 + [None]), dict(min_frac=1.0), [], 9)
    # no insertion anywhere
    one("no_site", case(4, [None] * 5), {}, [], 9)
    return H


def shapes():
    S = {}
    opts3 = dict(min_cov=3, min_alt=2, min_frac=0.2)

    # contigs of 1, T - 1, T, T + 1 and 2 T + 1 bases side by side and one without rows between them (no cbase behind the first is
    # a multiple of the tile), each under four whole-length reads, two of which insert at the first slot, the last slot, around the
    # tile borders - and two bases behind the contig's last position, which is position 0 of the next contig in the device's
    # position space: an edge insertion, no slot
    lens = [("one", 1), ("tm1", T - 1), ("t", T), ("m", 300), ("tp1", T + 1), ("t2p1", 2 * T + 1)]
    c = PI.Case([(n, _seq(ln, k)) for k, (n, ln) in enumerate(lens)])
    want = []
    for n, ln in lens:
        if n == "m":
            continue
        ref = dict(c.contigs)[n.encode()]
        slots = sorted(p for p in {1, T - 1, T, T + 1, 2 * T - 1, 2 * T, ln - 1} if 0 < p < ln)
        for k in range(4):
            at = {p: _seq(1 + p % 3, p) for p in slots} if k < 2 else {}
            if k < 2:
                at[ln] = b"GG"
            ins_row(c, ref, at, strand="+-"[k % 2], target=n)
        want += [(n.encode(), p, 4, 2, 0, 1 + p % 3, 2, _seq(1 + p % 3, p)) for p in slots]

    def where(sites, ins, summary, st, want=want):
        assert IM.ins_rows(ins) == want and sites == IM.VM.SITES_HEAD
        assert st["ins_edge"] == 2 * 5 and st["contigs_covered"] == 5 and st["slots_callable"] == sum(ln - 1 for n, ln in lens if n != "m")
    S["contig_lengths_and_tile_borders"] = Shape(c, opts3, where)

    # tile 0 holds an insertion site and no base site, tile 1 a base site and no insertion site, tile 2 neither, tile 3 an
    # insertion site on its first position (under rows that begin in tile 2), tile 4 (five positions) nothing
    ln = 4 * T + 5
    ref = _seq(ln, 3)
    c = PI.Case([("c", ref)])
    alt = VI.other_base(ref[T + 7])
    for k in range(3):
        ins_row(c, ref, {500: b"ACG"} if k < 2 else None, 0, T, "+-"[k % 2])
        ins_row(c, ref, None, T, 2 * T, "+-"[k % 2], sub={T + 7: alt} if k < 2 else None)
        ins_row(c, ref, None, 2 * T, 3 * T - 5)
        ins_row(c, ref, {3 * T: b"T"} if k < 2 else None, 3 * T - 5, ln, "-+"[k % 2])

    def where(sites, ins, summary, st):
        assert [(p, n) for _, p, _, _, _, n, _, _ in IM.ins_rows(ins)] == [(500, 3), (3 * T, 1)]
        assert [p for _, p, _ in VI.site_rows(sites)] == [T + 7] and st["callable"] == 4 * T + 5
    S["tiles_with_one_kind_of_site"] = Shape(c, opts3, where)

    # CIGARs of 63, 64, 65 and 513 ops: 16= / 17= runs with an X or, on ops 1, 63, 65 and the last odd one, a two-base I between
    # them; two such reads (one per strand) and one plain read
    for n_ops in (63, 64, 65, 513):
        i_ops = {k for k in (1, 63, 65, n_ops - 3 + n_ops % 2) if k < n_ops - 1}
        p, at, sub = 5, {}, {}
        for k in range(n_ops):
            if k % 2 == 0:
                p += 16 + (k // 2) % 2
            elif k in i_ops:
                at[p] = b"CA"
            else:
                sub[p] = None
                p += 1
        ln = p + 6
        ref = _seq(ln, n_ops)
        sub = {q: VI.other_base(ref[q]) for q in sub}
        c = PI.Case([("c", ref)])
        ins_row(c, ref, at, 5, p, "+", sub=sub)
        ins_row(c, ref, at, 5, p, "-", sub=sub)
        ins_row(c, ref)
        assert len(PI.cigar_ops(c.rows[0].split(b"cg:Z:")[1].decode())) == n_ops

        def where(sites, ins, summary, st, at=at, sub=sub):
            assert [(q, n, s) for _, q, _, _, _, n, _, s in IM.ins_rows(ins)] == [(q, 2, b"CA") for q in sorted(at)]
            assert [q for _, q, _ in VI.site_rows(sites)] == sorted(sub)
        S[f"cigar_of_{n_ops}_ops"] = Shape(c, dict(min_cov=2, min_alt=2, min_frac=0.5), where)

    # 4 097 rows insert at one slot, 1 366 one base, 1 366 two and 1 365 three: the lengths one and two tie
    ref = _seq(400, 1)
    c = pile(PI.Case([("c", ref)]), ref, 60, [(b"G", b"GT", b"GTA")[k % 3] for k in range(4097)], ts=40, te=80, strands="+-")

    def where(sites, ins, summary, st):
        assert IM.ins_rows(ins) == [(b"c", 60, 4097, 4097, 0, 1, 1366, b"G")] and st["slots_callable"] == 39
    S["deep_pile_on_one_slot"] = Shape(c, opts3, where)
    return S


def two_strains(genome_len=3000, read_len=1000, step=500, copies=3, slot=1400, bases=b"TGA"):
    """The contig is the major strain; the minor strain carries `bases` in front of position `slot`.  Error-free reads on a grid of
    starts, at every start `copies` of the minor strain and five times as many of the major one: one row in six inserts.  The
    same-strain list names the major strain's reads."""
    ref = _seq(genome_len, 2)
    c = PI.Case([("major_contig", ref)])
    same = b""
    for s in range(0, genome_len - read_len + 1, step):
        for k in range(6 * copies):
            minor = k % 6 == 0
            ins_row(c, ref, {slot: bases} if minor and s < slot < s + read_len else None, s, s + read_len, "-" if k % 2 else "+")
            if not minor:
                same += XI.row(c.reads[-1][0], b"major_contig", 14)
    return Strains(c, dict(min_frac=0.1), slot, bases, same)
