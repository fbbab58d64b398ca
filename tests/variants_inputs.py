"""Inputs of the variant-site tests (hlmi_variants against tests/variants_model.py), built with polish_inputs.Case.

hand_cases(): small piles on a 10-base contig with the answers written out by hand from the header's rules - ties, the own base
in the minority, N and lower case, every threshold one below and exactly at its border.
shapes(): piles at the smallest sizes where var_tile_kernel can go wrong - the tile is read from the kernel's header as
polish_inputs.kernel_constants() reads it.  Each shape comes with `where`, a function of the model's output that asserts the
case sits where it claims to (the test calls it before the library runs).

-> {name: Hand(case, opts, sites lines, summary lines, non-zero stats)}, {name: Shape(case, opts, where)}"""
import collections
import math

import polish_inputs as PI

T = PI.kernel_constants()["tile"]
REF = b"ACGTACGTAC"
Hand = collections.namedtuple("Hand", "case opts sites summary stats")
Shape = collections.namedtuple("Shape", "case opts where")


def _seq(n, k=0):
    return (b"ACGGTCATTG"[k % 7:] + b"ACGGTCATTG" * (n // 10 + 1))[:n]


def other_base(b, k=1):
    return b"ACGT"[(b"ACGT".index(bytes([b]).upper()) + k) % 4:][:1]


def add_pile(c, ref, pos, votes, target=None, ts=0, te=None, strands="+"):
    """one read over ref[ts:te) per entry of votes: a base (bytes) at `pos`, b"-" for a deleted `pos`, None for the contig's own"""
    te = len(ref) if te is None else te
    for i, v in enumerate(votes):
        seg, a, b = ref[ts:te].upper(), pos - ts, te - pos - 1
        ops = [(a, "="), (1, "D" if v == b"-" else "=" if v is None or v.upper() == seg[a:a + 1] else "X"), (b, "=")]
        aligned = seg[:a] + (b"" if v == b"-" else seg[a:a + 1] if v is None else v) + seg[a + 1:]
        c.add(ts, "".join(f"{n}{o}" for n, o in ops if n), aligned, strand=strands[i % len(strands)], target=target)
    return c


def hand_cases():
    H = {}
    full = dict(rows=5, rows_selected=5, contigs=1, contigs_covered=1, positions=10)

    def one(name, ref, pos, votes, opts, sites, callable_, **stats):
        c = add_pile(PI.Case([("c", ref)]), ref, pos, votes)
        n = len(votes)
        rate = b"%.6f" % (len(sites) / callable_ if callable_ else 0.0)
        H[name] = Hand(c, opts, sites, [b"c\t%d\t%d\t%d\t%d\t%s" % (len(ref), n, callable_, len(sites), rate)],
                       {**full, "rows": n, "rows_selected": n, "callable": callable_, "sites": len(sites), **stats})

    # own G on position 2; two A, two C, one G: A and C tie, A comes first
    one("tie_a_c", REF, 2, [b"A", b"A", b"C", b"C", None], {}, [b"c\t3\tG\t5\t2\t2\t1\t0\t0\tA\t2\t0.400000"], 10, sites_base=1)
    # own A on position 4; two T, two del, one A: T comes before del
    one("tie_t_del", REF, 4, [b"T", b"T", b"-", b"-", None], {}, [b"c\t5\tA\t5\t1\t0\t0\t2\t2\tT\t2\t0.400000"], 10, sites_base=1)
    # del alone against the own base
    one("alt_del", REF, 4, [b"-", b"-", None, None, None], {}, [b"c\t5\tA\t5\t3\t0\t0\t0\t2\t*\t2\t0.400000"], 10, sites_del=1)
    # own A has one vote of five, C four: the alternative is the majority
    one("own_minority", REF, 4, [b"C", b"C", b"C", b"C", None], {}, [b"c\t5\tA\t5\t1\t4\t0\t0\t0\tC\t4\t0.800000"], 10, sites_base=1)
    # own A has no vote at all: three C, two G
    one("own_without_votes", REF, 4, [b"C", b"C", b"C", b"G", b"G"], {}, [b"c\t5\tA\t5\t0\t3\t2\t0\t0\tC\t3\t0.600000"], 10, sites_base=1)
    # own N under five A: ref_other, never a site, not callable
    one("own_n", b"ACGTNCGTAC", 4, [b"A"] * 5, {}, [], 9, ref_other=1)
    # own c (lower case) under three G and two c (lower-case read bases vote): ref prints as C
    one("own_lower_case", b"AcGTACGTAC", 1, [b"G", b"G", b"g", b"c", None], {}, [b"c\t2\tC\t5\t0\t2\t3\t0\t0\tG\t3\t0.600000"], 10,
        sites_base=1)
    # an N of a read votes nothing: position 4 has four votes, and C's two are half of them
    one("read_n_votes_nothing", REF, 4, [b"N", b"C", b"C", None, None], {}, [b"c\t5\tA\t4\t2\t2\t0\t0\t0\tC\t2\t0.500000"], 10, sites_base=1)
    # min_cov: five votes are callable at 5 and not at 6 (no position is: callable 0)
    pile = [b"C", b"C", None, None, None]
    line = [b"c\t5\tA\t5\t3\t2\t0\t0\t0\tC\t2\t0.400000"]
    one("min_cov_at", REF, 4, pile, dict(min_cov=5), line, 10, sites_base=1)
    one("min_cov_below", REF, 4, pile, dict(min_cov=6), [], 0)
    # min_alt: two votes are a site at 2 and none at 3
    one("min_alt_at", REF, 4, pile, dict(min_alt=2), line, 10, sites_base=1)
    one("min_alt_below", REF, 4, pile, dict(min_alt=3), [], 10)
    # min_frac: 2 / 5 = 0.4 is a site at 0.4 and none at the next double; 1 / 5 at 0.2 and the next double (min_alt 1)
    one("min_frac_at_04", REF, 4, pile, dict(min_frac=0.4), line, 10, sites_base=1)
    one("min_frac_above_04", REF, 4, pile, dict(min_frac=math.nextafter(0.4, 1.0)), [], 10)
    one5 = [b"C", None, None, None, None]
    one("min_frac_one_of_five_at_02", REF, 4, one5, dict(min_alt=1, min_frac=0.2), [b"c\t5\tA\t5\t4\t1\t0\t0\t0\tC\t1\t0.200000"], 10,
        sites_base=1)
    one("min_frac_one_of_five_above_02", REF, 4, one5, dict(min_alt=1, min_frac=math.nextafter(0.2, 1.0)), [], 10)
    one("min_frac_zero_and_one", REF, 4, [b"C"] * 5, dict(min_frac=1.0), [b"c\t5\tA\t5\t0\t5\t0\t0\t0\tC\t5\t1.000000"], 10, sites_base=1)
    # no site at all: five reads that agree with the contig
    one("no_site", REF, 4, [None] * 5, {}, [], 10)

    # a contig of no bases in front, one without a row behind: both get a line of zeros in the summary
    c = add_pile(PI.Case([("e", b""), ("c", REF), ("n", b"ACGT")]), REF, 4, pile, target="c")
    H["empty_and_uncovered_contigs"] = Hand(c, {}, line, [b"e\t0\t0\t0\t0\t0.000000", b"c\t10\t5\t10\t1\t0.100000", b"n\t4\t0\t0\t0\t0.000000"],
                                            {**full, "contigs": 3, "positions": 14, "callable": 10, "sites": 1, "sites_base": 1})
    return H


def site_rows(sites):
    """sites bytes -> [(contig, 0-based position, alt letter)]"""
    return [(f[0], int(f[1]) - 1, f[9]) for f in (line.split(b"\t") for line in sites.split(b"\n")[1:] if line)]


def shapes():
    S = {}
    opts3 = dict(min_cov=3, min_alt=2, min_frac=0.2)

    # contigs of 1, T - 1, T, T + 1 and 2 T + 1 bases side by side, each under four whole-length reads, two of which carry another
    # base on position 0 and on the last one: the last position of a contig and the first of the next are both sites
    lens = [("one", 1), ("tm1", T - 1), ("t", T), ("tp1", T + 1), ("t2p1", 2 * T + 1)]
    c = PI.Case([(n, _seq(ln, k)) for k, (n, ln) in enumerate(lens)])
    for n, ln in lens:
        ref = dict(c.contigs)[n.encode()]
        for p in sorted({0, ln - 1}):
            add_pile(c, ref, p, [other_base(ref[p]), other_base(ref[p]), None, None][:4 if p == 0 else 2], target=n, strands="+-")
        if ln > 1:
            add_pile(c, ref, 0, [None, None], target=n)

    def where(sites, summary, st):
        got = site_rows(sites)
        assert got == [(n.encode(), p, other_base(_seq(ln, k)[p])) for k, (n, ln) in enumerate(lens) for p in sorted({0, ln - 1})]
        assert st["contigs_covered"] == 5 and st["callable"] == st["positions"] == 1 + 3 * T + 2 * T + 1
    S["contig_lengths_and_junctions"] = Shape(c, opts3, where)

    # sites at 0, T - 1, T and the last position of a contig of 4 T + 5 bases; rows that start or end exactly on a tile border, one
    # row over three tiles; tile 2 holds none: a tile without a site between two with sites
    ln = 4 * T + 5
    ref = _seq(ln, 3)
    c = PI.Case([("c", ref)])
    for ts, te, at in ((0, T, 0), (0, T, T - 1), (T, 2 * T, T), (3 * T, ln, ln - 1), (T - 7, 3 * T + 9, 3 * T)):
        add_pile(c, ref, at, [other_base(ref[at], 2), other_base(ref[at], 2), None], ts=ts, te=te, strands="-+")

    def where(sites, summary, st, ln=ln):
        assert [p for _, p, _ in site_rows(sites)] == [0, T - 1, T, 3 * T, ln - 1]
        assert st["rows_selected"] == 15 and st["callable"] == ln
    S["tile_borders_and_a_tile_without_a_site"] = Shape(c, opts3, where)

    # runs of 16 and 17 columns (the lane / wave switch) in CIGARs of 63, 64, 65 and 513 ops: k ops as 16= 1X 17= 1X ..., two such
    # reads (one per strand) and one plain read, so every X is a site
    for n_ops in (63, 64, 65, 513):
        runs = [(16 + (i // 2) % 2, "=") if i % 2 == 0 else (1, "X") for i in range(n_ops)]
        ln = sum(n for n, _ in runs) + 11
        ref = _seq(ln, n_ops)
        aligned, p, xs = bytearray(), 5, []
        for n, o in runs:
            if o == "X":
                xs.append(p)
                aligned += other_base(ref[p])
            else:
                aligned += ref[p:p + n]
            p += n
        cig = "".join(f"{n}{o}" for n, o in runs)
        c = PI.Case([("c", ref)])
        c.add(5, cig, bytes(aligned)).add(5, cig, bytes(aligned), strand="-").add(0, f"{ln}=", ref)

        def where(sites, summary, st, xs=tuple(xs), ln=ln):
            assert [p for _, p, _ in site_rows(sites)] == list(xs) and st["callable"] == ln - 11
            assert st["sites_base"] == len(xs) == st["sites"]
        S[f"cigar_of_{n_ops}_ops"] = Shape(c, dict(min_cov=2, min_alt=2, min_frac=0.5), where)

    # a D run of 40 columns across the tile border under two of three reads: 40 sites with alt '*', 20 in each tile
    ln = 2 * T
    ref = _seq(ln, 2)
    c = PI.Case([("c", ref)])
    for s in "+-":
        c.add(T - 300, "280=40D280=", ref[T - 300:T - 20] + ref[T + 20:T + 300], strand=s)
    c.add(T - 300, "600=", ref[T - 300:T + 300])

    def where(sites, summary, st):
        assert site_rows(sites) == [(b"c", p, b"*") for p in range(T - 20, T + 20)] and st["sites_del"] == 40 and st["sites_base"] == 0
    S["deletion_across_the_tile_border"] = Shape(c, opts3, where)

    # every one of the T positions of tile 1 a site: two reads of the next base at every position against one plain read
    ln = 3 * T
    ref = _seq(ln, 5)
    alt = bytes(other_base(b)[0] for b in ref[T:2 * T])
    c = PI.Case([("c", ref)])
    c.add(T, f"{T}X", alt).add(T, f"{T}X", alt, strand="-").add(T, f"{T}=", ref[T:2 * T])

    def where(sites, summary, st):
        assert [p for _, p, _ in site_rows(sites)] == list(range(T, 2 * T)) and st["callable"] == T
    S["a_tile_of_sites"] = Shape(c, opts3, where)

    # three contigs, the middle one without rows: the third's tiles start at a cbase that is no multiple of the tile
    lens3 = [("a", 700), ("m", 300), ("z", T + 500)]
    c = PI.Case([(n, _seq(k_len, k)) for k, (n, k_len) in enumerate(lens3)])
    ra, rz = dict(c.contigs)[b"a"], dict(c.contigs)[b"z"]
    add_pile(c, ra, 699, [b"-", b"-", None], target="a")
    add_pile(c, rz, 0, [other_base(rz[0]), other_base(rz[0]), None], target="z")
    add_pile(c, rz, T + 499, [other_base(rz[T + 499]), other_base(rz[T + 499]), None], target="z", ts=T - 30)

    def where(sites, summary, st):
        assert [(n, p) for n, p, _ in site_rows(sites)] == [(b"a", 699), (b"z", 0), (b"z", T + 499)]
        assert st["contigs_covered"] == 2 and st["contigs"] == 3 and summary.split(b"\n")[2] == b"m\t300\t0\t0\t0\t0.000000"
    S["middle_contig_without_rows"] = Shape(c, opts3, where)

    # 4 097 rows on one position (and its 39 neighbours): 1 366 carry another base
    ref = _seq(400, 1)
    c = PI.Case([("c", ref)])
    add_pile(c, ref, 60, [other_base(ref[60]) if i % 3 == 0 else None for i in range(4097)], ts=40, te=80, strands="+-")

    def where(sites, summary, st, ref=ref):
        assert sites.split(b"\n")[1].split(b"\t")[1:4] == [b"61", bytes([ref[60]]), b"4097"] and st["sites"] == 1 and st["callable"] == 40
        assert sites.split(b"\n")[1].split(b"\t")[10:] == [b"1366", b"0.333415"]
    S["deep_pile_on_one_position"] = Shape(c, opts3, where)
    return S
