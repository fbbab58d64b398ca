"""Inputs of the phasing tests (hlmi_phase against tests/phase_model.py), built with polish_inputs.Case.

hand_cases(): small piles on a 20-base contig with the three files written out by hand from the header's rules - cis, trans, a
chain, a tie, min_link and min_agree one below and exactly at their borders, a third base and a read N, del from a D run, the own
base in the minority, strand '-', a row over two blocks, a row that says nothing, hap ties.
shapes(): piles at the smallest sizes where the phase kernels can go wrong - PHASE_TILE is read from the kernels' header, the
position tile through polish_inputs.kernel_constants(), SHORT_RUN from polish_walk.h.  Each shape comes with `where`, a function
of the model's output that asserts the case sits where it claims to (the test calls it before the library runs).

-> {name: Hand(case, opts, sites lines, links lines, reads lines, non-zero stats)}, {name: Shape(case, opts, where)}"""
import collections
import math
import os
import re

import polish_inputs as PI

T = PI.kernel_constants()["tile"]
Hand = collections.namedtuple("Hand", "case opts sites links reads stats")
Shape = collections.namedtuple("Shape", "case opts where")


def _constant(header, pattern):
    m = re.findall(pattern, open(os.path.join(PI.ROOT, "hylight_amd", "csrc", header)).read())
    assert len(m) == 1, (header, pattern, m)
    return int(m[0])


PHASE_TILE = _constant("phase_internal.h", r"constexpr int PHASE_TILE = (\d+);")
SHORT_RUN = _constant("polish_walk.h", r"constexpr uint32_t SHORT_RUN = (\d+);")
REF = b"ACGT" * 5


def _seq(n, k=0):
    return (b"ACGGTCATTG"[k % 7:] + b"ACGGTCATTG" * (n // 10 + 1))[:n]


def other_base(b, k=1):
    return b"ACGT"[(b"ACGT".index(bytes([b]).upper()) + k) % 4:][:1]


def add_read(c, ref, ts, te, edits=None, strand="+", target=None, name=None):
    """one read over ref[ts:te): edits {position: base (an X where it differs, N included) | b"-" (a D column)}; neighbouring
    columns of one kind are one op"""
    edits = edits or {}
    ops, aligned = [], bytearray()
    for p in range(ts, te):
        e = edits.get(p)
        o = "=" if e is None or e.upper() == ref[p:p + 1].upper() else "D" if e == b"-" else "X"
        if o != "D":
            aligned += ref[p:p + 1] if o == "=" else e
        if ops and ops[-1][1] == o:
            ops[-1][0] += 1
        else:
            ops.append([1, o])
    c.add(ts, "".join(f"{n}{o}" for n, o in ops), bytes(aligned), strand=strand, target=target, name=name)
    return c


def pile(ref, reads, strands="+", contigs=None, target=None, c=None):
    """reads: [{position: edit}] or [(ts, te, {position: edit})], one read each"""
    c = c or PI.Case(contigs or [("c", ref)])
    for i, r in enumerate(reads):
        ts, te, e = (0, len(ref), r) if isinstance(r, dict) else r
        add_read(c, ref, ts, te, e, strand=strands[i % len(strands)], target=target)
    return c


def hand_cases():
    H = {}
    base = dict(contigs=1, contigs_covered=1, positions=20, callable=20)
    # REF: G on positions 2, 6, 10 (T is the other allele everywhere below), C on 5

    def one(name, reads, opts, site_lines, link_lines, read_lines, strands="+", **stats):
        n = len(reads)
        H[name] = Hand(pile(REF, reads, strands), opts, site_lines, link_lines, read_lines, {**base, "rows": n, "rows_selected": n, **stats})

    tt, gg = {2: b"T", 6: b"T"}, {}
    two_sites = [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t3\t3\t3\t0|1"]
    two = dict(sites=2, sites_base=2, links=1, alleles=12, read_records=6)
    cis_reads = [b"r%d\tc\t3\t2\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t2\t2\t0\t0\tA" % i for i in range(3, 6)]
    cis = dict(two, links_phased=1, blocks=1, blocks_multi=1, sites_phased=2, reads_a=3, reads_b=3)
    # three reads carry T on both sites, three the contig's G on both: n11 = 3, n00 = 3
    one("cis", [tt] * 3 + [gg] * 3, {}, two_sites, [b"c\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis"], cis_reads, **cis)
    # three reads carry T on the left site only, three on the right one only: n10 = 3, n01 = 3; bits 0, 1; the left-T reads read
    # alt ^ 0 and own ^ 1: hap B twice
    one("trans", [{2: b"T"}] * 3 + [{6: b"T"}] * 3, {}, [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t3\t3\t3\t1|0"],
        [b"c\t3\t7\t0\t3\t3\t0\t6\t1.000000\ttrans"], cis_reads, **cis)
    # the same on strand '-'
    one("trans_reverse_strand", [{2: b"T"}] * 3 + [{6: b"T"}] * 3, {}, [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t3\t3\t3\t1|0"],
        [b"c\t3\t7\t0\t3\t3\t0\t6\t1.000000\ttrans"], cis_reads, strands="-", **cis)
    # sites 2, 6, 10: T T G against G G T: cis, then trans: bits 0, 0, 1
    one("chain_cis_then_trans", [{2: b"T", 6: b"T"}] * 3 + [{10: b"T"}] * 3, {},
        [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t3\t3\t3\t0|1", b"c\t11\tG\tT\t6\t3\t3\t3\t1|0"],
        [b"c\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis", b"c\t7\t11\t0\t3\t3\t0\t6\t1.000000\ttrans"],
        [b"r%d\tc\t3\t3\t0\t3\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t3\t3\t0\t0\tA" % i for i in range(3, 6)],
        sites=3, sites_base=3, links=2, links_phased=2, blocks=1, blocks_multi=1, sites_phased=3, alleles=18, read_records=6, reads_a=3,
        reads_b=3)
    # one read of every combination: cis == trans == 2 of 4: not phased, two blocks, two lines per read
    one("tie_is_not_phased", [tt, gg, {2: b"T"}, {6: b"T"}], {}, [b"c\t3\tG\tT\t4\t2\t2\t3\t0|1", b"c\t7\tG\tT\t4\t2\t2\t7\t0|1"],
        [b"c\t3\t7\t1\t1\t1\t1\t4\t0.500000\t-"],
        [b"r0\tc\t3\t1\t0\t1\t0\tB", b"r0\tc\t7\t1\t0\t1\t0\tB", b"r1\tc\t3\t1\t1\t0\t0\tA", b"r1\tc\t7\t1\t1\t0\t0\tA",
         b"r2\tc\t3\t1\t0\t1\t0\tB", b"r2\tc\t7\t1\t1\t0\t0\tA", b"r3\tc\t3\t1\t1\t0\t0\tA", b"r3\tc\t7\t1\t0\t1\t0\tB"],
        sites=2, sites_base=2, links=1, blocks=2, alleles=8, read_records=8, reads_a=4, reads_b=4)
    # min_link: six informative rows phase at 6 and not at 7
    one("min_link_at", [tt] * 3 + [gg] * 3, dict(min_link=6), two_sites, [b"c\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis"], cis_reads, **cis)
    split = [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t7\tG\tT\t6\t3\t3\t7\t0|1"]
    split_reads = [b"r%d\tc\t%d\t1\t0\t1\t0\tB" % (i, b) for i in range(3) for b in (3, 7)] + \
                  [b"r%d\tc\t%d\t1\t1\t0\t0\tA" % (i, b) for i in range(3, 6) for b in (3, 7)]
    one("min_link_below", [tt] * 3 + [gg] * 3, dict(min_link=7), split, [b"c\t3\t7\t3\t0\t0\t3\t6\t1.000000\t-"], split_reads,
        **dict(two, blocks=2, read_records=12, reads_a=6, reads_b=6))
    # min_agree: four of five informative rows agree: 4 / 5 phases at 0.8 and not at the next double; r4 reads T then G: a tie
    five = [tt, tt, gg, gg, {2: b"T"}]
    s5 = [b"c\t3\tG\tT\t5\t2\t3\t3\t0|1", b"c\t7\tG\tT\t5\t3\t2\t3\t0|1"]
    one("min_agree_at_four_fifths", five, dict(min_agree=0.8), s5, [b"c\t3\t7\t2\t0\t1\t2\t5\t0.800000\tcis"],
        [b"r0\tc\t3\t2\t0\t2\t0\tB", b"r1\tc\t3\t2\t0\t2\t0\tB", b"r2\tc\t3\t2\t2\t0\t0\tA", b"r3\tc\t3\t2\t2\t0\t0\tA", b"r4\tc\t3\t2\t1\t1\t0\t-"],
        sites=2, sites_base=2, links=1, links_phased=1, blocks=1, blocks_multi=1, sites_phased=2, alleles=10, read_records=5, reads_a=2,
        reads_b=2, reads_tie=1)
    one("min_agree_above_four_fifths", five, dict(min_agree=math.nextafter(0.8, 1.0)), [s5[0], b"c\t7\tG\tT\t5\t3\t2\t7\t0|1"],
        [b"c\t3\t7\t2\t0\t1\t2\t5\t0.800000\t-"],
        [b"r0\tc\t3\t1\t0\t1\t0\tB", b"r0\tc\t7\t1\t0\t1\t0\tB", b"r1\tc\t3\t1\t0\t1\t0\tB", b"r1\tc\t7\t1\t0\t1\t0\tB",
         b"r2\tc\t3\t1\t1\t0\t0\tA", b"r2\tc\t7\t1\t1\t0\t0\tA", b"r3\tc\t3\t1\t1\t0\t0\tA", b"r3\tc\t7\t1\t1\t0\t0\tA",
         b"r4\tc\t3\t1\t0\t1\t0\tB", b"r4\tc\t7\t1\t1\t0\t0\tA"],
        sites=2, sites_base=2, links=1, blocks=2, alleles=10, read_records=10, reads_a=5, reads_b=5)
    # sites 2, 6, 10; r6 reads C (a third base) on 6 and r7 an N there: both leave both links, r7's N votes nothing
    ttt = {2: b"T", 6: b"T", 10: b"T"}
    one("third_base_and_read_n", [ttt] * 3 + [gg] * 3 + [{2: b"T", 6: b"C", 10: b"T"}, {6: b"N"}], {},
        [b"c\t3\tG\tT\t8\t4\t4\t3\t0|1", b"c\t7\tG\tT\t7\t3\t3\t3\t0|1", b"c\t11\tG\tT\t8\t4\t4\t3\t0|1"],
        [b"c\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis", b"c\t7\t11\t3\t0\t0\t3\t6\t1.000000\tcis"],
        [b"r%d\tc\t3\t3\t0\t3\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t3\t3\t0\t0\tA" % i for i in range(3, 6)] +
        [b"r6\tc\t3\t3\t0\t2\t1\tB", b"r7\tc\t3\t3\t2\t0\t0\tA"],
        sites=3, sites_base=3, links=2, links_phased=2, blocks=1, blocks_multi=1, sites_phased=3, alleles=24, read_records=8, reads_a=4,
        reads_b=4)
    # a D run over positions 5 and 6 in three of six reads: two sites with alt del
    dd = {5: b"-", 6: b"-"}
    one("alt_del_from_one_d_run", [dd] * 3 + [gg] * 3, {}, [b"c\t6\tC\t*\t6\t3\t3\t6\t0|1", b"c\t7\tG\t*\t6\t3\t3\t6\t0|1"],
        [b"c\t6\t7\t3\t0\t0\t3\t6\t1.000000\tcis"],
        [b"r%d\tc\t6\t2\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t6\t2\t2\t0\t0\tA" % i for i in range(3, 6)],
        **dict(cis, sites_base=0, sites_del=2))
    # the contig's G is the minority on both sites: four T reads are hap B, the two G reads hap A
    one("own_in_the_minority", [tt] * 4 + [gg] * 2, {}, [b"c\t3\tG\tT\t6\t2\t4\t3\t0|1", b"c\t7\tG\tT\t6\t2\t4\t3\t0|1"],
        [b"c\t3\t7\t2\t0\t0\t4\t6\t1.000000\tcis"],
        [b"r%d\tc\t3\t2\t0\t2\t0\tB" % i for i in range(4)] + [b"r%d\tc\t3\t2\t2\t0\t0\tA" % i for i in range(4, 6)],
        **dict(cis, reads_a=2, reads_b=4))
    # r6 covers [0, 5) with an N on the only site it spans: an allele byte and no line
    one("a_row_with_nothing_to_say", [tt] * 3 + [gg] * 3 + [(0, 5, {2: b"N"})], {}, two_sites, [b"c\t3\t7\t3\t0\t0\t3\t6\t1.000000\tcis"], cis_reads,
        **dict(cis, alleles=13))
    return H


def site_rows(sites):
    """phase sites bytes -> [(contig, 0-based position, alt letter, block id, phase)]"""
    return [(f[0], int(f[1]) - 1, f[3], int(f[7]), f[8]) for f in (line.split(b"\t") for line in sites.split(b"\n")[1:] if line)]


def link_rows(links):
    """-> [(contig, 0-based pos1, 0-based pos2, [n00, n01, n10, n11], phased)]"""
    return [(f[0], int(f[1]) - 1, int(f[2]) - 1, [int(x) for x in f[3:7]], f[9]) for f in (line.split(b"\t") for line in links.split(b"\n")[1:] if line)]


def read_rows(reads):
    """-> [(read, contig, block id, spanned, hap_a, hap_b, other, hap)]"""
    return [(f[0], f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), f[7])
            for f in (line.split(b"\t") for line in reads.split(b"\n")[1:] if line)]


def shapes():
    S = {}

    # sites exactly at a row's ts (10), te - 1 (19) and te (20): r6 over [10, 20) spans the first two; r7 over [40, 60) spans no
    # site, r8 over [25, 35) one
    ref = _seq(60, 2)
    at = (10, 19, 20, 30)
    alt = {p: other_base(ref[p]) for p in at}
    c = pile(ref, [alt] * 3 + [{}] * 3 + [(10, 20, alt), (40, 60, {}), (25, 35, alt)], strands="+-")

    def where(sites, links, reads, st, at=at):
        assert [p for _, p, _, _, _ in site_rows(sites)] == list(at) and st["alleles"] == 6 * 4 + 2 + 0 + 1
        rr = {r[0]: r for r in read_rows(reads)}
        assert rr[b"r6"][3:] == (2, 0, 2, 0, b"B") and b"r7" not in rr and rr[b"r8"][3:] == (1, 0, 1, 0, b"B")
        assert [n for _, _, _, n, _ in link_rows(links)] == [[3, 0, 0, 4], [3, 0, 0, 3], [3, 0, 0, 3]]
    S["sites_at_a_rows_ends"] = Shape(c, {}, where)

    # PHASE_TILE - 1, PHASE_TILE and PHASE_TILE + 1 links (PHASE_TILE .. PHASE_TILE + 2 sites, every second position): the last link
    # of tile 0 has its right site in tile 1; r5 covers the four sites around the border, r6 starts exactly on site PHASE_TILE; r4
    # carries the other base on every fifth site: those sites' links agree 4 : 1, which min_agree 0.9 does not phase - hundreds of
    # blocks under every whole-length row
    for n_sites in (PHASE_TILE, PHASE_TILE + 1, PHASE_TILE + 2):
        ln = 2 * n_sites + 9
        ref = _seq(ln, n_sites)
        at = [4 + 2 * i for i in range(n_sites)]
        alt = {p: other_base(ref[p]) for p in at}
        border = at[PHASE_TILE - 2]
        reads = [alt, alt, {}, {}, {p: alt[p] for p in at[::5]}, (border, min(ln, border + 7), alt)]
        if n_sites > PHASE_TILE:
            reads.append((at[PHASE_TILE], ln, alt))
        c = pile(ref, reads, strands="+-")

        def where(sites, links, reads, st, n_sites=n_sites, at=tuple(at)):
            assert [p for _, p, _, _, _ in site_rows(sites)] == list(at) and st["links"] == n_sites - 1 == len(link_rows(links))
            lr = link_rows(links)
            assert lr[PHASE_TILE - 2][1:4] == (at[PHASE_TILE - 2], at[PHASE_TILE - 1], [3, 0, 0, 3])      # neither is a fifth site
            if n_sites > PHASE_TILE:
                assert lr[PHASE_TILE - 1][1:3] == (at[PHASE_TILE - 1], at[PHASE_TILE]) and lr[PHASE_TILE - 1][3][3] == 3
            if n_sites > PHASE_TILE + 1:
                assert lr[PHASE_TILE][1:3] == (at[PHASE_TILE], at[PHASE_TILE + 1]) and lr[PHASE_TILE][3][3] == 4
            assert st["links_phased"] >= 1 and st["blocks"] >= 2
        S[f"sites_{n_sites}_around_the_link_tile"] = Shape(c, dict(min_agree=0.9), where)
    assert (PHASE_TILE - 2) % 5 and (PHASE_TILE - 1) % 5

    # the last position of contig a and the first of contig b are sites under six reads each: no link joins them, and b's block
    # starts at its position 1
    ra, rb = _seq(30, 1), _seq(30, 4)
    c = PI.Case([("a", ra), ("b", rb)])
    pile(ra, [{20: other_base(ra[20]), 29: other_base(ra[29])}] * 3 + [{}] * 3, c=c, target="a", strands="+-")
    pile(rb, [{0: other_base(rb[0]), 9: other_base(rb[9])}] * 3 + [{}] * 3, c=c, target="b", strands="-+")

    def where(sites, links, reads, st):
        assert [(n, p, b) for n, p, _, b, _ in site_rows(sites)] == [(b"a", 20, 21), (b"a", 29, 21), (b"b", 0, 1), (b"b", 9, 1)]
        assert [(n, p, q) for n, p, q, _, _ in link_rows(links)] == [(b"a", 20, 29), (b"b", 0, 9)]
        assert st["links"] == st["links_phased"] == st["blocks"] == st["blocks_multi"] == 2 and st["read_records"] == 12
    S["sites_on_both_sides_of_a_contig_junction"] = Shape(c, {}, where)

    # three contigs, the middle one without rows
    ra, rm, rz = _seq(700, 0), _seq(300, 1), _seq(T + 500, 2)
    c = PI.Case([("a", ra), ("m", rm), ("z", rz)])
    pile(ra, [(600, 700, {650: b"-", 699: other_base(ra[699])})] * 2 + [(600, 700, {})] * 2, c=c, target="a")
    pile(rz, [(0, 200, {0: other_base(rz[0]), 150: other_base(rz[150])})] * 2 + [(0, 200, {})] * 2, c=c, target="z", strands="-+")
    pile(rz, [(T - 30, T + 500, {T - 1: other_base(rz[T - 1]), T + 499: other_base(rz[T + 499])})] * 2 + [(T - 30, T + 500, {})] * 2, c=c,
         target="z")

    def where(sites, links, reads, st):
        assert [(n, p) for n, p, _, _, _ in site_rows(sites)] == [(b"a", 650), (b"a", 699), (b"z", 0), (b"z", 150), (b"z", T - 1), (b"z", T + 499)]
        assert st["contigs_covered"] == 2 and st["links"] == 4 and st["links_phased"] == 3 and st["blocks"] == 3
        assert link_rows(links)[2][3:] == ([0, 0, 0, 0], b"-")                 # no row spans z's sites 150 and T - 1
    S["middle_contig_without_rows"] = Shape(c, {}, where)

    # CIGARs of 63, 64, 65 and 513 ops: 3= 1X 1I 1X ... - every X a site, every second one behind an I that shifts the query column;
    # two such reads (one per strand) against two plain ones whose single op holds every site
    for n_ops in (63, 64, 65, 513):
        runs = [[(3, "="), (1, "X"), (1, "I"), (1, "X")][i % 4] for i in range(n_ops)]
        ln = sum(n for n, o in runs if o != "I") + 11
        ref = _seq(ln, n_ops)
        aligned, p, xs = bytearray(), 5, []
        for n, o in runs:
            if o == "X":
                xs.append(p)
                aligned += other_base(ref[p], 2)
            elif o == "I":
                aligned += b"T"
            else:
                aligned += ref[p:p + n]
            p += n if o != "I" else 0
        cig = "".join(f"{n}{o}" for n, o in runs)
        c = PI.Case([("c", ref)])
        c.add(5, cig, bytes(aligned)).add(5, cig, bytes(aligned), strand="-").add(0, f"{ln}=", ref).add(0, f"{ln}=", ref, strand="-")

        def where(sites, links, reads, st, xs=tuple(xs)):
            assert [p for _, p, _, _, _ in site_rows(sites)] == list(xs) and st["alleles"] == 4 * len(xs)
            assert all(n == [2, 0, 0, 2] and call == b"cis" for _, _, _, n, call in link_rows(links)) and st["blocks"] == 1
            assert [r[3:] for r in read_rows(reads)] == [(len(xs), len(xs), 0, 0, b"A")] * 2 + [(len(xs), 0, len(xs), 0, b"B")] * 2
        S[f"cigar_of_{n_ops}_ops"] = Shape(c, dict(min_cov=2, min_alt=2, min_frac=0.5), where)

    # one op holding SHORT_RUN and SHORT_RUN + 1 sites (the lane / wave switch): X runs of those lengths in two reads, every column
    # of them a site; the two plain reads' single op holds all of them
    ln = 2 * SHORT_RUN + 40
    ref = _seq(ln, 6)
    a, b = 10, 10 + SHORT_RUN + 5
    xs = list(range(a, a + SHORT_RUN)) + list(range(b, b + SHORT_RUN + 1))
    c = pile(ref, [{p: other_base(ref[p]) for p in xs}] * 2 + [{}] * 2, strands="+-")

    def where(sites, links, reads, st, xs=tuple(xs), c=c, ln=ln, b=b):
        assert [p for _, p, _, _, _ in site_rows(sites)] == list(xs) and st["links_phased"] == len(xs) - 1
        assert c.rows[0].split(b"\t")[-1] == b"cg:Z:10=%dX5=%dX%d=" % (SHORT_RUN, SHORT_RUN + 1, ln - b - SHORT_RUN - 1)
    S["ops_of_short_run_and_one_more_sites"] = Shape(c, dict(min_cov=2, min_alt=2, min_frac=0.5), where)

    # a D run of 40 columns across the position-tile border under two of four reads: 40 sites with alt '*', one block
    ln = 2 * T
    ref = _seq(ln, 2)
    c = PI.Case([("c", ref)])
    for s in "+-":
        c.add(T - 300, "280=40D280=", ref[T - 300:T - 20] + ref[T + 20:T + 300], strand=s)
        c.add(T - 300, "600=", ref[T - 300:T + 300], strand=s)

    def where(sites, links, reads, st):
        assert [(p, a, blk) for _, p, a, blk, _ in site_rows(sites)] == [(p, b"*", T - 19) for p in range(T - 20, T + 20)]
        assert st["sites_del"] == 40 and st["links_phased"] == 39 and st["blocks"] == 1 and st["alleles"] == 160
    S["deletion_across_the_position_tile_border"] = Shape(c, {}, where)

    # 4 097 rows on one link: every third carries the other base on both sites
    ref = _seq(400, 1)
    o55, o60 = other_base(ref[55]), other_base(ref[60])
    c = pile(ref, [(40, 80, {55: o55, 60: o60} if i % 3 == 0 else {}) for i in range(4097)], strands="+-")

    def where(sites, links, reads, st):
        assert link_rows(links) == [(b"c", 55, 60, [2731, 0, 0, 1366], b"cis")] and st["read_records"] == 4097 and st["reads_b"] == 1366
    S["deep_pile_on_one_link"] = Shape(c, {}, where)
    return S
