"""Inputs of the tests of hlmi_phase_ins (against tests/phase_ins_model.py), built with polish_inputs.Case and the helpers of
tests/phase_inputs.py and tests/phase_reach_inputs.py.

hand_cases(): piles on phase_inputs.REF with the three files written out by hand from the header's rules - an insertion and a SNP
in cis and in trans (the block's first site an insertion site: id "5+"), a SNP in front of an insertion, a position site and an
insertion site that print the same pos as two blocks "5" and "5+", an insertion site with len_count = min_alt - 1 and one of long
rows alone left out, rows that insert 16 bases (alt), 17 and 2 (other), a noisy insertion site bridged at reach 2.
shapes(): piles at the smallest sizes where phase_span_ins_kernel, phase_fill_ins_kernel and phase_allele_ins_kernel can go wrong
- PHASE_REACH_TILE and SHORT_RUN are read from the kernels' headers.  Each shape comes with the reaches to run it at and
`where`, a function of (reach, the model's output) that asserts the case sits where it claims to.
insertion_strains(): two error-free strains that differ by three insertions alone.

-> {name: Hand(case, opts, reach, sites lines, links lines, reads lines, non-zero stats)}, {name: Shape(case, opts, reaches, where)}"""
import collections

import phase_inputs as HI
import phase_reach_inputs as RI
import polish_inputs as PI

Hand = RI.Hand
Shape = RI.Shape
TILE = RI.TILE
SHORT_RUN = HI.SHORT_RUN
REF = HI.REF
S16 = b"ACGTTGCAACGTTGCA"


def row(c, ref, ts=0, te=None, at=None, edits=None, strand="+", target=None, name=None):
    """one read over ref[ts:te): at {slot p: the bases it inserts in front of position p; p == ts or te: an edge I op}, edits
    {position: base (an X where it differs) | b"-" (a D column)}; neighbouring columns of one kind are one op"""
    te = len(ref) if te is None else te
    at, edits = at or {}, edits or {}
    ops, aligned = [], bytearray()

    def op(n, o):
        if ops and ops[-1][1] == o:
            ops[-1][0] += n
        else:
            ops.append([n, o])
    for p in range(ts, te + 1):
        if p in at:
            op(len(at[p]), "I")
            aligned += at[p]
        if p == te:
            break
        e = edits.get(p)
        o = "=" if e is None or e.upper() == ref[p:p + 1].upper() else "D" if e == b"-" else "X"
        if o != "D":
            aligned += ref[p:p + 1] if o == "=" else e
        op(1, o)
    c.add(ts, "".join(f"{n}{o}" for n, o in ops), bytes(aligned), strand=strand, target=target, name=name)
    return c


def pile(ref, reads, strands="+", c=None, target=None, contigs=None):
    """reads: [(at, edits)] or [(ts, te, at, edits)], one read each"""
    c = c or PI.Case(contigs or [("c", ref)])
    for i, r in enumerate(reads):
        ts, te, at, edits = (0, len(ref)) + tuple(r) if len(r) == 2 else r
        row(c, ref, ts, te, at, edits, strand=strands[i % len(strands)], target=target)
    return c


def site_rows(sites):
    """phase_ins sites bytes -> [(contig, printed pos, alt text, block id (bytes, with its +), phase)]"""
    return [(f[0], int(f[1]), f[3], f[7], f[8]) for f in (line.split(b"\t") for line in sites.split(b"\n")[1:] if line)]


def link_rows(links):
    """-> [(contig, pos1 text, pos2 text, [n00, n01, n10, n11], phased)]"""
    return [(f[0], f[1], f[2], [int(x) for x in f[3:7]], f[9]) for f in (line.split(b"\t") for line in links.split(b"\n")[1:] if line)]


def read_rows(reads):
    """-> [(read, contig, block id text, spanned, hap_a, hap_b, other, hap)]"""
    return [(f[0], f[1], f[2], int(f[3]), int(f[4]), int(f[5]), int(f[6]), f[7])
            for f in (line.split(b"\t") for line in reads.split(b"\n")[1:] if line)]


def hand_cases():
    H = {}
    base = dict(contigs=1, contigs_covered=1, positions=20, callable=20, slots_callable=19)
    # REF: G on positions 2, 6, 10; A on 4 (in front of slot 5), C on 5 (in front of slot 6); T is the other base everywhere

    def one(name, reads, reach, site_lines, link_lines, read_lines, opts=None, **stats):
        n = len(reads)
        H[name] = Hand(pile(REF, reads), opts or {}, reach, site_lines, link_lines, read_lines, {**base, "rows": n, "rows_selected": n, **stats})

    tt, t10, none = {5: b"TT"}, {10: b"T"}, {}
    ins5 = b"c\t5\tA\t+TT\t6\t3\t3\t5+\t0|1"
    both = dict(sites=1, sites_base=1, links=1, links_phased=1, blocks=1, blocks_multi=1, sites_phased=2, alleles=12, read_records=6, reads_a=3,
                reads_b=3, ins_sites=1, ins_sites_phasing=1, ins_sites_phased=1)
    hap_reads = [b"r%d\tc\t5+\t2\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t5+\t2\t2\t0\t0\tA" % i for i in range(3, 6)]
    # three reads insert TT at slot 5 and carry T on 10, three read the contig: n11 = 3, n00 = 3; the block starts at the slot
    one("insertion_and_snp_cis", [(tt, t10)] * 3 + [(none, none)] * 3, 1, [ins5, b"c\t11\tG\tT\t6\t3\t3\t5+\t0|1"],
        [b"c\t5+\t11\t3\t0\t0\t3\t6\t1.000000\tcis"], hap_reads, **both)
    # three reads insert, the three others carry the T: n10 = 3, n01 = 3; bits 0, 1
    one("insertion_and_snp_trans", [(tt, none)] * 3 + [(none, t10)] * 3, 1, [ins5, b"c\t11\tG\tT\t6\t3\t3\t5+\t1|0"],
        [b"c\t5+\t11\t0\t3\t3\t0\t6\t1.000000\ttrans"], hap_reads, **both)
    # the SNP on 2 in front of the insertion at slot 5: the block's id is the SNP's, the link's right end carries the +
    one("snp_in_front_of_an_insertion", [(tt, {2: b"T"})] * 3 + [(none, none)] * 3, 1, [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t5\tA\t+TT\t6\t3\t3\t3\t0|1"],
        [b"c\t3\t5+\t3\t0\t0\t3\t6\t1.000000\tcis"], [r.replace(b"5+", b"3") for r in hap_reads], **both)
    # position 4 (printed 5) and slot 5 (printed 5): the position site first; one read of every combination, the link is a tie:
    # two blocks, 5 and 5+
    one("a_position_and_a_slot_that_print_the_same_pos", [(tt, {4: b"C"}), (none, {4: b"C"}), (tt, none), (none, none)], 1,
        [b"c\t5\tA\tC\t4\t2\t2\t5\t0|1", b"c\t5\tA\t+TT\t4\t2\t2\t5+\t0|1"], [b"c\t5\t5+\t1\t1\t1\t1\t4\t0.500000\t-"],
        [b"r0\tc\t5\t1\t0\t1\t0\tB", b"r0\tc\t5+\t1\t0\t1\t0\tB", b"r1\tc\t5\t1\t0\t1\t0\tB", b"r1\tc\t5+\t1\t1\t0\t0\tA",
         b"r2\tc\t5\t1\t1\t0\t0\tA", b"r2\tc\t5+\t1\t0\t1\t0\tB", b"r3\tc\t5\t1\t1\t0\t0\tA", b"r3\tc\t5+\t1\t1\t0\t0\tA"],
        sites=1, sites_base=1, links=1, blocks=2, alleles=8, read_records=8, reads_a=4, reads_b=4, ins_sites=1, ins_sites_phasing=1)
    # slot 5: one row inserts T, one GG - an insertion site (i = 2) whose called length 1 has one row: min_alt - 1; slot 12: two
    # rows of 17 bases - a site without a length.  Both are left out; the SNPs on 2 and 10 phase as hlmi_phase_reach's
    snps = {2: b"T", 10: b"T"}
    one("insertion_sites_left_out", [({5: b"T", 12: S16 + b"A"}, snps), ({5: b"GG", 12: S16 + b"C"}, snps), (none, snps)] + [(none, none)] * 3, 1,
        [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t11\tG\tT\t6\t3\t3\t3\t0|1"], [b"c\t3\t11\t3\t0\t0\t3\t6\t1.000000\tcis"],
        [r.replace(b"5+", b"3") for r in hap_reads],
        sites=2, sites_base=2, links=1, links_phased=1, blocks=1, blocks_multi=1, sites_phased=2, alleles=12, read_records=6, reads_a=3, reads_b=3,
        ins_sites=2, ins_long=2, ins_sites_left_out=2)
    # slot 5: r0 - r2 insert 16 bases (the called length: alt), r3 inserts 17 (a long row: other), r4 two (other), r5 - r7 nothing
    one("sixteen_is_alt_seventeen_and_two_are_other",
        [({5: S16}, t10)] * 3 + [({5: S16 + b"A"}, none), ({5: b"GT"}, none)] + [(none, none)] * 3, 1,
        [b"c\t5\tA\t+" + S16 + b"\t8\t3\t3\t5+\t0|1", b"c\t11\tG\tT\t8\t5\t3\t5+\t0|1"], [b"c\t5+\t11\t3\t0\t0\t3\t6\t1.000000\tcis"],
        [b"r%d\tc\t5+\t2\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t5+\t2\t1\t0\t1\tA" % i for i in (3, 4)] +
        [b"r%d\tc\t5+\t2\t2\t0\t0\tA" % i for i in range(5, 8)],
        **dict(both, alleles=16, read_records=8, reads_a=5, ins_long=1))
    # phase_reach_inputs's noisy site as a slot: r0 - r2 carry T on 2 and 10, r3 - r5 the contig; r0 and r3 insert T at slot 6.
    # Both links of the slot are ties, the link (3, 11) is cis 6 of 6: the insertion site is bridged
    noisy = [({6: b"T"}, snps), (none, snps), (none, snps), ({6: b"T"}, none), (none, none), (none, none)]
    one("noisy_insertion_site_bridged_at_reach_2", noisy, 2,
        [b"c\t3\tG\tT\t6\t3\t3\t3\t0|1", b"c\t6\tC\t+T\t6\t4\t2\t3\t.", b"c\t11\tG\tT\t6\t3\t3\t3\t0|1"],
        [b"c\t3\t6+\t2\t1\t2\t1\t6\t0.500000\t-", b"c\t3\t11\t3\t0\t0\t3\t6\t1.000000\tcis", b"c\t6+\t11\t2\t2\t1\t1\t6\t0.500000\t-"],
        [b"r%d\tc\t3\t3\t0\t2\t0\tB" % i for i in range(3)] + [b"r%d\tc\t3\t3\t2\t0\t0\tA" % i for i in range(3, 6)],
        sites=2, sites_base=2, links=2, blocks=1, blocks_multi=1, sites_phased=2, alleles=18, read_records=6, reads_a=3, reads_b=3, links_far=1,
        links_far_phased=1, joins_far=1, sites_bridged=1, ins_sites=1, ins_sites_phasing=1)
    return H


def shapes():
    Sh = {}
    two = dict(min_cov=2, min_alt=2, min_frac=0.2)

    # An I op as op 63, 64 and 65 of a CIGAR (0-based: the last op of walk_row's first step, the first and the second of the
    # next): every third position is an X (2= 1X 2= 1X ...), the I sits on the op border behind 63, 64 and 65 ops.  Per I a
    # read on either strand; all six carry every X; two plain reads
    ln = 330
    ref = HI._seq(ln, 4)
    xs = {p: HI.other_base(ref[p]) for p in range(7, ln - 5, 3)}          # ops from ts = 5: 2= (5, 6), 1X (7), ...
    slots = {m: 5 + 3 * (m // 2) + (2 if m % 2 else 0) for m in (63, 64, 65)}
    c = PI.Case([("c", ref)])
    for m, p in sorted(slots.items()):
        for s in "+-":
            row(c, ref, 5, ln - 3, {p: b"CA"}, xs, strand=s)
        assert PI.cigar_ops(c.rows[-1].split(b"cg:Z:")[1].decode())[m] == (2, "I"), (m, p)
    row(c, ref)
    row(c, ref, strand="-")

    def where(reach, sites, links, reads, st, slots=tuple(sorted(slots.values())), n_x=len(xs)):
        sr = site_rows(sites)
        assert [p for _, p, a, _, _ in sr if a.startswith(b"+")] == list(slots) and st["ins_sites_phasing"] == 3 and st["sites"] == n_x
        assert st["alleles"] == 8 * (n_x + 3)
        # a slot's link to the X behind it: the two inserting rows read 1 1, the four other X rows 0 1, the plain rows 0 0; the
        # second slot's right neighbour is the third slot, where no row inserts at both
        lr = {a: cnt for _, a, _, cnt, _ in link_rows(links)}
        assert [lr[b"%d+" % p] for p in slots] == [[2, 4, 0, 2], [4, 2, 2, 0], [2, 4, 0, 2]]
    Sh["i_op_as_op_63_64_65"] = Shape(c, dict(min_cov=3, min_alt=2, min_frac=0.2), (1,), where)

    # slots 10, 11, 29 and 30 are insertion sites under the whole-length rows r0 - r3 (r0, r1 insert).  r4, r5 over [10, 30):
    # their I ops at 10 (ts) and 30 (te) are edge ops and write nothing - the slots' keys lie outside their range - while 11
    # (ts + 1) and 29 (te - 1) are the first and the last site of it.  r6 over [10, 12) holds the single slot 11; r7 over
    # [28, 31) the slots 29 and 30 and no position site
    ref = HI._seq(60, 2)
    at = {10: b"G", 11: b"TT", 29: b"ACG", 30: b"C"}
    c = pile(ref, [(at, {})] * 2 + [({}, {})] * 2 + [(10, 30, at, {})] * 2 + [(10, 12, {}, {}), (28, 31, {29: b"ACG", 30: b"CC"}, {})], strands="+-")

    def where(reach, sites, links, reads, st):
        assert [(p, a) for _, p, a, _, _ in site_rows(sites)] == [(10, b"+G"), (11, b"+TT"), (29, b"+ACG"), (30, b"+C")] and st["sites"] == 0
        assert st["ins_edge"] == 4 and st["alleles"] == 4 * 4 + 2 * 2 + 1 + 2
        rr = {r[0]: r for r in read_rows(reads)}
        assert rr[b"r4"][3:] == (2, 0, 2, 0, b"B") and rr[b"r6"][3:] == (1, 1, 0, 0, b"A") and rr[b"r7"][3:] == (2, 0, 1, 1, b"B")
        assert st["blocks"] == 1 and st["ins_sites_phased"] == 4
    Sh["slots_at_a_rows_ends_and_rows_of_slots_only"] = Shape(c, two, (1, 2), where)

    # SHORT_RUN and SHORT_RUN + 1 sites of both kinds inside one = op: position sites on q + 4 i and insertion sites at the
    # slots q + 4 i + 2; r4's single = op holds exactly SHORT_RUN of them (a lane's own run), r5's SHORT_RUN + 1 and the whole
    # reads' every one (the wave's)
    n = SHORT_RUN + 6
    q = 12
    ref = HI._seq(q + 2 * n + 20, 6)
    pos = [q + 4 * i for i in range((n + 1) // 2)]
    slt = [p + 2 for p in pos][:n // 2]
    alt = ({p: b"GA" for p in slt}, {p: HI.other_base(ref[p]) for p in pos})
    keys = sorted([2 * p + 1 for p in pos] + [2 * p for p in slt])
    c = pile(ref, [alt] * 2 + [({}, {})] * 2 + [(q, keys[SHORT_RUN - 1] // 2 + 1, {}, {}), (q, keys[SHORT_RUN] // 2 + 1, {}, {})], strands="+-")

    def where(reach, sites, links, reads, st, n=n):
        assert len(site_rows(sites)) == n and st["ins_sites_phasing"] == n // 2 and st["blocks"] == 1
        rr = {r[0]: r for r in read_rows(reads)}
        assert rr[b"r4"][3:] == (SHORT_RUN, SHORT_RUN, 0, 0, b"A") and rr[b"r5"][3:] == (SHORT_RUN + 1, SHORT_RUN + 1, 0, 0, b"A")
        assert c.rows[4].split(b"\t")[-1].endswith(b"=") and c.rows[4].count(b"=") == 1
    Sh["an_op_over_short_run_and_one_more_mixed_sites"] = Shape(c, two, (1,), where)

    # TILE + 9 sites, position sites and insertion sites in turn: the left sites TILE - 1 (tile 0, its partner in tile 1), TILE
    # and TILE + 1 are of both kinds.  r0, r1 carry every alt, r2, r3 the contig; r4 spans six sites around the border, r5
    # starts on site TILE, r6 ends on site TILE + 4
    n = TILE + 9
    ln = 2 * n + 12
    ref = HI._seq(ln, 3)
    kind = [i % 2 for i in range(n)]                                        # 1: a slot
    where_at = [4 + 2 * i for i in range(n)]                                # position p, or slot p
    alt = ({p: b"T" for p, k in zip(where_at, kind) if k}, {p: HI.other_base(ref[p]) for p, k in zip(where_at, kind) if not k})
    c = pile(ref, [alt] * 2 + [({}, {})] * 2 + [(where_at[TILE - 3], where_at[TILE + 2] + 1) + alt, (where_at[TILE], ln, {}, {}),
                                               (where_at[TILE - 40], where_at[TILE + 4] + 1, {}, {})], strands="+-")

    def where(reach, sites, links, reads, st, n=n, where_at=tuple(where_at), kind=tuple(kind)):
        sr = site_rows(sites)
        assert [(r[1], r[2].startswith(b"+")) for r in sr] == [(p if k else p + 1, bool(k)) for p, k in zip(where_at, kind)]
        assert len(sr) == n and st["links"] == n - 1 and st["links_far"] == sum(n - d for d in range(2, reach + 1)) and st["blocks"] == 1
        lr = {(a, b): cnt for _, a, b, cnt, _ in link_rows(links)}
        lab = [b"%d+" % p if k else b"%d" % (p + 1) for p, k in zip(where_at, kind)]
        for left in (TILE - 2, TILE - 1, TILE, TILE + 1):
            for d in range(1, reach + 1):
                cnt = lr[(lab[left], lab[left + d])]
                assert cnt[1] == cnt[2] == 0 and cnt[0] >= 2 and cnt[3] >= 2 and sum(cnt) >= 5, (left, d, cnt)
    Sh["mixed_kinds_around_the_reach_tile"] = Shape(c, two, (1, 2), where)

    # contigs a, m (no rows) and b: a's last slot (29) and last position are sites, and so are b's position 0 and its first slot
    # (p = 1, the slot behind the junction's first position): no link joins the contigs, b's block starts at its position 1
    ra, rm, rb = HI._seq(30, 1), HI._seq(40, 3), HI._seq(30, 4)
    c = PI.Case([("a", ra), ("m", rm), ("b", rb)])
    pile(ra, [({29: b"GG"}, {29: HI.other_base(ra[29])})] * 3 + [({}, {})] * 3, c=c, target="a", strands="+-")
    pile(rb, [({1: b"T"}, {0: HI.other_base(rb[0])})] * 3 + [({}, {})] * 3, c=c, target="b", strands="-+")

    def where(reach, sites, links, reads, st):
        assert [(n, p, a[:1], b) for n, p, a, b, _ in site_rows(sites)] == [(b"a", 29, b"+", b"29+"), (b"a", 30, HI.other_base(ra[29]), b"29+"),
                                                                           (b"b", 1, HI.other_base(rb[0]), b"1"), (b"b", 1, b"+", b"1")]
        assert [(n, x, y) for n, x, y, _, _ in link_rows(links)] == [(b"a", b"29+", b"30"), (b"b", b"1", b"1+")]
        assert st["contigs_covered"] == 2 and st["links"] == st["blocks"] == 2 and st["links_far"] == 0 and st["read_records"] == 12
    Sh["a_slot_behind_a_contig_junction"] = Shape(c, {}, (1, 3), where)

    # 4 097 rows on the link between slot 55 and position 60: every third row inserts and carries the other base
    ref = HI._seq(400, 1)
    o60 = HI.other_base(ref[60])
    c = pile(ref, [(40, 80, {55: b"TGA"}, {60: o60}) if i % 3 == 0 else (40, 80, {}, {}) for i in range(4097)], strands="+-")

    def where(reach, sites, links, reads, st):
        assert link_rows(links) == [(b"c", b"55+", b"61", [2731, 0, 0, 1366], b"cis")] and st["read_records"] == 4097 and st["reads_b"] == 1366
    Sh["deep_pile_on_a_link_between_a_slot_and_a_position"] = Shape(c, {}, (1,), where)
    return Sh


Strains = collections.namedtuple("Strains", "case opts slots minor")


def insertion_strains(genome_len=1500, read_len=1000, step=500, copies=4, slots=((300, b"G"), (600, b"TGA"), (900, S16))):
    """The contig is the major strain; the minor strain carries 1, 3 and 16 bases more in front of the positions of `slots` and
    differs nowhere else.  Error-free reads on a grid of starts, `copies` of either strain at every start (eight reads a strain),
    named min_* and maj_*."""
    ref = HI._seq(genome_len, 2)
    c = PI.Case([("major_contig", ref)])
    for s in range(0, genome_len - read_len + 1, step):
        for k in range(2 * copies):
            minor = k % 2 == 0
            row(c, ref, s, s + read_len, {p: b for p, b in slots if s < p < s + read_len} if minor else {}, {},
                strand="-" if k % 4 >= 2 else "+", name=f"{'min' if minor else 'maj'}_{s}_{k}")
    return Strains(c, {}, tuple(p for p, _ in slots), b"min_")
