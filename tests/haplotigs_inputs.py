"""Inputs of the haplotig tests (hlmi_haplotigs against tests/haplotigs_model.py), built with polish_inputs.Case.

hand_cases(): small piles whose two files are written out by hand from the header's rules - two strains with substitutions,
insertions and a deletion; no split block; min_side one above the smaller side; a tied row; the extent's edges for positions and
for slots; a side below min_cov.
shapes(): piles at the smallest sizes where the kernels of haplotigs.hip can go wrong - HAP_TILE is read from the kernels' header,
SHORT_RUN from polish_walk.h.  Each shape comes with `where`, a function of the model's output that asserts the case sits where it
claims to (the test calls it before the library runs).

-> {name: Hand(case, opts, fasta, blocks lines, non-zero own stats)}, {name: Shape(case, opts, where)}"""
import collections

import haplotigs_model as GM
import phase_inputs as HI
import polish_inputs as PI

HAP_TILE = HI._constant("haplotigs_internal.h", r"constexpr int HAP_TILE = (\d+);")
SHORT_RUN = HI.SHORT_RUN
T = HAP_TILE
REF = HI.REF
Hand = collections.namedtuple("Hand", "case opts fasta blocks stats")
Shape = collections.namedtuple("Shape", "case opts where")
other_base = HI.other_base
_seq = HI._seq


def add_read(c, ref, ts, te, edits=None, ins=None, strand="+", target=None):
    """one read over ref[ts:te): edits as phase_inputs.add_read takes them, ins {position: bases inserted in front of it}"""
    edits, ins = edits or {}, ins or {}
    ops, aligned = [], bytearray()

    def push(n, o):
        if ops and ops[-1][1] == o:
            ops[-1][0] += n
        else:
            ops.append([n, o])
    for p in range(ts, te):
        if p in ins and p > ts:
            aligned += ins[p]
            push(len(ins[p]), "I")
        e = edits.get(p)
        o = "=" if e is None or e.upper() == ref[p:p + 1].upper() else "D" if e == b"-" else "X"
        if o != "D":
            aligned += ref[p:p + 1] if o == "=" else e
        push(1, o)
    c.add(ts, "".join(f"{n}{o}" for n, o in ops), bytes(aligned), strand=strand, target=target)
    return c


def sides(ref, sites, n_a, n_b, b_edits=None, b_ins=None, span=None, strands="+-", c=None, target=None, b_few=None):
    """n_a rows of the contig's own strain and n_b rows that carry the other base at every site, and b_edits / b_ins besides (b_few:
    only the first b_few of them carry those)"""
    c = c or PI.Case([("c", ref)])
    ts, te = span or (0, len(ref))
    alt = {p: other_base(ref[p]) for p in sites if ts <= p < te}
    k = 0
    for i in range(n_a):
        add_read(c, ref, ts, te, strand=strands[k % len(strands)], target=target)
        k += 1
    for i in range(n_b):
        more = b_few is None or i < b_few
        add_read(c, ref, ts, te, {**alt, **((b_edits or {}) if more else {})}, (b_ins or {}) if more else {}, strand=strands[k % len(strands)],
                 target=target)
        k += 1
    return c


def head(name, ln, rc, xc, hb=None, hp=None):
    h = b">%s LN:i:%d RC:i:%d XC:f:%s" % (name, ln, rc, xc)
    return h + (b" HB:i:%d HP:i:%d" % (hb, hp) if hb is not None else b"") + b"\n"


def _sub(seq, edits):
    s = bytearray(seq)
    for p, b in edits.items():
        s[p:p + 1] = b
    return bytes(s)


def hand_cases():
    H = {}
    # (a) two error-free strains: the contig is strain 1; strain 2 has another base on 5, 15, 25, 35, a T in front of 10, GCA in front
    # of 20 and lacks 29 and 30.  Four reads of each.  The two deleted positions are sites as well (alt del): six sites, one block
    # [5, 35].  hlmi_polish on the same input: every difference is a 4 : 4 tie or an insertion of half the rows - the contig stays
    ref = _seq(40, 3)
    subs = (5, 15, 25, 35)
    alt = {p: other_base(ref[p]) for p in subs}
    strain2 = _sub(ref, alt)
    strain2 = strain2[:10] + b"T" + strain2[10:20] + b"GCA" + strain2[20:29] + strain2[31:]
    c = sides(ref, subs, 4, 4, b_edits={29: b"-", 30: b"-"}, b_ins={10: b"T", 20: b"GCA"})
    H["two_strains"] = Hand(c, {}, head(b"c_hapA", 40, 8, b"1.000000", 1, 31) + ref + b"\n" + head(b"c_hapB", 42, 8, b"1.000000", 1, 31) + strain2 + b"\n",
                            [b"c\t6\t6\t36\t6\t4\t4\t1\t6"],
                            dict(blocks_split=1, contigs_split=1, positions_split=31, diff_positions=6, records=2, substituted=4, deleted=2,
                                 inserted_bases=4, slots_opened=2))
    # (b) one read of every combination on two sites: the link is a tie, two blocks of one site, nothing to split
    c = HI.hand_cases()["tie_is_not_phased"].case
    H["no_multi_site_block"] = Hand(c, {}, head(b"c", 20, 4, b"1.000000") + REF + b"\n", [], dict(records=1))
    # (c) three rows on either side: split at min_side 3, not at 4
    tt = {2: b"T", 6: b"T"}
    c = HI.pile(REF, [tt] * 3 + [{}] * 3)
    hap_b = _sub(REF, tt)
    H["min_side_at"] = Hand(c, dict(min_side=3), head(b"c_hapA", 20, 6, b"1.000000", 1, 5) + REF + b"\n" + head(b"c_hapB", 20, 6, b"1.000000", 1, 5) + hap_b + b"\n",
                            [b"c\t3\t3\t7\t2\t3\t3\t1\t2"],
                            dict(blocks_split=1, contigs_split=1, positions_split=5, diff_positions=2, records=2, substituted=2))
    H["min_side_above"] = Hand(c, dict(min_side=4), head(b"c", 20, 6, b"1.000000") + REF + b"\n", [b"c\t3\t3\t7\t2\t3\t3\t0\t0"], dict(records=1))
    # (d) two rows on either side and r4 (T then G: hap_a = hap_b = 1, a tie): r4 votes on both sides inside [2, 6], which gives
    # either side its third vote there (min_cov 3): XC is 1 on both, and side B's position 6 is T by 2 : 1
    c = HI.pile(REF, [tt, tt, {}, {}, {2: b"T"}])
    H["a_tied_row_votes_on_both_sides"] = Hand(
        c, dict(min_side=2), head(b"c_hapA", 20, 5, b"1.000000", 1, 5) + REF + b"\n" + head(b"c_hapB", 20, 5, b"1.000000", 1, 5) + hap_b + b"\n",
        [b"c\t3\t3\t7\t2\t2\t2\t1\t2"], dict(blocks_split=1, contigs_split=1, positions_split=5, diff_positions=2, records=2, substituted=2))
    # (e) sites 6 and 14; two of the three B rows carry another base on 5, 7, 13 and 15 as well - 2 of 6 votes, below min_frac 0.4,
    # no site.  7 and 13 lie inside the extent: side B decides them 2 : 1.  5 and 15 lie outside: all six rows vote, 4 : 2 for the contig
    at = {6: b"T", 14: b"T"}
    more = {p: other_base(REF[p], 2) for p in (5, 7, 13, 15)}
    c = sides(REF, (6, 14), 3, 3, b_edits=more, b_few=2, strands="+")
    hb = _sub(REF, {**at, 7: more[7], 13: more[13]})
    H["extent_edges_for_positions"] = Hand(
        c, dict(min_frac=0.4), head(b"c_hapA", 20, 6, b"1.000000", 1, 9) + REF + b"\n" + head(b"c_hapB", 20, 6, b"1.000000", 1, 9) + hb + b"\n",
        [b"c\t7\t7\t15\t2\t3\t3\t1\t4"], dict(blocks_split=1, contigs_split=1, positions_split=9, diff_positions=4, records=2, substituted=4))
    # (f) the B rows insert C in front of 6 (the slot in front of the first site lies outside: six rows span, three insert: shut), of
    # 7 and of 14 (inside: on side B three span and three insert: open; on side A nobody inserts)
    c = sides(REF, (6, 14), 3, 3, b_ins={6: b"C", 7: b"C", 14: b"C"})
    hb = _sub(REF, at)
    hb = hb[:7] + b"C" + hb[7:14] + b"C" + hb[14:]
    H["extent_edges_for_slots"] = Hand(
        c, {}, head(b"c_hapA", 20, 6, b"1.000000", 1, 9) + REF + b"\n" + head(b"c_hapB", 22, 6, b"1.000000", 1, 9) + hb + b"\n",
        [b"c\t7\t7\t15\t2\t3\t3\t1\t2"],
        dict(blocks_split=1, contigs_split=1, positions_split=9, diff_positions=2, records=2, substituted=2, inserted_bases=2, slots_opened=2))
    # (g) two A rows against four B rows at min_side 2: inside [6, 14] side A has two votes, below min_cov 3: the contig's bytes stay,
    # the lower case of 8 and 9 included, and 9 of 20 positions are not covered; side B decides them (upper case)
    low = REF[:8] + REF[8:10].lower() + REF[10:]
    c = sides(low, (6, 14), 2, 4)
    H["a_side_below_min_cov_keeps_the_contig"] = Hand(
        c, dict(min_side=2), head(b"c_hapA", 20, 6, b"0.550000", 1, 9) + low + b"\n" + head(b"c_hapB", 20, 6, b"1.000000", 1, 9) + _sub(REF, at) + b"\n",
        [b"c\t7\t7\t15\t2\t2\t4\t1\t9"], dict(blocks_split=1, contigs_split=1, positions_split=9, diff_positions=9, records=2, substituted=2))
    return H


def records(fasta):
    """-> [(name, {tag: value}, bases)]"""
    L = fasta.split(b"\n")
    out = []
    for h, s in zip(L[0::2], L[1::2]):
        f = h[1:].split(b" ")
        out.append((f[0], {t[:2]: t[5:] for t in f[1:]}, s))
    return out


def block_rows(blocks):
    """-> [(contig, 0-based start, 0-based end, sites, rows_a, rows_b, split, diff)]"""
    return [(f[0], int(f[2]) - 1, int(f[3]) - 1, int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]))
            for f in (line.split(b"\t") for line in blocks.split(b"\n")[1:] if line)]


def shapes():
    S = {}
    lo = dict(min_side=2, min_cov=2)

    # an extent across the count tile's border: sites on T - 2 and T + 2, the B rows insert GA in front of T
    ref = _seq(T + 40, 1)
    c = sides(ref, (T - 2, T + 2), 3, 3, b_ins={T: b"GA"}, span=(T - 30, T + 30))

    def where(fa, blocks, st, ref=ref):
        assert block_rows(blocks) == [(b"c", T - 2, T + 2, 2, 3, 3, 1, 2)]
        (_, ta, a), (_, tb, b) = records(fa)
        strain = _sub(ref, {T - 2: other_base(ref[T - 2]), T + 2: other_base(ref[T + 2])})
        assert a == ref and b == strain[:T] + b"GA" + strain[T:] and tb[b"HP"] == b"5"
    S["extent_across_the_tile_border"] = Shape(c, {}, where)

    # one extent ends on the tile's last position, the next starts on the next tile's first: no row spans both, the link between
    # T - 1 and T has no informative row.  Rows that end / start on the border exactly
    c = sides(ref, (T - 5, T - 1), 3, 3, span=(T - 25, T))
    sides(ref, (T, T + 4), 3, 3, span=(T, T + 25), c=c)

    def where(fa, blocks, st):
        assert block_rows(blocks) == [(b"c", T - 5, T - 1, 2, 3, 3, 1, 2), (b"c", T, T + 4, 2, 3, 3, 1, 2)] and st["positions_split"] == 10
    S["extents_on_both_sides_of_the_tile_border"] = Shape(c, {}, where)

    # a D run of SHORT_RUN + 4 columns across the extent's first position in one B row and across its last in one A row, under = runs
    # far longer than SHORT_RUN in every other row: one row's del is no site; inside the extent it is one of three votes of its side
    ref = _seq(200, 4)
    n = SHORT_RUN + 4
    c = sides(ref, (60, 140), 3, 3)
    add_read(c, ref, 0, 200, {140: other_base(ref[140]), **{p: b"-" for p in range(60 - n // 2, 60 + n // 2)}})
    add_read(c, ref, 0, 200, {p: b"-" for p in range(140 - n // 2, 140 + n // 2)}, strand="-")

    def where(fa, blocks, st):
        assert block_rows(blocks) == [(b"c", 60, 140, 2, 4, 4, 1, 2)] and st["sites"] == 2 and st["deleted"] == 0
    S["long_runs_across_the_extent_edges"] = Shape(c, {}, where)

    # 300 split blocks under two long rows: pairs of sites on 6k + 2 and 6k + 4; long row 0 reads the contig's base everywhere, long
    # row 1 the other base in every even pair - between two pairs one of them reads cis and one trans: a tie, no link; a short row
    # over every pair reads the other base on both.  min_link 1 and min_side 1: every pair is a split block, long row 0 is shut out
    # of side B in 300 extents - about 170 of them in one tile
    n_pairs = 300
    ref = _seq(6 * n_pairs + 8, 5)
    pairs = [(6 * k + 2, 6 * k + 4) for k in range(n_pairs)]
    c = PI.Case([("c", ref)])
    add_read(c, ref, 0, len(ref))
    add_read(c, ref, 0, len(ref), {p: other_base(ref[p]) for k, pq in enumerate(pairs) if k % 2 == 0 for p in pq}, strand="-")
    for k, (p, q) in enumerate(pairs):
        add_read(c, ref, p - 2, q + 2, {p: other_base(ref[p]), q: other_base(ref[q])}, strand="+-"[k % 2])

    def where(fa, blocks, st, ref=ref, pairs=tuple(pairs)):
        rows = block_rows(blocks)
        assert [(r[1], r[2]) for r in rows] == list(pairs) and all(r[3:7] == (2, 1 + k % 2, 2 - k % 2, 1) for k, r in enumerate(rows))
        assert st["blocks_split"] == n_pairs and st["links_phased"] == n_pairs and len(ref) > T + 600
    S["one_long_row_over_300_split_blocks"] = Shape(c, dict(min_link=1, min_side=1, min_cov=1, min_alt=1), where)

    # CIGARs of 63, 64 and 65 ops: 3= 1X 1I 1X ... in two rows (one per strand) - every X a site, every I an insertion of side B
    # inside the extent - against two plain rows
    for n_ops in (63, 64, 65):
        runs = [[(3, "="), (1, "X"), (1, "I"), (1, "X")][i % 4] for i in range(n_ops)]
        ln = sum(n for n, o in runs if o != "I") + 11
        ref = _seq(ln, n_ops)
        aligned, p, xs, n_i = bytearray(), 5, [], 0
        for n, o in runs:
            if o == "X":
                xs.append(p)
                aligned += other_base(ref[p], 2)
            elif o == "I":
                aligned += b"T"
                n_i += 1 if p < 5 + sum(m for m, k in runs if k != "I") else 0      # an I behind the last column belongs to no slot
            else:
                aligned += ref[p:p + n]
            p += n if o != "I" else 0
        cig = "".join(f"{n}{o}" for n, o in runs)
        c = PI.Case([("c", ref)])
        c.add(5, cig, bytes(aligned)).add(5, cig, bytes(aligned), strand="-").add(0, f"{ln}=", ref).add(0, f"{ln}=", ref, strand="-")

        def where(fa, blocks, st, xs=tuple(xs), n_i=n_i, ln=ln):
            assert block_rows(blocks) == [(b"c", xs[0], xs[-1], len(xs), 2, 2, 1, len(xs))]
            assert st["slots_opened"] == n_i and st["substituted"] == len(xs) and [len(s) for _, _, s in records(fa)] == [ln, ln + n_i]
        S[f"cigar_of_{n_ops}_ops"] = Shape(c, dict(lo, min_alt=2, min_frac=0.5), where)

    # two contigs with a split block next to the junction on either side; contig m has no row, contig z rows and no site
    ra, rb, rm, rz = _seq(30, 1), _seq(30, 4), _seq(25, 2), _seq(50, 6)
    for unpolished in (0, 1):
        c = PI.Case([("a", ra), ("m", rm), ("b", rb), ("z", rz)])
        sides(ra, (20, 29), 3, 3, c=c, target="a")
        sides(rb, (0, 9), 3, 3, c=c, target="b", strands="-+")
        sides(rz, (), 4, 0, c=c, target="z")

        def where(fa, blocks, st, unpolished=unpolished):
            assert block_rows(blocks) == [(b"a", 20, 29, 2, 3, 3, 1, 2), (b"b", 0, 9, 2, 3, 3, 1, 2)]
            assert [n for n, _, _ in records(fa)] == [b"a_hapA", b"a_hapB"] + [b"m"] * unpolished + [b"b_hapA", b"b_hapB", b"z"]
            assert st["contigs_split"] == 2 and st["records"] == 5 + unpolished
        S[f"junction_and_plain_contigs_unpolished_{unpolished}"] = Shape(c, dict(include_unpolished=unpolished), where)
    return S
