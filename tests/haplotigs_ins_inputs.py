"""Inputs of the tests of hlmi_haplotigs_ins (against tests/haplotigs_ins_model.py), built with phase_ins_inputs.row / pile.

cases(): {name: Case(case, opts, reaches, where)}; `where` is a function of (reach, the model's fasta, blocks, stats) that asserts
on the model what the case was built for - that its block is split and where its extent starts and ends - before the input is
used on the GPU.  HAP_TILE is read from the kernels' header as haplotigs_inputs.py reads it.
insertion_strains_only(): phase_ins_inputs.insertion_strains - a minority strain that differs from the contig by three insertions
alone - with what the calls must make of it."""
import collections

import haplotigs_inputs as GI
import phase_inputs as HI
import phase_ins_inputs as II
import polish_inputs as PI

T = GI.HAP_TILE
REF = HI.REF
Case = collections.namedtuple("Case", "case opts reaches where")
other_base = HI.other_base
LO = dict(min_side=2, min_cov=2)


def block_rows(blocks):
    """-> [(contig, block id, start, end, sites, rows_a, rows_b, split, diff_positions, diff_slots)]; ids and ends as printed"""
    return [(f[0], f[1], f[2], f[3]) + tuple(int(x) for x in f[4:10]) for f in (line.split(b"\t") for line in blocks.split(b"\n")[1:] if line)]


def strains(ref, at, edits, n_a=3, n_b=3, span=None, more=(), strands="+-"):
    """n_a rows of the contig's strain and n_b that carry `at` and `edits`, over span; more: further rows (ts, te, at, edits)"""
    ts, te = span or (0, len(ref))
    cut = lambda d: {p: v for p, v in d.items() if ts <= p <= te}          # noqa: E731
    return II.pile(ref, [(ts, te, {}, {})] * n_a + [(ts, te, cut(at), cut(edits))] * n_b + list(more), strands=strands)


def insertion_strains_only():
    return II.insertion_strains()


def cases():
    C = {}

    def one(name, case, opts, reaches, rows, **stats):
        def where(reach, fa, blocks, st, rows=rows, stats=stats):
            assert block_rows(blocks) == rows, block_rows(blocks)
            assert all(st[k] == v for k, v in stats.items()), {k: st[k] for k in stats}
        C[name] = Case(case, opts, reaches, where)

    # The extent starts at slot 5 and ends at slot 14 (keys 10 .. 28: positions 5 .. 13).  Three B rows insert at both edge slots
    # and carry T on 10.  Shut out of side A besides them: r6 starts on position 5 (its I at ts is an edge op), r7 ends on 14
    # (its I at te likewise), r8 inserts at slot 5 and ends on position 13; r9 is an A row that starts on 14 - position 14 lies
    # outside and slot 14 inside.  Side A keeps both slots shut, side B opens both
    at, t10 = {5: b"TT", 14: b"C"}, {10: b"T"}
    more = [(5, 20, at, t10), (0, 14, at, t10), (0, 14, {5: b"TT"}, t10), (9, 20, {}, {}), (14, 20, {}, {})]
    one("extent_from_a_slot_to_a_slot", strains(REF, at, t10, more=more), {}, (1,),
        [(b"c", b"5+", b"5+", b"14+", 3, 4, 6, 1, 1, 2)], positions_split=9, diff_slots=2, blocks_split=1)
    # ... from slot 5 to position 10, and from position 4 to slot 14: one edge of either kind
    one("extent_from_a_slot_to_a_position", strains(REF, {5: b"TT"}, t10, more=[(5, 20, {}, t10), (0, 11, {5: b"TT"}, t10)]), {}, (1,),
        [(b"c", b"5+", b"5+", b"11", 2, 3, 5, 1, 1, 1)], positions_split=6, diff_slots=1)
    one("extent_from_a_position_to_a_slot", strains(REF, {14: b"C"}, {4: b"C"}, more=[(0, 14, {}, {4: b"C"}), (14, 20, {}, {}), (3, 15, {14: b"C"}, {4: b"C"})]),
        {}, (1,), [(b"c", b"5", b"5", b"14+", 2, 3, 5, 1, 1, 1)], positions_split=10, diff_slots=1)
    # the smallest extents: slot 5 with position 5 (keys 10, 11), and position 4 with slot 5 (keys 9, 10): one position each
    one("slot_p_with_position_p", strains(REF, {5: b"TT"}, {5: b"G"}, more=[(5, 20, {}, {5: b"G"}), (0, 6, {5: b"TT"}, {5: b"G"})]), {}, (1,),
        [(b"c", b"5+", b"5+", b"6", 2, 3, 5, 1, 1, 1)], positions_split=1, diff_slots=1)
    one("position_p_with_slot_p_plus_1", strains(REF, {5: b"TT"}, {4: b"C"}, more=[(4, 20, {5: b"TT"}, {4: b"C"}), (0, 5, {}, {4: b"C"})]), {}, (1,),
        [(b"c", b"5", b"5", b"5+", 2, 3, 5, 1, 1, 1)], positions_split=1, diff_slots=1)

    # edges at the count tile's border.  An edge slot at tile offset 0 as a first site ...
    ref = HI._seq(T + 40, 1)
    oT3 = {T + 3: other_base(ref[T + 3])}
    one("first_site_the_slot_at_tile_offset_0", strains(ref, {T: b"GA"}, oT3, span=(T - 30, T + 30), more=[(T, T + 30, {}, oT3)]), {}, (1,),
        [(b"c", b"%d+" % T, b"%d+" % T, b"%d" % (T + 4), 2, 3, 4, 1, 1, 1)], positions_split=4, diff_slots=1)
    # ... and as a last site: the extent touches the next tile by that slot alone; a B row ends on T, an A row starts on it
    oT4 = {T - 4: other_base(ref[T - 4])}
    one("last_site_the_slot_at_tile_offset_0",
        strains(ref, {T: b"GA"}, oT4, span=(T - 30, T + 30), more=[(T - 30, T, {}, oT4), (T, T + 30, {}, {}), (T - 10, T + 1, {T: b"GA"}, oT4)]), {}, (1,),
        [(b"c", b"%d" % (T - 3), b"%d" % (T - 3), b"%d+" % T, 2, 3, 5, 1, 1, 1)], positions_split=4, diff_slots=1)
    # an extent that opens in the previous tile and ends at a slot in this one
    one("opens_in_the_previous_tile_ends_at_a_slot", strains(ref, {T + 2: b"C"}, oT4, span=(T - 30, T + 30), more=[(T - 2, T + 2, {}, {})]), {}, (1,),
        [(b"c", b"%d" % (T - 3), b"%d" % (T - 3), b"%d+" % (T + 2), 2, 3, 3, 1, 1, 1)], positions_split=6, diff_slots=1)

    # One row over HAP_TILE + 1 split extents that touch one tile, single-position extents of position p with slot p + 1 on
    # every p of [T - 20, 2 T + 20): four rows; in even blocks rows 2 and 3 carry the other base and the insertion, in odd
    # blocks rows 1 and 3 - inside a block the four agree (cis 2 : 2), between neighbouring blocks every combination occurs
    # once (a tie, no link).  The block on 2 T - 1 reaches tile 2 by its slot alone, tile 1 is touched by T + 1 extents
    ln = 3 * T
    ref = HI._seq(ln, 7)
    lo, hi = T - 20, 2 * T + 20
    reads = []
    for g in range(4):
        mine = [p for p in range(lo, hi) if (g >> 1 if (p - lo) % 2 == 0 else g & 1)]
        reads.append(({p + 1: b"T" for p in mine}, {p: other_base(ref[p]) for p in mine}))
    c = II.pile(ref, reads, strands="+-")

    def where(reach, fa, blocks, st, lo=lo, hi=hi):
        rows = block_rows(blocks)
        assert [(r[1], r[3]) for r in rows] == [(b"%d" % (p + 1), b"%d+" % (p + 1)) for p in range(lo, hi)]
        assert all(r[4:10] == (2, 2, 2, 1, 1, 1) for r in rows) and st["blocks_split"] == hi - lo
        touching = sum(1 for p in range(lo, hi) if 2 * p + 1 <= 2 * (2 * T) - 1 and 2 * (p + 1) >= 2 * T)
        assert touching == T + 1 > T // 2 + 1
    C["one_row_over_a_tile_of_single_position_extents"] = Case(c, dict(LO), (1,), where)

    # A block of mixed kinds around PHASE_REACH_TILE at reach 2 with a bridged insertion site inside the extent:
    # phase_ins_inputs's mixed shape - TILE + 9 sites, position sites and insertion sites in turn, r0, r1 carry every alt, r2, r3
    # the contig, r4 - r6 lie around the tile's border - with the slot next to site TILE made noisy as
    # noisy_insertion_site_bridged_at_reach_2 makes its slot: of the whole-length rows r0 (alt strain) and r2 (the contig's)
    # insert there, r1, r3 and the short rows do not.  Both of its links are ties, the link across it is cis: at reach 2 the
    # slot is bridged inside the one split block, which keeps its TILE + 9 sites; at reach 1 it cuts the block in two
    n = II.TILE + 9
    ln = 2 * n + 12
    ref = HI._seq(ln, 3)
    kind = [i % 2 for i in range(n)]                                        # 1: a slot
    where_at = [4 + 2 * i for i in range(n)]                                # position p, or slot p
    j = II.TILE + 1 - II.TILE % 2                                           # the noisy site: the slot at or behind site TILE
    slots = {p: b"T" for p, k in zip(where_at, kind) if k}
    subs = {p: other_base(ref[p]) for p, k in zip(where_at, kind) if not k}
    calm = {p: b for p, b in slots.items() if p != where_at[j]}
    c = II.pile(ref, [(slots, subs), (calm, subs), ({where_at[j]: b"T"}, {}), ({}, {}), (where_at[II.TILE - 3], where_at[II.TILE + 2] + 1, calm, subs),
                      (where_at[II.TILE], ln, {}, {}), (where_at[II.TILE - 40], where_at[II.TILE + 4] + 1, {}, {})], strands="+-")
    opts = dict(min_cov=2, min_alt=2, min_frac=0.2, min_side=2)

    def where(reach, fa, blocks, st, c=c, opts=opts, n=n, j=j, slot=where_at[j], last=where_at[n - 1]):
        import phase_ins_model as IM
        sites = IM.phase(c.contigs_bytes(), c.reads_bytes(), c.paf_bytes(), None, reach, **{k: v for k, v in opts.items() if k != "min_side"})[0]
        sr = II.site_rows(sites)
        assert len(sr) == n and sr[j][1:3] == (slot, b"+T") and kind[j] == 1 and II.TILE <= j <= II.TILE + 1
        rows = block_rows(blocks)
        if reach == 1:                                              # the noisy slot is a block of its own between two split ones
            assert [r[3] for r in rows] == [b"%d" % (where_at[j - 1] + 1), b"%d" % (last + 1)] and sr[j][3] == b"%d+" % slot and sr[j][4] != b"."
            assert [(r[4], r[7]) for r in rows] == [(j, 1), (n - j - 1, 1)]
            return
        assert sr[j][3:] == (b"5", b".") and all(r[4] != b"." for i, r in enumerate(sr) if i != j)          # bridged, and it alone
        assert rows == [(b"c", b"5", b"5", b"%d" % (last + 1), n, rows[0][5], rows[0][6], 1, rows[0][8], rows[0][9])]
        assert min(rows[0][5:7]) >= 2 and 2 * 4 + 1 <= 2 * slot <= 2 * last + 1                              # split; the slot inside the extent
        assert st["blocks_split"] == 1 and st["positions_split"] == last - 4 + 1 and st["ins_sites_phased"] == n // 2 - 1
        # per side the bridged slot stays shut (one of the side's rows inserts), every other slot opens on side B alone
        assert rows[0][9] == st["diff_slots"] == n // 2 - 1
    C["mixed_kinds_around_the_reach_tile_with_a_bridged_slot"] = Case(c, opts, (1, 2), where)
    # the same noise by hand on three sites (phase_ins_inputs's hand case): the extent [3, 11] holds the bridged slot 6
    h = II.hand_cases()["noisy_insertion_site_bridged_at_reach_2"]
    one("bridged_insertion_site_inside_the_extent", h.case, dict(h.opts), (2,), [(b"c", b"3", b"3", b"11", 3, 3, 3, 1, 2, 0)], positions_split=9)

    # CIGARs in which the I op of a slot is op 63, 64 and 65: phase_ins_inputs's shape; every slot lies inside the one extent,
    # and with the X columns on the rows that insert the first and the last site are position sites
    s = II.shapes()["i_op_as_op_63_64_65"]

    def where(reach, fa, blocks, st):
        rows = block_rows(blocks)
        assert len(rows) >= 1 and st["ins_sites_phasing"] == 3
    C["i_op_as_op_63_64_65"] = Case(s.case, dict(s.opts, min_side=2), (1,), where)
    # ... and as the op of an edge slot: the extent's last site is the slot whose I is op m of the B rows' CIGAR (2= 1X ...)
    for m in (63, 64, 65):
        n = 330
        ref = HI._seq(n, 4)
        xs_all = list(range(7, n - 5, 3))
        slot = 5 + 3 * (m // 2) + (2 if m % 2 else 0)
        xs = {p: other_base(ref[p]) for p in xs_all if p < slot}
        c = II.pile(ref, [(5, n - 3, {slot: b"CA"}, xs)] * 2 + [(0, n, {}, {})] * 2, strands="+-")
        assert PI.cigar_ops(c.rows[0].split(b"cg:Z:")[1].decode())[m] == (2, "I"), m

        def where(reach, fa, blocks, st, slot=slot, n_x=len(xs)):
            (r,) = block_rows(blocks)
            assert r[1:4] == (b"8", b"8", b"%d+" % slot) and r[4:8] == (n_x + 1, 2, 2, 1) and r[9] == 1
        C[f"edge_slot_as_op_{m}"] = Case(c, dict(LO), (1,), where)
    return C
