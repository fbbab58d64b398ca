"""Inputs of tests/test_gpu_depth.py (hlmi_depth against tests/depth_model.py): contigs with one read per span, every column '=',
built with polish_inputs.Case, at the smallest shapes where depth_tile_kernel and the run and median passes can go wrong.  The
tile is read from the kernel's header as polish_inputs.kernel_constants() reads it.  Each case comes with `where`, a function
of the model's output that asserts the case sits where it claims to (the test calls it before the library runs).

-> {name: Shape(case, where)}"""
import collections

import polish_inputs as PI

T = PI.kernel_constants()["tile"]
Shape = collections.namedtuple("Shape", "case where")


def _seq(n, k=0):
    return (b"ACGGTCATTG"[k % 7:] + b"ACGGTCATTG" * (n // 10 + 1))[:n]


def span_case(contigs, spans):
    """contigs: [(name, length)]; spans: [(contig name, ts, te)] in file order - one read per span"""
    c = PI.Case([(n, _seq(L, k)) for k, (n, L) in enumerate(contigs)])
    seqs = dict(c.contigs)
    for t, a, b in spans:
        assert 0 <= a < b <= len(seqs[t.encode()]), (t, a, b)
        c.add(a, f"{b - a}=", seqs[t.encode()][a:b], target=t)
    return c


def tile_row_ranges(spans, length):
    """polish_layout's tiles of one contig: spans [(ts, te)] -> {t0: (row_lo, row_hi)} over the rows sorted by (ts, line)"""
    rows = sorted(spans, key=lambda s: s[0])
    out, lo, hi = {}, 0, 0
    for t0 in range(0, length, T):
        n_pos = min(T, length - t0)
        while hi < len(rows) and rows[hi][0] < t0 + n_pos:
            hi += 1
        while lo < hi and rows[lo][1] <= t0:
            lo += 1
        if lo < hi:
            out[t0] = (lo, hi)
    return rows, out


def bed_rows(bed):
    return [(f[0], int(f[1]), int(f[2]), int(f[3])) for f in (line.split(b"\t") for line in bed.split(b"\n") if line)]


def depth_at(bed, name, p):
    for n, a, b, v in bed_rows(bed):
        if n == name and a <= p < b:
            return v
    raise AssertionError((name, p))


def shapes():
    S = {}

    # spans whose ts or te is t0 - 1, t0, t0 + 1 for t0 = T and 2 T, and one span over three tiles
    spans = []
    for t0 in (T, 2 * T):
        for e in (t0 - 1, t0, t0 + 1):
            spans += [("c", e, e + 37), ("c", e - 41, e), ("c", e - 23, e)]    # one starts and two end on e: the depth changes
    spans.append(("c", T - 100, 2 * T + 100))
    L = 3 * T + 50

    def where(tsv, bed, st):
        starts = {a for _, a, _, _ in bed_rows(bed)}
        assert {T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1} <= starts                  # the depth changes on all six
        assert depth_at(bed, b"c", T - 100) >= 1 and depth_at(bed, b"c", 2 * T + 99) >= 1 and depth_at(bed, b"c", 3 * T) == 0
        assert st["rows_selected"] == 19
    S["edges_of_two_tile_borders"] = Shape(span_case([("c", L)], spans), where)

    # a row inside a tile's row range that ended in front of the tile: A lives through tile 1, B (behind A in the order) ends in tile 0
    spans2 = [("c", 10, T + 300), ("c", 20, 60), ("c", T + 5, T + 80)]

    def where(tsv, bed, st):
        rows, ranges = tile_row_ranges([(a, b) for _, a, b in spans2], 2 * T)
        lo, hi = ranges[T]
        assert (lo, hi) == (0, 3) and rows[1] == (20, 60) and rows[1][1] <= T           # B is in [lo, hi) of the tile at T
        assert depth_at(bed, b"c", T) == 1 and depth_at(bed, b"c", T + 5) == 2
    S["row_in_range_ends_before_the_tile"] = Shape(span_case([("c", 2 * T)], spans2), where)

    # contigs of 1, T - 1, T, T + 1 bases side by side
    lens = [("one", 1), ("tm1", T - 1), ("t", T), ("tp1", T + 1)]
    spans3 = []
    for n, ln in lens:
        spans3 += [(n, 0, ln), (n, ln // 2, ln)]

    def where(tsv, bed, st):
        assert st["contigs_covered"] == 4 and st["covered"] == st["positions"] == 1 + 3 * T
        assert depth_at(bed, b"tp1", T) == 2 and depth_at(bed, b"one", 0) == 2
    S["contig_lengths_around_the_tile"] = Shape(span_case(lens, spans3), where)

    # three contigs, the middle one without rows: the third's tiles start at a cbase that is no multiple of the tile
    spans4 = [("a", 100, 650), ("a", 0, 700), ("z", 0, T + 200), ("z", T - 30, T + 500), ("z", 40, 90)]

    def where(tsv, bed, st):
        assert 700 % T != 0 and st["contigs_covered"] == 2 and st["contigs"] == 3
        assert (b"m", 0, 300, 0) in bed_rows(bed)
        assert depth_at(bed, b"z", T) == 2 and depth_at(bed, b"z", T + 499) == 1
    S["middle_contig_without_rows"] = Shape(span_case([("a", 700), ("m", 300), ("z", T + 500)], spans4), where)

    # 300 rows on one [ts, te): more rows than threads in the workgroup, every atomic on the same two LDS words
    def where(tsv, bed, st):
        assert bed_rows(bed) == [(b"c", 0, 40, 0), (b"c", 40, 140, 300), (b"c", 140, 400, 0)] and st["bases"] == 30000
    S["deep_pile_on_one_span"] = Shape(span_case([("c", 400)], [("c", 40, 140)] * 300), where)

    # the same depth on both sides of the tile border (two rows that meet there, and one that crosses it): one run, not two
    def where(tsv, bed, st):
        assert bed_rows(bed) == [(b"c", 0, 100, 0), (b"c", 100, T + 100, 1), (b"c", T + 100, 2 * T, 0)]
    S["equal_depth_across_the_border"] = Shape(span_case([("c", 2 * T)], [("c", 100, T), ("c", T, T + 100)]), where)

    # the depth changes exactly on the border
    def where(tsv, bed, st):
        assert (b"c", T - 50, T, 2) in bed_rows(bed) and (b"c", T, T + 60, 1) in bed_rows(bed)
    S["depth_change_on_the_border"] = Shape(span_case([("c", 2 * T)], [("c", T - 50, T), ("c", T - 60, T + 60)]), where)

    # two adjacent contigs with the same depth at their junction: two runs
    def where(tsv, bed, st):
        assert bed_rows(bed) == [(b"a", 0, 400, 0), (b"a", 400, 500, 1), (b"b", 0, 100, 1), (b"b", 100, 300, 0)]
    S["equal_depth_at_a_contig_junction"] = Shape(span_case([("a", 500), ("b", 300)], [("a", 400, 500), ("b", 0, 100)]), where)
    return S
