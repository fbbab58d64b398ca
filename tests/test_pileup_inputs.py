"""CPU: every input of tests/pileup_inputs.py sits on the edge of the SNP pile-up it is named for - proved from the oracle
alone (tests/test_gpu_pileup_edges.py would pass on any kernel if the inputs missed their edges).  The edges are the
constants of filter_stage.hip, read from its text: retuning one fails these tests instead of moving the inputs off the
edge unnoticed."""
import time
from collections import defaultdict

import pytest

import pileup_inputs as P
from oracle import filters as F

K = P.kernel_constants()
TILE, LIGHT, CACHE, TRIP, CAP = K["tile"], K["light_rows"], K["light_cache"], K["heavy_trip"], K["max_rows"]


def seg_class(n, mc):
    """pile_seg_class_kernel: 0 = statistics only, 1 = light kernel, 2 = heavy kernel."""
    return 0 if n < 2 * mc else 1 if n <= LIGHT else 2


def pile(name):
    c = P.get(name)
    return F.snp_pileup(P.sorted_rows(name), c.long_mode)


def spanning(intervals, read, pos):
    return sum(1 for s, e in intervals.get(read, ()) if s < pos < e)


def x_keys_of_row(f, long_mode):
    """[(op index, target key, query key)] of the X ops of one row (fields), as F.snp_pileup walks it."""
    ql, qs, qe, ts = int(f[1]), int(f[2]), int(f[3]), int(f[7])
    minus = f[4] != "+"
    qpos, tpos, out = (ql - qe) if minus else qs, ts, []
    for i, (n, op) in enumerate(F.cigar_ops(f[-1])):
        if op in "=XI":
            qpos += n
        if op in "=XD":
            tpos += n
        if op == "X":
            out.append((i, tpos, (ql - qpos + 1) if minus else qpos))
    return out


def test_the_inputs_were_designed_for_the_kernels_constants():
    assert (TILE, LIGHT, CACHE, TRIP, CAP) == (P.TILE, P.LIGHT_ROWS, P.LIGHT_CACHE, P.HEAVY_TRIP, P.MAX_ROWS)
    assert CAP < 1 << 16                                   # the heavy kernel's 16-bit counters


@pytest.mark.parametrize("name", P.NAMES)
def test_rows_reach_the_pile_up_and_the_oracles_agree(name):
    c = P.get(name)
    srt = P.sorted_rows(name)
    assert len(srt) == len(c.lines) - c.n_unfiltered       # contained rows: nothing lost to the window filter
    for h, d in c.hubs.items():                            # hub sizes as built = rows per read as the kernels count them
        if name.startswith("rowsel") and h == "T":
            continue
        assert P.segment_sizes(srt, c.long_mode)[h] == d["rows"]
    t0 = time.time()
    for mc in c.mcs:
        fast = P.counts(name, mc)
        slow = dict(F.supported_pair_counts(*F.snp_pileup(srt, c.long_mode), mc))
        assert fast == slow
    # measured: 4 s for each of the two cap hubs (60 000 rows, 3.1e5 events), both forms: no need to skip them
    assert time.time() - t0 < 120


@pytest.mark.parametrize("name", P.NAMES)
def test_probes_have_the_support_and_coverage_they_were_built_for(name):
    c = P.get(name)
    snp, partners, intervals = pile(name)
    seen = defaultdict(int)
    for mc in c.mcs if not c.long_mode else (c.mc,):
        for p in c.probes:
            key = (p["read"], p["pos"])
            if p["kind"] == "zero_x":
                assert snp[key] >= 1 and spanning(intervals, *key) - snp[key] < 1     # a key nobody can span
                continue
            v, span = snp[key], spanning(intervals, *key)
            assert (v, span - v) == (p["v"], p["further"]), p
            built_mc = 2 if not c.long_mode else c.mc                                 # short inputs are built for mc = 2
            if mc == built_mc:
                assert (v >= mc and span - v >= mc) == p["supported"], p
                seen[p["kind"], p["supported"]] += 1
                if p["kind"] == "sup" and p["supported"]:
                    assert span - v == mc                                             # exactly mc further rows
                if p["kind"] == "lowv":
                    assert v == mc - 1
                if p["kind"] == "lowspan" and v >= mc:
                    assert span - v < mc
    if name not in ("rowsel",):
        assert seen["sup", True] + seen["mc", True] >= 2 and any(not s for _, s in seen), seen


@pytest.mark.parametrize("name", P.NAMES)
def test_sweep_is_within_the_cap_and_not_vacuous(name):
    c = P.get(name)
    if c.long_mode:
        th = P.thresholds(name)
        cmax = max(P.counts(name).values())
        assert len(th) == cmax + 1 <= P.MAX_THRESHOLDS
        if name in P.CAP_NAMES:
            assert len(th) <= 6
        sweep = F.worker_sweep(c.lines, True, P.M, c.mc, 0.0, th)
        kept = [len(sweep[t]) for t in th]
        assert kept == sorted(kept) and len(set(kept)) == len(kept) or len(set(kept)) >= 2, kept
        assert kept[-1] == len({F.pair_key(l.split("\t")[0], l.split("\t")[5]) for l in P.sorted_rows(name)})  # top: every pair
    else:
        kept = [len(F.worker(c.lines, False, P.M, mc, 0.0)) for mc in c.mcs]
        assert len(set(kept)) >= 2, kept


# ---- tiles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rlen", P.TILE_LENGTHS)
def test_tile_inputs_put_keys_and_interval_ends_on_every_tile_border(rlen):
    name = f"tiles_{rlen}"
    c = P.get(name)
    n_tiles = -(-(rlen + 2) // TILE)                       # the kernels walk read_len + 2 positions
    assert n_tiles == {15357: 1, 15358: 1, 15359: 2, 15360: 2, 15361: 2, 30719: 3, 30720: 3, 30721: 3, 100000: 7}[rlen]
    snp, partners, intervals = pile(name)
    seg = P.segment_sizes(P.sorted_rows(name), True)
    starts = list(range(TILE, rlen + 2, TILE))
    for side in "qt":
        for cls, tag in ((1, "L"), (2, "H")):
            hubs = [h for h in c.hubs if h.startswith(side + tag)]
            assert hubs and all(seg_class(seg[h], c.mc) == cls for h in hubs)
            assert all(c.hubs[h]["len"] == rlen for h in hubs)
            keys = {pos for h in hubs for (r, pos) in snp if r == h}
            ivs = [iv for h in hubs for iv in intervals[h]]
            assert {1, rlen} <= keys
            sup = {p["pos"] for p in c.probes if p["read"] in hubs and p["supported"]}
            for t0 in starts:
                for d in (-1, 0, 1):
                    if t0 + d <= rlen:
                        assert t0 + d in keys, (side, tag, t0 + d)
                if t0 + 1 <= rlen:
                    assert {t0 - 1, t0, t0 + 1} & sup          # a supported key at the border ...
                    assert any(e == t0 for s, e in ivs) and any(e == t0 + 1 for s, e in ivs)
                    assert {s for s, e in ivs} >= {s for s in (t0 - 1, t0, t0 + 1) if s < rlen} or cls == 1
                    assert any(s in (t0 - 1, t0, t0 + 1) for s, e in ivs)
            for k in range(1, n_tiles):
                in_tile = [p for p in c.probes if p["read"] in hubs and p["supported"] and k * TILE <= p["pos"] < (k + 1) * TILE]
                if k * TILE + 1 <= rlen:
                    assert in_tile
            if rlen >= 2 * TILE:                           # begins in one tile, ends two tiles later; a supported key whose
                assert any(e // TILE - s // TILE >= 2 for s, e in ivs)      # rows all begin in an earlier tile
                assert any(all(s < p["pos"] // TILE * TILE for h in hubs if h == p["read"] for s, e in intervals[h] if s < p["pos"] < e)
                           for p in c.probes if p["read"] in hubs and p["supported"] and p["pos"] >= TILE)
        if side == "q":
            # qlen - pos + 1 with pos = 0: only a 0-length X op as the first op of a minus-strand row that ends at qlen gives
            # the key read_len + 1 (any op of length >= 1 gives at most qlen): the inputs carry such rows
            assert all((h, rlen + 1) in snp for h in c.hubs if h.startswith("q"))
            assert any({"+", "-"} <= set(c.hubs[h]["strands"]) for h in c.hubs if h.startswith("q"))


# ---- classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mc", P.CLASS_MCS)
def test_class_inputs_sit_on_both_sides_of_every_class_border(mc):
    name = f"classes_mc{mc}"
    c = P.get(name)
    seg = P.segment_sizes(P.sorted_rows(name), True)
    sizes = sorted({2 * mc - 1, 2 * mc, LIGHT - 1, LIGHT, LIGHT + 1})
    for side in "qt":
        assert sorted(seg[h] for h in c.hubs if h[0] == side) == sizes
    cls = {n: seg_class(n, mc) for n in sizes}
    assert cls[2 * mc - 1] == 0 and cls[2 * mc] >= 1
    if mc == 8:
        assert [n for n in sizes if cls[n] == 1] == [LIGHT]            # the light class is exactly 16 rows
    if mc == 9:
        assert 1 not in cls.values() and cls[LIGHT + 1] == 0 and cls[2 * mc] == 2     # ... and empty
    if mc <= 3:
        assert cls[LIGHT] == 1 and cls[LIGHT + 1] == 2
    for h, d in c.hubs.items():
        mine = [p for p in c.probes if p["read"] == h]
        if d["rows"] >= 2 * mc:
            assert any(p["supported"] and p["v"] == mc and p["further"] == mc for p in mine), h
        else:
            assert not any(p["supported"] for p in mine)
        if d["rows"] >= 2 * mc - 1:
            assert any(p["v"] >= mc and p["further"] == mc - 1 for p in mine), h
        if mc > 1 and d["rows"] >= 2 * mc:
            assert any(p["v"] == mc - 1 and p["further"] >= mc for p in mine), h


# ---- CIGAR lengths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,want_ops", [("cigar_light", 1, P.LIGHT_OPS), ("cigar_heavy", 2, P.HEAVY_OPS)])
def test_cigar_inputs_have_supported_x_in_every_part_of_the_op_list(name, cls, want_ops):
    c = P.get(name)
    assert set(P.LIGHT_OPS) == {CACHE - 1, CACHE, CACHE + 1, CACHE + 64, 1000}
    assert set(P.HEAVY_OPS) >= {63, 64, 65, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 1}
    srt = P.sorted_rows(name)
    seg = P.segment_sizes(srt, True)
    assert all(seg_class(seg[h], c.mc) == cls for h in c.hubs)
    supported = {(p["read"], p["pos"]) for p in c.probes if p["supported"]}
    where = defaultdict(set)                               # (side, strand, op count) -> parts of the op list with a supported X
    shapes = set()
    for f in P.selected_rows(srt, True):
        ops = F.cigar_ops(f[-1])
        n = len(ops)
        side, hub_read = ("t", f[5]) if f[5] in c.hubs else ("q", f[0])
        for i, tk, qk in x_keys_of_row(f, True):
            if (hub_read, tk if side == "t" else qk) in supported:
                part = "last" if i == n - 1 else "cached" if i < CACHE else "tail"
                where[side, f[4], n].add(part)
            if ops[i][0] > 1:
                shapes.add("run")
            if i and ops[i - 1][1] in "ID" or i + 1 < n and ops[i + 1][1] in "ID":
                shapes.add(("gap", f[4], ops[i - 1][1] if i and ops[i - 1][1] in "ID" else ops[i + 1][1]))
            if i and ops[i - 1][1] == "X":
                shapes.add("adjacent")
    for side in "qt":
        for n in want_ops:
            got = where[side, "+", n] | where[side, "-", n]
            assert "cached" in got and "last" in got, (side, n, got)
            if cls == 1 and n > CACHE + 2:
                assert "tail" in got, (side, n)
            if cls == 1 and n == CACHE + 1:
                assert "last" in where[side, "+", n] | where[side, "-", n]      # the one uncached op is a supported X
    assert {"run", "adjacent"} <= shapes
    assert {("gap", s, g) for s in "+-" for g in "ID"} <= shapes


# ---- deep positions, the row cap --------------------------------------------------------------------------------------
def test_deep_input_overflows_eight_bits_and_has_one_large_start_counter():
    c = P.get("deep")
    snp, partners, intervals = pile("deep")
    assert snp["all300", 2000] == 300 > 255 and spanning(intervals, "all300", 2000) == 300
    assert snp["sup300", 2000] == 300 and spanning(intervals, "sup300", 2000) == 300 + c.mc
    assert snp["low300", 2000] == 300 and spanning(intervals, "low300", 2000) == 300 + c.mc - 1
    got = P.counts("deep")
    assert sum(1 for (a, b), v in got.items() if "sup300" in (a, b) and v >= 1) >= 300
    starts = [s for s, e in intervals["start5000"]]
    assert len(starts) == 5000 and set(starts) == {100}


@pytest.mark.parametrize("n", [0, 1])
def test_cap_inputs_have_exactly_the_row_cap_and_one_more(n):
    name = P.CAP_NAMES[n]
    seg = P.segment_sizes(P.sorted_rows(name), True)        # from the oracle's row selection
    assert max(seg.values()) == seg["deep"] == CAP + n
    assert sorted(seg.values())[-2] == 1                     # every other read: one row
    snp, partners, intervals = pile(name)
    assert {s for s, e in intervals["deep"]} == {0}          # a start counter of CAP (+ 1) at position 1
    assert max(v for (r, p), v in snp.items() if r == "deep") == CAP + n - 1 < 1 << 16     # the "lowspan" key: all rows but mc - 1


# ---- row selection -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rowsel", "rowsel_short"])
def test_row_selection_input(name):
    c = P.get(name)
    long_mode = c.long_mode
    srt = list(P.sorted_rows(name))
    sel = ["\t".join(f) for f in P.selected_rows(srt, long_mode)]
    back, first = c.info["back"], c.lines[:c.info["first_block"]]
    assert len(back) == 11
    for b in back:
        f = b.split("\t")
        twin = [l for l in first if l.split("\t")[0] == f[5] and l.split("\t")[5] == "T"]
        assert len(twin) == 1                                                       # same pair, other direction ...
        assert c.lines.index(b) // F.WINDOW > c.lines.index(twin[0]) // F.WINDOW    # ... in a later window
        assert twin[0] in srt and b in srt                                          # both pass the window filter
        assert srt.index(b) < srt.index(twin[0])                                    # the later row of the file is first
        assert {k for _, k, _ in x_keys_of_row(twin[0].split("\t"), True)}.isdisjoint({k for _, _, k in x_keys_of_row(f, True)})
        if long_mode:
            assert b in sel and twin[0] not in sel
        else:
            assert b in sel and twin[0] in sel
    star = [l for l in c.lines if l.endswith("\tcg:Z:*")]
    assert len(star) == 1 and star[0] in sel                                        # no ops, but selected: an interval
    assert c.info["nox"] in sel and not x_keys_of_row(c.info["nox"].split("\t"), True)
    assert sum(1 for l in c.lines if l.split("\t")[0] == l.split("\t")[5]) == 1     # the self row
    assert {l.split("\t")[6] for l in c.lines if l.split("\t")[5] == "T"} == {"12000", "20000"}   # two stated lengths
    snp, partners, intervals = F.snp_pileup(srt, long_mode)
    assert snp["T", 16000] >= 2 and 16000 > 12000 and 16000 // TILE == 1
    if long_mode:
        assert sum(1 for l in c.lines if l.endswith("\t*")) == 1
        assert not [l for l in sel if l.endswith("\t*")]
        sides = {("t" if f.split("\t")[5] == "T" else "q") for f in sel if "T" in (f.split("\t")[0], f.split("\t")[5])}
        assert sides == {"t", "q"}                              # T's segment mixes target-side and query-side rows


# ---- the mixes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix1", "mix2", "mix3_short"])
def test_mixes_hold_every_class_several_tiles_and_spills_in_one_call(name):
    c = P.get(name)
    srt = P.sorted_rows(name)
    seg = P.segment_sizes(srt, c.long_mode)
    mc = 2
    assert {seg_class(seg[h], mc) for h in c.hubs} == {0, 1, 2} or not c.long_mode
    assert {seg_class(n, mc) for n in seg.values()} == {0, 1, 2}
    assert any(d["len"] + 2 > 2 * TILE for d in c.hubs.values()) and any(d["len"] + 2 <= TILE for d in c.hubs.values())
    light_spill = [h for h, d in c.hubs.items() if seg_class(seg[h], mc) == 1 and max(d["n_ops"]) > CACHE]
    heavy_long = [h for h, d in c.hubs.items() if seg_class(seg[h], mc) == 2 and max(d["n_ops"]) > TRIP]
    assert light_spill and heavy_long
