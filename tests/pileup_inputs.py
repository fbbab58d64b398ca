"""Hand-built PAF rows that put the SNP pile-up (filter_stage.hip, a5 + a6) on its internal borders: position tiles,
segment classes, CIGAR caches, counter widths, the row cap and the row selection.  No sequences, no overlapper: the
CIGARs are written directly.  tests/test_pileup_inputs.py proves from the oracle alone that every input has the property
it is named for; tests/test_gpu_pileup_edges.py runs them through the GPU chain.

Input model.  A *hub* is one read (target side "t" or query side "q") with N rows to N distinct small reads, each small
read contained whole in its row (overhang 0: the row passes the v4 window filter and pass 2).  Depth comes from distinct
small reads because the window filter caps a QUERY at 60 rows per 1000-row window (so a query-side hub has at most 60
rows).  Every row states the same columns 10 and 11 (M): pass 2 keeps a long-mode pair iff count / M <= thre, so the chain
run at thre = (c + 0.5) / M for c = 0 .. Cmax pins every pair's supported-key count exactly.

The constants below are the ones the inputs were designed around.  They are NOT what the CPU test checks against: it
reads the kernels' constants from the source text, so retuning a kernel makes that test fail instead of moving the inputs
off their edges silently.
"""
from __future__ import annotations

import functools
import os
import random
import re
from collections import defaultdict

from oracle import filters as F

M = 10000                  # columns 10 and 11 of every row
TILE = 15360               # positions per pile-up pass
LIGHT_ROWS = 16            # largest light segment
LIGHT_CACHE = 384          # CIGAR ops of a row the light kernel keeps in registers
HEAVY_TRIP = 256           # CIGAR ops per trip of the heavy kernel's walk
MAX_ROWS = 60000           # deepest segment the LDS pile-up takes
MAX_THRESHOLDS = 48

HIP_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hylight_amd", "csrc", "filter_stage.hip")


def kernel_constants(text=None):
    """The pile-up's constants as filter_stage.hip states them."""
    if text is None:
        with open(HIP_SOURCE) as f:
            text = f.read()

    def one(pattern):
        m = re.findall(pattern, text)
        assert len(set(m)) == 1, (pattern, m)
        return int(m[0])

    return dict(tile=one(r"constexpr int PILE_TILE = (\d+);"),
                light_rows=one(r"constexpr int PILE_LIGHT_ROWS = (\d+);"),
                light_cache=one(r"PILE_LIGHT_IT = (\d+);") * one(r"r\.cig_n > (\d+)u \* PILE_LIGHT_IT"),
                heavy_trip=one(r"k0 < r\.cig_n; k0 \+= (\d+)\) \{\s*uint32_t opv\[4\];"),
                max_rows=one(r"constexpr uint32_t PILE_MAX_ROWS = (\d+);"))


class Case:
    def __init__(self, name, long_mode, mc):
        self.name, self.long_mode = name, long_mode
        self.mcs = (mc,) if isinstance(mc, int) else tuple(mc)    # short mode varies mc instead of thre
        self.mc = self.mcs[0] if long_mode else None
        self.lines = []
        self.probes = []          # dict(read, pos, v, further, supported, kind): what the definitions must give
        self.hubs = {}            # hub read -> dict(side, rows, n_ops=[...], ivs=[(s, e)], len)
        self.n_unfiltered = 0     # rows the v4 window filter drops on purpose (self rows)
        self.rnd = random.Random(name)
        self.info = {}

    def text(self):
        return "\n".join(self.lines) + "\n"


# ---------------------------------------------------------------------------------------------------------------------
# CIGARs in "walk space": '=' and 'X' advance both reads, 'G' is a gap that consumes the hub read only, 'H' one that
# consumes the small read only (hub = target: G is D, H is I; hub = query: G is I, H is D)
# ---------------------------------------------------------------------------------------------------------------------
def walk_ops(L, marks, n_ops, rnd, zero_x=False):
    """Ops over L hub-read bases with X runs (w, r): r bases ending at walk offset w; padded to n_ops ops with gaps
    (often right next to another op, so I and D end up beside X runs)."""
    ops, pos = ([[0, "X"]] if zero_x else []), 0
    for w, r in sorted(marks):
        assert w - r >= pos and w <= L, (L, marks)
        if w - r > pos:
            ops.append([w - r - pos, "="])
        ops.append([r, "X"])
        pos = w
    if L > pos:
        ops.append([L - pos, "="])
    while n_ops is not None and len(ops) < n_ops:
        cand = [i for i, (n, o) in enumerate(ops) if o == "=" and n >= 3]
        assert cand, "hub interval too short for the op count"
        i = rnd.choice(cand)
        n = ops[i][0]
        gap = rnd.choice("GH")
        how = rnd.choice(("front", "back")) if len(ops) + 1 == n_ops else rnd.choice(("front", "back", "mid", "mid", "mid"))
        eq = n - 1 if gap == "G" else n            # G takes one hub base out of the '=' run
        if how == "front":
            ops[i:i + 1] = [[1, gap], [eq, "="]]
        elif how == "back":
            ops[i:i + 1] = [[eq, "="], [1, gap]]
        else:
            a = rnd.randint(1, eq - 1)
            ops[i:i + 1] = [[a, "="], [1, gap], [eq - a, "="]]
    assert n_ops is None or len(ops) == n_ops, (len(ops), n_ops)
    assert sum(n for n, o in ops if o in "=XG") == L
    return ops


def hub(case, name, rlen, rows, probes, mc, side="t", run_fwd=1):
    """One hub.  rows: dicts with s, e and optionally strand, n_ops, rlen (a different stated length), zero_x, star
    ("*" or "cg:Z:*": no CIGAR).  probes: (position, kind[, run]) on the hub read:
        sup      exactly mc further spanning rows: v = span - mc              (supported)
        mc       exactly mc supporters, the other spanning rows further       (supported)
        lowv     mc - 1 supporters                                            (not supported)
        lowspan  one supporter too many: mc - 1 further spanning rows         (not supported)
        end      every row ENDING at the position carries the X as its last op
        all      every spanning row carries it: no further row                (not supported)
    Where the rows spanning a position are too few for the kind, the probe falls back to what is possible; the record in
    case.probes is what was built, computed from the intervals by the definition."""
    rnd = case.rnd
    n = len(rows)
    for r in rows:
        r.setdefault("strand", rnd.choice("+-"))
        r.setdefault("marks", [])
        r["last"] = r["s"]                                  # hub bases below this are taken by earlier marks
    ok = {i for i in range(n) if not rows[i].get("star")}
    for pr in sorted(probes):
        P, kind = pr[0], pr[1]
        run = pr[2] if len(pr) > 2 else run_fwd
        span = [i for i in range(n) if rows[i]["s"] < P < rows[i]["e"]]
        free = [i for i in span if i in ok and P - 1 >= rows[i]["last"]]
        if kind == "end":
            sup = [i for i in sorted(ok) if rows[i]["e"] == P and P - 1 >= rows[i]["last"]]
        else:
            want = {"sup": len(span) - mc, "mc": mc, "lowv": mc - 1, "lowspan": len(span) - mc + 1, "all": len(span)}[kind]
            if kind in ("sup", "mc") and len(span) < 2 * mc:
                want = mc
            if kind == "lowspan" and want < mc:
                want = mc
            want = max(0, min(want, len(free)))
            sup = rnd.sample(free, want)
        if not sup:
            continue
        for i in sup:
            r = rows[i]
            fwd = side == "t" or r["strand"] == "+"
            k = run if fwd and P - run >= r["last"] else 1
            r["marks"].append((P, k))
            r["last"] = P
        v = len(sup)
        further = len(span) - v                              # slr2:394 (negative where supporters END at the key)
        case.probes.append(dict(read=name, pos=P, v=v, further=further, supported=v >= mc and further >= mc, kind=kind, side=side))
    n_ops = []
    for i, r in enumerate(rows):
        s, e, L = r["s"], r["e"], r["e"] - r["s"]
        small = f"{name}.{i}"
        fwd = side == "t" or r["strand"] == "+"
        if r.get("star"):
            ol, last = L, r["star"]
            n_ops.append(0)
        else:
            marks = [((P - s) if fwd else (e - P + 1), k) for P, k in r["marks"]]
            ops = walk_ops(L, marks, r.get("n_ops"), rnd, zero_x=r.get("zero_x", False))
            ol = sum(k for k, o in ops if o in "=XH")
            letter = {"=": "=", "X": "X", "G": "D" if side == "t" else "I", "H": "I" if side == "t" else "D"}
            last = "cg:Z:" + "".join(f"{k}{letter[o]}" for k, o in ops)
            n_ops.append(len(ops))
            if r.get("zero_x"):                             # the key a 0-length X gives: position before the first base walked
                case.probes.append(dict(read=name, pos=(e + 1) if not fwd else s, v=None, further=None, supported=False,
                                        kind="zero_x", side=side))
        rl = r.get("rlen", rlen)
        if side == "t":
            case.lines.append(f"{small}\t{ol}\t0\t{ol}\t{r['strand']}\t{name}\t{rl}\t{s}\t{e}\t{M}\t{M}\t0\t{last}")
        else:
            case.lines.append(f"{name}\t{rl}\t{s}\t{e}\t{r['strand']}\t{small}\t{ol}\t0\t{ol}\t{M}\t{M}\t0\t{last}")
    case.hubs[name] = dict(side=side, rows=n, n_ops=n_ops, ivs=[(r["s"], r["e"]) for r in rows],
                           len=max(r.get("rlen", rlen) for r in rows), strands=[r["strand"] for r in rows])


# ---------------------------------------------------------------------------------------------------------------------
# tile borders
# ---------------------------------------------------------------------------------------------------------------------
def tile_starts(rlen):
    return list(range(TILE, rlen + 2, TILE))


def _tile_hub(case, name, rlen, mc, heavy, phase, side):
    rows = [dict(s=0, e=rlen) for _ in range(2 * mc)]
    if len(tile_starts(rlen)) < 3:                          # (the seven-tile light hub is 16 rows without these)
        rows += [dict(s=1, e=rlen), dict(s=0, e=rlen - 1), dict(s=2, e=rlen - 2)]
    for j, t0 in enumerate(tile_starts(rlen)):
        far = max(0, t0 - 2 * TILE - 7)                    # begins two tiles earlier where the read has them
        for e in ([t0, t0 + 1] if heavy else [t0 + (j + phase) % 2]):
            if e <= rlen:
                rows.append(dict(s=far, e=e))
        for s in ([t0 - 1, t0, t0 + 1] if heavy else [t0 - 1 + (j + phase) % 3]):
            e = min(rlen, s + 2 * TILE + 11)                # ends two tiles later where the read has them
            if e - s >= 1:
                rows.append(dict(s=s, e=e))
    for i in range(max(0, LIGHT_ROWS + 2 - len(rows)) if heavy else 0):      # (few tiles: not yet a heavy segment)
        rows.append(dict(s=3 + i, e=rlen - 3 - 2 * i))
    if side == "q":
        # on the minus strand the query key is qlen - pos + 1: a 0-length X first on a row that ends at qlen gives
        # qlen + 1, the one key beyond the read's last base (the reason a read has read_len + 2 positions)
        rows[0].update(strand="-", zero_x=True)
        rows[1].update(strand="-", zero_x=True)
        rows[2].update(strand="+")
    kinds = ("sup", "lowspan", "mc")
    probes = {1: "sup", rlen: "end", rlen - 1: "sup", rlen - 2: "lowspan", rlen - 4: "mc"}
    for j, t0 in enumerate(tile_starts(rlen)):
        for d in (-1, 0, 1):
            if 1 <= t0 + d <= rlen:
                probes.setdefault(t0 + d, kinds[(j + phase + d) % 3])
        if t0 + 3 <= rlen:
            probes.setdefault(t0 + 3, "lowv")
    hub(case, name, rlen, rows, sorted(probes.items()), mc, side)


@functools.lru_cache(maxsize=None)
def tiles(rlen, long_mode=True):
    c = Case(f"tiles_{rlen}" + ("" if long_mode else "_short"), long_mode, 2 if long_mode else (1, 2, 3))
    sides = ("q", "t") if long_mode else ("t",)           # query hubs first: at most 60 rows per query and window
    for side in sides:
        for heavy in (False, True):
            for phase in (0, 1, 2):
                _tile_hub(c, f"{side}{'H' if heavy else 'L'}{phase}", rlen, 2, heavy, phase, side)
    c.info["rlen"] = rlen
    return c


TILE_LENGTHS = (15357, 15358, 15359, 15360, 15361, 30719, 30720, 30721, 100000)


# ---------------------------------------------------------------------------------------------------------------------
# segment classes
# ---------------------------------------------------------------------------------------------------------------------
def class_sizes(mc):
    return sorted({2 * mc - 1, 2 * mc, 15, 16, 17})


@functools.lru_cache(maxsize=None)
def classes(mc):
    """Per hub size n: rows 0 .. 2mc-2 span the whole read, row 2mc-1 ends at 2000, the others at 1000: positions below
    1000 are spanned by n rows, 1000..2000 by min(n, 2 mc), above by min(n, 2 mc - 1)."""
    c = Case(f"classes_mc{mc}", True, mc)
    for n in class_sizes(mc):
        for side in ("q", "t"):
            rows = [dict(s=0, e=3000 if i < 2 * mc - 1 else 2000 if i == 2 * mc - 1 else 1000) for i in range(n)]
            probes = [(1500, "mc"), (1600, "lowv"), (2500, "lowspan"), (500, "sup"), (600, "lowspan"), (700, "lowv"),
                      (1000, "sup"), (2000, "sup"), (1001, "mc"), (2001, "mc")]
            hub(c, f"{side}{n}", 3000, rows, probes, mc, side)
    return c


CLASS_MCS = (1, 2, 3, 8, 9)


# ---------------------------------------------------------------------------------------------------------------------
# CIGAR lengths
# ---------------------------------------------------------------------------------------------------------------------
LIGHT_OPS = (383, 384, 385, 448, 1000)
HEAVY_OPS = (63, 64, 65, 255, 256, 257, 513)


def _cigar_hub(case, name, op_counts, per, side, mc):
    rows = []
    for g, k in enumerate(op_counts):                       # group g: `per` rows of k ops that end together at e_g
        for j in range(per):
            rows.append(dict(s=0, e=6000 + 100 * g, n_ops=k, strand="+-"[(g + j) % 2]))
    n_wide = mc + 2
    rows += [dict(s=0, e=9000) for _ in range(n_wide)]
    probes = [(50, "mc", 3), (51, "sup"), (52, "lowspan"), (60, "mc", 2), (61, "mc"), (62, "mc", 1), (300, "lowv", 2)]
    probes += [(p, "mc", 1 + p % 3) for p in range(700, 5900, 260)]
    for g in range(len(op_counts)):
        e = 6000 + 100 * g
        probes += [(e - 3, "mc"), (e, "end", 2)]             # the last op but two, and the very last op
    hub(case, name, 9000, rows, probes, mc, side)


@functools.lru_cache(maxsize=None)
def cigar_light():
    c = Case("cigar_light", True, 2)
    for side in ("q", "t"):
        _cigar_hub(c, f"{side}A", LIGHT_OPS, 2, side, 2)      # 10 + 4 = 14 rows: light
        _cigar_hub(c, f"{side}B", LIGHT_OPS[::-1], 2, side, 2)
    return c


@functools.lru_cache(maxsize=None)
def cigar_heavy():
    c = Case("cigar_heavy", True, 2)
    for side in ("q", "t"):
        _cigar_hub(c, f"{side}A", HEAVY_OPS, 3, side, 2)      # 21 + 4 = 25 rows: heavy
        _cigar_hub(c, f"{side}B", HEAVY_OPS[::-1] + (1000,), 2, side, 2)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# deep positions, the row cap
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep(long_mode=True):
    mc = 2
    c = Case("deep" + ("" if long_mode else "_short"), long_mode, mc if long_mode else (1, 2, 3))
    # 300 rows with an X at one position: more than an 8-bit counter holds.  v = coverage: not supported
    hub(c, "all300", 4000, [dict(s=0, e=4000) for _ in range(300)], [(2000, "all"), (2100, "mc"), (2101, "lowv")], mc)
    # ... plus mc rows without it: supported; plus mc - 1: not
    hub(c, "sup300", 4000, [dict(s=0, e=4000) for _ in range(300 + mc)], [(2000, "sup"), (2100, "mc")], mc)
    hub(c, "low300", 4000, [dict(s=0, e=4000) for _ in range(300 + mc - 1)], [(2000, "lowspan"), (2100, "mc")], mc)
    # 5000 rows that begin at the same base: one large start counter (and two large end counters)
    rows = [dict(s=100, e=3000 if i % 2 else 3001 + i % 7) for i in range(5000)]
    hub(c, "start5000", 4000, rows, [(101, "mc"), (102, "lowv"), (2999, "mc"), (3000, "end"), (3001, "mc"), (3004, "lowspan"),
                                    (3007, "all"), (1500, "sup")], mc)
    return c


@functools.lru_cache(maxsize=None)
def cap(n_rows):
    """One hub of n_rows rows that all begin at base 0 (a start counter of n_rows: what the 16-bit counters must hold)."""
    mc = 2
    c = Case(f"cap_{n_rows}", True, mc)
    rows = [dict(s=0, e=1200 + i % 5, strand="+-"[i & 1]) for i in range(n_rows)]
    hub(c, "deep", 1300, rows, [(1, "sup"), (600, "mc"), (601, "lowv"), (700, "lowspan"), (1200, "mc"), (1201, "sup"),
                                (1202, "mc"), (1203, "mc")], mc)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# row selection
# ---------------------------------------------------------------------------------------------------------------------
def _filler(case, name, n):
    hub(case, name, 500, [dict(s=0, e=400) for _ in range(n)], [(100, "mc"), (200, "sup")], 2)


@functools.lru_cache(maxsize=None)
def rowsel(long_mode=True):
    """Window 1: a hub T with 20 rows; among them a self row, a "*" row (long mode only), a cg:Z:* row, a pair without X,
    two rows that state a longer T.  After more than 1000 filler rows: the pairs of T's first rows again, in the other
    direction (T as the query) and with X at other positions.  Long mode piles the first row of a pair in the intermediate
    order (target length first: the row with the small read as target), short mode every row."""
    mc = 2
    c = Case("rowsel" + ("" if long_mode else "_short"), long_mode, mc if long_mode else (1, 2, 3))
    rows = [dict(s=0, e=12000) for _ in range(16)]
    rows[4]["star"] = "cg:Z:*"                              # no ops, but an interval and the pair's first-row slot
    if long_mode:
        rows[5]["star"] = "*"                               # (short mode: the oracle is handed lines without their newline and
                                                            # so cannot restate slr2:253, which compares the unstripped field)
    rows += [dict(s=11000, e=19000, rlen=20000) for _ in range(2)] + [dict(s=10000, e=19500, rlen=20000) for _ in range(2)]
    probes = [(3000, "sup"), (3001, "lowspan"), (5000, "mc"), (5001, "mc"), (5002, "lowv"),
              (16000, "mc"), (16001, "lowv"), (11500, "mc")]   # 16000: beyond the length most rows state, in the second tile
    hub(c, "T", 12000, rows, probes, mc)
    c.lines.append(f"T\t12000\t0\t12000\t+\tT\t12000\t0\t12000\t{M}\t{M}\t0\tcg:Z:5000=1X6999=")          # self row
    c.n_unfiltered += 1
    nox = len(c.lines)
    c.lines.append(f"nox\t800\t0\t800\t-\tT\t12000\t100\t900\t{M}\t{M}\t0\tcg:Z:800=")                    # a pair with no X
    c.info["first_block"] = len(c.lines)
    _filler(c, "F1", 1100)
    # the other direction, second window onwards: T is the query (so at most 60 such rows), the small reads T.0 .. T.11
    # are targets; X at 7000 .. (T's key; nothing in the first block is there)
    # (a row of either direction has target length 12000 and the interval 0 .. 12000, so the order of a pair's two rows is
    # decided by the text: "T\t" sorts before "T.<i>\t", the LATER row of the file is the pair's first row)
    back = []
    for i in range(12):
        if i == 4:
            continue                                        # the cg:Z:* row stays its pair's only row: it is selected
        ol = int(c.lines[i].split("\t")[1])
        a = 7000 + i // 4
        back.append(f"T\t12000\t0\t{ol}\t+\tT.{i}\t{ol}\t0\t{ol}\t{M}\t{M}\t0\tcg:Z:{a}=1X{ol - a - 1}=")
    c.lines += back
    c.info["back"] = back
    c.info["nox"] = c.lines[nox]
    _filler(c, "F2", 30)
    if long_mode:
        # T's segment holds first-block rows (target side) and second-block rows (query side) of DIFFERENT pairs: what its
        # keys must give is left to the oracle here, the test states the selection instead
        c.probes = [p for p in c.probes if p["read"] != "T"]
    return c


# ---------------------------------------------------------------------------------------------------------------------
# a seeded mix
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mix(seed, long_mode=True):
    mc = 2
    c = Case(f"mix{seed}" + ("" if long_mode else "_short"), long_mode, mc if long_mode else (1, 2, 3))
    rnd = c.rnd
    lens = [TILE - 3, TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 2, 2 * TILE, 3 * TILE + 5, 4000, 9000, 50000]
    depths = [3, 4, 5, 15, 16, 17, 18, 40, 59, 60]
    for h in range(24):
        side = "t" if not long_mode else rnd.choice("tq")
        rlen = rnd.choice(lens)
        n = rnd.choice(depths) if side == "q" else rnd.choice(depths + [130, 400])
        borders = [1, rlen] + [t + d for t in tile_starts(rlen) for d in (-1, 0, 1) if 1 <= t + d <= rlen]
        rows = []
        for _ in range(n):
            a, b = rnd.choice(borders + [rnd.randint(1, rlen)]) - rnd.choice((0, 1)), rnd.choice(borders + [rnd.randint(1, rlen)])
            a, b = min(a, b), max(a, b)
            if rnd.random() < 0.5:
                a = max(0, a - rnd.choice((1, 700, TILE, 2 * TILE)))
            if b - a < 1 or rnd.random() < 0.4:
                a, b = max(0, a - 3000), min(rlen, b + 3000)
            r = dict(s=a, e=b)
            if b - a > 3200 and rnd.random() < 0.5:
                r["n_ops"] = rnd.choice(LIGHT_OPS + HEAVY_OPS)
            rows.append(r)
        pos = sorted(set(rnd.choice(borders + [rnd.randint(1, rlen)]) for _ in range(14)))
        probes = [(p, rnd.choice(("sup", "mc", "mc", "lowv", "lowspan", "end", "all")), rnd.choice((1, 1, 2, 5))) for p in pos]
        hub(c, f"h{h}{side}", rlen, rows, probes, mc, side)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the named inputs
# ---------------------------------------------------------------------------------------------------------------------
BUILDERS = {}
for _l in TILE_LENGTHS:
    BUILDERS[f"tiles_{_l}"] = functools.partial(tiles, _l)
for _mc in CLASS_MCS:
    BUILDERS[f"classes_mc{_mc}"] = functools.partial(classes, _mc)
BUILDERS.update({
    "cigar_light": cigar_light, "cigar_heavy": cigar_heavy, "deep": deep,
    f"cap_{MAX_ROWS}": functools.partial(cap, MAX_ROWS), f"cap_{MAX_ROWS + 1}": functools.partial(cap, MAX_ROWS + 1),
    "rowsel": rowsel, "mix1": functools.partial(mix, 1), "mix2": functools.partial(mix, 2),
    "tiles_15359_short": functools.partial(tiles, 15359, False), "tiles_30720_short": functools.partial(tiles, 30720, False),
    "deep_short": functools.partial(deep, False), "rowsel_short": functools.partial(rowsel, False),
    "mix3_short": functools.partial(mix, 3, False),
})
NAMES = tuple(BUILDERS)
CAP_NAMES = (f"cap_{MAX_ROWS}", f"cap_{MAX_ROWS + 1}")


def get(name):
    return BUILDERS[name]()


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's view of an input
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sorted_rows(name):
    """The rows the pile-up sees: v4 window filter, intermediate order (as F.worker_sweep)."""
    c = get(name)
    return tuple(F.sort_intermediate(F.window_filter(c.lines, variant=4, min_len=30, min_o=3)))


def selected_rows(srt, long_mode):
    """F.snp_pileup's row selection, restated: the rows that enter the pile-up."""
    used, out = set(), []
    for line in srt:
        f = line.split("\t")
        if f[0] == f[5] or f[-1] == "*":
            continue
        if long_mode:
            pk = F.pair_key(f[0], f[5])
            if pk in used:
                continue
            used.add(pk)
        out.append(f)
    return out


def segment_sizes(srt, long_mode):
    """Rows per read as the pile-up kernels count them: every selected row under its target, in long mode also under its
    query."""
    n = defaultdict(int)
    for f in selected_rows(srt, long_mode):
        n[f[5]] += 1
        if long_mode:
            n[f[0]] += 1
    return n


@functools.lru_cache(maxsize=None)
def counts(name, mc=None):
    c = get(name)
    mc = c.mc if mc is None else mc
    got = F.pair_counts_np(list(sorted_rows(name)), c.long_mode, mc)
    if got is None:                                         # (a cg:Z:* row: the definitional path)
        got = dict(F.supported_pair_counts(*F.snp_pileup(sorted_rows(name), c.long_mode), mc))
    return got


def thresholds(name):
    """Long mode: (c + 0.5) / M for every count up to the oracle's largest: a pair with count k is kept exactly from
    c = k on, so any other count differs from the oracle at some threshold.  Short mode: pass 2 does not look at thre."""
    c = get(name)
    if not c.long_mode:
        return [0.0025]
    cmax = max(counts(name).values(), default=0)
    return [(k + 0.5) / M for k in range(cmax + 1)]


def event_statistic(name):
    """What `snp_events` of hlmi_last_stats_json counts in both forms of the pile-up: one event per X op (a run of any
    length, a 0-length one included) of every selected row, counted once per side piled: target and query in long mode,
    target only in short mode.  Self rows, rows the window filter dropped, "*" rows and, in long mode, the later rows of a
    pair have none.  In the oracle's terms: the sum of F.snp_pileup's per-key run counts."""
    c = get(name)
    snp, _, _ = F.snp_pileup(sorted_rows(name), c.long_mode)
    return sum(snp.values())
