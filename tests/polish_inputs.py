"""Inputs of the polisher's tests (hlmi_polish, tests/polish_model.py): hand-built contigs, reads and PAF rows with their
answers written out, generated piles around the kernel's tile and CIGAR-batch edges, and the quality case.

A row is described from the contig's side: where it starts, its CIGAR, and the read's bases in alignment-column order
(`aligned`); build() turns that into the read (reverse-complemented for strand '-', with optional flanks) and the PAF line.
The tile size and the insertion cap are read from the kernel's header, as tests/pileup_inputs.py reads PILE_TILE.
"""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_HEADER = os.path.join(ROOT, "hylight_amd", "csrc", "polish_internal.h")


@functools.lru_cache(maxsize=None)
def kernel_constants():
    text = open(KERNEL_HEADER).read()

    def one(pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])
    return dict(tile=one(r"constexpr int POLISH_TILE = (\d+);"), cap=one(r"constexpr int POLISH_INS_CAP = (\d+);"))


_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(b):
    return b.translate(_RC)[::-1]


def cigar_ops(cigar):
    return [(int(n), o) for n, o in re.findall(r"(\d+)([^\d])", cigar)]


class Case:
    """contigs / reads: [(name, bases)]; rows: PAF lines (bytes, no newline); opts: hlmi_polish_opts fields."""

    def __init__(self, contigs, opts=None):
        self.contigs = [(n.encode() if isinstance(n, str) else n, s) for n, s in contigs]
        self.reads, self.rows, self.opts = [], [], dict(opts or {})
        self.want = None                                   # hand cases: (fasta bytes, stats that are not zero)

    def add(self, ts, cigar, aligned, strand="+", target=None, name=None, left=b"", right=b"", read=None):
        """One read and its row.  `read`: the name of an earlier read to reuse (its bases must fit)."""
        tname = self.contigs[0][0] if target is None else target.encode()
        tlen = len(dict(self.contigs)[tname])
        ops = cigar_ops(cigar)
        t_cols = sum(n for n, o in ops if o in "=XD")
        assert sum(n for n, o in ops if o in "=XI") == len(aligned), (cigar, len(aligned))
        if read is None:
            qname = (name or f"r{len(self.reads)}").encode()
            seq = left + (aligned if strand == "+" else revcomp(aligned)) + right
            self.reads.append((qname, seq))
        else:
            qname = read.encode()
            seq = dict(self.reads)[qname]
        qs = len(left)
        n_eq = sum(n for n, o in ops if o == "=")
        f = [qname, b"%d" % len(seq), b"%d" % qs, b"%d" % (qs + len(aligned)), strand.encode(), tname, b"%d" % tlen, b"%d" % ts,
             b"%d" % (ts + t_cols), b"%d" % n_eq, b"%d" % sum(n for n, _ in ops), b"60", b"cg:Z:" + cigar.encode()]
        self.rows.append(b"\t".join(f))
        return self

    def contigs_bytes(self):
        return b"".join(b">" + n + b"\n" + s + b"\n" for n, s in self.contigs)

    def reads_bytes(self):
        return b"".join(b">" + n + b"\n" + s + b"\n" for n, s in self.reads)

    def paf_bytes(self):
        return b"".join(r + b"\n" for r in self.rows)

    def write(self, d):
        d = os.fspath(d)
        os.makedirs(d, exist_ok=True)
        paths = [os.path.join(d, n) for n in ("contigs.fa", "reads.fa", "rows.paf")]
        for p, b in zip(paths, (self.contigs_bytes(), self.reads_bytes(), self.paf_bytes())):
            with open(p, "wb") as f:
                f.write(b)
        return paths


def _sub(seq, at, base):
    return seq[:at] + base + seq[at + 1:]


def _head(name, ln, rc, xc):
    return b">%s LN:i:%d RC:i:%d XC:f:%s\n" % (name, ln, rc, xc)


def hand_cases():
    """name -> Case with .want = (expected file, expected non-zero stats): each worked by hand from the header's rules."""
    C = {}
    ref = b"ACGTACGTAC"

    # two A and two C on position 4, whose own base is A: the contig's base is among the tied ones and stays
    c = Case([("c", ref)])
    for alt in (b"A", b"A", b"C", b"C"):
        c.add(0, "10=" if alt == b"A" else "4=1X5=", _sub(ref, 4, alt))
    c.want = (_head(b"c", 10, 4, b"1.000000") + ref + b"\n", dict(rows=4, rows_selected=4, contigs=1, contigs_polished=1))
    C["tie_own_among"] = c

    # two G and two C on position 4 (own base A): the first of A C G T among the tied ones, C
    c = Case([("c", ref)])
    for alt in (b"G", b"G", b"C", b"C"):
        c.add(0, "4=1X5=", _sub(ref, 4, alt))
    c.want = (_head(b"c", 10, 4, b"1.000000") + _sub(ref, 4, b"C") + b"\n",
              dict(rows=4, rows_selected=4, contigs=1, contigs_polished=1, substituted=1))
    C["tie_own_not_among"] = c

    # two of three rows delete position 4
    c = Case([("c", ref)])
    c.add(0, "10=", ref).add(0, "4=1D5=", ref[:4] + ref[5:]).add(0, "4=1D5=", ref[:4] + ref[5:])
    c.want = (_head(b"c", 9, 3, b"1.000000") + ref[:4] + ref[5:] + b"\n",
              dict(rows=3, rows_selected=3, contigs=1, contigs_polished=1, deleted=1))
    C["del_wins"] = c

    # two del and two T on position 4 (own base A): T comes before del
    c = Case([("c", ref)])
    c.add(0, "4=1D5=", ref[:4] + ref[5:]).add(0, "4=1D5=", ref[:4] + ref[5:])
    c.add(0, "4=1X5=", _sub(ref, 4, b"T")).add(0, "4=1X5=", _sub(ref, 4, b"T"))
    c.want = (_head(b"c", 10, 4, b"1.000000") + _sub(ref, 4, b"T") + b"\n",
              dict(rows=4, rows_selected=4, contigs=1, contigs_polished=1, substituted=1))
    C["tie_base_before_del"] = c

    # coverage 3 on [0, 4), 2 behind: T on position 2 is taken, T on position 5 is not; lower case goes where a position is
    # decided (1) and stays where it is not (7)
    low = b"AcGTACGtAC"
    c = Case([("c", low)])
    full = _sub(_sub(low.upper(), 2, b"T"), 5, b"T")
    c.add(0, "2=1X2=1X4=", full).add(0, "2=1X2=1X4=", full).add(0, "2=1X1=", full[:4])
    c.want = (_head(b"c", 10, 3, b"0.400000") + b"ACTTACGtAC\n",
              dict(rows=3, rows_selected=3, contigs=1, contigs_polished=1, substituted=1))
    C["coverage_edge"] = c

    # slot 4: four rows span, two insert (2 i = s): shut.  slot 8: three rows span (the fourth ends at 7), two insert: open
    ref12 = b"ACGTACGTACGT"
    c = Case([("c", ref12)])
    ins = ref12[:4] + b"T" + ref12[4:8] + b"G" + ref12[8:]
    c.add(0, "4=1I4=1I4=", ins).add(0, "4=1I4=1I4=", ins).add(0, "12=", ref12).add(0, "7=", ref12[:7])
    c.want = (_head(b"c", 13, 4, b"1.000000") + ref12[:8] + b"G" + ref12[8:] + b"\n",
              dict(rows=4, rows_selected=4, contigs=1, contigs_polished=1, slots_opened=1, inserted_bases=1))
    C["slot_majority"] = c

    # slot 5: two rows insert A, two insert CC: the smaller length, 1.  slot 8: G and C once each over three rows: C
    c = Case([("c", ref12)])
    for a, b in ((b"A", b"G"), (b"A", b"C"), (b"CC", b"")):
        c.add(0, f"5={len(a)}I3={len(b)}I4=".replace("0I", ""), ref12[:5] + a + ref12[5:8] + b + ref12[8:])
    c.add(0, "5=2I2=", ref12[:5] + b"CC" + ref12[5:7])
    c.want = (_head(b"c", 14, 4, b"1.000000") + ref12[:5] + b"A" + ref12[5:8] + b"C" + ref12[8:] + b"\n",
              dict(rows=4, rows_selected=4, contigs=1, contigs_polished=1, slots_opened=2, inserted_bases=2))
    C["slot_length_and_base_ties"] = c

    # 16 inserted bases are a vote, 17 are not (the row still spans)
    cap = kernel_constants()["cap"]
    i16, i17 = b"ACGGTTCAACGGTTCA"[:cap].ljust(cap, b"A"), b"T" * (cap + 1)
    c = Case([("c", ref)])
    for _ in range(3):
        c.add(0, f"3={cap}I4={cap + 1}I3=", ref[:3] + i16 + ref[3:7] + i17 + ref[7:])
    c.want = (_head(b"c", 10 + cap, 3, b"1.000000") + ref[:3] + i16 + ref[3:] + b"\n",
              dict(rows=3, rows_selected=3, contigs=1, contigs_polished=1, slots_opened=1, inserted_bases=cap, ins_long=3))
    C["insertion_cap"] = c

    # 2I 1I in front of position 3 are one insertion of three bases, the D takes position 3, 2I opens the slot behind it
    ref8 = b"ACGTACGT"
    c = Case([("c", ref8)])
    for _ in range(3):
        c.add(0, "3=2I1I1D2I4=", ref8[:3] + b"TTG" + b"CA" + ref8[4:])
    c.want = (_head(b"c", 12, 3, b"1.000000") + ref8[:3] + b"TTGCA" + ref8[4:] + b"\n",
              dict(rows=3, rows_selected=3, contigs=1, contigs_polished=1, slots_opened=2, inserted_bases=5, deleted=1))
    C["two_insertions_around_a_deletion"] = c

    # I at the very start (also on a row that starts inside the contig) and at the very end: no slot
    c = Case([("c", ref)])
    c.add(0, "2I10=", b"GG" + ref).add(2, "1I1I8=", b"TT" + ref[2:]).add(0, "10=3I", ref + b"CCC").add(0, "6=2I", ref[:6] + b"AA")
    c.want = (_head(b"c", 10, 4, b"1.000000") + ref + b"\n",
              dict(rows=4, rows_selected=4, contigs=1, contigs_polished=1, ins_edge=5))
    C["insertion_at_cigar_ends"] = c

    # strand '-': the read holds the reverse complement, with flanks outside [qs, qe)
    c = Case([("c", ref)])
    alt = ref[:2] + b"A" + ref[2:4] + b"C" + ref[5:]                  # 2= 1I 2= 1X 5=
    for k in range(3):
        c.add(0, "2=1I2=1X5=", alt, strand="-", left=b"GGA"[:k], right=b"TTTT")
    c.want = (_head(b"c", 11, 3, b"1.000000") + alt + b"\n",
              dict(rows=3, rows_selected=3, contigs=1, contigs_polished=1, slots_opened=1, inserted_bases=1, substituted=1))
    C["reverse_strand"] = c

    # N in a read does not vote (position 1 falls to two votes and stays, lower case kept); lower-case read bases vote;
    # an N of the contig under three A becomes A; an insertion of N alone is written as N
    refn = b"AcGTNCGTAC"
    c = Case([("c", refn)])
    c.add(0, "4=1X1I5=", b"ANGTANCGTAC").add(0, "4=1X1I5=", b"acgtancgtac").add(0, "4=1X1I5=", b"ACGTANCGTAC", strand="-")
    c.want = (_head(b"c", 11, 3, b"0.900000") + b"AcGTANCGTAC\n",
              dict(rows=3, rows_selected=3, contigs=1, contigs_polished=1, substituted=1, slots_opened=1, inserted_bases=1))
    C["n_and_lower_case"] = c

    # one row per read (min_cov 1): r0's two rows cover six bases each and the earlier line stays (T on 2, not on 6); r1's
    # later row covers five bases, its earlier one four: the longer stays (G on 9, not C G T A on 6..9); a row of the contig
    # against itself is skipped
    c = Case([("c", ref)], opts=dict(min_cov=1))
    c.add(0, "2=1X3=", b"ACTTAC", name="r0", right=ref[6:])
    c.add(4, "2=1X3=", b"ACTTAC", read="r0")
    c.add(6, "4X", b"CGTA", name="r1", right=b"G")
    c.add(5, "4=1X", b"CGTAG", read="r1")
    c.reads.append((b"c", ref))
    c.add(0, "10=", ref, read="c")
    c.want = (_head(b"c", 10, 2, b"1.000000") + b"ACTTACGTAG\n",
              dict(rows=5, rows_selected=2, contigs=1, contigs_polished=1, substituted=2))
    C["one_row_per_read"] = c

    # opened slots at T - 1, T and T + 1, T the count kernel's tile: three rows over [T - 200, T + 200), one that ends on the
    # border (it spans slot T - 1, not T) and one that starts on it (it spans slot T + 1, not T); every spanning row inserts
    T = kernel_constants()["tile"]
    rng = np.random.default_rng(9)
    seq = random_contig(rng, 2 * T + 1, lower=0, n_frac=0)
    planted = {T - 1: ("I", b"GA"), T: ("I", b"C"), T + 1: ("I", b"TT")}
    c = Case([("c", seq)])
    for a, b in ((T - 200, T + 200),) * 3 + ((T - 200, T), (T, T + 200)):
        c.add(a, *_mutate(rng, seq[a:b], planted, a, 0.0, 0.0, take=1.0), strand="+-"[a % 2])
    c.want = (_head(b"c", 2 * T + 6, 5, b"%.6f" % (400 / (2 * T + 1))) + seq[:T - 1] + b"GA" + seq[T - 1:T] + b"C" + seq[T:T + 1] + b"TT"
              + seq[T + 1:] + b"\n", dict(rows=5, rows_selected=5, contigs=1, contigs_polished=1, slots_opened=3, inserted_bases=5))
    C["slots_on_the_tile_border"] = c
    return C


def refusal_cases():
    """name -> (Case, 1-based line that must be named): a valid pile of three rows with row 2 broken one way at a time."""
    ref = b"ACGTACGTAC"

    def base():
        c = Case([("c", ref)])
        for _ in range(3):
            c.add(0, "4=1X5=", _sub(ref, 4, b"G"), right=b"TT")
        return c
    out = {}
    edits = {
        "no_cigar_tag": lambda f: f[:12] + [b"NM:i:1"],
        "eleven_columns": lambda f: f[:11],
        "op_m": lambda f: f[:12] + [b"cg:Z:10M"],
        "star": lambda f: f[:12] + [b"cg:Z:*"],
        "target_columns": lambda f: f[:12] + [b"cg:Z:4=1X4="],
        "query_columns": lambda f: f[:12] + [b"cg:Z:4=1X5=1I"],
        "target_end_outside": lambda f: f[:7] + [b"1", b"11"] + f[9:],
        "query_end_outside": lambda f: f[:2] + [b"3", b"13"] + f[4:],
        "unknown_query": lambda f: [b"nobody"] + f[1:],
        "unknown_target": lambda f: f[:5] + [b"nothing"] + f[6:],
        "cigar_ends_in_number": lambda f: f[:12] + [b"cg:Z:4=1X5=3"],
    }
    for name, fn in edits.items():
        c = base()
        c.rows[1] = b"\t".join(fn(c.rows[1].split(b"\t")))
        out[name] = (c, 2)
    return out


# ---- generated piles ---------------------------------------------------------------------------------------------------
def _mutate(rng, seg, planted, t0, noise, long_ins, take=0.85):
    """seg = contig[t0 : t0 + n] -> (cigar, aligned): the planted edits (contig position -> edit) taken with probability
    `take` each, random noise besides.  Edits: ("X", base) ("D",) ("I", bases in front of the position)."""
    ops, out = [], bytearray()

    def push(n, o):
        if ops and ops[-1][1] == o:
            ops[-1][0] += n
        else:
            ops.append([n, o])
    for k, b in enumerate(seg):
        e = planted.get(t0 + k)
        if e is not None and rng.random() >= take:
            e = None
        if e is None and rng.random() < noise:
            r = rng.random()
            e = ("X", b"ACGT"[rng.integers(4)]) if r < 0.5 else ("D",) if r < 0.75 else \
                ("I", bytes(b"ACGTN"[rng.integers(5)] for _ in range(int(rng.integers(1, 4)) if rng.random() > long_ins else 18)))
        if e is not None and e[0] == "I" and k > 0:
            out += e[1]
            push(len(e[1]), "I")
            e = None
        if e is None or e[0] == "I":
            out.append(b)
            push(1, "=")
        elif e[0] == "X":
            c = e[1] if e[1] != b else b"ACGT"[(b"ACGT".find(bytes([b]).upper()) + 1) % 4]
            out.append(c)
            push(1, "X" if bytes([c]).upper() != bytes([b]).upper() else "=")
        else:
            push(1, "D")
    return "".join(f"{n}{o}" for n, o in ops), bytes(out)


def random_contig(rng, n, lower=0.02, n_frac=0.005):
    s = bytearray(b"ACGT"[k] for k in rng.integers(0, 4, size=n))
    for k in np.flatnonzero(rng.random(n) < lower):
        s[k] = s[k] | 0x20
    for k in np.flatnonzero(rng.random(n) < n_frac):
        s[k] = 78
    return bytes(s)


def pile_case(seed, lens, starts_ends, planted_at=(), n_random=12, noise=0.01, opts=None):
    """Contigs of the given lengths (c0, c1, ...); on c0 rows over every (start, end) of starts_ends plus n_random random
    ones per contig; planted edits at the positions of planted_at on c0 (insertion, deletion, substitution in turn) and
    at random on all contigs."""
    rng = np.random.default_rng(seed)
    contigs = [(f"c{k}", random_contig(rng, n)) for k, n in enumerate(lens)]
    c = Case(contigs, opts)
    for k, (name, seq) in enumerate(contigs):
        n = len(seq)
        planted = {}
        kinds = [("I", b"GA"), ("D",), ("X", b"T"[0]), ("I", b"C")]
        if k == 0:
            for j, p in enumerate(planted_at):
                if 0 < p < n:
                    planted[p] = kinds[j % 4]
        for p in rng.integers(1, n, size=max(1, n // 150)):
            planted.setdefault(int(p), kinds[int(rng.integers(4))])
        spans = list(starts_ends) if k == 0 else []
        for _ in range(n_random):
            a = int(rng.integers(0, max(1, n - 40)))
            spans.append((a, int(min(n, a + rng.integers(40, max(41, n))))))
        for a, b in spans:
            a, b = max(0, a), min(n, b)
            if b - a < 2:
                continue
            cigar, aligned = _mutate(rng, seq[a:b], planted, a, noise, 0.1)
            if not aligned:
                continue
            c.add(a, cigar, aligned, strand="+-"[int(rng.integers(2))], target=name,
                  left=b"ACGT"[:int(rng.integers(4))], right=b"TG"[:int(rng.integers(3))])
    return c


def tile_cases():
    """Contigs of T - 1, T, T + 1, 2T - 1, 2T + 1 positions; rows that start or end exactly on a tile border; planted edits
    (so opened slots) at T - 1, T, T + 1."""
    T = kernel_constants()["tile"]
    out = {}
    for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
        borders = [(0, T), (T, n), (T - 300, T), (T, T + 300), (T - 1, n), (0, T - 1), (0, T + 1), (T + 1, n), (0, n), (0, n), (0, n),
                   (T - 200, T + 200), (T - 200, T + 200), (T - 200, T + 200), (T - 100, T + 100)]
        out[f"contig_{n}"] = pile_case(1000 + n, [n], borders, planted_at=(T - 1, T, T + 1, T + 2), n_random=6)
    return out


def ops_case(n_ops):
    """Four identical rows of exactly n_ops CIGAR ops (2= 1X 2= 1D 2= 1I ...) on a contig long enough for them, and one
    plain row: the X, D and I of the four win everywhere."""
    rng = np.random.default_rng(77 + n_ops)
    kinds = "XDI"
    ops, need = [], 0
    for k in range(n_ops):
        o = "=" if k % 2 == 0 else kinds[(k // 2) % 3]
        n = 2 if o == "=" else 1
        ops.append((n, o))
        need += n if o != "I" else 0
    seq = random_contig(rng, need + 7, lower=0, n_frac=0)
    aligned, p = bytearray(), 3
    for n, o in ops:
        if o == "=":
            aligned += seq[p:p + n]
        elif o == "X":
            aligned.append(b"ACGT"[(b"ACGT".find(seq[p:p + 1]) + 1) % 4])
        elif o == "I":
            aligned += b"G"
        p += n if o != "I" else 0
    cigar = "".join(f"{n}{o}" for n, o in ops)
    c = Case([("c", seq)])
    for k in range(4):
        c.add(3, cigar, bytes(aligned), strand="+-"[k % 2])
    c.add(0, f"{len(seq)}=", seq)
    return c


def three_contigs_case(include_unpolished):
    c = pile_case(31, [300, 200, 260], [], n_random=5, opts=dict(include_unpolished=include_unpolished))
    c.rows = [r for r in c.rows if r.split(b"\t")[5] != b"c1"]          # the middle contig gets no row
    return c


def no_usable_row_case():
    """Every row is too short for min_len: nothing is selected, the contigs come back as they are."""
    return pile_case(32, [300, 150], [], n_random=4, opts=dict(min_len=100000))


# ---- the quality case --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quality_case():
    """One simulated strain of 30 kb; the contig is the strain with ~300 planted substitutions, 1-base deletions and 1-3-base
    insertions; ~30x reads at the simulator's corrected-read error rates.  -> dict(truth, contig, reads_fa, planted)."""
    from hylight_amd import simulate as S
    reads, strains = S.simulate_reads(seed=4242, n_strains=1, genome_len=30000, n_reads=120, mean_len=8000, min_len=4000,
                                      max_len=14000)
    truth = strains[0].tobytes()
    rng = np.random.default_rng(4243)
    at = np.sort(rng.choice(np.arange(50, len(truth) - 50), size=300, replace=False))
    out, prev, kinds = bytearray(), 0, [0, 0, 0]
    for p in at:
        out += truth[prev:p]
        k = int(rng.integers(3))
        kinds[k] += 1
        if k == 0:                                            # substitution
            out.append(b"ACGT"[(b"ACGT".find(truth[p:p + 1]) + 1 + int(rng.integers(3))) % 4])
        elif k == 2:                                          # 1-3 bases too many, then the base itself
            out += bytes(b"ACGT"[j] for j in rng.integers(0, 4, size=int(rng.integers(1, 4))))
            out.append(truth[p])
        prev = p + 1                                          # (k == 1: the base is missing)
    out += truth[prev:]
    reads_fa = b"".join(b">" + r.name.encode() + b"\n" + r.seq.tobytes() + b"\n" for r in reads)
    return dict(truth=truth, contig=bytes(out), reads_fa=reads_fa, planted=tuple(kinds))
