"""Inputs of the tests of hlmi_polish_q / hlmi_polish_reads_q (tests/polish_qual_model.py): the cases of
tests/polish_inputs.py with a quality string per read.  A row's qualities are given in alignment-column order, like its bases;
QCase turns them into the read's own order (reversed for strand '-', flanks at Q40).  Hand cases carry their answers as
literals; generated piles draw a quality per base from a seeded generator and are judged by the model alone.
"""
import numpy as np

import polish_inputs as PI
import polish_reads_inputs as RI


def Q(*phred):
    return bytes(33 + q for q in phred)


class QCase(PI.Case):
    """PI.Case whose reads are FASTQ records: quals[name] = the read's quality string (None: a FASTA record)."""

    def __init__(self, contigs, opts=None):
        super().__init__(contigs, opts)
        self.quals = {}

    def addq(self, ts, cigar, aligned, qual=None, strand="+", left=b"", right=b"", lq=None, rq=None, **kw):
        n = len(self.reads)
        self.add(ts, cigar, aligned, strand=strand, left=left, right=right, **kw)
        if len(self.reads) > n:
            q = None
            if qual is not None:
                assert len(qual) == len(aligned)
                q = (lq or Q(40) * len(left)) + (qual if strand == "+" else qual[::-1]) + (rq or Q(40) * len(right))
            self.quals[self.reads[-1][0]] = q
        return self

    def reads_bytes(self):
        out = bytearray()
        for n, s in self.reads:
            q = self.quals.get(n)
            out += b">" + n + b"\n" + s + b"\n" if q is None else b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n"
        return bytes(out)


def with_quals(case, seed, choices=(2, 3, 5, 8, 12, 20, 30, 40), opts=None):
    """A PI.Case as a QCase: a quality per read base, drawn from `choices`."""
    rng = np.random.default_rng(seed)
    c = QCase([(n, s) for n, s in case.contigs], {**case.opts, **(opts or dict(qual_weight=1, min_avg_qual=0.0))})
    c.reads, c.rows = list(case.reads), list(case.rows)
    for n, s in c.reads:
        c.quals[n] = bytes(33 + int(q) for q in rng.choice(choices, size=len(s)))
    return c


def _sub(seq, at, base):
    return seq[:at] + base + seq[at + 1:]


def _col(n, default, **at):
    """n quality bytes of Phred `default`, with others at the given columns: _col(10, 40, c4=2)"""
    q = bytearray(Q(default) * n)
    for k, v in at.items():
        q[int(k[1:])] = 33 + v
    return bytes(q)


W = dict(qual_weight=1, min_avg_qual=0.0)


def hand_cases():
    """name -> QCase with .want = (expected file, expected non-zero stats), each worked by hand from the header's rules;
    .plain = the file polish_model gives for the same rows where the case says how the two differ (else None)."""
    C = {}
    ref = b"ACGTACGTAC"
    ref12 = b"ACGTACGTACGT"
    head = PI._head

    def done(name, c, want_seq, plain=None, rc=None, xc=b"1.000000", **stats):
        rc = len(c.rows) if rc is None else rc
        st = dict(rows=len(c.rows), rows_selected=rc, contigs=1, contigs_polished=1,
                  reads_with_qual=sum(q is not None for q in c.quals.values()))
        st.update(stats)
        c.want = (head(b"c", len(want_seq), rc, xc) + want_seq + b"\n", {k: v for k, v in st.items() if v})
        c.plain = None if plain is None else head(b"c", len(plain), rc, xc) + plain + b"\n"
        C[name] = c

    # two G at Q2 against one A at Q40 on position 4 (own base A), min_cov 3: 4 < 40, A stays; by count G wins
    c = QCase([("c", ref)], W)
    c.addq(0, "4=1X5=", _sub(ref, 4, b"G"), _col(10, 40, c4=2)).addq(0, "4=1X5=", _sub(ref, 4, b"G"), _col(10, 40, c4=2))
    c.addq(0, "10=", ref, _col(10, 40))
    done("q2_pair_against_q40", c, ref, plain=_sub(ref, 4, b"G"))

    # A at Q20 against two C at Q10: 20 = 20, the contig's own base is among the tied and stays
    c = QCase([("c", ref)], W)
    c.addq(0, "10=", ref, _col(10, 30, c4=20))
    c.addq(0, "4=1X5=", _sub(ref, 4, b"C"), _col(10, 30, c4=10)).addq(0, "4=1X5=", _sub(ref, 4, b"C"), _col(10, 30, c4=10))
    done("tie_own_among", c, ref, plain=_sub(ref, 4, b"C"))

    # T at Q30, G at Q30, two C at Q15 (own base A): 30 = 30 = 30, the first of A C G T del among them: C
    c = QCase([("c", ref)], W)
    c.addq(0, "4=1X5=", _sub(ref, 4, b"T"), _col(10, 30)).addq(0, "4=1X5=", _sub(ref, 4, b"G"), _col(10, 30))
    c.addq(0, "4=1X5=", _sub(ref, 4, b"C"), _col(10, 30, c4=15)).addq(0, "4=1X5=", _sub(ref, 4, b"C"), _col(10, 30, c4=15))
    done("tie_first_of_acgt", c, _sub(ref, 4, b"C"), plain=_sub(ref, 4, b"C"), substituted=1)

    # 2= 1D 1= 1D 5=: the first D lies between columns 1 and 2 (Q30, Q30): 30; the second between 2 and 3 (Q30, Q5): 5.  Three
    # such rows: del has 90 on position 2 and 15 on position 4; one plain row at Q20: position 2 goes, position 4 stays
    c = QCase([("c", ref)], W)
    for _ in range(3):
        c.addq(0, "2=1D1=1D5=", ref[:2] + ref[3:4] + ref[5:], _col(8, 30, c3=5))
    c.addq(0, "10=", ref, _col(10, 20))
    done("del_lower_flank", c, ref[:2] + ref[3:], plain=ref[:2] + ref[3:4] + ref[5:], deleted=1)

    # a D as the first op (only the column behind it exists: Q3) and as the last (only the one in front: Q25); three rows:
    # 9 and 75 against a plain row's 10 on both positions.  A row of 2D alone has no column at all: its dels weigh 1
    c = QCase([("c", ref)], W)
    for _ in range(3):
        c.addq(0, "1D8=1D", ref[1:9], _col(8, 30, c0=3, c7=25))
    c.addq(0, "10=", ref, _col(10, 10))
    c.addq(4, "2D", b"", b"", left=b"ACGT", lq=Q(40, 40, 40, 40))
    done("del_first_and_last_op", c, ref[:9], plain=ref[1:9], deleted=1)

    # strand '-': the quality string is reversed with the bases.  Column 4 (G, Q2) is read[qe - 1 - 4]; read the other way
    # round it would be column 5's Q40 and the two G would win
    c = QCase([("c", ref)], W)
    for k in range(2):
        c.addq(0, "4=1X5=", _sub(ref, 4, b"G"), _col(10, 40, c4=2), strand="-", left=b"GG", right=b"TTT"[:k + 1])
    c.addq(0, "10=", ref, _col(10, 40))
    done("reverse_strand_low_end", c, ref, plain=_sub(ref, 4, b"G"))

    # slot 5: three rows insert A at Q2 (length 1: 6), two insert CC at (Q30, Q20) (length 2: 20 + 20): CC; by count A
    c = QCase([("c", ref12)], W)
    for _ in range(3):
        c.addq(0, "5=1I7=", ref12[:5] + b"A" + ref12[5:], _col(13, 40, c5=2))
    for _ in range(2):
        c.addq(0, "5=2I7=", ref12[:5] + b"CC" + ref12[5:], _col(14, 40, c5=30, c6=20))
    done("slot_length_by_weight", c, ref12[:5] + b"CC" + ref12[5:], plain=ref12[:5] + b"A" + ref12[5:], slots_opened=1, inserted_bases=2)

    # slot 5, all rows insert two bases: AG (Q10, Q10), CG (Q5, Q30), CN (Q5, Q40): base 0: A 10 = C 10, the first: A (by
    # count C); base 1: G 40, N does not vote.  slot 8: N three times: N
    c = QCase([("c", ref12)], W)
    for ins, q in ((b"AG", (10, 10)), (b"CG", (5, 30)), (b"CN", (5, 40))):
        c.addq(0, "5=2I3=1I4=", ref12[:5] + ins + ref12[5:8] + b"N" + ref12[8:], _col(15, 40, c5=q[0], c6=q[1]))
    done("slot_base_votes_and_all_n", c, ref12[:5] + b"AG" + ref12[5:8] + b"N" + ref12[8:],
         plain=ref12[:5] + b"CG" + ref12[5:8] + b"N" + ref12[8:], slots_opened=2, inserted_bases=3)

    # the floor: r2's ten Phred values add up to 103; at min_avg_qual = 10.3 it stays (three G: decided), one step above it
    # goes (two votes: nothing is decided)
    for name, floor, kept in (("floor_mean_exactly", 103 / 10, True), ("floor_one_step_above_mean", np.nextafter(103 / 10, 100.0), False)):
        c = QCase([("c", ref)], dict(qual_weight=1, min_avg_qual=float(floor)))
        c.addq(0, "4=1X5=", _sub(ref, 4, b"G"), _col(10, 30)).addq(0, "4=1X5=", _sub(ref, 4, b"G"), _col(10, 30))
        c.addq(0, "4=1X5=", _sub(ref, 4, b"G"), _col(10, 10, c9=13))
        if kept:
            done(name, c, _sub(ref, 4, b"G"), substituted=1)
        else:
            done(name, c, ref, rc=2, xc=b"0.000000", rows_low_qual=1)

    # a low read (Q4 throughout) has the longest row of the contig, and a second row: both are dropped and counted, the three
    # shorter rows of other reads are selected as if it were not there
    c = QCase([("c", ref)], dict(qual_weight=1, min_avg_qual=10.0))
    c.addq(0, "10=", ref, _col(10, 4), name="low", right=ref[3:9], rq=Q(4) * 6)
    for _ in range(3):
        c.addq(2, "2=1X4=", _sub(ref, 4, b"G")[2:9], _col(7, 30))
    c.add(3, "6=", ref[3:9], read="low")
    c.rows[-1] = c.rows[-1].replace(b"\t0\t6\t+", b"\t10\t16\t+")          # the second row: the read's right flank
    done("low_read_with_the_longest_row", c, _sub(ref, 4, b"G"), rc=3, xc=b"0.700000", substituted=1, rows_low_qual=2)
    return C


# ---- generated piles ---------------------------------------------------------------------------------------------------
def qpile(seed, n, spans, planted, take=0.6, noise=0.01):
    """One contig of n bases; a row over every (start, end), each taking a planted edit with probability `take`; a quality
    per base from the seeded generator, so that the weights and not the counts decide where the rows disagree."""
    rng = np.random.default_rng(seed)
    seq = PI.random_contig(rng, n, lower=0.01, n_frac=0.002)
    c = QCase([("c", seq)], W)
    for k, (a, b) in enumerate(spans):
        cigar, aligned = PI._mutate(rng, seq[a:b], planted, a, noise, 0.0, take=take)
        qual = bytes(33 + int(q) for q in rng.choice((2, 3, 5, 8, 12, 20, 30, 40), size=len(aligned)))
        c.addq(a, cigar, aligned, qual, strand="+-"[k % 2], left=b"ACG"[:k % 4], right=b"TG"[:k % 3])
    return c


def quals_by_target(cigar, ts, fn):
    """a quality per query column of a row: fn(target position the column stands on - an inserted base: the position behind it)"""
    q, p = bytearray(), ts
    for n, o in PI.cigar_ops(cigar):
        if o in "=X":
            q += bytes(33 + fn(p + j) for j in range(n))
        elif o == "I":
            q += bytes(33 + fn(p) for _ in range(n))
        p += n if o != "I" else 0
    return bytes(q)


def tile_case(kind):
    """Rows around the count kernel's tile border T, four of one mind at Q2 - Q3 near the border against two at Q40.
    "sub_and_slot": the four carry a wrong base on T - 1, T and T + 1 and insert GA, C, TT in front of them; the two carry the
    contig's bases and insert A, GG, C: by count the four win six times, by weight never.  "del_across": the four have a 2D
    over T - 1 and T - its flanking columns stand on T - 2 and T + 1, in two tiles - one of them at Q3, and a 1D on T + 40
    between Q40 flanks: the first stays, the second goes.  A row ends on the border and one starts on it."""
    T = PI.kernel_constants()["tile"]
    rng = np.random.default_rng(501)
    seq = PI.random_contig(rng, 2 * T + 1, lower=0, n_frac=0)
    other = lambda p: b"ACGT"[(b"ACGT".find(seq[p:p + 1]) + 1) % 4]                          # noqa: E731
    if kind == "sub_and_slot":
        three = {T - 1: ("I", b"GA"), T: ("I", b"C"), T + 1: ("I", b"TT")}
        two = {T - 1: ("I", b"A"), T: ("I", b"GG"), T + 1: ("I", b"C")}
        low = lambda p: 2 if T - 2 <= p <= T + 2 else 30                                     # noqa: E731
    else:
        three = {T - 1: ("D",), T: ("D",), T + 40: ("D",)}
        two = {}
        low = lambda p: 3 if p == T - 2 else 40                                              # noqa: E731
    c = QCase([("c", seq)], W)
    a, b = T - 200, T + 200
    for k in range(6):
        cigar, aligned = PI._mutate(rng, seq[a:b], three if k < 4 else two, a, 0.0, 0.0, take=1.0)
        if kind == "sub_and_slot" and k < 4:                 # the wrong bases on T - 1, T, T + 1 (an X each, behind the I)
            al = bytearray(aligned)
            col, p, ops = 0, a, []
            for n, o in PI.cigar_ops(cigar):
                if o == "I":
                    ops.append([n, o])
                    col += n
                    continue
                for j in range(n):
                    x = T - 1 <= p + j <= T + 1
                    if x:
                        al[col + j] = other(p + j)
                    if ops and ops[-1][1] == "=X"[x]:
                        ops[-1][0] += 1
                    else:
                        ops.append([1, "=X"[x]])
                col += n
                p += n
            cigar, aligned = "".join(f"{n}{o}" for n, o in ops), bytes(al)
        c.addq(a, cigar, aligned, quals_by_target(cigar, a, low if k < 4 else (lambda p: 40)), strand="+-"[k % 2], left=b"AC"[:k % 3])
    for a, b in ((T - 200, T), (T, T + 200)):
        c.addq(a, f"{b - a}=", seq[a:b], Q(30) * (b - a), strand="+-"[a % 2])
    return c


def runs_case():
    """Runs of 16, 17 and 70 columns of = and of D (a lane votes up to 16 columns itself, the wave takes longer ones 64 at a
    step), a quality per column; four rows on each strand that disagree on the X columns between the runs."""
    rng = np.random.default_rng(77)
    cigar = "16=1X17=1X70=1X3=16D4=17D4=70D5="
    ops = PI.cigar_ops(cigar)
    need = sum(n for n, o in ops if o != "I")
    seq = PI.random_contig(rng, need + 9, lower=0, n_frac=0)
    c = QCase([("c", seq)], W)
    for k in range(8):
        aligned, p = bytearray(), 4
        for n, o in ops:
            if o == "=":
                aligned += seq[p:p + n]
            elif o == "X":
                aligned.append(b"ACGT"[(b"ACGT".find(seq[p:p + 1]) + 1 + k % 3) % 4])
            p += n
        qual = bytes(33 + int(q) for q in rng.choice((2, 3, 5, 8, 12, 20, 30, 40), size=len(aligned)))
        c.addq(4, cigar, bytes(aligned), qual, strand="+-"[k % 2], left=b"AC"[:k % 3])
    for k in range(5):                               # plain rows: the 16 / 17 / 70 D columns are contested
        qual = bytes(33 + int(q) for q in rng.choice((5, 12, 30, 40), size=len(seq)))
        c.addq(0, f"{len(seq)}=", seq, qual, strand="+-"[k % 2])
    return c


def insertion_case():
    """One slot, min quality at the first and at the last inserted base: two rows insert 16 bases (Q2 first / Q2 last, Q40
    between: 2 + 2), one row inserts one base at Q5 (5), one row 17 bases (it spans): the single base wins; a kernel that
    misses the first or the last base of the minimum gives the 16."""
    cap = PI.kernel_constants()["cap"]
    ref = b"ACGTACGTACGT"
    i16 = b"ACGGTTCAACGGTTCA"[:cap].ljust(cap, b"A")
    c = QCase([("c", ref)], W)
    c.addq(0, f"5={cap}I7=", ref[:5] + i16 + ref[5:], _col(12 + cap, 40, c5=2))
    c.addq(0, f"5={cap}I7=", ref[:5] + i16 + ref[5:], _col(12 + cap, 40, **{f"c{5 + cap - 1}": 2}), strand="-")
    c.addq(0, "5=1I7=", ref[:5] + b"T" + ref[5:], _col(13, 40, c5=5))
    c.addq(0, f"5={cap + 1}I7=", ref[:5] + b"G" * (cap + 1) + ref[5:], _col(13 + cap, 40))
    return c


def deep_case(n_rows):
    """n_rows identical rows vote T at Q93 on position 20 (705 x 93 = 65 565: past 16 bits) against one row's own base at
    Q93; the rows' 2-base insertion at Q93 opens the slot in front of position 23."""
    rng = np.random.default_rng(5)
    ref = PI.random_contig(rng, 40, lower=0, n_frac=0)
    alt = b"T" if ref[20:21] != b"T" else b"G"
    c = QCase([("c", ref)], W)
    for _ in range(n_rows):
        c.addq(18, "2=1X2=2I2=", ref[18:20] + alt + ref[21:23] + b"CA" + ref[23:25], Q(93) * 9)
    c.addq(0, "40=", ref, Q(93) * 40)
    return c, ref[:20] + alt + ref[21:23] + b"CA" + ref[23:]


# ---- reads with qualities for the overlapper (the fused call and its chain) ----------------------------------------------
def fastq(reads, quals):
    return b"".join(b">" + n.encode() + b"\n" + s + b"\n" if quals.get(n) is None else b"@" + n.encode() + b"\n" + s + b"\n+\n" + quals[n] + b"\n"
                    for n, s in reads)


def overlap_input(short, n_low=0, fasta_every=0):
    """-> (RI.Input, {read name: quality string or None}).  Contigs with errors cut from one genome; reads of it with a few
    wrong bases at Q2 - Q5, a wrong, low-quality 3' tail and, on one genome position in a hundred, the same wrong base at Q2 in
    most of the reads that cover it; the other bases at Q12 - Q40.  `n_low` reads are Q4 throughout,
    the longest read among them; every `fasta_every`-th read is a FASTA record."""
    rng = np.random.default_rng(9301 + short)
    if short:
        g = RI.genome(rng, 2500)
        contigs = [("c0", RI.with_errors(rng, g))]
        reads = RI.sample_reads(rng, g, 220, 150, 150, prefix="s")
        opts = dict(min_len=70)
    else:
        g = RI.genome(rng, 4000)
        contigs = [("c0", RI.with_errors(rng, g[:1500])), ("c1", RI.with_errors(rng, g[1500:]))]
        reads = RI.sample_reads(rng, g, 56, 600, 1200) + [("long", g[1000:2600])]
        opts = dict(min_len=300, min_iden=0.9)
    # positions of the genome where most reads carry one and the same wrong base, at Q2: by count it wins, by weight it cannot
    sys_at = {int(p): b"ACGT"[(b"ACGT".find(g[p:p + 1]) + 1 + int(p) % 3) % 4] for p in rng.choice(len(g), size=len(g) // 100, replace=False)}
    out, quals = [], {}
    low_names = {"long"} | {n for n, _ in reads[:max(0, n_low - 1)]} if n_low else set()
    for k, (name, seq) in enumerate(reads):
        s = bytearray(seq)
        q = bytearray(33 + int(v) for v in rng.choice((12, 20, 30, 40), size=len(s)))
        tail = 8 if short else 30
        wrong = list(rng.choice(len(s) - tail, size=3 if short else 8, replace=False)) + list(range(len(s) - tail, len(s), 3))
        for p in wrong:
            p = int(p)
            s[p] = b"ACGT"[(b"ACGT".find(bytes([s[p]])) + 1 + int(rng.integers(3))) % 4]
        for p in wrong[:-len(range(len(s) - tail, len(s), 3))]:
            q[int(p)] = 33 + int(rng.integers(2, 6))
        q[len(s) - tail:] = Q(2) * tail
        rev = g.find(seq) < 0
        at = g.find(RI.revcomp(seq) if rev else seq)
        for p, base in sys_at.items():
            if at <= p < at + len(s) and rng.random() < 0.7:
                k = at + len(s) - 1 - p if rev else p - at
                s[k] = RI.revcomp(bytes([base]))[0] if rev else base
                q[k] = 33 + 2
        if name in low_names:
            q = bytearray(Q(4) * len(s))
        out.append((name, bytes(s)))
        quals[name] = None if fasta_every and k % fasta_every == fasta_every - 1 and name not in low_names else bytes(q)
    return RI.Input(contigs, out, bool(short), opts), quals
