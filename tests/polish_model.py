"""MODEL (test infrastructure): the column pile-up consensus of hlmi_polish (include/hylight_mi.h) in plain Python, on
bytes.  This file is the contract: the library's output and stats equal this model's byte for byte.  It is not racon:
racon re-aligns with a partial-order aligner, this function only counts the columns of the CIGARs the overlapper wrote
(replaced by a function of our own, parity unpinned).

    polish(contigs, reads, paf, min_len=0, min_iden=0.0, min_cov=3, include_unpolished=1) -> (fasta bytes, stats dict)

Refusals raise Refused(line) with the 1-based PAF line (0: an option).  Rows are read the way paf_io.cpp:read_paf reads
them; the syntax of every row is checked before the meaning of any (a malformed row 9 is reported before an unknown name
in row 2).  A CIGAR op of length 0 is no op.  A row with te == ts is never selected.
"""
import re

CAP = 16                                  # longest insertion a row can vote for (polish_internal.h: POLISH_INS_CAP)
SYMS = b"ACGT"
DEL = 4
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}  # A<->T C<->G; anything else stays what it is (and never votes)
STAT_KEYS = ("rows", "rows_selected", "contigs", "contigs_polished", "substituted", "deleted", "inserted_bases",
             "slots_opened", "ins_long", "ins_edge")


class Refused(Exception):
    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


def _lines(data):
    out = data.split(b"\n")
    if out and out[-1] == b"":
        out.pop()
    return out


def parse_seqs(data):
    """paf_io.cpp:read_seqs - '>' / '@' records, multi-line, name = header up to the first blank or tab -> [(name, bases)]"""
    L = [l[:-1] if l.endswith(b"\r") else l for l in _lines(data)]
    i, recs = 0, []
    while i < len(L):
        h = L[i]
        if h[:1] not in (b">", b"@"):
            i += 1
            continue
        name = re.split(rb"[ \t]", h[1:], maxsplit=1)[0]
        i += 1
        seq = []
        while i < len(L) and L[i][:1] not in (b">", b"@", b"+"):
            seq.append(L[i])
            i += 1
        s = b"".join(seq)
        if h[:1] == b"@" and i < len(L) and L[i][:1] == b"+":
            i += 1
            q = 0
            while i < len(L) and q < len(s):
                q += len(L[i])
                i += 1
        recs.append((name, s))
    return recs


def _u32(f, ln, col):
    if not (1 <= len(f) <= 10) or not all(48 <= c <= 57 for c in f) or int(f) > 0xffffffff:
        raise Refused(ln, f"column {col} is not an unsigned integer")
    return int(f)


def parse_paf(data):
    """Syntax pass: -> rows as dicts (line, q, t, qs, qe, ts, te, rev, tag, ops) with ops = [(length, op byte)]."""
    rows = []
    for ln, line in enumerate(_lines(data), 1):
        f = line.split(b"\t")
        if len(f) < 11:
            raise Refused(ln, f"{len(f)} columns (< 11)")
        v = {c: _u32(f[c], ln, c + 1) for c in (1, 2, 3, 6, 7, 8, 9, 10)}
        if f[4] not in (b"+", b"-"):
            raise Refused(ln, "strand must be + or -")
        tag = f[-1][:5] == b"cg:Z:"
        ops = []
        if tag and f[-1] != b"cg:Z:*":
            num = None
            for c in f[-1][5:]:
                if 48 <= c <= 57:
                    num = (num or 0) * 10 + c - 48
                    if num >= 1 << 28:
                        raise Refused(ln, "CIGAR op too long")
                else:
                    if num is None:
                        raise Refused(ln, "malformed cg:Z: field")
                    ops.append((num, c))
                    num = None
        rows.append(dict(line=ln, short=len(f) < 12, trail=tag and f[-1][-1:].isdigit(), q=f[0], t=f[5], qs=v[2], qe=v[3], ts=v[7], te=v[8], rev=f[4] == b"-", tag=tag,
                         star=f[-1] == b"cg:Z:*", ops=[o for o in ops if o[0]]))
    for r in rows:                                    # what read_paf lets through and the polisher does not
        if r["short"]:
            raise Refused(r["line"], "11 columns (< 12)")
        if r["trail"]:
            raise Refused(r["line"], "cg:Z: ends in a number")
    return rows


def check_rows(rows, reads, contigs):
    """Meaning pass, in line order; per row in the order of the header's list."""
    for r in rows:
        ln = r["line"]
        if not r["tag"]:
            raise Refused(ln, "no cg:Z: tag in the last column")
        if r["star"] or any(o not in b"=XID" for _, o in r["ops"]):
            raise Refused(ln, "a CIGAR op other than = X I D")
        if r["q"] not in reads:
            raise Refused(ln, "query name is not among the reads")
        if r["t"] not in contigs:
            raise Refused(ln, "target name is not among the contigs")
        if not (r["qs"] <= r["qe"] <= len(reads[r["q"]])) or not (r["ts"] <= r["te"] <= len(contigs[r["t"]])):
            raise Refused(ln, "coordinates outside the sequences")
        if sum(n for n, o in r["ops"] if o in b"=XD") != r["te"] - r["ts"]:
            raise Refused(ln, "the CIGAR's target columns are not te - ts")
        if sum(n for n, o in r["ops"] if o in b"=XI") != r["qe"] - r["qs"]:
            raise Refused(ln, "the CIGAR's query columns are not qe - qs")


def select_rows(rows, min_len, min_iden):
    best = {}
    for r in rows:
        span = r["te"] - r["ts"]
        if r["q"] == r["t"] or span == 0 or span < min_len:
            continue
        n_eq = sum(n for n, o in r["ops"] if o == 61)
        n_all = sum(n for n, _ in r["ops"])
        if float(n_eq) / float(n_all) < min_iden:
            continue
        cur = best.get(r["q"])
        if cur is None or span > cur["te"] - cur["ts"]:          # a tie keeps the earliest line
            best[r["q"]] = r
    return sorted(best.values(), key=lambda r: r["line"])


def aligned_bases(r, read):
    """The read's bases in alignment-column order, upper-cased; strand '-': the reverse complement."""
    seg = read[r["qs"]:r["qe"]].upper()
    if r["rev"]:
        seg = bytes(_COMP.get(c, c) for c in reversed(seg))
    return seg


def row_votes(r, read):
    """-> (position votes [(p, symbol 0..4)], slot insertions {p: bases}, ins_long, ins_edge) of one selected row."""
    seg = aligned_bases(r, read)
    p, c = r["ts"], 0
    votes, at = [], {}
    ins_edge = 0
    for n, o in r["ops"]:
        if o == 73:                                   # I
            if p == r["ts"] or p == r["te"]:
                ins_edge += 1
            else:
                at[p] = at.get(p, b"") + seg[c:c + n]
            c += n
        elif o == 68:                                 # D
            votes.extend((p + j, DEL) for j in range(n))
            p += n
        else:                                         # = X
            for j in range(n):
                k = SYMS.find(seg[c + j:c + j + 1])
                if k >= 0:
                    votes.append((p + j, k))
            p += n
            c += n
    ins_long = sum(1 for b in at.values() if len(b) > CAP)
    return votes, {q: b for q, b in at.items() if len(b) <= CAP}, ins_long, ins_edge


def decide_position(cnt, own, min_cov):
    """cnt: votes of A C G T del; own: the contig's byte -> None (the byte stays), DEL, or 0..3."""
    if sum(cnt) < min_cov:
        return None
    top = max(cnt)
    tied = [k for k in range(5) if cnt[k] == top]
    k_own = SYMS.find(bytes([own]).upper())
    return k_own if k_own in tied else tied[0]


def decide_slot(span, inserts, min_cov):
    """inserts: the base strings of the inserting rows -> the inserted bases (b"" when the slot stays shut)."""
    if span < min_cov or 2 * len(inserts) <= span:
        return b""
    by_len = {}
    for b in inserts:
        by_len.setdefault(len(b), []).append(b)
    top = max(len(v) for v in by_len.values())
    n = min(k for k, v in by_len.items() if len(v) == top)
    out = bytearray()
    for j in range(n):
        cnt = [sum(1 for b in by_len[n] if b[j] == s) for s in SYMS]
        out.append(SYMS[cnt.index(max(cnt))] if max(cnt) else 78)
    return bytes(out)


def polish(contigs, reads, paf, min_len=0, min_iden=0.0, min_cov=3, include_unpolished=1):
    if min_cov < 1:
        raise Refused(0, "min_cov < 1")
    crecs, rrecs = parse_seqs(contigs), parse_seqs(reads)
    cdict, rdict = {}, {}
    for n, s in crecs:
        cdict.setdefault(n, s)
    for n, s in rrecs:
        rdict.setdefault(n, s)
    rows = parse_paf(paf)
    check_rows(rows, rdict, cdict)
    sel = select_rows(rows, min_len, min_iden)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["rows"], st["rows_selected"], st["contigs"] = len(rows), len(sel), len(crecs)
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    out = bytearray()
    done = set()
    for name, seq in crecs:
        mine = per.get(name, []) if name not in done else []    # rows name the first record of a name
        done.add(name)
        if not mine:
            if include_unpolished and seq:
                out += b">" + name + b"\n" + seq + b"\n"
            continue
        st["contigs_polished"] += 1
        L = len(seq)
        cnt = [[0] * 5 for _ in range(L)]
        span = [0] * (L + 1)
        ins = {}
        for r in mine:
            votes, at, il, ie = row_votes(r, rdict[r["q"]])
            st["ins_long"] += il
            st["ins_edge"] += ie
            for p, k in votes:
                cnt[p][k] += 1
            for p in range(r["ts"] + 1, r["te"]):
                span[p] += 1
            for p, b in at.items():
                ins.setdefault(p, []).append(b)
        new = bytearray()
        covered = 0
        for p in range(L):
            add = decide_slot(span[p], ins.get(p, []), min_cov)
            if add:
                st["slots_opened"] += 1
                st["inserted_bases"] += len(add)
                new += add
            d = decide_position(cnt[p], seq[p], min_cov)
            if d is None:
                new.append(seq[p])
                continue
            covered += 1
            if d == DEL:
                st["deleted"] += 1
                continue
            if SYMS[d] != bytes([seq[p]]).upper()[0]:
                st["substituted"] += 1
            new.append(SYMS[d])
        if new:
            out += b">%s LN:i:%d RC:i:%d XC:f:%s\n" % (name, len(new), len(mine), ("%.6f" % (covered / L)).encode())
            out += bytes(new) + b"\n"
    return bytes(out), st
