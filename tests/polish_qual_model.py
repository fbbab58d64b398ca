"""MODEL (test infrastructure): hlmi_polish_q (include/hylight_mi.h) in plain Python, on bytes - tests/polish_model.py with
base qualities: a vote weighs max(1, Phred) of its read base, and rows of reads whose mean Phred is below min_avg_qual are
dropped.  This file is the contract: the library's output and stats equal this model's byte for byte.  It is not racon
(which weights the edges of a partial-order graph); parity unpinned.

    polish_q(contigs, reads, paf, min_len=0, min_iden=0.0, min_cov=3, include_unpolished=1, qual_weight=1, min_avg_qual=10.0)
        -> (fasta bytes, stats dict)

Parsing of the PAF and every check of a row are polish_model's.  Refusals raise polish_model.Refused; one about a record's
quality string is a RefusedRecord with the record's name.
"""
import re

import polish_model as PM

SYMS, DEL, CAP = PM.SYMS, PM.DEL, PM.CAP
STAT_KEYS = PM.STAT_KEYS + ("reads_with_qual", "rows_low_qual")
W_MAX = 93                                 # 126 - 33


class RefusedRecord(PM.Refused):
    def __init__(self, record, why):
        super().__init__(0, f"record {record!r}: {why}")
        self.record = record


def parse_seqs_qual(data):
    """paf_io.cpp:read_seqs_qual - polish_model.parse_seqs, keeping the quality lines -> [(name, bases, quality string or None)].
    The quality string is what the reader consumed: whole lines until they hold as many bytes as the bases, or the file ends."""
    L = [l[:-1] if l.endswith(b"\r") else l for l in PM._lines(data)]
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
        qual = None
        if h[:1] == b"@" and i < len(L) and L[i][:1] == b"+":
            i += 1
            q = []
            while i < len(L) and sum(map(len, q)) < len(s):
                q.append(L[i])
                i += 1
            qual = b"".join(q)
        recs.append((name, s, qual))
    return recs


def check_quals(recs):
    """The refusals about qualities, record by record -> reads_with_qual"""
    n = 0
    for name, s, q in recs:
        if q is None:
            continue
        n += 1
        if len(q) != len(s):
            raise RefusedRecord(name, f"{len(s)} bases and {len(q)} quality bytes")
        for b in q:
            if not 33 <= b <= 126:
                raise RefusedRecord(name, f"quality byte {b} (outside 33..126)")
    return n


def is_low(s, q, min_avg_qual):
    """the read floor: one IEEE division, as in the library"""
    if q is None or min_avg_qual == 0.0 or not s:
        return False
    return float(sum(b - 33 for b in q)) / float(len(s)) < min_avg_qual


def weights(s, q, qual_weight):
    if q is None or not qual_weight:
        return [1] * len(s)
    return [max(1, b - 33) for b in q]


def select_rows_q(rows, min_len, min_iden, low):
    """polish_model.select_rows with the floor directly behind the qname == tname skip -> (selected rows, rows_low_qual)"""
    best, n_low = {}, 0
    for r in rows:
        span = r["te"] - r["ts"]
        if r["q"] == r["t"]:
            continue
        if r["q"] in low:
            n_low += 1
            continue
        if span == 0 or span < min_len:
            continue
        n_eq = sum(n for n, o in r["ops"] if o == 61)
        n_all = sum(n for n, _ in r["ops"])
        if float(n_eq) / float(n_all) < min_iden:
            continue
        cur = best.get(r["q"])
        if cur is None or span > cur["te"] - cur["ts"]:
            best[r["q"]] = r
    return sorted(best.values(), key=lambda r: r["line"]), n_low


def row_votes_q(r, read, wts):
    """-> (position votes [(p, symbol 0..4, weight)], slot insertions {p: (bases, weights)}, ins_long, ins_edge)"""
    seg = PM.aligned_bases(r, read)
    w = wts[r["qs"]:r["qe"]]
    if r["rev"]:
        w = w[::-1]                                   # column i: the quality of read[qe - 1 - i]
    p, c = r["ts"], 0
    votes, at = [], {}
    ins_edge = 0
    for n, o in r["ops"]:
        if o == 73:                                   # I
            if p == r["ts"] or p == r["te"]:
                ins_edge += 1
            else:
                b0, w0 = at.get(p, (b"", []))
                at[p] = (b0 + seg[c:c + n], w0 + w[c:c + n])
            c += n
        elif o == 68:                                 # D: the lower of the flanks that exist
            flanks = [w[k] for k in (c - 1, c) if 0 <= k < len(w)]
            wd = min(flanks) if flanks else 1
            votes.extend((p + j, DEL, wd) for j in range(n))
            p += n
        else:                                         # = X
            for j in range(n):
                k = SYMS.find(seg[c + j:c + j + 1])
                if k >= 0:
                    votes.append((p + j, k, w[c + j]))
            p += n
            c += n
    ins_long = sum(1 for b, _ in at.values() if len(b) > CAP)
    return votes, {q: v for q, v in at.items() if len(v[0]) <= CAP}, ins_long, ins_edge


def decide_position_q(wsum, n_votes, own, min_cov):
    """wsum: weight sums of A C G T del; n_votes: voting columns -> None (the byte stays), DEL, or 0..3"""
    if n_votes < min_cov:
        return None
    top = max(wsum)
    tied = [k for k in range(5) if wsum[k] == top]
    k_own = SYMS.find(bytes([own]).upper())
    return k_own if k_own in tied else tied[0]


def decide_slot_q(span, inserts, min_cov):
    """inserts: (bases, weights) of the inserting rows -> the inserted bases (b"" when the slot stays shut)"""
    if span < min_cov or 2 * len(inserts) <= span:
        return b""
    by_len = {}
    for b, w in inserts:
        by_len.setdefault(len(b), []).append((b, w))
    vote = {k: sum(min(w) for _, w in v) for k, v in by_len.items()}
    top = max(vote.values())
    n = min(k for k, v in vote.items() if v == top)
    out = bytearray()
    for j in range(n):
        cnt = [sum(w[j] for b, w in by_len[n] if b[j] == s) for s in SYMS]
        out.append(SYMS[cnt.index(max(cnt))] if max(cnt) else 78)
    return bytes(out)


def polish_q(contigs, reads, paf, min_len=0, min_iden=0.0, min_cov=3, include_unpolished=1, qual_weight=1, min_avg_qual=10.0):
    if min_cov < 1:
        raise PM.Refused(0, "min_cov < 1")
    if not min_avg_qual >= 0.0:
        raise PM.Refused(0, "min_avg_qual negative or not a number")
    crecs, rrecs = PM.parse_seqs(contigs), parse_seqs_qual(reads)
    reads_with_qual = check_quals(rrecs)
    cdict, rdict, wdict, low = {}, {}, {}, set()
    for n, s in crecs:
        cdict.setdefault(n, s)
    for n, s, q in rrecs:
        if n not in rdict:
            rdict[n] = s
            wdict[n] = weights(s, q, qual_weight)
            if is_low(s, q, min_avg_qual):
                low.add(n)
    rows = PM.parse_paf(paf)
    PM.check_rows(rows, rdict, cdict)
    sel, n_low = select_rows_q(rows, min_len, min_iden, low)
    if qual_weight and len(sel) * W_MAX >= 1 << 32:
        raise PM.Refused(0, "rows_selected x 93 >= 2^32")
    st = dict.fromkeys(STAT_KEYS, 0)
    st["rows"], st["rows_selected"], st["contigs"] = len(rows), len(sel), len(crecs)
    st["reads_with_qual"], st["rows_low_qual"] = reads_with_qual, n_low
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    out = bytearray()
    done = set()
    for name, seq in crecs:
        mine = per.get(name, []) if name not in done else []
        done.add(name)
        if not mine:
            if include_unpolished and seq:
                out += b">" + name + b"\n" + seq + b"\n"
            continue
        st["contigs_polished"] += 1
        L = len(seq)
        wsum = [[0] * 5 for _ in range(L)]
        nvote = [0] * L
        span = [0] * (L + 1)
        ins = {}
        for r in mine:
            votes, at, il, ie = row_votes_q(r, rdict[r["q"]], wdict[r["q"]])
            st["ins_long"] += il
            st["ins_edge"] += ie
            for p, k, w in votes:
                wsum[p][k] += w
                nvote[p] += 1
            for p in range(r["ts"] + 1, r["te"]):
                span[p] += 1
            for p, v in at.items():
                ins.setdefault(p, []).append(v)
        new = bytearray()
        covered = 0
        for p in range(L):
            add = decide_slot_q(span[p], ins.get(p, []), min_cov)
            if add:
                st["slots_opened"] += 1
                st["inserted_bases"] += len(add)
                new += add
            d = decide_position_q(wsum[p], nvote[p], seq[p], min_cov)
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
