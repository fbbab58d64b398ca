"""MODEL (test infrastructure): hlmi_variants_ins (include/hylight_mi.h) in plain Python, on bytes - from the FASTA, PAF and list
bytes to the sites' bytes, the insertion sites' bytes, the summary's bytes and the integer stats.  This file is the contract: the
library's files and stats equal this model's byte for byte, through hlmi_variants_ins and (on the PAF hlmi_ava writes) through
hlmi_variants_reads_ins.  It never calls the library, and it is written from the header's rules, not from the kernels.

    variants_ins(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2)
        -> (sites bytes, ins bytes, summary bytes, stats)

The selection is tests/depth_model.py's (select), the position votes and the site rule tests/variants_model.py's, a row's
insertions per slot tests/polish_model.py's (row_votes: neighbouring I ops concatenated, edge I ops counted apart); the slot's
span, the insertion site rule and a site's len, len_count and seq are stated below.
"""
import depth_model as DM
import polish_model as PM
import variants_model as VM

STAT_KEYS = VM.STAT_KEYS + ("slots_callable", "ins_sites", "ins_long", "ins_edge")
INS_HEAD = b"#contig\tpos\tref\tspan\tins\tins_long\tins_frac\tlen\tlen_count\tseq\n"
SUMMARY_HEAD = b"#contig\tlength\treads\tcallable\tsites\tsite_rate\tslots\tins_sites\tins_rate\n"
CAP = 16


def row_insertions(r, read):
    """-> ({slot p: the bases the row inserts there, concatenated, any length}, ins_edge) of one selected row"""
    seg = PM.aligned_bases(r, read)
    p, c, at, edge = r["ts"], 0, {}, 0
    for n, o in r["ops"]:                      # ops of length 0 are dropped by the parser
        if o == 73:                            # I
            if p == r["ts"] or p == r["te"]:
                edge += 1
            else:
                at[p] = at.get(p, b"") + seg[c:c + n]
            c += n
        elif o == 68:                          # D
            p += n
        else:
            p += n
            c += n
    return at, edge


def call_slot(inserts):
    """inserts: the base strings (1..16 bases) of the inserting rows -> (len, len_count, seq); (0, 0, b"*") with none"""
    if not inserts:
        return 0, 0, b"*"
    by_len = {}
    for b in inserts:
        by_len.setdefault(len(b), []).append(b)
    top = max(len(v) for v in by_len.values())
    n = min(k for k, v in by_len.items() if len(v) == top)          # a tie: the smallest
    seq = bytearray()
    for j in range(n):
        cnt = [sum(1 for b in by_len[n] if b[j] == s) for s in b"ACGT"]
        seq.append(b"ACGT"[cnt.index(max(cnt))] if max(cnt) else 78)       # a tie: the first of A C G T; none: N
    return n, top, bytes(seq)


def is_site(s, i, l, min_cov, min_alt, min_frac):
    """-> (callable, site)"""
    if s < min_cov:
        return False, False
    return True, i + l >= min_alt and float(i + l) / float(s) >= min_frac


def variants_ins(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2):
    sites, summary6, vst = VM.variants(contigs, reads, paf, pairs, min_len, min_iden, min_cov, min_alt, min_frac)   # and its refusals
    crecs, sel, _ = DM.select(contigs, reads, paf, pairs, min_len, min_iden)
    rdict = dict(PM.parse_seqs(reads))
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(vst)
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    ins = bytearray(INS_HEAD)
    summary = bytearray(SUMMARY_HEAD)
    lines6 = summary6.split(b"\n")[1:-1]
    for (name, seq), line6 in zip(crecs, lines6):
        L = len(seq)
        span, short, long_ = [0] * (L + 1), {}, {}
        for r in per.get(name, []):
            for p in range(r["ts"] + 1, r["te"]):      # ts < p < te
                span[p] += 1
            at, edge = row_insertions(r, rdict[r["q"]])
            st["ins_edge"] += edge
            for p, b in at.items():
                if len(b) > CAP:
                    long_[p] = long_.get(p, 0) + 1
                    st["ins_long"] += 1
                else:
                    short.setdefault(p, []).append(b)
        slots = n_ins = 0
        for p in range(1, L):
            i, l = len(short.get(p, [])), long_.get(p, 0)
            ok, site = is_site(span[p], i, l, min_cov, min_alt, min_frac)
            slots += ok
            if not site:
                continue
            n_ins += 1
            n, top, bases = call_slot(short.get(p, []))
            ins += b"%s\t%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%s\n" % (name, p, bytes([seq[p - 1]]).upper(), span[p], i, l,
                                                                 b"%.6f" % (float(i + l) / float(span[p])), n, top, bases)
        st["slots_callable"] += slots
        st["ins_sites"] += n_ins
        rate = float(n_ins) / float(slots) if slots else 0.0
        summary += line6 + b"\t%d\t%d\t%s\n" % (slots, n_ins, b"%.6f" % rate)
    return sites, bytes(ins), bytes(summary), st


def ins_rows(ins):
    """ins bytes -> [(contig, p, span, ins, ins_long, len, len_count, seq)]"""
    out = []
    for line in ins.split(b"\n")[1:]:
        if line:
            f = line.split(b"\t")
            out.append((f[0], int(f[1]), int(f[3]), int(f[4]), int(f[5]), int(f[7]), int(f[8]), f[9]))
    return out
