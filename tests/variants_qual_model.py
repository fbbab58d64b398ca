"""MODEL (test infrastructure): hlmi_variants_q and hlmi_variants_ins_q (include/hylight_mi.h) in plain Python, on bytes - the
variant calls of tests/variants_model.py and tests/variants_ins_model.py with a base-quality floor and hlmi_polish_q's read floor.
This file is the contract: the library's files and stats equal this model's byte for byte, through the _q calls and (on the PAF
hlmi_ava writes) through their _reads forms.  It never calls the library, and it is written from the header's rules.

    variants_q(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_base_qual=10,
               min_avg_qual=10.0) -> (sites bytes, summary bytes, stats)
    variants_ins_q(... the same ...) -> (sites bytes, ins bytes, summary bytes, stats)

The rules, where they differ from the older calls':
  qualities   validated and counted as tests/polish_qual_model.py does (check_quals, is_low); a row of a low read is dropped
              directly behind the qname == tname skip, in front of the pair list, and counted in rows_low_qual
  a column    of an = / X op whose base is A C G T passes iff its Phred (byte - 33; strand '-': of read[qe - 1 - i]) is not below
              min_base_qual; a D op's Phred is the lower one of query columns qc - 1 and qc (those inside [0, qe - qs); none: it
              passes), and its columns pass or fail together
  failing     columns cast no vote and count once each in columns_low_qual; columns that vote nothing anyway (N) count nowhere
  FASTA       records have no qualities: every column passes, the read is never low
  slots       take no quality into account: a failing column still spans
"""
import depth_model as DM  # noqa: F401  (the selection this one restates with the floor in it)
import polish_model as PM
import polish_pairs_model as XM
import polish_qual_model as QM
import variants_ins_model as IM
import variants_model as VM

QCOUNT_KEYS = ("reads_with_qual", "rows_low_qual", "columns_low_qual")
STAT_KEYS = VM.STAT_KEYS + QCOUNT_KEYS
INS_STAT_KEYS = IM.STAT_KEYS + QCOUNT_KEYS
Q_MAX = 93


def check_floors(min_base_qual, min_avg_qual):
    if not 0 <= min_base_qual <= Q_MAX:
        raise PM.Refused(0, "min_base_qual outside 0..93")
    if not min_avg_qual >= 0.0:
        raise PM.Refused(0, "min_avg_qual negative or not a number")


def select_q(contigs, reads, paf, pairs, min_len, min_iden, min_avg_qual):
    """depth_model.select with the read floor -> (contig records, selected rows, {read: quality string or None}, stats so far)"""
    crecs, rrecs = PM.parse_seqs(contigs), QM.parse_seqs_qual(reads)
    n_qual = QM.check_quals(rrecs)
    for what, names in (("contigs", [n for n, _ in crecs]), ("reads", [n for n, _, _ in rrecs])):
        seen = set()
        for n in names:
            if n in seen:
                raise PM.Refused(0, f"two records of {what} are named {n!r}")
            seen.add(n)
    cdict, rdict = dict(crecs), {n: s for n, s, _ in rrecs}
    low = {n for n, s, q in rrecs if QM.is_low(s, q, min_avg_qual)}
    rows = PM.parse_paf(paf)
    PM.check_rows(rows, rdict, cdict)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["rows"], st["contigs"], st["reads_with_qual"] = len(rows), len(crecs), n_qual
    listed = None
    if pairs is not None:
        listed_rows, bad = XM.parse_list(pairs)
        if bad:
            raise XM.ListRefused(bad, "a list row has fewer than 6 fields")
        listed, st["pairs_listed"], st["pairs_unknown"] = XM.pair_set(listed_rows, set(cdict) | set(rdict))
    keep = []
    for r in rows:
        if r["q"] == r["t"]:
            continue
        if r["q"] in low:
            st["rows_low_qual"] += 1
        elif listed is not None and (r["q"], r["t"]) not in listed:
            st["rows_not_listed"] += 1
        else:
            keep.append(r)
    sel, _ = QM.select_rows_q(keep, min_len, min_iden, set())
    st["rows_selected"] = len(sel)
    return crecs, sel, {n: q for n, _, q in rrecs}, st


def row_votes_q(r, read, qual, min_base_qual):
    """-> (position votes [(p, symbol 0..4)], the positions of the failing columns) of one selected row; qual None: FASTA"""
    seg = PM.aligned_bases(r, read)
    q = None
    if qual is not None:
        q = [b - 33 for b in qual[r["qs"]:r["qe"]]]
        if r["rev"]:
            q = q[::-1]                               # column i: the quality of read[qe - 1 - i]
    p, c = r["ts"], 0
    votes, failed = [], []
    for n, o in r["ops"]:
        if o == 73:                                   # I
            c += n
        elif o == 68:                                 # D: the lower of the flanks that exist
            flanks = [] if q is None else [q[k] for k in (c - 1, c) if 0 <= k < len(q)]
            ok = not flanks or min(flanks) >= min_base_qual
            if ok:
                votes.extend((p + j, PM.DEL) for j in range(n))
            else:
                failed.extend(p + j for j in range(n))
            p += n
        else:                                         # = X
            for j in range(n):
                k = PM.SYMS.find(seg[c + j:c + j + 1])
                if k < 0:
                    continue                          # votes nothing anyway: judged by no floor
                if q is None or q[c + j] >= min_base_qual:
                    votes.append((p + j, k))
                else:
                    failed.append(p + j)
            p += n
            c += n
    return votes, failed


def _call(contigs, reads, paf, pairs, min_len, min_iden, min_cov, min_alt, min_frac, min_base_qual, min_avg_qual):
    check_floors(min_base_qual, min_avg_qual)
    if min_cov < 1:
        raise PM.Refused(0, "min_cov < 1")
    if min_alt < 1:
        raise PM.Refused(0, "min_alt < 1")
    if not (0.0 <= min_frac <= 1.0):
        raise PM.Refused(0, "min_frac outside [0, 1] or not a number")
    crecs, sel, quals, st = select_q(contigs, reads, paf, pairs, min_len, min_iden, min_avg_qual)
    rdict = dict(PM.parse_seqs(reads))
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    sites, summary = bytearray(VM.SITES_HEAD), bytearray(VM.SUMMARY_HEAD)
    for name, seq in crecs:
        mine = per.get(name, [])
        cnt = [[0] * 5 for _ in seq]
        for r in mine:
            votes, failed = row_votes_q(r, rdict[r["q"]], quals[r["q"]], min_base_qual)
            st["columns_low_qual"] += len(failed)
            for p, k in votes:
                cnt[p][k] += 1
        callable_, n_sites = 0, 0
        for p, v in enumerate(cnt):
            what, alt = VM.site_at(v, seq[p], min_cov, min_alt, min_frac)
            if what == "other":
                st["ref_other"] += 1
            if what in ("callable", "site"):
                callable_ += 1
            if what == "site":
                n_sites += 1
                st["sites_del" if alt == PM.DEL else "sites_base"] += 1
                c = sum(v)
                sites += b"%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%s\n" % (
                    name, p + 1, bytes([seq[p]]).upper(), c, v[0], v[1], v[2], v[3], v[4], VM.LETTERS[alt:alt + 1], v[alt],
                    b"%.6f" % (float(v[alt]) / float(c)))
        st["contigs_covered"] += 1 if mine else 0
        st["positions"] += len(seq)
        st["callable"] += callable_
        st["sites"] += n_sites
        rate = float(n_sites) / float(callable_) if callable_ else 0.0
        summary += b"%s\t%d\t%d\t%d\t%d\t%s\n" % (name, len(seq), len(mine), callable_, n_sites, b"%.6f" % rate)
    return bytes(sites), bytes(summary), st, crecs, per, rdict


def variants_q(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_base_qual=10,
               min_avg_qual=10.0):
    return _call(contigs, reads, paf, pairs, min_len, min_iden, min_cov, min_alt, min_frac, min_base_qual, min_avg_qual)[:3]


def variants_ins_q(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_base_qual=10,
                   min_avg_qual=10.0):
    """the slots over the rows the floors' selection kept, by variants_ins_model's own rules: no quality takes part"""
    sites, summary6, vst, crecs, per, rdict = _call(contigs, reads, paf, pairs, min_len, min_iden, min_cov, min_alt, min_frac,
                                                    min_base_qual, min_avg_qual)
    st = dict.fromkeys(INS_STAT_KEYS, 0)
    st.update(vst)
    ins = bytearray(IM.INS_HEAD)
    summary = bytearray(IM.SUMMARY_HEAD)
    for (name, seq), line6 in zip(crecs, summary6.split(b"\n")[1:-1]):
        L = len(seq)
        span, short, long_ = [0] * (L + 1), {}, {}
        for r in per.get(name, []):
            for p in range(r["ts"] + 1, r["te"]):
                span[p] += 1
            at, edge = IM.row_insertions(r, rdict[r["q"]])
            st["ins_edge"] += edge
            for p, b in at.items():
                if len(b) > IM.CAP:
                    long_[p] = long_.get(p, 0) + 1
                    st["ins_long"] += 1
                else:
                    short.setdefault(p, []).append(b)
        slots = n_ins = 0
        for p in range(1, L):
            i, l = len(short.get(p, [])), long_.get(p, 0)
            ok, site = IM.is_site(span[p], i, l, min_cov, min_alt, min_frac)
            slots += ok
            if not site:
                continue
            n_ins += 1
            n, top, bases = IM.call_slot(short.get(p, []))
            ins += b"%s\t%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%s\n" % (name, p, bytes([seq[p - 1]]).upper(), span[p], i, l,
                                                                 b"%.6f" % (float(i + l) / float(span[p])), n, top, bases)
        st["slots_callable"] += slots
        st["ins_sites"] += n_ins
        rate = float(n_ins) / float(slots) if slots else 0.0
        summary += line6 + b"\t%d\t%d\t%s\n" % (slots, n_ins, b"%.6f" % rate)
    return sites, bytes(ins), bytes(summary), st
