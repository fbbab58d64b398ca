"""MODEL (test infrastructure): hlmi_depth (include/hylight_mi.h) in plain Python, on bytes - from the FASTA, PAF and list bytes to
the TSV bytes, the bedGraph bytes and the integer stats.  This file is the contract: the library's files and stats equal this
model's byte for byte, through hlmi_depth and (on the PAF hlmi_ava writes) through hlmi_depth_reads.  It never calls the library.

    depth(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, bedgraph=True) -> (tsv bytes, bedGraph bytes or None, stats)

The selection is the one tests/polish_pairs_model.py and tests/polish_qual_model.py state (no read is low: there is no floor);
a name twice among the contigs or among the reads is refused, since the table is keyed by name.
"""
import polish_model as PM
import polish_pairs_model as XM
import polish_qual_model as QM

STAT_KEYS = ("rows", "rows_selected", "contigs", "contigs_covered", "positions", "covered", "bases", "runs", "pairs_listed",
             "pairs_unknown", "rows_not_listed")
TSV_HEAD = b"#contig\tlength\treads\tbases\tcovered\tmean_depth\tmedian_depth\tabundance\n"


def select(contigs, reads, paf, pairs, min_len, min_iden):
    """-> (contig records [(name, bases)], selected rows, stats so far); the refusals in the library's order"""
    crecs, rrecs = PM.parse_seqs(contigs), QM.parse_seqs_qual(reads)
    QM.check_quals(rrecs)
    for what, names in (("contigs", [n for n, _ in crecs]), ("reads", [n for n, _, _ in rrecs])):
        seen = set()
        for n in names:
            if n in seen:
                raise PM.Refused(0, f"two records of {what} are named {n!r}")
            seen.add(n)
    cdict, rdict = dict(crecs), {n: s for n, s, _ in rrecs}
    rows = PM.parse_paf(paf)
    PM.check_rows(rows, rdict, cdict)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["rows"], st["contigs"] = len(rows), len(crecs)
    keep = rows
    if pairs is not None:
        listed_rows, bad = XM.parse_list(pairs)
        if bad:
            raise XM.ListRefused(bad, "a list row has fewer than 6 fields")
        listed, st["pairs_listed"], st["pairs_unknown"] = XM.pair_set(listed_rows, set(cdict) | set(rdict))
        keep = []
        for r in rows:
            if r["q"] != r["t"] and (r["q"], r["t"]) not in listed:
                st["rows_not_listed"] += 1
            else:
                keep.append(r)
    sel, _ = QM.select_rows_q(keep, min_len, min_iden, set())
    st["rows_selected"] = len(sel)
    return crecs, sel, st


def depths_of(length, spans):
    d = [0] * length
    for ts, te in spans:
        for p in range(ts, te):
            d[p] += 1
    return d


def runs_of(d):
    """maximal runs of equal depth -> [(start, end, depth)]"""
    out, a = [], 0
    for p in range(1, len(d) + 1):
        if p == len(d) or d[p] != d[a]:
            out.append((a, p, d[a]))
            a = p
    return out if d else []


def depth(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, bedgraph=True):
    crecs, sel, st = select(contigs, reads, paf, pairs, min_len, min_iden)
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append((r["ts"], r["te"]))
    recs, bed = [], bytearray()
    for name, seq in crecs:
        spans = per.get(name, [])
        d = depths_of(len(seq), spans)
        bases, covered = sum(d), sum(1 for x in d if x)
        median = sorted(d)[(len(d) - 1) // 2] if d else 0
        mean = float(bases) / float(len(d)) if d else 0.0
        recs.append((name, len(d), len(spans), bases, covered, mean, median))
        st["contigs_covered"] += 1 if spans else 0
        st["positions"] += len(d)
        st["covered"] += covered
        st["bases"] += bases
        for a, b, v in runs_of(d):
            bed += b"%s\t%d\t%d\t%d\n" % (name, a, b, v)
            st["runs"] += 1 if bedgraph else 0
    total = 0.0
    for r in recs:
        total = total + r[5]
    tsv = bytearray(TSV_HEAD)
    for name, length, n_reads, bases, covered, mean, median in recs:
        ab = mean / total if total != 0.0 else 0.0
        tsv += b"%s\t%d\t%d\t%d\t%d\t%s\t%d\t%s\n" % (name, length, n_reads, bases, covered, b"%.6f" % mean, median, b"%.6f" % ab)
    return bytes(tsv), (bytes(bed) if bedgraph else None), st
