"""MODEL (test infrastructure): hlmi_polish_pairs (include/hylight_mi.h) in plain Python, on bytes - tests/polish_qual_model.py
with a pair list: an alignment row may vote only if its (read, contig) pair is named by a row of the list.  This file is the
contract: the library's output and stats equal this model's byte for byte, through hlmi_polish_pairs and (on the PAF hlmi_ava
writes) through hlmi_polish_reads_pairs.  It is not racon; parity unpinned.

    polish_pairs(contigs, reads, paf, pairs, **options of polish_q) -> (fasta bytes, stats dict)

pairs None: polish_q, the three counters 0.  The list's rules:
    parse_list    lines end at \\n (a last line without one counts, a \\r stays in its field), fields split at TAB, fields 1 and
                  6 taken; a line of fewer than 6 fields raises ListRefused(line) - behind every refusal polish_q has about the
                  options, the files and the rows
    pair_set      a name is known when it names a record of the reads or of the contigs; a list row with an unknown name counts
                  in pairs_unknown; both orders of a pair of two different known names are listed
    selection     polish_q's, with "not listed -> dropped, counted in rows_not_listed" directly behind the read floor
"""
import polish_model as PM
import polish_qual_model as QM

STAT_KEYS = QM.STAT_KEYS + ("pairs_listed", "pairs_unknown", "rows_not_listed")


class ListRefused(PM.Refused):
    pass


def parse_list(data):
    """-> ([(field 1, field 6)], 1-based number of the first short line or 0); the rows in front of that line are returned"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                   # (the text ended in \n, or is empty)
    out = []
    for ln, line in enumerate(lines, 1):
        f = line.split(b"\t")
        if len(f) < 6:
            return out, ln
        out.append((f[0], f[5]))
    return out, 0


def pair_set(rows, known):
    """-> (set of listed (a, b), both orders; pairs_listed; pairs_unknown)"""
    s, n_unknown = set(), 0
    for a, b in rows:
        if a not in known or b not in known:
            n_unknown += 1
        elif a != b:
            s.add((a, b))
            s.add((b, a))
    return s, len(s) // 2, n_unknown


def polish_pairs(contigs, reads, paf, pairs, **opts):
    if pairs is None:
        out, st = QM.polish_q(contigs, reads, paf, **opts)
        return out, {**st, "pairs_listed": 0, "pairs_unknown": 0, "rows_not_listed": 0}
    known = {n for n, _ in PM.parse_seqs(contigs)} | {n for n, _, _ in QM.parse_seqs_qual(reads)}
    rows, bad = parse_list(pairs)
    listed, n_listed, n_unknown = pair_set(rows, known)
    mine = {"rows_not_listed": 0}
    inner = QM.select_rows_q

    def select(paf_rows, min_len, min_iden, low):
        """the model's selection over the rows that are listed; a row of a low read stays, to be counted by the floor"""
        if bad:                                       # the rows have been checked by now: the list's own refusal
            raise ListRefused(bad, "a list row has fewer than 6 fields")
        keep = []
        for r in paf_rows:
            if r["q"] != r["t"] and r["q"] not in low and (r["q"], r["t"]) not in listed:
                mine["rows_not_listed"] += 1
            else:
                keep.append(r)
        return inner(keep, min_len, min_iden, low)

    QM.select_rows_q = select                         # polish_q calls its module's select_rows_q: the one hook it needs
    try:
        out, st = QM.polish_q(contigs, reads, paf, **opts)
    finally:
        QM.select_rows_q = inner
    # polish_q counts rows before the selection, so `rows` is still the PAF's
    return out, {**st, "pairs_listed": n_listed, "pairs_unknown": n_unknown, **mine}
