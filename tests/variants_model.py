"""MODEL (test infrastructure): hlmi_variants (include/hylight_mi.h) in plain Python, on bytes - from the FASTA, PAF and list bytes
to the sites' bytes, the summary's bytes and the integer stats.  This file is the contract: the library's files and stats equal
this model's byte for byte, through hlmi_variants and (on the PAF hlmi_ava writes) through hlmi_variants_reads.  It never calls the
library.

    variants(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2)
        -> (sites bytes, summary bytes, stats)

The selection is tests/depth_model.py's (select), the votes are tests/polish_model.py's position votes (row_votes: slots take no
part), the site rule is site_at below.
"""
import depth_model as DM
import polish_model as PM

STAT_KEYS = ("rows", "rows_selected", "contigs", "contigs_covered", "positions", "callable", "ref_other", "sites", "sites_base",
             "sites_del", "pairs_listed", "pairs_unknown", "rows_not_listed")
SITES_HEAD = b"#contig\tpos\tref\tdepth\tA\tC\tG\tT\tdel\talt\talt_count\talt_frac\n"
SUMMARY_HEAD = b"#contig\tlength\treads\tcallable\tsites\tsite_rate\n"
LETTERS = b"ACGT*"


def site_at(v, own, min_cov, min_alt, min_frac):
    """v: votes of A C G T del; own: the contig's byte -> ("none" | "other" | "callable" | "site", alt or None)"""
    c = sum(v)
    if c < min_cov:
        return "none", None
    k_own = PM.SYMS.find(bytes([own]).upper())
    if k_own < 0:
        return "other", None
    alt = max((k for k in range(5) if k != k_own), key=lambda k: (v[k], -k))     # the most votes, the first of A C G T del on a tie
    if v[alt] >= min_alt and float(v[alt]) / float(c) >= min_frac:
        return "site", alt
    return "callable", alt


def variants(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2):
    if min_cov < 1:
        raise PM.Refused(0, "min_cov < 1")
    if min_alt < 1:
        raise PM.Refused(0, "min_alt < 1")
    if not (0.0 <= min_frac <= 1.0):
        raise PM.Refused(0, "min_frac outside [0, 1] or not a number")
    crecs, sel, dst = DM.select(contigs, reads, paf, pairs, min_len, min_iden)
    rdict = dict(PM.parse_seqs(reads))
    st = dict.fromkeys(STAT_KEYS, 0)
    for k in ("rows", "rows_selected", "contigs", "pairs_listed", "pairs_unknown", "rows_not_listed"):
        st[k] = dst[k]
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    sites, summary = bytearray(SITES_HEAD), bytearray(SUMMARY_HEAD)
    for name, seq in crecs:
        mine = per.get(name, [])
        cnt = [[0] * 5 for _ in seq]
        for r in mine:
            for p, k in PM.row_votes(r, rdict[r["q"]])[0]:
                cnt[p][k] += 1
        callable_, n_sites = 0, 0
        for p, v in enumerate(cnt):
            what, alt = site_at(v, seq[p], min_cov, min_alt, min_frac)
            if what == "other":
                st["ref_other"] += 1
            if what in ("callable", "site"):
                callable_ += 1
            if what == "site":
                n_sites += 1
                st["sites_del" if alt == PM.DEL else "sites_base"] += 1
                c = sum(v)
                sites += b"%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%s\n" % (
                    name, p + 1, bytes([seq[p]]).upper(), c, v[0], v[1], v[2], v[3], v[4], LETTERS[alt:alt + 1], v[alt],
                    b"%.6f" % (float(v[alt]) / float(c)))
        st["contigs_covered"] += 1 if mine else 0
        st["positions"] += len(seq)
        st["callable"] += callable_
        st["sites"] += n_sites
        rate = float(n_sites) / float(callable_) if callable_ else 0.0
        summary += b"%s\t%d\t%d\t%d\t%d\t%s\n" % (name, len(seq), len(mine), callable_, n_sites, b"%.6f" % rate)
    return bytes(sites), bytes(summary), st
