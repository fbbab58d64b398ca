"""MODEL (test infrastructure): hlmi_phase (include/hylight_mi.h) in plain Python, on bytes - from the FASTA, PAF and list bytes to
the bytes of the three files and the integer stats.  This file is the contract: the library's files and stats equal this model's
byte for byte, through hlmi_phase and (on the PAF hlmi_ava writes) through hlmi_phase_reads.  It never calls the library.

    phase(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8)
        -> (sites bytes, links bytes, reads bytes, stats)

The sites are tests/variants_model.py's (its sites file, read back), the selection tests/depth_model.py's, a row's alleles
tests/polish_model.py's position votes (row_votes); links, blocks, bits and the reads' records are the rules below.
"""
import depth_model as DM
import polish_model as PM
import variants_model as VM

STAT_KEYS = VM.STAT_KEYS + ("links", "links_phased", "blocks", "blocks_multi", "sites_phased", "alleles", "read_records", "reads_a",
                            "reads_b", "reads_tie")
SITES_HEAD = b"#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase\n"
LINKS_HEAD = b"#contig\tpos1\tpos2\tn00\tn01\tn10\tn11\tinformative\tagree\tphased\n"
READS_HEAD = b"#read\tcontig\tblock\tspanned\thap_a\thap_b\tother\thap\n"
NONE = None


def link_call(n, min_link, min_agree):
    """n = [n00, n01, n10, n11] -> (inf, agree as a float, b"cis" | b"trans" | b"-")"""
    cis, trans = n[0] + n[3], n[1] + n[2]
    inf, top = cis + trans, max(cis, trans)
    agree = float(top) / float(inf) if inf else 0.0
    if inf >= min_link and inf and agree >= min_agree:
        return inf, agree, b"cis" if cis > trans else b"trans"
    return inf, agree, b"-"


def allele(votes, p, own, alt):
    """votes: {position: symbol} of one row -> 0, 1, 2 or NONE"""
    k = votes.get(p)
    return NONE if k is None else 0 if k == own else 1 if k == alt else 2


def hap_of(a, b):
    return b"A" if a > b else b"B" if b > a else b"-"


def phase(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8):
    if min_cov < 1:
        raise PM.Refused(0, "min_cov < 1")
    if min_alt < 1:
        raise PM.Refused(0, "min_alt < 1")
    if not (0.0 <= min_frac <= 1.0):
        raise PM.Refused(0, "min_frac outside [0, 1] or not a number")
    if min_link < 1:
        raise PM.Refused(0, "min_link < 1")
    if not (0.5 < min_agree <= 1.0):
        raise PM.Refused(0, "min_agree outside (0.5, 1] or not a number")
    vsites, _, vst = VM.variants(contigs, reads, paf, pairs, min_len, min_iden, min_cov, min_alt, min_frac)
    crecs, sel, _ = DM.select(contigs, reads, paf, pairs, min_len, min_iden)
    rdict = dict(PM.parse_seqs(reads))
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(vst)
    by_contig = {}
    for f in (line.split(b"\t") for line in vsites.split(b"\n")[1:] if line):
        v = [int(x) for x in f[4:9]]
        by_contig.setdefault(f[0], []).append(dict(p=int(f[1]) - 1, own=PM.SYMS.find(f[2]), alt=VM.LETTERS.find(f[9]), depth=int(f[3]), v=v))
    per = {}
    for r in sel:                                                  # contigs in file order below; here (ts, line) inside one
        per.setdefault(r["t"], []).append(r)
    out_s, out_l, out_r = bytearray(SITES_HEAD), bytearray(LINKS_HEAD), bytearray(READS_HEAD)
    for name, seq in crecs:
        sites = by_contig.get(name, [])
        rows = sorted(per.get(name, []), key=lambda r: (r["ts"], r["line"]))
        votes = [dict(PM.row_votes(r, rdict[r["q"]])[0]) for r in rows]
        # rule 2: the allele table - per row, its sites inside [ts, te)
        table = []
        for r, vt in zip(rows, votes):
            mine = [(i, allele(vt, s["p"], s["own"], s["alt"])) for i, s in enumerate(sites) if r["ts"] <= s["p"] < r["te"]]
            table.append(dict(mine))
            st["alleles"] += len(mine)
        # rules 3 and 4
        bit, first = [0] * len(sites), [0] * len(sites)
        for i in range(1, len(sites)):
            n = [0, 0, 0, 0]
            for t in table:
                x, y = t.get(i - 1), t.get(i)
                if x in (0, 1) and y in (0, 1):
                    n[2 * x + y] += 1
            inf, agree, call = link_call(n, min_link, min_agree)
            st["links"] += 1
            out_l += b"%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (name, sites[i - 1]["p"] + 1, sites[i]["p"] + 1, n[0], n[1], n[2], n[3], inf,
                                                                  b"%.6f" % agree, call)
            if call == b"-":
                first[i] = i
            else:
                st["links_phased"] += 1
                first[i] = first[i - 1]
                bit[i] = bit[i - 1] ^ (1 if call == b"trans" else 0)
        for i, s in enumerate(sites):
            size = first.count(first[i])
            st["blocks"] += 1 if first[i] == i else 0
            st["blocks_multi"] += 1 if first[i] == i and size >= 2 else 0
            st["sites_phased"] += 1 if size >= 2 else 0
            out_s += b"%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (name, s["p"] + 1, PM.SYMS[s["own"]:s["own"] + 1], VM.LETTERS[s["alt"]:s["alt"] + 1],
                                                              s["depth"], s["v"][s["own"]], s["v"][s["alt"]], sites[first[i]]["p"] + 1,
                                                              b"1|0" if bit[i] else b"0|1")
        # rule 5
        for r, t in zip(rows, table):
            for b in sorted({first[i] for i in t}):
                mine = [(i, a) for i, a in sorted(t.items()) if first[i] == b]
                ha = sum(1 for i, a in mine if a in (0, 1) and a ^ bit[i] == 0)
                hb = sum(1 for i, a in mine if a in (0, 1) and a ^ bit[i] == 1)
                other = sum(1 for _, a in mine if a == 2)
                if ha + hb + other < 1:
                    continue
                h = hap_of(ha, hb)
                st["read_records"] += 1
                st["reads_a" if h == b"A" else "reads_b" if h == b"B" else "reads_tie"] += 1
                out_r += b"%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (r["q"], name, sites[b]["p"] + 1, len(mine), ha, hb, other, h)
    return bytes(out_s), bytes(out_l), bytes(out_r), st
