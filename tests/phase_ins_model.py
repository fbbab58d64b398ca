"""MODEL (test infrastructure): hlmi_phase_ins (include/hylight_mi.h) in plain Python, on bytes - from the FASTA, PAF and list
bytes to the bytes of the three files and the integer stats.  This file is the contract: the library's files and stats equal this
model's byte for byte, through hlmi_phase_ins and (on the PAF hlmi_ava writes) through hlmi_phase_reads_ins.  It never calls the
library, and it is written from the header's rules, not from the kernels.

    phase(contigs, reads, paf, pairs=None, reach=1, min_len=0, ..., min_link=3, min_agree=0.8)
        -> (sites bytes, links bytes, reads bytes, stats)

The position sites, the insertion sites and the slot stats are tests/variants_ins_model.py's (its two files, read back), the
selection tests/depth_model.py's, a row's position votes tests/polish_model.py's and its insertions variants_ins_model's
(row_insertions); the link rule, the hap rule and the block rule are phase_model's and phase_reach_model's (link_call, hap_of,
build_blocks).  New here: which insertion sites take part, the merged order, a row's allele at a slot, the `+` marks.
"""
import depth_model as DM
import phase_model as HM
import phase_reach_model as RM
import polish_model as PM
import variants_ins_model as IM
import variants_model as VM

INS_KEYS = ("slots_callable", "ins_sites", "ins_long", "ins_edge", "ins_sites_phasing", "ins_sites_left_out", "ins_sites_phased")
STAT_KEYS = RM.STAT_KEYS + INS_KEYS
BRIDGED = RM.BRIDGED


def takes_part(length, len_count, min_alt):
    return length >= 1 and len_count >= min_alt


def slot_allele(inserts, p, ts, te, length):
    """inserts: {slot: bases} of one row (variants_ins_model.row_insertions) -> 0, 1, 2, or None outside ts < p < te"""
    if not ts < p < te:
        return None
    b = inserts.get(p)
    return 0 if b is None else 1 if len(b) == length else 2


def phase(contigs, reads, paf, pairs=None, reach=1, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8):
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
    if not (1 <= reach <= RM.REACH_MAX):
        raise PM.Refused(0, "reach outside [1, 8]")
    vsites, ins, _, vst = IM.variants_ins(contigs, reads, paf, pairs, min_len, min_iden, min_cov, min_alt, min_frac)
    crecs, sel, _ = DM.select(contigs, reads, paf, pairs, min_len, min_iden)
    rdict = dict(PM.parse_seqs(reads))
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(vst)
    by_contig = {}
    for f in (line.split(b"\t") for line in vsites.split(b"\n")[1:] if line):
        v = [int(x) for x in f[4:9]]
        own, alt, p = PM.SYMS.find(f[2]), VM.LETTERS.find(f[9]), int(f[1]) - 1
        by_contig.setdefault(f[0], []).append(dict(
            key=2 * p + 1, slot=False, p=p, own=own, alt=alt, label=b"%d" % (p + 1),
            line=b"%d\t%s\t%s\t%d\t%d\t%d" % (p + 1, f[2], VM.LETTERS[alt:alt + 1], int(f[3]), v[own], v[alt])))
    for f in (line.split(b"\t") for line in ins.split(b"\n")[1:] if line):
        p, span, i, l, length, len_count = int(f[1]), int(f[3]), int(f[4]), int(f[5]), int(f[7]), int(f[8])
        if not takes_part(length, len_count, min_alt):
            st["ins_sites_left_out"] += 1
            continue
        st["ins_sites_phasing"] += 1
        by_contig.setdefault(f[0], []).append(dict(
            key=2 * p, slot=True, p=p, len=length, label=b"%d+" % p,
            line=b"%d\t%s\t+%s\t%d\t%d\t%d" % (p, f[2], f[9], span, span - i - l, len_count)))
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    out_s, out_l, out_r = bytearray(HM.SITES_HEAD), bytearray(HM.LINKS_HEAD), bytearray(HM.READS_HEAD)
    for name, seq in crecs:
        sites = sorted(by_contig.get(name, []), key=lambda s: s["key"])
        n = len(sites)
        rows = sorted(per.get(name, []), key=lambda r: (r["ts"], r["line"]))
        table = []
        for r in rows:
            vt = dict(PM.row_votes(r, rdict[r["q"]])[0])
            at, _ = IM.row_insertions(r, rdict[r["q"]])
            mine = {}
            for i, s in enumerate(sites):
                if 2 * r["ts"] + 1 <= s["key"] < 2 * r["te"]:
                    mine[i] = slot_allele(at, s["p"], r["ts"], r["te"], s["len"]) if s["slot"] else HM.allele(vt, s["p"], s["own"], s["alt"])
                    assert not (s["slot"] and mine[i] is None)                 # "none" does not occur inside the span
            table.append(mine)
            st["alleles"] += len(mine)
        calls = {}
        for i in range(n):
            for d in range(1, reach + 1):
                if i + d >= n:
                    break
                c = [0, 0, 0, 0]
                for t in table:
                    x, y = t.get(i), t.get(i + d)
                    if x in (0, 1) and y in (0, 1):
                        c[2 * x + y] += 1
                inf, agree, call = HM.link_call(c, min_link, min_agree)
                calls[(i, i + d)] = call
                st["links" if d == 1 else "links_far"] += 1
                if call != b"-":
                    st["links_phased" if d == 1 else "links_far_phased"] += 1
                out_l += b"%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (name, sites[i]["label"], sites[i + d]["label"], c[0], c[1], c[2], c[3], inf,
                                                                      b"%.6f" % agree, call)
        first, bit, joins_far, conflicts = RM.build_blocks(n, reach, lambda j, i: calls[(j, i)])
        st["joins_far"] += joins_far
        st["links_conflict"] += conflicts
        for i, s in enumerate(sites):
            members = sum(1 for k in range(n) if first[k] == first[i] and bit[k] is not BRIDGED)
            st["blocks"] += 1 if first[i] == i else 0
            st["blocks_multi"] += 1 if first[i] == i and members >= 2 else 0
            st["sites_phased"] += 1 if members >= 2 and bit[i] is not BRIDGED else 0
            st["ins_sites_phased"] += 1 if members >= 2 and bit[i] is not BRIDGED and s["slot"] else 0
            st["sites_bridged"] += 1 if bit[i] is BRIDGED else 0
            out_s += b"%s\t%s\t%s\t%s\n" % (name, s["line"], sites[first[i]]["label"], b"." if bit[i] is BRIDGED else b"1|0" if bit[i] else b"0|1")
        for r, t in zip(rows, table):
            for b in sorted({first[i] for i in t}):
                mine = [(i, a) for i, a in sorted(t.items()) if first[i] == b]
                said = [(i, a) for i, a in mine if bit[i] is not BRIDGED]
                ha = sum(1 for i, a in said if a in (0, 1) and a ^ bit[i] == 0)
                hb = sum(1 for i, a in said if a in (0, 1) and a ^ bit[i] == 1)
                other = sum(1 for _, a in said if a == 2)
                if ha + hb + other < 1:
                    continue
                h = HM.hap_of(ha, hb)
                st["read_records"] += 1
                st["reads_a" if h == b"A" else "reads_b" if h == b"B" else "reads_tie"] += 1
                out_r += b"%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (r["q"], name, sites[b]["label"], len(mine), ha, hb, other, h)
    return bytes(out_s), bytes(out_l), bytes(out_r), st
