"""MODEL (test infrastructure): hlmi_phase_reach (include/hylight_mi.h) in plain Python, on bytes - from the FASTA, PAF and list
bytes to the bytes of the three files and the integer stats.  This file is the contract: the library's files and stats equal this
model's byte for byte, through hlmi_phase_reach and (on the PAF hlmi_ava writes) through hlmi_phase_reads_reach.  It never calls
the library.

    phase(contigs, reads, paf, pairs=None, reach=1, min_len=0, ..., min_link=3, min_agree=0.8)
        -> (sites bytes, links bytes, reads bytes, stats)

Sites, selection and a row's alleles are what tests/phase_model.py uses (variants_model, depth_model, polish_model.row_votes, its
allele, link_call and hap_of); new here: links of every distance up to `reach`, the block rule with bridged sites, the conflict
count.  With reach = 1 the three files and the shared stats are phase_model.phase's (tests/test_phase_reach_model.py).
"""
import depth_model as DM
import phase_model as HM
import polish_model as PM
import variants_model as VM

REACH_MAX = 8
FAR_KEYS = ("links_far", "links_far_phased", "joins_far", "sites_bridged", "links_conflict")
STAT_KEYS = HM.STAT_KEYS + FAR_KEYS
BRIDGED = None                                                     # a bridged site's bit


def build_blocks(n, reach, call):
    """The block rule on n sites of one contig.  call(j, i) -> b"cis" | b"trans" | b"-" for j < i <= j + reach.
    -> (first: every site's block as the index of the block's first site, bit: 0 | 1 | BRIDGED, joins_far, conflicts)"""
    first, bit = [0] * n, [0] * n
    joins_far = conflicts = 0
    b = 0
    while b < n:
        members, last = [b], b
        bit[b] = 0
        i = b + 1
        while i < n and i - last <= reach:
            for j in reversed(members):                            # the nearest member first
                if j < i - reach:
                    break
                c = call(j, i)
                if c != b"-":
                    bit[i] = bit[j] ^ (1 if c == b"trans" else 0)
                    joins_far += 1 if i - j >= 2 else 0
                    members.append(i)
                    last = i
                    break
            i += 1
        for s in range(b, last + 1):
            first[s] = b
            if s not in members:
                bit[s] = BRIDGED
        for x, j in enumerate(members):
            for i in members[x + 1:]:
                if i - j <= reach and call(j, i) != b"-" and (call(j, i) == b"trans") != bool(bit[j] ^ bit[i]):
                    conflicts += 1
        b = last + 1
    return first, bit, joins_far, conflicts


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
    if not (1 <= reach <= REACH_MAX):
        raise PM.Refused(0, "reach outside [1, 8]")
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
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    out_s, out_l, out_r = bytearray(HM.SITES_HEAD), bytearray(HM.LINKS_HEAD), bytearray(HM.READS_HEAD)
    for name, seq in crecs:
        sites = by_contig.get(name, [])
        n = len(sites)
        rows = sorted(per.get(name, []), key=lambda r: (r["ts"], r["line"]))
        votes = [dict(PM.row_votes(r, rdict[r["q"]])[0]) for r in rows]
        table = []
        for r, vt in zip(rows, votes):
            mine = [(i, HM.allele(vt, s["p"], s["own"], s["alt"])) for i, s in enumerate(sites) if r["ts"] <= s["p"] < r["te"]]
            table.append(dict(mine))
            st["alleles"] += len(mine)
        # links: every pair (i, i + d), d <= reach, over the rows with 0 or 1 at both
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
                out_l += b"%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (name, sites[i]["p"] + 1, sites[i + d]["p"] + 1, c[0], c[1], c[2], c[3], inf,
                                                                      b"%.6f" % agree, call)
        first, bit, joins_far, conflicts = build_blocks(n, reach, lambda j, i: calls[(j, i)])
        st["joins_far"] += joins_far
        st["links_conflict"] += conflicts
        for i, s in enumerate(sites):
            members = sum(1 for k in range(n) if first[k] == first[i] and bit[k] is not BRIDGED)
            st["blocks"] += 1 if first[i] == i else 0
            st["blocks_multi"] += 1 if first[i] == i and members >= 2 else 0
            st["sites_phased"] += 1 if members >= 2 and bit[i] is not BRIDGED else 0
            st["sites_bridged"] += 1 if bit[i] is BRIDGED else 0
            out_s += b"%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (name, s["p"] + 1, PM.SYMS[s["own"]:s["own"] + 1], VM.LETTERS[s["alt"]:s["alt"] + 1],
                                                              s["depth"], s["v"][s["own"]], s["v"][s["alt"]], sites[first[i]]["p"] + 1,
                                                              b"." if bit[i] is BRIDGED else b"1|0" if bit[i] else b"0|1")
        # reads: phase_model's rule 5; a bridged site counts in spanned alone
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
                out_r += b"%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (r["q"], name, sites[b]["p"] + 1, len(mine), ha, hb, other, h)
    return bytes(out_s), bytes(out_l), bytes(out_r), st
