"""MODEL (test infrastructure): hlmi_haplotigs_ins (include/hylight_mi.h) in plain Python, on bytes: tests/haplotigs_model.py's
rules over the blocks of tests/phase_ins_model.py, with extents in key space.  This file is the contract of hlmi_haplotigs_ins and
(on the PAF hlmi_ava writes) of hlmi_haplotigs_reads_ins.  It never calls the library.

    haplotigs(contigs, reads, paf, pairs=None, reach=1, min_len=0, ..., min_side=3, include_unpolished=1)
        -> (fasta bytes, blocks bytes, stats)

A block's sites are read back from the phase_ins model's sites file - the lines that carry its id, bridged ones included; a line
whose alt starts with "+" is an insertion site at slot p = its pos (key 2 p), any other a position site on p = pos - 1 (key
2 p + 1) - and a row's side from its reads file.  A split block's extent is [key of its first site, key of its last]; position p is
inside iff its key is, slot p likewise.  Who votes, the decisions and the records are haplotigs_model's functions around these two
tests; the blocks file gains `+` marks and diff_slots.
"""
import depth_model as DM
import haplotigs_model as GM
import phase_ins_model as IM
import phase_model as HM
import phase_reach_model as RM
import polish_model as PM

INS_KEYS = IM.INS_KEYS + ("diff_slots",)
STAT_KEYS = GM.STAT_KEYS + tuple(k for k in INS_KEYS if k not in GM.STAT_KEYS)
BLOCKS_HEAD = GM.BLOCKS_HEAD[:-1] + b"\tdiff_slots\n"


def position_inside(shut, p):
    return any(kf <= 2 * p + 1 <= kl for kf, kl in shut)


def slot_inside(shut, p):
    return any(kf <= 2 * p <= kl for kf, kl in shut)


def positions_of(kf, kl):
    return ((kl - 1) >> 1) - (kf >> 1) + 1


def site_blocks(sites_b):
    """the sites file -> {contig: {block id (bytes): [(key, label)]}}, contigs, blocks and keys in file order (ascending)"""
    out = {}
    for f in (line.split(b"\t") for line in sites_b.split(b"\n")[1:] if line):
        slot = f[3].startswith(b"+")
        key = 2 * int(f[1]) if slot else 2 * (int(f[1]) - 1) + 1
        out.setdefault(f[0], {}).setdefault(f[7], []).append((key, f[1] + (b"+" if slot else b"")))
    return out


def takes_part(sites_b):
    """an insertion site among the model's sites"""
    return any(line.split(b"\t")[3].startswith(b"+") for line in sites_b.split(b"\n")[1:] if line)


def haplotigs(contigs, reads, paf, pairs=None, reach=1, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3,
              min_agree=0.8, min_side=3, include_unpolished=1):
    popts = dict(min_len=min_len, min_iden=min_iden, min_cov=min_cov, min_alt=min_alt, min_frac=min_frac, min_link=min_link,
                 min_agree=min_agree)
    if min_side < 1:
        HM.phase(b"", b"", b"", None, **popts)                     # the phase call's option refusals come first
        raise PM.Refused(0, "min_side < 1")
    if not (1 <= reach <= RM.REACH_MAX):
        raise PM.Refused(0, "reach outside [1, 8]")
    sites_b, _, reads_b, pst = IM.phase(contigs, reads, paf, pairs, reach, **popts)
    crecs, sel, _ = DM.select(contigs, reads, paf, pairs, min_len, min_iden)
    rdict = dict(PM.parse_seqs(reads))
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update({k: pst[k] for k in HM.STAT_KEYS + IM.INS_KEYS if k not in ("ins_long", "ins_edge")})
    blocks_of = site_blocks(sites_b)
    side = {}                                                      # (read, contig) -> {block id: b"A" | b"B" | b"-"}
    for f in (line.split(b"\t") for line in reads_b.split(b"\n")[1:] if line):
        side.setdefault((f[0], f[1]), {})[f[2]] = f[7]
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    fasta, table = bytearray(), bytearray(BLOCKS_HEAD)
    for name, seq in crecs:
        mine = per.get(name, [])
        multi = [(b, at) for b, at in blocks_of.get(name, {}).items() if len(at) >= 2]
        rows_ab = {b: [sum(1 for r in mine if side.get((r["q"], name), {}).get(b) == s) for s in GM.SIDES] for b, _ in multi}
        extents = [(at[0][0], at[-1][0], b) for b, at in multi if min(rows_ab[b]) >= min_side]
        diff = {b: (0, 0) for b, _ in multi}
        if not mine:
            if include_unpolished and seq:
                fasta += b">" + name + b"\n" + seq + b"\n"
                st["records"] += 1
            continue
        L = len(seq)
        votes = [PM.row_votes(r, rdict[r["q"]]) for r in mine]
        st["ins_long"] += sum(v[2] for v in votes)
        st["ins_edge"] += sum(v[3] for v in votes)
        done, opened = [], []
        for s in GM.SIDES if extents else GM.SIDES[:1]:
            cnt = [[0] * 5 for _ in range(L)]
            span = [0] * (L + 1)
            ins = {}
            for r, (vt, at, _, _) in zip(mine, votes):
                shut = GM.shut_out(extents, side.get((r["q"], name), {}), s)
                for p, k in vt:
                    if not position_inside(shut, p):
                        cnt[p][k] += 1
                for p in range(r["ts"] + 1, r["te"]):
                    if not slot_inside(shut, p):
                        span[p] += 1
                for p, b in at.items():
                    if not slot_inside(shut, p):
                        ins.setdefault(p, []).append(b)
            new, dec, covered, rst = GM.consensus(seq, cnt, span, ins, min_cov)
            for k, v in rst.items():
                st[k] += v
            done.append(dec)
            opened.append([len(PM.decide_slot(span[p], ins.get(p, []), min_cov)) for p in range(L)])
            if not new:
                continue
            st["records"] += 1
            head = b" LN:i:%d RC:i:%d XC:f:%s" % (len(new), len(mine), ("%.6f" % (covered / L)).encode())
            if extents:
                head = b"_hap" + s + head + b" HB:i:%d HP:i:%d" % (len(extents), sum(positions_of(kf, kl) for kf, kl, _ in extents))
            fasta += b">" + name + head + b"\n" + new + b"\n"
        if extents:
            st["contigs_split"] += 1
            st["blocks_split"] += len(extents)
            for kf, kl, b in extents:
                st["positions_split"] += positions_of(kf, kl)
                diff[b] = (sum(1 for p in range(L) if kf <= 2 * p + 1 <= kl and done[0][p] != done[1][p]),
                           sum(1 for p in range(L) if kf <= 2 * p <= kl and opened[0][p] != opened[1][p]))
                st["diff_positions"] += diff[b][0]
                st["diff_slots"] += diff[b][1]
        split = {b for _, _, b in extents}
        for b, at in multi:
            table += b"%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, b, at[0][1], at[-1][1], len(at), rows_ab[b][0], rows_ab[b][1],
                                                                    1 if b in split else 0, diff[b][0], diff[b][1])
    return bytes(fasta), bytes(table), st
