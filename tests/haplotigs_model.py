"""MODEL (test infrastructure): hlmi_haplotigs (include/hylight_mi.h) in plain Python, on bytes - from the FASTA, PAF and list bytes
to the bytes of the FASTA and of the blocks file and the integer stats.  This file is the contract: the library's files and stats
equal this model's byte for byte, through hlmi_haplotigs and (on the PAF hlmi_ava writes) through hlmi_haplotigs_reads.  It never
calls the library.

    haplotigs(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3,
              min_agree=0.8, min_side=3, include_unpolished=1) -> (fasta bytes, blocks bytes, stats)

Sites, blocks and bits are tests/phase_model.py's (its sites file, read back), a row's side per block its reads file's (one
selected row per read: the read's name identifies the row); a row's votes are tests/polish_model.py's row_votes, the decisions
its decide_position and decide_slot.  What is new here: which blocks are split, who votes on which side, the two records.
"""
import depth_model as DM
import phase_model as HM
import polish_model as PM

OWN_KEYS = ("blocks_split", "contigs_split", "positions_split", "diff_positions", "records", "substituted", "deleted", "inserted_bases",
            "slots_opened", "ins_long", "ins_edge")
STAT_KEYS = HM.STAT_KEYS + OWN_KEYS
BLOCKS_HEAD = b"#contig\tblock\tstart\tend\tsites\trows_a\trows_b\tsplit\tdiff_positions\n"
SIDES = (b"A", b"B")


def shut_out(extents, side_of, s):
    """the extents (first, last) of the split blocks in which the row reads the side other than s"""
    other = SIDES[1 - SIDES.index(s)]
    return [(f, l) for f, l, b in extents if side_of.get(b) == other]


def position_inside(shut, p):
    return any(f <= p <= l for f, l in shut)


def slot_inside(shut, p):
    """slot p is the gap in front of position p: inside iff first < p <= last"""
    return any(f < p <= l for f, l in shut)


def consensus(seq, cnt, span, ins, min_cov):
    """polish_model.polish's loop over one contig -> (new bytes, decisions, covered, stats of this record)"""
    st = dict(substituted=0, deleted=0, inserted_bases=0, slots_opened=0)
    new, dec, covered = bytearray(), [], 0
    for p in range(len(seq)):
        add = PM.decide_slot(span[p], ins.get(p, []), min_cov)
        if add:
            st["slots_opened"] += 1
            st["inserted_bases"] += len(add)
            new += add
        d = PM.decide_position(cnt[p], seq[p], min_cov)
        dec.append(d)
        if d is None:
            new.append(seq[p])
            continue
        covered += 1
        if d == PM.DEL:
            st["deleted"] += 1
            continue
        if PM.SYMS[d] != bytes([seq[p]]).upper()[0]:
            st["substituted"] += 1
        new.append(PM.SYMS[d])
    return bytes(new), dec, covered, st


def haplotigs(contigs, reads, paf, pairs=None, min_len=0, min_iden=0.0, min_cov=3, min_alt=2, min_frac=0.2, min_link=3, min_agree=0.8,
              min_side=3, include_unpolished=1):
    popts = dict(min_len=min_len, min_iden=min_iden, min_cov=min_cov, min_alt=min_alt, min_frac=min_frac, min_link=min_link,
                 min_agree=min_agree)
    if min_side < 1:
        HM.phase(b"", b"", b"", None, **popts)                     # the phase call's option refusals come first
        raise PM.Refused(0, "min_side < 1")
    sites_b, _, reads_b, pst = HM.phase(contigs, reads, paf, pairs, **popts)
    crecs, sel, _ = DM.select(contigs, reads, paf, pairs, min_len, min_iden)
    rdict = dict(PM.parse_seqs(reads))
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(pst)
    blocks_of = {}                                                 # contig -> {block id: [0-based positions]}, both ascending
    for f in (line.split(b"\t") for line in sites_b.split(b"\n")[1:] if line):
        blocks_of.setdefault(f[0], {}).setdefault(int(f[7]), []).append(int(f[1]) - 1)
    side = {}                                                      # (read, contig) -> {block id: b"A" | b"B" | b"-"}
    for f in (line.split(b"\t") for line in reads_b.split(b"\n")[1:] if line):
        side.setdefault((f[0], f[1]), {})[int(f[2])] = f[7]
    per = {}
    for r in sel:
        per.setdefault(r["t"], []).append(r)
    fasta, table = bytearray(), bytearray(BLOCKS_HEAD)
    for name, seq in crecs:
        mine = per.get(name, [])
        multi = [(b, at) for b, at in blocks_of.get(name, {}).items() if len(at) >= 2]
        rows_ab = {b: [sum(1 for r in mine if side.get((r["q"], name), {}).get(b) == s) for s in SIDES] for b, _ in multi}
        extents = [(at[0], at[-1], b) for b, at in multi if min(rows_ab[b]) >= min_side]
        diff = {b: 0 for b, _ in multi}
        if not mine:
            if include_unpolished and seq:
                fasta += b">" + name + b"\n" + seq + b"\n"
                st["records"] += 1
            continue
        L = len(seq)
        votes = [PM.row_votes(r, rdict[r["q"]]) for r in mine]
        st["ins_long"] += sum(v[2] for v in votes)
        st["ins_edge"] += sum(v[3] for v in votes)
        done = []
        for s in SIDES if extents else SIDES[:1]:
            cnt = [[0] * 5 for _ in range(L)]
            span = [0] * (L + 1)
            ins = {}
            for r, (vt, at, _, _) in zip(mine, votes):
                shut = shut_out(extents, side.get((r["q"], name), {}), s)
                for p, k in vt:
                    if not position_inside(shut, p):
                        cnt[p][k] += 1
                for p in range(r["ts"] + 1, r["te"]):
                    if not slot_inside(shut, p):
                        span[p] += 1
                for p, b in at.items():
                    if not slot_inside(shut, p):
                        ins.setdefault(p, []).append(b)
            new, dec, covered, rst = consensus(seq, cnt, span, ins, min_cov)
            for k, v in rst.items():
                st[k] += v
            done.append(dec)
            if not new:
                continue
            st["records"] += 1
            head = b" LN:i:%d RC:i:%d XC:f:%s" % (len(new), len(mine), ("%.6f" % (covered / L)).encode())
            if extents:
                head = b"_hap" + s + head + b" HB:i:%d HP:i:%d" % (len(extents), sum(l - f + 1 for f, l, _ in extents))
            fasta += b">" + name + head + b"\n" + new + b"\n"
        if extents:
            st["contigs_split"] += 1
            st["blocks_split"] += len(extents)
            for f, l, b in extents:
                st["positions_split"] += l - f + 1
                diff[b] = sum(1 for p in range(f, l + 1) if done[0][p] != done[1][p])
                st["diff_positions"] += diff[b]
        split = {b for _, _, b in extents}
        for b, at in multi:
            table += b"%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, b, at[0] + 1, at[-1] + 1, len(at), rows_ab[b][0], rows_ab[b][1],
                                                              1 if b in split else 0, diff[b])
    return bytes(fasta), bytes(table), st
