"""Plain-Python model of ViralQuasispecies --cliques=false --error_correction=false --threads 1 between writeGraphToFile
and findNextOverlaps (tools/HaploConduct/src, ViralQuasispecies.cpp:413-447, SRBuilder::mergeAlongEdges,
SRBuilder.cpp:1238-1384): what hlmi_vq_merge must write, file for file and byte for byte.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED, as for tests/vq_graph_model.py: the reference needs Boost and cannot be built here.  This module restates
its text in its own words, one function per step, each citing the lines it restates.

It continues from the final state of vq_graph_model.graph().  That function returns its stats only, so `graph_state` runs
it under a profile hook and takes the state from its frames as they return - the graph `m`, the inclusions, the tips, and
the labels of every labelling try with the number of edges the try would delete (the first try with the fewest is the one
whose labels the reference keeps as vertex_orientations, GraphAlgos.cpp:204-215, 247).  Nothing of the graph model is
restated here.
"""
from __future__ import annotations

import math
import os
import sys

import vq_graph_model as G

MERGE = dict(first_it=True, keep_singletons=300, store_tips_separately=True, min_clique_size=2)   # pipeline_per_stage.py:170-203
STATS = ("pairs", "merged", "dropped_empty", "dropped_n", "trivial", "trivial_reverse", "short_reads", "n_reads",
         "inclusion_reads", "tip_reads", "bases_in", "bytes_out")
OUTPUTS = ("singles.fastq", "subreads.txt", "removed_tip_sequences.fastq", "superread_map.txt")
MIN_QUAL = 0.9                       # ViralQuasispecies.cpp:62 (--min_qual default) -> SRBuilder.h:89
COMP = str.maketrans("ACGT", "TGCA")
NEG_INF = float("-inf")


# ---- consensus_pos (SRBuilder.cpp:297-402) --------------------------------------------------------------------------------
def _log10(x):
    return NEG_INF if x == 0.0 else math.log10(x)       # C's log10(0) is -inf; math.log10 raises


def c_round(x):
    """C round(): halves away from zero."""
    return math.floor(x + 0.5) if x >= 0 else math.ceil(x - 0.5)


def consensus_pos(nucleotides, qualities):
    """-> (base, quality character).  The expression order is the reference's: scores are added read by read, the four
    powers of total_prob in the order A, T, C, G, ties go to the first of A, T, C, G."""
    score = dict(A=0.0, C=0.0, T=0.0, G=0.0)
    for n, q in zip(nucleotides, qualities):
        p = math.pow(10, -(ord(q) - 33) / 10.0)          # phred_to_prob (:289-293)
        if n in score:
            for b in score:
                score[b] += _log10(1 - p) if b == n else _log10(p / 3.0)
    order = ("A", "T", "C", "G")
    max_score = max(score[b] for b in order)
    max_prob = math.pow(10.0, max_score)
    total_prob = math.pow(10.0, score["A"]) + math.pow(10.0, score["T"]) + math.pow(10.0, score["C"]) + math.pow(10.0, score["G"])
    if max_score == 0 or total_prob == 0.0:              # :354-359
        return "N", "$"
    p_incorrect = 1 - (max_prob / total_prob)
    if len(nucleotides) > 1 and (1 - p_incorrect) < MIN_QUAL:      # :362-368
        return "N", "$"
    assert p_incorrect == p_incorrect
    if p_incorrect < math.pow(10.0, -9.3):
        phred = 93
    else:
        phred = int(c_round(-10 * _log10(p_incorrect)))
    phred = min(max(phred, 0), 93)
    for b in order:                                      # :390-393
        if max_score == score[b]:
            return b, chr(phred + 33)
    raise AssertionError


_PAIR = {}


def pair_base(b1, q1, b2, q2):
    """The two-base function: consensus_pos of (b1, q1), (b2, q2), remembered."""
    k = (b1, q1, b2, q2)
    r = _PAIR.get(k)
    if r is None:
        r = _PAIR[k] = consensus_pos(b1 + b2, q1 + q2)
    return r


_ONE = {}


def one_base(b, q):
    r = _ONE.get((b, q))
    if r is None:
        r = _ONE[(b, q)] = consensus_pos(b, q)
    return r


# ---- consensus of two placed sequences (SRBuilder.cpp:406-533, error_correction false) ------------------------------------
def consensus_pair(seq1, qual1, seq2, qual2, pos):
    """Sequence 1 at 0, sequence 2 at pos >= 0, both oriented -> (sequence, qualities); ("", "") where the reference
    returns an empty consensus.  The loop of :453-521 with its two lists of length two."""
    if len(qual1) == len(seq1) > 0 and len(qual2) == len(seq2) > 0 and pos <= len(seq1):
        # no early return can fire (:478, :498) and every position has one or two active bases: the same answers, taken
        # stretch by stretch (tests/test_vq_merge_model.py holds this to the loop below)
        end = min(len(seq1), pos + len(seq2))
        out = [one_base(b, q) for b, q in zip(seq1[:pos], qual1[:pos])]
        out += [pair_base(a, x, b, y) for a, x, b, y in zip(seq1[pos:end], qual1[pos:end], seq2, qual2)]
        out += [one_base(b, q) for b, q in zip(seq1[end:], qual1[end:])]
        out += [one_base(b, q) for b, q in zip(seq2[end - pos:], qual2[end - pos:])]
        return "".join(o[0] for o in out), "".join(o[1] for o in out)
    return consensus_pair_loop(seq1, qual1, seq2, qual2, pos)


def consensus_pair_loop(seq1, qual1, seq2, qual2, pos):
    """The loop of :453-521 as it stands, for any input."""
    total_len = max(len(seq1), pos + len(seq2))          # base + left + right extension (:224-252)
    seqs, quals, starts = (seq1, seq2), (qual1, qual2), (0, pos)
    active, at = [False, False], [0, 0]
    nxt = 0
    out_s, out_q = [], []
    for cur in range(total_len):
        while nxt < 2 and cur == starts[nxt]:            # :455-459
            active[nxt] = True
            nxt += 1
        nuc, qu = "", ""
        for k in range(2):
            if active[k]:
                p = at[k]
                if p >= len(seqs[k]) or p >= len(quals[k]):          # :478-482
                    return "", ""
                nuc += seqs[k][p]
                qu += quals[k][p]
                if p + 1 < len(seqs[k]):
                    at[k] = p + 1
                else:
                    active[k] = False
        if not nuc:                                      # :498-501
            return "", ""
        b, q = one_base(nuc, qu) if len(nuc) == 1 else pair_base(nuc[0], qu[0], nuc[1], qu[1])
        out_s.append(b)
        out_q.append(q)
    return "".join(out_s), "".join(out_q)


def revcomp(s):
    return s.translate(COMP)[::-1]


def n_rate_ok(seq):
    """Read::test_N_rate (Read.h:214-233)."""
    return float(seq.count("N")) < 0.05 * len(seq)


# ---- the graph state -------------------------------------------------------------------------------------------------------
def graph_state(singles, overlaps, out_dir, scores=None, **opts):
    """vq_graph_model.graph(...) -> (its stats, state); state is None when the run stopped for want of an edge, else a
    dict: m (the final Model), quals, ids, orient, inclusions, tips."""
    cap = {"tries": [], "graph": None}
    gfile = G.graph.__code__.co_filename

    def hook(frame, event, arg):
        if event != "return" or frame.f_code.co_filename != gfile:
            return
        name = frame.f_code.co_name
        if name == "one_try" and arg is not None:
            cap["tries"].append((list(frame.f_locals["labels"]), len(arg[1])))
        elif name == "graph" and arg is not None:
            cap["graph"] = dict(frame.f_locals)

    old = sys.getprofile()
    assert old is None, "graph_state needs the profile hook for itself"
    sys.setprofile(hook)
    try:
        stats = G.graph(singles, overlaps, out_dir, scores=scores, **opts)
    finally:
        sys.setprofile(old)
    loc = cap["graph"]
    assert loc is not None and all(k in loc for k in ("o", "index", "quals")), "vq_graph_model.graph: locals renamed"
    if stats["edges_built"] == 0:
        return stats, None
    assert cap["tries"] and all(k in loc for k in ("m", "inclusions", "tips")), "vq_graph_model: locals renamed"
    m = loc["m"]
    best = min(range(len(cap["tries"])), key=lambda k: (cap["tries"][k][1], k))   # strictly fewer replaces: the first minimum
    assert cap["tries"][best][1] == stats["conflicts"]
    ids = [None] * m.V
    for rid, v in loc["index"].items():
        ids[v] = rid
    m.sort_edges()                                       # ViralQuasispecies.cpp:434
    return stats, dict(m=m, quals=loc["quals"], ids=ids, orient=cap["tries"][best][0], inclusions=list(loc["inclusions"]),
                       tips=set(loc["tips"]), ignore_inclusions=bool(loc["o"]["ignore_inclusions"]))


def read_subreads(path):
    """buildOriginalsDict, the subreads.txt branch (OverlapGraph.cpp:799-845) -> {read id: {original: [forward, index, len]}}."""
    d = {}
    for line in open(path).read().split("\n"):
        if not line:
            continue
        f = line.split("\t")
        entry = d.setdefault(G.OV._strtoul0(f[0]), {})
        for info in f[1:]:
            if not info:
                continue
            t = [x for x in info.replace(",", ":").split(":") if x]
            assert len(t) == 4, "paired-end original"
            entry.setdefault(G.OV._strtoul0(t[0]), [t[1] == "+", int(t[2]), int(t[3])])
    return d


def _line(new_id, originals):
    """:1449-1463 / :1489-1503, entries in ascending original id (stated deviation: the reference's unordered_map order)."""
    return str(new_id) + "".join(f"\t{k}:{'+' if o[0] else '-'}:{o[1]}:{o[2]}" for k, o in sorted(originals.items())) + "\n"


def merge_list(m):
    """getEdgesForMerging (GraphAlgos.cpp:112-148)."""
    taken, pairs = [False] * m.V, []
    for u in range(m.V):
        if taken[u]:
            continue
        for e in m.adj[u]:
            if not taken[e["v2"]]:
                pairs.append((u, e["v2"]))
                taken[u] = taken[e["v2"]] = True
                break
    return pairs


def merge(singles, overlaps, out_dir, subreads_in=None, scores=None, **opts):
    """The graph (vq_graph_model.graph, its files in out_dir) and then mergeAlongEdges -> (graph stats, merge stats)."""
    mo = dict(MERGE)
    for k in list(opts):
        if k in mo:
            mo[k] = opts.pop(k)
    gstats, st = graph_state(singles, overlaps, out_dir, scores=scores, **opts)
    stats = dict.fromkeys(STATS, 0)
    if st is None:                                       # ViralQuasispecies.cpp:282-291
        return gstats, stats
    m, quals, ids, orient = st["m"], st["quals"], st["ids"], st["orient"]
    seqs = m.seqs
    stats["bases_in"] = sum(len(s) for s in seqs)
    if mo["first_it"]:                                   # buildOriginalsDict (:772-798)
        originals_of = lambda v: {ids[v]: [True, 0, len(seqs[v])]}
    else:
        dic = read_subreads(subreads_in)
        originals_of = lambda v: {k: list(o) for k, o in dic[ids[v]].items()}

    def oriented(v):                                     # sort_vertices (:47-76, :134-141)
        return (seqs[v], quals[v]) if orient[v] else (revcomp(seqs[v]), quals[v][::-1])

    pairs = merge_list(m)
    stats["pairs"] = len(pairs)
    fastq, subreads = [], []
    visited = [False] * m.V
    new_id, offset = [-1] * m.V, [0] * m.V
    count = 0
    for u, w in pairs:                                   # process_cliques -> constructSuperread (:654-870)
        base, other = min(u, w), max(u, w)               # :658, :670-679
        edge = next((e for e in m.adj[base] if e["v2"] == other), None)          # getEdgeInfo (OverlapGraph.cpp:263-282)
        if edge is None:
            edge = next(e for e in m.adj[other] if e["v2"] == base)
        new_pos = edge["pos1"] if edge["v1"] == base else -edge["pos1"]          # :142-147
        # the sorted lists (:212-222: the other read goes in front of the base unless its position is greater), shifted to
        # start at 0 (:248-252)
        order = [(other, new_pos), (base, 0)] if new_pos <= 0 else [(base, 0), (other, new_pos)]
        shift = -order[0][1]
        order = [(v, p + shift) for v, p in order]
        (s1, q1), (s2, q2) = oriented(order[0][0]), oriented(order[1][0])
        l_ext, r_ext = max(0, -new_pos), max(0, len(seqs[other]) + new_pos - len(seqs[base]))      # :224-240
        cons_s, cons_q = consensus_pair(s1, q1, s2, q2, order[1][1])
        if cons_s:
            assert len(cons_s) == len(seqs[base]) + l_ext + r_ext
        if not cons_s:                                   # :999
            stats["dropped_empty"] += 1
            continue
        if not n_rate_ok(cons_s):
            stats["dropped_n"] += 1
            continue
        index = dict(order)                              # calcSubreadInfo with trim_pos 0 (:536-595)
        merged = {}
        for v in (base, other):                          # :750-806
            forward = bool(orient[v])
            for k, o in originals_of(v).items():
                if k in merged:
                    continue
                o = list(o)
                o[0] = o[0] == forward
                if mo["first_it"]:
                    o[1] = index[v]
                elif forward:
                    o[1] += index[v]
                else:
                    o[1] = len(seqs[v]) + index[v] - (o[2] + o[1])
                merged[k] = o
            visited[v] = True
            new_id[v], offset[v] = count, index[v]
        fastq.append(f"@{count}\n{cons_s}\n+\n{cons_q}\n")        # writeSinglesToFile (:1471-1507)
        subreads.append(_line(count, merged))
        count += 1
    stats["merged"] = count
    tips = []
    for v in range(m.V):                                 # :1282-1372
        if visited[v]:
            continue
        if len(seqs[v]) < mo["keep_singletons"]:
            stats["short_reads"] += 1
            continue
        if not n_rate_ok(seqs[v]):
            stats["n_reads"] += 1
            continue
        if st["ignore_inclusions"] and st["inclusions"][v]:
            stats["inclusion_reads"] += 1
            tips.append(v)
            continue
        if v in st["tips"] and mo["store_tips_separately"]:
            stats["tip_reads"] += 1
            tips.append(v)
            continue
        o = originals_of(v)
        if orient[v]:
            s, q = seqs[v], quals[v]
        else:                                            # :1337-1368
            s, q = revcomp(seqs[v]), quals[v][::-1]
            for x in o.values():
                x[0] = not x[0]
                x[1] = len(seqs[v]) - (x[1] + x[2])
            stats["trivial_reverse"] += 1
        stats["trivial"] += 1
        new_id[v] = count
        fastq.append(f"@{count}\n{s}\n+\n{q}\n")            # writeTrivialsToFile (:1416-1469)
        subreads.append(_line(count, o))
        count += 1
    text = "".join(fastq)
    stats["bytes_out"] = len(text)
    with open(os.path.join(out_dir, "singles.fastq"), "w", newline="") as f:
        f.write(text)
    with open(os.path.join(out_dir, "subreads.txt"), "w", newline="") as f:
        f.write("".join(subreads))
    if tips:                                             # writeTipsToFile (:1386-1414) appends
        with open(os.path.join(out_dir, "removed_tip_sequences.fastq"), "a", newline="") as f:
            f.write("".join(f"@{k}\n{seqs[v]}\n+\n{quals[v]}\n" for k, v in enumerate(tips)))
    with open(os.path.join(out_dir, "superread_map.txt"), "w", newline="") as f:
        f.write("".join(f"{v}\t{new_id[v]}\t{offset[v]}\t{'+' if orient[v] else '-'}\n" for v in range(m.V)))
    return gstats, stats
