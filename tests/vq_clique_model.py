"""Plain-Python model of ViralQuasispecies --cliques=true --threads 1 on single-end reads behind cliques.txt
(tools/HaploConduct/src, ViralQuasispecies.cpp:411-428, SRBuilder::cliquesToSuperreads, SRBuilder.cpp:1031-1235): what
hlmi_vq_cliques must write after the clique file, byte for byte.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED for this part, as for tests/vq_merge_model.py (the reference needs Boost); cliques.txt itself IS pinned, by
tests/golden/fxK_* and tests/test_vq_cliques_host.py, so this model takes the clique lines as given.  It restates the
reference's text in its own words, one function per step, each citing the lines it restates, on top of vq_merge_model's
consensus_pos and graph state.
"""
from __future__ import annotations

import os

import vq_merge_model as MM

CLIQUE = dict(min_clique_size=2, error_correction=False, first_it=True, keep_singletons=0)      # polyte.tune_params.py:684-738
STATS = ("cliques_read", "singletons", "below_min", "taken", "filtered", "superreads", "dropped_empty", "dropped_n",
         "dropped_support", "trivial", "trivial_reverse", "short_reads", "n_reads", "columns", "bases_in", "bytes_out")
OUTPUTS = ("cliques.txt", "singles.fastq", "subreads.txt", "clique_map.txt")


# ---- libstdc++ std::sort (bits/stl_algo.h): sortVerticesByEndpos compares the end position alone, so where two ends are equal
# the order is what introsort's data movement leaves ------------------------------------------------------------------------
def std_sort(a, less):
    n = len(a)

    def insertion(first, last):                          # __insertion_sort
        for i in range(first + 1, last):
            v = a[i]
            if less(v, a[first]):
                a[first + 1:i + 1] = a[first:i]
                a[first] = v
            else:
                j = i
                while less(v, a[j - 1]):
                    a[j] = a[j - 1]
                    j -= 1
                a[j] = v

    def unguarded(first, last):                          # __unguarded_insertion_sort
        for i in range(first, last):
            v, j = a[i], i
            while less(v, a[j - 1]):
                a[j] = a[j - 1]
                j -= 1
            a[j] = v

    def loop(first, last, depth):                        # __introsort_loop, _S_threshold 16
        while last - first > 16:
            if depth == 0:
                raise NotImplementedError("std::sort fell back to heap sort: not restated")
            depth -= 1
            x, y, z = first + 1, first + (last - first) // 2, last - 1       # __move_median_to_first
            if less(a[x], a[y]):
                k = y if less(a[y], a[z]) else z if less(a[x], a[z]) else x
            else:
                k = x if less(a[x], a[z]) else z if less(a[y], a[z]) else y
            a[first], a[k] = a[k], a[first]
            lo, hi = first + 1, last                     # __unguarded_partition around a[first]
            while True:
                while less(a[lo], a[first]):
                    lo += 1
                hi -= 1
                while less(a[first], a[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                a[lo], a[hi] = a[hi], a[lo]
                lo += 1
            loop(lo, last, depth)
            last = lo

    if n < 2:
        return
    loop(0, n, 2 * (n.bit_length() - 1))
    if n > 16:                                           # __final_insertion_sort
        insertion(0, 16)
        unguarded(16, n)
    else:
        insertion(0, n)


_COL = {}


def column(nuc, qu):
    """consensus_pos (:297-402) of one column, remembered."""
    r = _COL.get((nuc, qu))
    if r is None:
        r = _COL[(nuc, qu)] = MM.consensus_pos(nuc, qu)
    return r


def consensus(total_len, entries, min_clique_size, error_correction):
    """SRBuilder::consensus (:406-533) as it stands.  entries: [(offset, sequence, qualities)] in list order ->
    (sequence, qualities, trim_pos, columns with three and more bases); trim_pos -1: not enough support (:427-432)."""
    n = len(entries)
    if error_correction:                                 # :420-434
        if n < min_clique_size:
            return "", "", -1, 0
        trim = entries[min_clique_size - 1][0]
    else:
        trim = 0
    at = [trim - p if p < trim else 0 for p, _, _ in entries]              # :439-446
    active, nxt, prefix_removed = [False] * n, 0, False
    out_s, out_q, deep = [], [], 0
    for cur in range(total_len):
        while nxt < n and cur == entries[nxt][0]:        # :455-459
            active[nxt] = True
            nxt += 1
        if error_correction and sum(active) < min_clique_size:             # :466-473
            if nxt == n:
                break
            if not prefix_removed:
                continue
        prefix_removed = True
        nuc, qu = "", ""
        for k in range(n):
            if active[k]:
                p, s, q = at[k], entries[k][1], entries[k][2]
                if p >= len(s) or p >= len(q):           # :478-482
                    return "", "", 0, 0
                nuc += s[p]
                qu += q[p]
                if p + 1 < len(s):
                    at[k] = p + 1
                else:
                    active[k] = False
        if not nuc:                                      # :498-501
            return "", "", 0, 0
        b, q = column(nuc, qu)
        deep += len(nuc) >= 3
        out_s.append(b)
        out_q.append(q)
    return "".join(out_s), "".join(out_q), trim, deep


def place(clique, adj, seqs):
    """sort_vertices (:33-286), the 's' branch: clique ascending -> ([(offset, vertex)] in list order, total length)."""
    base = clique[0]
    order = [(0, base)]
    l_ext = r_ext = 0
    for v in clique[1:]:
        edge = next((e for e in adj[base] if e["v2"] == v), None)          # getEdgeInfo (OverlapGraph.cpp:263-282)
        if edge is None:
            edge = next(e for e in adj[v] if e["v2"] == base)
        new_pos = edge["pos1"] if edge["v1"] == base else -edge["pos1"]    # :142-147
        at = 0
        while at < len(order) and order[at][0] < new_pos:                  # :212-222
            at += 1
        order.insert(at, (new_pos, v))
        l_ext = max(l_ext, -new_pos)                     # :236-240
        r_ext = max(r_ext, len(seqs[v]) + new_pos - len(seqs[base]))
    if order[0][0] < 0:                                  # :248-252
        shift = -order[0][0]
        order = [(p + shift, v) for p, v in order]
    return order, len(seqs[base]) + l_ext + r_ext


def filter_subreads(num, base, order, seqs):
    """filter_subreads (:597-636): the entries of `order` that stay, in list order."""
    selected = {v for _, v in order[:num // 2]}
    selected.add(base)
    pairs = [(v, p + len(seqs[v])) for p, v in order]
    std_sort(pairs, lambda x, y: x[1] < y[1])            # sortVerticesByEndpos (:639-652)
    k = len(pairs)
    while len(selected) < num:
        k -= 1
        selected.add(pairs[k][0])
    return [(p, v) for p, v in order if v in selected]


def read_cliques(text):
    """The loop of :1056-1063: every line counts, the integers a line starts with are its clique."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    out = []
    for line in lines:
        clique = []
        for tok in line.split():
            if not tok.isdigit():
                break
            clique.append(int(tok))
        out.append(clique)
    return out


def superreads(state, clique_text, out_dir, subreads_in=None, **opts):
    """cliquesToSuperreads over a graph state (seqs, quals, ids, orient, adj) -> stats; `deep` (not a library counter) counts
    the consensus columns with three and more bases."""
    co = dict(CLIQUE)
    co.update(opts)
    seqs, quals, ids, orient, adj = (state[k] for k in ("seqs", "quals", "ids", "orient", "adj"))
    V, mcs = len(seqs), co["min_clique_size"]
    stats = dict.fromkeys(STATS, 0)
    stats["deep"] = 0
    stats["bases_in"] = sum(len(s) for s in seqs)
    if co["first_it"]:
        originals_of = lambda v: {ids[v]: [True, 0, len(seqs[v])]}
    else:
        dic = MM.read_subreads(subreads_in)
        originals_of = lambda v: {k: list(o) for k, o in dic[ids[v]].items()}

    def oriented(v):
        return (seqs[v], quals[v]) if orient[v] else (MM.revcomp(seqs[v]), quals[v][::-1])

    fastq, subreads, cmap = [], [], []
    visited = [False] * V
    count = 0
    for clique in read_cliques(clique_text):
        stats["cliques_read"] += 1
        if len(clique) == 1:                             # :1075-1084
            stats["singletons"] += 1
            continue
        if len(clique) < mcs or not clique:
            stats["below_min"] += len(clique) >= 2
            continue
        stats["taken"] += 1
        clique = sorted(clique)                          # constructSuperread :658
        order, total_len = place(clique, adj, seqs)
        used = order
        if len(clique) > 3 * mcs:                        # :721-734
            stats["filtered"] += 1
            used = filter_subreads(2 * mcs, clique[0], order, seqs)
        s, q, trim, deep = consensus(total_len, [(p,) + oriented(v) for p, v in used], mcs, co["error_correction"])
        if trim < 0:
            stats["dropped_support"] += 1
            continue
        if not s:                                        # :999
            stats["dropped_empty"] += 1
            continue
        stats["columns"] += len(s)
        stats["deep"] += deep
        if not MM.n_rate_ok(s):
            stats["dropped_n"] += 1
            continue
        offset = {v: p - trim for p, v in order}         # calcSubreadInfo (:536-595): index1 - startpos1
        merged = {}
        for v in clique:                                 # :750-806
            forward = bool(orient[v])
            for k, o in originals_of(v).items():
                if k in merged:
                    continue
                o = list(o)
                o[0] = o[0] == forward
                if co["first_it"]:
                    o[1] = offset[v]
                elif forward:
                    o[1] += offset[v]
                else:
                    o[1] = len(seqs[v]) + offset[v] - (o[2] + o[1])
                merged[k] = o
            visited[v] = True
        fastq.append(f"@{count}\n{s}\n+\n{q}\n")            # writeSinglesToFile
        subreads.append(MM._line(count, merged))
        cmap.append(f"{count}\t{trim}" + "".join(f"\t{v}:{p - trim}:{'+' if orient[v] else '-'}" for p, v in order) + "\n")
        count += 1
    stats["superreads"] = count
    for v in range(V):                                   # :1145-1222
        if visited[v]:
            continue
        if len(seqs[v]) < co["keep_singletons"]:
            stats["short_reads"] += 1
            continue
        if not MM.n_rate_ok(seqs[v]):
            stats["n_reads"] += 1
            continue
        o = originals_of(v)
        if orient[v]:
            s, q = seqs[v], quals[v]
        else:
            s, q = MM.revcomp(seqs[v]), quals[v][::-1]
            for x in o.values():
                x[0] = not x[0]
                x[1] = len(seqs[v]) - (x[1] + x[2])
            stats["trivial_reverse"] += 1
        stats["trivial"] += 1
        fastq.append(f"@{count}\n{s}\n+\n{q}\n")
        subreads.append(MM._line(count, o))
        count += 1
    text = "".join(fastq)
    stats["bytes_out"] = len(text)
    os.makedirs(out_dir, exist_ok=True)
    for name, body in (("cliques.txt", clique_text), ("singles.fastq", text), ("subreads.txt", "".join(subreads)),
                       ("clique_map.txt", "".join(cmap))):
        with open(os.path.join(out_dir, name), "w", newline="") as f:
            f.write(body)
    return stats


def cliques(singles, overlaps, out_dir, enumerate_cliques, subreads_in=None, scores=None, **opts):
    """The graph (vq_graph_model.graph, its files in out_dir), cliques.txt by `enumerate_cliques(graph.txt path, cliques.txt
    path)` - the pinned enumerator -, then cliquesToSuperreads -> (graph stats, clique stats)."""
    co = {k: opts.pop(k) for k in list(opts) if k in CLIQUE}
    gstats, st = MM.graph_state(singles, overlaps, out_dir, scores=scores, **opts)
    if st is None:
        return gstats, None
    enumerate_cliques(os.path.join(out_dir, "graph.txt"), os.path.join(out_dir, "cliques.txt"))
    m = st["m"]
    state = dict(seqs=m.seqs, quals=st["quals"], ids=st["ids"], orient=st["orient"], adj=m.adj)
    return gstats, superreads(state, open(os.path.join(out_dir, "cliques.txt")).read(), out_dir, subreads_in=subreads_in, **co)
