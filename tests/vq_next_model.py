"""Plain-Python restatement of SRBuilder::findNextOverlaps with --FNO=1 --optimize=false --cliques=false
--error_correction=false --threads 1 (tools/HaploConduct/src/FindNextOverlaps.cpp:25-327, :331-347, :351-385, :605-631,
:635-697, :816-887, :890-958; ViralQuasispecies.cpp:449-479) and of the stage-b loop of script/pipeline_per_stage.py
(:94-160, :170-275, :347-372).  It continues from vq_merge_model's state as that one continues from vq_graph_model's; what
their state lacks - the removed edges (OverlapGraph::branching_edges) and inclusion_edges - is recorded here while
vq_graph_model's own functions run.  The set of lines is a real ordered set of strings, the percentage numpy.float32.
The yardstick of hlmi_vq_iteration / hylight_amd.vq_stageb; the library is never its own."""
import os

import numpy as np

import vq_graph_model as G
import vq_merge_model as M

STATS = ("src_graph", "src_branching", "src_nonedge", "nonedge_skipped", "src_induced", "copied", "u2sr", "v2sr", "sr2sr",
         "claims_failed", "lines")
F32 = np.float32


class _Tap:
    """While vq_graph_model.graph runs: branching_edges in push order (removeTips GraphAlgos.cpp:630-636, removeBranches
    :918-931, reportCycle OverlapGraph.cpp:548-560), inclusion_edges (GraphAlgos.cpp:26-42) and graph_state's result."""

    def __enter__(self):
        self.branching, self.incl_lists, self.state, self.phase = [], [], None, None
        self.saved = (G.Model.remove, G.label_vertices, G.remove_inclusions, G.remove_transitive, G.remove_tips, G.remove_branches,
                      M.graph_state)
        remove, label, incl, trans, tips, branches, graph_state = self.saved
        tap = self

        def tapped_remove(m, u, v, opposite=None):
            e = remove(m, u, v, opposite)
            if tap.phase in ("tips", "branches", "cycles"):
                tap.branching.append(dict(e))                 # the Edge as it stood when it was removed
            return e

        def phase(name, fn):
            def run(*a, **k):
                tap.phase = name
                try:
                    return fn(*a, **k)
                finally:
                    tap.phase = "cycles"                      # what graph() itself removes later: the back edges
            return run

        def tapped_incl(m, inclusions):
            ins = m.in_lists()
            for v in range(m.V):
                if inclusions[v]:                             # :31-41: out-edges, then getEdgeInfo(inneighbour, v, false)
                    tap.incl_lists.append([dict(e) for e in m.adj[v]] +
                                          [dict(next(e for e in m.adj[u] if e["v2"] == v)) for u in ins[v]])
            return incl(m, inclusions)

        def tapped_state(*a, **k):
            r = graph_state(*a, **k)
            tap.state = r[1]
            return r

        G.Model.remove = tapped_remove
        G.label_vertices = phase("label", label)
        G.remove_inclusions = phase("incl", tapped_incl)
        G.remove_transitive = phase("trans", trans)
        G.remove_tips = phase("tips", tips)
        G.remove_branches = phase("branches", branches)
        M.graph_state = tapped_state
        return self

    def __exit__(self, *exc):
        (G.Model.remove, G.label_vertices, G.remove_inclusions, G.remove_transitive, G.remove_tips, G.remove_branches,
         M.graph_state) = self.saved


def check_edge(m, v, w):
    """OverlapGraph::checkEdge(v, w, reverse allowed) (OverlapGraph.cpp:233-258)."""
    for e in m.adj[v]:
        if e["v2"] == w:
            return e["score"]
    for e in m.adj[w]:
        if e["v2"] == v:
            return e["score"]
    return -1


def overlap_data(pos1, idx1, idx2, len1, len2):
    """computeOverlapData, S-S (:357-385) -> None on failure, else (ord1, new_pos1, overlap_len, perc)."""
    new_pos1 = (pos1 + idx1) - idx2
    if new_pos1 < 0:
        ord1, new_pos1, ln = "2", -new_pos1, len2
    else:
        ord1, ln = "1", len1
    ol = min(ln - new_pos1, len1, len2)
    if new_pos1 >= ln:                                        # :378-384
        return None
    perc = int(np.floor(max(F32(ol) / F32(len1), F32(ol) / F32(len2)) * F32(100)))    # :375
    return ord1, new_pos1, ol, perc


class Next:
    """updateOverlap (:25-327) over the tables mergeAlongEdges leaves.  ent[v]: new id of the read or its super-read, None
    for a visited vertex without a super-read; in_sr[v]; off[v]: findCliqueIndex; length[id]; orient[v]: the labelling."""

    def __init__(self, ent, in_sr, off, length, orient, no_inclusion_overlaps=0):
        self.ent, self.in_sr, self.off, self.length, self.orient = ent, in_sr, off, length, orient
        self.no_incl = no_inclusion_overlaps
        self.found = set()                                    # overlaps_found
        self.lines = set()                                    # std::set<std::string>
        self.stats = dict.fromkeys(STATS, 0)

    def update(self, e):
        u, v = e["v1"], e["v2"]
        if e["score"] == 0:                                   # :34-37
            o1 = "+" if bool(e["ori1"]) == bool(self.orient[u]) else "-"
            o2 = "+" if bool(e["ori2"]) == bool(self.orient[v]) else "-"
        else:
            o1 = o2 = "+"
        a, b = self.ent[u], self.ent[v]
        if not self.in_sr[u] and not self.in_sr[v] and a is not None and b is not None:      # :47-72
            if not (self.no_incl and e["perc"] == 100):
                self.lines.add(f"{a}\t{b}\t{e['pos1']}\t{e['pos2']}\t{e['ord']}\t{o1}\t{o2}\t{e['perc']}\t0\t{e['len1']}\t"
                               f"{e['len2']}\ts\ts")
                self.stats["copied"] += 1
            return
        if a is None or b is None:                            # visited, nodes_to_SR.at() is empty: no loop turn
            return
        kind = "u2sr" if not self.in_sr[u] else "v2sr" if not self.in_sr[v] else "sr2sr"
        if kind == "sr2sr" and a == b:                        # :255
            return
        key = (min(a, b), max(a, b))                          # :84-97, :162-175, :261-273
        if key in self.found:
            return
        self.found.add(key)
        r = overlap_data(e["pos1"], self.off[u] if self.in_sr[u] else 0, self.off[v] if self.in_sr[v] else 0,
                         self.length[a], self.length[b])
        if r is None:
            self.stats["claims_failed"] += 1
            return
        ord1, pos1, ol, perc = r
        first, second = (a, b) if ord1 == "1" else (b, a)     # :124-133, :202-211, :299-308
        if not (self.no_incl and perc == 100):
            self.lines.add(f"{first}\t{second}\t{pos1}\t0\t-\t{o1}\t{o2}\t{perc}\t0\t{ol}\t0\ts\ts")
            self.stats[kind] += 1

    def image(self):
        self.stats["lines"] = len(self.lines)
        return "".join(l + "\n" for l in sorted(self.lines, key=lambda l: l.encode()))      # byte order, as std::string


def induced_edges(lists, seqs, edge_threshold):
    """findInclusionOverlaps (:816-875) without the checkEdge test: the induced edges in loop order."""
    out = []
    for lst in lists:
        for i in range(len(lst)):
            for j in range(i + 1, len(lst)):
                e1, e2 = lst[i], lst[j]
                if e1["v1"] == e2["v1"]:
                    continue
                if e1["v1"] == e2["v2"]:
                    n1, n2, pos1, o1, o2 = e2["v1"], e1["v2"], e2["pos1"], e2["ori1"], e1["ori2"]
                elif e1["v2"] == e2["v1"]:
                    n1, n2, pos1, o1, o2 = e1["v1"], e2["v2"], e1["pos1"], e1["ori1"], e2["ori2"]
                else:
                    continue
                l1, l2 = len(seqs[n1]), len(seqs[n2])
                ln = min(l1 - pos1, l2)
                num, den = 100 * ln, min(l1, l2)
                perc = num // den if num >= 0 else -((-num) // den)          # integer division, as C++ truncates
                out.append(dict(v1=n1, v2=n2, pos1=pos1, pos2=0, ori1=o1, ori2=o2, ord="-", perc=perc, len1=ln, len2=0,
                                score=edge_threshold))
    return out


def nonedge_rows(path):
    rows = []
    for line in open(path).read().split("\n"):
        f = line.strip("\t ").split("\t")
        if len(f) != 13:
            continue
        second = f[3] != "-"                                  # Overlap.h:53-57
        rows.append(dict(id1=G.OV._strtoul0(f[0]), id2=G.OV._strtoul0(f[1]), pos1=int(f[2]), pos2=int(f[3]) if second else 0,
                         ord=f[4], ori1=f[5], ori2=f[6], perc1=int(f[7]), perc2=int(f[8]) if second else 0, len1=int(f[9]),
                         len2=int(f[10]) if second else 0, type1=f[11], type2=f[12]))
    return rows


def iteration(singles, overlaps, out_dir, subreads_in=None, scores=None, no_inclusion_overlaps=0, **opts):
    """One stage-b iteration: vq_merge_model.merge, then overlaps.txt and the stats.txt line -> (graph, merge, next stats)."""
    o = dict(G.STAGEB)
    o.update({k: v for k, v in opts.items() if k in o})
    cands, _, _ = G.OV.parse_overlaps(overlaps, o["min_overlap_len"], o["min_overlap_perc"], False, o["max_overlaps"])
    with _Tap() as tap:
        gstats, mstats = M.merge(singles, overlaps, out_dir, subreads_in=subreads_in, scores=scores, **opts)
    st = tap.state
    if st is None:
        return gstats, mstats, dict.fromkeys(STATS, 0)
    m, orient = st["m"], st["orient"]
    V = m.V
    ent, in_sr, off = [None] * V, [False] * V, [0] * V
    for line in open(os.path.join(out_dir, "superread_map.txt")).read().split("\n")[:-1]:
        v, nid, offset, _ = line.split("\t")
        v, nid = int(v), int(nid)
        ent[v] = None if nid < 0 else nid
        in_sr[v] = 0 <= nid < mstats["merged"]
        off[v] = int(offset)
    fq = open(os.path.join(out_dir, "singles.fastq")).read().split("\n")
    length = {int(fq[k][1:]): len(fq[k + 1]) for k in range(0, len(fq) - 1, 4)}
    nx = Next(ent, in_sr, off, length, orient, no_inclusion_overlaps)

    def as_source(e):
        return dict(v1=e["v1"], v2=e["v2"], pos1=e["pos1"], pos2=e["pos2"], ori1=e["ori1"], ori2=e["ori2"],
                    ord=cands[e["k"]]["ord"], perc=e["perc"], len1=e["len"], len2=0, score=e["score"])

    for u in range(V):                                        # reconsiderEdgeOverlaps (:605-631)
        for e in m.adj[u]:
            nx.stats["src_graph"] += 1
            nx.update(as_source(e))
    for e in tap.branching:
        nx.stats["src_branching"] += 1
        nx.update(as_source(e))
    for r in nonedge_rows(os.path.join(out_dir, "nonedge_overlaps.txt")):       # reconsiderNonedgeOverlaps (:635-697)
        assert r["type1"] == "s" and r["type2"] == "s", "paired-end row"
        v1, v2 = m.index[r["id1"]], m.index[r["id2"]]
        if check_edge(m, v1, v2) > 0:
            nx.stats["nonedge_skipped"] += 1
            continue
        nx.stats["src_nonedge"] += 1
        perc = int(0.5 * (r["perc1"] + r["perc2"])) if r["perc2"] > 0 else r["perc1"]
        nx.update(dict(v1=v1, v2=v2, pos1=r["pos1"], pos2=r["pos2"], ori1=r["ori1"] == "+", ori2=r["ori2"] == "+", ord=r["ord"],
                       perc=perc, len1=r["len1"], len2=r["len2"], score=0))
    for e in induced_edges(tap.incl_lists, m.seqs, o["edge_threshold"]):        # findInclusionOverlaps (:816-887)
        if check_edge(m, e["v1"], e["v2"]) == -1:
            nx.stats["src_induced"] += 1
            nx.update(e)
    image = nx.image()
    with open(os.path.join(out_dir, "overlaps.txt"), "w", newline="") as f:
        f.write(image)
    with open(os.path.join(out_dir, "stats.txt"), "a", newline="") as f:        # ViralQuasispecies.cpp:472-479
        f.write(f"{gstats['vertices']}\t{gstats['edges_final']}\t{nx.stats['lines']}\n")
    return gstats, mstats, nx.stats


# ---- the loop of pipeline_per_stage.py for stage b with --remove_branches true (:141-160) ---------------------------------
def count_records(path):
    return len(open(path).read().split("\n")) // 4 if os.path.isfile(path) else 0


def count_lines(path):
    return open(path).read().count("\n") if os.path.isfile(path) else 0


def edge_count(out_dir):                                      # get_edge_count (:347-354)
    p = os.path.join(out_dir, "graph.txt")
    return count_lines(p) - 2 if os.path.isfile(p) else -2


def stageb(fastq_dir, overlaps, out_dir, **opts):
    """-> dict(reads, overlaps, edges: the counts per iteration, iterations)."""
    os.makedirs(out_dir, exist_ok=True)
    for name in ("stats.txt", "removed_tip_sequences.fastq"):                   # :127-132
        open(os.path.join(out_dir, name), "w").close()
    reads, ovs, edges = [], [count_lines(overlaps)], []
    p = lambda n: os.path.join(out_dir, n)

    def record():
        reads.append(count_records(p("singles.fastq")))
        ovs.append(count_lines(p("overlaps.txt")))
        edges.append(edge_count(out_dir))

    iteration(os.path.join(fastq_dir, "singles.fastq"), overlaps, out_dir, first_it=1, **opts)      # run_first_it_merge
    record()
    const = 0
    while ovs[-1] > 0 and edges[-1] > 0 and const < 2:        # :145-152
        iteration(p("singles.fastq"), p("overlaps.txt"), out_dir, subreads_in=p("subreads.txt"), first_it=0,
                  **dict(opts, merge_contigs=0))
        record()
        const = const + 1 if reads[-1] == reads[-2] else 0
    return dict(reads=reads, overlaps=ovs, edges=edges, iterations=len(reads))


def fastq2fasta(fastq, fasta):
    lines = open(fastq).read().split("\n")
    with open(fasta, "w", newline="") as f:
        for k in range(0, len(lines) - 1, 4):
            f.write(">" + lines[k][1:] + "\n" + lines[k + 1] + "\n")
