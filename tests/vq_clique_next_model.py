"""Plain-Python restatement of SRBuilder::findNextOverlaps behind cliquesToSuperreads: ViralQuasispecies --cliques=true --FNO=1
--optimize=false --threads 1 on single-end reads to the end of main (tools/HaploConduct/src/FindNextOverlaps.cpp:25-327,
:331-347, :351-385, :605-631, :635-697, :816-887, :890-958; SRBuilder.cpp:1125-1160, :1219; ViralQuasispecies.cpp:397-479).
It continues from vq_clique_model.cliques' state - the files it wrote, clique_map.txt above all - and from vq_next_model._Tap's
record of branching and inclusion edges.  What differs from vq_next_model.Next is one fact: a vertex lies in a LIST of
super-reads (nodes_to_SR, :896-913) and updateOverlap loops over the list of u, of v, or over their product.  The set of lines
is a real ordered set of strings, the percentage numpy.float32.  The yardstick of hlmi_vq_clique_iteration; the library is
never its own.  TEST INFRASTRUCTURE ONLY."""
import itertools
import os

import vq_clique_model as CM
import vq_graph_model as G
import vq_merge_model as MM
import vq_next_model as NX

STATS = NX.STATS + ("candidates", "max_list", "in_several")


class CliqueNext:
    """updateOverlap (:25-327) over lists.  lists[v]: [(new id, findCliqueIndex)] in ascending super-read id; copied[v]: v is
    unvisited and was copied - its list is [(its new id, 0)]; a visited vertex in no super-read has an empty list;
    length[id]; orient[v]: the labelling."""

    def __init__(self, lists, copied, length, orient, no_inclusion_overlaps=0):
        self.lists, self.copied, self.length, self.orient = lists, copied, length, orient
        self.no_incl = no_inclusion_overlaps
        self.found = set()                                    # overlaps_found
        self.lines = set()                                    # std::set<std::string>
        self.stats = dict.fromkeys(STATS, 0)
        srl = [len(l) for l, c in zip(lists, copied) if not c]
        self.stats["max_list"] = max(srl, default=0)
        self.stats["in_several"] = sum(n >= 2 for n in srl)
        # what the tests ask of an input, not counters of the library
        self.late_owners = 0          # owners of a key that are not the first turn of their source edge that claims at all
        self.wide_sr2sr = 0           # sr2sr turns of an edge whose two lists both hold two entries and more
        self.min_idx = 0              # the smallest index an owner used
        self.max_turns = 0            # the most turns of one source edge

    def update(self, e):
        u, v = e["v1"], e["v2"]
        if e["score"] == 0:                                   # :34-37
            o1 = "+" if bool(e["ori1"]) == bool(self.orient[u]) else "-"
            o2 = "+" if bool(e["ori2"]) == bool(self.orient[v]) else "-"
        else:
            o1 = o2 = "+"
        lu, lv = self.lists[u], self.lists[v]
        if self.copied[u] and self.copied[v]:                 # :47-72: !visited[u] && !visited[v]
            if not (self.no_incl and e["perc"] == 100):
                self.lines.add(f"{lu[0][0]}\t{lv[0][0]}\t{e['pos1']}\t{e['pos2']}\t{e['ord']}\t{o1}\t{o2}\t{e['perc']}\t0\t"
                               f"{e['len1']}\t{e['len2']}\ts\ts")
                self.stats["copied"] += 1
            return
        if self.copied[u]:                                    # :73-150: the list of v
            kind, turns = "u2sr", [(lu[0], s) for s in lv]
        elif self.copied[v]:                                  # :151-228: the list of u
            kind, turns = "v2sr", [(s, lv[0]) for s in lu]
        else:                                                 # :229-326: the list of u outer, the list of v inner
            kind, turns = "sr2sr", itertools.product(lu, lv)
        self.max_turns = max(self.max_turns, len(lu) * len(lv))
        skip_same, found, claimants = kind == "sr2sr", self.found, 0
        for (a, i1), (b, i2) in turns:
            if skip_same and a == b:                          # :255, in front of the claim
                continue
            claimants += 1
            key = (a, b) if a < b else (b, a)                 # :84-97, :162-175, :261-273
            if key in found:
                continue
            found.add(key)
            self.late_owners += claimants > 1
            self.min_idx = min(self.min_idx, i1, i2)
            r = NX.overlap_data(e["pos1"], i1, i2, self.length[a], self.length[b])       # after the claim
            if r is None:
                self.stats["claims_failed"] += 1
                continue
            ord1, pos1, ol, perc = r
            first, second = (a, b) if ord1 == "1" else (b, a)  # :124-133, :202-211, :299-308
            if not (self.no_incl and perc == 100):
                self.lines.add(f"{first}\t{second}\t{pos1}\t0\t-\t{o1}\t{o2}\t{perc}\t0\t{ol}\t0\ts\ts")
                self.stats[kind] += 1
        self.stats["candidates"] += claimants
        if skip_same and len(lu) >= 2 and len(lv) >= 2:
            self.wide_sr2sr += claimants

    def image(self):
        self.stats["lines"] = len(self.lines)
        return "".join(l + "\n" for l in sorted(self.lines, key=lambda l: l.encode()))      # byte order, as std::string


def from_next_tables(ent, in_sr, off, length, orient, **k):
    """The tables of vq_next_model.Next as lists of one entry at the most."""
    lists = [[] if a is None else [(a, o if s else 0)] for a, s, o in zip(ent, in_sr, off)]
    copied = [a is not None and not s for a, s in zip(ent, in_sr)]
    return CliqueNext(lists, copied, length, orient, **k)


def tables(clique_map_text, seqs, keep_singletons):
    """nodes_to_SR and nodes_to_new_IDs from clique_map.txt - one line per KEPT super-read in ascending id, every member of
    its clique with index1 - startpos1 - and the rule of SRBuilder.cpp:1145-1160, :1219 for the vertices in none."""
    V = len(seqs)
    lists = [[] for _ in range(V)]
    n_sr = 0
    for line in clique_map_text.split("\n")[:-1]:
        f = line.split("\t")
        assert int(f[0]) == n_sr
        for member in f[2:]:
            v, idx, _ = member.split(":")
            lists[int(v)].append((n_sr, int(idx)))
        n_sr += 1
    copied, count = [False] * V, n_sr
    for v in range(V):
        if lists[v] or len(seqs[v]) < keep_singletons or not MM.n_rate_ok(seqs[v]):
            continue
        lists[v], copied[v] = [(count, 0)], True
        count += 1
    return lists, copied, count


class _Unsorted:
    """While vq_graph_model.graph and vq_merge_model.graph_state run: the adjacency lists as they stand when sort_edges is
    entered for the last time.  That call is graph_state's restatement of ViralQuasispecies.cpp:434, which the --cliques=true
    branch never reaches (:417-428): reconsiderEdgeOverlaps and checkEdge walk the lists as cycleRemovalHeuristic left them."""

    def __enter__(self):
        self.adj, self.saved = None, G.Model.sort_edges
        saved, keep = self.saved, self

        def sort_edges(m):
            keep.adj = [[dict(e) for e in l] for l in m.adj]
            return saved(m)

        G.Model.sort_edges = sort_edges
        return self

    def __exit__(self, *exc):
        G.Model.sort_edges = self.saved


class _Adj:
    def __init__(self, adj):
        self.adj = adj


def clique_iteration(singles, overlaps, out_dir, enumerate_cliques, subreads_in=None, scores=None, no_inclusion_overlaps=0, **opts):
    """One clique iteration: vq_clique_model.cliques, then overlaps.txt and the stats.txt line -> (graph stats, clique stats,
    next stats, the CliqueNext that made them); (graph stats, None, zeros, None) when the graph has no edge."""
    o = dict(G.STAGEB)
    o.update({k: v for k, v in opts.items() if k in o})
    keep_singletons = opts.get("keep_singletons", CM.CLIQUE["keep_singletons"])
    cands, _, _ = G.OV.parse_overlaps(overlaps, o["min_overlap_len"], o["min_overlap_perc"], False, o["max_overlaps"])
    with NX._Tap() as tap, _Unsorted() as unsorted:
        gstats, cstats = CM.cliques(singles, overlaps, out_dir, enumerate_cliques, subreads_in=subreads_in, scores=scores, **opts)
    st = tap.state
    if st is None:
        return gstats, None, dict.fromkeys(STATS, 0), None
    m, orient = st["m"], st["orient"]
    walked = _Adj(unsorted.adj)
    V = m.V
    lists, copied, count = tables(open(os.path.join(out_dir, "clique_map.txt")).read(), m.seqs, keep_singletons)
    fq = open(os.path.join(out_dir, "singles.fastq")).read().split("\n")
    length = {int(fq[k][1:]): len(fq[k + 1]) for k in range(0, len(fq) - 1, 4)}
    assert sorted(length) == list(range(count)), "clique_map.txt and singles.fastq disagree about the new reads"
    nx = CliqueNext(lists, copied, length, orient, no_inclusion_overlaps)

    def as_source(e):
        return dict(v1=e["v1"], v2=e["v2"], pos1=e["pos1"], pos2=e["pos2"], ori1=e["ori1"], ori2=e["ori2"],
                    ord=cands[e["k"]]["ord"], perc=e["perc"], len1=e["len"], len2=0, score=e["score"])

    for u in range(V):                                        # reconsiderEdgeOverlaps (:605-631)
        for e in walked.adj[u]:
            nx.stats["src_graph"] += 1
            nx.update(as_source(e))
    for e in tap.branching:
        nx.stats["src_branching"] += 1
        nx.update(as_source(e))
    for r in NX.nonedge_rows(os.path.join(out_dir, "nonedge_overlaps.txt")):    # reconsiderNonedgeOverlaps (:635-697)
        assert r["type1"] == "s" and r["type2"] == "s", "paired-end row"
        v1, v2 = m.index[r["id1"]], m.index[r["id2"]]
        if NX.check_edge(walked, v1, v2) > 0:
            nx.stats["nonedge_skipped"] += 1
            continue
        nx.stats["src_nonedge"] += 1
        perc = int(0.5 * (r["perc1"] + r["perc2"])) if r["perc2"] > 0 else r["perc1"]
        nx.update(dict(v1=v1, v2=v2, pos1=r["pos1"], pos2=r["pos2"], ori1=r["ori1"] == "+", ori2=r["ori2"] == "+", ord=r["ord"],
                       perc=perc, len1=r["len1"], len2=r["len2"], score=0))
    for e in NX.induced_edges(tap.incl_lists, m.seqs, o["edge_threshold"]):     # findInclusionOverlaps (:816-887)
        if NX.check_edge(walked, e["v1"], e["v2"]) == -1:
            nx.stats["src_induced"] += 1
            nx.update(e)
    image = nx.image()
    with open(os.path.join(out_dir, "overlaps.txt"), "w", newline="") as f:
        f.write(image)
    with open(os.path.join(out_dir, "stats.txt"), "a", newline="") as f:        # ViralQuasispecies.cpp:472-479
        f.write(f"{gstats['vertices']}\t{gstats['edges_final']}\t{nx.stats['lines']}\n")
    return gstats, cstats, nx.stats, nx
