"""Plain-Python model of ViralQuasispecies --graph_only=true --threads 1 on single-end reads (tools/HaploConduct/src,
ViralQuasispecies.cpp:250-398): what hlmi_vq_graph must write, file for file and byte for byte.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED.  The reference needs Boost, which this image lacks, so it cannot be built and nothing here has been
compared with a run of it.  This module restates its text in its own words, one function per step, each citing the lines
it restates; parsing and scoring come from oracle/vq.py, which it imports and does not change.  Randomness is glibc's
srand / rand (ctypes.CDLL(None)), and the two unstable sorts are libstdc++'s std::sort, restated in `std_sort`.
"""
from __future__ import annotations

import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import vq as OV  # noqa: E402

_libc = ctypes.CDLL(None)
_libc.srand.argtypes = [ctypes.c_uint]
_libc.rand.restype = ctypes.c_int

STAGEB = dict(min_overlap_len=300, min_overlap_perc=0, min_read_len=0, max_tip_len=1000, remove_trans=1,
              edge_threshold=1.0, ov_threshold=0.9, merge_contigs=0.0, mismatch=0.0, ignore_inclusions=True,
              remove_tips=True, remove_branches=True, remove_backedges=True, max_overlaps=100000000)
STATS = ("vertices", "candidates", "duplicates", "inclusions", "edges_built", "conflicts", "moved", "transitive",
         "tip_edges", "tip_reads", "branch_edges", "backedges", "edges_final")
U32 = 0xFFFFFFFF


# ---- libstdc++ pieces ---------------------------------------------------------------------------------------------------
def random_shuffle(seq, seed):
    """srand(seed); std::random_shuffle(seq) as libstdc++ 11 writes it (bits/stl_algo.h): for i = 1 .. n-1 swap item i
    with item rand() % (i + 1)."""
    _libc.srand(seed)
    for i in range(1, len(seq)):
        j = _libc.rand() % (i + 1)
        if i != j:
            seq[i], seq[j] = seq[j], seq[i]
    return seq


def std_sort(a, less):
    """libstdc++'s std::sort (introsort: median-of-three quicksort down to runs of 16, heapsort past depth 2 log2 n, a
    final insertion sort), in place.  Needed where the comparator has ties: std::sort is not stable."""
    def move_median_to_first(res, x, y, z):
        if less(a[x], a[y]):
            if less(a[y], a[z]):
                a[res], a[y] = a[y], a[res]
            elif less(a[x], a[z]):
                a[res], a[z] = a[z], a[res]
            else:
                a[res], a[x] = a[x], a[res]
        elif less(a[x], a[z]):
            a[res], a[x] = a[x], a[res]
        elif less(a[y], a[z]):
            a[res], a[z] = a[z], a[res]
        else:
            a[res], a[y] = a[y], a[res]

    def unguarded_partition(first, last, pivot):
        while True:
            while less(a[first], a[pivot]):
                first += 1
            last -= 1
            while less(a[pivot], a[last]):
                last -= 1
            if not first < last:
                return first
            a[first], a[last] = a[last], a[first]
            first += 1

    def adjust_heap(first, hole, length, value):
        top = hole
        child = hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if less(a[first + child], a[first + child - 1]):
                child -= 1
            a[first + hole] = a[first + child]
            hole = child
        if (length & 1) == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            a[first + hole] = a[first + child - 1]
            hole = child - 1
        parent = (hole - 1) // 2                      # __push_heap
        while hole > top and less(a[first + parent], value):
            a[first + hole] = a[first + parent]
            hole = parent
            parent = (hole - 1) // 2
        a[first + hole] = value

    def heap_sort(first, last):                       # __partial_sort(first, last, last): make_heap + sort_heap
        length = last - first
        if length >= 2:
            parent = (length - 2) // 2
            while True:
                adjust_heap(first, parent, length, a[first + parent])
                if parent == 0:
                    break
                parent -= 1
        while last - first > 1:
            last -= 1
            value = a[last]
            a[last] = a[first]
            adjust_heap(first, 0, last - first, value)

    def introsort_loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                heap_sort(first, last)
                return
            depth -= 1
            mid = first + (last - first) // 2
            move_median_to_first(first, first + 1, mid, last - 1)
            cut = unguarded_partition(first + 1, last, first)
            introsort_loop(cut, last, depth)
            last = cut

    def linear_insert(i):
        val = a[i]
        j = i - 1
        while less(val, a[j]):
            a[j + 1] = a[j]
            j -= 1
        a[j + 1] = val

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if less(a[i], a[first]):
                val = a[i]
                a[first + 1:i + 1] = a[first:i]
                a[first] = val
            else:
                linear_insert(i)

    n = len(a)
    if n > 1:
        introsort_loop(0, n, 2 * (n.bit_length() - 1))
        if n > 16:
            insertion_sort(0, 16)
            for i in range(16, n):
                linear_insert(i)
        else:
            insertion_sort(0, n)
    return a


# ---- reads and candidates ------------------------------------------------------------------------------------------------
def read_singles(path):
    """FastqStorage::read_singles (FastqStorage.cpp:92-150): 4-line records, id = strtoul(first word after '@', 0),
    sequence upper-cased; the vertex of a read is its position (ViralQuasispecies.cpp:262-276)."""
    lines = open(path, "rb").read().decode("latin-1").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    seqs, quals, index = [], [], {}
    for k in range(0, len(lines) - 3, 4):
        words = lines[k][1:].split()
        rid = OV._strtoul0(words[0]) if words else 0
        index[rid] = len(seqs)
        seqs.append(lines[k + 1].upper())
        quals.append(lines[k + 3])
    return seqs, quals, index


def overlap_line(o):
    """Overlap::get_overlap_line (Overlap.h:222-225)."""
    return "\t".join(str(o[k]) for k in ("id1", "id2", "pos1", "pos2", "ord", "ori1", "ori2", "perc1", "perc2", "len1",
                                         "len2", "type1", "type2")) + "\n"


def _nonedge_rows(path, min_len, max_overlaps):
    """The rows construct_edges writes back to nonedge_overlaps.txt (EdgeCalculator.cpp:628-631), in file order: valid
    13-field rows of two different reads that fail the length test (oracle/vq.py counts them, this lists them)."""
    rows = []
    data = open(path, "rb").read().decode("latin-1").split("\n")
    if data and data[-1] == "":
        data.pop()
    for i, line in enumerate(data):
        if i >= max_overlaps:
            break
        f = line.strip("\t ").split("\t") if line.strip("\t ") else []
        if len(f) != 13:
            continue
        dash = f[3] == "-"
        o = dict(id1=OV._strtoul0(f[0]), id2=OV._strtoul0(f[1]), pos1=OV._atoi(f[2]), pos2=0 if dash else OV._atoi(f[3]),
                 ord=f[4].replace(" ", ""), ori1=f[5].replace(" ", ""), ori2=f[6].replace(" ", ""),
                 perc1=OV._atoi(f[7]), perc2=0 if dash else OV._atoi(f[8]), len1=OV._atoi(f[9]),
                 len2=0 if dash else OV._atoi(f[10]), type1="".join(c for c in f[11] if c not in "\n\t "),
                 type2="".join(c for c in f[12] if c not in "\n\t "))
        if o["id1"] == o["id2"]:
            continue
        ss = o["type1"] == "s" and o["type2"] == "s"
        anyp = "p" in (o["type1"], o["type2"])
        if (o["len1"] >= min_len and ss) or (o["len1"] >= 0.5 * min_len and o["len2"] >= 0.5 * min_len and anyp):
            continue
        rows.append(o)
    return rows


# ---- the graph -----------------------------------------------------------------------------------------------------------
class Model:
    """adj[v]: the out-list of v, edges as dicts (v1, v2, pos1..pos4, ori1, ori2 as bools, len, perc, score, mr)."""

    def __init__(self, seqs):
        self.seqs = seqs
        self.V = len(seqs)
        self.adj = [[] for _ in range(self.V)]

    def in_lists(self):
        """adj_in as sortEdges rebuilds it (OverlapGraph.cpp:753-763)."""
        ins = [[] for _ in range(self.V)]
        for u in range(self.V):
            for e in self.adj[u]:
                ins[e["v2"]].append(u)
        return ins

    def n_edges(self):
        return sum(len(l) for l in self.adj)

    def remove(self, u, v, opposite=None):
        """removeEdge / removeEdgeWithOri (OverlapGraph.cpp:104-194): the first u -> v of u's list."""
        for k, e in enumerate(self.adj[u]):
            if e["v2"] == v and (opposite is None or (e["ori1"] == e["ori2"]) == opposite):
                del self.adj[u][k]
                return e
        raise AssertionError(f"edge {u} -> {v} not found")

    def nonoverlap(self, e):                          # Edge::get_nonoverlap_len, unsigned int arithmetic
        return (len(self.seqs[e["v1"]]) + len(self.seqs[e["v2"]]) - 2 * e["len"]) & U32

    def sort_edges(self):
        """sortEdges (OverlapGraph.cpp:722-764): std::sort by (non-overlap length, target)."""
        for u in range(self.V):
            pairs = [(e, self.nonoverlap(e)) for e in self.adj[u]]
            std_sort(pairs, lambda a, b: a[0]["v2"] < b[0]["v2"] if a[1] == b[1] else a[1] < b[1])
            self.adj[u] = [p[0] for p in pairs]

    def sort_adj_out(self):
        """sortAdjOut (GraphAlgos.cpp:806-833): std::sort by target alone."""
        for u in range(self.V):
            pairs = [(e["v2"], e) for e in self.adj[u]]
            std_sort(pairs, lambda a, b: a[0] < b[0])
            self.adj[u] = [p[1] for p in pairs]

    def by_indegree(self):
        """sortVerticesByIndegree (GraphAlgos.cpp:150-176)."""
        deg = [len(l) for l in self.in_lists()]
        return sorted(range(self.V), key=lambda v: (deg[v], v))


def flip(e):
    """Edge::switch_edge_orientation (Edge.h) on a copy, single-end ord '-': -> (copy, changed direction)."""
    e = dict(e)
    e["pos1"], e["pos3"] = e["pos3"], e["pos1"]
    e["pos2"], e["pos4"] = e["pos4"], e["pos2"]
    e["ori1"], e["ori2"] = not e["ori1"], not e["ori2"]
    moved = e["pos1"] < 0 or (e["pos1"] == 0 and e["v1"] > e["v2"])
    if moved:
        e["v1"], e["v2"] = e["v2"], e["v1"]
        e["ori1"], e["ori2"] = e["ori2"], e["ori1"]
        e["pos1"] = -e["pos1"]
    if e["pos2"] < 0:
        e["pos2"] = -e["pos2"]
    return e, moved


def _keeps(old, new):
    """process_overlaps' duplicate rule (EdgeCalculator.cpp:466-518): True when `old` stays against the later `new`."""
    if not new["score"] >= old["score"]:
        return True
    if new["score"] != old["score"]:
        return False
    for field, old_wins in (("len", lambda x, y: x > y), ("mr", lambda x, y: x < y), ("v1", lambda x, y: x < y),
                            ("ori1", lambda x, y: x), ("ori2", lambda x, y: x), ("pos1", lambda x, y: x < y),
                            ("pos2", lambda x, y: x < y)):
        if old[field] != new[field]:
            return bool(old_wins(old[field], new[field]))
    return False                                      # fully equal: the later one replaces


def build_edges(m, cands, scores, opts, stats):
    """construct_edges / process_overlaps (EdgeCalculator.cpp:389-532) at --threads 1 -> (edges in list order per vertex,
    inclusions, scored non-edge rows)."""
    edges, nonedges = [], []
    for k, (c, (score, mr, pos3)) in enumerate(zip(cands, scores)):
        if score > opts["edge_threshold"] or (mr != -1 and mr <= opts["merge_contigs"]):
            e = dict(v1=m.index[c["id1"]], v2=m.index[c["id2"]], pos1=c["pos1"], pos2=c["pos2"], pos3=pos3, pos4=0,
                     ori1=c["ori1"] == "+", ori2=c["ori2"] == "+", len=c["len1"],
                     perc=int(0.5 * (c["perc1"] + c["perc2"])) if c["perc2"] > 0 else c["perc1"], score=score, mr=mr, k=k)
            if e["pos1"] == 0 and e["v1"] > e["v2"]:
                e["v1"], e["v2"] = e["v2"], e["v1"]
                e["ori1"], e["ori2"] = e["ori2"], e["ori1"]
                e["pos3"], e["pos4"] = -e["pos3"], -e["pos4"]
            stats["inclusions"] += e["perc"] == 100
            edges.append(e)
        elif score > opts["ov_threshold"] and mr != -1:
            nonedges.append(c)
    stats["candidates"] = len(edges)
    inclusions = [0] * m.V
    holder = {}                                       # (min, max, opposite) -> edge in the graph
    for e in edges:
        key = (min(e["v1"], e["v2"]), max(e["v1"], e["v2"]), e["ori1"] == e["ori2"])
        old = holder.get(key)
        if old is None:
            holder[key] = e
            m.adj[e["v1"]].append(e)
            if opts["ignore_inclusions"] and e["perc"] == 100 and 0 <= e["mr"] < 0.000001:
                if e["pos3"] < 0:
                    if e["pos1"] == 0:
                        inclusions[e["v1"]] = 1
                else:
                    inclusions[e["v2"]] = 1
        elif not _keeps(old, e):
            m.adj[old["v1"]].remove(old)              # (identity: the very dict)
            m.adj[e["v1"]].append(e)
            holder[key] = e
    stats["edges_built"] = len(holder)
    stats["duplicates"] = stats["candidates"] - stats["edges_built"]
    return inclusions, nonedges


def label_vertices(m, stats):
    """vertexLabellingHeuristic / labelVertices (GraphAlgos.cpp:178-349)."""
    ins = m.in_lists()
    order = m.by_indegree()

    def edge_between(a, b):                           # getEdgeInfo(a, b), reverse allowed
        for e in m.adj[a]:
            if e["v2"] == b:
                return e
        for e in m.adj[b]:
            if e["v2"] == a:
                return e
        raise AssertionError

    def one_try(seed, labels):
        seen = [False] * m.V
        for s in order:
            if seen[s]:
                continue
            seen[s] = True                            # its label stays what `labels` holds
            queue = [s]
            qi = 0
            while qi < len(queue):
                node = queue[qi]
                qi += 1
                nbs = random_shuffle(list(ins[node]) + [e["v2"] for e in m.adj[node]], seed)
                for w in nbs:
                    if not seen[w]:
                        seen[w] = True
                        queue.append(w)
                        e = edge_between(node, w)
                        labels[w] = labels[node] if e["ori1"] == e["ori2"] else 1 - labels[node]
        moved, deleted = [], []
        for u in range(m.V):
            for pos, e in enumerate(m.adj[u]):
                t1, t2 = bool(labels[e["v1"]]), bool(labels[e["v2"]])
                if e["ori1"] == t1 and e["ori2"] == t2:
                    continue
                if (e["ori1"] == e["ori2"]) != (t1 == t2):
                    deleted.append(dict(e))
                    continue
                f, mv = flip(e)
                if mv:
                    moved.append(f)
                else:
                    m.adj[u][pos] = f                 # flipped in the list itself, for good
        return moved, deleted

    best_moved, best_deleted = one_try(1, [1] * m.V)
    count, labels = 1, [1] * m.V                      # tries 2.. share one bitset
    while count < 100 and best_deleted:
        count += 1
        mv, dl = one_try(count, labels)
        if len(dl) < len(best_deleted):
            best_moved, best_deleted = mv, dl
    for e in best_moved:
        m.remove(e["v2"], e["v1"], e["ori1"] == e["ori2"])
        m.adj[e["v1"]].append(e)
    for e in best_deleted:
        m.remove(e["v1"], e["v2"], e["ori1"] == e["ori2"])
    stats["conflicts"] = len(best_deleted)
    stats["moved"] = len(best_moved)


def remove_inclusions(m, inclusions):
    """removeInclusions (GraphAlgos.cpp:20-48): a set of pairs, one removeEdge each."""
    pairs = set()
    ins = m.in_lists()
    for v in range(m.V):
        if inclusions[v]:
            pairs.update((v, e["v2"]) for e in m.adj[v])
            pairs.update((u, v) for u in ins[v])
    for u, v in sorted(pairs):
        m.remove(u, v)


def transitive_targets(m, rounds):
    """findTransEdges with removeTrans false, `rounds` times (GraphAlgos.cpp:746-795, 956-966) -> per vertex the sorted
    targets of the last round's edges."""
    cur = [sorted(e["v2"] for e in m.adj[u]) for u in range(m.V)]
    for _ in range(rounds):
        ins = [[] for _ in range(m.V)]
        for u in range(m.V):
            for v in cur[u]:
                ins[v].append(u)
        insets = [set(l) for l in ins]
        cur = [[v for v in cur[u] if insets[v].intersection(cur[u])] for u in range(m.V)]
    return cur


def remove_transitive(m, rounds, stats, branch=None):
    """removeTransitiveEdges (GraphAlgos.cpp:938-1077).  branch: force the > 50 % rebuild (True) or the one-by-one
    removal (False); None takes the reference's own test.  Both must leave the same adj_out."""
    m.sort_adj_out()
    trans = transitive_targets(m, rounds)
    count = sum(len(l) for l in trans)
    stats["transitive"] = count
    if branch is None:
        branch = 1.0 * count > 0.5 * m.n_edges()
    if branch:                                        # :995-1061, a merge of each list with its transitive targets
        for u in range(m.V):
            t, keep = list(trans[u]), []
            for e in m.adj[u]:
                if t and e["v2"] == t[0]:
                    t.pop(0)
                else:
                    keep.append(e)
            m.adj[u] = keep
    else:                                             # :1063-1071
        for u in range(m.V):
            for v in trans[u]:
                m.remove(u, v)


def write_gfa(m, path):
    """write2GFA (OverlapGraph.cpp:468-543)."""
    with open(path, "w", newline="") as f:
        f.write("H\tVN:Z:1.0\n")
        for i in range(m.V):
            f.write(f"S\t{i}\t{m.seqs[i]}\n")
            for e in m.adj[i]:
                f.write(f"L\t{i}\t+\t{e['v2']}\t+\t{e['len']}M\n")


def remove_tips(m, max_tip_len, stats):
    """removeTips (GraphAlgos.cpp:543-637) -> the set of tip vertices."""
    pairs, tips = set(), set()
    ins = m.in_lists()
    for i in range(m.V):                              # out-tips
        if len(m.adj[i]) <= 1:
            continue
        short, every = [], True
        for e in m.adj[i]:
            v = e["v2"]
            if m.adj[v]:
                every = False
                continue
            ext = max(len(m.seqs[v]) - e["len"], 0)
            if ext == 0:
                pairs.add((i, v)); tips.add(v)
            elif ext < max_tip_len:
                short.append((i, v))
        if not every:
            pairs.update(short); tips.update(v for _, v in short)
    for i in range(m.V):                              # in-tips
        if len(ins[i]) <= 1:
            continue
        short, every = [], True
        for u in ins[i]:
            if ins[u]:
                every = False
                continue
            e = next(x for x in m.adj[u] if x["v2"] == i)
            ext = (e["pos1"] + e["pos2"]) & U32
            if ext == 0:
                pairs.add((u, i)); tips.add(u)
            elif ext < max_tip_len:
                short.append((u, i))
        if not every:
            pairs.update(short); tips.update(u for u, _ in short)
    for u, v in sorted(pairs):
        m.remove(u, v)
    stats["tip_edges"] = len(pairs)
    stats["tip_reads"] = len(tips)
    return tips


def remove_branches(m, stats):
    """removeBranches (GraphAlgos.cpp:835-936) with findBranchfreeGraph (:714-743)."""
    m.sort_adj_out()
    trans = transitive_targets(m, 1)
    new_out = [[] for _ in range(m.V)]
    new_in = [[] for _ in range(m.V)]
    for u in range(m.V):
        t = list(trans[u])
        for e in m.adj[u]:
            if t and e["v2"] == t[0]:
                t.pop(0)
                continue
            new_out[u].append(e["v2"])
            new_in[e["v2"]].append(u)
    cut_out = {u for u in range(m.V) if len(new_out[u]) > 1}
    cut_in = {v for v in range(m.V) if len(new_in[v]) > 1}
    for u in cut_out:
        new_out[u] = []
    for v in cut_in:
        new_in[v] = []
    comp = [-1] * m.V                                  # BFS; an edge counts only where both lists still hold it
    c = 0
    for s in range(m.V):
        if comp[s] >= 0:
            continue
        comp[s] = c
        stack = [s]
        while stack:
            x = stack.pop()
            for y in new_out[x]:
                if x in new_in[y] and comp[y] < 0:
                    comp[y] = c; stack.append(y)
            for y in new_in[x]:
                if x in new_out[y] and comp[y] < 0:
                    comp[y] = c; stack.append(y)
        c += 1
    gone = [(u, e["v2"]) for u in range(m.V) for e in m.adj[u] if comp[u] != comp[e["v2"]]]
    for u, v in gone:
        m.remove(u, v)
    stats["branch_edges"] = len(gone)


def find_cycles(m, order, randomize):
    """findCycles / dfs_helper (GraphAlgos.cpp:352-506), the recursion as a loop -> set of back edges."""
    visited, marked, back = [False] * m.V, [False] * m.V, set()
    keyf = {1: lambda e: (e["pos1"], e["v2"]), 2: lambda e: (-e["score"], e["v2"]), 3: lambda e: (-e["len"], e["v2"]),
            4: lambda e: (e["mr"], e["v2"])}

    def neighbours(x):
        if randomize in keyf:                       # ties only between equal (target, key) pairs: any sort will do
            return [e["v2"] for e in sorted(m.adj[x], key=keyf[randomize])]
        return random_shuffle([e["v2"] for e in m.adj[x]], randomize)

    for s in order:
        if visited[s]:
            continue
        marked[s] = True
        stack = [(s, neighbours(s), [0])]
        while stack:
            x, nbs, nxt = stack[-1]
            if nxt[0] < len(nbs):
                y = nbs[nxt[0]]
                nxt[0] += 1
                if marked[y]:
                    back.add((x, y))
                elif not visited[y]:
                    marked[y] = True
                    stack.append((y, neighbours(y), [0]))
            else:
                marked[x], visited[x] = False, True
                stack.pop()
    return back


def build(singles, overlaps, scores=None, **opts):
    """Vertices and edges as process_overlaps leaves them -> (model, inclusions, stats)."""
    o = dict(STAGEB)
    o.update(opts)
    stats = dict.fromkeys(STATS, 0)
    seqs, quals, index = read_singles(singles)
    m = Model(seqs)
    m.index = index
    cands, _, _ = OV.parse_overlaps(overlaps, o["min_overlap_len"], o["min_overlap_perc"], False, o["max_overlaps"])
    if scores is None:
        scores = score_candidates(cands, seqs, quals, index, o)
    inclusions, _ = build_edges(m, cands, scores, o, stats)
    return m, inclusions, stats


def score_candidates(cands, seqs, quals, index, o):
    return [OV.single_single_edge(seqs[index[c["id1"]]], quals[index[c["id1"]]], seqs[index[c["id2"]]],
                                  quals[index[c["id2"]]], c["pos1"], c["ori1"] == "+", c["ori2"] == "+",
                                  o["mismatch"], o["min_read_len"]) for c in cands]


def graph(singles, overlaps, out_dir, scores=None, trans_branch=None, **opts):
    """The whole --graph_only run (ViralQuasispecies.cpp:250-398) -> stats dict; writes out_dir's files.  scores: the
    (score, mismatch rate, pos3) per candidate when the caller has them (oracle/vq.py's scoring is slow in Python)."""
    o = dict(STAGEB)
    o.update(opts)
    os.makedirs(out_dir, exist_ok=True)
    stats = dict.fromkeys(STATS, 0)
    seqs, quals, index = read_singles(singles)
    m = Model(seqs)
    m.index = index
    stats["vertices"] = m.V
    cands, _, _ = OV.parse_overlaps(overlaps, o["min_overlap_len"], o["min_overlap_perc"], False, o["max_overlaps"])
    assert all(c["type1"] == "s" and c["type2"] == "s" for c in cands), "paired-end candidate"
    if scores is None:
        scores = score_candidates(cands, seqs, quals, index, o)
    inclusions, scored_nonedges = build_edges(m, cands, scores, o, stats)
    with open(os.path.join(out_dir, "nonedge_overlaps.txt"), "w", newline="") as f:
        for c in scored_nonedges + _nonedge_rows(overlaps, o["min_overlap_len"], o["max_overlaps"]):
            f.write(overlap_line(c))
    if stats["edges_built"] == 0:
        return stats
    m.sort_edges()
    label_vertices(m, stats)
    if o["ignore_inclusions"]:
        remove_inclusions(m, inclusions)
    else:
        inclusions = [0] * m.V
    if o["remove_trans"]:
        remove_transitive(m, o["remove_trans"], stats, trans_branch)
    write_gfa(m, os.path.join(out_dir, "graph.gfa"))
    tips = remove_tips(m, o["max_tip_len"], stats) if o["remove_tips"] else set()
    if o["remove_branches"]:
        assert o["remove_trans"] == 1
        remove_branches(m, stats)
    m.sort_edges()
    order = m.by_indegree()
    best = find_cycles(m, order, 1)
    count = 1
    while count < 20 and best:
        count += 1
        cur = find_cycles(m, order, count)
        if len(cur) < len(best):
            best = cur
    stats["backedges"] = len(best)
    cyc = os.path.join(out_dir, "cycles.txt")
    if os.path.exists(cyc):
        os.remove(cyc)
    if best:
        with open(cyc, "w", newline="") as f:
            for u, v in sorted(best):
                if o["remove_backedges"]:
                    m.remove(u, v)
                f.write(f"{u}\t{v}\n")
    count, lines = 0, []                              # writeGraphToFile (OverlapGraph.cpp:322-385)
    for i in range(m.V):
        if inclusions[i]:
            continue
        for e in m.adj[i]:
            j = e["v2"]
            if inclusions[j]:
                continue
            if j < i:
                back_edge = next((x for x in m.adj[j] if x["v2"] == i), None)
                if back_edge is not None and back_edge["score"] > 0:
                    continue
            lines.append(f"{i},{j}\n{j},{i}\n")
            count += 1
    with open(os.path.join(out_dir, "graph.txt"), "w", newline="") as f:
        f.write(f"{m.V}\n{2 * count}\n" + "".join(lines))
    write_gfa(m, os.path.join(out_dir, "graph_trimmed.gfa"))
    with open(os.path.join(out_dir, "digraph.txt"), "w", newline="") as f:
        f.write("".join(f"{i}\t{e['v2']}\n" for i in range(m.V) for e in m.adj[i]))
    with open(os.path.join(out_dir, "tips.txt"), "w", newline="") as f:
        f.write("".join(f"{v}\n" for v in sorted(tips)))
    stats["edges_final"] = m.n_edges()
    return stats


OUTPUTS = ("nonedge_overlaps.txt", "graph.gfa", "graph.txt", "graph_trimmed.gfa", "digraph.txt", "cycles.txt", "tips.txt")
