"""Plain-Python restatement of BranchReduction::readBasedBranchReduction (tools/HaploConduct/src/BranchReduction.cpp) and of
what ViralQuasispecies --branch_reduction=true changes around it: the edges_to_be_deleted rule of removeTransitiveEdges
(GraphAlgos.cpp:967-1077) and the call in place of removeBranches (ViralQuasispecies.cpp:326-351).  Sequential reference,
single-end vertices, diploid off.  The yardstick of hlmi_vq_branch_graph / hlmi_vq_branch_iteration; the library is never its
own.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED, as for every ViralQuasispecies step here (the reference needs Boost).  The text is restated literally, oddities
included; tests/test_vq_branch_model.py pins each with a hand-worked case.

It runs inside vq_graph_model.graph through `Hook`, which patches that module the way vq_next_model._Tap does: the edges it
removes and the missing edges it makes reach a _Tap's branching list in the reference's push order.

Two readings, stated: original_readcount (a command-line number of the reference, joint id = original_readcount + min(id, mate))
is se_count + 2 * pe_count; original_ID_dict.at(node) is read with the vertex's read id, and a run whose ids are not the file
positions is refused (every file this project writes numbers its reads from 0)."""
import os
import sys

import vq_graph_model as G
import vq_merge_model as MM

STATS = ("in_branches", "out_branches", "pairs", "diff_positions", "work_items", "evidence_ids", "missing_edges", "false_branches",
         "inclusion_pairs", "components", "components_kept", "dist_too_large", "scheduled", "edges_removed")
MAX_DIFF = 100

# libstdc++'s __prime_list (hashtable-aux.cc) as far as the model is held to the compiler's container
PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 103, 109, 113, 127, 137,
          139, 149, 157, 167, 179, 193, 199, 211, 227, 241, 257, 277, 293, 313, 337, 359, 383, 409, 439, 467, 503, 541, 577, 619,
          661, 709, 761, 823, 887, 953, 1031, 1109, 1193, 1289, 1381, 1493, 1613, 1741, 1879, 2029, 2179, 2357, 2549, 2753, 2971,
          3209, 3469, 3739, 4027, 4349, 4703, 5087, 5503, 5953, 6427, 6949, 7517, 8123, 8783, 9497, 10273, 11113, 12011, 12983)


def umap_order(keys):
    """The iteration order of a std::unordered_map<unsigned, T> of libstdc++ after insert() of `keys` (distinct) in this order:
    identity hash, bucket = key % bucket count; a node goes to the head of its bucket's run, into an empty bucket at the head of
    the whole list (_M_insert_bucket_begin); _Prime_rehash_policy: the first insert allocates 13 buckets (max(n, 11) + 1 -> the
    next listed prime), a later one that would exceed the count allocates the next listed prime >= 2 * count, and a rehash
    re-inserts the nodes in list order by the same rule (_M_rehash_aux)."""
    def insert(order, key, n):
        b = key % n
        for i, k in enumerate(order):
            if k % n == b:
                order.insert(i, key)
                return
        order.insert(0, key)

    order, n_bkt, next_resize = [], 1, 0
    for key in keys:
        n_elt = len(order)
        if n_elt + 1 > next_resize:
            min_bkts = max(n_elt + 1, 0 if next_resize else 11)
            if min_bkts >= n_bkt:
                want = max(min_bkts + 1, n_bkt * 2)
                n_bkt = next(p for p in PRIMES if p >= want)  # (StopIteration: past the table)
                old, order = order, []
                for k in old:
                    insert(order, k, n_bkt)
            next_resize = n_bkt                               # floor(bucket count * max_load_factor 1.0)
        insert(order, key, n_bkt)
    return order


def read_table(path):
    """:132-159: '#' and empty lines skipped, column 1 = dist, column 3 = min evidence, std::stoi each (leading blanks, a sign,
    digits; what follows is ignored; nothing to convert: refused).  Every line goes into ONE stringstream whose clear() resets
    flags only: what a line holds behind its third tab stays unread and goes in front of the next line's first column."""
    def stoi(s):
        t = s.lstrip(" \t\n\v\f\r")
        k = 1 if t[:1] in "+-" and t[:1] else 0
        j = k
        while j < len(t) and t[j].isdigit() and t[j].isascii():
            j += 1
        if j == k:
            raise ValueError(f"stoi: {s!r}")
        v = int(t[:j])
        if not -2 ** 31 <= v < 2 ** 31:
            raise ValueError(f"stoi: {s!r} out of range")
        return v

    table, carry = {}, ""
    with open(path, newline="") as f:
        for line in f.read().split("\n"):
            if not line or line[0] == "#":
                continue
            cols = (carry + line).split("\t", 3)
            carry = cols[3] if len(cols) == 4 else ""
            cols = cols[:3]
            cols += [cols[-1]] * (3 - len(cols))              # getline at the end of the stream leaves tmp as it was
            table[stoi(cols[0])] = stoi(cols[2])
    return table


def find_diff_pos(a, b):
    """findDiffPos (:693-713): the first 100 positions where two strings of one length differ."""
    out = []
    for k in range(len(a)):
        if a[k] != b[k]:
            out.append(k)
            if len(out) == MAX_DIFF:
                break
    return out


def check_read_evidence(contig, startpos, read, index, diff_list):
    """checkReadEvidence (:716-743)."""
    ok = False
    read_start = startpos + index
    read_end = read_start + len(read)
    for d in diff_list:
        if d < read_start or d >= read_end:
            continue
        if d < startpos or d >= startpos + len(contig):
            continue
        if read[d - read_start] != contig[d - startpos]:
            return False
        ok = True
    return ok


def _int32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


class Reduction:
    """One BranchReduction object.  m: a vq_graph_model.Model; orient[v]: the labelling; originals[v]: {original id: (forward,
    index1, len)}; oseq: {original id: sequence} of the original FASTQ."""

    def __init__(self, m, orient, originals, oseq, se_count, pe_count, table, careful=True, min_overlap_len=0, edge_threshold=1.0):
        self.m, self.orient, self.originals, self.oseq = m, orient, originals, oseq
        self.se, self.pe, self.table, self.careful = se_count, pe_count, table, careful
        self.mol, self.threshold = min_overlap_len, edge_threshold
        self.readcount = se_count + 2 * pe_count
        self.evidence = {}                                    # evidence_per_edge
        self.false_in, self.false_out = set(), set()
        self.missing = []                                     # missing_edges
        self.components = []                                  # branching_components
        self.report = []                                      # the lines of branch_components.txt
        self.stats = dict.fromkeys(STATS, 0)

    def edge(self, u, v):                                     # getEdgeInfo(u, v, false)
        return next(e for e in self.m.adj[u] if e["v2"] == v)

    def oriented(self, v, by):                                # :414-419, :556-561: by the BRANCHING vertex's label
        s = self.m.seqs[v]
        return s if self.orient[by] else MM.revcomp(s)

    # ---- buildDiffListOut / buildDiffListIn (:396-689) ------------------------------------------------------------------
    def _missing_edge(self, e_first, e_second, side, v1, v2, rel, ln, size_i, size_j):
        self.missing.append(dict(v1=v1, v2=v2, pos1=rel, pos2=0, pos3=0, pos4=0, ori1=e_first["ori" + side], ori2=e_second["ori" + side],
                                 len=ln, perc=(100 * ln) // min(size_i, size_j), score=self.threshold, mr=0.0, k=e_first["k"],
                                 ord="-"))

    def diff_list(self, node1, nbs, outbranch):
        """-> (sorted unique diff list, dist, sequences, startpos, inclusion pairs)."""
        if outbranch:
            edges = [self.edge(node1, v) for v in nbs]
            start = [e["pos1"] for e in edges]
            pos_vec = None
        else:
            edges = [self.edge(v, node1) for v in nbs]
            pos_vec = [e["pos1"] for e in edges]
            start = [max(pos_vec) - p for p in pos_vec]       # startpos = max_pos - pos
            node1_len = len(self.m.seqs[node1])
        seqs = [self.oriented(v, node1) for v in nbs]
        side = "2" if outbranch else "1"
        diffs, dists, inclusions = [], [], []
        for i in range(len(nbs)):
            for j in range(i + 1, len(nbs)):
                si, sj, pi, pj = seqs[i], seqs[j], start[i], start[j]
                if pi < pj:
                    rel, a, b, startpos = pj - pi, i, j, pj
                else:
                    rel, a, b, startpos = pi - pj, j, i, pi
                # the sequence that starts first is `a`; :449 / :461: relative_pos > int(size - min_overlap_len), size_t arithmetic
                if rel > _int32((len(seqs[a]) - self.mol) & 0xFFFFFFFFFFFFFFFF):
                    assert outbranch, "in-branches can't be the result of inclusions (:605)"
                    inclusions.append((nbs[a], nbs[b]))
                    self.stats["inclusion_pairs"] += 1
                    continue
                ln = min(len(seqs[a]) - rel, len(seqs[b]))
                sub_a, sub_b = seqs[a][rel:rel + ln], seqs[b][:ln]
                if not outbranch:
                    sub_a, sub_b = sub_a[::-1], sub_b[::-1]
                dp = find_diff_pos(sub_a, sub_b)
                self.stats["pairs"] += 1
                self.stats["diff_positions"] += len(dp)
                diffs += [p + startpos for p in dp] if outbranch else [ln - p + startpos for p in dp]
                if not dp:                                    # identical overlap: a missing edge and a false branch
                    first, second = (i, j) if pi < pj or (pi == pj and nbs[i] < nbs[j]) else (j, i)
                    self._missing_edge(edges[first], edges[second], side, nbs[first], nbs[second], rel, ln, len(si), len(sj))
                    (self.false_out if outbranch else self.false_in).add(node1)
                elif i == 0:                                  # distance_vec is fed by the pairs of the first neighbour alone
                    if outbranch:
                        dists.append(dp[0] + startpos)
                    else:
                        overlap_len = min(len(si) - pos_vec[i], len(sj) - pos_vec[j])
                        dists.append(dp[0] + node1_len - overlap_len)
        dist = int(0.5 * (min(dists) + max(dists))) if dists else 0
        return sorted(set(diffs)), dist, seqs, start, inclusions

    # ---- findBranchingEvidence (:229-394) ---------------------------------------------------------------------------------
    def branch_evidence(self, node1, nbs, outbranch):
        """-> (final_branch, dist)."""
        final = [node1] + list(nbs)
        diff_list, dist, seqs, start, inclusions = self.diff_list(node1, nbs, outbranch)
        sub1 = self.originals[node1]
        per_nb = {}
        for node2, contig, startpos in zip(nbs, seqs, start):
            ev = []
            for sid, (forward, index, _) in self.originals[node2].items():
                self.stats["work_items"] += 1
                if sid >= self.se + self.pe:
                    mate = sid - self.pe
                elif sid >= self.se:
                    mate = sid + self.pe
                else:
                    mate = None
                if sid in sub1 or (mate is not None and mate in sub1):
                    read = self.oseq[sid]                     # :306: the mate branch reads the subread itself again
                    ok = check_read_evidence(contig, startpos, read if forward else MM.revcomp(read), index, diff_list)
                    if ok and sid in sub1:
                        ev.append(sid)
                    if ok and mate is not None and mate in sub1:
                        ev.append(self.readcount + min(sid, mate))
            per_nb[node2] = sorted(set(ev))
            self.stats["evidence_ids"] += len(per_nb[node2])
        for included, _ in inclusions:                        # :328-335
            per_nb[included] = []
            if len(nbs) == 2:
                final = []
            elif included in final:
                final.remove(included)
        it = 1
        for nb in nbs:
            if it < len(final) and nb == final[it]:
                key = (node1, nb) if outbranch else (nb, node1)
                if key in self.evidence:                      # the second visit intersects, in the existing list's order
                    self.evidence[key] = [x for x in self.evidence[key] if x in per_nb[nb]]
                else:
                    self.evidence[key] = list(per_nb[nb])
                it += 1
        assert it == len(final) or not final
        return final, dist

    # ---- findBranchingComponents (:745-1007) ------------------------------------------------------------------------------
    def find_components(self, final_in, final_out, to_remove):
        seqs = self.m.seqs
        in_map = {b[0]: b[1:] for b, _ in final_in if b}
        out_map = {b[0]: b[1:] for b, _ in final_out if b}
        in_dist = {b[0]: d for b, d in final_in if b}
        out_dist = {b[0]: d for b, d in final_out if b}
        seen_in, seen_out = dict.fromkeys(in_map, False), dict.fromkeys(out_map, False)
        false = [False]

        def extend_out(comp, nbs):
            got, hit = (0, nbs[0]), False
            for node in nbs:
                if node not in seen_out or seen_out[node]:
                    continue
                if node in self.false_out:
                    false[0] = True
                branch = out_map[node]
                got, hit = (out_dist[node], node), True
                comp += [(node, w) for w in branch]
                seen_out[node] = True
                extend_in(comp, branch)
            return got if hit else (0, nbs[0])

        def extend_in(comp, nbs):
            for node in nbs:
                if node not in seen_in or seen_in[node]:
                    continue
                if node in self.false_in:
                    false[0] = True
                branch = in_map[node]
                comp += [(w, node) for w in branch]
                seen_in[node] = True
                extend_out(comp, branch)

        for node in umap_order(list(in_map)):                 # in_map was filled in ascending vertex order
            if seen_in[node]:
                continue
            nbs = in_map[node]
            comp = [(w, node) for w in nbs]
            false[0] = node in self.false_in
            seen_in[node] = True
            dist1 = in_dist[node]
            dist2, outnode = extend_out(comp, nbs)
            e = self.edge(outnode, node)
            len1, len2, ol = len(seqs[outnode]), len(seqs[node]), e["len"]
            if ol < 100:
                dist1 = max(dist1, len2 - ol + 100)
                dist2 = max(dist2, len1 - ol + 100)
            else:
                dist1, dist2 = max(dist1, len2), max(dist2, len1)
            dist = dist1 + dist2 - len1 - len2 + ol
            comp = sorted(set(comp))
            if false[0]:
                to_remove += comp
            else:
                self.components.append((comp, dist))
        for node in umap_order(list(out_map)):
            if seen_out[node]:
                continue
            nbs = out_map[node]
            comp = [(node, w) for w in nbs]
            dist1 = out_dist[node]
            e = self.edge(node, nbs[0])
            len1, len2, ol = len(seqs[node]), len(seqs[nbs[0]]), e["len"]
            if ol < 100:
                dist1, dist2 = max(dist1, len1 - ol + 100), len2 - ol + 100
            else:
                dist1, dist2 = max(dist1, len1), len2
            dist = dist1 + dist2 - len1 - len2 + ol
            if node in self.false_out:
                to_remove += comp
            else:
                self.components.append((comp, dist))
            seen_out[node] = True

    # ---- countUniqueEvidence (:1009-1272), diploid off -------------------------------------------------------------------
    def count_unique(self, comp, min_evidence, to_remove):
        """-> (keep, unique count per edge of comp).  The order of unique_evidence_per_edge (an unordered_map) decides only the
        order in which edges reach edges_to_remove, which is sorted before use; with diploid off nothing else reads it."""
        unique = {e: [] for e in comp}
        live = [bool(self.evidence[e]) for e in comp]
        while any(live):
            fronts = sorted(self.evidence[e][0] for e, l in zip(comp, live) if l)
            cur = fronts[0]
            unique_min = len(fronts) == 1 or cur < fronts[1]  # only a strictly unique minimum counts
            for k, e in enumerate(comp):
                if live[k] and self.evidence[e][0] == cur:
                    if unique_min:
                        unique[e].append(cur)
                    self.evidence[e].pop(0)
                    if not self.evidence[e]:
                        live[k] = False
        keep = False
        counts = []
        for e in comp:
            n = len(set(unique[e]))
            counts.append(n)
            if n < min_evidence:
                to_remove.append(e)
            else:
                keep = True
        return keep, counts

    # ---- readBasedBranchReduction (:41-227) --------------------------------------------------------------------------------
    def run(self):
        """-> (missing edges, removed edges): what is pushed to branching_edges, in push order."""
        m = self.m
        ins = [sorted(l) for l in m.in_lists()]               # sortAdjLists(adj_in)
        m.sort_adj_out()                                      # sortAdjOut sorts adj_out itself
        outs = [[e["v2"] for e in l] for l in m.adj]
        branch_out = [v for v in range(m.V) if len(outs[v]) > 1]
        branch_in = [v for v in range(m.V) if len(ins[v]) > 1]
        self.stats["in_branches"], self.stats["out_branches"] = len(branch_in), len(branch_out)
        final_in = [([], 0)] * m.V
        final_out = [([], 0)] * m.V
        for v in branch_in:
            b = self.branch_evidence(v, ins[v], False)
            if b[0]:
                final_in[v] = b
        for v in branch_out:
            b = self.branch_evidence(v, outs[v], True)
            if b[0]:
                final_out[v] = b
        self.stats["missing_edges"] = len(self.missing)
        self.stats["false_branches"] = len(self.false_in) + len(self.false_out)
        to_remove = []
        self.find_components(final_in, final_out, to_remove)
        self.stats["components"] = len(self.components)
        neighbours = []
        if self.careful:
            of_node = {}
            for idx, (comp, _) in enumerate(self.components):
                for u, v in comp:
                    of_node.setdefault(u, set()).add(idx)
                    of_node.setdefault(v, set()).add(idx)
            for comp, _ in self.components:
                neighbours.append(set().union(*(of_node[u] | of_node[v] for u, v in comp)))
        else:
            neighbours = [set() for _ in self.components]
        kept = set()
        for idx, (comp, dist) in enumerate(self.components):
            threshold, flag, counts = self.table.get(dist, -1), 0, [-1] * len(comp)
            if any(c != idx and c in kept for c in neighbours[idx]):
                to_remove += comp                             # next to a kept component
            elif dist in self.table:
                keep, counts = self.count_unique(comp, threshold, to_remove)
                if keep:
                    kept.add(idx)
                    flag = 1
            else:
                self.stats["dist_too_large"] += 1
                to_remove += comp
            self.report.append(f"{dist}\t{threshold}\t{flag}" + "".join(f"\t{u}>{v}:{n}" for (u, v), n in zip(comp, counts)) + "\n")
        self.stats["components_kept"] = len(kept)
        to_remove = sorted(set(to_remove))
        self.stats["edges_removed"] = len(to_remove)
        return self.missing, to_remove


# ---- removeTransitiveEdges with edges_to_be_deleted (GraphAlgos.cpp:938-1077) ----------------------------------------------
def remove_transitive_scheduling(m, rounds, stats, branch=None, scheduled_out=None):
    """vq_graph_model.remove_transitive plus the 3-clique rule (:967-993) in both removal branches (:995-1077).  The two differ
    where a list holds two edges to one target: the rebuild drops every scheduled copy, the one-by-one branch the first one."""
    assert rounds == 1
    m.sort_adj_out()
    trans = G.transitive_targets(m, 1)
    count = sum(len(l) for l in trans)
    stats["transitive"] = count
    scheduled = set()
    ins = m.in_lists()
    for u in range(m.V):
        for v in trans[u]:
            ovlen = next(e for e in m.adj[u] if e["v2"] == v)["len"]
            scheduled.update((u, e["v2"]) for e in m.adj[u] if e["len"] <= ovlen)
            scheduled.update((w, v) for w in ins[v] if next(e for e in m.adj[w] if e["v2"] == v)["len"] <= ovlen)
    if scheduled_out is not None:
        scheduled_out.append(len(scheduled))
    if branch is None:
        branch = 1.0 * count > 0.5 * m.n_edges()
    if branch:
        for u in range(m.V):
            t, keep = list(trans[u]), []
            for e in m.adj[u]:
                if t and e["v2"] == t[0]:
                    t.pop(0)
                elif (u, e["v2"]) not in scheduled:
                    keep.append(e)
            m.adj[u] = keep
    else:
        for u in range(m.V):
            for v in trans[u]:
                m.remove(u, v)
        for u, v in sorted(scheduled):
            if any(e["v2"] == v for e in m.adj[u]):
                m.remove(u, v)


def read_fastq_by_id(path):
    seqs, _, index = G.read_singles(path)
    return {rid: seqs[v] for rid, v in index.items()}, len(seqs)


class Hook:
    """While vq_graph_model.graph runs (directly, or under vq_clique_next_model.clique_iteration): --branch_reduction=true.
    Enter it OUTSIDE a _Tap, so that the tap wraps what it installs.  After the run: stats, report (branch_components.txt)."""

    def __init__(self, original_fastq, se_count, pe_count, table_path, careful=True, first_it=False, subreads_in=None,
                 min_overlap_len=G.STAGEB["min_overlap_len"], edge_threshold=G.STAGEB["edge_threshold"]):
        self.table = read_table(table_path)
        self.oseq, n = read_fastq_by_id(original_fastq)
        assert se_count + 2 * pe_count == n, "se_count + 2 * pe_count is not the number of original reads"
        self.se, self.pe, self.careful = se_count, pe_count, careful
        self.mol, self.threshold = min_overlap_len, edge_threshold
        self.dict = None if first_it else MM.read_subreads(subreads_in)
        self.stats, self.report, self.ran = dict.fromkeys(STATS, 0), [], False

    def __enter__(self):
        self.saved = (G.Model.sort_edges, G.Model.remove, G.remove_transitive, G.label_vertices)
        sort_edges, remove, _, label = self.saved
        hook = self
        hook.labels, hook.sorts, hook.scheduled = None, {}, []

        def tapped_label(m, stats):                           # the labels of the best try: the first with the fewest deletions
            tries = []
            gfile = G.graph.__code__.co_filename
            old = sys.getprofile()

            def prof(frame, event, arg):
                if event == "return" and frame.f_code.co_filename == gfile and frame.f_code.co_name == "one_try" and arg is not None:
                    tries.append((list(frame.f_locals["labels"]), len(arg[1])))
                if old is not None:
                    old(frame, event, arg)

            sys.setprofile(prof)
            try:
                r = label(m, stats)
            finally:
                sys.setprofile(old)
            assert tries, "vq_graph_model.label_vertices: one_try renamed"
            hook.labels = min(tries, key=lambda t: t[1])[0]
            return r

        def trans(m, rounds, stats, branch=None):
            return remove_transitive_scheduling(m, rounds, stats, branch, hook.scheduled)

        def tapped_remove(m, u, v, opposite=None):
            if isinstance(opposite, dict):                    # a missing edge on its way to branching_edges: nothing is removed
                return opposite
            return remove(m, u, v, opposite)

        def tapped_sort(m):
            n = hook.sorts[id(m)] = hook.sorts.get(id(m), 0) + 1
            if n == 2:                                        # ViralQuasispecies.cpp:359: the reduction ran just in front of it
                hook.reduce(m)
            return sort_edges(m)

        G.Model.sort_edges, G.Model.remove, G.remove_transitive, G.label_vertices = tapped_sort, tapped_remove, trans, tapped_label
        return self

    def __exit__(self, *exc):
        G.Model.sort_edges, G.Model.remove, G.remove_transitive, G.label_vertices = self.saved

    def reduce(self, m):
        ids = [None] * m.V
        for rid, v in m.index.items():
            ids[v] = rid
        assert ids == list(range(m.V)), "read ids are not the file positions"
        if self.dict is None:
            originals = [{v: (True, 0, len(m.seqs[v]))} for v in range(m.V)]
        else:
            originals = [{k: tuple(o) for k, o in self.dict[v].items()} for v in range(m.V)]
        for o in originals:
            assert all(k in self.oseq for k in o), "an original id outside the original FASTQ"
        r = Reduction(m, self.labels, originals, self.oseq, self.se, self.pe, self.table, self.careful, self.mol, self.threshold)
        missing, removed = r.run()
        for e in missing:
            m.remove(e["v1"], e["v2"], e)                     # (push only: see tapped_remove)
        for u, v in removed:
            m.remove(u, v)
        self.stats, self.report, self.ran = dict(r.stats, scheduled=self.scheduled[-1] if self.scheduled else 0), r.report, True


def branch_graph(singles, overlaps, subreads_in, original_fastq, table_path, out_dir, se_count, pe_count, careful=True,
                 first_it=False, scores=None, **opts):
    """hlmi_vq_branch_graph's yardstick -> (graph stats, branch stats); writes the graph's files and branch_components.txt."""
    assert opts.get("remove_trans", 1) == 1 and not opts.get("remove_branches", False)
    o = dict(G.STAGEB, **{k: v for k, v in opts.items() if k in G.STAGEB})
    with Hook(original_fastq, se_count, pe_count, table_path, careful, first_it, subreads_in, o["min_overlap_len"],
              o["edge_threshold"]) as h:
        gstats = G.graph(singles, overlaps, out_dir, scores=scores, **dict(opts, remove_trans=1, remove_branches=False))
    assert h.ran or gstats["edges_built"] == 0, "vq_graph_model.graph: the second sort_edges of a model was not reached"
    if h.ran:
        with open(os.path.join(out_dir, "branch_components.txt"), "w", newline="") as f:
            f.write("".join(h.report))
    return gstats, h.stats
