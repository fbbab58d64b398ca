// vq_graph_host.cpp - SURVEY 8f rank 3: the oriented, reduced overlap graph of ViralQuasispecies --graph_only=true
// (tools/HaploConduct/src, ViralQuasispecies.cpp:250-398) for HyLight's stage b.  Host side: the candidates and their
// order, the order-dependent steps (sortEdges, sortAdjOut, the labelling BFS, the cycle DFS) and the writers.  The two
// input files are parsed by vq_front.hip (read_singles, vq_parse_overlaps), each once per call; the per-edge / per-vertex
// steps are in vq_graph.hip.  The contract is the sequential reference (--threads 1).
// PARITY UNPINNED: the reference needs Boost and cannot be built here; tests/vq_graph_model.py restates it.
//
// The adjacency lists hold edge ids (the reference's std::list<Edge>); adj_in is rebuilt from them where it is read:
// after sortEdges the reference's adj_in is exactly that rebuild, and everywhere else only its contents count (removeTips
// collects sets, removeBranches sorts it, sortVerticesByIndegree takes sizes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "common.h"
#include "graph.h"
#include "paf_io.h"
#include "vq_internal.h"

namespace hlmi {
namespace {

// Overlap::get_overlap_line (Overlap.h:222-225)
void overlap_line(std::string &s, const hlmi_vq_overlap &o) {
    s += std::to_string(o.id1); s += '\t'; s += std::to_string(o.id2); s += '\t';
    s += std::to_string(o.pos1); s += '\t'; s += std::to_string(o.pos2); s += '\t';
    s += o.ord; s += '\t'; s += o.ori1; s += '\t'; s += o.ori2; s += '\t';
    s += std::to_string(o.perc1); s += '\t'; s += std::to_string(o.perc2); s += '\t';
    s += std::to_string(o.len1); s += '\t'; s += std::to_string(o.len2); s += '\t';
    s += o.type1; s += '\t'; s += o.type2; s += '\n';
}

// std::random_shuffle as libstdc++ implements it (bits/stl_algo.h: for i = 1 .. n-1, j = rand() % (i + 1), swap) after
// srand(seed), with glibc's srand / rand - written out because std::random_shuffle is deprecated.  The reference seeds
// before EVERY shuffle, so the permutation depends on (seed, size) only and is cached per size.
class Shuffler {
public:
    explicit Shuffler(unsigned seed) : seed_(seed) {}
    void apply(std::vector<uint32_t> &a) {
        const size_t n = a.size();
        if (n < 2) return;
        std::vector<uint32_t> &p = perm_[n];
        if (p.empty()) {
            p.resize(n);
            for (size_t i = 0; i < n; ++i) p[i] = (uint32_t)i;
            srand(seed_);
            for (size_t i = 1; i < n; ++i) {
                const size_t j = (size_t)rand() % (i + 1);
                if (i != j) std::swap(p[i], p[j]);
            }
        }
        std::vector<uint32_t> b(n);
        for (size_t i = 0; i < n; ++i) b[i] = a[p[i]];
        a.swap(b);
    }
private:
    unsigned seed_;
    std::unordered_map<size_t, std::vector<uint32_t>> perm_;
};

// ---- the graph ------------------------------------------------------------------------------------------------------------
struct Graph {
    uint32_t V = 0;
    std::vector<VqEdge> pool;                     // edges by id (a moved edge gets a new id)
    std::vector<std::vector<uint32_t>> out;       // adj_out: edge ids in list order
    std::vector<uint32_t> rlen;                   // read length per vertex

    size_t edge_count() const {
        size_t n = 0;
        for (const auto &l : out) n += l.size();
        return n;
    }
    // CSR of the out-lists in list order: off[V + 1], src / dst / edge id per position
    void flatten(std::vector<uint32_t> &off, std::vector<uint32_t> &src, std::vector<uint32_t> &dst, std::vector<uint32_t> &eid) const {
        off.assign((size_t)V + 1, 0);
        src.clear(); dst.clear(); eid.clear();
        for (uint32_t u = 0; u < V; ++u) {
            off[u] = (uint32_t)eid.size();
            for (uint32_t e : out[u]) { src.push_back(u); dst.push_back(pool[e].v2); eid.push_back(e); }
        }
        off[V] = (uint32_t)eid.size();
    }
    // drop the positions p of a flatten() with gone[p] != 0: every list keeps its order.  -> how many went
    size_t drop(const std::vector<uint8_t> &gone, const std::vector<uint32_t> &src, const std::vector<uint32_t> &eid) {
        size_t n_gone = 0;
        for (auto &l : out) l.clear();
        for (size_t p = 0; p < gone.size(); ++p) {
            if (gone[p]) ++n_gone;
            else out[src[p]].push_back(eid[p]);
        }
        return n_gone;
    }
    // adj_in as sortEdges rebuilds it (OverlapGraph.cpp:753-763): sources in vertex order, then list order
    std::vector<std::vector<uint32_t>> adj_in() const {
        std::vector<std::vector<uint32_t>> in(V);
        for (uint32_t u = 0; u < V; ++u)
            for (uint32_t e : out[u]) in[pool[e].v2].push_back(u);
        return in;
    }
    std::vector<uint32_t> indegree() const {
        std::vector<uint32_t> d(V, 0);
        for (const auto &l : out)
            for (uint32_t e : l) ++d[pool[e].v2];
        return d;
    }
    // Edge::get_nonoverlap_len: unsigned arithmetic, as the reference's
    uint32_t nonoverlap(const VqEdge &e) const { return rlen[e.v1] + rlen[e.v2] - 2u * (uint32_t)e.len; }
    // removeEdgeWithOri / removeEdge: the first u -> v of u's list (of the orientation class, when given)
    bool erase_first(uint32_t u, uint32_t v, int opposite) {
        auto &l = out[u];
        for (size_t k = 0; k < l.size(); ++k) {
            const VqEdge &e = pool[l[k]];
            if (e.v2 == v && (opposite < 0 || (int)(e.ori1 == e.ori2) == opposite)) {
                l.erase(l.begin() + (ptrdiff_t)k);
                return true;
            }
        }
        return false;
    }
};

// sortEdges (OverlapGraph.cpp:722-764): std::sort of (edge, non-overlap length) by (length, target).  The key ties when one
// pair holds an edge in both orientation classes with one length, and std::sort is not stable: the order of such a tie is
// whatever libstdc++'s introsort makes of the input sequence, so this is the host's std::sort on the same sequence with the
// same comparator (a device sort is not guaranteed to agree).
void sort_edges(Graph &g) {
    for (auto &l : g.out) {
        std::vector<std::pair<uint32_t, uint32_t>> pairs;                  // (edge id, non-overlap length)
        pairs.reserve(l.size());
        for (uint32_t e : l) pairs.emplace_back(e, g.nonoverlap(g.pool[e]));
        std::sort(pairs.begin(), pairs.end(), [&](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) {
            if (a.second == b.second) return g.pool[a.first].v2 < g.pool[b.first].v2;
            return a.second < b.second;
        });
        for (size_t k = 0; k < l.size(); ++k) l[k] = pairs[k].first;
    }
}

// sortAdjOut (GraphAlgos.cpp:806-833), which removeTransitiveEdges and removeBranches call for its side effect on adj_out:
// std::sort of (target, edge) by target only - again not stable for two edges to one target, so again the host's std::sort.
void sort_adj_out(Graph &g) {
    for (auto &l : g.out) {
        std::vector<std::pair<unsigned long, uint32_t>> pairs;
        pairs.reserve(l.size());
        for (uint32_t e : l) pairs.emplace_back((unsigned long)g.pool[e].v2, e);
        std::sort(pairs.begin(), pairs.end(), [](const std::pair<unsigned long, uint32_t> &a, const std::pair<unsigned long, uint32_t> &b) {
            return a.first < b.first;
        });
        for (size_t k = 0; k < l.size(); ++k) l[k] = pairs[k].second;
    }
}

// sortVerticesByIndegree (GraphAlgos.cpp:150-176): (in-degree, vertex) - a total order
std::vector<uint32_t> vertices_by_indegree(const Graph &g) {
    const std::vector<uint32_t> d = g.indegree();
    std::vector<uint32_t> v(g.V);
    for (uint32_t i = 0; i < g.V; ++i) v[i] = i;
    std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return d[a] == d[b] ? a < b : d[a] < d[b]; });
    return v;
}

// ---- vertexLabellingHeuristic (GraphAlgos.cpp:178-248) -----------------------------------------------------------------
struct Labelling { size_t conflicts = 0, moved = 0; std::vector<uint8_t> orient; };   // orient: vertex_orientations (:247)

Labelling label_vertices(Graph &g) {
    const uint32_t V = g.V;
    const std::vector<std::vector<uint32_t>> in = g.adj_in();
    const std::vector<uint32_t> order = vertices_by_indegree(g);
    std::vector<uint32_t> off, src, dst, eid;
    g.flatten(off, src, dst, eid);
    std::vector<VqEdge> flat(eid.size());
    for (size_t p = 0; p < eid.size(); ++p) flat[p] = g.pool[eid[p]];
    VqLabelPass pass(flat);

    // getEdgeInfo(node, neighbour) with reverse_allowed: the first edge node -> neighbour in node's list, else the first
    // neighbour -> node; only its orientation class (ori1 == ori2) is read, and an in-place flip does not change it
    auto same_class = [&](uint32_t a, uint32_t b) -> bool {
        for (uint32_t e : g.out[a]) if (g.pool[e].v2 == b) return g.pool[e].ori1 == g.pool[e].ori2;
        for (uint32_t e : g.out[b]) if (g.pool[e].v2 == a) return g.pool[e].ori1 == g.pool[e].ori2;
        fail(HLMI_EINVAL, "vq_graph: labelling found no edge %u - %u", a, b);
    };
    // labelVertices (:250-349): BFS from the vertices in sortVerticesByIndegree order; every vertex's neighbour list (its
    // adj_in, then its adj_out targets) is shuffled after srand(seed).  A start vertex keeps the label `orient` already
    // holds: all ones in the first two tries, and from the third try on the previous try's labels, because the reference
    // reuses that bitset and resize() does not reset it.
    std::vector<uint8_t> visited(V);
    std::vector<uint32_t> queue, nb;
    queue.reserve(V);
    auto bfs = [&](unsigned seed, std::vector<uint8_t> &orient) {
        Shuffler sh(seed);
        std::fill(visited.begin(), visited.end(), 0);
        for (uint32_t start : order) {
            if (visited[start]) continue;
            visited[start] = 1;
            queue.clear();
            queue.push_back(start);
            for (size_t qi = 0; qi < queue.size(); ++qi) {
                const uint32_t node = queue[qi];
                nb.assign(in[node].begin(), in[node].end());
                for (uint32_t e : g.out[node]) nb.push_back(g.pool[e].v2);
                sh.apply(nb);
                for (uint32_t w : nb) {
                    if (visited[w]) continue;
                    visited[w] = 1;
                    queue.push_back(w);
                    orient[w] = same_class(node, w) ? orient[node] : (uint8_t)!orient[node];
                }
            }
        }
    };
    std::vector<uint8_t> cls;
    std::vector<uint32_t> best_del;                    // positions deleted by the best try
    std::vector<VqEdge> best_del_e, best_moved;        // the edges as that try saw them; moved: flipped copies
    auto record = [&]() {
        const std::vector<VqEdge> st = pass.state();
        best_del_e.clear();
        best_moved.clear();
        for (size_t p = 0; p < cls.size(); ++p) {
            if (cls[p] == 1) best_del_e.push_back(st[p]);
            else if (cls[p] == 2) { VqEdge e = st[p]; switch_orientation(e); best_moved.push_back(e); }
        }
    };
    std::vector<uint8_t> opt(V, 1), cur(V, 1);
    bfs(1, opt);
    pass.run(opt, cls);
    record();
    size_t delete_count = best_del_e.size();
    for (int count = 1; count < 100 && delete_count > 0;) {          // k = 100 tries
        ++count;
        bfs((unsigned)count, cur);
        pass.run(cur, cls);
        size_t n_del = 0;
        for (uint8_t c : cls) n_del += c == 1;
        if (n_del < delete_count) {                                     // the first try with the fewest deletions wins
            record();
            delete_count = n_del;
            opt = cur;                                                  // opt_orientations = orientations (:211)
        }
    }
    // the in-place flips of every try stay (Edge::switch_edge_orientation on the listed edge, :341)
    const std::vector<VqEdge> st = pass.state();
    for (size_t p = 0; p < eid.size(); ++p) g.pool[eid[p]] = st[p];
    // moves first, in the winning try's order (adj_out order): removeEdgeWithOri(v, u) then addEdge appends to the list of
    // the new source - so a moved edge ends its new list, and graph.gfa shows it there (:220-226)
    for (const VqEdge &m : best_moved) {
        if (!g.erase_first(m.v2, m.v1, m.ori1 == m.ori2)) fail(HLMI_EINVAL, "vq_graph: moved edge not found");
        g.pool.push_back(m);
        g.out[m.v1].push_back((uint32_t)(g.pool.size() - 1));
    }
    for (const VqEdge &d : best_del_e)                                  // then the conflicting edges (:233-238)
        if (!g.erase_first(d.v1, d.v2, d.ori1 == d.ori2)) fail(HLMI_EINVAL, "vq_graph: conflicting edge not found");
    Labelling r;
    r.conflicts = delete_count;
    r.moved = best_moved.size();
    r.orient = std::move(opt);
    return r;
}

// ---- findCycles / cycleRemovalHeuristic (GraphAlgos.cpp:352-541) ---------------------------------------------------------
// dfs_helper is recursive in the reference; a path of 1e5 vertices would overflow a thread's stack, so this is the same
// visit order with an explicit stack: a frame is (vertex, its neighbours in visit order, next index).
std::set<std::pair<uint32_t, uint32_t>> find_cycles(const Graph &g, const std::vector<uint32_t> &order, int randomize) {
    const uint32_t V = g.V;
    std::vector<uint8_t> visited(V), marked(V);
    std::set<std::pair<uint32_t, uint32_t>> back;
    Shuffler sh((unsigned)randomize);
    // neighbour order (:378-474): 1 by pos1, 2 by score (descending), 3 by overlap length (descending), 4 by mismatch rate,
    // each then by target; from 5 on the list order shuffled after srand(randomize) - one srand per visited vertex
    auto neighbours = [&](uint32_t node) {
        std::vector<uint32_t> r;
        const auto &l = g.out[node];
        if (randomize >= 1 && randomize <= 4) {
            std::vector<std::pair<uint32_t, uint32_t>> pe;            // (target, edge id)
            for (uint32_t e : l) pe.emplace_back(g.pool[e].v2, e);
            std::sort(pe.begin(), pe.end(), [&](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) {
                const VqEdge &x = g.pool[a.second], &y = g.pool[b.second];
                switch (randomize) {
                    case 1: if (x.pos1 != y.pos1) return x.pos1 < y.pos1; break;
                    case 2: if (x.score != y.score) return x.score > y.score; break;
                    case 3: if (x.len != y.len) return x.len > y.len; break;
                    default: if (x.mr != y.mr) return x.mr < y.mr; break;
                }
                return a.first < b.first;
            });
            for (auto &p : pe) r.push_back(p.first);
        } else {
            for (uint32_t e : l) r.push_back(g.pool[e].v2);
            sh.apply(r);
        }
        return r;
    };
    struct Frame { uint32_t node; std::vector<uint32_t> nb; size_t next; };
    std::vector<Frame> stack;
    auto visit = [&](uint32_t parent, uint32_t node) {
        if (marked[node]) {
            back.insert(std::make_pair(parent, node));      // a back edge: node is on the current path
        } else if (!visited[node]) {
            marked[node] = 1;
            stack.push_back(Frame{node, neighbours(node), 0});
        }
    };
    for (uint32_t i : order) {
        if (visited[i]) continue;
        visit(V, i);
        while (!stack.empty()) {
            Frame &f = stack.back();
            if (f.next < f.nb.size()) {
                const uint32_t w = f.nb[f.next++];
                visit(f.node, w);                            // (may grow the stack: f is not used after this)
            } else {
                marked[f.node] = 0;
                visited[f.node] = 1;
                stack.pop_back();
            }
        }
    }
    return back;
}

// ---- writers (OverlapGraph.cpp:322-410, 468-543) -------------------------------------------------------------------------
void write_gfa(const Graph &g, const Singles &reads, const std::string &path) {
    std::string s = "H\tVN:Z:1.0\n";
    for (uint32_t i = 0; i < g.V; ++i) {
        s += "S\t"; s += std::to_string(i); s += '\t'; s += reads.seq[i]; s += '\n';
        for (uint32_t e : g.out[i]) {                    // contained or not, the link line is the same
            s += "L\t"; s += std::to_string(i); s += "\t+\t"; s += std::to_string(g.pool[e].v2); s += "\t+\t";
            s += std::to_string(g.pool[e].len); s += "M\n";
        }
    }
    write_file(path, s.data(), s.size());
}

// writeGraphToFile: undirected edge lines for quick-cliques.  An included vertex and edges into one are left out; an edge
// i -> j with j < i is left out when checkEdge(j, i, false) - the score of the first j -> i - is positive.
void write_graph_txt(const Graph &g, const std::vector<uint8_t> &incl, const std::string &path) {
    std::string body;
    uint64_t count = 0;
    for (uint32_t i = 0; i < g.V; ++i) {
        if (incl[i]) continue;
        for (uint32_t e : g.out[i]) {
            const uint32_t j = g.pool[e].v2;
            if (incl[j]) continue;
            if (j < i) {
                bool skip = false;
                for (uint32_t f : g.out[j])
                    if (g.pool[f].v2 == i) { skip = g.pool[f].score > 0; break; }
                if (skip) continue;
            }
            body += std::to_string(i); body += ','; body += std::to_string(j); body += '\n';
            body += std::to_string(j); body += ','; body += std::to_string(i); body += '\n';
            ++count;
        }
    }
    const std::string s = std::to_string(g.V) + "\n" + std::to_string(2 * count) + "\n" + body;
    write_file(path, s.data(), s.size());
}

void write_digraph(const Graph &g, const std::string &path) {
    std::string s;
    for (uint32_t i = 0; i < g.V; ++i)
        for (uint32_t e : g.out[i]) { s += std::to_string(i); s += '\t'; s += std::to_string(g.pool[e].v2); s += '\n'; }
    write_file(path, s.data(), s.size());
}

// ---- what findNextOverlaps reads beside the graph (for_next) -----------------------------------------------------------
// FindNextOverlaps.cpp:661-691: a score-0 source edge per row of nonedge_overlaps.txt.  A paired-end row is refused.
std::vector<VqSrcEdge> nonedge_src_edges(const std::vector<const hlmi_vq_overlap *> &rows, const Singles &reads) {
    std::vector<VqSrcEdge> r;
    for (const hlmi_vq_overlap *c : rows) {
        if (c->type1 != 's' || c->type2 != 's')
            fail(HLMI_ESTATE, "vq_iteration: a non-edge overlap row has a paired-end read; HyLight builds none (--num_pairs 0)");
        const auto i1 = reads.index_of.find(c->id1), i2 = reads.index_of.find(c->id2);
        if (i1 == reads.index_of.end() || i2 == reads.index_of.end())
            fail(HLMI_EINVAL, "vq_iteration: a non-edge overlap row names a read that is not in %s", reads.path.c_str());
        VqSrcEdge s{};
        s.v1 = i1->second; s.v2 = i2->second;
        s.pos1 = (int32_t)c->pos1; s.pos2 = (int32_t)c->pos2;
        s.len1 = (int32_t)c->len1; s.len2 = (int32_t)c->len2;
        s.perc = (int32_t)vq_perc(*c);
        s.ori1 = c->ori1 == '+'; s.ori2 = c->ori2 == '+';
        s.score0 = 1;
        s.ord = c->ord;
        r.push_back(s);
    }
    return r;
}

// inclusion_edges (GraphAlgos.cpp:26-42) per included vertex: its out-edges, then getEdgeInfo per in-neighbour
void inclusion_src_edges(const Graph &g, const std::vector<uint8_t> &incl, VqGraphState &keep) {
    const std::vector<std::vector<uint32_t>> in = g.adj_in();
    keep.incl_off.push_back(0);
    for (uint32_t v = 0; v < g.V; ++v) {
        if (!incl[v]) continue;
        for (uint32_t e : g.out[v]) keep.incl_edges.push_back(vq_src_edge(g.pool[e]));
        for (uint32_t u : in[v])
            for (uint32_t e : g.out[u])
                if (g.pool[e].v2 == v) { keep.incl_edges.push_back(vq_src_edge(g.pool[e])); break; }
        keep.incl_off.push_back((uint32_t)keep.incl_edges.size());
    }
}

}  // namespace

void vq_graph_opts_stageb(hlmi_vq_graph_opts *o) {
    *o = hlmi_vq_graph_opts{};
    o->min_overlap_len = 300;
    o->min_overlap_perc = 0;
    o->min_read_len = 0;
    o->max_tip_len = 1000;
    o->remove_trans = 1;
    o->edge_threshold = 1;
    o->ov_threshold = 0.9;
    o->merge_contigs = 0;
    o->mismatch = 0;
    o->ignore_inclusions = 1;
    o->remove_tips = 1;
    o->remove_branches = 1;
    o->remove_backedges = 1;
    o->max_overlaps = 100000000;
}

void vq_graph_run(const char *fastq, const char *overlaps, const hlmi_vq_graph_opts &o, const char *out_dir, hlmi_vq_graph_stats *st,
                  VqGraphState *keep, bool for_next, VqBranchRun *branch) {
    if (o.remove_trans > 3) fail(HLMI_EINVAL, "vq_graph: remove_trans must be 0 .. 3");
    if (o.remove_branches && o.remove_trans != 1)
        fail(HLMI_ESTATE, "vq_graph: remove_branches needs remove_trans 1 (findBranchfreeGraph asserts it, GraphAlgos.cpp:716)");
    *st = hlmi_vq_graph_stats{};
    if (for_next && !keep) fail(HLMI_EINVAL, "vq_graph: for_next needs a state to keep what findNextOverlaps reads");
    Singles reads = read_singles(fastq);
    if (keep) {
        *keep = VqGraphState{};
        vq_merge_check_reads(reads.seq, reads.qual);      // refused inputs are refused before a file is written
    }
    if (reads.seq.size() >= (1u << 31)) fail(HLMI_EINVAL, "vq_graph: more than 2^31 reads");
    if (branch) branch->prepare(o, reads);               // --branch_reduction=true: its refusals come before the first write
    Graph g;
    g.V = (uint32_t)reads.seq.size();
    g.out.resize(g.V);
    for (const auto &s : reads.seq) g.rlen.push_back((uint32_t)s.size());
    st->vertices = g.V;

    // candidates (EdgeCalculator.cpp:561-666): HyLight's path has no paired-end reads (--num_pairs 0, relax_PE_edges off)
    uint64_t n_nonedge = 0, n_skipped = 0;
    std::vector<hlmi_vq_overlap> cand, nonedge;
    vq_parse_overlaps(overlaps, o.min_overlap_len, o.min_overlap_perc, 0, o.max_overlaps, cand, &nonedge, &n_nonedge, &n_skipped);
    const uint64_t n_cand = cand.size();
    for (uint64_t k = 0; k < n_cand; ++k)
        if (cand[k].type1 != 's' || cand[k].type2 != 's')
            fail(HLMI_ESTATE, "vq_graph: overlap candidate %llu has a paired-end read; HyLight builds no paired-end edges "
                              "(--num_pairs 0)", (unsigned long long)k);
    if (n_cand >= (1ull << 32)) fail(HLMI_EINVAL, "vq_graph: more than 2^32 candidates");
    std::vector<double> score(n_cand), mr(n_cand);
    std::vector<int64_t> pos3(n_cand);
    if (n_cand) vq_score_overlaps(reads, cand.data(), n_cand, o.mismatch, o.min_read_len, score.data(), mr.data(), pos3.data());

    // process_overlaps (:389-419): edge when score > edge_threshold, or when the mismatch rate is known and <= merge_contigs;
    // otherwise kept as a non-edge when score > ov_threshold
    std::vector<VqEdge> edges;
    std::string ne_text;
    std::vector<const hlmi_vq_overlap *> ne_rows;        // for_next: the rows of nonedge_overlaps.txt in file order
    for (uint64_t k = 0; k < n_cand; ++k) {
        const hlmi_vq_overlap &c = cand[k];
        if (score[k] > o.edge_threshold || (mr[k] != -1 && mr[k] <= o.merge_contigs)) {
            VqEdge e{};
            e.v1 = reads.index_of.at(c.id1);
            e.v2 = reads.index_of.at(c.id2);
            e.pos1 = (int32_t)c.pos1; e.pos2 = (int32_t)c.pos2;
            e.pos3 = (int32_t)pos3[k]; e.pos4 = 0;
            e.ori1 = c.ori1 == '+'; e.ori2 = c.ori2 == '+';
            e.len = (int32_t)c.len1;
            e.perc = (int32_t)vq_perc(c);
            e.cand = (uint32_t)k;
            e.pad[0] = (uint8_t)c.ord;
            e.score = score[k]; e.mr = mr[k];
            if (e.pos1 == 0 && e.v1 > e.v2) {            // :443-448: an overlap at position 0 goes from the smaller vertex
                std::swap(e.v1, e.v2);
                std::swap(e.ori1, e.ori2);
                e.pos3 = -e.pos3;
                e.pos4 = -e.pos4;
            }
            if (e.perc == 100) ++st->inclusions;         // inclusion_count (:449-451)
            edges.push_back(e);
        } else if (score[k] > o.ov_threshold && mr[k] != -1) {
            overlap_line(ne_text, c);
            if (for_next) ne_rows.push_back(&c);
        }
    }
    // nonedge_overlaps.txt (:533-541, :654-661): each chunk of 1e6 candidates appends its scored non-edges, in candidate
    // order, and the parser's non-edges follow at the end - so all scored non-edges in file order, then the parser's
    for (const auto &c : nonedge) overlap_line(ne_text, c);
    if (for_next) {
        for (const auto &c : nonedge) ne_rows.push_back(&c);
        keep->nonedge = nonedge_src_edges(ne_rows, reads);
    }
    write_file(join_path(out_dir, "nonedge_overlaps.txt"), ne_text.data(), ne_text.size());
    st->candidates = edges.size();

    std::vector<uint32_t> winners;
    std::vector<uint8_t> incl;
    vq_select_edges(edges, g.V, o.ignore_inclusions != 0, winners, incl);
    st->edges_built = winners.size();
    st->duplicates = st->candidates - st->edges_built;
    if (winners.empty()) {                                // ViralQuasispecies.cpp:282-291: nothing to be done
        remove(join_path(out_dir, "graph.txt").c_str());
        return;
    }
    // adjacency order: a replacement removes the old edge and appends the new one (:522-530), so each list holds its
    // winners in the order of their file index
    g.pool.reserve(winners.size() + 16);
    for (uint32_t w : winners) {
        g.pool.push_back(edges[w]);
        g.out[edges[w].v1].push_back((uint32_t)(g.pool.size() - 1));
    }

    sort_edges(g);                                        // ViralQuasispecies.cpp:301
    const Labelling lab = label_vertices(g);
    st->conflicts = lab.conflicts;
    st->moved = lab.moved;

    // the reductions: the lists flattened, the positions that go flagged on the device, the lists without them
    std::vector<uint32_t> off, src, dst, eid;
    std::vector<uint8_t> gone;
    if (o.ignore_inclusions) {                            // removeInclusions
        if (for_next) inclusion_src_edges(g, incl, *keep);
        g.flatten(off, src, dst, eid);
        vq_inclusion_removed(off, src, dst, incl, gone);
        g.drop(gone, src, eid);
    } else {
        std::fill(incl.begin(), incl.end(), 0);
    }

    if (branch) {                                         // removeTransitiveEdges with edges_to_be_deleted (:967-993)
        sort_adj_out(g);
        g.flatten(off, src, dst, eid);
        std::vector<uint32_t> ovlen(eid.size());
        for (size_t p = 0; p < eid.size(); ++p) ovlen[p] = (uint32_t)g.pool[eid[p]].len;
        std::vector<uint8_t> flags(eid.size(), 0);
        uint64_t n_trans = 0;
        vq_transitive_edges(g.V, eid.size(), src.data(), dst.data(), ovlen.data(), 1, flags.data(), &n_trans);
        st->transitive = n_trans;
        std::set<std::pair<uint32_t, uint32_t>> scheduled;
        for (size_t p = 0; p < eid.size(); ++p) if (flags[p] & 2) scheduled.insert(std::make_pair(src[p], dst[p]));
        branch->st->scheduled = scheduled.size();
        gone.assign(eid.size(), 0);
        for (size_t p = 0; p < eid.size(); ++p) gone[p] = flags[p] & 1;
        if (1.0 * (double)n_trans > 0.5 * (double)eid.size()) {
            // :995-1061, the rebuild: a transitive edge is skipped, and so is EVERY other edge whose (source, target) is scheduled
            for (size_t p = 0; p < eid.size(); ++p) if (scheduled.count(std::make_pair(src[p], dst[p]))) gone[p] = 1;
            g.drop(gone, src, eid);
        } else {
            // :1063-1076, one by one: the transitive edges, then per scheduled pair in std::set order the FIRST edge still there.
            // The two branches differ only where a list holds two edges to one target, one of them scheduled and not transitive
            g.drop(gone, src, eid);
            for (const auto &pr : scheduled) g.erase_first(pr.first, pr.second, -1);
        }
    } else if (o.remove_trans) {                          // removeTransitiveEdges (GraphAlgos.cpp:938-1077)
        sort_adj_out(g);
        g.flatten(off, src, dst, eid);
        st->transitive = vq_trans_flags(g.V, src, dst, (int)o.remove_trans, gone);
        // the reference rebuilds adj_out when more than half of the edges go and erases them one by one otherwise; both
        // leave the sortAdjOut order minus the transitive edges (each listed target is matched once, and two edges to one
        // target are both listed), so one compaction stands for both
        g.drop(gone, src, eid);
    }
    write_gfa(g, reads, join_path(out_dir, "graph.gfa"));

    std::vector<uint8_t> tip(g.V, 0);
    if (o.remove_tips) {                                  // removeTips
        g.flatten(off, src, dst, eid);
        std::vector<uint32_t> in_off((size_t)g.V + 1, 0), in_src(dst.size()), fill((size_t)g.V, 0), fwd(dst.size()), bwd(dst.size());
        for (uint32_t v : dst) ++in_off[v + 1];
        for (uint32_t v = 0; v < g.V; ++v) in_off[v + 1] += in_off[v];
        for (size_t p = 0; p < dst.size(); ++p) in_src[in_off[dst[p]] + fill[dst[p]]++] = src[p];
        for (size_t p = 0; p < dst.size(); ++p) {
            const VqEdge &e = g.pool[eid[p]];
            fwd[p] = (uint32_t)std::max((int)g.rlen[e.v2] - e.len, 0);   // Edge::ext_len(true), single-end
            bwd[p] = (uint32_t)(e.pos1 + e.pos2);                         // Edge::ext_len(false), ord '-'
        }
        vq_tips(g.V, off, dst, in_off, in_src, fwd, bwd, o.max_tip_len, gone, tip);
        if (for_next) {                                   // :630-636: a std::set of (source, target), one removeEdge each
            std::vector<uint32_t> order;
            for (uint32_t p = 0; p < gone.size(); ++p) if (gone[p]) order.push_back(p);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                return src[a] != src[b] ? src[a] < src[b] : dst[a] < dst[b];
            });
            for (uint32_t p : order) keep->branching.push_back(vq_src_edge(g.pool[eid[p]]));
        }
        st->tip_edges = g.drop(gone, src, eid);
    }
    for (uint8_t t : tip) st->tip_reads += t;

    if (branch) {                                         // readBasedBranchReduction in removeBranches' place (:326-347)
        sort_adj_out(g);                                  // sortAdjOut sorts adj_out itself (BranchReduction.cpp:48)
        std::vector<std::vector<VqEdge>> lists(g.V);
        for (uint32_t u = 0; u < g.V; ++u)
            for (uint32_t e : g.out[u]) lists[u].push_back(g.pool[e]);
        std::vector<VqEdge> missing;
        std::vector<std::pair<uint32_t, uint32_t>> removed;
        std::string report;
        branch->reduce(o, reads.seq, reads.id, lists, lab.orient, missing, removed, report);
        // branching_edges: the missing edges (:83-85), then each removed edge as it stood (:217-225)
        if (for_next) for (const VqEdge &e : missing) keep->branching.push_back(vq_src_edge(e));
        for (const auto &pr : removed) {
            if (for_next)
                for (uint32_t e : g.out[pr.first])
                    if (g.pool[e].v2 == pr.second) { keep->branching.push_back(vq_src_edge(g.pool[e])); break; }
            if (!g.erase_first(pr.first, pr.second, -1)) fail(HLMI_EINVAL, "vq_branch: edge %u -> %u not found", pr.first, pr.second);
        }
        write_file(join_path(out_dir, "branch_components.txt"), report.data(), report.size());
    } else if (o.remove_branches) {                       // removeBranches
        sort_adj_out(g);
        g.flatten(off, src, dst, eid);
        std::vector<uint32_t> comp;
        vq_branch_components(g.V, src, dst, comp);
        gone.assign(src.size(), 0);                       // the cross-component edges of the current graph go (:917-931)
        for (size_t p = 0; p < src.size(); ++p) gone[p] = comp[src[p]] != comp[dst[p]];
        if (for_next)                                     // :918-931: vertices ascending, list order
            for (size_t p = 0; p < src.size(); ++p)
                if (gone[p]) keep->branching.push_back(vq_src_edge(g.pool[eid[p]]));
        st->branch_edges = g.drop(gone, src, eid);
    }

    sort_edges(g);                                        // ViralQuasispecies.cpp:352
    {
        const std::vector<uint32_t> order = vertices_by_indegree(g);
        std::set<std::pair<uint32_t, uint32_t>> best = find_cycles(g, order, 1);
        for (int count = 1; count < 20 && !best.empty();) {                 // up to 20 tries; the first smallest set wins
            ++count;
            std::set<std::pair<uint32_t, uint32_t>> cur = find_cycles(g, order, count);
            if (cur.size() < best.size()) best.swap(cur);
        }
        st->backedges = best.size();
        // cycles.txt: findCycles removes it, reportCycle appends the winning set in std::set order
        const std::string cyc = join_path(out_dir, "cycles.txt");
        remove(cyc.c_str());
        if (!best.empty()) {
            std::string s;
            for (const auto &pr : best) {
                if (o.remove_backedges) {
                    if (for_next)                         // reportCycle (OverlapGraph.cpp:548-560) pushes the removed edge
                        for (uint32_t e : g.out[pr.first])
                            if (g.pool[e].v2 == pr.second) { keep->branching.push_back(vq_src_edge(g.pool[e])); break; }
                    g.erase_first(pr.first, pr.second, -1);
                }
                s += std::to_string(pr.first); s += '\t'; s += std::to_string(pr.second); s += '\n';
            }
            write_file(cyc, s.data(), s.size());
        }
    }
    write_graph_txt(g, incl, join_path(out_dir, "graph.txt"));
    write_gfa(g, reads, join_path(out_dir, "graph_trimmed.gfa"));
    write_digraph(g, join_path(out_dir, "digraph.txt"));
    {
        std::string s;
        for (uint32_t v = 0; v < g.V; ++v) if (tip[v]) { s += std::to_string(v); s += '\n'; }
        write_file(join_path(out_dir, "tips.txt"), s.data(), s.size());
    }
    st->edges_final = g.edge_count();
    if (keep) {                                           // what SRBuilder reads (vq_superread_run.cpp)
        const auto unsorted = g.out;                      // what the --cliques=true branch walks: it never runs the sort below
        sort_edges(g);                                    // ViralQuasispecies.cpp:434, in front of mergeAlongEdges
        keep->built = true;
        keep->out.resize(g.V);
        for (uint32_t u = 0; u < g.V; ++u)
            for (uint32_t e : g.out[u]) keep->out[u].push_back(g.pool[e]);
        if (for_next && unsorted != g.out) {              // a tie moved: only findNextOverlaps behind the cliques reads this
            keep->out_unsorted.resize(g.V);
            for (uint32_t u = 0; u < g.V; ++u)
                for (uint32_t e : unsorted[u]) keep->out_unsorted[u].push_back(g.pool[e]);
        }
        keep->orient = lab.orient;
        keep->incl = incl;
        keep->tip = tip;
        keep->seq = std::move(reads.seq);
        keep->qual = std::move(reads.qual);
        keep->id = std::move(reads.id);
    }
}

}  // namespace hlmi
