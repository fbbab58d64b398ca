// vq_next.hip - SRBuilder::findNextOverlaps with --FNO=1 --optimize=false --threads 1, behind mergeAlongEdges and behind
// cliquesToSuperreads (tools/HaploConduct/src, FindNextOverlaps.cpp:25-327 updateOverlap, :331-347 findCliqueIndex, :351-385
// the S-S branch of computeOverlapData, :605-631, :635-697, :816-887, :890-958; ViralQuasispecies.cpp:449-479): the overlaps
// of the next iteration.  The reference pushes every source edge through updateOverlap, which loops over the super-reads of
// u, of v or over their product (nodes_to_SR, :896-913), and inserts each line as text into a std::set<std::string>; here a
// thread per source edge counts its loop turns, one scan numbers them - the number IS the reference's loop order -, a thread
// per turn (a candidate) works out case, ids and claim key, a stable radix sort of (key, candidate number) and its run heads
// decide the claims, a thread per line writes the text, and LSD radix passes over the lines' 8-byte big-endian words order
// them.  After a merge every list has one entry at the most and a candidate is a source edge: case_kernel makes the candidate
// records directly, as it did before the lists (count, scan and search cost the merge iteration 0.4 of its 2.1 ms, DESIGN.md
// 4.3d); everything behind the records is one code for both callers.  The rules are in include/hylight_mi.h.
// PARITY UNPINNED: the reference needs Boost and cannot be built here; tests/vq_next_model.py restates it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "common.h"
#include "dec_text.h"
#include "dev_prims.h"
#include "vq_internal.h"

namespace hlmi {
namespace {

using namespace vqn;
using vqk::grid1;

constexpr uint64_t NO_KEY = ~0ull;
enum { C_COPIED = 0, C_U2SR, C_V2SR, C_SR2SR, C_FAILED, C_MAXLEN, C_COUNT };

struct Tab {                                     // VqNextTables and the vertex labels, on the device
    const uint32_t *start, *id, *len;            // list of vertex v: entries [start[v], start[v + 1]); len per NEW read id
    const int32_t *idx;                          // findCliqueIndex per entry: signed
    const uint8_t *copied, *orient;              // per vertex
};
struct Cand {                                    // one turn of updateOverlap's loops (a copied edge: its one turn)
    uint32_t edge;                               // its source edge
    uint32_t id1, id2;                           // the new reads standing for u and for v
    int32_t idx1, idx2;                          // where u lies in id1, v in id2
    uint32_t kase;                               // 0 nothing (:255), 1 copied (:47), 2 u not in a super-read (:73), 3 v not (:151), 4 both (:229)
};
struct Graph {                                   // the final graph's edges as sorted (source << 32 | target) keys
    const uint64_t *key;                         // ascending; equal keys in list order (stable sort)
    const uint32_t *val;                         // position in the flattened out-lists
    const uint8_t *positive;                     // per position: the edge's score is > 0
    uint32_t n;
};
struct Line {                                    // the numbers of one line of overlaps.txt; kind 0: no line
    uint32_t a, b;
    int32_t pos1, pos2, perc, len1, len2;
    char ord, o1, o2;
    uint8_t kind;
};

// OverlapGraph::checkEdge(v, w, reverse allowed) (OverlapGraph.cpp:233-258) reduced to what its two callers test: -1 no
// edge v -> w and no edge w -> v; else whether the score of the first v -> w of v's list - failing that of the first
// w -> v - is positive
__device__ inline int check_edge(const Graph &g, uint32_t v, uint32_t w) {
    const uint64_t want[2] = {(uint64_t)v << 32 | w, (uint64_t)w << 32 | v};
    for (int d = 0; d < 2; ++d) {
        uint32_t lo = 0, hi = g.n;
        for (int it = 0; it < SEARCH_STEPS && lo < hi; ++it) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (g.key[mid] < want[d]) lo = mid + 1; else hi = mid;
        }
        if (lo < g.n && g.key[lo] == want[d]) return g.positive[g.val[lo]] ? 1 : 0;
    }
    return -1;
}

// rows of nonedge_overlaps.txt: valid[first + i] = 0 when checkEdge(v1, v2, true) > 0 (FindNextOverlaps.cpp:694-696)
__global__ void nonedge_check_kernel(const VqSrcEdge *rec, uint32_t first, uint32_t n, Graph g, uint8_t *valid) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const VqSrcEdge e = rec[first + i];
    valid[first + i] = check_edge(g, e.v1, e.v2) > 0 ? 0 : 1;
}

// findInclusionOverlaps (:816-887): thread t = pair (list, i, j) in the reference's loop order; pstart[l] = pairs of the
// lists in front of l, pstart[n_lists] = n_pairs
__global__ void induce_kernel(const VqSrcEdge *le, const uint32_t *loff, const uint64_t *pstart, uint32_t n_lists,
                              uint64_t n_pairs, const uint32_t *rlen, uint8_t score0, Graph g, VqSrcEdge *rec, uint32_t first,
                              uint8_t *valid) {
    const uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (t >= n_pairs) return;
    uint32_t lo = 0, hi = n_lists;                           // pstart[lo] <= t < pstart[hi]
    for (int it = 0; it < SEARCH_STEPS && hi - lo > 1; ++it) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pstart[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t base = loff[lo];
    const uint64_t L = loff[lo + 1] - base, p = t - pstart[lo];
    // row i holds the pairs (i, i + 1 .. L - 1); S(i) = i (2 L - i - 1) / 2 pairs lie in front of it
    uint32_t ilo = 0, ihi = (uint32_t)(L - 1);               // S(ilo) <= p < S(ihi)
    for (int it = 0; it < SEARCH_STEPS && ihi - ilo > 1; ++it) {
        const uint64_t mid = ilo + (ihi - ilo) / 2;
        if (mid * (2 * L - mid - 1) / 2 <= p) ilo = (uint32_t)mid; else ihi = (uint32_t)mid;
    }
    const uint64_t i = ilo, j = i + 1 + (p - i * (2 * L - i - 1) / 2);
    valid[first + t] = 0;
    if (j >= L) return;                                      // (cannot be: p < the list's pair count)
    const VqSrcEdge e1 = le[base + i], e2 = le[base + j];
    VqSrcEdge r{};
    if (e1.v1 == e2.v1) return;                              // :841-843
    if (e1.v1 == e2.v2) {                                    // :844-852
        r.v1 = e2.v1; r.v2 = e1.v2; r.pos1 = e2.pos1; r.ori1 = e2.ori1; r.ori2 = e1.ori2;
    } else if (e1.v2 == e2.v1) {                             // :853-861
        r.v1 = e1.v1; r.v2 = e2.v2; r.pos1 = e1.pos1; r.ori1 = e1.ori1; r.ori2 = e2.ori2;
    } else {
        return;                                              // :862-865
    }
    const int32_t l1 = (int32_t)rlen[r.v1], l2 = (int32_t)rlen[r.v2];
    const int32_t len = l1 - r.pos1 < l2 ? l1 - r.pos1 : l2;   // :870
    r.perc = (100 * len) / (l1 < l2 ? l1 : l2);              // :871, integers
    r.len1 = len; r.len2 = 0; r.pos2 = 0;
    r.score0 = score0; r.ord = '-';
    rec[first + t] = r;
    valid[first + t] = check_edge(g, r.v1, r.v2) == -1 ? 1 : 0;      // :876
}

__global__ void count_flags_kernel(const uint8_t *flag, uint32_t first, uint32_t n, uint32_t *out) {
    __shared__ uint32_t c;
    if (threadIdx.x == 0) c = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n && flag[first + i]) atomicAdd(&c, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && c) atomicAdd(out, c);
}

// loop turns of updateOverlap per source edge: |list(u)| * |list(v)| - an unvisited vertex is a list of one, its copied read;
// a visited vertex in no super-read is an empty list (nodes_to_SR.at() holds nothing) - and 0 for an edge that is left out.
// cnt has n + 1 entries, the last one 0: their exclusive scan ends in the total.  A product is capped at 2^32, which the
// total then reaches: the caller refuses it, and n < 2^32 such terms cannot wrap 64 bits.
__global__ void count_kernel(const VqSrcEdge *rec, const uint8_t *valid, uint32_t n, Tab t, uint64_t *cnt) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i > n) return;
    uint64_t c = 0;
    if (i < n && valid[i]) {
        const VqSrcEdge e = rec[i];
        c = (uint64_t)(t.start[e.v1 + 1] - t.start[e.v1]) * (t.start[e.v2 + 1] - t.start[e.v2]);
        if (c > (1ull << 32)) c = 1ull << 32;
    }
    cnt[i] = c;
}

// One turn of updateOverlap for source edge `edge` = e: entry i of u's list against entry j of v's -> its record and the pair
// it claims in overlaps_found (NO_KEY without a claim); true when the turn counts as a candidate (a claim is made)
__device__ inline bool make_cand(const Tab &t, const VqSrcEdge &e, uint32_t edge, uint32_t i, uint32_t j, Cand &k, uint64_t &claim) {
    const bool cu = t.copied[e.v1], cv = t.copied[e.v2];
    k.edge = edge;
    k.id1 = t.id[i]; k.id2 = t.id[j];
    k.idx1 = t.idx[i]; k.idx2 = t.idx[j];
    k.kase = 0;
    claim = NO_KEY;
    if (cu && cv) { k.kase = 1; return false; }
    if (!cu && !cv && k.id1 == k.id2) return false;              // :255 id1 == id2 is skipped before the claim
    k.kase = cu ? 2 : cv ? 3 : 4;
    claim = (uint64_t)min(k.id1, k.id2) << 32 | max(k.id1, k.id2);
    return true;
}

// Every list holds one entry at the most (always so behind a merge): a source edge has one turn or none and is its own
// candidate.  One thread per source edge, as before the lists; no count, no scan, no search.
__global__ void case_kernel(const VqSrcEdge *rec, const uint8_t *valid, uint32_t n, Tab t, Cand *cand, uint64_t *key,
                            uint32_t *seq, uint32_t *turns) {
    __shared__ uint32_t c_turns;
    if (threadIdx.x == 0) c_turns = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) {
        Cand k{};
        uint64_t claim = NO_KEY;
        k.edge = i;
        if (valid[i]) {
            const VqSrcEdge e = rec[i];
            const uint32_t su = t.start[e.v1], sv = t.start[e.v2];
            if (t.start[e.v1 + 1] > su && t.start[e.v2 + 1] > sv && make_cand(t, e, i, su, sv, k, claim)) atomicAdd(&c_turns, 1u);
        }
        cand[i] = k;
        key[i] = claim;
        seq[i] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0 && c_turns) atomicAdd(turns, c_turns);
}

// Lists of several entries: one thread per candidate c.  Its source edge is the one with cstart[edge] <= c < cstart[edge + 1]
// (cstart[n] = n_cand), the rest splits into (i, j) = (entry of u's list, entry of v's list), u's list outer as in :233-253;
// seq = c, the reference's loop order
__global__ void expand_kernel(const VqSrcEdge *rec, const uint64_t *cstart, uint32_t n, uint32_t n_cand, Tab t, Cand *cand,
                              uint64_t *key, uint32_t *seq, uint32_t *turns) {
    __shared__ uint32_t c_turns;
    if (threadIdx.x == 0) c_turns = 0;
    __syncthreads();
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c < n_cand) {
        uint32_t lo = 0, hi = n;                                 // cstart[lo] <= c < cstart[hi]
        for (int it = 0; it < SEARCH_STEPS && hi - lo > 1; ++it) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cstart[mid] <= c) lo = mid; else hi = mid;
        }
        const VqSrcEdge e = rec[lo];
        const uint32_t su = t.start[e.v1], sv = t.start[e.v2], nu = t.start[e.v1 + 1] - su, nv = t.start[e.v2 + 1] - sv;
        const uint32_t r = (uint32_t)(c - cstart[lo]);
        Cand k{};
        uint64_t claim = NO_KEY;
        if (nv && r / nv < nu && make_cand(t, e, lo, su + r / nv, sv + r % nv, k, claim)) atomicAdd(&c_turns, 1u);   // (r < nu * nv)
        cand[c] = k;
        key[c] = claim;
        seq[c] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0 && c_turns) atomicAdd(turns, c_turns);
}

// the first candidate of a key owns it (:84-97, :162-175, :261-273)
__global__ void owner_kernel(const uint64_t *key, const uint32_t *seq, const uint32_t *heads, uint32_t runs, uint8_t *owner) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= runs) return;
    const uint32_t h = heads[r];
    if (key[h] != NO_KEY) owner[seq[h]] = 1;
}

__device__ inline uint32_t line_len(const Line &l) {
    return dec_len(l.a) + dec_len(l.b) + dec_len_signed(l.pos1) + dec_len_signed(l.pos2) + dec_len_signed(l.perc) +
           dec_len_signed(l.len1) + dec_len_signed(l.len2) + 6 + 12;      // ord, ori1, ori2, "0", "s", "s"; 12 tabs
}

// one thread per candidate: the copied edges and the owners of a key produce their line's numbers (computeOverlapData)
__global__ void eval_kernel(const VqSrcEdge *rec, const Cand *cand, const uint8_t *owner, uint32_t n, Tab t, int no_incl,
                            Line *line, uint32_t *llen, uint8_t *has, uint32_t *counters) {
    __shared__ uint32_t c[C_COUNT];
    if (threadIdx.x < C_COUNT) c[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) {
        const Cand cd = cand[i];
        const uint32_t k = cd.kase;
        Line l{};
        if (k == 1 || (k >= 2 && owner[i])) {
            const VqSrcEdge e = rec[cd.edge];
            l.o1 = l.o2 = '+';
            if (e.score0) {                                  // :34-37
                l.o1 = e.ori1 == t.orient[e.v1] ? '+' : '-';
                l.o2 = e.ori2 == t.orient[e.v2] ? '+' : '-';
            }
            bool ok = true;
            if (k == 1) {                                    // :49-67
                l.a = cd.id1; l.b = cd.id2;
                l.pos1 = e.pos1; l.pos2 = e.pos2; l.ord = e.ord;
                l.perc = e.perc; l.len1 = e.len1; l.len2 = e.len2;
            } else {                                         // :357-385; a copied read lies at 0 in itself
                const int64_t len1 = t.len[cd.id1], len2 = t.len[cd.id2];
                int64_t np = ((int64_t)e.pos1 + cd.idx1) - cd.idx2, len;
                bool first = true;
                if (np < 0) { first = false; np = -np; len = len2; } else len = len1;
                int64_t ol = len - np;                             // std::min({len - new_pos1, len1, len2})
                if (len1 < ol) ol = len1;
                if (len2 < ol) ol = len2;
                if (np >= len) {
                    ok = false;
                    atomicAdd(&c[C_FAILED], 1u);
                } else {
                    const float f = fmaxf(__fdiv_rn((float)ol, (float)len1), __fdiv_rn((float)ol, (float)len2));
                    l.perc = (int32_t)floorf(__fmul_rn(f, 100.0f));
                    l.a = first ? cd.id1 : cd.id2;
                    l.b = first ? cd.id2 : cd.id1;
                    l.pos1 = (int32_t)np; l.pos2 = 0; l.ord = '-';
                    l.len1 = (int32_t)ol; l.len2 = 0;
                }
            }
            if (ok && !(no_incl && l.perc == 100)) {         // :68, :145, :223, :320
                l.kind = (uint8_t)k;
                atomicAdd(&c[k - 1], 1u);
            }
        }
        uint32_t w = 0;
        if (l.kind) {
            w = line_len(l);
            atomicMax(&c[C_MAXLEN], w);
        }
        line[i] = l;
        llen[i] = w;
        has[i] = l.kind != 0;
    }
    __syncthreads();
    if (threadIdx.x < C_COUNT && c[threadIdx.x]) {
        if (threadIdx.x == C_MAXLEN) atomicMax(&counters[C_MAXLEN], c[C_MAXLEN]);
        else atomicAdd(&counters[threadIdx.x], c[threadIdx.x]);
    }
}

// one thread per line: its text at text[start[i] .. start[i] + llen[i]) (no line end: the order reads the bare string)
__global__ void text_kernel(const Line *line, const uint32_t *llen, const uint64_t *start, uint32_t n, uint8_t *text) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n || !llen[i]) return;
    const Line l = line[i];
    char *o = (char *)text + start[i];
    o = put_dec(o, l.a); *o++ = '\t';
    o = put_dec(o, l.b); *o++ = '\t';
    o = put_dec_signed(o, l.pos1); *o++ = '\t';
    o = put_dec_signed(o, l.pos2); *o++ = '\t';
    *o++ = l.ord; *o++ = '\t';
    *o++ = l.o1; *o++ = '\t';
    *o++ = l.o2; *o++ = '\t';
    o = put_dec_signed(o, l.perc); *o++ = '\t';
    *o++ = '0'; *o++ = '\t';
    o = put_dec_signed(o, l.len1); *o++ = '\t';
    o = put_dec_signed(o, l.len2); *o++ = '\t';
    *o++ = 's'; *o++ = '\t'; *o++ = 's';
}

// key[k] = bytes 8 w .. 8 w + 7 of line perm[k], big-endian, zero behind its end
__global__ void word_kernel(const uint8_t *text, const uint64_t *start, const uint32_t *llen, const uint32_t *perm, uint32_t n,
                            uint32_t w, uint64_t *key) {
    const uint32_t k = blockIdx.x * WG + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = perm[k], len = llen[r];
    const uint8_t *s = text + start[r];
    uint64_t word = 0;
    for (uint32_t b = 0; b < 8; ++b) {
        const uint32_t pos = 8 * w + b;
        word = word << 8 | (pos < len ? s[pos] : 0);
    }
    key[k] = word;
}

// flag[k] = 1 when line perm[k] differs from line perm[k - 1] (sorted: equal lines are neighbours)
__global__ void distinct_kernel(const uint8_t *text, const uint64_t *start, const uint32_t *llen, const uint32_t *perm,
                                uint32_t n, uint8_t *flag) {
    const uint32_t k = blockIdx.x * WG + threadIdx.x;
    if (k >= n) return;
    uint8_t differs = 1;
    if (k > 0) {
        const uint32_t a = perm[k], b = perm[k - 1], len = llen[a];
        if (len == llen[b]) {
            const uint8_t *x = text + start[a], *y = text + start[b];
            differs = 0;
            for (uint32_t i = 0; i < len && i < LINE_WIDTH; ++i) differs |= x[i] != y[i];
        }
    }
    flag[k] = differs;
}

// olen[m] = bytes of output line m = line perm[sel[m]] and its '\n'
__global__ void out_len_kernel(const uint32_t *llen, const uint32_t *perm, const uint32_t *sel, uint32_t n, uint32_t *olen) {
    const uint32_t m = blockIdx.x * WG + threadIdx.x;
    if (m < n) olen[m] = llen[perm[sel[m]]] + 1;
}
__global__ void gather_kernel(const uint8_t *text, const uint64_t *start, const uint32_t *llen, const uint32_t *perm,
                              const uint32_t *sel, const uint64_t *ostart, uint32_t n, uint8_t *image) {
    const uint32_t m = blockIdx.x * WG + threadIdx.x;
    if (m >= n) return;
    const uint32_t r = perm[sel[m]], len = llen[r];
    const uint8_t *s = text + start[r];
    uint8_t *o = image + ostart[m];
    for (uint32_t i = 0; i < len && i < LINE_WIDTH; ++i) o[i] = s[i];
    o[len] = '\n';
}

}  // namespace

std::string vq_next_run(const VqGraphState &g, const std::vector<std::vector<VqEdge>> &out, const VqNextTables &t,
                        double edge_threshold, const hlmi_vq_next_opts &no, hlmi_vq_clique_next_stats *st) {
    const uint32_t V = (uint32_t)g.seq.size();
    // the final graph, flattened in list order: source edges 1, and the keys of the existence test
    std::vector<VqSrcEdge> recs;
    std::vector<uint32_t> src, dst, rlen(V);
    std::vector<uint8_t> positive;
    if (out.size() != V) fail(HLMI_EINVAL, "vq_next: %zu out-lists for %u vertices", out.size(), V);
    for (uint32_t u = 0; u < V; ++u) {
        rlen[u] = (uint32_t)g.seq[u].size();
        for (const VqEdge &e : out[u]) {
            recs.push_back(vq_src_edge(e));
            src.push_back(u); dst.push_back(e.v2); positive.push_back(e.score > 0);
        }
    }
    const size_t n_g = recs.size(), n_b = g.branching.size(), n_ne = g.nonedge.size();
    recs.insert(recs.end(), g.branching.begin(), g.branching.end());
    recs.insert(recs.end(), g.nonedge.begin(), g.nonedge.end());
    const size_t n_lists = g.incl_off.empty() ? 0 : g.incl_off.size() - 1;
    std::vector<uint64_t> pstart(n_lists + 1, 0);
    for (size_t l = 0; l < n_lists; ++l) {
        const uint64_t L = g.incl_off[l + 1] - g.incl_off[l];
        pstart[l + 1] = pstart[l] + L * (L ? L - 1 : 0) / 2;
    }
    const uint64_t n_pairs = pstart[n_lists];
    const uint64_t n64 = (uint64_t)recs.size() + n_pairs;
    if (n64 >= (1ull << 32) - WG) fail(HLMI_EINVAL, "vq_next: %llu source edges (2^32 and more)", (unsigned long long)n64);
    const uint32_t n = (uint32_t)n64, first_ne = (uint32_t)(n_g + n_b), first_pair = (uint32_t)recs.size();
    for (const VqSrcEdge &e : recs)                              // bounds before anything runs on the device
        if (e.v1 >= V || e.v2 >= V) fail(HLMI_EINVAL, "vq_next: a source edge names vertex %u / %u of %u", e.v1, e.v2, V);
    for (const VqSrcEdge &e : g.incl_edges)
        if (e.v1 >= V || e.v2 >= V) fail(HLMI_EINVAL, "vq_next: an inclusion edge names vertex %u / %u of %u", e.v1, e.v2, V);
    vq_next_tables_check(t, V);
    if (g.orient.size() != V) fail(HLMI_EINVAL, "vq_next: the labels do not cover the %u vertices", V);
    st->src_graph = n_g;
    st->src_branching = n_b;
    uint32_t max_entries = 0;
    for (uint32_t v = 0; v < V; ++v) {
        const uint32_t l = t.start[v + 1] - t.start[v];
        max_entries = std::max(max_entries, l);
        if (!t.copied[v]) {
            st->max_list = std::max<uint64_t>(st->max_list, l);
            st->in_several += l >= 2;
        }
    }
    if (!n) return std::string();

    DBuf<uint32_t> d_start, d_id, d_len, d_rlen, d_src, d_dst, d_gval(n_g ? n_g : 1);
    DBuf<int32_t> d_idx;
    DBuf<uint8_t> d_copied, d_orient, d_positive;
    DBuf<uint64_t> d_gkey(n_g ? n_g : 1);
    d_start.upload(t.start); d_id.upload(t.id); d_idx.upload(t.idx); d_len.upload(t.len); d_copied.upload(t.copied);
    d_orient.upload(g.orient);
    d_rlen.upload(rlen);
    const Tab tab{d_start.p, d_id.p, d_len.p, d_idx.p, d_copied.p, d_orient.p};
    if (n_g) {
        d_src.upload(src); d_dst.upload(dst); d_positive.upload(positive);
        hipLaunchKernelGGL(vqk::edge_keys_kernel, grid1(n_g), dim3(WG), 0, stream(), d_src.p, d_dst.p, (const uint32_t *)nullptr, n_g,
                           d_gkey.p, d_gval.p);
        sort_pairs_u64_u32(d_gkey.p, d_gval.p, n_g, 0, 64);      // stable: the edges of one pair stay in list order
    }
    const Graph graph{d_gkey.p, d_gval.p, d_positive.p, (uint32_t)n_g};

    DBuf<VqSrcEdge> d_rec(n);
    DBuf<uint8_t> valid(n);
    DBuf<uint32_t> d_cnt(C_COUNT + 3);
    d_cnt.zero();
    if (!recs.empty()) HIP_CHECK(hipMemcpyAsync(d_rec.p, recs.data(), recs.size() * sizeof(VqSrcEdge), hipMemcpyHostToDevice, stream()));
    HIP_CHECK(hipMemsetAsync(valid.p, 1, n, stream()));
    if (n_ne) {
        hipLaunchKernelGGL(nonedge_check_kernel, grid1(n_ne), dim3(WG), 0, stream(), d_rec.p, first_ne, (uint32_t)n_ne, graph, valid.p);
        hipLaunchKernelGGL(count_flags_kernel, grid1(n_ne), dim3(WG), 0, stream(), valid.p, first_ne, (uint32_t)n_ne, d_cnt.p + C_COUNT);
    }
    DBuf<VqSrcEdge> d_le;
    DBuf<uint32_t> d_loff;
    DBuf<uint64_t> d_pstart;
    if (n_pairs) {
        d_le.upload(g.incl_edges); d_loff.upload(g.incl_off); d_pstart.upload(pstart);
        hipLaunchKernelGGL(induce_kernel, grid1(n_pairs), dim3(WG), 0, stream(), d_le.p, d_loff.p, d_pstart.p, (uint32_t)n_lists,
                           n_pairs, d_rlen.p, (uint8_t)(edge_threshold == 0), graph, d_rec.p, first_pair, valid.p);
        hipLaunchKernelGGL(count_flags_kernel, grid1(n_pairs), dim3(WG), 0, stream(), valid.p, first_pair, (uint32_t)n_pairs,
                           d_cnt.p + C_COUNT + 1);
    }
    HIP_CHECK(hipGetLastError());

    auto counters = [&] {
        const std::vector<uint32_t> cnt = d_cnt.download(C_COUNT + 3);
        st->copied = cnt[C_COPIED]; st->u2sr = cnt[C_U2SR]; st->v2sr = cnt[C_V2SR]; st->sr2sr = cnt[C_SR2SR];
        st->claims_failed = cnt[C_FAILED];
        st->src_nonedge = cnt[C_COUNT];
        st->nonedge_skipped = n_ne - cnt[C_COUNT];
        st->src_induced = cnt[C_COUNT + 1];
        st->candidates = cnt[C_COUNT + 2];
        return cnt[C_MAXLEN];
    };
    // Case, ids and key per candidate.  Lists of one entry at the most (behind a merge: always): a candidate is a source edge
    // and case_kernel does what it did before the lists.  Otherwise the loop turns of every source edge are counted and
    // numbered in the reference's order, and a thread per turn works them out.  The timers run on the second path only: the
    // merge path is held to its time before the lists.
    const bool lists = max_entries > 1;
    auto timer = [&](const char *name) { return std::unique_ptr<KTimer>(lists ? new KTimer(name) : nullptr); };
    uint32_t nc = n;
    DBuf<uint64_t> cstart;
    if (lists) {
        DBuf<uint64_t> ccnt((size_t)n + 1);
        cstart.alloc((size_t)n + 1);
        {
            auto kt = timer("vq_next_count");
            hipLaunchKernelGGL(count_kernel, grid1((size_t)n + 1), dim3(WG), 0, stream(), d_rec.p, valid.p, n, tab, ccnt.p);
            exclusive_scan_u64(ccnt.p, cstart.p, (size_t)n + 1);
        }
        HIP_CHECK(hipGetLastError());
        const uint64_t n_cand64 = download_one(cstart.p + n);
        if (n_cand64 >= (1ull << 32) - 1)
            fail(HLMI_EINVAL, "vq_next: %llu and more candidates (2^32 - 1 and more)", (unsigned long long)n_cand64);
        nc = (uint32_t)n_cand64;
        if (!nc) { counters(); return std::string(); }
    }
    DBuf<Cand> cand(nc);
    DBuf<uint8_t> owner(nc), has(nc);
    DBuf<uint64_t> key(nc);
    DBuf<uint32_t> seq(nc), heads(nc);
    owner.zero();
    if (lists) {
        auto kt = timer("vq_next_expand");
        hipLaunchKernelGGL(expand_kernel, grid1(nc), dim3(WG), 0, stream(), d_rec.p, cstart.p, n, nc, tab, cand.p, key.p, seq.p,
                           d_cnt.p + C_COUNT + 2);
    } else {
        hipLaunchKernelGGL(case_kernel, grid1(n), dim3(WG), 0, stream(), d_rec.p, valid.p, n, tab, cand.p, key.p, seq.p,
                           d_cnt.p + C_COUNT + 2);
    }
    {                                                            // the claims: the first candidate of a key owns it
        auto kt = timer("vq_next_claim_sort");
        sort_pairs_u64_u32(key.p, seq.p, nc, 0, 64);             // stable: a key's claimants stay in loop order
        const size_t runs = select_run_heads_u64(key.p, nc, 0, heads.p);
        hipLaunchKernelGGL(owner_kernel, grid1(runs), dim3(WG), 0, stream(), key.p, seq.p, heads.p, (uint32_t)runs, owner.p);
    }

    DBuf<Line> line(nc);
    DBuf<uint32_t> llen((size_t)nc + 1);
    DBuf<uint64_t> start((size_t)nc + 1);
    llen.zero();
    {
        auto kt = timer("vq_next_eval");
        hipLaunchKernelGGL(eval_kernel, grid1(nc), dim3(WG), 0, stream(), d_rec.p, cand.p, owner.p, nc, tab,
                           no.no_inclusion_overlaps ? 1 : 0, line.p, llen.p, has.p, d_cnt.p);
    }
    HIP_CHECK(hipGetLastError());
    exclusive_scan_u32_to_u64(llen.p, start.p, (size_t)nc + 1);
    const uint32_t max_len = counters();
    const uint64_t text_bytes = download_one(start.p + nc);
    if (!text_bytes) return std::string();

    auto kt_order = timer("vq_next_order");
    DBuf<uint8_t> text(text_bytes);
    hipLaunchKernelGGL(text_kernel, grid1(nc), dim3(WG), 0, stream(), line.p, llen.p, start.p, nc, text.p);
    DBuf<uint32_t> perm(nc);
    const size_t n_l = select_flagged_indices(has.p, perm.p, nc);

    if (max_len > LINE_WIDTH) {                                  // a line wider than the device's order reads: the host's
        const std::vector<uint8_t> h_text = text.download(text_bytes);
        const std::vector<uint64_t> h_start = start.download(nc);
        const std::vector<uint32_t> h_len = llen.download(nc), h_idx = perm.download(n_l);
        std::vector<std::string_view> lines;
        lines.reserve(n_l);
        for (uint32_t r : h_idx) lines.emplace_back((const char *)h_text.data() + h_start[r], h_len[r]);
        std::sort(lines.begin(), lines.end());
        lines.erase(std::unique(lines.begin(), lines.end()), lines.end());
        std::string image;
        for (const std::string_view &l : lines) { image.append(l); image += '\n'; }
        st->lines = lines.size();
        return image;
    }
    // LSD over the words a line of this call can reach, last word first; each pass is stable
    DBuf<uint64_t> wkey(n_l);
    for (uint32_t w = (max_len + 7) / 8; w-- > 0;) {
        hipLaunchKernelGGL(word_kernel, grid1(n_l), dim3(WG), 0, stream(), text.p, start.p, llen.p, perm.p, (uint32_t)n_l, w, wkey.p);
        sort_pairs_u64_u32(wkey.p, perm.p, n_l, 0, 64);
    }
    DBuf<uint8_t> flag(n_l);
    DBuf<uint32_t> sel(n_l);
    hipLaunchKernelGGL(distinct_kernel, grid1(n_l), dim3(WG), 0, stream(), text.p, start.p, llen.p, perm.p, (uint32_t)n_l, flag.p);
    const size_t n_out = select_flagged_indices(flag.p, sel.p, n_l);
    DBuf<uint32_t> olen(n_out + 1);
    DBuf<uint64_t> ostart(n_out + 1);
    olen.zero();
    hipLaunchKernelGGL(out_len_kernel, grid1(n_out), dim3(WG), 0, stream(), llen.p, perm.p, sel.p, (uint32_t)n_out, olen.p);
    exclusive_scan_u32_to_u64(olen.p, ostart.p, n_out + 1);
    const uint64_t image_bytes = download_one(ostart.p + n_out);
    DBuf<uint8_t> image(image_bytes);
    hipLaunchKernelGGL(gather_kernel, grid1(n_out), dim3(WG), 0, stream(), text.p, start.p, llen.p, perm.p, sel.p, ostart.p,
                       (uint32_t)n_out, image.p);
    HIP_CHECK(hipGetLastError());
    const std::vector<uint8_t> h = image.download(image_bytes);
    st->lines = n_out;
    return std::string(h.begin(), h.end());
}

}  // namespace hlmi
