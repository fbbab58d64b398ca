// vq_graph.hip - SURVEY 8f rank 3: the device side of the oriented overlap graph of ViralQuasispecies --graph_only
// (tools/HaploConduct/src, ViralQuasispecies.cpp:250-398).  The per-edge and per-vertex steps run here; the order-dependent
// ones (sortEdges, the labelling BFS, the cycle DFS, the writers) are in vq_graph_host.cpp, the same split as graph_dev.hip /
// graph_host.cpp.  The transitive edges come from vq_front.hip's vq_trans_rounds.  Everything runs on the library's stream
// with its allocator.  PARITY UNPINNED (see vq_front.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "dev_prims.h"
#include "vq_internal.h"

namespace hlmi {
using namespace vqk;

namespace {
// ---------------------------------------------------------------------------------------------
// edge selection (EdgeCalculator.cpp:428-532)
// ---------------------------------------------------------------------------------------------
// key = (min vertex, max vertex, ori1 == ori2): the edge checkEdgeWithOri finds in either list (OverlapGraph.cpp:198-232).
// The candidates carry their fields after the swap of :443-448 (pos1 == 0: directed from the smaller vertex).
__global__ void select_keys_kernel(const VqEdge *c, size_t n, uint64_t *key, uint32_t *val) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t a = min(c[i].v1, c[i].v2), b = max(c[i].v1, c[i].v2);
    key[i] = (uint64_t)a << 32 | (uint64_t)b << 1 | (uint64_t)(c[i].ori1 == c[i].ori2);
    val[i] = (uint32_t)i;
}

// Does candidate c replace the edge w that holds its key?  process_overlaps :468-518: a lower score keeps w; a higher score
// replaces it; on an equal score the first field that differs decides - overlap length (longer stays), mismatch rate (lower
// stays), vertex(1) (smaller stays), ori1, ori2 ('+' stays), pos1, pos2 (smaller stays) - and a fully equal c replaces w.
__device__ __forceinline__ bool replaces(const VqEdge &w, const VqEdge &c) {
    if (!(c.score >= w.score)) return false;
    if (c.score != w.score) return true;
    if (w.len != c.len) return !(w.len > c.len);
    if (w.mr != c.mr) return !(w.mr < c.mr);
    if (w.v1 != c.v1) return !(w.v1 < c.v1);
    if (w.ori1 != c.ori1) return !w.ori1;
    if (w.ori2 != c.ori2) return !w.ori2;
    if (w.pos1 != c.pos1) return !(w.pos1 < c.pos1);
    if (w.pos2 != c.pos2) return !(w.pos2 < c.pos2);
    return true;
}

// One thread per key: the run of its candidates in file order (the radix sort is stable and the values start ascending),
// folded with `replaces`.  Only the run's first candidate - the one the reference adds while the key is new - can mark an
// inclusion (:455-465); a replacement never does.
__global__ void select_fold_kernel(const VqEdge *c, const uint32_t *val, const uint32_t *heads, uint32_t n_runs, size_t n,
                                   int ignore_inclusions, uint32_t *winner, uint8_t *incl) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    const size_t b = heads[r], e = r + 1 < n_runs ? heads[r + 1] : n;
    uint32_t w = val[b];
    const VqEdge f = c[w];
    if (ignore_inclusions && f.perc == 100 && f.mr < 0.000001 && f.mr >= 0) {
        if (f.pos3 < 0) {
            if (f.pos1 == 0) incl[f.v1] = 1;          // otherwise the rounding of the overlap percentage, not an inclusion
        } else {
            incl[f.v2] = 1;
        }
    }
    for (size_t k = b + 1; k < e; ++k) {
        const uint32_t x = val[k];
        if (replaces(c[w], c[x])) w = x;
    }
    winner[r] = w;
}

// ---------------------------------------------------------------------------------------------
// labelVertices' check pass (GraphAlgos.cpp:295-348)
// ---------------------------------------------------------------------------------------------
__global__ void label_check_kernel(VqEdge *edges, size_t n, const uint8_t *orient, uint8_t *cls) {
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= n) return;
    VqEdge e = edges[k];
    const bool t1 = orient[e.v1], t2 = orient[e.v2], o1 = e.ori1, o2 = e.ori2;
    uint8_t c;
    if (o1 == t1 && o2 == t2) {
        c = 0;
    } else if ((o1 == o2 && t1 != t2) || (o1 != o2 && t1 == t2)) {
        c = 1;
    } else {
        VqEdge s = e;
        if (switch_orientation(s)) {
            c = 2;                                    // the reference moves a flipped copy; the listed edge stays as it is
        } else {
            c = 3;
            edges[k] = s;                             // flipped in place: it stays flipped for the later tries
        }
    }
    cls[k] = c;
}

// ---------------------------------------------------------------------------------------------
// inclusions, tips: per-position marks over CSR adjacency lists
// ---------------------------------------------------------------------------------------------
// position of the first u -> v in u's list: the edge removeEdge(u, v) erases (OverlapGraph.cpp:104-147)
__device__ __forceinline__ uint32_t first_edge(const uint32_t *off, const uint32_t *dst, uint32_t u, uint32_t v) {
    const uint32_t b = off[u], e = off[u + 1];
    for (uint32_t p = b; p < e; ++p)
        if (dst[p] == v) return p;
    return e;                                         // (not reached for an edge of the graph)
}

__global__ void inclusion_keep_kernel(const uint32_t *off, const uint32_t *src, const uint32_t *dst, size_t n, const uint8_t *incl,
                                      uint8_t *keep) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t u = src[p], v = dst[p];
    // the pair (u, v) is scheduled once (a std::set of pairs), so only the first u -> v goes
    keep[p] = !((incl[u] || incl[v]) && first_edge(off, dst, u, v) == (uint32_t)p);
}

// One wave per vertex i.  Out-pass (:551-586): when i has more than one out-edge, an out-neighbour without out-edges is a
// tip candidate; an inclusion tip (ext_len(true) == 0) always goes, a short one (< max_tip_len) only when not all of i's
// out-neighbours are tips.  In-pass (:591-626): the same over in-neighbours without in-edges, with the first edge
// in-neighbour -> i (getEdgeInfo(.., false)) and ext_len(false).  Both passes read the graph before any removal.
__global__ __launch_bounds__(WG) void tips_kernel(uint32_t n_vertices, const uint32_t *off, const uint32_t *dst, const uint32_t *ioff,
                                                  const uint32_t *isrc, const uint32_t *ext_fwd, const uint32_t *ext_bwd,
                                                  uint32_t max_tip_len, uint8_t *removed, uint8_t *tip) {
    const int lane = threadIdx.x & 63;
    const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t i = wave; i < n_vertices; i += n_waves) {
        {
            const uint32_t b = off[i], e = off[i + 1];
            if (e - b > 1) {
                bool nontip = false;
                for (uint32_t p = b + (uint32_t)lane; p < e; p += 64) {
                    const uint32_t v = dst[p];
                    if (off[v + 1] != off[v]) nontip = true;
                }
                const bool alltips = !__any(nontip);
                for (uint32_t p = b + (uint32_t)lane; p < e; p += 64) {
                    const uint32_t v = dst[p];
                    if (off[v + 1] != off[v]) continue;
                    const uint32_t x = ext_fwd[p];
                    if (x == 0 || (x < max_tip_len && !alltips)) {
                        removed[first_edge(off, dst, (uint32_t)i, v)] = 1;
                        tip[v] = 1;
                    }
                }
            }
        }
        {
            const uint32_t b = ioff[i], e = ioff[i + 1];
            if (e - b > 1) {
                bool nontip = false;
                for (uint32_t p = b + (uint32_t)lane; p < e; p += 64) {
                    const uint32_t u = isrc[p];
                    if (ioff[u + 1] != ioff[u]) nontip = true;
                }
                const bool alltips = !__any(nontip);
                for (uint32_t p = b + (uint32_t)lane; p < e; p += 64) {
                    const uint32_t u = isrc[p];
                    if (ioff[u + 1] != ioff[u]) continue;
                    const uint32_t q = first_edge(off, dst, u, (uint32_t)i);
                    if (q >= off[u + 1]) continue;
                    const uint32_t x = ext_bwd[q];
                    if (x == 0 || (x < max_tip_len && !alltips)) {
                        removed[q] = 1;
                        tip[u] = 1;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// removeBranches' components: union-find over the joining edges
// ---------------------------------------------------------------------------------------------
__global__ void degree_kernel(const uint32_t *src, const uint32_t *dst, const uint8_t *trans, size_t n, uint32_t *outdeg, uint32_t *indeg) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n || trans[p]) return;
    atomicAdd(&outdeg[src[p]], 1u);
    atomicAdd(&indeg[dst[p]], 1u);
}
__global__ void iota_kernel(uint32_t *parent, size_t n) {
    const size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (v < n) parent[v] = (uint32_t)v;
}
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
    uint32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
    while (p != x) {                                   // path halving: a vertex only ever points to an ancestor
        const uint32_t g = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
        if (g != p) __atomic_store_n(&parent[x], g, __ATOMIC_RELAXED);
        x = p;
        p = g;
    }
    return x;
}
// new_adj_out[u] is cleared when u has more than one non-transitive out-edge, new_adj_in[v] when v has more than one
// non-transitive in-edge; the BFS of :865-912 follows u -> v only when the edge is still in both lists
__global__ void union_kernel(const uint32_t *src, const uint32_t *dst, const uint8_t *trans, size_t n, const uint32_t *outdeg,
                             const uint32_t *indeg, uint32_t *parent) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n || trans[p]) return;
    const uint32_t u = src[p], v = dst[p];
    if (outdeg[u] > 1 || indeg[v] > 1) return;
    for (;;) {
        uint32_t a = uf_find(parent, u), b = uf_find(parent, v);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        if (atomicCAS(&parent[a], a, b) == a) return;   // the larger root hangs under the smaller one
    }
}
__global__ void flatten_kernel(uint32_t *parent, size_t n, uint32_t *comp) {
    const size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (v < n) comp[v] = uf_find(parent, (uint32_t)v);
}
}  // namespace

// ---------------------------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------------------------
void vq_select_edges(const std::vector<VqEdge> &cand, uint32_t n_vertices, bool ignore_inclusions,
                     std::vector<uint32_t> &winners, std::vector<uint8_t> &incl) {
    const size_t n = cand.size();
    incl.assign(n_vertices, 0);
    winners.clear();
    if (!n) return;
    DBuf<VqEdge> d_c;
    d_c.upload(cand);
    DBuf<uint64_t> key(n);
    DBuf<uint32_t> val(n), heads(n);
    hipLaunchKernelGGL(select_keys_kernel, grid1(n), dim3(WG), 0, stream(), d_c.p, n, key.p, val.p);
    sort_pairs_u64_u32(key, val, n, 0, 64);              // stable: each key's candidates stay in file order
    const size_t runs = select_run_heads_u64(key.p, n, 0, heads.p);
    DBuf<uint32_t> win(runs);
    DBuf<uint8_t> d_incl(n_vertices ? n_vertices : 1);
    d_incl.zero();
    hipLaunchKernelGGL(select_fold_kernel, grid1(runs), dim3(WG), 0, stream(), d_c.p, val.p, heads.p, (uint32_t)runs, n,
                       ignore_inclusions ? 1 : 0, win.p, d_incl.p);
    HIP_CHECK(hipGetLastError());
    winners = win.download(runs);
    if (n_vertices) incl = d_incl.download(n_vertices);
    std::sort(winners.begin(), winners.end());
}

VqLabelPass::VqLabelPass(const std::vector<VqEdge> &edges) : n_(edges.size()) {
    d_edges_.upload(edges);
    d_cls_.alloc(n_ ? n_ : 1);
}
void VqLabelPass::run(const std::vector<uint8_t> &orient, std::vector<uint8_t> &cls) {
    d_orient_.upload(orient);
    cls.assign(n_, 0);
    if (!n_) return;
    hipLaunchKernelGGL(label_check_kernel, grid1(n_), dim3(WG), 0, stream(), d_edges_.p, n_, d_orient_.p, d_cls_.p);
    HIP_CHECK(hipGetLastError());
    cls = d_cls_.download(n_);
}
std::vector<VqEdge> VqLabelPass::state() const { return n_ ? d_edges_.download(n_) : std::vector<VqEdge>(); }

void vq_inclusion_removed(const std::vector<uint32_t> &off, const std::vector<uint32_t> &src, const std::vector<uint32_t> &dst,
                          const std::vector<uint8_t> &incl, std::vector<uint8_t> &removed) {
    const size_t n = dst.size();
    removed.clear();
    if (!n) return;
    DBuf<uint32_t> d_off, d_src, d_dst;
    DBuf<uint8_t> d_incl, keep(n);
    d_off.upload(off); d_src.upload(src); d_dst.upload(dst); d_incl.upload(incl);
    hipLaunchKernelGGL(inclusion_keep_kernel, grid1(n), dim3(WG), 0, stream(), d_off.p, d_src.p, d_dst.p, n, d_incl.p, keep.p);
    HIP_CHECK(hipGetLastError());
    removed = keep.download(n);
    for (uint8_t &f : removed) f = !f;
}

// vq_trans_flags over resident edges
static uint64_t trans_flags(uint32_t n_vertices, const DBuf<uint32_t> &d_src, const DBuf<uint32_t> &d_dst, size_t E, int rounds,
                            std::vector<uint8_t> &flags) {
    flags.assign(E, 0);
    DBuf<uint32_t> ids;
    const size_t found = vq_trans_rounds(n_vertices, d_src.p, d_dst.p, E, rounds, ids);
    if (found)
        for (uint32_t k : ids.download(found)) flags[k] = 1;
    return found;
}

uint64_t vq_trans_flags(uint32_t n_vertices, const std::vector<uint32_t> &src, const std::vector<uint32_t> &dst, int rounds,
                        std::vector<uint8_t> &flags) {
    DBuf<uint32_t> d_src, d_dst;
    d_src.upload(src);
    d_dst.upload(dst);
    return trans_flags(n_vertices, d_src, d_dst, src.size(), rounds, flags);
}

void vq_tips(uint32_t n_vertices, const std::vector<uint32_t> &off, const std::vector<uint32_t> &dst,
             const std::vector<uint32_t> &in_off, const std::vector<uint32_t> &in_src, const std::vector<uint32_t> &ext_fwd,
             const std::vector<uint32_t> &ext_bwd, uint32_t max_tip_len, std::vector<uint8_t> &removed, std::vector<uint8_t> &tip) {
    const size_t n = dst.size();
    removed.assign(n, 0);
    tip.assign(n_vertices, 0);
    if (!n || !n_vertices) return;
    DBuf<uint32_t> d_off, d_dst, d_ioff, d_isrc, d_fwd, d_bwd;
    d_off.upload(off); d_dst.upload(dst); d_ioff.upload(in_off); d_isrc.upload(in_src); d_fwd.upload(ext_fwd); d_bwd.upload(ext_bwd);
    DBuf<uint8_t> d_rm(n), d_tip(n_vertices);
    d_rm.zero();
    d_tip.zero();
    hipLaunchKernelGGL(tips_kernel, dim3(waves_grid(n_vertices)), dim3(WG), 0, stream(), n_vertices, d_off.p, d_dst.p, d_ioff.p,
                       d_isrc.p, d_fwd.p, d_bwd.p, max_tip_len, d_rm.p, d_tip.p);
    HIP_CHECK(hipGetLastError());
    removed = d_rm.download(n);
    tip = d_tip.download(n_vertices);
}

void vq_branch_components(uint32_t n_vertices, const std::vector<uint32_t> &src, const std::vector<uint32_t> &dst,
                          std::vector<uint32_t> &comp) {
    const size_t n = src.size();
    comp.resize(n_vertices);
    for (uint32_t v = 0; v < n_vertices; ++v) comp[v] = v;
    if (!n || !n_vertices) return;
    DBuf<uint32_t> d_src, d_dst, outdeg(n_vertices), indeg(n_vertices), parent(n_vertices), d_comp(n_vertices);
    DBuf<uint8_t> d_tr;
    d_src.upload(src); d_dst.upload(dst);
    std::vector<uint8_t> trans;
    trans_flags(n_vertices, d_src, d_dst, n, 1, trans);
    d_tr.upload(trans);
    outdeg.zero();
    indeg.zero();
    hipLaunchKernelGGL(degree_kernel, grid1(n), dim3(WG), 0, stream(), d_src.p, d_dst.p, d_tr.p, n, outdeg.p, indeg.p);
    hipLaunchKernelGGL(iota_kernel, grid1(n_vertices), dim3(WG), 0, stream(), parent.p, (size_t)n_vertices);
    hipLaunchKernelGGL(union_kernel, grid1(n), dim3(WG), 0, stream(), d_src.p, d_dst.p, d_tr.p, n, outdeg.p, indeg.p, parent.p);
    hipLaunchKernelGGL(flatten_kernel, grid1(n_vertices), dim3(WG), 0, stream(), parent.p, (size_t)n_vertices, d_comp.p);
    HIP_CHECK(hipGetLastError());
    comp = d_comp.download(n_vertices);
}

}  // namespace hlmi
