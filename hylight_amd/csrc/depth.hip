// depth.hip - the device part of hlmi_depth / hlmi_depth_reads (include/hylight_mi.h): read depth per contig position from the
// selected rows' spans, and what the tables need of it.
//   depth_span_kernel    (fused call) a thread per selected row: (contig record, ts, te) straight from the overlapper's record
//   depth_tile_kernel    a workgroup per tile of polish_layout: +1 / -1 of every span clipped to the tile into a difference array
//                        in LDS, a workgroup scan (DPP wave scan, wave totals through LDS), depth[cbase + p] out, and the tile's
//                        covered positions and depth sum added to its contig's two counters with one global atomic each
//   depth_key_kernel     a thread per position: slot << 32 | depth; two radix sorts over exactly the bits in use (the depth
//                        bits, then the slot bits: LSD, stable) order every contig's depths, depth_median_kernel takes element
//                        (length - 1) / 2 of every slot
//   depth_flag_kernel    (bedGraph) a thread per position: does a run start here (the contig starts, or the depth changes)?
//                        flag-select, then depth_run_kernel gathers the runs' depths: only the runs go to the host
// Why tiles and not one difference array in HBM with a device-wide segmented scan: the +1 / -1 of a deep pile stay LDS atomics
// (as the votes of polish_count_kernel do), and a tile owns its positions, so 4 B per position leave the CU and nothing else;
// the price is that a span record (12 B) is read once per tile it overlaps (DESIGN.md section 4.3i has the byte formula).
// Every loop is bounded by a count known at its head.
#include <hip/hip_runtime.h>

#include "common.h"
#include "depth_internal.h"
#include "dev_prims.h"
#include "polish_walk.h"
#include "wave_ops.h"

namespace hlmi {
namespace depth {

using namespace pol;

namespace {

constexpr int WG = 256, WAVES = WG / 64;
constexpr int PER = POLISH_TILE / WG;           // consecutive positions of a tile a thread scans
static_assert(PER == 4 && PER * WG == POLISH_TILE, "a thread reads its 4 difference words as one 16-byte LDS load");
constexpr unsigned MAX_GRID = 1u << 16;         // blocks of a strided launch
inline dim3 grid1(size_t n) { return dim3((unsigned)std::min<size_t>(cdiv(n ? n : 1, WG), MAX_GRID)); }

__global__ __launch_bounds__(WG) void depth_span_kernel(const PafRec *__restrict__ recs, const uint32_t *__restrict__ idx, size_t n_sel,
                                                        const uint32_t *__restrict__ crec_of_rank, PolSpan *__restrict__ span) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < n_sel; j += step) {
        const PafRec r = recs[idx[j]];
        span[j] = PolSpan{crec_of_rank[r.tid], r.ts, r.te};
    }
}

__global__ __launch_bounds__(WG) void depth_tile_kernel(const PolSpan *__restrict__ spans, uint32_t n_spans, const PolTile *__restrict__ tiles,
                                                        const uint32_t *__restrict__ cbase, uint32_t n_slots, uint32_t n_total,
                                                        uint32_t *__restrict__ depth, unsigned long long *__restrict__ slot_covered,
                                                        unsigned long long *__restrict__ slot_bases) {
    __shared__ __attribute__((aligned(16))) int diff[POLISH_TILE + PER];       // POLISH_TILE + 1 words in use
    __shared__ uint32_t wave_total[WAVES];
    __shared__ unsigned long long tile_bases;
    __shared__ uint32_t tile_covered;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PolTile t = tiles[blockIdx.x];
    const uint32_t t0 = t.t0, n_pos = min(t.n_pos, (uint32_t)POLISH_TILE), t1 = t0 + n_pos;
    for (int i = tid; i < POLISH_TILE + PER; i += WG) diff[i] = 0;
    if (tid == 0) { tile_bases = 0; tile_covered = 0; }
    __syncthreads();
    const uint32_t row_hi = min(t.row_hi, n_spans);
    for (uint32_t r = t.row_lo + (uint32_t)tid; r < row_hi; r += WG) {
        const PolSpan s = spans[r];
        const uint32_t a = max(s.ts, t0), b = min(s.te, t1);        // clipped: a row of the range that ended in front adds nothing
        if (a < b) {
            atomicAdd(&diff[a - t0], 1);
            atomicAdd(&diff[b - t0], -1);                           // b - t0 <= n_pos <= POLISH_TILE
        }
    }
    __syncthreads();
    const int4 d = reinterpret_cast<const int4 *>(diff)[tid];
    const int v0 = d.x, v1 = v0 + d.y, v2 = v1 + d.z, v3 = v2 + d.w;
    const uint32_t incl = wave_prefix_sum_incl_dpp((uint32_t)v3);
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t off = incl - (uint32_t)v3;
    for (int w = 0; w < WAVES; ++w) off += w < wave ? wave_total[w] : 0u;
    const uint32_t dep[PER] = {off + (uint32_t)v0, off + (uint32_t)v1, off + (uint32_t)v2, off + (uint32_t)v3};
    uint32_t cov = 0;
    unsigned long long sum = 0;
    const uint32_t p0 = (uint32_t)tid * PER;
    for (int k = 0; k < PER; ++k) {
        const uint32_t p = p0 + (uint32_t)k, g = t.cbase + t0 + p;
        if (p < n_pos && g < n_total) {
            depth[g] = dep[k];
            cov += dep[k] != 0;
            sum += dep[k];
        }
    }
    const uint32_t wave_cov = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(cov), 63);
    if (lane == 0 && wave_cov) atomicAdd(&tile_covered, wave_cov);
    if (sum) atomicAdd(&tile_bases, sum);
    __syncthreads();
    if (tid == 0) {
        const uint32_t j = slot_of_position(cbase, n_slots, t.cbase);
        if (tile_covered) atomicAdd(&slot_covered[j], (unsigned long long)tile_covered);
        if (tile_bases) atomicAdd(&slot_bases[j], tile_bases);
    }
}

__global__ __launch_bounds__(WG) void depth_key_kernel(const uint32_t *__restrict__ depth, uint32_t n_total, const uint32_t *__restrict__ cbase,
                                                       uint32_t n_slots, uint64_t *__restrict__ key) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t p = (size_t)blockIdx.x * WG + threadIdx.x; p < n_total; p += step)
        key[p] = (uint64_t)slot_of_position(cbase, n_slots, (uint32_t)p) << 32 | depth[p];
}

__global__ __launch_bounds__(WG) void depth_median_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ cbase, uint32_t n_slots,
                                                          uint32_t *__restrict__ median) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < n_slots; j += step) {
        const uint32_t b = cbase[j], len = cbase[j + 1] - b;
        median[j] = len ? (uint32_t)key[b + (len - 1) / 2] : 0u;
    }
}

__global__ __launch_bounds__(WG) void depth_flag_kernel(const uint32_t *__restrict__ depth, uint32_t n_total, const uint32_t *__restrict__ cbase,
                                                        uint32_t n_slots, uint8_t *__restrict__ flag) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t p = (size_t)blockIdx.x * WG + threadIdx.x; p < n_total; p += step) {
        const bool first = p == 0 || cbase[slot_of_position(cbase, n_slots, (uint32_t)p)] == (uint32_t)p;
        flag[p] = first ? 1 : depth[p] != depth[p - 1];
    }
}

__global__ __launch_bounds__(WG) void depth_run_kernel(const uint32_t *__restrict__ depth, const uint32_t *__restrict__ start, size_t n_runs,
                                                       uint32_t *__restrict__ run_depth) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n_runs; i += step) run_depth[i] = depth[start[i]];
}

}  // namespace

void depth_spans_from_rows(const PafRec *recs, const uint32_t *idx, size_t n_sel, const uint32_t *crec_of_rank, PolSpan *out) {
    if (!n_sel) return;
    KTimer kt("depth_spans");
    hipLaunchKernelGGL(depth_span_kernel, grid1(n_sel), dim3(WG), 0, stream(), recs, idx, n_sel, crec_of_rank, out);
    HIP_CHECK(hipGetLastError());
}

void depth_core(const DepthCoreIn &in, DeviceDepth &out) {
    out = DeviceDepth{};
    const std::vector<uint32_t> &cb = *in.h_cbase;
    const uint32_t n_slots = (uint32_t)(cb.size() - 1), N = cb.back();      // N < 2^31 (polish_layout)
    if (!n_slots || !N) return;
    if (in.n_spans >= (1ull << 32)) fail(HLMI_EINVAL, "hlmi_depth: %zu selected rows (2^32 and more)", in.n_spans);
    // depth 4 B, keys 8 B and the sort's second buffer 8 B per position, or flags and run starts 5 B behind the keys
    const size_t need = (size_t)N * 20 + (64u << 20), have = dev_available_bytes();
    if (have && need > have)
        fail(HLMI_EINVAL, "hlmi_depth: %u contig positions need %zu bytes of device memory for the depths and their sort keys, %zu are free",
             N, need, have);
    DBuf<uint32_t> d_depth(N), d_median(n_slots);
    DBuf<unsigned long long> d_counts(2 * (size_t)n_slots);
    d_counts.zero();
    d_depth.zero();                             // positions of a covered contig that no tile holds: depth 0
    if (in.n_tiles) {
        KTimer kt("depth_tile");
        hipLaunchKernelGGL(depth_tile_kernel, dim3(cdiv(in.n_tiles, 1)), dim3(WG), 0, stream(), in.spans, (uint32_t)in.n_spans, in.tiles,
                           in.cbase, n_slots, N, d_depth.p, d_counts.p, d_counts.p + n_slots);
        HIP_CHECK(hipGetLastError());
    }
    {
        KTimer kt("depth_median");
        DBuf<uint64_t> key(N);
        hipLaunchKernelGGL(depth_key_kernel, grid1(N), dim3(WG), 0, stream(), d_depth.p, N, in.cbase, n_slots, key.p);
        HIP_CHECK(hipGetLastError());
        sort_keys_u64(key, N, 0, bits_for(in.n_spans));                     // a depth is at most the number of rows
        if (n_slots > 1) sort_keys_u64(key, N, 32, 32 + bits_for(n_slots - 1));
        hipLaunchKernelGGL(depth_median_kernel, grid1(n_slots), dim3(WG), 0, stream(), key.p, in.cbase, n_slots, d_median.p);
        HIP_CHECK(hipGetLastError());
    }
    const std::vector<unsigned long long> counts = d_counts.download(2 * (size_t)n_slots);
    out.covered.assign(counts.begin(), counts.begin() + n_slots);
    out.bases.assign(counts.begin() + n_slots, counts.end());
    out.median = d_median.download(n_slots);
    if (in.want_runs) {
        KTimer kt("depth_runs");
        DBuf<uint8_t> flag(N);
        DBuf<uint32_t> start(N);
        hipLaunchKernelGGL(depth_flag_kernel, grid1(N), dim3(WG), 0, stream(), d_depth.p, N, in.cbase, n_slots, flag.p);
        HIP_CHECK(hipGetLastError());
        const size_t n_runs = select_flagged_indices(flag.p, start.p, N);
        DBuf<uint32_t> run_depth(std::max<size_t>(n_runs, 1));
        hipLaunchKernelGGL(depth_run_kernel, grid1(n_runs), dim3(WG), 0, stream(), d_depth.p, start.p, n_runs, run_depth.p);
        HIP_CHECK(hipGetLastError());
        out.run_start = start.download(n_runs);
        out.run_depth = run_depth.download(n_runs);
    }
}

}  // namespace depth
}  // namespace hlmi
