// phase_reach.hip - the link pass of hlmi_phase_reach / hlmi_phase_reads_reach (include/hylight_mi.h): how the alleles of two
// sites up to `reach` = K apart go together, over the allele table phase.hip left in device memory.
//   phase_link_reach_kernel   a workgroup per tile of PHASE_REACH_TILE left sites (a link belongs to its left site): 4 x K
//                             counters per left site in LDS, 16 K PHASE_REACH_TILE bytes sized at launch - a call with K = 1 or
//                             2 does not pay for 8.  A wave per row of the tile's row range walks the row's allele bytes, 64 left
//                             sites a step; every byte is read once: the step keeps the next 64 bytes, which are the partners
//                             of its last d lanes and the left sites of the step behind it.  The partner at distance d is the
//                             byte of the lane d above, moved up one lane per d (wave_shl1); lane 63 takes lane 0 of the next
//                             step's bytes, which move along.  n[x][y] of (j, d) is bumped where both bytes are 0 or 1, j lies
//                             in the tile and j + d inside the row; what the row reads in between plays no part.
// LDS order [n][d][left site]: the 64 lanes of one bump hold 64 consecutive left sites of one d - 64 different banks.  The flush
// writes one array of 16-byte entries with d running fastest, entry j * K + (d - 1): the K links of a left site are 16 K
// consecutive bytes, which is how the host's block walk reads them (site by site, the nearest member first), and consecutive
// threads of the flush write consecutive 16 bytes.  A row lies in one contig, so no link across a junction is ever counted; the
// entries that would cross one stay zero and the host does not read them.
// Every loop is bounded by a count known at its head.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "phase_internal.h"
#include "wave_ops.h"

namespace hlmi {
namespace ph {

namespace {

constexpr int WG = 256, WAVES = WG / 64;
constexpr uint32_t TILE = (uint32_t)PHASE_REACH_TILE;
static_assert(PHASE_REACH_MAX == HLMI_PHASE_REACH_MAX, "the header's largest reach is the host rule's");
static_assert(16 * PHASE_REACH_MAX * PHASE_REACH_TILE <= 65536, "the counters of a tile at the largest reach fit 64 KB of LDS");

__global__ __launch_bounds__(WG) void phase_link_reach_kernel(const LinkTile *__restrict__ tiles, uint32_t n_tiles, uint32_t n_left, uint32_t n_rows,
                                                              uint32_t K, const uint32_t *__restrict__ s_lo, const uint32_t *__restrict__ cnt,
                                                              const uint64_t *__restrict__ off, const uint8_t *__restrict__ table,
                                                              LinkCounts *__restrict__ links) {
    extern __shared__ uint32_t s_n[];           // [4][K][TILE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = blockIdx.x;
    if (tile >= n_tiles || K < 1 || K > (uint32_t)PHASE_REACH_MAX) return;
    const uint32_t l0 = tile * TILE;
    if (l0 >= n_left) return;
    const uint32_t l1 = l0 + min(TILE, n_left - l0);
    const uint32_t plane = K * TILE;            // words of one of the four counters
    for (uint32_t i = (uint32_t)tid; i < 4 * plane; i += WG) s_n[i] = 0;
    __syncthreads();
    const LinkTile t = tiles[tile];
    const uint32_t row_hi = min(t.row_hi, n_rows);
    for (uint32_t k = t.row_lo + (uint32_t)wave; k < row_hi; k += WAVES) {
        const uint32_t n = cnt[k], lo = s_lo[k];
        if (n < 2) continue;                                                    // (the same in every lane, as all below but j)
        // the left sites j inside the tile with a right neighbour in [lo, end)
        const uint32_t end = lo + n, j0 = max(lo, l0), j1 = min(end - 1, l1);
        if (j0 >= j1) continue;
        const uint8_t *a = table + off[k];
        const uint32_t steps = (j1 - j0 + 63) / 64;
        uint32_t j = j0 + (uint32_t)lane;
        int cur = j < end ? (int)a[j - lo] : (int)AL_NONE;
        for (uint32_t s = 0; s < steps; ++s, j += 64) {
            const int nxt = j + 64 < end ? (int)a[j + 64 - lo] : (int)AL_NONE;
            int p = cur, q = nxt;               // behind d shifts: p the byte of site j + d, q lane 0 the byte of site j0 + 64 (s + 1) + d - 1
            for (uint32_t d = 1; d <= K; ++d) {
                p = wave_shl1(p, __builtin_amdgcn_readlane(q, 0));
                q = wave_shl1(q, (int)AL_NONE);
                if (cur < 2 && p < 2 && j < j1 && j + d < end)                  // l0 <= j0 <= j < j1 <= l1 <= l0 + TILE
                    atomicAdd(&s_n[((uint32_t)(cur * 2 + p)) * plane + (d - 1) * TILE + (j - l0)], 1u);
            }
            cur = nxt;
        }
    }
    __syncthreads();
    const uint32_t m = (l1 - l0) * K;
    for (uint32_t i = (uint32_t)tid; i < m; i += WG) {
        const uint32_t site = i / K, d = i - site * K;
        const uint32_t *c = s_n + d * TILE + site;
        links[(size_t)l0 * K + i] = LinkCounts{c[0], c[plane], c[2 * plane], c[3 * plane]};
    }
}

}  // namespace

void link_reach(const char *who, const std::vector<uint32_t> &h_lo, const std::vector<uint32_t> &h_cnt, size_t n_links, const uint32_t *s_lo,
                const uint32_t *cnt, const uint64_t *off, const uint8_t *table, ReachLinks &out) {
    const size_t K = (size_t)out.reach;
    if (out.reach < 1 || out.reach > PHASE_REACH_MAX) fail(HLMI_ESTATE, "%s: reach %d in the link pass", who, out.reach);          // (never)
    out.n.assign(n_links * K, LinkCounts{0, 0, 0, 0});
    if (!n_links || h_lo.empty()) return;
    check_fits(who, "the link counters", (uint64_t)n_links * K * sizeof(LinkCounts));
    const std::vector<LinkTile> tiles = link_tiles(h_lo, h_cnt, n_links, PHASE_REACH_TILE);
    DBuf<LinkTile> d_tiles;
    d_tiles.upload(tiles);
    DBuf<LinkCounts> d_links(n_links * K);
    const size_t lds = 16 * K * (size_t)PHASE_REACH_TILE;
    hipLaunchKernelGGL(phase_link_reach_kernel, dim3((unsigned)tiles.size()), dim3(WG), lds, stream(), d_tiles.p, (uint32_t)tiles.size(),
                       (uint32_t)n_links, (uint32_t)h_lo.size(), (uint32_t)K, s_lo, cnt, off, table, d_links.p);
    HIP_CHECK(hipGetLastError());
    out.n = d_links.download(n_links * K);
}

}  // namespace ph
}  // namespace hlmi
