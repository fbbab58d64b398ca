// variants.hip - the device part of hlmi_variants / hlmi_variants_reads (include/hylight_mi.h): the votes of the selected rows per
// contig position, the site rule, and the sites' records.
//   var_tile_kernel<ENC, false>   a workgroup per tile of polish_layout: five 32-bit counters per position in LDS (A C G T del,
//                                 20 KiB), the rows walked and voted by the loops of polish_count_kernel (polish_walk.h); the flush
//                                 applies the site rule and writes one flag byte per position; the tile's callable, ref_other and
//                                 site counts are reduced in the workgroup and added to its contig's three 64-bit counters with
//                                 one global atomic each; one byte per tile says whether it holds a site
//   select_flagged_indices        over the position flags: the sites' positions, ascending; over the tile bytes: the tiles to revisit
//   var_tile_kernel<ENC, true>    over those tiles only: counts again, and a site's thread finds its place in the site array by
//                                 binary search and writes its 24-byte record (position, five counts) there
// Why two passes and no record per position: the counters of a position that is no site are never needed, and sites are few
// (a strain-pure contig has none), so what leaves the CU in pass 1 is one byte per position; the records' memory is 24 B per
// site, their order is the order of the selected flags - ascending by construction, whatever order the atomics ran in.  The
// price is that the tiles with a site are counted twice (DESIGN.md section 4.3j has the byte formula).  With no site the select
// over the tiles and the second pass are not launched.  Every loop is bounded by a count known at its head.
#include <hip/hip_runtime.h>

#include "common.h"
#include "dev_prims.h"
#include "polish_walk.h"
#include "variants_internal.h"
#include "wave_ops.h"

namespace hlmi {
namespace var {

using namespace pol;

namespace {

static_assert(N_SYM == 5 && S_DEL == (int)SYM_DEL && (int)C_OTHER == N_SYM, "the five symbols are the polisher's");
static_assert(sizeof(SiteRec) == 24, "a site's record is 24 bytes");

// the first index of the ascending a[0, n) whose value is not below v (n: none); n < 2^32: 32 steps at the most
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *__restrict__ a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (a[m] < v) lo = m + 1;
        else hi = m;
    }
    return lo;
}

struct VarArgs {
    const PolRow *rows;
    uint32_t n_rows;
    const uint32_t *ops;
    const uint8_t *reads, *contig;
    uint32_t n_contig;
    const PolTile *tiles;
    uint32_t n_tiles;
    const uint32_t *cbase;
    uint32_t n_slots;
    uint32_t min_cov, min_alt;
    double min_frac;
    uint8_t *flag, *tile_flag;                  // pass 1 out: per position, per tile
    unsigned long long *slot_counts;            // pass 1 out: callable, ref_other, sites - n_slots of each
    const uint32_t *tile_list;                  // pass 2: the tiles to run over (n_list of them), the sites' positions, the records
    uint32_t n_list;
    const uint32_t *site_pos;
    uint32_t n_sites;
    SiteRec *recs;
};

template <int ENC, bool EMIT>
__global__ __launch_bounds__(POLISH_WG) void var_tile_kernel(const VarArgs A) {
    __shared__ uint32_t s_cnt[N_SYM][POLISH_TILE];
    __shared__ uint32_t s_tot[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t tile = blockIdx.x;
    if constexpr (EMIT) {
        if (tile >= A.n_list) return;
        tile = A.tile_list[tile];
    }
    if (tile >= A.n_tiles) return;
    const PolTile t = A.tiles[tile];
    const uint32_t n_pos = min(t.n_pos, (uint32_t)POLISH_TILE), t_end = t.t0 + n_pos;
    for (int i = tid; i < N_SYM * POLISH_TILE; i += POLISH_WG) (&s_cnt[0][0])[i] = 0;
    if (tid < 3) s_tot[tid] = 0;
    __syncthreads();
    const uint32_t row_hi = min(t.row_hi, A.n_rows);
    for (uint32_t k = t.row_lo + (uint32_t)wave; k < row_hi; k += POLISH_WAVES) {
        const PolRow r = A.rows[k];
        if (r.te <= t.t0 || r.ts >= t_end) continue;
        auto vote = [&](uint32_t p, uint32_t code, uint32_t tp0, uint32_t qc0, uint32_t) {
            const uint32_t s = code == OP_D ? (uint32_t)SYM_DEL : column_symbol<ENC>(r, A.reads, qc0 + (p - tp0));
            if (s < (uint32_t)N_SYM) atomicAdd(&s_cnt[s][p - t.t0], 1u);           // t.t0 <= p < t_end: [a, b) is clipped
        };
        walk_row(r, A.ops, lane, t_end, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
            uint32_t a = 0, b = 0;              // the columns of this op inside the tile
            if (code == OP_EQ || code == OP_X || code == OP_D) {
                a = max(tp0, t.t0);
                b = max(a, min(tp0 + len, t_end));
            }
            vote_columns<false>(a, b, code, tp0, qc0, 1u, lane, vote);
        });
    }
    __syncthreads();
    uint32_t n_call = 0, n_other = 0, n_site = 0;
    for (uint32_t i = (uint32_t)tid; i < n_pos; i += POLISH_WG) {
        const uint32_t g = t.cbase + t.t0 + i;
        if (g >= A.n_contig) continue;                                             // (the layout holds every tile inside: never)
        uint32_t v[N_SYM], c = 0;
#pragma unroll
        for (int k = 0; k < N_SYM; ++k) { v[k] = s_cnt[k][i]; c += v[k]; }
        bool site = false;
        if (c >= A.min_cov) {
            const uint8_t own = A.contig[g] & 0xdfu;
            const int ko = own == 'A' ? 0 : own == 'C' ? 1 : own == 'G' ? 2 : own == 'T' ? 3 : -1;
            if (ko < 0) ++n_other;
            else {
                ++n_call;
                uint32_t best = 0;              // the alternative's votes: the first of A C G T del among the largest
                bool have = false;
#pragma unroll
                for (int k = 0; k < N_SYM; ++k)
                    if (k != ko && (!have || v[k] > best)) { best = v[k]; have = true; }
                site = best >= A.min_alt && (double)best / (double)c >= A.min_frac;     // one IEEE division; c >= min_cov >= 1
            }
        }
        if constexpr (!EMIT) {
            A.flag[g] = site;
            n_site += site;
        } else if (site) {
            const uint32_t at = lower_bound_u32(A.site_pos, A.n_sites, g);
            if (at < A.n_sites && A.site_pos[at] == g) A.recs[at] = SiteRec{g, {v[0], v[1], v[2], v[3], v[4]}};
        }
    }
    if constexpr (!EMIT) {
        const uint32_t w_call = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(n_call), 63);
        const uint32_t w_other = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(n_other), 63);
        const uint32_t w_site = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(n_site), 63);
        if (lane == 0) {
            if (w_call) atomicAdd(&s_tot[0], w_call);
            if (w_other) atomicAdd(&s_tot[1], w_other);
            if (w_site) atomicAdd(&s_tot[2], w_site);
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t j = slot_of_position(A.cbase, A.n_slots, t.cbase);
            if (s_tot[0]) atomicAdd(&A.slot_counts[j], (unsigned long long)s_tot[0]);
            if (s_tot[1]) atomicAdd(&A.slot_counts[A.n_slots + j], (unsigned long long)s_tot[1]);
            if (s_tot[2]) atomicAdd(&A.slot_counts[2 * (size_t)A.n_slots + j], (unsigned long long)s_tot[2]);
            A.tile_flag[tile] = s_tot[2] != 0;
        }
    }
}

template <bool EMIT>
void launch_tiles(ReadEnc enc, const VarArgs &a, uint32_t n_blocks) {
    if (enc == READS_CODES) hipLaunchKernelGGL((var_tile_kernel<READS_CODES, EMIT>), dim3(n_blocks), dim3(POLISH_WG), 0, stream(), a);
    else hipLaunchKernelGGL((var_tile_kernel<READS_ASCII, EMIT>), dim3(n_blocks), dim3(POLISH_WG), 0, stream(), a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

void variants_core(const PolCoreIn &in, const hlmi_variant_opts &o, DeviceVariants &out) {
    out = DeviceVariants{};
    const size_t G = in.n_contig;               // < 2^31 (polish_layout)
    const uint32_t n_slots = in.n_cbase ? (uint32_t)(in.n_cbase - 1) : 0u;
    out.callable.assign(n_slots, 0);
    out.ref_other.assign(n_slots, 0);
    out.sites.assign(n_slots, 0);
    out.tiles = in.n_tiles;
    if (!G || !n_slots || !in.n_tiles) return;
    if (in.n_tiles >= (1ull << 32)) fail(HLMI_EINVAL, "hlmi_variants: %zu tiles (2^32 and more)", in.n_tiles);      // (never: G < 2^31)
    DBuf<uint8_t> d_flag(G), d_tile_flag(in.n_tiles);
    DBuf<unsigned long long> d_counts(3 * (size_t)n_slots);
    d_flag.zero();                              // positions of a covered contig that no tile holds: no site
    d_counts.zero();
    VarArgs a{};
    a.rows = in.rows; a.n_rows = in.n_rows;
    a.ops = in.ops;
    a.reads = in.reads; a.contig = in.contig; a.n_contig = (uint32_t)G;
    a.tiles = in.tiles; a.n_tiles = (uint32_t)in.n_tiles;
    a.cbase = in.cbase; a.n_slots = n_slots;
    a.min_cov = (uint32_t)o.min_cov; a.min_alt = (uint32_t)o.min_alt; a.min_frac = o.min_frac;
    a.flag = d_flag.p; a.tile_flag = d_tile_flag.p; a.slot_counts = d_counts.p;
    {
        KTimer kt("variants_tile");
        launch_tiles<false>(in.enc, a, (uint32_t)in.n_tiles);
    }
    const std::vector<unsigned long long> counts = d_counts.download(3 * (size_t)n_slots);
    uint64_t n_sites = 0;
    for (uint32_t j = 0; j < n_slots; ++j) {
        out.callable[j] = counts[j];
        out.ref_other[j] = counts[n_slots + j];
        out.sites[j] = counts[2 * (size_t)n_slots + j];
        n_sites += out.sites[j];
    }
    if (!n_sites) return;                       // no select, no second pass
    // the counters gave the number of sites: the positions and the records take 28 bytes per site and nothing per position
    KTimer kt("variants_sites");
    DBuf<uint32_t> d_site_pos(n_sites), d_tile_list(in.n_tiles);
    DBuf<SiteRec> d_recs(n_sites);
    d_recs.fill_ff();
    if (select_flagged_indices(d_flag.p, d_site_pos.p, G) != n_sites) 
        fail(HLMI_ESTATE, "hlmi_variants: the site flags and the site counters differ");     // (never: one test sets both)
    const size_t n_list = select_flagged_indices(d_tile_flag.p, d_tile_list.p, in.n_tiles);
    out.tiles_revisited = n_list;
    a.tile_list = d_tile_list.p; a.n_list = (uint32_t)n_list;
    a.site_pos = d_site_pos.p; a.n_sites = (uint32_t)n_sites;
    a.recs = d_recs.p;
    if (n_list) launch_tiles<true>(in.enc, a, (uint32_t)n_list);
    out.recs = d_recs.download(n_sites);
}

}  // namespace var
}  // namespace hlmi
