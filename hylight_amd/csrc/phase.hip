// phase.hip - the device part of hlmi_phase / hlmi_phase_reads (include/hylight_mi.h): which allele every selected row reads at
// every variant site it spans, how the alleles of neighbouring sites go together, and how many sites of every block a row reads
// on either side.  The sites are hlmi_variants's (variants_core); the rows are sorted by (contig, ts) and the sites ascend, so
// the sites a row spans are a range [s_lo, s_hi) of the site array and the allele table is a CSR without an atomic.
//   phase_span_kernel     a thread per row: s_lo and s_hi - s_lo by two bounded binary searches; a scan gives the rows' offsets
//   phase_allele_kernel   a wave per row, walk_row over its compact CIGAR, lane = op: the sites inside the op's target range by
//                         two searches inside the row's range, the column's symbol against the site's own / alt (one packed byte
//                         per site), one allele byte written per site; an op with more than SHORT_RUN sites takes the wave
//                         (vote_columns).  The table is filled with AL_NONE first: columns no = X D op covers, and read bases
//                         that vote nothing, stay that
//   phase_link_kernel     a workgroup per tile of PHASE_TILE links (a link belongs to its left site): four counters per link in
//                         LDS; a wave per row of the tile's row range walks the row's allele bytes, 64 links a step, and bumps
//                         n[x][y] where both neighbours are 0 or 1; the flush writes 16 B per link.  A row lies in one contig, so
//                         no link across a junction is ever counted
//   (host)                blocks and phase bits from the link counters (phase_text.h: build_blocks); 5 B per site go back up
//   phase_slots_kernel    a thread per row: the blocks it touches, block_index[s_hi - 1] - block_index[s_lo] + 1; a scan
//   phase_assign_kernel   a thread per row walks its allele bytes once and writes one 24-byte record per block into its slots;
//                         <true> (hlmi_phase_reach): a site whose bit byte is BIT_BRIDGED counts in spanned alone
// With reach >= 1 the link pass is phase_reach.hip's, the blocks build_blocks_reach's; phase_ins.hip has a front of its own.
// Every loop is bounded by a count known at its head; the searches are counted.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "dev_prims.h"
#include "phase_internal.h"
#include "polish_walk.h"
#include "wave_ops.h"

namespace hlmi {
namespace ph {

using namespace pol;

namespace {

static_assert(sizeof(LinkCounts) == 16 && sizeof(ReadRec) == 24, "16 bytes per link, 24 per record");
static_assert(var::N_SYM == 5 && var::S_DEL == (int)SYM_DEL, "the five symbols are the polisher's");

constexpr int WG = 256, WAVES = WG / 64;
constexpr unsigned MAX_GRID = 1u << 16;         // blocks of a strided launch
inline dim3 grid1(size_t n) { return dim3((unsigned)std::min<size_t>(cdiv(n ? n : 1, WG), MAX_GRID)); }

// the first index of the ascending a[lo, hi) whose value is not below v (hi: none); hi - lo < 2^32: 32 steps at the most
__device__ __forceinline__ uint32_t lower_bound_in(const uint32_t *__restrict__ a, uint32_t lo, uint32_t hi, uint32_t v) {
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (a[m] < v) lo = m + 1;
        else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(WG) void phase_span_kernel(const PolRow *__restrict__ rows, uint32_t n_rows, const uint32_t *__restrict__ site_pos,
                                                        uint32_t n_sites, uint32_t *__restrict__ s_lo, uint32_t *__restrict__ cnt) {
    const uint32_t step = gridDim.x * WG;
    for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < n_rows; k += step) {
        const PolRow r = rows[k];
        const uint32_t lo = lower_bound_in(site_pos, 0, n_sites, r.cbase + r.ts);
        const uint32_t hi = lower_bound_in(site_pos, lo, n_sites, r.cbase + max(r.ts, r.te));
        s_lo[k] = lo;
        cnt[k] = hi - lo;
    }
}

struct AlleleArgs {
    const PolRow *rows;
    uint32_t n_rows;
    const uint32_t *ops;
    const uint8_t *reads;
    const uint32_t *site_pos;
    const uint8_t *site_pack;                   // own | alt << 4
    const uint32_t *s_lo, *cnt;
    const uint64_t *off;
    uint8_t *table;
};

template <int ENC>
__global__ __launch_bounds__(WG) void phase_allele_kernel(const AlleleArgs A) {
    const int lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * WAVES;
    for (uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6); k < A.n_rows; k += n_waves) {
        const uint32_t n = A.cnt[k];
        if (!n) continue;                                                       // (the same in every lane)
        const PolRow r = A.rows[k];
        const uint32_t lo = A.s_lo[k], hi = lo + n;
        uint8_t *out = A.table + A.off[k];
        // site s of [a, b) below lies inside this lane's op: lo <= a <= s < b <= hi, and its position inside [tp0, tp0 + len)
        auto put = [&](uint32_t s, uint32_t code, uint32_t tp0, uint32_t qc0, uint32_t) {
            const uint32_t p = A.site_pos[s] - r.cbase;
            const uint32_t sym = code == OP_D ? (uint32_t)SYM_DEL : column_symbol<ENC>(r, A.reads, qc0 + (p - tp0));
            if (sym >= (uint32_t)var::N_SYM) return;                            // an N of the read: AL_NONE stays
            const uint32_t pk = A.site_pack[s];
            out[s - lo] = sym == (pk & 15u) ? AL_OWN : sym == (pk >> 4) ? AL_ALT : AL_OTHER;
        };
        walk_row(r, A.ops, lane, r.te, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
            uint32_t a = 0, b = 0;              // the sites inside this op's target range
            if (len && (code == OP_EQ || code == OP_X || code == OP_D)) {
                const uint32_t t0 = max(tp0, r.ts), t1 = max(t0, min(tp0 + len, r.te));
                a = lower_bound_in(A.site_pos, lo, hi, r.cbase + t0);
                b = lower_bound_in(A.site_pos, a, hi, r.cbase + t1);
            }
            vote_columns<false>(a, b, code, tp0, qc0, 1u, lane, put);
        });
    }
}

__global__ __launch_bounds__(WG) void phase_link_kernel(const LinkTile *__restrict__ tiles, uint32_t n_tiles, uint32_t n_links, uint32_t n_rows,
                                                        const uint32_t *__restrict__ s_lo, const uint32_t *__restrict__ cnt,
                                                        const uint64_t *__restrict__ off, const uint8_t *__restrict__ table,
                                                        LinkCounts *__restrict__ links) {
    __shared__ uint32_t s_n[4][PHASE_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const uint32_t l0 = tile * (uint32_t)PHASE_TILE;
    if (l0 >= n_links) return;
    const uint32_t l1 = l0 + min((uint32_t)PHASE_TILE, n_links - l0);
    for (int i = tid; i < 4 * PHASE_TILE; i += WG) (&s_n[0][0])[i] = 0;
    __syncthreads();
    const LinkTile t = tiles[tile];
    const uint32_t row_hi = min(t.row_hi, n_rows);
    for (uint32_t k = t.row_lo + (uint32_t)wave; k < row_hi; k += WAVES) {
        const uint32_t n = cnt[k], lo = s_lo[k];
        if (n < 2) continue;
        // the links j whose two sites j and j + 1 both lie in [lo, lo + n), inside the tile
        const uint32_t j0 = max(lo, l0), j1 = min(lo + n - 1, l1);
        const uint8_t *a = table + off[k];
        for (uint32_t j = j0 + (uint32_t)lane; j < j1; j += 64) {
            const uint32_t x = a[j - lo], y = a[j + 1 - lo];
            if (x < 2 && y < 2) atomicAdd(&s_n[x * 2 + y][j - l0], 1u);         // l0 <= j < l1 <= l0 + PHASE_TILE
        }
    }
    __syncthreads();
    for (uint32_t i = (uint32_t)tid; i < l1 - l0; i += WG) links[l0 + i] = LinkCounts{s_n[0][i], s_n[1][i], s_n[2][i], s_n[3][i]};
}

__global__ __launch_bounds__(WG) void phase_slots_kernel(uint32_t n_rows, const uint32_t *__restrict__ s_lo, const uint32_t *__restrict__ cnt,
                                                         const uint32_t *__restrict__ block_index, uint32_t *__restrict__ slots) {
    const uint32_t step = gridDim.x * WG;
    for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < n_rows; k += step) {
        const uint32_t n = cnt[k], lo = s_lo[k];
        const uint32_t b0 = n ? block_index[lo] : 0u, b1 = n ? block_index[lo + n - 1] : 0u;
        slots[k] = n && b1 >= b0 ? b1 - b0 + 1 : 0u;                            // (block_index ascends: b1 >= b0)
    }
}

template <bool REACH>
__global__ __launch_bounds__(WG) void phase_assign_kernel(uint32_t n_rows, const uint32_t *__restrict__ s_lo, const uint32_t *__restrict__ cnt,
                                                          const uint64_t *__restrict__ off, const uint8_t *__restrict__ table,
                                                          const uint32_t *__restrict__ block_index, const uint8_t *__restrict__ bit,
                                                          const uint32_t *__restrict__ slots, const uint64_t *__restrict__ rec_off,
                                                          ReadRec *__restrict__ recs) {
    const uint32_t step = gridDim.x * WG;
    for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < n_rows; k += step) {
        const uint32_t n = cnt[k], n_slot = slots[k], lo = s_lo[k];
        if (!n || !n_slot) continue;
        const uint8_t *a = table + off[k];
        ReadRec *out = recs + rec_off[k];
        const uint32_t b0 = block_index[lo];
        ReadRec cur{k, b0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t blk = block_index[lo + i];
            if (blk != cur.block) {
                if (cur.block - b0 < n_slot) out[cur.block - b0] = cur;
                cur = ReadRec{k, blk, 0, 0, 0, 0};
            }
            const uint32_t al = a[i];
            ++cur.spanned;
            if (REACH && bit[lo + i] == BIT_BRIDGED) continue;
            if (al < 2) ++((al ^ (uint32_t)(bit[lo + i] & 1u)) == 0 ? cur.a : cur.b);
            else if (al == AL_OTHER) ++cur.other;
        }
        if (cur.block - b0 < n_slot) out[cur.block - b0] = cur;
    }
}

__global__ __launch_bounds__(WG) void phase_qrank_kernel(const PafRec *__restrict__ recs, const uint32_t *__restrict__ idx, size_t n_sel,
                                                         uint32_t *__restrict__ out) {
    const size_t step = (size_t)gridDim.x * WG;
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < n_sel; j += step) out[j] = recs[idx[j]].qid;
}

}  // namespace

void check_fits(const char *who, const char *what, uint64_t bytes) {
    const size_t avail = dev_available_bytes();             // 0: unknown
    if (avail && bytes > avail)
        fail(HLMI_EINVAL, "%s: %s of %llu bytes does not fit the device's free memory (%zu)", who, what, (unsigned long long)bytes, avail);
}

std::vector<LinkTile> link_tiles(const std::vector<uint32_t> &s_lo, const std::vector<uint32_t> &cnt, size_t n_links, size_t tile) {
    const size_t R = s_lo.size(), n_tiles = (n_links + tile - 1) / tile;
    std::vector<LinkTile> tiles(n_tiles);
    size_t lo = 0, hi = 0;
    for (size_t t = 0; t < n_tiles; ++t) {
        const uint64_t l0 = (uint64_t)t * tile, l1 = std::min<uint64_t>(l0 + tile, n_links);
        while (hi < R && s_lo[hi] < l1) ++hi;
        while (lo < hi && (uint64_t)s_lo[lo] + cnt[lo] < l0 + 2) ++lo;
        tiles[t] = LinkTile{(uint32_t)lo, (uint32_t)hi};
    }
    return tiles;
}

std::vector<uint32_t> selected_query_ranks(const PafRec *recs, const uint32_t *idx, size_t n_sel) {
    if (!n_sel) return {};
    DBuf<uint32_t> d(n_sel);
    hipLaunchKernelGGL(phase_qrank_kernel, grid1(n_sel), dim3(WG), 0, stream(), recs, idx, n_sel, d.p);
    HIP_CHECK(hipGetLastError());
    return d.download(n_sel);
}

void phase_core(const char *who, const PolCoreIn &in, const std::vector<PSite> &sites, const hlmi_phase_opts &o, DevicePhase &out,
                DevRecs *keep, int reach) {
    out = DevicePhase{};
    out.far.reach = reach;
    if (keep) *keep = DevRecs{};
    const size_t N = sites.size(), R = in.n_rows;
    DBuf<uint32_t> d_pos, d_lo, d_cnt;
    DBuf<uint8_t> d_pack, d_table;
    DBuf<uint64_t> d_off;
    if (N >= (1ull << 31)) fail(HLMI_EINVAL, "%s: %zu sites (2^31 and more)", who, N);              // (never: positions < 2^31)
    if (N && R) {
        d_lo.alloc(R);
        d_cnt.alloc(R);
        d_off.alloc(R);
        KTimer kt("phase_allele");
        std::vector<uint32_t> pos(N);
        std::vector<uint8_t> pack(N);
        for (size_t i = 0; i < N; ++i) {
            pos[i] = sites[i].gpos;
            pack[i] = (uint8_t)(sites[i].own | sites[i].alt << 4);
        }
        d_pos.upload(pos);
        d_pack.upload(pack);
        hipLaunchKernelGGL(phase_span_kernel, grid1(R), dim3(WG), 0, stream(), in.rows, (uint32_t)R, d_pos.p, (uint32_t)N, d_lo.p, d_cnt.p);
        HIP_CHECK(hipGetLastError());
        exclusive_scan_u32_to_u64(d_cnt.p, d_off.p, R);
        out.alleles = download_one(d_off.p + (R - 1)) + download_one(d_cnt.p + (R - 1));
        if (out.alleles >= (1ull << 32)) fail(HLMI_EINVAL, "%s: %llu alleles of rows at sites (2^32 and more)", who, (unsigned long long)out.alleles);
        check_fits(who, "the allele table", out.alleles);
        if (out.alleles) {
            d_table.alloc(out.alleles);
            d_table.fill_ff();                  // AL_NONE
            AlleleArgs a{in.rows, (uint32_t)R, in.ops, in.reads, d_pos.p, d_pack.p, d_lo.p, d_cnt.p, d_off.p, d_table.p};
            const dim3 g((unsigned)std::min<size_t>(cdiv(R, WAVES), MAX_GRID));
            if (in.enc == READS_CODES) hipLaunchKernelGGL((phase_allele_kernel<READS_CODES>), g, dim3(WG), 0, stream(), a);
            else hipLaunchKernelGGL((phase_allele_kernel<READS_ASCII>), g, dim3(WG), 0, stream(), a);
            HIP_CHECK(hipGetLastError());
        }
    }
    phase_tail(who, R, sites, o, out, keep, reach, d_lo, d_cnt, d_off, d_table);
}

void phase_tail(const char *who, size_t R, const std::vector<PSite> &sites, const hlmi_phase_opts &o, DevicePhase &out, DevRecs *keep, int reach,
                const DBuf<uint32_t> &d_lo, const DBuf<uint32_t> &d_cnt, const DBuf<uint64_t> &d_off, const DBuf<uint8_t> &d_table) {
    const size_t N = sites.size(), n_links = N ? N - 1 : 0;
    std::vector<uint32_t> s_lo, cnt;
    // the blocks from what the link pass left: neighbours alone (reach 0), or every distance up to reach
    auto blocks = [&]() {
        if (!reach) {
            out.blocks = build_blocks(sites, out.links, o.min_link, o.min_agree);
            return;
        }
        const ReachBlocks rb = build_blocks_reach(sites, out.far, o.min_link, o.min_agree);
        out.blocks = rb.base;
        out.links_far = rb.links_far;
        out.links_far_phased = rb.links_far_phased;
        out.joins_far = rb.joins_far;
        out.sites_bridged = rb.sites_bridged;
        out.links_conflict = rb.links_conflict;
    };
    out.links.assign(n_links, LinkCounts{0, 0, 0, 0});
    if (reach) out.far.n.assign(n_links * (size_t)reach, LinkCounts{0, 0, 0, 0});
    if (out.alleles && n_links && reach) {
        KTimer kt("phase_link_reach");
        s_lo = d_lo.download(R);
        cnt = d_cnt.download(R);
        link_reach(who, s_lo, cnt, n_links, d_lo.p, d_cnt.p, d_off.p, d_table.p, out.far);
        for (size_t j = 0; j < n_links; ++j) out.links[j] = out.far.at(j, 1);
    } else if (out.alleles && n_links) {
        KTimer kt("phase_link");
        s_lo = d_lo.download(R);
        cnt = d_cnt.download(R);
        // the rows of every tile of links as polish_layout finds a position tile's: from the first row that holds a link of the
        // tile or a later one to the last row that starts in front of the tile's end (s_lo ascends with the rows)
        const std::vector<LinkTile> tiles = link_tiles(s_lo, cnt, n_links, PHASE_TILE);
        const size_t n_tiles = tiles.size();
        DBuf<LinkTile> d_tiles;
        d_tiles.upload(tiles);
        DBuf<LinkCounts> d_links(n_links);
        hipLaunchKernelGGL(phase_link_kernel, dim3((unsigned)n_tiles), dim3(WG), 0, stream(), d_tiles.p, (uint32_t)n_tiles, (uint32_t)n_links,
                           (uint32_t)R, d_lo.p, d_cnt.p, d_off.p, d_table.p, d_links.p);
        HIP_CHECK(hipGetLastError());
        out.links = d_links.download(n_links);
    }
    blocks();
    if (out.alleles) {
        KTimer kt("phase_assign");
        DBuf<uint32_t> d_index, d_slots(R);
        DBuf<uint8_t> d_bit;
        DBuf<uint64_t> d_rec_off(R);
        d_index.upload(out.blocks.index);
        d_bit.upload(out.blocks.bit);
        hipLaunchKernelGGL(phase_slots_kernel, grid1(R), dim3(WG), 0, stream(), (uint32_t)R, d_lo.p, d_cnt.p, d_index.p, d_slots.p);
        HIP_CHECK(hipGetLastError());
        exclusive_scan_u32_to_u64(d_slots.p, d_rec_off.p, R);
        const uint64_t n_recs = download_one(d_rec_off.p + (R - 1)) + download_one(d_slots.p + (R - 1));
        if (n_recs > out.alleles) fail(HLMI_ESTATE, "%s: more (row, block) records than alleles", who);    // (never: a block has a site)
        check_fits(who, "the rows' block records", n_recs * sizeof(ReadRec));
        if (n_recs) {
            DBuf<ReadRec> d_recs(n_recs);
            d_recs.zero();
            if (reach)
                hipLaunchKernelGGL(phase_assign_kernel<true>, grid1(R), dim3(WG), 0, stream(), (uint32_t)R, d_lo.p, d_cnt.p, d_off.p, d_table.p,
                                   d_index.p, d_bit.p, d_slots.p, d_rec_off.p, d_recs.p);
            else
                hipLaunchKernelGGL(phase_assign_kernel<false>, grid1(R), dim3(WG), 0, stream(), (uint32_t)R, d_lo.p, d_cnt.p, d_off.p, d_table.p,
                                   d_index.p, d_bit.p, d_slots.p, d_rec_off.p, d_recs.p);
            HIP_CHECK(hipGetLastError());
            out.recs = d_recs.download(n_recs);
            if (keep) {
                keep->recs = std::move(d_recs);
                keep->off = std::move(d_rec_off);
                keep->cnt = std::move(d_slots);
                keep->n = n_recs;
            }
        }
    }
}

}  // namespace ph
}  // namespace hlmi
