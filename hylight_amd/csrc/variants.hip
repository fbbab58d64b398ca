// variants.hip - the device part of hlmi_variants / hlmi_variants_reads and of their _ins forms (include/hylight_mi.h): the votes of
// the selected rows per contig position, the site rule, and the sites' records; with INS the slots' counters, the insertion site
// rule and the insertion sites' records beside them.
//   var_tile_kernel<ENC, false, INS>  a workgroup per tile of polish_layout: five 32-bit counters per position in LDS (A C G T del,
//                                 20 KiB), the rows walked and voted by the loops of polish_count_kernel (polish_walk.h); the flush
//                                 applies the site rule and writes one flag byte per position; the tile's callable, ref_other and
//                                 site counts are reduced in the workgroup and added to its contig's three 64-bit counters with
//                                 one global atomic each; one byte per tile says whether it holds a site.
//                                 INS: four counters more per position (non-voting columns, row starts, inserting rows of 1..16
//                                 bases, long rows: 36 KiB); span = c + other - starts as polish_count_kernel's flush has it; the
//                                 flush applies both rules, writes a second flag byte per position, adds slots_callable and
//                                 ins_sites to two more 64-bit counters, and the tile's byte says "a site of either kind"
//   select_flagged_indices        over the position flags: the sites' positions, ascending; over the tile bytes: the tiles to revisit
//   var_tile_kernel<ENC, true, INS>   over those tiles only: counts again, and a site's thread finds its place in the site array by
//                                 binary search and writes its 24-byte record (position, five counts) there; INS: an insertion
//                                 site's thread writes (position, s, i, l) of its 40-byte record the same way
//   slot passes (INS)             over the insertion sites with an inserting row: polish_slot_votes (polish.hip) - the polisher's
//                                 own length votes, winning lengths and base votes, through a slot_of map of these sites; then
//                                 ins_call_kernel, a thread per insertion site: len, len_count and the bases into its record
// Why two passes and no record per position: the counters of a position that is no site are never needed, and sites are few
// (a strain-pure contig has none), so what leaves the CU in pass 1 is one byte per position; the records' memory is 24 B per
// site, their order is the order of the selected flags - ascending by construction, whatever order the atomics ran in.  The
// price is that the tiles with a site are counted twice (DESIGN.md section 4.3j has the byte formula).  With no site the select
// over the tiles and the second pass are not launched.  Every loop is bounded by a count known at its head.
// QF (hlmi_variants_q and its forms with min_base_qual > 0): a column whose Phred lies below the floor casts no vote, as an N
// column casts none (variants_qual.h has the judgement; with INS it still spans: C_OTHER).  The quality byte is fetched at the
// index column_symbol fetches the base at; a D op's pass or fail is its lane's, once per op, and travels as wd through
// vote_columns<true>.  The withheld votes are counted per lane, summed per wave, then in one LDS word, and reach one 64-bit
// counter of the call with one global atomic per workgroup - in pass 1 only.  No LDS plane is added.  QF = false is the kernel
// as it was: no quality byte is read.
#include <hip/hip_runtime.h>

#include "common.h"
#include "dev_prims.h"
#include "polish_walk.h"
#include "variants_internal.h"
#include "variants_qual.h"
#include "wave_ops.h"

namespace hlmi {
namespace var {

using namespace pol;

namespace {

static_assert(N_SYM == 5 && S_DEL == (int)SYM_DEL && (int)C_OTHER == N_SYM, "the five symbols are the polisher's");
static_assert(sizeof(SiteRec) == 24, "a site's record is 24 bytes");
static_assert(sizeof(InsRec) == 40 && INS_CAP == (uint32_t)POLISH_INS_CAP, "an insertion site's record is 40 bytes, the cap the polisher's");

// INS: the slots' counters behind the five symbols and C_OTHER (polish_walk.h) - row starts, inserting rows (1..16 bases), long rows
constexpr int C_START = 6, C_INS = 7, C_LONG = 8, N_CNT_INS = 9;

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
    // INS: the second flag per position; slot_counts holds slots_callable and ins_sites behind the three; the insertion sites'
    // positions and records, and per insertion site "a row inserts 1..16 bases here" for the slot passes
    uint8_t *ins_flag;
    const uint32_t *ins_pos;
    uint32_t n_ins;
    InsRec *ins_recs;
    uint8_t *ins_voted;
    // QF: the quality bytes, indexed exactly like `reads` by PolRow::read_off; the floor (1..93); pass 1 out: the withheld votes
    const uint8_t *quals;
    uint32_t min_base_qual;
    unsigned long long *low_count;
};

template <int ENC, bool EMIT, bool INS, bool QF>
__global__ __launch_bounds__(POLISH_WG) void var_tile_kernel(const VarArgs A) {
    constexpr int N_CNT = INS ? N_CNT_INS : N_SYM, N_TOT = INS ? 5 : 3;
    constexpr int N_WORDS = N_TOT + (QF && !EMIT ? 1 : 0);         // QF, pass 1: the workgroup's withheld votes behind the totals
    __shared__ uint32_t s_cnt[N_CNT][POLISH_TILE];
    __shared__ uint32_t s_tot[N_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t tile = blockIdx.x;
    if constexpr (EMIT) {
        if (tile >= A.n_list) return;
        tile = A.tile_list[tile];
    }
    if (tile >= A.n_tiles) return;
    const PolTile t = A.tiles[tile];
    const uint32_t n_pos = min(t.n_pos, (uint32_t)POLISH_TILE), t_end = t.t0 + n_pos;
    for (int i = tid; i < N_CNT * POLISH_TILE; i += POLISH_WG) (&s_cnt[0][0])[i] = 0;
    if (tid < N_WORDS) s_tot[tid] = 0;
    __syncthreads();
    uint32_t n_low = 0;                         // QF: the votes this lane withheld (a tile has at most POLISH_TILE x rows columns)
    const uint32_t row_hi = min(t.row_hi, A.n_rows);
    for (uint32_t k = t.row_lo + (uint32_t)wave; k < row_hi; k += POLISH_WAVES) {
        const PolRow r = A.rows[k];
        if (r.te <= t.t0 || r.ts >= t_end) continue;
        if constexpr (INS)
            if (lane == 0 && r.ts >= t.t0) atomicAdd(&s_cnt[C_START][r.ts - t.t0], 1u);        // r.ts < t_end
        auto vote = [&](uint32_t p, uint32_t code, uint32_t tp0, uint32_t qc0, uint32_t wd) {
            uint32_t s = code == OP_D ? (uint32_t)SYM_DEL : column_symbol<ENC>(r, A.reads, qc0 + (p - tp0));
            if constexpr (QF) {
                // A column that votes anyway (an N, another byte: s == C_OTHER) is not judged.  s < 4: column_symbol found
                // col < r.qn, so vq_index(...) < r.qn and the byte lies inside [read_off, read_off + qn) - the argument that
                // covers the base fetch.  A D column carries its op's verdict (wd: 1 passes, 0 fails).
                if (s < (uint32_t)N_SYM) {
                    const bool pass = code == OP_D ? wd != 0u
                                                   : vq_byte_passes(A.quals[r.read_off + vq_index(r.qn, r.rev, qc0 + (p - tp0))], A.min_base_qual);
                    if (!pass) {
                        s = (uint32_t)C_OTHER;
                        if constexpr (!EMIT) ++n_low;
                    }
                }
            }
            // t.t0 <= p < t_end: [a, b) is clipped.  INS counts the column that votes nothing too (s == C_OTHER): it spans
            if (s < (uint32_t)(INS ? C_OTHER + 1 : N_SYM)) atomicAdd(&s_cnt[s][p - t.t0], 1u);
        };
        walk_row(r, A.ops, lane, t_end, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
            if constexpr (INS)                  // one I op is one slot's insertion (polish_rows.h); at ts or te it belongs to none
                if (code == OP_I && len >= 1 && tp0 > r.ts && tp0 < r.te && tp0 >= t.t0 && tp0 < t_end)
                    atomicAdd(&s_cnt[len <= (uint32_t)POLISH_INS_CAP ? C_INS : C_LONG][tp0 - t.t0], 1u);
            uint32_t a = 0, b = 0;              // the columns of this op inside the tile
            if (code == OP_EQ || code == OP_X || code == OP_D) {
                a = max(tp0, t.t0);
                b = max(a, min(tp0 + len, t_end));
            }
            uint32_t wd = 1u;                   // QF: a D op's pass or fail, once per op, by its lane; its flanks are tested
            if constexpr (QF)                   // against [0, r.qn) inside vq_del_passes, whose bytes are the row's stretch
                if (code == OP_D && b > a) wd = vq_del_passes(A.quals + r.read_off, r.qn, r.rev, qc0, A.min_base_qual) ? 1u : 0u;
            vote_columns<QF>(a, b, code, tp0, qc0, wd, lane, vote);
        });
    }
    __syncthreads();
    uint32_t n_call = 0, n_other = 0, n_site = 0, n_slot = 0, n_ins = 0;
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
        if constexpr (INS) {
            // the slot in front of the position: the rows that cover it, less the ones that start on it, span it (position 0 of a
            // contig: every row that covers it starts on it, span 0 - no slot)
            const uint32_t span = c + s_cnt[C_OTHER][i] - s_cnt[C_START][i], ins = s_cnt[C_INS][i], lng = s_cnt[C_LONG][i];
            bool isite = false;
            if (span >= A.min_cov) {
                ++n_slot;
                const uint32_t alt = ins + lng;
                isite = alt >= A.min_alt && (double)alt / (double)span >= A.min_frac;          // one IEEE division; span >= 1
            }
            if constexpr (!EMIT) {
                A.ins_flag[g] = isite;
                n_ins += isite;
            } else if (isite) {
                const uint32_t at = lower_bound_u32(A.ins_pos, A.n_ins, g);
                if (at < A.n_ins && A.ins_pos[at] == g) {
                    InsRec *rec = A.ins_recs + at;      // len, len_count and seq are ins_call_kernel's
                    rec->pos = g; rec->span = span; rec->ins = ins; rec->ins_long = lng;
                    A.ins_voted[at] = ins != 0;
                }
            }
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
        if constexpr (INS) {
            const uint32_t w_slot = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(n_slot), 63);
            const uint32_t w_ins = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(n_ins), 63);
            if (lane == 0) {
                if (w_slot) atomicAdd(&s_tot[3], w_slot);
                if (w_ins) atomicAdd(&s_tot[4], w_ins);
            }
        }
        if constexpr (QF) {
            const uint32_t w_low = (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_incl_dpp(n_low), 63);
            if (lane == 0 && w_low) atomicAdd(&s_tot[N_TOT], w_low);
        }
        __syncthreads();
        if (tid == 0) {
            if constexpr (QF)
                if (s_tot[N_TOT]) atomicAdd(A.low_count, (unsigned long long)s_tot[N_TOT]);
            const uint32_t j = slot_of_position(A.cbase, A.n_slots, t.cbase);
            if (s_tot[0]) atomicAdd(&A.slot_counts[j], (unsigned long long)s_tot[0]);
            if (s_tot[1]) atomicAdd(&A.slot_counts[A.n_slots + j], (unsigned long long)s_tot[1]);
            if (s_tot[2]) atomicAdd(&A.slot_counts[2 * (size_t)A.n_slots + j], (unsigned long long)s_tot[2]);
            if constexpr (INS) {
                if (s_tot[3]) atomicAdd(&A.slot_counts[3 * (size_t)A.n_slots + j], (unsigned long long)s_tot[3]);
                if (s_tot[4]) atomicAdd(&A.slot_counts[4 * (size_t)A.n_slots + j], (unsigned long long)s_tot[4]);
                A.tile_flag[tile] = (s_tot[2] | s_tot[4]) != 0;
            } else
                A.tile_flag[tile] = s_tot[2] != 0;
        }
    }
}

// A thread per insertion site: the winning length, its rows and the bases from the counters the slot passes left (slot_of: the
// site's place among those with an inserting row, POLISH_NO_SLOT or no map at all: no row inserts 1..16 bases - len 0).  The
// base of an index is the first of A C G T among the most frequent, N with no vote: write_kernel's decision (polish.hip).
__global__ void ins_call_kernel(const uint32_t *__restrict__ ins_pos, uint32_t n_ins, const uint32_t *__restrict__ slot_of,
                                const uint8_t *__restrict__ win_len, const uint32_t *__restrict__ len_cnt,
                                const uint32_t *__restrict__ base_cnt, InsRec *__restrict__ recs) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_ins) return;
    const uint32_t s = slot_of ? slot_of[ins_pos[k]] : POLISH_NO_SLOT;
    uint32_t len = 0, len_count = 0;
    if (s != POLISH_NO_SLOT) {
        len = min((uint32_t)win_len[s], (uint32_t)POLISH_INS_CAP);
        if (len) len_count = len_cnt[(size_t)s * POLISH_INS_CAP + len - 1];
    }
    InsRec *rec = recs + k;
    rec->len = len;
    rec->len_count = len_count;
    for (uint32_t j = 0; j < (uint32_t)POLISH_INS_CAP; ++j) {
        char b = 'N';
        if (j < len) {
            const uint32_t *c = base_cnt + ((size_t)s * POLISH_INS_CAP + j) * 4;
            uint32_t best = 0;
            for (int q = 0; q < 4; ++q)
                if (c[q] > best) { best = c[q]; b = "ACGT"[q]; }
        }
        rec->seq[j] = b;
    }
}

__global__ void gather_u32_kernel(const uint32_t *__restrict__ from, const uint32_t *__restrict__ at, uint32_t n, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = from[at[i]];
}

template <bool EMIT, bool INS, bool QF>
void launch_tiles_of(ReadEnc enc, const VarArgs &a, uint32_t n_blocks) {
    if (enc == READS_CODES)
        hipLaunchKernelGGL((var_tile_kernel<READS_CODES, EMIT, INS, QF>), dim3(n_blocks), dim3(POLISH_WG), 0, stream(), a);
    else hipLaunchKernelGGL((var_tile_kernel<READS_ASCII, EMIT, INS, QF>), dim3(n_blocks), dim3(POLISH_WG), 0, stream(), a);
    HIP_CHECK(hipGetLastError());
}
// a.quals == nullptr: no floor, the kernel as it always was
template <bool EMIT, bool INS>
void launch_tiles(ReadEnc enc, const VarArgs &a, uint32_t n_blocks) {
    if (a.quals) launch_tiles_of<EMIT, INS, true>(enc, a, n_blocks);
    else launch_tiles_of<EMIT, INS, false>(enc, a, n_blocks);
}

// The slot passes of the _ins calls over the n_ins insertion sites at d_ins_pos, whose records hold (pos, s, i, l) and whose
// d_voted says which have an inserting row: the polisher's slot votes over those, then every record's len, len_count and seq.
// -> the sites the votes ran over.  No counter array comes to the host.
size_t ins_slot_passes(const PolCoreIn &in, const uint32_t *d_ins_pos, size_t n_ins, const uint8_t *d_voted, InsRec *d_recs) {
    constexpr int B = 256;
    KTimer kt("variants_slots");
    DBuf<uint32_t> d_at(n_ins);
    const size_t n_v = select_flagged_indices(d_voted, d_at.p, n_ins);
    DBuf<uint32_t> d_vpos(n_v), d_slot_of(n_v ? in.n_contig : 0), d_len_cnt(n_v * POLISH_INS_CAP), d_base_cnt(n_v * POLISH_INS_CAP * 4);
    DBuf<uint8_t> d_win_len(n_v);
    if (n_v) {
        hipLaunchKernelGGL(gather_u32_kernel, dim3(cdiv(n_v, B)), dim3(B), 0, stream(), d_ins_pos, d_at.p, (uint32_t)n_v, d_vpos.p);
        d_slot_of.fill_ff();
        d_len_cnt.zero();
        d_base_cnt.zero();
        PolCoreIn unweighted = in;              // no quality byte is read: the votes count rows
        unweighted.quals = nullptr;
        polish_slot_votes(unweighted, d_vpos.p, n_v, d_slot_of.p, d_win_len.p, d_len_cnt.p, d_base_cnt.p);
    }
    hipLaunchKernelGGL(ins_call_kernel, dim3(cdiv(n_ins, B)), dim3(B), 0, stream(), d_ins_pos, (uint32_t)n_ins, d_slot_of.p, d_win_len.p,
                       d_len_cnt.p, d_base_cnt.p, d_recs);
    HIP_CHECK(hipGetLastError());
    return n_v;
}

// ins == nullptr: hlmi_variants's device part as it always was.  min_base_qual > 0 (the _q calls; in.quals is then set unless
// there is no read byte at all): the floor, and *low gets the withheld votes; 0: no quality byte is read, *low stays 0.
template <bool INS>
void core_impl(const PolCoreIn &in, const hlmi_variant_opts &o, int min_base_qual, DeviceVariants &out, DeviceInsertions *ins,
               uint64_t *low) {
    constexpr size_t N_COUNTS = INS ? 5 : 3;
    out = DeviceVariants{};
    const size_t G = in.n_contig;               // < 2^31 (polish_layout)
    const uint32_t n_slots = in.n_cbase ? (uint32_t)(in.n_cbase - 1) : 0u;
    out.callable.assign(n_slots, 0);
    out.ref_other.assign(n_slots, 0);
    out.sites.assign(n_slots, 0);
    out.tiles = in.n_tiles;
    if constexpr (INS) {
        *ins = DeviceInsertions{};
        ins->slots_callable.assign(n_slots, 0);
        ins->ins_sites.assign(n_slots, 0);
    }
    if (!G || !n_slots || !in.n_tiles) return;
    if (in.n_tiles >= (1ull << 32)) fail(HLMI_EINVAL, "hlmi_variants: %zu tiles (2^32 and more)", in.n_tiles);      // (never: G < 2^31)
    DBuf<uint8_t> d_flag(G), d_tile_flag(in.n_tiles), d_ins_flag(INS ? G : 0);
    DBuf<unsigned long long> d_counts(N_COUNTS * (size_t)n_slots), d_low(1);
    d_flag.zero();                              // positions of a covered contig that no tile holds: no site
    d_ins_flag.zero();
    d_counts.zero();
    d_low.zero();
    VarArgs a{};
    a.rows = in.rows; a.n_rows = in.n_rows;
    a.ops = in.ops;
    a.reads = in.reads; a.contig = in.contig; a.n_contig = (uint32_t)G;
    a.tiles = in.tiles; a.n_tiles = (uint32_t)in.n_tiles;
    a.cbase = in.cbase; a.n_slots = n_slots;
    a.min_cov = (uint32_t)o.min_cov; a.min_alt = (uint32_t)o.min_alt; a.min_frac = o.min_frac;
    a.flag = d_flag.p; a.tile_flag = d_tile_flag.p; a.slot_counts = d_counts.p;
    a.ins_flag = d_ins_flag.p;
    if (min_base_qual > 0 && in.quals) {
        a.quals = in.quals; a.min_base_qual = (uint32_t)min_base_qual; a.low_count = d_low.p;
    }
    {
        KTimer kt("variants_tile");
        launch_tiles<false, INS>(in.enc, a, (uint32_t)in.n_tiles);
    }
    const std::vector<unsigned long long> counts = d_counts.download(N_COUNTS * (size_t)n_slots);
    if (low && a.quals) *low = download_one(d_low.p);
    uint64_t n_sites = 0, n_ins = 0;
    for (uint32_t j = 0; j < n_slots; ++j) {
        out.callable[j] = counts[j];
        out.ref_other[j] = counts[n_slots + j];
        out.sites[j] = counts[2 * (size_t)n_slots + j];
        n_sites += out.sites[j];
        if constexpr (INS) {
            ins->slots_callable[j] = counts[3 * (size_t)n_slots + j];
            ins->ins_sites[j] = counts[4 * (size_t)n_slots + j];
            n_ins += ins->ins_sites[j];
        }
    }
    if (!n_sites && !n_ins) return;             // no select, no second pass, no slot pass
    // the counters gave the number of sites: the positions and the records take 28 bytes per site and nothing per position
    // (44 per insertion site)
    DBuf<uint32_t> d_site_pos(n_sites), d_tile_list(in.n_tiles), d_ins_pos(n_ins);
    DBuf<SiteRec> d_recs(n_sites);
    DBuf<InsRec> d_ins_recs(n_ins);
    DBuf<uint8_t> d_ins_voted(n_ins);
    {
        KTimer kt("variants_sites");
        d_recs.fill_ff();
        d_ins_recs.fill_ff();
        d_ins_voted.zero();
        if (n_sites && select_flagged_indices(d_flag.p, d_site_pos.p, G) != n_sites)
            fail(HLMI_ESTATE, "hlmi_variants: the site flags and the site counters differ");     // (never: one test sets both)
        if (n_ins && select_flagged_indices(d_ins_flag.p, d_ins_pos.p, G) != n_ins)
            fail(HLMI_ESTATE, "hlmi_variants_ins: the insertion flags and their counters differ");       // (never, as above)
        const size_t n_list = select_flagged_indices(d_tile_flag.p, d_tile_list.p, in.n_tiles);
        out.tiles_revisited = n_list;
        a.tile_list = d_tile_list.p; a.n_list = (uint32_t)n_list;
        a.site_pos = d_site_pos.p; a.n_sites = (uint32_t)n_sites;
        a.recs = d_recs.p;
        a.ins_pos = d_ins_pos.p; a.n_ins = (uint32_t)n_ins;
        a.ins_recs = d_ins_recs.p; a.ins_voted = d_ins_voted.p;
        if (n_list) launch_tiles<true, INS>(in.enc, a, (uint32_t)n_list);
    }
    if constexpr (INS)
        if (n_ins) {
            ins->slot_sites = ins_slot_passes(in, d_ins_pos.p, n_ins, d_ins_voted.p, d_ins_recs.p);
            ins->recs = d_ins_recs.download(n_ins);
        }
    out.recs = d_recs.download(n_sites);
}

}  // namespace

void variants_core(const PolCoreIn &in, const hlmi_variant_opts &o, DeviceVariants &out) {
    core_impl<false>(in, o, 0, out, nullptr, nullptr);
}

void variants_ins_core(const PolCoreIn &in, const hlmi_variant_opts &o, DeviceVariants &out, DeviceInsertions &ins) {
    core_impl<true>(in, o, 0, out, &ins, nullptr);
}

void variants_q_core(const PolCoreIn &in, const hlmi_variant_opts &o, int min_base_qual, DeviceVariants &out, uint64_t &columns_low_qual) {
    columns_low_qual = 0;
    core_impl<false>(in, o, min_base_qual, out, nullptr, &columns_low_qual);
}

void variants_ins_q_core(const PolCoreIn &in, const hlmi_variant_opts &o, int min_base_qual, DeviceVariants &out, DeviceInsertions &ins,
                         uint64_t &columns_low_qual) {
    columns_low_qual = 0;
    core_impl<true>(in, o, min_base_qual, out, &ins, &columns_low_qual);
}

}  // namespace var
}  // namespace hlmi
