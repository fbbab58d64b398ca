// polish.hip - the device part of hlmi_polish (include/hylight_mi.h): column votes of the selected rows' CIGARs, the
// decisions per position and per slot, and the new contigs' bases.
//   count pass   a workgroup owns one tile of POLISH_TILE positions of one contig: eight 32-bit counters per position in LDS
//                (A C G T del, non-voting columns, row starts, inserting rows); its waves walk the CIGARs of the rows that
//                overlap the tile, 64 ops at a time with DPP prefix sums for the target and query columns; the tile then
//                decides its positions and slots itself and writes one decision byte and one slot flag per position - no
//                counter ever reaches global memory, and no global atomic is needed
//   slot passes  opened slots are few: a wave per row walks its CIGAR once more and votes with global atomics into the 16
//                length counters of each opened slot, then, the lengths decided, into the 16 x 4 base counters
//   write        a thread per position: output length, a device scan for the offsets, one kernel for the bytes
// Every counter is 32 bits wide: coverage needs no overflow path.  Every loop is bounded by a count known at its head.
// QW (hlmi_polish_q with qual_weight = 1): a vote weighs max(1, quality byte - 33) of its read base.  The count pass then keeps a
// ninth LDS counter per position - the number of voting columns, which the coverage test and the slot's span still are - and the
// five symbol counters hold weight sums; the slot passes add weights where they added 1.  QW = false is the kernels as they
// were: no quality byte is read, eight counters.
// polish_upload sends up what polish_host.cpp built from a PAF; hlmi_polish_reads (polish_rows.hip) runs polish_core over
// rows, CIGARs and reads that are in device memory already - its reads as the overlapper's codes (column_symbol).
// column_symbol, walk_row and the lane / wave switch of the vote loop are polish_walk.h's, shared with variants.hip.
// polish_tail is everything behind the count pass - slot index, slot passes, lengths, scan, write - over any position space:
// hlmi_haplotigs (haplotigs.hip) runs it over two sides side by side with slot votes of its own.  polish_slot_votes is the slot
// passes alone over slots the caller chose: hlmi_variants_ins (variants.hip) votes the lengths and bases of its insertion sites.
#include <hip/hip_runtime.h>

#include "common.h"
#include "dev_prims.h"
#include "polish_internal.h"
#include "polish_select.h"
#include "polish_walk.h"
#include "wave_ops.h"

namespace hlmi {
namespace pol {
namespace {

constexpr int C_START = 6, C_INS = 7, POLISH_CNT = 8;                  // counters behind the five symbols and C_OTHER (polish_walk.h)
constexpr int C_VOTES = 8, POLISH_CNT_QW = 9;                          // QW: voting columns, behind the others
constexpr uint32_t NO_SLOT = 0xffffffffu;

// weight of alignment column `col` of row r: max(1, Phred), the byte fetched at the index column_symbol fetches the base at
__device__ __forceinline__ uint32_t column_weight(const PolRow &r, const uint8_t *__restrict__ quals, uint32_t col) {
    if (col >= r.qn) return 1u;                                        // (validated on the host: never)
    const uint32_t q = quals[r.read_off + (r.rev ? r.qn - 1 - col : col)];
    return q > 34u ? q - 33u : 1u;
}
// weight of a D op whose first query column behind it is qc: the lower of its flanks, of those inside [0, qn); none: 1
__device__ __forceinline__ uint32_t del_weight(const PolRow &r, const uint8_t *__restrict__ quals, uint32_t qc) {
    uint32_t w = 0xffffffffu;
    if (qc >= 1 && qc - 1 < r.qn) w = column_weight(r, quals, qc - 1);
    if (qc < r.qn) w = min(w, column_weight(r, quals, qc));
    return w == 0xffffffffu ? 1u : w;
}

template <int ENC, bool QW>
__global__ __launch_bounds__(POLISH_WG) void polish_count_kernel(const PolRow *__restrict__ rows, const uint32_t *__restrict__ ops,
                                                                 const uint8_t *__restrict__ reads, const uint8_t *__restrict__ contig,
                                                                 const PolTile *__restrict__ tiles, int min_cov,
                                                                 uint8_t *__restrict__ sym, uint8_t *__restrict__ open,
                                                                 const uint8_t *__restrict__ quals) {
    constexpr int N_CNT = QW ? POLISH_CNT_QW : POLISH_CNT;
    __shared__ uint32_t s_cnt[N_CNT][POLISH_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PolTile t = tiles[blockIdx.x];
    const uint32_t t_end = t.t0 + t.n_pos;
    for (int i = tid; i < N_CNT * POLISH_TILE; i += POLISH_WG) (&s_cnt[0][0])[i] = 0;
    __syncthreads();
    for (uint32_t k = t.row_lo + (uint32_t)wave; k < t.row_hi; k += POLISH_WAVES) {
        const PolRow r = rows[k];
        if (r.te <= t.t0 || r.ts >= t_end) continue;
        if (lane == 0 && r.ts >= t.t0) atomicAdd(&s_cnt[C_START][r.ts - t.t0], 1u);
        // wd: the weight of the op's columns when it is a D op (QW only)
        auto vote = [&](uint32_t p, uint32_t code, uint32_t tp0, uint32_t qc0, uint32_t wd) {
            const uint32_t s = code == OP_D ? (uint32_t)SYM_DEL : column_symbol<ENC>(r, reads, qc0 + (p - tp0));
            if constexpr (QW) {
                if (s == C_OTHER) atomicAdd(&s_cnt[C_OTHER][p - t.t0], 1u);
                else {
                    atomicAdd(&s_cnt[s][p - t.t0], code == OP_D ? wd : column_weight(r, quals, qc0 + (p - tp0)));
                    atomicAdd(&s_cnt[C_VOTES][p - t.t0], 1u);
                }
            } else
                atomicAdd(&s_cnt[s][p - t.t0], 1u);
        };
        walk_row(r, ops, lane, t_end, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
            if (code == OP_I && len >= 1 && len <= (uint32_t)POLISH_INS_CAP && tp0 > r.ts && tp0 < r.te && tp0 >= t.t0 && tp0 < t_end)
                atomicAdd(&s_cnt[C_INS][tp0 - t.t0], 1u);
            // the columns of this op inside the tile
            uint32_t a = 0, b = 0;
            if (code == OP_EQ || code == OP_X || code == OP_D) {
                a = max(tp0, t.t0);
                b = max(a, min(tp0 + len, t_end));
            }
            const uint32_t n = b - a;
            uint32_t wd = 1u;                                          // a D op's weight: once per op, by its lane
            if constexpr (QW)
                if (code == OP_D && n) wd = del_weight(r, quals, qc0);
            vote_columns<QW>(a, b, code, tp0, qc0, wd, lane, vote);
        });
    }
    __syncthreads();
    for (uint32_t i = (uint32_t)tid; i < t.n_pos; i += POLISH_WG) {
        uint32_t v[5], c = 0, top = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) { v[k] = s_cnt[k][i]; c += v[k]; top = max(top, v[k]); }
        if constexpr (QW) c = s_cnt[C_VOTES][i];                       // the coverage test stays a count; v[] and top are weight sums
        const size_t g = (size_t)t.cbase + t.t0 + i;
        uint8_t d = SYM_KEEP;
        if (c >= (uint32_t)min_cov) {
            const uint8_t own = contig[g] & 0xdfu;
            const int ko = own == 'A' ? 0 : own == 'C' ? 1 : own == 'G' ? 2 : own == 'T' ? 3 : -1;
            if (ko >= 0 && v[ko] == top) d = (uint8_t)ko;
            else d = v[0] == top ? 0 : v[1] == top ? 1 : v[2] == top ? 2 : v[3] == top ? 3 : SYM_DEL;
        }
        sym[g] = d;
        // rows that cover the position, less the ones that start on it, span the slot in front of it
        const uint32_t span = c + s_cnt[C_OTHER][i] - s_cnt[C_START][i], ins = s_cnt[C_INS][i];
        open[g] = span >= (uint32_t)min_cov && 2ull * ins > span;
    }
}

__global__ void slot_index_kernel(const uint32_t *__restrict__ open_pos, uint32_t n_open, uint32_t *__restrict__ slot_of) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_open) slot_of[open_pos[s]] = s;
}

// MODE 0: the length every inserting row votes for at its opened slots; MODE 1: its bases, where its length won
// QW: the length vote weighs the lowest weight among the row's inserted bases, a base vote the base's own
template <int MODE, int ENC, bool QW>
__global__ __launch_bounds__(POLISH_WG) void polish_slot_kernel(const PolRow *__restrict__ rows, uint32_t n_rows,
                                                                const uint32_t *__restrict__ ops, const uint8_t *__restrict__ reads,
                                                                const uint32_t *__restrict__ slot_of, const uint8_t *__restrict__ win_len,
                                                                uint32_t *__restrict__ len_cnt, uint32_t *__restrict__ base_cnt,
                                                                const uint8_t *__restrict__ quals) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * POLISH_WAVES + (threadIdx.x >> 6);
    if (w >= n_rows) return;
    const PolRow r = rows[w];
    walk_row(r, ops, lane, 0xffffffffu, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
        if (code != OP_I || len < 1 || len > (uint32_t)POLISH_INS_CAP || tp0 <= r.ts || tp0 >= r.te) return;
        const uint32_t s = slot_of[(size_t)r.cbase + tp0];
        if (s == NO_SLOT) return;
        if (MODE == 0) {
            uint32_t w = 1u;
            if constexpr (QW) {
                w = 0xffffffffu;
                for (uint32_t j = 0; j < (uint32_t)POLISH_INS_CAP; ++j)
                    if (j < len) w = min(w, column_weight(r, quals, qc0 + j));
            }
            atomicAdd(&len_cnt[(size_t)s * POLISH_INS_CAP + len - 1], w);
        } else if (win_len[s] == len)
            for (uint32_t j = 0; j < len; ++j) {
                const uint32_t k = column_symbol<ENC>(r, reads, qc0 + j);
                if (k < 4) atomicAdd(&base_cnt[((size_t)s * POLISH_INS_CAP + j) * 4 + k], QW ? column_weight(r, quals, qc0 + j) : 1u);
            }
    });
}

__global__ void slot_len_kernel(const uint32_t *__restrict__ len_cnt, uint32_t n_open, uint8_t *__restrict__ win_len) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_open) return;
    uint32_t best = 0, n = 0;
    for (int l = 0; l < POLISH_INS_CAP; ++l) {
        const uint32_t c = len_cnt[(size_t)s * POLISH_INS_CAP + l];
        if (c > best) { best = c; n = (uint32_t)l + 1; }               // (a tie keeps the smaller length)
    }
    win_len[s] = (uint8_t)n;
}

// bytes position g adds to its contig: the slot in front of it, then itself; entry n (behind the last position): 0
__global__ void out_len_kernel(const uint8_t *__restrict__ sym, const uint32_t *__restrict__ slot_of, const uint8_t *__restrict__ win_len,
                               size_t n, uint32_t *__restrict__ out_len) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g > n) return;
    uint32_t l = 0;
    if (g < n) {
        l = sym[g] != SYM_DEL;
        const uint32_t s = slot_of[g];
        if (s != NO_SLOT) l += win_len[s];
    }
    out_len[g] = l;
}

__global__ void write_kernel(const uint8_t *__restrict__ sym, const uint32_t *__restrict__ slot_of, const uint8_t *__restrict__ win_len,
                             const uint32_t *__restrict__ base_cnt, const uint8_t *__restrict__ contig, const uint64_t *__restrict__ off,
                             size_t n, uint8_t *__restrict__ out) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= n) return;
    uint64_t o = off[g];
    const uint32_t s = slot_of[g];
    if (s != NO_SLOT) {
        const uint32_t len = min((uint32_t)win_len[s], (uint32_t)POLISH_INS_CAP);
        for (uint32_t j = 0; j < len; ++j) {
            const uint32_t *c = base_cnt + ((size_t)s * POLISH_INS_CAP + j) * 4;
            uint32_t best = 0;
            uint8_t b = 'N';
            for (int k = 0; k < 4; ++k)
                if (c[k] > best) { best = c[k]; b = (uint8_t)"ACGT"[k]; }
            out[o++] = b;
        }
    }
    const uint8_t d = sym[g];
    if (d != SYM_DEL) out[o] = d == SYM_KEEP ? contig[g] : (uint8_t)"ACGT"[d];
}

__global__ void gather_off_kernel(const uint64_t *__restrict__ off, const uint32_t *__restrict__ at, uint32_t n, uint64_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = off[at[i]];
}

template <int ENC, bool QW>
void launch_count(const PolCoreIn &in, uint8_t *d_sym, uint8_t *d_open) {
    hipLaunchKernelGGL((polish_count_kernel<ENC, QW>), dim3((unsigned)in.n_tiles), dim3(POLISH_WG), 0, stream(), in.rows, in.ops, in.reads,
                       in.contig, in.tiles, in.min_cov, d_sym, d_open, in.quals);
}
template <int MODE, int ENC, bool QW>
void launch_slot(const PolCoreIn &in, const uint32_t *d_slot_of, const uint8_t *d_win_len, uint32_t *d_len_cnt, uint32_t *d_base_cnt) {
    hipLaunchKernelGGL((polish_slot_kernel<MODE, ENC, QW>), dim3(cdiv(in.n_rows, POLISH_WAVES)), dim3(POLISH_WG), 0, stream(), in.rows,
                       in.n_rows, in.ops, in.reads, d_slot_of, d_win_len, d_len_cnt, d_base_cnt, in.quals);
}
// the instantiation of the call: the reads' encoding, weighted or not
template <int MODE>
void launch_slot_for(const PolCoreIn &in, const uint32_t *d_slot_of, const uint8_t *d_win_len, uint32_t *d_len_cnt, uint32_t *d_base_cnt) {
    const bool codes = in.enc == READS_CODES;
    if (in.quals) {
        if (codes) launch_slot<MODE, READS_CODES, true>(in, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
        else launch_slot<MODE, READS_ASCII, true>(in, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
    } else {
        if (codes) launch_slot<MODE, READS_CODES, false>(in, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
        else launch_slot<MODE, READS_ASCII, false>(in, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
    }
}

// the slots at pos[0, n) get their index in slot_of; length votes, the winning lengths, base votes (counters zeroed by the caller)
void slot_passes(const PolSlotVotes &votes, const uint32_t *d_pos, size_t n, uint32_t *d_slot_of, uint8_t *d_win_len, uint32_t *d_len_cnt,
                 uint32_t *d_base_cnt) {
    constexpr int B = 256;
    hipLaunchKernelGGL(slot_index_kernel, dim3(cdiv(n, B)), dim3(B), 0, stream(), d_pos, (uint32_t)n, d_slot_of);
    votes(0, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
    hipLaunchKernelGGL(slot_len_kernel, dim3(cdiv(n, B)), dim3(B), 0, stream(), d_len_cnt, (uint32_t)n, d_win_len);
    votes(1, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
    HIP_CHECK(hipGetLastError());
}

// polish_core's votes: polish_slot_kernel over every row of `in`
PolSlotVotes row_votes_of(const PolCoreIn &in) {
    return [&in](int mode, const uint32_t *d_slot_of, const uint8_t *d_win_len, uint32_t *d_len_cnt, uint32_t *d_base_cnt) {
        if (mode == 0) launch_slot_for<0>(in, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
        else launch_slot_for<1>(in, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
    };
}

}  // namespace

void polish_slot_votes(const PolCoreIn &in, const uint32_t *d_pos, size_t n, uint32_t *d_slot_of, uint8_t *d_win_len, uint32_t *d_len_cnt,
                       uint32_t *d_base_cnt) {
    if (n) slot_passes(row_votes_of(in), d_pos, n, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
}

void polish_upload(const PolDevIn &in, PolUploaded &up) {
    up.contig.upload((const uint8_t *)in.contigs.data(), in.contigs.size());
    up.reads.upload((const uint8_t *)in.reads.data(), in.reads.size());
    const bool weighted = !in.quals.empty();                 // (as long as `reads`: polish_host.cpp appends both)
    if (weighted && in.quals.size() != in.reads.size()) fail(HLMI_EINVAL, "hlmi_polish_q: quality bytes and read bytes differ in number");
    if (weighted) up.quals.upload((const uint8_t *)in.quals.data(), in.quals.size());
    up.rows.upload(in.rows);
    up.ops.upload(in.ops);
    up.tiles.upload(in.tiles);
    up.cbase.upload(in.cbase);
    PolCoreIn &c = up.core;
    c.rows = up.rows.p; c.n_rows = (uint32_t)in.rows.size();
    c.ops = up.ops.p;
    c.reads = up.reads.p; c.enc = READS_ASCII;
    c.quals = weighted ? up.quals.p : nullptr;
    c.contig = up.contig.p; c.n_contig = in.contigs.size();
    c.tiles = up.tiles.p; c.n_tiles = in.tiles.size();
    c.cbase = up.cbase.p; c.n_cbase = in.cbase.size();
    c.min_cov = in.min_cov;
}

void polish_core(const PolCoreIn &in, PolDevOut &out) {
    const size_t G = in.n_contig;
    const bool codes = in.enc == READS_CODES;
    out = PolDevOut{};
    out.start.assign(in.n_cbase, 0);
    if (!G) return;
    DBuf<uint8_t> d_sym(G), d_open(G);
    HIP_CHECK(hipMemsetAsync(d_sym.p, SYM_KEEP, G, stream()));
    d_open.zero();
    if (in.n_tiles) {
        KTimer kt("polish_count");
        if (in.quals) {
            if (codes) launch_count<READS_CODES, true>(in, d_sym.p, d_open.p);
            else launch_count<READS_ASCII, true>(in, d_sym.p, d_open.p);
        } else {
            if (codes) launch_count<READS_CODES, false>(in, d_sym.p, d_open.p);
            else launch_count<READS_ASCII, false>(in, d_sym.p, d_open.p);
        }
        HIP_CHECK(hipGetLastError());
    }
    polish_tail(PolTailIn{in.contig, G, &d_sym, &d_open, in.cbase, in.n_cbase, "polish_slots"}, row_votes_of(in), out);
}

void polish_tail(const PolTailIn &in, const PolSlotVotes &votes, PolDevOut &out) {
    const size_t G = in.n;
    constexpr int B = 256;
    const DBuf<uint8_t> &d_sym = *in.sym, &d_open = *in.open;
    DBuf<uint32_t> d_open_pos(G), d_slot_of(G);
    const size_t n_open = select_flagged_indices(d_open.p, d_open_pos.p, G);
    d_slot_of.fill_ff();
    DBuf<uint32_t> d_len_cnt(std::max<size_t>(n_open, 1) * POLISH_INS_CAP), d_base_cnt(std::max<size_t>(n_open, 1) * POLISH_INS_CAP * 4);
    DBuf<uint8_t> d_win_len(std::max<size_t>(n_open, 1));
    if (n_open) {
        KTimer kt(in.slots_timer);
        d_len_cnt.zero();
        d_base_cnt.zero();
        slot_passes(votes, d_open_pos.p, n_open, d_slot_of.p, d_win_len.p, d_len_cnt.p, d_base_cnt.p);
    }
    DBuf<uint32_t> d_out_len(G + 1);
    DBuf<uint64_t> d_off(G + 1), d_start(in.n_cbase);
    hipLaunchKernelGGL(out_len_kernel, dim3(cdiv(G + 1, B)), dim3(B), 0, stream(), d_sym.p, d_slot_of.p, d_win_len.p, G, d_out_len.p);
    exclusive_scan_u32_to_u64(d_out_len.p, d_off.p, G + 1);
    const uint64_t total = download_one(d_off.p + G);
    DBuf<uint8_t> d_out(std::max<uint64_t>(total, 1));
    {
        KTimer kt("polish_write");
        hipLaunchKernelGGL(write_kernel, dim3(cdiv(G, B)), dim3(B), 0, stream(), d_sym.p, d_slot_of.p, d_win_len.p, d_base_cnt.p,
                           in.contig, d_off.p, G, d_out.p);
        hipLaunchKernelGGL(gather_off_kernel, dim3(cdiv(in.n_cbase, B)), dim3(B), 0, stream(), d_off.p, in.cbase,
                           (uint32_t)in.n_cbase, d_start.p);
        HIP_CHECK(hipGetLastError());
    }
    out.start = d_start.download();
    const std::vector<uint8_t> bytes = d_out.download((size_t)total);
    out.bases.assign((const char *)bytes.data(), bytes.size());
    out.sym = d_sym.download(G);
    out.open_pos = d_open_pos.download(n_open);
    out.open_len = d_win_len.download(n_open);
}

}  // namespace pol
}  // namespace hlmi
