// polish_walk.h - the device code the tile kernels over the selected rows share: polish_count_kernel (polish.hip) and
// var_tile_kernel (variants.hip) walk the same compact CIGARs over the same tiles and vote the same columns, depth_tile_kernel
// (depth.hip) finds a tile's contig the same way.  One definition of a column's symbol, of the walk, of the lane / wave switch
// of the vote loop and of the slot search; what a vote adds to, and what a tile decides from its counters, is each kernel's own.
// Every loop is bounded by a count known at its head.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "paf_io.h"
#include "polish_internal.h"
#include "wave_ops.h"

namespace hlmi {
namespace pol {

constexpr int POLISH_WG = 256, POLISH_WAVES = POLISH_WG / 64;
constexpr int C_OTHER = 5;                 // a column that votes nothing: behind the five symbols A C G T del
constexpr uint32_t SHORT_RUN = 16;         // a lane votes a run of up to this many columns itself; longer ones take the wave

// symbol of alignment column `col` of row r: 0..3, or C_OTHER for anything that is not A C G T.
// ENC = READS_ASCII: `reads` holds the file's bytes, folded to upper case here.  ENC = READS_CODES: it holds the overlapper's
// resident codes (DevReads::codes(): 0..3 = A C G T of either case, 4 = anything else).  Code 4 is exactly the set of bytes the
// ASCII form refuses to count after `& 0xdf` - with one exception the encoder makes for the aligner, U / u -> 3: the caller
// (polish_rows.hip) sets those bases to 4 once the alignment is done, so that both forms count the same columns.
template <int ENC>
__device__ __forceinline__ uint32_t column_symbol(const PolRow &r, const uint8_t *__restrict__ reads, uint32_t col) {
    if (col >= r.qn) return C_OTHER;                                   // (validated on the host: never)
    uint8_t c = reads[r.read_off + (r.rev ? r.qn - 1 - col : col)];
    uint32_t k;
    if (ENC == READS_CODES) k = c < 4 ? (uint32_t)c : (uint32_t)C_OTHER;
    else {
        c &= 0xdfu;                                                    // upper case
        k = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : (uint32_t)C_OTHER;
    }
    return r.rev && k < 4 ? 3u - k : k;
}

// One wave walks the CIGAR of r: f(code, len, first target position, first query column) for every op, lane = op; stops
// in front of the first 64 ops that start at t_stop or behind it.  All 64 lanes call f together.
template <typename F>
__device__ __forceinline__ void walk_row(const PolRow &r, const uint32_t *__restrict__ ops, int lane, uint32_t t_stop, F &&f) {
    uint32_t tb = r.ts, qb = 0;
    const uint32_t *o = ops + r.cig_off;
    for (uint32_t k0 = 0; k0 < r.cig_n && tb < t_stop; k0 += 64) {
        const uint32_t idx = k0 + (uint32_t)lane;
        const uint32_t op = idx < r.cig_n ? o[idx] : 0u;
        const uint32_t len = op >> 4, code = op & 15u;
        const uint32_t tl = code == OP_I ? 0u : len, ql = code == OP_D ? 0u : len;
        const uint32_t te = wave_prefix_sum_incl_dpp(tl), qe = wave_prefix_sum_incl_dpp(ql);
        f(code, len, tb + te - tl, qb + qe - ql);
        tb += (uint32_t)__builtin_amdgcn_readlane((int)te, 63);
        qb += (uint32_t)__builtin_amdgcn_readlane((int)qe, 63);
    }
}

// The columns [a, b) of this lane's op (code, first target position tp0, first query column qc0; a == b: none) go to
// vote(p, code, tp0, qc0, wd): a run of up to SHORT_RUN columns by the lane itself, the longer ones of the wave one after the
// other, 64 columns a step.  All 64 lanes call together.  WD: the op carries a weight wd of its own (the QW kernels' D ops).
template <bool WD, typename V>
__device__ __forceinline__ void vote_columns(uint32_t a, uint32_t b, uint32_t code, uint32_t tp0, uint32_t qc0, uint32_t wd, int lane,
                                             V &&vote) {
    const uint32_t n = b - a;
    if (n <= SHORT_RUN)
        for (uint32_t p = a; p < b; ++p) vote(p, code, tp0, qc0, wd);
    unsigned long long longs = __ballot(n > SHORT_RUN);
    for (int it = 0; it < 64 && longs; ++it) {                 // the long runs, one after the other, 64 columns a step
        const int src = __ffsll(longs) - 1;
        longs &= longs - 1;
        const uint32_t a2 = (uint32_t)__shfl((int)a, src), b2 = (uint32_t)__shfl((int)b, src);
        const uint32_t code2 = (uint32_t)__shfl((int)code, src), tp2 = (uint32_t)__shfl((int)tp0, src),
                       qc2 = (uint32_t)__shfl((int)qc0, src);
        uint32_t wd2 = 1u;
        if constexpr (WD) wd2 = (uint32_t)__shfl((int)wd, src);
        for (uint32_t p = a2 + (uint32_t)lane; p < b2; p += 64) vote(p, code2, tp2, qc2, wd2);
    }
}

// the slot whose positions hold p: the last j < n_slots with cbase[j] <= p (cbase ascends strictly: a slot has a position)
__device__ __forceinline__ uint32_t slot_of_position(const uint32_t *__restrict__ cbase, uint32_t n_slots, uint32_t p) {
    uint32_t lo = 0, hi = n_slots;              // the answer lies in [lo, hi)
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cbase[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace pol
}  // namespace hlmi
