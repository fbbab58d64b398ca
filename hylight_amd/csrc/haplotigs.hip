// haplotigs.hip - the device part of hlmi_haplotigs / hlmi_haplotigs_reads (include/hylight_mi.h) behind the phasing: polish each
// side of a split block on its own.  A row is shut out of one side inside the extent of every split block in which it reads the
// other side; everywhere else it votes on both.  The rows are the polisher's (PolRow, compact CIGARs, reads as ASCII or codes), the
// records per (row, block) phase_core's, left in device memory (ph::DevRecs) - nothing per row goes up or comes down.
//   hap_iv_count_kernel   a thread per row: its records of split blocks with a side; the library's scan gives the rows' offsets
//   hap_iv_fill_kernel    the same loop once more: one interval (first | shut side << 31, last) per such record, in the device's
//                         position space.  A row's blocks ascend, so its intervals ascend and never overlap: a CSR without an atomic
//   hap_count_kernel      the two-sided count pass, the shape of polish_count_kernel: a workgroup per tile of HAP_TILE positions
//                         with 2 x 8 counters per position in LDS (64 KiB), a wave per row, walk_row / vote_columns /
//                         column_symbol.  A row's CIGAR is walked once and its bases are fetched once; the wave first copies the
//                         row's intervals that touch the tile into its own LDS list (22 bits each, clipped to the tile: at most
//                         HAP_TILE / 2 + 1 of them, since an extent holds two positions and extents do not overlap), and every
//                         column, the row-start mark and the insertion mark look their position up there - a counted binary search
//                         - to find which side's counters take the add.  The flush decides both sides' positions and slot flags;
//                         no counter reaches global memory
//   hap_slot_kernel       the sided slot passes: polish_slot_kernel over the slot space (side, position) - the same walk, the
//                         insertion's position looked up in the row's interval list in global memory
// The rest is polish.hip's polish_tail over both sides side by side.  Every loop is bounded by a count known at its head; the
// searches are counted.
//
// The key-space form (KEYS, hlmi_haplotigs_ins: blocks of hlmi_phase_ins, whose first or last site may be a slot).  An extent is
// [kf, kl] in ph::site_key's space - slot g has key 2 g, position g key 2 g + 1 - and holds every key in between: position g is
// inside iff kf <= 2 g + 1 <= kl, slot g iff kf <= 2 g <= kl.  With both ends odd that is the rule above.  The interval is
// KeyInterval, 12 bytes (two 32-bit keys and the shut side are 65 bits: the record grows, no call refuses more than before).
//   LDS entry   klo | khi << 11 | shut << 22: the extent clipped to the tile's 2 HAP_TILE keys, as offsets from key 2 g0.  That is the
//               position form's lo and hi with one more bit each, the keys' low bits: klo even - the slot in front of the first
//               inside position is inside; khi even - the slot behind the last inside position is inside while that position is
//               not.  key_sides finds both answers a column needs, its position's and its slot's, with one counted search.
//   the bound   An extent holds a position and one more site, so two keys at the least, and extents do not overlap.  One that
//               touches the tile has a key in it; all but two - the one across the tile's lower border and the one across its
//               upper - lie inside with both.  2 (n - 2) + 2 <= 2 HAP_TILE: n <= HAP_TILE + 1 = IV_CAP_KEYS (reached by an
//               extent that ends at the slot of offset 0 - it touches the tile by that slot alone - and HAP_TILE extents of a
//               position with the slot behind it).  One word per extent: 4 x 1025 x 4 = 16 400 bytes next to the 64 KiB of
//               counters, 81 936 bytes, 16 more than half a CU's LDS: a workgroup per CU for this form, where the position form
//               has two.  The choice is the plain list over a packed entry or a smaller tile; it is untimed beyond DESIGN 7
//   the span    The flush takes a slot's span from the counters of the position behind it: c + C_OTHER - C_START.  A row has
//               one column at position x.  Per side S it takes part in position x (P) or not, and in slot x (L) or not, and the
//               column adds: P and L - its vote, counted in c; L alone (the extent starts at position x) - C_OTHER; P alone (the
//               extent ended at slot x: the row votes at x and must not span the slot) - C_START, which the flush subtracts;
//               neither - nothing.  The two corrections are made only behind the row's first column; on its first column a row
//               spans no slot and lane 0 adds the C_START that takes its vote out, on the sides of P.  So a row moves a slot's
//               span on a side by one or by nothing, and the cases exclude each other: at most once per slot and side.
//               An extent that starts at slot x has klo even: the slot's lookup needs no exception for the first offset
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "dev_prims.h"
#include "haplotigs_internal.h"
#include "polish_walk.h"
#include "wave_ops.h"

namespace hlmi {
namespace hap {

using namespace pol;
using ph::ReadRec;

namespace {

constexpr int WG = 256;
constexpr unsigned MAX_GRID = 1u << 16;         // blocks of a strided launch
inline dim3 grid1(size_t n) { return dim3((unsigned)std::min<size_t>(cdiv(n ? n : 1, WG), MAX_GRID)); }

constexpr int C_START = 6, C_INS = 7, HAP_CNT = 8;                     // counters behind the five symbols and C_OTHER, per side
constexpr int IV_CAP = HAP_TILE / 2 + 2;                               // intervals of one row that touch one tile, and one to spare
constexpr uint32_t IV_NONE = 0xffffffffu, POS_MASK = 0x7fffffffu;
static_assert(HAP_TILE == POLISH_TILE, "the count pass runs over polish_layout's tiles");
static_assert(HAP_TILE <= 1024, "a tile offset has 10 bits in an LDS interval");
static_assert(sizeof(ReadRec) == 24, "24 bytes per record");
constexpr int IV_CAP_KEYS = HAP_TILE + 1;                              // ... in key space (the head comment's bound)
constexpr uint32_t KEY_MASK = 2047u;
static_assert(2 * HAP_TILE <= 2048, "a tile's key offset has 11 bits in an LDS interval");
static_assert(2 * (IV_CAP_KEYS - 2) + 2 >= 2 * HAP_TILE, "the list holds every n with 2 (n - 2) + 2 <= 2 HAP_TILE");
static_assert(IV_CAP_KEYS <= 2048, "key_sides's 12 steps");

// A row's exclusion interval in the device's position space (positions < 2^31): the row takes no part in side `shut` at the
// positions of [first, last] and at the slots of (first, last]
struct Interval {
    uint32_t first_shut;                // first | shut << 31
    uint32_t last;
};
// ... in key space (keys < 2^32): no part in side `shut` at every position and slot whose key lies in [kf, kl]
struct KeyInterval {
    uint32_t kf, kl, shut;
};
template <bool KEYS>
using IvOf = std::conditional_t<KEYS, KeyInterval, Interval>;

// the side a record shuts its row out of inside a split block: the other one than its own; 2: none (no side, or not split)
__device__ __forceinline__ uint32_t shut_side(const ReadRec &r, const uint8_t *__restrict__ split, uint32_t n_blocks) {
    if (r.block >= n_blocks || !split[r.block] || r.a == r.b) return 2u;
    return r.a > r.b ? 1u : 0u;
}

__global__ __launch_bounds__(WG) void hap_iv_count_kernel(uint32_t n_rows, const uint64_t *__restrict__ rec_off, const uint32_t *__restrict__ rec_cnt,
                                                          const ReadRec *__restrict__ recs, uint64_t n_recs, const uint8_t *__restrict__ split,
                                                          uint32_t n_blocks, uint32_t *__restrict__ cnt) {
    const uint32_t step = gridDim.x * WG;
    for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < n_rows; k += step) {
        const uint32_t n = rec_cnt[k];
        const uint64_t off = rec_off[k];
        uint32_t c = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (off + i < n_recs) c += shut_side(recs[off + i], split, n_blocks) < 2u;
        cnt[k] = c;
    }
}

// KEYS: gfirst and glast hold the blocks' kf and kl
template <bool KEYS>
__global__ __launch_bounds__(WG) void hap_iv_fill_kernel(uint32_t n_rows, const uint64_t *__restrict__ rec_off, const uint32_t *__restrict__ rec_cnt,
                                                         const ReadRec *__restrict__ recs, uint64_t n_recs, const uint8_t *__restrict__ split,
                                                         const uint32_t *__restrict__ gfirst, const uint32_t *__restrict__ glast, uint32_t n_blocks,
                                                         const uint64_t *__restrict__ iv_off, const uint32_t *__restrict__ iv_cnt,
                                                         IvOf<KEYS> *__restrict__ iv) {
    const uint32_t step = gridDim.x * WG;
    for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < n_rows; k += step) {
        const uint32_t n = rec_cnt[k], room = iv_cnt[k];
        const uint64_t off = rec_off[k];
        IvOf<KEYS> *out = iv + iv_off[k];
        uint32_t c = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (off + i >= n_recs) continue;
            const ReadRec r = recs[off + i];
            const uint32_t s = shut_side(r, split, n_blocks);
            if constexpr (KEYS) {
                if (s < 2u && c < room) out[c++] = KeyInterval{gfirst[r.block], glast[r.block], s};
            } else {
                if (s < 2u && c < room) out[c++] = Interval{(gfirst[r.block] & POS_MASK) | s << 31, glast[r.block]};
            }
        }
    }
}

// the first index of a[0, n) whose `last` is not below g (n: none); n < 2^32: 32 steps at the most
__device__ __forceinline__ uint32_t first_ending_at_or_behind(const Interval *__restrict__ a, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (a[m].last < g) lo = m + 1;
        else hi = m;
    }
    return lo;
}
// ... whose kl is not below key k
__device__ __forceinline__ uint32_t first_ending_at_or_behind(const KeyInterval *__restrict__ a, uint32_t n, uint32_t k) {
    uint32_t lo = 0, hi = n;
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (a[m].kl < k) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// An interval clipped to a tile, as the count pass keeps it in LDS: lo | hi << 10 | shut << 20 | open_left << 21 - tile offsets of
// its first and last position inside the tile, and whether it began in front of the tile.  The entry of s[0, n) (ascending) whose
// [lo, hi] holds x, or IV_NONE; n <= IV_CAP: 11 steps at the most
__device__ __forceinline__ uint32_t tile_interval_at(const uint32_t *s, uint32_t n, uint32_t x) {
    if (!n) return IV_NONE;
    uint32_t lo = 0, hi = n;                    // the last entry whose lo is not behind x lies in [lo, hi)
    for (int it = 0; it < 11 && hi - lo > 1; ++it) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if ((s[m] & 1023u) <= x) lo = m;
        else hi = m;
    }
    const uint32_t e = s[lo];
    return (e & 1023u) <= x && x <= (e >> 10 & 1023u) ? e : IV_NONE;
}
// bit S: the row takes part in side S at the position the entry was found for
__device__ __forceinline__ uint32_t position_sides(uint32_t e) { return e == IV_NONE ? 3u : 3u & ~(1u << (e >> 20 & 1u)); }
// ... at the slot in front of tile offset x: the slot in front of an extent's first position lies outside it
__device__ __forceinline__ uint32_t slot_sides(uint32_t e, uint32_t x) {
    if (e == IV_NONE || (x == (e & 1023u) && !(e >> 21 & 1u))) return 3u;
    return position_sides(e);
}

// The key-space entries (the head comment: klo | khi << 11 | shut << 22) of s[0, n), ascending: bits 0 and 1 - the row takes part in
// side A, B at the position of tile offset x; bits 2 and 3 - at the slot in front of it.  One search for the last entry that
// begins at or in front of the position's key; the slot's key, one below, lies in that entry, in the one in front of it when the
// entry begins at the position itself, or in none.  n <= IV_CAP_KEYS <= 2048: 12 steps at the most
__device__ __forceinline__ uint32_t key_sides(const uint32_t *s, uint32_t n, uint32_t x) {
    if (!n) return 15u;
    const uint32_t ks = 2u * x, kp = ks + 1u;
    uint32_t lo = 0, hi = n;                    // the last entry whose klo is not behind kp lies in [lo, hi)
    for (int it = 0; it < 12 && hi - lo > 1; ++it) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if ((s[m] & KEY_MASK) <= kp) lo = m;
        else hi = m;
    }
    const uint32_t e = s[lo], klo = e & KEY_MASK, khi = e >> 11 & KEY_MASK, out = 3u & ~(1u << (e >> 22 & 1u));
    const uint32_t mp = klo <= kp && kp <= khi ? out : 3u;
    uint32_t ms = 3u;
    if (klo <= ks) ms = ks <= khi ? out : 3u;
    else if (klo == kp && lo > 0) {             // the entry in front ends below kp: at the slot's key or in front of it
        const uint32_t f = s[lo - 1];
        if ((f >> 11 & KEY_MASK) == ks) ms = 3u & ~(1u << (f >> 22 & 1u));
    }
    return mp | ms << 2;
}

template <int ENC, bool KEYS = false>
__global__ __launch_bounds__(POLISH_WG) void hap_count_kernel(const PolRow *__restrict__ rows, const uint32_t *__restrict__ ops,
                                                              const uint8_t *__restrict__ reads, const uint8_t *__restrict__ contig,
                                                              const PolTile *__restrict__ tiles, int min_cov, const uint64_t *__restrict__ iv_off,
                                                              const uint32_t *__restrict__ iv_cnt, const IvOf<KEYS> *__restrict__ iv, size_t G,
                                                              uint8_t *__restrict__ sym, uint8_t *__restrict__ open) {
    constexpr uint32_t CAP = KEYS ? IV_CAP_KEYS : IV_CAP;
    __shared__ uint32_t s_cnt[2][HAP_CNT][HAP_TILE];
    __shared__ uint32_t s_iv[POLISH_WAVES][CAP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PolTile t = tiles[blockIdx.x];
    const uint32_t t_end = t.t0 + t.n_pos;
    const uint32_t g0 = t.cbase + t.t0, g1 = t.cbase + t_end;          // the tile in the device's position space
    for (int i = tid; i < 2 * HAP_CNT * HAP_TILE; i += POLISH_WG) (&s_cnt[0][0][0])[i] = 0;
    __syncthreads();
    uint32_t *siv = s_iv[wave];
    for (uint32_t k = t.row_lo + (uint32_t)wave; k < t.row_hi; k += POLISH_WAVES) {
        const PolRow r = rows[k];
        if (r.te <= t.t0 || r.ts >= t_end) continue;
        // the row's intervals that touch the tile, into the wave's list: they ascend, so they are one run of the row's list
        const uint32_t n_iv = iv_cnt[k];
        uint32_t n_t = 0;
        if (n_iv) {
            const IvOf<KEYS> *ri = iv + iv_off[k];
            const uint32_t lo = first_ending_at_or_behind(ri, n_iv, KEYS ? 2u * g0 : g0);
            for (uint32_t c = 0; c < CAP; c += 64) {
                const uint32_t j = c + (uint32_t)lane;
                bool ok = j < CAP && lo + j < n_iv;
                IvOf<KEYS> v{};
                if (ok) v = ri[lo + j];
                if constexpr (KEYS) {
                    const uint32_t k0 = 2u * g0, k1 = 2u * g1 - 1u;    // the tile's first and last key (g1 < 2^31)
                    ok = ok && v.kf <= k1 && v.kl >= k0;
                    if (ok) siv[j] = (v.kf > k0 ? v.kf - k0 : 0u) | (min(v.kl, k1) - k0) << 11 | (v.shut & 1u) << 22;
                } else {
                    const uint32_t first = v.first_shut & POS_MASK;
                    ok = ok && first < g1 && v.last >= g0;
                    if (ok)
                        siv[j] = (first > g0 ? first - g0 : 0u) | (min(v.last, g1 - 1) - g0) << 10 | (v.first_shut >> 31) << 20 |
                                 (uint32_t)(first < g0) << 21;
                }
                const uint32_t n_ok = (uint32_t)__popcll(__ballot(ok));
                n_t += n_ok;
                if (n_ok < 64u) break;                                 // (the same in every lane)
            }
            __builtin_amdgcn_s_waitcnt(0);                             // the list is read back by this wave's other lanes below
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0 && r.ts >= t.t0) {
            const uint32_t x = r.ts - t.t0, m = KEYS ? key_sides(siv, n_t, x) & 3u : position_sides(tile_interval_at(siv, n_t, x));
            if (m & 1u) atomicAdd(&s_cnt[0][C_START][x], 1u);
            if (m & 2u) atomicAdd(&s_cnt[1][C_START][x], 1u);
        }
        auto vote = [&](uint32_t p, uint32_t code, uint32_t tp0, uint32_t qc0, uint32_t) {
            const uint32_t x = p - t.t0;
            const uint32_t s = code == OP_D ? (uint32_t)SYM_DEL : column_symbol<ENC>(r, reads, qc0 + (p - tp0));
            if constexpr (KEYS) {
                const uint32_t both = key_sides(siv, n_t, x), m = both & 3u, ms = both >> 2;
                if (m & 1u) atomicAdd(&s_cnt[0][s][x], 1u);
                if (m & 2u) atomicAdd(&s_cnt[1][s][x], 1u);
                // behind the row's first column (the head comment's span): in the slot alone - a column that votes nothing; at
                // the position alone - the vote above is taken out of the slot's span
                if (m != ms && p > r.ts) {
                    const uint32_t only_slot = ms & ~m, only_pos = m & ~ms;
                    if (only_slot & 1u) atomicAdd(&s_cnt[0][C_OTHER][x], 1u);
                    if (only_slot & 2u) atomicAdd(&s_cnt[1][C_OTHER][x], 1u);
                    if (only_pos & 1u) atomicAdd(&s_cnt[0][C_START][x], 1u);
                    if (only_pos & 2u) atomicAdd(&s_cnt[1][C_START][x], 1u);
                }
            } else {
                const uint32_t e = tile_interval_at(siv, n_t, x), m = position_sides(e);
                if (m & 1u) atomicAdd(&s_cnt[0][s][x], 1u);
                if (m & 2u) atomicAdd(&s_cnt[1][s][x], 1u);
                // shut out of the position and still spanning the slot in front of it (the extent's first position): the span
                // below counts the row as it counts a column that votes nothing
                const uint32_t only_slot = slot_sides(e, x) & ~m;
                if (only_slot && p > r.ts) {
                    if (only_slot & 1u) atomicAdd(&s_cnt[0][C_OTHER][x], 1u);
                    if (only_slot & 2u) atomicAdd(&s_cnt[1][C_OTHER][x], 1u);
                }
            }
        };
        walk_row(r, ops, lane, t_end, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
            if (code == OP_I && len >= 1 && len <= (uint32_t)POLISH_INS_CAP && tp0 > r.ts && tp0 < r.te && tp0 >= t.t0 && tp0 < t_end) {
                const uint32_t x = tp0 - t.t0, m = KEYS ? key_sides(siv, n_t, x) >> 2 : slot_sides(tile_interval_at(siv, n_t, x), x);
                if (m & 1u) atomicAdd(&s_cnt[0][C_INS][x], 1u);
                if (m & 2u) atomicAdd(&s_cnt[1][C_INS][x], 1u);
            }
            uint32_t a = 0, b = 0;                                     // the columns of this op inside the tile
            if (code == OP_EQ || code == OP_X || code == OP_D) {
                a = max(tp0, t.t0);
                b = max(a, min(tp0 + len, t_end));
            }
            vote_columns<false>(a, b, code, tp0, qc0, 1u, lane, vote);
        });
        __builtin_amdgcn_wave_barrier();                               // the next row's list is written behind this row's reads
    }
    __syncthreads();
    for (uint32_t i = (uint32_t)tid; i < 2u * t.n_pos; i += POLISH_WG) {
        const uint32_t side = i >= t.n_pos ? 1u : 0u, x = i - side * t.n_pos;
        uint32_t v[5], c = 0, top = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) { v[k] = s_cnt[side][k][x]; c += v[k]; top = max(top, v[k]); }
        const size_t g = (size_t)t.cbase + t.t0 + x;
        uint8_t d = SYM_KEEP;
        if (c >= (uint32_t)min_cov) {
            const uint8_t own = contig[g] & 0xdfu;
            const int ko = own == 'A' ? 0 : own == 'C' ? 1 : own == 'G' ? 2 : own == 'T' ? 3 : -1;
            if (ko >= 0 && v[ko] == top) d = (uint8_t)ko;
            else d = v[0] == top ? 0 : v[1] == top ? 1 : v[2] == top ? 2 : v[3] == top ? 3 : SYM_DEL;
        }
        sym[side * G + g] = d;
        // rows that take part in the slot in front of the position and do not start on it span it
        const uint32_t span = c + s_cnt[side][C_OTHER][x] - s_cnt[side][C_START][x], ins = s_cnt[side][C_INS][x];
        open[side * G + g] = span >= (uint32_t)min_cov && 2ull * ins > span;
    }
}

// MODE 0: the length every inserting row votes for at its opened slots of the sides it takes part in; MODE 1: its bases, where
// its length won.  slot_of, and the counters behind it, run over (side, position): side B's positions lie G behind side A's
template <int MODE, int ENC, bool KEYS = false>
__global__ __launch_bounds__(POLISH_WG) void hap_slot_kernel(const PolRow *__restrict__ rows, uint32_t n_rows, const uint32_t *__restrict__ ops,
                                                             const uint8_t *__restrict__ reads, const uint64_t *__restrict__ iv_off,
                                                             const uint32_t *__restrict__ iv_cnt, const IvOf<KEYS> *__restrict__ iv, size_t G,
                                                             const uint32_t *__restrict__ slot_of, const uint8_t *__restrict__ win_len,
                                                             uint32_t *__restrict__ len_cnt, uint32_t *__restrict__ base_cnt) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * POLISH_WAVES + (threadIdx.x >> 6);
    if (w >= n_rows) return;
    const PolRow r = rows[w];
    const uint32_t n_iv = iv_cnt[w];
    const IvOf<KEYS> *ri = iv + iv_off[w];
    walk_row(r, ops, lane, 0xffffffffu, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
        if (code != OP_I || len < 1 || len > (uint32_t)POLISH_INS_CAP || tp0 <= r.ts || tp0 >= r.te) return;
        const uint32_t g = r.cbase + tp0;
        uint32_t sides = 3u;                    // slot g lies inside an interval iff first < g <= last; KEYS: iff kf <= 2 g <= kl
        if constexpr (KEYS) {
            if (n_iv) {
                const uint32_t j = first_ending_at_or_behind(ri, n_iv, 2u * g);
                if (j < n_iv && ri[j].kf <= 2u * g) sides = 3u & ~(1u << (ri[j].shut & 1u));
            }
        } else if (n_iv) {
            const uint32_t j = first_ending_at_or_behind(ri, n_iv, g);
            if (j < n_iv && (ri[j].first_shut & POS_MASK) < g) sides = 3u & ~(1u << (ri[j].first_shut >> 31));
        }
        for (uint32_t side = 0; side < 2; ++side) {
            if (!(sides >> side & 1u)) continue;
            const uint32_t s = slot_of[side * G + g];
            if (s == POLISH_NO_SLOT) continue;
            if (MODE == 0) atomicAdd(&len_cnt[(size_t)s * POLISH_INS_CAP + len - 1], 1u);
            else if (win_len[s] == len)
                for (uint32_t j = 0; j < len; ++j) {
                    const uint32_t k = column_symbol<ENC>(r, reads, qc0 + j);
                    if (k < 4) atomicAdd(&base_cnt[((size_t)s * POLISH_INS_CAP + j) * 4 + k], 1u);
                }
        }
    });
}

template <bool KEYS>
struct IvTable {
    DBuf<uint64_t> off;
    DBuf<uint32_t> cnt;
    DBuf<IvOf<KEYS>> iv;
};

template <int MODE, bool KEYS>
void launch_slot(const PolCoreIn &in, const IvTable<KEYS> &T, const uint32_t *d_slot_of, const uint8_t *d_win_len, uint32_t *d_len_cnt,
                 uint32_t *d_base_cnt) {
    const dim3 g(cdiv(in.n_rows, POLISH_WAVES));
    if (in.enc == READS_CODES)
        hipLaunchKernelGGL((hap_slot_kernel<MODE, READS_CODES, KEYS>), g, dim3(POLISH_WG), 0, stream(), in.rows, in.n_rows, in.ops, in.reads,
                           T.off.p, T.cnt.p, T.iv.p, in.n_contig, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
    else
        hipLaunchKernelGGL((hap_slot_kernel<MODE, READS_ASCII, KEYS>), g, dim3(POLISH_WG), 0, stream(), in.rows, in.n_rows, in.ops, in.reads,
                           T.off.p, T.cnt.p, T.iv.p, in.n_contig, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
}

// haplotig_core in either form
template <bool KEYS>
void core_in_form(const char *who, const PolCoreIn &in, const std::vector<uint32_t> &cbase, const ph::DevRecs &recs, const HapBlocksUp &blocks,
                  PolDevOut &out) {
    const size_t G = in.n_contig, R = in.n_rows, n_blocks = blocks.split.size();
    out = PolDevOut{};
    if (!G || !R || !in.n_tiles || cbase.empty() || blocks.gfirst.size() != n_blocks || blocks.glast.size() != n_blocks || recs.off.n < R ||
        recs.cnt.n < R)
        fail(HLMI_ESTATE, "%s: a split block without rows, tiles or records", who);                                  // (never)
    if (in.quals) fail(HLMI_ESTATE, "%s: the two-sided count pass takes no weights", who);                          // (never)
    IvTable<KEYS> T;
    {
        KTimer kt("hap_intervals");
        DBuf<uint32_t> d_gfirst, d_glast;
        DBuf<uint8_t> d_split;
        d_gfirst.upload(blocks.gfirst);
        d_glast.upload(blocks.glast);
        d_split.upload(blocks.split);
        T.cnt.alloc(R);
        T.off.alloc(R);
        hipLaunchKernelGGL(hap_iv_count_kernel, grid1(R), dim3(WG), 0, stream(), (uint32_t)R, recs.off.p, recs.cnt.p, recs.recs.p, recs.n,
                           d_split.p, (uint32_t)n_blocks, T.cnt.p);
        HIP_CHECK(hipGetLastError());
        exclusive_scan_u32_to_u64(T.cnt.p, T.off.p, R);
        const uint64_t n_iv = download_one(T.off.p + (R - 1)) + download_one(T.cnt.p + (R - 1));
        if (n_iv > recs.n) fail(HLMI_ESTATE, "%s: more intervals than (row, block) records", who);                   // (never)
        const size_t avail = dev_available_bytes();             // 0: unknown
        if (avail && n_iv * sizeof(IvOf<KEYS>) > avail)
            fail(HLMI_EINVAL, "%s: the rows' interval table of %llu bytes does not fit the device's free memory (%zu)", who,
                 (unsigned long long)(n_iv * sizeof(IvOf<KEYS>)), avail);
        T.iv.alloc(std::max<uint64_t>(n_iv, 1));
        T.iv.zero();
        hipLaunchKernelGGL(hap_iv_fill_kernel<KEYS>, grid1(R), dim3(WG), 0, stream(), (uint32_t)R, recs.off.p, recs.cnt.p, recs.recs.p, recs.n,
                           d_split.p, d_gfirst.p, d_glast.p, (uint32_t)n_blocks, T.off.p, T.cnt.p, T.iv.p);
        HIP_CHECK(hipGetLastError());
    }
    // the two sides side by side: side B's positions lie G behind side A's
    DBuf<uint8_t> d_sym(2 * G), d_open(2 * G), d_contig(2 * G);
    HIP_CHECK(hipMemsetAsync(d_sym.p, SYM_KEEP, 2 * G, stream()));
    d_open.zero();
    {
        KTimer kt("hap_count");
        if (in.enc == READS_CODES)
            hipLaunchKernelGGL((hap_count_kernel<READS_CODES, KEYS>), dim3((unsigned)in.n_tiles), dim3(POLISH_WG), 0, stream(), in.rows, in.ops, in.reads,
                               in.contig, in.tiles, in.min_cov, T.off.p, T.cnt.p, T.iv.p, G, d_sym.p, d_open.p);
        else
            hipLaunchKernelGGL((hap_count_kernel<READS_ASCII, KEYS>), dim3((unsigned)in.n_tiles), dim3(POLISH_WG), 0, stream(), in.rows, in.ops, in.reads,
                               in.contig, in.tiles, in.min_cov, T.off.p, T.cnt.p, T.iv.p, G, d_sym.p, d_open.p);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(d_contig.p, in.contig, G, hipMemcpyDeviceToDevice, stream()));
    HIP_CHECK(hipMemcpyAsync(d_contig.p + G, in.contig, G, hipMemcpyDeviceToDevice, stream()));
    std::vector<uint32_t> cbase2;               // every contig's start on side A, then on side B, then the total
    const size_t n = cbase.size() - 1;
    cbase2.reserve(2 * n + 1);
    for (size_t side = 0; side < 2; ++side)
        for (size_t j = 0; j < n; ++j) cbase2.push_back((uint32_t)(side * G) + cbase[j]);
    cbase2.push_back((uint32_t)(2 * G));
    DBuf<uint32_t> d_cbase2;
    d_cbase2.upload(cbase2);
    polish_tail(PolTailIn{d_contig.p, 2 * G, &d_sym, &d_open, d_cbase2.p, cbase2.size(), "hap_slots"},
                [&](int mode, const uint32_t *d_slot_of, const uint8_t *d_win_len, uint32_t *d_len_cnt, uint32_t *d_base_cnt) {
                    if (mode == 0) launch_slot<0, KEYS>(in, T, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
                    else launch_slot<1, KEYS>(in, T, d_slot_of, d_win_len, d_len_cnt, d_base_cnt);
                },
                out);
}

}  // namespace

void haplotig_core(const char *who, const PolCoreIn &in, const std::vector<uint32_t> &cbase, const ph::DevRecs &recs,
                   const HapBlocksUp &blocks, PolDevOut &out) {
    if (blocks.keys) core_in_form<true>(who, in, cbase, recs, blocks, out);
    else core_in_form<false>(who, in, cbase, recs, blocks, out);
}

}  // namespace hap
}  // namespace hlmi
