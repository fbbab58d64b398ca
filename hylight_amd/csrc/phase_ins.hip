// phase_ins.hip - the front of hlmi_phase_ins / hlmi_phase_reads_ins (include/hylight_mi.h): the allele table of the selected rows
// over the merged list of position sites and insertion sites (phase_ins_text.h: MergedSites).  A site's key is 2 g + 1 for
// position g of the device's position space and 2 g for the slot in front of it (g < 2^31, so the key fits 32 bits); the keys
// ascend strictly, the rows are sorted by (contig, ts), so the sites a row spans - the keys in [2 (cbase + ts) + 1,
// 2 (cbase + te)) - are a range [s_lo, s_hi) of the key array and the table is phase.hip's CSR.  Behind the table everything is
// phase.hip's tail (phase_tail): phase_reach.hip's link pass, build_blocks_reach, phase_slots_kernel, phase_assign_kernel<true>.
//   phase_span_ins_kernel     a thread per row: s_lo and s_hi - s_lo by two bounded binary searches on the keys; a scan gives the
//                             rows' offsets
//   phase_fill_ins_kernel     a wave per row: AL_NONE at the row's position sites, AL_OWN at its insertion sites (a row that spans
//                             a slot and inserts nothing there reads the contig's own allele).  A launch of its own in front of
//                             the allele kernel: no byte's value rests on the order of two lanes' stores
//   phase_allele_ins_kernel   a wave per row, walk_row over its compact CIGAR, lane = op.  = X D: the sites inside the op's target
//                             range by two searches on the keys inside the row's range; the position sites among them get
//                             phase_allele_kernel's byte, the slots are skipped by their key's low bit; an op with more than
//                             SHORT_RUN sites of either kind takes the wave (vote_columns).  An I op inside (ts, te): one search
//                             for the key of its slot; where the slot is a site, AL_ALT if the op's length is the site's called
//                             length, AL_OTHER otherwise.  The compact CIGAR has one I op per slot, so one lane writes the byte
// Table indices: a row's bytes are table[off[k] .. off[k] + cnt[k]), off the exclusive scan of cnt and the table's size their sum.
// Every store goes to out[s - lo] with lo <= s < hi = lo + cnt[k]: the searches run inside [lo, hi) and return hi for "none",
// which every use checks (s < b <= hi in the column loop, s < hi at an I op).  meta[s] and key[s] are read for s < hi <= n_sites.
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

static_assert(var::N_SYM == 5 && var::S_DEL == (int)SYM_DEL, "the five symbols are the polisher's");
static_assert(var::INS_CAP == (uint32_t)POLISH_INS_CAP, "a called length fits the meta byte");

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

__global__ __launch_bounds__(WG) void phase_span_ins_kernel(const PolRow *__restrict__ rows, uint32_t n_rows, const uint32_t *__restrict__ key,
                                                            uint32_t n_sites, uint32_t *__restrict__ s_lo, uint32_t *__restrict__ cnt) {
    const uint32_t step = gridDim.x * WG;
    for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < n_rows; k += step) {
        const PolRow r = rows[k];
        const uint32_t lo = lower_bound_in(key, 0, n_sites, 2u * (r.cbase + r.ts) + 1u);
        const uint32_t hi = lower_bound_in(key, lo, n_sites, 2u * (r.cbase + max(r.ts, r.te)));
        s_lo[k] = lo;
        cnt[k] = hi - lo;
    }
}

__global__ __launch_bounds__(WG) void phase_fill_ins_kernel(uint32_t n_rows, const uint32_t *__restrict__ key, const uint32_t *__restrict__ s_lo,
                                                            const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off,
                                                            uint8_t *__restrict__ table) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * WAVES;
    for (uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6); k < n_rows; k += n_waves) {
        const uint32_t n = cnt[k], lo = s_lo[k];
        uint8_t *out = table + off[k];
        for (uint32_t i = lane; i < n; i += 64) out[i] = (key[lo + i] & 1u) ? (uint8_t)AL_NONE : (uint8_t)AL_OWN;
    }
}

struct AlleleInsArgs {
    const PolRow *rows;
    uint32_t n_rows;
    const uint32_t *ops;
    const uint8_t *reads;
    const uint32_t *key;                        // 2 g + 1: position g; 2 g: the slot in front of it
    const uint8_t *meta;                        // a position site: own | alt << 4; an insertion site: its called length, 1 .. 16
    const uint32_t *s_lo, *cnt;
    const uint64_t *off;
    uint8_t *table;
};

template <int ENC>
__global__ __launch_bounds__(WG) void phase_allele_ins_kernel(const AlleleInsArgs A) {
    const int lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * WAVES;
    for (uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6); k < A.n_rows; k += n_waves) {
        const uint32_t n = A.cnt[k];
        if (!n) continue;                                                       // (the same in every lane)
        const PolRow r = A.rows[k];
        const uint32_t lo = A.s_lo[k], hi = lo + n;
        uint8_t *out = A.table + A.off[k];
        // site s of [a, b) below lies inside this lane's op: lo <= a <= s < b <= hi; a slot among them is no column of the op
        auto put = [&](uint32_t s, uint32_t code, uint32_t tp0, uint32_t qc0, uint32_t) {
            const uint32_t ky = A.key[s];
            if (!(ky & 1u)) return;
            const uint32_t p = (ky >> 1) - r.cbase;
            const uint32_t sym = code == OP_D ? (uint32_t)SYM_DEL : column_symbol<ENC>(r, A.reads, qc0 + (p - tp0));
            if (sym >= (uint32_t)var::N_SYM) return;                            // an N of the read: AL_NONE stays
            const uint32_t pk = A.meta[s];
            out[s - lo] = sym == (pk & 15u) ? AL_OWN : sym == (pk >> 4) ? AL_ALT : AL_OTHER;
        };
        walk_row(r, A.ops, lane, r.te, [&](uint32_t code, uint32_t len, uint32_t tp0, uint32_t qc0) {
            if (code == OP_I && len >= 1 && tp0 > r.ts && tp0 < r.te) {         // one I op is one slot's insertion; at ts or te: none's
                const uint32_t want = 2u * (r.cbase + tp0), s = lower_bound_in(A.key, lo, hi, want);
                if (s < hi && A.key[s] == want) out[s - lo] = len == (uint32_t)A.meta[s] ? AL_ALT : AL_OTHER;
            }
            uint32_t a = 0, b = 0;              // the sites of either kind inside this op's target range
            if (len && (code == OP_EQ || code == OP_X || code == OP_D)) {
                const uint32_t t0 = max(tp0, r.ts), t1 = max(t0, min(tp0 + len, r.te));
                a = lower_bound_in(A.key, lo, hi, 2u * (r.cbase + t0) + 1u);
                b = lower_bound_in(A.key, a, hi, 2u * (r.cbase + t1));
            }
            vote_columns<false>(a, b, code, tp0, qc0, 1u, lane, put);
        });
    }
}

}  // namespace

void phase_ins_core(const char *who, const PolCoreIn &in, const MergedSites &M, const hlmi_phase_opts &o, DevicePhase &out, int reach,
                    DevRecs *keep) {
    out = DevicePhase{};
    out.far.reach = reach;
    if (keep) *keep = DevRecs{};
    const size_t N = M.sites.size(), R = in.n_rows;
    if (reach < 1 || M.key.size() != N || M.ins_of.size() != N) fail(HLMI_ESTATE, "%s: the merged sites in the allele pass", who);     // (never)
    DBuf<uint32_t> d_key, d_lo, d_cnt;
    DBuf<uint8_t> d_meta, d_table;
    DBuf<uint64_t> d_off;
    if (N >= (1ull << 31)) fail(HLMI_EINVAL, "%s: %zu sites (2^31 and more)", who, N);
    if (N && R) {
        d_lo.alloc(R);
        d_cnt.alloc(R);
        d_off.alloc(R);
        KTimer kt("phase_allele_ins");
        std::vector<uint8_t> meta(N);
        for (size_t i = 0; i < N; ++i)
            meta[i] = M.slot(i) ? (uint8_t)M.ins[(size_t)M.ins_of[i]].len : (uint8_t)(M.sites[i].own | M.sites[i].alt << 4);
        d_key.upload(M.key);
        d_meta.upload(meta);
        hipLaunchKernelGGL(phase_span_ins_kernel, grid1(R), dim3(WG), 0, stream(), in.rows, (uint32_t)R, d_key.p, (uint32_t)N, d_lo.p, d_cnt.p);
        HIP_CHECK(hipGetLastError());
        exclusive_scan_u32_to_u64(d_cnt.p, d_off.p, R);
        out.alleles = download_one(d_off.p + (R - 1)) + download_one(d_cnt.p + (R - 1));
        if (out.alleles >= (1ull << 32)) fail(HLMI_EINVAL, "%s: %llu alleles of rows at sites (2^32 and more)", who, (unsigned long long)out.alleles);
        check_fits(who, "the allele table", out.alleles);
        if (out.alleles) {
            d_table.alloc(out.alleles);
            const dim3 g((unsigned)std::min<size_t>(cdiv(R, WAVES), MAX_GRID));
            hipLaunchKernelGGL(phase_fill_ins_kernel, g, dim3(WG), 0, stream(), (uint32_t)R, d_key.p, d_lo.p, d_cnt.p, d_off.p, d_table.p);
            HIP_CHECK(hipGetLastError());
            AlleleInsArgs a{in.rows, (uint32_t)R, in.ops, in.reads, d_key.p, d_meta.p, d_lo.p, d_cnt.p, d_off.p, d_table.p};
            if (in.enc == READS_CODES) hipLaunchKernelGGL((phase_allele_ins_kernel<READS_CODES>), g, dim3(WG), 0, stream(), a);
            else hipLaunchKernelGGL((phase_allele_ins_kernel<READS_ASCII>), g, dim3(WG), 0, stream(), a);
            HIP_CHECK(hipGetLastError());
        }
    }
    phase_tail(who, R, M.sites, o, out, keep, reach, d_lo, d_cnt, d_off, d_table);
}

}  // namespace ph
}  // namespace hlmi
