// vq_clique.hip - SRBuilder::cliquesToSuperreads (tools/HaploConduct/src/SRBuilder.cpp:1031-1235) for single-end reads: one
// pile-up consensus of up to 63 placed reads per maximal clique (constructSuperread :654-870, consensus :406-533,
// consensus_pos :297-402).  The cliques come from vq_clique_host.cpp, the graph from vq_graph_host.cpp.
//   pile_kernel   one wave per pile-up, lanes across 64 columns of a tile, a loop over the pile's reads inside: the four
//                 log-scores are summed in list order in double precision (the tables are the host's libm values, the build
//                 turns contraction off), one and two bases go through the tables of vq_merge.hip, more through the device's
//                 pow / log10 with a margin (vqc::MARGIN) inside which the column goes back to the host.  The
//                 end of the trimmed output - the first column with too little support once every read has started - is the
//                 first set bit of the wave's ballot, and the tile loop ends there.
// VqMergeDev::consensus_piles checks the pile-ups' bounds and launches it; vq_cliques_run (vq_superread_run.cpp) places the
// reads, decides the drops and writes the files.  Every loop on the device has an explicit bound.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "vq_internal.h"

namespace hlmi {
namespace vqc {
namespace {

using vqm::NQ;                                   // the consensus tables of vq_merge.hip
using vqm::base_code; using vqm::complement; using vqm::pair_base;
using vqm::T_ALL; using vqm::T_SINGLE; using vqm::T_WITH_N; using vqm::T_SAME; using vqm::T_DIFF;
constexpr int WAVES = WG / WAVE;

// consensus_pos (:351-401) behind the sums, for a column of three bases and more -> (base << 8) | quality, 0: the host decides
__device__ __forceinline__ uint32_t decide(double sA, double sC, double sG, double sT, double min_qual, double p93) {
    const double max_score = fmax(fmax(sA, sT), fmax(sC, sG));
    const double max_prob = pow(10.0, max_score);
    const double total_prob = pow(10.0, sA) + pow(10.0, sT) + pow(10.0, sC) + pow(10.0, sG);
    if (max_score == 0 || total_prob == 0.0) return 0;
    if (max_prob < MIN_PROB) return 0;          // towards the subnormals pow's relative error is no longer an ULP or two
    const double p_incorrect = 1 - (max_prob / total_prob);
    const double sure = 1 - p_incorrect;
    if (!(fabs(sure - min_qual) > MARGIN)) return 0;                       // (also a NaN)
    if (sure < min_qual) return ((uint32_t)'N' << 8) | '$';
    if (!(fabs(p_incorrect - p93) > MARGIN)) return 0;
    int phred = 93;
    if (p_incorrect >= p93) {
        const double x = -10 * log10(p_incorrect);
        if (!(fabs(x - (floor(x) + 0.5)) > X_SLOPE * MARGIN / p_incorrect + X_FLOOR)) return 0;
        phred = (int)round(x);
    }
    phred = phred < 0 ? 0 : phred > 93 ? 93 : phred;
    const uint32_t b = max_score == sA ? 'A' : max_score == sT ? 'T' : max_score == sC ? 'C' : 'G';     // the chain of :390-393
    return (b << 8) | (uint32_t)(phred + 33);
}

__global__ __launch_bounds__(WG) void pile_kernel(const Pile *piles, uint32_t n_piles, const Entry *entries, const uint8_t *bases,
                                                  const uint8_t *quals, const uint64_t *off, const uint16_t *tab,
                                                  const double *logs, double min_qual, double p93, uint32_t min_support, int ec,
                                                  uint8_t *out_b, uint8_t *out_q, Result *res) {
    __shared__ uint16_t lds_tab[T_ALL];
    __shared__ double lds_log[2 * NQ];           // log10(1 - p) per phred, then log10(p / 3)
    __shared__ uint64_t e_at[WAVES][WAVE];       // per wave: its pile's entries - first byte of the read,
    __shared__ uint32_t e_pos[WAVES][WAVE], e_len[WAVES][WAVE], e_rev[WAVES][WAVE];     // first column, bases, reversed
    for (int i = threadIdx.x; i < T_ALL; i += WG) lds_tab[i] = tab[i];
    for (int i = threadIdx.x; i < 2 * NQ; i += WG) lds_log[i] = logs[i];
    const uint32_t w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    for (uint32_t first_pile = blockIdx.x * WAVES; first_pile < n_piles; first_pile += gridDim.x * WAVES) {   // the same trips for all waves
        const uint32_t pile = first_pile + w;
        const bool active = pile < n_piles;
        Pile P{};
        if (active) P = piles[pile];
        if (active && lane < P.n) {              // (the host holds n <= MAX_PILE < WAVE)
            const Entry e = entries[P.first + lane];
            e_at[w][lane] = off[e.read];
            e_len[w][lane] = (uint32_t)(off[e.read + 1] - off[e.read]);
            e_pos[w][lane] = e.pos;
            e_rev[w][lane] = e.rev;
        }
        __syncthreads();                         // tables and entries are in place
        if (active) {
            const uint32_t last_start = e_pos[w][P.n - 1];                 // the list is ordered by offset
            uint32_t stop = P.total_len, empty = 0;
            for (uint32_t c0 = P.trim_pos; c0 < P.total_len; c0 += WAVE) { // at most 2^30 / 64 tiles
                const uint32_t c = c0 + lane;
                const bool valid = c < P.total_len;
                double sA = 0, sC = 0, sG = 0, sT = 0;
                uint32_t cnt = 0, c1 = 4, i1 = 0, c2 = 4, i2 = 0;
                uint8_t b1 = 'N', b2 = 'N';
                for (uint32_t r = 0; r < P.n; ++r) {
                    const uint32_t pos = e_pos[w][r], len = e_len[w][r];
                    if (!valid || c < pos || c - pos >= len) continue;
                    const uint32_t i = c - pos;
                    const uint64_t at = e_rev[w][r] ? e_at[w][r] + (len - 1 - i) : e_at[w][r] + i;
                    uint8_t b = bases[at];
                    const uint32_t q = (uint32_t)quals[at] - 33u;
                    if (e_rev[w][r]) b = complement(b);
                    const uint32_t code = base_code(b);
                    if (cnt == 0) { b1 = b; c1 = code; i1 = q; }
                    else if (cnt == 1) { b2 = b; c2 = code; i2 = q; }
                    ++cnt;
                    if (code < 4) {              // an N adds nothing (:343-348)
                        const double hit = lds_log[q], miss = lds_log[NQ + q];
                        sA += code == 0 ? hit : miss;
                        sC += code == 1 ? hit : miss;
                        sG += code == 2 ? hit : miss;
                        sT += code == 3 ? hit : miss;
                    }
                }
                // :466-473: too little support once every read has started ends the output; in front of that a column
                // without a read empties it (:498)
                const bool low = ec && valid && cnt < min_support && c >= last_start;
                const unsigned long long low_mask = __ballot(low);
                const uint32_t first_low = low_mask ? (uint32_t)__ffsll((long long)low_mask) - 1u : (uint32_t)WAVE;
                const bool mine = valid && lane < first_low;
                if (__ballot(mine && cnt == 0)) { empty = 1; break; }
                if (mine) {
                    uint32_t e;
                    if (cnt == 1) {
                        e = lds_tab[T_SINGLE + c1 * NQ + i1];
                    } else if (cnt == 2) {
                        if (c1 == 4 && c2 == 4) e = ((uint32_t)'N' << 8) | '$';                    // max_score == 0 (:354-357)
                        else if (c1 == 4 || c2 == 4) e = c1 == 4 ? lds_tab[T_WITH_N + c2 * NQ + i2] : lds_tab[T_WITH_N + c1 * NQ + i1];
                        else {
                            const uint32_t t = lds_tab[(c1 == c2 ? T_SAME : T_DIFF) + i1 * NQ + i2];
                            e = ((uint32_t)pair_base(t >> 8, b1, b2, c1, c2) << 8) | (t & 0xffu);
                        }
                    } else {
                        e = decide(sA, sC, sG, sT, min_qual, p93);
                    }
                    out_b[P.col0 + c] = (uint8_t)(e >> 8);
                    out_q[P.col0 + c] = (uint8_t)e;
                }
                if (low_mask) { stop = c0 + first_low; break; }
            }
            if (lane == 0) res[pile] = Result{stop, empty};
        }
        __syncthreads();                         // before the next piles' entries replace these
    }
}

}  // namespace
}  // namespace vqc

using namespace vqc;

void VqMergeDev::consensus_piles(const std::vector<Pile> &piles, const std::vector<Entry> &entries, uint32_t min_support,
                                 bool error_correction, double min_qual, std::vector<uint8_t> &bases, std::vector<uint8_t> &quals,
                                 std::vector<Result> &res) {
    bases.clear(); quals.clear(); res.clear();
    if (piles.empty()) return;
    vq_check_min_qual(min_qual, "vq_cliques");
    if (piles.size() >= (1ull << 31) || entries.size() >= (1ull << 32)) fail(HLMI_EINVAL, "vq_cliques: %zu pile-ups", piles.size());
    const std::vector<uint64_t> off = d_off_.download();
    uint64_t cols = 0;
    for (const Pile &p : piles) {                // bounds before anything runs on the device
        if (p.n == 0 || p.n > MAX_PILE || (uint64_t)p.first + p.n > entries.size() || p.total_len == 0 || p.total_len >= (1u << 30) ||
            p.trim_pos >= p.total_len || p.col0 != cols)
            fail(HLMI_EINVAL, "vq_cliques: bad pile-up (%u reads, %u columns)", p.n, p.total_len);
        for (uint32_t k = 0; k < p.n; ++k) {
            const Entry &e = entries[p.first + k];
            if (e.read >= n_reads_ || (k && e.pos < entries[p.first + k - 1].pos) ||
                (uint64_t)e.pos + (off[e.read + 1] - off[e.read]) > p.total_len)
                fail(HLMI_EINVAL, "vq_cliques: bad pile-up entry (read %u of %zu at %u of %u columns)", e.read, n_reads_, e.pos, p.total_len);
        }
        cols += p.total_len;
    }
    std::vector<double> logs(2 * vqm::NQ);
    for (int q = 0; q < vqm::NQ; ++q) {
        const double p = pow(10, -q / 10.0);                              // phred_to_prob (:289-293)
        logs[(size_t)q] = log10(1 - p);
        logs[(size_t)(vqm::NQ + q)] = log10(p / 3.0);
    }
    DBuf<Pile> d_piles;
    DBuf<Entry> d_entries;
    DBuf<double> d_logs;
    d_piles.upload(piles);
    d_entries.upload(entries);
    d_logs.upload(logs);
    DBuf<uint8_t> d_b(cols), d_q(cols);
    DBuf<Result> d_res(piles.size());
    d_b.zero();                                  // columns outside [trim_pos, stop) are never written
    d_q.zero();
    int dev = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint64_t per_wg = vqc::WG / vqc::WAVE, want = (piles.size() + per_wg - 1) / per_wg, cap = (uint64_t)(cus > 0 ? cus : 64) * 4;
    {
        KTimer t("vq_clique_piles");
        hipLaunchKernelGGL(pile_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(vqc::WG), 0, stream(), d_piles.p,
                           (uint32_t)piles.size(), d_entries.p, d_bases_.p, d_quals_.p, d_off_.p, d_tab_.p, d_logs.p, min_qual,
                           pow(10.0, -9.3), min_support, error_correction ? 1 : 0, d_b.p, d_q.p, d_res.p);
        HIP_CHECK(hipGetLastError());
    }
    bases = d_b.download();
    quals = d_q.download();
    res = d_res.download();
}

}  // namespace hlmi
