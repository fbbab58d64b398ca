// vq_clique.hip - SRBuilder::cliquesToSuperreads (tools/HaploConduct/src/SRBuilder.cpp:1031-1235) for single-end reads: one
// pile-up consensus of up to 63 placed reads per maximal clique (constructSuperread :654-870, consensus :406-533,
// consensus_pos :297-402).  The cliques come from vq_clique_host.cpp, the graph from vq_graph_host.cpp.
//   pile_kernel   one wave per pile-up, lanes across 64 columns of a tile, a loop over the pile's reads inside: the four
//                 log-scores are summed in list order in double precision (the tables are the host's libm values, the build
//                 turns contraction off), one and two bases go through the tables of vq_merge.hip, more through the device's
//                 pow / log10 with a margin (vqc::MARGIN) inside which the column goes back to the host.  The
//                 end of the trimmed output - the first column with too little support once every read has started - is the
//                 first set bit of the wave's ballot, and the tile loop ends there.
// The host part below places the reads (sort_vertices :33-286, filter_subreads :597-636 with the same std::sort), decides
// the drops, keeps the originals and writes the files.  Every loop on the device has an explicit bound.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "paf_io.h"
#include "vq_internal.h"

namespace hlmi {
namespace vqc {
namespace {

using vqm::NQ;                                   // the consensus tables of vq_merge.hip
using vqm::T_ALL; using vqm::T_SINGLE; using vqm::T_WITH_N; using vqm::T_SAME; using vqm::T_DIFF;
constexpr int WAVES = WG / WAVE;

__device__ __forceinline__ uint32_t base_code(uint8_t c) {      // A C G T N -> 0 .. 4 (the host refuses anything else)
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
__device__ __forceinline__ uint8_t complement(uint8_t c) {      // Read::build_rev_comp: N stays N
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

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
                            const uint32_t act = t >> 8;
                            e = ((uint32_t)(act == 0 ? 'N' : act == 2 ? b2 : b1) << 8) | (t & 0xffu);
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
                                 bool error_correction, std::vector<uint8_t> &bases, std::vector<uint8_t> &quals,
                                 std::vector<Result> &res) {
    bases.clear(); quals.clear(); res.clear();
    if (piles.empty()) return;
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
                           (uint32_t)piles.size(), d_entries.p, d_bases_.p, d_quals_.p, d_off_.p, d_tab_.p, d_logs.p, 0.9,
                           pow(10.0, -9.3), min_support, error_correction ? 1 : 0, d_b.p, d_q.p, d_res.p);
        HIP_CHECK(hipGetLastError());
    }
    bases = d_b.download();
    quals = d_q.download();
    res = d_res.download();
}

void vq_clique_opts_polyte(hlmi_vq_clique_opts *o, int error_correction) {
    *o = hlmi_vq_clique_opts{};
    o->min_clique_size = 2;                      // HyLight.py:228-242
    o->error_correction = error_correction != 0;
    o->first_it = 1;
    o->keep_singletons = error_correction ? 1000 : 0;        // polyte.tune_params.py:689-696
}

void vq_cliques_of_graph(const char *graph_txt, const char *cliques_out, uint64_t *n_cliques) {
    const VqCliqueList list = vq_enumerate_cliques(read_file(graph_txt));
    write_file(cliques_out, list.text.data(), list.text.size());
    *n_cliques = list.off.size() - 1;
}

void vq_cliques_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                    const hlmi_vq_clique_opts &co, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst) {
    *cst = hlmi_vq_clique_stats{};
    if (co.min_clique_size == 0 || co.min_clique_size > MAX_MIN_CLIQUE)
        fail(HLMI_EINVAL, "vq_cliques: min_clique_size %u is outside 1 .. %u", co.min_clique_size, MAX_MIN_CLIQUE);
    if (!co.first_it && !subreads_in) fail(HLMI_EINVAL, "vq_cliques: first_it is off and there is no subreads file");
    const uint32_t mcs = co.min_clique_size;
    VqGraphState g;
    vq_graph_run(fastq, overlaps, go, out_dir, gst, &g, false);
    if (!g.built) return;                        // ViralQuasispecies.cpp:282-291: nothing to be done
    const double t0 = now_ms();
    const uint32_t V = (uint32_t)g.seq.size();
    for (uint32_t v = 0; v < V; ++v) cst->bases_in += g.seq[v].size();
    std::map<uint64_t, VqOriginals> dict;
    if (!co.first_it) dict = vq_parse_subreads(read_file(subreads_in), subreads_in);
    auto originals_of = [&](uint32_t v) -> VqOriginals {
        if (co.first_it) return VqOriginals{{g.id[v], VqOrig{true, 0, (int)g.seq[v].size()}}};
        auto it = dict.find(g.id[v]);
        if (it == dict.end() || it->second.empty())
            fail(HLMI_EINVAL, "vq_cliques: read %llu has no line in %s", (unsigned long long)g.id[v], subreads_in);
        return it->second;
    };

    // cliques.txt (ViralQuasispecies.cpp:400-410)
    const VqCliqueList list = vq_enumerate_cliques(read_file(join_path(out_dir, "graph.txt").c_str()));
    write_file(join_path(out_dir, "cliques.txt"), list.text.data(), list.text.size());
    const double t_enumerated = now_ms();
    const size_t n_lines = list.off.size() - 1;
    cst->cliques_read = n_lines + 2;             // getline counts the two text lines as well (:1056-1057)

    // getEdgeInfo (OverlapGraph.cpp:263-282): the first u -> v of u's list
    auto edge_of = [&](uint32_t u, uint32_t v) -> const VqEdge * {
        for (const VqEdge &e : g.out[u])
            if (e.v2 == v) return &e;
        return nullptr;
    };

    // constructSuperread per clique: the placement
    struct Placed {
        std::vector<uint32_t> clique;            // ascending
        std::vector<std::pair<int64_t, uint32_t>> all;       // (offset, vertex) in list order, every member
        uint32_t pile;                           // its pile-up
    };
    std::vector<Placed> placed;
    std::vector<Pile> piles;
    std::vector<Entry> entries;
    uint64_t cols = 0;
    for (size_t k = 0; k < n_lines; ++k) {
        const size_t size = (size_t)(list.off[k + 1] - list.off[k]);
        if (size == 1) { ++cst->singletons; continue; }
        if (size < mcs) { ++cst->below_min; continue; }
        ++cst->taken;
        Placed P;
        P.clique.assign(list.members.begin() + (ptrdiff_t)list.off[k], list.members.begin() + (ptrdiff_t)list.off[k + 1]);
        for (uint32_t v : P.clique)
            if (v >= V) fail(HLMI_EINVAL, "vq_cliques: clique vertex %u of %u", v, V);
        std::sort(P.clique.begin(), P.clique.end());                       // :658
        const uint32_t base = P.clique[0];       // single-end reads: the first one is the base (:670-679)
        const int64_t base_len = (int64_t)g.seq[base].size();
        int64_t l_ext = 0, r_ext = 0;
        P.all.emplace_back(0, base);
        for (uint32_t v : P.clique) {
            if (v == base) continue;
            const VqEdge *found = edge_of(base, v);
            if (!found) found = edge_of(v, base);
            if (!found) fail(HLMI_EINVAL, "vq_cliques: no edge between %u and %u", base, v);
            const VqEdge &e = *found;
            const int64_t new_pos = e.v1 == base ? (int64_t)e.pos1 : -(int64_t)e.pos1;     // :142-147
            size_t at = 0;                       // in front of the first entry that is not smaller (:212-222)
            while (at < P.all.size() && P.all[at].first < new_pos) ++at;
            P.all.insert(P.all.begin() + (ptrdiff_t)at, std::make_pair(new_pos, v));
            l_ext = std::max(l_ext, -new_pos);                             // :236-240
            r_ext = std::max(r_ext, (int64_t)g.seq[v].size() + new_pos - base_len);
        }
        const int64_t total = base_len + l_ext + r_ext;
        if (total >= (1 << 30)) fail(HLMI_EINVAL, "vq_cliques: a super-read of %lld bases", (long long)total);
        const int64_t shift = P.all[0].first < 0 ? -P.all[0].first : 0;    // :248-252
        for (auto &pv : P.all) pv.first += shift;
        // filter_subreads (:597-636) when the clique is large (:721)
        std::vector<std::pair<int64_t, uint32_t>> used = P.all;
        if (size > 3 * (size_t)mcs) {
            ++cst->filtered;
            const size_t num = 2 * (size_t)mcs;
            std::unordered_map<uint32_t, bool> sel;
            for (size_t i = 0; i < num / 2; ++i) sel[P.all[i].second] = true;
            sel[base] = true;
            std::vector<std::pair<uint32_t, int>> by_end;                  // sortVerticesByEndpos (:639-652): the same std::sort
            for (const auto &pv : P.all) by_end.emplace_back(pv.second, (int)(pv.first + (int64_t)g.seq[pv.second].size()));
            std::sort(by_end.begin(), by_end.end(), [](const std::pair<uint32_t, int> &a, const std::pair<uint32_t, int> &b) { return a.second < b.second; });
            for (size_t i = by_end.size(); i > 0 && sel.size() < num; --i) sel[by_end[i - 1].first] = true;
            used.clear();
            for (const auto &pv : P.all) if (sel.count(pv.second)) used.push_back(pv);
        }
        // consensus (:420-446): where the output starts; a read in front of it that ends there empties it (:478)
        uint32_t trim = 0;
        bool empty = false;
        if (co.error_correction) {
            // :427-432 drops a pile without an entry number min_clique_size.  A clique taken here has min_clique_size
            // members and a filtered one 2 * min_clique_size, so the check never fires; it stays as the reference has it.
            if (used.size() < mcs) { ++cst->dropped_support; continue; }
            trim = (uint32_t)used[mcs - 1].first;
            for (const auto &pv : used)
                if (pv.first < (int64_t)trim && pv.first + (int64_t)g.seq[pv.second].size() <= (int64_t)trim) empty = true;
        }
        if (empty || trim >= total) { ++cst->dropped_empty; continue; }
        if (used.size() > MAX_PILE) fail(HLMI_EINVAL, "vq_cliques: a pile-up of %zu reads", used.size());
        Pile pl{};
        pl.first = (uint32_t)entries.size(); pl.n = (uint32_t)used.size();
        pl.total_len = (uint32_t)total; pl.trim_pos = trim; pl.col0 = cols;
        for (const auto &pv : used) entries.push_back(Entry{pv.second, (uint32_t)pv.first, g.orient[pv.second] ? 0u : 1u});
        cols += (uint64_t)total;
        P.pile = (uint32_t)piles.size();
        piles.push_back(pl);
        placed.push_back(std::move(P));
    }

    const double t_placed = now_ms();
    VqMergeDev dev(g.seq, g.qual, vq_consensus_tables());
    std::vector<uint8_t> cb, cq;
    std::vector<Result> res;
    dev.consensus_piles(piles, entries, mcs, co.error_correction != 0, cb, cq, res);
    const double t_device = now_ms();

    // process_cliques (:998-1001), writeSinglesToFile, the originals (:750-806)
    auto n_rate_ok = [](uint64_t n, uint64_t len) { return (double)n < 0.05 * (double)len; };       // Read.h:214-233
    std::string fastq_text, subreads, cmap;
    std::vector<uint8_t> visited(V, 0);
    uint32_t count = 0;
    std::vector<char> nuc(MAX_PILE);
    std::vector<int> phred(MAX_PILE);
    for (const Placed &P : placed) {
        const Pile &pl = piles[P.pile];
        const Result &r = res[P.pile];
        if (r.empty || r.stop <= pl.trim_pos || r.stop > pl.total_len) {
            if (!r.empty && r.stop > pl.total_len) fail(HLMI_EINVAL, "vq_cliques: the device ended a consensus at %u of %u", r.stop, pl.total_len);
            ++cst->dropped_empty;
            continue;
        }
        const uint32_t len = r.stop - pl.trim_pos;
        uint8_t *b = cb.data() + pl.col0 + pl.trim_pos, *q = cq.data() + pl.col0 + pl.trim_pos;
        uint64_t n_count = 0;
        for (uint32_t x = 0; x < len; ++x) {
            if (q[x] == 0) {                     // too close to a threshold for the device: the host's libm decides
                const uint32_t c = pl.trim_pos + x;
                int n = 0;
                for (uint32_t k = 0; k < pl.n; ++k) {
                    const Entry &e = entries[pl.first + k];
                    const std::string &s = g.seq[e.read], &ql = g.qual[e.read];
                    if (c < e.pos || c - e.pos >= s.size()) continue;
                    const size_t i = c - e.pos;
                    char ch = e.rev ? s[s.size() - 1 - i] : s[i];
                    if (e.rev) ch = ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch;
                    nuc[(size_t)n] = ch;
                    phred[(size_t)n++] = (e.rev ? ql[s.size() - 1 - i] : ql[i]) - 33;
                }
                const uint16_t e = vq_consensus_pos(nuc.data(), phred.data(), n);
                b[x] = (uint8_t)(e >> 8);
                q[x] = (uint8_t)e;
                ++cst->columns_host;
            }
            n_count += b[x] == 'N';
        }
        cst->columns += len;
        if (!n_rate_ok(n_count, len)) { ++cst->dropped_n; continue; }
        fastq_text += '@'; fastq_text += std::to_string(count); fastq_text += '\n';
        fastq_text.append((const char *)b, len); fastq_text += "\n+\n";
        fastq_text.append((const char *)q, len); fastq_text += '\n';
        std::unordered_map<uint32_t, int64_t> offset;        // calcSubreadInfo (:536-595): index1 - startpos1 = offset - trim_pos
        for (const auto &pv : P.all) offset.emplace(pv.second, pv.first - (int64_t)pl.trim_pos);
        VqOriginals merged;
        for (uint32_t v : P.clique) {
            vq_originals_add(merged, originals_of(v), g.orient[v] != 0, co.first_it != 0, (long)offset.at(v), (long)g.seq[v].size());
            visited[v] = 1;
        }
        vq_subreads_line(subreads, count, merged);
        cmap += std::to_string(count); cmap += '\t'; cmap += std::to_string(pl.trim_pos);
        for (const auto &pv : P.all) {
            cmap += '\t'; cmap += std::to_string(pv.second); cmap += ':'; cmap += std::to_string(pv.first - (int64_t)pl.trim_pos);
            cmap += ':'; cmap += g.orient[pv.second] ? '+' : '-';
        }
        cmap += '\n';
        ++count;
    }
    cst->superreads = count;

    // the reads in no kept super-read (:1145-1222)
    const std::vector<uint32_t> read_n = dev.read_n_counts();
    std::vector<vqm::Rec> recs;
    for (uint32_t v = 0; v < V; ++v) {
        if (visited[v]) continue;
        const uint32_t len = (uint32_t)g.seq[v].size();
        if (len < co.keep_singletons) { ++cst->short_reads; continue; }                  // :1149
        if (!n_rate_ok(read_n[v], len)) { ++cst->n_reads; continue; }                    // :1155
        vqm::Rec r{};
        r.a = v; r.b = vqm::NONE; r.len = len; r.id = count;
        VqOriginals o = originals_of(v);
        if (!g.orient[v]) {                      // :1186-1217: a forward copy of the reverse read
            r.flags = vqm::F_REV_A;
            vq_originals_mirror(o, (long)len);
            ++cst->trivial_reverse;
        }
        ++cst->trivial;
        vq_subreads_line(subreads, count, o);
        recs.push_back(r);
        ++count;
    }
    std::vector<uint64_t> start;
    fastq_text += dev.write(recs, start);
    cst->bytes_out = fastq_text.size();
    write_file(join_path(out_dir, "singles.fastq"), fastq_text.data(), fastq_text.size());         // (the reference removes it first, :1038)
    write_file(join_path(out_dir, "subreads.txt"), subreads.data(), subreads.size());
    write_file(join_path(out_dir, "clique_map.txt"), cmap.data(), cmap.size());
    cst->ms_cliques = now_ms() - t0;
    ktimer_flush();
    // the phases of ms_cliques for tools/vq_cliques_time.py: enumerator, placement, device (uploads, kernel, downloads), the rest
    stat_set("vq_clique_ms_enumerate", t_enumerated - t0);
    stat_set("vq_clique_ms_place", t_placed - t_enumerated);
    stat_set("vq_clique_ms_device", t_device - t_placed);
    stat_set("vq_clique_ms_finish", t0 + cst->ms_cliques - t_device);
    stat_set("vq_clique_piles", (double)piles.size());
}

}  // namespace hlmi
