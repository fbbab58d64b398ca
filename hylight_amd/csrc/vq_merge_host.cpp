// vq_merge_host.cpp - SRBuilder with --cliques=false --error_correction=false --threads 1 (tools/HaploConduct/src,
// ViralQuasispecies.cpp:413-447, SRBuilder::mergeAlongEdges, SRBuilder.cpp:1238-1384): the super-reads of the next stage-b
// iteration from the graph vq_graph_host.cpp leaves.  Host side: the consensus tables (libm), the greedy merge list, the
// placement of each pair, the drop decisions, the originals' index arithmetic and the text files.  The bases are read,
// combined and laid out as FASTQ text in vq_merge.hip.
// PARITY UNPINNED: the reference needs Boost and cannot be built here; tests/vq_merge_model.py restates it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "paf_io.h"
#include "vq_internal.h"

namespace hlmi {
namespace {

using namespace vqm;

constexpr double MIN_QUAL = 0.9;          // ViralQuasispecies.cpp:62 (--min_qual default) -> SRBuilder.h:89

}  // namespace

// SRBuilder::consensus_pos (:297-402) in its own expression order.  -> (base << 8) | quality
uint16_t vq_consensus_pos(const char *nuc, const int *phred, int n) {
    double score_A = 0, score_C = 0, score_T = 0, score_G = 0;
    for (int i = 0; i < n; ++i) {
        const double p = pow(10, -phred[i] / 10.0);                        // phred_to_prob (:289-293)
        switch (nuc[i]) {
            case 'A': score_A += log10(1 - p); score_C += log10(p / 3.0); score_T += log10(p / 3.0); score_G += log10(p / 3.0); break;
            case 'C': score_C += log10(1 - p); score_A += log10(p / 3.0); score_T += log10(p / 3.0); score_G += log10(p / 3.0); break;
            case 'T': score_T += log10(1 - p); score_C += log10(p / 3.0); score_A += log10(p / 3.0); score_G += log10(p / 3.0); break;
            case 'G': score_G += log10(1 - p); score_C += log10(p / 3.0); score_T += log10(p / 3.0); score_A += log10(p / 3.0); break;
            default: break;                                                // 'N' adds nothing (:343-348)
        }
    }
    const double max_score = std::max({score_A, score_T, score_C, score_G});
    const double max_prob = std::pow(10.0, max_score);
    const double total_prob = std::pow(10.0, score_A) + std::pow(10.0, score_T) + std::pow(10.0, score_C) + std::pow(10.0, score_G);
    const uint16_t n_out = (uint16_t)(('N' << 8) | '$');
    if (max_score == 0 || total_prob == 0.0) return n_out;                 // :354-359
    const double p_incorrect = 1 - (max_prob / total_prob);
    if (n > 1 && (1 - p_incorrect) < MIN_QUAL) return n_out;               // :362-368
    if (p_incorrect != p_incorrect) fail(HLMI_EINVAL, "vq_merge: consensus table entry is not a number");   // (:369-372: never)
    int phred_out;
    if (p_incorrect < std::pow(10.0, -9.3)) phred_out = 93;
    else phred_out = (int)round(-10 * log10(p_incorrect));
    if (phred_out < 0) phred_out = 0;
    else if (phred_out > 93) phred_out = 93;
    char b;
    if (max_score == score_A) b = 'A';                                     // the tie order of :390-393
    else if (max_score == score_T) b = 'T';
    else if (max_score == score_C) b = 'C';
    else b = 'G';
    return (uint16_t)((b << 8) | (phred_out + 33));
}

namespace {
inline uint16_t consensus_pos(const char *nuc, const int *phred, int n) { return vq_consensus_pos(nuc, phred, n); }

// The tables of vq_internal.h (vqm::T_*).  Every pair of (base, quality) is evaluated; the forms by class that fit LDS are
// kept only if the answer does not depend on which bases they are - it can, through the order of the four terms of
// total_prob - and the build fails otherwise (with glibc's libm it does not).
std::vector<uint16_t> build_consensus_tables() {
    std::vector<uint16_t> t((size_t)T_ALL);
    const char B[6] = "ACGTN";
    for (int c = 0; c < 5; ++c)
        for (int q = 0; q < NQ; ++q) t[T_SINGLE + c * NQ + q] = consensus_pos(&B[c], &q, 1);
    auto pair = [&](int c1, int c2, int q1, int q2) {
        const char nuc[2] = {B[c1], B[c2]};
        const int ph[2] = {q1, q2};
        return consensus_pos(nuc, ph, 2);
    };
    for (int c = 0; c < 4; ++c)
        for (int q = 0; q < NQ; ++q) {
            const uint16_t e = pair(c, 4, q, 0);
            for (int qn = 0; qn < NQ; ++qn)                                // an N adds nothing, whatever its quality and side
                if (pair(c, 4, q, qn) != e || pair(4, c, qn, q) != e) fail(HLMI_EINVAL, "vq_merge: N changes a consensus entry");
            t[T_WITH_N + c * NQ + q] = e;
        }
    for (int q1 = 0; q1 < NQ; ++q1)
        for (int q2 = 0; q2 < NQ; ++q2) {
            if (pair(4, 4, q1, q2) != (uint16_t)(('N' << 8) | '$')) fail(HLMI_EINVAL, "vq_merge: N against N is not N");
            uint16_t same = 0, diff = 0;
            bool first_same = true, first_diff = true;
            for (int c1 = 0; c1 < 4; ++c1)
                for (int c2 = 0; c2 < 4; ++c2) {
                    const uint16_t f = pair(c1, c2, q1, q2);
                    const char b = (char)(f >> 8);
                    const int act = b == 'N' ? 0 : b == B[c1] ? 1 : (c1 != c2 && b == B[c2]) ? 2 : -1;
                    const uint16_t cur = (uint16_t)((act << 8) | (f & 0xff));
                    uint16_t &slot = c1 == c2 ? same : diff;
                    bool &first = c1 == c2 ? first_same : first_diff;
                    if (act < 0 || (!first && cur != slot))
                        fail(HLMI_EINVAL, "vq_merge: the consensus of %c/Q%d and %c/Q%d depends on the bases' identity: the tables "
                                          "by class do not hold on this libm", B[c1], q1, B[c2], q2);
                    slot = cur;
                    first = false;
                }
            t[T_SAME + q1 * NQ + q2] = same;
            t[T_DIFF + q1 * NQ + q2] = diff;
        }
    return t;
}

}  // namespace

const std::vector<uint16_t> &vq_consensus_tables() {
    static const std::vector<uint16_t> tab = build_consensus_tables();     // (initialised once, also under concurrent calls)
    return tab;
}

namespace {
inline const std::vector<uint16_t> &consensus_tables() { return vq_consensus_tables(); }

void check_read(const char *seq, size_t len, const char *qual, size_t qlen, const char *what, size_t k) {
    for (size_t i = 0; i < len; ++i) {
        const char c = seq[i];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N')
            fail(HLMI_EINVAL, "%s %zu: base 0x%02x at %zu is none of A C G T N (SRBuilder.cpp:344 asserts)", what, k, (unsigned char)c, i);
    }
    for (size_t i = 0; i < qlen; ++i)
        if (qual[i] < '!' || qual[i] > '~')
            fail(HLMI_EINVAL, "%s %zu: quality 0x%02x at %zu is outside '!' .. '~'", what, k, (unsigned char)qual[i], i);
}

// the originals of subreads.txt: vq_clique_host.cpp, shared with the clique step
using Orig = VqOrig;
using Originals = VqOriginals;
std::map<uint64_t, Originals> read_subreads(const char *path) { return vq_parse_subreads(read_file(path), path); }
inline void subreads_line(std::string &s, uint64_t id, const Originals &o) { vq_subreads_line(s, id, o); }

}  // namespace

void vq_merge_check_reads(const std::vector<std::string> &seq, const std::vector<std::string> &qual) {
    for (size_t v = 0; v < seq.size(); ++v) {
        if (qual[v].size() != seq[v].size())
            fail(HLMI_EINVAL, "vq_merge: read %zu has %zu bases and %zu qualities", v, seq[v].size(), qual[v].size());
        check_read(seq[v].data(), seq[v].size(), qual[v].data(), qual[v].size(), "vq_merge: read", v);
    }
}

void vq_merge_opts_stageb(hlmi_vq_merge_opts *o) {
    *o = hlmi_vq_merge_opts{};
    o->first_it = 1;
    o->keep_singletons = 300;             // max(min_overlap_len, min_read_len), pipeline_per_stage.py:170-203
    o->store_tips_separately = 1;
    o->min_clique_size = 2;
}

void vq_consensus_pair(const char *seq1, const char *qual1, uint32_t len1, uint32_t qlen1, const char *seq2, const char *qual2,
                       uint32_t len2, uint32_t qlen2, uint32_t pos, char *out_seq, char *out_qual, uint32_t *out_len) {
    *out_len = 0;
    check_read(seq1, len1, qual1, qlen1, "hlmi_vq_consensus_pair: sequence", 1);
    check_read(seq2, len2, qual2, qlen2, "hlmi_vq_consensus_pair: sequence", 2);
    const uint64_t total = std::max<uint64_t>(len1, (uint64_t)pos + len2);   // base + left + right extension (:224-252)
    if (total >= (1u << 30)) fail(HLMI_EINVAL, "hlmi_vq_consensus_pair: %llu bases", (unsigned long long)total);
    // SRBuilder::consensus (:453-521).  Read 1 is active from position 0 and meets :478 at once when it is empty, or at
    // position qlen1 when its quality string ends first; read 2 turns active at `pos` if the loop gets there (pos < total),
    // with the same two ends; between len1 and pos no read is active (:498).
    if (total == 0) return;
    if (len1 == 0 || qlen1 < len1) return;
    if (pos > len1) return;
    if (pos < total && (len2 == 0 || qlen2 < len2)) return;
    std::vector<std::string> seq{std::string(seq1, len1), std::string(seq2, len2)}, qual{std::string(qual1, len1), std::string(qual2, len2)};
    Rec r{};
    r.a = 0; r.b = len2 ? 1u : NONE; r.p = pos; r.len = (uint32_t)total; r.flags = F_CONS; r.id = 0;
    VqMergeDev dev(seq, qual, consensus_tables());
    std::vector<uint64_t> start;
    const std::string text = dev.write(std::vector<Rec>{r}, start);
    memcpy(out_seq, text.data() + 3, total);                                // "@0\n"
    memcpy(out_qual, text.data() + 3 + total + 3, total);
    *out_len = (uint32_t)total;
}

// hlmi_vq_merge (no == NULL) and hlmi_vq_iteration: one path.  With `no` the call goes on to findNextOverlaps, and reads
// subreads_in in front of the graph's first write: the iteration loop runs in place, its inputs under the names written here.
static void merge_and_next(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                           const hlmi_vq_merge_opts &mo, const hlmi_vq_next_opts *no, const char *out_dir, hlmi_vq_graph_stats *gst,
                           hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst) {
    *mst = hlmi_vq_merge_stats{};
    if (nst) *nst = hlmi_vq_next_stats{};
    if (!mo.first_it && !subreads_in) fail(HLMI_EINVAL, "vq_merge: first_it is off and there is no subreads file");
    std::map<uint64_t, Originals> dict;
    if (no && !mo.first_it) dict = read_subreads(subreads_in);
    VqGraphState g;
    vq_graph_run(fastq, overlaps, go, out_dir, gst, &g, no != nullptr);   // the graph and its files: one path for all entry points
    if (!g.built) return;                                        // ViralQuasispecies.cpp:282-291: nothing to be done
    const double t0 = now_ms();
    const uint32_t V = (uint32_t)g.seq.size();
    for (uint32_t v = 0; v < V; ++v) mst->bases_in += g.seq[v].size();       // (checked by vq_graph_run: vq_merge_check_reads)
    // original_ID_dict (buildOriginalsDict): first_it: every read is its own original at index 0, forward
    if (!no && !mo.first_it) dict = read_subreads(subreads_in);
    auto originals_of = [&](uint32_t v) -> Originals {
        if (mo.first_it) return Originals{{g.id[v], Orig{true, 0, (int)g.seq[v].size()}}};
        auto it = dict.find(g.id[v]);
        if (it == dict.end() || it->second.empty())
            fail(HLMI_EINVAL, "vq_merge: read %llu has no line in %s", (unsigned long long)g.id[v], subreads_in);
        return it->second;
    };

    VqMergeDev dev(g.seq, g.qual, consensus_tables());

    // getEdgesForMerging (GraphAlgos.cpp:112-148): vertices ascending; each free one takes its first free out-neighbour
    std::vector<uint8_t> taken(V, 0);
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    for (uint32_t u = 0; u < V; ++u) {
        if (taken[u]) continue;
        for (const VqEdge &e : g.out[u])
            if (!taken[e.v2]) {
                pairs.emplace_back(u, e.v2);
                taken[u] = taken[e.v2] = 1;
                break;
            }
    }
    mst->pairs = pairs.size();

    // constructSuperread per pair: placement, then the emptiness the lengths decide
    struct Placed { uint32_t base, other, first, second, p, len; };
    std::vector<Placed> placed;
    std::vector<Rec> cand;
    for (const auto &pr : pairs) {
        Placed P{};
        P.base = std::min(pr.first, pr.second);                  // the clique is sorted; the first single-end read is the base (:658-679)
        P.other = std::max(pr.first, pr.second);
        const VqEdge *edge = nullptr;                            // getEdgeInfo(base, other): base -> other if it exists, else other -> base
        for (const VqEdge &e : g.out[P.base]) if (e.v2 == P.other) { edge = &e; break; }
        if (!edge) for (const VqEdge &e : g.out[P.other]) if (e.v2 == P.base) { edge = &e; break; }
        if (!edge) fail(HLMI_EINVAL, "vq_merge: no edge between %u and %u", P.base, P.other);
        // sort_vertices (:87-148): the other read at +pos1 when the base is the edge's read 1, else at -pos1; shifted to
        // start at 0 (:248-252) either way the edge's read 1 comes first and its read 2 lies pos1 behind it
        P.first = edge->v1;
        P.second = edge->v2;
        if (edge->pos1 < 0) fail(HLMI_EINVAL, "vq_merge: edge %u -> %u at position %d", edge->v1, edge->v2, edge->pos1);
        P.p = (uint32_t)edge->pos1;
        const uint64_t la = g.seq[P.first].size(), lb = g.seq[P.second].size();
        const uint64_t total = std::max<uint64_t>(la, (uint64_t)P.p + lb);      // base + l_ext + r_ext (:224-252)
        if (total >= (1u << 30)) fail(HLMI_EINVAL, "vq_merge: a super-read of %llu bases", (unsigned long long)total);
        P.len = P.p > la ? 0u : (uint32_t)total;                 // a position without an active base: empty consensus (:498-501)
        placed.push_back(P);
        if (P.len) {
            Rec r{};
            r.a = P.first; r.b = P.second; r.p = P.p; r.len = P.len;
            r.flags = F_CONS | (g.orient[P.first] ? 0u : F_REV_A) | (g.orient[P.second] ? 0u : F_REV_B);
            cand.push_back(r);
        }
    }
    const std::vector<uint32_t> cand_n = dev.count_n(cand);      // first pass: the 'N's each super-read would hold
    const std::vector<uint32_t> read_n = dev.read_n_counts();

    // process_cliques (:998-1001): kept when the consensus is not empty and test_N_rate passes (Read.h:214-233)
    auto n_rate_ok = [](uint32_t n, uint32_t len) { return (double)n < 0.05 * (double)len; };
    std::vector<Rec> recs;
    std::vector<uint8_t> visited(V, 0);
    std::vector<int64_t> new_id(V, -1);
    std::vector<uint32_t> offset(V, 0);
    std::string subreads;
    size_t ci = 0;
    for (const Placed &P : placed) {
        if (!P.len) { ++mst->dropped_empty; continue; }
        const Rec &c = cand[ci];
        const uint32_t n = cand_n[ci++];
        if (!n_rate_ok(n, P.len)) { ++mst->dropped_n; continue; }
        Rec r = c;
        r.id = (uint32_t)recs.size();
        // calcSubreadInfo with trim_pos 0 (:536-595): index = position in the super-read; then :750-806 per clique vertex in
        // sorted order, an original already there stays
        Originals merged;
        const uint32_t order[2] = {P.base, P.other};
        for (uint32_t v : order) {
            const long idx1 = v == P.first ? 0 : (long)P.p;
            vq_originals_add(merged, originals_of(v), g.orient[v] != 0, mo.first_it != 0, idx1, (long)g.seq[v].size());
            visited[v] = 1;
            new_id[v] = r.id;
            offset[v] = (uint32_t)idx1;
        }
        subreads_line(subreads, r.id, merged);
        recs.push_back(r);
    }
    mst->merged = recs.size();

    // the unmerged reads (:1282-1372), dropped pairs among them
    std::vector<Rec> tips;
    for (uint32_t v = 0; v < V; ++v) {
        if (visited[v]) continue;
        const uint32_t len = (uint32_t)g.seq[v].size();
        if (len < mo.keep_singletons) { ++mst->short_reads; continue; }                  // :1286
        if (!n_rate_ok(read_n[v], len)) { ++mst->n_reads; continue; }                    // :1292
        const bool incl = go.ignore_inclusions && g.incl[v];
        if (incl || (g.tip[v] && mo.store_tips_separately)) {                            // :1298-1311: forward, as read
            Rec r{};
            r.a = v; r.b = NONE; r.len = len; r.id = (uint32_t)tips.size();
            tips.push_back(r);
            if (incl) ++mst->inclusion_reads; else ++mst->tip_reads;
            continue;
        }
        Rec r{};
        r.a = v; r.b = NONE; r.len = len; r.id = (uint32_t)recs.size();
        Originals o = originals_of(v);
        if (!g.orient[v]) {                                                              // :1337-1368: a forward copy of the reverse read
            r.flags = F_REV_A;
            vq_originals_mirror(o, (long)len);
            ++mst->trivial_reverse;
        }
        ++mst->trivial;
        new_id[v] = r.id;
        subreads_line(subreads, r.id, o);
        recs.push_back(r);
    }

    // one gather writes both FASTQ files' text: singles.fastq, then the tip records
    const size_t n_singles = recs.size();
    recs.insert(recs.end(), tips.begin(), tips.end());
    std::vector<uint64_t> start;
    const std::string text = dev.write(recs, start);
    const uint64_t cut = start[n_singles];
    mst->bytes_out = cut;
    write_file(join_path(out_dir, "singles.fastq"), text.data(), cut);                  // (the reference removes it first, :1245)
    write_file(join_path(out_dir, "subreads.txt"), subreads.data(), subreads.size());
    if (!tips.empty())                                                                   // writeTipsToFile APPENDS (:1391)
        write_file(join_path(out_dir, "removed_tip_sequences.fastq"), text.data() + cut, text.size() - cut, "ab");
    std::string map;
    for (uint32_t v = 0; v < V; ++v) {
        map += std::to_string(v); map += '\t'; map += std::to_string(new_id[v]); map += '\t';
        map += std::to_string(offset[v]); map += '\t'; map += g.orient[v] ? '+' : '-'; map += '\n';
    }
    write_file(join_path(out_dir, "superread_map.txt"), map.data(), map.size());
    mst->ms_merge = now_ms() - t0;
    if (no) {                                                    // ViralQuasispecies.cpp:449-479
        const double t1 = now_ms();
        VqNextTables t;
        t.ent.resize(V); t.in_sr = visited; t.off = offset; t.len.assign(V, 0);
        for (uint32_t v = 0; v < V; ++v) {
            t.ent[v] = new_id[v] < 0 ? vqn::NONE : (uint32_t)new_id[v];
            if (new_id[v] >= 0) t.len[v] = recs[(size_t)new_id[v]].len;
        }
        const std::string image = vq_next_run(g, t, go.edge_threshold, *no, nst);
        write_file(join_path(out_dir, "overlaps.txt"), image.data(), image.size());
        const std::string line = std::to_string(gst->vertices) + "\t" + std::to_string(gst->edges_final) + "\t" +
                                 std::to_string(nst->lines) + "\n";
        write_file(join_path(out_dir, "stats.txt"), line.data(), line.size(), "ab");
        nst->ms_next = now_ms() - t1;
    }
    ktimer_flush();
}

void vq_merge_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                  const hlmi_vq_merge_opts &mo, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst) {
    merge_and_next(fastq, overlaps, subreads_in, go, mo, nullptr, out_dir, gst, mst, nullptr);
}

void vq_next_opts_stageb(hlmi_vq_next_opts *o) { *o = hlmi_vq_next_opts{}; }

void vq_iteration_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                      const hlmi_vq_merge_opts &mo, const hlmi_vq_next_opts &no, const char *out_dir, hlmi_vq_graph_stats *gst,
                      hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst) {
    merge_and_next(fastq, overlaps, subreads_in, go, mo, &no, out_dir, gst, mst, nst);
}

}  // namespace hlmi
