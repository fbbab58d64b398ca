// vq_superread.cpp - what SRBuilder's two entry points share (tools/HaploConduct/src/SRBuilder.cpp): mergeAlongEdges
// (:1238-1384) and cliquesToSuperreads (:1031-1235) both build a super-read through constructSuperread (:654-870), and to it
// a merged pair is a clique of two.  Pure host code: nothing here touches the device or a file, or depends on the rest of
// the library but common.h's fail().  The drivers that put these pieces in sequence are in vq_superread_run.cpp.
// PARITY UNPINNED: the reference needs Boost and cannot be built here; tests/vq_{merge,clique}_model.py restate it.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "vq_internal.h"

namespace hlmi {

using namespace vqm;

// --min_qual (ViralQuasispecies.cpp:62 -> SRBuilder.h:89) lies in [0, 1]: 0 never writes an N for disagreement, 1 nearly always
void vq_check_min_qual(double min_qual, const char *step) {
    if (!(min_qual >= 0.0 && min_qual <= 1.0)) fail(HLMI_EINVAL, "%s: min_qual %g is outside 0 .. 1", step, min_qual);
}

// SRBuilder::consensus_pos (:297-402) in its own expression order.  -> (base << 8) | quality
uint16_t vq_consensus_pos(const char *nuc, const int *phred, int n, double min_qual) {
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
    if (n > 1 && (1 - p_incorrect) < min_qual) return n_out;               // :362-368
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

// The tables of vq_internal.h (vqm::T_*) for one minQual.  Every pair of (base, quality) is evaluated; the forms by class that
// fit LDS are kept only if the answer does not depend on which bases they are - it can, through the order of the four terms of
// total_prob - and the build fails otherwise (with glibc's libm it does not).  Two dependences are part of the reference and
// have codes of their own, both through the chain of :390-393 once minQual no longer turns the column into N:
//   3  two different bases whose scores are EQUAL (a + b == b + a: equal qualities): the one that comes first in A, T, C, G
//   4  neither of the two wins: a base of Q0 or Q1 is more likely wrong than right (p > 3/4, so p / 3 > 1 - p), and when that
//      holds for both the bases that were NOT read tie for the best score: the first of them in A, T, C, G
static int atcg_rank(int c) { return c == 0 ? 0 : c == 3 ? 1 : c == 1 ? 2 : 3; }      // c: A C G T = 0 .. 3
static char first_other(int c1, int c2) {
    for (int c : {0, 3, 1, 2})
        if (c != c1 && c != c2) return "ACGT"[c];
    return 0;
}

static std::vector<uint16_t> build_consensus_tables(double min_qual) {
    std::vector<uint16_t> t((size_t)T_ALL);
    const char B[6] = "ACGTN";
    for (int c = 0; c < 5; ++c)
        for (int q = 0; q < NQ; ++q) t[T_SINGLE + c * NQ + q] = vq_consensus_pos(&B[c], &q, 1, min_qual);
    auto pair = [&](int c1, int c2, int q1, int q2) {
        const char nuc[2] = {B[c1], B[c2]};
        const int ph[2] = {q1, q2};
        return vq_consensus_pos(nuc, ph, 2, min_qual);
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
            // per class: the quality byte (one for all pairs), whether every pair gives one act of 0 / 1 / 2, whether every pair
            // gives the earlier base of the chain
            int same_act = -1, diff_act = -1, same_q = -1, diff_q = -1;
            bool same_one = true, diff_one = true, diff_chain = true;
            for (int c1 = 0; c1 < 4; ++c1)
                for (int c2 = 0; c2 < 4; ++c2) {
                    const uint16_t f = pair(c1, c2, q1, q2);
                    const char b = (char)(f >> 8);
                    const int act = b == 'N' ? 0 : b == B[c1] ? 1 : (c1 != c2 && b == B[c2]) ? 2 : b == first_other(c1, c2) ? 4 : -1;
                    int &cls_act = c1 == c2 ? same_act : diff_act, &cls_q = c1 == c2 ? same_q : diff_q;
                    if (cls_q < 0) { cls_act = act; cls_q = f & 0xff; }
                    if (act != cls_act) (c1 == c2 ? same_one : diff_one) = false;
                    if (c1 != c2 && act != (atcg_rank(c1) < atcg_rank(c2) ? 1 : 2)) diff_chain = false;
                    if (act < 0 || (f & 0xff) != cls_q || !same_one || (!diff_one && !diff_chain))
                        fail(HLMI_EINVAL, "vq_merge: the consensus of %c/Q%d and %c/Q%d depends on the bases' identity: the tables "
                                          "by class do not hold on this libm", B[c1], q1, B[c2], q2);
                }
            t[T_SAME + q1 * NQ + q2] = (uint16_t)((same_act << 8) | same_q);
            t[T_DIFF + q1 * NQ + q2] = (uint16_t)(((diff_one ? diff_act : 3) << 8) | diff_q);
        }
    return t;
}

// built once per distinct value (the bit pattern of the double is the key) and kept: a run uses one value, a process a few
const std::vector<uint16_t> &vq_consensus_tables(double min_qual) {
    vq_check_min_qual(min_qual, "vq_merge");
    if (min_qual == 0.0) min_qual = 0.0;                                   // (-0.0 compares like 0.0 everywhere: one entry)
    uint64_t key;
    memcpy(&key, &min_qual, sizeof key);
    static std::mutex lock;
    static std::map<uint64_t, std::vector<uint16_t>> built;                // (a map: an entry never moves once it is there)
    std::lock_guard<std::mutex> hold(lock);
    auto it = built.find(key);
    if (it == built.end()) it = built.emplace(key, build_consensus_tables(min_qual)).first;
    return it->second;
}

void vq_check_read(const char *seq, size_t len, const char *qual, size_t qlen, const char *what, size_t k) {
    for (size_t i = 0; i < len; ++i) {
        const char c = seq[i];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N')
            fail(HLMI_EINVAL, "%s %zu: base 0x%02x at %zu is none of A C G T N (SRBuilder.cpp:344 asserts)", what, k, (unsigned char)c, i);
    }
    for (size_t i = 0; i < qlen; ++i)
        if (qual[i] < '!' || qual[i] > '~')
            fail(HLMI_EINVAL, "%s %zu: quality 0x%02x at %zu is outside '!' .. '~'", what, k, (unsigned char)qual[i], i);
}

void vq_merge_check_reads(const std::vector<std::string> &seq, const std::vector<std::string> &qual) {
    for (size_t v = 0; v < seq.size(); ++v) {
        if (qual[v].size() != seq[v].size())
            fail(HLMI_EINVAL, "vq_merge: read %zu has %zu bases and %zu qualities", v, seq[v].size(), qual[v].size());
        vq_check_read(seq[v].data(), seq[v].size(), qual[v].data(), qual[v].size(), "vq_merge: read", v);
    }
}

// ---- originals -----------------------------------------------------------------------------------------------------------------
std::map<uint64_t, VqOriginals> vq_parse_subreads(const std::string &data, const char *path) {
    std::map<uint64_t, VqOriginals> dict;
    size_t pos = 0;
    while (pos < data.size()) {
        size_t e = data.find('\n', pos);
        if (e == std::string::npos) e = data.size();
        const std::string line = data.substr(pos, e - pos);
        pos = e + 1;
        if (line.empty()) continue;
        size_t t = line.find('\t');
        const uint64_t id = strtoul(line.substr(0, t).c_str(), nullptr, 0);
        VqOriginals &o = dict[id];
        while (t != std::string::npos) {
            const size_t b = t + 1;
            t = line.find('\t', b);
            const std::string info = line.substr(b, t == std::string::npos ? std::string::npos : t - b);
            if (info.empty()) continue;
            std::vector<std::string> f;
            size_t s = 0;
            for (size_t i = 0; i <= info.size(); ++i)
                if (i == info.size() || info[i] == ':' || info[i] == ',') {
                    if (i > s) f.push_back(info.substr(s, i - s));          // (token_compress_on)
                    s = i + 1;
                }
            if (f.size() == 6) fail(HLMI_ESTATE, "vq_merge: %s holds a paired-end original (%s); HyLight builds none", path, info.c_str());
            if (f.size() != 4) fail(HLMI_EINVAL, "vq_merge: %s: bad entry '%s'", path, info.c_str());
            VqOrig oi;
            oi.forward = f[1] == "+";
            oi.index = strtol(f[2].c_str(), nullptr, 10);
            oi.len = atoi(f[3].c_str());
            o.emplace(strtoul(f[0].c_str(), nullptr, 0), oi);               // (insert: the first entry of an id stays)
        }
    }
    return dict;
}

void vq_subreads_line(std::string &s, uint64_t id, const VqOriginals &o) {
    s += std::to_string(id);
    for (const auto &kv : o) {
        s += '\t'; s += std::to_string(kv.first); s += ':'; s += kv.second.forward ? '+' : '-'; s += ':';
        s += std::to_string(kv.second.index); s += ':'; s += std::to_string(kv.second.len);
    }
    s += '\n';
}

void vq_originals_add(VqOriginals &merged, const VqOriginals &of_read, bool forward, bool first_it, long idx1, long read_len) {
    for (const auto &kv : of_read) {
        if (merged.count(kv.first)) continue;                              // already inserted by another vertex (:762-764)
        VqOrig oi = kv.second;
        oi.forward = oi.forward == forward;
        if (first_it) oi.index = idx1;
        else if (forward) oi.index += idx1;
        else oi.index = read_len + idx1 - (oi.len + oi.index);
        merged.emplace(kv.first, oi);
    }
}

void vq_originals_mirror(VqOriginals &o, long read_len) {
    for (auto &kv : o) {
        kv.second.forward = !kv.second.forward;
        kv.second.index = read_len - (kv.second.index + kv.second.len);
    }
}

VqOriginalsDict::VqOriginalsDict(const char *step, bool first_it, const char *subreads_in)
    : step(step), subreads_in(subreads_in), first_it(first_it) {
    if (!first_it && !subreads_in) fail(HLMI_EINVAL, "%s: first_it is off and there is no subreads file", step);
}

VqOriginals VqOriginalsDict::originals_of(const VqGraphState &g, uint32_t v) const {
    if (first_it) return VqOriginals{{g.id[v], VqOrig{true, 0, (int)g.seq[v].size()}}};
    auto it = dict.find(g.id[v]);
    if (it == dict.end() || it->second.empty())
        fail(HLMI_EINVAL, "%s: read %llu has no line in %s", step, (unsigned long long)g.id[v], subreads_in);
    return it->second;
}

// ---- constructSuperread: the placement -------------------------------------------------------------------------------------------
const VqEdge *vq_edge_info(const VqGraphState &g, uint32_t u, uint32_t v) {
    for (const VqEdge &e : g.out[u])
        if (e.v2 == v) return &e;
    for (const VqEdge &e : g.out[v])
        if (e.v2 == u) return &e;
    return nullptr;
}

int64_t vq_place(const VqGraphState &g, const std::vector<uint32_t> &clique, const char *step, VqPlaced &order) {
    const uint32_t base = clique[0];             // single-end reads: the first one is the base (:670-679)
    const int64_t base_len = (int64_t)g.seq[base].size();
    int64_t l_ext = 0, r_ext = 0;
    order.assign(1, std::make_pair((int64_t)0, base));
    for (uint32_t v : clique) {
        if (v == base) continue;
        const VqEdge *e = vq_edge_info(g, base, v);
        if (!e) fail(HLMI_EINVAL, "%s: no edge between %u and %u", step, base, v);
        const int64_t new_pos = e->v1 == base ? (int64_t)e->pos1 : -(int64_t)e->pos1;     // :142-147
        size_t at = 0;                           // in front of the first entry that is not smaller (:212-222)
        while (at < order.size() && order[at].first < new_pos) ++at;
        order.insert(order.begin() + (ptrdiff_t)at, std::make_pair(new_pos, v));
        l_ext = std::max(l_ext, -new_pos);                                 // :236-240
        r_ext = std::max(r_ext, (int64_t)g.seq[v].size() + new_pos - base_len);
    }
    const int64_t total = base_len + l_ext + r_ext;
    if (total >= (1 << 30)) fail(HLMI_EINVAL, "%s: a super-read of %lld bases", step, (long long)total);
    const int64_t shift = order[0].first < 0 ? -order[0].first : 0;        // :248-252
    for (auto &pv : order) pv.first += shift;
    return total;
}

VqPlaced vq_filter_subreads(const VqGraphState &g, size_t num, uint32_t base, const VqPlaced &order) {
    std::unordered_map<uint32_t, bool> sel;
    for (size_t i = 0; i < num / 2; ++i) sel[order[i].second] = true;
    sel[base] = true;
    std::vector<std::pair<uint32_t, int>> by_end;                          // sortVerticesByEndpos (:639-652): the same std::sort
    for (const auto &pv : order) by_end.emplace_back(pv.second, (int)(pv.first + (int64_t)g.seq[pv.second].size()));
    std::sort(by_end.begin(), by_end.end(), [](const std::pair<uint32_t, int> &a, const std::pair<uint32_t, int> &b) { return a.second < b.second; });
    for (size_t i = by_end.size(); i > 0 && sel.size() < num; --i) sel[by_end[i - 1].first] = true;
    VqPlaced used;
    for (const auto &pv : order) if (sel.count(pv.second)) used.push_back(pv);
    return used;
}

uint16_t vq_consensus_column(const VqGraphState &g, const vqc::Entry *entries, uint32_t n_entries, uint32_t column, double min_qual) {
    std::vector<char> nuc(n_entries);
    std::vector<int> phred(n_entries);
    int n = 0;
    for (uint32_t k = 0; k < n_entries; ++k) {
        const vqc::Entry &e = entries[k];
        const std::string &s = g.seq[e.read], &ql = g.qual[e.read];
        if (column < e.pos || column - e.pos >= s.size()) continue;
        const size_t i = column - e.pos;
        char ch = e.rev ? s[s.size() - 1 - i] : s[i];
        if (e.rev) ch = ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch;
        nuc[n] = ch;
        phred[n++] = (e.rev ? ql[s.size() - 1 - i] : ql[i]) - 33;
    }
    return vq_consensus_pos(nuc.data(), phred.data(), n, min_qual);
}

bool vq_n_rate_ok(uint64_t n, uint64_t len) { return (double)n < 0.05 * (double)len; }

VqLoneCounts vq_lone_reads(const VqGraphState &g, const VqOriginalsDict &dict, const std::vector<uint8_t> &visited,
                           const std::vector<uint32_t> &read_n, uint32_t keep_singletons, const std::vector<uint8_t> *divert,
                           uint32_t first_id, std::vector<vqm::Rec> &recs, std::string &subreads, std::vector<uint32_t> *diverted) {
    VqLoneCounts c;
    uint32_t id = first_id;
    for (uint32_t v = 0; v < (uint32_t)g.seq.size(); ++v) {
        if (visited[v]) continue;
        const uint32_t len = (uint32_t)g.seq[v].size();
        if (len < keep_singletons) { ++c.short_reads; continue; }                        // :1149, :1286
        if (!vq_n_rate_ok(read_n[v], len)) { ++c.n_reads; continue; }                    // :1155, :1292
        if (divert && (*divert)[v]) { diverted->push_back(v); continue; }                // :1298-1311
        Rec r{};
        r.a = v; r.b = NONE; r.len = len; r.id = id;
        VqOriginals o = dict.originals_of(g, v);
        if (!g.orient[v]) {                      // :1186-1217, :1337-1368: a forward copy of the reverse read
            r.flags = F_REV_A;
            vq_originals_mirror(o, (long)len);
            ++c.trivial_reverse;
        }
        ++c.trivial;
        vq_subreads_line(subreads, id, o);
        recs.push_back(r);
        ++id;
    }
    return c;
}

// nodes_to_SR, nodes_to_new_IDs and findCliqueIndex as tables (FindNextOverlaps.cpp:896-913, :331-347, SRBuilder.cpp:1219): one
// counting pass over the members, which come super-read after super-read in ascending id, so every list is ascending too
VqNextTables vq_next_tables(uint32_t n_vertices, const std::vector<VqMember> &members, size_t n_superreads,
                            const std::vector<uint32_t> &superread_len, const std::vector<vqm::Rec> &lone) {
    if (superread_len.size() != n_superreads) fail(HLMI_EINVAL, "vq_next: %zu lengths for %zu super-reads", superread_len.size(), n_superreads);
    VqNextTables t;
    t.start.assign((size_t)n_vertices + 1, 0);
    t.copied.assign(n_vertices, 0);
    t.len = superread_len;
    t.len.resize(n_superreads + lone.size(), 0);
    for (const VqMember &m : members) {
        if (m.vertex >= n_vertices || m.id >= n_superreads)
            fail(HLMI_EINVAL, "vq_next: member %u of super-read %u (%u vertices, %zu super-reads)", m.vertex, m.id, n_vertices, n_superreads);
        ++t.start[m.vertex + 1];
    }
    for (const vqm::Rec &r : lone) {             // an unvisited read that was copied: a list of one, itself at 0
        if (r.a >= n_vertices || r.id < n_superreads || r.id >= t.len.size() || t.start[r.a + 1] || t.len[r.id])
            fail(HLMI_EINVAL, "vq_next: copied read %u as new read %u", r.a, r.id);
        t.start[r.a + 1] = 1;
        t.copied[r.a] = 1;
        t.len[r.id] = r.len;
    }
    for (uint32_t v = 0; v < n_vertices; ++v) t.start[v + 1] += t.start[v];
    t.id.assign(t.start[n_vertices], 0);
    t.idx.assign(t.start[n_vertices], 0);
    std::vector<uint32_t> fill(t.start.begin(), t.start.end() - 1);
    for (const VqMember &m : members) { t.id[fill[m.vertex]] = m.id; t.idx[fill[m.vertex]++] = m.idx; }
    for (const vqm::Rec &r : lone) t.id[fill[r.a]] = r.id;
    return t;
}

void vq_next_tables_check(const VqNextTables &t, uint32_t n_vertices) {
    bool ok = t.start.size() == (size_t)n_vertices + 1 && t.copied.size() == n_vertices && t.start[0] == 0 && t.id.size() == t.idx.size() &&
              t.id.size() < (1ull << 32);
    for (uint32_t v = 0; ok && v < n_vertices; ++v)
        ok = t.start[v] <= t.start[v + 1] && (!t.copied[v] || t.start[v + 1] - t.start[v] == 1);
    ok = ok && t.start[n_vertices] == t.id.size();
    for (size_t k = 0; ok && k < t.id.size(); ++k) ok = t.id[k] < t.len.size();
    if (!ok) fail(HLMI_EINVAL, "vq_next: the tables do not cover the %u vertices", n_vertices);
}

}  // namespace hlmi
