// vq_branch_host.cpp - BranchReduction::readBasedBranchReduction (tools/HaploConduct/src/BranchReduction.cpp) behind
// hlmi_vq_branch_graph / hlmi_vq_branch_iteration: ViralQuasispecies --branch_reduction=true --remove_branches=false
// --remove_trans=1 --threads 1, single-end vertices, diploid off.  The two base-comparison steps run on the device
// (vq_branch.hip); this file holds what is order-dependent and small: the branches, the difference lists, the components, the
// unique evidence, the thresholds and the list of edges to remove.  The text is restated literally, oddities included.
// PARITY UNPINNED: the reference needs Boost and cannot be built here; tests/vq_branch_model.py restates it.
//
// One result depends on container order: branch_in_map / branch_out_map (:755-756) are std::unordered_map<node_id_t, ..> filled
// in ascending vertex order and then iterated (:784, :882).  The start vertex of a component fixes its dist, and under `careful`
// the component order fixes which components survive.  This file uses the same container with the same insert sequence, so it
// equals a reference built with the same libstdc++.
//
// Two readings, stated: --original_readcount is se_count + 2 * pe_count; original_ID_dict.at(node) is read with the vertex's
// read id, and read ids that are not the file positions are refused (every file this project writes numbers its reads from 0).
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <set>
#include <unordered_map>
#include <unordered_set>

#include "paf_io.h"
#include "vq_internal.h"

namespace hlmi {

using namespace vqb;

void vq_branch_opts_polyte(hlmi_vq_branch_opts *o) {
    *o = hlmi_vq_branch_opts{};
    o->careful = 1;
}

namespace {

// std::stoi: leading blanks, a sign, digits; what follows is ignored
int stoi_like(const std::string &s, const char *path) {
    size_t k = 0;
    while (k < s.size() && isspace((unsigned char)s[k])) ++k;
    size_t d = k;
    if (d < s.size() && (s[d] == '+' || s[d] == '-')) ++d;
    if (d >= s.size() || !isdigit((unsigned char)s[d])) fail(HLMI_EINVAL, "vq_branch: %s: '%s' is no number", path, s.c_str());
    errno = 0;
    const long v = strtol(s.c_str() + k, nullptr, 10);
    if (errno || v < INT32_MIN || v > INT32_MAX) fail(HLMI_EINVAL, "vq_branch: %s: '%s' is out of range", path, s.c_str());
    return (int)v;
}

// :132-159: '#' and empty lines skipped, column 1 = dist, column 3 = min evidence.  The reference pushes every line into ONE
// stringstream and clear() resets its flags only: what a line holds behind its third tab stays unread and goes in front of the
// next line's first column ("300\t1\t2\textra" then "100\t..": std::stoi("extra100") throws - refused here).
std::map<int, int> read_table(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) fail(HLMI_EINVAL, "vq_branch: unable to open the evidence threshold table %s", path);
    fclose(f);
    const std::string data = read_file(path);
    std::map<int, int> table;
    std::string carry;
    size_t pos = 0;
    while (pos < data.size()) {
        size_t e = data.find('\n', pos);
        if (e == std::string::npos) e = data.size();
        std::string line = data.substr(pos, e - pos);
        pos = e + 1;
        if (line.empty() || line[0] == '#') continue;
        line = carry + line;
        carry.clear();
        std::string col[3];
        size_t b = 0;
        for (int c = 0; c < 3; ++c) {                 // getline at the end of the stream leaves tmp as it was
            if (b > line.size()) { col[c] = col[c - 1]; continue; }
            size_t t = line.find('\t', b);
            if (t == std::string::npos) t = line.size();
            col[c] = line.substr(b, t - b);
            b = t + 1;
        }
        if (b <= line.size()) carry = line.substr(b);     // behind the third tab: unread, in front of the next line
        const int dist = stoi_like(col[0], path);
        table[dist] = stoi_like(col[2], path);
    }
    return table;
}

using Originals = std::vector<VqOriginals>;       // per vertex

struct Reduction {
    const hlmi_vq_graph_opts &o;
    const VqBranchRun &run;
    const std::vector<std::string> &seq;
    const std::vector<std::vector<VqEdge>> &out;
    const std::vector<uint8_t> &orient;
    Originals originals;
    hlmi_vq_branch_stats &st;
    uint32_t V;

    struct Branch {
        uint32_t node;
        bool outbranch;
        std::vector<uint32_t> nbs;
        std::vector<const VqEdge *> edges;
        std::vector<int> start, pos_vec;
        struct Cmp { uint32_t i, j; int rel, len, startpos; int64_t pair; };     // pair < 0: decided by the lengths
        std::vector<Cmp> cmps;
        std::vector<int32_t> diff;                // sorted, uniqued
        int dist = 0;
        std::vector<std::pair<uint32_t, uint32_t>> inclusions;
        uint32_t slot0 = 0;
    };
    std::vector<Branch> branches;
    std::vector<Pair> pairs;
    std::vector<VqEdge> missing;
    std::unordered_set<uint32_t> false_in, false_out;
    std::unordered_map<uint64_t, std::list<uint32_t>> evidence;                  // evidence_per_edge
    std::vector<std::pair<std::vector<std::pair<uint32_t, uint32_t>>, int>> components;

    const VqEdge *edge(uint32_t u, uint32_t v) const {                          // getEdgeInfo(u, v, false)
        for (const VqEdge &e : out[u]) if (e.v2 == v) return &e;
        fail(HLMI_EINVAL, "vq_branch: no edge %u -> %u", u, v);
    }
    uint64_t key(uint32_t u, uint32_t v) const { return (uint64_t)u * V + v; }   // edgeToEvidenceIndex

    // buildDiffListOut / buildDiffListIn up to the comparisons (:396-470, :537-624): who is compared with whom, and where
    void plan(Branch &b) {
        const size_t n = b.nbs.size();
        for (uint32_t v : b.nbs) {
            const VqEdge *e = b.outbranch ? edge(b.node, v) : edge(v, b.node);
            b.edges.push_back(e);
            (b.outbranch ? b.start : b.pos_vec).push_back(e->pos1);
        }
        if (!b.outbranch) {
            const int max_pos = *std::max_element(b.pos_vec.begin(), b.pos_vec.end());
            for (int p : b.pos_vec) b.start.push_back(max_pos - p);             // startpos = max_pos - pos
        }
        const uint32_t flags = (orient[b.node] ? 0u : 1u) | (b.outbranch ? 0u : 2u);   // oriented by the BRANCHING vertex's label
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = i + 1; j < n; ++j) {
                const int pi = b.start[i], pj = b.start[j];
                const uint32_t a = pi < pj ? i : j, c = pi < pj ? j : i;        // a starts first
                const int rel = pi < pj ? pj - pi : pi - pj, startpos = pi < pj ? pj : pi;
                const size_t size_a = seq[b.nbs[a]].size(), size_c = seq[b.nbs[c]].size();
                // :449 / :461: relative_pos > int(size - min_overlap_len), the subtraction in size_t
                if (rel > (int)(uint32_t)(size_a - (size_t)o.min_overlap_len)) {
                    if (!b.outbranch)
                        fail(HLMI_EINVAL, "vq_branch: in-branch %u holds an inclusion pair (%u, %u): the reference asserts (:605)", b.node,
                             b.nbs[a], b.nbs[c]);
                    b.inclusions.emplace_back(b.nbs[a], b.nbs[c]);
                    b.cmps.push_back(Branch::Cmp{i, j, rel, 0, startpos, -1});
                    ++st.inclusion_pairs;
                    continue;
                }
                if ((size_t)rel >= size_a) fail(HLMI_EINVAL, "vq_branch: branch %u: position %d behind the end of read %u", b.node, rel, b.nbs[a]);
                const int len = (int)std::min(size_a - (size_t)rel, size_c);
                b.cmps.push_back(Branch::Cmp{i, j, rel, len, startpos, (int64_t)pairs.size()});
                pairs.push_back(Pair{b.nbs[a], b.nbs[c], (uint32_t)rel, (uint32_t)len, flags});
            }
    }

    // the rest of buildDiffList* (:471-534, :625-688) over what the device found
    void finish_diff(Branch &b, const std::vector<uint32_t> &cnt, const std::vector<uint32_t> &pos) {
        std::vector<int> distance;
        const int node1_len = (int)seq[b.node].size();
        for (const Branch::Cmp &c : b.cmps) {
            if (c.pair < 0) continue;
            const uint32_t n = cnt[(size_t)c.pair];
            const uint32_t *dp = pos.data() + (size_t)c.pair * MAX_DIFF;
            st.diff_positions += n;
            for (uint32_t k = 0; k < n; ++k)
                b.diff.push_back(b.outbranch ? (int)dp[k] + c.startpos : c.len - (int)dp[k] + c.startpos);
            const uint32_t i = c.i, j = c.j;
            if (n == 0) {                             // identical overlap: a missing edge, and the branch is false
                const int pi = b.start[i], pj = b.start[j];
                const bool i_first = pi < pj || (pi == pj && b.nbs[i] < b.nbs[j]);
                const uint32_t f = i_first ? i : j, s = i_first ? j : i;
                VqEdge e{};
                e.v1 = b.nbs[f]; e.v2 = b.nbs[s];
                e.pos1 = c.rel; e.pos2 = 0;
                e.ori1 = b.outbranch ? b.edges[f]->ori2 : b.edges[f]->ori1;
                e.ori2 = b.outbranch ? b.edges[s]->ori2 : b.edges[s]->ori1;
                e.len = c.len;
                e.perc = (int32_t)((size_t)(100 * c.len) / std::min(seq[b.nbs[i]].size(), seq[b.nbs[j]].size()));
                e.score = o.edge_threshold;
                e.pad[0] = (uint8_t)'-';
                missing.push_back(e);
                (b.outbranch ? false_out : false_in).insert(b.node);
            } else if (i == 0) {                      // distance_vec is fed by the first neighbour's pairs alone
                if (b.outbranch) distance.push_back((int)dp[0] + c.startpos);
                else {
                    const int overlap_len = (int)std::min(seq[b.nbs[i]].size() - (size_t)b.pos_vec[i], seq[b.nbs[j]].size() - (size_t)b.pos_vec[j]);
                    distance.push_back((int)dp[0] + node1_len - overlap_len);
                }
            }
        }
        if (!distance.empty())
            b.dist = (int)(0.5 * (*std::min_element(distance.begin(), distance.end()) + *std::max_element(distance.begin(), distance.end())));
        std::sort(b.diff.begin(), b.diff.end());
        b.diff.erase(std::unique(b.diff.begin(), b.diff.end()), b.diff.end());
    }

    // findBranchingEvidence behind the evidence lists (:327-393) -> final_branch
    std::list<uint32_t> store(const Branch &b, std::vector<std::list<uint32_t>> &per_nb) {
        std::list<uint32_t> final_branch(b.nbs.begin(), b.nbs.end());
        final_branch.push_front(b.node);
        for (const auto &pr : b.inclusions) {
            for (size_t k = 0; k < b.nbs.size(); ++k) if (b.nbs[k] == pr.first) per_nb[k].clear();
            if (b.nbs.size() == 2) final_branch.clear();
            else final_branch.remove(pr.first);
        }
        if (final_branch.empty()) return final_branch;
        auto it = std::next(final_branch.begin());
        for (size_t k = 0; k < b.nbs.size(); ++k) {
            if (it == final_branch.end() || b.nbs[k] != *it) continue;
            const uint64_t idx = b.outbranch ? key(b.node, b.nbs[k]) : key(b.nbs[k], b.node);
            auto ev = evidence.find(idx);
            if (ev != evidence.end()) {               // a second visit intersects, in the existing list's order
                std::list<uint32_t> both;
                for (uint32_t x : ev->second)
                    if (std::find(per_nb[k].begin(), per_nb[k].end(), x) != per_nb[k].end()) both.push_back(x);
                ev->second = both;
            } else {
                evidence.emplace(idx, per_nb[k]);
            }
            ++it;
        }
        return final_branch;
    }

    // ---- findBranchingComponents (:745-1007) ------------------------------------------------------------------------------
    using Comp = std::vector<std::pair<uint32_t, uint32_t>>;
    struct Maps {
        std::unordered_map<uint32_t, bool> seen_in, seen_out;
        std::unordered_map<uint32_t, std::list<uint32_t>> in_map, out_map;
        std::unordered_map<uint32_t, int> in_dist, out_dist;
    };
    std::pair<int, uint32_t> extend_out(Comp &comp, const std::list<uint32_t> &nbs, bool &has_false, Maps &m) {
        std::pair<int, uint32_t> r(0, nbs.front());
        bool extended = false;
        for (uint32_t node : nbs) {
            auto seen = m.seen_out.find(node);
            if (seen == m.seen_out.end() || seen->second) continue;
            if (false_out.count(node)) has_false = true;
            const std::list<uint32_t> branch = m.out_map.at(node);
            r = std::make_pair(m.out_dist.at(node), node);
            extended = true;
            for (uint32_t w : branch) comp.emplace_back(node, w);
            m.seen_out.at(node) = true;
            extend_in(comp, branch, has_false, m);
        }
        if (!extended) r = std::make_pair(0, nbs.front());
        return r;
    }
    void extend_in(Comp &comp, const std::list<uint32_t> &nbs, bool &has_false, Maps &m) {
        for (uint32_t node : nbs) {
            auto seen = m.seen_in.find(node);
            if (seen == m.seen_in.end() || seen->second) continue;
            if (false_in.count(node)) has_false = true;
            const std::list<uint32_t> branch = m.in_map.at(node);
            for (uint32_t w : branch) comp.emplace_back(w, node);
            m.seen_in.at(node) = true;
            extend_out(comp, branch, has_false, m);
        }
    }
    void find_components(const std::vector<std::pair<std::list<uint32_t>, int>> &final_in,
                         const std::vector<std::pair<std::list<uint32_t>, int>> &final_out, std::list<std::pair<uint32_t, uint32_t>> &to_remove) {
        Maps m;
        auto fill = [](const std::vector<std::pair<std::list<uint32_t>, int>> &fin, std::unordered_map<uint32_t, bool> &seen,
                       std::unordered_map<uint32_t, std::list<uint32_t>> &map, std::unordered_map<uint32_t, int> &dist) {
            for (const auto &info : fin) {
                std::list<uint32_t> branch = info.first;
                if (branch.empty()) continue;
                const uint32_t node = branch.front();
                branch.pop_front();
                seen.insert(std::make_pair(node, false));
                map.insert(std::make_pair(node, branch));
                dist.insert(std::make_pair(node, info.second));
            }
        };
        fill(final_in, m.seen_in, m.in_map, m.in_dist);
        fill(final_out, m.seen_out, m.out_map, m.out_dist);
        for (const auto &branch : m.in_map) {         // unordered_map order: see the head of this file
            const uint32_t node = branch.first;
            if (m.seen_in.at(node)) continue;
            const std::list<uint32_t> nbs = branch.second;
            Comp comp;
            bool has_false = false_in.count(node) != 0;
            for (uint32_t w : nbs) comp.emplace_back(w, node);
            m.seen_in.at(node) = true;
            int dist1 = m.in_dist.at(node);
            const std::pair<int, uint32_t> dn = extend_out(comp, nbs, has_false, m);
            int dist2 = dn.first;
            const uint32_t outnode = dn.second;
            const VqEdge *e = edge(outnode, node);
            const int len1 = (int)seq[outnode].size(), len2 = (int)seq[node].size(), overlap_len = e->len;
            if (overlap_len < 100) {
                if (dist1 < len2 - overlap_len + 100) dist1 = len2 - overlap_len + 100;
                if (dist2 < len1 - overlap_len + 100) dist2 = len1 - overlap_len + 100;
            } else {
                if (dist1 < len2) dist1 = len2;
                if (dist2 < len1) dist2 = len1;
            }
            const int dist = dist1 + dist2 - len1 - len2 + overlap_len;
            std::sort(comp.begin(), comp.end());
            comp.erase(std::unique(comp.begin(), comp.end()), comp.end());
            if (has_false) to_remove.insert(to_remove.end(), comp.begin(), comp.end());
            else components.emplace_back(comp, dist);
        }
        for (const auto &branch : m.out_map) {        // the out-branches no in-branch reached: trivial components
            const uint32_t node = branch.first;
            if (m.seen_out.at(node)) continue;
            const std::list<uint32_t> nbs = branch.second;
            Comp comp;
            for (uint32_t w : nbs) comp.emplace_back(node, w);
            int dist1 = m.out_dist.at(node), dist2;
            const VqEdge *e = edge(node, nbs.front());
            const int len1 = (int)seq[node].size(), len2 = (int)seq[nbs.front()].size(), overlap_len = e->len;
            if (overlap_len < 100) {
                if (dist1 < len1 - overlap_len + 100) dist1 = len1 - overlap_len + 100;
                dist2 = len2 - overlap_len + 100;
            } else {
                if (dist1 < len1) dist1 = len1;
                dist2 = len2;
            }
            const int dist = dist1 + dist2 - len1 - len2 + overlap_len;
            if (false_out.count(node)) to_remove.insert(to_remove.end(), comp.begin(), comp.end());
            else components.emplace_back(comp, dist);
            m.seen_out.at(node) = true;
        }
    }

    // countUniqueEvidence (:1009-1272), diploid off: a k-way comparison of the lists' fronts; only a strictly unique minimum
    // counts.  The reference collects the unique evidence in an unordered_map and walks it to fill edges_to_remove: that order
    // reaches nothing, because edges_to_remove is sorted and uniqued before use and, with diploid off, nothing else reads it.
    bool count_unique(const Comp &comp, int min_evidence, std::list<std::pair<uint32_t, uint32_t>> &to_remove, std::vector<int> &counts) {
        const size_t n = comp.size();
        std::vector<std::list<uint32_t> *> ev(n);
        std::vector<uint8_t> live(n);
        std::vector<std::vector<uint32_t>> unique(n);
        for (size_t k = 0; k < n; ++k) {
            auto it = evidence.find(key(comp[k].first, comp[k].second));
            if (it == evidence.end()) fail(HLMI_EINVAL, "vq_branch: no evidence list for edge %u -> %u", comp[k].first, comp[k].second);
            ev[k] = &it->second;
            live[k] = !it->second.empty();
        }
        std::vector<uint32_t> fronts;
        while (*std::max_element(live.begin(), live.end()) == 1) {
            fronts.clear();
            for (size_t k = 0; k < n; ++k) if (live[k]) fronts.push_back(ev[k]->front());
            std::sort(fronts.begin(), fronts.end());
            const uint32_t cur = fronts.front();
            const bool unique_min = fronts.size() == 1 || cur < fronts[1];
            for (size_t k = 0; k < n; ++k)
                if (live[k] && ev[k]->front() == cur) {
                    if (unique_min) unique[k].push_back(cur);
                    ev[k]->pop_front();
                    if (ev[k]->empty()) live[k] = 0;
                }
        }
        bool keep = false;
        counts.assign(n, 0);
        for (size_t k = 0; k < n; ++k) {
            std::sort(unique[k].begin(), unique[k].end());
            counts[k] = (int)(std::unique(unique[k].begin(), unique[k].end()) - unique[k].begin());
            if (counts[k] < min_evidence) to_remove.push_back(comp[k]);
            else keep = true;
        }
        return keep;
    }

    // readBasedBranchReduction (:41-227)
    void reduce(std::vector<std::pair<uint32_t, uint32_t>> &removed, std::string &report) {
        const double t0 = now_ms();
        std::vector<std::vector<uint32_t>> ins(V);                              // sortAdjLists(adj_in): sources ascending
        for (uint32_t u = 0; u < V; ++u)
            for (const VqEdge &e : out[u]) ins[e.v2].push_back(u);
        for (uint32_t v = 0; v < V; ++v)                                        // in-branches first, ascending; then out-branches
            if (ins[v].size() > 1) { branches.push_back(Branch{v, false, ins[v]}); ++st.in_branches; }
        for (uint32_t u = 0; u < V; ++u)
            if (out[u].size() > 1) {
                Branch b{u, true};
                for (const VqEdge &e : out[u]) b.nbs.push_back(e.v2);
                branches.push_back(std::move(b));
                ++st.out_branches;
            }
        for (Branch &b : branches) plan(b);
        st.pairs = pairs.size();
        if (branches.empty()) { st.ms_branch = now_ms() - t0; return; }

        Dev dev(seq, run.originals.seq);
        std::vector<uint32_t> cnt, pos;
        for (const Pair &p : pairs)                   // what the kernel indexes with, once more
            if (p.a >= V || p.b >= V || !p.len || (size_t)p.rel + p.len > seq[p.a].size() || p.len > seq[p.b].size())
                fail(HLMI_EINVAL, "vq_branch: a pair outside its reads");
        dev.diff_positions(pairs, cnt, pos);
        sync();
        st.ms_diff = now_ms() - t0;
        for (Branch &b : branches) finish_diff(b, cnt, pos);

        // the originals as a CSR, the slots, the items
        const double t1 = now_ms();
        std::vector<uint32_t> ooff((size_t)V + 1, 0), oid, orow, item0;
        std::vector<uint8_t> ofwd;
        std::vector<int32_t> oidx, diff;
        for (uint32_t v = 0; v < V; ++v) {
            for (const auto &kv : originals[v]) {
                oid.push_back((uint32_t)kv.first);
                orow.push_back(run.originals.index_of.at(kv.first));
                ofwd.push_back(kv.second.forward);
                oidx.push_back((int32_t)kv.second.index);
            }
            ooff[v + 1] = (uint32_t)oid.size();
        }
        std::vector<Slot> slots;
        item0.push_back(0);
        for (Branch &b : branches) {
            const uint32_t d0 = (uint32_t)diff.size();
            diff.insert(diff.end(), b.diff.begin(), b.diff.end());
            b.slot0 = (uint32_t)slots.size();
            for (size_t k = 0; k < b.nbs.size(); ++k) {
                slots.push_back(Slot{b.node, b.nbs[k], b.start[k], orient[b.node] ? 0u : 1u, d0, (uint32_t)diff.size()});
                const uint64_t next = (uint64_t)item0.back() + (ooff[b.nbs[k] + 1] - ooff[b.nbs[k]]);
                if (next >= (1ull << 31)) fail(HLMI_EINVAL, "vq_branch: 2^31 evidence items and more");
                item0.push_back((uint32_t)next);
            }
        }
        st.work_items = item0.back();
        std::vector<uint32_t> ev;
        dev.evidence(slots, item0, diff, ooff, oid, orow, ofwd, oidx, run.bo.se_count, run.bo.pe_count, ev);
        sync();
        st.ms_evidence = now_ms() - t1;

        std::vector<std::pair<std::list<uint32_t>, int>> final_in(V), final_out(V);
        for (const Branch &b : branches) {
            std::vector<std::list<uint32_t>> per_nb(b.nbs.size());
            for (size_t k = 0; k < b.nbs.size(); ++k) {
                std::vector<uint32_t> ids;
                for (size_t t = 2 * (size_t)item0[b.slot0 + k]; t < 2 * (size_t)item0[b.slot0 + k + 1]; ++t)
                    if (ev[t] != NONE) ids.push_back(ev[t]);
                std::sort(ids.begin(), ids.end());                              // evidence_list.sort(); unique()
                ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
                st.evidence_ids += ids.size();
                per_nb[k].assign(ids.begin(), ids.end());
            }
            std::list<uint32_t> fb = store(b, per_nb);
            if (!fb.empty()) (b.outbranch ? final_out : final_in)[b.node] = std::make_pair(fb, b.dist);
        }
        st.missing_edges = missing.size();
        st.false_branches = false_in.size() + false_out.size();

        std::list<std::pair<uint32_t, uint32_t>> to_remove;
        find_components(final_in, final_out, to_remove);
        st.components = components.size();
        std::vector<std::set<unsigned>> neighbours(components.size());
        if (run.bo.careful) {
            std::map<uint32_t, std::set<unsigned>> of_node;
            for (unsigned idx = 0; idx < components.size(); ++idx)
                for (const auto &np : components[idx].first) { of_node[np.first].insert(idx); of_node[np.second].insert(idx); }
            for (unsigned idx = 0; idx < components.size(); ++idx)
                for (const auto &np : components[idx].first) {
                    neighbours[idx].insert(of_node[np.first].begin(), of_node[np.first].end());
                    neighbours[idx].insert(of_node[np.second].begin(), of_node[np.second].end());
                }
        }
        std::set<unsigned> kept;
        for (unsigned idx = 0; idx < components.size(); ++idx) {
            const Comp &comp = components[idx].first;
            const int dist = components[idx].second;
            const auto th = run.table.find(dist);
            std::vector<int> counts(comp.size(), -1);
            bool skip = false, keep = false;
            for (unsigned c : neighbours[idx])
                if (c != idx && kept.count(c)) { to_remove.insert(to_remove.end(), comp.begin(), comp.end()); skip = true; }
            if (!skip) {
                if (th != run.table.end()) {
                    keep = count_unique(comp, th->second, to_remove, counts);
                    if (keep) kept.insert(idx);
                } else {                              // distance too large: the component goes
                    ++st.dist_too_large;
                    to_remove.insert(to_remove.end(), comp.begin(), comp.end());
                }
            }
            report += std::to_string(dist); report += '\t';
            report += std::to_string(th != run.table.end() ? th->second : -1); report += '\t';
            report += keep ? '1' : '0';
            for (size_t k = 0; k < comp.size(); ++k) {
                report += '\t'; report += std::to_string(comp[k].first); report += '>'; report += std::to_string(comp[k].second);
                report += ':'; report += std::to_string(counts[k]);
            }
            report += '\n';
        }
        st.components_kept = kept.size();
        to_remove.sort();
        to_remove.unique();
        removed.assign(to_remove.begin(), to_remove.end());
        st.edges_removed = removed.size();
        st.ms_branch = now_ms() - t0;
    }
};

}  // namespace

void VqBranchRun::prepare(const hlmi_vq_graph_opts &o, const Singles &reads) {
    if (o.remove_trans != 1) fail(HLMI_EINVAL, "vq_branch: the branch reduction needs remove_trans 1 (findBranchfreeGraph asserts it)");
    if (o.remove_branches) fail(HLMI_EINVAL, "vq_branch: remove_branches and the branch reduction exclude each other (ViralQuasispecies.cpp:326-351)");
    table = read_table(table_path);
    originals = read_singles(original_fastq);
    if ((uint64_t)bo.se_count + 2ull * bo.pe_count != originals.seq.size())
        fail(HLMI_EINVAL, "vq_branch: se_count %u + 2 * pe_count %u is not the %zu reads of %s", bo.se_count, bo.pe_count,
             originals.seq.size(), original_fastq);
    if (originals.seq.size() >= (1u << 30)) fail(HLMI_EINVAL, "vq_branch: 2^30 original reads and more");
    for (size_t v = 0; v < reads.id.size(); ++v) {
        if (reads.id[v] != v) fail(HLMI_EINVAL, "vq_branch: read %zu of %s has id %llu; the ids must be the file positions", v,
                                   reads.path.c_str(), (unsigned long long)reads.id[v]);
        if (dict->first_it) {
            if (!originals.index_of.count(reads.id[v]))
                fail(HLMI_EINVAL, "vq_branch: original %llu is not in %s", (unsigned long long)reads.id[v], original_fastq);
            continue;
        }
        const auto it = dict->dict.find(reads.id[v]);
        if (it == dict->dict.end() || it->second.empty())
            fail(HLMI_EINVAL, "vq_branch: read %zu has no line in %s", v, dict->subreads_in);
        for (const auto &kv : it->second)
            if (!originals.index_of.count(kv.first))
                fail(HLMI_EINVAL, "vq_branch: original %llu of read %zu is not in %s", (unsigned long long)kv.first, v, original_fastq);
    }
}

void VqBranchRun::reduce(const hlmi_vq_graph_opts &o, const std::vector<std::string> &seq, const std::vector<uint64_t> &id,
                         const std::vector<std::vector<VqEdge>> &out, const std::vector<uint8_t> &orient, std::vector<VqEdge> &missing,
                         std::vector<std::pair<uint32_t, uint32_t>> &removed, std::string &report) {
    Reduction r{o, *this, seq, out, orient, {}, *st, (uint32_t)seq.size()};
    r.originals.resize(seq.size());
    for (size_t v = 0; v < seq.size(); ++v)
        r.originals[v] = dict->first_it ? VqOriginals{{id[v], VqOrig{true, 0, (int)seq[v].size()}}} : dict->dict.at(id[v]);
    r.reduce(removed, report);
    missing = std::move(r.missing);
}

void vq_branch_graph_run(const char *fastq, const char *overlaps, const char *subreads_in, const char *original_fastq, const char *table,
                         const hlmi_vq_graph_opts &go, const hlmi_vq_branch_opts &bo, const char *out_dir, hlmi_vq_graph_stats *gst,
                         hlmi_vq_branch_stats *bst) {
    *bst = hlmi_vq_branch_stats{};
    VqOriginalsDict dict("vq_branch", subreads_in == nullptr, subreads_in);
    if (subreads_in) dict.dict = vq_parse_subreads(read_file(subreads_in), subreads_in);
    VqBranchRun br;
    br.bo = bo; br.original_fastq = original_fastq; br.table_path = table; br.dict = &dict; br.st = bst;
    vq_graph_run(fastq, overlaps, go, out_dir, gst, nullptr, false, &br);
    ktimer_flush();
}

}  // namespace hlmi
