// vq_clique_host.cpp - the order-dependent host half of ViralQuasispecies --cliques=true (tools/HaploConduct/src,
// ViralQuasispecies.cpp:397-428): the maximal cliques of graph.txt in the order the reference's enumerator lists them - the
// reader, the listing, vq_enumerate_cliques - and nothing else.  Pure host code: nothing here touches the device, and nothing
// here depends on the rest of the library but common.h's fail().
//
// Why the enumeration is not a kernel: the order of the lines of cliques.txt decides the id of every new read, and that
// order is a product of the enumerator's data movement - a backtracking search over one array of vertices that is permuted
// in place, where which vertex sits where decides the pivot, the candidates' order and so the listing.  It is linear in its
// output.  PARITY PINNED: tests/golden/fxK_*.cliques.txt hold what the reference's own binary printed.
//
// The procedure below is that of quick-cliques v2.0beta (tools/HaploConduct/quick-cliques, GNU GPL v3.0, Copyright (c)
// 2011-2016 Darren Strash), --algorithm=degeneracy: the algorithm of Eppstein, Loeffler and Strash (ISAAC 2010 / SEA 2011)
// over the pivoting of Tomita et al. (2006).  Byte-identical output requires the same procedure; it is restated here over this
// library's own data structures.  Notice of that program: "This program is free software: you can redistribute it and/or
// modify it under the terms of the GNU General Public License as published by the Free Software Foundation, either version 3
// of the License, or (at your option) any later version.  This program is distributed in the hope that it will be useful, but
// WITHOUT ANY WARRANTY; without even the implied warranty of MERCHANTABILITY or FITNESS FOR A PARTICULAR PURPOSE."
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "vq_internal.h"

namespace hlmi {
namespace {

// ---- the reader (Tools.cpp:320-375: n, m, then m times "u<char>v"; adjacency lists in file order) -------------------------
struct Scanner {
    const std::string &s;
    size_t at = 0;
    bool integer(long &v) {                     // operator>>(int): blanks skipped, an optional sign, digits
        while (at < s.size() && isspace((unsigned char)s[at])) ++at;
        size_t b = at;
        if (b < s.size() && (s[b] == '-' || s[b] == '+')) ++b;
        if (b >= s.size() || !isdigit((unsigned char)s[b])) return false;
        char *end = nullptr;
        v = strtol(s.c_str() + at, &end, 10);
        at = (size_t)(end - s.c_str());
        return true;
    }
    bool character() {                          // operator>>(char): blanks skipped, one character
        while (at < s.size() && isspace((unsigned char)s[at])) ++at;
        if (at >= s.size()) return false;
        ++at;
        return true;
    }
};

std::vector<std::vector<int>> read_adjacency(const std::string &text) {
    Scanner sc{text};
    long n = 0, m = 0;
    if (!sc.integer(n) || !sc.integer(m) || n < 0 || m < 0 || n >= (1l << 31) || m >= (1l << 31))
        fail(HLMI_EINVAL, "vq_cliques: graph file does not start with its vertex and edge-line counts");
    std::vector<std::vector<int>> adj((size_t)n);
    for (long i = 0; i < m; ++i) {
        long u = 0, v = 0;
        if (!sc.integer(u) || !sc.character() || !sc.integer(v)) fail(HLMI_EINVAL, "vq_cliques: graph file: edge line %ld of %ld is missing", i + 1, m);
        if (u < 0 || u >= n || v < 0 || v >= n || u == v)        // (the reference asserts)
            fail(HLMI_EINVAL, "vq_cliques: graph file: edge line %ld names %ld,%ld among %ld vertices", i + 1, u, v, n);
        adj[(size_t)u].push_back((int)v);
    }
    for (long v = 0; v < n; ++v)                // a degree of n or more (repeated lines) indexes past the reference's buckets
        if ((long)adj[(size_t)v].size() >= n) fail(HLMI_EINVAL, "vq_cliques: graph file: vertex %ld has %zu edge lines", v, adj[(size_t)v].size());
    return adj;
}

// ---- the listing -------------------------------------------------------------------------------------------------------------
class Lister {
public:
    explicit Lister(const std::vector<std::vector<int>> &adj) : n_((int)adj.size()), later_(adj.size()), earlier_(adj.size()) {
        order(adj);
    }
    void run(VqCliqueList &out) {
        out_ = &out;
        slot_.resize((size_t)n_);
        where_.resize((size_t)n_);
        in_p_.assign((size_t)n_, std::vector<int>(1, 0));
        n_in_p_.assign((size_t)n_, 1);
        for (int i = 0; i < n_; ++i) slot_[(size_t)i] = where_[(size_t)i] = i;
        for (int v = 0; v < n_; ++v) {           // the vertices by number; later / earlier follow the degeneracy order
            clique_.push_back(v);
            int x, p, r;
            seed(v, n_, x, p, r);                // (R gives its place back after every vertex, :497)
            expand(x, p, r);
            clique_.pop_back();
        }
    }

private:
    int n_;
    std::vector<std::vector<int>> later_, earlier_;    // per vertex: its neighbours removed after / before it
    std::vector<int> slot_, where_;                    // | .. | X | P | R |: slot_[where_[v]] == v
    std::vector<std::vector<int>> in_p_;               // per vertex of X and P: neighbours, those in P first
    std::vector<int> n_in_p_;
    std::vector<int> clique_;
    VqCliqueList *out_ = nullptr;

    // computeDegeneracyOrderArray (DegeneracyTools.cpp:321-428): the vertex of the smallest remaining degree goes next, the
    // head of its degree's list; a vertex whose degree drops goes to the head of its new list
    void order(const std::vector<std::vector<int>> &adj) {
        const int none = -1;
        std::vector<int> head((size_t)n_, none), next((size_t)n_, none), prev((size_t)n_, none), degree((size_t)n_);
        auto push_front = [&](int d, int v) {
            next[(size_t)v] = head[(size_t)d];
            prev[(size_t)v] = none;
            if (head[(size_t)d] != none) prev[(size_t)head[(size_t)d]] = v;
            head[(size_t)d] = v;
        };
        auto unlink = [&](int d, int v) {
            if (prev[(size_t)v] != none) next[(size_t)prev[(size_t)v]] = next[(size_t)v]; else head[(size_t)d] = next[(size_t)v];
            if (next[(size_t)v] != none) prev[(size_t)next[(size_t)v]] = prev[(size_t)v];
        };
        for (int v = 0; v < n_; ++v) {
            degree[(size_t)v] = (int)adj[(size_t)v].size();
            push_front(degree[(size_t)v], v);
        }
        int d = 0;
        for (int removed = 0; removed < n_;) {
            if (head[(size_t)d] == none) { ++d; continue; }
            const int v = head[(size_t)d];
            unlink(d, v);
            degree[(size_t)v] = -1;
            for (int w : adj[(size_t)v]) {
                if (degree[(size_t)w] == -1) { earlier_[(size_t)v].push_back(w); continue; }
                unlink(degree[(size_t)w], w);
                later_[(size_t)v].push_back(w);
                if (--degree[(size_t)w] != -1) push_front(degree[(size_t)w], w);
            }
            ++removed;
            d = 0;
        }
    }

    void place(int v, int at) {                 // v and the vertex at `at` change places
        const int from = where_[(size_t)v], other = slot_[(size_t)at];
        slot_[(size_t)from] = other;
        where_[(size_t)other] = from;
        slot_[(size_t)at] = v;
        where_[(size_t)v] = at;
    }
    bool inside(int v, int lo, int hi) const { return where_[(size_t)v] >= lo && where_[(size_t)v] < hi; }

    // fillInPandXForRecursiveCallDegeneracy (DegeneracyAlgorithm.cpp:290-406): R = {v}, P = its later, X = its earlier neighbours
    void seed(int v, int begin_r, int &x, int &p, int &r) {
        r = begin_r - 1;
        place(v, r);
        p = r;
        for (int w : later_[(size_t)v]) place(w, --p);
        x = p;
        for (int w : earlier_[(size_t)v]) {
            place(w, --x);
            std::vector<int> &list = in_p_[(size_t)w];
            list.assign((size_t)std::min<int>(r - p, (int)later_[(size_t)w].size()), 0);
            int k = 0;
            for (int u : later_[(size_t)w]) if (inside(u, p, r)) list[(size_t)k++] = u;
            n_in_p_[(size_t)w] = k;
        }
        for (int j = p; j < r; ++j) {
            const int u = slot_[(size_t)j];
            n_in_p_[(size_t)u] = 0;
            in_p_[(size_t)u].assign((size_t)std::min<int>(r - p, (int)(later_[(size_t)u].size() + earlier_[(size_t)u].size())), 0);
        }
        for (int j = p; j < r; ++j) {
            const int u = slot_[(size_t)j];
            for (int w : later_[(size_t)u])
                if (inside(w, p, r)) {
                    in_p_[(size_t)u][(size_t)n_in_p_[(size_t)u]++] = w;
                    in_p_[(size_t)w][(size_t)n_in_p_[(size_t)w]++] = u;
                }
        }
    }

    // findBestPivotNonNeighborsDegeneracy (:144-251): the first vertex of X, P with the most neighbours in P; the candidates are
    // P without its neighbours, compacted by moving the last one into a freed place
    std::vector<int> candidates(int x, int p, int r) const {
        int pivot = -1, best = -1;
        for (int j = x; j < r; ++j) {
            const int v = slot_[(size_t)j];
            const int lim = std::min(r - p, n_in_p_[(size_t)v]);
            int c = 0;
            while (c < lim && inside(in_p_[(size_t)v][(size_t)c], p, r)) ++c;
            if (c > best) { pivot = v; best = c; }
        }
        std::vector<int> cand(slot_.begin() + p, slot_.begin() + r);
        const int lim = std::min(r - p, n_in_p_[(size_t)pivot]);
        for (int j = 0; j < lim; ++j) {
            const int w = in_p_[(size_t)pivot][(size_t)j];
            if (!inside(w, p, r)) break;
            cand[(size_t)(where_[(size_t)w] - p)] = -1;
        }
        int count = r - p;
        for (int j = 0; j < count;) {
            if (cand[(size_t)j] == -1) cand[(size_t)j] = cand[(size_t)--count];
            else ++j;
        }
        cand.resize((size_t)count);
        return cand;
    }

    // moveToRDegeneracy (:563-671): v leaves P for R; the new X and P are those of the old ones that list v among their
    // neighbours in P, gathered around the old border; their lists are put in order again
    void take(int v, int x, int p, int &r, int &nx, int &np, int &nr) {
        --r;
        place(v, r);
        nx = np = nr = p;
        const int size_p = r - p;
        for (int j = x; j < nx;) {
            const int w = slot_[(size_t)j];
            const int lim = std::min(size_p, n_in_p_[(size_t)w]);
            bool stay = true;
            for (int k = 0; k < lim; ++k)
                if (in_p_[(size_t)w][(size_t)k] == v) {
                    --nx;
                    const int other = slot_[(size_t)nx];
                    slot_[(size_t)j] = other; where_[(size_t)other] = j;
                    slot_[(size_t)nx] = w; where_[(size_t)w] = nx;
                    stay = false;
                }
            if (stay) ++j;
        }
        for (int j = p; j < r; ++j) {
            const int w = slot_[(size_t)j];
            const int lim = std::min(size_p, n_in_p_[(size_t)w]);
            for (int k = 0; k < lim; ++k)
                if (in_p_[(size_t)w][(size_t)k] == v) {
                    const int other = slot_[(size_t)nr];
                    slot_[(size_t)j] = other; where_[(size_t)other] = j;
                    slot_[(size_t)nr] = w; where_[(size_t)w] = nr;
                    ++nr;
                }
        }
        for (int j = nx; j < nr; ++j) {
            const int w = slot_[(size_t)j];
            std::vector<int> &list = in_p_[(size_t)w];
            const int lim = std::min(size_p, n_in_p_[(size_t)w]);
            int front = 0;
            for (int k = 0; k < lim; ++k) {
                const int u = list[(size_t)k];
                if (inside(u, np, nr)) {
                    list[(size_t)k] = list[(size_t)front];
                    list[(size_t)front++] = u;
                }
            }
        }
    }

    // listAllMaximalCliquesDegeneracyRecursive (:741-857)
    void expand(int x, int p, int r) {
        if (x >= p && p >= r) {                  // nothing left to add, nothing that was listed before: maximal
            VqCliqueList &o = *out_;
            for (int v : clique_) {
                o.text += std::to_string(v);
                o.text += ' ';                   // printList (Tools.cpp:497-512) puts a blank behind every vertex
                o.members.push_back((uint32_t)v);
            }
            o.text += '\n';
            o.off.push_back(o.members.size());
            return;
        }
        if (p >= r) return;
        const std::vector<int> cand = candidates(x, p, r);
        for (int v : cand) {
            clique_.push_back(v);
            int nx, np, nr;
            take(v, x, p, r, nx, np, nr);
            expand(nx, np, nr);
            clique_.pop_back();
            place(v, p);                         // moveFromRToXDegeneracy (:691-710): v joins X
            ++p;
            ++r;
        }
        for (int v : cand) place(v, --p);        // and back into P for the caller (:836-848)
    }
};

}  // namespace

VqCliqueList vq_enumerate_cliques(const std::string &graph_text) {
    const std::vector<std::vector<int>> adj = read_adjacency(graph_text);
    VqCliqueList out;
    out.text = "NOTE: Quick Cliques v2.0beta.\nReading .edges file format. \n";     // main.cpp:89-92, :163
    out.off.push_back(0);
    Lister(adj).run(out);
    return out;
}

}  // namespace hlmi
