// chain_gpu_check.cpp - a direct check of the middle of the overlapper (csrc/ava_chain.hip): build_index, plan_seeds and
// seed_and_chain against plain sequential host C++, at the fixed sizes of the kernels.  Compiled as HIP by
// tests/test_gpu_chain_direct.py and linked against libhylight_mi.so: it calls the hlmi:: functions themselves (the library
// exports them), no C-ABI entry point and no hook is added; existing hooks are set with setenv + hooks_refresh between cases.
//
//   chain_gpu_check --host          what needs no device: the references below against hand-worked literal cases
//   chain_gpu_check --dump FILE     the reference chains of the anchor groups in FILE.  A group is a line
//                                   "group k max_gap bandwidth min_chain_score min_cnt n" and n lines "tpos qpos span" in chaining
//                                   order; the answer is "group <i> pieces=<p>", then per piece "<chain> <piece> <n_fp> q t q t ..."
//   chain_gpu_check --cases FILE    writes the anchor groups of the device cases in that format (no device needed): the CPU test
//                                   feeds them to --dump and to the oracle
//   chain_gpu_check                 hlmi_init(0, 0), then the groups index_cutoff, index_order, seed_count, seed_fill, chain_sizes,
//                                   chain_window, chain_limits, chain_ties, emit_windows, emit_splits, refusal, seed_group in one process; one
//                                   line "group <name> cases=<n> ok" each
// Exit 1 at the first mismatch, exit 2 at the first HIP error or hlmi::Error; nothing is launched after either.  Everything is
// integer and compared exactly.
//
// Nothing in this layer reads a base: the index is built from an array of minimizers, the seeds from the query minimizers, the
// rank arrays and the read lengths.  A case therefore FABRICATES minimizers: one hash per wanted anchor, a target entry at tpos
// and a query minimizer at qpos, a span byte, a strand bit; a read "of" 2^28 bases costs eight bytes.
//
// The references are written from DESIGN.md section 5 items 2-5, not from the kernels and not from oracle/ava_oracle.c;
// tests/test_gpu_chain_direct.py compares --dump with the oracle's own chain_group (oracle.ava.chain_pieces) on the CPU.
//
// Reading anchors: they are internal to seed_and_chain.  With max_gap = 0, min_cnt = 1, min_chain_score = 1 no anchor has a
// predecessor (0 < dq <= 0 never holds; every form of the DP tests the gaps against max_gap before anything else), so every anchor
// is a chain of one piece with two fixed points: (qe - span, te - span) and (qe, te), chain = its index inside its group.
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <tuple>

#include "ava_internal.h"

using namespace hlmi;

namespace {

struct Mismatch {};
const char *g_group = "";
std::string g_case;
size_t g_cases = 0;

uint64_t g_rng = 0x9e3779b97f4a7c15ull;           // splitmix64, fixed seed
uint64_t rnd() {
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ z >> 27) * 0x94d049bb133111ebull;
    return z ^ z >> 31;
}

void set_case(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_case = buf;
    ++g_cases;
}
[[noreturn]] void mismatch(const char *what, size_t idx, unsigned long long want, unsigned long long got) {
    printf("MISMATCH group %s case %s %s index=%zu want=%llu (0x%llx) got=%llu (0x%llx)\n", g_group, g_case.c_str(), what, idx, want,
           want, got, got);
    fflush(stdout);
    throw Mismatch{};
}
template <typename T>
void expect_eq(const char *what, const std::vector<T> &want, const std::vector<T> &got) {
    for (size_t i = 0; i < std::min(want.size(), got.size()); ++i)
        if (want[i] != got[i]) mismatch(what, i, (unsigned long long)want[i], (unsigned long long)got[i]);
    if (want.size() != got.size()) mismatch(what, std::min(want.size(), got.size()), want.size(), got.size());
}
void expect_one(const char *what, unsigned long long want, unsigned long long got) {
    if (want != got) mismatch(what, 0, want, got);
}
void expect_true(const char *what, bool ok, unsigned long long a = 0, unsigned long long b = 0) {
    if (!ok) mismatch(what, 0, a, b);
}

// ------------------------------------------------------------------------------------------
// the fabricated input: reads that are a length, a name rank and a list of minimizers
// ------------------------------------------------------------------------------------------
struct World {
    int k = 19;
    std::vector<uint64_t> tlen, qlen;
    std::vector<uint32_t> rank_t, rank_q, chunk_of_t;
    uint32_t n_chunks = 1;
    uint64_t n_ranks = 0;
    std::vector<std::vector<Mz>> tmz, qmz;        // per read, in position order; y carries the read's own index
    size_t add_target(uint64_t len, uint32_t rank, uint32_t chunk = 0) {
        tlen.push_back(len); rank_t.push_back(rank); chunk_of_t.push_back(chunk); tmz.emplace_back();
        n_chunks = std::max(n_chunks, chunk + 1); n_ranks = std::max<uint64_t>(n_ranks, rank + 1);
        return tlen.size() - 1;
    }
    size_t add_query(uint64_t len, uint32_t rank) {
        qlen.push_back(len); rank_q.push_back(rank); qmz.emplace_back();
        n_ranks = std::max<uint64_t>(n_ranks, rank + 1);
        return qlen.size() - 1;
    }
    void t_entry(size_t t, uint64_t hash, uint32_t pos, int strand = 0, int span = 19) {
        tmz[t].push_back(Mz{hash << 8 | (uint64_t)span, (uint64_t)t << 32 | (uint64_t)pos << 1 | (uint64_t)strand});
    }
    void q_entry(size_t q, uint64_t hash, uint32_t pos, int strand = 0, int span = 19) {
        qmz[q].push_back(Mz{hash << 8 | (uint64_t)span, (uint64_t)q << 32 | (uint64_t)pos << 1 | (uint64_t)strand});
    }
    void sort_positions() {                       // a sketch is in position order; equal positions keep their order
        auto by_pos = [](const Mz &a, const Mz &b) { return (uint32_t)a.y < (uint32_t)b.y; };
        for (auto &v : tmz) std::stable_sort(v.begin(), v.end(), by_pos);
        for (auto &v : qmz) std::stable_sort(v.begin(), v.end(), by_pos);
    }
};

int bit_length(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// ------------------------------------------------------------------------------------------
// reference: index (DESIGN.md section 5 item 2, and the entry order of ava_internal.h)
// ------------------------------------------------------------------------------------------
struct RefIndex {
    std::vector<uint64_t> key, y, ck;
    std::vector<uint32_t> rk, mid_occ, bucket;
    int rank_bits = 0, bucket_bits = 0, bucket_shift = 0;
};
RefIndex ref_index(const World &w, const hlmi_ava_opts &o, bool no_rank_word) {
    struct Ent { uint64_t key, y; uint32_t rk; };
    std::vector<Ent> e;
    for (size_t t = 0; t < w.tmz.size(); ++t) for (const Mz &m : w.tmz[t]) e.push_back(Ent{m.x >> 8, m.y, 0});
    // occurrences per (chunk, hash)
    std::map<std::pair<uint32_t, uint64_t>, uint32_t> occ;
    for (const Ent &x : e) ++occ[{w.chunk_of_t[x.y >> 32], x.key}];
    RefIndex r;
    r.mid_occ.assign(w.n_chunks, (uint32_t)o.min_mid_occ);
    if (o.mid_occ_frac > 0)
        for (uint32_t c = 0; c < w.n_chunks; ++c) {
            std::vector<uint32_t> counts;                       // one per distinct hash of the chunk
            for (const auto &kv : occ) if (kv.first.first == c) counts.push_back(kv.second);
            if (counts.empty()) continue;
            std::sort(counts.begin(), counts.end());
            uint64_t q = (uint64_t)(uint32_t)((1.0 - o.mid_occ_frac) * (double)counts.size());
            if (q >= counts.size()) q = counts.size() - 1;
            uint64_t cut = (uint64_t)counts[q] + 1;
            cut = std::max<uint64_t>(cut, (uint64_t)o.min_mid_occ);
            cut = std::min<uint64_t>(cut, 1000000);
            r.mid_occ[c] = (uint32_t)cut;
        }
    for (Ent &x : e) {
        const uint32_t t = (uint32_t)(x.y >> 32), c = w.chunk_of_t[t];
        x.rk = occ[{c, x.key}] > r.mid_occ[c] ? 0u : w.rank_t[t] + 1u;
    }
    // by hash, inside a hash by rank word; equal rank words stay in (target, position) order = the order they were listed in
    std::stable_sort(e.begin(), e.end(), [](const Ent &a, const Ent &b) { return a.key != b.key ? a.key < b.key : a.rk < b.rk; });
    for (const Ent &x : e) { r.key.push_back(x.key); r.y.push_back(x.y); r.rk.push_back(x.rk); }
    r.rank_bits = std::max(1, bit_length(w.n_ranks + 1));
    if (2 * w.k + r.rank_bits > 64 || no_rank_word) r.rank_bits = 0;
    if (r.rank_bits) for (const Ent &x : e) r.ck.push_back(x.key << r.rank_bits | x.rk);
    r.bucket_bits = std::min(2 * w.k, std::max(1, bit_length(e.size() >> 4)));      // about one bucket per 16 entries
    r.bucket_shift = 2 * w.k - r.bucket_bits;
    size_t first = 0;                                           // bucket[b] = first entry with key >> bucket_shift >= b
    for (uint64_t b = 0; b <= (1ull << r.bucket_bits); ++b) {
        while (first < e.size() && (e[first].key >> r.bucket_shift) < b) ++first;
        r.bucket.push_back((uint32_t)first);
    }
    return r;
}

// ------------------------------------------------------------------------------------------
// reference: seeds (item 3)
// ------------------------------------------------------------------------------------------
struct Anc { int t, q, sp; };                     // last base on the target, on the query in aligned orientation, span
struct RefSeeds {
    std::vector<uint32_t> cnt, lo, len;           // per query minimizer (all queries, in order)
    std::vector<uint64_t> per_query;
    // per query: (target, strand) -> anchors in generation order
    std::vector<std::map<std::pair<uint32_t, uint32_t>, std::vector<Anc>>> groups;
};
RefSeeds ref_seeds(const World &w, const RefIndex &ix, int pair_once) {
    RefSeeds s;
    s.groups.resize(w.qmz.size());
    for (size_t q = 0; q < w.qmz.size(); ++q) {
        uint64_t per = 0;
        for (const Mz &m : w.qmz[q]) {
            const uint64_t h = m.x >> 8;
            const uint32_t rq = w.rank_q[q];
            uint32_t c = 0;
            size_t first = ix.key.size(), last = 0;      // run: the hash's entries this query may pair with, the read's own included
            // (the entries of equal hash are one stretch of the index: the walk starts at its first entry)
            for (size_t e = std::lower_bound(ix.key.begin(), ix.key.end(), h) - ix.key.begin(); e < ix.key.size() && ix.key[e] == h; ++e) {
                if (ix.rk[e] == 0) continue;                                 // too frequent
                if (pair_once && ix.rk[e] <= rq + 1) continue;               // rank <= the query's (self among them)
                first = std::min(first, e); last = e + 1;
                if (ix.rk[e] == rq + 1) continue;                            // self
                ++c;
                const uint32_t span = (uint32_t)(m.x & 0xff), qpos = (uint32_t)m.y >> 1, qz = (uint32_t)m.y & 1;
                const uint32_t t = (uint32_t)(ix.y[e] >> 32), tpos = (uint32_t)ix.y[e] >> 1, strand = qz ^ ((uint32_t)ix.y[e] & 1);
                const uint32_t qp = strand ? (uint32_t)w.qlen[q] - (qpos + 1 - span) - 1 : qpos;
                // (a fabricated anchor lies inside both reads: the anchor words have the bits of the read lengths and no more)
                expect_true("generator: anchor inside the query", qp < w.qlen[q], qp, w.qlen[q]);
                expect_true("generator: anchor inside the target", tpos < w.tlen[t], tpos, w.tlen[t]);
                s.groups[q][{t, strand}].push_back(Anc{(int)tpos, (int)qp, (int)span});
            }
            s.cnt.push_back(c);
            s.lo.push_back(last ? (uint32_t)first : 0u);
            s.len.push_back(last ? (uint32_t)(last - first) : 0u);
            per += c;
        }
        s.per_query.push_back(per);
    }
    // chaining order: the query's minimizer order in aligned orientation = generation order, backwards on the reverse strand
    for (auto &gq : s.groups) for (auto &kv : gq) if (kv.first.second) std::reverse(kv.second.begin(), kv.second.end());
    return s;
}

// ------------------------------------------------------------------------------------------
// reference: chains and fixed points (items 4 and 5)
// ------------------------------------------------------------------------------------------
struct ChainOpt { int k, max_gap, bw, min_score, min_cnt; };
struct RefPiece { uint32_t chain, piece; std::vector<std::pair<int, int>> fp; };
constexpr int SPEC_PRED = 64, SPEC_BLOCK_MIN = 32, SPEC_SHIFT_MAX = 39;

int gap_cost(int d, int k) {                      // gamma(d) = d k / 100 + (floor(log2 d) >> 1), gamma(0) = 0
    if (d == 0) return 0;
    int lg = 0;
    while ((d >> (lg + 1)) != 0) ++lg;
    return d * k / 100 + (lg >> 1);
}
// far_pred (optional): does some anchor take a predecessor 17 .. 64 back?
std::vector<RefPiece> ref_chain_group(const std::vector<Anc> &a, const ChainOpt &o, bool *far_pred = nullptr,
                                      std::vector<int> *f_out = nullptr, std::vector<int> *p_out = nullptr) {
    const int n = (int)a.size();
    std::vector<int> f(n), p(n, -1), bc(n, -1);
    if (far_pred) *far_pred = false;
    for (int i = 0; i < n; ++i) {
        long best = -(1l << 40);
        int bj = -1;
        for (int j = std::max(0, i - SPEC_PRED); j < i; ++j) {
            const int dq = a[i].q - a[j].q, dr = a[i].t - a[j].t;
            if (!(0 < dq && dq <= o.max_gap && 0 < dr && dr <= o.max_gap)) continue;
            const int d = dr > dq ? dr - dq : dq - dr;
            if (d > o.bw) continue;
            const long c = (long)f[j] + std::min(a[i].sp, std::min(dq, dr)) - gap_cost(d, o.k);
            if (c >= best) { best = c; bj = j; }              // ties to the later predecessor
        }
        if (bj >= 0 && best > a[i].sp) { f[i] = (int)best; p[i] = bj; } else f[i] = a[i].sp;
        if (far_pred && p[i] >= 0 && i - p[i] >= 17) *far_pred = true;
    }
    for (int i = 0; i < n; ++i)                                 // best child: larger f, then smaller index
        if (p[i] >= 0 && (bc[p[i]] < 0 || f[i] > f[bc[p[i]]])) bc[p[i]] = i;
    if (f_out) *f_out = f;
    if (p_out) *p_out = p;
    const int shift_max = o.bw == 0 ? 0 : SPEC_SHIFT_MAX;
    std::vector<RefPiece> out;
    for (int s = 0; s < n; ++s) {
        if (p[s] >= 0 && bc[p[s]] == s) continue;               // inside its parent's chain
        std::vector<int> mem{s};
        size_t peak = 0;
        for (int c = bc[s]; c >= 0; c = bc[c]) {
            mem.push_back(c);
            if (f[c] > f[mem[peak]]) peak = mem.size() - 1;     // the first highest f
        }
        mem.resize(peak + 1);
        if (f[mem[peak]] - (p[s] >= 0 ? f[p[s]] : 0) < o.min_score || (int)mem.size() < o.min_cnt) continue;
        bool open = false;
        int cq = 0, ct = 0;
        uint32_t np = 0;
        RefPiece cur;
        auto block_ok = [&](int q0, int t0, int q1, int t1) {
            const int m = q1 - q0, nn = t1 - t0;
            return m >= 0 && nn >= 0 && std::abs(nn - m) <= shift_max;
        };
        for (size_t x = 0; x < mem.size(); ++x) {
            const Anc &an = a[mem[x]];
            const int qe = an.q + 1, te = an.t + 1;
            if (!open) {                                        // the start of this member, moved along its diagonal into both reads
                int q0 = qe - an.sp, t0 = te - an.sp;
                const int sh = std::max(0, std::max(-q0, -t0));
                q0 += sh; t0 += sh;
                if (!block_ok(q0, t0, qe, te)) continue;        // a start whose own block fails is skipped
                cur = RefPiece{(uint32_t)s, np, {{q0, t0}, {qe, te}}};
                cq = qe; ct = te; open = true;
                continue;
            }
            const bool far = qe - cq >= SPEC_BLOCK_MIN && te - ct >= SPEC_BLOCK_MIN;
            if (!(far || x + 1 == mem.size())) continue;
            if (qe <= cq || te <= ct) continue;
            if (block_ok(cq, ct, qe, te)) { cur.fp.push_back({qe, te}); cq = qe; ct = te; }
            else { out.push_back(cur); ++np; open = false; --x; }              // split: reopen at this member
        }
        if (open) out.push_back(cur);
    }
    return out;
}

// everything seed_and_chain should deliver for the queries [q_lo, q_hi)
typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t> PieceKey;     // q, t, strand, chain, piece
typedef std::map<PieceKey, std::vector<std::pair<int, int>>> PieceMap;
struct RefChains { PieceMap pieces; size_t n_fp = 0, anchors = 0, groups = 0, big = 0, small = 0, small_kept = 0, big_far = 0; };
RefChains ref_chains(const RefSeeds &s, const ChainOpt &o, size_t q_lo, size_t q_hi) {
    RefChains r;
    for (size_t q = q_lo; q < q_hi; ++q)
        for (const auto &kv : s.groups[q]) {
            bool far = false;
            ++r.groups;
            r.anchors += kv.second.size();
            if (kv.second.size() > 32) ++r.big; else ++r.small;
            if (kv.second.size() <= 32 && (int)kv.second.size() >= o.min_cnt) ++r.small_kept;      // (seed_group.hip records no smaller group)
            for (const RefPiece &p : ref_chain_group(kv.second, o, &far)) {
                r.pieces[PieceKey{(uint32_t)q, kv.first.first, kv.first.second, p.chain, p.piece}] = p.fp;
                r.n_fp += p.fp.size();
            }
            if (far && kv.second.size() > 32 && (int)kv.second.size() >= o.min_cnt) ++r.big_far;
        }
    return r;
}

// ------------------------------------------------------------------------------------------
// case builder: a list of wanted (query, target, strand) groups in aligned coordinates -> a World
// ------------------------------------------------------------------------------------------
struct WantGroup { uint32_t q, t, strand; std::vector<Anc> a; };
uint64_t g_hash_ctr = 0;
uint64_t fresh_hash(int k) {                      // distinct values spread over the 2k bits (an odd multiplier is a bijection)
    const uint64_t mask = 2 * k == 64 ? ~0ull : (1ull << 2 * k) - 1;
    return (++g_hash_ctr * 0x9e3779b97f4a7c15ull) & mask;
}
// queries rank below every target (pair-once keeps every pair); n_q / n_t reads of the given lengths
World world_of(const std::vector<WantGroup> &groups, size_t n_q, size_t n_t, uint64_t ql, uint64_t tl, int k = 19) {
    World w;
    w.k = k;
    for (size_t q = 0; q < n_q; ++q) w.add_query(ql, (uint32_t)q);
    for (size_t t = 0; t < n_t; ++t) w.add_target(tl, (uint32_t)(n_q + t));
    for (const WantGroup &g : groups) {
        const size_t n = g.a.size();
        for (size_t x = 0; x < n; ++x) {
            const Anc &an = g.a[g.strand ? n - 1 - x : x];       // generation order
            const uint64_t h = fresh_hash(k);
            w.t_entry(g.t, h, (uint32_t)an.t, 0, an.sp);
            const uint32_t raw = g.strand ? (uint32_t)(w.qlen[g.q] + (uint64_t)an.sp - 2 - (uint64_t)an.q) : (uint32_t)an.q;
            w.q_entry(g.q, h, raw, (int)g.strand, an.sp);
        }
    }
    w.sort_positions();
    return w;
}
// the groups the reference derives from the world are the wanted ones, in the wanted order: the case sits where it was meant to
void expect_groups(const std::vector<WantGroup> &want, const RefSeeds &s) {
    size_t total = 0;
    for (const auto &gq : s.groups) total += gq.size();
    expect_one("generator: groups", want.size(), total);
    for (const WantGroup &g : want) {
        const auto it = s.groups[g.q].find({g.t, g.strand});
        expect_true("generator: group exists", it != s.groups[g.q].end(), g.q, g.t);
        expect_one("generator: group size", g.a.size(), it->second.size());
        for (size_t i = 0; i < g.a.size(); ++i)
            if (g.a[i].t != it->second[i].t || g.a[i].q != it->second[i].q || g.a[i].sp != it->second[i].sp)
                mismatch("generator: anchor order", i, (unsigned long long)g.a[i].q, (unsigned long long)it->second[i].q);
    }
}

hlmi_ava_opts base_opts() {
    hlmi_ava_opts o{};
    o.k = 19; o.w = 5; o.hpc = 1; o.min_chain_score = 100; o.max_gap = 10000; o.bandwidth = 2000; o.min_cnt = 3;
    o.min_mid_occ = 10; o.mid_occ_frac = 2e-4; o.match = 2; o.mismatch = 4; o.gap_open = 4; o.gap_ext = 2; o.ambi = 1;
    o.min_dp_score = 80; o.end_bonus = 0; o.pair_once = 1; o.gap_open2 = 24; o.gap_ext2 = 1; o.stub_oh = -1; o.zdrop = 400;
    return o;
}
hlmi_ava_opts isolating(hlmi_ava_opts o) { o.max_gap = 0; o.min_cnt = 1; o.min_chain_score = 1; return o; }
ChainOpt chain_opt(const hlmi_ava_opts &o) { return ChainOpt{o.k, o.max_gap, o.bandwidth, o.min_chain_score, o.min_cnt}; }

// a collinear run of n anchors: step dq on the query, dt on the target, from (q0, t0)
std::vector<Anc> line(int n, int q0, int t0, int dq, int dt, int sp = 19) {
    std::vector<Anc> a;
    for (int i = 0; i < n; ++i) a.push_back(Anc{t0 + i * dt, q0 + i * dq, sp});
    return a;
}
// two or three chains on parallel diagonals `off` apart, their anchors alternating in query order
std::vector<Anc> interleaved(int chains, int n_each, int q0, int t0, int step, int off, int sp = 19) {
    std::vector<Anc> a;
    for (int i = 0; i < n_each; ++i)
        for (int c = 0; c < chains; ++c) a.push_back(Anc{t0 + i * step + c * off + c, q0 + i * step + c, sp});
    return a;
}

// ------------------------------------------------------------------------------------------
// the device cases' anchor groups, shared by the device run and by --cases (the CPU comparison with the oracle)
// ------------------------------------------------------------------------------------------
struct ChainCase { std::string group, name; hlmi_ava_opts o; std::vector<std::vector<Anc>> groups; uint64_t ql, tl; const char *hook; bool fwd_only = false; };
void add_case(std::vector<ChainCase> &v, const char *group, const std::string &name, const hlmi_ava_opts &o,
              const std::vector<std::vector<Anc>> &groups, uint64_t ql = 200000, uint64_t tl = 200000, const char *hk = nullptr) {
    v.push_back(ChainCase{group, name, o, groups, ql, tl, hk, false});
}

std::vector<ChainCase> chain_cases() {
    std::vector<ChainCase> v;
    const hlmi_ava_opts L = base_opts();
    // ---- chain_sizes: SMALL_N 32, rows of 16, 64-anchor windows, the 16-bit size key ----
    {
        std::vector<std::vector<Anc>> sizes;
        for (int n : {1, 2, 3, 16, 17, 32, 33, 63, 64, 65, 255, 256, 257}) sizes.push_back(line(n, 100, 300, 25, 25));
        add_case(v, "chain_sizes", "sizes_min_cnt3", L, sizes);
        hlmi_ava_opts m5 = L;
        m5.min_cnt = 5;                              // min_cnt - 1 = 4 and min_cnt = 5 anchors
        add_case(v, "chain_sizes", "min_cnt5", m5, {line(4, 100, 300, 30, 30), line(5, 100, 300, 30, 30), line(40, 50, 90, 30, 31)});
        add_case(v, "chain_sizes", "over_65535", L, {line(65540, 30, 40, 3, 3), line(40, 100, 100, 25, 25)}, 400000, 400000);
        for (int nb : {1, 3, 4, 5, 15, 16, 17}) {    // big groups in one launch, small ones beside them
            std::vector<std::vector<Anc>> gs;
            for (int i = 0; i < nb; ++i) gs.push_back(line(33 + 7 * i, 100 + i, 300 + 3 * i, 25, 25 + (i & 1)));
            gs.push_back(line(5, 100, 100, 40, 40));
            add_case(v, "chain_sizes", "big_groups_" + std::to_string(nb), L, gs);
        }
    }
    // ---- chain_window: the predecessor at distance 1 .. 64, a better one at 65 ----
    {
        // a head of `head` collinear anchors, then `dist - 1` strays, then one anchor collinear with the head's last: its
        // predecessor lies `dist` back.  Strays: beyond the bandwidth of everything (target far away, 5 apart on the query so that
        // they do not chain among themselves either: dr = 0), or on the last head anchor's query position (dq = 0).
        auto windowed = [&](int dist, int kind, int total) {
            std::vector<Anc> a = line(20, 1000, 5000, 30, 30);
            const Anc last = a.back();
            for (int s = 0; s < dist - 1; ++s)
                a.push_back(kind == 0 ? Anc{150000, last.q + 1 + s / 8, 19} : Anc{last.t + 3000 + 40 * s, last.q, 19});
            a.push_back(Anc{last.t + 100, last.q + 100, 19});
            const Anc tail = a.back();
            while ((int)a.size() < total) a.push_back(Anc{tail.t + 30 * ((int)a.size() - 19), tail.q + 30 * ((int)a.size() - 19), 19});
            return a;
        };
        for (int kind = 0; kind < 2; ++kind) {
            std::vector<std::vector<Anc>> gs;
            for (int dist : {1, 15, 16, 17, 63, 64, 65}) gs.push_back(windowed(dist, kind, 120));
            gs.push_back(line(100, 100, 100, 25, 25));           // purely collinear big groups
            gs.push_back(line(40, 100, 100, 25, 26));
            gs.push_back(windowed(17, kind, 0));                 // 20 + 16 + 1 = 37 anchors: just above SMALL_N
            gs.push_back(windowed(9, kind, 0));                  // 29 anchors: chain_small_kernel
            const char *nm = kind ? "strays_dq0" : "strays_off_band";
            add_case(v, "chain_window", nm, L, gs);
            add_case(v, "chain_window", std::string(nm) + "_no_dp16", L, gs, 200000, 200000, "HLMI_CHAIN_NO_DP16");
            add_case(v, "chain_window", std::string(nm) + "_no_small", L, gs, 200000, 200000, "HLMI_CHAIN_NO_SMALL");
            add_case(v, "chain_window", std::string(nm) + "_unpacked", L, gs, 200000, 200000, "HLMI_CHAIN_UNPACKED");
        }
    }
    // ---- chain_limits: max_gap, bandwidth, the gap cost, the table forms ----
    {
        // pairs of anchors (and a third that makes min_cnt): the second's gaps to the first are (dq, dr)
        auto pairs = [&](const hlmi_ava_opts &o, const std::vector<std::pair<int, int>> &gaps, int pad) {
            std::vector<std::vector<Anc>> gs;
            for (const auto &g : gaps) {
                std::vector<Anc> a = line(3, 1000, 20000, 25, 25);
                const Anc l = a.back();
                a.push_back(Anc{l.t + g.second, l.q + g.first, 19});
                a.push_back(Anc{a.back().t + 25, a.back().q + 25, 19});
                a.push_back(Anc{a.back().t + 25, a.back().q + 25, 19});
                if (pad) { const std::vector<Anc> more = line(pad, a.back().q + 25, a.back().t + 25, 25, 25); a.insert(a.end(), more.begin(), more.end()); }
                gs.push_back(a);
            }
            (void)o;
            return gs;
        };
        hlmi_ava_opts o = L;
        o.max_gap = 500; o.bandwidth = 300; o.min_chain_score = 40;
        const int G = 500, bw = 300;
        std::vector<std::pair<int, int>> gaps = {{G, G}, {G + 1, G + 1}, {G, G - 10}, {G - 10, G}, {G + 1, G - 10}, {G - 10, G + 1},
                                                 {30, 0}, {30, -40}, {0, 30}, {30, 30 + bw}, {30, 31 + bw}, {30 + bw, 30}, {31 + bw, 30}};
        for (int d : {1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, bw}) { gaps.push_back({40, 40 + d}); gaps.push_back({40 + d, 40}); }
        for (int pad : {0, 40}) {                                // small groups, and the same as big ones
            add_case(v, "chain_limits", pad ? "gaps_big" : "gaps_small", o, pairs(o, gaps, pad));
            add_case(v, "chain_limits", pad ? "gaps_big_no_dp16" : "gaps_small_no_small", o, pairs(o, gaps, pad), 200000, 200000,
                     pad ? "HLMI_CHAIN_NO_DP16" : "HLMI_CHAIN_NO_SMALL");
            add_case(v, "chain_limits", pad ? "gaps_big_unpacked" : "gaps_small_unpacked", o, pairs(o, gaps, pad), 200000, 200000, "HLMI_CHAIN_UNPACKED");
        }
        hlmi_ava_opts z = o;
        z.bandwidth = 0;                                         // bandwidth 0: only dr = dq chains, any shift splits
        add_case(v, "chain_limits", "bw0", z, pairs(z, {{30, 30}, {30, 31}, {31, 30}, {G, G}}, 40));
        add_case(v, "chain_limits", "bw0_small", z, pairs(z, {{30, 30}, {30, 31}, {31, 30}, {G, G}}, 0));
        for (int b : {2046, 2047}) {                             // PEN_TAB 2048: bandwidth + 2 fits the table, or the computed form runs
            hlmi_ava_opts t = L;
            t.bandwidth = b; t.min_chain_score = 40;
            add_case(v, "chain_limits", "bandwidth" + std::to_string(b), t,
                     pairs(t, {{40, 40 + b}, {40, 41 + b}, {40 + b, 40}, {41 + b, 40}, {40, 40 + 1024}, {40, 40 + 1023}, {50, 50}}, 40));
        }
        for (int b : {1263, 1264}) {                             // k = 19: 1263 * 19 / 100 + 16 = 255 fits a byte, 1264 does not
            hlmi_ava_opts t = L;
            t.bandwidth = b; t.min_chain_score = 40;
            add_case(v, "chain_limits", "unpacked_bandwidth" + std::to_string(b), t,
                     pairs(t, {{40, 40 + b}, {40, 41 + b}, {40 + b, 40}, {40, 40 + 1024}, {40, 40 + 1023}, {50, 50}}, 40), 200000, 200000,
                     "HLMI_CHAIN_UNPACKED");
        }
        // either side of the packed form: queries of 2^22 - 257 / 2^22 - 256 bases, targets of 2^28 - 1 / 2^28 bases, anchors at the far ends
        for (uint64_t ql : {(1ull << 22) - 257, (1ull << 22) - 256})
            for (uint64_t tl : {(1ull << 28) - 1, 1ull << 28}) {
                hlmi_ava_opts t = L;
                t.min_chain_score = 40;
                std::vector<std::vector<Anc>> gs = {line(40, (int)ql - 40 * 30, (int)tl - 40 * 30, 30, 30), line(5, 100, 100, 30, 30),
                                                    line(70, 200, (int)tl - 70 * 31, 30, 31)};
                add_case(v, "chain_limits", "ql" + std::to_string(ql) + "_tl" + std::to_string(tl), t, gs, ql, tl);
            }
        // one collinear chain of span-255 anchors over the longest query of the packed form (2^22 - 257 = 4194047 bases): 255 apart,
        // every anchor adds 255; 16447 anchors, the last ending at base 254 + 16446 * 255 = 4193984 (the next would end behind the
        // query), score 255 * 16447 = 4193985 = 2^22 - 319: within 62 of the query length
        {
            hlmi_ava_opts t = L;
            t.max_gap = 10000;
            const uint64_t ql = (1ull << 22) - 257;
            const int n = (int)((ql - 255) / 255) + 1;
            add_case(v, "chain_limits", "score_near_2_22", t, {line(n, 254, 254, 255, 255, 255)}, ql, 1ull << 23);
        }
    }
    // ---- chain_ties ----
    {
        hlmi_ava_opts o = L;
        o.min_chain_score = 40; o.max_gap = 500; o.bandwidth = 300;
        // equal candidates: two predecessors one base apart on both sequences with equal f (both chain starts of span 19, the
        // second not reachable from the first: dq = 0) give the third the same candidate - the later one wins
        std::vector<Anc> later = {{5000, 1000, 19}, {5003, 1000, 19}, {5040, 1040, 19}, {5070, 1070, 19}, {5100, 1100, 19}};
        // equal children: two children of one parent with equal f - the smaller index keeps the trunk
        std::vector<Anc> child = {{5000, 1000, 19}, {5030, 1030, 19}, {5060, 1060, 19}, {5063, 1060, 19}, {5100, 1100, 19}, {5130, 1130, 19}};
        // equal peaks: the chain's last anchors add nothing (gap cost = gain): the first highest f ends the chain
        std::vector<Anc> peaks = line(6, 1000, 5000, 30, 30);
        peaks.push_back(Anc{peaks.back().t + 19 + 100, peaks.back().q + 19, 19});       // + 19 - gamma(100) = 19 - (19 + 3) < 0 ...
        peaks.push_back(Anc{peaks.back().t + 1, peaks.back().q + 1 + 5, 19});           // ... and small steps around f's maximum
        peaks.push_back(Anc{peaks.back().t + 1, peaks.back().q + 1, 19});
        for (int pad : {0, 40}) {
            auto padded = [&](std::vector<Anc> a) {
                if (pad) { const std::vector<Anc> more = line(pad, a.back().q + 400, a.back().t + 1400, 25, 25); a.insert(a.end(), more.begin(), more.end()); }
                return a;
            };
            const std::vector<std::vector<Anc>> gs = {padded(later), padded(child), padded(peaks)};
            add_case(v, "chain_ties", pad ? "ties_big" : "ties_small", o, gs);
            add_case(v, "chain_ties", pad ? "ties_big_no_dp16" : "ties_small_no_small", o, gs, 200000, 200000, pad ? "HLMI_CHAIN_NO_DP16" : "HLMI_CHAIN_NO_SMALL");
            add_case(v, "chain_ties", pad ? "ties_big_unpacked" : "ties_small_unpacked", o, gs, 200000, 200000, "HLMI_CHAIN_UNPACKED");
        }
        // score equal to min_chain_score and one below: n collinear anchors 19 apart score 19 n
        for (int ms : {19 * 6, 19 * 6 + 1})
            for (int n : {6, 40}) {
                hlmi_ava_opts t = o;
                t.min_chain_score = ms;
                add_case(v, "chain_ties", "score" + std::to_string(ms) + "_n" + std::to_string(n), t,
                         {line(6, 1000, 5000, 19, 19), n == 40 ? line(40, 100, 100, 2, 2) : line(6, 300, 700, 19, 19)});
            }
        // member count equal to min_cnt and one below, two chains interleaved: the count needs the second and third window
        for (int mc : {2, 3, 70, 130})
            for (int each : {mc - 1, mc}) {
                hlmi_ava_opts t = o;
                t.min_cnt = mc; t.min_chain_score = 19;
                if (each < 1) continue;
                add_case(v, "chain_ties", "min_cnt" + std::to_string(mc) + "_members" + std::to_string(each), t,
                         {interleaved(2, each, 1000, 5000, 30, 1000)});
                add_case(v, "chain_ties", "min_cnt" + std::to_string(mc) + "_members" + std::to_string(each) + "_no_small", t,
                         {interleaved(2, each, 1000, 5000, 30, 1000)}, 200000, 200000, "HLMI_CHAIN_NO_SMALL");
            }
    }
    // ---- emit_windows: 64-anchor windows of emit_chain, the last 8 lanes ----
    {
        hlmi_ava_opts o = L;
        o.min_chain_score = 40;
        std::vector<std::vector<Anc>> gs;
        for (int n : {63, 64, 65, 128, 129}) gs.push_back(line(n, 1000, 5000, 40, 40));
        for (int c : {2, 3})
            for (int n : {40, 64, 70}) gs.push_back(interleaved(c, n, 1000, 5000, 40, 700));
        // the peak at lane 0 and at lane 63 of a window: a chain of 65 / 128 members whose tail adds nothing
        for (int n : {65, 128}) {
            std::vector<Anc> a = line(n, 1000, 5000, 40, 40);
            a.push_back(Anc{a.back().t + 19 + 200, a.back().q + 19, 19});
            a.push_back(Anc{a.back().t + 40, a.back().q + 40, 19});
            gs.push_back(a);
        }
        // member spacing 1 (more than 64 members between two fixed points), 31, 32, 33, in either sequence alone and in both
        for (int sp : {1, 31, 32, 33}) {
            gs.push_back(line(150, 1000, 5000, sp, sp));
            gs.push_back(line(150, 1000, 5000, sp, 40));
            gs.push_back(line(150, 1000, 5000, 40, sp));
        }
        // a qualifying member with 7 and with 8 anchors left in its window: spacing 8 makes every fourth member a fixed point
        // (32 apart); chains of 64 - r members end their window r lanes early
        for (int n : {57, 58, 59, 60, 61, 62, 121, 122, 123, 124}) gs.push_back(line(n, 1000, 5000, 8, 8));
        // a first anchor closer to the read start than its span: in the query, in the target, in both
        gs.push_back(line(40, 5, 5000, 40, 40));
        gs.push_back(line(40, 1000, 7, 40, 40));
        gs.push_back(line(40, 3, 9, 40, 40));
        gs.push_back(line(40, 0, 0, 40, 40));
        gs.push_back(line(5, 5, 5000, 40, 40));
        gs.push_back(line(5, 1000, 7, 40, 40));
        gs.push_back(line(5, 3, 9, 40, 40));
        add_case(v, "emit_windows", "windows", o, gs);
        add_case(v, "emit_windows", "windows_no_dp16", o, gs, 200000, 200000, "HLMI_CHAIN_NO_DP16");
        add_case(v, "emit_windows", "windows_unpacked", o, gs, 200000, 200000, "HLMI_CHAIN_UNPACKED");
    }
    // ---- emit_splits: SHIFT_MAX 39, PIECE_BUF 32 ----
    {
        hlmi_ava_opts o = L;
        o.min_chain_score = 40;
        // a collinear chain whose link `at` shifts the diagonal by `shift`
        auto shifted = [&](int n, const std::vector<int> &at, int shift) {
            std::vector<Anc> a;
            int q = 1000, t = 5000;
            for (int i = 0; i < n; ++i) {
                q += 40; t += 40;
                if (std::find(at.begin(), at.end(), i) != at.end()) { if (shift > 0) t += shift; else q -= shift; }   // the target gains, or the query
                a.push_back(Anc{t, q, 19});
            }
            return a;
        };
        std::vector<std::vector<Anc>> gs;
        for (int shift : {39, 40, -39, -40}) {
            for (int n : {10, 50}) {
                gs.push_back(shifted(n, {5}, shift));
                gs.push_back(shifted(n, {n - 1}, shift));            // at the last member
                gs.push_back(shifted(n, {1}, shift));                // immediately after a start
                gs.push_back(shifted(n, {1, 2, 3}, shift));
            }
        }
        for (int pieces : {31, 32, 33, 65}) {                        // pieces in one chain: a split at every second link
            std::vector<int> at;
            for (int i = 0; i < pieces - 1; ++i) at.push_back(2 + 2 * i);
            gs.push_back(shifted(2 * pieces + 2, at, 40));
        }
        add_case(v, "emit_splits", "splits", o, gs);
        add_case(v, "emit_splits", "splits_no_small", o, gs, 200000, 200000, "HLMI_CHAIN_NO_SMALL");
        // a wave's share of groups: four big groups of equal size, forward strand only (one wave takes exactly these four, in this
        // order), with 8 + 8 + 8 + 7, 8 x 4, 8 + 8 + 8 + 9 and 16 + 16 + 16 + 17 pieces
        for (int total : {31, 32, 33, 65}) {
            std::vector<std::vector<Anc>> g4;
            const int each = (total + 1) / 4;
            for (int i = 0; i < 4; ++i) {
                const int pieces = i == 3 ? total - 3 * each : each;
                std::vector<int> at;
                for (int j = 0; j < pieces - 1; ++j) at.push_back(2 + 5 * j);
                g4.push_back(shifted(100, at, 40));
            }
            add_case(v, "emit_splits", "wave_share_" + std::to_string(total), o, g4);
            v.back().fwd_only = true;
        }
    }
    return v;
}

// the groups of a case as the builder takes them: group i is query i % n_q (forward) or its reverse strand on the next target
std::vector<WantGroup> want_groups(const ChainCase &c, size_t &n_q, size_t &n_t) {
    // every group is laid twice: forward on target 2 i of query i % 3, reverse strand on target 2 i + 1
    std::vector<WantGroup> w;
    n_q = 3;
    n_t = 2 * c.groups.size();
    for (size_t i = 0; i < c.groups.size(); ++i) {
        w.push_back(WantGroup{(uint32_t)(i % 3), (uint32_t)(2 * i), 0, c.groups[i]});
        if (!c.fwd_only) w.push_back(WantGroup{(uint32_t)((i + 1) % 3), (uint32_t)(2 * i + 1), 1, c.groups[i]});
    }
    return w;
}

// ------------------------------------------------------------------------------------------
// --host: the references against hand-worked cases
// ------------------------------------------------------------------------------------------
#define HOST_EXPECT(cond)                                                                                  \
    do {                                                                                                   \
        ++g_cases;                                                                                         \
        if (!(cond)) { printf("MISMATCH host %s: %s (line %d)\n", g_group, #cond, __LINE__); return 1; }   \
    } while (0)
int host_done() { printf("host %s cases=%zu ok\n", g_group, g_cases); g_cases = 0; return 0; }

typedef std::vector<std::pair<int, int>> FP;
bool pieces_are(const std::vector<RefPiece> &got, std::initializer_list<std::tuple<int, int, FP>> want) {
    if (got.size() != want.size()) { printf("(%zu pieces, %zu expected)\n", got.size(), want.size()); return false; }
    size_t i = 0;
    for (const auto &w : want) {
        if ((int)got[i].chain != std::get<0>(w) || (int)got[i].piece != std::get<1>(w) || got[i].fp != std::get<2>(w)) { printf("(piece %zu)\n", i); return false; }
        ++i;
    }
    return true;
}

int run_host() {
    g_group = "ref_gap_cost";
    // gamma(d) = d k / 100 + (floor(log2 d) >> 1), k = 19: 1 -> 0 + 0; 2 -> 0 + 0 (log 1); 3 -> 0 + 0; 4 -> 0 + 1 (log 2); 7 -> 1 + 1;
    // 8 -> 1 + 1 (log 3); 16 -> 3 + 2; 100 -> 19 + 3 (log 6); 2000 -> 380 + 5 (log 10)
    HOST_EXPECT(gap_cost(0, 19) == 0 && gap_cost(1, 19) == 0 && gap_cost(2, 19) == 0 && gap_cost(3, 19) == 0 && gap_cost(4, 19) == 1);
    HOST_EXPECT(gap_cost(7, 19) == 2 && gap_cost(8, 19) == 2 && gap_cost(16, 19) == 5 && gap_cost(100, 19) == 22 && gap_cost(2000, 19) == 385);
    HOST_EXPECT(gap_cost(50, 21) == 10 + 2);
    host_done();

    g_group = "ref_chain";
    const ChainOpt o{19, 500, 300, 40, 3};
    std::vector<int> f, p;
    {   // 1. three collinear anchors 30 apart: f = 19, 38, 57 (min(19, 30) each, no gap cost); one chain, score 57 >= 40; fixed points:
        // start of the first (1000 - 18 = 982 / 4982, ends are exclusive: 1001 - 19), its end (1001, 5001), the second's end is 30 < 32
        // away and skipped, the peak always (1061, 5061)
        const std::vector<Anc> a = {{5000, 1000, 19}, {5030, 1030, 19}, {5060, 1060, 19}};
        const auto r = ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT((f == std::vector<int>{19, 38, 57}) && (p == std::vector<int>{-1, 0, 1}));
        HOST_EXPECT(pieces_are(r, {{0, 0, FP{{982, 4982}, {1001, 5001}, {1061, 5061}}}}));
    }
    {   // 2. a tie: anchors 0 and 1 at one query position (dq = 0: they do not chain), f = 19 both; anchor 2 is 40 / 40 and 40 / 37 from
        // them: candidates 19 + 19 - gamma(0) = 38 and 19 + 19 - gamma(3) = 38 - 0: equal, the later predecessor (1) wins.  Anchor 3:
        // 38 + 19 = 57.  Chain 0 is anchor 0 alone (19 < 40, dropped); chain 1 = 1, 2, 3 scores 57.  From (1001, 5004): (1041, 5041) is
        // 40 / 37 away, shift 3, both >= 32: a fixed point; (1081, 5081) the peak
        const std::vector<Anc> a = {{5000, 1000, 19}, {5003, 1000, 19}, {5040, 1040, 19}, {5080, 1080, 19}};
        const auto r = ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT((f == std::vector<int>{19, 19, 38, 57}) && (p == std::vector<int>{-1, -1, 1, 2}));
        HOST_EXPECT(pieces_are(r, {{1, 0, FP{{982, 4985}, {1001, 5004}, {1041, 5041}, {1081, 5081}}}}));
    }
    {   // 3. a dropped stray: anchor 2 lies 301 off the diagonal (beyond bw = 300): it chains with nobody (f = 19, a chain of one
        // anchor, below min_cnt); 0, 1, 3 chain: 3 is 80 / 80 from 1: 38 + 19 = 57
        const std::vector<Anc> a = {{5000, 1000, 19}, {5040, 1040, 19}, {5401, 1100, 19}, {5120, 1120, 19}};
        const auto r = ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT((f == std::vector<int>{19, 38, 19, 57}) && (p == std::vector<int>{-1, 0, -1, 1}));
        HOST_EXPECT(pieces_are(r, {{0, 0, FP{{982, 4982}, {1001, 5001}, {1041, 5041}, {1121, 5121}}}}));
    }
    {   // 4. a cut at the peak: the fourth anchor is 19 / 119 from the third: 57 + 19 - gamma(100) = 57 + 19 - 22 = 54 < 57 but > its
        // span: it has the third as its predecessor and is its best child, yet the chain is cut at the first highest f (anchor 2)
        const std::vector<Anc> a = {{5000, 1000, 19}, {5040, 1040, 19}, {5080, 1080, 19}, {5199, 1099, 19}};
        const auto r = ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT((f == std::vector<int>{19, 38, 57, 54}) && (p == std::vector<int>{-1, 0, 1, 2}));
        HOST_EXPECT(pieces_are(r, {{0, 0, FP{{982, 4982}, {1001, 5001}, {1041, 5041}, {1081, 5081}}}}));
    }
    {   // 5. a split: the third anchor is 40 / 80 from the second (shift 40 > 39): 38 + 19 - gamma(40) = 57 - (7 + 2) = 48, the fourth
        // 48 + 19 = 67.  Piece 0 closes at (1041, 5041); piece 1 reopens at the third anchor's start (1081 - 19, 5121 - 19)
        const std::vector<Anc> a = {{5000, 1000, 19}, {5040, 1040, 19}, {5120, 1080, 19}, {5160, 1120, 19}};
        const auto r = ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT((f == std::vector<int>{19, 38, 48, 67}) && (p == std::vector<int>{-1, 0, 1, 2}));
        HOST_EXPECT(pieces_are(r, {{0, 0, FP{{982, 4982}, {1001, 5001}, {1041, 5041}}}, {0, 1, FP{{1062, 5102}, {1081, 5121}, {1121, 5161}}}}));
        // shift 39 stays one piece: gamma(39) = 7 + 2 as well
        const std::vector<Anc> b = {{5000, 1000, 19}, {5040, 1040, 19}, {5119, 1080, 19}, {5159, 1120, 19}};
        HOST_EXPECT(pieces_are(ref_chain_group(b, o), {{0, 0, FP{{982, 4982}, {1001, 5001}, {1041, 5041}, {1081, 5120}, {1121, 5160}}}}));
    }
    {   // 6. a clamped start: the first anchor ends at query base 4 (exclusive end 5): 5 - 19 = -14, the start moves 14 along the
        // diagonal: (0, 5001 - 19 + 14 = 4996).  In the target: ends at 7 (exclusive 8): 8 - 19 = -11 -> (1001 - 19 + 11 = 993, 0)
        const std::vector<Anc> a = {{5000, 4, 19}, {5040, 44, 19}, {5080, 84, 19}};
        HOST_EXPECT(pieces_are(ref_chain_group(a, o), {{0, 0, FP{{0, 4996}, {5, 5001}, {45, 5041}, {85, 5081}}}}));
        const std::vector<Anc> b = {{7, 1000, 19}, {47, 1040, 19}, {87, 1080, 19}};
        HOST_EXPECT(pieces_are(ref_chain_group(b, o), {{0, 0, FP{{993, 0}, {1001, 8}, {1041, 48}, {1081, 88}}}}));
    }
    {   // 7. equal children: anchors 2 and 3 (one query position) are both children of 1 with f = 57 and 57 - gamma(3) = 57: the
        // smaller index keeps the trunk, 3 starts a chain of its own with parent f = 38: anchor 4 hangs on 3 (later, tie 76 = 76):
        // chain 3 = 3, 4 scores 76 - 38 = 38 < 40 (dropped), chain 0 = 0, 1, 2 scores 57
        const std::vector<Anc> a = {{5000, 1000, 19}, {5030, 1030, 19}, {5060, 1060, 19}, {5063, 1060, 19}, {5100, 1100, 19}};
        const auto r = ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT((f == std::vector<int>{19, 38, 57, 57, 76}) && (p == std::vector<int>{-1, 0, 1, 1, 3}));
        HOST_EXPECT(pieces_are(r, {{0, 0, FP{{982, 4982}, {1001, 5001}, {1061, 5061}}}}));
    }
    {   // 8. the window: 66 anchors one query base apart on one target diagonal chain one after the other (+1 each: min(19, 1)):
        // f(i) = 19 + i.  An anchor 65 back is never asked: remove the chain between by making anchors 1 .. 64 strays (dr = 0 among
        // them, far off the band of 0 and 65): anchor 65 then starts a chain although anchor 0 is 65 / 65 away
        std::vector<Anc> a = {{5000, 1000, 19}};
        for (int i = 1; i <= 64; ++i) a.push_back(Anc{90000, 1000 + i, 19});
        a.push_back(Anc{5065, 1065, 19});
        ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT(p[65] == -1 && f[65] == 19);
        a.erase(a.begin() + 1);                                 // 64 back: taken, 19 + 19
        ref_chain_group(a, o, nullptr, &f, &p);
        HOST_EXPECT(p[64] == 0 && f[64] == 38);
    }
    host_done();

    g_group = "ref_index";
    {   // two targets in one chunk, f = 0.5, min_mid_occ = 1.  Hash 5 three times (t0 twice, t1 once), hash 9 once, hash 2 twice,
        // hash 7 five times: counts sorted 1 2 3 5, quantile index floor(0.5 * 4) = 2 -> 3, cut-off 4: hash 7 is too frequent
        World w;
        w.k = 19;
        w.add_target(1000, 1); w.add_target(1000, 0);
        w.t_entry(0, 5, 10); w.t_entry(0, 7, 20); w.t_entry(0, 5, 30); w.t_entry(0, 2, 40); w.t_entry(0, 7, 50); w.t_entry(0, 7, 60);
        w.t_entry(1, 7, 5); w.t_entry(1, 9, 15); w.t_entry(1, 5, 25); w.t_entry(1, 2, 35); w.t_entry(1, 7, 45);
        hlmi_ava_opts io = base_opts();
        io.min_mid_occ = 1; io.mid_occ_frac = 0.5;
        const RefIndex r = ref_index(w, io, false);
        HOST_EXPECT(r.mid_occ == std::vector<uint32_t>{4});
        // by hash; rank word = rank + 1 (t0: 2, t1: 1), hash 7: 0 everywhere, in (target, position) order
        HOST_EXPECT((r.key == std::vector<uint64_t>{2, 2, 5, 5, 5, 7, 7, 7, 7, 7, 9}));
        HOST_EXPECT((r.rk == std::vector<uint32_t>{1, 2, 1, 2, 2, 0, 0, 0, 0, 0, 1}));
        const uint64_t T1 = 1ull << 32;
        HOST_EXPECT((r.y == std::vector<uint64_t>{T1 | 70, 80, T1 | 50, 20, 60, 40, 100, 120, T1 | 10, T1 | 90, T1 | 30}));
        // 2 names: rank words up to 2, three values and 0: bits for 3 = 2; 11 entries: one bucket bit, shift 37
        HOST_EXPECT(r.rank_bits == 2 && r.bucket_bits == 1 && r.bucket_shift == 37 && (r.bucket == std::vector<uint32_t>{0, 11, 11}));
        HOST_EXPECT(r.ck[0] == (2u << 2 | 1u) && r.ck[5] == (7u << 2) && r.ck[10] == (9u << 2 | 1u));
        // the same with a cut-off of 2 by the clamp: f <= 0 -> min_mid_occ = 2: hashes 5 and 7 too frequent
        io.mid_occ_frac = 0; io.min_mid_occ = 2;
        const RefIndex r2 = ref_index(w, io, false);
        HOST_EXPECT(r2.mid_occ == std::vector<uint32_t>{2} && (r2.rk == std::vector<uint32_t>{1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1}));
        // seeds, pair-once: a query of rank 0 (the name of t1) with hashes 2 and 5 pairs with t0 only (rank 1 > 0)
        io.mid_occ_frac = 0.5; io.min_mid_occ = 1;
        w.add_query(500, 0);
        w.q_entry(0, 2, 100, 1, 19); w.q_entry(0, 5, 200, 0, 19); w.q_entry(0, 7, 300); w.q_entry(0, 11, 400);
        const RefSeeds s = ref_seeds(w, r, 1);
        HOST_EXPECT((s.cnt == std::vector<uint32_t>{1, 2, 0, 0}) && s.per_query == std::vector<uint64_t>{3});
        HOST_EXPECT(s.lo[0] == 1 && s.len[0] == 1 && s.lo[1] == 3 && s.len[1] == 2 && s.len[2] == 0 && s.len[3] == 0);
        // reverse strand: ql - (qpos + 1 - span) - 1 = 500 - (100 + 1 - 19) - 1 = 417
        const std::vector<Anc> &rev = s.groups[0].at({0, 1});
        HOST_EXPECT(rev.size() == 1 && rev[0].q == 417 && rev[0].t == 40 && rev[0].sp == 19);
        const std::vector<Anc> &fwd = s.groups[0].at({0, 0});
        HOST_EXPECT(fwd.size() == 2 && fwd[0].t == 10 && fwd[1].t == 30 && fwd[0].q == 200);
        // both directions: t1 is the read itself (equal rank) and is skipped; the run still spans the hash's entries
        const RefSeeds s2 = ref_seeds(w, r, 0);
        HOST_EXPECT((s2.cnt == std::vector<uint32_t>{1, 2, 0, 0}) && s2.lo[0] == 0 && s2.len[0] == 2 && s2.lo[1] == 2 && s2.len[1] == 3);
    }
    {   // two chunks with a cut-off each: chunk 0 holds hash 3 four times and hash 4 once (counts 1 4 -> index 1 -> 4, cut-off 5);
        // chunk 1 holds hash 3 once and hash 8 twice (1 2 -> 2, cut-off 3): occurrences count inside the chunk only
        World w;
        w.k = 19;
        w.add_target(1000, 0, 0); w.add_target(1000, 1, 1);
        for (int i = 0; i < 4; ++i) w.t_entry(0, 3, 10 * i);
        w.t_entry(0, 4, 100);
        w.t_entry(1, 3, 7); w.t_entry(1, 8, 17); w.t_entry(1, 8, 27);
        hlmi_ava_opts io = base_opts();
        io.min_mid_occ = 1; io.mid_occ_frac = 0.5;
        const RefIndex r = ref_index(w, io, false);
        HOST_EXPECT((r.mid_occ == std::vector<uint32_t>{5, 3}));
        HOST_EXPECT((r.rk == std::vector<uint32_t>{1, 1, 1, 1, 2, 1, 2, 2}));
        io.mid_occ_frac = 0.75;                                  // index floor(0.25 * 2) = 0: cut-offs 2 and 2: hash 3 of chunk 0 goes
        const RefIndex r2 = ref_index(w, io, false);
        HOST_EXPECT((r2.mid_occ == std::vector<uint32_t>{2, 2}));
        HOST_EXPECT((r2.key == std::vector<uint64_t>{3, 3, 3, 3, 3, 4, 8, 8}) && (r2.rk == std::vector<uint32_t>{0, 0, 0, 0, 2, 1, 2, 2}));
    }
    host_done();
    return 0;
}

// ------------------------------------------------------------------------------------------
// --dump / --cases
// ------------------------------------------------------------------------------------------
int run_dump(const char *path) {
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return 64; }
    std::string word;
    size_t gi = 0;
    while (f >> word) {
        if (word != "group") { fprintf(stderr, "bad file\n"); return 64; }
        ChainOpt o;
        int n;
        f >> o.k >> o.max_gap >> o.bw >> o.min_score >> o.min_cnt >> n;
        std::vector<Anc> a(n);
        for (Anc &x : a) f >> x.t >> x.q >> x.sp;
        const std::vector<RefPiece> r = ref_chain_group(a, o);
        printf("group %zu pieces=%zu\n", gi++, r.size());
        for (const RefPiece &p : r) {
            printf("%u %u %zu", p.chain, p.piece, p.fp.size());
            for (const auto &x : p.fp) printf(" %d %d", x.first, x.second);
            printf("\n");
        }
    }
    return 0;
}
int run_cases(const char *path) {
    FILE *f = fopen(path, "w");
    if (!f) return 64;
    std::set<std::string> seen;
    for (const ChainCase &c : chain_cases()) {
        if (c.hook) continue;                                     // the same groups once more under a hook
        // the generator holds here already: the world's anchors lie inside the reads and form the wanted groups in the wanted order
        g_group = c.group.c_str();
        g_case = c.name;
        try {
            size_t n_q, n_t;
            const std::vector<WantGroup> want = want_groups(c, n_q, n_t);
            const World w = world_of(want, n_q, n_t, c.ql, c.tl, c.o.k);
            hlmi_ava_opts o = c.o;
            o.mid_occ_frac = 0; o.min_mid_occ = 10;
            expect_groups(want, ref_seeds(w, ref_index(w, o, false), o.pair_once));
        } catch (const Mismatch &) {
            fclose(f);
            return 1;
        }
        for (const auto &g : c.groups) {
            fprintf(f, "group %d %d %d %d %d %zu\n", c.o.k, c.o.max_gap, c.o.bandwidth, c.o.min_chain_score, c.o.min_cnt, g.size());
            for (const Anc &a : g) fprintf(f, "%d %d %d\n", a.t, a.q, a.sp);
        }
    }
    fclose(f);
    return 0;
}

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
void group_done() {
    printf("group %s cases=%zu ok\n", g_group, g_cases);
    fflush(stdout);
}
struct HookScope {                                // sets an existing test hook of the library for the scope
    std::string name;
    HookScope(const char *n, const char *value = "1") : name(n ? n : "") {
        if (!name.empty()) { setenv(name.c_str(), value, 1); hooks_refresh(); }
    }
    ~HookScope() { if (!name.empty()) { unsetenv(name.c_str()); hooks_refresh(); } }
};
bool hook_set(const char *n) { const char *e = getenv(n); return e && *e; }

struct DevWorld {
    DevReads T, Q;
    DevSketch tsk;
    DBuf<uint32_t> d_rank_t, d_rank_q, d_chunk, d_qlen, d_tlen;
    DBuf<Mz> d_qmz;
    AvaInput in;
    template <typename V> static void up(DBuf<V> &d, std::vector<V> h) { if (h.empty()) h.push_back(V{}); d.upload(h); }
    explicit DevWorld(const World &w) {
        T.n = w.tlen.size(); Q.n = w.qlen.size();
        T.h_off.assign(1, 0); Q.h_off.assign(1, 0);
        for (uint64_t l : w.tlen) T.h_off.push_back(T.h_off.back() + l);
        for (uint64_t l : w.qlen) Q.h_off.push_back(Q.h_off.back() + l);
        T.total = T.h_off.back(); Q.total = Q.h_off.back();
        std::vector<Mz> tm, qm;
        in.qmz_off.assign(1, 0);
        // (a hash has 2k bits: seed_kernel takes its bucket from the top bits of the query's hash)
        for (const auto &v : w.tmz) for (const Mz &m : v) expect_true("generator: target hash within 2k bits", ((m.x >> 8) >> 2 * w.k) == 0, m.x >> 8, (unsigned long long)w.k);
        for (const auto &v : w.qmz) for (const Mz &m : v) expect_true("generator: query hash within 2k bits", ((m.x >> 8) >> 2 * w.k) == 0, m.x >> 8, (unsigned long long)w.k);
        for (const auto &v : w.tmz) tm.insert(tm.end(), v.begin(), v.end());
        for (const auto &v : w.qmz) { qm.insert(qm.end(), v.begin(), v.end()); in.qmz_off.push_back(qm.size()); }
        tsk.n = tm.size();
        up(tsk.mz, tm);
        up(d_qmz, qm);
        up(d_rank_t, w.rank_t); up(d_rank_q, w.rank_q); up(d_chunk, w.chunk_of_t);
        std::vector<uint32_t> ql, tl;
        for (uint64_t l : w.qlen) ql.push_back((uint32_t)l);
        for (uint64_t l : w.tlen) tl.push_back((uint32_t)l);
        up(d_qlen, ql); up(d_tlen, tl);
        in.T = &T; in.Q = &Q; in.d_rank_t = d_rank_t.p; in.d_rank_q = d_rank_q.p; in.n_ranks = w.n_ranks;
        in.d_chunk_of_t = d_chunk.p; in.n_chunks = w.n_chunks; in.d_qmz = d_qmz.p;
        sync();
    }
};

void check_index(const World &w, const hlmi_ava_opts &o, DevWorld &d, DevIndex &ix, RefIndex &ref) {
    ref = ref_index(w, o, hook_set("HLMI_NO_RANK_WORD"));
    build_index(d.tsk, d.d_chunk.p, d.d_rank_t.p, w.n_chunks, w.n_ranks, o, ix);
    if (hook_set("HLMI_SEED_GROUP")) seed_group_prepare(d.in, ix);      // once per index, as ava_device does under the hook
    const size_t n = ref.key.size();
    expect_one("index n", n, ix.n);
    expect_eq("index key", ref.key, ix.key.download(n));
    expect_eq("index y", ref.y, ix.y.download(n));
    expect_eq("index rk", ref.rk, ix.rk.download(n));
    expect_eq("index mid_occ", ref.mid_occ, ix.mid_occ.download(w.n_chunks));
    expect_one("index rank_bits", (unsigned long long)ref.rank_bits, (unsigned long long)ix.rank_bits);
    if (ref.rank_bits) expect_eq("index ck", ref.ck, ix.ck.download(n));
    expect_one("index bucket_bits", (unsigned long long)ref.bucket_bits, (unsigned long long)ix.bucket_bits);
    expect_one("index bucket_shift", (unsigned long long)ref.bucket_shift, (unsigned long long)ix.bucket_shift);
    expect_eq("index bucket", ref.bucket, ix.bucket.download(ref.bucket.size()));
    expect_one("index pair_once", (unsigned long long)o.pair_once, (unsigned long long)ix.pair_once);
}
void check_plan(const World &w, const hlmi_ava_opts &o, DevWorld &d, const DevIndex &ix, const RefIndex &rix, SeedPlan &plan, RefSeeds &ref) {
    ref = ref_seeds(w, rix, o.pair_once);
    plan_seeds(d.in, ix, plan);
    const size_t n = ref.cnt.size();
    expect_eq("plan per_query", ref.per_query, plan.per_query);
    if (!n) return;
    expect_eq("plan cnt", ref.cnt, plan.cnt.download(n));
    if (!ix.n) return;                                           // (no index: the plan is zeros, no run was looked for)
    const std::vector<uint32_t> lo = plan.lo.download(n), len = plan.len.download(n);
    expect_eq("plan len", ref.len, len);
    for (size_t i = 0; i < n; ++i) if (ref.len[i] && ref.lo[i] != lo[i]) mismatch("plan lo", i, ref.lo[i], lo[i]);
}
struct RunResult { RefChains ref; double small = 0, full_dp = 0, grouped = 0; bool group_path = false; };
RunResult check_chains(const hlmi_ava_opts &o, DevWorld &d, const DevIndex &ix, const SeedPlan &plan, const RefSeeds &rs, size_t q_lo, size_t q_hi) {
    RunResult rr;
    rr.ref = ref_chains(rs, chain_opt(o), q_lo, q_hi);
    // HLMI_SEED_GROUP: does the batch take seed_group.hip?  The widths as seed_and_chain derives them from the reads' lengths
    if (hook_set("HLMI_SEED_GROUP") && o.pair_once && rr.ref.anchors) {
        uint64_t max_tlen = 1, max_qlen = 1;
        for (size_t t = 0; t < d.T.n; ++t) max_tlen = std::max<uint64_t>(max_tlen, d.T.h_off[t + 1] - d.T.h_off[t]);
        for (size_t q = q_lo; q < q_hi; ++q) max_qlen = std::max<uint64_t>(max_qlen, d.Q.h_off[q + 1] - d.Q.h_off[q]);
        rr.group_path = seed_group_supported(ix, rr.ref.anchors, std::max(1, bit_length(max_tlen)), std::max(1, bit_length(max_qlen)));
    }
    ChainOut out;
    SeedStats st;
    stat_reset();
    seed_and_chain(d.in, ix, o, plan, d.d_qlen.p, d.d_tlen.p, q_lo, q_hi, out, st);
    sync();
    {   // the batch went through seed_group.hip exactly when it could: no quiet return to the sort path
        auto &sg = stats();
        rr.grouped = sg.count("anchors_grouped_in_lds") ? sg["anchors_grouped_in_lds"] : 0;
        expect_one("anchors_grouped_in_lds", rr.group_path ? rr.ref.anchors : 0, (unsigned long long)rr.grouped);
    }
    expect_one("anchors", rr.ref.anchors, st.anchors);
    expect_one("groups", rr.ref.groups, st.groups);
    expect_one("n_pieces", rr.ref.pieces.size(), out.n_pieces);
    expect_one("n_fp", rr.ref.n_fp, out.n_fp);
    if (out.n_pieces) {
        const std::vector<Piece> pc = out.pieces.download(out.n_pieces);
        const std::vector<FixPt> fp = out.fps.download(out.fps.n);
        PieceMap got;
        for (size_t i = 0; i < pc.size(); ++i) {
            const Piece &p = pc[i];
            expect_true("piece fixed points inside the array", (size_t)p.fp_off + p.n_fp <= fp.size(), p.fp_off, p.n_fp);
            std::vector<std::pair<int, int>> v;
            for (uint32_t x = 0; x < p.n_fp; ++x) v.push_back({(int)fp[p.fp_off + x].q, (int)fp[p.fp_off + x].t});
            const PieceKey key{p.q, p.t, p.strand, p.chain, p.piece};
            expect_true("piece reported once", got.find(key) == got.end(), p.q, p.chain);
            got[key] = v;
        }
        auto a = rr.ref.pieces.begin();
        auto b = got.begin();
        for (size_t i = 0; a != rr.ref.pieces.end(); ++a, ++b, ++i) {
            if (a->first != b->first)
                mismatch("piece key (chain of the first differing piece)", i, std::get<3>(a->first), std::get<3>(b->first));
            if (a->second.size() != b->second.size()) mismatch("piece n_fp", i, a->second.size(), b->second.size());
            for (size_t x = 0; x < a->second.size(); ++x) {
                if (a->second[x].first != b->second[x].first) mismatch("fixed point q", i * 1000 + x, a->second[x].first, b->second[x].first);
                if (a->second[x].second != b->second[x].second) mismatch("fixed point t", i * 1000 + x, a->second[x].second, b->second[x].second);
            }
        }
    }
    auto &s = stats();
    rr.small = s.count("chain_groups_small") ? s["chain_groups_small"] : 0;
    rr.full_dp = s.count("chain_groups_full_dp") ? s["chain_groups_full_dp"] : 0;
    return rr;
}
// index, plan and chains of a world; the chains in two batches, the second not starting at query 0
struct WorldResult { RefIndex rix; RefSeeds rs; std::vector<RunResult> runs; };
WorldResult check_world(const World &w, const hlmi_ava_opts &o, bool chains = true) {
    WorldResult r;
    DevWorld d(w);
    DevIndex ix;
    check_index(w, o, d, ix, r.rix);
    SeedPlan plan;
    check_plan(w, o, d, ix, r.rix, plan, r.rs);
    if (!chains) return r;
    const size_t nQ = w.qlen.size();
    r.runs.push_back(check_chains(o, d, ix, plan, r.rs, 0, nQ));
    if (nQ > 1) {
        r.runs.push_back(check_chains(o, d, ix, plan, r.rs, 1, nQ));
        r.runs.push_back(check_chains(o, d, ix, plan, r.rs, 0, 1));
    }
    return r;
}

// the anchors themselves, through the isolating options: every anchor a chain of one piece (see the head of the file)
void check_anchors(const World &w, const hlmi_ava_opts &o) {
    size_t n_mz = 0;
    for (const auto &v : w.qmz) n_mz += v.size();
    const WorldResult r = check_world(w, isolating(o));
    expect_true("isolating options: the batch fits the piece array", r.runs[0].ref.anchors <= 2048, r.runs[0].ref.anchors, n_mz);
    expect_one("isolating options: one piece per anchor", r.runs[0].ref.anchors, r.runs[0].ref.pieces.size());
}

size_t g_grouped_runs = 0;                        // cases whose whole batch went through seed_group.hip
void run_chain_case(const ChainCase &c) {
    set_case("%s", c.name.c_str());
    size_t n_q, n_t;
    const std::vector<WantGroup> want = want_groups(c, n_q, n_t);
    const World w = world_of(want, n_q, n_t, c.ql, c.tl, c.o.k);
    HookScope hs(c.hook);
    hlmi_ava_opts o = c.o;
    o.mid_occ_frac = 0; o.min_mid_occ = 10;
    const WorldResult r = check_world(w, o);
    expect_groups(want, r.rs);
    const RunResult &all = r.runs[0];
    if (all.group_path) expect_one("chain_groups_small", all.ref.small_kept, (unsigned long long)all.small);
    else if (!c.hook || strcmp(c.hook, "HLMI_CHAIN_NO_SMALL") != 0) expect_one("chain_groups_small", all.ref.small, (unsigned long long)all.small);
    else expect_one("chain_groups_small", 0, (unsigned long long)all.small);
    if (all.group_path) ++g_grouped_runs;
    if (c.group == "chain_window") {
        const bool dp16 = !c.hook || strcmp(c.hook, "HLMI_CHAIN_NO_SMALL") == 0;
        const size_t big = c.hook && !strcmp(c.hook, "HLMI_CHAIN_NO_SMALL") ? all.ref.groups : all.ref.big;
        expect_true("reference: a big group with a predecessor 17 .. 64 back", all.ref.big_far > 0);
        if (dp16) {
            expect_true("chain_groups_full_dp >= big groups with a far predecessor", all.full_dp >= (double)all.ref.big_far, all.ref.big_far, (unsigned long long)all.full_dp);
            expect_true("chain_groups_full_dp < big groups (collinear ones are proven)", all.full_dp < (double)big, big, (unsigned long long)all.full_dp);
        }
    }
    // the anchors of the same world through the isolating options (one word; the forms are seed_fill's business)
    // where the batch fits the piece array (anchors / 2 + 1024 pieces: up to 2048 anchors)
    if (!c.hook && all.ref.anchors <= 2048) {
        set_case("%s/anchors", c.name.c_str());
        check_anchors(w, o);
    }
}
void run_chain_group(const char *name) {
    g_group = name; g_cases = 0;
    for (const ChainCase &c : chain_cases()) if (c.group == name) run_chain_case(c);
    group_done();
}
// the chain_* and emit_* sets once more with the anchors grouped by seed_group.hip (HLMI_SEED_GROUP, after seed_group_prepare)
// where seed_group_supported holds: the kernels then read their groups from records (gsize / gq / gts), not from the sorted batch.
// A batch that may take the path must take it (anchors_grouped_in_lds = its anchors), one that may not (a target of 2^28
// bases: 32-bit index entries have no room) must not.
void group_seed_group() {
    g_group = "seed_group"; g_cases = 0;
    HookScope hs("HLMI_SEED_GROUP");
    g_grouped_runs = 0;
    size_t n_run = 0;
    for (const ChainCase &c : chain_cases())
        if (!c.hook) { run_chain_case(c); ++n_run; }
    expect_true("most cases took the grouped path", g_grouped_runs + 4 >= n_run && g_grouped_runs > 0, n_run, g_grouped_runs);
    group_done();
}

// ------------------------------------------------------------------------------------------
// index_cutoff
// ------------------------------------------------------------------------------------------
// `count` occurrences of a hash on target t, at fresh positions
void occ(World &w, size_t t, uint64_t hash, int count, uint32_t &pos) { for (int i = 0; i < count; ++i) w.t_entry(t, hash, pos += 3); }

void group_index_cutoff() {
    g_group = "index_cutoff"; g_cases = 0;
    hlmi_ava_opts o = base_opts();
    o.min_mid_occ = 1; o.mid_occ_frac = 0.5;
    auto run = [&](const World &w, const hlmi_ava_opts &oo, double exact) {
        stat_reset();
        check_world(w, oo, false);
        auto &s = stats();
        expect_one("index_exact_quantiles", (unsigned long long)exact, (unsigned long long)(s.count("index_exact_quantiles") ? s["index_exact_quantiles"] : 0));
    };
    // counts around the cut-off: 1 9 10 11 12 -> index 2 -> 10, cut-off 11: the hash with 11 stays, the one with 12 goes
    for (int chunks : {1, 2, 257}) {
        set_case("at_and_above/chunks%d", chunks);
        World w;
        uint32_t pos = 0;
        for (int c = 0; c < chunks; ++c) {
            const size_t t = w.add_target(100000, (uint32_t)c, (uint32_t)c), t2 = w.add_target(100000, (uint32_t)(chunks + c), (uint32_t)c);
            int h = 100;
            for (int cnt : {1, 9, 10, 11, 12}) { occ(w, t, (uint64_t)h, cnt / 2, pos); occ(w, t2, (uint64_t)h, cnt - cnt / 2, pos); ++h; }
            // run lengths 7 / 8 / 9 (HIST_LDS_LEN 8) are in: 9 and 10, 11, 12 go straight to memory, 1 through LDS; add 7 and 8
            occ(w, t, 200, 7, pos); occ(w, t2, 201, 8, pos);
        }
        w.add_query(1000, 0);
        w.q_entry(0, 103, 50); w.q_entry(0, 104, 60);
        run(w, o, 0);
        set_case("at_and_above/chunks%d/f0", chunks);            // f <= 0: the cut-off is min_mid_occ
        hlmi_ava_opts f0 = o;
        f0.mid_occ_frac = 0; f0.min_mid_occ = 9;
        run(w, f0, 0);
        f0.mid_occ_frac = -1;
        run(w, f0, 0);
        set_case("at_and_above/chunks%d/clamp", chunks);         // quantile + 1 = 11 below min_mid_occ = 12: everything stays
        hlmi_ava_opts cl = o;
        cl.min_mid_occ = 12;
        run(w, cl, 0);
    }
    // the quantile run length at the end of the 1024-bin histogram: counts 1, L, L + 700 -> index 1 -> L; L >= 1023 leaves the
    // histogram (its last bin collects everything from 1023 on): exact quantile, with the runs of the chunks ahead as its offset
    for (int where = 0; where < 3; ++where)                      // chunk 0 of one, chunk 0 of three, chunk 2 of three
        for (int L : {1022, 1023, 1024}) {
            set_case("quantile%d/%s", L, where == 0 ? "one_chunk" : where == 1 ? "chunk0_of_3" : "chunk2_of_3");
            World w;
            uint32_t pos = 0;
            const int n_chunks = where ? 3 : 1, hot = where == 2 ? 2 : 0;
            for (int c = 0; c < n_chunks; ++c) {
                const size_t t = w.add_target(1 << 20, (uint32_t)c, (uint32_t)c);
                if (c == hot) { occ(w, t, 50, 1, pos); occ(w, t, 60, L, pos); occ(w, t, 70, L + 700, pos); }
                else { occ(w, t, 50, 2, pos); occ(w, t, 61, 5, pos); occ(w, t, 62, 5, pos); occ(w, t, 70, 9, pos); occ(w, t, 71, 1, pos); }
            }
            run(w, o, L >= 1023 ? 1 : 0);
        }
    group_done();
}

// ------------------------------------------------------------------------------------------
// index_order
// ------------------------------------------------------------------------------------------
void group_index_order() {
    g_group = "index_order"; g_cases = 0;
    hlmi_ava_opts o = base_opts();
    o.min_mid_occ = 3; o.mid_occ_frac = 0;
    // n entries over four targets, two of them with one name; hashes repeat inside a target and over targets, some too frequent
    for (int n : {0, 1, 2, 15, 16, 17, 31, 32, 33, 300}) {
        for (int norank = 0; norank < 2; ++norank) {
            set_case("n%d%s", n, norank ? "/no_rank_word" : "");
            HookScope hs(norank ? "HLMI_NO_RANK_WORD" : nullptr);
            World w;
            const uint32_t ranks[4] = {2, 0, 2, 1};
            for (int t = 0; t < 4; ++t) w.add_target(100000, ranks[t]);
            for (int i = 0; i < n; ++i) w.t_entry(rnd() % 4, 1 + rnd() % (uint64_t)std::max(1, n / 3), (uint32_t)(10 * i), (int)(rnd() & 1));
            w.sort_positions();
            w.add_query(1000, 1);
            for (uint64_t h = 0; h < 6; ++h) w.q_entry(0, h, (uint32_t)(20 * h));
            check_world(w, o, false);
            hlmi_ava_opts both = o;
            both.pair_once = 0;
            check_world(w, both, false);
        }
    }
    // bucket_bits capped by 2k: k = 3 with 2000 entries (bits_for(125) = 7 > 6)
    set_case("k3_bucket_cap");
    {
        World w;
        w.k = 3;
        for (int t = 0; t < 5; ++t) w.add_target(100000, (uint32_t)t);
        for (int i = 0; i < 2000; ++i) w.t_entry(rnd() % 5, rnd() & 63, (uint32_t)(10 * i));
        w.sort_positions();
        w.add_query(1000, 0);
        w.q_entry(0, 63, 10); w.q_entry(0, 0, 20);
        hlmi_ava_opts k3 = o;
        k3.k = 3; k3.min_mid_occ = 100;
        const WorldResult r = check_world(w, k3, false);
        expect_one("bucket_bits", 6, (unsigned long long)r.rix.bucket_bits);
    }
    // rank_bits = 0 reached by widths: k = 27 (54 key bits) and 1023 names need 11 bits of rank word
    for (int names : {1022, 1023}) {
        set_case("k27_names%d", names);
        World w;
        w.k = 27;
        for (int t = 0; t < names - 1; ++t) w.add_target(4000, (uint32_t)(t + 1));
        for (int i = 0; i < 3000; ++i) w.t_entry(rnd() % (uint64_t)(names - 1), (rnd() % 40) << 48 | rnd() % 7, (uint32_t)i);
        w.sort_positions();
        w.add_query(1000, 0);
        for (uint64_t h = 0; h < 40; ++h) w.q_entry(0, h << 48 | 3, (uint32_t)(20 * h));
        hlmi_ava_opts k27 = o;
        k27.k = 27; k27.min_mid_occ = 1000;
        const WorldResult r = check_world(w, k27);
        expect_one("rank_bits", names == 1023 ? 0 : 10, (unsigned long long)r.rix.rank_bits);
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// seed_count: the 16-word bucket fetch and the 16-word guess window of seed_kernel<false>
// ------------------------------------------------------------------------------------------
void group_seed_count() {
    g_group = "seed_count"; g_cases = 0;
    // ONE hash carried by n_t targets of even rank 2 i (positions 100 + i), `head` smaller hashes in front of it and `tail` larger
    // ones behind it in the same bucket (all keys are tiny: bucket 0).  Queries of every rank 0 .. 2 n_t + 1 carry the hash: the
    // first partner of rank r sits at r / 2 of the run - the guess window answers inside, before and behind itself and is clamped
    // at either end; queries of even rank are a target's own name: their entries sit at the start, in the middle, at the end of a run.
    for (int n_t : {1, 12, 13, 14, 15, 16, 17, 33, 40, 100})
        for (int head : {0, 3})
            for (int tail : {0, 2}) {
                World w;
                for (int t = 0; t < n_t; ++t) { w.add_target(10000, (uint32_t)(2 * t + 2)); w.t_entry(t, 500, (uint32_t)(100 + t), t & 1); }
                for (int i = 0; i < head; ++i) w.t_entry(i % n_t, 490 + i, 7);
                for (int i = 0; i < tail; ++i) w.t_entry((i + 1) % n_t, 510 + i, 9);
                w.sort_positions();
                w.add_query(900, 0);                             // a query without minimizers first ...
                for (int r = 0; r <= 2 * n_t + 3; ++r) {
                    const size_t q = w.add_query(1000, (uint32_t)r);
                    w.q_entry(q, 500, 300);
                    if (r % 3 == 0) { w.q_entry(q, 490, 310); w.q_entry(q, 511, 320); w.q_entry(q, 700, 330); }
                    if (r == n_t) w.add_query(800, (uint32_t)r); // ... in the middle ...
                }
                w.add_query(700, 1);                             // ... and last
                hlmi_ava_opts o = base_opts();
                o.mid_occ_frac = 0; o.min_mid_occ = 1000;
                for (int po = 0; po < 2; ++po)
                    for (int hk = 0; hk < 3; ++hk) {
                        set_case("targets%d_head%d_tail%d/%s/%s", n_t, head, tail, po ? "pair_once" : "both", hk == 0 ? "plain" : hk == 1 ? "no_guess" : "no_rank_word");
                        HookScope hs(hk == 1 ? "HLMI_SEED_NO_GUESS" : hk == 2 ? "HLMI_NO_RANK_WORD" : nullptr);
                        o.pair_once = po;
                        check_world(w, o, false);
                    }
            }
    group_done();
}

// ------------------------------------------------------------------------------------------
// seed_fill: SHORT_RUN 32, four short runs at a time, the anchor word forms
// ------------------------------------------------------------------------------------------
// One query whose minimizers have runs of the given lengths (run i: that many targets carry hash i), spans 1 and 255 among
// them, both strands; a second query with the same on other positions
World fill_world(const std::vector<int> &runs, size_t n_t, uint64_t ql, uint64_t tl, size_t n_q = 2) {
    World w;
    for (size_t q = 0; q < n_q; ++q) w.add_query(ql, (uint32_t)q);
    for (size_t t = 0; t < n_t; ++t) w.add_target(tl, (uint32_t)(n_q + t));
    for (size_t q = 0; q < n_q; ++q)
        for (size_t i = 0; i < runs.size(); ++i) {
            const uint64_t h = fresh_hash(19);
            const int span = i % 5 == 0 ? 1 : i % 5 == 1 ? 255 : 19 + (int)(i % 7);
            const uint32_t qpos = (uint32_t)(300 + 40 * i + (ql > 100000 ? ql - 100000 : 0));
            w.q_entry(q, h, qpos, (int)(i & 1), span);
            for (int e = 0; e < runs[i]; ++e) {
                const size_t t = (size_t)((i * 7 + (size_t)e * (n_t > 200 ? n_t / 150 : 1)) % n_t);
                w.t_entry(t, h, (uint32_t)(tl - 1 - (uint64_t)(13 * i + e)), (int)((i >> 1) & 1), span);
            }
        }
    w.sort_positions();
    return w;
}
void group_seed_fill() {
    g_group = "seed_fill"; g_cases = 0;
    hlmi_ava_opts o = base_opts();
    o.mid_occ_frac = 0; o.min_mid_occ = 1000;
    const std::vector<int> lens = {0, 1, 16, 17, 32, 33, 64, 65, 129, 0, 0, 5, 0, 31, 2, 0, 0, 0, 0, 3, 1, 1, 1, 32, 0, 32};
    std::vector<int> many = lens;                                // more than 64 minimizers: a wave boundary inside the query
    // (seed_and_chain has room for anchors / 2 + 1024 pieces: a batch read through the isolating options stays below 2048 anchors)
    for (int i = 0; i < 60; ++i) many.push_back((int)(rnd() % 8 == 0 ? 33 + rnd() % 20 : rnd() % 4));
    struct Form { const char *name; size_t n_t; uint64_t ql, tl; const char *hook, *value; };
    const Form forms[] = {
        {"one_word", 140, 5000, 100000, nullptr, nullptr},
        // qbits 1 + tb + 1 + pb 28 + qpb 23 + 8: with 32768 targets tb = 15: 76 > 64 -> split, 16 key bits: 2 bytes; 32769: 4 bytes
        {"split_2byte_by_width", 32768, (1ull << 22) + 5, (1ull << 27) + 1, nullptr, nullptr},
        {"split_4byte_by_width", 32769, (1ull << 22) + 5, (1ull << 27) + 1, nullptr, nullptr},
        {"key_value_by_width", 140, 1ull << 24, 100000, nullptr, nullptr},             // qpb = 25 > 24
        {"split_2byte_by_hook", 140, 5000, 100000, "HLMI_ANCHOR_SPLIT", "1"},
        {"split_4byte_by_hook", 140, 5000, 100000, "HLMI_ANCHOR_SPLIT", "4"},
        {"key_value_by_hook", 140, 5000, 100000, "HLMI_ANCHOR_PAIRS", "1"},
    };
    for (const Form &f : forms)
        for (int which = 0; which < 2; ++which) {
            set_case("%s/%s", f.name, which ? "many_minimizers" : "run_lengths");
            const World w = fill_world(which ? many : lens, f.n_t, f.ql, f.tl);
            HookScope hs(f.hook, f.value ? f.value : "1");
            check_anchors(w, o);
            hlmi_ava_opts both = o;
            both.pair_once = 0;
            check_anchors(w, both);
        }
    // both directions with the read's own entries inside long and short runs: targets named like the queries
    set_case("own_entries_in_runs");
    {
        World w = fill_world(lens, 140, 5000, 100000);
        for (size_t t = 0; t < w.rank_t.size(); t += 9) w.rank_t[t] = (uint32_t)(t / 9 % 2);
        hlmi_ava_opts both = o;
        both.pair_once = 0;
        check_anchors(w, both);
        check_anchors(w, o);
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// refusal: limits are tested before anything is launched; the lengths are numbers
// ------------------------------------------------------------------------------------------
void group_refusal() {
    g_group = "refusal"; g_cases = 0;
    const hlmi_ava_opts o = base_opts();
    auto refused = [&](const char *name, size_t n_q, size_t n_t, uint64_t ql, uint64_t tl, size_t q_lo, size_t q_hi, bool want) {
        set_case("%s", name);
        World w;
        for (size_t q = 0; q < n_q; ++q) w.add_query(q == 0 ? ql : 1000, 0);
        for (size_t t = 0; t < n_t; ++t) w.add_target(t == 0 ? tl : 1000, 1);
        w.t_entry(0, 77, 500);
        w.q_entry(0, 77, 400);
        DevWorld d(w);
        DevIndex ix;
        build_index(d.tsk, d.d_chunk.p, d.d_rank_t.p, 1, w.n_ranks, o, ix);
        SeedPlan plan;
        plan_seeds(d.in, ix, plan);
        ChainOut out;
        SeedStats st;
        int code = 0;
        try {
            seed_and_chain(d.in, ix, o, plan, d.d_qlen.p, d.d_tlen.p, q_lo, q_hi, out, st);
        } catch (const Error &e) {
            if (e.code != HLMI_EINVAL) throw;
            code = e.code;
        }
        expect_one("error code (0: no refusal)", (unsigned long long)(long long)(want ? HLMI_EINVAL : 0), (unsigned long long)(long long)code);
        if (want) expect_one("anchors counted before the refusal", 0, st.anchors);
        else expect_one("pieces", 0, out.n_pieces);               // (one anchor: below min_cnt)
    };
    refused("queries_2_16_plus_1", (1u << 16) + 1, 2, 1000, 1000, 0, (1u << 16) + 1, true);
    refused("queries_2_16", (1u << 16) + 1, 2, 1000, 1000, 1, (1u << 16) + 1, false);
    refused("targets_2_21_plus_1", 2, (1u << 21) + 1, 1000, 1000, 0, 2, true);
    refused("target_2_29_bases", 2, 2, 1000, 1ull << 29, 0, 2, true);
    refused("target_2_29_minus_1_bases", 2, 2, 1000, (1ull << 29) - 1, 0, 2, false);
    refused("query_2_26_bases", 2, 2, 1ull << 26, 1000, 0, 2, true);
    refused("query_2_26_minus_1_bases", 2, 2, (1ull << 26) - 1, 1000, 0, 2, false);
    // 16 query + 21 target + 1 strand + 28 position bits = 66
    refused("key_over_64_bits", 1u << 16, 1u << 21, 1000, 1ull << 27, 0, 1u << 16, true);
    group_done();
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1) {
        if (argc == 2 && strcmp(argv[1], "--host") == 0) return run_host();
        if (argc == 3 && strcmp(argv[1], "--dump") == 0) return run_dump(argv[2]);
        if (argc == 3 && strcmp(argv[1], "--cases") == 0) return run_cases(argv[2]);
        fprintf(stderr, "usage: %s [--host | --dump FILE | --cases FILE]\n", argv[0]);
        return 64;
    }
    if (hlmi_init(0, 0) != HLMI_OK) { printf("hlmi_init: %s\n", hlmi_last_error()); return 2; }
    hooks_refresh();
    try {
        group_index_cutoff();
        group_index_order();
        group_seed_count();
        group_seed_fill();
        for (const char *g : {"chain_sizes", "chain_window", "chain_limits", "chain_ties", "emit_windows", "emit_splits"}) run_chain_group(g);
        group_refusal();
        group_seed_group();
    } catch (const Mismatch &) {
        return 1;
    } catch (const Error &e) {
        printf("ERROR group %s case %s: %s\n", g_group, g_case.c_str(), e.what());
        return 2;
    }
    hlmi_shutdown();
    return 0;
}
