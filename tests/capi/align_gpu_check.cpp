// align_gpu_check.cpp - a direct check of the alignment pass (csrc/ava_align.hip): align_pieces itself on FABRICATED pieces
// against plain sequential host C++, at the fixed sizes of the kernels.  Compiled as HIP by tests/test_gpu_align_direct.py and
// linked against libhylight_mi.so: it calls the hlmi:: functions themselves (the library exports them); no C-ABI entry point and
// no hook is added, existing hooks are set with setenv + hooks_refresh between runs.
//
//   align_gpu_check --host          what needs no device: the reference below against hand-worked literal cases, and against the
//                                   enumeration of all alignments on tasks up to 6 x 6
//   align_gpu_check --cases FILE    writes the device cases (no device needed): per case
//                                     case <name> / opts <20 ints, hlmi_ava_opts without mid_occ_frac> / reads <nQ> <nT> / one base
//                                     string per line / pieces <P> / per piece "q t strand chain piece n_fp q0 t0 q1 t1 ..."
//   align_gpu_check --dump FILE     the reference's rows for such a file: "case <i> <name>", then per piece "-" (dropped) or
//                                   "qs qe ts te nmatch blen cigar" (PAF columns 3, 4, 8, 9, 10, 11 and cg; "*" for a bare row)
//   align_gpu_check                 hlmi_init(0, 0), then the device groups in one process; one line "group <name> cases=<n> ok"
//                                   each, with "kept=<rows> dropped=<pieces>" behind the count
// Exit 1 at the first mismatch, exit 2 at the first HIP error or hlmi::Error; nothing is launched after either.  Everything is
// integer and compared exactly.
//
// A case uploads real bases (upload_reads, which packs them), fabricates the ChainOut - Piece records and FixPt lists written by
// the case, not by seed_and_chain -, d_qlen, d_tlen, name ranks and chunk slots, and calls align_pieces.
//
// INPUT CONTRACT.  The fixed points of a case stay inside what emit_chain (csrc/ava_chain.hip) can emit, DESIGN.md section 5
// item 5: n_fp >= 2; strictly increasing in both coordinates; inside both reads; |shift| of a block <= SHIFT_MAX (39), 0 under
// bandwidth 0; consecutive fixed points >= BLOCK_MIN (32) apart in both reads except before the last one; rows and columns of a
// block <= long_rows_cap(o).  (emit_chain's first block is a k-mer's span with shift 0; the pass treats it like any other
// block, and so do the cases.)  check_contract() refuses anything else: a
// case outside the contract is not a test of this layer.
//
// The reference is written from DESIGN.md section 5 items 5 and 7; it shares no code with the kernels or with
// oracle/ava_oracle.c.  Per task it holds full (m + 1) x (n + 1) tables of H, of the diagonal arrival and of the gap states of
// both pieces of the gap cost, with an explicit band mask, and walks back by comparing table values (no traceback bits).
// tests/test_gpu_align_direct.py compares --dump with the oracle (oracle.ava.align_pieces) on the CPU.
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>

#include "align_score_setup.h"
#include "ava_internal.h"

using namespace hlmi;

namespace {

struct Mismatch {};
const char *g_group = "";
std::string g_case;
size_t g_cases = 0, g_kept = 0, g_dropped = 0;

uint64_t g_rng = 0x9e3779b97f4a7c15ull;           // splitmix64, fixed seed
uint64_t rnd() {
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ z >> 27) * 0x94d049bb133111ebull;
    return z ^ z >> 31;
}
[[noreturn]] void mismatch(const char *what, size_t idx, long long want, long long got) {
    printf("MISMATCH group %s case %s %s index=%zu want=%lld got=%lld\n", g_group, g_case.c_str(), what, idx, want, got);
    fflush(stdout);
    throw Mismatch{};
}
void expect_one(const char *what, long long want, long long got, size_t idx = 0) { if (want != got) mismatch(what, idx, want, got); }
void expect_true(const char *what, bool ok, long long a = 0, long long b = 0) { if (!ok) mismatch(what, 0, a, b); }

// ------------------------------------------------------------------------------------------
// reference: one DP task
// ------------------------------------------------------------------------------------------
constexpr int NONE = -(1 << 28);                 // "no such cell / state"
struct Cost { int match, mismatch, ambi, open[2], ext[2]; int pieces; };
Cost cost_of(const hlmi_ava_opts &o, bool one_piece) {
    Cost c{o.match, o.mismatch, o.ambi, {o.gap_open, o.gap_open2}, {o.gap_ext, o.gap_ext2}, o.gap_open2 > 0 && !one_piece ? 2 : 1};
    return c;
}
int pair_score(const Cost &c, int a, int b) { return a > 3 || b > 3 ? -c.ambi : a == b ? c.match : -c.mismatch; }

std::vector<int> *g_drop_log = nullptr;       // case construction: best so far minus the row's best at rows 32, 64, ...
struct TaskResult {
    int score = 0, rank = 0;                     // extension: rank = score + bonus of the chosen cell
    int rows = 0, cols = 0;                      // cell the path ends in
    std::vector<uint8_t> ops;                    // one code per column of the alignment, in the order of the sequences given
};
// q[0, m), t[0, n): the task's sequences in walking order.  Band: diagonals j - i in [dlo, dlo + W).  ext: best cell instead of
// (m, n); bonus_row >= 0: the row that reaches the query end.
TaskResult ref_task(const uint8_t *q, int m, const uint8_t *t, int n, int dlo, int W, const Cost &c, bool ext, int bonus_row, int bonus,
                    int zdrop) {
    const int S = n + 1;
    std::vector<int> H((size_t)(m + 1) * S, NONE), D = H, E[2] = {H, H}, F[2] = {H, H};
    auto in_band = [&](int i, int j) { return i >= 0 && j >= 0 && i <= m && j <= n && j - i >= dlo && j - i < dlo + W; };
    auto at = [&](const std::vector<int> &tab, int i, int j) { return in_band(i, j) ? tab[(size_t)i * S + j] : NONE; };
    auto gap_state = [&](int from_h, int from_gap, int p) {      // open is preferred over extend
        const int op = from_h > NONE ? from_h - c.open[p] - c.ext[p] : NONE, ex = from_gap > NONE ? from_gap - c.ext[p] : NONE;
        return op >= ex ? op : ex;
    };
    auto best_gap = [&](const std::vector<int> *g, int i, int j, int &piece) {   // first piece before the second
        int v = at(g[0], i, j);
        piece = 0;
        if (c.pieces == 2 && at(g[1], i, j) > v) { v = at(g[1], i, j); piece = 1; }
        return v;
    };
    bool have = false;
    int best_rank = 0, best_i = 0, best_j = 0;
    for (int i = 0; i <= m; ++i) {
        int row_max = NONE;
        for (int j = 0; j <= n; ++j) {
            if (!in_band(i, j)) continue;
            const size_t x = (size_t)i * S + j;
            if (i == 0 && j == 0) H[x] = 0;
            else {
                if (at(H, i - 1, j - 1) > NONE) D[x] = at(H, i - 1, j - 1) + pair_score(c, q[i - 1], t[j - 1]);
                for (int p = 0; p < c.pieces; ++p) {
                    if (in_band(i, j - 1)) E[p][x] = gap_state(at(H, i, j - 1), at(E[p], i, j - 1), p);
                    if (in_band(i - 1, j)) F[p][x] = gap_state(at(H, i - 1, j), at(F[p], i - 1, j), p);
                }
                int pe, pf;
                const int e = best_gap(E, i, j, pe), f = best_gap(F, i, j, pf);
                H[x] = D[x] >= e && D[x] >= f ? D[x] : e >= f ? e : f;           // M > E > F
            }
            if (H[x] <= NONE) continue;
            row_max = std::max(row_max, H[x]);
            if (ext) {
                const int r = H[x] + (i == bonus_row ? bonus : 0);
                // score + bonus, then smallest i + j, then smallest i
                if (!have || r > best_rank || (r == best_rank && (i + j < best_i + best_j || (i + j == best_i + best_j && i < best_i)))) {
                    have = true; best_rank = r; best_i = i; best_j = j;
                }
            }
        }
        if (ext && g_drop_log && i > 0 && i % ZDROP_STEP == 0) g_drop_log->push_back(row_max == NONE ? -1 : best_rank - row_max);
        if (ext && zdrop > 0 && i > 0 && i % ZDROP_STEP == 0 && (row_max == NONE || best_rank - row_max > zdrop)) break;
    }
    TaskResult r;
    int i = ext ? best_i : m, j = ext ? best_j : n;
    expect_true("reference: the end cell is inside the band", at(H, i, j) > NONE, i, j);
    r.score = at(H, i, j);
    r.rank = ext ? best_rank : r.score;
    r.rows = i; r.cols = j;
    int state = 0, piece = 0;                    // 0: H, 1: E (consumes target, D), 2: F (consumes query, I)
    std::vector<uint8_t> back;
    while (i > 0 || j > 0) {
        if (state == 0) {
            int pe, pf;
            const int d = at(D, i, j), e = best_gap(E, i, j, pe), f = best_gap(F, i, j, pf);
            if (d >= e && d >= f) { back.push_back(q[i - 1] == t[j - 1] ? OP_EQ : OP_X); --i; --j; }
            else if (e >= f) { state = 1; piece = pe; }
            else { state = 2; piece = pf; }
        } else if (state == 1) {
            back.push_back(OP_D);
            const int op = at(H, i, j - 1) > NONE ? at(H, i, j - 1) - c.open[piece] - c.ext[piece] : NONE;
            const int ex = at(E[piece], i, j - 1) > NONE ? at(E[piece], i, j - 1) - c.ext[piece] : NONE;
            if (op >= ex) state = 0;
            --j;
        } else {
            back.push_back(OP_I);
            const int op = at(H, i - 1, j) > NONE ? at(H, i - 1, j) - c.open[piece] - c.ext[piece] : NONE;
            const int ex = at(F[piece], i - 1, j) > NONE ? at(F[piece], i - 1, j) - c.ext[piece] : NONE;
            if (op >= ex) state = 0;
            --i;
        }
    }
    r.ops.assign(back.rbegin(), back.rend());
    return r;
}

// ------------------------------------------------------------------------------------------
// reference: one piece -> its row (section 5 items 5 and 7), and the class of every task by the band rule
// ------------------------------------------------------------------------------------------
struct ClassCount {
    long long tasks = 0, live = 0;               // all tasks; tasks with rows and columns
    long long narrow = 0, narrow_long = 0, wide = 0, wide_short = 0, long64 = 0, long32 = 0, ungapped = 0;   // if the task goes to a DP
    long long ext_one = 0;                       // extensions the one-piece certificate marks TASK_ONE (see ref_piece)
    void add(const ClassCount &o) {
        tasks += o.tasks; live += o.live; narrow += o.narrow; narrow_long += o.narrow_long; wide += o.wide; wide_short += o.wide_short;
        long64 += o.long64; long32 += o.long32; ungapped += o.ungapped; ext_one += o.ext_one;
    }
};
struct RefRow {
    bool row = false, bare = false;
    int qs = 0, qe = 0, ts = 0, te = 0;          // aligned orientation
    long long nmatch = 0, blen = 0, score = 0;
    std::vector<uint32_t> cigar;                 // len << 4 | code
};
void push_op(std::vector<uint32_t> &cg, uint32_t code, uint32_t len) {
    if (!len) return;
    if (!cg.empty() && (cg.back() & 15u) == code) cg.back() += len << 4; else cg.push_back(len << 4 | code);
}
int ext_rows_of(const hlmi_ava_opts &o) { return std::max(256, o.max_gap); }

// qa: the query in aligned orientation; fps: (q, t) pairs
RefRow ref_piece(const std::vector<uint8_t> &qa, const std::vector<uint8_t> &tc, const std::vector<std::pair<int, int>> &fps,
                 const hlmi_ava_opts &o, ClassCount &cc, bool all_ext_long, bool full_rows = false) {
    const int ql = (int)qa.size(), tl = (int)tc.size(), X = ext_rows_of(o);
    const bool ungapped = o.bandwidth == 0;
    RefRow r;
    r.qs = fps.front().first; r.ts = fps.front().second; r.qe = fps.back().first; r.te = fps.back().second;
    cc.tasks += (long long)fps.size() + 1;
    for (size_t k = 0; k + 1 < fps.size(); ++k) {                     // the blocks
        const int q0 = fps[k].first, t0 = fps[k].second, m = fps[k + 1].first - q0, n = fps[k + 1].second - t0;
        const int shift = n - m, ad = std::abs(shift);
        const bool lng = m > 256 || n > 256;
        int W, dlo;
        bool one = false;
        if (ungapped) { W = 1; dlo = 0; }
        else if (!lng && ad <= 5) { W = 16; dlo = std::min(shift, 0) - 5; }
        else if (!lng) { W = 64; dlo = std::min(shift, 0) - 12; }
        else { W = ad <= 7 ? 32 : 64; dlo = std::min(shift, 0) - (W - 1 - ad) / 2; one = W == 32; }     // centred on the corners' diagonals
        ++cc.live;
        if (ungapped) ++cc.ungapped;
        else if (lng) ++(W == 32 ? cc.long32 : cc.long64);
        else if (W == 16) ++(m > 128 ? cc.narrow_long : cc.narrow);
        else ++(std::min(m, n - dlo) <= 128 ? cc.wide_short : cc.wide);
        const TaskResult b = ref_task(qa.data() + q0, m, tc.data() + t0, n, dlo, W, cost_of(o, one), false, -1, 0, 0);
        r.score += b.score;
        for (uint8_t c : b.ops) push_op(r.cigar, c, 1);
    }
    // stub rule (item 7)
    const int h = o.stub_oh;
    const bool cand = h >= 0 && ((r.qs > X + h && r.ts > X + 64 + h) || (ql - r.qe > X + h && tl - r.te > X + 64 + h));
    const bool stub = cand && r.score >= o.min_dp_score + std::max(o.end_bonus, 0);
    for (int side = 0; side < 2; ++side) {                            // left, then right extension
        const int q_left = side ? ql - r.qe : r.qs, t_left = side ? tl - r.te : r.ts;
        const int m = std::min(q_left, X), n = std::min(t_left, X + 64);
        if (m <= 0 || n <= 0) continue;
        ++cc.live;
        const bool lng = std::min(m, n + 31) > 256;                   // the 64-diagonal band stays inside the target for more than 256 rows
        if (ungapped) ++cc.ungapped;
        else if (lng) ++cc.long32;
        else if (all_ext_long) ++cc.long64;
        else ++(std::min(m, n + 31) <= 128 ? cc.wide_short : cc.wide);
        std::vector<uint8_t> qs(m), ts(n);                            // walking away from the fixed point
        const int q_from = side ? fps.back().first : fps.front().first, t_from = side ? fps.back().second : fps.front().second;
        for (int x = 0; x < m; ++x) qs[x] = side ? qa[q_from + x] : qa[q_from - 1 - x];
        for (int x = 0; x < n; ++x) ts[x] = side ? tc[t_from + x] : tc[t_from - 1 - x];
        if (!ungapped && !lng && o.gap_open2 > 0 && o.gap_ext > o.gap_ext2 && o.end_bonus == 0) {
            // the one-piece certificate of classify_kernel: k substitutions and no ambiguous base on the first min(m, n) pairs of
            // the diagonal, 1 <= k and (match + mismatch) k < cost of the shortest gap the second piece prices lower
            const int g = std::max(1, (o.gap_open2 - o.gap_open + (o.gap_ext - o.gap_ext2) - 1) / (o.gap_ext - o.gap_ext2));
            const int allow = (o.gap_open2 + o.gap_ext2 * g - 1) / (o.match + o.mismatch);
            int k = 0;
            bool amb = false;
            for (int x = 0; x < std::min(m, n); ++x) { amb = amb || qs[x] > 3 || ts[x] > 3; k += qs[x] != ts[x]; }
            if (!amb && k >= 1 && k <= allow) ++cc.ext_one;
        }
        if (stub) continue;
        const int W = ungapped ? 1 : lng ? 32 : 64, dlo = ungapped ? 0 : -(W / 2 - 1);
        const TaskResult e = ref_task(qs.data(), m, ts.data(), n, dlo, W, cost_of(o, lng && !ungapped), true, q_left <= X ? q_left : -1,
                                      o.end_bonus, o.zdrop);
        if (e.rank <= 0 || e.ops.empty()) continue;                   // kept only when it gains; the bonus decides but is not scored
        r.score += e.score;
        if (side) { for (uint8_t c : e.ops) push_op(r.cigar, c, 1); r.qe += e.rows; r.te += e.cols; }
        else {
            std::vector<uint32_t> cg;
            for (size_t x = e.ops.size(); x-- > 0;) push_op(cg, e.ops[x], 1);
            for (uint32_t op : r.cigar) push_op(cg, op & 15u, op >> 4);
            r.cigar.swap(cg);
            r.qs -= e.rows; r.ts -= e.cols;
        }
    }
    r.row = !r.cigar.empty() && r.score >= o.min_dp_score;
    r.bare = cand && !full_rows;
    if (r.bare) r.cigar.clear();
    for (uint32_t op : r.cigar) { r.blen += op >> 4; if ((op & 15u) == OP_EQ) r.nmatch += op >> 4; }
    return r;
}

// ------------------------------------------------------------------------------------------
// cases
// ------------------------------------------------------------------------------------------
struct CasePiece { uint32_t q, t, strand, chain, piece; std::vector<std::pair<int, int>> fp; };
struct Case {
    std::string group, name;
    hlmi_ava_opts o;
    std::vector<std::string> Q, T;               // as in their files (a strand-1 piece counts on its query's reverse complement)
    std::vector<CasePiece> pieces;
    std::vector<std::pair<std::string, std::string>> hooks;
    bool all_dp = false;                         // every live task is built to need a DP: the class counts are asserted
    int defer = 0;                               // 1: with a DeferredPieces; 2: behind an earlier part
    int want_deferred = -1;                      // pieces the driver must set aside (-1: not asserted)
    bool spans = false;                          // HLMI_ALIGN_SPAN_TASKS: align_spans must be reported
    bool full_rows = false;                      // HLMI_STUB_FULL_ROWS: the stub candidates' rows carry their CIGARs
    bool count_one = false;                      // align_tasks_wide_one_piece is asserted, and must lie strictly between 0 and the extensions
};

uint8_t code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
std::vector<uint8_t> codes_of(const std::string &s) { std::vector<uint8_t> v(s.size()); for (size_t i = 0; i < s.size(); ++i) v[i] = code_of(s[i]); return v; }
std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return r;
}
std::string rand_seq(int n) { std::string s(n, 'A'); for (char &c : s) c = "ACGT"[rnd() & 3]; return s; }
char other_base(char c) { const char *b = "ACGT"; for (;;) { const char d = b[rnd() & 3]; if (d != c) return d; } }
void substitute(std::string &s, int pos) { s[pos] = other_base(s[pos]); }

void check_contract(const Case &c) {
    for (const CasePiece &p : c.pieces) {
        const int ql = (int)c.Q[p.q].size(), tl = (int)c.T[p.t].size();
        const int cap = long_rows_cap(c.o);
        expect_true("contract: n_fp >= 2", p.fp.size() >= 2, (long long)p.fp.size());
        for (size_t k = 0; k < p.fp.size(); ++k) {
            expect_true("contract: inside the reads", p.fp[k].first >= 0 && p.fp[k].first <= ql && p.fp[k].second >= 0 && p.fp[k].second <= tl, p.fp[k].first, p.fp[k].second);
            if (!k) continue;
            const int m = p.fp[k].first - p.fp[k - 1].first, n = p.fp[k].second - p.fp[k - 1].second;
            expect_true("contract: strictly increasing", m > 0 && n > 0, m, n);
            expect_true("contract: shift", std::abs(n - m) <= (c.o.bandwidth == 0 ? 0 : SHIFT_MAX), m, n);
            expect_true("contract: block length", m <= cap && n <= cap, m, n);
            if (k + 1 < p.fp.size()) expect_true("contract: BLOCK_MIN", m >= BLOCK_MIN && n >= BLOCK_MIN, m, n);
        }
    }
}

// A piece under construction: query (aligned orientation) and target grow block by block.
struct Build {
    std::string q, t;
    std::vector<std::pair<int, int>> fp;
    void left_flank(int lq, int lt, const std::vector<int> &subs_from_fp = {}, int amb_from_fp = -1) {
        const std::string f = rand_seq(std::max(lq, lt));
        q = f.substr(f.size() - lq); t = f.substr(f.size() - lt);
        for (int d : subs_from_fp) if (d < lq && d < lt) substitute(q, lq - 1 - d);
        if (amb_from_fp >= 0 && amb_from_fp < lq) q[lq - 1 - amb_from_fp] = 'N';
        fp.push_back({lq, lt});
    }
    // a block of m rows and n columns: one indel of |n - m| bases at `indel_at` (row), substitutions at the given rows
    void block(int m, int n, const std::vector<int> &subs = {}, int indel_at = -1, int amb_at = -1) {
        std::string bq = rand_seq(m), bt = bq;
        if (indel_at < 0) indel_at = m / 2;
        indel_at = std::min(indel_at, std::min(m, n) - 1);
        if (n > m) bt.insert(indel_at, rand_seq(n - m));
        else if (n < m) bt.erase(indel_at, m - n);
        for (int s : subs) if (s >= 0 && s < m) substitute(bq, s);
        if (amb_at >= 0 && amb_at < m) bq[amb_at] = 'N';
        q += bq; t += bt;
        fp.push_back({(int)q.size(), (int)t.size()});
    }
    // block from explicit strings
    void block_str(const std::string &bq, const std::string &bt) { q += bq; t += bt; fp.push_back({(int)q.size(), (int)t.size()}); }
    void right_flank(int rq, int rt, const std::vector<int> &subs_from_fp = {}, int amb_from_fp = -1) {
        const std::string f = rand_seq(std::max(rq, rt));
        std::string fq = f.substr(0, rq), ft = f.substr(0, rt);
        for (int d : subs_from_fp) if (d < rq && d < rt) substitute(fq, d);
        if (amb_from_fp >= 0 && amb_from_fp < rq) fq[amb_from_fp] = 'N';
        q += fq; t += ft;
    }
};
// rows with `k` substitutions spread so that no certificate of the classifier can settle the block: >= 4, two on either side
// of the indel, the last one in the last row of the query (no suffix to trim); m: the block's rows
std::vector<int> dp_subs(int m) { return {1, m / 4, m / 2 + 3, (3 * m) / 4, m - 1}; }

void add_piece(Case &c, const Build &b, int strand, uint32_t chain = 0, uint32_t piece = 0) {
    c.Q.push_back(strand ? revcomp(b.q) : b.q);
    c.T.push_back(b.t);
    c.pieces.push_back(CasePiece{(uint32_t)c.Q.size() - 1, (uint32_t)c.T.size() - 1, (uint32_t)strand, chain, piece, b.fp});
}

hlmi_ava_opts variant(int v) {
    hlmi_ava_opts o = v == 1 ? ava_opts_short() : ava_opts_long();
    if (v == 2) o.gap_open2 = 0;
    if (v == 3) { o.match = 1; o.mismatch = 1; o.gap_open = 1; o.gap_ext = 1; o.gap_open2 = 0; }
    if (v == 4) { o.mismatch = 16; o.gap_open = 20; o.gap_ext = 2; o.gap_open2 = 0; }
    return o;
}
const char *VARIANT_NAME[5] = {"long", "short", "one_piece", "all_ones", "wide_scores"};
const std::vector<std::pair<std::string, std::string>> NO_CERTS = {{"HLMI_NO_SHIFT_CERT", "1"}, {"HLMI_NO_GAP1_CERT", "1"}, {"HLMI_NO_GAP2_CERT", "1"},
    {"HLMI_NO_SUFFIX_TRIM", "1"}, {"HLMI_NO_ONE_PIECE_CERT", "1"}, {"HLMI_NO_EXT_CERT", "1"}};

std::string fmt(const char *f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

std::string cigar_text(const struct RefRow &r);
// the reference's row of a piece under construction (case construction asserts on it)
RefRow build_row(const Build &b, const hlmi_ava_opts &o, bool full_rows = false) {
    ClassCount cc;
    return ref_piece(codes_of(b.q), codes_of(b.t), b.fp, o, cc, false, full_rows);
}

std::vector<Case> build_cases() {
    std::vector<Case> out;
    g_rng = 0x9e3779b97f4a7c15ull;
    auto new_case = [&](const char *group, const std::string &name, const hlmi_ava_opts &o) {
        Case c; c.group = group; c.name = name; c.o = o; out.push_back(c); return out.size() - 1;
    };
    // ---- task_geometry: build_task ------------------------------------------------------------------------
    for (int gap : {200, 1000}) {
        hlmi_ava_opts o = ava_opts_long();
        o.max_gap = gap; o.min_dp_score = 40;
        const int X = std::max(256, gap);
        for (int strand = 0; strand < 2; ++strand) {
            const size_t ci = new_case("task_geometry", fmt("query_left gap=%d strand=%d", gap, strand), o);
            int pad = 0;
            for (int left : {0, 1, X - 1, X, X + 1}) {
                for (int side = 0; side < 2; ++side) {
                    Build b;
                    const std::vector<int> subs = {3, 9, 20, 40};              // the extension needs its DP
                    if (side == 0) b.left_flank(left, left + 40, subs); else b.left_flank(0, 0);
                    b.block(40, 40, {5, 17});
                    b.block(33, 34, {7});
                    if (side == 1) b.right_flank(left, left + 40, subs);
                    add_piece(out[ci], b, strand);
                }
                // a short read between the pieces' reads: the reads' offsets take every residue modulo 4
                ++pad;
                out[ci].Q.push_back(rand_seq(pad % 4 + 1)); out[ci].T.push_back(rand_seq((pad + 1) % 4 + 1));
            }
            const size_t cj = new_case("task_geometry", fmt("target_left gap=%d strand=%d", gap, strand), o);
            const int m = 70;
            for (int tleft : {0, 1, m + 63, m + 64, m + 65}) {
                for (int side = 0; side < 2; ++side) {
                    Build b;
                    if (side == 0) b.left_flank(m, tleft, {4, 11, 30, 50}); else b.left_flank(0, 0);
                    b.block(48, 48, {9});
                    b.block(36, 33, {2, 30});
                    if (side == 1) b.right_flank(m, tleft, {4, 11, 30, 50});
                    add_piece(out[cj], b, strand);
                }
            }
        }
    }
    // ---- band_rule: the class of every block and extension, asserted from the statistics -----------------------
    for (int strand = 0; strand < 2; ++strand) {
        hlmi_ava_opts o = ava_opts_long();
        o.min_dp_score = 20; o.max_gap = 1000;
        for (int m : {255, 256, 257})
            for (int shift : {0, 5, -5, 6, -6, 7, -7, 8, -8, 39, -39}) {
                for (int n0 : {255, 256, 257}) {
                    // rows m; columns m + shift, and columns n0 with rows n0 - shift: both sides of 256 in rows and in columns
                    const size_t ci = new_case("band_rule", fmt("block m=%d n0=%d shift=%d strand=%d", m, n0, shift, strand), o);
                    out[ci].all_dp = true;
                    Build b; b.left_flank(0, 0); b.block(m, m + shift, dp_subs(m)); add_piece(out[ci], b, strand);
                    Build b2; b2.left_flank(0, 0); b2.block(n0 - shift, n0, dp_subs(n0 - shift)); add_piece(out[ci], b2, strand);
                }
            }
        for (int m : {63, 64, 65, 128, 129}) {                           // NR_SMALL, NR_SHORT
            const size_t ci = new_case("band_rule", fmt("narrow m=%d strand=%d", m, strand), o);
            out[ci].all_dp = true;
            for (int shift : {0, 3, -5}) { Build b; b.left_flank(0, 0); b.block(m, m + shift, dp_subs(m)); add_piece(out[ci], b, strand); }
        }
        for (int r : {128, 129, 256, 257}) {                             // WIDE_SHORT, EXT_MAX: min(m, n - dlo) of wide blocks and extensions
            const size_t ci = new_case("band_rule", fmt("wide rows=%d strand=%d", r, strand), o);
            out[ci].all_dp = true;
            if (r <= 256) {
                { Build b; b.left_flank(0, 0); b.block(r, r + 9, dp_subs(r)); add_piece(out[ci], b, strand); }        // min(m, n + 12) = m
                { Build b; b.left_flank(0, 0); b.block(r + 20, r + 20 - 32, dp_subs(r + 20)); add_piece(out[ci], b, strand); }   // dlo = -44: n + 44 = r + 32 > m
            }
            { Build b; b.left_flank(r, r + 100, {2, 8, 19, 33, 60}); b.block(40, 40, dp_subs(40)); add_piece(out[ci], b, strand); }     // rows = m
            { Build b; b.left_flank(0, 0); b.block(40, 40, dp_subs(40)); b.right_flank(r + 50, r - 31, {2, 8, 19, 33, 60}); add_piece(out[ci], b, strand); }   // rows = n + 31
        }
        // a path that needs the band's first / last diagonal: the whole shift as ONE indel, and NARROW_PAD / BAND_PAD more as a pair
        for (int m : {120, 300})
            for (int shift : {5, -5, 6, -6, 7, -7, 8, -8, 39, -39}) {
                const size_t ci = new_case("band_rule", fmt("pad m=%d shift=%d strand=%d", m, shift, strand), o);
                const int ad = std::abs(shift), lng = m > 256;
                const int W = !lng && ad <= 5 ? 16 : lng && ad <= 7 ? 32 : 64, pad = !lng ? (ad <= 5 ? 5 : 12) : (W - 1 - ad) / 2;
                for (int extra : {pad, pad + 1})
                    for (int dir = 0; dir < 2; ++dir) {
                        // q: A x B C ;  t: A B y C with an extra indel pair around B next to the block's own indel
                        const std::string A = rand_seq(30), B = rand_seq(m - 90), C = rand_seq(60), x = rand_seq(extra), y = rand_seq(extra);
                        std::string bq = dir ? A + x + B + C : A + B + y + C, bt = dir ? A + B + y + C : A + x + B + C;
                        if (shift > 0) bt.insert(dir ? 30 + (int)B.size() : 30, rand_seq(shift)); else bq.insert(dir ? 30 : 30 + (int)B.size(), rand_seq(-shift));
                        Build b; b.left_flank(0, 0); b.block_str(bq, bt); add_piece(out[ci], b, strand);
                    }
            }
    }
    // ---- certificates: granted and refused, one step apart; the rows are the same with the certificates off and from bytes ----
    for (int v : {0, 1, 4})
        for (int form = 0; form < 3; ++form)
            for (int strand = 0; strand < 2; ++strand) {
                g_rng = 0x1234567ull + 977 * v + strand;                 // the three forms see the same sequences
                hlmi_ava_opts o = variant(v);
                o.min_dp_score = 20;
                const size_t ci = new_case("certificates", fmt("%s form=%d strand=%d", VARIANT_NAME[v], form, strand), o);
                if (form == 1) out[ci].hooks = NO_CERTS;
                if (form == 2) out[ci].hooks = {{"HLMI_CLASSIFY_BYTES", "1"}};
                const int m = 70;
                for (int k = 0; k <= 5; ++k)
                    for (int at : {0, 31, 32, 33, m - 1}) {
                        std::vector<int> subs;
                        for (int x = 0; x < k; ++x) subs.push_back((at + 13 * x) % m);
                        Build b; b.left_flank(0, 0); b.block(m, m, subs); add_piece(out[ci], b, strand);
                    }
                for (int rep = 0; rep < 8; ++rep) {                      // fourth certificate: a one-base shift that matches, or not
                    const std::string unit = rep & 1 ? "AC" : "A";
                    std::string bq = rand_seq(20);
                    for (int x = 0; x < 12; ++x) bq += unit;
                    bq += rand_seq(24);
                    std::string bt = bq;
                    for (int x = 0; x < 1 + rep / 2; ++x) substitute(bq, 21 + 5 * x);
                    Build b; b.left_flank(0, 0); b.block_str(bq, bt); add_piece(out[ci], b, strand);
                }
                for (int d : {1, -1})                                    // |n - m| = 1 with 0, 1, 2, 3 substitutions; repeats: the shifted self-match
                    for (int k = 0; k <= 3; ++k)
                        for (int rep = 0; rep < 2; ++rep) {
                            std::string bq = rep ? rand_seq(10) + std::string(30, 'G') + rand_seq(10) + "TCTCTCTCTCTCTCTCTCTC" + rand_seq(8) : rand_seq(78);
                            std::string bt = bq;
                            if (d > 0) bt.insert(40, rand_seq(1)); else bt.erase(40, 1);
                            for (int x = 0; x < k; ++x) substitute(bq, 12 + 25 * x);
                            Build b; b.left_flank(0, 0); b.block_str(bq, bt); add_piece(out[ci], b, strand);
                        }
                for (int k = 0; k <= 3; ++k)                             // extensions with k substitutions, with and without the bonus row
                    for (int reach = 0; reach < 2; ++reach) {
                        std::vector<int> subs;
                        for (int x = 0; x < k; ++x) subs.push_back(10 + 17 * x);
                        Build b; b.left_flank(60, reach ? 90 : 40, subs); b.block(50, 50); b.right_flank(reach ? 60 : 300, 70, subs); add_piece(out[ci], b, strand);
                    }
                for (int amb : {20, 49, 50}) {                           // an ambiguous base inside the block, in its last row, a base behind it
                    Build b; b.left_flank(0, 0); b.block(50, 50, {}, -1, amb < 50 ? amb : -1); b.block(40, 40, {3}); b.right_flank(30, 30, {}, amb == 50 ? 0 : -1);
                    add_piece(out[ci], b, strand);
                }
                for (int keep : {0, 1, m - 1}) {                         // suffix trim: matching bases behind the last substitution
                    Build b; b.left_flank(0, 0); b.block(m, m + 2, {1, 20, 30, m - 1 - keep}, 10); add_piece(out[ci], b, strand);
                }
            }
    // ---- gap_cost ------------------------------------------------------------------------------------
    for (int v : {0, 1, 2})
        for (int strand = 0; strand < 2; ++strand) {
            hlmi_ava_opts o = variant(v);
            o.min_dp_score = 20;
            const size_t ci = new_case("gap_cost", fmt("%s strand=%d", VARIANT_NAME[v], strand), o);
            for (int g : {14, 15, 16, 19, 20, 21, 22, 30})
                for (int d : {1, -1})
                    for (int shift : {0, 4, 12}) {
                        // one gap of g bases and one of g - shift the other way, 60 rows apart: the block's shift is `shift`
                        const std::string A = rand_seq(45), B = rand_seq(60), C = rand_seq(45), x = rand_seq(g), y = rand_seq(std::max(g - shift, 0));
                        const std::string lng = A + x + B + C, sht = A + B + y + C;
                        Build b; b.left_flank(0, 0); b.block_str(d > 0 ? sht : lng, d > 0 ? lng : sht);
                        if (std::abs(b.fp.back().second - b.fp.back().first) <= SHIFT_MAX) add_piece(out[ci], b, strand);
                    }
            for (int g : {3, 19, 20, 21, 25}) {                          // the same gaps inside an end extension (TASK_ONE or not)
                for (int d : {1, -1}) {
                    const std::string A = rand_seq(50), B = rand_seq(80), x = rand_seq(g);
                    Build b; b.left_flank(0, 0); b.block(45, 45, {7});
                    b.q += d > 0 ? A + B : A + x + B; b.t += d > 0 ? A + x + B : A + B;
                    add_piece(out[ci], b, strand);
                }
            }
            // ties built by hand: a repeat where the gap can sit in either sequence (E / F), or be a substitution run (M / gap)
            for (int u = 1; u <= 4; ++u) {
                const std::string A = rand_seq(40), C = rand_seq(40), R = std::string("ACGT").substr(0, u);
                std::string rq, rt;
                for (int x = 0; x < 6; ++x) rq += R;
                for (int x = 0; x < 7; ++x) rt += R;
                Build b; b.left_flank(0, 0); b.block_str(A + rq + C, A + rt + C); b.block_str(A + rt + C, A + rq + C);
                b.block_str(A + "G" + C.substr(0, 20) + "T" + C, A + "T" + C.substr(0, 20) + "GA" + C);
                add_piece(out[ci], b, strand);
            }
        }
    for (int strand = 0; strand < 2; ++strand) {
        // TASK_ONE extensions against ones that are not: 1 .. 7 substitutions on the diagonal (6 k < 44, the cost of the 20-base gap
        // from which the second piece is the cheaper one) against 8 and more, and against an ambiguous base
        hlmi_ava_opts o = ava_opts_long();
        o.min_dp_score = 20;
        const size_t ci = new_case("gap_cost", fmt("task_one strand=%d", strand), o);
        out[ci].count_one = true;
        for (int k : {2, 6, 7, 8, 9, 14}) {
            std::vector<int> subs;
            for (int x = 0; x < k; ++x) subs.push_back(9 + 13 * x);
            Build b; b.left_flank(200, 200, subs); b.block(45, 45, {7}); b.right_flank(200, 230, subs, k == 6 ? 150 : -1); add_piece(out[ci], b, strand);
        }
    }
    for (int strand = 0; strand < 2; ++strand) {
        // the best-cell rule's last clause: cells (1, 2) = 1D1= and (2, 1) = 1I1= tie in score and in i + j; the smaller i wins
        g_case = "best cell";
        hlmi_ava_opts m3 = variant(3);
        m3.match = 3; m3.min_dp_score = 10;
        const size_t ci = new_case("gap_cost", fmt("best_cell strand=%d", strand), m3);
        Build b; b.left_flank(0, 0); b.block(50, 50, {4});
        b.q += "AC" + std::string(20, 'T'); b.t += "CA" + std::string(20, 'G');
        const RefRow r = build_row(b, m3);
        expect_true("best cell: the reference takes (1, 2)", r.qe == 51 && r.te == 52, r.qe, r.te);
        add_piece(out[ci], b, strand);
    }
    for (int strand = 0; strand < 2; ++strand) {
        // a tie for each pair of M, E and F, from the hand-worked literals of --host, inside blocks of 70 rows whose other bases
        // match; one substitution far from the tie and the certificates off, so that the DP kernels decide them
        g_case = "ties";
        hlmi_ava_opts ones = variant(3), ef = variant(3);
        ef.mismatch = 5;
        ones.min_dp_score = ef.min_dp_score = 10;
        const std::string P = "ACGTTGCAAGGCTTAACCGGTTAAACGTTGCAT", S = "TGCATCGGATTACAGGCATCGATCGGCTAAGCTAG";
        struct Tie { const char *name; hlmi_ava_opts o; std::string q, t; const char *want; };
        const std::vector<Tie> ties = {
            {"E=F", ef, P + "A" + S, P + "C" + S, "1I1D"},            // X costs 5, a deleted and an inserted base 4: E is taken first walking back
            {"M=F", ones, P + "GG" + S, P + "G" + S, "1I"},            // the match is taken first walking back: the gap sits at the leftmost place
            {"M=E", ones, P + "G" + S, P + "GG" + S, "1D"},
        };
        for (int form = 0; form < 2; ++form)
            for (const Tie &t : ties) {
                const size_t ci = new_case("gap_cost", fmt("tie %s form=%d strand=%d", t.name, form, strand), t.o);
                out[ci].hooks = NO_CERTS;
                if (form) { out[ci].hooks.push_back({"HLMI_NARROW_UNPACKED", "1"}); }
                Build b; b.left_flank(0, 0);
                std::string q = t.q, tt = t.t;
                q[3] = tt[3] == 'A' ? 'C' : 'A';                        // the far substitution
                b.block_str(q, tt);
                const RefRow r = build_row(b, t.o);
                const std::string cg = cigar_text(r);
                const std::string want = std::string("3=") + (t.o.mismatch == 5 ? "1I1D" : "1X") + std::to_string((int)P.size() - 4) + "=" + t.want;      // (under these costs the far substitution is such a tie itself)
                if (cg.compare(0, want.size(), want) != 0) printf("tie %s: reference %s, wanted to begin with %s\n", t.name, cg.c_str(), want.c_str());
                expect_true("ties: the reference resolves the tie as the hand-worked literal", cg.compare(0, want.size(), want) == 0, (long long)cg.size());
                add_piece(out[ci], b, strand);
            }
    }
    // ---- run_buffers: tracebacks of a chosen number of runs ------------------------------------------------
    for (int form = 0; form < 3; ++form)
        for (int strand = 0; strand < 2; ++strand) {
            g_rng = 0x777ull + strand;
            hlmi_ava_opts o = ava_opts_long();
            o.min_dp_score = -100000; o.max_gap = 1000;
            const size_t ci = new_case("run_buffers", fmt("form=%d strand=%d", form, strand), o);
            if (form == 1) out[ci].hooks = {{"HLMI_RUN_BUF_CAP", "3"}};
            if (form == 2) out[ci].hooks = {{"HLMI_NARROW_UNPACKED", "1"}, {"HLMI_NARROW_LONG_UNPACKED", "1"}};
            // k isolated substitutions two rows apart give 2 k + 1 runs (2 k when the first sits in row 0); an indel in the matching
            // tail adds two.  The reference's CIGAR of the block must have exactly the intended number of runs.
            auto runs_block = [&](int runs, int m, int shift) {
                std::vector<int> subs;
                int left = runs - (shift ? 2 : 0);
                if (left % 2 == 0) { subs.push_back(0); left -= 1; }
                for (int x = 0; x < (left - 1) / 2; ++x) subs.push_back(2 + 2 * x);
                Build b;
                RefRow r;
                for (int attempt = 0; attempt < 20; ++attempt) {         // (random bases: a substitution next to a chance match can become a gap pair)
                    // t = ACGT ACGT ..., q = t with base + 2 in the substituted rows: no shift of 1 .. 3 diagonals matches anything, so
                    // the diagonal is the path; the indel sits in a tail of 24 random bases behind the last substitution
                    std::string bt(m, 'A');
                    for (int x = 0; x < m; ++x) bt[x] = "ACGT"[x & 3];
                    if (shift) bt.replace(m - 24, 24, rand_seq(24));
                    std::string bq = bt;
                    for (int x : subs) bq[x] = "ACGT"[((x & 3) + 2) & 3];
                    expect_true("run_buffers: the substitutions end before the tail", shift == 0 || subs.empty() || subs.back() < m - 25, m, shift);
                    if (shift > 0) bt.insert(m - 12, rand_seq(shift)); else if (shift < 0) bt.erase(m - 12 + shift / 2, -shift);
                    b = Build(); b.left_flank(0, 0); b.block_str(bq, bt);
                    r = build_row(b, o);
                    if ((int)r.cigar.size() == runs) break;
                }
                if ((int)r.cigar.size() != runs) printf("run_buffers m=%d shift=%d: %s\n", m, shift, cigar_text(r).c_str());
                expect_true("run_buffers: the block's traceback has the intended runs", (int)r.cigar.size() == runs, runs, (long long)r.cigar.size());
                add_piece(out[ci], b, strand);
            };
            g_case = "run_buffers";
            for (int r : {47, 48, 49}) { runs_block(r, 120, 0); runs_block(r, 128, 3); runs_block(r, 200, -4); }        // RUN_BUF_NARROW
            for (int r : {127, 128, 129}) { runs_block(r, 250, 9); runs_block(r, 200, -20); runs_block(r, 180, 39); }   // RUN_BUF_WIDE
            for (int r : {255, 256}) runs_block(r, 256, 0);                                                             // RUN_CHUNK_SMALL: a narrow task has at most 256 runs
            for (int r : {255, 256, 257}) { runs_block(r, 300, 0); runs_block(r, 520, 20); }                            // ... 257 in a LONG one
            {
                // a LONG task near its run buffer of 2 long_rows_cap + 64 = 2336 entries.  An optimal path never alternates 1I 1D row
                // after row (grouping the gaps costs no more, and the traceback's priorities group them), so the densest one has
                // three runs for two rows: q = (AG)^n against t = (AC)^n under costs where a substitution is dearer than two gap
                // bases - 1= 1D 1I per unit, 1704 runs in the 1136 rows a block may have under max_gap 1000
                hlmi_ava_opts d = o;
                d.match = 1; d.mismatch = 30; d.gap_open = 0; d.gap_ext = 1; d.gap_open2 = 0; d.ambi = 1;
                const size_t cd = new_case("run_buffers", fmt("dense form=%d strand=%d", form, strand), d);
                out[cd].hooks = out[ci].hooks;
                std::string bq, bt;
                for (int x = 0; x < 568; ++x) { bq += "AG"; bt += "AC"; }
                Build b; b.left_flank(0, 0); b.block_str(bq, bt);
                const RefRow r = build_row(b, d);
                expect_true("run_buffers: the dense LONG task has three runs for two rows", r.cigar.size() == 1704, 1704, (long long)r.cigar.size());
                add_piece(out[cd], b, strand);
            }
        }
    // ---- long_tasks ----------------------------------------------------------------------------------
    for (int v : {0, 2})
        for (int strand = 0; strand < 2; ++strand) {
            hlmi_ava_opts o = variant(v);
            o.min_dp_score = 20; o.max_gap = 1000;
            for (int n_half = 1; n_half <= 3; ++n_half) {
                const size_t ci = new_case("long_tasks", fmt("%s long32 x%d strand=%d", VARIANT_NAME[v], n_half, strand), o);
                out[ci].all_dp = true;
                for (int x = 0; x < n_half; ++x) { Build b; b.left_flank(0, 0); b.block(300 + x, 303 + x, dp_subs(300)); add_piece(out[ci], b, strand); }
            }
            const size_t ci = new_case("long_tasks", fmt("%s tiles strand=%d", VARIANT_NAME[v], strand), o);
            for (int m : {256, 257, 512, 513})
                for (int shift : {0, 7, 8, -20}) {
                    { Build b; b.left_flank(0, 0); b.block(m, m + shift, {3, 100, 254, 255, 256, 257, m - 2}, 128); add_piece(out[ci], b, strand); }
                    { Build b; b.left_flank(0, 0); b.block(m, m + shift, {255}, 255); b.block(m, m + shift, {256}, 256); add_piece(out[ci], b, strand); }
                }
            for (int m : {256, 257, 512, 513}) {                        // LONG extensions, an edit on both sides of a tile edge
                Build b; b.left_flank(m, m + 80, {100, 255, 256, 300}); b.block(40, 40, {5}); b.right_flank(m, m + 80, {30, 254, 257, 511, 512}); add_piece(out[ci], b, strand);
            }
        }
    for (int zd : {60, 400})                                           // z-drop: the drop begins at a chosen row; zdrop and zdrop + 1
        for (int strand = 0; strand < 2; ++strand) {
            hlmi_ava_opts o = ava_opts_long();
            o.min_dp_score = 20; o.max_gap = 1000; o.zdrop = zd;
            const size_t ci = new_case("long_tasks", fmt("zdrop=%d strand=%d", zd, strand), o);
            for (int start : {31, 32, 33, 63, 64, 65})
                for (int junk : {8, 9, 10, 11, 12, 13, 20, 40}) {
                    // matching bases up to `start`, then `junk` bases of unrelated sequence in both reads, then matching again
                    const std::string A = rand_seq(start), B = rand_seq(400);
                    Build b; b.left_flank(0, 0); b.block(50, 50, {4});
                    b.q += A + rand_seq(junk) + B; b.t += A + rand_seq(junk) + B;
                    add_piece(out[ci], b, strand);
                }
        }
    for (int strand = 0; strand < 2; ++strand) {
        // a drop of exactly zdrop and of zdrop + 1 at row 64: 32 matching rows, 36 rows of unrelated sequence, a long matching tail.
        // The reference, run without a z-drop, says how far row 64's best cell lies below the best so far: D.  Under zdrop = D
        // the extension goes on and takes the tail; under zdrop = D - 1 it ends at row 64.
        g_case = "zdrop exact";
        hlmi_ava_opts o = ava_opts_long();
        o.min_dp_score = 20; o.max_gap = 1000; o.zdrop = 0;
        const std::string A = rand_seq(32), B = rand_seq(180), jq = rand_seq(36), jt = rand_seq(36);      // 248 rows: the 64-diagonal LONG kernel
        Build b; b.left_flank(0, 0); b.block(50, 50, {4});
        b.q += A + jq + B; b.t += A + jt + B;
        std::vector<int> drops;
        g_drop_log = &drops;
        const RefRow free_row = build_row(b, o);
        g_drop_log = nullptr;
        expect_true("zdrop: the check rows were logged", drops.size() >= 3 && drops[1] > 20, (long long)drops.size());
        const int D = drops[1];
        for (int zd : {D, D - 1}) {
            o.zdrop = zd;
            AlignScoreHooks hk;
            expect_true("zdrop: this option set sends every extension to the LONG kernel", align_score_setup(o, hk).ext_all_long);
            const RefRow r = build_row(b, o);
            expect_true("zdrop: a drop of zdrop goes on, a drop of zdrop + 1 ends the extension", zd == D ? r.qe == free_row.qe && r.qe > 50 + 64 : r.qe <= 50 + 64, r.qe, free_row.qe);
            const size_t ci = new_case("long_tasks", fmt("drop=%d zdrop=%d strand=%d", D, zd, strand), o);
            add_piece(out[ci], b, strand);
            Build l; l.left_flank(0, 0); l.block(50, 50, {4}); l.q += A + jq + B + B; l.t += A + jt + B + B;       // the same in a LONG32 extension
            add_piece(out[ci], l, strand);
        }
    }
    // ---- ungapped: bandwidth 0 ---------------------------------------------------------------------------
    for (int strand = 0; strand < 2; ++strand) {
        hlmi_ava_opts o = ava_opts_long();
        o.bandwidth = 0; o.min_dp_score = 20; o.max_gap = 1000; o.zdrop = 60;
        const size_t ci = new_case("ungapped", fmt("strand=%d", strand), o);
        for (int m : {1, 33, 64, 257, 400})
            for (int k : {0, 1, 4, 9}) {
                std::vector<int> subs, fl;
                for (int x = 0; x < k; ++x) { subs.push_back((7 + 29 * x) % m); fl.push_back(3 + 11 * x); }
                Build b; b.left_flank(70 + k, 90, fl); b.block(40, 40, {1}); b.block(m, m, subs); b.right_flank(300, 280 + m % 3, fl); add_piece(out[ci], b, strand);
            }
        for (int at : {5, 6, 7}) {                                       // ties go to the shorter prefix: +2 -4 +2 comes back to the same score
            Build b; b.left_flank(0, 0); b.block(40, 40, {1}); b.right_flank(at + 1, at + 1, {at - 1}); add_piece(out[ci], b, strand);
            Build b2; b2.left_flank(0, 0); b2.block(40, 40, {1}); b2.right_flank(at + 2, at + 2, {at - 2}); add_piece(out[ci], b2, strand);
        }
        for (int junk : {10, 20, 40}) {                                  // z-drop on the diagonal
            const std::string A = rand_seq(40), B = rand_seq(300);
            Build b; b.left_flank(0, 0); b.block(50, 50, {4}); b.q += A + rand_seq(junk) + B; b.t += A + rand_seq(junk) + B; add_piece(out[ci], b, strand);
        }
    }
    // ---- assembly ----------------------------------------------------------------------------------------
    for (int form = 0; form < 3; ++form)
        for (int strand = 0; strand < 2; ++strand) {
            g_rng = 0x5151ull + strand;
            hlmi_ava_opts o = ava_opts_long();
            o.min_dp_score = 80; o.max_gap = 400;
            std::vector<std::pair<std::string, std::string>> hooks;
            if (form == 1) hooks = {{"HLMI_ASM_STAGE_CAP", "0"}};
            if (form == 2) hooks = {{"HLMI_ASM_WAVE", "1"}};
            {   // pieces of 63 / 64 / 65 / 129 tasks; neighbouring tasks whose runs merge (=, X, I, D), also across a step boundary
                const size_t ci = new_case("assembly", fmt("tasks form=%d strand=%d", form, strand), o);
                out[ci].hooks = hooks;
                for (int tasks : {63, 64, 65, 129})
                    for (int style = 0; style < 4; ++style) {
                        Build b; b.left_flank(style & 1 ? 20 : 0, 30, style == 3 ? std::vector<int>{0} : std::vector<int>{});
                        for (int k = 0; k < tasks - 2; ++k) {
                            const int m = 33 + (int)(rnd() % 6);
                            if (style == 0) b.block(m, m);                                       // = next to =
                            else if (style == 1) b.block(m, m, {0, m - 1});                     // X next to X
                            else if (style == 2) { const std::string s = rand_seq(m); b.block_str(s + (k & 1 ? "" : "ACG"), s + (k & 1 ? "ACG" : "")); }   // I / D at the ends
                            else b.block(m, m + (k % 3 == 0 ? 2 : 0), k % 5 == 0 ? std::vector<int>{3, 9, 14, 20} : k % 5 == 1 ? std::vector<int>{m - 1} : std::vector<int>{});
                        }
                        b.right_flank(style & 2 ? 25 : 0, 40, style == 3 ? std::vector<int>{0} : std::vector<int>{});
                        add_piece(out[ci], b, strand);
                    }
            }
            for (int slots : {1023, 1024, 1025}) {                       // one step of 64 tasks that writes this many slots
                const size_t ci = new_case("assembly", fmt("slots=%d form=%d strand=%d", slots, form, strand), o);
                out[ci].hooks = hooks;
                // 61 blocks of 17 runs (8 isolated substitutions in ACGT ACGT ..., = at both ends: neighbours merge) and no extensions;
                // the last block brings the rest: its substitutions are counted up until the reference's CIGAR has `slots` ops
                auto periodic = [](int m, int k, bool x_last) {
                    std::string t(m, 'A');
                    for (int x = 0; x < m; ++x) t[x] = "ACGT"[x & 3];
                    std::string q = t;
                    for (int x = 0; x < k; ++x) q[2 + 2 * x] = "ACGT"[((2 + 2 * x) & 3) + 2 & 3];
                    if (x_last) q[m - 1] = "ACGT"[((m - 1) & 3) + 2 & 3];
                    return std::make_pair(q, t);
                };
                Build b;
                g_case = "slots";
                bool found = false;
                for (int kk = 0; kk < 76 && !found; ++kk) {
                    b = Build(); b.left_flank(0, 0);
                    for (int k = 0; k < 61; ++k) { const auto s = periodic(40, 8, false); b.block_str(s.first, s.second); }
                    const auto s = periodic(80, kk / 2, kk & 1);
                    b.block_str(s.first, s.second);
                    found = (int)build_row(b, o).cigar.size() == slots;
                }
                expect_true("assembly: the step writes the intended slots", found, slots);
                add_piece(out[ci], b, strand);
            }
            {   // both sides of NT <= 17 P: pieces of 16 and 17 fixed points
                for (int nfp : {16, 17}) {
                    const size_t ci = new_case("assembly", fmt("n_fp=%d form=%d strand=%d", nfp, form, strand), o);
                    out[ci].hooks = hooks;
                    for (int rep = 0; rep < 3; ++rep) { Build b; b.left_flank(10, 10); for (int k = 1; k < nfp; ++k) b.block(35, 35 + (k == 3), {k}); b.right_flank(10, 10); add_piece(out[ci], b, strand); }
                }
            }
            {   // tasks of 1, 2, 4, 5 runs; extensions that score 0, 1 (all_ones), or are kept by the bonus alone; min_dp_score - 1 / min_dp_score
                hlmi_ava_opts s = ava_opts_short();
                s.min_dp_score = 60;
                const size_t ci = new_case("assembly", fmt("keep_drop form=%d strand=%d", form, strand), s);
                out[ci].hooks = hooks;
                for (int len : {14, 15, 16, 17}) { Build b; b.left_flank(0, 0); b.block(len, len); add_piece(out[ci], b, strand); }   // 4 per base: 56 .. 68
                { Build b; b.left_flank(0, 0); b.block(40, 40); b.right_flank(3, 9, {0, 1}); add_piece(out[ci], b, strand); }       // 2 X + 1 =: -4 + 4 = 0 ... with the bonus
                { Build b; b.left_flank(0, 0); b.block(40, 40); b.right_flank(300, 9, {0, 1}); add_piece(out[ci], b, strand); }     // the same without it
                { Build b; b.left_flank(2, 9, {1}); b.block(40, 40); add_piece(out[ci], b, strand); }
                hlmi_ava_opts a1 = variant(3);
                a1.min_dp_score = 30;
                const size_t cj = new_case("assembly", fmt("all_ones form=%d strand=%d", form, strand), a1);
                out[cj].hooks = hooks;
                for (int len : {29, 30, 31}) { Build b; b.left_flank(0, 0); b.block(len, len); add_piece(out[cj], b, strand); }
                { Build b; b.left_flank(0, 0); b.block(40, 40); b.right_flank(2, 5, {0}); add_piece(out[cj], b, strand); }          // X =: 0
                { Build b; b.left_flank(0, 0); b.block(40, 40); b.right_flank(3, 5, {0}); add_piece(out[cj], b, strand); }          // X = =: 1
                for (int runs : {1, 2, 4, 5}) { Build b; b.left_flank(0, 0); for (int k = 0; k < 6; ++k) { std::vector<int> s; for (int x = 0; x + 1 < runs; x += 2) s.push_back(runs % 2 ? 4 + 3 * x : 3 * x); b.block(36, 36, s); } add_piece(out[cj], b, strand); }
            }
        }
    // ---- driver --------------------------------------------------------------------------------------------
    for (int strand = 0; strand < 2; ++strand) {
        hlmi_ava_opts o = ava_opts_long();
        o.min_dp_score = 40; o.max_gap = 1000;
        auto short_piece = [&](Case &c) { Build b; b.left_flank(12, 12); b.block(40, 40, {9}); b.block(35, 36, {1}); b.right_flank(20, 20, {5}); add_piece(c, b, strand); };
        auto long_piece = [&](Case &c) { Build b; b.left_flank(12, 12); b.block(40, 40, {9}); b.block(300, 301, {1, 150}); b.right_flank(20, 20); add_piece(c, b, strand); };
        for (int total : {9, 10, 11}) {
            const size_t ci = new_case("driver", fmt("1 LONG among %d strand=%d", total, strand), o);
            out[ci].defer = 1 + (total == 11); out[ci].want_deferred = total >= 10 ? 1 : 0;
            for (int k = 0; k < total; ++k) if (k == 4) long_piece(out[ci]); else short_piece(out[ci]);
        }
        {
            const size_t ci = new_case("driver", fmt("all LONG strand=%d", strand), o);
            out[ci].defer = 1; out[ci].want_deferred = 0;
            for (int k = 0; k < 3; ++k) long_piece(out[ci]);
        }
        {   // a LONG extension sets a piece aside as well
            const size_t ci = new_case("driver", fmt("LONG extension strand=%d", strand), o);
            out[ci].defer = 2; out[ci].want_deferred = 1;
            for (int k = 0; k < 12; ++k) if (k == 11) { Build b; b.left_flank(400, 500, {7}); b.block(40, 40, {9}); add_piece(out[ci], b, strand); } else short_piece(out[ci]);
        }
        for (int nfp : {16, 17}) {                                       // n_fp <= 16 P: the lane and the wave form of the flag kernels
            const size_t ci = new_case("driver", fmt("flag n_fp=%d strand=%d", nfp, strand), o);
            out[ci].defer = 1; out[ci].want_deferred = 1;
            for (int k = 0; k < 10; ++k) { Build b; b.left_flank(5, 5); for (int x = 1; x < nfp; ++x) b.block(x == nfp - 1 && k == 9 ? 260 : 34, x == nfp - 1 && k == 9 ? 262 : 34, {x}); add_piece(out[ci], b, strand); }
        }
        {
            const size_t ci = new_case("driver", fmt("spans strand=%d", strand), o);
            out[ci].hooks = {{"HLMI_ALIGN_SPAN_TASKS", "64"}}; out[ci].spans = true;
            for (int k = 0; k < 60; ++k) { if (k % 7 == 3) { Build b; b.left_flank(3, 3); b.block(10, 10); add_piece(out[ci], b, strand); } else short_piece(out[ci]); }
        }
        for (int v : {0, 1, 10, 11}) {                                   // stub rule, h = 3; 10, 11: once more with the candidates' full rows
            const bool full = v >= 10;
            v %= 10;
            hlmi_ava_opts s = variant(v);
            s.stub_oh = 3; s.max_gap = 200;
            const int X = 256, h = 3;
            const size_t ci = new_case("driver", fmt("stub %s full_rows=%d strand=%d", VARIANT_NAME[v], (int)full, strand), s);
            if (full) { out[ci].hooks = {{"HLMI_STUB_FULL_ROWS", "1"}}; out[ci].full_rows = true; }
            for (int dq : {0, 1})
                for (int dt : {0, 1})
                    for (int blocks : {1, 3})
                        for (int side = 0; side < 2; ++side) {
                            // blocks = 1: 20 bases - below min_dp_score + end_bonus under either preset: the late round
                            Build b;
                            const int fq = X + h + dq, ft = X + 64 + h + dt;
                            if (side == 0) b.left_flank(fq, ft, {30}); else b.left_flank(7, 7);
                            for (int k = 0; k < blocks; ++k) b.block(blocks == 1 ? 20 : 60, blocks == 1 ? 20 : 60, {9});
                            if (side == 1) b.right_flank(fq, ft, {30}); else b.right_flank(7, 7);
                            add_piece(out[ci], b, strand);
                        }
        }
    }
    for (Case &c : out) {
        g_group = c.group.c_str(); g_case = c.name;
        check_contract(c);
    }
    return out;
}

// ------------------------------------------------------------------------------------------
// the case file
// ------------------------------------------------------------------------------------------
void opts_write(std::ostream &f, const hlmi_ava_opts &o) {
    f << "opts " << o.k << ' ' << o.w << ' ' << o.hpc << ' ' << o.min_chain_score << ' ' << o.max_gap << ' ' << o.bandwidth << ' ' << o.min_cnt << ' '
      << o.min_mid_occ << ' ' << o.match << ' ' << o.mismatch << ' ' << o.gap_open << ' ' << o.gap_ext << ' ' << o.ambi << ' ' << o.min_dp_score << ' '
      << o.end_bonus << ' ' << o.pair_once << ' ' << o.gap_open2 << ' ' << o.gap_ext2 << ' ' << o.stub_oh << ' ' << o.zdrop << '\n';
}
bool opts_read(std::istream &f, hlmi_ava_opts &o) {
    std::string w;
    o = ava_opts_long();
    return (bool)(f >> w >> o.k >> o.w >> o.hpc >> o.min_chain_score >> o.max_gap >> o.bandwidth >> o.min_cnt >> o.min_mid_occ >> o.match >> o.mismatch >>
                  o.gap_open >> o.gap_ext >> o.ambi >> o.min_dp_score >> o.end_bonus >> o.pair_once >> o.gap_open2 >> o.gap_ext2 >> o.stub_oh >> o.zdrop) && w == "opts";
}
void write_cases(const std::vector<Case> &cases, const char *path) {
    std::ofstream f(path);
    for (const Case &c : cases) {
        std::string name = c.group + ":" + c.name;
        for (char &ch : name) if (ch == ' ') ch = '_';
        f << "case " << name << '\n';
        opts_write(f, c.o);
        f << "reads " << c.Q.size() << ' ' << c.T.size() << '\n';
        for (const std::string &s : c.Q) f << s << '\n';
        for (const std::string &s : c.T) f << s << '\n';
        f << "pieces " << c.pieces.size() << '\n';
        for (const CasePiece &p : c.pieces) {
            f << p.q << ' ' << p.t << ' ' << p.strand << ' ' << p.chain << ' ' << p.piece << ' ' << p.fp.size();
            for (auto &x : p.fp) f << ' ' << x.first << ' ' << x.second;
            f << '\n';
        }
    }
}
std::vector<Case> read_cases(const char *path) {
    std::ifstream f(path);
    std::vector<Case> out;
    std::string w;
    while (f >> w) {
        Case c;
        if (w != "case" || !(f >> c.name) || !opts_read(f, c.o)) { printf("bad case file at case %zu\n", out.size()); exit(2); }
        size_t nq, nt, np;
        f >> w >> nq >> nt;
        c.Q.resize(nq); c.T.resize(nt);
        for (auto &s : c.Q) f >> s;
        for (auto &s : c.T) f >> s;
        f >> w >> np;
        c.pieces.resize(np);
        for (CasePiece &p : c.pieces) {
            size_t nf;
            f >> p.q >> p.t >> p.strand >> p.chain >> p.piece >> nf;
            p.fp.resize(nf);
            for (auto &x : p.fp) f >> x.first >> x.second;
        }
        if (!f) { printf("bad case file at case %zu\n", out.size()); exit(2); }
        out.push_back(std::move(c));
    }
    return out;
}

struct CaseRef { std::vector<RefRow> rows; std::vector<ClassCount> cc; };      // per piece
CaseRef ref_case(const Case &c, bool all_ext_long) {
    CaseRef r;
    for (const CasePiece &p : c.pieces) {
        const std::vector<uint8_t> qa = codes_of(p.strand ? revcomp(c.Q[p.q]) : c.Q[p.q]), tc = codes_of(c.T[p.t]);
        ClassCount one;
        r.rows.push_back(ref_piece(qa, tc, p.fp, c.o, one, all_ext_long, c.full_rows));
        r.cc.push_back(one);
    }
    return r;
}
std::string cigar_text(const RefRow &r) {
    if (r.bare) return "*";
    std::string s;
    for (uint32_t op : r.cigar) { s += std::to_string(op >> 4); s += (op & 15u) == OP_EQ ? '=' : (op & 15u) == OP_X ? 'X' : (op & 15u) == OP_I ? 'I' : 'D'; }
    return s;
}
int dump(const char *path) {
    const std::vector<Case> cases = read_cases(path);
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case &c = cases[i];
        printf("case %zu %s\n", i, c.name.c_str());
        const CaseRef r = ref_case(c, false);
        for (size_t k = 0; k < c.pieces.size(); ++k) {
            const RefRow &w = r.rows[k];
            if (!w.row) { printf("-\n"); continue; }
            const int ql = (int)c.Q[c.pieces[k].q].size();
            printf("%d %d %d %d %lld %lld %s\n", c.pieces[k].strand ? ql - w.qe : w.qs, c.pieces[k].strand ? ql - w.qs : w.qe, w.ts, w.te, w.nmatch, w.blen,
                   cigar_text(w).c_str());
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// --host: the reference against literals and against the enumeration of all alignments
// ------------------------------------------------------------------------------------------
// best score over ALL global alignments of q[i..] and t[j..] under the two-piece cost (gap runs may not touch a run of the same kind)
int enum_best(const std::vector<uint8_t> &q, const std::vector<uint8_t> &t, size_t i, size_t j, int last, const Cost &c) {
    if (i == q.size() && j == t.size()) return 0;
    int best = NONE;
    auto gap = [&](int L) { int v = c.open[0] + c.ext[0] * L; if (c.pieces == 2) v = std::min(v, c.open[1] + c.ext[1] * L); return v; };
    if (i < q.size() && j < t.size()) best = std::max(best, pair_score(c, q[i], t[j]) + enum_best(q, t, i + 1, j + 1, 0, c));
    if (last != 1) for (size_t L = 1; j + L <= t.size(); ++L) best = std::max(best, -gap((int)L) + enum_best(q, t, i, j + L, 1, c));
    if (last != 2) for (size_t L = 1; i + L <= q.size(); ++L) best = std::max(best, -gap((int)L) + enum_best(q, t, i + L, j, 2, c));
    return best;
}
size_t g_host_cases = 0;
bool g_host_ok = true;
#define HOST_EXPECT(cond)                                                                                  \
    do { ++g_host_cases; if (!(cond)) { printf("HOST FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); g_host_ok = false; } } while (0)
std::string ops_text(const TaskResult &r) {
    RefRow w;
    for (uint8_t c : r.ops) push_op(w.cigar, c, 1);
    return cigar_text(w);
}
TaskResult host_block(const std::string &q, const std::string &t, const hlmi_ava_opts &o, int dlo, int W, bool one = false) {
    const std::vector<uint8_t> a = codes_of(q), b = codes_of(t);
    return ref_task(a.data(), (int)a.size(), b.data(), (int)b.size(), dlo, W, cost_of(o, one), false, -1, 0, 0);
}
TaskResult host_ext(const std::string &q, const std::string &t, const hlmi_ava_opts &o, int bonus_row, int dlo = -31, int W = 64) {
    const std::vector<uint8_t> a = codes_of(q), b = codes_of(t);
    return ref_task(a.data(), (int)a.size(), b.data(), (int)b.size(), dlo, W, cost_of(o, false), true, bonus_row, o.end_bonus, o.zdrop);
}
int host_checks() {
    const hlmi_ava_opts L = ava_opts_long(), S = ava_opts_short();
    hlmi_ava_opts ones = variant(3);
    {   // ---- hand-worked blocks (A 2, B 4, O 4,24, E 2,1) ----
        TaskResult r = host_block("ACGTACGT", "ACGTACGT", L, -5, 16);
        HOST_EXPECT(r.score == 16 && ops_text(r) == "8=");
        r = host_block("ACGTACGT", "ACGAACGT", L, -5, 16);
        HOST_EXPECT(r.score == 10 && ops_text(r) == "3=1X4=");
        r = host_block("ACGTTACGT", "ACGTACGT", L, -6, 16);              // one inserted T of a run of two: the traceback leaves the end diagonal as late as it can
        HOST_EXPECT(r.score == 16 - 6 && ops_text(r) == "3=1I5=");
        r = host_block("ACGTACGT", "ACGTTACGT", L, -5, 16);
        HOST_EXPECT(r.score == 16 - 6 && ops_text(r) == "3=1D5=");
        r = host_block("ACNTACGT", "ACGTACGT", L, -5, 16);               // an ambiguous base: -1, written X
        HOST_EXPECT(r.score == 14 - 1 && ops_text(r) == "2=1X5=");
        // M > E > F: under all-ones costs q = AC, t = CA ties 2X (-2) against 1D1=1I (1 - 2 - 2 = -3): M alone; q = A, t = C: X (-1)
        r = host_block("A", "C", ones, -5, 16);
        HOST_EXPECT(r.score == -1 && ops_text(r) == "1X");
        // M against a gap pair: q = AG, t = GA with match 1, mismatch 1, open 1, ext 1: 2X = -2; 1D 1= 1I = 1 - 2 - 2 = -3
        r = host_block("AG", "GA", ones, -5, 16);
        HOST_EXPECT(r.score == -2 && ops_text(r) == "2X");
        // E against F: q = AAC.., the cell is entered by a deletion or an insertion of the same cost: built with costs where
        // X = -5 and a gap base = -2: q = A, t = C becomes 1D1I or 1I1D at -4; E is preferred at the LAST cell (walking back), so the
        // deletion is the last column: 1I1D
        hlmi_ava_opts ef = ones; ef.mismatch = 5;
        r = host_block("A", "C", ef, -5, 16);
        HOST_EXPECT(r.score == -4 && ops_text(r) == "1I1D");
        // M ties E: q = AA, t = A, match 1, open 1, ext 1: (2, 1) is reached by M from (1, 0) [-2 + 1 = -1] and by F from (1, 1) [1 - 2 = -1];
        // M wins: the walk takes the match last: 1I1=
        r = host_block("AA", "A", ones, -6, 16);
        HOST_EXPECT(r.score == -1 && ops_text(r) == "1I1=");
        r = host_block("A", "AA", ones, -5, 16);
        HOST_EXPECT(r.score == -1 && ops_text(r) == "1D1=");
        // open before extend, first piece before second: a gap of 20 costs 44 under either piece (4 + 40 = 24 + 20): the first
        {
            const std::string a = "ACGTTGCAAGGCTTAACCGGTTAA", g = "CCCCCCCCCCCCCCCCCCCC";
            r = host_block(a + a, a + g + a, L, -12, 64);
            HOST_EXPECT(r.score == 96 - 44 && ops_text(r) == "24=20D24=");
            r = host_block(a + a, a + g + "C" + a, L, -12, 64);          // 21 bases: the second piece, 45 against 46
            HOST_EXPECT(r.score == 96 - 45);
            r = host_block(a + a, a + g + "C" + a, L, -12, 64, true);    // the one-piece cost
            HOST_EXPECT(r.score == 96 - 46);
        }
        // the band mask: a path that needs diagonal dlo - 1 is not found
        r = host_block("ACGTACGTAC" "GG", "GG" "ACGTACGTAC", ones, -1, 3);
        HOST_EXPECT(r.score < 10 - 2 * 3);
        r = host_block("ACGTACGTAC" "GG", "GG" "ACGTACGTAC", ones, -2, 5);
        HOST_EXPECT(r.score == 10 - 3 - 3 && ops_text(r) == "2D10=2I");
    }
    {   // ---- extensions ----
        TaskResult r = host_ext("ACGTAC", "ACGTAC", L, 6);
        HOST_EXPECT(r.score == 12 && r.rows == 6 && r.cols == 6 && ops_text(r) == "6=");
        r = host_ext("ACGTACTT", "ACGTACGG", L, 8);                      // stops before the mismatches
        HOST_EXPECT(r.score == 12 && r.rows == 6 && r.cols == 6);
        r = host_ext("ACTAC", "ACGAC", L, -1);                           // 2= (4) against 2=1X2= (4): the tie goes to the smaller i + j
        HOST_EXPECT(r.score == 4 && r.rows == 2 && r.cols == 2);
        r = host_ext("TTTT", "GGGG", L, -1);                             // nothing gained: the cell (0, 0)
        HOST_EXPECT(r.score == 0 && r.rank == 0 && r.ops.empty());
        // smallest i on equal i + j: q = AC, t = CA under all-ones: cells (1, 2) = 1D1= (1 - 2 = -1) ... the best is (0, 0); with
        // match 3: (1, 2) = 3 - 2 = 1 and (2, 1) = 1: i + j equal, the smaller i = 1 wins
        hlmi_ava_opts m3 = ones; m3.match = 3;
        r = host_ext("AC", "CA", m3, -1);
        HOST_EXPECT(r.score == 1 && r.rows == 1 && r.cols == 2 && ops_text(r) == "1D1=");
        // the bonus ranks but is not scored (short preset: A 4, B 2, bonus 100)
        r = host_ext("ACGTTT", "ACGAAA", S, 6);
        HOST_EXPECT(r.score == 12 - 6 && r.rank == 106 && r.rows == 6 && r.cols == 6);
        r = host_ext("ACGTTT", "ACGAAA", S, -1);
        HOST_EXPECT(r.score == 12 && r.rows == 3);
        // z-drop after row 32: 32 matching rows, then unrelated sequence for 32 rows, then a long match the drop never sees
        {
            hlmi_ava_opts z = L; z.zdrop = 40;
            const std::string a = "ACGTTGCAAGGCTTAACCGGTTAAACGTTGCA", junk_q(32, 'A'), junk_t(32, 'C');
            std::string tail;
            for (int x = 0; x < 6; ++x) tail += a;
            r = host_ext(a + junk_q + tail, a + junk_t + tail, z, -1);
            HOST_EXPECT(r.score == 64 && r.rows == 32);                  // row 64: best of the row far below 64 - 40
            z.zdrop = 400;
            r = host_ext(a + junk_q + tail, a + junk_t + tail, z, -1);
            HOST_EXPECT(r.score == 64 - 2 * 56 + 2 * 192 && r.rows == 256);      // 32 D and 32 I (24 + 32 each) are cheaper than 32 X
        }
        // bandwidth 0: the best prefix of the diagonal, the shorter one on a tie
        r = host_ext("ACGTAAC", "ACGTCCC", L, -1, 0, 1);
        HOST_EXPECT(r.score == 8 && r.rows == 4);
        r = host_ext("ACTAC", "ACGAC", L, -1, 0, 1);
        HOST_EXPECT(r.score == 4 && r.rows == 2);
    }
    const size_t n_task = g_host_cases;
    {   // ---- every task up to 6 x 6 whose band covers the table: the score is the best over ALL alignments ----
        g_rng = 42;
        size_t n = 0;
        for (int rep = 0; rep < 400; ++rep) {
            const int m = 1 + (int)(rnd() % 6), nn = 1 + (int)(rnd() % 6);
            std::string q(m, 'A'), t(nn, 'A');
            for (char &c : q) c = "ACGN"[rnd() % (rep % 5 == 0 ? 4 : 2)];
            for (char &c : t) c = "ACGN"[rnd() % (rep % 5 == 0 ? 4 : 2)];
            for (const hlmi_ava_opts &o : {L, S, ones, variant(4)}) {
                hlmi_ava_opts oo = o;
                if (rep & 1) { oo.gap_open2 = oo.gap_open + 3; oo.gap_ext2 = 0; }       // a second piece that takes over at small lengths
                const TaskResult r = host_block(q, t, oo, -8, 16);
                const int want = enum_best(codes_of(q), codes_of(t), 0, 0, 0, cost_of(oo, false));
                if (r.score != want) { printf("HOST FAIL enumeration q=%s t=%s got %d want %d\n", q.c_str(), t.c_str(), r.score, want); g_host_ok = false; }
                // the path scores what the table says
                int sc = 0, i = 0, j = 0;
                const Cost c = cost_of(oo, false);
                for (size_t x = 0; x < r.ops.size();) {
                    size_t y = x;
                    while (y < r.ops.size() && r.ops[y] == r.ops[x]) ++y;
                    const int len = (int)(y - x);
                    if (r.ops[x] == OP_EQ || r.ops[x] == OP_X) { for (int k = 0; k < len; ++k) sc += pair_score(c, code_of(q[i + k]), code_of(t[j + k])); i += len; j += len; }
                    else { int g = c.open[0] + c.ext[0] * len; if (c.pieces == 2) g = std::min(g, c.open[1] + c.ext[1] * len); sc -= g; (r.ops[x] == OP_I ? i : j) += len; }
                    x = y;
                }
                // (an I run next to a D run is two gaps: fine; an ambiguous pair is written X or =)
                if (sc != r.score || i != m || j != nn) { printf("HOST FAIL path q=%s t=%s path %d table %d\n", q.c_str(), t.c_str(), sc, r.score); g_host_ok = false; }
                ++n;
            }
        }
        g_host_cases += n;
    }
    const size_t n_enum = g_host_cases - n_task;
    {   // ---- pieces: merged neighbours, a dropped extension in between, min_dp_score ----
        hlmi_ava_opts o = L; o.min_dp_score = 20;
        const std::string a = "ACGTTGCAAGGCTTAACCGGTTAAACGTTGCA";            // 32
        ClassCount cc;
        RefRow r = ref_piece(codes_of(a + a), codes_of(a + a), {{0, 0}, {32, 32}, {64, 64}}, o, cc, false);
        HOST_EXPECT(r.row && cigar_text(r) == "64=" && r.score == 128 && cc.tasks == 4 && cc.live == 2 && cc.narrow == 2);
        r = ref_piece(codes_of("TT" + a + "GG"), codes_of("TT" + a + "CC"), {{2, 2}, {34, 34}}, o, cc, false);
        HOST_EXPECT(r.row && cigar_text(r) == "34=" && r.qs == 0 && r.qe == 34);
        o.min_dp_score = 69;
        r = ref_piece(codes_of("TT" + a + "GG"), codes_of("TT" + a + "CC"), {{2, 2}, {34, 34}}, o, cc, false);
        HOST_EXPECT(!r.row);
        o.min_dp_score = 68;
        r = ref_piece(codes_of("TT" + a + "GG"), codes_of("TT" + a + "CC"), {{2, 2}, {34, 34}}, o, cc, false);
        HOST_EXPECT(r.row);
    }
    printf("host ref_task cases=%zu %s\n", n_task, g_host_ok ? "ok" : "FAILED");
    printf("host ref_enumeration cases=%zu %s\n", n_enum, g_host_ok ? "ok" : "FAILED");
    printf("host ref_piece cases=%zu %s\n", g_host_cases - n_task - n_enum, g_host_ok ? "ok" : "FAILED");
    return g_host_ok ? 0 : 1;
}

// ------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------
struct HookScope {                                // sets existing test hooks of the library for the scope
    std::vector<std::string> names;
    explicit HookScope(const std::vector<std::pair<std::string, std::string>> &h) {
        for (auto &kv : h) { setenv(kv.first.c_str(), kv.second.c_str(), 1); names.push_back(kv.first); }
        if (!names.empty()) hooks_refresh();
    }
    ~HookScope() { for (auto &n : names) unsetenv(n.c_str()); if (!names.empty()) hooks_refresh(); }
};
std::map<std::string, double> stats_json() {       // hlmi_last_stats_json, parsed: "key": value pairs of one flat object
    std::vector<char> buf(1 << 20);
    if (hlmi_last_stats_json(buf.data(), (int64_t)buf.size()) != HLMI_OK) { printf("hlmi_last_stats_json: %s\n", hlmi_last_error()); exit(2); }
    std::map<std::string, double> m;
    const char *p = buf.data();
    while ((p = strchr(p, '"'))) {
        const char *e = strchr(p + 1, '"');
        if (!e) break;
        const std::string key(p + 1, e);
        const char *colon = strchr(e, ':');
        if (!colon) break;
        m[key] = strtod(colon + 1, nullptr);
        p = colon + 1;
    }
    return m;
}
double stat_of(const std::map<std::string, double> &m, const char *k) { auto it = m.find(k); return it == m.end() ? 0.0 : it->second; }

bool g_seen_ext_all_long[2] = {false, false};
struct DevRows { std::vector<PafRec> recs; std::vector<uint32_t> ops; std::vector<uint64_t> hi, lo; size_t n_ops = 0; };

void run_case(const Case &c) {
    g_case = c.name;
    ++g_cases;
    HookScope hs(c.hooks);
    SeqSet Q, T;
    auto fill = [](SeqSet &s, const std::vector<std::string> &reads, const char *prefix) {
        s.off.push_back(0);
        for (size_t i = 0; i < reads.size(); ++i) { s.names.push_back(prefix + std::to_string(i)); s.bases += reads[i]; s.off.push_back(s.bases.size()); s.first_line.push_back(0); }
    };
    fill(Q, c.Q, "q"); fill(T, c.T, "t");
    DevReads dQ, dT;
    upload_reads(Q, 0, Q.size(), dQ);
    upload_reads(T, 0, T.size(), dT);
    std::vector<uint32_t> qlen, tlen, rank_q, rank_t, chunk;
    for (size_t i = 0; i < c.Q.size(); ++i) { qlen.push_back((uint32_t)c.Q[i].size()); rank_q.push_back((uint32_t)(3 * i + 1)); }
    for (size_t i = 0; i < c.T.size(); ++i) { tlen.push_back((uint32_t)c.T[i].size()); rank_t.push_back((uint32_t)(3 * i + 2)); chunk.push_back((uint32_t)(i % 3)); }
    DBuf<uint32_t> d_qlen, d_tlen, d_rq, d_rt, d_chunk;
    d_qlen.upload(qlen); d_tlen.upload(tlen); d_rq.upload(rank_q); d_rt.upload(rank_t); d_chunk.upload(chunk);
    AvaInput in;
    in.T = &dT; in.Q = &dQ; in.d_rank_t = d_rt.p; in.d_rank_q = d_rq.p; in.n_ranks = 3 * std::max(c.Q.size(), c.T.size()) + 3;
    in.d_chunk_of_t = d_chunk.p; in.n_chunks = 3;
    // the fabricated ChainOut; the fixed points of a piece need not follow those of the piece before: a gap of a few unused entries
    std::vector<Piece> pieces;
    std::vector<FixPt> fps;
    for (size_t i = 0; i < c.pieces.size(); ++i) {
        const CasePiece &p = c.pieces[i];
        pieces.push_back(Piece{p.q, p.t, p.strand, p.chain + (uint32_t)i, p.piece + (uint32_t)(i % 3), (uint32_t)fps.size(), (uint32_t)p.fp.size(), 0});
        for (auto &x : p.fp) fps.push_back(FixPt{(uint32_t)x.first, (uint32_t)x.second});
    }
    ChainOut ch;
    ch.n_pieces = pieces.size(); ch.n_fp = fps.size();
    ch.pieces.upload(pieces); ch.fps.upload(fps);
    sync();

    AlignScoreHooks hk;                              // (what align_span derives: ext_all_long for the reference's class counts)
    const AlignScoreSetup sc = align_score_setup(c.o, hk);
    CaseRef ref = ref_case(c, sc.ext_all_long);

    DeferredPieces defer;
    if (c.defer == 2) {                              // an earlier batch left a part: fp_base of the new one counts behind it
        DeferredPieces::Part part;
        part.n_pieces = 1; part.n_fp = 5; part.fp_base = 0;
        defer.n_pieces = 1; defer.n_fp = 5;
        defer.parts.push_back(std::move(part));
    }
    const size_t parts_before = defer.parts.size(), fp_before = defer.n_fp;
    std::vector<AlignOut> outs;
    stat_reset();
    align_pieces(in, c.o, d_qlen.p, d_tlen.p, ch, outs, c.defer ? &defer : nullptr);
    sync();
    ktimer_flush();
    const std::map<std::string, double> st = stats_json();

    // ---- the set-aside part ----
    std::vector<char> set_aside(c.pieces.size(), 0);
    if (c.defer) {
        std::vector<size_t> lng;                     // pieces with a LONG block or a LONG extension (band rule)
        for (size_t i = 0; i < c.pieces.size(); ++i) {
            if (ref.cc[i].long32 + (sc.ext_all_long ? 0 : ref.cc[i].long64)) lng.push_back(i);      // (blocks alone are LONG with 64 diagonals: no driver case has ext_all_long)
        }
        const bool aside = c.o.bandwidth != 0 && !lng.empty() && lng.size() * 10 <= c.pieces.size();
        if (c.want_deferred >= 0) expect_one("case built for this many set-aside pieces", c.want_deferred, aside ? (long long)lng.size() : 0);
        expect_one("align_pieces_deferred", aside ? (long long)lng.size() : 0, (long long)stat_of(st, "align_pieces_deferred"));
        expect_one("deferred parts", (long long)parts_before + (aside ? 1 : 0), (long long)defer.parts.size());
        if (aside) {
            const DeferredPieces::Part &part = defer.parts.back();
            size_t nfp = 0;
            for (size_t i : lng) nfp += c.pieces[i].fp.size();
            expect_one("part n_pieces", (long long)lng.size(), (long long)part.n_pieces);
            expect_one("part n_fp", (long long)nfp, (long long)part.n_fp);
            expect_one("part fp_base", (long long)fp_before, (long long)part.fp_base);
            expect_one("defer n_fp", (long long)(fp_before + nfp), (long long)defer.n_fp);
            const std::vector<Piece> pp = part.pieces.download(part.n_pieces);
            const std::vector<FixPt> pf = part.fps.download(part.n_fp);
            size_t off = 0;
            for (size_t k = 0; k < lng.size(); ++k) {
                const Piece &w = pieces[lng[k]];
                expect_one("part piece q", w.q, pp[k].q, k); expect_one("part piece t", w.t, pp[k].t, k); expect_one("part piece strand", w.strand, pp[k].strand, k);
                expect_one("part piece chain", w.chain, pp[k].chain, k); expect_one("part piece piece", w.piece, pp[k].piece, k);
                expect_one("part piece n_fp", w.n_fp, pp[k].n_fp, k);
                expect_one("part piece fp_off", (long long)(fp_before + off), pp[k].fp_off, k);
                for (uint32_t x = 0; x < w.n_fp; ++x) {
                    expect_one("part fixed point q", fps[w.fp_off + x].q, pf[off + x].q, off + x);
                    expect_one("part fixed point t", fps[w.fp_off + x].t, pf[off + x].t, off + x);
                }
                off += w.n_fp;
                set_aside[lng[k]] = 1;
            }
        }
    }
    // ---- rows ----
    DevRows got;
    for (const AlignOut &ao : outs) {
        expect_true("a span with rows", ao.n_rows > 0);
        const std::vector<PafRec> r = ao.recs.download(ao.n_rows);
        const std::vector<uint32_t> ops = ao.n_ops ? ao.ops.download(ao.n_ops) : std::vector<uint32_t>();
        const std::vector<uint64_t> hi = ao.ord_hi.download(ao.n_rows), lo = ao.ord_lo.download(ao.n_rows);
        uint64_t next = 0;
        for (size_t i = 0; i < r.size(); ++i) {
            expect_one("cig_off follows the row before", (long long)next, (long long)r[i].cig_off, got.recs.size() + i);
            next += r[i].cig_n;
            PafRec w = r[i];
            w.cig_off += got.ops.size();
            got.recs.push_back(w);
        }
        expect_one("n_ops of the span", (long long)next, (long long)ao.n_ops);
        got.ops.insert(got.ops.end(), ops.begin(), ops.end());
        got.hi.insert(got.hi.end(), hi.begin(), hi.end()); got.lo.insert(got.lo.end(), lo.begin(), lo.end());
    }
    size_t row = 0;
    ClassCount cc;
    size_t n_fp_kept = 0, n_kept_pieces = 0;
    for (size_t i = 0; i < c.pieces.size(); ++i) {
        if (set_aside[i]) continue;
        ++n_kept_pieces; n_fp_kept += c.pieces[i].fp.size();
        const RefRow &w = ref.rows[i];
        if (!w.row) { ++g_dropped; continue; }
        ++g_kept;
        if (row >= got.recs.size()) mismatch("n_rows (a row is missing for piece)", i, (long long)row + 1, (long long)got.recs.size());
        const PafRec &r = got.recs[row];
        const Piece &p = pieces[i];
        const uint32_t ql = qlen[p.q];
        // a row in the wrong place shows as a wrong order key first
        expect_one("ord_hi", (long long)((uint64_t)chunk[p.t] << 32 | p.q), (long long)got.hi[row], i);
        expect_one("ord_lo", (long long)((uint64_t)p.t << 43 | (uint64_t)p.strand << 42 | (uint64_t)(p.chain & 0x3fffffu) << 20 | (p.piece & 0xfffffu)), (long long)got.lo[row], i);
        expect_one("qid", rank_q[p.q], r.qid, i); expect_one("tid", rank_t[p.t], r.tid, i);
        expect_one("qlen", ql, r.qlen, i); expect_one("tlen", tlen[p.t], r.tlen, i);
        expect_one("qs", p.strand ? ql - w.qe : w.qs, r.qs, i); expect_one("qe", p.strand ? ql - w.qs : w.qe, r.qe, i);
        expect_one("ts", w.ts, r.ts, i); expect_one("te", w.te, r.te, i);
        expect_one("nmatch", w.nmatch, r.nmatch, i); expect_one("blen", w.blen, r.blen, i);
        expect_one("flags", p.strand ? PF_REV : 0, r.flags, i); expect_one("chunk", chunk[p.t], r.chunk, i);
        expect_one("tie", 0, r.tie, i);
        expect_one("cig_n", (long long)w.cigar.size(), r.cig_n, i);
        for (size_t x = 0; x < w.cigar.size(); ++x) expect_one("CIGAR op", w.cigar[x], got.ops[r.cig_off + x], i * 100000 + x);
        ++row;
    }
    expect_one("n_rows", (long long)row, (long long)got.recs.size());
    // ---- counts ----
    for (size_t i = 0; i < c.pieces.size(); ++i) if (!set_aside[i]) cc.add(ref.cc[i]);      // the class counts of the kept pieces
    if (c.spans) expect_one("align_tasks over all spans", cc.tasks, (long long)stat_of(st, "align_tasks"));
    if (n_kept_pieces && !c.spans) {
        expect_one("align_tasks", cc.tasks, (long long)stat_of(st, "align_tasks"));
        const long long fast = (long long)stat_of(st, "align_tasks_fast"), dp = (long long)stat_of(st, "align_tasks_dp");
        const long long narrow = (long long)stat_of(st, "align_tasks_narrow"), wide = (long long)stat_of(st, "align_tasks_wide"), lng = (long long)stat_of(st, "align_tasks_long");
        if (c.o.stub_oh < 0) {
            expect_one("align_tasks_fast + align_tasks_dp = tasks with rows and columns", cc.live, fast + dp);
            expect_one("align_tasks_narrow + _wide + _long = align_tasks_dp", dp, narrow + wide + lng);
        }
        const long long l64 = (long long)stat_of(st, "kernel_launches.align_long"), l32 = (long long)stat_of(st, "kernel_launches.align_long32");
        if (c.all_dp) {                              // built for a class: every live task needs its DP, in the class the band rule gives it
            expect_one("a case built for the DP has no certified task", 0, fast);
            expect_one("align_tasks_dp", cc.live, dp);
            expect_one("align_tasks_narrow", cc.narrow + cc.narrow_long, narrow);
            expect_one("align_tasks_wide", cc.wide + cc.wide_short, wide);
            expect_one("align_tasks_long", cc.long32 + cc.long64 + cc.ungapped, lng);
            expect_one("align_n.align_narrow_long", cc.narrow_long, (long long)stat_of(st, "align_n.align_narrow_long"));
            expect_one("align_n.align_wide", cc.wide, (long long)stat_of(st, "align_n.align_wide"));
            expect_one("align_n.align_wide_short", cc.wide_short, (long long)stat_of(st, "align_n.align_wide_short"));
            expect_one("align_n.align_long", cc.long64, (long long)stat_of(st, "align_n.align_long"));
            expect_one("align_n.align_long32", cc.long32, (long long)stat_of(st, "align_n.align_long32"));
            expect_true("kernel_launches.align_long", (l64 > 0) == (cc.long64 > 0), l64, cc.long64);
            expect_true("kernel_launches.align_long32", (l32 > 0) == (cc.long32 > 0), l32, cc.long32);
            if (c.group == "long_tasks") g_seen_ext_all_long[sc.ext_all_long ? 1 : 0] = true;
        } else if (c.o.bandwidth != 0) {
            if (c.group == "long_tasks") g_seen_ext_all_long[sc.ext_all_long ? 1 : 0] = true;
            // LONG blocks take no certificate: they are in the launches whatever the extensions did
            expect_true("kernel_launches.align_long", l64 > 0 || cc.long64 == 0 || c.o.stub_oh >= 0, l64, cc.long64);
            expect_true("align_tasks_long within the band rule's count", lng <= cc.long32 + cc.long64, lng, cc.long32 + cc.long64);
        }
    }
    if (c.count_one) {
        long long exts = 0;
        for (const CasePiece &p : c.pieces) exts += 2;
        const long long one = (long long)stat_of(st, "align_tasks_wide_one_piece");
        expect_one("align_tasks_wide_one_piece", cc.ext_one, one);
        expect_true("TASK_ONE extensions and others", one > 0 && one < exts, one, exts);
    }
    if (c.spans) {
        const long long NT = (long long)(n_fp_kept + n_kept_pieces);
        expect_one("align_spans", (NT + 63) / 64, (long long)stat_of(st, "align_spans"));
        expect_true("more than one span with rows", outs.size() > 1, (long long)outs.size());
    }
}

int run_device() {
    const std::vector<Case> cases = build_cases();
    const char *GROUPS[] = {"task_geometry", "band_rule", "certificates", "gap_cost", "run_buffers", "long_tasks", "ungapped", "assembly", "driver"};
    for (const char *g : GROUPS) {
        g_group = g; g_cases = g_kept = g_dropped = 0;
        double fast_default = -1, fast_off = -1;
        for (const Case &c : cases) {
            if (c.group != g) continue;
            run_case(c);
            if (c.group == "certificates") {         // granted by default, fewer with the certificates off
                const std::map<std::string, double> st = stats_json();
                const double f = stat_of(st, "align_tasks_fast") + stat_of(st, "align_ext_certified");
                if (c.hooks.empty()) { fast_default = f; expect_true("certificates are granted by default", stat_of(st, "align_tasks_fast") > 0 && stat_of(st, "align_ext_certified") > 0); }
                else if (c.hooks.size() > 1) { fast_off = f; expect_true("fewer certified tasks with the certificates off", fast_off < fast_default, (long long)fast_default, (long long)fast_off); }
            }
        }
        if (std::string(g) == "long_tasks") expect_true("an option set with ext_all_long and one without", g_seen_ext_all_long[0] && g_seen_ext_all_long[1]);
        printf("group %s cases=%zu kept=%zu dropped=%zu ok\n", g, g_cases, g_kept, g_dropped);
        fflush(stdout);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && std::string(argv[1]) == "--host") return host_checks();
        if (argc >= 3 && std::string(argv[1]) == "--cases") { write_cases(build_cases(), argv[2]); return 0; }
        if (argc >= 3 && std::string(argv[1]) == "--dump") return dump(argv[2]);
        if (argc != 1) { printf("usage: align_gpu_check [--host | --cases FILE | --dump FILE]\n"); return 2; }
        if (hlmi_init(0, 0) != HLMI_OK) { printf("hlmi_init: %s\n", hlmi_last_error()); return 2; }
        const int rc = run_device();
        hlmi_shutdown();
        return rc;
    } catch (const Mismatch &) {
        return 1;
    } catch (const std::exception &e) {
        printf("ERROR group %s case %s: %s\n", g_group, g_case.c_str(), e.what());
        return 2;
    }
}
