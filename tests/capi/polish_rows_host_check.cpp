// Stand-alone check of the per-op rule of hylight_amd/csrc/polish_rows.h - what turns a row's CIGAR into the compact CIGAR the
// polisher's kernels walk, with ins_edge and ins_long - on op lists the overlapper cannot be made to write.  Host compiler only,
// no GPU, no Python, meant for the host sanitizers as tests/capi/clique_host_check.cpp is:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/capi/polish_rows_host_check.cpp \
//       -o polish_rows_host_check
//   ./polish_rows_host_check
// Every case states, written out by hand, what the two loops of polish_host.cpp gave for the list before the rule moved into the
// header (compact ops, the slot of every I op, ins_edge, ins_long).  Those two loops are restated below as well and run on the
// cases and on random lists: the walk must give what they give.  Exit status 0 when everything holds.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../hylight_amd/csrc/polish_rows.h"

using namespace hlmi::pol;

enum : uint32_t { EQ = 7, X = 8, I = 1, D = 2 };            // common.h: OP_EQ, OP_X, OP_I, OP_D
static constexpr uint32_t NO = ROW_NO_SLOT;
static uint32_t W(uint32_t len, uint32_t code) { return len << 4 | code; }

struct Answer {
    std::vector<RowOp> ops;
    uint32_t ins_edge = 0, ins_long = 0;
};

static Answer walk(uint32_t ts, uint32_t te, const std::vector<uint32_t> &in) {
    Answer a;
    RowWalk w;
    RowOp done;
    row_walk_begin(w, ts, te);
    for (uint32_t word : in)
        if (row_walk_op(w, word, &done)) a.ops.push_back(done);
    if (row_walk_end(w, &done)) a.ops.push_back(done);
    if (w.n_out != a.ops.size()) a.ins_edge = 0xdeadu;      // (n_out counts the finished ops)
    else { a.ins_edge = w.ins_edge; a.ins_long = w.ins_long; }
    return a;
}

// polish_host.cpp before the header existed: the loop that compacts and counts ins_edge, the loop that counts ins_long
static Answer host_loops(uint32_t ts, uint32_t te, const std::vector<uint32_t> &in) {
    Answer a;
    std::vector<uint32_t> ops;
    uint32_t p = ts;
    for (uint32_t word : in) {
        const uint32_t len = word >> 4, code = word & 15u;
        if (!len) continue;
        if (code == I) {
            if (p == ts || p == te) ++a.ins_edge;
            if (!ops.empty() && (ops.back() & 15u) == I) {
                ops.back() += len << 4;
                continue;
            }
        } else p += len;
        ops.push_back(word);
    }
    p = ts;
    for (uint32_t w : ops) {
        uint32_t slot = NO;
        if ((w & 15u) != I) p += w >> 4;
        else if (p != ts && p != te) {
            slot = p;
            if ((w >> 4) > 16u) ++a.ins_long;
        }
        a.ops.push_back(RowOp{w, (w & 15u) == I ? slot : NO});
    }
    return a;
}

static int bad = 0;
static bool same(const Answer &a, const Answer &b) {
    if (a.ops.size() != b.ops.size() || a.ins_edge != b.ins_edge || a.ins_long != b.ins_long) return false;
    for (size_t k = 0; k < a.ops.size(); ++k)
        if (a.ops[k].word != b.ops[k].word || a.ops[k].slot != b.ops[k].slot) return false;
    return true;
}
static void check(const char *name, uint32_t ts, uint32_t te, const std::vector<uint32_t> &in, const Answer &want) {
    if (!same(walk(ts, te, in), want)) { ++bad; printf("FAILED %s: the walk differs from the answer written out\n", name); }
    if (!same(host_loops(ts, te, in), want)) { ++bad; printf("FAILED %s: the restated loops differ from the answer written out\n", name); }
}

int main() {
    // two I ops in a row are one insertion of five bases in front of position 15
    check("two I", 10, 19, {W(5, EQ), W(2, I), W(3, I), W(4, EQ)}, {{{W(5, EQ), NO}, {W(5, I), 15}, {W(4, EQ), NO}}, 0, 0});
    // three: 2 + 3 + 12 = 17 bases, each op within the cap and the insertion beyond it
    check("three I", 10, 19, {W(5, EQ), W(2, I), W(3, I), W(12, I), W(4, EQ)},
          {{{W(5, EQ), NO}, {W(17, I), 15}, {W(4, EQ), NO}}, 0, 1});
    // ops of length 0 are no ops: the I ops around them are neighbours
    check("zero-length ops between I", 10, 19, {W(5, EQ), W(2, I), W(0, D), W(3, I), W(0, EQ), W(0, I), W(1, I), W(4, EQ)},
          {{{W(5, EQ), NO}, {W(6, I), 15}, {W(4, EQ), NO}}, 0, 0});
    // ... and two = ops around an I of length 0 stay two ops
    check("zero-length I between =", 10, 17, {W(3, EQ), W(0, I), W(4, EQ)}, {{{W(3, EQ), NO}, {W(4, EQ), NO}}, 0, 0});
    // an I first and last in the row: no slot, one ins_edge each
    check("I first and last", 10, 16, {W(2, I), W(6, EQ), W(3, I)}, {{{W(2, I), NO}, {W(6, EQ), NO}, {W(3, I), NO}}, 2, 0});
    // two I ops first: one op, counted twice (ins_edge counts the ops of the CIGAR as it came)
    check("two I first", 10, 18, {W(1, I), W(1, I), W(8, EQ)}, {{{W(2, I), NO}, {W(8, EQ), NO}}, 2, 0});
    // 17 bases at the edge are an ins_edge, not an ins_long
    check("long I first", 10, 15, {W(17, I), W(5, EQ)}, {{{W(17, I), NO}, {W(5, EQ), NO}}, 1, 0});
    // 16 bases vote, 17 do not
    check("I of 16 and 17", 10, 20, {W(3, EQ), W(16, I), W(4, X), W(17, I), W(3, EQ)},
          {{{W(3, EQ), NO}, {W(16, I), 13}, {W(4, X), NO}, {W(17, I), 17}, {W(3, EQ), NO}}, 0, 1});
    // a D between two I ops keeps them apart: slots 13 and 14
    check("I D I", 10, 18, {W(3, EQ), W(2, I), W(1, D), W(2, I), W(4, EQ)},
          {{{W(3, EQ), NO}, {W(2, I), 13}, {W(1, D), NO}, {W(2, I), 14}, {W(4, EQ), NO}}, 0, 0});
    // rows of one op
    check("one =", 10, 17, {W(7, EQ)}, {{{W(7, EQ), NO}}, 0, 0});
    check("one D", 10, 11, {W(1, D)}, {{{W(1, D), NO}}, 0, 0});
    check("one I", 10, 10, {W(4, I)}, {{{W(4, I), NO}}, 1, 0});
    // nothing but ops of length 0, and no op at all
    check("only zero-length ops", 10, 10, {W(0, EQ), W(0, I)}, {{}, 0, 0});
    check("empty", 10, 10, {}, {{}, 0, 0});

    // random lists, short ops with many I and many zeros: the walk against the restated loops
    std::mt19937 rng(20240611);
    const uint32_t codes[4] = {EQ, X, I, D};
    for (int t = 0; t < 20000; ++t) {
        const int n = (int)(rng() % 12);
        std::vector<uint32_t> in;
        uint32_t t_cols = 0;
        for (int k = 0; k < n; ++k) {
            const uint32_t code = codes[rng() % 4 == 0 ? rng() % 4 : 2 * (rng() % 2)];       // mostly = and I
            const uint32_t len = rng() % 3 == 0 ? 0u : rng() % 4 == 0 ? 9u + rng() % 12 : 1u + rng() % 3;
            in.push_back(W(len, code));
            if (code != I) t_cols += len;
        }
        const uint32_t ts = rng() % 50;
        if (!same(walk(ts, ts + t_cols, in), host_loops(ts, ts + t_cols, in))) {
            if (++bad <= 10) printf("FAILED random list %d: the walk differs from the restated loops\n", t);
        }
    }
    if (bad) { printf("%d checks failed\n", bad); return 1; }
    printf("polish_rows_host_check: ok\n");
    return 0;
}
