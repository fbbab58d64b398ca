// Plain reference for the alignment side of the overlapper: the textbook affine-gap recurrence with a two-piece gap cost,
// written from the scoring rules of DESIGN.md section 5 and from nothing else.  Host only, no project header, no library.
//
//   align_ref_check [--path] JOBFILE
//
// One task per line of JOBFILE, one answer per line of the output:
//   global A B match mismatch ambi o1 e1 o2 e2 dlo dhi    best score of a global alignment of A and B whose cells (i, j) all have
//                                                         dlo <= j - i <= dhi; "none" when no such alignment exists.  With --path
//                                                         one optimal CIGAR follows the score (for reading, never for asserting).
//   extend A B match mismatch ambi o1 e1 o2 e2 rows cols b    best score over all cells i <= rows, j <= cols, |j - i| <= b of an
//                                                         alignment of A[0, i) with B[0, j) that starts in the corner; the empty
//                                                         extension scores 0.
// A and B are base strings in aligned orientation ("-" is the empty string).  A runs along i, B along j.
//
// Scores.  A column of two ACGT bases (case folded, U = T) scores +match when they are equal and -mismatch when not; any other
// byte on either side scores -ambi.  A gap of L bases costs min(o1 + e1 L, o2 + e2 L); o2 == 0 means the first piece alone.  A
// gap in A next to a gap in B is two gaps.
//
// Recurrence, for every cell inside the corridor, per gap piece p:
//   D_p(i, j) = max(H(i, j-1) - o_p - e_p, D_p(i, j-1) - e_p)     a gap that consumes B[j-1]
//   I_p(i, j) = max(H(i-1, j) - o_p - e_p, I_p(i-1, j) - e_p)     a gap that consumes A[i-1]
//   H(i, j)   = max(H(i-1, j-1) + column(A[i-1], B[j-1]), D_1, D_2, I_1, I_2),  H(0, 0) = 0
// A gap that changes its piece half way costs at least the cheaper piece for its whole length, so the maximum over the pieces
// is the min() of the gap cost.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static const int NONE = -(1 << 28);   // "no alignment ends here"; far below any score, far above overflow

struct Scores { int match, mismatch, ambi, open[2], ext[2], pieces; };

static int base_code(char c) {
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
    }
}

static int column(const Scores &s, char a, char b) {
    const int x = base_code(a), y = base_code(b);
    if (x == 4 || y == 4) return -s.ambi;
    return x == y ? s.match : -s.mismatch;
}

struct Row {   // one row of the matrices: H and the two gap states of either piece, valid for columns lo .. hi (the corridor)
    std::vector<int> H, D[2], I[2];
    int lo = 0, hi = -1;
    explicit Row(size_t n) : H(n, NONE) { for (int p = 0; p < 2; ++p) { D[p].assign(n, NONE); I[p].assign(n, NONE); } }
    bool has(int j) const { return j >= lo && j <= hi; }
    int h(int j) const { return has(j) ? H[j] : NONE; }          // a cell outside the corridor: no alignment ends there
    int d(int p, int j) const { return has(j) ? D[p][j] : NONE; }
    int i(int p, int j) const { return has(j) ? I[p][j] : NONE; }
};

static int minus(int v, int cost) { return v <= NONE ? NONE : v - cost; }

// Fills the corridor dlo <= j - i <= dhi of the (m+1) x (n+1) matrix.  Returns H(m, n) (global) or the maximum of H over all
// cells (extend).  keep: every row is kept for the path.
static int fill(const std::string &A, const std::string &B, const Scores &s, int dlo, int dhi, bool extend, std::vector<Row> *keep) {
    const int m = (int)A.size(), n = (int)B.size();
    Row prev(n + 1), cur(n + 1);
    int best = NONE;
    for (int i = 0; i <= m; ++i) {
        cur.lo = std::max(0, i + dlo);
        cur.hi = std::min(n, i + dhi);
        for (int j = cur.lo; j <= cur.hi; ++j) {
            for (int p = 0; p < 2; ++p) cur.D[p][j] = cur.I[p][j] = NONE;
            if (i == 0 && j == 0) { cur.H[j] = 0; continue; }
            int h = NONE;
            if (i > 0 && j > 0) h = minus(prev.h(j - 1), -column(s, A[i - 1], B[j - 1]));
            for (int p = 0; p < s.pieces; ++p) {
                cur.D[p][j] = std::max(minus(cur.h(j - 1), s.open[p] + s.ext[p]), minus(cur.d(p, j - 1), s.ext[p]));
                cur.I[p][j] = std::max(minus(prev.h(j), s.open[p] + s.ext[p]), minus(prev.i(p, j), s.ext[p]));
                h = std::max(h, std::max(cur.D[p][j], cur.I[p][j]));
            }
            cur.H[j] = h;
            best = std::max(best, h);
        }
        if (keep) keep->push_back(cur);
        std::swap(prev, cur);           // prev is row i from here on (row -1 has no column: hi < lo)
    }
    if (extend) return std::max(best, 0);
    return prev.h(n);
}

// One optimal path, found by asking every cell which of its sources gives its value.
static std::string path(const std::string &A, const std::string &B, const Scores &s, const std::vector<Row> &R) {
    std::string ops;          // one letter per column, last column first
    int i = (int)A.size(), j = (int)B.size();
    char state = 'H';
    int p = 0;
    while (i > 0 || j > 0) {
        if (state == 'H') {
            const int h = R[i].h(j);
            if (i > 0 && j > 0 && h == minus(R[i - 1].h(j - 1), -column(s, A[i - 1], B[j - 1]))) {
                ops += base_code(A[i - 1]) == base_code(B[j - 1]) ? '=' : 'X';
                --i; --j;
                continue;
            }
            for (p = 0; p < s.pieces && state == 'H'; ++p) {
                if (h == R[i].d(p, j)) state = 'D';
                else if (h == R[i].i(p, j)) state = 'I';
            }
            if (state == 'H') return "?";
            --p;
        } else if (state == 'D') {
            ops += 'D';
            if (R[i].d(p, j) == minus(R[i].h(j - 1), s.open[p] + s.ext[p])) state = 'H';
            --j;
        } else {
            ops += 'I';
            if (R[i].i(p, j) == minus(R[i - 1].h(j), s.open[p] + s.ext[p])) state = 'H';
            --i;
        }
    }
    std::reverse(ops.begin(), ops.end());
    std::string cg;
    for (size_t a = 0; a < ops.size();) {
        size_t b = a;
        while (b < ops.size() && ops[b] == ops[a]) ++b;
        cg += std::to_string(b - a) + ops[a];
        a = b;
    }
    return cg.empty() ? "*" : cg;
}

int main(int argc, char **argv) {
    bool want_path = false;
    const char *file = nullptr;
    for (int a = 1; a < argc; ++a) {
        if (std::string(argv[a]) == "--path") want_path = true;
        else file = argv[a];
    }
    if (!file) { std::fprintf(stderr, "usage: align_ref_check [--path] JOBFILE\n"); return 2; }
    std::ifstream in(file);
    if (!in) { std::fprintf(stderr, "align_ref_check: cannot read %s\n", file); return 2; }
    std::string line;
    long lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        if (line.empty()) continue;
        std::istringstream f(line);
        std::string kind, A, B;
        Scores s;
        int x, y, z = 0;
        f >> kind >> A >> B >> s.match >> s.mismatch >> s.ambi >> s.open[0] >> s.ext[0] >> s.open[1] >> s.ext[1] >> x >> y;
        if (kind == "extend") f >> z;
        if (!f || (kind != "global" && kind != "extend")) { std::fprintf(stderr, "align_ref_check: line %ld: bad task\n", lineno); return 2; }
        s.pieces = s.open[1] > 0 ? 2 : 1;
        if (A == "-") A.clear();
        if (B == "-") B.clear();
        if (kind == "extend") {
            if (x < 0 || y < 0 || z < 0) { std::fprintf(stderr, "align_ref_check: line %ld: negative bound\n", lineno); return 2; }
            A = A.substr(0, std::min((size_t)x, A.size()));
            B = B.substr(0, std::min((size_t)y, B.size()));
            std::cout << fill(A, B, s, -z, z, true, nullptr) << "\n";
            continue;
        }
        std::vector<Row> rows;
        const int score = fill(A, B, s, x, y, false, want_path ? &rows : nullptr);
        if (score <= NONE) std::cout << "none\n";
        else if (want_path) std::cout << score << " " << path(A, B, s, rows) << "\n";
        else std::cout << score << "\n";
    }
    return 0;
}
