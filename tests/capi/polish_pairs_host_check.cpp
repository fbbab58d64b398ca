// polish_pairs_host_check.cpp - hylight_amd/csrc/pair_list.h (the list scan and the pair set of hlmi_polish_pairs) held to
// literal answers, with the host compiler alone (tests/test_polish_pairs_surface.py builds it plain and with
// -fsanitize=address,undefined and runs it).  The answers are the header's rules (include/hylight_mi.h: "List file format",
// "Meaning") worked by hand.
#include <cstdio>
#include <string>
#include <vector>

#include "../../hylight_amd/csrc/pair_list.h"

using namespace hlmi::pol;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

struct Got {
    uint64_t bad;
    std::vector<PairLine> lines;
    PairSet set;
};

static Got run(const std::string &text, const KnownNames &known) {
    Got g;
    g.bad = scan_pair_list(text, g.lines);
    g.set = make_pair_set(g.lines, known);
    return g;
}

int main() {
    const std::vector<std::string> reads = {"r1", "r10", "r2", "r1"}, contigs = {"c", "c2"};      // (r1 twice: one id)
    KnownNames known;
    known.add(reads);
    known.add(contigs);
    EXPECT(known.id.size() == 5 && known.find("r1") == 0 && known.find("r10") == 1 && known.find("c") == 3 && known.find("r") == -1);
    const uint32_t r1 = 0, r10 = 1, r2 = 2, c = 3, c2 = 4;

    {   // 6, 12 and 14 fields (the stage's trailing TAB), either order, duplicates, no trailing newline
        const std::string t = "r1\t1\t2\t3\t+\tc\n"
                              "c\t1\t2\t3\t+\tr10\t7\t8\t9\t10\t11\t12\n"
                              "r1\t1\t2\t3\t+\tc\t7\t8\t9\t10\t11\t0.9\t3\t1.0\t\n"
                              "c2\t\t\t\t\tr2";
        const Got g = run(t, known);
        EXPECT(g.bad == 0 && g.lines.size() == 4 && g.lines[3].a == "c2" && g.lines[3].b == "r2" && g.lines[1].b == "r10");
        EXPECT(g.set.listed == 3 && g.set.unknown == 0 && g.set.keys.size() == 6);
        EXPECT(g.set.has(r1, c) && g.set.has(c, r1) && g.set.has(r10, c) && g.set.has(c, r10) && g.set.has(r2, c2) && g.set.has(c2, r2));
        EXPECT(!g.set.has(r2, c) && !g.set.has(r10, c2) && !g.set.has(r1, r10));
    }
    {   // a prefix is another name; a \r stays in the last field; unknown names are counted per row
        const std::string t = "r1\t\t\t\t\tc\r\nr\t\t\t\t\tc\nr1\t\t\t\t\tc2\r\tx\r\nr100\t\t\t\t\tnobody\nr1\t\t\t\t\tr1\n";
        const Got g = run(t, known);                     // (the lines are views into t)
        EXPECT(g.bad == 0 && g.lines.size() == 5 && g.lines[0].b == "c\r" && g.lines[2].b == "c2\r");
        EXPECT(g.set.listed == 0 && g.set.unknown == 4 && g.set.keys.empty() && !g.set.has(r1, c));
    }
    {   // fewer than 6 fields: the 1-based line, an empty line included; the rows in front of it are kept
        std::vector<PairLine> l;
        EXPECT(scan_pair_list("r1\t\t\t\t\tc\nr1\t\t\t\tc\n", l) == 2 && l.size() == 1);
        l.clear();
        EXPECT(scan_pair_list("r1\t\t\t\t\tc\n\nr2\t\t\t\t\tc\n", l) == 2);
        l.clear();
        EXPECT(scan_pair_list("\n", l) == 1);
        l.clear();
        EXPECT(scan_pair_list("a\tb\tc\td\te", l) == 1);
        l.clear();
        EXPECT(scan_pair_list("", l) == 0 && l.empty());
        l.clear();
        EXPECT(scan_pair_list("\t\t\t\t\t", l) == 0 && l.size() == 1 && l[0].a.empty() && l[0].b.empty());
        l.clear();
        EXPECT(scan_pair_list("a\t\t\t\t\tb\tc", l) == 0 && l[0].a == "a" && l[0].b == "b");
    }
    {   // an empty list lists nothing
        const std::string t;
        const Got g = run(t, known);
        EXPECT(g.bad == 0 && g.set.listed == 0 && g.set.unknown == 0 && !g.set.has(r1, c));
    }
    if (n_bad) return 1;
    printf("polish_pairs_host_check: ok\n");
    return 0;
}
