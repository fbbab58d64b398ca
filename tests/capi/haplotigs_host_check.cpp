// haplotigs_host_check.cpp - hylight_amd/csrc/haplotigs_text.h (a row's side, the split rule, the extents, who is inside, the
// positions two sides decide differently, the blocks file's lines and a haplotig's header) held to literal answers, with the host
// compiler alone (tests/test_haplotigs_surface.py builds it with -fsanitize=address,undefined and runs it).  The answers are the
// header's rules (include/hylight_mi.h: hlmi_haplotigs) worked by hand; tests/test_haplotigs_model.py holds the model to the same.
#include <cstdio>
#include <string>
#include <vector>

#include "../../hylight_amd/csrc/haplotigs_text.h"

using namespace hlmi::hap;
using namespace hlmi::ph;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

typedef std::vector<std::string> Lines;
static const std::string HEAD = "#contig\tblock\tstart\tend\tsites\trows_a\trows_b\tsplit\tdiff_positions";

static PSite site(uint32_t contig, uint32_t pos, uint32_t gpos) {
    PSite s{};
    s.contig = contig;
    s.pos = pos;
    s.gpos = gpos;
    s.own = 2;
    s.alt = 3;
    return s;
}

int main() {
    {   // a row's side: hap_of of its record
        EXPECT(side_of({0, 0, 2, 2, 1, 0}) == SIDE_A && side_of({0, 0, 2, 0, 1, 0}) == SIDE_B);
        EXPECT(side_of({0, 0, 2, 1, 1, 0}) == SIDE_NONE && side_of({0, 0, 1, 0, 0, 1}) == SIDE_NONE);
    }
    {   // inside: a position of [first, last]; a slot of (first, last]
        EXPECT(!position_inside(6, 14, 5) && position_inside(6, 14, 6) && position_inside(6, 14, 14) && !position_inside(6, 14, 15));
        EXPECT(!slot_inside(6, 14, 6) && slot_inside(6, 14, 7) && slot_inside(6, 14, 14) && !slot_inside(6, 14, 15));
    }
    {   // contig a (slot 0): sites 2 6 10 in one block and site 15 alone; contig b (starts at 20): sites 0 and 7 in one block.
        // a's block has three records on A, two on B and a tie; b's two on A and three on B
        const Lines names = {"a", "n", "b"};
        const std::vector<PSite> sites = {site(0, 2, 2), site(0, 6, 6), site(0, 10, 10), site(0, 15, 15), site(2, 0, 20), site(2, 7, 27)};
        const std::vector<LinkCounts> links = {{3, 0, 0, 3}, {3, 0, 0, 3}, {1, 1, 1, 1}, {9, 9, 9, 9}, {0, 3, 3, 0}};
        const Blocks B = build_blocks(sites, links, 3, 0.8);
        EXPECT((B.first == std::vector<uint32_t>{0, 3, 4}));
        const std::vector<ReadRec> recs = {{0, 0, 3, 3, 0, 0}, {1, 0, 3, 2, 1, 0}, {2, 0, 3, 3, 0, 0}, {3, 0, 3, 0, 3, 0}, {4, 0, 2, 0, 2, 0},
                                           {5, 0, 2, 1, 1, 0}, {5, 1, 1, 1, 0, 0}, {6, 2, 2, 2, 0, 0}, {7, 2, 2, 1, 0, 1}, {8, 2, 2, 0, 2, 0},
                                           {9, 2, 2, 0, 1, 0}, {10, 2, 1, 0, 1, 0}};
        std::vector<HBlock> hb;
        EXPECT(haplotig_blocks(sites, B, recs, 2, hb) && hb.size() == 2);
        EXPECT(hb[0].block == 0 && hb[0].contig == 0 && hb[0].n_sites == 3 && hb[0].first == 2 && hb[0].last == 10 && hb[0].gfirst == 2 &&
               hb[0].glast == 10 && hb[0].rows_a == 3 && hb[0].rows_b == 2 && hb[0].split);
        EXPECT(hb[1].block == 2 && hb[1].contig == 2 && hb[1].first == 0 && hb[1].last == 7 && hb[1].gfirst == 20 && hb[1].glast == 27 &&
               hb[1].rows_a == 2 && hb[1].rows_b == 3 && hb[1].split);
        // min_side 3: a's B side and b's A side are one short
        std::vector<HBlock> h3;
        EXPECT(haplotig_blocks(sites, B, recs, 3, h3) && h3.size() == 2 && !h3[0].split && !h3[1].split);
        EXPECT((haplotig_block_lines(names, h3) == Lines{HEAD, "a\t3\t3\t11\t3\t3\t2\t0\t0", "b\t1\t1\t8\t2\t2\t3\t0\t0"}));
        // the decisions of 28 positions on two sides: they differ on 2 and 10 of a's extent and on 20 of b's; 15 differs outside
        std::vector<uint8_t> sym(56, 5);
        sym[2] = 2; sym[28 + 2] = 3; sym[28 + 10] = 4; sym[15] = 1; sym[20] = 0; sym[28 + 20] = 5; sym[6] = 2; sym[28 + 6] = 2;
        hb[0].diff = diff_positions(sym, 28, hb[0].gfirst, hb[0].glast);
        hb[1].diff = diff_positions(sym, 28, hb[1].gfirst, hb[1].glast);
        EXPECT(hb[0].diff == 2 && hb[1].diff == 1);
        EXPECT((haplotig_block_lines(names, hb) == Lines{HEAD, "a\t3\t3\t11\t3\t3\t2\t1\t2", "b\t1\t1\t8\t2\t2\t3\t1\t1"}));
        // a record of a block that does not exist: refused
        EXPECT(!haplotig_blocks(sites, B, {{0, 3, 1, 1, 0, 0}}, 2, hb));
        // no record at all: nothing is split; no site: no block
        EXPECT(haplotig_blocks(sites, B, {}, 1, hb) && hb.size() == 2 && !hb[0].split && hb[0].rows_a == 0);
        EXPECT(haplotig_blocks({}, build_blocks({}, {}, 3, 0.8), {}, 1, hb) && hb.empty());
        EXPECT((haplotig_block_lines(names, hb) == Lines{HEAD}));
    }
    {   // the headers
        EXPECT(haplotig_head("c", 'A', 40, 8, 40, 40, 1, 31) == ">c_hapA LN:i:40 RC:i:8 XC:f:1.000000 HB:i:1 HP:i:31");
        EXPECT(haplotig_head("c", 'B', 42, 8, 11, 20, 2, 9) == ">c_hapB LN:i:42 RC:i:8 XC:f:0.550000 HB:i:2 HP:i:9");
        EXPECT(haplotig_head("c", '\0', 10, 3, 4, 10, 0, 0) == ">c LN:i:10 RC:i:3 XC:f:0.400000");
    }
    if (n_bad) return 1;
    printf("haplotigs_host_check: ok\n");
    return 0;
}
