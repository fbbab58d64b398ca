// phase_ins_host_check.cpp - hylight_amd/csrc/phase_ins_text.h (which insertion sites take part, the merge of position sites and
// insertion sites into the site order, the site, link and read lines with their `+` marks, the three counters) held to literal
// answers, with the host compiler alone (tests/test_phase_ins_surface.py builds it with -fsanitize=address,undefined and runs
// it).  The answers are the header's rules (include/hylight_mi.h: hlmi_phase_ins) worked by hand; tests/phase_ins_inputs.py holds
// the model to hand cases of the same kind.
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../hylight_amd/csrc/phase_ins_text.h"

using namespace hlmi::ph;
using hlmi::var::DeviceInsertions;
using hlmi::var::InsRec;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

static const std::string SITES = "#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase";
static const std::string LINKS = "#contig\tpos1\tpos2\tn00\tn01\tn10\tn11\tinformative\tagree\tphased";
static const std::string READS = "#read\tcontig\tblock\tspanned\thap_a\thap_b\tother\thap";
typedef std::vector<std::string> Lines;
static const LinkCounts CIS = {3, 0, 0, 3}, TRANS = {0, 3, 3, 0}, TIE = {1, 1, 1, 1}, NONE = {0, 0, 0, 0};

static InsRec ins(uint32_t pos, uint32_t span, uint32_t i, uint32_t l, uint32_t len, uint32_t len_count, const char *seq) {
    InsRec r{};
    r.pos = pos; r.span = span; r.ins = i; r.ins_long = l; r.len = len; r.len_count = len_count;
    memcpy(r.seq, seq, strlen(seq));
    return r;
}
// a position site on 0-based position p of contig c (own G, alt T, three votes each)
static PSite snp(uint32_t c, uint32_t p, uint32_t gbase) { return PSite{c, p, gbase + p, 2, 3, {0, 0, 3, 3, 0}}; }

int main() {
    // contigs a (20 bases, covered), m (no rows), b (12 bases, covered): the covered ones side by side, cbase 0, 20, 32
    const std::string sa = "ACGTACGTACGTACGTACGT", sm = "ACGT", sb = "acgtacgtacgt";
    const std::vector<std::string_view> seq = {sa, sm, sb};
    const std::vector<std::string> names = {"a", "m", "b"};
    const std::vector<uint32_t> rc = {6, 0, 6}, slot_of_contig = {0, 0, 1}, cbase = {0, 20, 32};

    {   // the takes-part rule: a length, and min_alt rows behind it
        EXPECT(ins_takes_part(ins(5, 6, 3, 0, 2, 3, "TT"), 2) && ins_takes_part(ins(5, 6, 2, 0, 2, 2, "TT"), 2));
        EXPECT(!ins_takes_part(ins(5, 6, 2, 0, 1, 1, "T"), 2) && !ins_takes_part(ins(5, 6, 0, 2, 0, 0, ""), 1));
        EXPECT(site_key(5, true) == 10 && site_key(5, false) == 11 && site_key(4, false) == 9);
        EXPECT(site_key(0x7fffffffu, false) == 0xffffffffu);
    }
    {   // mark_field: the + behind a field in the middle, the last one, the first one
        std::string l = "c\t5\t11\tx";
        mark_field(l, 1);
        EXPECT(l == "c\t5+\t11\tx");
        mark_field(l, 3);
        EXPECT(l == "c\t5+\t11\tx+");
        mark_field(l, 0);
        EXPECT(l == "c+\t5+\t11\tx+");
    }
    // a: position 4 (prints 5), slot 5 (prints 5, behind it), slot 6 left out (one row of its length), position 10, slot 12 of
    // long rows alone left out; b: slot 1 (g = 21, anchor 'a' -> A) in front of position 1 (g = 21), position 0 in front of both
    const std::vector<PSite> positions = {snp(0, 4, 0), snp(0, 10, 0), snp(2, 0, 20), snp(2, 1, 20)};
    DeviceInsertions dev;
    dev.recs = {ins(5, 6, 3, 0, 2, 3, "TT"), ins(6, 6, 2, 0, 1, 1, "G"), ins(12, 6, 0, 2, 0, 0, ""), ins(21, 8, 4, 1, 16, 3, "ACGTTGCAACGTTGCA")};
    MergedSites M;
    EXPECT(merge_sites(seq, rc, slot_of_contig, cbase, positions, dev, 2, M));
    EXPECT(M.sites.size() == 6 && M.ins.size() == 2 && M.ins_sites_phasing == 2 && M.ins_sites_left_out == 2);
    EXPECT((M.key == std::vector<uint32_t>{9, 10, 21, 41, 42, 43}));
    EXPECT((M.ins_of == std::vector<int32_t>{-1, 0, -1, -1, 1, -1}));
    EXPECT(M.sites.size() == 6 && M.sites[1].contig == 0 && M.sites[1].pos == 4 && M.sites[4].contig == 2 && M.sites[4].pos == 0);
    EXPECT((M.anchor == std::vector<char>{'A', 'A'}));
    {   // min_alt 4: no insertion site takes part and the list is the position sites
        MergedSites P;
        EXPECT(merge_sites(seq, rc, slot_of_contig, cbase, positions, dev, 4, P));
        EXPECT(P.sites.size() == 4 && P.ins.empty() && P.ins_sites_phasing == 0 && P.ins_sites_left_out == 4);
        EXPECT((P.key == std::vector<uint32_t>{9, 21, 41, 43}));
        const Blocks B = build_blocks_reach(P.sites, ReachLinks{1, {CIS, NONE, CIS}}, 3, 0.8).base;
        EXPECT(phase_ins_site_lines(names, P, B) == phase_reach_site_lines(names, P.sites, B));
        EXPECT(phase_ins_link_lines(names, P, ReachLinks{1, {CIS, NONE, CIS}}, 3, 0.8) ==
               phase_reach_link_lines(names, P.sites, ReachLinks{1, {CIS, NONE, CIS}}, 3, 0.8));
        EXPECT(ins_sites_phased(P, B) == 0);
    }
    {   // a record at slot 0 of its contig (b's: a's length), behind the last contig, and one of 17 bases are no sites
        DeviceInsertions bad;
        MergedSites X;
        bad.recs = {ins(20, 6, 3, 0, 2, 3, "TT")};
        EXPECT(!merge_sites(seq, rc, slot_of_contig, cbase, positions, bad, 2, X));
        bad.recs = {ins(32, 6, 3, 0, 2, 3, "TT")};
        EXPECT(!merge_sites(seq, rc, slot_of_contig, cbase, positions, bad, 2, X));
        bad.recs = {ins(5, 6, 3, 0, 17, 3, "TT")};
        EXPECT(!merge_sites(seq, rc, slot_of_contig, cbase, positions, bad, 2, X));
    }
    // reach 2 over the six sites.  a: (5, 5+) a tie, (5, 11) cis, (5+, 11) a tie: the slot is bridged inside block 5.  b:
    // (1, 1+) unphased, (1, 2) unphased, (1+, 2) trans: blocks 1 and 1+
    ReachLinks L;
    L.reach = 2;
    L.n = {TIE, CIS, TIE, NONE, NONE, NONE, TIE, TIE, TRANS, NONE};
    const ReachBlocks R = build_blocks_reach(M.sites, L, 3, 0.8);
    const Blocks &B = R.base;
    EXPECT((B.first == std::vector<uint32_t>{0, 3, 4}) && R.sites_bridged == 1 && B.blocks_multi == 2 && B.sites_phased == 4);
    EXPECT(ins_sites_phased(M, B) == 1);
    EXPECT((phase_ins_site_lines(names, M, B) ==
            Lines{SITES, "a\t5\tG\tT\t6\t3\t3\t5\t0|1", "a\t5\tA\t+TT\t6\t3\t3\t5\t.", "a\t11\tG\tT\t6\t3\t3\t5\t0|1", "b\t1\tG\tT\t6\t3\t3\t1\t0|1",
                  "b\t1\tA\t+ACGTTGCAACGTTGCA\t8\t3\t3\t1+\t0|1", "b\t2\tG\tT\t6\t3\t3\t1+\t1|0"}));
    EXPECT((phase_ins_link_lines(names, M, L, 3, 0.8) ==
            Lines{LINKS, "a\t5\t5+\t1\t1\t1\t1\t4\t0.500000\t-", "a\t5\t11\t3\t0\t0\t3\t6\t1.000000\tcis", "a\t5+\t11\t1\t1\t1\t1\t4\t0.500000\t-",
                  "b\t1\t1+\t1\t1\t1\t1\t4\t0.500000\t-", "b\t1\t2\t1\t1\t1\t1\t4\t0.500000\t-", "b\t1+\t2\t0\t3\t3\t0\t6\t1.000000\ttrans"}));
    {   // the records of three rows: one over block 0 with nothing to say (dropped), one over blocks 1 and 2, one tie
        const std::vector<ReadRec> recs = {{0, 0, 3, 0, 0, 0}, {1, 1, 1, 0, 1, 0}, {1, 2, 2, 2, 0, 0}, {2, 2, 2, 1, 1, 1}};
        const std::vector<std::string> reads = {"r0", "r1", "r2"};
        const std::vector<uint32_t> of_row = {0, 1, 2};
        Lines lines;
        ReadTotals t;
        EXPECT(phase_ins_read_lines(names, reads, of_row, M, B, recs, &lines, &t));
        EXPECT((lines == Lines{READS, "r1\tb\t1\t1\t0\t1\t0\tB", "r1\tb\t1+\t2\t2\t0\t0\tA", "r2\tb\t1+\t2\t1\t1\t1\t-"}));
        EXPECT(t.records == 3 && t.a == 1 && t.b == 1 && t.tie == 1);
        ReadTotals alone;
        EXPECT(phase_ins_read_lines(names, reads, {}, M, B, recs, nullptr, &alone) && alone.records == 3);
        const std::vector<ReadRec> bad = {{0, 3, 1, 1, 0, 0}};
        EXPECT(!phase_ins_read_lines(names, reads, of_row, M, B, bad, &lines, &t));
    }
    {   // nothing at all
        MergedSites E;
        EXPECT(merge_sites(seq, rc, slot_of_contig, cbase, {}, DeviceInsertions{}, 2, E) && E.sites.empty());
        const Blocks B0 = build_blocks_reach(E.sites, ReachLinks{}, 3, 0.8).base;
        EXPECT((phase_ins_site_lines(names, E, B0) == Lines{SITES}) && (phase_ins_link_lines(names, E, ReachLinks{}, 3, 0.8) == Lines{LINKS}));
        EXPECT(ins_sites_phased(E, B0) == 0);
    }
    if (n_bad) return 1;
    printf("phase_ins_host_check: ok\n");
    return 0;
}
