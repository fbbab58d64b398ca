// variants_ins_host_check.cpp - hylight_amd/csrc/variants_ins_text.h (the insertion sites' records per contig, ins_rate, the lines
// of out_ins and of the summary of hlmi_variants_ins) held to literal answers, with the host compiler alone
// (tests/test_variants_ins_surface.py builds it with -fsanitize=address,undefined and runs it).  The answers are the header's
// rules (include/hylight_mi.h: hlmi_variants_ins) worked by hand; tests/test_variants_ins_model.py holds the model to literals of
// the same kind.
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "../../hylight_amd/csrc/variants_ins_text.h"

using namespace hlmi::var;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

static const std::string INS = "#contig\tpos\tref\tspan\tins\tins_long\tins_frac\tlen\tlen_count\tseq";
static const std::string SUMMARY = "#contig\tlength\treads\tcallable\tsites\tsite_rate\tslots\tins_sites\tins_rate";
typedef std::vector<std::string> Lines;

// a record whose seq holds `bases` and 0xff behind them, as the device's memset leaves what no kernel wrote
static InsRec rec(uint32_t pos, uint32_t span, uint32_t ins, uint32_t lng, uint32_t len, uint32_t len_count, const char *bases) {
    InsRec r;
    memset(&r, 0xff, sizeof r);
    r.pos = pos; r.span = span; r.ins = ins; r.ins_long = lng; r.len = len; r.len_count = len_count;
    memcpy(r.seq, bases, strlen(bases) < sizeof r.seq ? strlen(bases) : sizeof r.seq);
    return r;
}

int main() {
    EXPECT(sizeof(InsRec) == 40 && INS_CAP == 16);
    {   // one contig of 10 bases: slot 4 behind a lower-case t (two of five rows insert G), slot 9, the last one (sixteen bases,
        // and a long row beside the two that insert them), slot 1, the first one (long rows alone)
        const Lines names = {"c"};
        const std::vector<std::string_view> seq = {"ACGtACGTnC"};
        const std::vector<uint64_t> length = {10};
        const std::vector<uint32_t> rc = {5}, slot = {0}, cbase = {0, 10};
        DeviceVariants d;
        d.callable = {10}; d.ref_other = {0}; d.sites = {0};
        DeviceInsertions di;
        di.slots_callable = {9}; di.ins_sites = {3};
        di.recs = {rec(1, 5, 0, 2, 0, 0, ""), rec(4, 5, 2, 0, 1, 2, "G"), rec(9, 7, 2, 1, 16, 2, "ACGTTGCAACGTTGCN")};
        InsTotals t;
        const std::vector<ContigInsertions> irecs = contig_insertions(rc, slot, di, &t);
        EXPECT(t.slots_callable == 9 && t.ins_sites == 3 && irecs.size() == 1 && irecs[0].slots == 9 && irecs[0].ins_sites == 3);
        Lines lines;
        EXPECT(ins_lines(names, seq, rc, slot, cbase, di, lines));
        EXPECT((lines == Lines{INS, "c\t1\tA\t5\t0\t2\t0.400000\t0\t0\t*", "c\t4\tT\t5\t2\t0\t0.400000\t1\t2\tG",
                               "c\t9\tN\t7\t2\t1\t0.428571\t16\t2\tACGTTGCAACGTTGCN"}));                // ref is upper-cased
        const std::vector<ContigVariants> recs = contig_records(names, length, rc, slot, d, nullptr);
        EXPECT((ins_summary_lines(recs, irecs) == Lines{SUMMARY, "c\t10\t5\t10\t0\t0.000000\t9\t3\t0.333333"}));
        // the first six columns are summary_lines's
        EXPECT(ins_summary_lines(recs, irecs)[1].rfind(summary_lines(recs)[1], 0) == 0);
    }
    {   // a (8 bases), n (6 bases, no row), e (no bases), b (10 bases): a and b lie side by side in the device's positions (b
        // starts at 8): a's last slot (7) and b's first (9 = 8 + 1) are sites; b has 2 sites in 9 slots
        const Lines names = {"a", "n", "e", "b"};
        const std::vector<std::string_view> seq = {"ACGTACGT", "ACGTAC", "", "GNACGTACGT"};
        const std::vector<uint64_t> length = {8, 6, 0, 10};
        const std::vector<uint32_t> rc = {2, 0, 0, 7}, slot = {0, 0, 0, 1}, cbase = {0, 8, 18};
        DeviceVariants d;
        d.callable = {8, 3}; d.ref_other = {0, 1}; d.sites = {1, 1};
        DeviceInsertions di;
        di.slots_callable = {7, 9}; di.ins_sites = {1, 2};
        di.recs = {rec(7, 2, 2, 0, 3, 1, "TGA"), rec(9, 7, 3, 0, 2, 2, "NA"), rec(17, 6, 1, 1, 1, 1, "C")};
        InsTotals t;
        const std::vector<ContigInsertions> irecs = contig_insertions(rc, slot, di, &t);
        EXPECT(t.slots_callable == 16 && t.ins_sites == 3 && irecs.size() == 4 && irecs[1].slots == 0 && irecs[3].ins_sites == 2);
        Lines lines;
        EXPECT(ins_lines(names, seq, rc, slot, cbase, di, lines));
        EXPECT((lines == Lines{INS, "a\t7\tG\t2\t2\t0\t1.000000\t3\t1\tTGA", "b\t1\tG\t7\t3\t0\t0.428571\t2\t2\tNA",
                               "b\t9\tG\t6\t1\t1\t0.333333\t1\t1\tC"}));
        const std::vector<ContigVariants> recs = contig_records(names, length, rc, slot, d, nullptr);
        EXPECT((ins_summary_lines(recs, irecs) ==
                Lines{SUMMARY, "a\t8\t2\t8\t1\t0.125000\t7\t1\t0.142857", "n\t6\t0\t0\t0\t0.000000\t0\t0\t0.000000",
                      "e\t0\t0\t0\t0\t0.000000\t0\t0\t0.000000", "b\t10\t7\t3\t1\t0.333333\t9\t2\t0.222222"}));
        // records that do not fit their contig are refused, not written
        const auto refused = [&](std::vector<InsRec> recs_) {
            DeviceInsertions bad = di;
            bad.recs = std::move(recs_);
            return !ins_lines(names, seq, rc, slot, cbase, bad, lines);
        };
        EXPECT(refused({rec(0, 2, 2, 0, 1, 2, "A")}));                     // position 0 of a contig: no slot
        EXPECT(refused({rec(8, 7, 3, 0, 1, 3, "A")}));                     // position 0 of b
        EXPECT(refused({rec(18, 7, 3, 0, 1, 3, "A")}));                    // behind the last contig
        EXPECT(refused({rec(0xffffffffu, 7, 3, 0, 1, 3, "A")}));           // never written
        EXPECT(refused({rec(9, 7, 3, 0, 1, 3, "A"), rec(7, 2, 2, 0, 1, 2, "A")}));     // out of order
        EXPECT(refused({rec(7, 2, 2, 1, 1, 2, "A")}));                     // i + l > s
        EXPECT(refused({rec(7, 0, 0, 0, 0, 0, "")}));                      // no spanning row
        EXPECT(refused({rec(7, 4, 2, 0, 1, 3, "A")}));                     // len_count > i
        EXPECT(refused({rec(7, 40, 20, 0, 17, 3, "ACGTACGTACGTACGT")}));   // len > 16
        EXPECT(refused({rec(7, 4, 2, 0, 0, 0, "")}));                      // inserting rows and no length
        EXPECT(refused({rec(7, 4, 0, 2, 1, 0, "A")}));                     // a length and no inserting row
        EXPECT(refused({rec(7, 4, 2, 0, 2, 2, "A")}));                     // seq[1] was never written
        EXPECT(refused({rec(7, 4, 2, 0, 1, 2, "a")}));                     // a byte the device does not write
        EXPECT(!refused({rec(7, 4, 2, 2, 1, 2, "A")}));                    // i + l == s is fine
    }
    {   // nothing selected anywhere: the header line alone, a summary of zeros; no device output at all
        const Lines names = {"e", "c"};
        const std::vector<std::string_view> seq = {"", "ACGT"};
        const std::vector<uint64_t> length = {0, 4};
        const std::vector<uint32_t> rc = {0, 0}, slot = {0, 0}, cbase = {0};
        const DeviceVariants d;
        const DeviceInsertions di;
        InsTotals t;
        const std::vector<ContigInsertions> irecs = contig_insertions(rc, slot, di, &t);
        Lines lines;
        EXPECT(ins_lines(names, seq, rc, slot, cbase, di, lines) && lines == Lines{INS});
        EXPECT(t.slots_callable == 0 && t.ins_sites == 0);
        EXPECT((ins_summary_lines(contig_records(names, length, rc, slot, d, nullptr), irecs) ==
                Lines{SUMMARY, "e\t0\t0\t0\t0\t0.000000\t0\t0\t0.000000", "c\t4\t0\t0\t0\t0.000000\t0\t0\t0.000000"}));
    }
    {   // no contig at all
        const DeviceVariants d;
        const DeviceInsertions di;
        Lines lines;
        EXPECT(ins_lines({}, {}, {}, {}, {0}, di, lines) && lines == Lines{INS});
        EXPECT((ins_summary_lines(contig_records({}, {}, {}, {}, d, nullptr), contig_insertions({}, {}, di, nullptr)) == Lines{SUMMARY}));
    }
    if (n_bad) return 1;
    printf("variants_ins_host_check: ok\n");
    return 0;
}
