// depth_host_check.cpp - hylight_amd/csrc/depth_text.h (the contig records, the abundance, the TSV and bedGraph lines of
// hlmi_depth) held to literal answers, with the host compiler alone (tests/test_depth_surface.py builds it with
// -fsanitize=address,undefined and runs it).  The answers are the header's rules (include/hylight_mi.h: hlmi_depth) worked by
// hand; tests/test_depth_model.py holds the model to the same literals.
#include <cstdio>
#include <string>
#include <vector>

#include "../../hylight_amd/csrc/depth_text.h"

using namespace hlmi::depth;

static int n_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++n_bad; } \
    } while (0)

static const std::string HEAD = "#contig\tlength\treads\tbases\tcovered\tmean_depth\tmedian_depth\tabundance";
typedef std::vector<std::string> Lines;

int main() {
    {   // one contig of 10 bases under [0,4) [2,10) [2,6): depths 1 1 3 3 2 2 1 1 1 1
        const Lines names = {"c"};
        const std::vector<uint64_t> length = {10};
        const std::vector<uint32_t> rc = {3}, slot = {0}, cbase = {0, 10};
        DeviceDepth d;
        d.covered = {10}; d.bases = {16}; d.median = {1};
        d.run_start = {0, 2, 4, 6}; d.run_depth = {1, 3, 2, 1};
        DepthTotals t;
        const std::vector<ContigDepth> recs = contig_records(names, length, rc, slot, d, &t);
        EXPECT(t.contigs_covered == 1 && t.positions == 10 && t.covered == 10 && t.bases == 16);
        EXPECT((tsv_lines(recs) == Lines{HEAD, "c\t10\t3\t16\t10\t1.600000\t1\t1.000000"}));
        EXPECT((bedgraph_lines(names, length, rc, slot, cbase, d) == Lines{"c\t0\t2\t1", "c\t2\t4\t3", "c\t4\t6\t2", "c\t6\t10\t1"}));
    }
    {   // a (8 bases, mean 1.5), n (6 bases, no row), e (no bases), b (10 bases, mean 0.5): abundances 0.75, 0, 0, 0.25; the runs of
        // a and b lie side by side in the device's positions (b starts at 8) and the last run of a ends where a ends
        const Lines names = {"a", "n", "e", "b"};
        const std::vector<uint64_t> length = {8, 6, 0, 10};
        const std::vector<uint32_t> rc = {2, 0, 0, 1}, slot = {0, 0, 0, 1}, cbase = {0, 8, 18};
        DeviceDepth d;
        d.covered = {8, 5}; d.bases = {12, 5}; d.median = {1, 0};
        d.run_start = {0, 2, 6, 8, 13}; d.run_depth = {1, 2, 1, 0, 1};
        DepthTotals t;
        const std::vector<ContigDepth> recs = contig_records(names, length, rc, slot, d, &t);
        EXPECT(t.contigs_covered == 2 && t.positions == 24 && t.covered == 13 && t.bases == 17);
        EXPECT((tsv_lines(recs) == Lines{HEAD, "a\t8\t2\t12\t8\t1.500000\t1\t0.750000", "n\t6\t0\t0\t0\t0.000000\t0\t0.000000",
                                         "e\t0\t0\t0\t0\t0.000000\t0\t0.000000", "b\t10\t1\t5\t5\t0.500000\t0\t0.250000"}));
        EXPECT((bedgraph_lines(names, length, rc, slot, cbase, d) ==
                Lines{"a\t0\t2\t1", "a\t2\t6\t2", "a\t6\t8\t1", "n\t0\t6\t0", "b\t0\t5\t0", "b\t5\t10\t1"}));
        const std::vector<double> ab = abundances(recs);
        EXPECT(ab.size() == 4 && ab[0] == 0.75 && ab[1] == 0.0 && ab[2] == 0.0 && ab[3] == 0.25);
    }
    {   // two adjacent contigs with the same depth at their junction are two runs: the device flags a contig's first position
        const Lines names = {"a", "b"};
        const std::vector<uint64_t> length = {5, 3};
        const std::vector<uint32_t> rc = {1, 1}, slot = {0, 1}, cbase = {0, 5, 8};
        DeviceDepth d;
        d.covered = {2, 1}; d.bases = {2, 1}; d.median = {0, 0};
        d.run_start = {0, 3, 5, 6}; d.run_depth = {0, 1, 1, 0};
        EXPECT((bedgraph_lines(names, length, rc, slot, cbase, d) == Lines{"a\t0\t3\t0", "a\t3\t5\t1", "b\t0\t1\t1", "b\t1\t3\t0"}));
    }
    {   // nothing selected anywhere: the sum of the means is 0 and every abundance prints as 0.000000; no device output at all
        const Lines names = {"e", "c"};
        const std::vector<uint64_t> length = {0, 4};
        const std::vector<uint32_t> rc = {0, 0}, slot = {0, 0}, cbase = {0};
        const DeviceDepth d;
        DepthTotals t;
        const std::vector<ContigDepth> recs = contig_records(names, length, rc, slot, d, &t);
        EXPECT(t.contigs_covered == 0 && t.positions == 4 && t.covered == 0 && t.bases == 0);
        EXPECT((tsv_lines(recs) == Lines{HEAD, "e\t0\t0\t0\t0\t0.000000\t0\t0.000000", "c\t4\t0\t0\t0\t0.000000\t0\t0.000000"}));
        EXPECT((bedgraph_lines(names, length, rc, slot, cbase, d) == Lines{"c\t0\t4\t0"}));
    }
    {   // no contig at all: the header line alone
        const DeviceDepth d;
        EXPECT((tsv_lines(contig_records({}, {}, {}, {}, d, nullptr)) == Lines{HEAD}));
        EXPECT(bedgraph_lines({}, {}, {}, {}, {0}, d).empty());
    }
    if (n_bad) return 1;
    printf("depth_host_check: ok\n");
    return 0;
}
