// depth_text.h - the host half of hlmi_depth / hlmi_depth_reads (include/hylight_mi.h) that is text and arithmetic: the record
// of every contig (those that never reached the device included), the abundance, the TSV and the bedGraph lines.  Host-only and
// free of any HIP include, as seq_scan.h and pair_list.h are: tests/capi/depth_host_check.cpp compiles it with the plain host
// compiler under the sanitizers.  The arithmetic is the header's: mean = (double)bases / (double)length, the sum of the means in
// file order with one double addition per contig, abundance = mean / sum - compiled without contraction like the rest of the
// host code (there is no multiply-add to contract here, the flag is the build's).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace hlmi {
namespace depth {

struct ContigDepth {
    std::string name;
    uint64_t length = 0, reads = 0, bases = 0, covered = 0, median = 0;
};

// what the device found, per covered contig ("slot": its place among the contigs with a selected row) and per run
struct DeviceDepth {
    std::vector<uint64_t> covered, bases;       // per slot
    std::vector<uint32_t> median;               // per slot
    std::vector<uint32_t> run_start, run_depth; // runs over the covered contigs side by side, ascending; start counts from
                                                // the first covered contig's first position (cbase of the layout)
};

struct DepthTotals {
    uint64_t contigs_covered = 0, positions = 0, covered = 0, bases = 0;
};

// Every contig in file order.  rc: selected rows per contig; slot_of_contig: its slot when rc != 0.
inline std::vector<ContigDepth> contig_records(const std::vector<std::string> &names, const std::vector<uint64_t> &length,
                                               const std::vector<uint32_t> &rc, const std::vector<uint32_t> &slot_of_contig,
                                               const DeviceDepth &dev, DepthTotals *tot) {
    std::vector<ContigDepth> out(names.size());
    DepthTotals t;
    for (size_t c = 0; c < names.size(); ++c) {
        ContigDepth &r = out[c];
        r.name = names[c];
        r.length = length[c];
        r.reads = rc[c];
        if (rc[c]) {
            const uint32_t j = slot_of_contig[c];
            r.bases = dev.bases[j];
            r.covered = dev.covered[j];
            r.median = dev.median[j];
            ++t.contigs_covered;
        }
        t.positions += r.length;
        t.covered += r.covered;
        t.bases += r.bases;
    }
    if (tot) *tot = t;
    return out;
}

inline double mean_depth(const ContigDepth &r) { return r.length ? (double)r.bases / (double)r.length : 0.0; }

// the share of every contig's mean depth in the sum of all of them (0.0 each when the sum is 0)
inline std::vector<double> abundances(const std::vector<ContigDepth> &recs) {
    double sum = 0.0;
    for (const ContigDepth &r : recs) sum = sum + mean_depth(r);
    std::vector<double> a(recs.size(), 0.0);
    if (sum != 0.0)
        for (size_t c = 0; c < recs.size(); ++c) a[c] = mean_depth(recs[c]) / sum;
    return a;
}

// the lines of out_tsv, without their '\n': the header line, then one per contig
inline std::vector<std::string> tsv_lines(const std::vector<ContigDepth> &recs) {
    std::vector<std::string> lines;
    lines.reserve(recs.size() + 1);
    lines.push_back("#contig\tlength\treads\tbases\tcovered\tmean_depth\tmedian_depth\tabundance");
    const std::vector<double> ab = abundances(recs);
    for (size_t c = 0; c < recs.size(); ++c) {
        const ContigDepth &r = recs[c];
        char buf[192];
        snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%llu\t%.6f\t%llu\t%.6f", (unsigned long long)r.length, (unsigned long long)r.reads,
                 (unsigned long long)r.bases, (unsigned long long)r.covered, mean_depth(r), (unsigned long long)r.median, ab[c]);
        lines.push_back(r.name + buf);
    }
    return lines;
}

// The lines of out_bedgraph, without their '\n'.  cbase: where every slot starts in the run positions, and the total behind the
// last.  A contig without a selected row is one run of depth 0, one of no bases writes nothing; a run ends where the next one
// starts or where its contig ends.
inline std::vector<std::string> bedgraph_lines(const std::vector<std::string> &names, const std::vector<uint64_t> &length,
                                               const std::vector<uint32_t> &rc, const std::vector<uint32_t> &slot_of_contig,
                                               const std::vector<uint32_t> &cbase, const DeviceDepth &dev) {
    std::vector<std::string> lines;
    size_t k = 0;                               // next run
    const size_t n_runs = dev.run_start.size();
    char buf[96];
    for (size_t c = 0; c < names.size(); ++c) {
        if (!length[c]) continue;
        if (!rc[c]) {
            snprintf(buf, sizeof buf, "\t0\t%llu\t0", (unsigned long long)length[c]);
            lines.push_back(names[c] + buf);
            continue;
        }
        const uint32_t j = slot_of_contig[c];
        const uint64_t b = cbase[j], e = cbase[j + 1];
        while (k < n_runs && dev.run_start[k] < b) ++k;          // (none: the runs follow the slots)
        for (; k < n_runs && dev.run_start[k] < e; ++k) {
            const uint64_t end = k + 1 < n_runs && dev.run_start[k + 1] < e ? dev.run_start[k + 1] : e;
            snprintf(buf, sizeof buf, "\t%llu\t%llu\t%u", (unsigned long long)(dev.run_start[k] - b), (unsigned long long)(end - b),
                     dev.run_depth[k]);
            lines.push_back(names[c] + buf);
        }
    }
    return lines;
}

}  // namespace depth
}  // namespace hlmi
