// seq_scan.h - the record scan of the FASTA / FASTQ reader (paf_io.cpp: read_seqs, read_seqs_subset, read_seqs_qual) and what
// hlmi_polish_q / hlmi_polish_reads_q do with a read file's quality strings before a row is looked at (include/hylight_mi.h:
// validation, reads_with_qual, the mean, the read floor).  Nothing of HIP's is included: tests/capi/polish_qual_host_check.cpp
// compiles this header with the host compiler alone.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <string_view>
#include <vector>

namespace hlmi {

// Sequence file reader with the record detection of kseq (FASTA '>' / FASTQ '@', multi-line).
struct SeqSet {
    std::vector<std::string> names;
    std::string bases;               // concatenated, as in the file (no case folding)
    std::vector<uint64_t> off;       // size n+1
    std::vector<uint32_t> first_line;  // 0-based line number of each record's header line
    uint64_t n_lines = 0;            // `wc -l` of the file (utils.py:44)
    size_t size() const { return names.size(); }
    uint32_t len(size_t i) const { return (uint32_t)(off[i + 1] - off[i]); }
};

// The quality strings of a SeqSet (read_seqs_qual).  `quals` is as long as SeqSet::bases and record i's bytes lie at
// SeqSet::off[i], so whatever indexes a base indexes its quality.  A record without a quality string (FASTA, or '@' with no '+'
// line) is filled with '!'.  A string that is not as long as the bases keeps its true length in qual_len; in `quals` it is cut,
// or filled up with 0 bytes.
struct SeqQual {
    std::string quals;
    std::vector<uint8_t> has_qual;   // per record
    std::vector<uint64_t> qual_len;  // per record: bytes of the quality string in the file (0 without one)
};

// The scan.  QUAL = false is the reader every caller but the polisher's _q calls uses: the quality lines are stepped over.
// `want` (may be null): only the records it accepts bring their bases along.
template <bool QUAL>
inline void scan_seq_records(std::string_view d, const std::function<bool(std::string_view)> *want, SeqSet &out, SeqQual *qual) {
    size_t N = d.size(), pos = 0;
    uint32_t line_no = 0;
    out.off.push_back(0);
    auto next_line = [&](std::string_view &L) -> bool {
        if (pos >= N) return false;
        size_t e = d.find('\n', pos);
        if (e == std::string::npos) e = N;
        size_t end = e;
        if (end > pos && d[end - 1] == '\r') --end;
        L = d.substr(pos, end - pos);
        pos = e + 1;
        ++line_no;
        return true;
    };
    std::string_view L;
    bool have = next_line(L);
    while (have) {
        if (L.empty() || (L[0] != '>' && L[0] != '@')) {  // kseq skips to the next header
            have = next_line(L);
            continue;
        }
        bool fq = L[0] == '@';
        size_t ws = L.find_first_of(" \t", 1);
        const std::string_view name = L.substr(1, (ws == std::string_view::npos ? L.size() : ws) - 1);
        const bool keep = !want || (*want)(name);             // a record that is not wanted keeps its name, with no bases
        out.names.emplace_back(name);
        out.first_line.push_back(line_no - 1);
        size_t slen = 0;
        have = next_line(L);
        while (have && !(L.size() && (L[0] == '>' || L[0] == '@' || L[0] == '+'))) {
            if (keep) out.bases.append(L);
            slen += L.size();
            have = next_line(L);
        }
        size_t q = 0;
        bool with_qual = false;
        if (fq && have && L.size() && L[0] == '+') {
            with_qual = true;
            have = next_line(L);
            while (have && q < slen) {
                if (QUAL && keep) qual->quals.append(L.substr(0, std::min(L.size(), slen - q)));
                q += L.size();
                have = next_line(L);
            }
        }
        out.off.push_back(out.bases.size());
        if (QUAL) {
            qual->quals.resize(out.bases.size(), with_qual ? '\0' : '!');
            qual->has_qual.push_back(with_qual);
            qual->qual_len.push_back(q);
        }
    }
}

namespace pol {

// What the quality strings of a read file say, in the header's order: the first record that breaks a rule (the call is
// refused), reads_with_qual, and per record "this read is low" (its mean Phred below min_avg_qual; empty when the test is off).
struct QualFacts {
    int64_t bad_rec = -1;            // -1: every record is fine
    int bad_kind = 0;                // 1: the quality string is not as long as the bases; 2: a byte outside 33..126
    uint64_t bad_at = 0;             // kind 2: 0-based index inside the record
    uint8_t bad_byte = 0;
    uint64_t reads_with_qual = 0, reads_low = 0;
    std::vector<uint8_t> low;
};

inline QualFacts quality_facts(const SeqSet &s, const SeqQual &q, double min_avg_qual) {
    QualFacts f;
    const bool floor_on = min_avg_qual != 0.0;
    if (floor_on) f.low.assign(s.size(), 0);
    for (size_t i = 0; i < s.size(); ++i) {
        if (!q.has_qual[i]) continue;
        ++f.reads_with_qual;
        const uint64_t n = s.off[i + 1] - s.off[i];
        if (q.qual_len[i] != n) { f.bad_rec = (int64_t)i; f.bad_kind = 1; return f; }
        uint64_t sum = 0;
        for (uint64_t k = 0; k < n; ++k) {
            const uint8_t b = (uint8_t)q.quals[s.off[i] + k];
            if (b < 33 || b > 126) { f.bad_rec = (int64_t)i; f.bad_kind = 2; f.bad_at = k; f.bad_byte = b; return f; }
            sum += (uint64_t)(b - 33);
        }
        if (floor_on && n && (double)sum / (double)n < min_avg_qual) { f.low[i] = 1; ++f.reads_low; }
    }
    return f;
}

// the weight sums are 32 bits wide and a vote weighs 93 at the most: rows_selected x 93 must stay below 2^32
constexpr uint64_t QUAL_WEIGHT_MAX = 93;
inline bool weight_sums_fit(uint64_t rows_selected) { return rows_selected * QUAL_WEIGHT_MAX < (1ull << 32); }

}  // namespace pol
}  // namespace hlmi
