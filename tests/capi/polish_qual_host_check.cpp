// Stand-alone check of hylight_amd/csrc/seq_scan.h: the sequence reader that keeps the quality strings (read_seqs_qual's scan) and
// what hlmi_polish_q does with them before it looks at a row - validation, reads_with_qual, the mean, the read floor - and the
// refusal of rows_selected x 93 >= 2^32.  Host compiler only, no GPU, no Python, meant for the host sanitizers too:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/capi/polish_qual_host_check.cpp
//       -o polish_qual_host_check
//   ./polish_qual_host_check
// Every case is a small file's text with its answers written out by hand.  `--facts` prints, per case, the text (hex), the floor
// and the facts found, one line each: tests/test_polish_qual_surface.py runs tests/polish_qual_model.py on the same texts.
// Exit status 0 when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hylight_amd/csrc/seq_scan.h"

using namespace hlmi;
using namespace hlmi::pol;

struct Case {
    const char *name;
    std::string text;
    double floor;
    // the answers
    std::vector<std::string> names, bases, quals;   // quals: what SeqQual holds per record
    std::string has;                                // per record '1' / '0'
    std::vector<uint64_t> qlen;
    int64_t bad_rec;
    int bad_kind;
    uint64_t with_qual;
    std::string low;                                // per record '1' / '0'; "-": the test is off or the file is refused
};

static int failures = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) { ++failures; printf("FAILED %s: ", c.name); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static std::string hex(const std::string &s) {
    std::string o;
    char b[3];
    for (unsigned char ch : s) { snprintf(b, sizeof b, "%02x", ch); o += b; }
    return o;
}

static std::string bits(const std::vector<uint8_t> &v) {
    std::string s;
    for (uint8_t x : v) s += x ? '1' : '0';
    return s;
}

int main(int argc, char **argv) {
    const bool print_facts = argc > 1 && !strcmp(argv[1], "--facts");
    std::vector<Case> cases = {
        {"multi_line", "@r1 first read\nACGT\nAC\n+\nIIII\n5I\n@r2\tx\nGG\n+\n!~\n", 0.0,
         {"r1", "r2"}, {"ACGTAC", "GG"}, {"IIII5I", "!~"}, "11", {6, 2}, -1, 0, 2, "-"},
        {"crlf", "@a\r\nACGT\r\n+\r\nI#I#\r\n>f\r\nAC\r\n", 10.0,
         {"a", "f"}, {"ACGT", "AC"}, {"I#I#", "!!"}, "10", {4, 0}, -1, 0, 1, "00"},
        {"plus_name_line", "@a\nACGT\n+a some words\n&&&&\n", 6.0,
         {"a"}, {"ACGT"}, {"&&&&"}, "1", {4}, -1, 0, 1, "1"},
        {"quality_begins_with_at_or_gt", "@a\nACGT\n+\n@III\n@b\nAC\nG\n+\n>\nII\n", 0.0,
         {"a", "b"}, {"ACGT", "ACG"}, {"@III", ">II"}, "11", {4, 3}, -1, 0, 2, "-"},
        {"truncated_then_header_eaten", "@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", 0.0,
         {"a"}, {"ACGT"}, {"III@"}, "1", {5}, 0, 1, 1, "-"},
        {"truncated_at_end_of_file", "@a\nAC\n+\nII\n@b\nACGT\n+\nII\n", 0.0,
         {"a", "b"}, {"AC", "ACGT"}, {"II", std::string("II") + std::string(2, '\0')}, "11", {2, 2}, 1, 1, 2, "-"},
        {"byte_32", "@a\nACG\n+\nI I\n", 0.0, {"a"}, {"ACG"}, {"I I"}, "1", {3}, 0, 2, 1, "-"},
        {"byte_127", "@a\nAC\n+\nII\n@b\nACG\n+\nII\x7f\n", 0.0, {"a", "b"}, {"AC", "ACG"}, {"II", "II\x7f"}, "11", {2, 3}, 1, 2, 2, "-"},
        {"fasta_between_fastq", "@a\nAC\n+\nII\n>f\nACGT\n@b\nGG\n+\n##\n", 10.0,
         {"a", "f", "b"}, {"AC", "ACGT", "GG"}, {"II", "!!!!", "##"}, "101", {2, 0, 2}, -1, 0, 2, "001"},
        {"at_record_without_plus", "@a\nACGT\n>f\nAC\n", 10.0, {"a", "f"}, {"ACGT", "AC"}, {"!!!!", "!!"}, "00", {0, 0}, -1, 0, 0, "00"},
        // ten bases whose Phred values add up to 103: kept at a floor of exactly 103 / 10, dropped one step above it
        {"mean_exactly_the_floor", "@a\nACGTACGTAC\n+\n+++++++++.\n", 103.0 / 10.0,
         {"a"}, {"ACGTACGTAC"}, {"+++++++++."}, "1", {10}, -1, 0, 1, "0"},
        {"mean_one_step_below_the_floor", "@a\nACGTACGTAC\n+\n+++++++++.\n", std::nextafter(103.0 / 10.0, 100.0),
         {"a"}, {"ACGTACGTAC"}, {"+++++++++."}, "1", {10}, -1, 0, 1, "1"},
        {"empty_record_is_never_low", "@a\n+\n@b\nA\n+\n\"\n", 5.0, {"a", "b"}, {"", "A"}, {"", "\""}, "11", {0, 1}, -1, 0, 2, "01"},
    };
    for (const Case &c : cases) {
        SeqSet s;
        SeqQual q;
        scan_seq_records<true>(c.text, nullptr, s, &q);
        SeqSet plain;                                        // the scan every other caller uses sees the same records
        scan_seq_records<false>(c.text, nullptr, plain, nullptr);
        CHECK(plain.names == s.names && plain.bases == s.bases && plain.off == s.off, "the two scans differ");
        CHECK(s.names == c.names, "names");
        CHECK(s.size() == c.bases.size() && s.off.size() == s.size() + 1 && q.quals.size() == s.bases.size(), "sizes");
        CHECK(bits(q.has_qual) == c.has, "has_qual %s", bits(q.has_qual).c_str());
        CHECK(q.qual_len == c.qlen, "qual_len");
        for (size_t i = 0; i < s.size() && i < c.bases.size(); ++i) {
            CHECK(s.bases.substr(s.off[i], s.len(i)) == c.bases[i], "bases of record %zu", i);
            CHECK(q.quals.substr(s.off[i], s.len(i)) == c.quals[i], "quals of record %zu: %s", i, hex(q.quals.substr(s.off[i], s.len(i))).c_str());
        }
        const QualFacts f = quality_facts(s, q, c.floor);
        CHECK(f.bad_rec == c.bad_rec && f.bad_kind == c.bad_kind, "bad record %lld kind %d", (long long)f.bad_rec, f.bad_kind);
        const std::string low = f.bad_rec >= 0 || c.floor == 0.0 ? "-" : bits(f.low);
        if (f.bad_rec < 0) CHECK(f.reads_with_qual == c.with_qual, "reads_with_qual %llu", (unsigned long long)f.reads_with_qual);
        CHECK(low == c.low, "low %s", low.c_str());
        if (print_facts) {
            std::string names;
            for (const std::string &n : s.names) names += (names.empty() ? "" : ",") + n;
            printf("%s\t%s\t%a\tbad=%lld;kind=%d;with=%llu;low=%s;has=%s;names=%s;quals=%s\n", c.name, hex(c.text).c_str(), c.floor,
                   (long long)f.bad_rec, f.bad_kind, f.bad_rec < 0 ? (unsigned long long)f.reads_with_qual : 0ull, low.c_str(),
                   bits(q.has_qual).c_str(), names.c_str(), f.bad_rec < 0 ? hex(q.quals).c_str() : "-");
        }
    }
    // byte 32 and 127: where, and which
    {
        SeqSet s;
        SeqQual q;
        scan_seq_records<true>(std::string("@a\nACG\n+\nI I\n"), nullptr, s, &q);
        const QualFacts f = quality_facts(s, q, 0.0);
        if (f.bad_at != 1 || f.bad_byte != 32) { ++failures; printf("FAILED byte 32: at %llu byte %u\n", (unsigned long long)f.bad_at, f.bad_byte); }
    }
    // the 32-bit weight sums: 46 182 444 x 93 = 4 294 967 292 is the last product below 2^32
    if (!weight_sums_fit(0) || !weight_sums_fit(706) || !weight_sums_fit(46182444ull) || weight_sums_fit(46182445ull) ||
        weight_sums_fit(1ull << 32)) {
        ++failures;
        printf("FAILED weight_sums_fit\n");
    }
    if (failures) return 1;
    printf("polish_qual_host_check: ok (%zu cases)\n", cases.size());
    return 0;
}
