// paf_io.h - host-side text I/O for the path: PAF parsing, FASTA/FASTQ reading, final row
// formatting and the GNU-sort orders the reference pipes its text through.
#pragma once
#include <functional>
#include <string>
#include <string_view>
#include <vector>

#include "common.h"
#include "row_score.h"
#include "seq_scan.h"

namespace hlmi {

// Name dictionary: equal names <=> equal ids (the reference compares qseqid == sseqid as
// strings and keys its dicts by "a:b" of the sorted name pair, filter_overlap_slr2.py:88).
struct NameDict {
    std::vector<std::string> names;
    std::unordered_map<std::string, uint32_t> index;
    uint32_t put(std::string_view s);
};

struct PafText {
    std::string data;                 // whole file
    std::vector<size_t> line_off;     // start of each line
    std::vector<uint32_t> line_len;   // length without the newline
    std::vector<PafRec> recs;         // one per line
    std::vector<uint32_t> ops;        // concatenated CIGAR ops of the last field
    NameDict dict;
    std::string_view line(size_t i) const { return std::string_view(data).substr(line_off[i], line_len[i]); }
};

// Reads and parses a PAF file.  Rows need >= 11 tab-separated columns with integer columns
// 2-4 and 7-11 (anything else is HLMI_EINVAL - the reference's int() would raise there).
// chunk is set to 0 and `tie` to the rank of the whole line in byte order (GNU sort's
// last-resort comparison under LC_ALL=C).
void read_paf(const char *path, PafText &out, bool need_tie_rank);

// SeqSet, SeqQual and the record scan (kseq's detection: FASTA '>' / FASTQ '@', multi-line): seq_scan.h
void read_seqs(const char *path, SeqSet &out);
// the same scan, but only the records `want` accepts bring their bases along (the others keep their name and have
// length 0; n_lines is not counted)
void read_seqs_subset(const char *path, const std::function<bool(std::string_view)> *want, SeqSet &out);
// read_seqs, and the quality strings at the bases' offsets with a per-record "has quality" flag (SeqQual, seq_scan.h): the
// polisher's _q calls.  Nothing is refused here: pol::quality_facts judges the strings.
void read_seqs_qual(const char *path, SeqSet &out, SeqQual &qual);

// Final 14-column row of filter_overlap_slr2.py:142-151 (with the trailing TAB); returns
// false when the row is dropped by the identity test `float(score2) < iden` (slr2:146).
// "%.4f" of v, the bytes printf writes, into dst (>= 64 bytes); returns the length (tests/capi/fixed4_check.cpp)
size_t format_fixed4(double v, char *dst);
// sort_key (optional): column 12 as an integer (value x 10^4) for sort_scored_lines, 0xffffffff when it is not plain digits
// below SCORE_KEY_LIMIT (row_score.h).
bool format_scored_row(const PafRec &r, const std::string &qname, const std::string &tname,
                       uint32_t x_digit_sum, double iden, std::string &out, uint32_t *sort_key = nullptr);

// `sort -k12 -nr` (utils.py:54,69): numeric descending on column 12, ties by reversed
// whole-line byte order.  Lines carry no newline.
void sort_scored_lines(std::vector<std::string> &lines);
// the same on views into text the caller keeps alive (the stage formats its rows into a few large buffers: one
// allocation per thread instead of one per line)
// (keys: the sort_key of every line, from format_scored_row - spares the parse of column 12)
void sort_scored_lines(std::vector<std::string_view> &lines, const std::vector<uint32_t> *keys = nullptr);

void write_lines(const char *path, const std::vector<std::string> &lines);
void write_lines(const char *path, const std::vector<std::string_view> &lines);
std::string read_file(const char *path);
// the whole of data[0, n) into path as fopen's `mode` opens it ("ab": appended); HLMI_EIO when it cannot be opened or written
void write_file(const std::string &path, const char *data, size_t n, const char *mode = "wb");
std::string join_path(const char *dir, const char *name);      // dir + '/' + name (no second '/' behind one)
double now_ms();                                               // steady clock, for the ms_* fields of the stats

}  // namespace hlmi
