// haplotigs_text.h - the host half of hlmi_haplotigs / hlmi_haplotigs_reads (include/hylight_mi.h) that is text and arithmetic: a
// row's side in a block, which blocks are split and their extents, who takes part where, the number of positions two sides
// decided differently, the lines of the blocks file and a haplotig's header.  Host-only and free of any HIP include, as
// phase_text.h is: tests/capi/haplotigs_host_check.cpp compiles it with the plain host compiler under the sanitizers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "phase_text.h"

namespace hlmi {
namespace hap {

enum : uint8_t { SIDE_A = 0, SIDE_B = 1, SIDE_NONE = 2 };
// rule 1: a row's side in a block is hap_of(a, b) of its record
inline uint8_t side_of(const ph::ReadRec &r) {
    const char h = ph::hap_of(r.a, r.b);
    return h == 'A' ? (uint8_t)SIDE_A : h == 'B' ? (uint8_t)SIDE_B : (uint8_t)SIDE_NONE;
}

// A block of two or more sites.  block: its index among all blocks of the call (ReadRec::block); first / last: its extent in the
// contig's own positions (0-based, both ends included), gfirst / glast the same in the device's position space
struct HBlock {
    uint32_t block, contig, n_sites, first, last, gfirst, glast;
    uint64_t rows_a = 0, rows_b = 0, diff = 0;
    bool split = false;
};

// rule 2: the blocks of two or more sites in order, the sides of their records counted, split iff both reach min_side.
// A record of a block that does not exist: -> false.
inline bool haplotig_blocks(const std::vector<ph::PSite> &sites, const ph::Blocks &B, const std::vector<ph::ReadRec> &recs, int min_side,
                            std::vector<HBlock> &out) {
    out.clear();
    const size_t nb = B.first.size();
    std::vector<uint64_t> na(nb, 0), nb_(nb, 0);
    for (const ph::ReadRec &r : recs) {
        if (r.block >= nb) return false;
        const uint8_t s = side_of(r);
        if (s == SIDE_A) ++na[r.block];
        else if (s == SIDE_B) ++nb_[r.block];
    }
    for (size_t b = 0; b < nb; ++b) {
        const size_t s0 = B.first[b], s1 = b + 1 < nb ? B.first[b + 1] : sites.size();
        if (s0 >= sites.size() || s1 > sites.size() || s1 < s0 + 2) continue;
        HBlock h;
        h.block = (uint32_t)b;
        h.contig = sites[s0].contig;
        h.n_sites = (uint32_t)(s1 - s0);
        h.first = sites[s0].pos;
        h.last = sites[s1 - 1].pos;
        h.gfirst = sites[s0].gpos;
        h.glast = sites[s1 - 1].gpos;
        h.rows_a = na[b];
        h.rows_b = nb_[b];
        h.split = min_side >= 1 && na[b] >= (uint64_t)min_side && nb_[b] >= (uint64_t)min_side;
        out.push_back(h);
    }
    return true;
}

// rule 2: position p lies inside [first, last]; slot p - the gap in front of position p - iff first < p <= last
inline bool position_inside(uint32_t first, uint32_t last, uint32_t p) { return first <= p && p <= last; }
inline bool slot_inside(uint32_t first, uint32_t last, uint32_t p) { return first < p && p <= last; }

// rule 6: the positions of [gfirst, glast] whose decision bytes differ between the two sides (side B lies n positions behind A)
inline uint64_t diff_positions(const std::vector<uint8_t> &sym, size_t n, uint32_t gfirst, uint32_t glast) {
    uint64_t d = 0;
    for (size_t g = gfirst; g <= glast && g < n && n + g < sym.size(); ++g) d += sym[g] != sym[n + g];
    return d;
}

inline std::vector<std::string> haplotig_block_lines(const std::vector<std::string> &names, const std::vector<HBlock> &blocks) {
    std::vector<std::string> lines;
    lines.reserve(blocks.size() + 1);
    lines.push_back("#contig\tblock\tstart\tend\tsites\trows_a\trows_b\tsplit\tdiff_positions");
    for (const HBlock &h : blocks) {
        char buf[192];
        snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%u\t%llu\t%llu\t%d\t%llu", (unsigned long long)h.first + 1, (unsigned long long)h.first + 1,
                 (unsigned long long)h.last + 1, h.n_sites, (unsigned long long)h.rows_a, (unsigned long long)h.rows_b, h.split ? 1 : 0,
                 (unsigned long long)(h.split ? h.diff : 0));
        lines.push_back(names[h.contig] + buf);
    }
    return lines;
}

// rule 5: ">name_hapA LN:i: RC:i: XC:f: HB:i: HP:i:" (side 'A' or 'B'); side 0: hlmi_polish's header, ">name LN:i: RC:i: XC:f:"
inline std::string haplotig_head(const std::string &name, char side, uint64_t new_len, uint32_t rc, uint64_t covered, uint64_t len,
                                 uint64_t n_split, uint64_t positions) {
    char head[96], tail[64] = "";
    snprintf(head, sizeof head, " LN:i:%llu RC:i:%u XC:f:%.6f", (unsigned long long)new_len, rc, (double)covered / (double)len);
    if (side) snprintf(tail, sizeof tail, " HB:i:%llu HP:i:%llu", (unsigned long long)n_split, (unsigned long long)positions);
    return ">" + name + (side ? std::string("_hap") + side : std::string()) + head + tail;
}

}  // namespace hap
}  // namespace hlmi
