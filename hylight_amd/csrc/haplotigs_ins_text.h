// haplotigs_ins_text.h - the host half of hlmi_haplotigs_ins / hlmi_haplotigs_reads_ins (include/hylight_mi.h) that is text and
// arithmetic: a block's extent in key space (phase_ins_text.h: site_key - slot p has key 2 p, position p key 2 p + 1), the two
// inside tests, the positions an extent holds, the slots two sides opened to different lengths and the ten-column lines of the
// blocks file with their `+` marks.  The split rule and the nine columns are haplotigs_text.h's, the merged list and mark_field
// phase_ins_text.h's, called and not restated.  Host-only and free of any HIP include, as they are:
// tests/capi/haplotigs_ins_host_check.cpp compiles it with the plain host compiler under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "haplotigs_text.h"
#include "phase_ins_text.h"

namespace hlmi {
namespace hap {

// position p lies inside the extent [kf, kl] of keys iff its key does; slot p - the gap in front of position p - likewise.  With
// both ends at positions (odd keys) these are haplotigs_text.h's position_inside and slot_inside
inline bool key_position_inside(uint32_t kf, uint32_t kl, uint32_t p) { return kf <= 2ull * p + 1 && 2ull * p + 1 <= kl; }
inline bool key_slot_inside(uint32_t kf, uint32_t kl, uint32_t p) { return kf <= 2ull * p && 2ull * p <= kl; }
// the first and the last position inside, and their number: an extent holds a position (kf < kl, or kf == kl odd)
inline uint32_t key_first_position(uint32_t kf) { return kf >> 1; }
inline uint32_t key_last_position(uint32_t kl) { return (kl - 1) >> 1; }
inline uint64_t key_positions(uint32_t kf, uint32_t kl) { return (uint64_t)key_last_position(kl) - key_first_position(kf) + 1; }

// A block of haplotig_blocks over the merged list with its extent in the device's key space: h.first / h.last are the printed
// positions minus one of its first and last site (at slot p: p - 1, the anchor), h.gfirst / h.glast those sites' gpos
struct KBlock {
    HBlock h;
    uint32_t kf = 0, kl = 0;
    bool first_slot = false, last_slot = false;
    uint64_t diff_slots = 0;
};

// haplotig_blocks over M.sites, then every block's keys.  A record of a block that does not exist, a list whose keys do not
// ascend inside a block or an extent without a position: -> false
inline bool key_blocks(const ph::MergedSites &M, const ph::Blocks &B, const std::vector<ph::ReadRec> &recs, int min_side, std::vector<KBlock> &out) {
    out.clear();
    std::vector<HBlock> hb;
    if (M.key.size() != M.sites.size() || M.ins_of.size() != M.sites.size() || !haplotig_blocks(M.sites, B, recs, min_side, hb)) return false;
    for (const HBlock &h : hb) {
        const size_t s0 = B.first[h.block], s1 = s0 + h.n_sites - 1;
        if (s1 >= M.sites.size()) return false;
        KBlock k;
        k.h = h;
        k.kf = M.key[s0];
        k.kl = M.key[s1];
        k.first_slot = M.slot(s0);
        k.last_slot = M.slot(s1);
        if (k.kf >= k.kl || (!out.empty() && out.back().kl >= k.kf)) return false;
        out.push_back(k);
    }
    return true;
}

// the slots inside [kf, kl] (device key space) that the two sides opened to different lengths; a shut slot has length 0.
// open_pos (ascending) / open_len: PolDevOut's over the two sides side by side, side B's positions n behind side A's
inline uint64_t diff_slots(const std::vector<uint32_t> &open_pos, const std::vector<uint8_t> &open_len, size_t n, uint32_t kf, uint32_t kl) {
    if (open_len.size() != open_pos.size()) return 0;
    const uint64_t g0 = ((uint64_t)kf + 1) >> 1, g1 = (uint64_t)(kl >> 1) + 1;      // the slots [g0, g1)
    if (g0 >= g1) return 0;
    auto a = std::lower_bound(open_pos.begin(), open_pos.end(), g0), a1 = std::lower_bound(a, open_pos.end(), g1);
    auto b = std::lower_bound(a1, open_pos.end(), n + g0), b1 = std::lower_bound(b, open_pos.end(), n + g1);
    uint64_t d = 0;
    while (a != a1 || b != b1) {
        const uint64_t pa = a != a1 ? *a : UINT64_MAX, pb = b != b1 ? *b - n : UINT64_MAX;
        if (pa == pb) {
            d += open_len[a - open_pos.begin()] != open_len[b - open_pos.begin()];
            ++a;
            ++b;
        } else {
            d += open_len[(pa < pb ? a : b) - open_pos.begin()] != 0;
            ++(pa < pb ? a : b);
        }
    }
    return d;
}

// the blocks file: haplotig_block_lines's nine columns, `+` behind block and start where the first site is an insertion site,
// behind end where the last one is, and diff_slots as the tenth
inline std::vector<std::string> haplotig_ins_block_lines(const std::vector<std::string> &names, const std::vector<KBlock> &blocks) {
    std::vector<HBlock> hb;
    hb.reserve(blocks.size());
    for (const KBlock &k : blocks) hb.push_back(k.h);
    std::vector<std::string> lines = haplotig_block_lines(names, hb);
    if (lines.size() != blocks.size() + 1) return lines;                        // (never)
    lines[0] += "\tdiff_slots";
    for (size_t i = 0; i < blocks.size(); ++i) {
        const KBlock &k = blocks[i];
        std::string &line = lines[i + 1];
        if (k.last_slot) ph::mark_field(line, 3);
        if (k.first_slot) {
            ph::mark_field(line, 2);
            ph::mark_field(line, 1);
        }
        line += "\t" + std::to_string(k.h.split ? k.diff_slots : 0);
    }
    return lines;
}

}  // namespace hap
}  // namespace hlmi
