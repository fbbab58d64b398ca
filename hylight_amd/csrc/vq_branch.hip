// vq_branch.hip - the device side of BranchReduction::readBasedBranchReduction (tools/HaploConduct/src/BranchReduction.cpp;
// the host side and the contract are in vq_branch_host.cpp): the two base-comparison steps, over reads and original reads that
// are resident, bases concatenated as VqMergeDev lays them out.  Reverse complements are made on the fly.
//   diff_kernel       findDiffPos (:693-713) of every compared neighbour pair of a branch: one wave per pair, 64 bases a step
//   evidence_kernel   the look-ups and checkReadEvidence (:264-321, :716-743) of every (branch, neighbour, original): one thread
//                     per triple (DESIGN.md 4.3g says why not a wave)
#include <hip/hip_runtime.h>

#include "vq_internal.h"

namespace hlmi {
namespace vqb {
namespace {

// base `i` of read r as the branch sees it: reverse-complemented when rc
__device__ __forceinline__ uint8_t oriented(const uint8_t *bases, uint64_t off, uint32_t len, uint32_t i, bool rc) {
    return rc ? vqm::complement(bases[off + (len - 1 - i)]) : bases[off + i];
}

// One wave per pair.  Compare position p (0 .. len - 1) is base rel + p of a against base p of b, or with flag 2 (an in-branch:
// the reference reverses both stretches, :609-610) base rel + len - 1 - p against base len - 1 - p.  The wave appends the
// mismatching p in ascending order - ballot, then each lane's rank among the set bits below it - and stops behind the step that
// holds the 100th.  Loop bound: ceil(len / 64) steps.
__global__ __launch_bounds__(WG) void diff_kernel(const Pair *pairs, uint32_t n_pairs, const uint8_t *bases, const uint64_t *off,
                                                  uint32_t *cnt, uint32_t *pos) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t waves = gridDim.x * (WG / WAVE);
    for (uint32_t p = blockIdx.x * (WG / WAVE) + threadIdx.x / WAVE; p < n_pairs; p += waves) {
        const Pair pr = pairs[p];
        const uint64_t oa = off[pr.a], ob = off[pr.b];
        const uint32_t la = (uint32_t)(off[pr.a + 1] - oa), lb = (uint32_t)(off[pr.b + 1] - ob);
        const bool rc = pr.flags & 1, reversed = pr.flags & 2;
        uint32_t found = 0;
        for (uint32_t s = 0; s < pr.len && found < MAX_DIFF; s += WAVE) {
            const uint32_t q = s + lane;
            bool differ = false;
            if (q < pr.len) {
                const uint32_t x = reversed ? pr.len - 1 - q : q;
                differ = oriented(bases, oa, la, pr.rel + x, rc) != oriented(bases, ob, lb, x, rc);
            }
            const uint64_t mask = __ballot(differ);
            const uint32_t rank = found + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
            if (differ && rank < MAX_DIFF) pos[(size_t)p * MAX_DIFF + rank] = q;
            found += (uint32_t)__popcll(mask);
        }
        if (lane == 0) cnt[p] = found < MAX_DIFF ? found : MAX_DIFF;
    }
}

// whether the ascending ids[b, e) hold id; at most SEARCH_STEPS steps
__device__ __forceinline__ bool holds(const uint32_t *ids, uint32_t b, uint32_t e, uint32_t id) {
    uint32_t lo = b, hi = e;
    for (int step = 0; step < SEARCH_STEPS && lo < hi; ++step) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < e && ids[lo] == id;
}

// One thread per item t = (slot, original of the slot's neighbour).  The slot is found by binary search in item0; the id and,
// under the SE / PE rule of :270-284, its mate's id in the branching vertex's originals.  On a hit the original read - reverse-
// complemented when !forward, at startpos + index1, which may be negative - is tested against the contig at the positions of the
// branch's difference list both cover: a search for the first one, then at most diff1 - diff0 turns.  The mate branch tests the
// subread itself again (:306), so one test serves both ids.
__global__ __launch_bounds__(WG) void evidence_kernel(const Slot *slots, uint32_t n_slots, const uint32_t *item0, uint32_t n_items,
                                                      const int32_t *diff, const uint32_t *ooff, const uint32_t *oid,
                                                      const uint32_t *orow, const uint8_t *ofwd, const int32_t *oidx,
                                                      const uint8_t *rbases, const uint64_t *roff, const uint8_t *obases,
                                                      const uint64_t *obase_off, uint32_t se, uint32_t pe, uint32_t readcount,
                                                      uint32_t *ev) {
    const uint32_t t = blockIdx.x * WG + threadIdx.x;
    if (t >= n_items) return;
    uint32_t lo = 0, hi = n_slots;                    // the last slot whose first item is <= t
    for (int step = 0; step < SEARCH_STEPS && hi - lo > 1; ++step) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (item0[mid] <= t) lo = mid; else hi = mid;
    }
    const Slot sl = slots[lo];
    const uint32_t e = ooff[sl.nb] + (t - item0[lo]);
    const uint32_t sid = oid[e];
    const uint32_t b1 = ooff[sl.node], e1 = ooff[sl.node + 1];
    const bool hit = holds(oid, b1, e1, sid);
    bool has_mate = false, hit_mate = false;
    uint32_t mate = 0;
    if (sid >= se + pe) { mate = sid - pe; has_mate = true; }
    else if (sid >= se) { mate = sid + pe; has_mate = true; }
    if (has_mate) hit_mate = holds(oid, b1, e1, mate);
    uint32_t out0 = NONE, out1 = NONE;
    if (hit || hit_mate) {
        const uint32_t row = orow[e];
        const uint64_t ro = obase_off[row];
        const uint32_t rlen = (uint32_t)(obase_off[row + 1] - ro);
        const uint64_t co = roff[sl.nb];
        const uint32_t clen = (uint32_t)(roff[sl.nb + 1] - co);
        const int64_t read_start = (int64_t)sl.startpos + oidx[e], read_end = read_start + rlen;
        const int64_t contig_start = sl.startpos, contig_end = contig_start + clen;
        const int64_t from = read_start > contig_start ? read_start : contig_start;
        const int64_t to = read_end < contig_end ? read_end : contig_end;
        uint32_t a = sl.diff0, z = sl.diff1;          // the first listed position >= from
        for (int step = 0; step < SEARCH_STEPS && a < z; ++step) {
            const uint32_t mid = a + ((z - a) >> 1);
            if ((int64_t)diff[mid] < from) a = mid + 1; else z = mid;
        }
        bool covered = false, agree = true;
        for (uint32_t k = a; k < sl.diff1 && agree; ++k) {
            const int64_t d = diff[k];
            if (d >= to) break;
            covered = true;
            const uint8_t r = oriented(obases, ro, rlen, (uint32_t)(d - read_start), !ofwd[e]);
            const uint8_t c = oriented(rbases, co, clen, (uint32_t)(d - contig_start), sl.rc != 0);
            agree = r == c;
        }
        if (covered && agree) {
            if (hit) out0 = sid;
            if (hit_mate) out1 = readcount + (sid < mate ? sid : mate);
        }
    }
    ev[2 * (size_t)t] = out0;
    ev[2 * (size_t)t + 1] = out1;
}

void concat(const std::vector<std::string> &seq, DBuf<uint8_t> &d_bases, DBuf<uint64_t> &d_off) {
    std::vector<uint64_t> off(seq.size() + 1, 0);
    for (size_t r = 0; r < seq.size(); ++r) off[r + 1] = off[r] + seq[r].size();
    std::vector<uint8_t> bases(off.back());
    for (size_t r = 0; r < seq.size(); ++r) memcpy(bases.data() + off[r], seq[r].data(), seq[r].size());
    d_bases.upload(bases);
    d_off.upload(off);
    sync();                                           // the host vectors go out of scope
}

}  // namespace

Dev::Dev(const std::vector<std::string> &reads, const std::vector<std::string> &originals) {
    concat(reads, d_reads_, d_roff_);
    concat(originals, d_orig_, d_ooff_);
}

void Dev::diff_positions(const std::vector<Pair> &pairs, std::vector<uint32_t> &cnt, std::vector<uint32_t> &pos) {
    cnt.clear();
    pos.clear();
    if (pairs.empty()) return;
    if (pairs.size() >= (1u << 25)) fail(HLMI_EINVAL, "vq_branch: %zu neighbour pairs", pairs.size());
    DBuf<Pair> d_pairs;
    d_pairs.upload(pairs);
    DBuf<uint32_t> d_cnt(pairs.size()), d_pos(pairs.size() * MAX_DIFF);
    {
        KTimer kt("vq_branch_diff");
        hipLaunchKernelGGL(diff_kernel, dim3(vqk::waves_grid(pairs.size())), dim3(WG), 0, stream(), d_pairs.p, (uint32_t)pairs.size(),
                           d_reads_.p, d_roff_.p, d_cnt.p, d_pos.p);
    }
    HIP_CHECK(hipGetLastError());
    cnt = d_cnt.download(pairs.size());
    pos = d_pos.download(pairs.size() * MAX_DIFF);    // (entries past cnt[p] are not written and not read)
}

void Dev::evidence(const std::vector<Slot> &slots, const std::vector<uint32_t> &item0, const std::vector<int32_t> &diff,
                   const std::vector<uint32_t> &ooff, const std::vector<uint32_t> &oid, const std::vector<uint32_t> &orow,
                   const std::vector<uint8_t> &ofwd, const std::vector<int32_t> &oidx, uint32_t se_count, uint32_t pe_count,
                   std::vector<uint32_t> &ev) {
    ev.clear();
    const size_t n_items = item0.empty() ? 0 : item0.back();
    if (!n_items) return;
    if (n_items >= (1u << 31)) fail(HLMI_EINVAL, "vq_branch: %zu evidence items", n_items);
    DBuf<Slot> d_slots;
    DBuf<uint32_t> d_item0, d_ooff, d_oid, d_orow, d_ev(2 * n_items);
    DBuf<int32_t> d_diff(std::max<size_t>(diff.size(), 1)), d_oidx;
    DBuf<uint8_t> d_ofwd;
    d_slots.upload(slots);
    d_item0.upload(item0);
    d_diff.upload(diff.data(), diff.size());
    d_ooff.upload(ooff);
    d_oid.upload(oid);
    d_orow.upload(orow);
    d_ofwd.upload(ofwd);
    d_oidx.upload(oidx);
    {
        KTimer kt("vq_branch_evidence");
        hipLaunchKernelGGL(evidence_kernel, dim3(cdiv(n_items, (size_t)WG)), dim3(WG), 0, stream(), d_slots.p, (uint32_t)slots.size(),
                           d_item0.p, (uint32_t)n_items, d_diff.p, d_ooff.p, d_oid.p, d_orow.p, d_ofwd.p, d_oidx.p, d_reads_.p, d_roff_.p,
                           d_orig_.p, d_ooff_.p, se_count, pe_count, se_count + 2 * pe_count, d_ev.p);
    }
    HIP_CHECK(hipGetLastError());
    ev = d_ev.download(2 * n_items);
}

}  // namespace vqb
}  // namespace hlmi
