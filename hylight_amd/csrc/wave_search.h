// wave_search.h - membership of one key in a sorted array of distinct 64-bit keys, searched by a whole wave: the 64 lanes read
// 64 evenly spaced pivots of the range, one ballot says between which two the key lies, and the range shrinks to one step.
// ceil(log64 n) dependent loads and one more where a thread's lower_bound (dev_search.h) takes log2 n.  Used by pr_facts_kernel
// (polish_rows.hip) for the pair list of hlmi_polish_reads_pairs: a wave works on one row, so the key is the same in every lane.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace hlmi {

constexpr int WAVE_SEARCH_ROUNDS = 6;           // 64^6 = 2^36 keys; a range shrinks by a factor of 64 a round

// All 64 lanes of the wave call this together with the same arguments (the ballots count every lane).
__device__ __forceinline__ bool wave_contains_u64(const uint64_t *__restrict__ keys, size_t n, uint64_t key) {
    const size_t lane = threadIdx.x & 63;
    size_t lo = 0, hi = n;                      // the key, if present, lies in keys[lo, hi)
    bool found = false;
    for (int round = 0; round < WAVE_SEARCH_ROUNDS; ++round) {
        const size_t size = hi - lo;
        if (size == 0) break;
        const size_t step = (size + 63) / 64;   // 1: every key of the range is a pivot, and this round answers
        const size_t at = lo + lane * step;
        const bool in = at < hi;
        const uint64_t v = in ? keys[at] : 0;
        const int n_le = __popcll(__ballot(in && v <= key));       // the pivots ascend: the lanes with v <= key are the first n_le
        if (n_le == 0) break;                                       // below the range's first key
        if (step == 1) {
            found = __ballot(in && v == key) != 0;
            break;
        }
        lo += (size_t)(n_le - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return found;
}

}  // namespace hlmi
