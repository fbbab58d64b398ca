// dev_search.h - binary search in a sorted device array, one definition for ava_chain.hip, graph_dev.hip and filter_stage.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hlmi {
// the first position of the ascending a[0, n) whose value is not below v (n: none)
__device__ __forceinline__ size_t lower_bound_u64(const uint64_t *a, size_t n, uint64_t v) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t m = (lo + hi) >> 1;
        if (a[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}
}  // namespace hlmi
