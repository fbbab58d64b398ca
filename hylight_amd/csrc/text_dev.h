// text_dev.h - the text kernels graph_dev.hip (PAF -> overlap graph) shares with cluster.hip (short-read clustering):
// line starts, and the name hash / byte compare of its "hash, stable group, compare neighbours" name tables.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace hlmi {

// flags of the window txt[base .. base + n): 1 where a line starts
__global__ void line_start_kernel(const uint8_t *txt, size_t base, size_t n, uint8_t *flag);

// 64-bit hash of the name txt[off .. off + len) under `seed` (a caller that finds two different names with one hash
// starts over with another seed)
__device__ __forceinline__ uint64_t name_hash64(const uint8_t *txt, uint64_t off, uint32_t len, uint64_t seed) {
    uint64_t h = seed ^ (0x9e3779b97f4a7c15ull * (len + 1));
    for (uint32_t i = 0; i < len; ++i) {
        h = (h ^ txt[off + i]) * 0x100000001b3ull;
        h ^= h >> 29;
    }
    h ^= h >> 32;
    return h * 0xd6e8feb86659fd93ull;
}

__device__ __forceinline__ bool bytes_equal(const uint8_t *s1, uint64_t o1, uint32_t l1, const uint8_t *s2, uint64_t o2,
                                            uint32_t l2) {
    bool same = l1 == l2;
    for (uint32_t k = 0; same && k < l1; ++k) same = s1[o1 + k] == s2[o2 + k];
    return same;
}

}  // namespace hlmi
