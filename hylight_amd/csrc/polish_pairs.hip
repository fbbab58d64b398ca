// polish_pairs.hip - the pair list of hlmi_polish_reads_pairs (include/hylight_mi.h), parsed where the overlapper's rows are: the
// list of the third polishing site has millions of rows, and the fused call exists so that no row crosses to the host.  The text
// goes up as it is; what comes out is the sorted array of distinct keys rank_a << 32 | rank_b that pr_facts_kernel
// (polish_rows.hip) searches with wave_search.h.  The machinery is cluster.hip's (text_dev.h):
//   pp_hash_kernel    a thread per name of the call (the union of read and contig names, AvaPairCall::name_of_rank): its hash;
//                     sorted by hash, pp_check_kernel compares equal neighbours byte for byte (a collision: another seed)
//   pp_row_kernel     a thread per list line: split at TABs, fields 1 and 6 looked up (hash, then bytes); both orders of the pair
//                     as keys, or two sentinels and the unknown counter; a line of fewer than 6 fields leaves its index (atomicMin)
//   pp_head_kernel    behind the sort: 1 where a key is no sentinel and differs from the key in front of it; counts a < b
//   pp_gather_kernel  the flagged keys, in order
// pair_list.h is the same rule on the host (hlmi_polish_pairs); tests/polish_pairs_model.py states it.  Byte work: HBM-bound.
#include <hip/hip_runtime.h>

#include "common.h"
#include "dev_prims.h"
#include "paf_io.h"
#include "polish_internal.h"
#include "text_dev.h"

namespace hlmi {
namespace pol {

namespace {

constexpr int WG = 256;
inline dim3 grid1(size_t n) { return grid_for(n, WG); }
constexpr uint32_t NO_LINE = 0xffffffffu;
constexpr uint32_t NO_RANK = 0xffffffffu;
enum : uint32_t { TAB_DUP = 1u, TAB_COLLISION = 2u };

__global__ __launch_bounds__(WG) void pp_hash_kernel(const uint8_t *__restrict__ names, const uint64_t *__restrict__ off,
                                                     const uint32_t *__restrict__ len, size_t n_names, uint64_t seed,
                                                     uint64_t *__restrict__ hash, uint32_t *__restrict__ rank) {
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= n_names) return;
    hash[k] = name_hash64(names, off[k], len[k], seed);
    rank[k] = (uint32_t)k;
}

__global__ __launch_bounds__(WG) void pp_check_kernel(const uint8_t *__restrict__ names, const uint64_t *__restrict__ off,
                                                      const uint32_t *__restrict__ len, const uint64_t *__restrict__ hash,
                                                      const uint32_t *__restrict__ rank, size_t n_names, uint32_t *__restrict__ bits) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i == 0 || i >= n_names || hash[i] != hash[i - 1]) return;
    const uint32_t u = rank[i - 1], v = rank[i];
    atomicOr(bits, bytes_equal(names, off[u], len[u], names, off[v], len[v]) ? TAB_DUP : TAB_COLLISION);
}

// rank of the name txt[o .. o + l) (NO_RANK: not a name of the call)
__device__ uint32_t pp_lookup(const uint8_t *txt, uint64_t o, uint32_t l, const uint8_t *names, const uint64_t *noff,
                              const uint32_t *nlen, const uint64_t *hash, const uint32_t *rank, size_t n_names, uint64_t seed) {
    const uint64_t h = name_hash64(txt, o, l, seed);
    size_t lo = 0, hi = n_names;
    for (int step = 0; step < 64 && lo < hi; ++step) {       // (a range halves every step)
        const size_t m = lo + (hi - lo) / 2;
        if (hash[m] < h) lo = m + 1;
        else hi = m;
    }
    if (lo >= n_names || hash[lo] != h) return NO_RANK;
    const uint32_t v = rank[lo];
    return bytes_equal(txt, o, l, names, noff[v], nlen[v]) ? v : NO_RANK;
}

// line r = txt[ls[r], ls[r + 1]) without its '\n' (the last line ends at n, with or without one)
__global__ __launch_bounds__(WG) void pp_row_kernel(const uint8_t *__restrict__ txt, size_t n, const uint32_t *__restrict__ ls,
                                                    size_t n_lines, const uint8_t *__restrict__ names, const uint64_t *__restrict__ noff,
                                                    const uint32_t *__restrict__ nlen, const uint64_t *__restrict__ hash,
                                                    const uint32_t *__restrict__ rank, size_t n_names, uint64_t seed, uint64_t sentinel,
                                                    uint64_t *__restrict__ keys, unsigned long long *__restrict__ n_unknown,
                                                    uint32_t *__restrict__ bad_line) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_lines) return;
    const size_t a = ls[r];
    size_t e = r + 1 < n_lines ? (size_t)ls[r + 1] : n;
    if (e > a && txt[e - 1] == '\n') --e;
    uint32_t fields = 1;
    size_t e0 = e, s5 = e, e5 = e;
    for (size_t k = a; k < e; ++k) {
        if (txt[k] != '\t') continue;
        if (fields == 1) e0 = k;
        if (fields == 5) s5 = k + 1;
        if (fields == 6) e5 = k;
        ++fields;
    }
    uint64_t k0 = sentinel, k1 = sentinel;
    if (fields < 6) {
        atomicMin(bad_line, (uint32_t)r);
    } else {
        const uint32_t ra = pp_lookup(txt, a, (uint32_t)(e0 - a), names, noff, nlen, hash, rank, n_names, seed);
        const uint32_t rb = pp_lookup(txt, s5, (uint32_t)(e5 - s5), names, noff, nlen, hash, rank, n_names, seed);
        if (ra == NO_RANK || rb == NO_RANK) {
            atomicAdd(n_unknown, 1ull);
        } else {
            k0 = (uint64_t)ra << 32 | rb;
            k1 = (uint64_t)rb << 32 | ra;
        }
    }
    keys[2 * r] = k0;
    keys[2 * r + 1] = k1;
}

// keys sorted: the sentinels lie behind every key of a pair
__global__ __launch_bounds__(WG) void pp_head_kernel(const uint64_t *__restrict__ keys, size_t n, uint64_t sentinel,
                                                     uint8_t *__restrict__ flag, unsigned long long *__restrict__ n_listed) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    bool head = false, pair = false;
    if (i < n) {
        const uint64_t k = keys[i];
        head = k != sentinel && (i == 0 || keys[i - 1] != k);
        pair = head && (uint32_t)(k >> 32) < (uint32_t)k;
        flag[i] = head ? 1 : 0;
    }
    const int c = __popcll(__ballot(pair));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_listed, (unsigned long long)c);
}

__global__ __launch_bounds__(WG) void pp_gather_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, size_t n,
                                                       uint64_t *__restrict__ out) {
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j < n) out[j] = keys[idx[j]];
}

}  // namespace

void pair_keys_device(const char *who, const std::vector<std::string> &name_of_rank, PolPairCall &pc, PairKeys &out) {
    out.keys.alloc(1);
    out.n = 0;
    pc.pairs_listed = pc.pairs_unknown = 0;
    const std::string text = read_file(pc.path);
    const size_t n = text.size();
    if (n >= (1ull << 31)) fail(HLMI_EINVAL, "%s: %s: a pair list of 2^31 bytes or more", who, pc.path);
    if (!n) return;
    KTimer kt("polish_pairs");
    DBuf<uint8_t> txt, flag(n);
    txt.upload((const uint8_t *)text.data(), n);
    // the host has the bytes: one count of '\n' sizes the line starts (4 bytes a line, not 4 a byte of the list)
    const size_t L = (size_t)std::count(text.begin(), text.end(), '\n') + (text.back() != '\n');
    DBuf<uint32_t> ls(L);
    hipLaunchKernelGGL(line_start_kernel, grid1(n), dim3(WG), 0, stream(), txt.p, (size_t)0, n, flag.p);
    HIP_CHECK(hipGetLastError());
    if (select_flagged_indices(flag.p, ls.p, n) != L) fail(HLMI_EINVAL, "%s: %s: the device counts other lines than the host", who, pc.path);   // (never)
    flag.release();

    // the name table: re-seeded until no two names share a hash
    const size_t N = name_of_rank.size();
    std::string all;
    std::vector<uint64_t> h_off(N);
    std::vector<uint32_t> h_len(N);
    for (size_t k = 0; k < N; ++k) {
        h_off[k] = all.size();
        h_len[k] = (uint32_t)name_of_rank[k].size();
        all += name_of_rank[k];
    }
    DBuf<uint8_t> names(std::max<size_t>(all.size(), 1));
    names.upload((const uint8_t *)all.data(), all.size());
    DBuf<uint64_t> noff(std::max<size_t>(N, 1)), hash(std::max<size_t>(N, 1));
    DBuf<uint32_t> nlen(std::max<size_t>(N, 1)), rank(std::max<size_t>(N, 1)), bits(1);
    noff.upload(h_off);
    nlen.upload(h_len);
    uint64_t seed = 0x243f6a8885a308d3ull;
    for (int tries = 0; N; ++tries, seed += 0x9e3779b97f4a7c15ull) {
        if (tries == 64) fail(HLMI_EINVAL, "%s: no collision-free name table in 64 seeds", who);       // (never)
        hipLaunchKernelGGL(pp_hash_kernel, grid1(N), dim3(WG), 0, stream(), names.p, noff.p, nlen.p, N, seed, hash.p, rank.p);
        sort_pairs_u64_u32(hash.p, rank.p, N);
        bits.zero();
        hipLaunchKernelGGL(pp_check_kernel, grid1(N), dim3(WG), 0, stream(), names.p, noff.p, nlen.p, hash.p, rank.p, N, bits.p);
        HIP_CHECK(hipGetLastError());
        const uint32_t b = download_one(bits.p);
        if (b & TAB_DUP) fail(HLMI_EINVAL, "%s: one name under two ranks", who);                        // (never: the ranks are of distinct names)
        if (!(b & TAB_COLLISION)) break;
    }

    // a key of two ranks is below N << 32 | N: the sentinel sorts behind them all, inside the same bits
    const uint64_t sentinel = (uint64_t)N << 32 | (uint64_t)N;
    DBuf<uint64_t> keys(2 * L);
    DBuf<unsigned long long> counts(2);         // unknown rows, listed pairs
    DBuf<uint32_t> bad(1);
    counts.zero();
    bad.fill_ff();
    hipLaunchKernelGGL(pp_row_kernel, grid1(L), dim3(WG), 0, stream(), txt.p, n, ls.p, L, names.p, noff.p, nlen.p, hash.p, rank.p, N,
                       seed, sentinel, keys.p, counts.p, bad.p);
    HIP_CHECK(hipGetLastError());
    const uint32_t bad_line = download_one(bad.p);
    if (bad_line != NO_LINE) fail(HLMI_EINVAL, "%s: %s:%llu: a list row has fewer than 6 fields", who, pc.path, (unsigned long long)bad_line + 1);
    sort_keys_u64(keys.p, 2 * L, 0, 32 + bits_for(N));
    DBuf<uint8_t> head(2 * L);
    DBuf<uint32_t> idx(2 * L);
    hipLaunchKernelGGL(pp_head_kernel, grid1(2 * L), dim3(WG), 0, stream(), keys.p, 2 * L, sentinel, head.p, counts.p + 1);
    HIP_CHECK(hipGetLastError());
    const size_t K = select_flagged_indices(head.p, idx.p, 2 * L);
    if (K) {
        out.keys.alloc(K);
        hipLaunchKernelGGL(pp_gather_kernel, grid1(K), dim3(WG), 0, stream(), keys.p, idx.p, K, out.keys.p);
        HIP_CHECK(hipGetLastError());
    }
    out.n = K;
    const std::vector<unsigned long long> c = counts.download(2);
    pc.pairs_unknown = c[0];
    pc.pairs_listed = c[1];
}

}  // namespace pol
}  // namespace hlmi
