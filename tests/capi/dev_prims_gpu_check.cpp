// dev_prims_gpu_check.cpp - a direct check of the device primitives (csrc/dev_prims.hip), the wave operations
// (csrc/wave_ops.h) and the device binary search (csrc/dev_search.h) against plain host C++, at the sizes and bit patterns
// where such code goes wrong.  Compiled as HIP by tests/test_gpu_dev_prims.py and linked against libhylight_mi.so: it calls
// the hlmi:: functions themselves (the library exports them: no visibility flag in the build), no C-ABI entry point is added.
//
//   dev_prims_gpu_check --host    what needs no device: bits_for, and every host reference below against literal hand cases
//   dev_prims_gpu_check           hlmi_init(0, 0), then the groups select, classes4, heads, sort, scan, search, wave, refusal in
//                                 this order in one process; one line "group <name> cases=<n> ok" each
// Exit 1 at the first mismatch (group, case, n, first differing index, want / got), exit 2 at the first HIP error or
// hlmi::Error; nothing is launched after either.  Everything is integer and compared exactly.  Inputs come from a fixed-seed
// generator; there are no files.
//
// Sizes: one block of the four-per-thread kernels covers 1024 elements, one wave of them 256, one mask word 64.
// Sort sizes add 16383 .. 16385 (one histogram block of the project's onesweep configurations, 1024 x 16) and SORT_BIG.
// rocPRIM's dispatcher (rocprim/device/device_radix_sort.hpp, radix_sort_impl: "size <= merge_sort_limit && (sizeof(key_type)
// > 2 || size < 100000)") sorts up to merge_sort_limit items by merge sort and takes the onesweep path above;
// merge_sort_limit is the fourth parameter of radix_sort_config (rocprim/device/device_radix_sort_config.hpp), 1024 * 1024 by
// default, and neither of the project's two configurations sets it.  So the 64- and 32-bit keys reach onesweep above 1048576
// elements (SORT_BIG = 1048576 + 1029) and the 16-bit keys from 100000 on (the edge size 100003 already does).
//
// Wave operations run on full waves only.  Every call site in csrc was read for this: each sits in control flow that is
// uniform over the wave (loops bounded by a row's fields or by a readfirstlane value, one row or one task list per wave,
// kernels without an early return in front of the call), and lanes without work take part with a neutral operand (0, the
// identity, a skipped op) instead of being masked off.  No call site with fewer than 64 active lanes was found, so no
// partial-wave pattern is tested.  The two same-width scans are not tested in place: no caller in csrc passes in == out.
#include <climits>
#include <cstdlib>
#include <functional>
#include <numeric>

#include "common.h"
#include "dev_prims.h"
#include "dev_search.h"
#include "wave_ops.h"

using namespace hlmi;

namespace {

const size_t EDGE_SIZES[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 100003};
constexpr size_t SORT_BIG = 1048576 + 1029;
constexpr size_t GUARD = 64;                      // sentinel words behind an output's n entries

struct Mismatch {};                               // thrown after the report is printed
const char *g_group = "";
std::string g_case;
size_t g_cases = 0;

uint64_t g_rng = 0x9e3779b97f4a7c15ull;           // splitmix64, fixed seed
uint64_t rnd() {
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ z >> 27) * 0x94d049bb133111ebull;
    return z ^ z >> 31;
}

void set_case(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_case = buf;
    ++g_cases;
}

[[noreturn]] void mismatch(size_t n, const char *what, size_t idx, unsigned long long want, unsigned long long got) {
    printf("MISMATCH group %s case %s n=%zu %s index=%zu want=%llu (0x%llx) got=%llu (0x%llx)\n", g_group, g_case.c_str(), n, what, idx,
           want, want, got, got);
    fflush(stdout);
    throw Mismatch{};
}

template <typename T>
void expect_eq(size_t n, const char *what, const T *want, const T *got, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (want[i] != got[i]) mismatch(n, what, i, (unsigned long long)want[i], (unsigned long long)got[i]);
}
template <typename T>
void expect_all(size_t n, const char *what, const T *got, size_t first, size_t count, T value) {
    for (size_t i = 0; i < count; ++i)
        if (got[first + i] != value) mismatch(n, what, first + i, (unsigned long long)value, (unsigned long long)got[first + i]);
}
void expect_one(size_t n, const char *what, unsigned long long want, unsigned long long got) {
    if (want != got) mismatch(n, what, 0, want, got);
}

// ------------------------------------------------------------------------------------------
// host references
// ------------------------------------------------------------------------------------------
std::vector<uint32_t> ref_select(const std::vector<uint8_t> &flags) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < flags.size(); ++i) if (flags[i] != 0) out.push_back((uint32_t)i);
    return out;
}
void ref_classes4(const std::vector<uint8_t> &cls, std::vector<uint32_t> out[4]) {
    for (int c = 0; c < 4; ++c) out[c].clear();
    for (size_t i = 0; i < cls.size(); ++i) if (cls[i] >= 1 && cls[i] <= 4) out[cls[i] - 1].push_back((uint32_t)i);
}
std::vector<uint32_t> ref_heads_u64(const std::vector<uint64_t> &key, int shift) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < key.size(); ++i) if (i == 0 || (key[i] >> shift) != (key[i - 1] >> shift)) out.push_back((uint32_t)i);
    return out;
}
std::vector<uint32_t> ref_heads_split(const std::vector<uint32_t> &skey, const std::vector<uint64_t> &val, int shift) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < val.size(); ++i)
        if (i == 0 || skey[i] != skey[i - 1] || (val[i] >> shift) != (val[i - 1] >> shift)) out.push_back((uint32_t)i);
    return out;
}
// the stable order by the key bits [b0, b1): perm[i] = input index of the i-th element
template <typename K>
std::vector<uint32_t> ref_sort_perm(const std::vector<K> &keys, int b0, int b1) {
    const int nb = b1 - b0;
    const uint64_t mask = nb >= 64 ? ~0ull : (1ull << nb) - 1ull;
    std::vector<uint32_t> perm(keys.size());
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
        return (((uint64_t)keys[a] >> b0) & mask) < (((uint64_t)keys[b] >> b0) & mask);
    });
    return perm;
}
template <typename T>
std::vector<uint64_t> ref_scan(const std::vector<T> &in) {          // 64-bit sequential sum; a 32-bit scan is its low half
    std::vector<uint64_t> out(in.size());
    uint64_t s = 0;
    for (size_t i = 0; i < in.size(); ++i) { out[i] = s; s += (uint64_t)in[i]; }
    return out;
}
size_t ref_lower_bound(const std::vector<uint64_t> &a, uint64_t v) { return (size_t)(std::lower_bound(a.begin(), a.end(), v) - a.begin()); }

// wave operations: x, y = the 64 lanes' operands, u / sel / mask = wave-uniform operands; a per-lane loop each
enum WaveOp { W_MAX_U32, W_MIN_U32, W_MAX_I32, W_PMAX, W_PSUM, W_ROW_SHL1, W_ROW_SHR1, W_ROW_PMAX, W_WRITELANE, W_SELECT, W_SAD,
              W_SCALAR_ADD, W_ROW_SHL1_Z, W_WAVE_SHL1_Z, W_WAVE_SHR1, W_WAVE_SHL1, W_N_OPS };
const char *const WAVE_NAMES[W_N_OPS] = {"wave_max_u32_dpp", "wave_min_u32_dpp", "wave_max_i32_dpp", "wave_prefix_max_incl_dpp",
                                         "wave_prefix_sum_incl_dpp", "row_shl1", "row_shr1", "row_prefix_max_incl_dpp", "writelane_i32",
                                         "select_by_mask", "sad_u32", "scalar_add", "row_shl1_z", "wave_shl1_z", "wave_shr1", "wave_shl1"};
struct WaveUni { int u; int sel; unsigned long long mask; };
void ref_wave(int op, const int *x, const int *y, WaveUni w, int *out) {
    for (int l = 0; l < 64; ++l) {
        const int row0 = l & ~15;
        switch (op) {
        case W_MAX_U32: { uint32_t m = 0; for (int k = 0; k < 64; ++k) m = std::max(m, (uint32_t)x[k]); out[l] = (int)m; break; }
        case W_MIN_U32: { uint32_t m = ~0u; for (int k = 0; k < 64; ++k) m = std::min(m, (uint32_t)x[k]); out[l] = (int)m; break; }
        case W_MAX_I32: { int m = INT_MIN; for (int k = 0; k < 64; ++k) m = std::max(m, x[k]); out[l] = m; break; }
        case W_PMAX: { int m = INT_MIN; for (int k = 0; k <= l; ++k) m = std::max(m, x[k]); out[l] = m; break; }
        case W_PSUM: { uint32_t s = 0; for (int k = 0; k <= l; ++k) s += (uint32_t)x[k]; out[l] = (int)s; break; }
        case W_ROW_SHL1: out[l] = (l & 15) == 15 ? y[l] : x[l + 1]; break;
        case W_ROW_SHR1: out[l] = (l & 15) == 0 ? y[l] : x[l - 1]; break;
        case W_ROW_PMAX: { int m = INT_MIN; for (int k = row0; k <= l; ++k) m = std::max(m, x[k]); out[l] = m; break; }
        case W_WRITELANE: out[l] = l == w.sel ? w.u : x[l]; break;
        case W_SELECT: out[l] = (w.mask >> l) & 1ull ? x[l] : y[l]; break;
        case W_SAD: { const uint32_t a = (uint32_t)x[l], b = (uint32_t)y[l]; out[l] = (int)((a > b ? a - b : b - a) + (uint32_t)w.u); break; }
        case W_SCALAR_ADD: out[l] = (int)((uint32_t)x[0] + (uint32_t)y[0]); break;
        case W_ROW_SHL1_Z: out[l] = (l & 15) == 15 ? 0 : x[l + 1]; break;
        case W_WAVE_SHL1_Z: out[l] = l == 63 ? 0 : x[l + 1]; break;
        case W_WAVE_SHR1: out[l] = l == 0 ? y[l] : x[l - 1]; break;
        case W_WAVE_SHL1: out[l] = l == 63 ? y[l] : x[l + 1]; break;
        }
    }
}

// ------------------------------------------------------------------------------------------
// --host: bits_for, and the references against hand cases
// ------------------------------------------------------------------------------------------
#define HOST_EXPECT(cond)                                                                                  \
    do {                                                                                                   \
        ++g_cases;                                                                                         \
        if (!(cond)) { printf("MISMATCH host %s: %s (line %d)\n", g_group, #cond, __LINE__); return 1; }   \
    } while (0)
template <typename T>
bool same(const std::vector<T> &a, std::initializer_list<T> b) { return a == std::vector<T>(b); }
int host_done() { printf("host %s cases=%zu ok\n", g_group, g_cases); g_cases = 0; return 0; }

int run_host() {
    g_group = "bits_for";
    HOST_EXPECT(bits_for(0) == 1); HOST_EXPECT(bits_for(1) == 1); HOST_EXPECT(bits_for(2) == 2); HOST_EXPECT(bits_for(3) == 2);
    const int ks[] = {8, 16, 31, 32, 63};
    for (int k : ks) { HOST_EXPECT(bits_for((1ull << k) - 1) == k); HOST_EXPECT(bits_for(1ull << k) == k + 1); }
    HOST_EXPECT(bits_for(~0ull) == 64);
    host_done();

    g_group = "ref_select";
    HOST_EXPECT(same<uint32_t>(ref_select({0, 1, 0, 2, 0x80, 0, 0xff}), {1, 3, 4, 6}));
    HOST_EXPECT(same<uint32_t>(ref_select({0, 0, 0}), {}));
    HOST_EXPECT(same<uint32_t>(ref_select({7}), {0}));
    host_done();

    g_group = "ref_classes4";
    {
        std::vector<uint32_t> o[4];
        ref_classes4({0, 1, 2, 3, 4, 5, 255, 4, 1, 1}, o);
        HOST_EXPECT(same<uint32_t>(o[0], {1, 8, 9})); HOST_EXPECT(same<uint32_t>(o[1], {2}));
        HOST_EXPECT(same<uint32_t>(o[2], {3})); HOST_EXPECT(same<uint32_t>(o[3], {4, 7}));
        ref_classes4({5, 0, 255}, o);
        HOST_EXPECT(o[0].empty() && o[1].empty() && o[2].empty() && o[3].empty());
    }
    host_done();

    g_group = "ref_heads";
    HOST_EXPECT(same<uint32_t>(ref_heads_u64({4, 5, 6, 6, 8}, 0), {0, 1, 2, 4}));
    HOST_EXPECT(same<uint32_t>(ref_heads_u64({4, 5, 6, 6, 8}, 1), {0, 2, 4}));          // 2 2 3 3 4
    HOST_EXPECT(same<uint32_t>(ref_heads_u64({1, 1ull << 32 | 1, 1ull << 33 | 1, 1ull << 33 | 1}, 0), {0, 1, 2}));
    HOST_EXPECT(same<uint32_t>(ref_heads_u64({}, 0), {}));
    HOST_EXPECT(same<uint32_t>(ref_heads_split({7, 7, 8, 8, 8}, {16, 17, 17, 33, 34}, 4), {0, 2, 3}));   // val >> 4: 1 1 1 2 2
    HOST_EXPECT(same<uint32_t>(ref_heads_split({0xffff, 0xffff, 0}, {0, 0, 0}, 0), {0, 2}));
    HOST_EXPECT(same<uint32_t>(ref_heads_split({3, 3, 3}, {0, 1ull << 40, 1ull << 40 | 5}, 40), {0, 1}));
    host_done();

    g_group = "ref_sort";
    HOST_EXPECT(same<uint32_t>(ref_sort_perm<uint64_t>({3, 1, 2, 1, 3, 0}, 0, 64), {5, 1, 3, 2, 0, 4}));
    HOST_EXPECT(same<uint32_t>(ref_sort_perm<uint64_t>({3, 1, 2, 1, 3, 0}, 0, 1), {2, 5, 0, 1, 3, 4}));          // bit 0: 1 1 0 1 1 0
    HOST_EXPECT(same<uint32_t>(ref_sort_perm<uint32_t>({0x0200, 0x01ff, 0x0100, 0x02ff}, 8, 16), {1, 2, 0, 3}));  // bits 8..15: 2 1 1 2
    HOST_EXPECT(same<uint32_t>(ref_sort_perm<uint16_t>({0x8000, 0x7fff, 0xffff}, 0, 16), {1, 0, 2}));
    host_done();

    g_group = "ref_scan";
    HOST_EXPECT(same<uint64_t>(ref_scan<uint32_t>({3, 0, 4, 1}), {0, 3, 3, 7}));
    HOST_EXPECT(same<uint64_t>(ref_scan<uint32_t>({0xffffffffu, 0xffffffffu, 1}), {0, 0xffffffffull, 0x1fffffffeull}));
    HOST_EXPECT(same<uint64_t>(ref_scan<uint64_t>({1ull << 40, 1, 2}), {0, 1ull << 40, (1ull << 40) + 1}));
    host_done();

    g_group = "ref_lower_bound";
    HOST_EXPECT(ref_lower_bound({5, 5, 9, 9, 9, 12}, 0) == 0); HOST_EXPECT(ref_lower_bound({5, 5, 9, 9, 9, 12}, 9) == 2);
    HOST_EXPECT(ref_lower_bound({5, 5, 9, 9, 9, 12}, 10) == 5); HOST_EXPECT(ref_lower_bound({5, 5, 9, 9, 9, 12}, 13) == 6);
    HOST_EXPECT(ref_lower_bound({}, 1) == 0);
    host_done();

    g_group = "ref_wave";
    {
        int x[64], y[64], o[64];
        for (int l = 0; l < 64; ++l) { x[l] = l + 1; y[l] = 1000 + l; }
        const WaveUni w{-5, 32, 0x8000000000000001ull};
        ref_wave(W_MAX_U32, x, y, w, o); HOST_EXPECT(o[0] == 64 && o[63] == 64);
        x[7] = (int)0x80000001u;
        ref_wave(W_MAX_U32, x, y, w, o); HOST_EXPECT((uint32_t)o[20] == 0x80000001u);
        ref_wave(W_MAX_I32, x, y, w, o); HOST_EXPECT(o[20] == 64);
        ref_wave(W_MIN_U32, x, y, w, o); HOST_EXPECT(o[5] == 1);
        x[7] = 8;
        ref_wave(W_PSUM, x, y, w, o); HOST_EXPECT(o[0] == 1 && o[3] == 10 && o[63] == 2080);
        ref_wave(W_PMAX, x, y, w, o); HOST_EXPECT(o[0] == 1 && o[40] == 41);
        x[3] = 500;
        ref_wave(W_PMAX, x, y, w, o); HOST_EXPECT(o[2] == 3 && o[3] == 500 && o[63] == 500);
        ref_wave(W_ROW_PMAX, x, y, w, o); HOST_EXPECT(o[15] == 500 && o[16] == 17 && o[31] == 32);
        x[3] = 4;
        ref_wave(W_ROW_SHL1, x, y, w, o); HOST_EXPECT(o[0] == 2 && o[15] == 1015 && o[16] == 18 && o[63] == 1063);
        ref_wave(W_ROW_SHR1, x, y, w, o); HOST_EXPECT(o[0] == 1000 && o[1] == 1 && o[16] == 1016 && o[63] == 63);
        ref_wave(W_ROW_SHL1_Z, x, y, w, o); HOST_EXPECT(o[14] == 16 && o[15] == 0 && o[47] == 0 && o[62] == 64);
        ref_wave(W_WAVE_SHL1_Z, x, y, w, o); HOST_EXPECT(o[15] == 17 && o[63] == 0);
        ref_wave(W_WAVE_SHR1, x, y, w, o); HOST_EXPECT(o[0] == 1000 && o[16] == 16 && o[63] == 63);
        ref_wave(W_WAVE_SHL1, x, y, w, o); HOST_EXPECT(o[0] == 2 && o[15] == 17 && o[63] == 1063);
        ref_wave(W_WRITELANE, x, y, w, o); HOST_EXPECT(o[31] == 32 && o[32] == -5 && o[33] == 34);
        ref_wave(W_SELECT, x, y, w, o); HOST_EXPECT(o[0] == 1 && o[1] == 1001 && o[62] == 1062 && o[63] == 64);
        x[2] = 0; y[2] = -1; x[4] = -1; y[4] = 1;
        ref_wave(W_SAD, x, y, WaveUni{7, 0, 0}, o);
        HOST_EXPECT((uint32_t)o[2] == 0xffffffffu + 7u && (uint32_t)o[4] == 0xfffffffeu + 7u && o[0] == 999 + 7);
        ref_wave(W_SCALAR_ADD, x, y, w, o); HOST_EXPECT(o[0] == 1001 && o[63] == 1001);
    }
    host_done();
    return 0;
}

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
// a device copy of h, at least one element long (no null pointer goes to a primitive)
template <typename T>
DBuf<T> to_device(const std::vector<T> &h) {
    DBuf<T> d(h.empty() ? 1 : h.size());
    if (!h.empty()) {
        HIP_CHECK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream()));
        sync();
    }
    return d;
}
template <typename T>
DBuf<T> device_filled(size_t count, T value) { return to_device(std::vector<T>(count, value)); }

constexpr uint32_t SENT32 = 0xa5a5a5a5u;
constexpr uint64_t SENT64 = 0xa5a5a5a5a5a5a5a5ull;

void group_done() {
    printf("group %s cases=%zu ok\n", g_group, g_cases);
    fflush(stdout);
}

// ------------------------------------------------------------------------------------------
// select
// ------------------------------------------------------------------------------------------
uint8_t set_byte() { const uint8_t v[4] = {1, 2, 0x80, 0xff}; return v[rnd() & 3]; }

void group_select() {
    g_group = "select"; g_cases = 0;
    const char *pat_name[8] = {"none", "all", "first", "last", "every64", "every64m1", "half", "one_in_50"};
    for (size_t n : EDGE_SIZES)
        for (int pat = 0; pat < 8; ++pat) {
            std::vector<uint8_t> flags(n, 0);
            for (size_t i = 0; i < n; ++i) {
                bool f = false;
                switch (pat) {
                case 1: f = true; break;
                case 2: f = i == 0; break;
                case 3: f = i == n - 1; break;
                case 4: f = i % 64 == 0; break;
                case 5: f = i % 64 == 63; break;
                case 6: f = (rnd() & 1) != 0; break;
                case 7: f = rnd() % 50 == 0; break;
                }
                flags[i] = f ? set_byte() : 0;
            }
            const std::vector<uint32_t> want = ref_select(flags);
            DBuf<uint8_t> d_flags = to_device(flags);
            for (int async = 0; async < 2; ++async) {
                set_case("%s/%s", pat_name[pat], async ? "async" : "sync");
                DBuf<uint32_t> d_out = device_filled<uint32_t>(n + GUARD, SENT32);
                size_t count;
                if (async) {
                    DBuf<uint32_t> d_count = device_filled<uint32_t>(1, SENT32);
                    select_flagged_indices_async(d_flags.p, d_out.p, n, d_count.p);
                    count = d_count.download(1)[0];
                } else {
                    count = select_flagged_indices(d_flags.p, d_out.p, n);
                }
                expect_one(n, "count", want.size(), count);
                const std::vector<uint32_t> got = d_out.download(n + GUARD);
                expect_eq(n, "list", want.data(), got.data(), want.size());
                expect_all(n, "guard", got.data(), n, GUARD, SENT32);
            }
        }
    group_done();
}

// ------------------------------------------------------------------------------------------
// classes4
// ------------------------------------------------------------------------------------------
void group_classes4() {
    g_group = "classes4"; g_cases = 0;
    const uint8_t ALL[7] = {0, 1, 2, 3, 4, 5, 255};
    auto other_than = [&](int c) { uint8_t v; do v = ALL[rnd() % 7]; while (v == c); return v; };
    for (size_t n : EDGE_SIZES) {
        // (pattern, class): 0 random; 1 all c; 2 c absent; 3 c only in the last n mod 4; 4 c only at 63 mod 64; 5 c only at 0 mod 256
        for (int pat = 0; pat < 6; ++pat)
            for (int c = 1; c <= (pat == 0 ? 1 : 4); ++c) {
                std::vector<uint8_t> cls(n);
                for (size_t i = 0; i < n; ++i) {
                    switch (pat) {
                    case 0: cls[i] = ALL[rnd() % 7]; break;
                    case 1: cls[i] = (uint8_t)c; break;
                    case 2: cls[i] = other_than(c); break;
                    case 3: cls[i] = i >= n - n % 4 ? (uint8_t)c : other_than(c); break;
                    case 4: cls[i] = i % 64 == 63 ? (uint8_t)c : other_than(c); break;
                    case 5: cls[i] = i % 256 == 0 ? (uint8_t)c : other_than(c); break;
                    }
                }
                const char *pn[6] = {"random", "all", "absent", "tail_only", "only_63_mod_64", "only_0_mod_256"};
                set_case("%s/class%d", pn[pat], c);
                std::vector<uint32_t> want[4];
                ref_classes4(cls, want);
                DBuf<uint8_t> d_cls = to_device(cls);
                DBuf<uint32_t> d_out[4];
                for (int k = 0; k < 4; ++k) d_out[k] = device_filled<uint32_t>(n + GUARD, SENT32);
                DBuf<uint32_t> d_counts = device_filled<uint32_t>(4, SENT32);
                select_classes4_async(d_cls.p, n, d_out[0].p, d_out[1].p, d_out[2].p, d_out[3].p, d_counts.p);
                const std::vector<uint32_t> counts = d_counts.download(4);
                for (int k = 0; k < 4; ++k) {
                    char what[32];
                    snprintf(what, sizeof what, "count%d", k + 1);
                    expect_one(n, what, want[k].size(), counts[k]);
                    const std::vector<uint32_t> got = d_out[k].download(n + GUARD);
                    snprintf(what, sizeof what, "list%d", k + 1);
                    expect_eq(n, what, want[k].data(), got.data(), want[k].size());
                    snprintf(what, sizeof what, "guard%d", k + 1);
                    expect_all(n, what, got.data(), n, GUARD, SENT32);
                }
            }
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// heads
// ------------------------------------------------------------------------------------------
// head flags of n elements (index 0 is always one): the run of an element is the number of heads at or before it, minus one
std::vector<uint8_t> head_pattern(size_t n, int pat, size_t arg) {
    std::vector<uint8_t> h(n, 0);
    for (size_t i = 0; i < n; ++i) {
        switch (pat) {
        case 0: break;                                         // one run
        case 1: h[i] = 1; break;                               // every element
        case 2: h[i] = i % arg == 0; break;                    // on the multiples of arg
        case 3: h[i] = i % arg == arg - 1; break;              // one before them
        case 4: h[i] = rnd() % 3 == 0; break;
        }
    }
    if (pat == 5) for (size_t k = 0; k < arg; ++k) h[k * n / arg] = 1;      // arg heads, evenly spread (arg < n: all distinct)
    if (n) h[0] = 1;
    return h;
}

enum { HI_ONLY = 1 };                                          // runs differ only in bits 32 and above of val >> shift
// val of an element of run r: the run's value above the shift, noise below it (neighbours inside a run differ there)
uint64_t run_val(uint64_t r, int shift, int flags) {
    const uint64_t top = (flags & HI_ONLY) ? (r + 1) << 32 | 0x1234567u : r + 3;
    const uint64_t low = shift ? rnd() & ((1ull << shift) - 1ull) : 0ull;
    return top << shift | low;
}

void heads_case(size_t n, int shift, const std::vector<uint8_t> &heads, const char *pname) {
    // the run number of every element
    std::vector<uint64_t> run(n);
    uint64_t r = 0;
    for (size_t i = 0; i < n; ++i) { if (i && heads[i]) ++r; run[i] = r; }
    auto check = [&](const std::vector<uint32_t> &want, size_t count, const DBuf<uint32_t> &d_out) {
        expect_one(n, "count", want.size(), count);
        const std::vector<uint32_t> got = d_out.download(n + GUARD);
        expect_eq(n, "list", want.data(), got.data(), want.size());
        expect_all(n, "guard", got.data(), n, GUARD, SENT32);
    };
    for (int hi = 0; hi < (shift < 2 ? 2 : 1); ++hi) {
        std::vector<uint64_t> val(n);
        for (size_t i = 0; i < n; ++i) val[i] = run_val(run[i], shift, hi ? HI_ONLY : 0);
        DBuf<uint64_t> d_val = to_device(val);
        {
            set_case("u64/%s/shift%d/%s", pname, shift, hi ? "high_half_only" : "low");
            const std::vector<uint32_t> want = ref_heads_u64(val, shift);
            DBuf<uint32_t> d_out = device_filled<uint32_t>(n + GUARD, SENT32);
            const size_t count = select_run_heads_u64(d_val.p, n, shift, d_out.p);
            check(want, count, d_out);
        }
        for (int kb = 2; kb <= 4; kb += 2) {
            // the short key constant at its largest value: only val >> shift changes
            const uint32_t kmask = kb == 2 ? 0xffffu : 0xffffffffu;
            set_case("split%d/%s/shift%d/%s/val_only", kb, pname, shift, hi ? "high_half_only" : "low");
            std::vector<uint32_t> skey(n, kmask);
            auto run_split = [&](const std::vector<uint32_t> &sk, const std::vector<uint64_t> &v, const DBuf<uint64_t> &d_v) {
                const std::vector<uint32_t> want = ref_heads_split(sk, v, shift);
                DBuf<uint32_t> d_out = device_filled<uint32_t>(n + GUARD, SENT32);
                size_t count;
                if (kb == 2) {
                    std::vector<uint16_t> s16(sk.begin(), sk.end());
                    DBuf<uint16_t> d_s = to_device(s16);
                    count = select_run_heads_split(d_s.p, 2, d_v.p, n, shift, d_out.p);
                } else {
                    DBuf<uint32_t> d_s = to_device(sk);
                    count = select_run_heads_split(d_s.p, 4, d_v.p, n, shift, d_out.p);
                }
                check(want, count, d_out);
            };
            run_split(skey, val, d_val);
            if (hi) continue;
            // only the short key changes (it passes through its largest value and wraps to 0); val differs below the shift
            set_case("split%d/%s/shift%d/skey_only", kb, pname, shift);
            std::vector<uint64_t> cval(n);
            for (size_t i = 0; i < n; ++i) { skey[i] = (uint32_t)(kmask - 2 + run[i]) & kmask; cval[i] = run_val(9, shift, 0); }
            DBuf<uint64_t> d_cval = to_device(cval);
            run_split(skey, cval, d_cval);
            // odd runs start with a change of the short key, even ones with a change of val >> shift
            set_case("split%d/%s/shift%d/alternating", kb, pname, shift);
            for (size_t i = 0; i < n; ++i) { skey[i] = (uint32_t)(kmask - 1 + (run[i] + 1) / 2) & kmask; cval[i] = run_val(run[i] / 2, shift, 0); }
            DBuf<uint64_t> d_aval = to_device(cval);
            run_split(skey, cval, d_aval);
        }
    }
}

void group_heads() {
    g_group = "heads"; g_cases = 0;
    const int shifts[4] = {0, 1, 32, 40};
    for (size_t n : EDGE_SIZES)
        for (int shift : shifts) {
            heads_case(n, shift, head_pattern(n, 0, 0), "one_run");
            heads_case(n, shift, head_pattern(n, 1, 0), "every_element");
            heads_case(n, shift, head_pattern(n, 2, 64), "on_64"); heads_case(n, shift, head_pattern(n, 3, 64), "before_64");
            heads_case(n, shift, head_pattern(n, 2, 256), "on_256"); heads_case(n, shift, head_pattern(n, 3, 256), "before_256");
            heads_case(n, shift, head_pattern(n, 2, 1024), "on_1024"); heads_case(n, shift, head_pattern(n, 3, 1024), "before_1024");
            heads_case(n, shift, head_pattern(n, 4, 0), "random_third");
            if (n == 4096 || n == 100003) {                    // either side of n_heads * 16 < n: the word and the key scatter
                heads_case(n, shift, head_pattern(n, 5, n / 16 - 1), "sparse_n16m1");
                heads_case(n, shift, head_pattern(n, 5, n / 16 + 1), "dense_n16p1");
            }
        }
    group_done();
}

// ------------------------------------------------------------------------------------------
// sort
// ------------------------------------------------------------------------------------------
template <typename K>
std::vector<K> few_keys(size_t n) {                            // six distinct values, random in every bit
    K tab[6];
    for (int i = 0; i < 6; ++i) {
        bool again;
        do { tab[i] = (K)rnd(); again = false; for (int j = 0; j < i; ++j) again |= tab[j] == tab[i]; } while (again);
    }
    std::vector<K> k(n);
    for (size_t i = 0; i < n; ++i) k[i] = tab[rnd() % 6];
    return k;
}
template <typename T> T sentinel() { return (T)SENT64; }

// pointer form: buffers of n + GUARD, the guard must stay
template <typename K, typename V, typename F>
void sort_ptr_case(const char *ep, const std::vector<K> &keys, const std::vector<uint32_t> &perm, int b0, int b1, bool with_vals, F call) {
    const size_t n = keys.size();
    set_case("%s/bits%d_%d", ep, b0, b1);
    std::vector<K> hk(n + GUARD, sentinel<K>());
    std::vector<V> hv(n + GUARD, sentinel<V>());
    for (size_t i = 0; i < n; ++i) { hk[i] = keys[i]; hv[i] = (V)i; }
    DBuf<K> dk = to_device(hk);
    DBuf<V> dv = to_device(hv);
    call(dk.p, dv.p, n, b0, b1);
    const std::vector<K> gk = dk.download(n + GUARD);
    const std::vector<V> gv = dv.download(n + GUARD);
    if (n < 2) {                                               // untouched
        expect_eq(n, "keys", hk.data(), gk.data(), n + GUARD);
        expect_eq(n, "vals", hv.data(), gv.data(), n + GUARD);
        return;
    }
    std::vector<K> wk(n);
    std::vector<V> wv(n);
    for (size_t i = 0; i < n; ++i) { wk[i] = keys[perm[i]]; wv[i] = (V)perm[i]; }
    expect_eq(n, "keys", wk.data(), gk.data(), n);
    expect_all(n, "key guard", gk.data(), n, GUARD, sentinel<K>());
    if (with_vals) expect_eq(n, "vals", wv.data(), gv.data(), n);
    else expect_eq(n, "untouched vals", hv.data(), gv.data(), n);
    expect_all(n, "val guard", gv.data(), n, GUARD, sentinel<V>());
}
// DBuf form: the result is in keys.p / vals.p whichever buffer that now is, the sizes are kept
template <typename K, typename V, typename F>
void sort_dbuf_case(const char *ep, const std::vector<K> &keys, const std::vector<uint32_t> &perm, int b0, int b1, size_t extra, F call) {
    const size_t n = keys.size(), cap = n + extra;
    set_case("%s/bits%d_%d/cap%zu", ep, b0, b1, cap);
    std::vector<K> hk(cap, sentinel<K>());
    std::vector<V> hv(cap, sentinel<V>());
    for (size_t i = 0; i < n; ++i) { hk[i] = keys[i]; hv[i] = (V)i; }
    DBuf<K> dk = to_device(hk);
    DBuf<V> dv = to_device(hv);
    const K *const k_before = dk.p;
    const V *const v_before = dv.p;
    call(dk, dv, n, b0, b1);
    expect_one(n, "keys.n", cap, dk.n);
    expect_one(n, "vals.n", cap, dv.n);
    if (n < 2) {                                               // untouched: the same buffers with the same content
        expect_one(n, "keys.p", (unsigned long long)(uintptr_t)k_before, (unsigned long long)(uintptr_t)dk.p);
        expect_one(n, "vals.p", (unsigned long long)(uintptr_t)v_before, (unsigned long long)(uintptr_t)dv.p);
        const std::vector<K> gk = dk.download(cap);
        const std::vector<V> gv = dv.download(cap);
        expect_eq(n, "keys", hk.data(), gk.data(), cap);
        expect_eq(n, "vals", hv.data(), gv.data(), cap);
        return;
    }
    const std::vector<K> gk = dk.download(n);
    const std::vector<V> gv = dv.download(n);
    std::vector<K> wk(n);
    std::vector<V> wv(n);
    for (size_t i = 0; i < n; ++i) { wk[i] = keys[perm[i]]; wv[i] = (V)perm[i]; }
    expect_eq(n, "keys", wk.data(), gk.data(), n);
    expect_eq(n, "vals", wv.data(), gv.data(), n);
}

void group_sort() {
    g_group = "sort"; g_cases = 0;
    std::vector<size_t> sizes(std::begin(EDGE_SIZES), std::end(EDGE_SIZES));
    for (size_t s : {(size_t)16383, (size_t)16384, (size_t)16385, SORT_BIG}) sizes.push_back(s);
    // bit ranges by key width: all bits; [0, 1); [8, 24) (16-bit keys: [4, 12), the same two digits' worth inside the key); the
    // upper half; a range with differing bits on both sides of it.  One, two, three, four and eight 8-bit passes: results that
    // land in either buffer.
    const int R64[5][2] = {{0, 64}, {0, 1}, {8, 24}, {32, 64}, {20, 44}};
    const int R32[5][2] = {{0, 32}, {0, 1}, {8, 24}, {16, 32}, {4, 28}};
    const int R16[5][2] = {{0, 16}, {0, 1}, {4, 12}, {8, 16}, {3, 14}};
    for (size_t n : sizes) {
        const std::vector<uint64_t> k64 = few_keys<uint64_t>(n);
        const std::vector<uint32_t> k32 = few_keys<uint32_t>(n);
        const std::vector<uint16_t> k16 = few_keys<uint16_t>(n);
        for (int ri = 0; ri < 5; ++ri) {
            const size_t extra = n < 2 ? 5 : (ri == 1 || ri == 4 ? 37 : 0);          // DBuf forms: buffers larger than n for two ranges
            {
                const int b0 = R64[ri][0], b1 = R64[ri][1];
                const std::vector<uint32_t> perm = ref_sort_perm(k64, b0, b1);
                sort_ptr_case<uint64_t, uint32_t>("sort_pairs_u64_u32(ptr)", k64, perm, b0, b1, true,
                                                  [](uint64_t *k, uint32_t *v, size_t m, int a, int b) { sort_pairs_u64_u32(k, v, m, a, b); });
                sort_ptr_case<uint64_t, uint64_t>("sort_pairs_u64_u64(ptr)", k64, perm, b0, b1, true,
                                                  [](uint64_t *k, uint64_t *v, size_t m, int a, int b) { sort_pairs_u64_u64(k, v, m, a, b); });
                sort_ptr_case<uint64_t, uint32_t>("sort_keys_u64(ptr)", k64, perm, b0, b1, false,
                                                  [](uint64_t *k, uint32_t *, size_t m, int a, int b) { sort_keys_u64(k, m, a, b); });
                sort_dbuf_case<uint64_t, uint32_t>("sort_keys_u64(DBuf)", k64, perm, b0, b1, extra,
                                                   [&](DBuf<uint64_t> &k, DBuf<uint32_t> &v, size_t m, int a, int b) {
                                                       sort_keys_u64(k, m, a, b);
                                                       // (no values: put them in the keys' order so that the shared check holds)
                                                       if (m >= 2) { std::vector<uint32_t> pv(perm); pv.resize(v.n, (uint32_t)SENT64); v = to_device(pv); }
                                                   });
                sort_dbuf_case<uint64_t, uint32_t>("sort_pairs_u64_u32(DBuf)", k64, perm, b0, b1, extra,
                                                   [](DBuf<uint64_t> &k, DBuf<uint32_t> &v, size_t m, int a, int b) { sort_pairs_u64_u32(k, v, m, a, b); });
            }
            {
                const int b0 = R32[ri][0], b1 = R32[ri][1];
                const std::vector<uint32_t> perm = ref_sort_perm(k32, b0, b1);
                sort_ptr_case<uint32_t, uint32_t>("sort_pairs_u32_u32(ptr)", k32, perm, b0, b1, true,
                                                  [](uint32_t *k, uint32_t *v, size_t m, int a, int b) { sort_pairs_u32_u32(k, v, m, a, b); });
                sort_dbuf_case<uint32_t, uint32_t>("sort_pairs_u32_u32(DBuf)", k32, perm, b0, b1, extra,
                                                   [](DBuf<uint32_t> &k, DBuf<uint32_t> &v, size_t m, int a, int b) { sort_pairs_u32_u32(k, v, m, a, b); });
                sort_dbuf_case<uint32_t, uint64_t>("sort_pairs_u32_u64(DBuf)", k32, perm, b0, b1, extra,
                                                   [](DBuf<uint32_t> &k, DBuf<uint64_t> &v, size_t m, int a, int b) { sort_pairs_u32_u64(k, v, m, a, b); });
            }
            {
                const int b0 = R16[ri][0], b1 = R16[ri][1];
                const std::vector<uint32_t> perm = ref_sort_perm(k16, b0, b1);
                sort_dbuf_case<uint16_t, uint64_t>("sort_pairs_u16_u64(DBuf)", k16, perm, b0, b1, extra,
                                                   [](DBuf<uint16_t> &k, DBuf<uint64_t> &v, size_t m, int a, int b) { sort_pairs_u16_u64(k, v, m, a, b); });
            }
        }
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// scan
// ------------------------------------------------------------------------------------------
void group_scan() {
    g_group = "scan"; g_cases = 0;
    const char *in_name[4] = {"zeros", "ones", "random", "all_ff"};
    for (size_t n : EDGE_SIZES)
        for (int pat = 0; pat < 4; ++pat) {
            std::vector<uint32_t> in32(n);
            std::vector<uint64_t> in64(n);
            for (size_t i = 0; i < n; ++i) {
                in32[i] = pat == 0 ? 0u : pat == 1 ? 1u : pat == 2 ? (uint32_t)rnd() : 0xffffffffu;
                in64[i] = pat == 0 ? 0ull : pat == 1 ? 1ull : rnd();
            }
            const std::vector<uint64_t> w32 = ref_scan(in32), w64 = ref_scan(in64);
            DBuf<uint32_t> d_in32 = to_device(in32);
            {
                set_case("exclusive_scan_u32_to_u64/%s", in_name[pat]);
                DBuf<uint64_t> d_out = device_filled<uint64_t>(n + GUARD, SENT64);
                exclusive_scan_u32_to_u64(d_in32.p, d_out.p, n);
                const std::vector<uint64_t> got = d_out.download(n + GUARD);
                expect_eq(n, "sums", w32.data(), got.data(), n);
                expect_all(n, "guard", got.data(), n, GUARD, SENT64);
            }
            if (pat == 3) continue;                            // (the repeated 0xffffffff is the widening scan's case)
            {
                set_case("exclusive_scan_u32/%s", in_name[pat]);
                std::vector<uint32_t> want(n);
                for (size_t i = 0; i < n; ++i) want[i] = (uint32_t)w32[i];
                DBuf<uint32_t> d_out = device_filled<uint32_t>(n + GUARD, SENT32);
                exclusive_scan_u32(d_in32.p, d_out.p, n);
                const std::vector<uint32_t> got = d_out.download(n + GUARD);
                expect_eq(n, "sums", want.data(), got.data(), n);
                expect_all(n, "guard", got.data(), n, GUARD, SENT32);
            }
            {
                set_case("exclusive_scan_u64/%s", in_name[pat]);
                DBuf<uint64_t> d_in = to_device(in64);
                DBuf<uint64_t> d_out = device_filled<uint64_t>(n + GUARD, SENT64);
                exclusive_scan_u64(d_in.p, d_out.p, n);
                const std::vector<uint64_t> got = d_out.download(n + GUARD);
                expect_eq(n, "sums", w64.data(), got.data(), n);
                expect_all(n, "guard", got.data(), n, GUARD, SENT64);
            }
        }
    group_done();
}

// ------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lower_bound_kernel(const uint64_t *a, size_t n, const uint64_t *q, size_t nq, uint64_t *out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < nq) out[i] = (uint64_t)lower_bound_u64(a, n, q[i]);
}

void group_search() {
    g_group = "search"; g_cases = 0;
    const size_t lens[7] = {0, 1, 2, 63, 64, 65, 100003};
    for (size_t n : lens) {
        set_case("len%zu", n);
        std::vector<uint64_t> a(n);
        for (size_t i = 0; i < n; ++i) a[i] = 10 * (rnd() % (n / 3 + 1)) + 5;          // duplicates, gaps between the values
        std::sort(a.begin(), a.end());
        std::vector<uint64_t> q = {0, 4, ~0ull, 1ull << 63};                           // below the first, above the last
        for (size_t i = 0; i < n; ++i)
            if (i == 0 || a[i] != a[i - 1]) { q.push_back(a[i]); q.push_back(a[i] - 1); q.push_back(a[i] + 1); q.push_back(a[i] + 5); }
        std::vector<uint64_t> want(q.size());
        for (size_t i = 0; i < q.size(); ++i) want[i] = ref_lower_bound(a, q[i]);
        DBuf<uint64_t> d_a = to_device(a), d_q = to_device(q);
        DBuf<uint64_t> d_out = device_filled<uint64_t>(q.size() + GUARD, SENT64);
        hipLaunchKernelGGL(lower_bound_kernel, dim3(cdiv(q.size(), 256)), dim3(256), 0, stream(), d_a.p, n, d_q.p, q.size(), d_out.p);
        HIP_CHECK(hipGetLastError());
        const std::vector<uint64_t> got = d_out.download(q.size() + GUARD);
        expect_eq(n, "position", want.data(), got.data(), q.size());
        expect_all(n, "guard", got.data(), q.size(), GUARD, SENT64);
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// wave
// ------------------------------------------------------------------------------------------
// 256 threads = four full waves per block, one input row of 64 lanes per wave; x, y, out hold rows x 64 values
template <int OP>
__global__ __launch_bounds__(256) void wave_kernel(const int *x, const int *y, int *out, WaveUni w) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const int a = x[i], b = y[i];
    int r = 0;
    if constexpr (OP == W_MAX_U32) r = (int)wave_max_u32_dpp((uint32_t)a);
    if constexpr (OP == W_MIN_U32) r = (int)wave_min_u32_dpp((uint32_t)a);
    if constexpr (OP == W_MAX_I32) r = wave_max_i32_dpp(a);
    if constexpr (OP == W_PMAX) r = wave_prefix_max_incl_dpp(a);
    if constexpr (OP == W_PSUM) r = (int)wave_prefix_sum_incl_dpp((uint32_t)a);
    if constexpr (OP == W_ROW_SHL1) r = row_shl1(a, b);
    if constexpr (OP == W_ROW_SHR1) r = row_shr1(a, b);
    if constexpr (OP == W_ROW_PMAX) r = row_prefix_max_incl_dpp(a);
    if constexpr (OP == W_WRITELANE) r = writelane_i32(a, w.u, w.sel);
    if constexpr (OP == W_SELECT) r = select_by_mask(w.mask, a, b);
    if constexpr (OP == W_SAD) r = (int)sad_u32((uint32_t)a, (uint32_t)b, (uint32_t)w.u);
    if constexpr (OP == W_SCALAR_ADD) r = scalar_add(__builtin_amdgcn_readfirstlane(a), __builtin_amdgcn_readfirstlane(b));
    if constexpr (OP == W_ROW_SHL1_Z) r = row_shl1_z(a);
    if constexpr (OP == W_WAVE_SHL1_Z) r = wave_shl1_z(a);
    if constexpr (OP == W_WAVE_SHR1) r = wave_shr1(a, b);
    if constexpr (OP == W_WAVE_SHL1) r = wave_shl1(a, b);
    out[i] = r;
}

template <int OP>
void launch_wave(int blocks, const int *x, const int *y, int *out, WaveUni w) {
    hipLaunchKernelGGL(wave_kernel<OP>, dim3(blocks), dim3(256), 0, stream(), x, y, out, w);
}
using WaveLaunch = void (*)(int, const int *, const int *, int *, WaveUni);
template <int... I>
void wave_table(WaveLaunch *t, std::integer_sequence<int, I...>) { ((t[I] = launch_wave<I>), ...); }

constexpr int WAVE_ROWS = 16;                                  // four blocks of four waves
// the rows of one operand: all equal, ascending, descending, one lane other than `ident` at each DPP row / bank border,
// five random rows; `flip` moves the ramps into the signed order
std::vector<int> wave_rows(int ident, int special, int equal, uint32_t flip) {
    const int at[8] = {0, 15, 16, 31, 32, 47, 48, 63};
    std::vector<int> v(WAVE_ROWS * 64);
    for (int r = 0; r < WAVE_ROWS; ++r)
        for (int l = 0; l < 64; ++l) {
            int &o = v[r * 64 + l];
            if (r == 0) o = equal;
            else if (r == 1) o = (int)(((uint32_t)l * 0x04000001u + 3u) ^ flip);
            else if (r == 2) o = (int)(((uint32_t)(63 - l) * 0x04000001u + 3u) ^ flip);
            else if (r < 11) o = l == at[r - 3] ? special : ident;
            else { uint32_t x = (uint32_t)rnd(); if (x >> 24 == 0x7fu) x ^= 0x01000000u; o = (int)x; }
        }
    return v;
}

void group_wave() {
    g_group = "wave"; g_cases = 0;
    WaveLaunch launch[W_N_OPS];
    wave_table(launch, std::make_integer_sequence<int, W_N_OPS>{});
    // the second operand: the fill of the shifts (0x7f...: no lane's own value has that top byte except where said), the `no`
    // side of the select, the subtrahend
    std::vector<int> fill(WAVE_ROWS * 64);
    for (int i = 0; i < WAVE_ROWS * 64; ++i) fill[i] = (int)(0x7f000000u | (uint32_t)i << 8 | 0x5au);
    // operands near 0 and near 2^32 - 1 for the absolute difference
    const uint32_t near[8] = {0u, 1u, 2u, 0xffffffffu, 0xfffffffeu, 0x80000000u, 0x7fffffffu, 0xfffffff0u};
    std::vector<int> sad_a(WAVE_ROWS * 64), sad_b(WAVE_ROWS * 64);
    for (int i = 0; i < WAVE_ROWS * 64; ++i) { sad_a[i] = (int)near[i & 7]; sad_b[i] = (int)near[(i * 3 + 1 + i / 64) & 7]; }

    auto run = [&](int op, const char *variant, const std::vector<int> &x, const std::vector<int> &y, WaveUni w) {
        set_case("%s/%s", WAVE_NAMES[op], variant);
        std::vector<int> want(WAVE_ROWS * 64);
        for (int r = 0; r < WAVE_ROWS; ++r) ref_wave(op, &x[r * 64], &y[r * 64], w, &want[r * 64]);
        DBuf<int> d_x = to_device(x), d_y = to_device(y);
        DBuf<int> d_out = device_filled<int>(WAVE_ROWS * 64 + GUARD, (int)SENT32);
        launch[op](WAVE_ROWS / 4, d_x.p, d_y.p, d_out.p, w);
        HIP_CHECK(hipGetLastError());
        const std::vector<int> got = d_out.download(WAVE_ROWS * 64 + GUARD);
        for (size_t i = 0; i < want.size(); ++i)
            if (want[i] != got[i]) {
                printf("(row %zu lane %zu)\n", i / 64, i % 64);
                mismatch(64, "lane value", i, (uint32_t)want[i], (uint32_t)got[i]);
            }
        expect_all(64, "guard", got.data(), want.size(), GUARD, (int)SENT32);
    };
    const WaveUni none{0, 0, 0};
    // unsigned extrema: values at and above 2^31
    run(W_MAX_U32, "high", wave_rows(0, (int)0x80000005u, (int)0xfffffffeu, 0), fill, none);
    run(W_MAX_U32, "low", wave_rows(0, 7, 0, 0), fill, none);
    run(W_MIN_U32, "high", wave_rows(-1, (int)0x80000005u, (int)0x80000000u, 0), fill, none);
    run(W_MIN_U32, "low", wave_rows(-1, 7, -1, 0), fill, none);
    // signed maxima: negatives and INT_MIN
    for (int op : {W_MAX_I32, W_PMAX, W_ROW_PMAX}) {
        run(op, "negative", wave_rows(INT_MIN, -7, INT_MIN, 0x80000000u), fill, none);
        run(op, "int_min_special", wave_rows(-3, INT_MIN, -1, 0x80000000u), fill, none);
        run(op, "positive", wave_rows(INT_MIN, INT_MAX, 5, 0x80000000u), fill, none);
    }
    // sums that wrap 2^32
    run(W_PSUM, "wrapping", wave_rows(0, (int)0xfffffff0u, (int)0x90000001u, 0), fill, none);
    run(W_PSUM, "ones", wave_rows(1, 1000, 1, 0), fill, none);
    for (int op : {W_ROW_SHL1, W_ROW_SHR1, W_ROW_SHL1_Z, W_WAVE_SHL1_Z, W_WAVE_SHR1, W_WAVE_SHL1})
        run(op, "fill_differs", wave_rows(11, -2, 0x12345678, 0), fill, none);
    for (int sel : {0, 31, 32, 63}) {
        char name[32];
        snprintf(name, sizeof name, "sel%d", sel);
        run(W_WRITELANE, name, wave_rows(11, -2, 0x12345678, 0), fill, WaveUni{(int)0xdeadbeefu, sel, 0});
    }
    const unsigned long long masks[6] = {0ull, ~0ull, 1ull, 1ull << 63, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull};
    for (int m = 0; m < 6; ++m) {
        char name[32];
        snprintf(name, sizeof name, "mask%d", m);
        run(W_SELECT, name, wave_rows(11, -2, 0x12345678, 0), fill, WaveUni{0, 0, masks[m]});
    }
    run(W_SAD, "a_b", sad_a, sad_b, WaveUni{0, 0, 0});
    run(W_SAD, "b_a", sad_b, sad_a, WaveUni{0, 0, 0});
    run(W_SAD, "a_b_plus7", sad_a, sad_b, WaveUni{7, 0, 0});
    run(W_SAD, "b_a_plus7", sad_b, sad_a, WaveUni{7, 0, 0});
    run(W_SAD, "random", wave_rows(0, -1, 1, 0), wave_rows(-1, 0, 1, 0), WaveUni{3, 0, 0});
    run(W_SCALAR_ADD, "uniform", wave_rows(11, -2, 0x7ffffff0, 0), wave_rows(5, 9, 0x20, 0), none);
    group_done();
}

// ------------------------------------------------------------------------------------------
// refusal: 2^32 elements are refused before anything is allocated, launched or dereferenced (read in dev_prims.hip: each of
// the four tests n directly behind its n == 0 exit)
// ------------------------------------------------------------------------------------------
void group_refusal() {
    g_group = "refusal"; g_cases = 0;
    const size_t n = 1ull << 32;
    DBuf<uint8_t> d_b = device_filled<uint8_t>(4, 0);
    DBuf<uint64_t> d_v = device_filled<uint64_t>(4, 0);
    DBuf<uint32_t> d_o = device_filled<uint32_t>(4, SENT32);
    const std::function<void()> calls[5] = {
        [&] { select_flagged_indices_async(d_b.p, d_o.p, n, d_o.p + 1); },
        [&] { select_classes4_async(d_b.p, n, d_o.p, d_o.p, d_o.p, d_o.p, d_o.p); },
        [&] { (void)select_run_heads_u64(d_v.p, n, 0, d_o.p); },
        [&] { (void)select_run_heads_split(d_b.p, 2, d_v.p, n, 0, d_o.p); },
        [&] { (void)select_run_heads_split(d_b.p, 4, d_v.p, n, 0, d_o.p); },
    };
    const char *names[5] = {"select_flagged_indices_async", "select_classes4_async", "select_run_heads_u64", "select_run_heads_split/2",
                            "select_run_heads_split/4"};
    for (int i = 0; i < 5; ++i) {
        set_case("%s", names[i]);
        int code = 0;
        try { calls[i](); } catch (const Error &e) { if (e.code != HLMI_EINVAL) throw; code = e.code; }
        expect_one(n, "error code (0: no refusal)", (unsigned long long)(long long)HLMI_EINVAL, (unsigned long long)(long long)code);
    }
    const std::vector<uint32_t> got = d_o.download(4);
    expect_all(n, "output", got.data(), 0, 4, SENT32);
    group_done();
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1) {
        if (strcmp(argv[1], "--host") != 0) { fprintf(stderr, "usage: %s [--host]\n", argv[0]); return 64; }
        return run_host();
    }
    if (hlmi_init(0, 0) != HLMI_OK) { printf("hlmi_init: %s\n", hlmi_last_error()); return 2; }
    void (*const groups[])() = {group_select, group_classes4, group_heads, group_sort, group_scan, group_search, group_wave, group_refusal};
    for (auto g : groups) {
        try {
            g();
        } catch (const Mismatch &) {
            return 1;
        } catch (const Error &e) {
            printf("ERROR group %s case %s: %s\n", g_group, g_case.c_str(), e.what());
            return 2;
        }
    }
    hlmi_shutdown();
    return 0;
}
