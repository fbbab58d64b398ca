// sketch_gpu_check.cpp - a direct check of the read store and the sketch (csrc/sketch.hip): upload_reads (both overloads),
// subset_reads_device, DevReads::pack, sketch_device and sketch_device_into against plain sequential host C++, at the k, w
// and tile edges of the kernels.  Compiled as HIP by tests/test_gpu_sketch_direct.py and linked against libhylight_mi.so: it
// calls the hlmi:: functions themselves (the library exports them), no C-ABI entry point is added.
//
//   sketch_gpu_check --host                  what needs no device: the references below against literal hand cases
//   sketch_gpu_check --dump FILE k w hpc     the reference sketch of the sequences in FILE (one per line, an empty line is an
//                                            empty read): "read <i> n=<count>", then one "<x> <y>" line per minimizer (decimal)
//   sketch_gpu_check                         hlmi_init(0, 0), then the groups encode, pack, subset, sketch_grid, sketch_lengths,
//                                            sketch_tiles, sketch_ties, sketch_spans, sketch_many_reads, sketch_parts, refusal in
//                                            this order in one process; one line "group <name> cases=<n> ok" each
// Exit 1 at the first mismatch (group, case, first differing index, want / got), exit 2 at the first HIP error or
// hlmi::Error; nothing is launched after either.  Everything is integer and compared exactly.  Inputs come from a fixed-seed
// generator.
//
// The references are written from the definitions (the header comments of sketch.hip and ava.h), not from the kernels and
// not from oracle/ava_oracle.c: no queue of run lengths, no rolling k-mer word, no tile.  tests/test_gpu_sketch_direct.py
// compares --dump with oracle.ava.sketch on the CPU, so the two restatements hold each other.
//
// Sizes: the sketch kernels cut the slot array into workgroup tiles of 256 slots with w + k - 2 (symbols) and w - 1 (keys)
// slots of halo; pack_kernel writes one flag word per half wave of 32 granules.  k is odd in [3, 28], w in [1, 64].
#include <cstdlib>
#include <fstream>
#include <functional>

#include "ava.h"
#include "seq_scan.h"

using namespace hlmi;

namespace {

constexpr size_t PAD = DevReads::PAD;
constexpr size_t GUARD = 64;                      // sentinel entries behind an output's n entries
constexpr uint32_t SENT32 = 0xa5a5a5a5u;
constexpr uint64_t SENT64 = 0xa5a5a5a5a5a5a5a5ull;

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

[[noreturn]] void mismatch(const char *what, size_t idx, unsigned long long want, unsigned long long got) {
    printf("MISMATCH group %s case %s %s index=%zu want=%llu (0x%llx) got=%llu (0x%llx)\n", g_group, g_case.c_str(), what, idx, want,
           want, got, got);
    fflush(stdout);
    throw Mismatch{};
}
template <typename T>
void expect_eq(const char *what, const T *want, const T *got, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (want[i] != got[i]) mismatch(what, i, (unsigned long long)want[i], (unsigned long long)got[i]);
}
template <typename T>
void expect_all(const char *what, const T *got, size_t first, size_t count, T value) {
    for (size_t i = 0; i < count; ++i)
        if (got[first + i] != value) mismatch(what, first + i, (unsigned long long)value, (unsigned long long)got[first + i]);
}
void expect_one(const char *what, unsigned long long want, unsigned long long got) {
    if (want != got) mismatch(what, 0, want, got);
}

// ------------------------------------------------------------------------------------------
// host references
// ------------------------------------------------------------------------------------------
// encode: A C G T (either case) and U u are 0 1 2 3, every other byte is 4.  Rows of 16: 0x41 'A', 0x43 'C', 0x47 'G', 0x54 'T',
// 0x55 'U', 0x61 'a', 0x63 'c', 0x67 'g', 0x74 't', 0x75 'u'.
const uint8_t ENC[256] = {
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x00
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x10
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x20
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x30
    4, 0, 4, 1, 4, 4, 4, 2, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x40  @ A B C D E F G
    4, 4, 4, 4, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x50  P Q R S T U
    4, 0, 4, 1, 4, 4, 4, 2, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x60  ` a b c d e f g
    4, 4, 4, 4, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x70  p q r s t u
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x80
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0x90
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0xa0
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0xb0
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0xc0
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0xd0
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0xe0
    4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,   // 0xf0
};

// a read set as the device holds it
struct HostReads {
    std::vector<uint64_t> off;        // n + 1
    std::vector<uint8_t> store;       // PAD codes 4, the codes of all reads, PAD codes 4
    std::vector<uint8_t> packed;      // 2 bits per base of the store, whole granules, and 16 zero bytes
    std::vector<uint32_t> nflag;      // a bit per granule, whole words, and two words of ones
    size_t n() const { return off.size() - 1; }
    uint64_t total() const { return off.back(); }
};

// pack: base i of the store (padding included) has the two bits code & 3 at bit 2 (i & 3) of byte i >> 2; granule g = bases
// 32 g .. 32 g + 31 is flagged when one of them is code 4 or lies behind the store (the padding is code 4, so its granules are
// set; so are the granules behind the array that fill up the last flag word)
void ref_pack(HostReads &h) {
    const uint64_t n_store = h.store.size(), n_gran = (n_store + 31) / 32, n_words = (n_gran + 31) / 32;
    h.packed.assign(n_gran * 8 + 16, 0);
    for (uint64_t i = 0; i < n_store; ++i) h.packed[i >> 2] |= (uint8_t)((h.store[i] & 3) << (2 * (i & 3)));
    h.nflag.assign(n_words + 2, 0);
    for (uint64_t g = 0; g < n_words * 32; ++g) {
        bool amb = false;
        for (uint64_t i = 32 * g; i < 32 * g + 32; ++i) amb = amb || i >= n_store || h.store[i] == 4;
        if (amb) h.nflag[g / 32] |= 1u << (g % 32);
    }
    h.nflag[n_words] = h.nflag[n_words + 1] = 0xffffffffu;
}

HostReads ref_reads(const std::vector<std::string> &reads) {
    HostReads h;
    h.off.push_back(0);
    h.store.assign(PAD, 4);
    for (const std::string &r : reads) {
        for (char c : r) h.store.push_back(ENC[(uint8_t)c]);
        h.off.push_back(h.off.back() + r.size());
    }
    h.store.insert(h.store.end(), PAD, 4);
    ref_pack(h);
    return h;
}

uint64_t ref_hash(uint64_t key, uint64_t mask) {            // the seven steps of Li 2016 section 2.2 (pinned by tests/test_oracle_ava.py)
    key = (~key + (key << 21)) & mask;
    key = key ^ key >> 24;
    key = ((key + (key << 3)) + (key << 8)) & mask;
    key = key ^ key >> 14;
    key = ((key + (key << 2)) + (key << 4)) & mask;
    key = key ^ key >> 28;
    key = (key + (key << 31)) & mask;
    return key;
}

// The (k, w)-minimizers of one read, in position order, from the definition:
//   1. slots: a homopolymer run with hpc, a single base without it or when the base is ambiguous
//   2. per slot the number of symbol slots since the last ambiguous one (itself included)
//   3. the forward word of the slot's last k symbols (first symbol in the highest two bits) and the word of their reverse complement
//   4. the span in bases: the k run lengths with hpc, k without
//   5. a key hash(canonical word) << 8 | span, only with k symbols and span < 256
//   6. y = rid << 32 | (last base of the slot) << 1 | strand (1: the reverse complement is the smaller word)
//   7. a slot with a key is a minimizer iff one of the windows of w consecutive slots of the read that contain it has w + k - 1
//      unambiguous trailing symbols and that slot's key as its minimum (a slot without a key counts as the largest value)
// k is odd, so a k-mer never equals its reverse complement (the middle symbol would be its own complement): there is no
// palindrome case to arrange.
std::vector<Mz> ref_sketch_read(const uint8_t *codes, size_t len, uint32_t rid, int k, int w, int hpc) {
    const uint64_t NOKEY = ~0ull, mask = (1ull << 2 * k) - 1;
    std::vector<uint8_t> sym;
    std::vector<uint64_t> last, runlen;
    for (size_t i = 0; i < len;) {
        size_t run = 1;
        if (hpc && codes[i] < 4) while (i + run < len && codes[i + run] == codes[i]) ++run;
        sym.push_back(codes[i]);
        last.push_back(i + run - 1);
        runlen.push_back(run);
        i += run;
    }
    const long ns = (long)sym.size();
    std::vector<long> cnt(ns);
    std::vector<uint64_t> key(ns, NOKEY), y(ns, 0);
    for (long s = 0; s < ns; ++s) {
        cnt[s] = sym[s] < 4 ? (s ? cnt[s - 1] : 0) + 1 : 0;
        if (cnt[s] < k) continue;
        uint64_t fwd = 0, rev = 0, span = 0;
        for (int t = 0; t < k; ++t) {                        // t-th symbol of the k-mer
            const uint64_t c = sym[s - k + 1 + t];
            fwd |= c << 2 * (k - 1 - t);
            rev |= (3 - c) << 2 * t;
            span += hpc ? runlen[s - k + 1 + t] : 1;
        }
        if (span >= 256) continue;
        const uint64_t strand = fwd < rev ? 0 : 1;
        key[s] = ref_hash(strand ? rev : fwd, mask) << 8 | span;
        y[s] = (uint64_t)rid << 32 | last[s] << 1 | strand;
    }
    std::vector<Mz> out;
    for (long j = 0; j < ns; ++j) {
        if (key[j] == NOKEY) continue;
        bool sel = false;
        for (long a = j - w + 1; a <= j && !sel; ++a) {      // the window [a, a + w - 1]
            const long e = a + w - 1;
            if (a < 0 || e >= ns || cnt[e] < w + k - 1) continue;
            uint64_t mn = NOKEY;
            for (long t = a; t <= e; ++t) mn = std::min(mn, key[t]);
            sel = mn == key[j];
        }
        if (sel) out.push_back(Mz{key[j], y[j]});
    }
    return out;
}

struct RefSketch { std::vector<Mz> mz; std::vector<uint32_t> counts; };
// reads [lo, hi) of a set; read i gets rid_base + (i - lo)
RefSketch ref_sketch_set(const std::vector<std::string> &reads, size_t lo, size_t hi, int k, int w, int hpc, uint32_t rid_base) {
    RefSketch r;
    for (size_t i = lo; i < hi; ++i) {
        std::vector<uint8_t> codes(reads[i].size());
        for (size_t b = 0; b < codes.size(); ++b) codes[b] = ENC[(uint8_t)reads[i][b]];
        const std::vector<Mz> m = ref_sketch_read(codes.data(), codes.size(), rid_base + (uint32_t)(i - lo), k, w, hpc);
        r.mz.insert(r.mz.end(), m.begin(), m.end());
        r.counts.push_back((uint32_t)m.size());
    }
    return r;
}

// ------------------------------------------------------------------------------------------
// --host: the references against hand cases
// ------------------------------------------------------------------------------------------
#define HOST_EXPECT(cond)                                                                                  \
    do {                                                                                                   \
        ++g_cases;                                                                                         \
        if (!(cond)) { printf("MISMATCH host %s: %s (line %d)\n", g_group, #cond, __LINE__); return 1; }   \
    } while (0)
int host_done() { printf("host %s cases=%zu ok\n", g_group, g_cases); g_cases = 0; return 0; }

// one minimizer as a hand case writes it: the canonical k-mer word before hashing, span, position, strand
struct HandMz { uint64_t word; int span; int pos; int strand; };
bool sketch_is(const std::string &seq, int k, int w, int hpc, std::initializer_list<HandMz> want) {
    const RefSketch r = ref_sketch_set({seq}, 0, 1, k, w, hpc, 7);
    if (r.counts.size() != 1 || r.counts[0] != r.mz.size()) return false;
    if (r.mz.size() != want.size()) { printf("(%.40s: %zu minimizers, %zu expected)\n", seq.c_str(), r.mz.size(), want.size()); return false; }
    size_t i = 0;
    for (const HandMz &m : want) {
        const uint64_t x = ref_hash(m.word, (1ull << 2 * k) - 1) << 8 | (uint64_t)m.span;
        const uint64_t y = 7ull << 32 | (uint64_t)m.pos << 1 | (uint64_t)m.strand;
        if (r.mz[i].x != x || r.mz[i].y != y) { printf("(%.40s: minimizer %zu)\n", seq.c_str(), i); return false; }
        ++i;
    }
    return true;
}

int run_host() {
    g_group = "ref_encode";
    {
        int n[5] = {0, 0, 0, 0, 0};
        for (int c = 0; c < 256; ++c) ++n[ENC[c]];
        HOST_EXPECT(n[0] == 2 && n[1] == 2 && n[2] == 2 && n[3] == 4 && n[4] == 246);
        HOST_EXPECT(ENC['A'] == 0 && ENC['a'] == 0 && ENC['C'] == 1 && ENC['c'] == 1 && ENC['G'] == 2 && ENC['g'] == 2);
        HOST_EXPECT(ENC['T'] == 3 && ENC['t'] == 3 && ENC['U'] == 3 && ENC['u'] == 3);
        HOST_EXPECT(ENC['N'] == 4 && ENC['n'] == 4 && ENC['R'] == 4 && ENC['-'] == 4 && ENC[0] == 4 && ENC[255] == 4 && ENC['@'] == 4);
    }
    host_done();

    g_group = "ref_hash";
    // literal answers of tests/test_oracle_ava.py (HASH_KAT), and the 6-bit hash of k = 3 the hand cases below order their keys by
    HOST_EXPECT(ref_hash(0x0, (1ull << 38) - 1) == 0x1df06f29bcull);
    HOST_EXPECT(ref_hash(0x123456789ull, (1ull << 38) - 1) == 0xa635aa6a1ull);
    HOST_EXPECT(ref_hash(0x3fffffffffull, (1ull << 38) - 1) == 0x1c5d2677beull);
    HOST_EXPECT(ref_hash(0x2, (1ull << 42) - 1) == 0x33f6f2a0674ull);
    HOST_EXPECT(ref_hash(0x3ffffffffffull, (1ull << 42) - 1) == 0xddf0b551bfull);
    {
        uint64_t seen = 0;
        for (uint64_t v = 0; v < 64; ++v) seen |= 1ull << ref_hash(v, 63);
        HOST_EXPECT(seen == ~0ull);                            // invertible on 6 bits
    }
    // k = 3: AAA = 0 -> 3, AAC = 1 -> 6, ACA = 4 -> 15, ACG = 6 -> 21, CAC = 17 -> 54, CGA = 24 -> 11, GAC = 33 -> 38, GTA = 44 -> 7
    HOST_EXPECT(ref_hash(0, 63) == 3); HOST_EXPECT(ref_hash(1, 63) == 6); HOST_EXPECT(ref_hash(4, 63) == 15); HOST_EXPECT(ref_hash(6, 63) == 21);
    HOST_EXPECT(ref_hash(17, 63) == 54); HOST_EXPECT(ref_hash(24, 63) == 11); HOST_EXPECT(ref_hash(33, 63) == 38); HOST_EXPECT(ref_hash(44, 63) == 7);
    host_done();

    g_group = "ref_pack";
    {
        // 70 bases: 17 x ACGT, then GT, with base 37 (a C) replaced by N.  Store: 64 padding bases (16 bytes of 0), the bases, 64 padding
        // bases; 198 bases are 7 granules (56 bytes) and 16 bytes of slack.  ACGT packs to 0 | 1 << 2 | 2 << 4 | 3 << 6 = 0xe4; the N's
        // group A N G T to 0xe0 (byte 16 + 37 / 4 = 25); G T to 2 | 3 << 2 = 0x0e (byte 16 + 17 = 33).
        std::string s;
        for (int i = 0; i < 17; ++i) s += "ACGT";
        s += "GT";
        s[37] = 'N';
        const HostReads h = ref_reads({s});
        std::vector<uint8_t> want(72, 0);
        for (int b = 16; b < 33; ++b) want[b] = 0xe4;
        want[25] = 0xe0;
        want[33] = 0x0e;
        HOST_EXPECT(h.store.size() == 198 && h.off == (std::vector<uint64_t>{0, 70}));
        HOST_EXPECT(h.packed == want);
        // granules 0, 1: padding; 2: bases 0..31, clean; 3: bases 32..63 with the N; 4: bases 64..69 and padding; 5: padding; 6: padding
        // and 26 bases behind the store; 7..31 behind the array.  Every bit but bit 2.
        HOST_EXPECT(h.nflag == (std::vector<uint32_t>{0xfffffffbu, 0xffffffffu, 0xffffffffu}));
        // no base at all: the two paddings, 4 granules
        const HostReads e = ref_reads({});
        HOST_EXPECT(e.store == std::vector<uint8_t>(128, 4) && e.packed == std::vector<uint8_t>(48, 0));
        HOST_EXPECT(e.nflag == (std::vector<uint32_t>{0xffffffffu, 0xffffffffu, 0xffffffffu}));
        // 960 clean bases: 1088 store bases, 34 granules, two flag words; granules 2..31 clean, 32 and 33 are the back padding
        const HostReads c = ref_reads({std::string(960, 'T')});
        HOST_EXPECT(c.nflag == (std::vector<uint32_t>{0x00000003u, 0xffffffffu, 0xffffffffu, 0xffffffffu}));
        HOST_EXPECT(c.packed.size() == 34 * 8 + 16 && c.packed[15] == 0 && c.packed[16] == 0xff && c.packed[255] == 0xff && c.packed[256] == 0);
    }
    host_done();

    g_group = "ref_sketch";
    // one k-mer, smaller than its reverse complement CGT
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21
    HOST_EXPECT(sketch_is("ACG", 3, 1, 0, {{6, 3, 2, 0}}));
    // the reverse complement ACG is the smaller word: strand 1
    //   canonical k-mer, strand, last base, hash: ACG-@2:h=21
    HOST_EXPECT(sketch_is("CGT", 3, 1, 0, {{6, 3, 2, 1}}));
    // w = 1: every k-mer
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  ACG-@3:h=21  AAC-@4:h=6
    HOST_EXPECT(sketch_is("ACGTT", 3, 1, 0, {{6, 3, 2, 0}, {6, 3, 3, 1}, {1, 3, 4, 1}}));
    // TT is one slot: its k-mer CGT ends at base 4 and spans 4
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  ACG-@4:h=21
    HOST_EXPECT(sketch_is("ACGTT", 3, 1, 1, {{6, 3, 2, 0}, {6, 4, 4, 1}}));
    // lower case, u is T
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  ACG-@3:h=21
    HOST_EXPECT(sketch_is("acgu", 3, 1, 0, {{6, 3, 2, 0}, {6, 3, 3, 1}}));
    // 4 slots, a window needs w + k - 1 = 5: none
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  ACG-@3:h=21
    HOST_EXPECT(sketch_is("ACGT", 3, 3, 0, {}));
    // 5 slots: the one window [2, 4]
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  ACG-@3:h=21  GTA+@4:h=7
    HOST_EXPECT(sketch_is("ACGTA", 3, 3, 0, {{44, 3, 4, 0}}));
    // one run, one slot: none
    HOST_EXPECT(sketch_is("AAAAAAA", 3, 1, 1, {}));
    // AAA five times (TTT is larger)
    //   canonical k-mer, strand, last base, hash: AAA+@2:h=3  AAA+@3:h=3  AAA+@4:h=3  AAA+@5:h=3  AAA+@6:h=3
    HOST_EXPECT(sketch_is("AAAAAAA", 3, 1, 0, {{0, 3, 2, 0}, {0, 3, 3, 0}, {0, 3, 4, 0}, {0, 3, 5, 0}, {0, 3, 6, 0}}));
    // the N ends a stretch of 3 symbols (4 needed for a window); behind it 5 symbols, windows end at slots 7 and 8
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  ACG+@6:h=21  ACG-@7:h=21  GTA+@8:h=7
    HOST_EXPECT(sketch_is("ACGNACGTA", 3, 2, 0, {{6, 3, 6, 0}, {6, 3, 7, 1}, {44, 3, 8, 0}}));
    // w = 1: a k-mer on each side of the N
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  ACG+@6:h=21
    HOST_EXPECT(sketch_is("ACGNACG", 3, 1, 0, {{6, 3, 2, 0}, {6, 3, 6, 0}}));
    // period 3: equal keys three slots apart
    //   canonical k-mer, strand, last base, hash: ACG+@2:h=21  CGA+@3:h=11  GAC+@4:h=38  ACG+@5:h=21  CGA+@6:h=11  GAC+@7:h=38  ACG+@8:h=21  CGA+@9:h=11
    HOST_EXPECT(sketch_is("ACGACGACGA", 3, 2, 0, {{24, 3, 3, 0}, {6, 3, 5, 0}, {24, 3, 6, 0}, {6, 3, 8, 0}, {24, 3, 9, 0}}));
    // period 2: ACA and GTG|CAC alternate, a tie in every window of w = 3 or more
    //   canonical k-mer, strand, last base, hash: ACA+@2:h=15  CAC+@3:h=54  ACA+@4:h=15  CAC+@5:h=54  ACA+@6:h=15  CAC+@7:h=54  ACA+@8:h=15
    HOST_EXPECT(sketch_is("ACACACACA", 3, 2, 0, {{4, 3, 2, 0}, {4, 3, 4, 0}, {4, 3, 6, 0}, {4, 3, 8, 0}}));
    // the same with w = 3: every window holds its minimum twice or the other key twice; all ties kept
    //   canonical k-mer, strand, last base, hash: ACA+@2:h=15  CAC+@3:h=54  ACA+@4:h=15  CAC+@5:h=54  ACA+@6:h=15  CAC+@7:h=54  ACA+@8:h=15
    HOST_EXPECT(sketch_is("ACACACACA", 3, 3, 0, {{4, 3, 2, 0}, {4, 3, 4, 0}, {4, 3, 6, 0}, {4, 3, 8, 0}}));
    // k = 5; the two copies of the unit give equal keys 7 apart
    //   canonical k-mer, strand, last base, hash: GATTA+@4:h=1015  ATTAC+@5:h=854  TGTAA-@6:h=339  CTGTA-@7:h=775  ACAGA+@8:h=283  ATCTG-@9:h=93  AATCT-@10:h=680  GATTA+@11:h=1015  ATTAC+@12:h=854  TGTAA-@13:h=339
    HOST_EXPECT(sketch_is("GATTACAGATTACA", 5, 3, 0, {{944, 5, 6, 1}, {72, 5, 8, 0}, {222, 5, 9, 1}, {55, 5, 10, 1}, {944, 5, 13, 1}}));
    // the same with TT as one slot
    //   canonical k-mer, strand, last base, hash: GATAC+@5:h=790  ATACA+@6:h=399  CTGTA-@7:h=775  ACAGA+@8:h=283  ATCTG-@10:h=93  AGATA+@11:h=743  GATAC+@12:h=790  ATACA+@13:h=399
    HOST_EXPECT(sketch_is("GATTACAGATTACA", 5, 3, 1, {{196, 6, 6, 0}, {72, 5, 8, 0}, {222, 6, 10, 1}, {196, 6, 13, 0}}));
    // span 253 + 1 + 1 = 255: the last one with a key
    HOST_EXPECT(sketch_is(std::string(253, 'A') + "CG", 3, 1, 1, {{6, 255, 254, 0}}));
    // span 256: no key
    HOST_EXPECT(sketch_is(std::string(254, 'A') + "CG", 3, 1, 1, {}));
    // A(300) C G has no key, C G T has
    HOST_EXPECT(sketch_is(std::string(300, 'A') + "CGT", 3, 1, 1, {{6, 3, 302, 1}}));
    // without hpc the span is k and every base is a slot: AAA twice, AAC, ACG, then CGT as ACG on strand 1
    HOST_EXPECT(sketch_is(std::string(4, 'A') + "CGT", 3, 1, 0, {{0, 3, 2, 0}, {0, 3, 3, 0}, {1, 3, 4, 0}, {6, 3, 5, 0}, {6, 3, 6, 1}}));
    host_done();
    return 0;
}

int run_dump(const char *path, int k, int w, int hpc) {
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return 64; }
    std::vector<std::string> reads;
    for (std::string line; std::getline(f, line);) reads.push_back(line);
    for (size_t i = 0; i < reads.size(); ++i) {
        const RefSketch r = ref_sketch_set(reads, i, i + 1, k, w, hpc, (uint32_t)i);
        printf("read %zu n=%zu\n", i, r.mz.size());
        for (const Mz &m : r.mz) printf("%llu %llu\n", (unsigned long long)m.x, (unsigned long long)m.y);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// generators and device helpers
// ------------------------------------------------------------------------------------------
const char ACGT[5] = "ACGT";
std::string rand_seq(size_t n) { std::string s(n, 'A'); for (char &c : s) c = ACGT[rnd() & 3]; return s; }
// no two neighbours equal: every base is a slot with and without hpc; `before` is the base in front of the first one
std::string nohp_seq(size_t n, char before = 0) {
    std::string s(n, 'A');
    for (char &c : s) { do c = ACGT[rnd() & 3]; while (c == before); before = c; }
    return s;
}
// every base of s becomes a run of 1..4 (an ambiguous one stays single: each of them is a slot of its own)
std::string stretch(const std::string &s) {
    std::string o;
    for (char c : s) o.append(ENC[(uint8_t)c] < 4 ? 1 + (rnd() & 3) : 1, c);
    return o;
}
std::vector<std::string> stretch(const std::vector<std::string> &v) {
    std::vector<std::string> o;
    for (const std::string &s : v) o.push_back(stretch(s));
    return o;
}

SeqSet make_set(const std::vector<std::string> &reads) {
    SeqSet s;
    s.off.push_back(0);
    for (size_t i = 0; i < reads.size(); ++i) {
        s.names.push_back("r" + std::to_string(i));
        s.bases += reads[i];
        s.off.push_back(s.bases.size());
    }
    return s;
}

template <typename T>
DBuf<T> device_filled(size_t count, T value) {
    std::vector<T> h(count, value);
    DBuf<T> d(count);
    HIP_CHECK(hipMemcpyAsync(d.p, h.data(), count * sizeof(T), hipMemcpyHostToDevice, stream()));
    sync();
    return d;
}

void group_done() {
    printf("group %s cases=%zu ok\n", g_group, g_cases);
    fflush(stdout);
}

// everything a DevReads holds against the reference of the same reads
void check_reads(const DevReads &d, const HostReads &h, bool packed) {
    expect_one("n", h.n(), d.n);
    expect_one("total", h.total(), d.total);
    expect_one("h_off size", h.off.size(), d.h_off.size());
    expect_eq("h_off", h.off.data(), d.h_off.data(), h.off.size());
    const std::vector<uint64_t> off = d.off.download(h.off.size());
    expect_eq("off", h.off.data(), off.data(), h.off.size());
    expect_one("store size", h.store.size(), d.store.n);
    const std::vector<uint8_t> store = d.store.download(h.store.size());
    expect_eq("store", h.store.data(), store.data(), h.store.size());
    if (!packed) return;
    expect_one("packed_store size", h.packed.size(), d.packed_store.n);
    const std::vector<uint8_t> pk = d.packed_store.download(h.packed.size());
    expect_eq("packed_store", h.packed.data(), pk.data(), h.packed.size());
    expect_one("nflag size", h.nflag.size(), d.nflag.n);
    const std::vector<uint32_t> nf = d.nflag.download(h.nflag.size());
    expect_eq("nflag", h.nflag.data(), nf.data(), h.nflag.size());
}

void expect_sketch(const RefSketch &want, size_t n_got, const std::vector<Mz> &mz, const std::vector<uint32_t> &counts) {
    for (size_t i = 0; i < std::min(want.mz.size(), n_got); ++i) {
        if (want.mz[i].y != mz[i].y) mismatch("mz.y", i, want.mz[i].y, mz[i].y);
        if (want.mz[i].x != mz[i].x) mismatch("mz.x", i, want.mz[i].x, mz[i].x);
    }
    expect_one("minimizers", want.mz.size(), n_got);
    expect_eq("counts", want.counts.data(), counts.data(), want.counts.size());
}

// sketch_device of an uploaded set against the reference
void check_sketch(const std::vector<std::string> &reads, const DevReads &d, int k, int w, int hpc, uint32_t rid_base = 0) {
    const RefSketch want = ref_sketch_set(reads, 0, reads.size(), k, w, hpc, rid_base);
    DevSketch sk;
    sketch_device(d, k, w, hpc, rid_base, sk);
    const std::vector<Mz> mz = sk.mz.download(sk.n);
    const std::vector<uint32_t> counts = sk.counts.download(reads.size());
    expect_sketch(want, sk.n, mz, counts);
}
// sketch_device_into of an uploaded set: the buffer has `cap` entries and GUARD sentinel entries behind them
int64_t check_sketch_into(const RefSketch &want, const DevReads &d, int k, int w, int hpc, uint32_t rid_base, size_t cap) {
    DBuf<Mz> out = device_filled<Mz>(cap + GUARD, Mz{SENT64, SENT64});
    DBuf<uint32_t> cnt = device_filled<uint32_t>(d.n + GUARD, SENT32);
    const int64_t n = sketch_device_into(d, k, w, hpc, rid_base, out.p, (int64_t)cap, cnt.p);
    const std::vector<Mz> mz = out.download(cap + GUARD);
    const std::vector<uint32_t> counts = cnt.download(d.n + GUARD);
    expect_sketch(want, (size_t)n, mz, counts);
    for (size_t i = (size_t)n; i < cap + GUARD; ++i)
        if (mz[i].x != SENT64 || mz[i].y != SENT64) mismatch("mz guard", i, SENT64, mz[i].x != SENT64 ? mz[i].x : mz[i].y);
    expect_all("counts guard", counts.data(), d.n, GUARD, SENT32);
    return n;
}

struct Kwh { int k, w, hpc; };
// upload (the range overload), check the store, sketch at every setting
void sketch_case(const char *name, const std::vector<std::string> &reads, std::initializer_list<Kwh> settings) {
    const SeqSet s = make_set(reads);
    DevReads d;
    upload_reads(s, 0, s.size(), d);
    for (const Kwh &p : settings) {
        set_case("%s/k%d_w%d_h%d", name, p.k, p.w, p.hpc);
        check_sketch(reads, d, p.k, p.w, p.hpc);
    }
}

// ------------------------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------------------------
void group_encode() {
    g_group = "encode"; g_cases = 0;
    std::string all(256, 0);
    for (int c = 0; c < 256; ++c) all[c] = (char)c;
    auto run = [&](const char *name, const std::vector<std::string> &reads) {
        set_case("%s", name);
        const SeqSet s = make_set(reads);
        DevReads d;
        upload_reads(s, 0, s.size(), d);
        check_reads(d, ref_reads(reads), true);
    };
    run("one_read", {all});
    // lengths 0 1 2 63 64 65, twice over and one more of 61: 256 bytes
    const size_t lens[13] = {0, 1, 2, 63, 64, 65, 0, 1, 2, 63, 64, 65, 61};
    for (int rot = 0; rot < 2; ++rot) {
        std::vector<std::string> reads;
        size_t at = 0;
        for (size_t l : lens) {
            std::string r(l, 0);
            for (char &c : r) c = all[(at++ + 97 * rot) & 255];
            reads.push_back(r);
        }
        run(rot ? "spread_rotated" : "spread", reads);
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------
void group_pack() {
    g_group = "pack"; g_cases = 0;
    auto run = [&](const std::vector<std::string> &reads) {
        const SeqSet s = make_set(reads);
        DevReads d;
        upload_reads(s, 0, s.size(), d);
        check_reads(d, ref_reads(reads), true);
        return d.nflag.download();
    };
    // PAD = 64: n_gran = (total + 128 + 31) / 32 passes 32 at total 865, 64 at 1889 and 256 at 8033 ... the sizes below put the
    // store's end on both sides of a granule, of a flag word (half a wave) and of a workgroup of pack_kernel
    const size_t totals[] = {0, 1, 31, 32, 33, 63, 64, 65, 864, 865, 896, 897, 959, 960, 961, 1023, 1024, 1025, 1888, 1889, 1920, 1921,
                             8031, 8032, 8033, 8064, 8065, 8127, 8128, 8129};
    for (size_t total : totals)
        for (int pat = 0; pat < 3; ++pat) {                    // clean; an N in about one granule of three; all ambiguous
            set_case("total%zu/%s", total, pat == 0 ? "clean" : pat == 1 ? "sprinkled" : "all_n");
            std::string r = rand_seq(total);
            if (pat == 1) for (char &c : r) if (rnd() % 96 == 0) c = 'N';
            if (pat == 2) r.assign(total, 'N');
            run({r});
        }
    // one ambiguous base through every position of one granule (store bases 1056..1087 = read bases 992..1023), then at the first
    // and the last base of the set: exactly one flag bit outside the padding
    const std::string clean = rand_seq(4096);
    std::vector<size_t> at;
    for (size_t i = 992; i < 1024; ++i) at.push_back(i);
    at.push_back(0);
    at.push_back(4095);
    for (size_t i : at) {
        set_case("moving_n/base%zu", i);
        std::string r = clean;
        r[i] = 'N';
        const std::vector<uint32_t> nf = run({r});
        const size_t g_first = PAD / 32, g_end = (PAD + 4096) / 32;            // granules of the bases alone
        size_t set = 0, where = 0;
        for (size_t g = g_first; g < g_end; ++g) if (nf[g / 32] >> (g % 32) & 1u) { ++set; where = g; }
        expect_one("flag bits outside the padding", 1, set);
        expect_one("flagged granule", (PAD + i) / 32, where);
    }
    // the partial 8-byte group at the end of the store: every total mod 8, the last bases not code 0
    for (size_t total = 4089; total <= 4104; ++total) {
        set_case("tail_group/total%zu", total);
        std::string r = rand_seq(total);
        for (size_t i = total - 9; i < total; ++i) r[i] = "GT"[i & 1];
        run({r});
    }
    // the same over several reads, empty ones among them
    set_case("several_reads");
    run({"", rand_seq(33), "", "", rand_seq(1), "N", rand_seq(700), ""});
    group_done();
}

// ------------------------------------------------------------------------------------------
// subset
// ------------------------------------------------------------------------------------------
void group_subset() {
    g_group = "subset"; g_cases = 0;
    std::vector<std::string> reads = {rand_seq(100), "", rand_seq(31), rand_seq(257), "", "", rand_seq(1), rand_seq(64), "acgtnNRYacgu",
                                      rand_seq(1000), ""};
    reads[3][100] = 'N';
    const SeqSet s = make_set(reads);
    DevReads all;
    upload_reads(s, 0, s.size(), all);
    set_case("whole_set");
    check_reads(all, ref_reads(reads), true);
    struct IdCase { const char *name; std::vector<uint32_t> ids; };
    const IdCase cases[] = {
        {"ascending", {0, 2, 3, 7, 9}},
        {"ascending_with_empty", {0, 1, 2, 4, 5, 8, 10}},
        {"descending", {10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0}},
        {"repeated", {3, 3, 3, 0, 9, 0, 3}},
        {"repeated_empty", {1, 1, 4, 1}},
        {"only_empty", {4, 5, 10}},
        {"one", {9}},
        {"one_base", {6}},
        {"all", {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}},
        {"empty", {}},
    };
    for (const IdCase &c : cases) {
        std::vector<std::string> picked;
        for (uint32_t id : c.ids) picked.push_back(reads[id]);
        const HostReads want = ref_reads(picked);
        // a fresh upload of the same reads in the same order: the reference holds for it, and the three other ways equal it
        set_case("%s/fresh_upload", c.name);
        const SeqSet ps = make_set(picked);
        DevReads fresh;
        upload_reads(ps, 0, ps.size(), fresh);
        check_reads(fresh, want, true);
        set_case("%s/upload_ids", c.name);
        DevReads by_ids;
        upload_reads(s, c.ids, by_ids);
        check_reads(by_ids, want, true);
        set_case("%s/subset_packed", c.name);
        DevReads sub;
        subset_reads_device(all, c.ids, sub, true);
        check_reads(sub, want, true);
        set_case("%s/subset_unpacked", c.name);
        DevReads sub_np;
        subset_reads_device(all, c.ids, sub_np, false);
        check_reads(sub_np, want, false);
        // a subset is sketched like any other set
        set_case("%s/subset_sketch", c.name);
        check_sketch(picked, sub_np, 5, 2, 1);
    }
    // a range of the set that starts and ends inside it
    set_case("range_2_9");
    DevReads part;
    upload_reads(s, 2, 9, part);
    check_reads(part, ref_reads(std::vector<std::string>(reads.begin() + 2, reads.begin() + 9)), true);
    group_done();
}

// ------------------------------------------------------------------------------------------
// sketch_grid
// ------------------------------------------------------------------------------------------
// about 40 reads and 20 kbases: random reads, stretched homopolymers, Ns, lower case, U and IUPAC letters, empty reads at the
// front, in the middle (two in a row) and at the end
std::vector<std::string> mixed_set() {
    std::vector<std::string> v;
    v.push_back("");
    for (int i = 0; i < 12; ++i) v.push_back(rand_seq(200 + rnd() % 900));
    for (int i = 0; i < 6; ++i) v.push_back(stretch(stretch(nohp_seq(80 + rnd() % 150))));
    v.push_back("");
    v.push_back("");
    for (int i = 0; i < 2; ++i) {                               // Ns: single ones, a pair, a stretch, one near each end
        std::string r = rand_seq(900);
        for (size_t at : {(size_t)3, (size_t)200, (size_t)201, (size_t)420, (size_t)890}) r[at + i] = 'N';
        for (size_t at = 600; at < 610 + 40 * (size_t)i; ++at) r[at] = 'N';
        v.push_back(r);
    }
    { std::string r = rand_seq(700); for (char &c : r) c = (char)(c | 0x20); v.push_back(r); }
    {
        std::string r = rand_seq(800);
        for (char &c : r) if (c == 'T' && (rnd() & 1)) c = (rnd() & 1) ? 'U' : 'u';
        const char iupac[] = "RYKMSWBDHVN-*";
        for (int i = 0; i < 10; ++i) r[rnd() % r.size()] = iupac[rnd() % 13];
        v.push_back(r);
    }
    for (int i = 0; i < 12; ++i) v.push_back(i % 3 ? rand_seq(100 + rnd() % 700) : stretch(rand_seq(100 + rnd() % 300)));
    v.push_back(rand_seq(18));
    v.push_back(rand_seq(1));
    v.push_back("");
    return v;
}

void group_sketch_grid() {
    g_group = "sketch_grid"; g_cases = 0;
    const std::vector<std::string> reads = mixed_set();
    const SeqSet s = make_set(reads);
    DevReads d;
    upload_reads(s, 0, s.size(), d);
    set_case("store");
    check_reads(d, ref_reads(reads), true);
    for (int k : {3, 5, 15, 19, 21, 27})
        for (int w : {1, 2, 5, 11, 63, 64})
            for (int hpc = 0; hpc < 2; ++hpc) {
                set_case("k%d_w%d_h%d", k, w, hpc);
                check_sketch(reads, d, k, w, hpc);
            }
    group_done();
}

// ------------------------------------------------------------------------------------------
// sketch_lengths
// ------------------------------------------------------------------------------------------
void group_sketch_lengths() {
    g_group = "sketch_lengths"; g_cases = 0;
    for (const Kwh &p : {Kwh{19, 5, 1}, Kwh{21, 11, 0}, Kwh{27, 64, 1}, Kwh{3, 1, 0}}) {
        const int k = p.k, w = p.w;
        const size_t lens[8] = {0, 1, (size_t)k - 1, (size_t)k, (size_t)(k + w - 2), (size_t)(k + w - 1), (size_t)(k + w), (size_t)(k + 2 * w)};
        std::vector<std::string> all;
        for (size_t l : lens) {
            const std::string r = nohp_seq(l);
            all.push_back(r);
            char name[64];
            snprintf(name, sizeof name, "alone/slots%zu", l);
            sketch_case(name, {r}, {p});
            snprintf(name, sizeof name, "alone_stretched/slots%zu", l);
            sketch_case(name, {stretch(r)}, {p});
        }
        sketch_case("together", all, {p});
        sketch_case("together_stretched", stretch(all), {p});
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// sketch_tiles: reads without homopolymers, so a slot is a base with and without hpc and slot indices are base indices; the
// stretched forms keep the slot indices and move the bases (hpc settings only)
// ------------------------------------------------------------------------------------------
void group_sketch_tiles() {
    g_group = "sketch_tiles"; g_cases = 0;
    for (const Kwh &p : {Kwh{19, 5, 1}, Kwh{27, 64, 1}, Kwh{21, 11, 0}}) {
        auto run = [&](const char *what, size_t at, const std::vector<std::string> &reads) {
            char name[64];
            snprintf(name, sizeof name, "%s/slot%zu", what, at);
            sketch_case(name, reads, {p});
            if (p.hpc) {
                snprintf(name, sizeof name, "%s_stretched/slot%zu", what, at);
                sketch_case(name, stretch(reads), {p});
            }
        };
        const size_t need = (size_t)(p.w + p.k - 1);
        for (size_t border : {256, 512, 768})
            for (size_t at = border - 1; at <= border + 1; ++at) {
                // the first slot of a read at `at` (the read in front ends at at - 1); once more with an empty read between them
                const std::string a = nohp_seq(at), b = nohp_seq(300);
                run("read_boundary", at, {a, b});
                run("read_boundary_empty_between", at, {a, "", b});
                // an ambiguous base at `at`
                std::string n = nohp_seq(at + 300);
                n[at] = 'N';
                run("ambiguous", at, {n});
                // the first slot of a read that ends a valid window (its slot w + k - 2) at `at`, behind a read start and behind an N
                run("first_window", at, {nohp_seq(at - (need - 1)), nohp_seq(300)});
                std::string n2 = nohp_seq(at + 300);
                n2[at - need] = 'N';
                run("first_window_after_n", at, {n2});
                // the last slot of the whole set at `at`: one read, and a short last read
                run("set_end", at, {nohp_seq(at + 1)});
                run("set_end_short_last_read", at, {nohp_seq(at + 1 - (need + 1)), nohp_seq(need + 1)});
            }
        for (size_t m = 1; m <= 3; ++m)
            for (size_t total : {256 * m - 1, 256 * m, 256 * m + 1}) {
                run("total_one_read", total, {nohp_seq(total)});
                run("total_three_reads", total, {nohp_seq(total / 3), nohp_seq(total / 3), nohp_seq(total - 2 * (total / 3))});
            }
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// sketch_ties
// ------------------------------------------------------------------------------------------
std::string repeat_unit(const std::string &unit, size_t len) {
    std::string s;
    while (s.size() < len) s += unit;
    s.resize(len);
    return s;
}

void group_sketch_ties() {
    g_group = "sketch_ties"; g_cases = 0;
    // a period-p repeat has p distinct k-mers: every window of w >= p slots holds its minimum more than once
    const std::initializer_list<Kwh> off = {Kwh{3, 2, 0}, Kwh{3, 64, 0}, Kwh{5, 5, 0}, Kwh{15, 11, 0}, Kwh{19, 5, 0}, Kwh{21, 11, 0}, Kwh{27, 64, 0}};
    sketch_case("period2", {repeat_unit("AC", 600)}, off);
    sketch_case("period3", {repeat_unit("ACG", 600)}, off);
    sketch_case("period7", {repeat_unit("ACGTTGA", 600)}, off);
    sketch_case("period7_hpc", {repeat_unit("ACGTTGA", 600)}, {Kwh{3, 2, 1}, Kwh{5, 5, 1}, Kwh{19, 5, 1}});
    sketch_case("periods_as_reads", {repeat_unit("AC", 300), repeat_unit("ACG", 301), repeat_unit("ACGTTGA", 302), repeat_unit("CA", 255)}, off);
    // two exact copies of a unit back to back: with w above the unit's length the copies' equal keys meet in one window
    const std::string unit = rand_seq(300);
    sketch_case("unit300_twice", {unit + unit}, {Kwh{19, 5, 1}, Kwh{21, 11, 0}, Kwh{15, 8, 1}, Kwh{27, 64, 0}});
    const std::string unit40 = nohp_seq(40, 'A');
    sketch_case("unit40_x8", {repeat_unit(unit40, 320)}, {Kwh{19, 64, 0}, Kwh{19, 64, 1}, Kwh{5, 41, 0}, Kwh{27, 40, 1}});
    group_done();
}

// ------------------------------------------------------------------------------------------
// sketch_spans
// ------------------------------------------------------------------------------------------
void group_sketch_spans() {
    g_group = "sketch_spans"; g_cases = 0;
    const std::initializer_list<Kwh> k19 = {Kwh{19, 5, 1}, Kwh{19, 1, 1}, Kwh{19, 5, 0}};
    // 18 runs of one base and one run of sum - 18: every 19-mer that holds the long run spans `sum` bases
    for (int sum : {254, 255, 256, 257}) {
        char name[32];
        snprintf(name, sizeof name, "kmer_span%d", sum);
        std::string left = nohp_seq(40);
        if (left.back() == 'A') left.back() = left[38] == 'C' ? 'G' : 'C';
        sketch_case(name, {left + std::string((size_t)sum - 18, 'A') + nohp_seq(40, 'A')}, k19);
    }
    // the same with all 19 runs long: 18 runs of 13 and the tenth of 21, 22 or 23
    for (int first : {21, 22, 23}) {                           // 18 x 13 = 234; + 21 = 255, + 22 = 256, + 23 = 257
        char name[32];
        snprintf(name, sizeof name, "all_runs_long%d", first);
        std::string r = nohp_seq(30), mid = nohp_seq(19, r.back());
        for (size_t i = 0; i < 19; ++i) r.append(i == 9 ? (size_t)first : 13, mid[i]);
        r += nohp_seq(30, r.back());
        sketch_case(name, {r}, k19);
    }
    const std::string a = nohp_seq(120, 'G'), b = nohp_seq(120, 'G');
    sketch_case("run400_start", {std::string(400, 'G') + a}, k19);
    sketch_case("run400_middle", {a.substr(0, 119) + (a[118] == 'G' ? "A" : "") + std::string(400, 'G') + b}, k19);
    sketch_case("run400_end", {a.substr(0, 119) + (a[118] == 'G' ? "A" : "") + std::string(400, 'G')}, k19);
    sketch_case("run400_three_reads", {std::string(400, 'G') + a, b + std::string(400, 'T'), std::string(400, 'T')}, k19);
    for (size_t len : {1, 2, 255, 256, 400, 1000}) {
        char name[32];
        snprintf(name, sizeof name, "single_run%zu", len);
        sketch_case(name, {std::string(len, 'C')}, {Kwh{19, 5, 1}, Kwh{3, 1, 1}, Kwh{3, 1, 0}});
    }
    // an N inside a run: two runs and an ambiguous slot between them
    sketch_case("n_in_run", {nohp_seq(60, 'A') + "AAAANAAAA" + nohp_seq(60, 'A'), "AAAANAAAA", "NAAAA", "AAAAN", "N", "NN"},
                {Kwh{19, 5, 1}, Kwh{3, 1, 1}, Kwh{3, 2, 1}, Kwh{5, 2, 0}});
    // the first read ends with the base the second begins with: two slots
    const std::string x = nohp_seq(50), yv = nohp_seq(50);
    sketch_case("same_base_across_reads", {x + "TTT", "TTT" + yv, "T", "T", "TT" + x}, {Kwh{19, 5, 1}, Kwh{3, 1, 1}, Kwh{3, 2, 1}, Kwh{5, 2, 1}});
    group_done();
}

// ------------------------------------------------------------------------------------------
// sketch_many_reads
// ------------------------------------------------------------------------------------------
void group_sketch_many_reads() {
    g_group = "sketch_many_reads"; g_cases = 0;
    const std::initializer_list<Kwh> settings = {Kwh{19, 5, 1}, Kwh{3, 1, 0}, Kwh{3, 2, 1}, Kwh{3, 1, 1}};
    std::vector<std::string> reads;
    for (int i = 0; i < 5000; ++i) reads.push_back(rand_seq(rnd() & 3));
    reads.push_back(rand_seq(2000));
    sketch_case("short5000_long1", reads, settings);
    std::reverse(reads.begin(), reads.end());
    sketch_case("long1_short5000", reads, settings);
    sketch_case("all_empty", std::vector<std::string>(10, ""), settings);
    sketch_case("one_empty", {""}, settings);
    // no read at all: nothing is written, n is 0
    set_case("no_reads");
    {
        DevReads d;
        upload_reads(make_set({}), 0, 0, d);
        check_reads(d, ref_reads({}), true);
        DevSketch sk;
        sketch_device(d, 19, 5, 1, 0, sk);
        expect_one("minimizers", 0, sk.n);
        const RefSketch none;
        expect_one("returned", 0, (unsigned long long)check_sketch_into(none, d, 19, 5, 1, 0, 4));
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// sketch_parts
// ------------------------------------------------------------------------------------------
void group_sketch_parts() {
    g_group = "sketch_parts"; g_cases = 0;
    const std::vector<std::string> reads = mixed_set();
    const SeqSet s = make_set(reads);
    const size_t n = reads.size();
    size_t mid_empty = 0;                                      // the first of the two empty reads in a row
    for (size_t i = 1; i + 1 < n; ++i) if (reads[i].empty() && reads[i + 1].empty()) { mid_empty = i; break; }
    const size_t cuts[4][2] = {{0, 7}, {mid_empty, n}, {mid_empty + 1, mid_empty + 9}, {5, n - 1}};
    for (const Kwh &p : {Kwh{19, 5, 1}, Kwh{21, 11, 0}, Kwh{27, 64, 1}}) {
        const RefSketch whole = ref_sketch_set(reads, 0, n, p.k, p.w, p.hpc, 0);
        std::vector<size_t> first(n + 1, 0);
        for (size_t i = 0; i < n; ++i) first[i + 1] = first[i] + whole.counts[i];
        for (const auto &c : cuts) {
            const size_t a = c[0], b = c[1];
            set_case("cut%zu_%zu/k%d_w%d_h%d", a, b, p.k, p.w, p.hpc);
            RefSketch slice;                                   // the whole set's entries of reads [a, b): they carry rid a ..
            slice.mz.assign(whole.mz.begin() + first[a], whole.mz.begin() + first[b]);
            slice.counts.assign(whole.counts.begin() + a, whole.counts.begin() + b);
            DevReads d;
            upload_reads(s, a, b, d);
            const size_t count = slice.mz.size();
            expect_one("returned", count, (unsigned long long)check_sketch_into(slice, d, p.k, p.w, p.hpc, (uint32_t)a, count));   // cap == count
            // one entry less is refused, and nothing is written
            set_case("cut%zu_%zu/k%d_w%d_h%d/cap_one_short", a, b, p.k, p.w, p.hpc);
            DBuf<Mz> out = device_filled<Mz>(count + GUARD, Mz{SENT64, SENT64});
            DBuf<uint32_t> cnt(d.n);
            int code = 0;
            try {
                (void)sketch_device_into(d, p.k, p.w, p.hpc, (uint32_t)a, out.p, (int64_t)count - 1, cnt.p);
            } catch (const Error &e) {
                if (e.code != HLMI_EINVAL) throw;
                code = e.code;
            }
            expect_one("error code (0: no refusal)", (unsigned long long)(long long)HLMI_EINVAL, (unsigned long long)(long long)code);
            const std::vector<Mz> got = out.download(count + GUARD);
            for (size_t i = count ? count - 1 : 0; i < count + GUARD; ++i)
                if (got[i].x != SENT64 || got[i].y != SENT64) mismatch("entries from cap on", i, SENT64, got[i].x);
        }
        // the high bit of rid_base arrives in y's upper word
        set_case("rid_base_2_31/k%d_w%d_h%d", p.k, p.w, p.hpc);
        DevReads d;
        upload_reads(s, 0, n, d);
        check_sketch(reads, d, p.k, p.w, p.hpc, 1u << 31);
        set_case("rid_base_max/k%d_w%d_h%d", p.k, p.w, p.hpc);
        check_sketch(reads, d, p.k, p.w, p.hpc, 0xffffffffu - (uint32_t)n + 1u);
    }
    group_done();
}

// ------------------------------------------------------------------------------------------
// refusal: k and w outside the admitted range are refused before anything is launched (sketch_core tests them first)
// ------------------------------------------------------------------------------------------
void group_refusal() {
    g_group = "refusal"; g_cases = 0;
    const std::vector<std::string> reads = {rand_seq(500), rand_seq(300)};
    const SeqSet s = make_set(reads);
    DevReads d;
    upload_reads(s, 0, 2, d);
    const int bad[][2] = {{4, 5}, {18, 5}, {28, 5}, {1, 5}, {29, 5}, {-3, 5}, {19, 0}, {19, 65}, {19, -1}};
    for (const auto &kw : bad)
        for (int into = 0; into < 2; ++into) {
            set_case("k%d_w%d/%s", kw[0], kw[1], into ? "sketch_device_into" : "sketch_device");
            DBuf<Mz> out = device_filled<Mz>(GUARD, Mz{SENT64, SENT64});
            DBuf<uint32_t> cnt = device_filled<uint32_t>(GUARD, SENT32);
            int code = 0;
            try {
                DevSketch sk;
                if (into) (void)sketch_device_into(d, kw[0], kw[1], 1, 0, out.p, (int64_t)GUARD, cnt.p);
                else sketch_device(d, kw[0], kw[1], 1, 0, sk);
            } catch (const Error &e) {
                if (e.code != HLMI_EINVAL) throw;
                code = e.code;
            }
            expect_one("error code (0: no refusal)", (unsigned long long)(long long)HLMI_EINVAL, (unsigned long long)(long long)code);
            const std::vector<Mz> mz = out.download(GUARD);
            for (size_t i = 0; i < GUARD; ++i) if (mz[i].x != SENT64 || mz[i].y != SENT64) mismatch("output", i, SENT64, mz[i].x);
            const std::vector<uint32_t> counts = cnt.download(GUARD);
            expect_all("counts", counts.data(), 0, GUARD, SENT32);
        }
    // the edges of the range are admitted
    set_case("admitted_edges");
    check_sketch(reads, d, 3, 1, 1);
    check_sketch(reads, d, 27, 64, 0);
    group_done();
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1) {
        if (argc == 2 && strcmp(argv[1], "--host") == 0) return run_host();
        if (argc == 6 && strcmp(argv[1], "--dump") == 0) return run_dump(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
        fprintf(stderr, "usage: %s [--host | --dump FILE k w hpc]\n", argv[0]);
        return 64;
    }
    if (hlmi_init(0, 0) != HLMI_OK) { printf("hlmi_init: %s\n", hlmi_last_error()); return 2; }
    void (*const groups[])() = {group_encode, group_pack, group_subset, group_sketch_grid, group_sketch_lengths, group_sketch_tiles,
                                group_sketch_ties, group_sketch_spans, group_sketch_many_reads, group_sketch_parts, group_refusal};
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
