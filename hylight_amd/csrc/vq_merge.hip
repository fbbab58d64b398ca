// vq_merge.hip - SRBuilder::mergeAlongEdges (tools/HaploConduct/src/SRBuilder.cpp:1238-1384) on the device: the bases of the
// super-reads and the text of singles.fastq / removed_tip_sequences.fastq.  The host (vq_superread_run.cpp) chooses the pairs
// and decides what is dropped; the kernels here read every base once per pass.
//   read_n_kernel     one wave per read: its 'N's (Read::test_N_rate, Read.h:214-233)
//   rec_size_kernel   per record: bases and bytes, scanned by dev_prims into starts
//   merge_kernel      walks the OUTPUT positions of all records in spans of SPAN positions - a workgroup's work is a span,
//                     never a read: records run from 151 bases to hundreds of kilobases.  <false> counts the 'N's a merged
//                     record would hold (the 5 % rule), <true> writes the FASTQ bytes, headers and separators included.
// Every loop has an explicit bound.
#include <hip/hip_runtime.h>

#include "common.h"
#include "dec_text.h"
#include "dev_prims.h"
#include "vq_internal.h"

namespace hlmi {
namespace vqm {
namespace {

__global__ __launch_bounds__(WG) void read_n_kernel(const uint8_t *bases, const uint64_t *off, uint32_t n_reads, uint32_t *n_count) {
    const uint32_t r = blockIdx.x * (WG / WAVE) + threadIdx.x / WAVE;
    if (r >= n_reads) return;
    const uint32_t lane = threadIdx.x % WAVE;
    const uint64_t b = off[r], len = off[r + 1] - b;
    uint32_t c = 0;
    for (uint64_t i = lane; i < len; i += WAVE) c += bases[b + i] == 'N';
    for (int d = WAVE / 2; d >= 1; d >>= 1) c += __shfl_down(c, d, WAVE);
    if (lane == 0) n_count[r] = c;
}

// len[r] = bases, bytes[r] = "@<id>\n" + bases + "\n+\n" + qualities + "\n"; entry n_rec of both is 0 (the scans' totals)
__global__ void rec_size_kernel(const Rec *rec, uint32_t n_rec, uint32_t *len, uint32_t *bytes) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { len[r] = 0; bytes[r] = 0; return; }
    len[r] = rec[r].len;
    bytes[r] = 2u + (uint32_t)dec_len(rec[r].id) + 2u * rec[r].len + 4u;
}

// the record that holds position c: the largest r in [lo, hi] with pos0[r] <= c
__device__ __forceinline__ uint32_t find_rec(const uint64_t *pos0, uint32_t lo, uint32_t hi, uint64_t c) {
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (pos0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void fetch(const uint8_t *bases, const uint8_t *quals, const uint64_t *off, uint32_t read, uint32_t i,
                                      bool rev, uint8_t &b, uint8_t &q) {
    const uint64_t s = off[read], e = off[read + 1];
    const uint64_t at = rev ? e - 1 - i : s + i;          // reverse: the complement of the mirrored base, the mirrored quality
    b = bases[at];
    q = quals[at];
    if (rev) b = complement(b);
}

template <bool WRITE>
__global__ __launch_bounds__(WG) void merge_kernel(const Rec *rec, const uint64_t *pos0, const uint64_t *byte0, uint32_t n_rec,
                                                   uint64_t n_spans, const uint8_t *bases, const uint8_t *quals,
                                                   const uint64_t *off, const uint16_t *tab, uint8_t *out, uint32_t *n_count) {
    __shared__ uint16_t lds_tab[T_ALL];
    __shared__ uint32_t cnt[CNT_SLOTS];
    for (int i = threadIdx.x; i < T_ALL; i += WG) lds_tab[i] = tab[i];
    const uint64_t total = pos0[n_rec];
    for (uint64_t s = blockIdx.x; s < n_spans; s += gridDim.x) {          // spans of this workgroup (grid-stride, bounded)
        const uint64_t span0 = s * SPAN;
        const uint64_t span_last = span0 + SPAN - 1 < total - 1 ? span0 + SPAN - 1 : total - 1;
        const uint32_t rlo = find_rec(pos0, 0, n_rec - 1, span0), rhi = find_rec(pos0, rlo, n_rec - 1, span_last);
        if (!WRITE) {
            cnt[threadIdx.x] = 0;                                          // (CNT_SLOTS == WG)
        }
        __syncthreads();                                                   // tables loaded / counters cleared
        for (int k = 0; k < SPAN / WG; ++k) {
            const uint64_t c = span0 + (uint64_t)k * WG + threadIdx.x;     // consecutive lanes, consecutive output bytes
            if (c >= total) break;
            const uint32_t r = find_rec(pos0, rlo, rhi, c);
            const Rec R = rec[r];
            const uint32_t x = (uint32_t)(c - pos0[r]);
            const uint32_t len_a = (uint32_t)(off[R.a + 1] - off[R.a]);
            const bool has_a = x < len_a;
            bool has_b = false;
            if (R.b != NONE && x >= R.p) has_b = x - R.p < (uint32_t)(off[R.b + 1] - off[R.b]);
            uint8_t b1 = 'N', q1 = '!', b2 = 'N', q2 = '!';
            if (has_a) fetch(bases, quals, off, R.a, x, R.flags & F_REV_A, b1, q1);
            if (has_b) fetch(bases, quals, off, R.b, x - R.p, R.flags & F_REV_B, b2, q2);
            uint8_t ob, oq;
            if (!(R.flags & F_CONS)) {                                     // a trivial super-read or a tip: the read itself
                ob = b1; oq = q1;
            } else if (has_a != has_b) {                                   // one base: consensus_pos of that base alone
                if (has_b) { b1 = b2; q1 = q2; }
                const uint16_t e = lds_tab[T_SINGLE + base_code(b1) * NQ + (q1 - 33)];
                ob = (uint8_t)(e >> 8); oq = (uint8_t)e;
            } else {                                                       // two bases (the host admits no position without one)
                const uint32_t c1 = base_code(b1), c2 = base_code(b2), i1 = q1 - 33, i2 = q2 - 33;
                if (c1 == 4 && c2 == 4) {                                  // no score at all: max_score == 0 (:354-357)
                    ob = 'N'; oq = '$';
                } else if (c1 == 4 || c2 == 4) {
                    const uint16_t e = c1 == 4 ? lds_tab[T_WITH_N + c2 * NQ + i2] : lds_tab[T_WITH_N + c1 * NQ + i1];
                    ob = (uint8_t)(e >> 8); oq = (uint8_t)e;
                } else {
                    const uint16_t e = lds_tab[(c1 == c2 ? T_SAME : T_DIFF) + i1 * NQ + i2];
                    oq = (uint8_t)e;
                    ob = pair_base(e >> 8, b1, b2, c1, c2);
                }
            }
            if (WRITE) {
                const uint32_t w = (uint32_t)dec_len(R.id);
                uint8_t *o = out + byte0[r];
                const uint64_t seq0 = 2u + w;
                o[seq0 + x] = ob;
                o[seq0 + R.len + 3u + x] = oq;
                if (x == 0) {                                              // the record's own bytes: "@<id>\n", "\n+\n", "\n"
                    o[0] = '@';
                    put_dec((char *)o + 1, R.id);                          // (w bytes: the thread of x == 0 writes the whole id)
                    o[1 + w] = '\n';
                    o[seq0 + R.len] = '\n';
                    o[seq0 + R.len + 1] = '+';
                    o[seq0 + R.len + 2] = '\n';
                    o[seq0 + 2ull * R.len + 3] = '\n';
                }
            } else if (ob == 'N') {
                const uint32_t slot = r - rlo;                             // a counter block per workgroup, not one word for all
                if (slot < CNT_SLOTS) atomicAdd(&cnt[slot], 1u);
                else atomicAdd(&n_count[r], 1u);
            }
        }
        if (!WRITE) {
            __syncthreads();
            const uint32_t v = cnt[threadIdx.x];
            if (v) atomicAdd(&n_count[rlo + threadIdx.x], v);              // (v != 0 only for slots <= rhi - rlo)
        }
        __syncthreads();                                                   // before the next span clears the counters
    }
}

}  // namespace
}  // namespace vqm

using namespace vqm;
static_assert(CNT_SLOTS == WG, "one counter per thread");

VqMergeDev::VqMergeDev(const std::vector<std::string> &seq, const std::vector<std::string> &qual, const std::vector<uint16_t> &tables)
    : n_reads_(seq.size()) {
    require_device();
    if (tables.size() != (size_t)T_ALL) fail(HLMI_EINVAL, "vq_merge: consensus tables of %zu entries", tables.size());
    std::vector<uint64_t> off(seq.size() + 1, 0);
    for (size_t r = 0; r < seq.size(); ++r) off[r + 1] = off[r] + seq[r].size();
    std::vector<uint8_t> b(off.back()), q(off.back());
    for (size_t r = 0; r < seq.size(); ++r) {
        memcpy(b.data() + off[r], seq[r].data(), seq[r].size());
        memcpy(q.data() + off[r], qual[r].data(), seq[r].size());           // (the host made sure qual[r] is as long)
    }
    d_bases_.upload(b);
    d_quals_.upload(q);
    d_off_.upload(off);
    d_tab_.upload(tables);
    sync();
}

std::vector<uint32_t> VqMergeDev::read_n_counts() {
    if (!n_reads_) return {};
    DBuf<uint32_t> d(n_reads_);
    {
        KTimer t("vq_read_n");
        hipLaunchKernelGGL(read_n_kernel, dim3(cdiv(n_reads_, (size_t)(WG / WAVE))), dim3(WG), 0, stream(), d_bases_.p, d_off_.p,
                           (uint32_t)n_reads_, d.p);
        HIP_CHECK(hipGetLastError());
    }
    return d.download();
}

void VqMergeDev::layout(const std::vector<Rec> &recs, DBuf<Rec> &d_rec, DBuf<uint64_t> &pos0, DBuf<uint64_t> &byte0) {
    const size_t n = recs.size();
    for (const Rec &r : recs)                             // bounds before anything runs on the device
        if (r.a >= n_reads_ || (r.b != NONE && r.b >= n_reads_) || r.len == 0 || r.len >= (1u << 30))
            fail(HLMI_EINVAL, "vq_merge: bad record (reads %u, %u of %zu, %u bases)", r.a, r.b, n_reads_, r.len);
    d_rec.upload(recs);
    DBuf<uint32_t> len(n + 1), bytes(n + 1);
    pos0.alloc(n + 1);
    byte0.alloc(n + 1);
    KTimer t("vq_rec_layout");
    hipLaunchKernelGGL(rec_size_kernel, dim3(cdiv(n + 1, (size_t)WG)), dim3(WG), 0, stream(), d_rec.p, (uint32_t)n, len.p, bytes.p);
    HIP_CHECK(hipGetLastError());
    exclusive_scan_u32_to_u64(len.p, pos0.p, n + 1);
    exclusive_scan_u32_to_u64(bytes.p, byte0.p, n + 1);
    sync();                                               // len / bytes are released on return
}

static unsigned merge_grid(uint64_t n_spans) {
    int dev = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint64_t cap = (uint64_t)(cus > 0 ? cus : 64) * 4;          // 37 KiB of LDS each: four workgroups share a CU
    return (unsigned)(n_spans < cap ? n_spans : cap);
}

std::vector<uint32_t> VqMergeDev::count_n(const std::vector<Rec> &recs) {
    if (recs.empty()) return {};
    if (recs.size() >= (1ull << 31)) fail(HLMI_EINVAL, "vq_merge: more than 2^31 records");
    DBuf<Rec> d_rec;
    DBuf<uint64_t> pos0, byte0;
    layout(recs, d_rec, pos0, byte0);
    const uint64_t total = download_one(pos0.p + recs.size());
    const uint64_t n_spans = (total + SPAN - 1) / SPAN;
    DBuf<uint32_t> cnt(recs.size());
    cnt.zero();
    {
        KTimer t("vq_merge_count");
        hipLaunchKernelGGL(merge_kernel<false>, dim3(merge_grid(n_spans)), dim3(WG), 0, stream(), d_rec.p, pos0.p, byte0.p,
                           (uint32_t)recs.size(), n_spans, d_bases_.p, d_quals_.p, d_off_.p, d_tab_.p, (uint8_t *)nullptr, cnt.p);
        HIP_CHECK(hipGetLastError());
    }
    return cnt.download();
}

std::string VqMergeDev::write(const std::vector<Rec> &recs, std::vector<uint64_t> &start) {
    start.assign(1, 0);
    if (recs.empty()) return std::string();
    if (recs.size() >= (1ull << 31)) fail(HLMI_EINVAL, "vq_merge: more than 2^31 records");
    DBuf<Rec> d_rec;
    DBuf<uint64_t> pos0, byte0;
    layout(recs, d_rec, pos0, byte0);
    start = byte0.download();
    const uint64_t total = download_one(pos0.p + recs.size());
    const uint64_t n_spans = (total + SPAN - 1) / SPAN;
    DBuf<uint8_t> out(start.back());
    {
        KTimer t("vq_merge_write");
        hipLaunchKernelGGL(merge_kernel<true>, dim3(merge_grid(n_spans)), dim3(WG), 0, stream(), d_rec.p, pos0.p, byte0.p,
                           (uint32_t)recs.size(), n_spans, d_bases_.p, d_quals_.p, d_off_.p, d_tab_.p, out.p, (uint32_t *)nullptr);
        HIP_CHECK(hipGetLastError());
    }
    std::string text(start.back(), '\0');
    HIP_CHECK(hipMemcpyAsync(text.data(), out.p, text.size(), hipMemcpyDeviceToHost, stream()));
    sync();
    return text;
}

}  // namespace hlmi
