// row_text.hip - the stage's final rows as text, written by the GPU (filter_overlap_slr2.py:138-151).
//
// A short-read call keeps millions of rows per pass (C4s: 3.2 M per call); turning them into the 14 tab-separated columns
// on the host threads was a third of such a step.  Here a thread per kept row does what paf_io.cpp:format_scored_row does
// (both through row_score.h: one definition, checked on the host by tests/capi/dec_text_host_check.cpp):
//   score  = 0.4 mc / ((ql + tl) / 2) + 0.6 mc / len,   score2 = 1 - sum_of_X_digits / mc,   score3 = mc / len
// as IEEE doubles in the reference's evaluation order (the library is built with -ffp-contract=off; double division on
// gfx950 is correctly rounded), "%.4f" by the exact integer conversion of dec_text.h (v x 10^4 rounded to
// nearest, ties to even), the `float(score2) < iden` test on the four printed decimals, the sort key of column 12 as an
// integer.  A value outside that conversion's range (negative, non-finite, >= 2^40) is left to the host formatter: the row
// is flagged, never guessed.  Two passes: lengths (+ key), exclusive scan, bytes.
#include "row_text.h"

#include "dev_prims.h"
#include "row_score.h"

namespace hlmi {

namespace {
constexpr int WG = 256;
inline dim3 grid1(size_t n) { return grid_for(n, WG); }

constexpr uint32_t ROW_DROPPED = 0u, ROW_TO_HOST = 0xffffffffu;

struct RowTextArgs {
    const PafRec *recs;
    const uint32_t *idx, *xsum;
    size_t n;
    const char *names;
    const uint64_t *name_off;
    double iden;
};

__global__ __launch_bounds__(WG) void row_len_kernel(RowTextArgs a, uint32_t *len, uint32_t *key) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const PafRec r = a.recs[a.idx[i]];
    RowScore s;
    const int st = row_score(r.nmatch, r.blen, r.qlen, r.tlen, a.xsum[i], a.iden, s);
    if (st != SCORE_KEPT) { len[i] = st == SCORE_GENERAL ? ROW_TO_HOST : ROW_DROPPED; key[i] = 0xffffffffu; return; }
    const uint32_t nq = (uint32_t)(a.name_off[r.qid + 1] - a.name_off[r.qid]), nt = (uint32_t)(a.name_off[r.tid + 1] - a.name_off[r.tid]);
    // 14 columns, a TAB behind every one of them (the 14th too: slr2:151), no newline (the writer adds it)
    len[i] = nq + nt + (uint32_t)(dec_len(r.qlen) + dec_len(r.qs) + dec_len(r.qe) + 1 + dec_len(r.tlen) + dec_len(r.ts) + dec_len(r.te) +
                                   dec_len(r.nmatch) + dec_len(r.blen) + fixed4_len(s.q1) + fixed4_len(s.q2) + fixed4_len(s.q3)) + 14u;
    key[i] = s.key;
}

__global__ __launch_bounds__(WG) void row_write_kernel(RowTextArgs a, const uint32_t *len, const uint64_t *off, char *text) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= a.n || len[i] == ROW_DROPPED || len[i] == ROW_TO_HOST) return;
    const PafRec r = a.recs[a.idx[i]];
    RowScore s;
    row_score(r.nmatch, r.blen, r.qlen, r.tlen, a.xsum[i], a.iden, s);
    char *p = text + off[i];
    auto name = [&](uint32_t id) {
        const char *src = a.names + a.name_off[id];
        const uint32_t n = (uint32_t)(a.name_off[id + 1] - a.name_off[id]);
        for (uint32_t k = 0; k < n; ++k) p[k] = src[k];
        p += n;
    };
    name(r.qid); *p++ = '\t';
    p = put_dec(p, r.qlen); *p++ = '\t';
    p = put_dec(p, r.qs); *p++ = '\t';
    p = put_dec(p, r.qe); *p++ = '\t';
    *p++ = (r.flags & PF_REV) ? '-' : '+'; *p++ = '\t';
    name(r.tid); *p++ = '\t';
    p = put_dec(p, r.tlen); *p++ = '\t';
    p = put_dec(p, r.ts); *p++ = '\t';
    p = put_dec(p, r.te); *p++ = '\t';
    p = put_dec(p, r.nmatch); *p++ = '\t';
    p = put_dec(p, r.blen); *p++ = '\t';
    p = put_fixed4(p, s.q1); *p++ = '\t';
    p = put_fixed4(p, s.q2); *p++ = '\t';
    p = put_fixed4(p, s.q3); *p++ = '\t';
}

// len with the two flag values read as 0
__global__ __launch_bounds__(WG) void row_len_clean_kernel(const uint32_t *len, uint32_t *clean, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) clean[i] = len[i] == ROW_TO_HOST ? 0u : len[i];
}
}  // namespace

void DevNames::upload(const std::vector<std::string> &names_by_id) {
    std::vector<uint64_t> off(names_by_id.size() + 1, 0);
    for (size_t i = 0; i < names_by_id.size(); ++i) off[i + 1] = off[i] + names_by_id[i].size();
    std::string all;
    all.reserve(off.back());
    for (const auto &s : names_by_id) all.append(s);
    text.alloc(all.size() ? all.size() : 1);
    if (all.size()) HIP_CHECK(hipMemcpyAsync(text.p, all.data(), all.size(), hipMemcpyHostToDevice, stream()));
    this->off.upload(off);
    sync();
    n = names_by_id.size();
}

void format_rows_device(const PafRec *d_recs, const std::vector<uint32_t> &idx, const std::vector<uint32_t> &xsum, const DevNames &names,
                        double iden, RowText &out) {
    const size_t n = idx.size();
    out.at.assign(n, 0); out.len.assign(n, 0); out.key.assign(n, 0xffffffffu);
    out.text.clear();
    if (!n) return;
    DBuf<uint32_t> d_idx, d_x, d_len(n), d_key(n), d_clean(n);
    d_idx.upload(idx);
    d_x.upload(xsum);
    RowTextArgs a{d_recs, d_idx.p, d_x.p, n, names.text.p, names.off.p, iden};
    DBuf<uint64_t> d_off(n);
    {
        KTimer kt("row_text");
        hipLaunchKernelGGL(row_len_kernel, grid1(n), dim3(WG), 0, stream(), a, d_len.p, d_key.p);
        hipLaunchKernelGGL(row_len_clean_kernel, grid1(n), dim3(WG), 0, stream(), d_len.p, d_clean.p, n);
        exclusive_scan_u32_to_u64(d_clean.p, d_off.p, n);
    }
    HIP_CHECK(hipGetLastError());
    out.len = d_len.download(n);
    out.key = d_key.download(n);
    const std::vector<uint64_t> off = d_off.download(n);
    const uint64_t total = off[n - 1] + (out.len[n - 1] == ROW_TO_HOST ? 0u : out.len[n - 1]);
    DBuf<char> d_text(total ? total : 1);
    {
        KTimer kt("row_text");
        hipLaunchKernelGGL(row_write_kernel, grid1(n), dim3(WG), 0, stream(), a, d_len.p, d_off.p, d_text.p);
    }
    HIP_CHECK(hipGetLastError());
    out.text.resize(total);
    if (total) HIP_CHECK(hipMemcpyAsync(&out.text[0], d_text.p, total, hipMemcpyDeviceToHost, stream()));
    sync();
    for (size_t i = 0; i < n; ++i) out.at[i] = off[i];
}

}  // namespace hlmi
