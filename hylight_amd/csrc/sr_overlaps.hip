// sr_overlaps.hip - a read set's self-overlaps as a SAVAGE overlaps file in one call (hlmi_sr_overlaps): what POLYTE's
// run_sfo chain (polyte.tune_params.py:488-529, :534-579) leaves behind -
//   minimap2 --sr -X -c ... -r0 | cut -f1-12 | filter_ovlp_inline.py m 0.98 1 0.8 | minimap22sfo.py -m 0 -p 0 |
//   sfo2overlaps.py --num_pairs 0
// - without the three text files between its links.  The overlapper's rows stay in HBM (ava_device), the inline filter reads
// them there (ovlp_inline_device, in the overlapper's row order: its 1000-row windows depend on it), and the tail of the chain
// is four small kernels, a thread per kept row each:
//   sr_record_kernel   PAF row -> SFO row -> sfo2overlaps' sorted-file row (sr_overlaps.h) and its id-pair key
//   (radix sort by the pair key: `sort -k1,1n -k2,2n -k3,3n -k4,4n` - columns 3, 4 repeat 1, 2)
//   sr_tie_kernel      the whole-line order among the rows of one pair (sfo.cpp:58-61): a row's place is the number of rows
//                      of its pair that sort before it; pairs hold one to a handful of rows (-X: one direction per pair)
//   sr_len_kernel      the 13-column line of every row, dropped when it equals the line before it (`uniq` on the sorted
//                      rows and the writer's own test, sfo.cpp:66,95: equal rows give equal lines and are neighbours)
//   sr_write_kernel    the bytes, as row_text.hip does for PAF rows
// Integer work, one 64-byte row load per thread, no LDS.
#include "sr_overlaps.h"

#include "ava.h"
#include "dev_prims.h"
#include "filter_stage.h"
#include "paf_io.h"

namespace hlmi {

namespace {
constexpr int WG = 256;
inline dim3 grid1(size_t n) { return grid_for(n, WG); }

struct SrTables {
    const uint32_t *num_of_rank;      // name rank (the overlapper's qid / tid) -> rank of the name's NUMBER
    const int64_t *val_of_num;        // numeric rank -> the number
};

__global__ __launch_bounds__(WG) void sr_record_kernel(const PafRec *__restrict__ recs, const uint32_t *__restrict__ idx, size_t n,
                                                       SrTables t, int id_bits, SrRec *__restrict__ out, uint64_t *__restrict__ key,
                                                       uint32_t *__restrict__ perm) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PafRec r = recs[idx[i]];
    SrRowIn in;
    in.qlen = r.qlen; in.qs = r.qs; in.tlen = r.tlen; in.ts = r.ts; in.te = r.te; in.nmatch = r.nmatch; in.blen = r.blen;
    in.rev = (r.flags & PF_REV) ? 1u : 0u;
    in.q_str = r.qid; in.t_str = r.tid;
    in.q_num = t.num_of_rank[r.qid]; in.t_num = t.num_of_rank[r.tid];
    const SrRec o = sr_record(in);
    out[i] = o;
    key[i] = (uint64_t)o.na << id_bits | o.nb;
    perm[i] = (uint32_t)i;
}

// order[first row of the pair + rows of the pair that sort before this one] = this row
__global__ __launch_bounds__(WG) void sr_tie_kernel(const SrRec *__restrict__ recs, const uint64_t *__restrict__ key,
                                                    const uint32_t *__restrict__ perm, size_t n, uint32_t *__restrict__ order) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t k = key[p];
    size_t s = p, e = p + 1;
    while (s > 0 && key[s - 1] == k) --s;
    while (e < n && key[e] == k) ++e;
    const uint32_t me = perm[p];
    if (e - s == 1) { order[p] = me; return; }
    const SrRec mine = recs[me];
    size_t before = 0;
    for (size_t j = s; j < e; ++j) {
        if (j == p) continue;
        const int c = sr_cmp_rec(recs[perm[j]], mine);
        if (c < 0 || (c == 0 && j < p)) ++before;
    }
    order[s + before] = me;
}

// len[p]: bytes of the line at place p with its newline, 0 when it repeats the line before it.  *bad: a row whose shorter
// read would have no bases (sfo.cpp:88 refuses the file).
__global__ __launch_bounds__(WG) void sr_len_kernel(const SrRec *__restrict__ recs, const uint32_t *__restrict__ order, size_t n,
                                                    SrTables t, uint32_t *__restrict__ len, uint32_t *__restrict__ bad) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const SrLine l = sr_line(recs[order[p]]);
    if (l.minlen <= 0) { atomicOr(bad, 1u); len[p] = 0; return; }
    if (p > 0 && sr_line_equal(l, sr_line(recs[order[p - 1]]))) { len[p] = 0; return; }
    // id1 id2 pos1 - - ori1 ori2 perc - ovlen - s s
    len[p] = (uint32_t)(dec_len_signed(t.val_of_num[l.n1]) + dec_len_signed(t.val_of_num[l.n2]) + dec_len_signed(l.pos1) +
                        dec_len_signed(l.perc) + dec_len_signed(l.ovlen)) + 8u /* - - o o - - s s */ + 12u /* TABs */ + 1u;
}

__global__ __launch_bounds__(WG) void sr_write_kernel(const SrRec *__restrict__ recs, const uint32_t *__restrict__ order, size_t n,
                                                      SrTables t, const uint32_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                      char *__restrict__ text) {
    const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (p >= n || !len[p]) return;
    const SrLine l = sr_line(recs[order[p]]);
    char *q = text + off[p];
    q = put_dec_signed(q, t.val_of_num[l.n1]); *q++ = '\t';
    q = put_dec_signed(q, t.val_of_num[l.n2]); *q++ = '\t';
    q = put_dec_signed(q, l.pos1); *q++ = '\t';
    *q++ = '-'; *q++ = '\t'; *q++ = '-'; *q++ = '\t';
    *q++ = l.ori1; *q++ = '\t'; *q++ = l.ori2; *q++ = '\t';
    q = put_dec_signed(q, l.perc); *q++ = '\t';
    *q++ = '-'; *q++ = '\t';
    q = put_dec_signed(q, l.ovlen); *q++ = '\t';
    *q++ = '-'; *q++ = '\t'; *q++ = 's'; *q++ = '\t'; *q++ = 's'; *q++ = '\n';
}

// a read name as the number sfo2overlaps reads from it: decimal digits only, below 10^18
int64_t name_number(const std::string &s, const char *path) {
    if (s.empty() || s.size() > 18) fail(HLMI_EINVAL, "hlmi_sr_overlaps: %s: read name '%s' is no decimal integer below 10^18", path, s.c_str());
    int64_t v = 0;
    for (const char c : s) {
        if (c < '0' || c > '9') fail(HLMI_EINVAL, "hlmi_sr_overlaps: %s: read name '%s' is no decimal integer", path, s.c_str());
        v = v * 10 + (c - '0');
    }
    return v;
}
}  // namespace

void sr_overlaps_run(const char *reads, int min_ovlp_len, double min_identity, int o, double r, const char *out_overlaps,
                     uint64_t *n_lines) {
    stat_reset();
    *n_lines = 0;
    SeqSet S;
    read_seqs(reads, S);
    const size_t n = S.size();
    // ---- the names: numbers, each once (before anything is written) -------------------------------------------------------------
    std::vector<int64_t> val(n);
    for (size_t i = 0; i < n; ++i) val[i] = name_number(S.names[i], reads);
    std::vector<uint32_t> by_num(n);
    for (size_t i = 0; i < n; ++i) by_num[i] = (uint32_t)i;
    std::sort(by_num.begin(), by_num.end(), [&](uint32_t a, uint32_t b) { return val[a] < val[b]; });
    for (size_t i = 1; i < n; ++i)
        if (val[by_num[i]] == val[by_num[i - 1]])
            fail(HLMI_EINVAL, "hlmi_sr_overlaps: %s: two reads are named %lld", reads, (long long)val[by_num[i]]);
    if (n < 2) { write_file(out_overlaps, "", 0); return; }

    // ---- the overlapper, as ava_files runs it with driver.contig_ava_opts() -----------------------------------------------------
    hlmi_ava_opts ao = ava_opts_short();
    ao.pair_once = 1;                  // -X
    ao.bandwidth = 0;                  // -r 0
    std::vector<uint32_t> rt, rq;
    std::vector<std::string> name_of_rank;
    name_ranks(S.names, S.names, rt, rq, name_of_rank);
    const size_t n_ranks = name_of_rank.size();
    std::vector<uint32_t> num_of_rank(n_ranks, 0);
    std::vector<int64_t> val_of_num(n);
    for (size_t k = 0; k < n; ++k) { val_of_num[k] = val[by_num[k]]; num_of_rank[rq[by_num[k]]] = (uint32_t)k; }
    DevReads dR;
    upload_reads(S, 0, n, dR);
    DBuf<uint32_t> d_rank, d_chunk(n);
    d_rank.upload(rq);
    d_chunk.zero();
    DevSketch qsk;
    sketch_device(dR, ao.k, ao.w, ao.hpc, 0, qsk);
    const std::vector<uint32_t> qc = qsk.counts.download(n);
    AvaInput in;
    in.T = &dR; in.Q = &dR; in.d_rank_t = d_rank.p; in.d_rank_q = d_rank.p; in.d_chunk_of_t = d_chunk.p; in.n_chunks = 1;
    in.n_ranks = n_ranks;
    in.d_qmz = qsk.mz.p;
    in.qmz_off.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) in.qmz_off[i + 1] = in.qmz_off[i] + qc[i];
    AvaRows rows;
    ava_device(in, ao, rows);
    const size_t R = rows.n_rows;
    stat_set("sr_rows_raw", (double)R);
    if (!R) { write_file(out_overlaps, "", 0); return; }
    if (R >= (1ull << 32)) fail(HLMI_EINVAL, "hlmi_sr_overlaps: %zu overlapper rows (2^32 and more)", R);

    // ---- filter_ovlp_inline.py on the rows where they are -----------------------------------------------------------------------
    DBuf<uint8_t> keep(R);
    DBuf<uint32_t> first_of(R), idx(R);
    ovlp_inline_device(rows.recs.p, R, min_ovlp_len, min_identity, o, r, keep.p, first_of.p);
    first_of.release();
    const size_t K = select_flagged_indices(keep.p, idx.p, R);
    keep.release();
    stat_set("sr_rows_kept", (double)K);
    if (!K) { write_file(out_overlaps, "", 0); return; }

    // ---- PAF row -> SFO -> SAVAGE record, sort / uniq, text ---------------------------------------------------------------------
    DBuf<uint32_t> d_num_of_rank;
    DBuf<int64_t> d_val_of_num;
    d_num_of_rank.upload(num_of_rank);
    d_val_of_num.upload(val_of_num);
    const SrTables tb{d_num_of_rank.p, d_val_of_num.p};
    const int id_bits = bits_for(n - 1);                       // two numeric ranks in one key: n < 2^32
    DBuf<SrRec> recs(K);
    DBuf<uint64_t> key(K), off(K);
    DBuf<uint32_t> perm(K), order(K), len(K), bad(1);
    bad.zero();
    {
        KTimer kt("sr_overlaps");
        hipLaunchKernelGGL(sr_record_kernel, grid1(K), dim3(WG), 0, stream(), rows.recs.p, idx.p, K, tb, id_bits, recs.p, key.p, perm.p);
        sort_pairs_u64_u32(key.p, perm.p, K, 0, 2 * id_bits);
        hipLaunchKernelGGL(sr_tie_kernel, grid1(K), dim3(WG), 0, stream(), recs.p, key.p, perm.p, K, order.p);
        hipLaunchKernelGGL(sr_len_kernel, grid1(K), dim3(WG), 0, stream(), recs.p, order.p, K, tb, len.p, bad.p);
        exclusive_scan_u32_to_u64(len.p, off.p, K);
    }
    HIP_CHECK(hipGetLastError());
    if (download_one(bad.p)) fail(HLMI_EINVAL, "sfo2overlaps: non-positive read length");
    const uint64_t total = download_one(off.p + (K - 1)) + download_one(len.p + (K - 1));
    std::string text(total, '\0');
    if (total) {
        DBuf<char> d_text(total);
        {
            KTimer kt("sr_overlaps");
            hipLaunchKernelGGL(sr_write_kernel, grid1(K), dim3(WG), 0, stream(), recs.p, order.p, K, tb, len.p, off.p, d_text.p);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&text[0], d_text.p, total, hipMemcpyDeviceToHost, stream()));
        sync();
    }
    *n_lines = (uint64_t)std::count(text.begin(), text.end(), '\n');
    write_file(out_overlaps, text.data(), text.size());
    stat_set("sr_lines", (double)*n_lines);
}

}  // namespace hlmi
