// capi.cpp - the extern "C" boundary of libhylight_mi.so (include/hylight_mi.h).
#include <charconv>
#include <chrono>

#include "ava.h"
#include "common.h"
#include "depth_internal.h"
#include "filter_stage.h"
#include "graph.h"
#include "paf_io.h"
#include "polish_internal.h"
#include "stage.h"
#include "textpass.h"
#include "haplotigs_internal.h"
#include "phase_internal.h"
#include "variants_internal.h"
#include "vq_internal.h"

namespace hlmi {
void init_device(int device, int threads);
void cluster_run(const char *paf, const char *fastq, const hlmi_cluster_opts &o, const char *out_dir, hlmi_cluster_stats *st);
void sr_overlaps_run(const char *reads, int min_ovlp_len, double min_identity, int o, double r, const char *out_overlaps,
                     uint64_t *n_lines);
void shutdown_device();
const std::string &last_error();
}  // namespace hlmi

using namespace hlmi;

namespace {
template <typename F>
int guarded(F &&f) {
    try {
        hooks_refresh();         // test hooks / tuning switches of this call (the one place the environment is read)
        f();
        ktimer_flush();          // kernel timers of this call end here: none leaks into the next call's statistics
        return HLMI_OK;
    } catch (const Error &e) {
        ktimer_discard();
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        ktimer_discard();
        set_last_error("out of host memory");
        return HLMI_ENOMEM;
    } catch (const std::exception &e) {
        ktimer_discard();
        set_last_error(e.what());
        return HLMI_EINVAL;
    }
}

std::string py_float_repr(double v) {   // Python str(float) for the magnitudes that occur here
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v);
    std::string s(buf, r.ptr);
    if (s.find('.') == std::string::npos && s.find('e') == std::string::npos && s.find("inf") == std::string::npos &&
        s.find("nan") == std::string::npos)
        s += ".0";
    return s;
}
}  // namespace

extern "C" {

int hlmi_init(int device, int host_threads) {
    return guarded([&] { init_device(device, host_threads); });
}
int hlmi_abi_version(void) { return HLMI_ABI_VERSION; }
void hlmi_shutdown(void) { shutdown_device(); }
const char *hlmi_last_error(void) { return last_error().c_str(); }
const char *hlmi_version(void) { return "hylight-mi355x 0.1 (gfx950)"; }

int hlmi_filter_chunk(const char *paf_in, const char *out_paf, int len_over, int mc, double iden, double thre,
                      int min_o, int long_mode) {
    return guarded([&] {
        if (!paf_in || !out_paf) fail(HLMI_EINVAL, "hlmi_filter_chunk: NULL path");
        require_device();
        stat_reset();
        PafText pt;
        read_paf(paf_in, pt, true);
        DBuf<PafRec> d_recs;
        DBuf<uint32_t> d_ops;
        d_recs.upload(pt.recs);
        d_ops.upload(pt.ops.data(), pt.ops.size());
        if (pt.ops.empty()) d_ops.alloc(1);
        FilterCfg cfg;
        cfg.len_over = len_over; cfg.mc = mc; cfg.thre = thre; cfg.min_o = min_o; cfg.long_mode = long_mode != 0;
        FilterOut fo;
        filter_stage_device(d_recs.p, pt.recs.size(), d_ops.p, {0, (uint64_t)pt.recs.size()}, cfg, fo);
        std::vector<std::string> lines;
        std::string s;
        for (size_t i = 0; i < fo.rows.size(); ++i) {
            const PafRec &r = pt.recs[fo.rows[i]];
            if (format_scored_row(r, pt.dict.names[r.qid], pt.dict.names[r.tid], fo.x_digit_sum[i], iden, s))
                lines.push_back(s);
        }
        write_lines(out_paf, lines);
        stat_set("rows_in", (double)pt.recs.size());
        stat_set("rows_after_v4", (double)fo.n_after_v4);
        stat_set("snp_events", (double)fo.n_events);
        stat_set("pairs", (double)fo.n_pairs);
        stat_set("rows_out", (double)lines.size());
    });
}

int hlmi_paf_window_filter(int variant, int min_len, double min_iden, int min_o, int sfo, const char *in_paf,
                           const char *out_path) {
    return guarded([&] {
        if (!in_paf || !out_path) fail(HLMI_EINVAL, "hlmi_paf_window_filter: NULL path");
        if (variant != 3 && variant != 4) fail(HLMI_EINVAL, "variant must be 3 or 4");
        require_device();
        if (min_iden < 0) min_iden = variant == 4 ? 0.6 : 0.8;
        PafText pt;
        read_paf(in_paf, pt, false);
        size_t n = pt.recs.size();
        std::vector<std::string> lines;
        if (n) {
            DBuf<PafRec> d_recs;
            d_recs.upload(pt.recs);
            DBuf<uint8_t> keep(n);
            window_filter_device(d_recs.p, n, {0, (uint64_t)n}, variant, min_len, min_iden, min_o, keep.p);
            std::vector<uint8_t> hk = keep.download(n);
            for (size_t i = 0; i < n; ++i) {
                if (!hk[i]) continue;
                if (variant == 4) {
                    lines.emplace_back(pt.line(i));
                    continue;
                }
                const PafRec &r = pt.recs[i];
                const std::string &q = pt.dict.names[r.qid], &t = pt.dict.names[r.tid];
                if (sfo) {   // filter_trans_ovlp_inline_v3.py:83-102
                    int64_t ql = r.qlen, qs = r.qs, tl = r.tlen, ts = r.ts, te = r.te, oha, ohb;
                    bool rev = r.flags & PF_REV;
                    if (!rev) { oha = qs - ts; ohb = tl - ts - (ql - qs); }
                    else { oha = qs - (tl - te); ohb = te - (ql - qs); }
                    int64_t ola = oha >= 0 ? std::min(ql - oha, tl) : std::min(tl + oha, ql);
                    char buf[160];
                    snprintf(buf, sizeof buf, "\t%c\t%lld\t%lld\t%lld\t%lld\t%lld", rev ? 'I' : 'N', (long long)oha,
                             (long long)ohb, (long long)ola, (long long)ola, (long long)r.blen - (long long)r.nmatch);
                    lines.push_back(q + "\t" + t + buf);
                } else {     // filter_trans_ovlp_inline_v3.py:79
                    double mlen = (double)((uint64_t)r.qlen + r.tlen) / 2.0;
                    double a = 0.1 * ((double)r.blen / mlen), b = 0.9 * ((double)r.nmatch / (double)r.blen);
                    lines.push_back(q + "\t" + t + "\t" + py_float_repr(a + b));
                }
            }
        }
        write_lines(out_path, lines);
    });
}

int hlmi_filter_ovlp_inline(const char *in_paf, const char *out_paf, int min_ovlp_len, double min_identity, int o, double r) {
    return guarded([&] {
        if (!in_paf || !out_paf) fail(HLMI_EINVAL, "hlmi_filter_ovlp_inline: NULL path");
        require_device();
        PafText pt;
        read_paf(in_paf, pt, false);
        const size_t n = pt.recs.size();
        std::vector<std::string> lines;
        if (n) {
            DBuf<PafRec> d_recs;
            d_recs.upload(pt.recs);
            DBuf<uint8_t> keep(n);
            DBuf<uint32_t> first_of(n);
            ovlp_inline_device(d_recs.p, n, min_ovlp_len, min_identity, o, r, keep.p, first_of.p);
            std::vector<uint8_t> hk = keep.download(n);
            std::vector<uint32_t> hf = first_of.download(n);
            std::vector<std::pair<uint32_t, uint32_t>> order;      // (print position, row)
            for (size_t i = 0; i < n; ++i) if (hk[i]) order.emplace_back(hf[i], (uint32_t)i);
            std::sort(order.begin(), order.end());
            for (auto &pr : order) lines.emplace_back(pt.line(pr.second));
        }
        write_lines(out_paf, lines);
    });
}

int hlmi_filter_non_atcg(const char *fastx, const char *out_fa, int is_fastq) {
    return guarded([&] {
        if (!fastx || !out_fa) fail(HLMI_EINVAL, "hlmi_filter_non_atcg: NULL path");
        filter_non_atcg_run(fastx, out_fa, is_fastq != 0);
    });
}

int hlmi_gfa2fa(const char *gfa, const char *out_fa) {
    return guarded([&] {
        if (!gfa || !out_fa) fail(HLMI_EINVAL, "hlmi_gfa2fa: NULL path");
        gfa2fa_run(gfa, out_fa);
    });
}

int hlmi_pick_up(const char *ovlap_paf, const char *fastx, const char *out_fastx, int is_fastq) {
    return guarded([&] {
        if (!ovlap_paf || !fastx || !out_fastx) fail(HLMI_EINVAL, "hlmi_pick_up: NULL path");
        pick_up_run(ovlap_paf, fastx, out_fastx, is_fastq != 0);
    });
}

int hlmi_minimap22sfo(const char *in_paf, const char *out_sfo, int min_overlap_len, double min_pident) {
    return guarded([&] {                                         // script/minimap22sfo.py:28-75 - a text converter
        if (!in_paf || !out_sfo) fail(HLMI_EINVAL, "hlmi_minimap22sfo: NULL path");
        PafText pt;
        read_paf(in_paf, pt, false);
        std::vector<std::string> lines;
        for (const PafRec &rc : pt.recs) {
            if ((int64_t)rc.blen < (int64_t)min_overlap_len) continue;
            if ((double)rc.nmatch / (double)rc.blen < min_pident / 100.0) continue;
            const bool rev = rc.flags & PF_REV;
            int64_t ql = rc.qlen, qs = rc.qs, tl = rc.tlen, ts = rc.ts, te = rc.te, oha, ohb;
            if (!rev) { oha = qs - ts; ohb = tl - ts - (ql - qs); }
            else { oha = qs - (tl - te); ohb = te - (ql - qs); }
            const int64_t ola = oha >= 0 ? std::min(ql - oha, tl) : std::min(tl + oha, ql);
            const std::string *a = &pt.dict.names[rc.qid], *b = &pt.dict.names[rc.tid];
            if (*a > *b) {                                       // ids in string order; read A forward
                std::swap(a, b);
                if (!rev) { oha = -oha; ohb = -ohb; } else std::swap(oha, ohb);
            }
            char buf[160];
            snprintf(buf, sizeof buf, "\t%c\t%lld\t%lld\t%lld\t%lld\t%lld", rev ? 'I' : 'N', (long long)oha, (long long)ohb,
                     (long long)ola, (long long)ola, (long long)rc.blen - (long long)rc.nmatch);
            lines.push_back(*a + "\t" + *b + buf);
        }
        write_lines(out_sfo, lines);
    });
}

int hlmi_merge_scored_paf(const char *const *in_pafs, int n_in, const char *out_paf) {
    return guarded([&] {
        std::vector<std::string> data((size_t)n_in);         // the parts stay whole, the lines are views into them
        std::vector<std::string_view> lines;
        for (int i = 0; i < n_in; ++i) {
            data[(size_t)i] = read_file(in_pafs[i]);
            const std::string &d = data[(size_t)i];
            size_t pos = 0;
            while (pos < d.size()) {
                size_t e = d.find('\n', pos);
                if (e == std::string::npos) e = d.size();
                lines.emplace_back(d.data() + pos, e - pos);
                pos = e + 1;
            }
        }
        sort_scored_lines(lines);
        write_lines(out_paf, lines);
    });
}

int hlmi_split_reads2(const char *reads_fa, const char *ref_fa, int nsplit, const char *out_dir, const char *out_paf,
                      int threads, int len_over, int mc, double iden, int long_mode) {
    return hlmi_split_reads2_shard(reads_fa, ref_fa, nsplit, out_dir, out_paf, threads, len_over, mc, iden, long_mode,
                                   0, 1);
}

int hlmi_split_reads2_shard(const char *reads_fa, const char *ref_fa, int nsplit, const char *out_dir,
                            const char *out_paf, int threads, int len_over, int mc, double iden, int long_mode,
                            int rank, int world) {
    (void)out_dir; (void)threads;
    return guarded([&] {
        if (!reads_fa || !ref_fa || !out_paf) fail(HLMI_EINVAL, "hlmi_split_reads2: NULL path");
        if (nsplit < 1 || world < 1 || rank < 0 || rank >= world) fail(HLMI_EINVAL, "bad nsplit/rank/world");
        require_device();
        Job job(reads_fa, ref_fa, nsplit, long_mode != 0);
        job.sketch_all_queries();
        job.run(rank, world, len_over, mc, iden, out_paf);
    });
}

void hlmi_ava_opts_long(hlmi_ava_opts *o) {
    if (!o) return;
    *o = ava_opts_long();
}
void hlmi_ava_opts_short(hlmi_ava_opts *o) {
    if (!o) return;
    *o = ava_opts_short();
}

int hlmi_ava(const char *target_fa, const char *query_fa, const hlmi_ava_opts *opts, const char *out_paf) {
    return guarded([&] {
        if (!target_fa || !query_fa || !out_paf) fail(HLMI_EINVAL, "hlmi_ava: NULL path");
        require_device();
        hlmi_ava_opts o = opts ? *opts : ava_opts_long();
        ava_files(target_fa, query_fa, o, out_paf);
    });
}

int hlmi_miniasm(const char *paf, const char *reads_fa, int bub_dist, int n_rounds_arg, int max_ext, int min_dp,
                 const char *outfmt, const char *out_path) {
    return guarded([&] {
        if (!paf || !out_path) fail(HLMI_EINVAL, "hlmi_miniasm: NULL path");
        require_device();
        miniasm_run(paf, reads_fa, bub_dist, n_rounds_arg, max_ext, min_dp, outfmt ? outfmt : "ug", out_path);
    });
}

int hlmi_sfo2overlaps(const char *in_sfo, const char *out_savage, int num_singles, int num_pairs) {
    return guarded([&] {
        if (!in_sfo || !out_savage) fail(HLMI_EINVAL, "hlmi_sfo2overlaps: NULL path");
        sfo2overlaps_run(in_sfo, out_savage, num_singles, num_pairs);
    });
}

int hlmi_sr_overlaps(const char *reads, int min_ovlp_len, double min_identity, int o, double r, const char *out_overlaps,
                     uint64_t *n_lines) {
    return guarded([&] {
        if (!reads || !out_overlaps || !n_lines) fail(HLMI_EINVAL, "hlmi_sr_overlaps: NULL argument");
        require_device();
        sr_overlaps_run(reads, min_ovlp_len, min_identity, o, r, out_overlaps, n_lines);
    });
}

int hlmi_vq_parse_overlaps(const char *savage_path, uint32_t min_overlap_len, uint32_t min_overlap_perc, int relax_pe,
                           uint64_t max_overlaps, hlmi_vq_overlap *out, uint64_t cap, uint64_t *n_out,
                           uint64_t *n_nonedge, uint64_t *n_skipped) {
    return guarded([&] {
        if (!savage_path || !n_out || !n_nonedge || !n_skipped || (cap && !out)) fail(HLMI_EINVAL, "hlmi_vq_parse_overlaps: NULL argument");
        vq_parse_overlaps(savage_path, min_overlap_len, min_overlap_perc, relax_pe, max_overlaps, out, cap, n_out, n_nonedge, n_skipped);
    });
}

int hlmi_vq_transitive_edges(uint32_t n_vertices, uint64_t n_edges, const uint32_t *src, const uint32_t *dst,
                             const uint32_t *ovlen, int remove_trans, uint8_t *flags, uint64_t *n_transitive) {
    return guarded([&] {
        if (!n_transitive || (n_edges && (!src || !dst || !flags))) fail(HLMI_EINVAL, "hlmi_vq_transitive_edges: NULL argument");
        require_device();
        vq_transitive_edges(n_vertices, n_edges, src, dst, ovlen, remove_trans, flags, n_transitive);
    });
}

int hlmi_vq_overlap_scores(const char *fastq_singles, const hlmi_vq_overlap *ov, uint64_t n, double mismatch,
                           uint32_t min_read_len, double *score, double *mismatch_rate, int64_t *pos3) {
    return guarded([&] {
        if (!fastq_singles || (n && (!ov || !score || !mismatch_rate || !pos3))) fail(HLMI_EINVAL, "hlmi_vq_overlap_scores: NULL argument");
        require_device();
        vq_overlap_scores(fastq_singles, ov, n, mismatch, min_read_len, score, mismatch_rate, pos3);
    });
}

void hlmi_vq_graph_opts_stageb(hlmi_vq_graph_opts *o) {
    if (o) vq_graph_opts_stageb(o);
}

int hlmi_vq_graph(const char *singles_fastq, const char *overlaps, const hlmi_vq_graph_opts *o, const char *out_dir,
                  hlmi_vq_graph_stats *st) {
    return guarded([&] {
        if (!singles_fastq || !overlaps || !o || !out_dir || !st) fail(HLMI_EINVAL, "hlmi_vq_graph: NULL argument");
        require_device();
        vq_graph_run(singles_fastq, overlaps, *o, out_dir, st);
    });
}

void hlmi_vq_merge_opts_stageb(hlmi_vq_merge_opts *o) {
    if (o) vq_merge_opts_stageb(o);
}

int hlmi_vq_merge_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                     const hlmi_vq_merge_opts *mo, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                     hlmi_vq_merge_stats *mst) {
    return guarded([&] {
        if (!singles_fastq || !overlaps || !go || !mo || !out_dir || !gst || !mst) fail(HLMI_EINVAL, "hlmi_vq_merge: NULL argument");
        require_device();
        vq_merge_run(singles_fastq, overlaps, subreads_in, *go, *mo, min_qual, out_dir, gst, mst);
    });
}

int hlmi_vq_merge(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                  const hlmi_vq_merge_opts *mo, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst) {
    return hlmi_vq_merge_mq(singles_fastq, overlaps, subreads_in, go, mo, VQ_MIN_QUAL, out_dir, gst, mst);
}

void hlmi_vq_next_opts_stageb(hlmi_vq_next_opts *o) {
    if (o) vq_next_opts_stageb(o);
}

int hlmi_vq_iteration_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                         const hlmi_vq_merge_opts *mo, const hlmi_vq_next_opts *no, double min_qual, const char *out_dir,
                         hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst) {
    return guarded([&] {
        if (!singles_fastq || !overlaps || !go || !mo || !no || !out_dir || !gst || !mst || !nst)
            fail(HLMI_EINVAL, "hlmi_vq_iteration: NULL argument");
        require_device();
        vq_iteration_run(singles_fastq, overlaps, subreads_in, *go, *mo, *no, min_qual, out_dir, gst, mst, nst);
    });
}

int hlmi_vq_iteration(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                      const hlmi_vq_merge_opts *mo, const hlmi_vq_next_opts *no, const char *out_dir, hlmi_vq_graph_stats *gst,
                      hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst) {
    return hlmi_vq_iteration_mq(singles_fastq, overlaps, subreads_in, go, mo, no, VQ_MIN_QUAL, out_dir, gst, mst, nst);
}

int hlmi_vq_consensus_pair_mq(const char *seq1, const char *qual1, uint32_t len1, uint32_t qlen1, const char *seq2,
                              const char *qual2, uint32_t len2, uint32_t qlen2, uint32_t pos, double min_qual, char *out_seq,
                              char *out_qual, uint32_t *out_len) {
    return guarded([&] {
        if (!out_len || (len1 && !seq1) || (qlen1 && !qual1) || (len2 && !seq2) || (qlen2 && !qual2) || !out_seq || !out_qual)
            fail(HLMI_EINVAL, "hlmi_vq_consensus_pair: NULL argument");
        require_device();
        vq_consensus_pair(seq1, qual1, len1, qlen1, seq2, qual2, len2, qlen2, pos, min_qual, out_seq, out_qual, out_len);
    });
}

int hlmi_vq_consensus_pair(const char *seq1, const char *qual1, uint32_t len1, uint32_t qlen1, const char *seq2,
                           const char *qual2, uint32_t len2, uint32_t qlen2, uint32_t pos, char *out_seq, char *out_qual,
                           uint32_t *out_len) {
    return hlmi_vq_consensus_pair_mq(seq1, qual1, len1, qlen1, seq2, qual2, len2, qlen2, pos, VQ_MIN_QUAL, out_seq, out_qual, out_len);
}

void hlmi_vq_clique_opts_polyte(hlmi_vq_clique_opts *o, int error_correction) {
    if (o) vq_clique_opts_polyte(o, error_correction);
}

int hlmi_vq_cliques_of_graph(const char *graph_txt, const char *cliques_out, uint64_t *n_cliques) {
    return guarded([&] {                                       // host code: no device is asked for
        if (!graph_txt || !cliques_out || !n_cliques) fail(HLMI_EINVAL, "hlmi_vq_cliques_of_graph: NULL argument");
        vq_cliques_of_graph(graph_txt, cliques_out, n_cliques);
    });
}

int hlmi_vq_cliques_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                       const hlmi_vq_clique_opts *co, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                       hlmi_vq_clique_stats *cst) {
    return guarded([&] {
        if (!singles_fastq || !overlaps || !go || !co || !out_dir || !gst || !cst) fail(HLMI_EINVAL, "hlmi_vq_cliques: NULL argument");
        require_device();
        vq_cliques_run(singles_fastq, overlaps, subreads_in, *go, *co, min_qual, out_dir, gst, cst);
    });
}

int hlmi_vq_cliques(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                    const hlmi_vq_clique_opts *co, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst) {
    return hlmi_vq_cliques_mq(singles_fastq, overlaps, subreads_in, go, co, VQ_MIN_QUAL, out_dir, gst, cst);
}

int hlmi_vq_clique_iteration_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in,
                                const hlmi_vq_graph_opts *go, const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no,
                                double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst,
                                hlmi_vq_clique_next_stats *nst) {
    return guarded([&] {
        if (!singles_fastq || !overlaps || !go || !co || !no || !out_dir || !gst || !cst || !nst)
            fail(HLMI_EINVAL, "hlmi_vq_clique_iteration: NULL argument");
        require_device();
        vq_clique_iteration_run(singles_fastq, overlaps, subreads_in, *go, *co, *no, min_qual, out_dir, gst, cst, nst);
    });
}

int hlmi_vq_clique_iteration(const char *singles_fastq, const char *overlaps, const char *subreads_in,
                             const hlmi_vq_graph_opts *go, const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no,
                             const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst,
                             hlmi_vq_clique_next_stats *nst) {
    return hlmi_vq_clique_iteration_mq(singles_fastq, overlaps, subreads_in, go, co, no, VQ_MIN_QUAL, out_dir, gst, cst, nst);
}

void hlmi_vq_branch_opts_polyte(hlmi_vq_branch_opts *o) {
    if (o) vq_branch_opts_polyte(o);
}

int hlmi_vq_branch_graph(const char *singles_fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                         const char *threshold_table, const hlmi_vq_graph_opts *go, const hlmi_vq_branch_opts *bo,
                         const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_branch_stats *bst) {
    return guarded([&] {
        if (!singles_fastq || !overlaps || !original_fastq || !threshold_table || !go || !bo || !out_dir || !gst || !bst)
            fail(HLMI_EINVAL, "hlmi_vq_branch_graph: NULL argument");
        require_device();
        vq_branch_graph_run(singles_fastq, overlaps, subreads_in, original_fastq, threshold_table, *go, *bo, out_dir, gst, bst);
    });
}

int hlmi_vq_branch_iteration_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                                const char *threshold_table, const hlmi_vq_graph_opts *go, const hlmi_vq_branch_opts *bo,
                                const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no, double min_qual, const char *out_dir,
                                hlmi_vq_graph_stats *gst, hlmi_vq_branch_stats *bst, hlmi_vq_clique_stats *cst,
                                hlmi_vq_clique_next_stats *nst) {
    return guarded([&] {
        if (!singles_fastq || !overlaps || !original_fastq || !threshold_table || !go || !bo || !co || !no || !out_dir || !gst || !bst ||
            !cst || !nst)
            fail(HLMI_EINVAL, "hlmi_vq_branch_iteration: NULL argument");
        require_device();
        vq_branch_iteration_run(singles_fastq, overlaps, subreads_in, original_fastq, threshold_table, *go, *bo, *co, *no, min_qual,
                                out_dir, gst, bst, cst, nst);
    });
}

int hlmi_vq_branch_iteration(const char *singles_fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                             const char *threshold_table, const hlmi_vq_graph_opts *go, const hlmi_vq_branch_opts *bo,
                             const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no, const char *out_dir,
                             hlmi_vq_graph_stats *gst, hlmi_vq_branch_stats *bst, hlmi_vq_clique_stats *cst,
                             hlmi_vq_clique_next_stats *nst) {
    return hlmi_vq_branch_iteration_mq(singles_fastq, overlaps, subreads_in, original_fastq, threshold_table, go, bo, co, no, VQ_MIN_QUAL,
                                       out_dir, gst, bst, cst, nst);
}

void hlmi_cluster_opts_default(hlmi_cluster_opts *o) {
    if (o) *o = hlmi_cluster_opts{15000, 20, 0, 0};            // HyLight.py --size, -t
}

int hlmi_cluster_short(const char *paf, const char *fastq, const hlmi_cluster_opts *o, const char *out_dir,
                       hlmi_cluster_stats *st) {
    return guarded([&] {
        if (!paf || !fastq || !o || !out_dir || !st) fail(HLMI_EINVAL, "hlmi_cluster_short: NULL argument");
        require_device();
        cluster_run(paf, fastq, *o, out_dir, st);
    });
}

void hlmi_polish_opts_default(hlmi_polish_opts *o) {
    if (o) *o = hlmi_polish_opts{0, 0.0, 3, 1};
}

int hlmi_polish(const char *contigs, const char *reads, const char *paf, const hlmi_polish_opts *o, const char *out_fa,
                hlmi_polish_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_polish: NULL argument");
        require_device();
        polish_run(contigs, reads, paf, *o, out_fa, st);
    });
}

int hlmi_polish_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_opts *po,
                      const char *out_fa, hlmi_polish_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !po || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_polish_reads: NULL argument");
        require_device();
        polish_reads_run(contigs, reads, ao ? *ao : ava_opts_long(), *po, out_fa, st);
    });
}

void hlmi_polish_qopts_default(hlmi_polish_qopts *o) {
    if (o) *o = hlmi_polish_qopts{0, 0.0, 3, 1, 1, 10.0};
}

namespace {
hlmi_polish_opts polish_base_opts(const hlmi_polish_qopts &q) { return hlmi_polish_opts{q.min_len, q.min_iden, q.min_cov, q.include_unpolished}; }

// what the _q and _pairs calls hand polish_run / polish_reads_run, and how it comes back
struct PairsCall {
    pol::PolQualCall qc;
    pol::PolPairCall pc;
    PairsCall(const hlmi_polish_qopts &o, const char *pairs_paf) {
        qc.qual_weight = o.qual_weight != 0;
        qc.min_avg_qual = o.min_avg_qual;
        pc.path = pairs_paf;
    }
    pol::PolPairCall *list() { return pc.path ? &pc : nullptr; }      // no list: the _q call
    void to(hlmi_polish_qstats *st) const {
        st->reads_with_qual = qc.reads_with_qual;
        st->rows_low_qual = qc.rows_low_qual;
    }
    void to(hlmi_polish_pstats *st) const {
        to(&st->q);
        st->pairs_listed = pc.pairs_listed;
        st->pairs_unknown = pc.pairs_unknown;
        st->rows_not_listed = pc.rows_not_listed;
    }
};
}  // namespace

int hlmi_polish_q(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, const char *out_fa,
                  hlmi_polish_qstats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_polish_q: NULL argument");
        require_device();
        *st = hlmi_polish_qstats{};
        PairsCall c(*o, nullptr);
        polish_run(contigs, reads, paf, polish_base_opts(*o), out_fa, &st->base, &c.qc);
        c.to(st);
    });
}

int hlmi_polish_reads_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_qopts *po,
                        const char *out_fa, hlmi_polish_qstats *st) {
    return guarded([&] {
        if (!contigs || !reads || !po || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_polish_reads_q: NULL argument");
        require_device();
        *st = hlmi_polish_qstats{};
        PairsCall c(*po, nullptr);
        polish_reads_run(contigs, reads, ao ? *ao : ava_opts_long(), polish_base_opts(*po), out_fa, &st->base, &c.qc);
        c.to(st);
    });
}

int hlmi_polish_pairs(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, const char *pairs_paf,
                      const char *out_fa, hlmi_polish_pstats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_polish_pairs: NULL argument");
        require_device();
        *st = hlmi_polish_pstats{};
        PairsCall c(*o, pairs_paf);
        polish_run(contigs, reads, paf, polish_base_opts(*o), out_fa, &st->q.base, &c.qc, c.list());
        c.to(st);
    });
}

int hlmi_polish_reads_pairs(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_qopts *po,
                            const char *pairs_paf, const char *out_fa, hlmi_polish_pstats *st) {
    return guarded([&] {
        if (!contigs || !reads || !po || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_polish_reads_pairs: NULL argument");
        require_device();
        *st = hlmi_polish_pstats{};
        PairsCall c(*po, pairs_paf);
        polish_reads_run(contigs, reads, ao ? *ao : ava_opts_long(), polish_base_opts(*po), out_fa, &st->q.base, &c.qc, c.list());
        c.to(st);
    });
}

void hlmi_depth_opts_default(hlmi_depth_opts *o) {
    if (o) *o = hlmi_depth_opts{0, 0.0};
}

int hlmi_depth(const char *contigs, const char *reads, const char *paf, const hlmi_depth_opts *o, const char *pairs_paf,
               const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_tsv || !st) fail(HLMI_EINVAL, "hlmi_depth: NULL argument");
        require_device();
        depth_run(contigs, reads, paf, *o, pairs_paf, out_tsv, out_bedgraph, st);
    });
}

int hlmi_depth_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_depth_opts *o,
                     const char *pairs_paf, const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_tsv || !st) fail(HLMI_EINVAL, "hlmi_depth_reads: NULL argument");
        require_device();
        depth_reads_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, pairs_paf, out_tsv, out_bedgraph, st);
    });
}

void hlmi_variant_opts_default(hlmi_variant_opts *o) {
    if (o) *o = hlmi_variant_opts{0, 0.0, 3, 2, 0.2};
}

int hlmi_variants(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, const char *pairs_paf,
                  const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_variants: NULL argument");
        require_device();
        variants_run(contigs, reads, paf, *o, pairs_paf, out_sites, out_summary, st);
    });
}

int hlmi_variants_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o,
                        const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_variants_reads: NULL argument");
        require_device();
        variants_reads_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, pairs_paf, out_sites, out_summary, st);
    });
}

int hlmi_variants_ins(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, const char *pairs_paf,
                      const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st) {
    return guarded([&] {
        if (!out_ins) fail(HLMI_EINVAL, "hlmi_variants_ins: out_ins is NULL");
        if (!contigs || !reads || !paf || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_variants_ins: NULL argument");
        require_device();
        variants_ins_run(contigs, reads, paf, *o, pairs_paf, out_sites, out_summary, out_ins, st);
    });
}

int hlmi_variants_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o,
                            const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                            hlmi_variant_ins_stats *st) {
    return guarded([&] {
        if (!out_ins) fail(HLMI_EINVAL, "hlmi_variants_reads_ins: out_ins is NULL");
        if (!contigs || !reads || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_variants_reads_ins: NULL argument");
        require_device();
        variants_reads_ins_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, pairs_paf, out_sites, out_summary, out_ins, st);
    });
}

void hlmi_variant_qopts_default(hlmi_variant_qopts *o) {
    if (o) *o = hlmi_variant_qopts{0, 0.0, 3, 2, 0.2, 10, 10.0};
}

// the _q forms refuse in the header's order: the floors (they need o), then out_ins == NULL (ins), then the other arguments
static void variant_q_arguments(const char *who, const hlmi_variant_qopts *o, bool ins, const char *out_ins, bool others) {
    if (!o) fail(HLMI_EINVAL, "%s: NULL argument", who);
    var::check_variant_qfloors(who, *o);
    if (ins && !out_ins) fail(HLMI_EINVAL, "%s: out_ins is NULL", who);
    if (!others) fail(HLMI_EINVAL, "%s: NULL argument", who);
}

int hlmi_variants_q(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts *o, const char *pairs_paf,
                    const char *out_sites, const char *out_summary, hlmi_variant_stats *st, hlmi_variant_qcounts *qc) {
    return guarded([&] {
        variant_q_arguments("hlmi_variants_q", o, false, nullptr, contigs && reads && paf && out_sites && st && qc);
        require_device();
        variants_q_run(contigs, reads, paf, *o, pairs_paf, out_sites, out_summary, st, qc);
    });
}

int hlmi_variants_reads_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_qopts *o,
                          const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st,
                          hlmi_variant_qcounts *qc) {
    return guarded([&] {
        variant_q_arguments("hlmi_variants_reads_q", o, false, nullptr, contigs && reads && out_sites && st && qc);
        require_device();
        variants_reads_q_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, pairs_paf, out_sites, out_summary, st, qc);
    });
}

int hlmi_variants_ins_q(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts *o, const char *pairs_paf,
                        const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st,
                        hlmi_variant_qcounts *qc) {
    return guarded([&] {
        variant_q_arguments("hlmi_variants_ins_q", o, true, out_ins, contigs && reads && paf && out_sites && st && qc);
        require_device();
        variants_ins_q_run(contigs, reads, paf, *o, pairs_paf, out_sites, out_summary, out_ins, st, qc);
    });
}

int hlmi_variants_reads_ins_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_qopts *o,
                              const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                              hlmi_variant_ins_stats *st, hlmi_variant_qcounts *qc) {
    return guarded([&] {
        variant_q_arguments("hlmi_variants_reads_ins_q", o, true, out_ins, contigs && reads && out_sites && st && qc);
        require_device();
        variants_reads_ins_q_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, pairs_paf, out_sites, out_summary, out_ins, st, qc);
    });
}

void hlmi_phase_opts_default(hlmi_phase_opts *o) {
    if (o) *o = hlmi_phase_opts{0, 0.0, 3, 2, 0.2, 3, 0.8};
}

int hlmi_phase(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, const char *pairs_paf,
               const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_phase: NULL argument");
        require_device();
        phase_run(contigs, reads, paf, *o, pairs_paf, out_sites, out_links, out_reads, st);
    });
}

int hlmi_phase_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_phase_reads: NULL argument");
        require_device();
        phase_reads_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, pairs_paf, out_sites, out_links, out_reads, st);
    });
}

int hlmi_phase_reach(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, int reach, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_reach_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_phase_reach: NULL argument");
        require_device();
        phase_reach_run(contigs, reads, paf, *o, reach, pairs_paf, out_sites, out_links, out_reads, st);
    });
}

int hlmi_phase_reads_reach(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, int reach,
                           const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                           hlmi_phase_reach_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_phase_reads_reach: NULL argument");
        require_device();
        phase_reads_reach_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, reach, pairs_paf, out_sites, out_links, out_reads, st);
    });
}

int hlmi_phase_ins(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, int reach, const char *pairs_paf,
                   const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_ins_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_phase_ins: NULL argument");
        require_device();
        phase_ins_run(contigs, reads, paf, *o, reach, pairs_paf, out_sites, out_links, out_reads, st);
    });
}

int hlmi_phase_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, int reach,
                         const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                         hlmi_phase_ins_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_sites || !st) fail(HLMI_EINVAL, "hlmi_phase_reads_ins: NULL argument");
        require_device();
        phase_reads_ins_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, reach, pairs_paf, out_sites, out_links, out_reads, st);
    });
}

void hlmi_haplotig_opts_default(hlmi_haplotig_opts *o) {
    if (o) *o = hlmi_haplotig_opts{0, 0.0, 3, 2, 0.2, 3, 0.8, 3, 1};
}

int hlmi_haplotigs(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, const char *pairs_paf,
                   const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_haplotigs: NULL argument");
        require_device();
        haplotigs_run(contigs, reads, paf, *o, pairs_paf, out_fa, out_blocks, st);
    });
}

int hlmi_haplotigs_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o,
                         const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_haplotigs_reads: NULL argument");
        require_device();
        haplotigs_reads_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, pairs_paf, out_fa, out_blocks, st);
    });
}

int hlmi_haplotigs_reach(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, int reach,
                         const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_haplotigs_reach: NULL argument");
        require_device();
        haplotigs_reach_run(contigs, reads, paf, *o, reach, pairs_paf, out_fa, out_blocks, st);
    });
}

int hlmi_haplotigs_reads_reach(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o, int reach,
                               const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_haplotigs_reads_reach: NULL argument");
        require_device();
        haplotigs_reads_reach_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, reach, pairs_paf, out_fa, out_blocks, st);
    });
}

int hlmi_haplotigs_ins(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, int reach,
                       const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !paf || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_haplotigs_ins: NULL argument");
        require_device();
        haplotigs_ins_run(contigs, reads, paf, *o, reach, pairs_paf, out_fa, out_blocks, st);
    });
}

int hlmi_haplotigs_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o, int reach,
                             const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st) {
    return guarded([&] {
        if (!contigs || !reads || !o || !out_fa || !st) fail(HLMI_EINVAL, "hlmi_haplotigs_reads_ins: NULL argument");
        require_device();
        haplotigs_reads_ins_run(contigs, reads, ao ? *ao : ava_opts_long(), *o, reach, pairs_paf, out_fa, out_blocks, st);
    });
}

hlmi_job *hlmi_job_open(const char *reads_fa, const char *ref_fa, int nsplit, int long_mode) {
    hlmi_job *j = nullptr;
    guarded([&] {
        if (!reads_fa || !ref_fa || nsplit < 1) fail(HLMI_EINVAL, "hlmi_job_open: bad arguments");
        require_device();
        j = reinterpret_cast<hlmi_job *>(new Job(reads_fa, ref_fa, nsplit, long_mode != 0));
    });
    return j;
}
void hlmi_job_close(hlmi_job *j) { delete reinterpret_cast<Job *>(j); }
int64_t hlmi_job_num_queries(const hlmi_job *j) { return j ? (int64_t) reinterpret_cast<const Job *>(j)->num_queries() : -1; }
int64_t hlmi_job_num_chunks(const hlmi_job *j) { return j ? (int64_t) reinterpret_cast<const Job *>(j)->num_chunks() : -1; }
int64_t hlmi_job_sketch_bound(const hlmi_job *j, int64_t lo, int64_t hi) {
    int64_t v = -1;
    guarded([&] { v = reinterpret_cast<const Job *>(j)->sketch_bound(lo, hi); });
    return v;
}
int hlmi_job_sketch(hlmi_job *j, int64_t lo, int64_t hi, void *dev_mz, int64_t cap, void *dev_counts, int64_t *n_out) {
    return guarded([&] {
        if (!j || !dev_mz || !dev_counts || !n_out) fail(HLMI_EINVAL, "hlmi_job_sketch: NULL argument");
        *n_out = reinterpret_cast<Job *>(j)->sketch_range(lo, hi, dev_mz, cap, dev_counts);
    });
}
int hlmi_job_sketch_own(hlmi_job *j) {
    return guarded([&] {
        if (!j) fail(HLMI_EINVAL, "hlmi_job_sketch_own: NULL job");
        reinterpret_cast<Job *>(j)->sketch_all_queries();
    });
}
int hlmi_job_set_query_sketch(hlmi_job *j, const void *dev_mz, int64_t n, const void *dev_counts) {
    return guarded([&] {
        if (!j || !dev_mz || !dev_counts) fail(HLMI_EINVAL, "hlmi_job_set_query_sketch: NULL argument");
        reinterpret_cast<Job *>(j)->set_query_sketch(dev_mz, n, dev_counts);
    });
}
int hlmi_job_run(hlmi_job *j, int rank, int world, int len_over, int mc, double iden, const char *out_paf) {
    return guarded([&] {
        if (!j || !out_paf || world < 1 || rank < 0 || rank >= world) fail(HLMI_EINVAL, "hlmi_job_run: bad arguments");
        reinterpret_cast<Job *>(j)->run(rank, world, len_over, mc, iden, out_paf);
    });
}

int hlmi_last_stats_json(char *buf, int64_t cap) {
    return guarded([&] {
        std::string s = "{";
        bool first = true;
        for (auto &kv : stats()) {
            char tmp[128];
            snprintf(tmp, sizeof tmp, "%s\"%s\": %.17g", first ? "" : ", ", kv.first.c_str(), kv.second);
            s += tmp;
            first = false;
        }
        s += "}";
        if ((int64_t)s.size() + 1 > cap) fail(HLMI_EINVAL, "stats buffer too small");
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}

}  // extern "C"
