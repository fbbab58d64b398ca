// vq_superread_run.cpp - SRBuilder's drivers (tools/HaploConduct/src), each a sequence over the host pieces of vq_superread.cpp:
//   merge_and_next   --cliques=false --error_correction=false --threads 1 (ViralQuasispecies.cpp:413-447, mergeAlongEdges,
//                    SRBuilder.cpp:1238-1384) behind hlmi_vq_merge / hlmi_vq_iteration: the greedy merge list, each pair placed as
//                    a clique of two, the drops, the text files; vq_merge.hip reads, combines and lays out the bases
//   cliques_and_next --cliques=true, single-end (cliquesToSuperreads, :1031-1235) behind hlmi_vq_cliques / hlmi_vq_clique_iteration:
//                    the cliques of vq_clique_host.cpp placed, one pile-up consensus each in vq_clique.hip, the drops, the text
//                    files; vq_cliques_of_graph: the enumerator alone
// Both end, when asked, in findNextOverlaps (vq_next.hip) over the lists vq_next_tables builds of what they placed.
// and hlmi_vq_consensus_pair with the three option defaults.  PARITY UNPINNED, as vq_superread.cpp says.
#include <algorithm>
#include <cstring>

#include "paf_io.h"
#include "vq_internal.h"

namespace hlmi {

using namespace vqm;

void vq_merge_opts_stageb(hlmi_vq_merge_opts *o) {
    *o = hlmi_vq_merge_opts{};
    o->first_it = 1;
    o->keep_singletons = 300;             // max(min_overlap_len, min_read_len), pipeline_per_stage.py:170-203
    o->store_tips_separately = 1;
    o->min_clique_size = 2;
}

void vq_clique_opts_polyte(hlmi_vq_clique_opts *o, int error_correction) {
    *o = hlmi_vq_clique_opts{};
    o->min_clique_size = 2;                      // HyLight.py:228-242
    o->error_correction = error_correction != 0;
    o->first_it = 1;
    o->keep_singletons = error_correction ? 1000 : 0;        // polyte.tune_params.py:689-696
}

void vq_next_opts_stageb(hlmi_vq_next_opts *o) { *o = hlmi_vq_next_opts{}; }

void vq_consensus_pair(const char *seq1, const char *qual1, uint32_t len1, uint32_t qlen1, const char *seq2, const char *qual2,
                       uint32_t len2, uint32_t qlen2, uint32_t pos, double min_qual, char *out_seq, char *out_qual, uint32_t *out_len) {
    *out_len = 0;
    const std::vector<uint16_t> &tables = vq_consensus_tables(min_qual);
    vq_check_read(seq1, len1, qual1, qlen1, "hlmi_vq_consensus_pair: sequence", 1);
    vq_check_read(seq2, len2, qual2, qlen2, "hlmi_vq_consensus_pair: sequence", 2);
    const uint64_t total = std::max<uint64_t>(len1, (uint64_t)pos + len2);   // base + left + right extension (:224-252)
    if (total >= (1u << 30)) fail(HLMI_EINVAL, "hlmi_vq_consensus_pair: %llu bases", (unsigned long long)total);
    // SRBuilder::consensus (:453-521).  Read 1 is active from position 0 and meets :478 at once when it is empty, or at
    // position qlen1 when its quality string ends first; read 2 turns active at `pos` if the loop gets there (pos < total),
    // with the same two ends; between len1 and pos no read is active (:498).
    if (total == 0) return;
    if (len1 == 0 || qlen1 < len1) return;
    if (pos > len1) return;
    if (pos < total && (len2 == 0 || qlen2 < len2)) return;
    std::vector<std::string> seq{std::string(seq1, len1), std::string(seq2, len2)}, qual{std::string(qual1, len1), std::string(qual2, len2)};
    Rec r{};
    r.a = 0; r.b = len2 ? 1u : NONE; r.p = pos; r.len = (uint32_t)total; r.flags = F_CONS; r.id = 0;
    VqMergeDev dev(seq, qual, tables);
    std::vector<uint64_t> start;
    const std::string text = dev.write(std::vector<Rec>{r}, start);
    memcpy(out_seq, text.data() + 3, total);                                // "@0\n"
    memcpy(out_qual, text.data() + 3 + total + 3, total);
    *out_len = (uint32_t)total;
}

// original_ID_dict of a run that is not the first iteration: the lines of its subreads file
static void read_originals(VqOriginalsDict &d) {
    if (!d.first_it) d.dict = vq_parse_subreads(read_file(d.subreads_in), d.subreads_in);
}

// ViralQuasispecies.cpp:449-479 behind either builder: overlaps.txt and the line of stats.txt
static void next_and_stats(const VqGraphState &g, const std::vector<std::vector<VqEdge>> &out, const VqNextTables &t,
                           const hlmi_vq_graph_opts &go, const hlmi_vq_next_opts &no, const char *out_dir, const hlmi_vq_graph_stats *gst,
                           hlmi_vq_clique_next_stats *nst) {
    const std::string image = vq_next_run(g, out, t, go.edge_threshold, no, nst);
    write_file(join_path(out_dir, "overlaps.txt"), image.data(), image.size());
    const std::string line = std::to_string(gst->vertices) + "\t" + std::to_string(gst->edges_final) + "\t" +
                             std::to_string(nst->lines) + "\n";
    write_file(join_path(out_dir, "stats.txt"), line.data(), line.size(), "ab");
}

// hlmi_vq_merge (no == NULL) and hlmi_vq_iteration: one path.  With `no` the call goes on to findNextOverlaps, and reads
// subreads_in in front of the graph's first write: the iteration loop runs in place, its inputs under the names written here.
// min_qual reaches the tables the two passes of merge_kernel read, and through the 'N's they count, test_N_rate.
static void merge_and_next(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                           const hlmi_vq_merge_opts &mo, const hlmi_vq_next_opts *no, double min_qual, const char *out_dir,
                           hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst) {
    *mst = hlmi_vq_merge_stats{};
    if (nst) *nst = hlmi_vq_next_stats{};
    const std::vector<uint16_t> &tables = vq_consensus_tables(min_qual);     // refuses a bad min_qual in front of the first write
    VqOriginalsDict dict("vq_merge", mo.first_it != 0, subreads_in);
    if (no) read_originals(dict);
    VqGraphState g;
    vq_graph_run(fastq, overlaps, go, out_dir, gst, &g, no != nullptr);   // the graph and its files: one path for all entry points
    if (!g.built) return;                                        // ViralQuasispecies.cpp:282-291: nothing to be done
    const double t0 = now_ms();
    const uint32_t V = (uint32_t)g.seq.size();
    for (uint32_t v = 0; v < V; ++v) mst->bases_in += g.seq[v].size();       // (checked by vq_graph_run: vq_merge_check_reads)
    if (!no) read_originals(dict);

    VqMergeDev dev(g.seq, g.qual, tables);

    // getEdgesForMerging (GraphAlgos.cpp:112-148): vertices ascending; each free one takes its first free out-neighbour
    std::vector<uint8_t> taken(V, 0);
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    for (uint32_t u = 0; u < V; ++u) {
        if (taken[u]) continue;
        for (const VqEdge &e : g.out[u])
            if (!taken[e.v2]) {
                pairs.emplace_back(u, e.v2);
                taken[u] = taken[e.v2] = 1;
                break;
            }
    }
    mst->pairs = pairs.size();

    // constructSuperread per pair, a clique of two: placement, then the emptiness the lengths decide
    std::vector<Rec> placed, cand;               // per pair (len 0: empty); those with a consensus
    std::vector<uint32_t> clique(2);
    VqPlaced order;
    for (const auto &pr : pairs) {
        clique[0] = std::min(pr.first, pr.second);               // the clique is sorted (:658)
        clique[1] = std::max(pr.first, pr.second);
        const VqEdge *edge = vq_edge_info(g, clique[0], clique[1]);          // (none: the placement refuses it)
        if (edge && edge->pos1 < 0) fail(HLMI_EINVAL, "vq_merge: edge %u -> %u at position %d", edge->v1, edge->v2, edge->pos1);
        const uint64_t total = (uint64_t)vq_place(g, clique, "vq_merge", order);
        Rec r{};                                 // the edge's read 1 first, also where both lie at offset 0 and the list has
        r.a = edge->v1; r.b = edge->v2;          // them the other way round
        r.p = (uint32_t)order[1].first;
        r.len = r.p > g.seq[r.a].size() ? 0u : (uint32_t)total;  // a position without an active base: empty consensus (:498-501)
        r.flags = F_CONS | (g.orient[r.a] ? 0u : F_REV_A) | (g.orient[r.b] ? 0u : F_REV_B);
        placed.push_back(r);
        if (r.len) cand.push_back(r);
    }
    const std::vector<uint32_t> cand_n = dev.count_n(cand);      // first pass: the 'N's each super-read would hold
    const std::vector<uint32_t> read_n = dev.read_n_counts();

    // process_cliques (:998-1001): kept when the consensus is not empty and test_N_rate passes (Read.h:214-233)
    std::vector<Rec> recs;
    std::vector<uint8_t> visited(V, 0);
    std::vector<int64_t> new_id(V, -1);
    std::vector<uint32_t> offset(V, 0);
    std::vector<VqMember> sr_members;            // of the kept super-reads: what findNextOverlaps reads of them
    std::vector<uint32_t> sr_len;
    std::string subreads;
    size_t ci = 0;
    for (Rec r : placed) {
        if (!r.len) { ++mst->dropped_empty; continue; }
        if (!vq_n_rate_ok(cand_n[ci++], r.len)) { ++mst->dropped_n; continue; }
        r.id = (uint32_t)recs.size();
        // calcSubreadInfo with trim_pos 0 (:536-595): index = position in the super-read; then :750-806 per clique vertex in
        // sorted order, an original already there stays
        VqOriginals merged;
        const uint32_t members[2] = {std::min(r.a, r.b), std::max(r.a, r.b)};
        for (uint32_t v : members) {
            const long idx1 = v == r.a ? 0 : (long)r.p;
            vq_originals_add(merged, dict.originals_of(g, v), g.orient[v] != 0, dict.first_it, idx1, (long)g.seq[v].size());
            visited[v] = 1;
            new_id[v] = r.id;
            offset[v] = (uint32_t)idx1;
            sr_members.push_back(VqMember{v, r.id, (int32_t)idx1});
        }
        sr_len.push_back(r.len);
        vq_subreads_line(subreads, r.id, merged);
        recs.push_back(r);
    }
    mst->merged = recs.size();

    // the unmerged reads (:1282-1372), dropped pairs among them; tips and inclusions go to a file of their own, forward, as read
    std::vector<uint8_t> divert(V, 0);
    for (uint32_t v = 0; v < V; ++v) divert[v] = (go.ignore_inclusions && g.incl[v]) || (g.tip[v] && mo.store_tips_separately);
    std::vector<uint32_t> diverted;
    const VqLoneCounts lone = vq_lone_reads(g, dict, visited, read_n, mo.keep_singletons, &divert, (uint32_t)mst->merged, recs, subreads, &diverted);
    mst->short_reads = lone.short_reads; mst->n_reads = lone.n_reads;
    mst->trivial = lone.trivial; mst->trivial_reverse = lone.trivial_reverse;
    for (size_t k = mst->merged; k < recs.size(); ++k) new_id[recs[k].a] = recs[k].id;

    // one gather writes both FASTQ files' text: singles.fastq, then the tip records
    const size_t n_singles = recs.size();
    for (uint32_t v : diverted) {
        recs.push_back(Rec{v, NONE, 0, (uint32_t)g.seq[v].size(), 0, (uint32_t)(recs.size() - n_singles)});
        if (go.ignore_inclusions && g.incl[v]) ++mst->inclusion_reads; else ++mst->tip_reads;
    }
    std::vector<uint64_t> start;
    const std::string text = dev.write(recs, start);
    const uint64_t cut = start[n_singles];
    mst->bytes_out = cut;
    write_file(join_path(out_dir, "singles.fastq"), text.data(), cut);                  // (the reference removes it first, :1245)
    write_file(join_path(out_dir, "subreads.txt"), subreads.data(), subreads.size());
    if (!diverted.empty())                                                               // writeTipsToFile APPENDS (:1391)
        write_file(join_path(out_dir, "removed_tip_sequences.fastq"), text.data() + cut, text.size() - cut, "ab");
    std::string map;
    for (uint32_t v = 0; v < V; ++v) {
        map += std::to_string(v); map += '\t'; map += std::to_string(new_id[v]); map += '\t';
        map += std::to_string(offset[v]); map += '\t'; map += g.orient[v] ? '+' : '-'; map += '\n';
    }
    write_file(join_path(out_dir, "superread_map.txt"), map.data(), map.size());
    mst->ms_merge = now_ms() - t0;
    if (no) {                                                    // ViralQuasispecies.cpp:449-479
        const double t1 = now_ms();
        // a merged vertex is a list of one super-read, a copied one a list of itself: the lists of at most one entry
        const std::vector<Rec> lone(recs.begin() + (ptrdiff_t)mst->merged, recs.begin() + (ptrdiff_t)n_singles);
        hlmi_vq_clique_next_stats x{};
        next_and_stats(g, g.out, vq_next_tables(V, sr_members, mst->merged, sr_len, lone), go, *no, out_dir, gst, &x);
        nst->src_graph = x.src_graph; nst->src_branching = x.src_branching; nst->src_nonedge = x.src_nonedge;
        nst->nonedge_skipped = x.nonedge_skipped; nst->src_induced = x.src_induced;
        nst->copied = x.copied; nst->u2sr = x.u2sr; nst->v2sr = x.v2sr; nst->sr2sr = x.sr2sr;
        nst->claims_failed = x.claims_failed; nst->lines = x.lines;
        nst->ms_next = now_ms() - t1;
    }
    ktimer_flush();
}

void vq_merge_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                  const hlmi_vq_merge_opts &mo, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst) {
    merge_and_next(fastq, overlaps, subreads_in, go, mo, nullptr, min_qual, out_dir, gst, mst, nullptr);
}

void vq_iteration_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                      const hlmi_vq_merge_opts &mo, const hlmi_vq_next_opts &no, double min_qual, const char *out_dir,
                      hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst) {
    merge_and_next(fastq, overlaps, subreads_in, go, mo, &no, min_qual, out_dir, gst, mst, nst);
}

void vq_cliques_of_graph(const char *graph_txt, const char *cliques_out, uint64_t *n_cliques) {
    const VqCliqueList list = vq_enumerate_cliques(read_file(graph_txt));
    write_file(cliques_out, list.text.data(), list.text.size());
    *n_cliques = list.off.size() - 1;
}

// hlmi_vq_cliques (no == NULL) and hlmi_vq_clique_iteration: one path, as merge_and_next is.  min_qual reaches the tables, the
// pile-up kernel and the host's redo of a marked column: the three places a column is decided
static void cliques_and_next(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                             const hlmi_vq_clique_opts &co, const hlmi_vq_next_opts *no, double min_qual, const char *out_dir,
                             hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst, hlmi_vq_clique_next_stats *nst,
                             VqBranchRun *branch = nullptr) {
    using namespace vqc;
    *cst = hlmi_vq_clique_stats{};
    if (nst) *nst = hlmi_vq_clique_next_stats{};
    const std::vector<uint16_t> &tables = vq_consensus_tables(min_qual);     // refuses a bad min_qual in front of the first write
    if (co.min_clique_size == 0 || co.min_clique_size > MAX_MIN_CLIQUE)
        fail(HLMI_EINVAL, "vq_cliques: min_clique_size %u is outside 1 .. %u", co.min_clique_size, MAX_MIN_CLIQUE);
    VqOriginalsDict dict("vq_cliques", co.first_it != 0, subreads_in);
    const uint32_t mcs = co.min_clique_size;
    if (no) read_originals(dict);                // in place: subreads_in may be the subreads.txt written below
    VqGraphState g;
    if (branch) branch->dict = &dict;            // --branch_reduction=true reads the same original_ID_dict
    vq_graph_run(fastq, overlaps, go, out_dir, gst, &g, no != nullptr, branch);
    if (!g.built) return;                        // ViralQuasispecies.cpp:282-291: nothing to be done
    const double t0 = now_ms();
    const uint32_t V = (uint32_t)g.seq.size();
    for (uint32_t v = 0; v < V; ++v) cst->bases_in += g.seq[v].size();
    if (!no) read_originals(dict);

    // cliques.txt (ViralQuasispecies.cpp:400-410)
    const VqCliqueList list = vq_enumerate_cliques(read_file(join_path(out_dir, "graph.txt").c_str()));
    write_file(join_path(out_dir, "cliques.txt"), list.text.data(), list.text.size());
    const double t_enumerated = now_ms();
    const size_t n_lines = list.off.size() - 1;
    cst->cliques_read = n_lines + 2;             // getline counts the two text lines as well (:1056-1057)

    // constructSuperread per clique: the placement
    struct Placed {
        std::vector<uint32_t> clique;            // ascending
        VqPlaced all;                            // (offset, vertex) in list order, every member
        uint32_t pile;                           // its pile-up
    };
    std::vector<Placed> placed;
    std::vector<Pile> piles;
    std::vector<Entry> entries;
    uint64_t cols = 0;
    for (size_t k = 0; k < n_lines; ++k) {
        const size_t size = (size_t)(list.off[k + 1] - list.off[k]);
        if (size == 1) { ++cst->singletons; continue; }
        if (size < mcs) { ++cst->below_min; continue; }
        ++cst->taken;
        Placed P;
        P.clique.assign(list.members.begin() + (ptrdiff_t)list.off[k], list.members.begin() + (ptrdiff_t)list.off[k + 1]);
        for (uint32_t v : P.clique)
            if (v >= V) fail(HLMI_EINVAL, "vq_cliques: clique vertex %u of %u", v, V);
        std::sort(P.clique.begin(), P.clique.end());                       // :658
        const int64_t total = vq_place(g, P.clique, "vq_cliques", P.all);
        // filter_subreads (:597-636) when the clique is large (:721)
        VqPlaced used = P.all;
        if (size > 3 * (size_t)mcs) {
            ++cst->filtered;
            used = vq_filter_subreads(g, 2 * (size_t)mcs, P.clique[0], P.all);
        }
        // consensus (:420-446): where the output starts; a read in front of it that ends there empties it (:478)
        uint32_t trim = 0;
        bool empty = false;
        if (co.error_correction) {
            // :427-432 drops a pile without an entry number min_clique_size.  A clique taken here has min_clique_size
            // members and a filtered one 2 * min_clique_size, so the check never fires; it stays as the reference has it.
            if (used.size() < mcs) { ++cst->dropped_support; continue; }
            trim = (uint32_t)used[mcs - 1].first;
            for (const auto &pv : used)
                if (pv.first < (int64_t)trim && pv.first + (int64_t)g.seq[pv.second].size() <= (int64_t)trim) empty = true;
        }
        if (empty || trim >= total) { ++cst->dropped_empty; continue; }
        if (used.size() > MAX_PILE) fail(HLMI_EINVAL, "vq_cliques: a pile-up of %zu reads", used.size());
        Pile pl{};
        pl.first = (uint32_t)entries.size(); pl.n = (uint32_t)used.size();
        pl.total_len = (uint32_t)total; pl.trim_pos = trim; pl.col0 = cols;
        for (const auto &pv : used) entries.push_back(Entry{pv.second, (uint32_t)pv.first, g.orient[pv.second] ? 0u : 1u});
        cols += (uint64_t)total;
        P.pile = (uint32_t)piles.size();
        piles.push_back(pl);
        placed.push_back(std::move(P));
    }

    const double t_placed = now_ms();
    VqMergeDev dev(g.seq, g.qual, tables);
    std::vector<uint8_t> cb, cq;
    std::vector<Result> res;
    dev.consensus_piles(piles, entries, mcs, co.error_correction != 0, min_qual, cb, cq, res);
    const double t_device = now_ms();

    // process_cliques (:998-1001), writeSinglesToFile, the originals (:750-806)
    std::string fastq_text, subreads, cmap;
    std::vector<uint8_t> visited(V, 0);
    std::vector<VqMember> sr_members;            // of the kept super-reads: what findNextOverlaps reads of them
    std::vector<uint32_t> sr_len;
    uint32_t count = 0;
    for (const Placed &P : placed) {
        const Pile &pl = piles[P.pile];
        const Result &r = res[P.pile];
        if (r.empty || r.stop <= pl.trim_pos || r.stop > pl.total_len) {
            if (!r.empty && r.stop > pl.total_len) fail(HLMI_EINVAL, "vq_cliques: the device ended a consensus at %u of %u", r.stop, pl.total_len);
            ++cst->dropped_empty;
            continue;
        }
        const uint32_t len = r.stop - pl.trim_pos;
        uint8_t *b = cb.data() + pl.col0 + pl.trim_pos, *q = cq.data() + pl.col0 + pl.trim_pos;
        uint64_t n_count = 0;
        for (uint32_t x = 0; x < len; ++x) {
            if (q[x] == 0) {                     // too close to a threshold for the device: the host's libm decides
                const uint16_t e = vq_consensus_column(g, &entries[pl.first], pl.n, pl.trim_pos + x, min_qual);
                b[x] = (uint8_t)(e >> 8);
                q[x] = (uint8_t)e;
                ++cst->columns_host;
            }
            n_count += b[x] == 'N';
        }
        cst->columns += len;
        if (!vq_n_rate_ok(n_count, len)) { ++cst->dropped_n; continue; }
        fastq_text += '@'; fastq_text += std::to_string(count); fastq_text += '\n';
        fastq_text.append((const char *)b, len); fastq_text += "\n+\n";
        fastq_text.append((const char *)q, len); fastq_text += '\n';
        std::unordered_map<uint32_t, int64_t> offset;        // calcSubreadInfo (:536-595): index1 - startpos1 = offset - trim_pos
        for (const auto &pv : P.all) offset.emplace(pv.second, pv.first - (int64_t)pl.trim_pos);
        VqOriginals merged;
        for (uint32_t v : P.clique) {
            vq_originals_add(merged, dict.originals_of(g, v), g.orient[v] != 0, dict.first_it, (long)offset.at(v), (long)g.seq[v].size());
            visited[v] = 1;
        }
        vq_subreads_line(subreads, count, merged);
        cmap += std::to_string(count); cmap += '\t'; cmap += std::to_string(pl.trim_pos);
        for (const auto &pv : P.all) {
            cmap += '\t'; cmap += std::to_string(pv.second); cmap += ':'; cmap += std::to_string(pv.first - (int64_t)pl.trim_pos);
            cmap += ':'; cmap += g.orient[pv.second] ? '+' : '-';
            if (no) sr_members.push_back(VqMember{pv.second, count, (int32_t)(pv.first - (int64_t)pl.trim_pos)});
        }
        cmap += '\n';
        sr_len.push_back(len);
        ++count;
    }
    cst->superreads = count;

    // the reads in no kept super-read (:1145-1222)
    std::vector<vqm::Rec> recs;
    const VqLoneCounts lone = vq_lone_reads(g, dict, visited, dev.read_n_counts(), co.keep_singletons, nullptr, count, recs, subreads, nullptr);
    cst->short_reads = lone.short_reads; cst->n_reads = lone.n_reads;
    cst->trivial = lone.trivial; cst->trivial_reverse = lone.trivial_reverse;
    std::vector<uint64_t> start;
    fastq_text += dev.write(recs, start);
    cst->bytes_out = fastq_text.size();
    write_file(join_path(out_dir, "singles.fastq"), fastq_text.data(), fastq_text.size());         // (the reference removes it first, :1038)
    write_file(join_path(out_dir, "subreads.txt"), subreads.data(), subreads.size());
    write_file(join_path(out_dir, "clique_map.txt"), cmap.data(), cmap.size());
    cst->ms_cliques = now_ms() - t0;
    ktimer_flush();
    // the phases of ms_cliques for tools/vq_cliques_time.py: enumerator, placement, device (uploads, kernel, downloads), the rest
    stat_set("vq_clique_ms_enumerate", t_enumerated - t0);
    stat_set("vq_clique_ms_place", t_placed - t_enumerated);
    stat_set("vq_clique_ms_device", t_device - t_placed);
    stat_set("vq_clique_ms_finish", t0 + cst->ms_cliques - t_device);
    stat_set("vq_clique_piles", (double)piles.size());
    if (no) {                                    // ViralQuasispecies.cpp:449-479
        const double t1 = now_ms();
        next_and_stats(g, vq_cliques_out(g), vq_next_tables(V, sr_members, count, sr_len, recs), go, *no, out_dir, gst, nst);
        nst->ms_next = now_ms() - t1;
        ktimer_flush();
    }
}

void vq_cliques_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                    const hlmi_vq_clique_opts &co, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                    hlmi_vq_clique_stats *cst) {
    cliques_and_next(fastq, overlaps, subreads_in, go, co, nullptr, min_qual, out_dir, gst, cst, nullptr);
}

void vq_clique_iteration_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                             const hlmi_vq_clique_opts &co, const hlmi_vq_next_opts &no, double min_qual, const char *out_dir,
                             hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst, hlmi_vq_clique_next_stats *nst) {
    cliques_and_next(fastq, overlaps, subreads_in, go, co, &no, min_qual, out_dir, gst, cst, nst);
}

// hlmi_vq_branch_iteration: hlmi_vq_clique_iteration's path with the branch reduction inside its graph
void vq_branch_iteration_run(const char *fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                             const char *table, const hlmi_vq_graph_opts &go, const hlmi_vq_branch_opts &bo, const hlmi_vq_clique_opts &co,
                             const hlmi_vq_next_opts &no, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                             hlmi_vq_branch_stats *bst, hlmi_vq_clique_stats *cst, hlmi_vq_clique_next_stats *nst) {
    *bst = hlmi_vq_branch_stats{};
    VqBranchRun br;
    br.bo = bo; br.original_fastq = original_fastq; br.table_path = table; br.st = bst;
    cliques_and_next(fastq, overlaps, subreads_in, go, co, &no, min_qual, out_dir, gst, cst, nst, &br);
}

}  // namespace hlmi
