/* hylight_mi.h - C ABI of libhylight_mi.so: the MI355X-native overlap -> filter -> graph hot path
 * of HyLight.
 *
 * The reference (kangxiongbin/HyLight @ 2024_10_08) has no FFI: the path sits behind process
 * boundaries.  Each entry point below replaces one of those
 * boundaries and cites it; `INTEGRATION.md` shows the ctypes stub a maintainer would add on the
 * reference side.  Conventions:
 *   - plain C types only; strings are caller-owned NUL-terminated paths; outputs are files,
 *     so no memory ownership crosses the boundary (device pointers, where they appear, are
 *     caller-owned HIP allocations passed as void*);
 *   - every call returns 0 on success or a negative HLMI_E* code; the message is available
 *     from hlmi_last_error() (thread-local);
 *   - calls need a HIP device: the library has NO CPU fallback and fails with HLMI_ENODEV
 *     when none is usable.
 */
#ifndef HYLIGHT_MI_H
#define HYLIGHT_MI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HLMI_OK        0
#define HLMI_EINVAL   -1   /* bad argument / malformed input file */
#define HLMI_EIO      -2   /* cannot open / read / write a file */
#define HLMI_ENODEV   -3   /* no usable HIP device (there is no CPU fallback) */
#define HLMI_EHIP     -4   /* a HIP runtime call or kernel failed */
#define HLMI_ENOMEM   -5
#define HLMI_ESTATE   -6   /* call sequence error (e.g. job step called out of order) */

/* ---- library state -------------------------------------------------------------------- */
/* Select the HIP device used by this process (one process per GPU).  device < 0 keeps the
 * current device.  host_threads bounds host-side helper threads (text formatting, sorting,
 * the output writer); <= 0: the CPUs this process may run on, 16 at most. */
/* ABI version: bumped whenever a public struct grows or an EXISTING entry point changes its signature (5: hlmi_ava_opts ends
 * in zdrop; 6: hlmi_vq_merge, hlmi_vq_consensus_pair).  It guards struct layouts and the signatures of existing symbols.  A
 * caller compares hlmi_abi_version() with the HLMI_ABI_VERSION of the header it was built against BEFORE passing structs: a
 * caller of an older header would hand over a shorter hlmi_ava_opts than the library reads.  A NEW symbol beside the old ones
 * (the hlmi_vq_*_mq calls) leaves the version alone: it is found, or not found, when the library is loaded. */
#define HLMI_ABI_VERSION 7
int         hlmi_abi_version(void);
int         hlmi_init(int device, int host_threads);
void        hlmi_shutdown(void);
const char *hlmi_last_error(void);
const char *hlmi_version(void);

/* ---- B1: whole stage = utils.split_reads2 (script/utils.py:41-71) ----------------------- */
/* reads_fa = query reads (`-r`), ref_fa = targets that get --nsplit-chunked (`-c`); writes the
 * merged, score-sorted 14-column PAF (trailing TAB before newline, filter_overlap_slr2.py:151)
 * to out_paf.  `threads` is accepted for signature parity (the reference uses it for xargs -P
 * and minimap2 -t; here the GPU does the work).  rank/world shard the target chunks
 * (chunk i -> rank i % world); with world > 1 each rank writes `out_paf` for its own chunks and
 * hlmi_merge_scored_paf() combines them. */
int hlmi_split_reads2(const char *reads_fa, const char *ref_fa, int nsplit, const char *out_dir,
                      const char *out_paf, int threads, int len_over, int mc, double iden,
                      int long_mode);
int hlmi_split_reads2_shard(const char *reads_fa, const char *ref_fa, int nsplit, const char *out_dir,
                            const char *out_paf, int threads, int len_over, int mc, double iden,
                            int long_mode, int rank, int world);
/* merge of per-rank outputs = the final `sort -k12 -nr` of utils.py:69 */
int hlmi_merge_scored_paf(const char *const *in_pafs, int n_in, const char *out_paf);

/* ---- B2: one chunk of filter_overlap_slr2.main after the overlapper (slr2:57-152) ------- */
/* paf_in: overlapper output (PAF with cg:Z: as LAST field, slr2:312).  Runs the v4 window
 * filter (-len 30 -oh 3, slr2:51), the intermediate order (slr2:57), the SNP pile-up
 * (slr2:229-367), mutation_re (slr2:370-405) and pass 2 (slr2:77-152) on the GPU and writes
 * <chunk>_tmp_overlap4.paf-format rows (unsorted, in pass-2 order) to out_paf. */
int hlmi_filter_chunk(const char *paf_in, const char *out_overlap4_paf, int len_over, int mc,
                      double iden, double thre /*0.0025*/, int min_o /*4*/, int long_mode);

/* ---- a4 / a17: filter_trans_ovlp_inline_v4.py:31-85 and _v3.py:39-102 ------------------- */
/* variant 4: rows are copied through unchanged; variant 3: sfo != 0 writes SFO rows, else
 * "q t score" rows.  min_iden < 0 selects the script default (0.6 for v4, 0.8 for v3). */
int hlmi_paf_window_filter(int variant, int min_len, double min_iden, int min_o, int sfo,
                           const char *in_paf, const char *out_path);

/* ---- the short-read cluster path's filter and converter ----------------- */
/* filter_ovlp_inline.py <min_ovlp_len> <min_identity> <o> <r> (script/filter_ovlp_inline.py:12-106,
 * called at polyte.tune_params.py:507-511): 1000-row windows, internal-match test, longest overlap per
 * pair.  Runs on the GPU. */
int hlmi_filter_ovlp_inline(const char *in_paf, const char *out_paf, int min_ovlp_len, double min_identity,
                            int o, double r);
/* minimap22sfo.py --in --out -m <min_overlap_len> -p <min_pident> (script/minimap22sfo.py:28-75): PAF -> SFO with
 * the ids in string order.  Pure text conversion (host). */
int hlmi_minimap22sfo(const char *in_paf, const char *out_sfo, int min_overlap_len, double min_pident);

/* ---- the line-oriented text passes either side of the path (host I/O, no GPU work) ----
 * Same text conventions as the Python originals (universal newlines, str.strip()/split() white space).
 *
 * utils.filter_non_atcg(fq, out_dir, model) (script/utils.py:81-114): sequences upper-cased with every character
 * outside ATGCN replaced by N, headers cut at the first space; `is_fastq` = (model == "fastq").  The reference
 * derives the output path (<out_dir>/1.split_fastx/s1.fa); here the caller passes it. */
int hlmi_filter_non_atcg(const char *fastx, const char *out_fa, int is_fastq);
/* HyLight.gfa2fa(gfa, fa) (script/HyLight.py:328-337): S lines -> FASTA records.  An empty line is an error
 * (the reference raises IndexError on it). */
int hlmi_gfa2fa(const char *gfa, const char *out_fa);
/* HyLight.pick_up(ovlap, outdir, fq) (script/HyLight.py:347-378): the records of `fastx` whose name (text before
 * the first '/', without the leading '@' or '>') appears in neither column 1 nor column 6 of the PAF.  The
 * reference names the output <outdir>/sub<clock digits>_remain.fq; here the caller passes the path.  As in the
 * reference an existing file is removed first and no file is created when nothing is kept. */
int hlmi_pick_up(const char *ovlap_paf, const char *fastx, const char *out_fastx, int is_fastq);

/* ---- a3: the overlapper (replaces the external minimap2 call, slr2:51 / slr2:55) -------- */
typedef struct {
    int k;                 /* 19 (long, -Hk19) */
    int w;                 /* 5  (ava-pb)      */
    int hpc;               /* 1  (-H)          */
    int min_chain_score;   /* 100   (-m100)    */
    int max_gap;           /* 10000 (-g10000)  */
    int bandwidth;         /* chaining band, 2000 */
    int min_cnt;           /* 3 minimizers per chain (-n default) */
    int min_mid_occ;       /* 10 */
    double mid_occ_frac;   /* 2e-4; <= 0: the cut-off is min_mid_occ itself (-f INT) */
    int match, mismatch, gap_open, gap_ext, ambi;   /* 2 4 4 2 1 */
    int min_dp_score;      /* alignment pieces below this DP score are dropped: 80 (long), 60 (-s 60, short) */
    int end_bonus;         /* bonus for an end extension that reaches the query end: 0 (long), 100 (short) */
    int pair_once;         /* 1: report a pair only with strcmp(qname,tname) < 0 (ava-pb -X); 0: every non-self pair */
    int gap_open2, gap_ext2;   /* second piece of the gap cost: a gap of L bases costs min(gap_open + gap_ext L, gap_open2 +
                                  gap_ext2 L): 24, 1 (long: the preset's -O4,24 -E2,1), 32, 1 (short: --sr's -O12,32 -E2,1);
                                  gap_open2 <= 0: one piece.  The second piece must not be the cheaper one for gaps of
                                  fewer than 16 bases (the 16-diagonal kernels work with the first piece alone). */
    int stub_oh;           /* >= 0: the rows go to a consumer that drops internal matches with this overhang bound
                              (filter_trans_ovlp_inline_v4.py:52-64 with -oh 3, slr2:51,55).  An alignment piece that is
                              certain to be reported (block score >= min_dp_score + end_bonus) and certain to fail that test
                              whatever its end extensions find (an end more than X + stub_oh query and X + 64 + stub_oh target
                              bases inside both sequences, X = max(256, max_gap) = the reach of an end extension) is then
                              reported WITHOUT end extensions: the consumer only counts it as a line of its 1000-line windows.
                              < 0: every piece is extended (hlmi_ava's default; the stage entry points use 3). */
    int zdrop;             /* > 0: an end extension (up to max(256, max_gap) rows) stops at the first of its rows 32, 64, ...
                              whose best cell lies more than this below the best cell so far: 400 (long: minimap2's -z of the
                              ava-pb preset); 0: no z-drop (short: extensions stay within 256 rows) */
} hlmi_ava_opts;
void hlmi_ava_opts_long(hlmi_ava_opts *o);    /* the constants of slr2:51 (ava-pb -Hk19 -m100 -g10000) */
void hlmi_ava_opts_short(hlmi_ava_opts *o);   /* the constants of slr2:55 (--sr -k21 -w11 -s60 -m30 -n2 -A4 -B2 --end-bonus=100) */
/* target_fa = one chunk, query_fa = all reads; writes minimap2-style PAF rows (12 columns +
 * NM, tp, cg:Z: tags, cg last) in query-file order. */
int hlmi_ava(const char *target_fa, const char *query_fa, const hlmi_ava_opts *opts,
             const char *out_paf);

/* ---- B3: miniasm (tools/miniasm/main.c:32-211) with the flags HyLight passes ------------- */
/* HyLight.py:137,140,171:  miniasm -d <bub_dist> -n <n_rounds_arg> -e <max_ext> -c <min_dp>
 * -f <reads_fa> <paf> > <out_gfa>.  reads_fa may be NULL (S lines then carry '*').
 * outfmt: "ug" (GFA, default when NULL), "sg", "paf", "bed" (main.c:146-150). */
int hlmi_miniasm(const char *paf, const char *reads_fa, int bub_dist, int n_rounds_arg,
                 int max_ext, int min_dp, const char *outfmt, const char *out_path);

/* ---- a18: sfo2overlaps.py (--num_pairs 0 branch, HyLight.py:315-318) --------------------- */
int hlmi_sfo2overlaps(const char *in_sfo, const char *out_savage, int num_singles, int num_pairs);

/* ---- POLYTE's run_sfo chain in one call (polyte.tune_params.py:488-529, :534-579) ---------------------------------------
 * The self-overlaps of a read set as a SAVAGE overlaps file: byte for byte what
 *   hlmi_ava(reads, reads, <-X -r 0 short-read options>) -> hlmi_filter_ovlp_inline(min_ovlp_len, min_identity, o, r) ->
 *   hlmi_minimap22sfo(0, 0.0) -> hlmi_sfo2overlaps(num_singles = reads, num_pairs = 0)
 * write when chained on the reads as FASTA, without the three text files in between: the overlapper's rows stay on the device,
 * the inline filter reads them there in the overlapper's order, and the SFO / SAVAGE conversion, the sort | uniq and the text
 * are kernels (csrc/sr_overlaps.hip).  `reads`: FASTQ or FASTA whose names are non-negative decimal integers below 10^18 (the
 * files POLYTE renumbers, singles.fastq).  *n_lines: lines written.  An input without overlaps leaves an empty file and 0.
 * HLMI_EINVAL before anything is written: a NULL argument, a name that is no decimal integer, two reads of one name (or of one
 * number: 7 and 007). */
int hlmi_sr_overlaps(const char *reads, int min_ovlp_len, double min_identity, int o, double r, const char *out_overlaps,
                     uint64_t *n_lines);

/* ---- f3 (STARTED): front end of the SAVAGE overlap-graph assembler ------ */
/* tools/HaploConduct/src (ViralQuasispecies) needs Boost and cannot be built here: the entry points below restate its
 * text of record and are checked against oracle/vq.py and tests/vq_graph_model.py only (parity unpinned).  Built: the
 * parser, the quality-aware overlap score, transitive edges, and the oriented, reduced overlap graph of a --graph_only run
 * (hlmi_vq_graph), and the step that reads it with --cliques=false: SRBuilder::mergeAlongEdges, the super-reads of the next
 * iteration (hlmi_vq_merge), and SRBuilder::findNextOverlaps behind it (hlmi_vq_iteration: one whole stage-b iteration; the
 * loop of pipeline_per_stage.py is hylight_amd/vq_stageb.py), and the step of --cliques=true for single-end reads: the maximal
 * cliques of graph.txt and SRBuilder::cliquesToSuperreads (hlmi_vq_cliques; cliques.txt is pinned to the reference's own
 * enumerator), findNextOverlaps behind the clique step (hlmi_vq_clique_iteration), and the read-evidence branch reduction of
 * --branch_reduction=true (hlmi_vq_branch_graph, hlmi_vq_branch_iteration).  Not built: FindNextOverlaps3, the diploid
 * resolution of BranchReduction, paired-end vertices, --min_qual=0. */
typedef struct {
    uint64_t id1, id2;                 /* strtoul(..., 0) of columns 1, 2                        (Overlap.h:39-40, Types.h:99)  */
    uint32_t pos1, pos2, perc1, perc2, len1, len2;   /* atoi; pos2 = perc2 = len2 = 0 when column 4 is "-" (Overlap.h:53-57) */
    char ord, ori1, ori2, type1, type2; /* '1' '2' '-';  '+' '-';  's' 'p'                                                  */
    char pad[3];
} hlmi_vq_overlap;
/* EdgeCalculator.cpp:561-666 construct_edges, the part in front of process_overlaps: lines are trimmed of outer tabs and
 * blanks and split at tabs; a line without 13 fields is skipped ("incorrect overlap"), as is id1 == id2; an overlap is an
 * edge candidate when (s,s: len1 >= min_len) or (a 'p' type: len1, len2 >= min_len / 2, or with relax_pe len1 + len2 >=
 * min_len) and perc >= min_perc, where perc = (perc1 + perc2) / 2 truncated when perc2 > 0, else perc1 (Overlap.h:196).
 * Reads at most max_overlaps lines.  Candidates go to out[0 .. min(*n_out, cap)) in file order; *n_nonedge counts the rows
 * the reference writes back to nonedge_overlaps.txt, *n_skipped the other ones.  out may be NULL (cap 0) to count. */
int hlmi_vq_parse_overlaps(const char *savage_path, uint32_t min_overlap_len, uint32_t min_overlap_perc, int relax_pe,
                           uint64_t max_overlaps, hlmi_vq_overlap *out, uint64_t cap, uint64_t *n_out,
                           uint64_t *n_nonedge, uint64_t *n_skipped);
/* GraphAlgos.cpp:746-795 (findTransEdges, nonemptyIntersect) and :938-993 (removeTransitiveEdges up to the deletion):
 * edge k = src[k] -> dst[k] of a directed graph on n_vertices vertices.  An edge u -> v is transitive when some w has
 * u -> w and w -> v.  remove_trans = 1: flags bit 0 marks the transitive edges; 2 / 3: the search is repeated on the graph
 * of the edges found so far ("double" / "triple" transitive), bit 0 marks the last round's set - the edges the reference
 * then removes.  With remove_trans == 1 and ovlen != NULL (branch_reduction > 0, :970-993) bit 1 marks the edges
 * scheduled for deletion: for every transitive edge u -> v of overlap length L, every out-edge of u and every in-edge of v
 * whose length is <= L.  GPU: one wave per vertex, its out-neighbours in an LDS hash table, the in-lists streamed by the
 * lanes. */
int hlmi_vq_transitive_edges(uint32_t n_vertices, uint64_t n_edges, const uint32_t *src, const uint32_t *dst,
                             const uint32_t *ovlen, int remove_trans, uint8_t *flags, uint64_t *n_transitive);
/* EdgeCalculator::overlap_score (EdgeCalculator.cpp:26-139) for the single-single overlaps of an overlaps file
 * (compute_overlap's "s"-"s" branch, :186-222 - the only one HyLight reaches: --num_pairs 0): for overlap k of `ov`
 * (as returned by hlmi_vq_parse_overlaps) score[k] = exp(mean log-probability that the overlapping bases of the two reads
 * of fastq_singles come from one sequence, given their phred qualities), 0 when a position's probability falls below
 * `mismatch`, a read is shorter than `min_read_len` or pos1 lies behind read 1; mismatch_rate[k] as the reference sets it
 * (1.0 where it returns early); pos3[k] = len1 - pos1 - len2 (Edge::set_extra_pos).  The per-position sums are taken in
 * sequence order in double precision, log / pow / exp are the host's libm (tables by quality pair): the same arithmetic as
 * the reference's.  Reads are looked up by the integer id of their "@<id>" line (strtoul base 0, FastqStorage.cpp:109-117). */
int hlmi_vq_overlap_scores(const char *fastq_singles, const hlmi_vq_overlap *ov, uint64_t n, double mismatch,
                           uint32_t min_read_len, double *score, double *mismatch_rate, int64_t *pos3);

/* ViralQuasispecies --graph_only=true (ViralQuasispecies.cpp:250-398) on single-end reads: the options it reads. */
typedef struct {
    uint32_t min_overlap_len, min_overlap_perc, min_read_len, max_tip_len, remove_trans;
    double edge_threshold, ov_threshold, merge_contigs, mismatch;
    int ignore_inclusions, remove_tips, remove_branches, remove_backedges;
    uint64_t max_overlaps;
} hlmi_vq_graph_opts;
/* The values HyLight's first stage-b iteration passes (HyLight.py:320-324 -> pipeline_per_stage.py:170-200):
 * min_overlap_len 300, min_overlap_perc 0, edge_threshold 1, merge_contigs 0, remove_trans 1, remove_branches 1,
 * ignore_inclusions 1, max_tip_len 1000; the rest ViralQuasispecies' defaults (ViralQuasispecies.cpp:55-100):
 * ov_threshold 0.9, mismatch 0, min_read_len 0, remove_tips 1, remove_backedges 1 (error_correction false),
 * max_overlaps 1e8. */
void hlmi_vq_graph_opts_stageb(hlmi_vq_graph_opts *o);
typedef struct {
    uint64_t vertices;      /* reads of singles_fastq (vertex = position in the file)                                   */
    uint64_t candidates;    /* scored candidates that passed the edge rule (score > edge_threshold, or mismatch rate
                               <= merge_contigs)                                                                         */
    uint64_t duplicates;    /* candidates - edges_built: candidates of a (pair, orientation class) already in the graph */
    uint64_t inclusions;    /* candidates with perc 100 (the reference's inclusion_count)                               */
    uint64_t edges_built;   /* edges after process_overlaps: one per (pair, orientation class)                          */
    uint64_t conflicts;     /* edges deleted by the orientation labelling (its best try)                                */
    uint64_t moved;         /* edges the labelling moved to the other endpoint's list                                   */
    uint64_t transitive;    /* edges removeTransitiveEdges removed                                                      */
    uint64_t tip_edges;     /* edges removeTips removed                                                                 */
    uint64_t tip_reads;     /* reads it marked as tips (the lines of tips.txt)                                          */
    uint64_t branch_edges;  /* edges removeBranches removed                                                             */
    uint64_t backedges;     /* back edges of the best DFS (the lines of cycles.txt)                                     */
    uint64_t edges_final;   /* edges of the final graph (the lines of digraph.txt)                                      */
} hlmi_vq_graph_stats;
/* Builds and reduces the overlap graph of `overlaps` (13 columns, single-end rows) over the reads of singles_fastq the way
 * ViralQuasispecies --graph_only=true --threads 1 does, and writes into out_dir (which must exist), byte for byte in the
 * reference's formats: nonedge_overlaps.txt, graph.gfa (after transitive-edge removal), graph.txt, graph_trimmed.gfa,
 * digraph.txt, cycles.txt (only when there are back edges: the reference removes it and writes it back edge by edge), and
 * the project's own tips.txt (ascending ids of the vertices whose reads removeTips marked as tips).  When no edge is
 * built, the reference stops after nonedge_overlaps.txt (and removes graph.txt); so does this call.
 * The contract is the sequential reference: with several threads the reference adds each chunk's edges in the order its
 * critical sections run (EdgeCalculator.cpp:395-419), so the first candidate of a (pair, orientation class) - the only
 * one that can mark an inclusion - may differ between its multi-thread runs.
 * Refused with HLMI_ESTATE (not on HyLight's path): an edge candidate of type 'p' (HyLight runs --num_pairs 0),
 * remove_branches with remove_trans != 1 (the reference asserts).  add_duplicates and resolve_orientations = false are not
 * options here: this call always resolves orientations by labelling.  branch_reduction is hlmi_vq_branch_graph, below; this
 * call never reduces branches by read evidence.  remove_trans > 3 is HLMI_EINVAL. */
int hlmi_vq_graph(const char *singles_fastq, const char *overlaps, const hlmi_vq_graph_opts *o, const char *out_dir,
                  hlmi_vq_graph_stats *st);

/* ---- SRBuilder with --cliques=false --error_correction=false --threads 1 (ViralQuasispecies.cpp:413-447,
 * SRBuilder::mergeAlongEdges, SRBuilder.cpp:1238-1384): the contigs of the next stage-b iteration ---------------------- */
/* SRBuilder::consensus with error_correction = false (SRBuilder.cpp:406-533) and consensus_pos (:297-402) for two sequences
 * that are already oriented, the second one `pos` bases behind the first; computed by the device kernel hlmi_vq_merge
 * uses.  seq1 / seq2 hold len1 / len2 bases of A C G T N, qual1 / qual2 hold qlen1 / qlen2 quality characters '!' .. '~'
 * (anything else: HLMI_EINVAL; the reference asserts).  out_seq / out_qual need room for max(len1, pos + len2) bytes (no
 * NUL is added); *out_len = that length, or 0 where the reference returns an empty consensus: a position without an active
 * base (pos > len1: the loop of :453-521 meets :498), or a read whose position reaches the end of its sequence or of its
 * quality string while it is active (:478: an empty sequence, a quality string shorter than its sequence).  pos == len1
 * is NOT empty: read 1 goes inactive at its last base (:487-492) and read 2 becomes active at position pos (:455-459).
 * minQual is the reference's default 0.9 (ViralQuasispecies.cpp:62 -> SRBuilder.h:89; HyLight's path does not pass
 * --min_qual); hlmi_vq_consensus_pair_mq, below, takes another.  Per position (:297-402): log10 / pow / round are the host's libm in the reference's expression order, kept
 * in tables by (bases, qualities) - the device only looks up.  A position with ONE active base goes through consensus_pos
 * too: the base comes back with its quality except that Q0 and Q1 give another base (the three others score higher: an A
 * becomes T, a T, C or G becomes A; quality '#' for Q0, '"' for Q1), and an N comes back as N with quality '$' (:354-357).
 * Two different bases of equal quality give N '$': each has probability 1/2 < minQual. */
int hlmi_vq_consensus_pair(const char *seq1, const char *qual1, uint32_t len1, uint32_t qlen1, const char *seq2,
                           const char *qual2, uint32_t len2, uint32_t qlen2, uint32_t pos, char *out_seq, char *out_qual,
                           uint32_t *out_len);
/* ---- --min_qual.  Every hlmi_vq_*_mq call is its sibling with ViralQuasispecies' --min_qual as one more argument, in front of
 * out_dir (here: of out_seq); the sibling is the same call at 0.9.  A column of two bases and more whose best base is less than
 * min_qual sure is N (SRBuilder.cpp:362-368); 0 never writes such an N, which is what POLYTE passes ("never insert N's",
 * polyte.tune_params.py:737).  The value reaches the three places a column is decided: the tables of one and two bases, the
 * pile-up kernel's comparison, and the host's redo of a column the kernel hands back; through the 'N's, test_N_rate.  What
 * changes below 1/2: two different bases of equal quality score exactly alike and consensus_pos picks by its chain A, T, C, G
 * (:390-393): A beats everything, T beats C, G loses to all; A/Q40 against G/Q40 at min_qual 0 is A with quality '$'
 * (p_incorrect 0.500017).  And where both bases are Q0 or Q1 - each more likely wrong than right - the best score belongs to
 * the bases that were NOT read, and the first of those in the chain is written (A/Q0 against C/Q0: T).
 * HLMI_EINVAL, before any file is written: min_qual outside [0, 1], a NaN included; and a min_qual at which the reference's
 * answer for two bases depends on the order it sums four probabilities in, so that no table by quality holds it.  With glibc
 * that is 1 alone (1 - p_incorrect < 1 is decided by the last bit of a quotient: twice C at Q61 / Q93 is N, twice A is A);
 * every other value tried, 0.999999 among them, builds. */
int hlmi_vq_consensus_pair_mq(const char *seq1, const char *qual1, uint32_t len1, uint32_t qlen1, const char *seq2,
                              const char *qual2, uint32_t len2, uint32_t qlen2, uint32_t pos, double min_qual, char *out_seq,
                              char *out_qual, uint32_t *out_len);
typedef struct {
    int first_it;               /* --first_it: every read is its own original (OverlapGraph::buildOriginalsDict, :772-798) */
    uint32_t keep_singletons;   /* --keep_singletons: an unmerged read shorter than this is not kept (:1286)               */
    int store_tips_separately;  /* --separate_tips: an unmerged tip read goes to removed_tip_sequences.fastq (:1305)       */
    uint32_t min_clique_size;   /* --min_clique_size: read for parity only - a pair never exceeds 3 * min_clique_size
                                   (:721) and without error correction the minimum support is not applied (:420-437)     */
} hlmi_vq_merge_opts;
/* pipeline_per_stage.py:170-203 on HyLight's path: keep_singletons = max(min_overlap_len, min_read_len) = 300,
 * separate_tips true, min_clique_size 2, first_it true */
void hlmi_vq_merge_opts_stageb(hlmi_vq_merge_opts *o);
typedef struct {
    uint64_t pairs;             /* edges taken by getEdgesForMerging                                                        */
    uint64_t merged;            /* super-reads written from them                                                            */
    uint64_t dropped_empty;     /* pairs whose consensus is empty                                                           */
    uint64_t dropped_n;         /* pairs whose consensus fails test_N_rate                                                  */
    uint64_t trivial;           /* unmerged reads written as they are                                                       */
    uint64_t trivial_reverse;   /* ... of them reverse-complemented                                                         */
    uint64_t short_reads;       /* unmerged reads left out: shorter than keep_singletons                                    */
    uint64_t n_reads;           /* ... too many N                                                                           */
    uint64_t inclusion_reads;   /* ... included in another read (to removed_tip_sequences.fastq)                            */
    uint64_t tip_reads;         /* ... tips (to removed_tip_sequences.fastq)                                                */
    uint64_t bases_in;          /* bases of singles_fastq                                                                   */
    uint64_t bytes_out;         /* bytes of the new singles.fastq                                                           */
    double ms_merge;            /* wall time of the step after the graph                                                    */
} hlmi_vq_merge_stats;
/* hlmi_vq_graph (same code, same files in out_dir) and then the reference's next step.  subreads_in: the subreads.txt of
 * the previous iteration when first_it is 0 (buildOriginalsDict, OverlapGraph.cpp:799-845), NULL when first_it is set.
 * Written into out_dir in the reference's formats:
 *   singles.fastq   the merged super-reads, ids from 0 in merge-list order (writeSinglesToFile, :1471-1507), then the
 *                   unmerged reads in ascending vertex order (writeTrivialsToFile, :1416-1469); a read whose vertex
 *                   orientation is reverse is written reverse-complemented with its qualities reversed (:1331-1368)
 *   subreads.txt    per new read: "<id>" and per original read "\t<original>:<+|->:<index>:<length>" (:1449-1463, :1489-1503)
 *   removed_tip_sequences.fastq   only when a read goes there (writeTipsToFile, :1386-1414): the unmerged inclusions and
 *                   tips in vertex order, forward, ids from 0.  The reference APPENDS to this file; so does this call
 *   superread_map.txt   the project's own: per vertex "vertex<TAB>new id or -1<TAB>offset of the read in its super-read
 *                   <TAB>+|-" - what visited, nodes_to_new_IDs and the subread map hold for findNextOverlaps
 * Rules:
 *   merge list   getEdgesForMerging (GraphAlgos.cpp:112-148): vertices ascending, each free vertex with its first free
 *                out-neighbour in the order sortEdges leaves (ViralQuasispecies.cpp:434)
 *   placement    the smaller vertex is the base (constructSuperread, :658-679); the edge is getEdgeInfo(base, other): base ->
 *                other if there is one, else other -> base; the other read lies at +pos1 when the base is the edge's read 1,
 *                else at -pos1 (sort_vertices, :87-148), so the edge's read 1 starts the super-read and its read 2 lies pos1
 *                behind; reads are reverse-complemented by their vertex orientation; length = base + left + right
 *                extension (:224-252)
 *   drops        an empty consensus, or Read::test_N_rate (Read.h:214-233: kept when N_count < 0.05 * length, compared as
 *                doubles); the vertices of a dropped pair stay unvisited and come back as unmerged reads
 *   unmerged     in this order (:1282-1372): shorter than keep_singletons; N rate; inclusion (with ignore_inclusions);
 *                tip (with store_tips_separately); else written, forward as it is or reversed with its originals mirrored
 *   originals    calcSubreadInfo (:536-595) and :750-806: first_it: index = offset of the read in the super-read; else a
 *                forward read adds its offset, a reverse read gives |read| + offset - (length + index); the base vertex's
 *                entry wins where both reads hold one original
 * Deviations (stated): the contract is --threads 1 (with more, the reference concatenates per-thread results in the order
 * their critical sections run, :1004-1011).  The entries of a subreads.txt line are in ascending original id (the reference:
 * iteration order of a libstdc++ unordered_map; its only reader puts them back into a map).  Paired reads are not built:
 * HLMI_ESTATE as for hlmi_vq_graph; the empty paired1.fastq / paired2.fastq the reference leaves behind are not written,
 * nor merge_self_overlap / filter_subreads (a pair never exceeds 3 * min_clique_size).  A read with a character outside
 * A C G T N, a quality outside '!' .. '~' or a quality line of another length than its sequence is HLMI_EINVAL (the
 * reference asserts on the first two and would drop every merge of the third).  When the graph has no edge the reference
 * returns before this step (ViralQuasispecies.cpp:282-291): so does this call, and none of the four files is written. */
int hlmi_vq_merge(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                  const hlmi_vq_merge_opts *mo, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst);
/* hlmi_vq_merge with --min_qual (see hlmi_vq_consensus_pair_mq); hlmi_vq_merge is this call at 0.9 */
int hlmi_vq_merge_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                     const hlmi_vq_merge_opts *mo, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                     hlmi_vq_merge_stats *mst);

/* ---- SRBuilder with --cliques=true --threads 1 on single-end reads (ViralQuasispecies.cpp:397-428: quick-cliques'
 * `qc --algorithm=degeneracy --input-file=graph.txt > cliques.txt`, then SRBuilder::cliquesToSuperreads, SRBuilder.cpp:
 * 1031-1235): the step POLYTE runs in the first iteration of every cluster, in its branch-reduction iterations and in the
 * diploid stage (polyte.tune_params.py:607-645).  It ends where hlmi_vq_merge ends: in front of findNextOverlaps. */
typedef struct {
    uint32_t min_clique_size;   /* --min_clique_size: smaller cliques give no super-read; 1 .. 21                           */
    int error_correction;       /* --error_correction: trim to the columns with min_clique_size reads (:420-473)            */
    int first_it;               /* as hlmi_vq_merge_opts                                                                    */
    uint32_t keep_singletons;   /* an unvisited read shorter than this is left out (:1149)                                  */
} hlmi_vq_clique_opts;
/* What run_viralquasispecies passes (polyte.tune_params.py:684-738): first_it 1; keep_singletons 1000 with error correction,
 * else 0; min_clique_size 2, as HyLight calls POLYTE (HyLight.py:228-242).  The matching graph options are the caller's to
 * set in hlmi_vq_graph_opts: remove_trans 2 with error correction, else 1; remove_branches 1 on the --no_EC first iteration
 * (cliques with neither error correction nor a haplotype coverage), else 0; remove_backedges 0 with error correction, else 1
 * (ViralQuasispecies.cpp); remove_tips 0; ignore_inclusions 0; edge_threshold = POLYTE's --edge1.
 * Not an option of this struct: run_viralquasispecies always adds --min_qual=0 (:737), so the reference never turns a column
 * into N for disagreement.  That is the min_qual argument of hlmi_vq_cliques_mq, hlmi_vq_clique_iteration_mq and
 * hlmi_vq_branch_iteration_mq: with these options and min_qual 0 the call is POLYTE's call of ViralQuasispecies.  hlmi_vq_cliques
 * itself keeps minQual at SRBuilder's default 0.9 - columns whose best base is less than 90 % sure become N, and a super-read
 * can fall to the N rate where POLYTE keeps it - and reproduces ViralQuasispecies at its default --min_qual.  The loop POLYTE
 * runs around these calls (polyte.tune_params.py:583-682) is hylight_amd/polyte.py, its threshold table hylight_amd/min_ev.py. */
void hlmi_vq_clique_opts_polyte(hlmi_vq_clique_opts *o, int error_correction);
typedef struct {
    uint64_t cliques_read;      /* lines of cliques.txt, its two text lines included (clique_count, :1057)                  */
    uint64_t singletons;        /* lines with one vertex (:1075)                                                            */
    uint64_t below_min;         /* lines with 2 .. min_clique_size - 1 vertices                                             */
    uint64_t taken;             /* cliques of min_clique_size and more: one constructSuperread each (:1078)                 */
    uint64_t filtered;          /* ... of more than 3 * min_clique_size vertices, cut down by filter_subreads (:721)        */
    uint64_t superreads;        /* super-reads written                                                                      */
    uint64_t dropped_empty;     /* cliques whose consensus is empty (:478, :498)                                            */
    uint64_t dropped_n;         /* ... fails test_N_rate (:999)                                                             */
    uint64_t dropped_support;   /* ... has no entry number min_clique_size (:427-432)                                       */
    uint64_t trivial;           /* reads in no kept super-read, written as they are                                         */
    uint64_t trivial_reverse;   /* ... of them reverse-complemented                                                         */
    uint64_t short_reads;       /* reads left out: shorter than keep_singletons                                             */
    uint64_t n_reads;           /* ... too many N                                                                           */
    uint64_t columns;           /* consensus columns of the cliques whose consensus is not empty                            */
    uint64_t columns_host;      /* ... of them redone on the host: too close to a threshold for the device's pow / log10    */
    uint64_t bases_in;          /* bases of singles_fastq                                                                   */
    uint64_t bytes_out;         /* bytes of the new singles.fastq                                                           */
    double ms_cliques;          /* wall time of the step after the graph                                                    */
} hlmi_vq_clique_stats;
/* The maximal cliques of graph_txt - vertex count, edge-line count, then every edge as "u,v" and "v,u", as hlmi_vq_graph
 * writes it - into cliques_out, byte for byte what `qc --algorithm=degeneracy --input-file=graph.txt` prints to stdout: its
 * two text lines ("NOTE: Quick Cliques v2.0beta.", "Reading .edges file format. "), then one clique per line, every vertex
 * followed by a blank.  The order of the lines and of the vertices in a line are the enumerator's (Eppstein-Loeffler-Strash
 * over a degeneracy order, quick-cliques/src/DegeneracyAlgorithm.cpp): they decide the id of every new read.  PARITY PINNED:
 * tests/golden/fxK_*.cliques.txt were printed by the reference's binary.  *n_cliques = the clique lines.  Host code: needs
 * no GPU.  HLMI_EINVAL: a file that does not hold its counts and that many "u,v" lines, a vertex outside 0 .. n - 1, a loop,
 * a vertex with n or more edge lines (the reference asserts or indexes out of bounds).  The reference picks another reader
 * for a file name holding ".graph"; this call always reads the format of graph.txt. */
int hlmi_vq_cliques_of_graph(const char *graph_txt, const char *cliques_out, uint64_t *n_cliques);
/* hlmi_vq_graph (same code, same files in out_dir) and then the clique step.  subreads_in as for hlmi_vq_merge.  Written into
 * out_dir:
 *   cliques.txt     as hlmi_vq_cliques_of_graph writes it for out_dir's graph.txt
 *   singles.fastq   the super-reads, ids from 0 in the order of their lines in cliques.txt (writeSinglesToFile), then the
 *                   vertices in no KEPT super-read in ascending order (:1145-1222), reverse ones reverse-complemented
 *   subreads.txt    as hlmi_vq_merge writes it
 *   clique_map.txt  the project's own: per super-read "id<TAB>trim_pos" and per member, in the order of sorted_vertices,
 *                   "<TAB>vertex:offset:+|-" - offset = index1 - startpos1 of calcSubreadInfo (negative for a read that
 *                   starts in front of trim_pos): what findNextOverlaps reads of a super-read
 * Rules (constructSuperread :654-870 with the 's' branch only, per line of min_clique_size vertices and more):
 *   placement    sort_vertices (:33-286): base = the smallest vertex; for every other member in ascending order the edge is
 *                getEdgeInfo(base, v), its offset +pos1 when the base is the edge's read 1, else -pos1; it goes in front of the
 *                first list entry whose offset is not smaller (equal offsets: the later member first); offsets shifted to start
 *                at 0; length = base + largest left + largest right extension; reads reverse-complemented by vertex label
 *   filtering    more than 3 * min_clique_size members (:721-734, filter_subreads :597-636): the leftmost min_clique_size
 *                entries, the base, then entries by descending end position until 2 * min_clique_size are chosen, where
 *                sortVerticesByEndpos is libstdc++'s std::sort over (vertex, end) in list order, compared by end alone -
 *                ties fall as that algorithm leaves them, and the host calls the same std::sort; the chosen keep list order;
 *                the originals still see every member
 *   consensus    (:406-533) read r counts in column c when pos_r <= c < pos_r + len_r.  Without error correction every
 *                column is written and a column without a read empties the consensus.  With it trim_pos = the offset of entry
 *                number min_clique_size; the output starts there and stops in front of the first column with fewer than
 *                min_clique_size reads at which every read has started; the consensus is empty when a column in between has
 *                no read or when a read that starts in front of trim_pos ends at or before it
 *   column       consensus_pos (:297-402) as for hlmi_vq_consensus_pair, the scores summed in list order.  One or two bases:
 *                the tables of hlmi_vq_merge.  More: the sums (of libm's log10 values, plain double adds) are the reference's
 *                bit for bit and decide the base; the device computes pow, log10 and round itself and hands a column to
 *                the host's libm when a comparison lies within the margin of DESIGN.md section 4.3f (columns_host), so every
 *                byte is the reference's arithmetic.  minQual is the default 0.9 as for hlmi_vq_merge; hlmi_vq_cliques_mq
 *                takes another
 *   drops        an empty consensus, test_N_rate; the members stay unvisited unless another kept super-read holds them
 *   trivial      an unvisited read: left out when shorter than keep_singletons or failing the N rate, else written forward
 *                or reversed with mirrored originals.  No inclusion or tip rule on this path
 *   originals    :750-806 over the clique in ascending vertex order, the first vertex holding an original wins; first_it:
 *                index = offset; else the forward / reverse formulas of hlmi_vq_merge.  Lines in ascending original id
 * When the graph has no edge the call stops where hlmi_vq_graph stops.  HLMI_ESTATE: a paired-end row, as elsewhere.
 * HLMI_EINVAL: min_clique_size 0; min_clique_size above 21 (a pile-up then never exceeds 63 reads, which one wave handles);
 * the reads hlmi_vq_merge refuses.  remove_multi_occ, merge_self_overlap (paired only) and threads > 1 are not options here:
 * the contract is the sequential reference with a clique kept whole.  --min_qual is hlmi_vq_cliques_mq. */
int hlmi_vq_cliques(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                    const hlmi_vq_clique_opts *co, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst);
/* hlmi_vq_cliques with --min_qual (see hlmi_vq_consensus_pair_mq; POLYTE: 0); hlmi_vq_cliques is this call at 0.9.  Towards
 * min_qual 1 more columns of three bases and more lie within the device's margin of the threshold and are redone on the host
 * (columns_host): the output is the same, the call slower.  At 0 none does: the best of four is at least 1/4 sure. */
int hlmi_vq_cliques_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                       const hlmi_vq_clique_opts *co, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                       hlmi_vq_clique_stats *cst);

/* ---- SRBuilder::findNextOverlaps with --FNO=1 --optimize=false --cliques=false --error_correction=false --threads 1, to the
 * end of main (FindNextOverlaps.cpp:25-327 updateOverlap, :331-347 findCliqueIndex, :351-565 computeOverlapData - the S-S
 * branch :357-385 only -, :605-631 reconsiderEdgeOverlaps, :635-697 reconsiderNonedgeOverlaps, :816-887
 * findInclusionOverlaps, :890-958 findNextOverlaps, ViralQuasispecies.cpp:449-479): the overlaps of the next iteration. */
typedef struct {
    int no_inclusion_overlaps;  /* --no_inclusion_overlaps: lines with percentage 100 are left out (:68, :145, :223, :320)  */
} hlmi_vq_next_opts;
/* pipeline_per_stage.py does not pass the option: 0 */
void hlmi_vq_next_opts_stageb(hlmi_vq_next_opts *o);
typedef struct {
    uint64_t src_graph;         /* source edges: the final graph's out-lists (:612-623)                                     */
    uint64_t src_branching;     /* ... branching_edges: tip edges, removeBranches' edges, back edges (:628-629)            */
    uint64_t src_nonedge;       /* ... rows of nonedge_overlaps.txt that were kept (:697)                                   */
    uint64_t nonedge_skipped;   /* rows left out because checkEdge(v1, v2, reverse allowed) > 0 (:694-696)                  */
    uint64_t src_induced;       /* ... edges induced through an included vertex and kept: checkEdge == -1 (:876-879)        */
    uint64_t copied, u2sr, v2sr, sr2sr;   /* the reference's four counters: lines per case, before identical lines collapse  */
    uint64_t claims_failed;     /* owners of a key whose computeOverlapData failed (new_pos1 >= len, :378-384)              */
    uint64_t lines;             /* distinct lines = the lines of overlaps.txt = the third column of the stats.txt line      */
    double ms_next;             /* wall time of the step after the merge                                                    */
} hlmi_vq_next_stats;
/* One stage-b iteration: hlmi_vq_merge (same code, same files in out_dir), then overlaps.txt - the std::set<std::string> of
 * :918-948 in ascending byte order, one '\n' per line - and one line APPENDED to stats.txt: "<vertices>\t<edges of the final
 * graph>\t<lines>\n" (ViralQuasispecies.cpp:472-479).  All inputs are read before any output is written: the iteration loop
 * calls this with singles_fastq, overlaps and subreads_in lying in out_dir under the names it writes.  When the graph has
 * no edge the call stops where hlmi_vq_merge stops: no overlaps.txt, no stats.txt line.
 * Source edges, in this order (the order decides which one owns a key):
 *   1  the final graph: vertices ascending, each out-list in the order of the sortEdges of ViralQuasispecies.cpp:434
 *   2  branching_edges in push order: the tip edges in ascending (source, target) (GraphAlgos.cpp:630-636), the edges
 *      removeBranches removed (:918-931), the back edges reportCycle removed (OverlapGraph.cpp:548-560), each as it stood
 *   3  the rows of nonedge_overlaps.txt in file order as score-0 edges (:661-691), a row left out when
 *      checkEdge(v1, v2, true) > 0: the score of the first v1 -> v2 of v1's list, else of the first v2 -> v1
 *   4  per included vertex (ascending; its out-edges, then per in-neighbour the first edge from it: GraphAlgos.cpp:26-42,
 *      copied after the labelling) every pair i < j of the list that chains through it (:841-865): score = edge_threshold,
 *      len = min(|r1| - pos1, |r2|), perc = floor(100 * len / min(|r1|, |r2|)) in integers; kept when checkEdge == -1
 * Per source edge u -> v (updateOverlap): both unvisited: the edge is copied with the new ids, its own positions, perc and
 * lengths (:47-72); a vertex in a super-read stands for that super-read, lying at its offset (:73-326): new_pos1 = pos1 +
 * offset(u) - offset(v); negative: the second entity comes first, new_pos1 = -new_pos1, len = its length; overlap length =
 * min(len - new_pos1, len1, len2); percentage = (int)floor(max(ol / float(len1), ol / float(len2)) * 100) with the
 * division and the product rounded to float one after the other; no line when new_pos1 >= len.  A vertex that is visited
 * but in no super-read (too short, N rate, inclusion, tip: SRBuilder.cpp:1286-1311) gives nothing; the same super-read on
 * both sides is skipped (:255).  A case with a super-read first claims (min id, max id) in overlaps_found (:84-97, :162-175,
 * :261-273): the first source edge in the order above owns the pair, later ones are dropped, and when the owner's
 * computeOverlapData fails the pair gets no line.  Copied edges never consult the table.  ori1 / ori2: for a score-0 edge
 * '+' where the edge's orientation equals the vertex label, else '-' (:34-37); '+' for every other edge.
 * Device: one thread per source edge for case and key (a candidate in the words of hlmi_vq_clique_iteration, whose lists make
 * several of one edge), a stable radix sort of (key, sequence number) and its run heads for the claims, one thread per line for the text, LSD radix passes over the lines' 8-byte big-endian words for the order (a
 * line padded with zero bytes orders as the string does) - lines longer than 64 bytes make the call order on the host.
 * Refused with HLMI_ESTATE before anything is written: a paired-end row ('p') among the candidates or the non-edge rows.
 * add_duplicates and resolve_orientations = false are not options; FindNextOverlaps3 is not built; behind the cliques:
 * hlmi_vq_clique_iteration. */
int hlmi_vq_iteration(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                      const hlmi_vq_merge_opts *mo, const hlmi_vq_next_opts *no, const char *out_dir, hlmi_vq_graph_stats *gst,
                      hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst);
/* hlmi_vq_iteration with --min_qual (see hlmi_vq_consensus_pair_mq); hlmi_vq_iteration is this call at 0.9 */
int hlmi_vq_iteration_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts *go,
                         const hlmi_vq_merge_opts *mo, const hlmi_vq_next_opts *no, double min_qual, const char *out_dir,
                         hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst);

/* ---- findNextOverlaps behind the cliques: ViralQuasispecies --cliques=true --FNO=1 --optimize=false --threads 1 on
 * single-end reads to the end of main - what POLYTE runs in the first iteration of every cluster and in every
 * branch-reduction iteration (polyte.tune_params.py:607-645, --FNO=1 at :698). */
typedef struct {
    uint64_t src_graph, src_branching, src_nonedge, nonedge_skipped, src_induced;   /* as hlmi_vq_next_stats               */
    uint64_t copied, u2sr, v2sr, sr2sr;
    uint64_t claims_failed;
    uint64_t lines;
    uint64_t candidates;        /* turns of updateOverlap's three loops (:78, :156, :233-253) after the id1 == id2 skip of  */
                                /* :255; a copied edge (:47-72) runs no loop and is not counted                             */
    uint64_t max_list;          /* the longest super-read list of a vertex (nodes_to_SR, :896-913)                          */
    uint64_t in_several;        /* vertices in two or more kept super-reads                                                 */
    double ms_next;             /* wall time of the step after the clique step                                              */
} hlmi_vq_clique_next_stats;
/* One clique iteration: hlmi_vq_cliques (same code, same files in out_dir), then overlaps.txt and one line APPENDED to
 * stats.txt, both exactly as hlmi_vq_iteration documents them.  All inputs are read before any output is written, so
 * singles_fastq, overlaps and subreads_in may lie in out_dir under the names written here.  When the graph has no edge the
 * call stops where hlmi_vq_cliques stops: no overlaps.txt, no stats.txt line.
 * What differs from hlmi_vq_iteration is one fact: behind mergeAlongEdges a vertex lies in one super-read at the most, behind
 * cliquesToSuperreads in a LIST of them, and updateOverlap loops over the list of u, of v, or over their product.
 *   the list      (FindNextOverlaps.cpp:896-913) of vertex v: the KEPT super-reads whose sorted_clique(0) holds v - every
 *                 member of the clique, those filter_subreads left out of the pile-up included (SRBuilder.cpp:864) - in
 *                 ascending super-read id (single_SR_vec order, :900-906).  A dropped clique (empty consensus, N rate, no
 *                 support) adds nothing
 *   visited       (SRBuilder.cpp:1125-1160) the members of kept super-reads; an unvisited vertex that is shorter than
 *                 keep_singletons or fails the N rate is marked visited with an EMPTY list - every source edge at it gives
 *                 nothing -; every other unvisited vertex is copied under a new id (nodes_to_new_IDs, :1219)
 *   index         findCliqueIndex (:331-347) = index1 - startpos1 of calcSubreadInfo (SRBuilder.cpp:536-595) = the offset
 *                 column of clique_map.txt: NEGATIVE for a read that starts in front of trim_pos under error correction.
 *                 new_pos1 = pos1 + idx(u) - idx(v) (:360) is signed arithmetic throughout
 *   loop order    per source edge u -> v (:47, :73, :151, :229): both unvisited: copied; u unvisited: the list of v (:78); v
 *                 unvisited: the list of u (:156); both visited: the list of u outer, the list of v inner (:233, :253), and
 *                 id1 == id2 is skipped BEFORE the claim (:255).  Every turn claims (min id, max id) in overlaps_found before
 *                 computeOverlapData runs (:84-97, :162-175, :261-273): the first turn in source-edge order, then loop order,
 *                 owns the pair, and an owner that fails (new_pos1 >= len, :378-384) leaves the pair without a line though a
 *                 later turn might have succeeded
 *   source edges  the four groups of hlmi_vq_iteration in its order, with one difference in group 1: the --cliques=true branch
 *                 never runs the sortEdges of ViralQuasispecies.cpp:434 (:417-428), so reconsiderEdgeOverlaps (:612) and
 *                 checkEdge walk each out-list as cycleRemovalHeuristic left it: the order of the sortEdges of :359 without
 *                 the back edges that were removed.  The two orders differ only where std::sort moves tying keys of a sorted
 *                 list (more than 16 edges, two of one length to one target); this call carries the unsorted lists then.
 *                 What hlmi_vq_cliques writes does not depend on it and is unchanged
 * Device: one thread per source edge counts its turns (|list(u)| * |list(v)|, 64 bits), one exclusive scan numbers them, one
 * thread per turn finds its edge by binary search and works out case, ids, indices and claim key; the turn's number is the
 * reference's loop order and the sequence number of the stable claim sort.  No thread or wave loops over a list: a vertex in
 * hundreds of super-reads costs as many threads as it has turns.  Everything behind that - claims, computeOverlapData, text,
 * order - is hlmi_vq_iteration's code; there, and wherever no list holds more than one entry, a source edge is its own turn
 * and needs no count, scan or search.
 * HLMI_EINVAL: 2^32 - 1 turns and more in one call (the limit of the sequence numbers); what hlmi_vq_cliques refuses.
 * HLMI_ESTATE: a paired-end row among the candidates or the non-edge rows.  Paired-end reads, add_duplicates and
 * FindNextOverlaps3 (--FNO=3) are not built, as for hlmi_vq_cliques; --min_qual is hlmi_vq_clique_iteration_mq; BranchReduction
 * is hlmi_vq_branch_iteration, below. */
int hlmi_vq_clique_iteration(const char *singles_fastq, const char *overlaps, const char *subreads_in,
                             const hlmi_vq_graph_opts *go, const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no,
                             const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst,
                             hlmi_vq_clique_next_stats *nst);
/* hlmi_vq_clique_iteration with --min_qual (see hlmi_vq_cliques_mq): with hlmi_vq_clique_opts_polyte, its graph options and
 * min_qual 0, a POLYTE first-iteration call.  hlmi_vq_clique_iteration is this call at 0.9 */
int hlmi_vq_clique_iteration_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in,
                                const hlmi_vq_graph_opts *go, const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no,
                                double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst,
                                hlmi_vq_clique_next_stats *nst);

/* ---- read-evidence branch reduction: ViralQuasispecies --branch_reduction=true --remove_branches=false --remove_trans=1
 * --threads 1 on single-end reads, diploid off (BranchReduction::readBasedBranchReduction, BranchReduction.cpp; the
 * edges_to_be_deleted rule of removeTransitiveEdges, GraphAlgos.cpp:967-1077) - the iteration POLYTE runs after every merge
 * round (polyte.tune_params.py:641-645).  PARITY UNPINNED; tests/vq_branch_model.py restates the reference. */
typedef struct {
    uint32_t se_count, pe_count;   /* --branch_SE_c / --branch_PE_c: the original reads are numbered singles, /1 mates, /2
                                      mates; se_count + 2 * pe_count must be the number of reads of original_fastq, and is
                                      what this call takes for --original_readcount                                         */
    int careful;                   /* --careful_diploid: a component next to a kept one is removed (default true, :97)      */
} hlmi_vq_branch_opts;
void hlmi_vq_branch_opts_polyte(hlmi_vq_branch_opts *o);       /* careful 1, the counts 0 */
typedef struct {
    uint64_t in_branches, out_branches;   /* vertices with more than one in- / out-edge (findBranchfreeGraph)              */
    uint64_t pairs;                /* neighbour pairs compared on the device (inclusion pairs are not)                      */
    uint64_t diff_positions;       /* first-difference positions they gave, at most 100 each                                */
    uint64_t work_items;           /* (branch, neighbour, original of the neighbour) triples of the evidence kernel         */
    uint64_t evidence_ids;         /* evidence ids over all (branch, neighbour) lists, sorted and uniqued                   */
    uint64_t missing_edges;        /* identical overlaps: edges pushed to branching_edges for the next iteration            */
    uint64_t false_branches;       /* branching vertices with one                                                           */
    uint64_t inclusion_pairs;      /* pairs of an out-branch decided by the lengths (:449, :461)                            */
    uint64_t components;           /* branching components without a false branch                                           */
    uint64_t components_kept;      /* ... with an edge of enough unique evidence                                            */
    uint64_t dist_too_large;       /* ... whose distance the table does not hold                                            */
    uint64_t scheduled;            /* edges_to_be_deleted of removeTransitiveEdges (the 3-clique rule)                      */
    uint64_t edges_removed;        /* edges_to_remove after sort and unique                                                 */
    double ms_diff, ms_evidence;   /* wall time of the two device steps (upload, kernel, download)                          */
    double ms_branch;              /* wall time of the whole reduction                                                      */
} hlmi_vq_branch_stats;
/* hlmi_vq_graph (same code, same files) with the reduction where removeBranches would run (ViralQuasispecies.cpp:326-351) and
 * the 3-clique rule in removeTransitiveEdges, plus the project's own branch_components.txt: one line per component of
 * branching_components in the reference's order, "dist<TAB>threshold (-1: not in the table)<TAB>kept 0|1" and per edge
 * "<TAB>u>v:unique evidence count" (-1 where countUniqueEvidence never ran: no threshold, or next to a kept component).
 * subreads_in: the previous iteration's subreads.txt (NULL: every read is its own original, --first_it);  original_fastq: the
 * reads the originals name, looked up by id;  threshold_table: the reference's evidence_threshold_table.tsv ('#' and empty
 * lines skipped, column 1 = distance, column 3 = minimum evidence, std::stoi each).
 * Device: one wave per neighbour pair of a branch walks the common stretch 64 bases a step (reversed for in-branches) and
 * appends the first 100 mismatch positions by ballot and popcount; one thread per (branch, neighbour, original) looks the id
 * and its mate up in the branching vertex's id-sorted originals and tests the original read against the neighbour at the
 * branch's difference list.  Components, unique evidence, thresholds and removals run on the host.
 * Refused before anything is written: remove_trans != 1, remove_branches set, se_count + 2 * pe_count != reads of
 * original_fastq, a table that cannot be opened or holds a line std::stoi rejects, an original id that original_fastq does not
 * hold, read ids that are not the file positions (HLMI_EINVAL); a paired-end row (HLMI_ESTATE).  Refused during the reduction
 * (HLMI_EINVAL): an in-branch pair the reference's assertion of :605 rejects.  The table is read as the reference reads it,
 * through one stringstream: what a line holds behind its third column goes in front of the next line's first column.
 * Not built: diploid (the typical-double-branch resolution), paired-end vertices (POLYTE as HyLight runs it needs neither; its
 * loop is hylight_amd/polyte.py, its threshold table hylight_amd/min_ev.py).  The graph has no consensus in it: --min_qual belongs to hlmi_vq_branch_iteration_mq. */
int hlmi_vq_branch_graph(const char *singles_fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                         const char *threshold_table, const hlmi_vq_graph_opts *go, const hlmi_vq_branch_opts *bo,
                         const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_branch_stats *bst);
/* The same graph, then everything hlmi_vq_clique_iteration does behind its graph (same code): one branch-reduction iteration of
 * POLYTE.  co->first_it decides the originals as there (subreads_in NULL only with first_it). */
int hlmi_vq_branch_iteration(const char *singles_fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                             const char *threshold_table, const hlmi_vq_graph_opts *go, const hlmi_vq_branch_opts *bo,
                             const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no, const char *out_dir,
                             hlmi_vq_graph_stats *gst, hlmi_vq_branch_stats *bst, hlmi_vq_clique_stats *cst,
                             hlmi_vq_clique_next_stats *nst);
/* hlmi_vq_branch_iteration with --min_qual for its clique step (see hlmi_vq_cliques_mq; POLYTE: 0); hlmi_vq_branch_iteration
 * is this call at 0.9 */
int hlmi_vq_branch_iteration_mq(const char *singles_fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                                const char *threshold_table, const hlmi_vq_graph_opts *go, const hlmi_vq_branch_opts *bo,
                                const hlmi_vq_clique_opts *co, const hlmi_vq_next_opts *no, double min_qual, const char *out_dir,
                                hlmi_vq_graph_stats *gst, hlmi_vq_branch_stats *bst, hlmi_vq_clique_stats *cst,
                                hlmi_vq_clique_next_stats *nst);

/* ---- short-read clustering (HyLight.py:215-226: get_readnames.py, bin_pointer_limited_filechunks_shortpath2.py,
 * getclusters.py, get_fq_cluster.py with cwd = tmp/ and run id HiStrain).  Parity pinned: tests/golden/fxH_cluster_*.json
 * hold what the reference scripts themselves wrote. */
typedef struct {
    int64_t size;             /* HyLight --size: the cluster size cap (default 15000)                                   */
    int32_t threads;          /* HyLight -t: chunks per session and the slicing of getclusters.py (default 20), 1..100  */
    int32_t pad;
    uint64_t window_bytes;    /* PAF bytes uploaded per window of whole sessions (0: 512 MiB; at most 2 GiB; a window
                                 holds one session at least, so 1 gives one session per window)                          */
} hlmi_cluster_opts;
void hlmi_cluster_opts_default(hlmi_cluster_opts *o);
typedef struct {
    uint64_t names;           /* lines of readnames.txt (nodes)                                                          */
    uint64_t rows;            /* PAF rows                                                                                */
    uint64_t chunks;          /* chunkify's byte chunks of 2 600 000 bytes to the end of a line                         */
    uint64_t sessions;        /* groups of `threads` chunks                                                              */
    uint64_t windows;         /* PAF windows uploaded                                                                    */
    uint64_t survivors;       /* rows kept by the prefilter (different clusters, size1 + size2 < size at session start)  */
    uint64_t strict_rejects;  /* rows refused only because size1 + size2 == size at session start                        */
    uint64_t unions;          /* merges of the sequential pass                                                           */
    uint64_t clusters_ge20;   /* final clusters of size >= 20                                                            */
    uint64_t reads_sliced;    /* reads of clusters >= 20 dropped by getclusters' slicing                                 */
    uint64_t files;           /* .fq files written (2 per JSON key)                                                      */
    double ms_fastq, ms_paf, ms_prefilter, ms_union, ms_refresh, ms_group, ms_demux, ms_write, ms_total;
} hlmi_cluster_stats;
/* Clusters the short reads of `fastq` by the overlap rows of `paf` (the scored 14-column shortr2.paf, LF line ends) and
 * writes into out_dir (which must exist), byte for byte as the reference leaves it after its cmd_rm: readnames.txt,
 * HiStrain_max<size>_final_clusters_grouped.json and fq_<size>/<cid>/<cid>.1.fq and .2.fq for every JSON key (both always
 * created; fq_<size>/ exists even when there is no key).  Nothing else is left behind; an existing fq_<size>/ is replaced
 * whole.  Rules (script line numbers in DESIGN.md):
 *   names      FASTQ line i % 4 == 0 holding "/1" anywhere -> line[1:-3]; node id = rank; lookup key = that after rstrip
 *   rows       PAF columns 1 and 6 minus their last two characters
 *   sessions   2 600 000-byte chunks to the end of a line, `threads` chunks per session; every row of a session is
 *              tested against the state frozen at its start (kept iff the cluster ids differ and size1 + size2 < size),
 *              the kept ones are merged in file order against the live state (size1 + size2 <= size); the root with the
 *              shorter path hangs under the other, ties hang root 1 under root 2; cluster id = rank of the root
 *   grouping   nodes of clusters >= 20 in readnames order; only the first min(threads, 60) * int(K / threads) survive;
 *              JSON keys: slice 0's ids ascending, then each later slice's new ids ascending (json.dump defaults)
 *   demux      record -> cluster of re.split('[@/]', header)[-2]; .1.fq if the header matches /1$, else .2.fq
 * Refused with HLMI_EINVAL (the reference would crash, truncate a chunk silently, or parse the text otherwise), before
 * anything is written: threads < 1 or > 100, size < 1; an empty FASTQ, a FASTA input, a FASTQ header line without '@',
 * '\r' or a byte >= 0x80 in the FASTQ; a duplicate readnames name or one with '"'; in the PAF '\r', a byte >= 0x80,
 * '"' or another str.splitlines() separator (\v \f \x1c-\x1e), a row with fewer than 12 columns, an endpoint whose
 * name is not in readnames. */
int hlmi_cluster_short(const char *paf, const char *fastq, const hlmi_cluster_opts *o, const char *out_dir,
                       hlmi_cluster_stats *st);

/* ---- contig polishing (replaces the external `racon --no-trimming -u` of HyLight.py:152,182,203) ------------------------
 * A function of the project's own, NOT racon's: racon re-aligns with a partial-order aligner; this call only counts the
 * columns of the CIGARs the overlapper wrote.  Parity unpinned; tests/polish_model.py is the contract, byte for byte. */
typedef struct {
    int min_len;              /* rows with te - ts below this are dropped                                                 */
    double min_iden;          /* rows with (sum of '=' lengths) / (sum of all op lengths) below this are dropped         */
    int min_cov;              /* votes a position needs to be decided, rows a slot needs to be opened (>= 1)              */
    int include_unpolished;   /* racon's -u: a contig without a selected row is written as it is                          */
} hlmi_polish_opts;
void hlmi_polish_opts_default(hlmi_polish_opts *o);   /* 0, 0.0, 3, 1 */
typedef struct {
    uint64_t rows;              /* PAF rows                                                                                 */
    uint64_t rows_selected;     /* rows that vote (one per read at most)                                                    */
    uint64_t contigs;           /* records of `contigs`                                                                     */
    uint64_t contigs_polished;  /* ... with a selected row                                                                  */
    uint64_t substituted;       /* positions decided as a base other than the contig's own (upper-cased)                    */
    uint64_t deleted;           /* positions decided as `del`                                                               */
    uint64_t inserted_bases;    /* bases written at opened slots                                                            */
    uint64_t slots_opened;
    uint64_t ins_long;          /* (row, slot) pairs whose insertion is longer than 16 bases: the row spans, it does not insert */
    uint64_t ins_edge;          /* I ops at the very start or end of a selected row's CIGAR: they belong to no slot         */
    double ms_device;           /* wall time of the device part: uploads, kernels, read-backs                               */
    double ms_total;
} hlmi_polish_stats;
/* contigs, reads: FASTA or FASTQ; paf: rows of >= 12 columns whose LAST field is a cg:Z: CIGAR in = X I D (what hlmi_ava
 * writes).  Writes the polished contigs to out_fa (under a temporary name, renamed on success).
 * Refused with HLMI_EINVAL before anything is written (the message names the 1-based PAF line; malformed rows - columns,
 * integers, strand, CIGAR numbers - of the whole file are reported before the following): no cg:Z: tag; an op other than
 * = X I D; a query name not in `reads`; a target name not in `contigs`; coordinates outside the sequences (the sequences'
 * own lengths count, not columns 2 and 7); sum(= X D) != te - ts; sum(= X I) != qe - qs.  Also min_cov < 1, and a
 * sequence of 2^28 bases or more.  A name that occurs twice means its first record.  An op of length 0 is no op.
 * Row selection, in this order: rows with qname == tname are skipped; rows with te == ts or te - ts < min_len are dropped;
 * rows with (double)n_eq / (double)n_all < min_iden are dropped; per query name the row with the largest te - ts stays,
 * the earliest line on a tie (one row per read is racon's rule as well).
 * Votes: alignment column i of a row reads read[qs + i] on strand '+' and the complement of read[qe - 1 - i] on '-',
 * upper-cased.  Position p in [ts, te): an = or X column votes its base if that is A, C, G or T and nothing otherwise; a D
 * column votes `del`.  Slot p, ts < p < te, is the gap in front of position p: every selected row with ts < p < te spans
 * it; the I ops the row has there (none of = X D between them) are concatenated; a row with 1..16 bases there inserts
 * them, one with more spans without inserting (ins_long); I ops at p == ts or p == te belong to no slot (ins_edge).
 * Decisions: position: c = its votes; c < min_cov: the contig's byte stays, case included; else the symbol with the most
 * votes, on a tie the contig's own upper-cased base if it is among the tied ones, else the first of A, C, G, T, del; del
 * omits the position.  Slot: s spanning rows, i inserting rows; opened when s >= min_cov and 2 i > s; its length is the
 * most frequent one among the inserting rows (tie: the smallest), base j the most frequent of A, C, G, T at index j among
 * the rows that insert exactly that length (tie: the first of A, C, G, T; none: N).
 * Output: the contigs in file order, two lines each: ">name LN:i:<new length> RC:i:<rows selected on it> XC:f:<share of
 * its positions with c >= min_cov, %.6f>"; a contig without a selected row is written as ">name" and its bytes when
 * include_unpolished is set, else left out; a contig whose consensus is empty is not written.
 * Device: every counter is 32 bits wide, so coverage has no limit below 2^32 rows. */
int hlmi_polish(const char *contigs, const char *reads, const char *paf, const hlmi_polish_opts *o, const char *out_fa,
                hlmi_polish_stats *st);
/* The two calls hlmi_ava(contigs, reads, ao, P) and hlmi_polish(contigs, reads, P, po, out_fa, st) in one, without the PAF P:
 * out_fa and every integer field of *st are byte for byte what that chain gives (ao NULL: hlmi_ava's default, the long
 * constants).  No PAF is written and no row or CIGAR op travels to the host: the overlapper's rows are selected, ordered and
 * compacted in device memory (csrc/polish_rows.hip; a row's index there is its line in P) and the reads are voted from the
 * overlapper's resident copy.  Three differences from the chain:
 *  - two records of one name in `reads`, or in `contigs`, are HLMI_EINVAL before anything is written (the chain aligns the
 *    second record and then votes with the first record's bases);
 *  - ao->stub_oh >= 0 is HLMI_EINVAL: the bare rows of stub candidates have no CIGAR (the chain refuses those rows too);
 *  - 2^32 overlapper rows or more are HLMI_EINVAL.
 * hlmi_polish's own refusals that can still occur are kept: min_cov < 1, a sequence of 2^28 bases or more, 2^31 contig
 * bases to polish in one call.  What hlmi_polish checks only because a PAF is foreign text does not arise here. */
int hlmi_polish_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_opts *po,
                      const char *out_fa, hlmi_polish_stats *st);

/* ---- polishing with base qualities (racon weights every base of a FASTQ read by its Phred score and, -q 10, drops reads of a
 * mean quality below 10).  hlmi_polish_q and hlmi_polish_reads_q are hlmi_polish and hlmi_polish_reads with these two rules as
 * options; the two older calls keep their signatures and their bytes, and HLMI_ABI_VERSION stays where it is (new symbols, as
 * for the hlmi_vq_*_mq calls).  A function of the project's own like hlmi_polish: PARITY with racon UNPINNED;
 * tests/polish_qual_model.py is the contract, byte for byte. */
typedef struct {
    int min_len;              /* the four fields of hlmi_polish_opts, with their meaning                                  */
    double min_iden;
    int min_cov;
    int include_unpolished;
    int qual_weight;          /* 0: every vote weighs 1 (hlmi_polish's function); 1: the rules below                      */
    double min_avg_qual;      /* 0.0: off; else rows of reads whose mean Phred is below it are dropped (racon -q)          */
} hlmi_polish_qopts;
void hlmi_polish_qopts_default(hlmi_polish_qopts *o);   /* 0, 0.0, 3, 1, 1, 10.0 */
typedef struct {
    hlmi_polish_stats base;
    uint64_t reads_with_qual;   /* records of `reads` that have a quality string                                           */
    uint64_t rows_low_qual;     /* rows dropped because their query's mean quality is below min_avg_qual                   */
} hlmi_polish_qstats;
/* Where a rule below is silent, hlmi_polish's rule holds unchanged.
 * Qualities: a FASTQ record's quality string must be as long as its bases and every quality byte must be in 33..126;
 * otherwise the call returns HLMI_EINVAL, names the record, and writes nothing (whatever the two options are; also
 * min_avg_qual negative or not a number).  Weight of a read base: w = max(1, byte - 33).  A FASTA record has no qualities:
 * each of its bases weighs 1, and min_avg_qual never drops it.  reads_with_qual = the number of records that have a quality
 * string.
 * Read floor: a read with qualities is low when (double)sum(byte - 33) / (double)len < min_avg_qual, the sum over the whole
 * record (a record of no bases is never low).  Rows whose query is a low read are dropped directly after the
 * qname == tname skip and counted in rows_low_qual (every row is still checked as hlmi_polish checks it).  With
 * min_avg_qual == 0.0 the test is not made.
 * Alignment-column order: on strand '-' the qualities are reversed together with the bases: column i has the quality of
 * read[qe - 1 - i].
 * Position votes (qual_weight = 1): an = / X column with an A C G T base adds its w to that symbol.  A D op adds the same weight
 * to `del` on each of its columns: min(w of query column qc - 1, w of query column qc), qc the first query column behind
 * the op, only the columns that exist inside [0, qe - qs) counting; with neither present the weight is 1.  The coverage test
 * stays a count: c = number of voting columns, decided when c >= min_cov.  The winner is the symbol with the largest weight
 * sum; on a tie the contig's own upper-cased base if it is among the tied, otherwise the first of A, C, G, T, del.
 * Slots: spanning rows, inserting rows and the opening test (s >= min_cov and 2 i > s) stay counts, as do ins_long and
 * ins_edge.  An inserting row's length vote weighs the minimum w over its 1..16 inserted bases; the length with the largest
 * sum wins, on a tie the smallest.  Base j: among the rows that insert exactly the winning length each adds the w of its
 * base j; the largest sum wins, on a tie the first of A, C, G, T; with no A C G T there the base is N.
 * Counter width: counters stay 32 bits wide; with qual_weight = 1 a call whose rows_selected x 93 >= 2^32 is HLMI_EINVAL
 * before anything is written.
 * Identities: with qual_weight = 0 and min_avg_qual = 0.0 both calls give hlmi_polish's / hlmi_polish_reads's file and `base`
 * stats byte for byte; so they do with qual_weight = 1 on a FASTA read file or on a FASTQ file whose qualities are all '"'
 * (Q1): every weight is then 1. */
int hlmi_polish_q(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, const char *out_fa,
                  hlmi_polish_qstats *st);
/* hlmi_polish_reads with the same options: the file and every integer stat equal the chain hlmi_ava -> hlmi_polish_q; the three
 * stated differences of hlmi_polish_reads still apply.  The read floor is applied where the rows are selected (a low row
 * claims nothing, so it cannot shadow a shorter row of another read); rows_low_qual comes from a device counter. */
int hlmi_polish_reads_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_qopts *po,
                        const char *out_fa, hlmi_polish_qstats *st);

/* ---- strain-aware polishing: only the pairs a list names vote.  HyLight's strain awareness is the SNP-support filter of its
 * overlap stage (filter_overlap_slr2.py), and the reference hands racon the FILTERED read-to-contig rows (HyLight.py:152,182,203:
 * ov_long_ref.paf, ov_long_ref2.paf, shortr1.paf).  hlmi_polish_pairs and hlmi_polish_reads_pairs are hlmi_polish_q and
 * hlmi_polish_reads_q with such a list as an option; the older calls keep their signatures and their bytes, and HLMI_ABI_VERSION
 * stays where it is (new symbols).  A rule of the project's own: PARITY with racon UNPINNED; tests/polish_pairs_model.py is the
 * contract, byte for byte. */
typedef struct {
    hlmi_polish_qstats q;
    uint64_t pairs_listed;     /* distinct unordered pairs of two different names of the list with BOTH names known          */
    uint64_t pairs_unknown;    /* list rows with a name that is neither a read nor a contig of this call (ignored)           */
    uint64_t rows_not_listed;  /* alignment rows dropped because their pair is not listed                                    */
} hlmi_polish_pstats;
/* Where a rule below is silent, hlmi_polish_q's rule holds unchanged.
 * No list: with pairs_paf == NULL the call is hlmi_polish_q: the same file, the same `q` stats, the three counters 0.
 * List file format: a PAF-like text, in practice the stage's scored 14-column rows.  Lines end at '\n'; a last line without
 * one counts; a '\r' in front of the '\n' belongs to the line's last field and is not stripped.  Fields are split at TAB and
 * only fields 1 and 6 are read: 12-column PAF, the stage's 14-column rows and rows with tags are all accepted.  A line with fewer
 * than 6 fields, an empty line included, is HLMI_EINVAL; the message names the 1-based line and nothing is written.  An empty
 * file is a valid list of no pairs: no row votes.
 * Meaning: a name is known when it is the name of a record of `reads` or of `contigs`.  A list row with an unknown name is
 * ignored and counted in pairs_unknown (the driver's ov_long_ref.paf grows by rows against other contig sets).  An alignment
 * row (query q, target t) is listed when some list row of two known names has fields (1, 6) equal to (q, t) or to (t, q),
 * compared byte for byte: the order inside a list row does not matter.  Duplicate list rows are allowed.  A list row that names
 * one name twice lists nothing (rows with qname == tname are skipped before the list is asked) and counts nowhere.
 * Where in the selection: qname == tname skip; the read floor (rows_low_qual); a row that is not listed is dropped and counted
 * in rows_not_listed; then te == ts / min_len; min_iden; one row per read.  A row that is not listed claims nothing: it cannot
 * shadow a shorter listed row of the same read.
 * Refusals: every refusal of hlmi_polish_q about the options, the files and the rows comes first, in its order; then a list that
 * cannot be read (HLMI_EIO) or has a short line; then the refusals about the selected rows (the counter width, 2^31 contig
 * bases).  Nothing is written in any of these cases. */
int hlmi_polish_pairs(const char *contigs, const char *reads, const char *paf, const hlmi_polish_qopts *o, const char *pairs_paf,
                      const char *out_fa, hlmi_polish_pstats *st);
/* hlmi_polish_reads_q with the same option: the file and every integer stat equal the chain hlmi_ava -> hlmi_polish_pairs.  The
 * list never visits the host's parser: its bytes go to the device, where the lines are split, fields 1 and 6 are looked up in a
 * hash table of the call's names and the listed pairs become a sorted array of keys that the row selection searches
 * (csrc/polish_pairs.hip).  The aligner still aligns every pair; the list only decides who votes.  One more refusal: a list of
 * 2^31 bytes or more is HLMI_EINVAL. */
int hlmi_polish_reads_pairs(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_polish_qopts *po,
                            const char *pairs_paf, const char *out_fa, hlmi_polish_pstats *st);

/* ---- read depth and relative abundance per contig: how many of the selected reads lie over every position of the contigs, and
 * each contig's share of the sample.  hlmi_depth reads a PAF as hlmi_polish_pairs does, hlmi_depth_reads aligns in the call as
 * hlmi_polish_reads_pairs does.  New symbols: the older calls keep their signatures and their bytes, and HLMI_ABI_VERSION stays
 * where it is.  A function of the project's own (the reference's build_abundance_between_contigs*.py are overlap filters, not an
 * abundance estimate): PARITY UNPINNED; tests/depth_model.py is the contract, byte for byte. */
typedef struct {
    int min_len;              /* rows with te - ts below this are dropped                                                 */
    double min_iden;          /* rows with (sum of '=' lengths) / (sum of all op lengths) below this are dropped         */
} hlmi_depth_opts;
void hlmi_depth_opts_default(hlmi_depth_opts *o);   /* 0, 0.0 */
typedef struct {
    uint64_t rows;              /* PAF rows / overlapper rows                                                               */
    uint64_t rows_selected;     /* rows that count (one per read at most)                                                   */
    uint64_t contigs;           /* records of `contigs`                                                                     */
    uint64_t contigs_covered;   /* ... with a selected row                                                                  */
    uint64_t positions;         /* bases of ALL contigs                                                                     */
    uint64_t covered;           /* positions with depth >= 1, over all contigs                                              */
    uint64_t bases;             /* sum of the depths, over all contigs                                                      */
    uint64_t runs;              /* bedGraph lines written (0 when out_bedgraph is NULL)                                     */
    uint64_t pairs_listed;      /* the three counters of hlmi_polish_pstats; 0 without a list                              */
    uint64_t pairs_unknown;
    uint64_t rows_not_listed;
    double ms_device;           /* wall time of the device part: uploads, kernels, read-backs                               */
    double ms_total;
} hlmi_depth_stats;
/* contigs, reads, paf: as for hlmi_polish_pairs.  pairs_paf and out_bedgraph may be NULL.
 * Selection: exactly hlmi_polish_pairs's without the quality floor: rows with qname == tname are skipped; with a list, a row
 * whose pair is not listed is dropped and counted in rows_not_listed; rows with te == ts or te - ts < min_len are dropped; rows
 * with (double)n_eq / (double)n_all < min_iden are dropped; per query name the row with the largest te - ts stays, the earliest
 * line on a tie.  The list's format and meaning are hlmi_polish_pairs's, word for word (pairs_paf == NULL: no list, every row
 * may count; an empty file: a valid list of no pairs, no row counts).  The polisher and this call run one implementation.
 * Depth: a selected row covers every position of [ts, te) of its contig, the columns of its D ops included; depth[p] is the
 * number of selected rows that cover p.  No CIGAR op is read behind the selection.
 * Per contig, in file order, EVERY contig: length; reads = selected rows on it; bases = sum of its depths; covered = positions
 * with depth >= 1; mean_depth = (double)bases / (double)length; median_depth = element (length - 1) / 2 (integer division) of
 * its depths in ascending order; abundance = mean_depth / (sum of all mean_depth), the sum taken in file order with one double
 * addition per contig, 0.000000 when the sum is 0.  A contig of 0 bases gets a row of zeros.
 * out_tsv (under a temporary name, renamed on success): the line
 * "#contig\tlength\treads\tbases\tcovered\tmean_depth\tmedian_depth\tabundance", then one line per contig; mean_depth and
 * abundance print as %.6f, everything else is an integer.
 * out_bedgraph (optional): lines "name\tstart\tend\tdepth": the maximal runs of equal depth inside one contig, depth 0 included,
 * contigs in file order, runs ascending; a run never continues into the next contig; a contig without a selected row is one run
 * [0, length) of depth 0, a contig of 0 bases writes nothing.
 * Refusals (HLMI_EINVAL unless said otherwise, nothing is written): every refusal hlmi_polish_pairs makes about the files, the rows
 * and the list, in its order (min_cov and the counter width do not apply); 2^31 bases or more of contigs with a selected row;
 * depths and sort keys that do not fit the device's memory.  Two records of one name in `contigs`, or in `reads`, are refused
 * when the files are read: the table is keyed by name. */
int hlmi_depth(const char *contigs, const char *reads, const char *paf, const hlmi_depth_opts *o, const char *pairs_paf,
               const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st);
/* The two calls hlmi_ava(contigs, reads, ao, P) and hlmi_depth(contigs, reads, P, o, pairs_paf, ...) in one, without the PAF P:
 * both files and every integer field of *st are byte for byte what that chain gives (ao NULL: the long constants).  The
 * overlapper's rows are selected where they are, by the kernels hlmi_polish_reads_pairs selects with; a selected row's span is
 * all that is read of it (csrc/depth.hip).  The three stated differences of hlmi_polish_reads apply (a name twice, stub_oh >= 0,
 * 2^32 rows), the list refusals of hlmi_polish_reads_pairs, a sequence of 2^28 bases or more, and 2^31 contig bases. */
int hlmi_depth_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_depth_opts *o,
                     const char *pairs_paf, const char *out_tsv, const char *out_bedgraph, hlmi_depth_stats *st);

/* ---- variant sites per contig: the positions where a second symbol has real support among the selected reads' votes - a
 * collapsed strain, a mis-join or a polishing error - and per contig how many there are.  A contig without a site is strain-pure
 * as far as the reads can tell.  hlmi_variants reads a PAF as hlmi_depth does, hlmi_variants_reads aligns in the call as
 * hlmi_depth_reads does.  New symbols: the older calls keep their signatures and their bytes, and HLMI_ABI_VERSION stays where it
 * is.  A function of the project's own: PARITY UNPINNED; tests/variants_model.py is the contract, byte for byte. */
typedef struct {
    int min_len;              /* selection, as hlmi_depth_opts                                                             */
    double min_iden;
    int min_cov;              /* votes a position needs to be callable (>= 1)                                              */
    int min_alt;              /* votes the alternative symbol needs (>= 1)                                                 */
    double min_frac;          /* ... and its share of the position's votes, in [0, 1]                                      */
} hlmi_variant_opts;
void hlmi_variant_opts_default(hlmi_variant_opts *o);   /* 0, 0.0, 3, 2, 0.2 */
typedef struct {
    uint64_t rows;              /* PAF rows / overlapper rows                                                               */
    uint64_t rows_selected;     /* rows that vote (one per read at most)                                                    */
    uint64_t contigs;           /* records of `contigs`                                                                     */
    uint64_t contigs_covered;   /* ... with a selected row                                                                  */
    uint64_t positions;         /* bases of ALL contigs                                                                     */
    uint64_t callable;          /* positions with votes >= min_cov whose own base is A C G T                                */
    uint64_t ref_other;         /* positions with votes >= min_cov whose own byte is not A C G T                            */
    uint64_t sites;             /* sites = sites_base + sites_del                                                           */
    uint64_t sites_base;        /* ... whose alternative is a base                                                          */
    uint64_t sites_del;         /* ... whose alternative is del                                                             */
    uint64_t pairs_listed;      /* the three counters of hlmi_polish_pstats; 0 without a list                              */
    uint64_t pairs_unknown;
    uint64_t rows_not_listed;
    double ms_device;           /* wall time of the device part: uploads, kernels, read-backs                               */
    double ms_total;
} hlmi_variant_stats;
/* contigs, reads, paf: as for hlmi_depth.  pairs_paf and out_summary may be NULL.
 * Selection: exactly hlmi_depth's, run by the same code: hlmi_polish_pairs's selection without the quality floor, the list's
 * format and meaning word for word (pairs_paf == NULL: no list, every row may vote; an empty file: a valid list of no pairs, no
 * row votes).
 * Votes: exactly hlmi_polish's position votes, unweighted.  A selected row's '=' or 'X' column votes its read base at the
 * column's contig position if that base is A, C, G or T of either case (strand '-': its complement) and nothing otherwise; a 'D'
 * column votes del.  Slots (the columns of I ops) and base qualities take no part.
 * Site rule at position p: v[A], v[C], v[G], v[T], v[del] are the votes and c their sum; own is the contig's byte, upper-cased.
 * c < min_cov: the position is not callable.  c >= min_cov and own is not A C G T: the position counts in ref_other and is never a
 * site.  Otherwise the position is callable; alt is the symbol other than own with the most votes, on a tie the first in the
 * order A, C, G, T, del; the position is a site iff v[alt] >= min_alt and (double)v[alt] / (double)c >= min_frac (one IEEE
 * division).  own may be the minority symbol: the position is still a site, with alt chosen by the same rule.
 * out_sites (under a temporary name, renamed on success): the line
 * "#contig\tpos\tref\tdepth\tA\tC\tG\tT\tdel\talt\talt_count\talt_frac", then one line per site, contigs in file order,
 * positions ascending: pos is 1-based, ref the upper-cased own base, depth is c, then the five votes, alt the letter or '*' for
 * del, alt_count = v[alt], alt_frac the quotient above as %.6f.  With no site the file is the header line alone.
 * out_summary (optional): the line "#contig\tlength\treads\tcallable\tsites\tsite_rate", then one line per contig in file order,
 * EVERY contig, those without a selected row and those of 0 bases included (zeros): reads = selected rows on it; site_rate =
 * (double)sites / (double)callable as %.6f, 0.000000 when callable is 0.
 * Refusals (HLMI_EINVAL unless said otherwise, nothing is written): min_cov < 1, min_alt < 1, min_frac outside [0, 1] or not a
 * number; then every refusal hlmi_depth makes about the files, the rows and the list, in its order: two records of one name in
 * `contigs` or in `reads` (the tables are keyed by name), and 2^31 bases or more of contigs with a selected row, among them. */
int hlmi_variants(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, const char *pairs_paf,
                  const char *out_sites, const char *out_summary, hlmi_variant_stats *st);
/* The two calls hlmi_ava(contigs, reads, ao, P) and hlmi_variants(contigs, reads, P, o, pairs_paf, ...) in one, without the PAF P:
 * both files and every integer field of *st are byte for byte what that chain gives (ao NULL: the long constants).  The
 * overlapper's rows are selected and compacted where they are, by the kernels hlmi_polish_reads_pairs runs, and voted from the
 * overlapper's resident read codes (csrc/variants.hip).  The three stated differences of hlmi_polish_reads apply (a name twice,
 * stub_oh >= 0, 2^32 rows), the list refusals of hlmi_polish_reads_pairs, a sequence of 2^28 bases or more, and 2^31 contig
 * bases. */
int hlmi_variants_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o,
                        const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);

/* ---- variant sites with insertion sites: hlmi_variants reports nothing where the reads carry bases the contig lacks; these calls
 * add the slots' votes - hlmi_polish's slots - and list the slots where inserting rows have real support, whether or not
 * hlmi_polish would open them (it opens a slot only when 2 i > s).  hlmi_variants_ins reads a PAF as hlmi_variants does,
 * hlmi_variants_reads_ins aligns in the call as hlmi_variants_reads does.  New symbols: the older calls keep their signatures and
 * their bytes, and HLMI_ABI_VERSION stays where it is.  Options: hlmi_variant_opts unchanged; min_cov, min_alt and min_frac rule
 * the slots as they rule the positions.  A function of the project's own: PARITY UNPINNED; tests/variants_ins_model.py is the
 * contract, byte for byte. */
typedef struct {
    uint64_t rows;              /* the thirteen integer fields of hlmi_variant_stats, with hlmi_variants's values         */
    uint64_t rows_selected;
    uint64_t contigs;
    uint64_t contigs_covered;
    uint64_t positions;
    uint64_t callable;
    uint64_t ref_other;
    uint64_t sites;
    uint64_t sites_base;
    uint64_t sites_del;
    uint64_t pairs_listed;
    uint64_t pairs_unknown;
    uint64_t rows_not_listed;
    uint64_t slots_callable;    /* slots with s >= min_cov                                                                  */
    uint64_t ins_sites;         /* ... that are insertion sites                                                             */
    uint64_t ins_long;          /* as hlmi_polish_stats counts them: (row, slot) with more than 16 inserted bases           */
    uint64_t ins_edge;          /* ... and I ops at a row's ts or te                                                        */
    double ms_device;           /* wall time of the device part: uploads, kernels, read-backs                               */
    double ms_total;
} hlmi_variant_ins_stats;
/* contigs, reads, paf, o, pairs_paf, out_sites, out_summary: as for hlmi_variants; out_ins must not be NULL.
 * Selection, position votes, out_sites: exactly hlmi_variants's, run by the same code; out_sites is byte for byte the file
 * hlmi_variants writes for the same arguments.  With a pair list an unlisted row neither votes nor spans nor inserts.
 * Slots: hlmi_polish's definition, unweighted.  Slot p, 0 < p < length, is the gap in front of 0-based position p.  A selected row
 * with ts < p < te spans it; s counts the spanning rows.  A row's I ops there are concatenated (one op of the compact CIGAR: I ops
 * with nothing or only zero-length ops between them).  A row with 1..16 bases there inserts; i counts the inserting rows.  A row
 * with more than 16 bases there is a long row; l counts the long rows, and such a row also counts in ins_long.  I ops at p == ts or
 * p == te belong to no slot and count in ins_edge.  A row whose column at p votes nothing (an N) still spans; a row that starts at
 * p does not span.
 * Insertion site rule: a slot is callable iff s >= min_cov and counts in slots_callable; a callable slot is an insertion site iff
 * i + l >= min_alt and (double)(i + l) / (double)s >= min_frac (one IEEE division).  The contig's own byte at p or p - 1 plays no
 * part: a slot next to an N can be a site.
 * Per site: len is the most frequent length among the i inserting rows, on a tie the smallest, 0 when i == 0; len_count the number
 * of rows with that length; seq[j] the most frequent of A, C, G, T at index j among the rows that insert exactly len bases, on a
 * tie the first of A, C, G, T, with none N - hlmi_polish's slot decisions.  Strand '-' rows insert the reverse complement.
 * out_ins (under a temporary name, renamed on success): the line
 * "#contig\tpos\tref\tspan\tins\tins_long\tins_frac\tlen\tlen_count\tseq", then one line per insertion site, contigs in file
 * order, slots ascending: pos = p, the 1-based position of the base in front of the inserted bases (VCF's convention), ref that
 * base, upper-cased, span = s, ins = i, ins_long = l, ins_frac the quotient above as %.6f, len and len_count as above, seq the len
 * bases or '*' when len is 0.  With no insertion site the file is the header line alone.
 * out_summary (optional): hlmi_variants's line plus three columns:
 * "#contig\tlength\treads\tcallable\tsites\tsite_rate\tslots\tins_sites\tins_rate": slots = callable slots, ins_rate =
 * (double)ins_sites / (double)slots as %.6f, 0.000000 when slots is 0; the first six columns are byte for byte hlmi_variants's.
 * Refusals (HLMI_EINVAL, nothing is written): out_ins == NULL first, then hlmi_variants's refusals in its order.
 * One count pass holds the five symbol counters and four slot counters per position (csrc/variants.hip); the lengths and bases of
 * the insertion sites are voted by hlmi_polish's slot kernels, and 40 bytes per insertion site come to the host. */
int hlmi_variants_ins(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts *o, const char *pairs_paf,
                      const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st);
/* The two calls hlmi_ava(contigs, reads, ao, P) and hlmi_variants_ins(contigs, reads, P, o, pairs_paf, ...) in one, without the PAF
 * P: the three files and every integer field of *st are byte for byte what that chain gives (ao NULL: the long constants).  It
 * refuses as hlmi_variants_reads does, behind out_ins == NULL. */
int hlmi_variants_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_opts *o,
                            const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                            hlmi_variant_ins_stats *st);

/* ---- variant calls with base qualities: in the four calls above every vote counts the same, a Q3 base like a Q40 base, which on
 * noisy reads is the main source of false sites.  The _q forms add what pile-up callers have (samtools mpileup -Q / -q): a
 * per-base floor - a column below it casts no vote, exactly as an N column casts none - and hlmi_polish_q's read floor.  A floor
 * and not hlmi_polish_q's weights: min_alt, depth, alt_count and alt_frac are counts of reads and stay counts.  New symbols: the
 * older calls keep their signatures and their bytes, and HLMI_ABI_VERSION stays where it is.  The default floors 10 and 10.0 are
 * --polish_min_avg_qual's value; no real data in this repository supports either figure.  A function of the project's own: PARITY
 * UNPINNED; tests/variants_qual_model.py is the contract, byte for byte. */
typedef struct {
    int min_len;              /* the five fields of hlmi_variant_opts, same meaning                                          */
    double min_iden;
    int min_cov;
    int min_alt;
    double min_frac;
    int min_base_qual;        /* 0: off; 1..93: a column whose Phred is below it casts no vote                               */
    double min_avg_qual;      /* 0.0: off; else hlmi_polish_q's read floor, word for word                                    */
} hlmi_variant_qopts;
void hlmi_variant_qopts_default(hlmi_variant_qopts *o);   /* 0, 0.0, 3, 2, 0.2, 10, 10.0 */
typedef struct {
    uint64_t reads_with_qual;   /* as hlmi_polish_qstats                                                                    */
    uint64_t rows_low_qual;
    uint64_t columns_low_qual;  /* (selected row, column) votes withheld by the base floor                                  */
} hlmi_variant_qcounts;
/* Where a rule below is silent, the rule of hlmi_variants / hlmi_variants_ins holds.
 * Qualities: validation, reads_with_qual, the read floor and rows_low_qual follow hlmi_polish_q, run by the same code: a record's
 * quality string must be as long as its bases and hold bytes of 33..126 only (HLMI_EINVAL naming the record); a read whose mean
 * Phred is below min_avg_qual is low, and a row whose query is a low read is dropped directly behind the qname == tname skip - in
 * front of the pair list - and counted in rows_low_qual.  On strand '-', column i has the quality of read[qe - 1 - i].
 * Column Phred: q = byte - 33.  An '=' / 'X' column whose base is A C G T passes iff q >= min_base_qual.
 * D op: its q is the lower q of query columns qc - 1 and qc, qc the first query column behind the op, only the columns that exist
 * inside [0, qe - qs) counting; with neither present the op passes.  All columns of the op pass or fail together.
 * A failing column casts no vote and counts once in columns_low_qual (in the first pass over the tiles only, never again when a
 * tile is revisited for its records).  A column that would have voted nothing anyway (N, other bytes) counts nowhere new.  c,
 * depth, the five counts, callable, ref_other and the site rule then follow from the remaining votes unchanged.
 * FASTA records have no qualities: every column of such a read passes every floor, and the read is never low.
 * Slots (the _ins_q forms): a failing column still spans - it is counted where an N column is counted.  span, ins, ins_long,
 * len, len_count and seq take no quality into account: they differ from hlmi_variants_ins's only through rows the read floor
 * dropped.  out_sites of an _ins_q call is byte for byte the _q call's.
 * Refusals (HLMI_EINVAL, nothing is written): min_base_qual outside 0..93, or min_avg_qual negative or not a number, before
 * anything is read; then out_ins == NULL for the _ins_q forms; then the older call's refusals, in its order.  There is no
 * rows_selected x 93 refusal: the counters hold counts.
 * Identities: the calls give the older calls' files and every integer stat byte for byte with min_base_qual = 0 and min_avg_qual =
 * 0.0; on a FASTA `reads` file at any floors; and on a FASTQ whose bytes all pass and whose reads are all above the read floor.
 * The _reads_q forms: the files and the integer fields equal the chain hlmi_ava -> hlmi_variants_q (or hlmi_variants_ins_q); the
 * three stated differences of hlmi_variants_reads still apply. */
int hlmi_variants_q(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts *o, const char *pairs_paf,
                    const char *out_sites, const char *out_summary, hlmi_variant_stats *st, hlmi_variant_qcounts *qc);
int hlmi_variants_reads_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_qopts *o,
                          const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st,
                          hlmi_variant_qcounts *qc);
int hlmi_variants_ins_q(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts *o, const char *pairs_paf,
                        const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st,
                        hlmi_variant_qcounts *qc);
int hlmi_variants_reads_ins_q(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_variant_qopts *o,
                              const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                              hlmi_variant_ins_stats *st, hlmi_variant_qcounts *qc);

/* ---- phased variant sites: do the minor alleles of neighbouring sites ride on the same reads (a collapsed sister strain that can
 * be separated) or not (noise, a mis-join, a polishing error), and which read belongs to which side.  hlmi_phase reads a PAF as
 * hlmi_variants does, hlmi_phase_reads aligns in the call as hlmi_variants_reads does.  New symbols: the older calls keep their
 * signatures and their bytes, and HLMI_ABI_VERSION stays where it is.  A function of the project's own: PARITY UNPINNED;
 * tests/phase_model.py is the contract, byte for byte. */
typedef struct {
    int min_len;              /* the five fields of hlmi_variant_opts, same meaning and defaults                           */
    double min_iden;
    int min_cov;
    int min_alt;
    double min_frac;
    int min_link;             /* informative rows a link needs to be phased (>= 1)                                         */
    double min_agree;         /* ... and the share of them on the link's majority side, in (0.5, 1]                        */
} hlmi_phase_opts;
void hlmi_phase_opts_default(hlmi_phase_opts *o);   /* 0, 0.0, 3, 2, 0.2, 3, 0.8 */
typedef struct {
    uint64_t rows;              /* the thirteen integer fields of hlmi_variant_stats, with hlmi_variants's values         */
    uint64_t rows_selected;
    uint64_t contigs;
    uint64_t contigs_covered;
    uint64_t positions;
    uint64_t callable;
    uint64_t ref_other;
    uint64_t sites;
    uint64_t sites_base;
    uint64_t sites_del;
    uint64_t pairs_listed;
    uint64_t pairs_unknown;
    uint64_t rows_not_listed;
    uint64_t links;             /* pairs of consecutive sites of one contig                                                 */
    uint64_t links_phased;
    uint64_t blocks;
    uint64_t blocks_multi;      /* blocks of two or more sites                                                              */
    uint64_t sites_phased;      /* sites inside blocks of two or more sites                                                 */
    uint64_t alleles;           /* sum over the selected rows of the sites inside [ts, te): the size of the allele table    */
    uint64_t read_records;      /* lines of out_reads (counted also when out_reads is NULL)                                 */
    uint64_t reads_a;           /* ... with hap A, B, -                                                                     */
    uint64_t reads_b;
    uint64_t reads_tie;
    double ms_device;           /* wall time of the device part: uploads, kernels, read-backs                               */
    double ms_total;
} hlmi_phase_stats;
/* contigs, reads, paf: as for hlmi_variants.  pairs_paf, out_links and out_reads may be NULL.
 * Sites: exactly hlmi_variants's - the same selection (the pair list included, an empty list included), the same votes, the same
 * site rule, run by the same code.  A site has own (A C G T) and alt (A C G T del).
 * A row's allele at a site p of its contig: the symbol the row votes at p under hlmi_variants's vote rule is 0 if it is own, 1
 * if it is alt, 2 if it is another of the five symbols; none if the row does not cover p or its column at p votes nothing (an N
 * of the read).  A D column votes del.  I columns take no part, but they do shift the query column.
 * Links: one per pair of consecutive sites of one contig, in ascending order; a link never joins two contigs.  Over the rows whose
 * allele is 0 or 1 at both sites: n00, n01, n10, n11, the first digit the allele at the left site; cis = n00 + n11, trans = n01 +
 * n10, inf = cis + trans, top = max(cis, trans).  The link is phased iff inf >= min_link and (double)top / (double)inf >= min_agree
 * (one IEEE division); its direction is cis if cis > trans, otherwise trans.
 * Blocks: a maximal run of consecutive sites of one contig joined by phased links; a site with no phased link is a block of one.
 * A block's id is the 1-based position of its first site.  Phase bit: 0 at the block's first site, at each following site the
 * previous bit XOR (the link is trans).  Hap A carries own where the bit is 0 and alt where it is 1, hap B the other allele.
 * Reads: for a selected row and a block, over the block's sites inside the row's [ts, te): hap_a = sites whose allele is 0 or 1
 * with allele XOR bit == 0, hap_b = those with that XOR 1, other = sites with allele 2, spanned = all of those sites, none
 * included.  The pair (row, block) gets a record iff hap_a + hap_b + other >= 1; hap is A if hap_a > hap_b, B if hap_b > hap_a,
 * - on a tie.
 * Files, each under a temporary name and renamed on success:
 * out_sites: the line "#contig\tpos\tref\talt\tdepth\tref_count\talt_count\tblock\tphase", then one line per site, contigs in
 * file order, positions ascending: pos 1-based, alt as hlmi_variants prints it, depth, ref_count = v[own] and alt_count = v[alt]
 * from the site's five votes, phase "0|1" for bit 0 and "1|0" for bit 1.  With no site the file is the header line alone.
 * out_links (optional): the line "#contig\tpos1\tpos2\tn00\tn01\tn10\tn11\tinformative\tagree\tphased", then one line per link;
 * agree is the quotient above as %.6f, 0.000000 when inf is 0; phased is cis, trans or -.
 * out_reads (optional): the line "#read\tcontig\tblock\tspanned\thap_a\thap_b\tother\thap", then one line per record: contigs in
 * file order, rows in selection order (contig, ts, line), a row's blocks ascending.
 * Refusals (HLMI_EINVAL unless said otherwise, nothing is written): hlmi_variants's option refusals, in its order; min_link < 1;
 * min_agree not a number, <= 0.5 or > 1 (with agreement above one half a tie can never phase); then every refusal hlmi_variants
 * makes about the files, the rows and the list, in its order; the sum over the selected rows of the sites inside [ts, te) is 2^32
 * or more, or does not fit the device's free memory.
 * The allele table (one byte per row and spanned site) and the link counters live and are read in device memory
 * (csrc/phase.hip); 16 bytes per link and 24 bytes per (row, block) come to the host. */
int hlmi_phase(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, const char *pairs_paf,
               const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);
/* The two calls hlmi_ava(contigs, reads, ao, P) and hlmi_phase(contigs, reads, P, o, pairs_paf, ...) in one, without the PAF P: the
 * three files and every integer field of *st are byte for byte what that chain gives (ao NULL: the long constants).  The stated
 * differences of hlmi_variants_reads apply; the selected rows' read names cost 4 bytes per row on the way to the host. */
int hlmi_phase_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_stats *st);

/* ---- phasing across a noisy site: links between sites up to `reach` apart.  hlmi_phase joins sites through the link between
 * neighbours only, so one unreliable site - a homopolymer error called as a site, a site with few informative rows - cuts a block in
 * two although the reads that span it say that the sites on either side belong together.  These calls read that evidence.  New
 * symbols: the older calls keep their signatures and their bytes, and HLMI_ABI_VERSION stays where it is.  A function of the
 * project's own: PARITY UNPINNED; tests/phase_reach_model.py is the contract, byte for byte. */
#define HLMI_PHASE_REACH_MAX 8
typedef struct {
    hlmi_phase_stats base;      /* as hlmi_phase's; links and links_phased count the links of distance 1, blocks_multi the blocks
                                   of two or more sites, sites_phased the members of such blocks (bridged sites are not included) */
    uint64_t links_far;         /* links of distance 2 .. reach inside one contig                                           */
    uint64_t links_far_phased;
    uint64_t joins_far;         /* members that joined their block through a link of distance >= 2                          */
    uint64_t sites_bridged;     /* sites inside a block that are no member of it                                            */
    uint64_t links_conflict;    /* phased links between two members of one block that contradict their bits                 */
} hlmi_phase_reach_stats;
/* contigs, reads, paf, o, pairs_paf and the three files: as for hlmi_phase.  reach = K, 1 <= K <= HLMI_PHASE_REACH_MAX.
 * Everything up to and including a row's allele at a site is hlmi_phase's, run by the same code.
 * Links: one per pair of sites (i, i + d) of one contig, 1 <= d <= K, the sites counted in ascending order.  The four counters, inf,
 * agree and the phased / cis / trans decision are hlmi_phase's link rule, over the rows whose allele is 0 or 1 at both sites; what
 * the rows read at the sites in between plays no part.
 * Blocks, per contig, sites ascending: a block starts at its first site b, a member with bit 0.  Going up from b + 1, site i joins
 * the block iff one of the members j with i - K <= j < i has a phased link (j, i); the nearest such member decides: bit[i] = bit[j]
 * XOR (the link is trans).  The walk ends at the first site more than K sites behind the last member, or with the contig.  The block
 * is the sites b .. last member - still a run of consecutive sites, its id the 1-based position of its first site - and the next
 * block starts behind it.  The sites among them that did not join are bridged: a bridged site has no phase bit.  With K = 1 this is
 * hlmi_phase's rule.
 * Conflicts: a phased link (j, i), i - j <= K, between two members of one block whose direction is not bit[j] XOR bit[i] is
 * counted in links_conflict and changes nothing.
 * Reads: hlmi_phase's records over these blocks; a bridged site counts in spanned and in none of hap_a, hap_b, other.
 * Files: the three files of hlmi_phase, same header lines and columns.  out_sites: a bridged site has its block's id in the block
 * column and "." in the phase column.  out_links: one line per link of any distance, ordered by (left site, right site).
 * With reach = 1 the three files are byte for byte hlmi_phase's and the integer fields of base equal hlmi_phase's.
 * Refusals: hlmi_phase's option refusals, in its order; reach < 1 or > HLMI_PHASE_REACH_MAX; then every other refusal of hlmi_phase,
 * in its order; the link counters do not fit the device's free memory.
 * The counters of 64 K bytes at the most per tile of left sites live in LDS (csrc/phase_reach.hip); 16 K bytes per site come to
 * the host. */
int hlmi_phase_reach(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, int reach, const char *pairs_paf,
                     const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_reach_stats *st);
/* hlmi_phase_reads with the rule above: the two calls hlmi_ava(contigs, reads, ao, P) and hlmi_phase_reach(contigs, reads, P, o,
 * reach, pairs_paf, ...) in one, without the PAF P; the stated differences of hlmi_phase_reads apply. */
int hlmi_phase_reads_reach(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, int reach,
                           const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                           hlmi_phase_reach_stats *st);

/* ---- insertion sites as phasing evidence: hlmi_phase and its _reach forms phase the sites hlmi_variants calls, which carry the five
 * symbols A C G T del; a slot where a share of the rows inserts bases (hlmi_variants_ins) is a site of a third kind that no row's
 * allele was ever read at.  These calls read it: two strains that differ by an insertion and a SNP are one block, and strains that
 * differ by insertions alone are phased at all.  hlmi_phase_ins reads a PAF as hlmi_phase_reach does, hlmi_phase_reads_ins aligns in
 * the call as hlmi_phase_reads_reach does.  New symbols: the older calls keep their signatures and their bytes, and
 * HLMI_ABI_VERSION stays where it is.  A function of the project's own: PARITY UNPINNED; tests/phase_ins_model.py is the contract,
 * byte for byte. */
typedef struct {
    hlmi_phase_reach_stats reach;   /* as hlmi_phase_reach's, over the merged list of sites: links, blocks, alleles and the rest
                                       count sites of both kinds; the thirteen variant fields (sites among them) stay hlmi_variants's */
    uint64_t slots_callable;        /* the four slot fields of hlmi_variant_ins_stats, with hlmi_variants_ins's values            */
    uint64_t ins_sites;
    uint64_t ins_long;
    uint64_t ins_edge;
    uint64_t ins_sites_phasing;     /* insertion sites that take part                                                           */
    uint64_t ins_sites_left_out;    /* ... and those that do not: ins_sites = ins_sites_phasing + ins_sites_left_out            */
    uint64_t ins_sites_phased;      /* insertion sites that are members of blocks of two or more sites                          */
} hlmi_phase_ins_stats;
/* contigs, reads, paf, o, reach, pairs_paf and the three files: as for hlmi_phase_reach.  reach = K, 1 <= K <= HLMI_PHASE_REACH_MAX;
 * with K = 1 the links are those between neighbours, counted by the kernel of the _reach calls.
 * Sites: the merged list of two kinds.  Position sites: exactly hlmi_variants's.  Insertion sites: those of hlmi_variants_ins under
 * the same options (both kinds come from its one count pass) that take part: an insertion site at slot p - the gap in front of
 * 0-based position p, 0 < p < length, printed as pos = p - takes part iff len >= 1 and len_count >= min_alt, so that its called
 * length has the support a position site's alt needs.  The others count in ins_sites_left_out and appear in none of the three
 * files.  Order inside a contig: slot p sorts directly in front of position p (key 2 p for the slot, 2 p + 1 for the position);
 * with the printed 1-based positions, a position site and an insertion site that print the same pos come position site first.
 * Alleles: at a position site hlmi_phase's, run by the same code.  At an insertion site at slot p a row spans the slot iff
 * ts < p < te (hlmi_variants_ins's span); with b what the row inserts at p as hlmi_variants_ins counts it (the one I op of the
 * compact CIGAR at that slot, never an edge op), the row's allele is 0 (own) if it inserts nothing there, 1 (alt) if the length of
 * b is the site's len, 2 (other) for any other length, more than 16 bases included.  The alt is matched by length alone: the
 * inserted bases, N included, play no part.  "None" does not occur inside the span.  A row's sites are the keys in
 * [2 ts + 1, 2 te): one run of the merged list, so alleles and its 2^32 refusal are hlmi_phase's over both kinds.
 * Links, blocks, phase bits, conflicts, bridged sites, read records: hlmi_phase_reach's rules over the merged list, run by the same
 * code.
 * Files: the three files of hlmi_phase_reach, same header lines.  out_sites, at an insertion site: pos = p, ref the upper-cased
 * base in front of the slot (as out_ins of hlmi_variants_ins has it), alt '+' followed by the site's seq, depth = span, ref_count =
 * span - ins - ins_long, alt_count = len_count.  out_links: pos1 and pos2 are the printed positions; a slot endpoint carries a
 * trailing '+'.  A block's id is the printed pos of its first site, with a trailing '+' when that site is an insertion site
 * (otherwise a position site and an insertion site that print the same pos could start two blocks with one id); the same id
 * stands in out_reads.
 * On an input where no insertion site takes part the three files are byte for byte hlmi_phase_reach's at the same reach and
 * st->reach equals hlmi_phase_reach's stats in every integer field.
 * Refusals: hlmi_phase_reach's, in its order, under these names.  The doubled key needs none of its own: hlmi_polish's limit of 2^31
 * contig bases, which these calls make as hlmi_phase does, keeps 2 p + 1 below 2^32.
 * The merged list lives in device memory as 5 bytes per site; the table is filled by kind and written by csrc/phase_ins.hip, and
 * everything behind it is hlmi_phase_reach's device code. */
int hlmi_phase_ins(const char *contigs, const char *reads, const char *paf, const hlmi_phase_opts *o, int reach, const char *pairs_paf,
                   const char *out_sites, const char *out_links, const char *out_reads, hlmi_phase_ins_stats *st);
/* hlmi_phase_reads_reach with the rules above: the two calls hlmi_ava(contigs, reads, ao, P) and hlmi_phase_ins(contigs, reads, P, o,
 * reach, pairs_paf, ...) in one, without the PAF P; the stated differences of hlmi_phase_reads apply. */
int hlmi_phase_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_phase_opts *o, int reach,
                         const char *pairs_paf, const char *out_sites, const char *out_links, const char *out_reads,
                         hlmi_phase_ins_stats *st);

/* ---- haplotigs: polish each side of a phased block on its own.  hlmi_polish lets every read vote in every column, so inside a phased
 * block the majority strain wins; these calls give two consensus sequences where the reads prove two sides, and hlmi_polish's bytes
 * everywhere else.  hlmi_haplotigs reads a PAF as hlmi_phase does, hlmi_haplotigs_reads aligns in the call as hlmi_phase_reads does.
 * New symbols: the older calls keep their signatures and their bytes, and HLMI_ABI_VERSION stays where it is.  A function of the
 * project's own: PARITY UNPINNED; tests/haplotigs_model.py is the contract, byte for byte. */
typedef struct {
    int min_len;              /* the seven fields of hlmi_phase_opts, same meaning and defaults                            */
    double min_iden;
    int min_cov;
    int min_alt;
    double min_frac;
    int min_link;
    double min_agree;
    int min_side;             /* records a block needs on side A, and on side B, to be split (>= 1)                        */
    int include_unpolished;   /* as in hlmi_polish_opts                                                                    */
} hlmi_haplotig_opts;
void hlmi_haplotig_opts_default(hlmi_haplotig_opts *o);   /* 0, 0.0, 3, 2, 0.2, 3, 0.8, 3, 1 */
typedef struct {
    hlmi_phase_stats phase;     /* of the phasing, with hlmi_phase's values; its ms_device ends where the phasing does      */
    uint64_t blocks_split;
    uint64_t contigs_split;     /* contigs with a split block: they give two records                                        */
    uint64_t positions_split;   /* positions inside the extents of split blocks                                             */
    uint64_t diff_positions;    /* ... that the two sides decided differently                                               */
    uint64_t records;           /* records written to out_fa                                                                */
    uint64_t substituted;       /* these four as in hlmi_polish_stats, summed over the records: a split contig gives both   */
    uint64_t deleted;
    uint64_t inserted_bases;
    uint64_t slots_opened;
    uint64_t ins_long;          /* these two as in hlmi_polish_stats, once per row                                          */
    uint64_t ins_edge;
    double ms_device;           /* wall time of the device part: uploads, kernels, read-backs                               */
    double ms_total;
} hlmi_haplotig_stats;
/* contigs, reads, paf: as for hlmi_phase.  pairs_paf and out_blocks may be NULL.
 * 1. Phasing: selection (the pair list included), rows, sites, links, blocks, phase bits and every row's hap_a / hap_b per block are
 * hlmi_phase's, run by the same code.  A row's side in a block is A if hap_a > hap_b, B if hap_b > hap_a, none on a tie or without a
 * record.
 * 2. Split blocks: a block with at least two sites is split iff at least min_side of its (row, block) records have side A and at
 * least min_side have side B.  Its extent is the positions [first site, last site] of its contig, both ends included; slot p (the
 * gap in front of position p) lies inside the extent iff first < p <= last.  Extents of different blocks never overlap.
 * 3. Who votes: row r takes part in side S at position or slot p unless p lies inside the extent of a split block and the row's side
 * in that block is the other side.  A row votes on both sides wherever p is outside every extent, and a row with no side in a block
 * votes on both sides inside that block's extent.  Where a row takes part it does so exactly as in hlmi_polish, unweighted: its
 * column vote, its spanning of a slot, its insertion of 1..16 bases, ins_long, ins_edge.
 * 4. Decisions: hlmi_polish's rules, once per side on that side's counters: a position keeps the contig's byte when the side's votes
 * are below min_cov; a tie prefers the contig's own base; a slot opens when s >= min_cov and 2 i > s over the side's spanning and
 * inserting rows; its length and bases come from the side's inserting rows.
 * 5. out_fa (under a temporary name, renamed on success), contigs in file order.  A contig with selected rows and no split block
 * gives one record, byte for byte what hlmi_polish writes for it (">name LN:i: RC:i: XC:f:").  A contig with a split block gives
 * two records, ">name_hapA LN:i:<length> RC:i:<rows selected on the contig> XC:f:<that side's share of positions with votes >=
 * min_cov> HB:i:<split blocks> HP:i:<positions inside their extents>" and the same for _hapB.  A contig without a selected row is
 * written as it is when include_unpolished is set.  A record whose consensus is empty is not written.  Side A of a block is the
 * side that holds the contig's own allele at the block's first site; the sides of different blocks of one contig are independent
 * of each other (pseudo-haplotigs: _hapA joins the A sides of all blocks, which need not be one strain).
 * 6. out_blocks (optional): the line "#contig\tblock\tstart\tend\tsites\trows_a\trows_b\tsplit\tdiff_positions", then one line per
 * block with at least two sites, contigs in file order, blocks ascending: block is the block's id (the 1-based position of its
 * first site), start and end its extent, 1-based; rows_a and rows_b the records with side A and B; split 1 or 0; diff_positions the
 * number of positions of the extent whose decision (keep, a base, del) differs between the two sides, 0 when the block is not split.
 * 7. Stats: substituted, deleted, inserted_bases and slots_opened are counted per record as hlmi_polish counts them for a contig (a
 * consensus that turns out empty still counts) and summed.
 * Consequence: with no split block in the call - min_side above the number of rows is enough - out_fa is byte for byte hlmi_polish's
 * on the same input and options; the single-sided count pass produces it and no kernel of csrc/haplotigs.hip is launched.
 * Out of scope: quality weights; joining blocks across a contig.  (Links between sites that are not neighbours:
 * hlmi_haplotigs_reach below; insertion sites as phasing evidence: hlmi_haplotigs_ins below.)
 * Refusals (HLMI_EINVAL unless said otherwise, nothing is written): hlmi_phase's option refusals, in its order; min_side < 1; then
 * every refusal hlmi_phase makes about the files, the rows, the list and its tables, in its order; the rows' interval table does not
 * fit the device's free memory; hlmi_polish's limits (2^28 bases in a sequence, 2^31 contig bases).
 * Device: the records per (row, block) stay in device memory behind the phasing; 9 bytes per block go up (extent and split flag) and
 * nothing per row comes down.  Two sides of counters live in LDS only (csrc/haplotigs.hip). */
int hlmi_haplotigs(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, const char *pairs_paf,
                   const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);
/* The two calls hlmi_ava(contigs, reads, ao, P) and hlmi_haplotigs(contigs, reads, P, o, pairs_paf, ...) in one, without the PAF P:
 * both files and every integer field of *st are byte for byte what that chain gives (ao NULL: the long constants).  The three stated
 * differences of hlmi_polish_reads apply (a name twice - which hlmi_haplotigs refuses as well -, stub_oh >= 0, 2^32 rows). */
int hlmi_haplotigs_reads(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o,
                         const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);
/* hlmi_haplotigs over the blocks of hlmi_phase_reach's rule, 1 <= reach <= HLMI_PHASE_REACH_MAX: the phasing is hlmi_phase_reach's
 * (st->phase holds its base), every rule of hlmi_haplotigs stands as it is.  A block's extent runs from its first to its last
 * site, the sites column of out_blocks counts every site in that range, bridged ones included, and a row's side comes from its
 * record (which leaves bridged sites out).  With reach = 1 both files and the integer stats equal hlmi_haplotigs's byte for byte.
 * Refusals: hlmi_haplotigs's option refusals, in its order; reach < 1 or > HLMI_PHASE_REACH_MAX; then the rest as hlmi_haplotigs. */
int hlmi_haplotigs_reach(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, int reach,
                         const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);
/* hlmi_haplotigs_reads in the same way: hlmi_ava and hlmi_haplotigs_reach in one call, without the PAF. */
int hlmi_haplotigs_reads_reach(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o, int reach,
                               const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_stats *st);

/* ---- haplotigs over blocks with insertion sites: hlmi_haplotigs and its _reach form phase the position sites alone, so a strain
 * that differs from the contig by insertions alone is phased by hlmi_phase_ins and written by nobody: the majority vote never opens
 * its slots.  These calls polish each side of hlmi_phase_ins's split blocks.  hlmi_haplotigs_ins reads a PAF as hlmi_phase_ins does,
 * hlmi_haplotigs_reads_ins aligns in the call as hlmi_phase_reads_ins does.  New symbols: the older calls keep their signatures and
 * their bytes, and HLMI_ABI_VERSION stays where it is.  A function of the project's own: PARITY UNPINNED;
 * tests/haplotigs_ins_model.py is the contract, byte for byte. */
typedef struct {
    hlmi_haplotig_stats base;       /* as hlmi_haplotigs_reach's; its phase part holds hlmi_phase_ins's values of the shared fields,
                                       over the merged list of sites (the thirteen variant fields stay hlmi_variants's)            */
    uint64_t slots_callable;        /* the seven insertion counters of hlmi_phase_ins_stats, with its values, by the same code      */
    uint64_t ins_sites;
    uint64_t ins_long;
    uint64_t ins_edge;
    uint64_t ins_sites_phasing;
    uint64_t ins_sites_left_out;
    uint64_t ins_sites_phased;
    uint64_t diff_slots;            /* slots inside the extents of split blocks that the two sides opened to different lengths      */
} hlmi_haplotig_ins_stats;
/* contigs, reads, paf, o, reach, pairs_paf and the two files: as for hlmi_haplotigs_reach.  The rules of hlmi_haplotigs hold except
 * where changed here.
 * Phasing: hlmi_phase_ins's at the same reach, run by the same code: the merged list of position sites and the insertion sites that
 * take part, alleles, links, blocks, bridged sites and records.  A row's side in a block is A if hap_a > hap_b of its record, B if
 * hap_b > hap_a, none otherwise.  Side A holds the own allele at the block's first site; at an insertion site the own allele is
 * "inserts nothing".
 * Extent: a split block's extent lies in hlmi_phase_ins's key space - slot p has key 2 p, position p key 2 p + 1 - and is [kf, kl],
 * the keys of its first and its last site.  Position p is inside iff kf <= 2 p + 1 <= kl, slot p iff kf <= 2 p <= kl.  Between two
 * position sites that is hlmi_haplotigs's rule: positions [first, last], slots (first, last].  An extent that starts at an insertion
 * site at slot p shuts the other side's rows out of slot p as well; one that ends at an insertion site at slot p shuts them out of
 * slot p and not out of position p.  Every extent holds a position; extents never overlap.
 * Who votes, decisions, out_fa: hlmi_haplotigs's rules 3, 4, 5 and 7 with these inside tests - so an insertion site inside a split
 * block is decided per side: the side whose rows insert opens the slot, the other keeps it shut.  positions_split and HP:i: count
 * the positions inside, ((kl - 1) >> 1) - (kf >> 1) + 1 per extent.
 * out_blocks: the nine columns of hlmi_haplotigs and a tenth, diff_slots.  block is the id hlmi_phase_ins prints: the printed pos of
 * the first site, with a trailing '+' where that is an insertion site.  start and end are the printed pos of the first and the last
 * site, each with a trailing '+' when that site is an insertion site.  sites counts both kinds, bridged sites included.
 * diff_positions runs over the positions inside.  diff_slots is the number of slots inside the extent whose opened length differs
 * between the two sides - a shut slot has length 0, the bases play no part - and 0 when the block is not split; st->diff_slots is
 * the sum over the blocks.
 * Where no insertion site takes part, out_fa is byte for byte hlmi_haplotigs_reach's at the same reach, out_blocks is its file with
 * the tenth column (0) added, and st->base equals its stats in every integer field.  With no split block hlmi_polish's count pass
 * gives the bytes and no kernel of csrc/haplotigs.hip is launched, as in hlmi_haplotigs.
 * Out of scope: quality weights; joining blocks across a contig; insertions of more than 16 bases (hlmi_polish's cap: such a row
 * reads "other" at the site and opens no slot).
 * Refusals: hlmi_haplotigs_reach's, in its order, under these names.  None of their own: a row's interval holds two 32-bit keys and
 * the shut side in 12 bytes, and hlmi_polish's limit of 2^31 contig bases keeps 2 p + 1 below 2^32.
 * Device: as hlmi_haplotigs; the records are hlmi_phase_ins's, 9 bytes per block go up (kf, kl, split flag), the count pass and the
 * slot passes run in their key-space instantiations (csrc/haplotigs.hip). */
int hlmi_haplotigs_ins(const char *contigs, const char *reads, const char *paf, const hlmi_haplotig_opts *o, int reach,
                       const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st);
/* hlmi_haplotigs_reads_reach in the same way: hlmi_ava and hlmi_haplotigs_ins in one call, without the PAF. */
int hlmi_haplotigs_reads_ins(const char *contigs, const char *reads, const hlmi_ava_opts *ao, const hlmi_haplotig_opts *o, int reach,
                             const char *pairs_paf, const char *out_fa, const char *out_blocks, hlmi_haplotig_ins_stats *st);

/* ---- staged multi-GPU job: sketch shard -> (RCCL all-gather by the caller) -> run -------- */
/* One process per GPU.  Every rank opens the same files, sketches its slice of the query
 * reads into a caller-owned device buffer (16 B per minimizer: two uint64), the caller
 * all-gathers the buffers over RCCL (torch.distributed), hands the gathered sketch back and
 * runs its share of the target chunks. */
typedef struct hlmi_job hlmi_job;
hlmi_job *hlmi_job_open(const char *reads_fa, const char *ref_fa, int nsplit, int long_mode);
void      hlmi_job_close(hlmi_job *j);
int64_t   hlmi_job_num_queries(const hlmi_job *j);
int64_t   hlmi_job_num_chunks(const hlmi_job *j);
/* upper bound of minimizers for query reads [lo,hi): capacity needed by hlmi_job_sketch */
int64_t   hlmi_job_sketch_bound(const hlmi_job *j, int64_t lo, int64_t hi);
/* sketch query reads [lo,hi) on the GPU into dev_mz (capacity cap entries of 16 B), sorted by
 * (read, position); per-read counts go to dev_counts[hi-lo] (uint32).  *n_out = entries. */
int       hlmi_job_sketch(hlmi_job *j, int64_t lo, int64_t hi, void *dev_mz, int64_t cap,
                          void *dev_counts, int64_t *n_out);
/* install the complete query sketch (all reads, read-major): dev_mz[n] + dev_counts[nq] */
/* single-GPU form of the two calls around it: sketches ALL query reads into buffers of the job's own, sized exactly
 * (hlmi_job_sketch needs room for the bound - one entry per base - which is 80 GB for 5 Gbases of reads), and installs them */
int       hlmi_job_sketch_own(hlmi_job *j);
int       hlmi_job_set_query_sketch(hlmi_job *j, const void *dev_mz, int64_t n, const void *dev_counts);
/* overlap + filter the chunks {c : c % world == rank}; writes the rank's score-sorted PAF */
int       hlmi_job_run(hlmi_job *j, int rank, int world, int len_over, int mc, double iden,
                       const char *out_paf);

/* ---- measurement hooks (bench.py) -------------------------------------------------------- */
/* Counters of the last stage run in this process: name -> value, written as JSON to buf. */
int hlmi_last_stats_json(char *buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* HYLIGHT_MI_H */
