// vq_internal.h - what the stage-b sources (the SAVAGE / ViralQuasispecies overlap-graph assembler) share,
// in the order of the pipeline:
//   front  vq_front.hip                          the two input files (singles.fastq, the 13-column overlaps), the overlap
//                                                score, and the rounds of findTransEdges (GraphAlgos.cpp:746-795)
//   graph  vq_graph.hip / vq_graph_host.cpp      the oriented, reduced overlap graph (ViralQuasispecies --graph_only)
//   merge  vq_merge.hip                          super-reads along its edges (SRBuilder::mergeAlongEdges)
//   cliques  vq_clique_host.cpp / vq_clique.hip  the maximal cliques of the graph, one pile-up consensus each (--cliques=true)
//   superread  vq_superread.cpp / .._run.cpp     what the two share through constructSuperread (pure host) / their drivers
//   next   vq_next.hip                           the overlaps of the next iteration (SRBuilder::findNextOverlaps), behind either
// Everything on the device runs on the library's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace hlmi {

// ---- front: vq_front.hip -------------------------------------------------------------------------------------------------
// singles.fastq: 4-line records, vertex = position in the file (FastqStorage.cpp:92-150, ViralQuasispecies.cpp:262-276)
struct Singles {
    std::string path;                                  // for messages
    std::vector<std::string> seq;                      // upper-cased
    std::vector<std::string> qual;                     // the quality line as it stands
    std::vector<uint64_t> id;                          // read id per vertex
    std::unordered_map<uint64_t, uint32_t> index_of;   // read id (strtoul base 0 of the first word) -> vertex
};
// refuses (HLMI_EINVAL) an id line without '@' and an empty sequence; the qualities are checked by whoever reads them
// (vq_score_overlaps, vq_merge_check_reads)
Singles read_singles(const char *path);

// The rows of a 13-column overlaps file (EdgeCalculator.cpp:561-666, Overlap.h:37-72): `edges` = the edge candidates in
// file order; `nonedges` (may be NULL) = the rows the reference writes back to nonedge_overlaps.txt (too short for an edge,
// :628-631), in file order.  Only the first max_overlaps lines are looked at.
void vq_parse_overlaps(const char *path, uint32_t min_len, uint32_t min_perc, int relax_pe, uint64_t max_overlaps,
                       std::vector<hlmi_vq_overlap> &edges, std::vector<hlmi_vq_overlap> *nonedges, uint64_t *n_nonedge,
                       uint64_t *n_skipped);
// Overlap::get_perc (Overlap.h:196-203)
inline uint32_t vq_perc(const hlmi_vq_overlap &o) { return o.perc2 > 0 ? (uint32_t)(0.5 * (double)(o.perc1 + o.perc2)) : o.perc1; }

// vq_overlap_scores (graph.h) over reads that are already parsed.  Refuses (HLMI_EINVAL) a quality line of another length
// than its sequence and a quality character outside '!' .. '~' in ANY read, then an overlap that names a read not there.
void vq_score_overlaps(const Singles &reads, const hlmi_vq_overlap *ov, uint64_t n, double mismatch, uint32_t min_read_len,
                       double *score, double *mismatch_rate, int64_t *pos3);

namespace vqk {
constexpr int WG = 256;
constexpr int WAVES = WG / 64;
constexpr uint32_t SET_CAP = 2048;                 // LDS hash slots per wave: vertices with up to SET_CAP / 2 out-edges
constexpr uint32_t EMPTY = 0xffffffffu;
constexpr int SEARCH_STEPS = 33;                 // a binary search over fewer than 2^32 entries ends within this many steps
inline dim3 grid1(size_t n) { return grid_for(n, WG); }
// blocks of a one-wave-per-item kernel that strides over its items
inline unsigned waves_grid(size_t n_items) { return (unsigned)std::max<size_t>(1, std::min<size_t>(cdiv(n_items, (size_t)WAVES), 256 * 16)); }

// key[i] = a[k] << 32 | b[k], val[i] = k for k = ids[i] (ids NULL: k = i)
__global__ void edge_keys_kernel(const uint32_t *a, const uint32_t *b, const uint32_t *ids, size_t n, uint64_t *key, uint32_t *val);
// off[v] = first position whose key's high word is >= v, for v = 0 .. n_vertices
__global__ void offsets_kernel(const uint64_t *key, size_t n, uint32_t n_vertices, uint32_t *off);
// flag[oval[k]] = 1 when out-edge k of (okey, ooff) is transitive (an in-neighbour of its target is an out-neighbour of its
// source), 0 otherwise; one wave per source vertex, vertices with more than SET_CAP / 2 out-edges go to big_list
__global__ void trans_kernel(const uint64_t *okey, const uint32_t *oval, const uint32_t *ooff, const uint64_t *ikey,
                             const uint32_t *ioff, uint32_t n_vertices, uint8_t *flag, uint32_t *big_list, uint32_t *n_big);
__global__ void trans_big_kernel(const uint64_t *okey, const uint32_t *oval, const uint32_t *ooff, const uint64_t *ikey,
                                 const uint32_t *ioff, const uint32_t *big_list, uint32_t n_big, uint8_t *flag);
}  // namespace vqk

// rounds of findTransEdges over the edges (d_src[k] -> d_dst[k]), k < E, both resident; ids receives the edge numbers
// of the last round's set (ascending); returns their count
size_t vq_trans_rounds(uint32_t n_vertices, const uint32_t *d_src, const uint32_t *d_dst, size_t E, int rounds, DBuf<uint32_t> &ids);

// ---- graph: vq_graph.hip / vq_graph_host.cpp (ViralQuasispecies --graph_only) ----------------------------------------------
// One edge of the graph: the fields of Edge.h a single-end overlap uses.  Reads and vertices are one to one, so read1 /
// read2 are implied by v1 / v2 (Edge::swap_reads and switch_edge_orientation swap both together).
struct VqEdge {
    uint32_t v1, v2;                   // out-vertex, in-vertex
    int32_t pos1, pos2, pos3, pos4;    // pos3 = |read1| - pos1 - |read2| (set_extra_pos), pos4 = 0
    uint8_t ori1, ori2, pad[2];        // 1: '+'
    int32_t len;                       // overlap length (get_len(0) = column 10)
    int32_t perc;                      // Overlap::get_perc
    uint32_t cand;                     // file index of the candidate it came from
    double score, mr;                  // overlap score, mismatch rate
};
// (pad[0] carries Edge::ord, the overlap row's column 5: findNextOverlaps copies it)

// Edge::switch_edge_orientation (Edge.h) for a single-end edge; returns true when the edge changes direction
__host__ __device__ inline bool switch_orientation(VqEdge &e) {
    int32_t t = e.pos1; e.pos1 = e.pos3; e.pos3 = t;
    t = e.pos2; e.pos2 = e.pos4; e.pos4 = t;
    e.ori1 = !e.ori1;
    e.ori2 = !e.ori2;
    if (e.pos1 < 0 || (e.pos1 == 0 && e.v1 > e.v2)) {
        uint32_t v = e.v1; e.v1 = e.v2; e.v2 = v;
        uint8_t o = e.ori1; e.ori1 = e.ori2; e.ori2 = o;
        e.pos1 = -e.pos1;
        if (e.pos2 < 0) e.pos2 = -e.pos2;
        return true;
    }
    if (e.pos2 < 0) e.pos2 = -e.pos2;
    return false;
}
// (the move branch leaves pos3 / pos4 as swapped: Edge.h negates nothing there)

// Edge selection (EdgeCalculator.cpp:428-532) on the device: winners[] = the candidate index that holds each (min vertex,
// max vertex, ori1 == ori2) key at the end of process_overlaps, ascending; incl[v] = 1 for the vertices the first candidate
// of a key marks as included (only with ignore_inclusions).
void vq_select_edges(const std::vector<VqEdge> &cand, uint32_t n_vertices, bool ignore_inclusions,
                     std::vector<uint32_t> &winners, std::vector<uint8_t> &incl);

// The check pass of labelVertices (GraphAlgos.cpp:295-348) over the edges in adjacency-list order, kept on the device
// across the tries of vertexLabellingHeuristic: cls[k] = 0 edge agrees with the labels, 1 contradiction (to be deleted),
// 2 flipped and moved to the other endpoint's list (left unchanged here), 3 flipped in place (applied here, and kept for
// the later tries, as the reference's in-place Edge::switch_edge_orientation is).
class VqLabelPass {
public:
    explicit VqLabelPass(const std::vector<VqEdge> &edges);
    void run(const std::vector<uint8_t> &orient, std::vector<uint8_t> &cls);
    std::vector<VqEdge> state() const;
private:
    DBuf<VqEdge> d_edges_;
    DBuf<uint8_t> d_orient_, d_cls_;
    size_t n_;
};

// The reductions below all speak of the positions of Graph::flatten (vq_graph_host.cpp): src[p] -> dst[p], lists in off[].
// removeInclusions (GraphAlgos.cpp:20-48): removed[p] = 1 for the positions that go.  Every out- and in-edge pair of an
// included vertex goes, one edge per pair: removeEdge takes the first u -> v of u's list.
void vq_inclusion_removed(const std::vector<uint32_t> &off, const std::vector<uint32_t> &src, const std::vector<uint32_t> &dst,
                          const std::vector<uint8_t> &incl, std::vector<uint8_t> &removed);
// findTransEdges repeated `rounds` times (GraphAlgos.cpp:746-776, 956-966, vq_trans_rounds): flags[p] = 1 for the edges of
// the last round's set (transitive, double transitive, ...); returns their number
uint64_t vq_trans_flags(uint32_t n_vertices, const std::vector<uint32_t> &src, const std::vector<uint32_t> &dst, int rounds,
                        std::vector<uint8_t> &flags);
// removeTips (GraphAlgos.cpp:543-637): one wave per vertex over its out-list and its in-list.  ext_fwd[p] / ext_bwd[p] =
// Edge::ext_len(true / false) of the edge at position p.  removed[p] = 1 for the edges that go, tip[v] = 1 for the reads
// marked as tips.
void vq_tips(uint32_t n_vertices, const std::vector<uint32_t> &off, const std::vector<uint32_t> &dst,
             const std::vector<uint32_t> &in_off, const std::vector<uint32_t> &in_src, const std::vector<uint32_t> &ext_fwd,
             const std::vector<uint32_t> &ext_bwd, uint32_t max_tip_len, std::vector<uint8_t> &removed, std::vector<uint8_t> &tip);
// removeBranches (GraphAlgos.cpp:835-936): comp[v] = a component label of the branch-free graph; only equality is meant.
// A non-transitive edge joins its endpoints only when its source keeps its out-list and its target its in-list (the
// one-sided clearing of :855-901).
// The non-transitive edges are those vq_trans_flags(.., 1, ..) leaves unflagged: one upload of src / dst serves both passes.
void vq_branch_components(uint32_t n_vertices, const std::vector<uint32_t> &src, const std::vector<uint32_t> &dst,
                          std::vector<uint32_t> &comp);

// vq_graph_host.cpp: hlmi_vq_graph_opts_stageb / hlmi_vq_graph (include/hylight_mi.h)
void vq_graph_opts_stageb(hlmi_vq_graph_opts *o);
// One source edge of findNextOverlaps: what updateOverlap reads of an Edge (FindNextOverlaps.cpp:25-72)
struct VqSrcEdge {
    uint32_t v1, v2;
    int32_t pos1, pos2, len1, len2, perc;
    uint8_t ori1, ori2;                // 1: '+'
    uint8_t score0;                    // get_score() == 0: a non-edge overlap (:34)
    char ord;
};
// what findNextOverlaps reads of a graph edge; single-end: get_len(1) = len, get_len(2) = 0
inline VqSrcEdge vq_src_edge(const VqEdge &e) {
    VqSrcEdge s{};
    s.v1 = e.v1; s.v2 = e.v2;
    s.pos1 = e.pos1; s.pos2 = e.pos2;
    s.len1 = e.len; s.len2 = 0;
    s.perc = e.perc;
    s.ori1 = e.ori1; s.ori2 = e.ori2;
    s.score0 = e.score == 0;
    s.ord = (char)e.pad[0];
    return s;
}
// What SRBuilder reads of the finished graph (keep != NULL): the reads, the out-lists after the sortEdges of
// ViralQuasispecies.cpp:434, the vertex orientations of the winning labelling, the inclusions and the tip reads.  built is
// false when the run stopped for want of an edge (ViralQuasispecies.cpp:282-291).
struct VqGraphState {
    bool built = false;
    std::vector<std::string> seq, qual;
    std::vector<uint64_t> id;
    std::vector<std::vector<VqEdge>> out;
    std::vector<uint8_t> orient, incl, tip;
    // for findNextOverlaps (for_next): OverlapGraph::branching_edges in push order, the rows of nonedge_overlaps.txt in file
    // order as the edges of FindNextOverlaps.cpp:661-691, and inclusion_edges (GraphAlgos.cpp:26-42): list l = incl_edges
    // [incl_off[l], incl_off[l + 1])
    std::vector<VqSrcEdge> branching, nonedge, incl_edges;
    std::vector<uint32_t> incl_off;
    // for_next: the out-lists as the cycle removal left them, kept only where the sortEdges of :434 moved an edge.  The
    // --cliques=true branch never runs that sort (ViralQuasispecies.cpp:417-428), so this is the adj_out its findNextOverlaps
    // walks; std::sort may move the ties of a list of more than 16 edges that was sorted before
    std::vector<std::vector<VqEdge>> out_unsorted;
};
inline const std::vector<std::vector<VqEdge>> &vq_cliques_out(const VqGraphState &g) { return g.out_unsorted.empty() ? g.out : g.out_unsorted; }
struct VqBranchRun;
// for_next: also keep what findNextOverlaps reads, and refuse a paired-end non-edge row before a file is written.  branch:
// --branch_reduction=true (vq_branch_host.cpp): the 3-clique rule in removeTransitiveEdges and readBasedBranchReduction where
// removeBranches would run; without it nothing changes
void vq_graph_run(const char *fastq, const char *overlaps, const hlmi_vq_graph_opts &o, const char *out_dir, hlmi_vq_graph_stats *st,
                  VqGraphState *keep = nullptr, bool for_next = false, VqBranchRun *branch = nullptr);

// ---- merge: vq_merge.hip (SRBuilder::mergeAlongEdges on the device; its driver is in vq_superread_run.cpp) -----------------
namespace vqm {
constexpr int WG = 256;
constexpr int WAVE = 64;
constexpr int SPAN = 4096;                       // output positions per workgroup step (a span of the position space, not a read)
constexpr int NQ = 94;                           // phred 0 .. 93 ('!' .. '~')
constexpr int CNT_SLOTS = 256;                   // N counters in LDS per span; a span with more records counts the rest in global memory
constexpr uint32_t NONE = 0xffffffffu;
// The answers of SRBuilder::consensus_pos as 16-bit entries, low byte = quality character.
//   single[c][q]      one base c (A C G T N = 0 .. 4): high byte = the base written
//   with_n[c][q]      base c (0 .. 3) against an N of any quality: high byte = the base written
//   same[q1][q2]      twice one base: high byte 1 = that base, 0 = N, 4 = the first of A, T, C, G that is another base
//   diff[q1][q2]      two different bases: 0 = N, 1 = the first, 2 = the second, 3 = the one of the two that comes first in
//                     A, T, C, G, 4 = the first of A, T, C, G that is neither
// The host evaluates every (base, quality) pair for the call's minQual and builds same / diff only if the answer is the same
// whichever bases they are (it depends on them through the order of the four terms of total_prob) or is the tie rule of
// consensus_pos (:390-393) in every pair: 3 for two different bases of equal score, 4 where both bases are Q0 / Q1 and the
// bases that were not read score best - columns a minQual of 1/2 and more turns into N.  Otherwise the call fails.
constexpr int T_SINGLE = 0, T_WITH_N = T_SINGLE + 5 * NQ, T_SAME = T_WITH_N + 4 * NQ, T_DIFF = T_SAME + NQ * NQ,
              T_ALL = T_DIFF + NQ * NQ;
constexpr uint32_t F_REV_A = 1, F_REV_B = 2, F_CONS = 4;
struct Rec {                                     // one FASTQ record of the output
    uint32_t a, b;                               // reads: a at 0, b (NONE: a copy of a) at p
    uint32_t p, len;                             // len = output bases
    uint32_t flags, id;                          // F_*; id = the number after '@'
};
__device__ __forceinline__ uint32_t base_code(uint8_t c) {      // A C G T N -> 0 .. 4 (the host refuses anything else)
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
__device__ __forceinline__ uint8_t complement(uint8_t c) {      // Read::build_rev_comp: N stays N
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
// the base a two-base cell of same / diff stands for: b1 / b2 with base codes c1 / c2 (0 .. 3), act = the cell's high byte
__device__ __forceinline__ uint8_t pair_base(uint32_t act, uint8_t b1, uint8_t b2, uint32_t c1, uint32_t c2) {
    const uint32_t first2 = ((0x1320u >> (4 * c2)) & 3u) < ((0x1320u >> (4 * c1)) & 3u);      // rank in A, T, C, G per nibble
    const uint32_t read = (1u << c1) | (1u << c2);                        // bit per base code: A C G T
    const uint8_t other = !(read & 1u) ? 'A' : !(read & 8u) ? 'T' : !(read & 2u) ? 'C' : 'G';
    return act == 0 ? (uint8_t)'N' : act == 4 ? other : (act == 2) | ((act == 3) & first2) ? b2 : b1;
}
}  // namespace vqm

namespace vqc { struct Pile; struct Entry; struct Result; }
// The device side of a merge over resident reads (vq_merge.hip): bases / quals concatenated, read r at [off[r], off[r + 1]).
class VqMergeDev {
public:
    VqMergeDev(const std::vector<std::string> &seq, const std::vector<std::string> &qual, const std::vector<uint16_t> &tables);
    std::vector<uint32_t> read_n_counts();                                  // 'N's per read
    std::vector<uint32_t> count_n(const std::vector<vqm::Rec> &recs);       // 'N's each record would hold
    // the records' FASTQ text, one after the other; start[r] = first byte of record r, start[n] = the size
    std::string write(const std::vector<vqm::Rec> &recs, std::vector<uint64_t> &start);
    // vq_clique.hip: SRBuilder::consensus of every pile-up, one wave each.  bases / quals receive the piles' columns (pile k
    // at col0), a quality byte of 0 marks a column the host has to redo (vqc::MARGIN); res[k] as vqc::Result says
    // min_qual: the value the tables handed to the constructor were built for
    void consensus_piles(const std::vector<vqc::Pile> &piles, const std::vector<vqc::Entry> &entries, uint32_t min_support,
                         bool error_correction, double min_qual, std::vector<uint8_t> &bases, std::vector<uint8_t> &quals,
                         std::vector<vqc::Result> &res);
private:
    void layout(const std::vector<vqm::Rec> &recs, DBuf<vqm::Rec> &d_rec, DBuf<uint64_t> &pos0, DBuf<uint64_t> &byte0);
    DBuf<uint8_t> d_bases_, d_quals_;
    DBuf<uint64_t> d_off_;
    DBuf<uint16_t> d_tab_;
    size_t n_reads_;
};

// ---- cliques: vq_clique_host.cpp (the enumerator) / vq_clique.hip (the pile-up kernel; ViralQuasispecies --cliques=true) -----
// The maximal cliques of a graph.txt image (n, m, then m lines "u,v") in the order and with the vertex order quick-cliques'
// degeneracy algorithm lists them: `text` = what `qc --algorithm=degeneracy` prints, cliques = the vertices, clique k at
// [off[k], off[k + 1]).  Pure host code.
struct VqCliqueList {
    std::string text;
    std::vector<uint32_t> members;
    std::vector<uint64_t> off;
};
VqCliqueList vq_enumerate_cliques(const std::string &graph_text);

namespace vqc {
constexpr int WG = 256;
constexpr int WAVE = 64;
constexpr uint32_t MAX_PILE = 63;                // reads of one pile-up: 3 * min_clique_size with min_clique_size <= 21
constexpr uint32_t MAX_MIN_CLIQUE = 21;
// The margin of DESIGN.md 4.3f: a column whose 1 - p_incorrect lies this close to minQual, or whose p_incorrect lies this close
// to 10^-9.3, goes back to the host; the value in front of round() gets X_SLOPE * MARGIN / p_incorrect + X_FLOOR.
constexpr double MARGIN = 0x1p-44;
constexpr double X_SLOPE = 4.35;                 // > 10 / ln 10
constexpr double X_FLOOR = 0x1p-36;
constexpr double MIN_PROB = 1e-290;              // a best base less likely than this goes back too: pow near the subnormals
struct Pile {                                    // one clique's pile-up
    uint32_t first, n;                           // its entries
    uint32_t total_len, trim_pos;                // columns; the first one that is written (0 without error correction)
    uint64_t col0;                               // its first column in the column buffers
};
struct Entry { uint32_t read, pos, rev; };      // read `read` (reverse-complemented when rev) from column pos on
struct Result { uint32_t stop, empty; };         // columns [trim_pos, stop) are the consensus; empty: a column without a read
}  // namespace vqc

// ---- superread: vq_superread.cpp (what mergeAlongEdges and cliquesToSuperreads share; pure host, no file is touched) --------
// refused in a read (HLMI_EINVAL): a base outside A C G T N, a quality outside '!' .. '~', a quality line of another length
void vq_check_read(const char *seq, size_t len, const char *qual, size_t qlen, const char *what, size_t k);
void vq_merge_check_reads(const std::vector<std::string> &seq, const std::vector<std::string> &qual);
constexpr double VQ_MIN_QUAL = 0.9;                           // ViralQuasispecies.cpp:62 (--min_qual default) -> SRBuilder.h:89
void vq_check_min_qual(double min_qual, const char *step);     // HLMI_EINVAL outside [0, 1], a NaN included
// SRBuilder::consensus_pos (:297-402) of n >= 1 nucleotides (A C G T N) with their phreds, in the reference's expression order
// with the host's libm -> (base << 8) | quality character.  The one evaluation: tables and column redo both come from it
uint16_t vq_consensus_pos(const char *nuc, const int *phred, int n, double min_qual = VQ_MIN_QUAL);
// the vqm::T_* tables of one minQual, built once per distinct value; refuses a value vq_check_min_qual refuses
const std::vector<uint16_t> &vq_consensus_tables(double min_qual);

// OriginalIndex of a single-end original (Types.h): forward, index1, len1
struct VqOrig { bool forward; long index; int len; };
using VqOriginals = std::map<uint64_t, VqOrig>;                // ascending original id: the order the lines are written in
// buildOriginalsDict, the branch that reads subreads.txt (OverlapGraph.cpp:799-845), over the file's text
std::map<uint64_t, VqOriginals> vq_parse_subreads(const std::string &data, const char *path);
void vq_subreads_line(std::string &s, uint64_t id, const VqOriginals &o);
// constructSuperread :750-806 for one member of a super-read: its originals go into `merged` unless already there.  forward =
// the vertex label, idx1 = index1 - startpos1 of calcSubreadInfo (the read's offset minus trim_pos), read_len = |read|
void vq_originals_add(VqOriginals &merged, const VqOriginals &of_read, bool forward, bool first_it, long idx1, long read_len);
// a reverse read written forward (:1204-1216): orientation flipped, index mirrored
void vq_originals_mirror(VqOriginals &o, long read_len);
// original_ID_dict (buildOriginalsDict): first_it: every read is its own original at index 0, forward; else `dict` = the lines
// of subreads_in (the driver fills it) and a read without one is refused.  `step` names the caller in messages.
struct VqOriginalsDict {
    VqOriginalsDict(const char *step, bool first_it, const char *subreads_in);     // refuses first_it off without a file
    VqOriginals originals_of(const VqGraphState &g, uint32_t v) const;
    const char *step, *subreads_in;
    bool first_it;
    std::map<uint64_t, VqOriginals> dict;
};
// getEdgeInfo(u, v) (OverlapGraph.cpp:263-282): the first u -> v of u's list, else the first v -> u of v's; NULL: neither
const VqEdge *vq_edge_info(const VqGraphState &g, uint32_t u, uint32_t v);
using VqPlaced = std::vector<std::pair<int64_t, uint32_t>>;    // (offset, vertex) in list order
// sort_vertices (:33-286), single-end: `clique` ascending, its first vertex the base -> order = every member, each in front of
// the first entry that is not smaller, shifted to start at 0; returns the total length.  Refuses a member without an edge to
// the base and a total of 2^30 and more.
int64_t vq_place(const VqGraphState &g, const std::vector<uint32_t> &clique, const char *step, VqPlaced &order);
// filter_subreads (:597-636) with sortVerticesByEndpos (:639-652, std::sort on the end alone): the `num` entries that stay
VqPlaced vq_filter_subreads(const VqGraphState &g, size_t num, uint32_t base, const VqPlaced &order);
// consensus_pos of one pile-up column by the host's libm: the entries that cover it in list order, reversed ones complemented
uint16_t vq_consensus_column(const VqGraphState &g, const vqc::Entry *entries, uint32_t n_entries, uint32_t column,
                             double min_qual = VQ_MIN_QUAL);
bool vq_n_rate_ok(uint64_t n, uint64_t len);                   // Read::test_N_rate (Read.h:214-233)
// The reads in no super-read (:1145-1222, :1282-1372), vertices ascending: dropped when shorter than keep_singletons or failing
// the N rate (read_n = 'N's per read), to `diverted` when flagged in `divert` (NULL: none), else a record from id first_id on
// - a reverse read as its forward copy with mirrored originals - and its subreads.txt line.
struct VqLoneCounts { uint64_t short_reads = 0, n_reads = 0, trivial = 0, trivial_reverse = 0; };
VqLoneCounts vq_lone_reads(const VqGraphState &g, const VqOriginalsDict &dict, const std::vector<uint8_t> &visited,
                           const std::vector<uint32_t> &read_n, uint32_t keep_singletons, const std::vector<uint8_t> *divert,
                           uint32_t first_id, std::vector<vqm::Rec> &recs, std::string &subreads, std::vector<uint32_t> *diverted);

// ---- branch: vq_branch_host.cpp / vq_branch.hip (BranchReduction::readBasedBranchReduction, --branch_reduction=true) --------
namespace vqb {
constexpr int WG = 256;
constexpr int WAVE = 64;
constexpr uint32_t MAX_DIFF = 100;               // findDiffPos keeps the first 100 positions of a pair (:703)
constexpr uint32_t NONE = 0xffffffffu;
using vqk::SEARCH_STEPS;
struct Pair {                                    // one compared neighbour pair: sequence a from `rel` on against b from 0
    uint32_t a, b;                               // vertices
    uint32_t rel, len;                           // len >= 1 common bases
    uint32_t flags;                              // 1: both reverse-complemented (the branching vertex's label), 2: compared reversed
};
struct Slot {                                    // one (branch, neighbour)
    uint32_t node, nb;                           // the branching vertex, the neighbour (the contig)
    int32_t startpos;
    uint32_t rc;                                 // the contig is reverse-complemented
    uint32_t diff0, diff1;                       // the branch's sorted, uniqued difference list: diff[diff0, diff1)
};
// The device side: reads and original reads resident, bases concatenated, read r at [off[r], off[r + 1]) (VqMergeDev's layout)
class Dev {
public:
    Dev(const std::vector<std::string> &reads, const std::vector<std::string> &originals);
    // cnt[p] = mismatches found (at most MAX_DIFF), pos[p * MAX_DIFF + k] = the k-th one's position in compare order
    void diff_positions(const std::vector<Pair> &pairs, std::vector<uint32_t> &cnt, std::vector<uint32_t> &pos);
    // Originals of the vertices as a CSR (vertex v: [ooff[v], ooff[v + 1]), ascending id): id, row in the original FASTQ,
    // forward, index1.  Item t of slot s (items [item0[s], item0[s + 1])) is original t - item0[s] of slots[s].nb.
    // -> ev[2 * t], ev[2 * t + 1] = the subread's id / the joint id where checkReadEvidence holds, else NONE
    void evidence(const std::vector<Slot> &slots, const std::vector<uint32_t> &item0, const std::vector<int32_t> &diff,
                  const std::vector<uint32_t> &ooff, const std::vector<uint32_t> &oid, const std::vector<uint32_t> &orow,
                  const std::vector<uint8_t> &ofwd, const std::vector<int32_t> &oidx, uint32_t se_count, uint32_t pe_count,
                  std::vector<uint32_t> &ev);
private:
    DBuf<uint8_t> d_reads_, d_orig_;
    DBuf<uint64_t> d_roff_, d_ooff_;
};
}  // namespace vqb
// What vq_graph_run needs for --branch_reduction=true.  prepare() runs in front of the graph's first write and refuses what
// hlmi_vq_branch_graph documents; reduce() is readBasedBranchReduction over the graph as removeTips left it (out-lists already
// through sortAdjOut): the missing edges and the (source, target) pairs to remove, both in the reference's push order.
struct VqBranchRun {
    hlmi_vq_branch_opts bo{};
    const char *original_fastq = nullptr, *table_path = nullptr;
    const VqOriginalsDict *dict = nullptr;
    hlmi_vq_branch_stats *st = nullptr;
    Singles originals;
    std::map<int, int> table;
    void prepare(const hlmi_vq_graph_opts &o, const Singles &reads);
    void reduce(const hlmi_vq_graph_opts &o, const std::vector<std::string> &seq, const std::vector<uint64_t> &id,
                const std::vector<std::vector<VqEdge>> &out, const std::vector<uint8_t> &orient, std::vector<VqEdge> &missing,
                std::vector<std::pair<uint32_t, uint32_t>> &removed, std::string &report);
};
void vq_branch_opts_polyte(hlmi_vq_branch_opts *o);
void vq_branch_graph_run(const char *fastq, const char *overlaps, const char *subreads_in, const char *original_fastq, const char *table,
                         const hlmi_vq_graph_opts &go, const hlmi_vq_branch_opts &bo, const char *out_dir, hlmi_vq_graph_stats *gst,
                         hlmi_vq_branch_stats *bst);
void vq_branch_iteration_run(const char *fastq, const char *overlaps, const char *subreads_in, const char *original_fastq,
                             const char *table, const hlmi_vq_graph_opts &go, const hlmi_vq_branch_opts &bo, const hlmi_vq_clique_opts &co,
                             const hlmi_vq_next_opts &no, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                             hlmi_vq_branch_stats *bst, hlmi_vq_clique_stats *cst, hlmi_vq_clique_next_stats *nst);

// ---- drivers: vq_superread_run.cpp (include/hylight_mi.h; vq_iteration_run is declared with `next` below).  min_qual is
// --min_qual: it reaches the tables, the pile-up kernel and the host's column redo, and is checked before a file is written ----
void vq_merge_opts_stageb(hlmi_vq_merge_opts *o);
void vq_merge_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                  const hlmi_vq_merge_opts &mo, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst);
void vq_consensus_pair(const char *seq1, const char *qual1, uint32_t len1, uint32_t qlen1, const char *seq2, const char *qual2,
                       uint32_t len2, uint32_t qlen2, uint32_t pos, double min_qual, char *out_seq, char *out_qual, uint32_t *out_len);
void vq_clique_opts_polyte(hlmi_vq_clique_opts *o, int error_correction);
void vq_cliques_of_graph(const char *graph_txt, const char *cliques_out, uint64_t *n_cliques);
void vq_cliques_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                    const hlmi_vq_clique_opts &co, double min_qual, const char *out_dir, hlmi_vq_graph_stats *gst,
                    hlmi_vq_clique_stats *cst);

// ---- next: vq_next.hip (SRBuilder::findNextOverlaps, FNO 1) ---------------------------------------------------------------
namespace vqn {
constexpr int WG = 256;
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t LINE_WIDTH = 64;              // lines up to this many bytes are ordered on the device (8 words of 8 bytes)
using vqk::SEARCH_STEPS;
}  // namespace vqn
// What SRBuilder leaves per vertex for updateOverlap: nodes_to_SR as a CSR over the vertices, one (new id, findCliqueIndex)
// per entry in ascending id, and the new reads' lengths.  An unvisited vertex that was copied is a list of one entry, its new
// id at index 0, and flagged; a visited vertex in no super-read (too short, N rate, diverted) is an empty list.
struct VqNextTables {
    std::vector<uint32_t> start;                 // list of vertex v: entries [start[v], start[v + 1])
    std::vector<uint32_t> id;                    // new id of the super-read (of the copied read)
    std::vector<int32_t> idx;                    // index1 - startpos1 of the vertex in it: SIGNED (negative in front of trim_pos)
    std::vector<uint8_t> copied;                 // per vertex
    std::vector<uint32_t> len;                   // per new id: the read's length
};
struct VqMember { uint32_t vertex, id; int32_t idx; };          // one member of kept super-read `id`
// vq_superread.cpp (pure host): members = those of the kept super-reads 0 .. n_superreads - 1 in ascending id, lone = the records
// vq_lone_reads made (ids from n_superreads on)
VqNextTables vq_next_tables(uint32_t n_vertices, const std::vector<VqMember> &members, size_t n_superreads,
                            const std::vector<uint32_t> &superread_len, const std::vector<vqm::Rec> &lone);
void vq_next_tables_check(const VqNextTables &t, uint32_t n_vertices);      // HLMI_EINVAL: an index the device would follow out of bounds
void vq_next_opts_stageb(hlmi_vq_next_opts *o);
// -> the image of overlaps.txt.  out = the out-lists that are source group 1 and that checkEdge walks: g.out behind a merge,
// vq_cliques_out(g) behind the cliques.  HLMI_EINVAL: 2^32 - 1 candidates and more.
std::string vq_next_run(const VqGraphState &g, const std::vector<std::vector<VqEdge>> &out, const VqNextTables &t,
                        double edge_threshold, const hlmi_vq_next_opts &no, hlmi_vq_clique_next_stats *st);
void vq_iteration_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                      const hlmi_vq_merge_opts &mo, const hlmi_vq_next_opts &no, double min_qual, const char *out_dir,
                      hlmi_vq_graph_stats *gst, hlmi_vq_merge_stats *mst, hlmi_vq_next_stats *nst);
void vq_clique_iteration_run(const char *fastq, const char *overlaps, const char *subreads_in, const hlmi_vq_graph_opts &go,
                             const hlmi_vq_clique_opts &co, const hlmi_vq_next_opts &no, double min_qual, const char *out_dir,
                             hlmi_vq_graph_stats *gst, hlmi_vq_clique_stats *cst, hlmi_vq_clique_next_stats *nst);

}  // namespace hlmi
