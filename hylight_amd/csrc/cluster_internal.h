// cluster_internal.h - what cluster.hip (the data-parallel half of the short-read clustering, HyLight.py:215-226) offers
// cluster_host.cpp (the session layout, the sequential union pass and the writers).  Everything lives in HBM between
// the calls; the host only sees the survivors of each session's prefilter, the grouped node order and the demultiplexed
// record bytes.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

namespace hlmi {

constexpr uint32_t CL_NONE = 0xffffffffu;

// per readnames entry (node v = index + 1): where get_readnames.py's line[1:-3] starts in the FASTQ, its length, and the
// length of the key bin_pointer uses (the same bytes after str.rstrip())
struct ClNode {
    uint64_t off;
    uint32_t raw_len, key_len;
};

struct ClusterDev {
    // FASTQ (uploaded whole)
    DBuf<uint8_t> fq;
    size_t fq_bytes = 0, n_lines = 0, n_records = 0;
    DBuf<uint64_t> fq_line;            // line starts
    DBuf<uint32_t> rec_dm_len, rec_flags;   // demux name length, bit 0 mate-1 header, bit 1 written at all
    DBuf<uint64_t> rec_dm_off;
    // node table: key hashes sorted, node id beside each
    size_t n_nodes = 0;
    DBuf<uint64_t> node_off;           // key offsets (index v - 1)
    DBuf<uint32_t> node_len;
    DBuf<uint64_t> tab_hash;
    DBuf<uint32_t> tab_node;
    uint64_t seed = 0;
    // union state frozen at session start (index v, 0 unused)
    DBuf<uint32_t> root_of, size_of, new_root;
    // current PAF window
    DBuf<uint8_t> paf;
    size_t paf_cap = 0;
    DBuf<uint32_t> row_a, row_b;
    DBuf<uint8_t> flag;
    DBuf<uint32_t> idx;
};

// FASTQ: upload, line / record scan, byte checks (throws HLMI_EINVAL), the readnames list and the node table.
std::vector<ClNode> cl_load_fastq(ClusterDev &d, const uint8_t *fq, size_t n);
// the rows of the window txt[0 .. n) (whole lines): node ids of their endpoints on the device; returns the line starts
// (relative to the window).  Refuses bad bytes, short rows and unknown names.
std::vector<uint32_t> cl_load_window(ClusterDev &d, const uint8_t *txt, size_t n);
// getchunkfile over window rows [r0, r1) against the frozen state: the surviving (a, b) pairs in row order; *strict gets
// the rows refused only because their sum equals `size`
std::vector<uint32_t> cl_prefilter(ClusterDev &d, size_t r0, size_t r1, int64_t size, uint64_t *strict);
// the session's attachments: new_root of every root that was hung under another one, and the new sizes of the roots
// that grew; root_of is then brought up to date for every node
void cl_apply(ClusterDev &d, const std::vector<uint32_t> &attach, const std::vector<uint32_t> &sizes);
// getclusters.py: the kept nodes of the slices in (JSON key, node) order, with the run length of each key; *k_ge20 gets
// the number of nodes in clusters of size >= 20
void cl_group(ClusterDev &d, int threads, std::vector<uint32_t> &nodes, std::vector<uint32_t> &key_cid,
              std::vector<uint32_t> &key_len, uint64_t *k_ge20);
// get_fq_cluster.py: node_key[v] = JSON key rank of node v (CL_NONE: not kept); the records of every key's two files in
// FASTQ order, gathered into `out`, file f = rank * 2 + (mate 2) spans [fstart[f], fend[f])
void cl_demux(ClusterDev &d, const std::vector<uint32_t> &node_key, size_t n_keys, std::vector<uint8_t> &out,
              std::vector<uint64_t> &fstart, std::vector<uint64_t> &fend);

}  // namespace hlmi
