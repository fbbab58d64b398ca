// cluster.hip - the data-parallel half of HyLight's short-read clustering (script/HyLight.py:215-226: get_readnames.py,
// bin_pointer_limited_filechunks_shortpath2.py, getclusters.py, get_fq_cluster.py).  cluster_host.cpp drives it.
//
//   FASTQ     one thread per 4-line record: the readnames rule ('/1' anywhere in the header -> line[1:-3]), the key
//             bin_pointer looks up (that name after str.rstrip()), the demux name (re.split('[@/]', header)[-2]) and
//             the mate rule (/1$); keys hashed, sorted, neighbours compared byte by byte (duplicates refused,
//             collisions re-seeded) - the name table of graph_dev.hip (text_dev.h)
//   PAF       one thread per row of a window: columns 1 and 6 minus two characters, looked up in the table
//   sessions  getchunkfile: every row of a session against root_of / size_of frozen at its start, then a compaction;
//             after the host's union pass the attached roots get their new root and every node is moved along
//   grouping  root -> cluster id (= the root's rank), the >= 20 filter, getclusters' slicing (a scan over the keep
//             flags), the JSON key order (first slice, then cluster id) by two sorts
//   demux     per record the file index (key rank * 2 + mate), a stable sort by it, the record bytes gathered into one
//             buffer that the host cuts into files
// Integer and byte work: HBM-bound, no MFMA.
#include "cluster_internal.h"
#include "dev_prims.h"
#include "text_dev.h"

namespace hlmi {

namespace {
constexpr int WG = 256;
inline dim3 grid1(size_t n) { return grid_for(n, WG); }
constexpr size_t SLAB = size_t(1) << 31;          // line-start selections per slab (32-bit indices)

enum : uint32_t {
    TXT_CR = 1u,           // '\r'
    TXT_HIGH = 2u,         // byte >= 0x80
    TXT_SPLIT = 4u,        // another str.splitlines() separator (\v \f \x1c \x1d \x1e) or '"' (csv quoting)
};
enum : uint32_t {
    ROW_SHORT = 1u,        // fewer than 12 columns
    ROW_UNKNOWN = 2u,      // endpoint not in readnames
    FQ_NOT_AT = 4u,        // header line without '@'
    FQ_QUOTE = 8u,         // readnames key with '"'
    TAB_DUP = 16u,         // two readnames keys equal
    TAB_COLLISION = 32u,   // two different keys, one hash
};

__global__ void byte_class_kernel(const uint8_t *txt, size_t n, uint32_t *bits) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    uint32_t b = 0;
    for (size_t k = i * 16, e = k + 16 < n ? k + 16 : n; k < e; ++k) {
        const uint8_t c = txt[k];
        if (c == '\r') b |= TXT_CR;
        if (c >= 0x80) b |= TXT_HIGH;
        if (c == 0x0b || c == 0x0c || c == 0x1c || c == 0x1d || c == 0x1e || c == '"') b |= TXT_SPLIT;
    }
    if (b) atomicOr(bits, b);
}

__global__ void add_base_u64_kernel(const uint32_t *rel, size_t n, uint64_t base, uint64_t *out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = base + rel[i];
}

__device__ __forceinline__ bool py_space(uint8_t c) {    // str.isspace() on ASCII
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f);
}

// record r: header line [a, e) (e past its '\n' when there is one)
__global__ void fq_record_kernel(const uint8_t *txt, size_t n, const uint64_t *ls, size_t n_lines, size_t n_rec,
                                 uint8_t *is_name, uint64_t *dm_off, uint32_t *dm_len, uint32_t *rflags, uint32_t *bits) {
    size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    const size_t L = 4 * r;
    const uint64_t a = ls[L], e = L + 1 < n_lines ? ls[L + 1] : n;
    if (txt[a] != '@') atomicOr(bits, FQ_NOT_AT);
    bool slash1 = false;
    int64_t p1 = -1, p2 = -1;                                   // the last two '@' / '/' positions
    for (uint64_t k = a; k < e; ++k) {
        const uint8_t c = txt[k];
        if (c == '/' && k + 1 < e && txt[k + 1] == '1') slash1 = true;
        if (c == '@' || c == '/') { p1 = p2; p2 = (int64_t)(k - a); }
    }
    is_name[r] = slash1 ? 1 : 0;
    // re.split(...)[-2]: the piece before the last separator (the header starts with '@': there is one)
    dm_off[r] = a + (uint64_t)(p1 + 1);
    dm_len[r] = (uint32_t)(p2 < 0 ? 0 : p2 - (p1 + 1));
    const uint64_t len = e - a;
    const bool nl = len && txt[e - 1] == '\n';
    const uint64_t t = nl ? e - 1 : e;                           // /1$: at the end or before a final newline
    const bool mate1 = t - a >= 2 && txt[t - 2] == '/' && txt[t - 1] == '1';
    // get_fq_cluster.py writes a record when it meets the next header (i > 0) or at the end when the last line index i > 0
    const bool written = n_lines > 1;
    rflags[r] = (mate1 ? 1u : 0u) | (written ? 2u : 0u);
}

// node v = k + 1 for the k-th record with a readnames entry: line[1:-3], then rstrip
__global__ void node_kernel(const uint8_t *txt, size_t n, const uint64_t *ls, size_t n_lines, const uint32_t *name_rec,
                            size_t n_nodes, uint64_t *off, uint32_t *raw_len, uint32_t *key_len, uint32_t *bits) {
    size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= n_nodes) return;
    const size_t L = 4 * (size_t)name_rec[k];
    const uint64_t a = ls[L], e = L + 1 < n_lines ? ls[L + 1] : n;
    const uint64_t len = e - a;
    const uint32_t raw = (uint32_t)(len > 4 ? len - 4 : 0);
    uint32_t kl = raw;
    while (kl && py_space(txt[a + 1 + kl - 1])) --kl;
    for (uint32_t i = 0; i < kl; ++i)
        if (txt[a + 1 + i] == '"') atomicOr(bits, FQ_QUOTE);
    off[k] = a + 1;
    raw_len[k] = raw;
    key_len[k] = kl;
}

__global__ void node_hash_kernel(const uint8_t *txt, const uint64_t *off, const uint32_t *len, size_t n_nodes, uint64_t seed,
                                 uint64_t *hash, uint32_t *node) {
    size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= n_nodes) return;
    hash[k] = name_hash64(txt, off[k], len[k], seed);
    node[k] = (uint32_t)(k + 1);
}

// sorted table: equal neighbours are a duplicate name or a collision
__global__ void table_check_kernel(const uint8_t *txt, const uint64_t *off, const uint32_t *len, const uint64_t *hash,
                                   const uint32_t *node, size_t n, uint32_t *bits) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i == 0 || i >= n || hash[i] != hash[i - 1]) return;
    const uint32_t u = node[i - 1] - 1, v = node[i] - 1;
    atomicOr(bits, bytes_equal(txt, off[u], len[u], txt, off[v], len[v]) ? TAB_DUP : TAB_COLLISION);
}

// node id of the name s[o .. o + l) (0: not in the table)
__device__ uint32_t lookup(const uint8_t *s, uint64_t o, uint32_t l, const uint8_t *fq, const uint64_t *noff,
                           const uint32_t *nlen, const uint64_t *hash, const uint32_t *node, size_t n, uint64_t seed) {
    const uint64_t h = name_hash64(s, o, l, seed);
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t m = (lo + hi) / 2;
        if (hash[m] < h) lo = m + 1;
        else hi = m;
    }
    if (lo == n || hash[lo] != h) return 0;
    const uint32_t v = node[lo];
    return bytes_equal(s, o, l, fq, noff[v - 1], nlen[v - 1]) ? v : 0;
}

// one PAF row: split the line (without its '\n', right-stripped) at tabs; columns 1 and 6 lose two characters
__global__ void paf_row_kernel(const uint8_t *txt, size_t n, const uint32_t *ls, size_t n_rows, const uint8_t *fq,
                               const uint64_t *noff, const uint32_t *nlen, const uint64_t *hash, const uint32_t *node,
                               size_t n_nodes, uint64_t seed, uint32_t *ra, uint32_t *rb, uint32_t *bits) {
    size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t a = ls[r];
    uint64_t e = r + 1 < n_rows ? ls[r + 1] : n;
    if (e > a && txt[e - 1] == '\n') --e;
    while (e > a && py_space(txt[e - 1])) --e;
    uint32_t fields = 1;
    uint64_t s0 = a, e0 = e, s5 = e, e5 = e;
    for (uint64_t k = a; k < e; ++k) {
        if (txt[k] != '\t') continue;
        if (fields == 1) e0 = k;
        if (fields == 5) s5 = k + 1;
        if (fields == 6) e5 = k;
        ++fields;
    }
    if (fields < 12) {
        atomicOr(bits, ROW_SHORT);
        ra[r] = rb[r] = 0;
        return;
    }
    const uint32_t l0 = (uint32_t)(e0 - s0), l5 = (uint32_t)(e5 - s5);
    const uint32_t v1 = lookup(txt, s0, l0 > 2 ? l0 - 2 : 0, fq, noff, nlen, hash, node, n_nodes, seed);
    const uint32_t v2 = lookup(txt, s5, l5 > 2 ? l5 - 2 : 0, fq, noff, nlen, hash, node, n_nodes, seed);
    if (!v1 || !v2) atomicOr(bits, ROW_UNKNOWN);
    ra[r] = v1;
    rb[r] = v2;
}

__global__ void init_state_kernel(uint32_t *root_of, uint32_t *size_of, uint32_t *new_root, size_t n) {
    size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (v > n) return;
    root_of[v] = (uint32_t)v;
    size_of[v] = 1;
    new_root[v] = 0;
}

// getchunkfile (bin_pointer:95-109): different cluster ids and size1 + size2 < size, both at session start
__global__ void prefilter_kernel(const uint32_t *ra, const uint32_t *rb, size_t r0, size_t n, const uint32_t *root_of,
                                 const uint32_t *size_of, int64_t size, uint8_t *flag, uint32_t *strict) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = root_of[ra[r0 + i]], y = root_of[rb[r0 + i]];
    const int64_t s = (int64_t)size_of[x] + size_of[y];
    flag[i] = (x != y && s < size) ? 1 : 0;
    if (x != y && s == size) atomicAdd(strict, 1u);
}
__global__ void gather_pairs_kernel(const uint32_t *ra, const uint32_t *rb, size_t r0, const uint32_t *idx, size_t n,
                                    uint32_t *out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[2 * i] = ra[r0 + idx[i]];
    out[2 * i + 1] = rb[r0 + idx[i]];
}

// attach[2 k] hangs (now) under attach[2 k + 1]; sizes[2 k] is a root of size sizes[2 k + 1]
__global__ void scatter_kernel(const uint32_t *attach, size_t n_att, const uint32_t *sizes, size_t n_sz, uint32_t *new_root,
                               uint32_t *size_of) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n_att) new_root[attach[2 * i]] = attach[2 * i + 1];
    if (i < n_sz) size_of[sizes[2 * i]] = sizes[2 * i + 1];
}
__global__ void refresh_kernel(uint32_t *root_of, const uint32_t *new_root, size_t n) {
    size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x + 1;
    if (v > n) return;
    const uint32_t nr = new_root[root_of[v]];
    if (nr) root_of[v] = nr;
}
__global__ void unscatter_kernel(const uint32_t *attach, size_t n_att, uint32_t *new_root) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n_att) new_root[attach[2 * i]] = 0;
}

// getclusters.py: keep[v - 1] = final size of v's cluster >= 20
__global__ void keep_kernel(const uint32_t *root_of, const uint32_t *size_of, size_t n, uint32_t *keep) {
    size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k < n) keep[k] = size_of[root_of[k + 1]] >= 20 ? 1u : 0u;
}
// the first min(threads, 60) * dictsize kept nodes survive the slicing
__global__ void slice_kernel(const uint32_t *keep, const uint32_t *rank, size_t n, uint64_t limit, uint8_t *flag) {
    size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k < n) flag[k] = keep[k] && rank[k] < limit ? 1 : 0;
}
__global__ void cid_key_kernel(const uint32_t *idx, size_t n, const uint32_t *root_of, uint64_t *key) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) key[i] = (uint64_t)root_of[idx[i] + 1] << 32 | (idx[i] + 1);
}
// cluster c (run heads[c] of the (cid, node) order): key (slice of its first node, cid); slice = kept rank / dictsize
__global__ void cluster_key_kernel(const uint64_t *key, const uint32_t *heads, size_t n_cl, const uint32_t *rank,
                                   uint64_t dictsize, uint64_t *ckey, uint32_t *cval) {
    size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (c >= n_cl) return;
    const uint64_t k = key[heads[c]];
    const uint32_t v = (uint32_t)k, cid = (uint32_t)(k >> 32);
    ckey[c] = (uint64_t)(rank[v - 1] / dictsize) << 32 | cid;
    cval[c] = (uint32_t)c;
}

// get_fq_cluster.py: file index of record r (CL_NONE: not written)
__global__ void rec_file_kernel(const uint8_t *fq, const uint64_t *dm_off, const uint32_t *dm_len, const uint32_t *rflags,
                                size_t n_rec, const uint64_t *noff, const uint32_t *nlen, const uint64_t *hash,
                                const uint32_t *node, size_t n_nodes, uint64_t seed, const uint32_t *node_key,
                                uint32_t *file, uint8_t *flag) {
    size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    uint32_t f = CL_NONE;
    if (rflags[r] & 2u) {
        const uint32_t v = lookup(fq, dm_off[r], dm_len[r], fq, noff, nlen, hash, node, n_nodes, seed);
        if (v && node_key[v] != CL_NONE) f = node_key[v] * 2 + ((rflags[r] & 1u) ? 0u : 1u);
    }
    file[r] = f;
    flag[r] = f != CL_NONE ? 1 : 0;
}
__global__ void rec_select_kernel(const uint32_t *file, const uint32_t *idx, size_t n, uint32_t *key) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) key[i] = file[idx[i]];
}
__global__ void rec_len_kernel(const uint32_t *rec, size_t n, const uint64_t *ls, size_t n_lines, size_t fq_bytes,
                               uint32_t *len) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t L = 4 * (size_t)rec[i];
    const uint64_t a = ls[L], e = L + 4 < n_lines ? ls[L + 4] : fq_bytes;
    len[i] = (uint32_t)(e - a);
}
// one wave per record
__global__ void rec_gather_kernel(const uint8_t *fq, const uint32_t *rec, const uint64_t *ls, const uint64_t *at,
                                  const uint32_t *len, size_t n, uint8_t *out) {
    const size_t i = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    if (i >= n) return;
    const uint64_t a = ls[4 * (size_t)rec[i]], o = at[i];
    for (uint32_t k = lane; k < len[i]; k += 64) out[o + k] = fq[a + k];
}
__global__ void file_span_kernel(const uint32_t *key, const uint64_t *at, const uint32_t *len, size_t n, uint64_t *fstart,
                                 uint64_t *fend) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || key[i] != key[i - 1]) fstart[key[i]] = at[i];
    if (i + 1 == n || key[i] != key[i + 1]) fend[key[i]] = at[i] + len[i];
}

// line starts of txt[0 .. n) as 64-bit offsets (slabs of 2^31 bytes for the 32-bit selection)
DBuf<uint64_t> line_starts64(const uint8_t *txt, size_t n) {
    std::vector<DBuf<uint64_t>> parts;
    size_t total = 0;
    DBuf<uint8_t> flag(std::min(n, SLAB));
    DBuf<uint32_t> rel(std::min(n, SLAB));
    for (size_t base = 0; base < n; base += SLAB) {
        const size_t m = std::min(SLAB, n - base);
        hipLaunchKernelGGL(line_start_kernel, grid1(m), dim3(WG), 0, stream(), txt, base, m, flag.p);
        const size_t c = select_flagged_indices(flag.p, rel.p, m);
        DBuf<uint64_t> part(c);
        if (c) hipLaunchKernelGGL(add_base_u64_kernel, grid1(c), dim3(WG), 0, stream(), rel.p, c, (uint64_t)base, part.p);
        total += c;
        parts.push_back(std::move(part));
    }
    if (parts.size() == 1) return std::move(parts[0]);
    DBuf<uint64_t> out(total);
    size_t at = 0;
    for (auto &p : parts) {
        if (p.n) HIP_CHECK(hipMemcpyAsync(out.p + at, p.p, p.n * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream()));
        at += p.n;
    }
    return out;
}

uint32_t text_bits(const uint8_t *txt, size_t n) {
    DBuf<uint32_t> bits(1);
    bits.zero();
    if (n) hipLaunchKernelGGL(byte_class_kernel, grid1(cdiv(n, 16)), dim3(WG), 0, stream(), txt, n, bits.p);
    return download_one(bits.p);
}
}  // namespace

std::vector<ClNode> cl_load_fastq(ClusterDev &d, const uint8_t *h, size_t n) {
    KTimer kt("cluster_fastq");
    d.fq.upload(h, n);
    d.fq_bytes = n;
    const uint32_t tb = text_bits(d.fq.p, n);
    if (tb & TXT_CR) fail(HLMI_EINVAL, "cluster: FASTQ with CR line ends (the reference reads it with universal newlines)");
    if (tb & TXT_HIGH) fail(HLMI_EINVAL, "cluster: FASTQ byte >= 0x80 (names are ASCII; the reference decodes UTF-8)");
    d.fq_line = line_starts64(d.fq.p, n);
    d.n_lines = d.fq_line.n;
    d.n_records = (d.n_lines + 3) / 4;
    const size_t R = d.n_records;
    DBuf<uint8_t> is_name(R);
    d.rec_dm_off.alloc(R);
    d.rec_dm_len.alloc(R);
    d.rec_flags.alloc(R);
    DBuf<uint32_t> bits(1);
    bits.zero();
    if (R)
        hipLaunchKernelGGL(fq_record_kernel, grid1(R), dim3(WG), 0, stream(), d.fq.p, n, d.fq_line.p, d.n_lines, R, is_name.p,
                           d.rec_dm_off.p, d.rec_dm_len.p, d.rec_flags.p, bits.p);
    DBuf<uint32_t> name_rec(R);
    const size_t N = R ? select_flagged_indices(is_name.p, name_rec.p, R) : 0;
    if (N >= CL_NONE - 1) fail(HLMI_EINVAL, "cluster: %zu read names (node ids are 32-bit)", N);
    d.n_nodes = N;
    d.node_off.alloc(N);
    d.node_len.alloc(N);
    DBuf<uint32_t> raw_len(N);
    if (N)
        hipLaunchKernelGGL(node_kernel, grid1(N), dim3(WG), 0, stream(), d.fq.p, n, d.fq_line.p, d.n_lines, name_rec.p, N,
                           d.node_off.p, raw_len.p, d.node_len.p, bits.p);
    uint32_t b = download_one(bits.p);
    if (b & FQ_NOT_AT) fail(HLMI_EINVAL, "cluster: a FASTQ header line does not start with '@' (FASTA input?)");
    if (b & FQ_QUOTE) fail(HLMI_EINVAL, "cluster: read name with '\"' (bin_pointer's csv reader would unquote it)");
    // the name table: re-seeded until no two different keys share a hash
    d.tab_hash.alloc(N);
    d.tab_node.alloc(N);
    for (d.seed = 0x243f6a8885a308d3ull;; d.seed += 0x9e3779b97f4a7c15ull) {
        if (!N) break;
        hipLaunchKernelGGL(node_hash_kernel, grid1(N), dim3(WG), 0, stream(), d.fq.p, d.node_off.p, d.node_len.p, N, d.seed,
                           d.tab_hash.p, d.tab_node.p);
        sort_pairs_u64_u32(d.tab_hash.p, d.tab_node.p, N);
        bits.zero();
        hipLaunchKernelGGL(table_check_kernel, grid1(N), dim3(WG), 0, stream(), d.fq.p, d.node_off.p, d.node_len.p,
                           d.tab_hash.p, d.tab_node.p, N, bits.p);
        b = download_one(bits.p);
        if (b & TAB_DUP) fail(HLMI_EINVAL, "cluster: duplicate read name in readnames.txt (bin_pointer keeps the last rank)");
        if (!(b & TAB_COLLISION)) break;
    }
    d.root_of.alloc(N + 1);
    d.size_of.alloc(N + 1);
    d.new_root.alloc(N + 1);
    hipLaunchKernelGGL(init_state_kernel, grid1(N + 1), dim3(WG), 0, stream(), d.root_of.p, d.size_of.p, d.new_root.p, N);
    const std::vector<uint64_t> off = d.node_off.download();
    const std::vector<uint32_t> raw = raw_len.download(), key = d.node_len.download();
    std::vector<ClNode> nodes(N);
    for (size_t k = 0; k < N; ++k) nodes[k] = ClNode{off[k], raw[k], key[k]};
    return nodes;
}

std::vector<uint32_t> cl_load_window(ClusterDev &d, const uint8_t *h, size_t n) {
    KTimer kt("cluster_paf");
    if (n > d.paf_cap) {
        d.paf.alloc(n);
        d.paf_cap = n;
    }
    if (n) HIP_CHECK(hipMemcpyAsync(d.paf.p, h, n, hipMemcpyHostToDevice, stream()));
    const uint32_t tb = text_bits(d.paf.p, n);
    if (tb & TXT_CR) fail(HLMI_EINVAL, "cluster: PAF with CR line ends");
    if (tb & TXT_HIGH) fail(HLMI_EINVAL, "cluster: PAF byte >= 0x80");
    if (tb & TXT_SPLIT)
        fail(HLMI_EINVAL, "cluster: PAF holds '\"' (csv quoting) or a str.splitlines() separator (\\v \\f \\x1c-\\x1e)");
    if (n > d.flag.n) d.flag.alloc(n);
    if (n > d.idx.n) d.idx.alloc(n);
    hipLaunchKernelGGL(line_start_kernel, grid1(n), dim3(WG), 0, stream(), d.paf.p, (size_t)0, n, d.flag.p);
    const size_t rows = n ? select_flagged_indices(d.flag.p, d.idx.p, n) : 0;
    if (rows > d.row_a.n) {
        d.row_a.alloc(rows);
        d.row_b.alloc(rows);
    }
    DBuf<uint32_t> bits(1);
    bits.zero();
    if (rows)
        hipLaunchKernelGGL(paf_row_kernel, grid1(rows), dim3(WG), 0, stream(), d.paf.p, n, d.idx.p, rows, d.fq.p,
                           d.node_off.p, d.node_len.p, d.tab_hash.p, d.tab_node.p, d.n_nodes, d.seed, d.row_a.p, d.row_b.p,
                           bits.p);
    const uint32_t b = download_one(bits.p);
    if (b & ROW_SHORT) fail(HLMI_EINVAL, "cluster: PAF row with fewer than 12 columns");
    if (b & ROW_UNKNOWN)
        fail(HLMI_EINVAL, "cluster: PAF endpoint (column 1 or 6 minus two characters) not in readnames "
                          "(the reference's chunk worker dies on it and truncates its chunk)");
    std::vector<uint32_t> ls(rows);
    if (rows) {
        HIP_CHECK(hipMemcpyAsync(ls.data(), d.idx.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
        sync();
    }
    return ls;
}

std::vector<uint32_t> cl_prefilter(ClusterDev &d, size_t r0, size_t r1, int64_t size, uint64_t *strict) {
    KTimer kt("cluster_prefilter");
    const size_t n = r1 - r0;
    std::vector<uint32_t> pairs;
    *strict = 0;
    if (!n) return pairs;
    DBuf<uint32_t> cnt(1);
    cnt.zero();
    hipLaunchKernelGGL(prefilter_kernel, grid1(n), dim3(WG), 0, stream(), d.row_a.p, d.row_b.p, r0, n, d.root_of.p,
                       d.size_of.p, size, d.flag.p, cnt.p);
    const size_t m = select_flagged_indices(d.flag.p, d.idx.p, n);
    *strict = download_one(cnt.p);
    if (!m) return pairs;
    DBuf<uint32_t> out(2 * m);
    hipLaunchKernelGGL(gather_pairs_kernel, grid1(m), dim3(WG), 0, stream(), d.row_a.p, d.row_b.p, r0, d.idx.p, m, out.p);
    return out.download();
}

void cl_apply(ClusterDev &d, const std::vector<uint32_t> &attach, const std::vector<uint32_t> &sizes) {
    KTimer kt("cluster_refresh");
    const size_t na = attach.size() / 2, ns = sizes.size() / 2, m = std::max(na, ns);
    if (!m) return;
    DBuf<uint32_t> a, s;
    a.upload(attach);
    s.upload(sizes);
    hipLaunchKernelGGL(scatter_kernel, grid1(m), dim3(WG), 0, stream(), a.p, na, s.p, ns, d.new_root.p, d.size_of.p);
    if (na) {
        hipLaunchKernelGGL(refresh_kernel, grid1(d.n_nodes), dim3(WG), 0, stream(), d.root_of.p, d.new_root.p, d.n_nodes);
        hipLaunchKernelGGL(unscatter_kernel, grid1(na), dim3(WG), 0, stream(), a.p, na, d.new_root.p);
    }
    sync();                                  // (a and s leave scope)
}

void cl_group(ClusterDev &d, int threads, std::vector<uint32_t> &nodes, std::vector<uint32_t> &key_cid,
              std::vector<uint32_t> &key_len, uint64_t *k_ge20) {
    KTimer kt("cluster_group");
    const size_t N = d.n_nodes;
    nodes.clear();
    key_cid.clear();
    key_len.clear();
    *k_ge20 = 0;
    if (!N) return;
    DBuf<uint32_t> keep(N), rank(N);
    hipLaunchKernelGGL(keep_kernel, grid1(N), dim3(WG), 0, stream(), d.root_of.p, d.size_of.p, N, keep.p);
    exclusive_scan_u32(keep.p, rank.p, N);
    const uint64_t K = (uint64_t)download_one(rank.p + N - 1) + download_one(keep.p + N - 1);
    *k_ge20 = K;
    const uint64_t dictsize = K / (uint64_t)threads;                  // int(len / threads)
    const uint64_t limit = (uint64_t)std::min(threads, 60) * dictsize;
    if (!limit) return;
    DBuf<uint8_t> flag(N);
    hipLaunchKernelGGL(slice_kernel, grid1(N), dim3(WG), 0, stream(), keep.p, rank.p, N, limit, flag.p);
    DBuf<uint32_t> idx(N);
    const size_t M = select_flagged_indices(flag.p, idx.p, N);
    DBuf<uint64_t> key(M);
    hipLaunchKernelGGL(cid_key_kernel, grid1(M), dim3(WG), 0, stream(), idx.p, M, d.root_of.p, key.p);
    sort_keys_u64(key.p, M, 0, 32 + bits_for(N));
    DBuf<uint32_t> heads(M);
    const size_t C = select_run_heads_u64(key.p, M, 32, heads.p);
    DBuf<uint64_t> ckey(C);
    DBuf<uint32_t> cval(C);
    hipLaunchKernelGGL(cluster_key_kernel, grid1(C), dim3(WG), 0, stream(), key.p, heads.p, C, rank.p, dictsize, ckey.p,
                       cval.p);
    sort_pairs_u64_u32(ckey.p, cval.p, C);
    const std::vector<uint64_t> k = key.download();
    const std::vector<uint32_t> h = heads.download(), order = cval.download();
    nodes.reserve(M);
    for (uint32_t c : order) {
        const size_t a = h[c], e = c + 1 < C ? h[c + 1] : M;
        key_cid.push_back((uint32_t)(k[a] >> 32));
        key_len.push_back((uint32_t)(e - a));
        for (size_t i = a; i < e; ++i) nodes.push_back((uint32_t)k[i]);
    }
}

void cl_demux(ClusterDev &d, const std::vector<uint32_t> &node_key, size_t n_keys, std::vector<uint8_t> &out,
              std::vector<uint64_t> &fstart, std::vector<uint64_t> &fend) {
    KTimer kt("cluster_demux");
    const size_t R = d.n_records;
    fstart.assign(2 * n_keys, 0);
    fend.assign(2 * n_keys, 0);
    out.clear();
    if (!R || !n_keys) return;
    DBuf<uint32_t> nk;
    nk.upload(node_key);
    DBuf<uint32_t> file(R), sel(R);
    DBuf<uint8_t> flag(R);
    hipLaunchKernelGGL(rec_file_kernel, grid1(R), dim3(WG), 0, stream(), d.fq.p, d.rec_dm_off.p, d.rec_dm_len.p,
                       d.rec_flags.p, R, d.node_off.p, d.node_len.p, d.tab_hash.p, d.tab_node.p, d.n_nodes, d.seed, nk.p,
                       file.p, flag.p);
    const size_t m = select_flagged_indices(flag.p, sel.p, R);
    if (!m) return;
    DBuf<uint32_t> key(m), len(m);
    hipLaunchKernelGGL(rec_select_kernel, grid1(m), dim3(WG), 0, stream(), file.p, sel.p, m, key.p);
    sort_pairs_u32_u32(key.p, sel.p, m, 0, bits_for(2 * n_keys));   // stable: FASTQ order inside a file
    hipLaunchKernelGGL(rec_len_kernel, grid1(m), dim3(WG), 0, stream(), sel.p, m, d.fq_line.p, d.n_lines, d.fq_bytes, len.p);
    DBuf<uint64_t> at(m);
    exclusive_scan_u32_to_u64(len.p, at.p, m);
    const uint64_t total = download_one(at.p + m - 1) + download_one(len.p + m - 1);
    DBuf<uint8_t> buf(total);
    hipLaunchKernelGGL(rec_gather_kernel, grid1(m * 64), dim3(WG), 0, stream(), d.fq.p, sel.p, d.fq_line.p, at.p, len.p, m,
                       buf.p);
    DBuf<uint64_t> fs(2 * n_keys), fe(2 * n_keys);
    fs.zero();
    fe.zero();
    hipLaunchKernelGGL(file_span_kernel, grid1(m), dim3(WG), 0, stream(), key.p, at.p, len.p, m, fs.p, fe.p);
    out.resize(total);
    if (total) HIP_CHECK(hipMemcpyAsync(out.data(), buf.p, total, hipMemcpyDeviceToHost, stream()));
    sync();
    fstart = fs.download();
    fend = fe.download();
}

}  // namespace hlmi
