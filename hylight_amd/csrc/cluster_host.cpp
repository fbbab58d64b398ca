// cluster_host.cpp - the host half of HyLight's short-read clustering (HyLight.py:215-226, see cluster.hip for the device
// half): bin_pointer's chunk / session layout, its sequential union pass over each session's prefilter survivors, and the
// writers of readnames.txt, HiStrain_max<size>_final_clusters_grouped.json and fq_<size>/<cid>/<cid>.{1,2}.fq.
//
// The reference's forest has no path compression and its union rule reads the depth of both endpoints (pathlen), so the
// forest can grow deep.  Here each node keeps a parent and the depth offset to it ("potential"); find() compresses the
// path and adds the offsets up, which gives the reference's exact depth at O(alpha)-like cost.  A root hung under another
// root gets offset 1: every node of its tree moves one level down, as in the reference.
#include <chrono>
#include <cstdio>
#include <filesystem>
#include <string>
#include <thread>
#include <atomic>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "cluster_internal.h"
#include "paf_io.h"

namespace hlmi {

namespace {
namespace fs = std::filesystem;

constexpr uint64_t CHUNK = 2600000;                 // bin_pointer:30
constexpr uint64_t WINDOW_DEFAULT = 512ull << 20;
constexpr uint64_t WINDOW_MAX = 2ull << 30;         // 32-bit line offsets inside a window
const char *RUN_ID = "HiStrain";                    // HyLight.py:69

std::vector<uint8_t> read_all(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) fail(HLMI_EIO, "cluster: cannot open %s", path);
    std::vector<uint8_t> b;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    b.resize(n > 0 ? (size_t)n : 0);
    const size_t got = b.empty() ? 0 : fread(b.data(), 1, b.size(), f);
    fclose(f);
    if (got != b.size()) fail(HLMI_EIO, "cluster: short read on %s", path);
    return b;
}

struct PafFile {
    int fd = -1;
    uint64_t size = 0;
    explicit PafFile(const char *path) {
        fd = open(path, O_RDONLY);
        if (fd < 0) fail(HLMI_EIO, "cluster: cannot open %s", path);
        struct stat sb;
        fstat(fd, &sb);
        size = (uint64_t)sb.st_size;
    }
    ~PafFile() { if (fd >= 0) close(fd); }
    void read(uint64_t at, size_t n, uint8_t *out) const {
        size_t done = 0;
        while (done < n) {
            const ssize_t r = pread(fd, out + done, n - done, (off_t)(at + done));
            if (r <= 0) fail(HLMI_EIO, "cluster: short read on the PAF");
            done += (size_t)r;
        }
    }
    // bin_pointer:30-41 chunkify: seek CHUNK forward from the previous end, readline, tell
    std::vector<std::pair<uint64_t, uint64_t>> chunks() const {
        std::vector<std::pair<uint64_t, uint64_t>> out;
        std::vector<uint8_t> buf(1 << 16);
        uint64_t pos = 0;
        for (;;) {
            const uint64_t q = pos + CHUNK;
            uint64_t e = q;                           // past the end: tell() reports the seek target
            if (q < size) {
                e = size;                             // no '\n' after q: readline reads to the end
                for (uint64_t at = q; at < size;) {
                    const size_t m = (size_t)std::min<uint64_t>(buf.size(), size - at);
                    read(at, m, buf.data());
                    const void *nl = memchr(buf.data(), '\n', m);
                    if (nl) { e = at + ((const uint8_t *)nl - buf.data()) + 1; break; }
                    at += m;
                }
            }
            out.emplace_back(pos, e);
            if (e > size) break;
            pos = e;
        }
        return out;
    }
};

// the reference forest with potentials (see the file comment)
struct Forest {
    std::vector<uint32_t> par, off, sz;
    std::vector<uint32_t> path;
    explicit Forest(size_t n) : par(n + 1), off(n + 1, 0), sz(n + 1, 1) {
        for (size_t v = 0; v <= n; ++v) par[v] = (uint32_t)v;
    }
    // -> root (= cluster id); *depth = pathlen - 1
    uint32_t find(uint32_t x, uint64_t *depth) {
        path.clear();
        while (par[x] != x) { path.push_back(x); x = par[x]; }
        uint64_t acc = 0;
        for (size_t k = path.size(); k-- > 0;) {
            acc += off[path[k]];
            off[path[k]] = (uint32_t)acc;
            par[path[k]] = x;
        }
        *depth = path.empty() ? 0 : off[path[0]];
        return x;
    }
};

void json_string(std::string &s, const uint8_t *p, size_t n) {     // json.dumps, ensure_ascii (bytes < 0x80 here)
    static const char *hex = "0123456789abcdef";
    s += '"';
    for (size_t i = 0; i < n; ++i) {
        const uint8_t c = p[i];
        switch (c) {
            case '"': s += "\\\""; break;
            case '\\': s += "\\\\"; break;
            case '\n': s += "\\n"; break;
            case '\r': s += "\\r"; break;
            case '\t': s += "\\t"; break;
            case '\b': s += "\\b"; break;
            case '\f': s += "\\f"; break;
            default:
                if (c < 0x20) { s += "\\u00"; s += hex[c >> 4]; s += hex[c & 15]; }
                else s += (char)c;
        }
    }
    s += '"';
}

void write_file(const std::string &path, const uint8_t *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) fail(HLMI_EIO, "cluster: cannot write %s", path.c_str());
    const size_t w = n ? fwrite(p, 1, n, f) : 0;
    if (fclose(f) != 0 || w != n) fail(HLMI_EIO, "cluster: short write on %s", path.c_str());
}
void write_renamed(const std::string &path, const uint8_t *p, size_t n) {
    const std::string tmp = path + ".partial";
    write_file(tmp, p, n);
    if (rename(tmp.c_str(), path.c_str()) != 0) fail(HLMI_EIO, "cluster: cannot rename %s", tmp.c_str());
}
}  // namespace

void cluster_run(const char *paf_path, const char *fastq, const hlmi_cluster_opts &o, const char *out_dir,
                 hlmi_cluster_stats *st) {
    const double t0 = now_ms();
    *st = hlmi_cluster_stats{};
    if (o.threads < 1 || o.threads > 100)
        fail(HLMI_EINVAL, "cluster: threads %d outside 1..100 (bin_pointer's sess %% threads == 100 checkpoint)", o.threads);
    if (o.size < 1) fail(HLMI_EINVAL, "cluster: size %lld < 1", (long long)o.size);
    const int threads = o.threads;
    const int64_t size = o.size;
    const uint64_t window = std::min<uint64_t>(o.window_bytes ? o.window_bytes : WINDOW_DEFAULT, WINDOW_MAX);

    // FASTQ
    double t = now_ms();
    const std::vector<uint8_t> fq = read_all(fastq);
    if (fq.empty()) fail(HLMI_EINVAL, "cluster: empty FASTQ (get_fq_cluster.py reads no line)");
    if (fq[0] == '>') fail(HLMI_EINVAL, "cluster: FASTA input; the short reads must be FASTQ");
    ClusterDev d;
    const std::vector<ClNode> nodes = cl_load_fastq(d, fq.data(), fq.size());
    const size_t N = nodes.size();
    st->names = N;
    st->ms_fastq = now_ms() - t;

    // PAF: chunks -> sessions of `threads` chunks -> windows of whole sessions
    PafFile paf(paf_path);
    if (paf.size) {
        uint8_t c0;
        paf.read(0, 1, &c0);
        if (c0 == '>') fail(HLMI_EINVAL, "cluster: FASTA input in place of the PAF");
    }
    const auto chunks = paf.chunks();
    st->chunks = chunks.size();
    std::vector<std::pair<uint64_t, uint64_t>> sessions;            // byte ranges, clamped to the file
    for (size_t c = 0; c < chunks.size(); c += threads) {
        const size_t last = std::min(chunks.size(), c + threads) - 1;
        sessions.emplace_back(std::min(chunks[c].first, paf.size), std::min(chunks[last].second, paf.size));
    }
    st->sessions = sessions.size();
    Forest F(N);
    std::vector<uint8_t> wbuf;
    std::vector<uint32_t> attach, grown;
    for (size_t s0 = 0; s0 < sessions.size();) {
        size_t s1 = s0 + 1;
        while (s1 < sessions.size() && sessions[s1].second - sessions[s0].first <= window) ++s1;
        const uint64_t w0 = sessions[s0].first, w1 = sessions[s1 - 1].second;
        t = now_ms();
        wbuf.resize(w1 - w0);
        if (w1 > w0) paf.read(w0, w1 - w0, wbuf.data());
        const std::vector<uint32_t> ls = cl_load_window(d, wbuf.data(), wbuf.size());
        st->rows += ls.size();
        ++st->windows;
        st->ms_paf += now_ms() - t;
        for (size_t s = s0; s < s1; ++s) {
            const size_t r0 = std::lower_bound(ls.begin(), ls.end(), (uint32_t)(sessions[s].first - w0)) - ls.begin();
            const size_t r1 = std::lower_bound(ls.begin(), ls.end(), (uint32_t)(sessions[s].second - w0)) - ls.begin();
            t = now_ms();
            uint64_t strict = 0;
            const std::vector<uint32_t> pairs = cl_prefilter(d, r0, r1, size, &strict);
            st->strict_rejects += strict;
            st->survivors += pairs.size() / 2;
            st->ms_prefilter += now_ms() - t;
            // clusteralgorithm (bin_pointer:73-93): file order, live state, '<='; pathlen2 < pathlen1 keeps cluster 1
            t = now_ms();
            attach.clear();
            grown.clear();
            for (size_t i = 0; i < pairs.size(); i += 2) {
                uint64_t d1, d2;
                const uint32_t r1 = F.find(pairs[i], &d1), r2 = F.find(pairs[i + 1], &d2);
                if (r1 == r2 || (int64_t)F.sz[r1] + F.sz[r2] > size) continue;
                ++st->unions;
                const uint32_t up = d2 < d1 ? r1 : r2, down = d2 < d1 ? r2 : r1;
                F.par[down] = up;
                F.off[down] = 1;
                F.sz[up] += F.sz[down];
                attach.push_back(down);
                grown.push_back(up);
            }
            std::vector<uint32_t> att, szs;
            att.reserve(2 * attach.size());
            for (uint32_t x : attach) {
                uint64_t dd;
                att.push_back(x);
                att.push_back(F.find(x, &dd));
            }
            for (uint32_t r : grown)
                if (F.par[r] == r) { szs.push_back(r); szs.push_back(F.sz[r]); }
            st->ms_union += now_ms() - t;
            t = now_ms();
            cl_apply(d, att, szs);
            st->ms_refresh += now_ms() - t;
        }
        s0 = s1;
    }

    // getclusters.py
    t = now_ms();
    for (size_t v = 1; v <= N; ++v)
        if (F.par[v] == v && F.sz[v] >= 20) ++st->clusters_ge20;
    std::vector<uint32_t> kept, key_cid, key_len;
    uint64_t K = 0;
    cl_group(d, threads, kept, key_cid, key_len, &K);
    st->reads_sliced = K - kept.size();
    std::string js = "{";
    std::vector<uint32_t> node_key(N + 1, CL_NONE);
    for (size_t k = 0, at = 0; k < key_cid.size(); ++k) {
        if (k) js += ", ";
        js += '"' + std::to_string(key_cid[k]) + "\": [";
        for (uint32_t i = 0; i < key_len[k]; ++i, ++at) {
            const uint32_t v = kept[at];
            if (i) js += ", ";
            json_string(js, fq.data() + nodes[v - 1].off, nodes[v - 1].key_len);
            node_key[v] = (uint32_t)k;
        }
        js += ']';
    }
    js += '}';
    st->ms_group = now_ms() - t;

    // get_fq_cluster.py
    t = now_ms();
    std::vector<uint8_t> recs;
    std::vector<uint64_t> fstart, fend;
    cl_demux(d, node_key, key_cid.size(), recs, fstart, fend);
    st->ms_demux = now_ms() - t;

    // writers: nothing is written before every input has been accepted; fq_<size>/ appears whole (rename)
    t = now_ms();
    const std::string out = out_dir;
    std::string rn;
    rn.reserve(N * 16);
    for (const ClNode &nd : nodes) {
        rn.append((const char *)fq.data() + nd.off, nd.raw_len);
        rn += '\n';
    }
    write_renamed(out + "/readnames.txt", (const uint8_t *)rn.data(), rn.size());
    write_renamed(out + "/" + RUN_ID + "_max" + std::to_string(size) + "_final_clusters_grouped.json",
                  (const uint8_t *)js.data(), js.size());
    const std::string final_dir = out + "/fq_" + std::to_string(size);
    const std::string part_dir = out + "/.fq_" + std::to_string(size) + ".partial";
    std::error_code ec;
    fs::remove_all(part_dir, ec);
    if (!fs::create_directory(part_dir, ec)) fail(HLMI_EIO, "cluster: cannot create %s", part_dir.c_str());
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto worker = [&] {
        for (size_t k; (k = next++) < key_cid.size();) {
            const std::string c = std::to_string(key_cid[k]);
            const std::string dir = part_dir + "/" + c;
            try {
                fs::create_directory(dir);
                write_file(dir + "/" + c + ".1.fq", recs.data() + fstart[2 * k], fend[2 * k] - fstart[2 * k]);
                write_file(dir + "/" + c + ".2.fq", recs.data() + fstart[2 * k + 1], fend[2 * k + 1] - fstart[2 * k + 1]);
            } catch (...) {
                bad = 1;
            }
        }
    };
    std::vector<std::thread> pool;
    const int nt = std::max(1, std::min<int>(host_threads(), (int)key_cid.size()));
    for (int i = 0; i < nt; ++i) pool.emplace_back(worker);
    for (auto &th : pool) th.join();
    if (bad) fail(HLMI_EIO, "cluster: cannot write the cluster files under %s", part_dir.c_str());
    fs::remove_all(final_dir, ec);
    if (rename(part_dir.c_str(), final_dir.c_str()) != 0) fail(HLMI_EIO, "cluster: cannot rename %s", part_dir.c_str());
    st->files = 2 * key_cid.size();
    st->ms_write = now_ms() - t;
    st->ms_total = now_ms() - t0;
}

}  // namespace hlmi
