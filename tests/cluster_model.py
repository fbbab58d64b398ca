"""Plain-Python restatement of HyLight's short-read clustering (script/HyLight.py:215-226 with cwd = tmp/): the four
reference scripts get_readnames.py, bin_pointer_limited_filechunks_shortpath2.py (bin_pointer below),
getclusters.py and get_fq_cluster.py, on bytes, with the stats counters hlmi_cluster_short reports.

    files, stats = run(paf_bytes, fastq_bytes, size, threads)

`files` maps every relative output path to its bytes, and every output directory (path ending in '/') to None: the tree
the reference leaves behind after its cmd_rm.  Refused inputs raise Refused (the library's HLMI_EINVAL).
"""
from __future__ import annotations

import json
import re

RUN_ID = "HiStrain"                    # HyLight.py:69
CHUNK = 2_600_000                      # bin_pointer:30
SPLITS = 60                            # getclusters.py:11 (po.map over dcl[0] .. dcl[59])
WS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"  # what str.rstrip() strips from an ASCII name (bin_pointer:118)
PAF_BAD = b"\r\x0b\x0c\x1c\x1d\x1e\""  # str.splitlines() separators (getchunkfile) and csv quoting (clusteralgorithm)


class Refused(ValueError):
    pass


def _lines(b):
    """file iteration in text mode: lines with their '\\n' (\\r is refused before)"""
    out, i = [], 0
    while i < len(b):
        j = b.find(b"\n", i)
        j = len(b) if j < 0 else j + 1
        out.append(b[i:j])
        i = j
    return out


def chunkify(n_bytes, paf):
    """bin_pointer:30-41: seek CHUNK forward from the previous end, then read to the end of that line"""
    chunks, pos = [], 0
    while True:
        q = pos + CHUNK
        if q < n_bytes:
            j = paf.find(b"\n", q)
            e = n_bytes if j < 0 else j + 1
        else:
            e = q                       # seek past the end: tell() reports the seek target
        chunks.append((pos, e - pos))
        if e > n_bytes:
            break
        pos = e
    return chunks


def readnames(fq):
    """get_readnames.py: line i % 4 == 0 holding '/1' anywhere -> line[1:-3]"""
    return [line[1:-3] for i, line in enumerate(_lines(fq)) if i % 4 == 0 and b"/1" in line]


def check_fastq(fq):
    if not fq:
        raise Refused("empty FASTQ (get_fq_cluster.py reads no line)")
    if b"\r" in fq:
        raise Refused("FASTQ with CR line ends")
    if any(c >= 0x80 for c in fq):
        raise Refused("FASTQ byte >= 0x80")
    for i, line in enumerate(_lines(fq)):
        if i % 4 == 0 and not line.startswith(b"@"):
            raise Refused("FASTQ header line does not start with '@' (a FASTA input?)")


class Forest:
    """bin_pointer's `clusters` / `clusterlist`: node v (1-based readnames rank) points at its parent, a root keeps its
    cluster id - always its own rank, because a surviving root is never re-pointed.  No path compression (findhead_lim
    leaves its `adapt` list unused), so pathlen is the true depth + 1."""

    def __init__(self, n):
        self.parent = [0] * (n + 1)        # 0: root
        self.size = [1] * (n + 1)          # clusterlist, valid at roots

    def find(self, v):
        """findhead_lim: (root = cluster id, pathlen)"""
        pathlen = 1
        while self.parent[v]:
            v = self.parent[v]
            pathlen += 1
        return v, pathlen


def run(paf, fq, size, threads):
    if threads < 1 or threads > 100:
        raise Refused("threads must be in 1..100 (the sess % threads == 100 checkpoint, bin_pointer:161)")
    if size < 1:
        raise Refused("size must be >= 1")
    check_fastq(fq)
    if paf[:1] == b">" or fq[:1] == b">":
        raise Refused("FASTA input")
    for c in PAF_BAD:
        if c in paf:
            raise Refused("PAF with CR line ends, a str.splitlines() separator or a '\"' (csv quoting)")
    if any(c >= 0x80 for c in paf):
        raise Refused("PAF byte >= 0x80")

    names_raw = readnames(fq)
    node = {}
    for i, nm in enumerate(names_raw, 1):
        key = nm.rstrip(WS)
        if b'"' in key:
            raise Refused("read name with '\"' (csv quoting)")
        if key in node:
            raise Refused("duplicate read name in readnames.txt")
        node[key] = i
    n = len(names_raw)
    st = dict(names=n, rows=0, chunks=0, sessions=0, survivors=0, strict_rejects=0, unions=0, clusters_ge20=0,
              reads_sliced=0, files=0)

    # rows -> node ids (the reference's apply_async worker dies on an unknown name: refused here)
    rows = []
    chunks = chunkify(len(paf), paf)
    for start, ln in chunks:
        ids = []
        for line in paf[start:start + ln].splitlines():
            f = line.rstrip().split(b"\t")
            if len(f) < 12:
                raise Refused("PAF row with fewer than 12 columns")
            a, b = node.get(f[0][:-2]), node.get(f[5][:-2])
            if a is None or b is None:
                raise Refused("PAF endpoint not in readnames")
            ids.append((a, b))
        rows.append(ids)
    st["rows"] = sum(len(r) for r in rows)
    st["chunks"] = len(chunks)

    F = Forest(n)
    for s0 in range(0, len(chunks), threads):          # one multiprocessing.Pool round = one session
        st["sessions"] += 1
        session = [r for c in rows[s0:s0 + threads] for r in c]
        frozen = [(F.find(a)[0], F.find(b)[0]) for a, b in session]
        kept = []
        for (a, b), (ra, rb) in zip(session, frozen):   # getchunkfile: state frozen at session start, strict '<'
            if ra != rb:
                s = F.size[ra] + F.size[rb]
                if s < size:
                    kept.append((a, b))
                elif s == size:
                    st["strict_rejects"] += 1
        st["survivors"] += len(kept)
        # The stale Chunkfile_<run>_<k> of the previous full session (nfiles is reset inside the loop, :132-135, :176-179)
        # are appended to a short last session.  Every such row was seen before: merged (same cluster now) or refused on
        # size (sizes only grow), so re-running it changes nothing - not emulated.
        for a, b in kept:                               # clusteralgorithm, live state, '<='
            r1, p1 = F.find(a)
            r2, p2 = F.find(b)
            if r1 != r2 and F.size[r1] + F.size[r2] <= size:
                st["unions"] += 1
                if p2 < p1:
                    F.parent[r2] = r1
                    F.size[r1] += F.size[r2]
                else:
                    F.parent[r1] = r2
                    F.size[r2] += F.size[r1]

    # getclusters.py
    key_names = [nm.rstrip(WS) for nm in names_raw]
    cid = [F.find(v)[0] for v in range(1, n + 1)]
    st["clusters_ge20"] = sum(1 for v in range(1, n + 1) if not F.parent[v] and F.size[v] >= 20)
    large = [(key_names[v], cid[v]) for v in range(n) if F.size[cid[v]] >= 20]
    K = len(large)
    dictsize = int(K / threads)
    groups = {}
    used = 0
    for i in range(min(threads, SPLITS)):
        part = large[i * dictsize:min((i + 1) * dictsize, K)]
        used += len(part)
        sub = {}
        for c in sorted(set(c for _, c in part)):
            sub[str(c)] = [k for k, v in part if v == c]
        for k, v in sub.items():
            groups.setdefault(k, []).extend(v)
    st["reads_sliced"] = K - used
    grouped = json.dumps({k.decode("latin-1") if isinstance(k, bytes) else k: [x.decode("latin-1") for x in v]
                          for k, v in groups.items()}).encode()

    # get_fq_cluster.py
    folder = "fq_%d/" % size
    files = {"readnames.txt": b"".join(nm + b"\n" for nm in names_raw),
             "%s_max%d_final_clusters_grouped.json" % (RUN_ID, size): grouped, folder: None}
    read2cluster = {r.encode("latin-1"): k for k, v in groups.items() for r in [x.decode("latin-1") for x in v]}
    out = {}
    for k in groups:
        files[folder + k + "/"] = None
        out[k] = [[], []]
    lines = _lines(fq)
    for r in range(0, len(lines), 4):
        flush_at = r + 4 if r + 4 < len(lines) else len(lines) - 1    # the `i and ...` of :31 and :46
        if not flush_at:
            continue
        header = lines[r]
        name = re.split(rb"[@/]", header)[-2]
        if name in read2cluster:
            out[read2cluster[name]][0 if re.search(rb"/1$", header) else 1].append(b"".join(lines[r:r + 4]))
    for k, (m1, m2) in out.items():
        files["%s%s/%s.1.fq" % (folder, k, k)] = b"".join(m1)
        files["%s%s/%s.2.fq" % (folder, k, k)] = b"".join(m2)
    st["files"] = 2 * len(out)
    return files, st


def tree(out_dir):
    """the files and directories under out_dir in run()'s form"""
    import os
    got = {}
    for root, dirs, fs in os.walk(out_dir):
        rel = os.path.relpath(root, out_dir)
        for d in dirs:
            got[os.path.normpath(os.path.join(rel, d)) + "/"] = None
        for f in fs:
            with open(os.path.join(root, f), "rb") as fh:
                got[os.path.normpath(os.path.join(rel, f))] = fh.read()
    return got


def manifest_of(files):
    """{path: [bytes, sha256]} for files, {dir/: None} for directories"""
    import hashlib
    return {k: (None if v is None else [len(v), hashlib.sha256(v).hexdigest()]) for k, v in sorted(files.items())}
