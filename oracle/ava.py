"""ORACLE loader (test infrastructure): ctypes access to oracle/liboracle_ava.so, the CPU
restatement of the overlapper spec (oracle/ava_oracle.c).  Never imported by hylight_amd/."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "liboracle_ava.so")


class Opts(C.Structure):
    _fields_ = [("k", C.c_int), ("w", C.c_int), ("hpc", C.c_int), ("min_chain_score", C.c_int),
                ("max_gap", C.c_int), ("bandwidth", C.c_int), ("min_cnt", C.c_int),
                ("min_mid_occ", C.c_int), ("mid_occ_frac", C.c_double),
                ("match", C.c_int), ("mismatch", C.c_int), ("gap_open", C.c_int), ("gap_ext", C.c_int),
                ("ambi", C.c_int), ("min_dp_score", C.c_int), ("end_bonus", C.c_int), ("pair_once", C.c_int),
                ("gap_open2", C.c_int), ("gap_ext2", C.c_int), ("stub_oh", C.c_int), ("zdrop", C.c_int)]


def opts_long():
    """The constants of script/filter_overlap_slr2.py:51 (ava-pb -Hk19 -m100 -g10000)."""
    return Opts(19, 5, 1, 100, 10000, 2000, 3, 10, 2e-4, 2, 4, 4, 2, 1, 80, 0, 1, 24, 1, -1, 400)       # -O4,24 -E2,1 -z400 (preset defaults)


def opts_short():
    """The constants of script/filter_overlap_slr2.py:55 (--sr -k21 -w11 -s60 -m30 -n2 -A4 -B2 --end-bonus=100; from the
    --sr preset: -g200 -r50 -O12 -E2 -f1000)."""
    return Opts(21, 11, 0, 30, 200, 50, 2, 1000, 0.0, 4, 2, 12, 2, 1, 60, 100, 0, 32, 1, -1, 0)     # --sr: -O12,32 -E2,1; extensions stay within 256 rows (max_gap 200): no z-drop


_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "ava_oracle.c")
        if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < os.path.getmtime(src):
            subprocess.check_call(["make", "-C", _HERE, "oracle"], stdout=subprocess.DEVNULL)
        l = C.CDLL(_LIB)
        l.oracle_hash64.restype = C.c_uint64
        l.oracle_hash64.argtypes = [C.c_uint64, C.c_uint64]
        l.oracle_sketch.restype = C.c_int64
        l.oracle_sketch.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
        l.oracle_ava.restype = C.c_int
        l.oracle_ava.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Opts), C.c_char_p]
        l.oracle_last_counts.restype = None
        l.oracle_last_counts.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
        l.oracle_chain_pieces.restype = C.c_long
        l.oracle_chain_pieces.argtypes = [C.c_void_p, C.c_int, C.POINTER(Opts), C.c_void_p, C.c_long]
        l.oracle_align_pieces.restype = C.c_long
        l.oracle_align_pieces.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(Opts),
                                          C.c_char_p, C.c_long]
        _lib = l
    return _lib


def hash64(key, mask):
    return lib().oracle_hash64(key, mask)


def sketch(seq: bytes, rid=0, k=19, w=5, hpc=1):
    """(n,2) uint64 array of minimizers (x = hash<<8|span, y = rid<<32|pos<<1|strand)."""
    cap = max(len(seq), 1)
    out = np.zeros((cap, 2), dtype=np.uint64)
    n = lib().oracle_sketch(seq, len(seq), rid, k, w, hpc, out.ctypes.data, cap)
    return out[:n].copy()


def ava(target_fa, query_fa, out_paf, opts=None):
    o = opts or opts_long()
    rc = lib().oracle_ava(os.fspath(target_fa).encode(), os.fspath(query_fa).encode(), C.byref(o),
                          os.fspath(out_paf).encode())
    if rc != 0:
        raise RuntimeError(f"oracle_ava failed: {rc}")
    return out_paf


def chain_pieces(anchors, opts):
    """The oracle's own chain_group on one (query, target, strand) group: `anchors` is a list of (tpos, qpos, qspan) in chaining
    order.  Returns [(chain start, piece index, [(q, t), ...fixed points])] in the order align_chain closes the pieces; nothing
    is aligned and no sequence is read."""
    a = np.ascontiguousarray(np.asarray(anchors, dtype=np.uint32).reshape(-1, 3))
    n = a.shape[0]
    out = np.zeros(16 * n + 16, dtype=np.int32)
    w = lib().oracle_chain_pieces(a.ctypes.data, n, C.byref(opts), out.ctypes.data, out.size)
    if w < 0:
        raise RuntimeError("oracle_chain_pieces: output buffer too small")
    res, x = [], 0
    while x < w:
        chain, piece, nf = int(out[x]), int(out[x + 1]), int(out[x + 2])
        res.append((chain, piece, [(int(out[x + 3 + 2 * i]), int(out[x + 4 + 2 * i])) for i in range(nf)]))
        x += 3 + 2 * nf
    return res


_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def align_pieces(qseq, tseq, strand, fixed_points, opts):
    """The oracle's own align_block / extend_left / extend_right / close_piece on ONE alignment piece: `qseq` (as in its file) and
    `tseq` are base strings or code arrays, `fixed_points` a list of (q, t) in aligned orientation (on the query's reverse
    complement when strand is 1).  Returns the PAF row as a list of columns (names "q" and "t"), or None when the piece is
    dropped."""
    def codes(s):
        if isinstance(s, str):
            s = s.encode()
        if isinstance(s, (bytes, bytearray)):
            return np.ascontiguousarray(_CODE[np.frombuffer(s, dtype=np.uint8)])
        return np.ascontiguousarray(np.asarray(s, dtype=np.uint8))
    q, t = codes(qseq), codes(tseq)
    fp = np.ascontiguousarray(np.asarray(fixed_points, dtype=np.int32).reshape(-1, 2))
    cap = 4096 + 16 * (q.size + t.size)
    buf = C.create_string_buffer(cap)
    n = lib().oracle_align_pieces(q.ctypes.data, q.size, t.ctypes.data, t.size, int(strand), fp.ctypes.data, fp.shape[0],
                                  C.byref(opts), buf, cap)
    if n < 0:
        raise RuntimeError("oracle_align_pieces: fixed points outside the contract, or the row does not fit")
    return buf.raw[:n].decode().rstrip("\n").split("\t") if n else None


def last_counts():
    """(pieces reported, of them written as stubs) of the last ava() call of this process."""
    a, b = C.c_long(0), C.c_long(0)
    lib().oracle_last_counts(C.byref(a), C.byref(b))
    return a.value, b.value
