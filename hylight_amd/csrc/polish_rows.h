// polish_rows.h - the per-op rule that turns a row's CIGAR into the compact CIGAR the polisher's kernels walk (PolDevIn::ops):
// an op of length 0 is no op, neighbouring I ops are one op (one slot's insertion), every other op stays as it is.  The same
// walk counts what include/hylight_mi.h calls ins_edge and ins_long.  polish_host.cpp (rows of a PAF) and polish_rows.hip
// (rows of the overlapper, in HBM) both run it; tests/capi/polish_rows_host_check.cpp checks it with the host compiler alone,
// so this header includes nothing of HIP's.
#pragma once
#include <cstdint>

#include "hd.h"

namespace hlmi {
namespace pol {

constexpr uint32_t ROW_OP_I = 1u;               // OP_I of common.h (polish_rows.hip asserts both)
constexpr uint32_t ROW_INS_CAP = 16u;           // POLISH_INS_CAP of polish_internal.h
constexpr uint32_t ROW_NO_SLOT = 0xffffffffu;

// a finished op of the compact CIGAR: len << 4 | code, and for an I op the slot it belongs to - the target position it sits
// in front of, ROW_NO_SLOT at the row's very start or end (ts < slot < te is the header's rule)
struct RowOp {
    uint32_t word, slot;
};

// The walk over one row.  Ops are written one behind: the last op waits in `pend` until the next one shows that no I joins it.
struct RowWalk {
    uint32_t ts, te;        // the row's target range
    uint32_t p;             // target position in front of the next op
    uint32_t pend;          // the op that waits (0: none)
    uint32_t n_out;         // ops finished so far
    uint32_t ins_edge;      // I ops of the ORIGINAL CIGAR (length > 0) at p == ts or p == te
    uint32_t ins_long;      // finished I ops inside (ts, te) of more than ROW_INS_CAP bases
};

HLMI_HD void row_walk_begin(RowWalk &w, uint32_t ts, uint32_t te) {
    w.ts = ts; w.te = te; w.p = ts;
    w.pend = 0; w.n_out = 0; w.ins_edge = 0; w.ins_long = 0;
}

// the waiting op leaves: true when there was one (then *out holds it and it is op number n_out - 1)
HLMI_HD bool row_walk_flush(RowWalk &w, RowOp *out) {
    if (!w.pend) return false;
    out->word = w.pend;
    out->slot = ROW_NO_SLOT;
    if ((w.pend & 15u) == ROW_OP_I && w.p != w.ts && w.p != w.te) {
        out->slot = w.p;
        if ((w.pend >> 4) > ROW_INS_CAP) ++w.ins_long;
    }
    w.pend = 0;
    ++w.n_out;
    return true;
}

// the next op of the row's CIGAR; true when an op was finished by it (*out, op number n_out - 1)
HLMI_HD bool row_walk_op(RowWalk &w, uint32_t word, RowOp *out) {
    const uint32_t len = word >> 4;
    if (!len) return false;
    if ((word & 15u) == ROW_OP_I) {
        if (w.p == w.ts || w.p == w.te) ++w.ins_edge;
        if ((w.pend & 15u) == ROW_OP_I && w.pend) {        // the same slot: one op
            w.pend += len << 4;
            return false;
        }
        const bool done = row_walk_flush(w, out);
        w.pend = word;
        return done;
    }
    const bool done = row_walk_flush(w, out);              // (an I that waited sits in front of p as it is now)
    w.p += len;
    w.pend = word;
    return done;
}

// behind the last op
HLMI_HD bool row_walk_end(RowWalk &w, RowOp *out) { return row_walk_flush(w, out); }

}  // namespace pol
}  // namespace hlmi
