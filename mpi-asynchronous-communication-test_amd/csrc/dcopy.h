// dcopy.h -- the table records the host builds and the kernels read: one definition for both
// (kernels.h and host/plan_tables.h include it).  No HIP here.
#pragma once
#include <stdint.h>

namespace xgk {

constexpr int kThreads = 256;

struct DCopy {          // one workgroup's piece of a transfer (absolute device pointers)
    const uint8_t *src;
    uint8_t *dst;
    int64_t len;
};

// Piece table fix-up after the scan: piece k of a packed copy c moves
// [o, o + len) of it; its staging side (dst of a pack, src of an unpack) is
// staging base + disp[c] + o.
struct DFix {
    int piece;          // index into the plan's piece table
    int copy;           // index into disp[]
    int64_t off;        // byte offset of the piece inside its copy
    int side;           // 0: patch dst (pack), 1: patch src (unpack)
    int pad;
};

}  // namespace xgk
