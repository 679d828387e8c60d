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

// One row of a strided placement (copy_kernel_v; built by host/vec_tables.cc from an xg_vrow):
// `count` blocks of `len` bytes, block j from src + j * src_step to dst + j * dst_step.  The
// kernel derives every block from these six numbers (xg_vec_piece_at): no descriptor per block.
struct DVRow {
    const uint8_t *src;
    uint8_t *dst;
    int64_t src_step, dst_step;
    int64_t len, count;
};

// One view of a strided placement (copy_kernel_vv; built by host/vec_tables.cc from xg_vrow_views):
// device rows [row0, row0 + k), equal in len, count and steps, their offsets len apart on one side;
// a tile takes jb blocks of each of them (xg_view_piece_at).
struct DView {
    int32_t row0, k, jb, pad;
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
