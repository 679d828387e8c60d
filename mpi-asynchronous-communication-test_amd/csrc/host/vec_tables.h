// vec_tables.h -- internal header of the row-launch table builder (vec_tables.cc, libxghost): what one
// copy_kernel_v launch over a GPU's xg_vrow list reads, all of it decided on the host.  Plain C++17,
// no HIP: the runtime (csrc/runtime/vecplace.hip) includes it and uploads rows and tile0; a CPU test
// builds the same tables through the xg_vec_tables_* group of xg_sched.h.  Not part of the public ABI.
#pragma once

#include <stdint.h>

#include <vector>

#include "../dcopy.h"
#include "xg.h"

struct xg_vec_tables {
    uint64_t base[XG_NBUF] = {};            // the regions the rows' pointers lie in
    int64_t bytes[XG_NBUF] = {};
    int64_t tile_bytes = 0, launch_max = 0;
    int tile_pieces = 0;
    std::vector<xgk::DVRow> rows;           // one per xg_vrow, absolute pointers
    std::vector<int32_t> tile0;             // rows + 1: tile0[k] = the tiles of rows [0, k)
    // the launch's dispatches: dispatch k = tiles [cuts[k], cuts[k + 1]) and copies dbytes[k] bytes;
    // a launch without tiles has none (cuts = {0})
    std::vector<int32_t> cuts;
    std::vector<int64_t> dbytes;
    int64_t total = 0;                      // bytes the launch copies
};
typedef xg_vec_tables VecTables;

// Non-temporal or plain, for a launch of `bytes` over regions of `foot` bytes in all: the rule the
// plan tables apply to a placement plan's one launch (plan_tables.cc copy_variant / plan_streams;
// kNtMin, kNtStream and the 256 MiB Infinity Cache).
static inline bool vec_launch_nt(int variant, int64_t bytes, int64_t foot)
{
    if (variant) return variant == 6;
    const bool streaming = (2 * bytes < foot ? 2 * bytes : foot) > ((int64_t)256 << 20);
    return bytes >= ((int64_t)128 << 20) || (streaming && bytes >= ((int64_t)4 << 20));
}
