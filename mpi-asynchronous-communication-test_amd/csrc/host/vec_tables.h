// vec_tables.h -- internal header of the row-launch table builder (vec_tables.cc, libxghost): what one
// copy_kernel_v launch over a GPU's xg_vrow list reads, all of it decided on the host.  Plain C++17,
// no HIP: the runtime (csrc/runtime/vecplace.hip) includes it and uploads rows and tile0; a CPU test
// builds the same tables through the xg_vec_tables_* group of xg_sched.h.  Not part of the public ABI.
// xg_view_tables: the same for a view launch (copy_kernel_vv, xg_view_tables_* of xg_sched.h).
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

// ... and what one copy_kernel_vv launch over the same list reads (xg_view_tables_* of xg_sched.h)
struct xg_view_tables {
    uint64_t base[XG_NBUF] = {};
    int64_t bytes[XG_NBUF] = {};
    int64_t tile_bytes = 0, launch_max = 0;
    int tile_pieces = 0;
    std::vector<int64_t> order;             // device row i is list row order[i] (xg_vrow_views)
    std::vector<xgk::DVRow> rows;           // the rows in view order, absolute pointers
    std::vector<xgk::DView> views;          // one per view
    std::vector<int32_t> kind;              // XG_VIEW_* per view (the dump's; the device never reads it)
    std::vector<int32_t> tile0;             // views + 1: tile0[v] = the tiles of views [0, v)
    std::vector<int32_t> cuts;              // as xg_vec_tables'
    std::vector<int64_t> dbytes;
    int64_t total = 0;
    int64_t multi = 0;                      // views of k > 1
};
typedef xg_view_tables ViewTables;

// Non-temporal or plain, for a launch of `bytes` over regions of `foot` bytes in all: the rule the
// plan tables apply to a placement plan's one launch (plan_tables.cc copy_variant / plan_streams;
// kNtMin, kNtStream and the 256 MiB Infinity Cache).
static inline bool vec_launch_nt(int variant, int64_t bytes, int64_t foot)
{
    if (variant) return variant == 6;
    const bool streaming = (2 * bytes < foot ? 2 * bytes : foot) > ((int64_t)256 << 20);
    return bytes >= ((int64_t)128 << 20) || (streaming && bytes >= ((int64_t)4 << 20));
}
