// vecplace.hip -- xg_vecplace_*: one GPU's strided placement as ONE copy_kernel_v launch over its row
// list, or (xg_vecplace_load_views) ONE copy_kernel_vv launch over the list's views.  Everything the
// launch reads was decided by libxghost (host/vec_tables.cc: the device rows, the views, tile0, the
// dispatch cuts -- code the CPU suite builds, walks and sanitizes); this file uploads rows, views and
// tile0 and walks the finished cut table.  No loop here has a trip count that depends on
// anything but the sizes of those finished tables.
#include "rt.h"
#include "../host/vec_tables.h"

struct xg_vecplace {
    xg_ctx *ctx = nullptr;
    xg_regions *reg = nullptr;
    xg_vec_tables *t = nullptr;              // the host tables (libxghost's) of a row launch ...
    xg_view_tables *vt = nullptr;            // ... or of a view launch: one of the two
    // what either holds, by reference
    const std::vector<xgk::DVRow> *rows = nullptr;
    const std::vector<int32_t> *tile0 = nullptr, *cuts = nullptr;
    int64_t tile_bytes = 0;
    int tile_pieces = 0;
    xgk::DVRow *d_rows = nullptr;            // *rows
    xgk::DView *d_views = nullptr;           // vt->views
    int *d_tile0 = nullptr;                  // *tile0
    unsigned long long *d_stamp = nullptr;   // the run's start and end marks
    bool nt = false;                         // non-temporal (vec_launch_nt)
};

extern "C" int xg_vecplace_free(xg_vecplace *v)
{
    if (!v) return XG_OK;
    if (v->d_rows) (void)hipFree(v->d_rows);
    if (v->d_views) (void)hipFree(v->d_views);
    if (v->d_tile0) (void)hipFree(v->d_tile0);
    if (v->d_stamp) (void)hipFree(v->d_stamp);
    xg_vec_tables_free(v->t);
    xg_view_tables_free(v->vt);
    delete v;
    return XG_OK;
}

static int vecplace_upload(xg_vecplace *v)
{
    HIPCHK(hipMalloc(&v->d_stamp, 16));
    if (v->rows->empty()) return XG_OK;
    HIPCHK(hipMalloc(&v->d_rows, sizeof(xgk::DVRow) * v->rows->size()));
    HIPCHK(hipMemcpy(v->d_rows, v->rows->data(), sizeof(xgk::DVRow) * v->rows->size(), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&v->d_tile0, sizeof(int32_t) * v->tile0->size()));
    HIPCHK(hipMemcpy(v->d_tile0, v->tile0->data(), sizeof(int32_t) * v->tile0->size(), hipMemcpyHostToDevice));
    if (v->vt) {
        HIPCHK(hipMalloc(&v->d_views, sizeof(xgk::DView) * v->vt->views.size()));
        HIPCHK(hipMemcpy(v->d_views, v->vt->views.data(), sizeof(xgk::DView) * v->vt->views.size(), hipMemcpyHostToDevice));
    }
    return XG_OK;
}

// by rows (views == false) or by views: the host builder, then the upload
static int vecplace_load(xg_ctx *c, xg_regions *r, const xg_vrow *rows, int64_t n, bool views, xg_vecplace **out)
{
    if (out) *out = nullptr;
    if (!c || !r || !out || r->ctx != c || n < 0 || n > INT32_MAX || (n > 0 && !rows)) return XG_EARG;
    uint64_t base[XG_NBUF];
    int64_t foot = 0;
    for (int i = 0; i < XG_NBUF; ++i) {
        base[i] = (uint64_t)(uintptr_t)r->ptr[i];
        foot += std::max<int64_t>(0, r->bytes[i]);
    }
    xg_vec_tables *t = nullptr;
    xg_view_tables *vt = nullptr;
    // host only: nothing is allocated or launched for a list the builder refuses
    if (const int rc = views ? xg_view_tables_build(rows, n, base, r->bytes, c->extent_tile, kExtTilePieces, c->launch_max, &vt)
                             : xg_vec_tables_build(rows, n, base, r->bytes, c->extent_tile, kExtTilePieces, c->launch_max, &t))
        return rc;
    xg_vecplace *v = new xg_vecplace();
    v->ctx = c; v->reg = r; v->t = t; v->vt = vt;
    if (vt) { v->rows = &vt->rows; v->tile0 = &vt->tile0; v->cuts = &vt->cuts; }
    else { v->rows = &t->rows; v->tile0 = &t->tile0; v->cuts = &t->cuts; }
    v->tile_bytes = c->extent_tile;
    v->tile_pieces = kExtTilePieces;
    v->nt = vec_launch_nt(c->variant, vt ? vt->total : t->total, foot);
    if (hipSetDevice(c->device) != hipSuccess) {
        xg_vecplace_free(v);
        return XG_EHIP;
    }
    if (const int rc = vecplace_upload(v)) {
        xg_vecplace_free(v);
        return rc;
    }
    *out = v;
    return XG_OK;
}

extern "C" int xg_vecplace_load(xg_ctx *c, xg_regions *r, const xg_vrow *rows, int64_t n, xg_vecplace **out)
{
    return vecplace_load(c, r, rows, n, false, out);
}

extern "C" int xg_vecplace_load_views(xg_ctx *c, xg_regions *r, const xg_vrow *rows, int64_t n, xg_vecplace **out)
{
    return vecplace_load(c, r, rows, n, true, out);
}

extern "C" int64_t xg_vecplace_tiles(const xg_vecplace *v) { return v ? v->tile0->back() : -1; }
extern "C" int xg_vecplace_dispatches(const xg_vecplace *v) { return v ? (int)v->cuts->size() - 1 : -1; }
extern "C" int64_t xg_vecplace_views(const xg_vecplace *v) { return v && v->vt ? v->vt->multi : 0; }

// A start mark, one dispatch per cut pair (grid = its tiles, base = its first tile), an end mark;
// *device_seconds = end - start.
extern "C" int xg_vecplace_run(xg_vecplace *v, double *device_seconds)
{
    if (!v) return XG_EARG;
    xg_ctx *c = v->ctx;
    const std::vector<int32_t> &cuts = *v->cuts;
    HIPCHK(hipSetDevice(c->device));
    where("xg_vecplace_run", 0, 1, "posting the dispatches");
    hipLaunchKernelGGL(xgk::clock_kernel, dim3(1), dim3(64), 0, c->stream, v->d_stamp);
    HIPCHK(hipGetLastError());
    const auto k = v->nt ? xgk::copy_kernel_v<true> : xgk::copy_kernel_v<false>;
    const auto kv = v->nt ? xgk::copy_kernel_vv<true> : xgk::copy_kernel_vv<false>;
    const size_t ndisp = cuts.size() - 1;
    for (size_t d = 0; d < ndisp; ++d) {
        const int32_t b = cuts[d], e = cuts[d + 1];
        if (v->vt)
            hipLaunchKernelGGL(kv, dim3((unsigned)(e - b)), dim3(xgk::kThreads), 0, c->stream, v->d_rows, v->d_views,
                               v->d_tile0, (int)v->vt->views.size(), (uint32_t)b, v->tile_bytes,
                               (unsigned long long *)nullptr);
        else
            hipLaunchKernelGGL(k, dim3((unsigned)(e - b)), dim3(xgk::kThreads), 0, c->stream, v->d_rows, v->d_tile0,
                               (int)v->rows->size(), (uint32_t)b, v->tile_bytes, v->tile_pieces,
                               (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(xgk::clock_kernel, dim3(1), dim3(64), 0, c->stream, v->d_stamp + 1);
    HIPCHK(hipGetLastError());
    where("xg_vecplace_run", 1, 1, "waiting for the device (hipStreamSynchronize)");
    HIPCHK(hipStreamSynchronize(c->stream));
    where("idle", -1, 0, "");
    unsigned long long st[2];
    HIPCHK(hipMemcpy(st, v->d_stamp, sizeof st, hipMemcpyDeviceToHost));
    if (device_seconds) *device_seconds = (double)(st[1] - st[0]) / c->wall_hz;
    return XG_OK;
}
