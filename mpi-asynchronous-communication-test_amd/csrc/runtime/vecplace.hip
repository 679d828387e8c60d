// vecplace.hip -- xg_vecplace_*: one GPU's strided placement as ONE copy_kernel_v launch over its row
// list.  Everything the launch reads was decided by libxghost (host/vec_tables.cc: the device rows,
// tile0, the dispatch cuts -- code the CPU suite builds, walks and sanitizes); this file uploads
// rows and tile0 and walks the finished cut table.  No loop here has a trip count that depends on
// anything but the sizes of those finished tables.
#include "rt.h"
#include "../host/vec_tables.h"

struct xg_vecplace {
    xg_ctx *ctx = nullptr;
    xg_regions *reg = nullptr;
    xg_vec_tables *t = nullptr;              // the host tables (libxghost's)
    xgk::DVRow *d_rows = nullptr;            // t->rows
    int *d_tile0 = nullptr;                  // t->tile0
    unsigned long long *d_stamp = nullptr;   // the run's start and end marks
    bool nt = false;                         // non-temporal (vec_launch_nt)
};

extern "C" int xg_vecplace_free(xg_vecplace *v)
{
    if (!v) return XG_OK;
    if (v->d_rows) (void)hipFree(v->d_rows);
    if (v->d_tile0) (void)hipFree(v->d_tile0);
    if (v->d_stamp) (void)hipFree(v->d_stamp);
    xg_vec_tables_free(v->t);
    delete v;
    return XG_OK;
}

static int vecplace_upload(xg_vecplace *v)
{
    const VecTables *t = v->t;
    HIPCHK(hipMalloc(&v->d_stamp, 16));
    if (t->rows.empty()) return XG_OK;
    HIPCHK(hipMalloc(&v->d_rows, sizeof(xgk::DVRow) * t->rows.size()));
    HIPCHK(hipMemcpy(v->d_rows, t->rows.data(), sizeof(xgk::DVRow) * t->rows.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&v->d_tile0, sizeof(int32_t) * t->tile0.size()));
    HIPCHK(hipMemcpy(v->d_tile0, t->tile0.data(), sizeof(int32_t) * t->tile0.size(), hipMemcpyHostToDevice));
    return XG_OK;
}

extern "C" int xg_vecplace_load(xg_ctx *c, xg_regions *r, const xg_vrow *rows, int64_t n, xg_vecplace **out)
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
    // host only: nothing is allocated or launched for a list the builder refuses
    if (const int rc = xg_vec_tables_build(rows, n, base, r->bytes, c->extent_tile, kExtTilePieces, c->launch_max, &t))
        return rc;
    HIPCHK(hipSetDevice(c->device));
    xg_vecplace *v = new xg_vecplace();
    v->ctx = c; v->reg = r; v->t = t;
    v->nt = vec_launch_nt(c->variant, t->total, foot);
    if (const int rc = vecplace_upload(v)) {
        xg_vecplace_free(v);
        return rc;
    }
    *out = v;
    return XG_OK;
}

extern "C" int64_t xg_vecplace_tiles(const xg_vecplace *v) { return v ? xg_vec_tables_tiles(v->t) : -1; }
extern "C" int xg_vecplace_dispatches(const xg_vecplace *v) { return v ? xg_vec_tables_dispatches(v->t) : -1; }

// A start mark, one dispatch per cut pair (grid = its tiles, base = its first tile), an end mark;
// *device_seconds = end - start.
extern "C" int xg_vecplace_run(xg_vecplace *v, double *device_seconds)
{
    if (!v) return XG_EARG;
    xg_ctx *c = v->ctx;
    const VecTables *t = v->t;
    HIPCHK(hipSetDevice(c->device));
    where("xg_vecplace_run", 0, 1, "posting the dispatches");
    hipLaunchKernelGGL(xgk::clock_kernel, dim3(1), dim3(64), 0, c->stream, v->d_stamp);
    HIPCHK(hipGetLastError());
    const auto k = v->nt ? xgk::copy_kernel_v<true> : xgk::copy_kernel_v<false>;
    const size_t ndisp = t->cuts.size() - 1;
    for (size_t d = 0; d < ndisp; ++d) {
        const int32_t b = t->cuts[d], e = t->cuts[d + 1];
        hipLaunchKernelGGL(k, dim3((unsigned)(e - b)), dim3(xgk::kThreads), 0, c->stream, v->d_rows, v->d_tile0,
                           (int)t->rows.size(), (uint32_t)b, t->tile_bytes, t->tile_pieces,
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
