// plan_load.hip -- xg_plan_load: the tables libxghost builds from a device plan
// (host/plan_tables.cc: pieces, copy launches, engine segments) go to the device, and the
// staging displacements are scanned there.
#include "rt.h"

static uint64_t next_plan_id()
{
    static uint64_t n = 0;
    return __atomic_add_fetch(&n, 1, __ATOMIC_RELAXED);
}

// The solo constants the host builder reads as XG_SOLO_* (xg_sched.h) are the kernels' own.
static_assert(xgk::kSoloWaves == XG_SOLO_WAVES && xgk::kSoloMaxRails == XG_SOLO_MAX_RAILS &&
                  xgk::kSoloPiece == XG_SOLO_PIECE && xgk::kSoloK == XG_SOLO_K &&
                  xgk::kSoloMaxSteps == XG_SOLO_MAX_STEPS && xgk::kSoloMaxPieces == XG_SOLO_MAX_PIECES &&
                  xgk::kSoloOffMax == XG_SOLO_OFF_MAX && xgk::kSoloWideOffMax == XG_SOLO_WIDE_OFF_MAX,
              "solo engine constants: kernels.h and xg_sched.h disagree");

// The staging displacements of the packed segments (DisplScan, plan_tables.h) on the device: one
// scan group per step and direction, then the pack pieces' destinations / unpack pieces' sources
// are patched.  The host's own layout (xg_devplan_build) is the cross-check: a mismatch
// refuses the plan before any copy runs.
static int run_displ_scan(xg_plan *p, DisplScan &ds)
{
    xg_ctx *c = p->ctx;
    p->ndisp = (int)ds.len.size();
    if (!p->ndisp) return XG_OK;
    const int ng = (int)ds.groups.size() - 1;
    DevMem m_len, m_base, m_groups, m_fix;     // freed on every return (the cross-check's included)
    const std::vector<int64_t> base(ng, 0);    // every step's staging starts at 0 (xg_devplan_build)
    HIPCHK(hipMalloc(&p->d_disp, sizeof(int64_t) * p->ndisp));   // the plan's (xg_plan_free)
    HIPCHK(hipMalloc(&m_len.p, sizeof(int64_t) * p->ndisp));
    HIPCHK(hipMalloc(&m_base.p, sizeof(int64_t) * ng));
    HIPCHK(hipMalloc(&m_groups.p, sizeof(int) * (ng + 1)));
    HIPCHK(hipMalloc(&m_fix.p, sizeof(xgk::DFix) * ds.fix.size()));
    int64_t *d_len = m_len.as<int64_t>(), *d_base = m_base.as<int64_t>();
    int *d_groups = m_groups.as<int>();
    xgk::DFix *d_fix = m_fix.as<xgk::DFix>();
    HIPCHK(hipMemcpyAsync(d_len, ds.len.data(), sizeof(int64_t) * p->ndisp, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_base, base.data(), sizeof(int64_t) * ng, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_groups, ds.groups.data(), sizeof(int) * (ng + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_fix, ds.fix.data(), sizeof(xgk::DFix) * ds.fix.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(xgk::displ_scan_kernel, dim3(ng), dim3(xgk::kThreads), 0, c->stream, d_len, d_groups, d_base,
                       p->d_disp);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> got(p->ndisp);
    HIPCHK(hipMemcpyAsync(got.data(), p->d_disp, sizeof(int64_t) * p->ndisp, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < p->ndisp; ++i)
        if (got[i] != ds.host[i]) {
            fprintf(stderr, "xg_plan_load: device displacement %d = %lld, host layout %lld\n", i, (long long)got[i],
                    (long long)ds.host[i]);
            return XG_EARG;
        }
    const int nfix = (int)ds.fix.size();
    hipLaunchKernelGGL(xgk::displ_apply_kernel, dim3((nfix + xgk::kThreads - 1) / xgk::kThreads), dim3(xgk::kThreads),
                       0, c->stream, p->d_pieces, d_fix, nfix, p->d_disp, p->reg->ptr[XG_BUF_STAGE_SEND],
                       p->reg->ptr[XG_BUF_STAGE_RECV]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return XG_OK;
}


// A table of the plan on the device (none for an empty one).
template <class T, class D>
static int upload(const std::vector<T> &v, D **d)
{
    if (v.empty()) return XG_OK;
    HIPCHK(hipMalloc(d, sizeof(T) * v.size()));
    HIPCHK(hipMemcpy(*d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return XG_OK;
}

// Device half of a plan load: the piece, row and tile tables, the fork / join events, the
// displacement scan, the engine tables and the chain stamps.  On an error the caller frees the plan
// (xg_plan_free takes a half-loaded one: every handle starts null).
static int plan_upload(xg_plan *p)
{
    int rc;
    if ((rc = upload(p->pieces, &p->d_pieces)) || (rc = upload(p->rows, &p->d_rows)) ||
        (rc = upload(p->xt_begin, &p->d_xt)))
        return rc;
    p->need_mark.assign(p->nsteps, 1);
    p->fork.assign(p->nsteps, nullptr);
    p->join.assign(p->nsteps, nullptr);
    for (int s = 0; s < p->nsteps; ++s)
        for (int i = p->steps[s].l_b; i < p->steps[s].l_rccl; ++i)
            if (p->launches[i].side) {
                HIPCHK(hipEventCreateWithFlags(&p->fork[s], hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&p->join[s], hipEventDisableTiming));
            }
    HIPCHK(hipMalloc(&p->d_gstamp, 8 * ((size_t)p->nsteps + 1)));
    if ((rc = run_displ_scan(p, p->ds))) return rc;
    if (!p->segs.empty()) {
        if ((rc = upload(p->sb, &p->d_sb)) || (rc = upload(p->ep, &p->d_epieces)) ||
            (rc = upload(p->solo_desc, &p->d_solo)))
            return rc;
        const size_t eb = sizeof(xgk::EngineState) + 8 * (size_t)p->nsteps * p->stamp_rails;
        HIPCHK(hipMalloc(&p->d_engine, eb));
        HIPCHK(hipMemset(p->d_engine, 0, eb));
        if (p->may_arm) {       // xg_plan_run arms it: the doorbell lives in host memory
            HIPCHK(hipHostMalloc((void **)&p->db, sizeof(xgk::Doorbell), hipHostMallocCoherent));
            memset((void *)p->db, 0, sizeof(xgk::Doorbell));
        }
    }
    if (p->any_chain) HIPCHK(hipMalloc(&p->d_cstamp, 8 * (size_t)p->nsteps));
    return XG_OK;
}

extern "C" int xg_plan_load(xg_ctx *c, xg_regions *r, const xg_devplan *dp, xg_plan **out)
{
    if (!c || !r || !dp || !out) return XG_EARG;
    if (dp->ngpus != c->nranks || dp->gpu != c->rank) {
        fprintf(stderr, "xg_plan_load: plan for gpu %d/%d loaded on rank %d/%d\n", dp->gpu, dp->ngpus, c->rank,
                c->nranks);
        return XG_EARG;
    }
    for (int i = 0; i < XG_NBUF; ++i)
        if (dp->region_bytes[i] > r->bytes[i]) {
            fprintf(stderr, "xg_plan_load: region %d too small (%lld < %lld)\n", i, (long long)r->bytes[i],
                    (long long)dp->region_bytes[i]);
            return XG_EARG;
        }
    HIPCHK(hipSetDevice(c->device));
    xg_plan *p = new xg_plan();
    p->ctx = c; p->reg = r; p->id = next_plan_id();
    uint64_t base[XG_NBUF];
    for (int i = 0; i < XG_NBUF; ++i) base[i] = (uint64_t)(uintptr_t)r->ptr[i];
    if (const int rc = plan_tables_build(p, dp, c, base, r->bytes)) {      // host only: nothing is allocated yet
        delete p;
        return rc;
    }
    if (const int rc = plan_upload(p)) {
        xg_plan_free(p);        // frees whatever the upload got to
        return rc;
    }
    *out = p;
    return XG_OK;
}

extern "C" int xg_plan_free(xg_plan *p)
{
    if (!p) return XG_OK;
    // release everything even after an error (a half-loaded plan included); report the first
    hipError_t first = hipSuccess;
    auto keep = [&](hipError_t e) {
        if (e != hipSuccess && first == hipSuccess) first = e;
    };
    keep(hipStreamSynchronize(p->ctx->stream));
    keep(hipStreamSynchronize(p->ctx->side));
    for (void *q : {(void *)p->d_pieces, (void *)p->d_sb, (void *)p->d_epieces, (void *)p->d_engine,
                    (void *)p->d_disp, (void *)p->d_solo, (void *)p->d_cstamp, (void *)p->d_gstamp, (void *)p->d_xt,
                    (void *)p->d_rows})
        if (q) keep(hipFree(q));
    if (p->db) keep(hipHostFree((void *)p->db));
    for (auto &e : p->fork) if (e) keep(hipEventDestroy(e));
    for (auto &e : p->join) if (e) keep(hipEventDestroy(e));
    for (hipGraphExec_t g : {p->g_enq, p->g_run, p->vg.exec})
        if (g) keep(hipGraphExecDestroy(g));
    delete p;
    if (first != hipSuccess) {
        fprintf(stderr, "xg: HIP error %s while freeing a plan\n", hipGetErrorString(first));
        return XG_EHIP;
    }
    return XG_OK;
}

// The plan's introspection is defined once, over the host tables (plan_tables.cc).
extern "C" int xg_plan_nsteps(const xg_plan *p) { return xg_plan_tables_nsteps(p); }
extern "C" int xg_plan_launches(const xg_plan *p) { return xg_plan_tables_launches(p); }
extern "C" int xg_plan_step_form(const xg_plan *p, int s) { return xg_plan_tables_step_form(p, s); }
extern "C" int xg_plan_kind_launches(const xg_plan *p, int kind) { return xg_plan_tables_kind_launches(p, kind); }
extern "C" int xg_plan_wave_launches(const xg_plan *p, int *grid, int *max_pieces_per_wave)
{
    return xg_plan_tables_wave_launches(p, grid, max_pieces_per_wave);
}
extern "C" int xg_plan_small_launches(const xg_plan *p, int *kib) { return xg_plan_tables_small_launches(p, kib); }
extern "C" int xg_plan_shift_launches(const xg_plan *p) { return xg_plan_tables_shift_launches(p); }
extern "C" int xg_plan_extent_launches(const xg_plan *p) { return xg_plan_tables_extent_launches(p); }
extern "C" int xg_plan_engine(const xg_plan *p) { return xg_plan_tables_engine(p); }
extern "C" int xg_plan_engine_rails(const xg_plan *p) { return xg_plan_tables_engine_rails(p); }
extern "C" int xg_plan_engine_steps(const xg_plan *p, int *nseg, int *nhaz)
{
    return xg_plan_tables_engine_steps(p, nseg, nhaz);
}
extern "C" const xg_plan_tables *xg_plan_tables_of(const xg_plan *p) { return p; }

extern "C" int xg_plan_displs(const xg_plan *p, int64_t *out, int n)
{
    if (!out) return p->ndisp;
    if (n < p->ndisp) return XG_EARG;
    if (p->ndisp) HIPCHK(hipMemcpy(out, p->d_disp, sizeof(int64_t) * p->ndisp, hipMemcpyDeviceToHost));
    return XG_OK;
}

