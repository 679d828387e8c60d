/*
 * exchange_w.c -- the placed exchanges (xg.h): xg_exchange_v with the aggregator side placed by an
 * offset-length list (xg_exchange_w) or by strided runs (xg_exchange_wv).  The exchange itself is
 * xg_exchange_v, unchanged, over a dense intermediate the library owns; one extra GPU-local placement
 * scatters that intermediate into the caller's domain buffer after the exchange (a2m, the collective
 * write) or gathers it out of the domain buffer before the exchange (m2a, the collective read).
 *   xg_exchange_w   the placement is a plan (xg_place_plan_build: one copy per extent, run on
 *                   copy_kernel_x where its runs are short);
 *   xg_exchange_wv  the placement is ONE launch of copy_kernel_v over this GPU's rows (of
 *                   copy_kernel_vv over their views with XG_VEC_VIEWS=1)
 *                   (xg_vec_rows_build, xg_vecplace_load): no extent list, no plan, no descriptor per
 *                   block is ever built.  A list of few, long blocks (mean above kVecLenMax) goes
 *                   through xg_vecs_expand into xg_exchange_w, as every list did before.
 * Placement posts no RCCL call of its own; what the ranks must agree on (the list, the domain
 * lengths, every rank's set-up, the road) is settled by agree.h's reductions before the exchange's
 * first call.  Both operators share their two ends (front, back); the set-up between them is each
 * one's own.  A translation unit of its own, as exchange.c is.
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"
#include "agree.h"

#define WHAT "setting up or running this placement"

/* one call's arguments, as the operator got them, and what front makes of them */
typedef struct {
    const char *name;       /* the calling operator */
    xg_ctx *ctx; int method, procs, cb_nodes; const int *rank_list; int comm_size; void *send, *recv;
    xg_timer *timers; int iter, ntimes; const xg_run_opts *opts; int64_t *bad_slots, *bad_items; double *place_s;
    char *err; size_t errlen;
    int g, G, scatter;
    xg_run_opts dflt;
    char ebuf[512];
} placed;

/* The front of both operators: the defaults, the out-parameters zeroed, the context.  -> XG_EARG
 * (an early return: no rank of a real job gets past it alone) or XG_OK with g, G, scatter set. */
static int front(placed *p)
{
    if (!p->opts) { xg_run_opts_default(&p->dflt); p->opts = &p->dflt; }
    if (!p->err) { p->err = p->ebuf; p->errlen = sizeof p->ebuf; }
    p->err[0] = 0;
    if (p->bad_slots) *p->bad_slots = 0;
    if (p->bad_items) *p->bad_items = 0;
    if (p->place_s) *p->place_s = 0;
    if (!p->ctx || xg_is_virtual(p->ctx)) {
        snprintf(p->err, p->errlen, "%s needs a real context (a virtual GPU's plans run only together)", p->name);
        return XG_EARG;
    }
    p->g = xg_rank(p->ctx); p->G = xg_nranks(p->ctx);
    p->scatter = xg_method_direction(p->method) == XG_A2M;
    return XG_OK;
}

/* ... and, once the lists agree, what it refuses before the list is looked at: local errors that
 * flow into the first agree_peers -- a return here would leave the peers waiting */
static int refused(const placed *p)
{
    if (xg_method_direction(p->method) < 0) {
        snprintf(p->err, p->errlen, "method %d is not one of 1..20", p->method);
        return XG_EARG;
    }
    if (!p->rank_list) {
        snprintf(p->err, p->errlen, "%s: no aggregator list", p->name);
        return XG_EARG;
    }
    return XG_OK;
}

static int adopt(const placed *p, const int64_t *region_bytes, xg_regions **reg)
{
    const int rc = xg_regions_adopt(p->ctx, region_bytes, p->scatter ? NULL : p->send, p->scatter ? p->recv : NULL, reg);
    if (rc)
        snprintf(p->err, p->errlen, "regions of %lld (dense) + %lld (domain) bytes around the caller's domain buffer %p: "
                 "refused or allocation failed (%d, see stderr)",
                 (long long)region_bytes[p->scatter ? XG_BUF_SEND : XG_BUF_RECV],
                 (long long)region_bytes[p->scatter ? XG_BUF_RECV : XG_BUF_SEND], p->scatter ? p->recv : p->send, rc);
    return rc;
}

/* The back of both operators, from rc = the set-up's outcome as the ranks agreed on it: the exchange
 * and the placement in the direction's order over reg's dense side.  run(u, &seconds) places (and
 * takes first whatever its check needs from before); check(u, &n) counts the `items` that differ
 * from their source. */
static int back(const placed *p, int rc, xg_regions *reg, const int64_t *lens, int (*run)(void *, double *),
                int (*check)(void *, int64_t *), void *u, const char *items)
{
    int64_t nbad = 0;
    double secs = 0;
    if (rc == XG_OK) {
        void *dense = xg_regions_ptr(reg, p->scatter ? XG_BUF_SEND : XG_BUF_RECV);
        if (p->scatter)         /* collective write: exchange into the dense layout, then scatter it */
            rc = xg_exchange_v(p->ctx, p->method, p->procs, p->cb_nodes, lens, p->rank_list, p->comm_size, p->send, dense,
                               p->timers, p->iter, p->ntimes, p->opts, p->bad_slots, p->err, p->errlen);
        if (rc == XG_OK) {      /* else every rank alike: xg_exchange_v agreed on it */
            rc = run(u, &secs);
            if (rc == XG_OK && p->place_s) *p->place_s = secs;
            if (rc == XG_OK && p->opts->verify && (rc = check(u, &nbad)) == XG_OK) {
                if (nbad) fprintf(stderr, "gpu %d: %lld placed %s differ from their source\n", p->g, (long long)nbad, items);
                if (p->bad_items) *p->bad_items = nbad;
            }
            if (rc && p->err[0] == 0) snprintf(p->err, p->errlen, "placement: device error %d (see stderr)", rc);
            /* a failed placement stops every rank here */
            if (p->G > 1) rc = agree_peers(p->ctx, rc, NULL, WHAT, p->err, p->errlen);
            if (rc == XG_OK && !p->scatter)     /* collective read: gathered, now exchange the dense layout */
                rc = xg_exchange_v(p->ctx, p->method, p->procs, p->cb_nodes, lens, p->rank_list, p->comm_size, dense, p->recv,
                                   p->timers, p->iter, p->ntimes, p->opts, p->bad_slots, p->err, p->errlen);
        }
    }
    if (rc && p->err[0] == 0) snprintf(p->err, p->errlen, "device error %d (see stderr)", rc);
    return rc;
}

/* ------------------------------------------------------------------ xg_exchange_w */

/* every rank passed the same list and domain lengths (field by field: the struct has no padding
 * today, but a hash must not depend on that) */
static int exts_agree(xg_ctx *ctx, int procs, int cb_nodes, const xg_ext *exts, int64_t n, const int64_t *dom_bytes,
                      char *err, size_t errlen)
{
    uint64_t h = AGREE_FNV_INIT;
    int64_t i, v[4];
    int rc, differ;
    v[0] = procs; v[1] = cb_nodes; v[2] = n; v[3] = (exts != NULL) | ((dom_bytes != NULL) << 1);
    h = agree_fnv(h, v, sizeof v);
    if (exts)
        for (i = 0; i < n; ++i) {
            v[0] = exts[i].rank; v[1] = exts[i].agg; v[2] = exts[i].off; v[3] = exts[i].len;
            h = agree_fnv(h, v, sizeof v);
        }
    if (dom_bytes && cb_nodes > 0) h = agree_fnv(h, dom_bytes, sizeof(int64_t) * (size_t)cb_nodes);
    if ((rc = agree_digest(ctx, h, &differ)) || !differ) return rc;
    snprintf(err, errlen, "the GPU processes passed different inputs to the placement (extent lists or "
             "domain lengths differ between ranks)");
    return XG_EARG;
}

typedef struct {
    xg_regions *reg;
    xg_devplan *pd;
    xg_plan *plan;
    int verify;
    xg_bufspan *sp;
    uint64_t *c_src, *c_dst;
} ext_place;

/* xg_chk64 of one side of every hosted extent (the placement plan's copies, in list order) */
static int chk_exts(const ext_place *e, int dst_side, uint64_t *chk)
{
    const xg_devplan *pd = e->pd;
    int k;
    for (k = 0; k < pd->ncopy; ++k) {
        e->sp[k].buf = dst_side ? pd->copies[k].dst_buf : pd->copies[k].src_buf; e->sp[k].pad = 0;
        e->sp[k].off = dst_side ? pd->copies[k].dst_off : pd->copies[k].src_off;
        e->sp[k].len = pd->copies[k].len;
    }
    return xg_chk_spans(e->reg, e->sp, pd->ncopy, chk);
}

/* the source's checksums are taken before the plan runs, the destination's after */
static int ext_run(void *u, double *secs)
{
    ext_place *e = (ext_place *)u;
    double done[2] = {0, 0}, post[2] = {0, 0}, wall = 0;
    int rc = e->verify ? chk_exts(e, 0, e->c_src) : XG_OK;
    if (rc == XG_OK) rc = xg_plan_run(e->plan, done, post, &wall);
    *secs = done[0];
    return rc;
}

static int ext_check(void *u, int64_t *nbad)
{
    ext_place *e = (ext_place *)u;
    const int rc = chk_exts(e, 1, e->c_dst);
    int k;
    for (k = 0; rc == XG_OK && k < e->pd->ncopy; ++k) *nbad += e->c_src[k] != e->c_dst[k];
    return rc;
}

int xg_exchange_w(xg_ctx *ctx, int method, int procs, int cb_nodes, const xg_ext *exts, int64_t n,
                  const int64_t *dom_bytes, const int *rank_list, int comm_size, void *send, void *recv,
                  xg_timer *timers, int iter, int ntimes, const xg_run_opts *opts, int64_t *bad_slots,
                  int64_t *bad_exts, double *place_s, char *err, size_t errlen)
{
    placed p = {"xg_exchange_w", ctx, method, procs, cb_nodes, rank_list, comm_size, send, recv, timers, iter, ntimes,
                opts, bad_slots, bad_exts, place_s, err, errlen, 0, 0, 0, {0}, {0}};
    ext_place e = {NULL, NULL, NULL, 0, NULL, NULL, NULL};
    xg_sched *s = NULL;
    int64_t *lens = NULL;
    int rc;
    if ((rc = front(&p))) return rc;
    err = p.err; errlen = p.errlen; opts = p.opts;
    if (p.G > 1 && (rc = exts_agree(ctx, procs, cb_nodes, exts, n, dom_bytes, err, errlen))) return rc;
    /* this rank's set-up: the list, the matrix, the placement plan, the regions around the caller's
     * domain buffer and the library's dense intermediate, the plan upload */
    if ((rc = refused(&p)) == XG_OK) rc = xg_exts_check(exts, n, procs, cb_nodes, dom_bytes, p.scatter, err, errlen);
    if (rc == XG_OK && !(lens = (int64_t *)malloc(sizeof *lens * (size_t)procs * (size_t)cb_nodes + 8))) {
        snprintf(err, errlen, "placement: out of host memory");
        rc = XG_ENOMEM;
    }
    if (rc == XG_OK && (rc = xg_exts_lens(exts, n, procs, cb_nodes, lens)))
        snprintf(err, errlen, "extent list: the lengths of one (rank, aggregator) pair overflow");
    if (rc == XG_OK && !(s = xg_sched_build_v(method, procs, cb_nodes, lens, comm_size, rank_list, ntimes, opts->proc_node,
                                              opts->barrier_type, opts->eager_limit, iter, err, errlen)))
        rc = XG_ESCHED;
    if (rc == XG_OK && !(e.pd = xg_place_plan_build(s, p.G, p.g, exts, n, dom_bytes))) {
        snprintf(err, errlen, "placement plan: out of host memory");
        rc = XG_ENOMEM;
    }
    if (rc == XG_OK) rc = adopt(&p, e.pd->region_bytes, &e.reg);
    if (rc == XG_OK && (rc = xg_plan_load(ctx, e.reg, e.pd, &e.plan)))
        snprintf(err, errlen, "placement plan: not loaded (%d, see stderr)", rc);
    if (rc == XG_OK && opts->verify) {
        e.sp = (xg_bufspan *)malloc(sizeof *e.sp * ((size_t)e.pd->ncopy + 1));
        e.c_src = (uint64_t *)calloc((size_t)e.pd->ncopy + 1, sizeof *e.c_src);
        e.c_dst = (uint64_t *)calloc((size_t)e.pd->ncopy + 1, sizeof *e.c_dst);
        if (!e.sp || !e.c_src || !e.c_dst) {
            snprintf(err, errlen, "placement check: out of host memory");
            rc = XG_ENOMEM;
        }
    }
    e.verify = opts->verify;
    if (p.G > 1) rc = agree_peers(ctx, rc, NULL, WHAT, err, errlen);    /* before the exchange's first call */
    rc = back(&p, rc, e.reg, lens, ext_run, ext_check, &e, "extents");
    free(e.sp); free(e.c_src); free(e.c_dst); free(lens);
    if (e.plan) xg_plan_free(e.plan);
    if (e.reg) xg_regions_free(e.reg);
    xg_devplan_free(e.pd);
    xg_sched_free(s);
    return rc;
}

/* ------------------------------------------------------------------ xg_exchange_wv */

/* Rows of blocks up to this mean length run copy_kernel_v.  It started at the project's threshold for
 * one workgroup per tile against one workgroup per run (kExtMeanMax) and profiles/vec_copy_ab.py's
 * table confirmed it (profiles/r13/vec_copy/summary.txt, DESIGN.md section 4: the row copy wins at
 * L = 64, ties up to 1024 and loses at 4096 by bench.py's CHOICE_RULE); it moves only by that
 * table.  XG_VEC_LEN_MAX overrides it for that A/B alone. */
static const int64_t kVecLenMax = 1024;
/* spans per xg_chk_spans launch of the placement check */
#define VEC_CHK_BATCH 65536

static int64_t g_last_tiles = 0, g_last_views = 0;

int64_t xg_exchange_wv_tiles(void) { return g_last_tiles; }
int64_t xg_exchange_wv_views(void) { return g_last_views; }

/* every rank passed the same list and domain lengths (every vec field by field: a hash must not
 * depend on the struct's padding) */
static int vecs_agree(xg_ctx *ctx, int procs, int cb_nodes, const xg_vec *v, int64_t n, const int64_t *dom_bytes,
                      char *err, size_t errlen)
{
    uint64_t h = AGREE_FNV_INIT;
    int64_t i, f[6];
    int rc, differ;
    f[0] = procs; f[1] = cb_nodes; f[2] = n; f[3] = (v != NULL) | ((dom_bytes != NULL) << 1); f[4] = f[5] = 0;
    h = agree_fnv(h, f, sizeof f);
    if (v)
        for (i = 0; i < n; ++i) {
            f[0] = v[i].rank; f[1] = v[i].agg; f[2] = v[i].off; f[3] = v[i].len; f[4] = v[i].stride; f[5] = v[i].count;
            h = agree_fnv(h, f, sizeof f);
        }
    if (dom_bytes && cb_nodes > 0) h = agree_fnv(h, dom_bytes, sizeof(int64_t) * (size_t)cb_nodes);
    if ((rc = agree_digest(ctx, h, &differ)) || !differ) return rc;
    snprintf(err, errlen, "the GPU processes passed different inputs to the placement (vec lists or "
             "domain lengths differ between ranks)");
    return XG_EARG;
}

typedef struct {
    xg_regions *reg;
    xg_vecplace *vp;
    xg_vrow *rows;
    int64_t nrows;
} vec_place;

/* The placement check: every block of every row on both sides, VEC_CHK_BATCH spans a launch; bad[k]
 * = 1 for a row with a differing block.  sp: VEC_CHK_BATCH spans, row_of: as many row indices,
 * cs / cd: as many checksums. */
static int chk_batch(xg_regions *reg, const xg_vrow *rows, xg_bufspan *sp, const int64_t *row_of, const int64_t *blk_of,
                     int m, uint64_t *cs, uint64_t *cd, char *bad)
{
    int i, rc;
    for (i = 0; i < m; ++i) {
        const xg_vrow *r = &rows[row_of[i]];
        sp[i].buf = r->src_buf; sp[i].pad = 0; sp[i].off = r->src_off + blk_of[i] * r->src_step; sp[i].len = r->len;
    }
    if ((rc = xg_chk_spans(reg, sp, m, cs))) return rc;
    for (i = 0; i < m; ++i) {
        const xg_vrow *r = &rows[row_of[i]];
        sp[i].buf = r->dst_buf; sp[i].off = r->dst_off + blk_of[i] * r->dst_step;
    }
    if ((rc = xg_chk_spans(reg, sp, m, cd))) return rc;
    for (i = 0; i < m; ++i)
        if (cs[i] != cd[i]) bad[row_of[i]] = 1;
    return XG_OK;
}

/* both sides after the placement */
static int chk_rows(void *u, int64_t *nbad)
{
    const vec_place *w = (const vec_place *)u;
    const xg_vrow *rows = w->rows;
    const int64_t nrows = w->nrows;
    xg_bufspan *sp = (xg_bufspan *)malloc(sizeof *sp * VEC_CHK_BATCH);
    int64_t *row_of = (int64_t *)malloc(sizeof *row_of * VEC_CHK_BATCH * 2), *blk_of = row_of ? row_of + VEC_CHK_BATCH : NULL;
    uint64_t *cs = (uint64_t *)malloc(sizeof *cs * VEC_CHK_BATCH * 2), *cd = cs ? cs + VEC_CHK_BATCH : NULL;
    char *bad = (char *)calloc((size_t)nrows + 1, 1);
    int64_t k, j;
    int m = 0, rc = XG_OK;
    *nbad = 0;
    if (!sp || !row_of || !cs || !bad) rc = XG_ENOMEM;
    for (k = 0; k < nrows && rc == XG_OK; ++k)
        for (j = 0; j < rows[k].count && rc == XG_OK; ++j) {
            row_of[m] = k; blk_of[m] = j;
            if (++m == VEC_CHK_BATCH) {
                rc = chk_batch(w->reg, rows, sp, row_of, blk_of, m, cs, cd, bad);
                m = 0;
            }
        }
    if (rc == XG_OK && m) rc = chk_batch(w->reg, rows, sp, row_of, blk_of, m, cs, cd, bad);
    for (k = 0; k < nrows && rc == XG_OK; ++k) *nbad += bad[k];
    free(sp); free(row_of); free(cs); free(bad);
    return rc;
}

static int vec_run(void *u, double *secs) { return xg_vecplace_run(((vec_place *)u)->vp, secs); }

/* the list by its expansion through xg_exchange_w: the road every list took before copy_kernel_v */
static int by_expansion(const placed *p, const xg_vec *v, int64_t n, const int64_t *dom_bytes)
{
    const int64_t m = xg_vecs_expand(v, n, NULL, 0);
    xg_ext *exts;
    int rc;
    if (m < 0) {
        snprintf(p->err, p->errlen, "vec list: a negative len, count or stride, or an offset overflow");
        return XG_EARG;
    }
    /* out of memory: the NULL list goes on, so that xg_exchange_w's own agreement fails every rank alike */
    if ((exts = (xg_ext *)malloc(sizeof *exts * ((size_t)m + 1)))) xg_vecs_expand(v, n, exts, m);
    rc = xg_exchange_w(p->ctx, p->method, p->procs, p->cb_nodes, exts, m, dom_bytes, p->rank_list, p->comm_size, p->send,
                       p->recv, p->timers, p->iter, p->ntimes, p->opts, p->bad_slots, p->bad_items, p->place_s, p->err,
                       p->errlen);
    free(exts);
    return rc;
}

int xg_exchange_wv(xg_ctx *ctx, int method, int procs, int cb_nodes, const xg_vec *v, int64_t n,
                   const int64_t *dom_bytes, const int *rank_list, int comm_size, void *send, void *recv,
                   xg_timer *timers, int iter, int ntimes, const xg_run_opts *opts, int64_t *bad_slots,
                   int64_t *bad_vecs, double *place_s, char *err, size_t errlen)
{
    placed p = {"xg_exchange_wv", ctx, method, procs, cb_nodes, rank_list, comm_size, send, recv, timers, iter, ntimes,
                opts, bad_slots, bad_vecs, place_s, err, errlen, 0, 0, 0, {0}, {0}};
    vec_place w = {NULL, NULL, NULL, 0};
    xg_sched *s = NULL;
    int64_t *lens = NULL, k, region_bytes[XG_NBUF];
    int64_t len_max = kVecLenMax;
    const char *env;
    int rc, expand = 0, views = 0;
    g_last_tiles = g_last_views = 0;
    if ((rc = front(&p))) return rc;
    err = p.err; errlen = p.errlen; opts = p.opts;
    if (p.G > 1 && (rc = vecs_agree(ctx, procs, cb_nodes, v, n, dom_bytes, err, errlen))) return rc;
    /* this rank's set-up: the list, the matrix, the schedule, the rows, the regions around the
     * caller's domain buffer and the library's dense intermediate */
    if ((rc = refused(&p)) == XG_OK) rc = xg_vecs_check(v, n, procs, cb_nodes, dom_bytes, p.scatter, err, errlen);
    if (rc == XG_OK && !(lens = (int64_t *)calloc((size_t)procs * (size_t)cb_nodes + 1, sizeof *lens))) {
        snprintf(err, errlen, "placement: out of host memory");
        rc = XG_ENOMEM;
    }
    if (rc == XG_OK && (rc = xg_vecs_lens(v, n, procs, cb_nodes, lens)))
        snprintf(err, errlen, "vec list: the lengths of one (rank, aggregator) pair overflow");
    if (rc == XG_OK && !(s = xg_sched_build_v(method, procs, cb_nodes, lens, comm_size, rank_list, ntimes, opts->proc_node,
                                              opts->barrier_type, opts->eager_limit, iter, err, errlen)))
        rc = XG_ESCHED;
    if (rc == XG_OK) {
        w.nrows = xg_vec_rows_build(s, p.G, p.g, v, n, dom_bytes, NULL, NULL, region_bytes);
        if (w.nrows < 0 || !(w.rows = (xg_vrow *)malloc(sizeof *w.rows * ((size_t)w.nrows + 1))) ||
            xg_vec_rows_build(s, p.G, p.g, v, n, dom_bytes, w.rows, NULL, NULL) != w.nrows) {
            snprintf(err, errlen, "placement rows: out of host memory");
            rc = XG_ENOMEM;
        }
    }
    if (rc == XG_OK) {      /* the road: few, long blocks go as the extents they are */
        int64_t blocks = 0, bytes = 0;
        if ((env = getenv("XG_VEC_LEN_MAX")) && atoll(env) > 0) len_max = atoll(env);
        for (k = 0; k < w.nrows; ++k) {
            blocks += w.rows[k].count;
            bytes += w.rows[k].len * w.rows[k].count;
        }
        expand = blocks > 0 && bytes / blocks >= len_max && bytes > len_max * blocks;     /* mean > len_max */
        if ((env = getenv("XG_VEC_COPY")) && atoi(env) == 0) expand = 1;
    }
    /* ... which every rank takes when any would (the two roads post different RCCL calls, so no rank
     * may choose alone): the flag rides on the set-up's agreement */
    if (p.G > 1) rc = agree_peers(ctx, rc, &expand, "setting up this placement", err, errlen);
    if (rc == XG_OK && expand) {
        free(w.rows); free(lens);
        xg_sched_free(s);
        return by_expansion(&p, v, n, dom_bytes);
    }
    if (rc == XG_OK) rc = adopt(&p, region_bytes, &w.reg);
    /* XG_VEC_VIEWS=1: a tile per view (copy_kernel_vv).  The placement posts no RCCL call, so this
     * rank decides alone.  Off by default; it moves only by profiles/vec_views_ab.py's table */
    if ((env = getenv("XG_VEC_VIEWS")) && atoi(env) != 0) views = 1;
    if (rc == XG_OK && (rc = views ? xg_vecplace_load_views(ctx, w.reg, w.rows, w.nrows, &w.vp)
                                   : xg_vecplace_load(ctx, w.reg, w.rows, w.nrows, &w.vp)))
        snprintf(err, errlen, "placement rows: not loaded (%d, see stderr)", rc);
    if (p.G > 1) rc = agree_peers(ctx, rc, NULL, WHAT, err, errlen);    /* before the exchange's first call */
    if (rc == XG_OK) {
        g_last_tiles = xg_vecplace_tiles(w.vp);
        g_last_views = xg_vecplace_views(w.vp);
    }
    rc = back(&p, rc, w.reg, lens, vec_run, chk_rows, &w, "vecs");
    free(w.rows); free(lens);
    if (w.vp) xg_vecplace_free(w.vp);
    if (w.reg) xg_regions_free(w.reg);
    xg_sched_free(s);
    return rc;
}
