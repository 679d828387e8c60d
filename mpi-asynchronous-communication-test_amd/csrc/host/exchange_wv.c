/*
 * exchange_wv.c -- xg_exchange_wv (xg.h): xg_exchange_w with the aggregator side described by strided
 * runs (xg_vec, xg_sched.h).  The exchange itself is xg_exchange_v, unchanged, over a dense
 * intermediate the library owns; the placement is ONE launch of copy_kernel_v over this GPU's rows
 * (xg_vec_rows_build, xg_vecplace_load): no extent list, no plan, no descriptor per block is ever
 * built.  A list of few, long blocks (mean above kVecLenMax) goes through xg_vecs_expand into
 * xg_exchange_w, as every list did before.  A translation unit of its own, as exchange_w.c is.
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"

/* Rows of blocks up to this mean length run copy_kernel_v.  It started at the project's threshold for
 * one workgroup per tile against one workgroup per run (kExtMeanMax) and profiles/vec_copy_ab.py's
 * table confirmed it (profiles/r13/vec_copy/summary.txt, DESIGN.md section 4: the row copy wins at
 * L = 64, ties up to 1024 and loses at 4096 by bench.py's CHOICE_RULE); it moves only by that
 * table.  XG_VEC_LEN_MAX overrides it for that A/B alone. */
static const int64_t kVecLenMax = 1024;
/* spans per xg_chk_spans launch of the placement check */
#define VEC_CHK_BATCH 65536

static int64_t g_last_tiles = 0;

int64_t xg_exchange_wv_tiles(void) { return g_last_tiles; }

/* exchange.c: peers_agree */
static int peers_agree(xg_ctx *ctx, int local_rc, char *err, size_t errlen)
{
    double red[2];
    int rc;
    red[0] = local_rc ? 1.0 : 0.0;
    red[1] = (double)local_rc;
    if ((rc = xg_allreduce_max(ctx, red, 2))) return local_rc ? local_rc : rc;
    if (red[0] == 0.0) return XG_OK;
    if (local_rc) return local_rc;
    snprintf(err, errlen, "another GPU of the job failed (code %d) setting up or running this placement", (int)red[1]);
    return (int)red[1];
}

/* peers_agree, and with it which road the placement takes: *expand becomes 1 on every rank when any
 * rank's is (one all-reduce; the two roads post different RCCL calls, so no rank may choose alone) */
static int peers_route(xg_ctx *ctx, int local_rc, int *expand, char *err, size_t errlen)
{
    double red[3];
    int rc;
    red[0] = local_rc ? 1.0 : 0.0;
    red[1] = (double)local_rc;
    red[2] = *expand ? 1.0 : 0.0;
    if ((rc = xg_allreduce_max(ctx, red, 3))) return local_rc ? local_rc : rc;
    *expand = red[2] != 0.0;
    if (red[0] == 0.0) return XG_OK;
    if (local_rc) return local_rc;
    snprintf(err, errlen, "another GPU of the job failed (code %d) setting up this placement", (int)red[1]);
    return (int)red[1];
}

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t i;
    for (i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

/* every rank passed the same list and domain lengths (every vec field by field: a hash must not
 * depend on the struct's padding) */
static int lists_agree(xg_ctx *ctx, int procs, int cb_nodes, const xg_vec *v, int64_t n, const int64_t *dom_bytes,
                       char *err, size_t errlen)
{
    double red[8];
    uint64_t h = 0xcbf29ce484222325ull;
    int64_t i, f[6];
    int rc, j;
    f[0] = procs; f[1] = cb_nodes; f[2] = n; f[3] = (v != NULL) | ((dom_bytes != NULL) << 1); f[4] = f[5] = 0;
    h = fnv(h, f, sizeof f);
    if (v)
        for (i = 0; i < n; ++i) {
            f[0] = v[i].rank; f[1] = v[i].agg; f[2] = v[i].off; f[3] = v[i].len; f[4] = v[i].stride; f[5] = v[i].count;
            h = fnv(h, f, sizeof f);
        }
    if (dom_bytes && cb_nodes > 0) h = fnv(h, dom_bytes, sizeof(int64_t) * (size_t)cb_nodes);
    for (j = 0; j < 4; ++j) {
        red[j] = (double)((h >> (16 * j)) & 0xffff);
        red[4 + j] = -red[j];
    }
    if ((rc = xg_allreduce_max(ctx, red, 8))) return rc;
    for (j = 0; j < 4; ++j)
        if (red[j] != -red[4 + j]) {
            snprintf(err, errlen, "the GPU processes passed different inputs to the placement (vec lists or "
                     "domain lengths differ between ranks)");
            return XG_EARG;
        }
    return XG_OK;
}

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

static int chk_rows(xg_regions *reg, const xg_vrow *rows, int64_t nrows, int64_t *nbad)
{
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
                rc = chk_batch(reg, rows, sp, row_of, blk_of, m, cs, cd, bad);
                m = 0;
            }
        }
    if (rc == XG_OK && m) rc = chk_batch(reg, rows, sp, row_of, blk_of, m, cs, cd, bad);
    for (k = 0; k < nrows && rc == XG_OK; ++k) *nbad += bad[k];
    free(sp); free(row_of); free(cs); free(bad);
    return rc;
}

/* the list by its expansion through xg_exchange_w: the road every list took before copy_kernel_v */
static int by_expansion(xg_ctx *ctx, int method, int procs, int cb_nodes, const xg_vec *v, int64_t n,
                        const int64_t *dom_bytes, const int *rank_list, int comm_size, void *send, void *recv,
                        xg_timer *timers, int iter, int ntimes, const xg_run_opts *opts, int64_t *bad_slots,
                        int64_t *bad_vecs, double *place_s, char *err, size_t errlen)
{
    const int64_t m = xg_vecs_expand(v, n, NULL, 0);
    xg_ext *exts;
    int rc;
    if (m < 0) {
        snprintf(err, errlen, "vec list: a negative len, count or stride, or an offset overflow");
        return XG_EARG;
    }
    /* out of memory: the NULL list goes on, so that xg_exchange_w's own agreement fails every rank alike */
    if ((exts = (xg_ext *)malloc(sizeof *exts * ((size_t)m + 1)))) xg_vecs_expand(v, n, exts, m);
    rc = xg_exchange_w(ctx, method, procs, cb_nodes, exts, m, dom_bytes, rank_list, comm_size, send, recv, timers, iter,
                       ntimes, opts, bad_slots, bad_vecs, place_s, err, errlen);
    free(exts);
    return rc;
}

int xg_exchange_wv(xg_ctx *ctx, int method, int procs, int cb_nodes, const xg_vec *v, int64_t n,
                   const int64_t *dom_bytes, const int *rank_list, int comm_size, void *send, void *recv,
                   xg_timer *timers, int iter, int ntimes, const xg_run_opts *opts, int64_t *bad_slots,
                   int64_t *bad_vecs, double *place_s, char *err, size_t errlen)
{
    xg_run_opts dflt;
    char ebuf[512];
    xg_sched *s = NULL;
    xg_regions *reg = NULL;
    xg_vecplace *vp = NULL;
    xg_vrow *rows = NULL;
    int64_t *lens = NULL, nrows = 0, nbad = 0, k, region_bytes[XG_NBUF];
    int64_t len_max = kVecLenMax;
    double secs = 0;
    void *dense = NULL;
    const char *env;
    int g, G, rc = XG_OK, dir, scatter, expand = 0;
    if (!opts) { xg_run_opts_default(&dflt); opts = &dflt; }
    if (!err) { err = ebuf; errlen = sizeof ebuf; }
    err[0] = 0;
    if (bad_slots) *bad_slots = 0;
    if (bad_vecs) *bad_vecs = 0;
    if (place_s) *place_s = 0;
    g_last_tiles = 0;
    if (!ctx || xg_is_virtual(ctx)) {
        snprintf(err, errlen, "xg_exchange_wv needs a real context (a virtual GPU's plans run only together)");
        return XG_EARG;
    }
    g = xg_rank(ctx); G = xg_nranks(ctx);
    dir = xg_method_direction(method);
    scatter = dir == XG_A2M;
    if (G > 1 && (rc = lists_agree(ctx, procs, cb_nodes, v, n, dom_bytes, err, errlen))) return rc;
    /* this rank's set-up: the list, the matrix, the schedule, the rows, the regions around the
     * caller's domain buffer and the library's dense intermediate */
    if (dir < 0) {
        snprintf(err, errlen, "method %d is not one of 1..20", method);
        rc = XG_EARG;
    } else if (!rank_list) {
        snprintf(err, errlen, "xg_exchange_wv: no aggregator list");
        rc = XG_EARG;
    } else {
        rc = xg_vecs_check(v, n, procs, cb_nodes, dom_bytes, scatter, err, errlen);
    }
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
        nrows = xg_vec_rows_build(s, G, g, v, n, dom_bytes, NULL, NULL, region_bytes);
        if (nrows < 0 || !(rows = (xg_vrow *)malloc(sizeof *rows * ((size_t)nrows + 1))) ||
            xg_vec_rows_build(s, G, g, v, n, dom_bytes, rows, NULL, NULL) != nrows) {
            snprintf(err, errlen, "placement rows: out of host memory");
            rc = XG_ENOMEM;
        }
    }
    if (rc == XG_OK) {      /* the road: few, long blocks go as the extents they are */
        int64_t blocks = 0, bytes = 0;
        if ((env = getenv("XG_VEC_LEN_MAX")) && atoll(env) > 0) len_max = atoll(env);
        for (k = 0; k < nrows; ++k) {
            blocks += rows[k].count;
            bytes += rows[k].len * rows[k].count;
        }
        expand = blocks > 0 && bytes / blocks >= len_max && bytes > len_max * blocks;     /* mean > len_max */
        if ((env = getenv("XG_VEC_COPY")) && atoi(env) == 0) expand = 1;
    }
    if (G > 1) rc = peers_route(ctx, rc, &expand, err, errlen);
    if (rc == XG_OK && expand) {
        free(rows); free(lens);
        xg_sched_free(s);
        return by_expansion(ctx, method, procs, cb_nodes, v, n, dom_bytes, rank_list, comm_size, send, recv, timers, iter,
                            ntimes, opts, bad_slots, bad_vecs, place_s, err, errlen);
    }
    if (rc == XG_OK && (rc = xg_regions_adopt(ctx, region_bytes, scatter ? NULL : send, scatter ? recv : NULL, &reg)))
        snprintf(err, errlen, "regions of %lld (dense) + %lld (domain) bytes around the caller's domain buffer %p: "
                 "refused or allocation failed (%d, see stderr)",
                 (long long)region_bytes[scatter ? XG_BUF_SEND : XG_BUF_RECV],
                 (long long)region_bytes[scatter ? XG_BUF_RECV : XG_BUF_SEND], scatter ? recv : send, rc);
    if (rc == XG_OK && (rc = xg_vecplace_load(ctx, reg, rows, nrows, &vp)))
        snprintf(err, errlen, "placement rows: not loaded (%d, see stderr)", rc);
    if (G > 1) rc = peers_agree(ctx, rc, err, errlen);      /* before the exchange's first call */
    if (rc) goto out;
    g_last_tiles = xg_vecplace_tiles(vp);
    dense = xg_regions_ptr(reg, scatter ? XG_BUF_SEND : XG_BUF_RECV);
    if (scatter) {          /* collective write: exchange into the dense layout, then scatter it */
        if ((rc = xg_exchange_v(ctx, method, procs, cb_nodes, lens, rank_list, comm_size, send, dense, timers, iter,
                                ntimes, opts, bad_slots, err, errlen)))
            goto out;       /* every rank alike: xg_exchange_v agreed on it */
    }
    rc = xg_vecplace_run(vp, &secs);
    if (rc == XG_OK && place_s) *place_s = secs;
    if (rc == XG_OK && opts->verify && (rc = chk_rows(reg, rows, nrows, &nbad)) == XG_OK) {
        if (nbad) fprintf(stderr, "gpu %d: %lld placed vecs differ from their source\n", g, (long long)nbad);
        if (bad_vecs) *bad_vecs = nbad;
    }
    if (rc && err[0] == 0) snprintf(err, errlen, "placement: device error %d (see stderr)", rc);
    if (G > 1) rc = peers_agree(ctx, rc, err, errlen);      /* a failed placement stops every rank here */
    if (rc == XG_OK && !scatter)   /* collective read: gathered, now exchange the dense layout */
        rc = xg_exchange_v(ctx, method, procs, cb_nodes, lens, rank_list, comm_size, dense, recv, timers, iter,
                           ntimes, opts, bad_slots, err, errlen);
out:
    if (rc && err[0] == 0) snprintf(err, errlen, "device error %d (see stderr)", rc);
    free(rows); free(lens);
    if (vp) xg_vecplace_free(vp);
    if (reg) xg_regions_free(reg);
    xg_sched_free(s);
    return rc;
}
