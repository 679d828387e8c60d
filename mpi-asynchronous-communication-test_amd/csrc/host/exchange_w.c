/*
 * exchange_w.c -- xg_exchange_w (xg.h): xg_exchange_v with the aggregator side placed by an
 * offset-length list.  The exchange itself is xg_exchange_v, unchanged, over a dense intermediate
 * the library owns; one extra GPU-local copy step (xg_place_plan_build: one copy per extent, run on
 * copy_kernel_x where its runs are short) scatters that intermediate into the caller's domain
 * buffer after the exchange (a2m, the collective write) or gathers it out of the domain buffer
 * before the exchange (m2a, the collective read).  Placement posts no RCCL call of its own; what the
 * ranks must agree on (the list, the domain lengths, every rank's set-up) is settled with the MAX
 * all-reduce before the exchange's first call.  A translation unit of its own, as exchange.c is.
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"

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

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t i;
    for (i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

/* every rank passed the same list and domain lengths (field by field: the struct has no padding
 * today, but a hash must not depend on that) */
static int lists_agree(xg_ctx *ctx, int procs, int cb_nodes, const xg_ext *exts, int64_t n, const int64_t *dom_bytes,
                       char *err, size_t errlen)
{
    double red[8];
    uint64_t h = 0xcbf29ce484222325ull;
    int64_t i, v[4];
    int rc, j;
    v[0] = procs; v[1] = cb_nodes; v[2] = n; v[3] = (exts != NULL) | ((dom_bytes != NULL) << 1);
    h = fnv(h, v, sizeof v);
    if (exts)
        for (i = 0; i < n; ++i) {
            v[0] = exts[i].rank; v[1] = exts[i].agg; v[2] = exts[i].off; v[3] = exts[i].len;
            h = fnv(h, v, sizeof v);
        }
    if (dom_bytes && cb_nodes > 0) h = fnv(h, dom_bytes, sizeof(int64_t) * (size_t)cb_nodes);
    for (j = 0; j < 4; ++j) {
        red[j] = (double)((h >> (16 * j)) & 0xffff);
        red[4 + j] = -red[j];
    }
    if ((rc = xg_allreduce_max(ctx, red, 8))) return rc;
    for (j = 0; j < 4; ++j)
        if (red[j] != -red[4 + j]) {
            snprintf(err, errlen, "the GPU processes passed different inputs to the placement (extent lists or "
                     "domain lengths differ between ranks)");
            return XG_EARG;
        }
    return XG_OK;
}

/* xg_chk64 of one side of every hosted extent (the placement plan's copies, in list order) */
static int chk_exts(xg_regions *reg, const xg_devplan *pd, int dst_side, xg_bufspan *sp, uint64_t *chk)
{
    int k;
    for (k = 0; k < pd->ncopy; ++k) {
        sp[k].buf = dst_side ? pd->copies[k].dst_buf : pd->copies[k].src_buf; sp[k].pad = 0;
        sp[k].off = dst_side ? pd->copies[k].dst_off : pd->copies[k].src_off;
        sp[k].len = pd->copies[k].len;
    }
    return xg_chk_spans(reg, sp, pd->ncopy, chk);
}

int xg_exchange_w(xg_ctx *ctx, int method, int procs, int cb_nodes, const xg_ext *exts, int64_t n,
                  const int64_t *dom_bytes, const int *rank_list, int comm_size, void *send, void *recv,
                  xg_timer *timers, int iter, int ntimes, const xg_run_opts *opts, int64_t *bad_slots,
                  int64_t *bad_exts, double *place_s, char *err, size_t errlen)
{
    xg_run_opts dflt;
    char ebuf[512];
    xg_sched *s = NULL;
    xg_devplan *pd = NULL;
    xg_regions *reg = NULL;
    xg_plan *plan = NULL;
    xg_bufspan *sp = NULL;
    uint64_t *c_src = NULL, *c_dst = NULL;
    int64_t *lens = NULL, nbad = 0;
    double done[2] = {0, 0}, post[2] = {0, 0}, wall = 0;
    void *dense = NULL;
    int g, G, rc = XG_OK, dir, k, scatter;
    if (!opts) { xg_run_opts_default(&dflt); opts = &dflt; }
    if (!err) { err = ebuf; errlen = sizeof ebuf; }
    err[0] = 0;
    if (bad_slots) *bad_slots = 0;
    if (bad_exts) *bad_exts = 0;
    if (place_s) *place_s = 0;
    if (!ctx || xg_is_virtual(ctx)) {
        snprintf(err, errlen, "xg_exchange_w needs a real context (a virtual GPU's plans run only together)");
        return XG_EARG;
    }
    g = xg_rank(ctx); G = xg_nranks(ctx);
    dir = xg_method_direction(method);
    scatter = dir == XG_A2M;
    if (G > 1 && (rc = lists_agree(ctx, procs, cb_nodes, exts, n, dom_bytes, err, errlen))) return rc;
    /* this rank's set-up: the list, the matrix, the placement plan, the regions around the caller's
     * domain buffer and the library's dense intermediate, the plan upload */
    if (dir < 0) {
        snprintf(err, errlen, "method %d is not one of 1..20", method);
        rc = XG_EARG;
    } else if (!rank_list) {
        snprintf(err, errlen, "xg_exchange_w: no aggregator list");
        rc = XG_EARG;
    } else {
        rc = xg_exts_check(exts, n, procs, cb_nodes, dom_bytes, scatter, err, errlen);
    }
    if (rc == XG_OK && !(lens = (int64_t *)malloc(sizeof *lens * (size_t)procs * (size_t)cb_nodes + 8))) {
        snprintf(err, errlen, "placement: out of host memory");
        rc = XG_ENOMEM;
    }
    if (rc == XG_OK && (rc = xg_exts_lens(exts, n, procs, cb_nodes, lens)))
        snprintf(err, errlen, "extent list: the lengths of one (rank, aggregator) pair overflow");
    if (rc == XG_OK && !(s = xg_sched_build_v(method, procs, cb_nodes, lens, comm_size, rank_list, ntimes, opts->proc_node,
                                              opts->barrier_type, opts->eager_limit, iter, err, errlen)))
        rc = XG_ESCHED;
    if (rc == XG_OK && !(pd = xg_place_plan_build(s, G, g, exts, n, dom_bytes))) {
        snprintf(err, errlen, "placement plan: out of host memory");
        rc = XG_ENOMEM;
    }
    if (rc == XG_OK && (rc = xg_regions_adopt(ctx, pd->region_bytes, scatter ? NULL : send, scatter ? recv : NULL, &reg)))
        snprintf(err, errlen, "regions of %lld (dense) + %lld (domain) bytes around the caller's domain buffer %p: "
                 "refused or allocation failed (%d, see stderr)",
                 (long long)pd->region_bytes[scatter ? XG_BUF_SEND : XG_BUF_RECV],
                 (long long)pd->region_bytes[scatter ? XG_BUF_RECV : XG_BUF_SEND], scatter ? recv : send, rc);
    if (rc == XG_OK && (rc = xg_plan_load(ctx, reg, pd, &plan)))
        snprintf(err, errlen, "placement plan: not loaded (%d, see stderr)", rc);
    if (rc == XG_OK && opts->verify) {
        sp = (xg_bufspan *)malloc(sizeof *sp * ((size_t)pd->ncopy + 1));
        c_src = (uint64_t *)calloc((size_t)pd->ncopy + 1, sizeof *c_src);
        c_dst = (uint64_t *)calloc((size_t)pd->ncopy + 1, sizeof *c_dst);
        if (!sp || !c_src || !c_dst) {
            snprintf(err, errlen, "placement check: out of host memory");
            rc = XG_ENOMEM;
        }
    }
    if (G > 1) rc = peers_agree(ctx, rc, err, errlen);      /* before the exchange's first call */
    if (rc) goto out;
    dense = xg_regions_ptr(reg, scatter ? XG_BUF_SEND : XG_BUF_RECV);
    if (scatter) {          /* collective write: exchange into the dense layout, then scatter it */
        if ((rc = xg_exchange_v(ctx, method, procs, cb_nodes, lens, rank_list, comm_size, send, dense, timers, iter,
                                ntimes, opts, bad_slots, err, errlen)))
            goto out;       /* every rank alike: xg_exchange_v agreed on it */
    }
    if (opts->verify) rc = chk_exts(reg, pd, 0, sp, c_src);
    if (rc == XG_OK) rc = xg_plan_run(plan, done, post, &wall);
    if (rc == XG_OK && place_s) *place_s = done[0];
    if (rc == XG_OK && opts->verify && (rc = chk_exts(reg, pd, 1, sp, c_dst)) == XG_OK) {
        for (k = 0; k < pd->ncopy; ++k) nbad += c_src[k] != c_dst[k];
        if (nbad) fprintf(stderr, "gpu %d: %lld placed extents differ from their source\n", g, (long long)nbad);
        if (bad_exts) *bad_exts = nbad;
    }
    if (rc && err[0] == 0) snprintf(err, errlen, "placement: device error %d (see stderr)", rc);
    if (G > 1) rc = peers_agree(ctx, rc, err, errlen);      /* a failed placement stops every rank here */
    if (rc == XG_OK && !scatter)   /* collective read: gathered, now exchange the dense layout */
        rc = xg_exchange_v(ctx, method, procs, cb_nodes, lens, rank_list, comm_size, dense, recv, timers, iter,
                           ntimes, opts, bad_slots, err, errlen);
out:
    if (rc && err[0] == 0) snprintf(err, errlen, "device error %d (see stderr)", rc);
    free(sp); free(c_src); free(c_dst); free(lens);
    if (plan) xg_plan_free(plan);
    if (reg) xg_regions_free(reg);
    xg_devplan_free(pd);
    xg_sched_free(s);
    return rc;
}
