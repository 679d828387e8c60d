/*
 * exchange.c -- a method's exchange over the CALLER's device buffers (xg_exchange, xg.h).
 * The flow of xg_run_method (methods.c) with three changes: the SEND / RECV regions are adopted
 * (xg_regions_adopt), nothing is filled, and delivery is checked by span checksums of bytes the
 * library does not know (xg_chk_spans over xg_deliveries) instead of a fingerprint.
 * xg_exchange_v is the same exchange with a length per (rank, aggregator) pair (xg_sched_build_v).
 * A translation unit of its own: methods.c stays free of the entry points used here, so what
 * links methods.c against another device half keeps linking.  The two agreement helpers are
 * the ones of methods.c.
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"

#define TRY(x) do { rc = (x); if (rc) goto out; } while (0)

/* methods.c: peers_agree */
static int peers_agree(xg_ctx *ctx, int local_rc, char *err, size_t errlen)
{
    double red[2];
    int rc;
    red[0] = local_rc ? 1.0 : 0.0;
    red[1] = (double)local_rc;
    if ((rc = xg_allreduce_max(ctx, red, 2))) return local_rc ? local_rc : rc;
    if (red[0] == 0.0) return XG_OK;
    if (local_rc) return local_rc;
    snprintf(err, errlen, "another GPU of the job failed (code %d) setting up or running this exchange", (int)red[1]);
    return (int)red[1];
}

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t i;
    for (i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

/* methods.c: inputs_agree (the fingerprint is not an input here, verify is: the ranks share the
 * source checksums in a collective only when it is set) */
static int inputs_agree(xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int64_t *lens,
                        int ragged, const int *rank_list, int comm_size, int iter, int ntimes, const xg_run_opts *o,
                        char *err, size_t errlen)
{
    int64_t v[15];
    double red[8];
    uint64_t h = 0xcbf29ce484222325ull;
    int i, rc;
    v[0] = method; v[1] = procs; v[2] = cb_nodes; v[3] = data_size; v[4] = comm_size; v[5] = iter;
    v[6] = ntimes; v[7] = o->eager_limit; v[8] = o->pack_max_seg; v[9] = o->pack_min_bytes;
    v[10] = o->proc_node; v[11] = o->barrier_type; v[12] = o->pack_form; v[13] = xg_self_max(ctx);
    v[14] = o->verify != 0;
    h = fnv(h, v, sizeof v);
    h = fnv(h, rank_list, sizeof(int) * (size_t)cb_nodes);
    if (ragged) {           /* xg_exchange_v: the whole matrix (or that there is none) */
        const int64_t have = lens != NULL;
        h = fnv(h, &have, sizeof have);
        if (lens && procs > 0 && cb_nodes > 0) h = fnv(h, lens, sizeof(int64_t) * (size_t)procs * (size_t)cb_nodes);
    }
    for (i = 0; i < 4; ++i) {
        red[i] = (double)((h >> (16 * i)) & 0xffff);
        red[4 + i] = -red[i];
    }
    if ((rc = xg_allreduce_max(ctx, red, 8))) return rc;
    for (i = 0; i < 4; ++i)
        if (red[i] != -red[4 + i]) {
            snprintf(err, errlen, "the GPU processes planned the exchange (method %d) from different inputs "
                     "(arguments or options differ between ranks)", method);
            return XG_EARG;
        }
    return XG_OK;
}

static int pairing_ok(const xg_sched *s, int G, const xg_run_opts *o, int64_t self_max, char *err, size_t errlen)
{
    xg_devplan **plans = (xg_devplan **)calloc(G, sizeof *plans);
    int g, rc = XG_OK;
    char why[400];
    if (!plans) {
        snprintf(err, errlen, "pairing check: out of host memory");
        return XG_ENOMEM;
    }
    for (g = 0; g < G && rc == XG_OK; ++g)
        if (!(plans[g] = xg_devplan_build_form(s, G, g, o->pack_max_seg, o->pack_min_bytes, o->pack_form))) {
            snprintf(err, errlen, "pairing check: out of host memory building GPU %d's plan", g);
            rc = XG_ENOMEM;
        }
    if (rc == XG_OK && xg_devplans_match((const xg_devplan *const *)plans, G, self_max, NULL, 0, why, sizeof why) < 0) {
        snprintf(err, errlen, "the GPUs' RCCL calls do not pair: %s", why);
        rc = XG_EARG;
    }
    for (g = 0; g < G; ++g) xg_devplan_free(plans[g]);
    free(plans);
    return rc;
}

/* One GPU's set-up (untimed, no collective call): schedule, pairing proof, device plan, the
 * regions around the caller's buffers, plan upload and the host arrays. */
static int setup(xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int64_t *lens, int ragged,
                 const int *rank_list, int comm_size,
                 void *send, void *recv, int iter, int ntimes, const xg_run_opts *o, xg_sched **s, xg_devplan **dp,
                 xg_regions **reg, xg_plan **plan, double **done, double **post, char *err, size_t errlen)
{
    const int g = xg_rank(ctx), G = xg_nranks(ctx);
    uint8_t *need;
    int rc;
    if (ragged)
        *s = xg_sched_build_v(method, procs, cb_nodes, lens, comm_size, rank_list, ntimes, o->proc_node,
                              o->barrier_type, o->eager_limit, iter, err, errlen);
    else
        *s = xg_sched_build_iter(method, procs, cb_nodes, data_size, comm_size, rank_list, ntimes, o->proc_node,
                                 o->barrier_type, o->eager_limit, iter, err, errlen);
    if (!*s) return XG_ESCHED;
    if (G > 1 && (rc = pairing_ok(*s, G, o, xg_self_max(ctx), err, errlen))) return rc;
    if (!(*dp = xg_devplan_build_form(*s, G, g, o->pack_max_seg, o->pack_min_bytes, o->pack_form))) {
        snprintf(err, errlen, "device plan: out of host memory");
        return XG_ENOMEM;
    }
    if ((rc = xg_regions_adopt(ctx, (*dp)->region_bytes, send, recv, reg))) {
        snprintf(err, errlen, "regions of %lld (SEND) + %lld (RECV) + %lld + %lld + %lld bytes around the caller's "
                 "buffers %p / %p: refused or allocation failed (%d, see stderr)",
                 (long long)(*dp)->region_bytes[0], (long long)(*dp)->region_bytes[1],
                 (long long)(*dp)->region_bytes[2], (long long)(*dp)->region_bytes[3],
                 (long long)(*dp)->region_bytes[4], send, recv, rc);
        return rc;
    }
    *done = (double *)calloc(xg_sched_nsteps(*s) + 1, sizeof(double));
    *post = (double *)calloc(xg_sched_nsteps(*s) + 1, sizeof(double));
    need = (uint8_t *)malloc((size_t)xg_sched_nsteps(*s) + 1);
    if (!*done || !*post || !need) {
        free(need);
        snprintf(err, errlen, "out of host memory");
        return XG_ENOMEM;
    }
    if ((rc = xg_plan_load(ctx, *reg, *dp, plan)) == XG_OK) {
        xg_sched_timed_steps(*s, need);          /* mark only the steps whose completion a Timer reads */
        rc = xg_plan_set_step_marks(*plan, need);
    }
    free(need);
    return rc;
}

/* xg_chk64 of side `recv` of the deliveries this GPU hosts (delivery k: dlen[k] bytes, xg_delivery_lens),
 * into chk[k] (the others untouched) */
static int chk_side(xg_regions *reg, const xg_delivery *dl, int nd, int g, int recv, const int64_t *dlen,
                    xg_bufspan *sp, int *idx, uint64_t *tmp, uint64_t *chk)
{
    int k, n = 0, rc;
    for (k = 0; k < nd; ++k) {
        if ((recv ? dl[k].dst_gpu : dl[k].src_gpu) != g) continue;
        sp[n].buf = recv ? XG_BUF_RECV : XG_BUF_SEND; sp[n].pad = 0;
        sp[n].off = recv ? dl[k].recv_off : dl[k].send_off; sp[n].len = dlen[k];
        idx[n++] = k;
    }
    if ((rc = xg_chk_spans(reg, sp, n, tmp))) return rc;
    for (k = 0; k < n; ++k) chk[idx[k]] = tmp[k];
    return XG_OK;
}

/* xg_exchange (ragged = 0: data_size) and xg_exchange_v (ragged = 1: lens) */
static int exchange(xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int64_t *lens, int ragged,
                    const int *rank_list, int comm_size, void *send, void *recv, xg_timer *timers, int iter,
                    int ntimes, const xg_run_opts *opts, int64_t *bad_slots, char *err, size_t errlen)
{
    xg_run_opts dflt;
    char ebuf[512];
    xg_sched *s = NULL;
    xg_devplan *dp = NULL;
    xg_regions *reg = NULL;
    xg_plan *plan = NULL;
    xg_delivery *dl = NULL;
    xg_bufspan *sp = NULL;
    uint64_t *src_chk = NULL, *dst_chk = NULL, *tmp = NULL;
    double *done = NULL, *post = NULL, wall = 0, *red = NULL;
    int64_t nbad = 0, *dlen = NULL;
    int *idx = NULL;
    int g, G, rc = 0, agreed = 0, lo, hi, r, k, j, nd = 0;
    if (!opts) { xg_run_opts_default(&dflt); opts = &dflt; }
    if (!err) { err = ebuf; errlen = sizeof ebuf; }
    err[0] = 0;
    if (bad_slots) *bad_slots = 0;
    if (!ctx || xg_is_virtual(ctx)) {
        snprintf(err, errlen, "xg_exchange / xg_exchange_v needs a real context (a virtual GPU's plans run only together)");
        return XG_EARG;
    }
    g = xg_rank(ctx); G = xg_nranks(ctx);
    if (G > 1 && (rc = inputs_agree(ctx, method, procs, cb_nodes, data_size, lens, ragged, rank_list, comm_size, iter,
                                    ntimes, opts, err, errlen)))
        return rc;
    rc = setup(ctx, method, procs, cb_nodes, data_size, lens, ragged, rank_list, comm_size, send, recv, iter, ntimes,
               opts, &s, &dp, &reg, &plan, &done, &post, err, errlen);
    if (rc == XG_OK && opts->verify) {
        /* the source checksums this GPU owns: before the run, while SEND is what the caller gave */
        nd = xg_deliveries(s, G, NULL);
        dl = (xg_delivery *)malloc(sizeof *dl * (nd + 1));
        sp = (xg_bufspan *)malloc(sizeof *sp * (nd + 1));
        idx = (int *)malloc(sizeof *idx * (nd + 1));
        dlen = (int64_t *)malloc(sizeof *dlen * (nd + 1));
        src_chk = (uint64_t *)calloc(nd + 1, sizeof *src_chk);
        dst_chk = (uint64_t *)calloc(nd + 1, sizeof *dst_chk);
        tmp = (uint64_t *)calloc(nd + 1, sizeof *tmp);
        red = (double *)calloc(4 * (size_t)nd + 1, sizeof *red);
        if (!dl || !sp || !idx || !dlen || !src_chk || !dst_chk || !tmp || !red) {
            snprintf(err, errlen, "payload check: out of host memory");
            rc = XG_ENOMEM;
        } else {
            xg_deliveries(s, G, dl);
            xg_delivery_lens(s, G, dlen);
            rc = chk_side(reg, dl, nd, g, 0, dlen, sp, idx, tmp, src_chk);
        }
    }
    if (G > 1) rc = peers_agree(ctx, rc, err, errlen);      /* before the first call of the exchange */
    if (rc) goto out;
    agreed = 1;
    if (opts->verify) {
        /* every GPU learns every segment's checksum: 16-bit parts (exact as doubles), the owner
         * contributes part + 1, the others 0; a part still 0 has no owner */
        for (k = 0; k < nd; ++k)
            for (j = 0; j < 4; ++j)
                red[4 * k + j] = dl[k].src_gpu == g ? (double)((src_chk[k] >> (16 * j)) & 0xffff) + 1.0 : 0.0;
        TRY(xg_allreduce_max(ctx, red, 4 * nd));
        for (k = 0; k < nd; ++k) {
            uint64_t c = 0;
            for (j = 0; j < 4; ++j) {
                if (red[4 * k + j] < 1.0) {
                    snprintf(err, errlen, "payload check: no GPU sent the checksum of rank %d's segment %d",
                             dl[k].src, dl[k].seed);
                    rc = XG_EARG;
                    goto out;
                }
                c |= (uint64_t)(red[4 * k + j] - 1.0) << (16 * j);
            }
            src_chk[k] = c;
        }
    }
    TRY(xg_barrier(ctx));                                   /* MPI_Barrier before total_start */
    TRY(xg_plan_run(plan, done, post, &wall));
    xg_block_range(procs, G, g, &lo, &hi);
    if (timers)
        for (r = lo; r < hi; ++r) xg_sched_rank_timer(s, G, r, done, post, &timers[r - lo]);
    if (opts->rep_timers && ntimes > 0)
        for (r = lo; r < hi; ++r)
            xg_sched_rank_rep_timers(s, G, r, done, post, opts->rep_timers + (size_t)(r - lo) * ntimes);
    if (opts->verify) {
        TRY(chk_side(reg, dl, nd, g, 1, dlen, sp, idx, tmp, dst_chk));
        for (k = 0; k < nd; ++k)
            if (dl[k].dst_gpu == g && dst_chk[k] != src_chk[k]) {
                if (nbad == 0) fprintf(stderr, "rank %d, message is wrong from rank %d\n", dl[k].dst, dl[k].src);
                ++nbad;
            }
        if (bad_slots) *bad_slots = nbad;
    }
out:
    if (G > 1 && agreed) rc = peers_agree(ctx, rc, err, errlen);
    if (rc && err[0] == 0) snprintf(err, errlen, "device error %d (see stderr)", rc);
    free(dl); free(sp); free(idx); free(dlen); free(src_chk); free(dst_chk); free(tmp); free(red); free(done); free(post);
    if (plan) xg_plan_free(plan);
    if (reg) xg_regions_free(reg);
    xg_devplan_free(dp);
    xg_sched_free(s);
    return rc;
}

int xg_exchange(xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int *rank_list,
                int comm_size, void *send, void *recv, xg_timer *timers, int iter, int ntimes,
                const xg_run_opts *opts, int64_t *bad_slots, char *err, size_t errlen)
{
    return exchange(ctx, method, procs, cb_nodes, data_size, NULL, 0, rank_list, comm_size, send, recv, timers, iter,
                    ntimes, opts, bad_slots, err, errlen);
}

int xg_exchange_v(xg_ctx *ctx, int method, int procs, int cb_nodes, const int64_t *lens, const int *rank_list,
                  int comm_size, void *send, void *recv, xg_timer *timers, int iter, int ntimes,
                  const xg_run_opts *opts, int64_t *bad_slots, char *err, size_t errlen)
{
    return exchange(ctx, method, procs, cb_nodes, 0, lens, 1, rank_list, comm_size, send, recv, timers, iter, ntimes,
                    opts, bad_slots, err, errlen);
}
