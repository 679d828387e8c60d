/*
 * exchange.c -- a method's exchange over the CALLER's device buffers (xg_exchange, xg.h).
 * The flow of xg_run_method (methods.c) with three changes: the SEND / RECV regions are adopted
 * (xg_regions_adopt), nothing is filled, and delivery is checked by span checksums of bytes the
 * library does not know (xg_chk_spans over xg_deliveries) instead of a fingerprint.
 * xg_exchange_v is the same exchange with a length per (rank, aggregator) pair (xg_sched_build_v).
 * A translation unit of its own: methods.c stays free of the entry points used here, so what
 * links methods.c against another device half keeps linking.  The agreements are agree.h's, the
 * set-up around the regions is job.h's (defined in methods.c).
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"
#include "agree.h"
#include "job.h"

#define TRY(x) do { rc = (x); if (rc) goto out; } while (0)
#define WHAT "setting up or running this exchange"

/* the digest of everything the plan is derived from (agree.h; the fingerprint is not an input here,
 * verify is: the ranks share the source checksums in a collective only when it is set) */
static int inputs_agree(xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int64_t *lens,
                        int ragged, const int *rank_list, int comm_size, int iter, int ntimes, const xg_run_opts *o,
                        char *err, size_t errlen)
{
    int64_t v[15];
    uint64_t h = AGREE_FNV_INIT;
    int rc, differ;
    v[0] = method; v[1] = procs; v[2] = cb_nodes; v[3] = data_size; v[4] = comm_size; v[5] = iter;
    v[6] = ntimes; v[7] = o->eager_limit; v[8] = o->pack_max_seg; v[9] = o->pack_min_bytes;
    v[10] = o->proc_node; v[11] = o->barrier_type; v[12] = o->pack_form; v[13] = xg_self_max(ctx);
    v[14] = o->verify != 0;
    h = agree_fnv(h, v, sizeof v);
    h = agree_fnv(h, rank_list, sizeof(int) * (size_t)cb_nodes);
    if (ragged) {           /* xg_exchange_v: the whole matrix (or that there is none) */
        const int64_t have = lens != NULL;
        h = agree_fnv(h, &have, sizeof have);
        if (lens && procs > 0 && cb_nodes > 0)
            h = agree_fnv(h, lens, sizeof(int64_t) * (size_t)procs * (size_t)cb_nodes);
    }
    if ((rc = agree_digest(ctx, h, &differ)) || !differ) return rc;
    snprintf(err, errlen, "the GPU processes planned the exchange (method %d) from different inputs "
             "(arguments or options differ between ranks)", method);
    return XG_EARG;
}

/* One GPU's set-up (untimed, no collective call): job_plan, the regions around the caller's
 * buffers, job_load. */
static int setup(xg_ctx *ctx, job *j, int method, int procs, int cb_nodes, int data_size, const int64_t *lens,
                 int ragged, const int *rank_list, int comm_size, void *send, void *recv, int iter, int ntimes,
                 const xg_run_opts *o, char *err, size_t errlen)
{
    int rc;
    if ((rc = job_plan(j, ctx, method, procs, cb_nodes, data_size, lens, ragged, rank_list, comm_size, iter, ntimes, o,
                       err, errlen)))
        return rc;
    if ((rc = xg_regions_adopt(ctx, j->dp->region_bytes, send, recv, &j->reg))) {
        snprintf(err, errlen, "regions of %lld (SEND) + %lld (RECV) + %lld + %lld + %lld bytes around the caller's "
                 "buffers %p / %p: refused or allocation failed (%d, see stderr)",
                 (long long)j->dp->region_bytes[0], (long long)j->dp->region_bytes[1],
                 (long long)j->dp->region_bytes[2], (long long)j->dp->region_bytes[3],
                 (long long)j->dp->region_bytes[4], send, recv, rc);
        return rc;
    }
    return job_load(j, ctx, err, errlen);
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
    job jb = {0};
    xg_delivery *dl = NULL;
    xg_bufspan *sp = NULL;
    uint64_t *src_chk = NULL, *dst_chk = NULL, *tmp = NULL;
    double wall = 0, *red = NULL;
    int64_t nbad = 0, *dlen = NULL;
    int *idx = NULL;
    int g, G, rc = 0, agreed = 0, k, j, nd = 0;
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
    rc = setup(ctx, &jb, method, procs, cb_nodes, data_size, lens, ragged, rank_list, comm_size, send, recv, iter, ntimes,
               opts, err, errlen);
    if (rc == XG_OK && opts->verify) {
        /* the source checksums this GPU owns: before the run, while SEND is what the caller gave */
        nd = xg_deliveries(jb.s, G, NULL);
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
            xg_deliveries(jb.s, G, dl);
            xg_delivery_lens(jb.s, G, dlen);
            rc = chk_side(jb.reg, dl, nd, g, 0, dlen, sp, idx, tmp, src_chk);
        }
    }
    if (G > 1) rc = agree_peers(ctx, rc, NULL, WHAT, err, errlen);  /* before the first call of the exchange */
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
    TRY(xg_plan_run(jb.plan, jb.done, jb.post, &wall));
    job_timers(&jb, ctx, procs, timers, ntimes, opts);
    if (opts->verify) {
        TRY(chk_side(jb.reg, dl, nd, g, 1, dlen, sp, idx, tmp, dst_chk));
        for (k = 0; k < nd; ++k)
            if (dl[k].dst_gpu == g && dst_chk[k] != src_chk[k]) {
                if (nbad == 0) fprintf(stderr, "rank %d, message is wrong from rank %d\n", dl[k].dst, dl[k].src);
                ++nbad;
            }
        if (bad_slots) *bad_slots = nbad;
    }
out:
    if (G > 1 && agreed) rc = agree_peers(ctx, rc, NULL, WHAT, err, errlen);
    if (rc && err[0] == 0) snprintf(err, errlen, "device error %d (see stderr)", rc);
    free(dl); free(sp); free(idx); free(dlen); free(src_chk); free(dst_chk); free(tmp); free(red);
    job_free(&jb);
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
