/*
 * methods.c -- the reference's per-method operators on the MI355X runtime.
 * One call = prepare_*_data (regions + fingerprint, untimed) -> MPI_Barrier ->
 * the timed exchange -> Timer of every hosted logical rank -> clean_* ;
 * plus optional verification (the reference's commented-out check_buffer).
 * Compiled into libxg.so; links libxghost.so for schedules.
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"
#include "agree.h"
#include "job.h"

void xg_run_opts_default(xg_run_opts *o)
{
    o->verify = 0;
    o->fingerprint = XG_FP_REFERENCE;
    o->eager_limit = XG_MPICH_EAGER_LIMIT;
    o->pack_max_seg = 4 << 20;
    o->proc_node = 1;
    o->barrier_type = 0;
    o->rep_timers = NULL;
    o->pack_min_bytes = 64 << 10;   /* latency-bound steps: one RCCL launch (profiles/r03/hybrid/) */
    o->pack_form = XG_PACK_FORM_DEFAULT;
}

#define TRY(x) do { rc = (x); if (rc) goto out; } while (0)
#define WHAT "setting up or running this method"

/* ------------------------------------------------------------------ one GPU's share of a run (job.h)
 * Defined here, not in a unit of their own: whatever links methods.c against another device half
 * (tests/host_dev.c) gets them with it.  They call only what every device half has. */

int job_pairing_ok(const xg_sched *s, int G, const xg_run_opts *o, int64_t self_max, char *err, size_t errlen)
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

int job_plan(job *j, xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int64_t *lens, int ragged,
             const int *rank_list, int comm_size, int iter, int ntimes, const xg_run_opts *o, char *err, size_t errlen)
{
    const int g = xg_rank(ctx), G = xg_nranks(ctx);
    int rc;
    if (ragged)
        j->s = xg_sched_build_v(method, procs, cb_nodes, lens, comm_size, rank_list, ntimes, o->proc_node,
                                o->barrier_type, o->eager_limit, iter, err, errlen);
    else
        j->s = xg_sched_build_iter(method, procs, cb_nodes, data_size, comm_size, rank_list, ntimes, o->proc_node,
                                   o->barrier_type, o->eager_limit, iter, err, errlen);
    if (!j->s) return XG_ESCHED;
    /* every GPU derives every GPU's calls from the same schedule, so every GPU refuses a job
     * that would not pair alike -- before any of them posts a call that could wait forever */
    if (G > 1 && (rc = job_pairing_ok(j->s, G, o, xg_self_max(ctx), err, errlen))) return rc;
    if (!(j->dp = xg_devplan_build_form(j->s, G, g, o->pack_max_seg, o->pack_min_bytes, o->pack_form))) {
        snprintf(err, errlen, "device plan: out of host memory");
        return XG_ENOMEM;
    }
    return XG_OK;
}

int job_load(job *j, xg_ctx *ctx, char *err, size_t errlen)
{
    const size_t n = (size_t)xg_sched_nsteps(j->s) + 1;
    uint8_t *need = (uint8_t *)malloc(n);
    int rc;
    j->done = (double *)calloc(n, sizeof(double));
    j->post = (double *)calloc(n, sizeof(double));
    if (!j->done || !j->post || !need) {
        free(need);
        snprintf(err, errlen, "out of host memory");
        return XG_ENOMEM;
    }
    if ((rc = xg_plan_load(ctx, j->reg, j->dp, &j->plan)) == XG_OK) {
        xg_sched_timed_steps(j->s, need);          /* mark only the steps whose completion a Timer reads */
        rc = xg_plan_set_step_marks(j->plan, need);
    }
    free(need);
    return rc;
}

void job_timers(const job *j, xg_ctx *ctx, int procs, xg_timer *timers, int ntimes, const xg_run_opts *o)
{
    const int G = xg_nranks(ctx);
    int lo, hi, r;
    xg_block_range(procs, G, xg_rank(ctx), &lo, &hi);
    if (timers)
        for (r = lo; r < hi; ++r) xg_sched_rank_timer(j->s, G, r, j->done, j->post, &timers[r - lo]);
    if (o->rep_timers && ntimes > 0)
        for (r = lo; r < hi; ++r)
            xg_sched_rank_rep_timers(j->s, G, r, j->done, j->post, o->rep_timers + (size_t)(r - lo) * ntimes);
}

void job_free(job *j)
{
    free(j->done); free(j->post);
    if (j->plan) xg_plan_free(j->plan);
    if (j->reg) xg_regions_free(j->reg);
    xg_devplan_free(j->dp);
    xg_sched_free(j->s);
}

/* ------------------------------------------------------------------ xg_run_method */

/* Every GPU of a job must plan from the same inputs (agree.h): the digest of all that the plan is
 * derived from, compared before anything that could diverge. */
static int inputs_agree(xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int *rank_list,
                        int comm_size, int iter, int ntimes, const xg_run_opts *o, char *err, size_t errlen)
{
    int64_t v[14];
    uint64_t h = AGREE_FNV_INIT;
    int rc, differ;
    v[0] = method; v[1] = procs; v[2] = cb_nodes; v[3] = data_size; v[4] = comm_size; v[5] = iter;
    v[6] = ntimes; v[7] = o->eager_limit; v[8] = o->pack_max_seg; v[9] = o->pack_min_bytes;
    v[10] = o->proc_node; v[11] = o->barrier_type; v[12] = o->pack_form; v[13] = xg_self_max(ctx);
    h = agree_fnv(h, v, sizeof v);
    h = agree_fnv(h, rank_list, sizeof(int) * (size_t)cb_nodes);
    if ((rc = agree_digest(ctx, h, &differ)) || !differ) return rc;
    snprintf(err, errlen, "the GPU processes planned method %d from different inputs (arguments or "
             "options differ between ranks)", method);
    return XG_EARG;
}

/* Set-up of one GPU's part (untimed, no collective call): job_plan, the regions, the fingerprint
 * fill, job_load.  -> XG_OK or the first error. */
static int setup(xg_ctx *ctx, job *j, int method, int procs, int cb_nodes, int data_size, const int *rank_list,
                 int comm_size, int iter, int ntimes, const xg_run_opts *o, char *err, size_t errlen)
{
    const int g = xg_rank(ctx), G = xg_nranks(ctx);
    xg_segrun *runs;
    int rc, nruns;
    if ((rc = job_plan(j, ctx, method, procs, cb_nodes, data_size, NULL, 0, rank_list, comm_size, iter, ntimes, o, err,
                       errlen)))
        return rc;
    if ((rc = xg_regions_alloc(ctx, j->dp->region_bytes, &j->reg))) {
        snprintf(err, errlen, "HBM regions of %lld + %lld + %lld + %lld + %lld bytes: allocation failed (%d)",
                 (long long)j->dp->region_bytes[0], (long long)j->dp->region_bytes[1],
                 (long long)j->dp->region_bytes[2], (long long)j->dp->region_bytes[3],
                 (long long)j->dp->region_bytes[4], rc);
        return rc;
    }
    nruns = xg_fill_runs(j->s, G, g, NULL);
    if (!(runs = (xg_segrun *)malloc(sizeof(xg_segrun) * (nruns + 1)))) {
        snprintf(err, errlen, "out of host memory");
        return XG_ENOMEM;
    }
    xg_fill_runs(j->s, G, g, runs);
    rc = xg_fill(j->reg, runs, nruns, data_size, iter, o->fingerprint);
    free(runs);
    return rc ? rc : job_load(j, ctx, err, errlen);
}

int xg_run_method(xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int *rank_list,
                  int comm_size, xg_timer *timers, int iter, int ntimes, const xg_run_opts *opts,
                  int64_t *bad_slots, char *err, size_t errlen)
{
    xg_run_opts dflt;
    const int g = xg_rank(ctx), G = xg_nranks(ctx);
    char ebuf[512];
    job j = {0};
    xg_slot *slots = NULL;
    int64_t *bad = NULL, nbad = 0;
    double wall = 0;
    int rc = 0, agreed = 0, i;
    if (!opts) { xg_run_opts_default(&dflt); opts = &dflt; }
    if (!err) { err = ebuf; errlen = sizeof ebuf; }
    err[0] = 0;
    if (bad_slots) *bad_slots = 0;
    if (G > 1 && (rc = inputs_agree(ctx, method, procs, cb_nodes, data_size, rank_list, comm_size, iter, ntimes, opts,
                                    err, errlen)))
        return rc;
    rc = setup(ctx, &j, method, procs, cb_nodes, data_size, rank_list, comm_size, iter, ntimes, opts, err, errlen);
    if (G > 1) rc = agree_peers(ctx, rc, NULL, WHAT, err, errlen);  /* before the first call of the exchange */
    if (rc) goto out;
    agreed = 1;
    TRY(xg_barrier(ctx));                                   /* MPI_Barrier before total_start */
    TRY(xg_plan_run(j.plan, j.done, j.post, &wall));
    job_timers(&j, ctx, procs, timers, ntimes, opts);
    if (opts->verify) {
        int ns = xg_verify_slots(j.s, G, g, NULL);
        slots = (xg_slot *)malloc(sizeof(xg_slot) * (ns + 1));
        bad = (int64_t *)calloc(ns + 1, sizeof(int64_t));
        if (!slots || !bad) {
            snprintf(err, errlen, "verify: out of host memory");
            rc = XG_ENOMEM;
            goto out;
        }
        xg_verify_slots(j.s, G, g, slots);
        TRY(xg_verify(j.reg, slots, ns, data_size, iter, opts->fingerprint, NULL, bad, NULL));
        for (i = 0; i < ns; ++i)
            if (bad[i]) {
                if (nbad == 0) fprintf(stderr, "rank %d, message is wrong from rank %d\n", slots[i].dst, slots[i].src);
                ++nbad;
            }
        if (bad_slots) *bad_slots = nbad;
    }
out:
    /* a GPU that failed after the set-up (the run, the verify) tells its peers too: the caller's
     * next collective (the timer reduction) must not wait for it.  A run that failed inside RCCL
     * may leave the communicator unusable -- then this reports that error as well. */
    if (G > 1 && agreed) rc = agree_peers(ctx, rc, NULL, WHAT, err, errlen);
    if (rc && err[0] == 0) snprintf(err, errlen, "device error %d (see stderr)", rc);
    free(slots); free(bad);
    job_free(&j);
    return rc;
}

#define XG_METHOD_DEF(name, m)                                                                    \
    XG_METHOD_DECL(name)                                                                          \
    {                                                                                             \
        char e[512];                                                                              \
        int rc = xg_run_method(ctx, m, procs, cb_nodes, data_size, rank_list, comm_size, timers,  \
                               iter, ntimes, NULL, NULL, e, sizeof e);                            \
        if (rc == XG_ESCHED) fprintf(stderr, "%s: %s\n", #name, e);                               \
        return rc;                                                                                \
    }
XG_METHOD_DEF(xg_all_to_many, 1)
XG_METHOD_DEF(xg_many_to_all, 2)
XG_METHOD_DEF(xg_all_to_many_balanced, 3)
XG_METHOD_DEF(xg_many_to_all_balanced, 4)
XG_METHOD_DEF(xg_many_to_all_benchmark, 5)
XG_METHOD_DEF(xg_all_to_many_sync, 6)
XG_METHOD_DEF(xg_all_to_many_half_sync, 7)
XG_METHOD_DEF(xg_all_to_many_benchmark, 8)
XG_METHOD_DEF(xg_all_to_many_pairwise, 9)
XG_METHOD_DEF(xg_many_to_all_pairwise, 10)
XG_METHOD_DEF(xg_many_to_all_half_sync, 11)
XG_METHOD_DEF(xg_all_to_many_half_sync2, 12)
XG_METHOD_DEF(xg_many_to_all_scattered, 14)
XG_METHOD_DEF(xg_all_to_many_balanced_control, 18)
XG_METHOD_DEF(xg_all_to_many_scattered_isend, 19)
XG_METHOD_DEF(xg_all_to_many_balanced_pre_send, 20)

int xg_all_to_many_scattered(xg_ctx *ctx, int procs, int cb_nodes, int data_size, int *rank_list, int comm_size,
                             int barrier_type, xg_timer *timers, xg_timer *rep_timers, int iter, int ntimes)
{
    xg_run_opts o;
    char e[512];
    int rc;
    xg_run_opts_default(&o);
    o.barrier_type = barrier_type;
    o.rep_timers = rep_timers;
    rc = xg_run_method(ctx, 13, procs, cb_nodes, data_size, rank_list, comm_size, timers, iter, ntimes, &o, NULL,
                       e, sizeof e);
    if (rc == XG_ESCHED) fprintf(stderr, "xg_all_to_many_scattered: %s\n", e);
    return rc;
}

static int run_with_proc_node(xg_ctx *ctx, int method, const char *name, int procs, int cb_nodes, int data_size,
                              int *rank_list, int comm_size, int proc_node, xg_timer *timers, int iter, int ntimes)
{
    xg_run_opts o;
    char e[512];
    int rc;
    xg_run_opts_default(&o);
    o.proc_node = proc_node;
    rc = xg_run_method(ctx, method, procs, cb_nodes, data_size, rank_list, comm_size, timers, iter, ntimes, &o, NULL,
                       e, sizeof e);
    if (rc == XG_ESCHED) fprintf(stderr, "%s: %s\n", name, e);
    return rc;
}

int xg_all_to_many_node_robin(xg_ctx *ctx, int procs, int cb_nodes, int data_size, int *rank_list, int comm_size,
                              int proc_node, xg_timer *timers, int iter, int ntimes)
{
    return run_with_proc_node(ctx, 17, "xg_all_to_many_node_robin", procs, cb_nodes, data_size, rank_list, comm_size,
                              proc_node, timers, iter, ntimes);
}

int xg_many_to_all_tam(xg_ctx *ctx, int procs, int cb_nodes, int data_size, int *rank_list, int comm_size,
                       int procs_node, xg_timer *timers, int iter, int ntimes)
{
    return run_with_proc_node(ctx, 16, "xg_many_to_all_tam", procs, cb_nodes, data_size, rank_list, comm_size,
                              procs_node, timers, iter, ntimes);
}

int xg_all_to_many_tam(xg_ctx *ctx, int procs, int cb_nodes, int data_size, int *rank_list, int comm_size,
                       int procs_node, xg_timer *timers, int iter, int ntimes)
{
    return run_with_proc_node(ctx, 15, "xg_all_to_many_tam", procs, cb_nodes, data_size, rank_list, comm_size,
                              procs_node, timers, iter, ntimes);
}
