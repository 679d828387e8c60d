/*
 * job.h -- one GPU's share of a method run (internal to libxg.so; methods.c): what xg_run_method and
 * xg_exchange / xg_exchange_v both do around their own regions.  In order:
 *   job_plan   the schedule, the pairing proof (G > 1), this GPU's device plan
 *   (the caller makes j->reg from j->dp->region_bytes: allocated and filled, or adopted)
 *   job_load   the host arrays, the plan upload, the step marks
 *   (the caller: xg_barrier, xg_plan_run(j->plan, j->done, j->post, ...))
 *   job_timers the Timer of every hosted logical rank
 *   job_free   everything above, j->reg included
 * None posts a collective call.  Uses only the entry points every device half has.
 */
#ifndef XG_JOB_H
#define XG_JOB_H

#include <stddef.h>
#include <stdint.h>

#include "xg.h"
#include "xg_sched.h"

#define JOB_LOCAL __attribute__((visibility("hidden")))

typedef struct {
    xg_sched *s;
    xg_devplan *dp;
    xg_regions *reg;        /* the caller's to make, job_free's to free */
    xg_plan *plan;
    double *done, *post;    /* xg_plan_run's step times */
} job;                      /* starts zeroed */

/* A G-GPU job's RCCL calls pair step by step as RCCL pairs them (xg_devplans_match over every GPU's
 * plan, calls.c), the calls listed with the self_max this process posts with (xg_self_max: the exact
 * lists enqueue_step hands RCCL).  -> XG_OK, XG_EARG (err says which call would not pair) or
 * XG_ENOMEM. */
JOB_LOCAL int job_pairing_ok(const xg_sched *s, int G, const xg_run_opts *opts, int64_t self_max, char *err,
                             size_t errlen);
/* lens: a length per (rank, aggregator) pair (xg_sched_build_v; ragged set, NULL refused there), else
 * data_size for every pair (xg_sched_build_iter).  -> XG_OK or the first error, err saying which. */
JOB_LOCAL int job_plan(job *j, xg_ctx *ctx, int method, int procs, int cb_nodes, int data_size, const int64_t *lens,
                       int ragged, const int *rank_list, int comm_size, int iter, int ntimes, const xg_run_opts *opts,
                       char *err, size_t errlen);
JOB_LOCAL int job_load(job *j, xg_ctx *ctx, char *err, size_t errlen);
/* after the run; timers and opts->rep_timers may be NULL */
JOB_LOCAL void job_timers(const job *j, xg_ctx *ctx, int procs, xg_timer *timers, int ntimes, const xg_run_opts *opts);
JOB_LOCAL void job_free(job *j);

#endif
