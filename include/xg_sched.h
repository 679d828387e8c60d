/*
 * xg_sched.h -- host-side (plain C, no HIP headers) half of the MI355X
 * aggregator-exchange framework.
 *
 * The reference (QiaoK/MPI-Asynchronous-Communication-Test, mpi_test.c) runs
 * one MPI process per rank; each method issues Irecv/Issend/Send/Recv/
 * Sendrecv/Waitall/Alltoallw calls.  Here every logical rank's program is
 * restated literally (same loops, same quirks), matched with MPI semantics,
 * and compiled into a list of device-wide STEPS: step s holds every segment
 * that can move once everything of steps < s is delivered (earliest-step
 * schedule; MPI eager protocol for small blocking sends).  Each GPU then
 * executes its share of each step as one gather/scatter kernel + one grouped
 * RCCL exchange (xg.h).
 *
 * Interfaces replaced (reference file:line):
 *   xg_aggregator_list  <- create_aggregator_list        mpi_test.c:1952-2006
 *   xg_sched_build      <- the body of each method       mpi_test.c:421-1950
 *                          (+ *_alltoall_translate :233-302; TAM m15/m16
 *                          :313-419 -> collective_write +
 *                          static_node_assignment, lustre_driver_test.c:359-429, :944-1309)
 *   xg_sched_rank_timer <- the MPI_Wtime brackets filling Timer   :25-31
 *   xg_summarize_results<- summarize_results             mpi_test.c:2068-2118
 */
#ifndef XG_SCHED_H
#define XG_SCHED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Timer of the reference, field order preserved (mpi_test.c:25-31): MPI_Reduce
 * reduces it as 5 doubles. */
typedef struct {
    double post_request_time;
    double send_wait_all_time;
    double recv_wait_all_time;
    double barrier_time;
    double total_time;
} xg_timer;

enum { XG_A2M = 0, XG_M2A = 1 };

/* One matched message (one d-byte segment; zero-length for the pairwise
 * methods' non-participating pairs).  sseg: index of the segment in the
 * sender's send buffer; dslot: index of the slot in the receiver's receive
 * buffer (-1 when the message lives elsewhere: TAM aggregation buffers).
 * sbuf/soff and dbuf/doff: where its bytes are read and written, as a region
 * (XG_BUF_SEND / RECV / SCRATCH) and a byte offset inside that rank's part of
 * it.  step: the device-wide step it moves in.  Self memcpy's of m3/m4/m6
 * (mpi_test.c:1473, :1646, :1714) and of TAM (lustre_driver_test.c:1069-1285)
 * are messages with src == dst and XG_MSG_COPY. */
typedef struct {
    int32_t src, sseg, dst, dslot;
    int64_t len;
    int32_t step;
    int32_t flags;
    int32_t sbuf, dbuf;       /* -1: host-side control data (XG_MSG_CTRL) */
    int64_t soff, doff;
} xg_msg;

#define XG_MSG_COPY 1
#define XG_MSG_COLL 2   /* part of an MPI_Alltoallw */
#define XG_MSG_CTRL 4   /* TAM size exchange (MPI_INT arrays): orders steps, moves no device bytes */

#define XG_MPICH_EAGER_LIMIT 65424   /* see DESIGN.md "blocking-send semantics" */

typedef struct xg_sched xg_sched;

/* create_aggregator_list (mpi_test.c:1952-2006).  Returns 0, or -1 for an
 * aggregator type the reference does not define. */
int xg_aggregator_list(int procs, int cb_nodes, int proc_node, int type, int *rank_list);

/* Label printed by summarize_results for a method (mpi_test.c:2186-2337), NULL if not 1..20. */
const char *xg_method_label(int method);
/* XG_A2M or XG_M2A (the buffer layout of the method); -1 if not 1..20. */
int xg_method_direction(int method);

/* Build the schedule of one method run (all `ntimes` repetitions), methods
 * 1..20.  proc_node (-p) matters to m17 (node_robin_map, :1116-1133) and to
 * m15/m16 (processes per node of static_node_assignment type 0); barrier_type
 * (-b) to m13.  The schedule of m15/m16 depends on the iteration (its tags
 * carry +100*iter): build it with xg_sched_build_iter.
 * eager_limit: blocking sends and Isends of <= eager_limit bytes complete
 * locally (XG_MPICH_EAGER_LIMIT reproduces the reference on the image's MPICH).
 * Returns NULL and writes a message into err on failure, e.g. when the
 * programs deadlock under MPI semantics (the reference hangs there too). */
xg_sched *xg_sched_build(int method, int procs, int cb_nodes, int64_t data_size, int comm_size,
                         const int *rank_list, int ntimes, int proc_node, int barrier_type,
                         int64_t eager_limit, char *err, size_t errlen);
xg_sched *xg_sched_build_iter(int method, int procs, int cb_nodes, int64_t data_size, int comm_size,
                              const int *rank_list, int ntimes, int proc_node, int barrier_type,
                              int64_t eager_limit, int iter, char *err, size_t errlen);
/* The same with a length per (rank, aggregator) pair, as MPI_Alltoallv counts would give them.
 * lens[r * cb_nodes + a]: bytes between logical rank r and aggregator index a (a2m: r sends them to
 * rank_list[a]; m2a: rank_list[a] sends them to r).  >= 0; 0 = an empty segment.
 * A matrix whose entries all equal d IS the schedule xg_sched_build_iter builds with d (messages,
 * steps, traces, layout, device plans; xg_sched_ragged is 0).  Otherwise the schedule is RAGGED:
 * every post and self copy of the method carries its own segment's length, and the layout is dense
 * -- a rank's SEND part is its segments back to back in segment order, its RECV part its slots back
 * to back in slot order (xg_seg_offset / xg_slot_offset: prefix sums of the lengths).  A zero-length
 * segment behaves as zero-length messages do in the uniform schedules (Alltoallw and the scattered
 * methods post nothing for it, the pairwise methods a 0-byte Sendrecv).  Methods 1..14 and 17..20;
 * m15 / m16 (TAM) return NULL for a matrix that is not uniform. */
xg_sched *xg_sched_build_v(int method, int procs, int cb_nodes, const int64_t *lens, int comm_size,
                           const int *rank_list, int ntimes, int proc_node, int barrier_type,
                           int64_t eager_limit, int iter, char *err, size_t errlen);
void xg_sched_free(xg_sched *s);
int xg_sched_ragged(const xg_sched *s);                               /* 1: lengths differ */
/* byte offset of segment `seg` inside the rank's SEND part / of slot `slot` inside its RECV part
 * (seg / slot may equal the count: the part's size); -1 when the rank has no such part or the index
 * is out of range */
int64_t xg_seg_offset(const xg_sched *s, int rank, int seg);
int64_t xg_slot_offset(const xg_sched *s, int rank, int slot);

int xg_sched_nmsg(const xg_sched *s);
const xg_msg *xg_sched_msgs(const xg_sched *s);
int xg_sched_nsteps(const xg_sched *s);
int xg_sched_direction(const xg_sched *s);
int xg_sched_procs(const xg_sched *s);

/* Canonical MPI call trace of one logical rank (same token format as the
 * PMPI capture in tests/golden/); returns the length written (truncated to
 * buflen-1) or the needed length if buf is NULL.  Pairwise m9/m10 above P = 1024
 * (or with XG_PAIRWISE_FAST=1) are planned in a fast form that leaves out the
 * 0-byte MPI_Sendrecv rounds: their trace is then NOT the reference's call trace
 * (same byte-carrying posts, other completions; tests/test_host_sched.py). */
size_t xg_sched_trace(const xg_sched *s, int rank, char *buf, size_t buflen);

/* Per-rank timer from device step timestamps (ranks block-mapped on ngpus):
 *   step_done[s]  seconds from the timed-region start until step s completed
 *                 on the GPU that hosts `rank`;
 *   step_post[s]  host seconds spent enqueuing step s on that GPU (may be NULL);
 *                 it is shared out over the requests that GPU's ranks post in s.
 * Each reference timer bracket (MPI_Wtime pairs) becomes an interval of the
 * rank's logical clock, which advances at completion points to the step
 * completion time of the awaited messages; a post bracket adds the share of
 * enqueue time of the requests it posts. */
int xg_sched_rank_timer(xg_sched *s, int ngpus, int rank, const double *step_done,
                        const double *step_post, xg_timer *out);
/* timers[m] of every repetition (m13, mpi_test.c:829-874; zero for other methods):
 * reps has xg_sched_ntimes(s) entries. */
int xg_sched_rank_rep_timers(xg_sched *s, int ngpus, int rank, const double *step_done,
                             const double *step_post, xg_timer *reps);
int xg_sched_ntimes(const xg_sched *s);
/* The steps whose completion time some rank's Timer reads (need[nsteps]: 1 = read; the last
 * step always is).  Every other step may be timed as the next read step without changing any
 * Timer field (a run then marks only these: xg_plan_set_step_marks).  -> how many. */
int xg_sched_timed_steps(const xg_sched *s, uint8_t *need);
/* step after which the k-th MPI_Barrier of the method completes (-1: before step 0);
 * returns the number of barriers (out may be NULL). */
int xg_sched_barrier_epochs(const xg_sched *s, int32_t *out);

/* ---------------------------------------------------------------- device plan
 * Block mapping of logical ranks onto G GPUs: gpu(r) = r / ceil(P/G).
 * Buffers of GPU g (byte offsets inside four regions):
 *   XG_BUF_SEND  send segments of its ranks (a2m: each local rank A segs;
 *                m2a: each local aggregator rank P segs), rank-major
 *   XG_BUF_RECV  receive slots (a2m: each local aggregator rank P slots;
 *                m2a: each local rank A slots), rank-major
 *   XG_BUF_STAGE_SEND / XG_BUF_STAGE_RECV  packed per-peer staging
 *   XG_BUF_SCRATCH  TAM aggregation buffers of its ranks (aggregate_buf,
 *                send_buf2, recv_buf of collective_write), rank-major
 */
enum { XG_BUF_SEND = 0, XG_BUF_RECV = 1, XG_BUF_STAGE_SEND = 2, XG_BUF_STAGE_RECV = 3, XG_BUF_SCRATCH = 4,
       XG_NBUF = 5 };

typedef struct {
    int64_t src_off, dst_off, len;
    int32_t src_buf, dst_buf;
} xg_copy;

typedef struct {
    int64_t off, len;
    int32_t peer, buf;
    int32_t is_send;
    int32_t group;                    /* RCCL group of the step: 0, or 1 (relay form: the forwards) */
} xg_p2p;

typedef struct {
    int32_t pre_begin, pre_count;     /* local copies + packs   (before the exchange) */
    int32_t p2p_begin, p2p_count;     /* grouped RCCL send/recv                       */
    int32_t post_begin, post_count;   /* unpacks                (after the exchange)  */
    int32_t sync_after;               /* 1: device-side barrier of all GPUs after it  */
    int32_t stage_count;              /* the first stage_count pre copies (rank-local
                                         memcpy's through SCRATCH) run in a launch of
                                         their own, ahead of the other pre copies     */
    int32_t posts;                    /* request posts (Isend/Irecv/... ) the GPU's ranks
                                         make in this step: a graph replay shares its
                                         launch time out in proportion (xg_plan_run)  */
} xg_stepplan;

/* What a valid xg_devplan means, whoever built it (xg_plan_load takes any).  Steps run in order.
 * Inside a step four phases run in order: the stage copies; the other pre copies (local copies,
 * then packs); the p2p groups (group 0, then group 1); the post copies (unpacks).  The copies of
 * one phase, and the calls of one p2p group, are simultaneous: none writes bytes another of the
 * same phase reads or writes.  Phases and steps may depend on each other in any way -- read
 * after write, write after write with other bytes, write after read -- and the runtime, which
 * merges and overlaps phases where a host predicate (xg_engine_hazards, xg_engine_rail_safe,
 * xg_step_*_meet*) finds them independent, must leave every region as that order leaves it.
 * One limit: a step's LOCAL copies may run beside its own p2p groups and unpacks (on the side
 * stream, or inside the RCCL group), so they touch no byte those write and write none those read.
 * tests/dep_plan.py executes exactly these semantics on numpy regions. */
#define XG_DP_RAGGED 1               /* xg_devplan.flags bit 0: built from a ragged schedule */
#define XG_DP_EXTENTS 2              /* bit 1: a placement plan (xg_place_plan_build): launches of many
                                        short copies, which the runtime may run on copy_kernel_x */
typedef struct {
    int32_t gpu, ngpus, nsteps, flags;
    int64_t region_bytes[XG_NBUF];    /* send, recv, stage_send, stage_recv, scratch  */
    int32_t ncopy, np2p;
    xg_copy *copies;
    xg_p2p *p2p;
    xg_stepplan *steps;
    int64_t local_bytes, remote_send_bytes, remote_recv_bytes;   /* per whole plan  */
} xg_devplan;

/* Ranks hosted by GPU g: [*lo, *hi). */
void xg_block_range(int procs, int ngpus, int g, int *lo, int *hi);
int xg_gpu_of(int procs, int ngpus, int rank);

/* Region sizes and per-rank region offsets (-1 if the rank has no such buffer
 * on that GPU). */
int64_t xg_send_offset(const xg_sched *s, int ngpus, int rank);
int64_t xg_recv_offset(const xg_sched *s, int ngpus, int rank);
int64_t xg_scratch_offset(const xg_sched *s, int ngpus, int rank);
int64_t xg_region_bytes(const xg_sched *s, int ngpus, int g, int buf);

/* Build GPU g's share of every step.  pack_max_seg: per (step, peer), pack the
 * segments into one staging buffer when there are >= 2 and their mean length
 * is < pack_max_seg (0 = never pack); otherwise one RCCL op per segment. */
xg_devplan *xg_devplan_build(const xg_sched *s, int ngpus, int g, int64_t pack_max_seg);
/* The same, packing a (step, peer) transfer list only when it also moves >= pack_min bytes
 * (smaller lists go one RCCL call per segment: cheaper than a pack and an unpack launch). */
xg_devplan *xg_devplan_build_ex(const xg_sched *s, int ngpus, int g, int64_t pack_max_seg, int64_t pack_min);
/* The same with the form of a packed list chosen (the two above use XG_PACK_FORM_DEFAULT):
 *   XG_PACK_TWO_SIDED  one staging buffer per peer per direction: the sender packs every
 *                      segment, one RCCL call, the receiver unpacks every segment;
 *   XG_PACK_ONE_SIDED  the list in destination (or source) order, merged into runs that are
 *                      contiguous there: one RCCL call per run, straight into (out of) the
 *                      slots; only the runs not contiguous on the other side are staged, by
 *                      the sender (or the receiver) -- each byte copied on one side at most.
 *                      Of the two orders the one with fewer copied bytes + XG_RUN_CALL_BYTES
 *                      per call; ties: destination order (devplan.c, oneside).
 * One-sided halves the copied bytes but posts more calls (configs[2] on 8 GPUs: 2 per peer and
 * direction instead of 1).  On one MI355X, where a virtual 8-GPU job moves every pair as an
 * RCCL self send/recv and those serialize at ~3 us per call, two-sided is the faster form
 * (profiles/r03/pack_forms/), so it is the default; bench.py times direct, one-sided and
 * two-sided per method at N > 1 and keeps the fastest.  Any other form value means
 * XG_PACK_FORM_DEFAULT.  The alltoallw translate this replaces: mpi_test.c:233-302. */
/*   XG_RELAY           no packing; two-phase (Valiant) routing of the steps it pays for: each
 *                      cross-GPU message of such a step is cut into G 16-B aligned pieces; pieces
 *                      0 and 1 go straight to the destination (piece 0 in the step's first RCCL
 *                      group, piece 1 in its second), piece 2 + i through relay GPU R[i] (the G - 2
 *                      GPUs other than source and destination, ascending): received into the
 *                      relay's STAGE_RECV in the first group, forwarded in the second.  Every link
 *                      (a -> h) then carries egress(a) / G in group 0 and every link (h -> b)
 *                      ingress(b) / G in group 1, whatever the traffic matrix.  A step is relayed
 *                      when (max egress + max ingress) / G <= XG_RELAY_GAIN x its busiest GPU pair's
 *                      bytes and every cross-GPU message is >= XG_RELAY_MIN_BYTES: pairwise m9 / m10
 *                      (one XOR partner per round, 16 -> 4 MiB of link time per round at configs[3]),
 *                      configs[4]'s half-sync m11.  Other steps: direct.  No copy kernel touches a
 *                      relayed byte (link-load table).
 *   XG_RELAY_COALESCED the relay form's steps, pieces and hops (the same link load), with each
 *                      hop's pieces gathered into one call: group 0, per peer h, one call for the
 *                      pieces that end at h and one for those h relays (by destination); group 1,
 *                      per peer b, one call for this GPU's own second pieces and one per source
 *                      whose pieces it forwards to b.  A call of one piece moves in place; a longer
 *                      one is packed into STAGE_SEND / unpacked out of STAGE_RECV.  Pairwise rounds:
 *                      G - 1 sends + G - 1 receives per group, where XG_RELAY posts a call per
 *                      piece (RCCL's per-call cost: profiles/r06/relay_cost.log).  A step the
 *                      uniform cut does not help may take a weighted two-hop split instead
 *                      (Frank-Wolfe per step, shares in 1/1024ths of each GPU pair) when that
 *                      carries <= 0.85 of its busiest pair's bytes: configs[4]'s m7. */
enum { XG_PACK_TWO_SIDED = 0, XG_PACK_ONE_SIDED = 1, XG_RELAY = 2, XG_RELAY_COALESCED = 3 };
#define XG_PACK_FORM_DEFAULT XG_PACK_TWO_SIDED
#define XG_RUN_CALL_BYTES (1 << 20)
#define XG_RELAY_MIN_BYTES (1 << 20)
#define XG_RELAY_GAIN 0.8
xg_devplan *xg_devplan_build_form(const xg_sched *s, int ngpus, int g, int64_t pack_max_seg, int64_t pack_min,
                                  int form);
/* All three return NULL (nothing leaked) when the host runs out of memory while building: every
 * rank of a job builds plans, and xg_run_method turns a NULL on any rank into an error all ranks
 * agree on before any of them posts a call.  xg_devplan_free(NULL) is a no-op. */
void xg_devplan_free(xg_devplan *p);

/* ---------------------------------------------------------------- RCCL calls (calls.c)
 * The calls GPU dp->gpu posts in step `step`, in issue order: its send/recv calls
 * (one ncclGroupStart/End around them; a relay step's second group follows an
 * XG_CALL_FENCE), then XG_CALL_BARRIER (one ncclAllReduce)
 * when the step ends in an in-loop MPI_Barrier.  self_max > 0: a step that posts
 * cross-GPU calls and whose local gather/scatter copies move <= self_max bytes
 * posts those copies inside the same group as self send/recv pairs (peer = dp->gpu,
 * send then receive per copy; xg_devplan_step_self_calls counts them, 0 = the copies
 * stay copy-kernel launches) -- one RCCL launch then carries the whole step.  The
 * runtime posts exactly this list (replaces the Issend/Irecv/Sendrecv/Alltoallw
 * posts, mpi_test.c:1776,1790, :551,558, :627,912).  Returns the count (out may be
 * NULL), -1 for a bad step. */
enum { XG_CALL_SEND = 1, XG_CALL_RECV = 2, XG_CALL_BARRIER = 3, XG_CALL_FENCE = 4 };
typedef struct {
    int32_t kind, peer, buf, pad;     /* peer: GPU; buf: region (XG_BUF_*) */
    int64_t off, len;
} xg_call;
int xg_devplan_step_calls(const xg_devplan *dp, int step, int64_t self_max, xg_call *out);
int xg_devplan_step_self_calls(const xg_devplan *dp, int step, int64_t self_max);

/* RCCL's pairing of the calls of a G-GPU job: per ordered GPU pair (src, dst), the
 * k-th send of src to dst with the k-th receive of dst from src, in issue order
 * over the WHOLE run (RCCL's per-peer FIFO knows no steps).  calls[g] / step_begin[g]
 * (nsteps + 1 entries): GPU g's calls and where each step's start.  Accepted only if
 * every pair falls in one step and one group of it (groups: separated by XG_CALL_FENCE)
 * with one length and every GPU ends the same steps with a barrier (each its step's
 * last call) -- then no group can wait for one a peer posts later.  Returns the number
 * of pairs, written in (step, group) order (inside a group by src, dst, k) to out when
 * max_pairs suffices; -1 and a reason in err otherwise. */
typedef struct {
    int32_t step, src, dst;
    int32_t send_call, recv_call;     /* indices into calls[src] / calls[dst] */
    int32_t group;                    /* the step's RCCL group both calls are in */
    int64_t len;
} xg_call_pair;
int64_t xg_calls_match(int ngpus, int nsteps, const xg_call *const *calls, const int32_t *const *step_begin,
                       xg_call_pair *out, int64_t max_pairs, char *err, size_t errlen);
/* The same over the G device plans of one job (plans[g]: GPU g's, same schedule), their
 * calls listed with self_max as xg_devplan_step_calls lists them. */
int64_t xg_devplans_match(const xg_devplan *const *plans, int ngpus, int64_t self_max, xg_call_pair *out,
                          int64_t max_pairs, char *err, size_t errlen);

/* Step engine ordering (xg.h xg_plan_engine; kernels.h step_engine_kernel).  The
 * transfers of step s are xfer[step_begin[s] .. step_begin[s+1]) (device addresses
 * as integers).  flags[s] says what the barrier after step s orders:
 *   2  step s+1 reads bytes written since the last hazard point, or rewrites them
 *      with other bytes (another source at another dst-src offset): stores drained
 *      + agent release/acquire, and no early load of step s+1;
 *   1  stores drained before arriving (the last step; every step with force);
 *   0  nothing (identical rewrites of the -k repetitions are not hazards).
 * Returns the number of hazard points (flag 2). */
typedef struct { uint64_t src, dst, len; } xg_span;
int xg_engine_hazards(const xg_span *xfer, const int *step_begin, int nsteps, int force, int *flags);
/* May these steps run on the solo engine's rails, which never wait for each other (no
 * ordering between steps at all, unlike the grid engine's barrier)?  1 if no transfer's
 * source range meets the destination range of a transfer of another step, in either step
 * order -- so write-after-read, which gets no flag above, is excluded too; 0 otherwise.
 * A rail segment needs this AND no hazard point. */
int xg_engine_rail_safe(const xg_span *xfer, const int *step_begin, int nsteps);

/* Solo engine tables of one hazard-free run of steps (xg.h XG_SOLO_RAILS; kernels.h
 * solo_engine_kernel, whose constants must equal these).  Pieces of <= XG_SOLO_PIECE
 * bytes, every transfer 16-B aligned and within XG_SOLO_OFF_MAX 16-B units of
 * src_base / dst_base; dealt round-robin over rails = min(rails_max, pieces / waves, >= 1).
 * Per rail r, npieces descriptors at descs[r * npieces]: bits 0-23 source offset,
 * 24-47 destination offset (16-B units from the bases), 48-54 length (16-B units;
 * 0 = empty padding), 55-59 `before` = how many of its row's step barriers precede
 * it.  meta: [rails][nrows + 1] barriers per row (rows of `waves` pieces), then
 * [rails][nsteps] the step each barrier closes, in order, -1 past the last (a rail
 * places a barrier only after a step it had pieces in, in front of its next piece),
 * then [rails] the rows that hold real pieces (the rest is padding, never executed).
 * descs / meta NULL: fill *shape only.  Returns 0, or XG_EARG (xg.h) for bad input or
 * npieces > XG_SOLO_MAX_PIECES (*shape still filled), XG_ENOMEM. */
#define XG_SOLO_WAVES 16         /* waves of a workgroup rail; `waves` = 1: every rail one wave */
#define XG_SOLO_MAX_RAILS 512
#define XG_SOLO_PIECE 1024
#define XG_SOLO_K 8
#define XG_SOLO_MAX_STEPS 2048
#define XG_SOLO_MAX_PIECES 4608
#define XG_SOLO_OFF_MAX (1ull << 24)
/* waves = 1 (one-wave rails): the WIDE form -- descriptor = src | dst << 32 (granules, so
 * windows of XG_SOLO_WIDE_OFF_MAX granules), and each row's meta word = barrier count (bits
 * 0-7, all preceding the row's one piece) | the piece's length in granules << 8. */
#define XG_SOLO_WIDE_OFF_MAX (1ull << 32)
typedef struct { int32_t rails, npieces, nrows, nmeta; } xg_solo_shape;
int xg_solo_tables(const xg_span *xfer, const int *step_begin, int nsteps, int rails_max, int waves,
                   uint64_t src_base, uint64_t dst_base, xg_solo_shape *shape, uint64_t *descs, int *meta);
/* The same with offsets and lengths in units of `granule` bytes (16, 4 or 1; 4 and 1 only
 * for one-wave rails): every transfer granule-aligned, offsets within XG_SOLO_OFF_MAX
 * granules of the bases; bits 0-23 source, 24-47 destination offset, then the length
 * (7, 9 or 11 bits: up to XG_SOLO_PIECE bytes), then `before` at XG_SOLO_BEFORE_SHIFT.
 * Segment sizes that are not multiples of 16 (any -d) run on 4-B or 1-B accesses. */
#define XG_SOLO_BEFORE_SHIFT(g) ((g) == 16 ? 55 : (g) == 4 ? 57 : 59)
int xg_solo_tables_g(const xg_span *xfer, const int *step_begin, int nsteps, int rails_max, int waves, int granule,
                     uint64_t src_base, uint64_t dst_base, xg_solo_shape *shape, uint64_t *descs, int *meta);
/* Step times of a solo segment [s0, s1) from its rails' stamps (stamps[r * stride + t], 0 =
 * the rail closed nothing there): out[t] = max over rails of the rail's latest stamp <= t. */
void xg_solo_reduce_stamps(const uint64_t *stamps, int rails, int64_t stride, int s0, int s1, uint64_t *out);
/* last[rails]: each rail's last step with pieces under the deal of xg_solo_tables_g (-1: none). */
int xg_solo_rail_last(const xg_span *xfer, const int *step_begin, int nsteps, int rails, int32_t *last);
/* Before the reduction: the kernel writes a rail's closing stamp to EVERY step behind the rail's
 * last barrier, which closes the last step but one it has pieces in.  In the steps between that
 * one and last[r] the rail had nothing: their stamps are zeroed here, so that the reduction carries
 * the rail's previous stamp (else the time of a heavy last step lands on the first step some rail
 * sat out before it).  cstep: the tables' [rails][n] closed steps of a segment of n steps whose
 * first step's stamp is stamps[r * stride + s0]. */
void xg_solo_carry_tail(uint64_t *stamps, int rails, int64_t stride, int s0, int n, const int *cstep,
                        const int32_t *last);
/* step_done[nsteps], seconds from a run's start, from the wall-clock stamps it left (ticks of
 * wall_hz; every difference is taken in 64 bits, so a wrapped counter is harmless).  The one
 * place where stamps become times: xg_plan_run, its armed form and xg_vplans_run all call it.
 *   marks[nsteps + 1]     marks[0] the start's mark, marks[s + 1] the mark behind step s
 *   chain_stamps[nsteps]  step t's stamp, written by the first workgroup of launch t + 1 (the
 *                         chain's last by a clock kernel); NULL: the run stamped no chain
 *   engine_stamps[nsteps] the engine's stamp of step t (solo segments already reduced over their
 *                         rails, xg_solo_reduce_stamps); NULL: a plan without segments
 *   seg_of[nsteps], seg_end[]   step s's engine segment (-1: none), and each segment's end s1
 *   chain_end[nsteps]     != 0 at a chain's first step: the chain's end; NULL: no chains
 *   need_mark[nsteps]     != 0: a step outside segments and chains was marked; NULL: all were
 * A chain [s, ce) is anchored at marks[ce], a segment [s, e) at marks[e], both BACKWARDS:
 * step_done[t] = end - (stamp[last] - stamp[t]) / wall_hz, the last step's = end; a time that
 * would fall before the run's start is reported as 0.  A marked step outside both ends at its
 * mark; one that was not marked when the next marked step does (no Timer reads it, and the last
 * step is always marked).  host_total >= 0 (an armed run, xg.h XG_ENGINE_ARM): ONE segment
 * covers every step and is anchored at host_total, the host-measured seconds from the ring to
 * the engine's completion; the marks and the tables may then be NULL.  host_total < 0: none.
 * What a time means: an engine stamp before its segment's last is an ISSUE time (the step's
 * loads are over, its stores may still land); a segment's last stamp, a chain stamp (the next
 * launch starts when the step's own has ended) and a mark are DELIVERED times.
 * Returns 0 (also for nsteps == 0, whatever the pointers) or XG_EARG. */
int xg_step_times(int nsteps, const uint64_t *marks, const uint64_t *chain_stamps, const uint64_t *engine_stamps,
                  const int32_t *seg_of, const int32_t *seg_end, const int32_t *chain_end, const uint8_t *need_mark,
                  double wall_hz, double host_total, double *step_done);

/* Piece (= workgroup) size of one copy launch over copies of lengths lens[n]: among chunk,
 * chunk/2, ... >= 4 KiB (16-B multiples), the one whose busiest CU -- ceil(pieces / cus)
 * pieces of (size + wg_cost) bytes -- has the least work; ties keep the larger (pieces.c). */
int64_t xg_piece_size(const int64_t *lens, int n, int64_t chunk, int cus, int64_t wg_cost);
/* 1 if a local gather/scatter copy of step s (after its stage copies, before its packs)
 * reads or writes bytes that step s-1's unpacks write -- then the two may not share one copy
 * launch; 0 if they may; -1 for a bad step (pieces.c). */
int xg_step_local_meets_unpacks(const xg_devplan *dp, int s);
/* The same for step s's packs: 1 if one reads bytes that step s-1's unpacks write (it forwards
 * received bytes: a pack's source may lie in any region) or writes such bytes; 0 if packs and
 * unpacks may share one copy launch; -1 for a bad step (pieces.c). */
int xg_step_packs_meet_unpacks(const xg_devplan *dp, int s);
/* 1 if a pre copy of step s after its stage copies (local gather/scatter, packs) reads or writes
 * bytes a stage copy writes, or writes bytes one reads -- then the stage copies keep a launch of
 * their own; 0 if all may share one launch; -1 for a bad step (pieces.c). */
int xg_step_stage_meets_rest(const xg_devplan *dp, int s);
/* Tiles of one copy_kernel_x dispatch over the ordered pieces of lengths lens[n] (one workgroup per
 * tile): a tile is a maximal run of consecutive pieces with at most tile_pieces pieces and at most
 * tile_bytes bytes; a single piece longer than tile_bytes is a tile of its own.  Tile t is pieces
 * [begin[t], begin[t + 1]).  Returns the tile count (0 for n <= 0; -1 for a cap < 1); begin has
 * count + 1 entries and may be NULL to query (pieces.c). */
int xg_extent_tiles(const int64_t *lens, int n, int64_t tile_bytes, int tile_pieces, int32_t *begin);

/* Small-piece launches (copy_kernel_q, kernels.h): a UNIFORM launch -- `copies` copies of `len`
 * bytes each, listed one table row per copy -- in pieces of `piece` bytes, one workgroup per piece,
 * with no per-piece table: workgroup b finds its piece by arithmetic.  ppc = ceil(len / piece)
 * pieces per copy, copies * ppc workgroups in all (< 2^31: the callers check).  The copies are
 * taken in groups of k consecutive rows (the last group may be shorter): inside a group the
 * workgroups go round the group's copies piece by piece -- workgroup r of a group of kk copies
 * serves the group's copy r % kk, piece r / kk -- so k = 1 is plain row order.  A copy's last
 * piece holds the rest of it (n <= piece).  The same function runs in the kernel (every operand
 * is workgroup-uniform) and on the host (dispatch byte counts, tests); libxghost exports both
 * (pieces.c holds their external definitions). */
#if defined(__HIPCC__)
#define XG_HD __host__ __device__
#else
#define XG_HD
#endif
typedef struct { uint32_t copy; int64_t off, n; } xg_small_at;
inline XG_HD uint32_t xg_small_ppc(int64_t len, int64_t piece) { return (uint32_t)((len + piece - 1) / piece); }
inline XG_HD xg_small_at xg_small_index(uint32_t b, uint32_t copies, int64_t len, int64_t piece, uint32_t k)
{
    const uint32_t gs = k * xg_small_ppc(len, piece);      /* workgroups of a full group */
    const uint32_t g = b / gs, r = b - g * gs;
    const uint32_t left = copies - g * k, kk = left < k ? left : k;
    const uint32_t j = r / kk;
    xg_small_at a;
    a.copy = g * k + (r - j * kk);
    a.off = (int64_t)j * piece;
    a.n = len - a.off < piece ? len - a.off : piece;
    return a;
}
/* xg_small_index for callers that cannot inline it (pieces.c); returns 0, or -1 when b is not a
 * workgroup of the launch or an argument is out of range. */
int xg_small_piece_at(int64_t b, int64_t copies, int64_t len, int64_t piece, int k, int64_t *copy, int64_t *off,
                      int64_t *n);

/* The step engines' launch counters (kernels.h EngineState).  Every counter is
 * a cumulative 32-bit word in device memory that no launch resets: a launch is told what the
 * launches before it added (a BASE the host keeps) and compares the word with base + its own share,
 * by difference or by equality, in uint32_t arithmetic -- which agrees with the word modulo 2^32
 * whatever the divisor, so nothing here changes when a counter passes 2^31 or 2^32.  The same
 * functions run in the kernels (every "which value do I wait for / am I the last" decision there is
 * one of these) and on the host; pieces.c holds their external definitions, and
 * tests/test_engine_counters.py walks them across the wrap.
 *
 * Grid engine (step_engine_kernel), counter `count`: one ticket per workgroup and barrier.  A
 * launch of W workgroups over n steps takes xg_eng_grid_tickets of them: an armed launch passes one
 * more barrier, in front of step 0, whose target xg_eng_grid_pre_target is also the base of its
 * steps; the barrier behind step s opens at xg_eng_grid_target.  A workgroup whose ticket (the
 * counter after its own increment) is the target arrived last; the others wait while
 * xg_eng_waiting.  (The counter then reads at most W - 1 past the target: workgroups that went on
 * to the next barrier.) */
inline XG_HD uint32_t xg_eng_grid_tickets(uint32_t W, uint32_t nsteps, int armed)
{
    return (nsteps + (armed ? 1u : 0u)) * W;
}
inline XG_HD uint32_t xg_eng_grid_pre_target(uint32_t base, uint32_t W) { return base + W; }
inline XG_HD uint32_t xg_eng_grid_target(uint32_t base, uint32_t W, uint32_t s) { return base + (s + 1u) * W; }
inline XG_HD int xg_eng_waiting(uint32_t count, uint32_t target) { return (int32_t)(count - target) < 0; }
inline XG_HD int xg_eng_last(uint32_t ticket, uint32_t target) { return ticket == target; }
/* Solo engine (solo_engine_kernel), ARMED launches of R rails only; base = the armed launches of
 * the segment since the state was last zeroed.  `arrive` counts resident rails: rail 0 announces
 * `ready` once the word reaches xg_eng_solo_arrive_target (waiting while xg_eng_waiting).  Finished
 * rails count on XG_ENG_LINES lines, rail r on line r % L with L = xg_eng_solo_lines(R);
 * line l holds xg_eng_solo_per_line(R, l) rails.  The rail whose increment of fin[l] gives a has
 * xg_eng_solo_line_last: it counts on `rails`, and the one whose increment there gives b with
 * xg_eng_solo_rails_last is the launch's last rail to finish. */
#define XG_ENG_LINES 16
inline XG_HD uint32_t xg_eng_solo_lines(uint32_t R) { return R < XG_ENG_LINES ? R : XG_ENG_LINES; }
inline XG_HD uint32_t xg_eng_solo_per_line(uint32_t R, uint32_t line)
{
    return (R - line - 1u) / xg_eng_solo_lines(R) + 1u;
}
inline XG_HD uint32_t xg_eng_solo_arrive_target(uint32_t base, uint32_t R) { return (base + 1u) * R; }
inline XG_HD int xg_eng_solo_line_last(uint32_t a, uint32_t base, uint32_t R, uint32_t line)
{
    return a == (base + 1u) * xg_eng_solo_per_line(R, line);
}
inline XG_HD int xg_eng_solo_rails_last(uint32_t b, uint32_t base, uint32_t R)
{
    return b == (base + 1u) * xg_eng_solo_lines(R);
}
/* The solo words as `armed` armed launches of R rails leave them from a zeroed state: go = the
 * last launch's epoch on every relay line (pieces.c; xg.h xg_plan_engine_preset writes these). */
typedef struct { uint32_t arrive, rails, go, fin[XG_ENG_LINES]; } xg_eng_solo_state;
void xg_eng_solo_state_after(uint32_t R, uint32_t armed, xg_eng_solo_state *out);

/* The kernel of one copy launch (pieces.c).  A launch of bytes > 0 runs exactly one KIND, chosen
 * once at plan load from what the launch is (facts) and the context's knobs (rules), by this
 * precedence:
 *   1. EXTENT (copy_kernel_x): a placement plan (XG_DP_EXTENTS), extent_copy on, chunk <= 16 MiB,
 *      bytes <= npos * extent_mean_max (short copies).  Pieces by xg_piece_size.
 *   2. WAVE (copy_kernel_w<kib>): cross, wave_min <= bytes <= wave_max, everything 16-B aligned, the
 *      cut plain (!nt_cut).  Pieces of kib KiB: wave_kib if forced, else by bytes and cus (8 / 4 /
 *      2).  When the run is non-temporal all the same (nt_run; they differ in one launch, the local +
 *      pack launch of a step whose packs are all empty) the kind is PIECE over those wave-sized pieces.
 *   3. SHIFT (copy_kernel_s): a ragged plan (XG_DP_RAGGED), ragged_copy on, an offset or length off
 *      the 16-B grid.  Pieces by xg_piece_size.
 *   4. PIECE (copy_kernel_g<4>) otherwise.  Pieces by xg_piece_size.
 *   5. SMALL (copy_kernel_q<kib / 4>) replaces PIECE only: may_small, small_pieces on, aligned,
 *      bytes >= small_piece_min, uniform_len > 0, and npos * ppc and small_order * ppc within
 *      INT32_MAX (ppc = pieces per copy; xg_small_index works in 32 bits).  kib = small_kib, order =
 *      small_order; the launch has rows, no pieces.
 * nt is nt_run in every case (WAVE is reached only with a plain run). */
enum { XG_COPY_PIECE = 0, XG_COPY_WAVE, XG_COPY_SHIFT, XG_COPY_EXTENT, XG_COPY_SMALL, XG_COPY_NKIND };
typedef struct {
    int64_t bytes, npos;        /* over the positive copies: their bytes, their number ...            */
    uint64_t bits;              /* ... the OR of their offsets and lengths (the alignment bits) ...    */
    int64_t uniform_len;        /* ... and their common length; -1 once two differ or one packs or     */
                                /* unpacks (dst STAGE_SEND / src STAGE_RECV); 0 before the first       */
    const int64_t *lens;        /* every copy's length, for xg_piece_size                              */
    int32_t nlens;
    int32_t dp_flags;           /* the plan's XG_DP_*                                                  */
    int32_t cross;              /* a launch of a cross-GPU step, or of a local step too large for the engine */
    int32_t may_small;          /* a step's own local (+ pack) launch                                  */
    int32_t nt_cut, nt_run;     /* non-temporal by the runtime's copy_variant: for the cut, for the kernel */
} xg_launch_facts;
typedef struct {
    int64_t chunk;              /* default bytes per piece (xg_set_copy_params)                        */
    int64_t wave_min, wave_max; /* WAVE from .. to this many bytes (XG_COPY_WAVE_MIN; kWaveMax)        */
    int64_t wg_cost;            /* xg_piece_size's per-workgroup start (kWgCost)                       */
    int64_t extent_mean_max;    /* EXTENT up to this mean positive length (kExtMeanMax)                */
    int64_t small_piece_min;    /* SMALL from this many bytes (kSmallMin; XG_SMALL_PIECE_MIN)          */
    int32_t cus;                /* compute units                                                       */
    int32_t wave_kib;           /* XG_WAVE_KIB: 2 / 4 / 8 forced, 0 = by launch bytes                  */
    int32_t ragged_copy;        /* 0 (XG_RAGGED_COPY=0): no SHIFT                                      */
    int32_t extent_copy;        /* 0 (XG_EXTENT_COPY=0): no EXTENT                                     */
    int32_t small_pieces;       /* 0 (XG_SMALL_PIECES=0): no SMALL                                     */
    int32_t small_kib;          /* SMALL's piece size, 4 or 8 KiB (kSmallKiB; XG_SMALL_PIECE_KIB)      */
    int32_t small_order;        /* copies per group of its piece order (xg_small_index's k)            */
} xg_copy_rules;
typedef struct {
    int32_t kind, nt;
    int32_t kib;                /* WAVE: 2 / 4 / 8; SMALL: 4 / 8; else 0                               */
    int32_t order;              /* SMALL: xg_small_index's k; else 0                                   */
    int64_t piece;              /* bytes per piece the launch's copies are cut to (SMALL: by the kernel) */
} xg_copy_choice;
/* one copy of the launch into zeroed facts (lens / nlens and the six fields below them are the caller's) */
void xg_launch_facts_add(xg_launch_facts *f, const xg_copy *c);
/* 0, or -1 for a NULL argument or a launch without bytes (it has no kernel) */
int xg_copy_launch_choose(const xg_launch_facts *f, const xg_copy_rules *r, xg_copy_choice *out);

/* ---------------------------------------------------------------- placement (place.c)
 * Where the segments of an exchange lie in the aggregators' collective buffers (ROMIO's
 * others_req[i].offsets / lens): a list of n extents describes the whole job, and every rank
 * passes the same list.  Extent e: len bytes of pair (rank, aggregator INDEX agg) at byte `off` of
 * aggregator agg's domain.  The extents of one pair, in list order, carry consecutive bytes of that
 * pair's segment, so their lengths sum to the pair's length; len == 0 is allowed and ignored; a
 * pair with no extent has length 0. */
typedef struct { int32_t rank, agg; int64_t off, len; } xg_ext;
/* lens[r * cb_nodes + a] (the matrix xg_sched_build_v takes) = sum of the pair's extent lengths.
 * XG_EARG (xg.h) for a rank or aggregator out of range, a negative length or a sum past int64. */
int xg_exts_lens(const xg_ext *exts, int64_t n, int procs, int cb_nodes, int64_t *lens);
/* dom_bytes[a]: the length of aggregator a's domain.  XG_EARG with a reason in err for a rank or
 * aggregator out of range, a negative off or len, off + len > dom_bytes[agg] (or past int64), a
 * negative domain length, and -- scatter != 0, the collective write, where two writers to one byte
 * have no defined result -- two positive extents of one aggregator that overlap (a sort per
 * aggregator).  A gather (scatter == 0) may read a byte twice.  XG_ENOMEM; XG_OK. */
int xg_exts_check(const xg_ext *exts, int64_t n, int procs, int cb_nodes, const int64_t *dom_bytes, int scatter,
                  char *err, size_t errlen);
/* A GPU's domain buffer: its hosted aggregators' domains back to back, unpadded, in the order
 * their RECV (a2m) / SEND (m2a) parts have (by aggregator rank).  xg_domain_offset: where
 * aggregator index a's domain starts in its GPU's buffer (-1: a out of range); xg_domain_bytes:
 * GPU g's buffer size. */
int64_t xg_domain_offset(const xg_sched *s, int ngpus, int a, const int64_t *dom_bytes);
int64_t xg_domain_bytes(const xg_sched *s, int ngpus, int g, const int64_t *dom_bytes);
/* GPU g's placement plan: one step of pre copies, one per positive extent of the aggregators it
 * hosts, in list order; no p2p; flags = XG_DP_RAGGED | XG_DP_EXTENTS.  s is the exchange's schedule
 * (xg_sched_build_v over xg_exts_lens' matrix).  a2m (scatter, after the exchange): region SEND is
 * the exchange's dense RECV layout -- an extent's source is xg_recv_offset(aggregator rank) +
 * xg_slot_offset(aggregator rank, rank) + the bytes of the pair's earlier extents -- and region
 * RECV is the domain buffer.  m2a (gather, before the exchange): SEND is the domain buffer, RECV
 * the exchange's dense SEND layout (xg_send_offset + xg_seg_offset + ...).  Only those two entries
 * of region_bytes are set.  The list must have passed xg_exts_check; NULL on out of memory (or a
 * list that names a rank or aggregator out of range). */
xg_devplan *xg_place_plan_build(const xg_sched *s, int ngpus, int g, const xg_ext *exts, int64_t n,
                                const int64_t *dom_bytes);

/* ---------------------------------------------------------------- strided runs (vecs.c)
 * The same placement described by STRIDED RUNS, the form a regular file view has (MPI_Type_vector /
 * MPI_Type_create_subarray: each rank's block of a global array, interleaved row by row with the
 * other ranks' blocks): a few numbers per (rank, aggregator) pair instead of one xg_ext per row.
 * Vec v: `count` blocks of `len` bytes of pair (rank, aggregator INDEX agg), block j at byte
 * off + j * stride of aggregator agg's domain.  The vecs of one pair, in list order, and within a
 * vec the blocks in order of j, carry consecutive bytes of the pair's segment.  A vec with len == 0
 * or count == 0 is allowed and ignored (its other fields are not looked at, negative ones aside); a
 * vec with count == 1 is an xg_ext and its stride is not looked at.  Every rank passes the same list. */
typedef struct { int32_t rank, agg; int64_t off, len, stride, count; } xg_vec;
/* The extent list a vec list means -- one xg_ext per block of every positive vec (len > 0 and
 * count > 0), in order: the DEFINITION of the semantics and the tests' oracle; xg_exchange_w takes its
 * output.  Nothing else here calls it (it is O(blocks)).  Returns the count
 * (out may be NULL to query it; at most cap are written), -1 for a negative len, count or (count > 1)
 * stride, a count that does not fit int64 or an offset past int64. */
int64_t xg_vecs_expand(const xg_vec *v, int64_t n, xg_ext *out, int64_t cap);
/* lens[r * cb_nodes + a] += count * len over the positive vecs (= xg_exts_lens of the expansion).
 * XG_EARG for a positive vec's rank or aggregator out of range, a negative len or count, a product
 * or a sum past int64. */
int xg_vecs_lens(const xg_vec *v, int64_t n, int procs, int cb_nodes, int64_t *lens);
/* Accepts and refuses what xg_exts_check accepts and refuses for the expansion, naming the same kind
 * of fault in err ("out of range", "negative", "overflow", "past the domain end", "overlap"), without
 * ever building the expansion: O(n) extra memory, bounds from a vec's last block in O(1).  It also
 * refuses a negative count, a negative stride (count > 1) and off + (count - 1) * stride + len past
 * int64.  A gather (scatter == 0) may read a byte twice: any stride >= 0 passes, 0 included.  A
 * scatter finds every pair of overlapping blocks: inside a vec (stride < len with count > 1), and
 * between the vecs of one aggregator -- sorted by hull [off, off + (count - 1) * stride + len); a vec
 * whose hull meets no other is done; a cluster of meeting hulls whose vecs all have count > 1 and one
 * common stride S is accepted without walking a block when their circular intervals [off mod S,
 * off mod S + len) are pairwise disjoint on the circle of S (the striped view); any other cluster is
 * walked block by block in ascending order (a k-way merge through a binary heap, one block per vec in
 * memory), each block against the one before.  XG_EARG / XG_ENOMEM / XG_OK. */
int xg_vecs_check(const xg_vec *v, int64_t n, int procs, int cb_nodes, const int64_t *dom_bytes, int scatter,
                  char *err, size_t errlen);
/* One table row of a strided placement -- what a copy kernel that derives every block by arithmetic
 * reads in place of a descriptor per block (copy_kernel_v):
 * `count` blocks of `len` bytes, block j from src_off + j * src_step of region src_buf to
 * dst_off + j * dst_step of region dst_buf. */
typedef struct { int32_t src_buf, dst_buf; int64_t src_off, dst_off, src_step, dst_step, len, count; } xg_vrow;
/* GPU g's rows: one per positive vec of the aggregators it hosts, in list order (vec_index[k]: row
 * k's list index; may be NULL), at the offsets xg_place_plan_build gives the expansion's copies --
 * the dense side advances by len per block from the pair's dense offset plus the bytes of the pair's
 * earlier vecs, the domain side by stride from xg_domain_offset + off (count == 1: both steps 0).
 * a2m: the dense side is SEND, the domain RECV; m2a the other way round.  region_bytes (XG_NBUF
 * entries, may be NULL) as xg_place_plan_build sets them.  Returns the row count (rows may be NULL to
 * query it), -1 for bad arguments or a list that names a rank or aggregator out of range.  The list
 * must have passed xg_vecs_check. */
int64_t xg_vec_rows_build(const xg_sched *s, int ngpus, int g, const xg_vec *v, int64_t n, const int64_t *dom_bytes,
                          xg_vrow *rows, int64_t *vec_index, int64_t *region_bytes);
/* Tile arithmetic of a row table, host and device code alike as xg_small_index is (pieces.c holds
 * the external definitions): how a row's blocks are dealt to workgroups, one TILE of a row each.
 * Blocks of len <= tile_bytes go
 * bpt = clamp(tile_bytes / len, 1, tile_pieces) to a tile, lane i of tile t taking block t * bpt + i;
 * a longer block is cut into ceil(len / tile_bytes) pieces of tile_bytes (the last one shorter), one
 * piece per tile, lane 0's.  All offsets and products are 64-bit.  xg_vec_row_tiles: a row's tile
 * count (0 for len <= 0 or count <= 0; INT64_MAX when it does not fit). */
inline XG_HD int64_t xg_vec_bpt(int64_t len, int64_t tile_bytes, int tile_pieces)
{
    const int64_t b = tile_bytes / len;
    return b < 1 ? 1 : b > tile_pieces ? tile_pieces : b;
}
inline XG_HD int64_t xg_vec_row_tiles(int64_t len, int64_t count, int64_t tile_bytes, int tile_pieces)
{
    if (len <= 0 || count <= 0 || tile_bytes < 1 || tile_pieces < 1) return 0;
    if (len <= tile_bytes) {
        const int64_t bpt = xg_vec_bpt(len, tile_bytes, tile_pieces);
        return count / bpt + (count % bpt != 0);
    } else {
        const int64_t ppb = len / tile_bytes + (len % tile_bytes != 0);
        return ppb > INT64_MAX / count ? INT64_MAX : ppb * count;
    }
}
/* Piece i (lane i) of tile t of a row: n bytes from src_off to dst_off; n = 0 past the tile's last
 * piece.  t in [0, xg_vec_row_tiles), i in [0, tile_pieces). */
typedef struct { int64_t src_off, dst_off, n; } xg_vec_at;
inline XG_HD xg_vec_at xg_vec_piece_at(int64_t src_off, int64_t dst_off, int64_t src_step, int64_t dst_step,
                                          int64_t len, int64_t count, int64_t tile_bytes, int tile_pieces, int64_t t,
                                          int i)
{
    xg_vec_at p;
    p.src_off = p.dst_off = p.n = 0;
    if (len <= tile_bytes) {
        const int64_t bpt = xg_vec_bpt(len, tile_bytes, tile_pieces);
        const int64_t j = t * bpt + i;
        if (i < bpt && j < count) {
            p.src_off = src_off + j * src_step;
            p.dst_off = dst_off + j * dst_step;
            p.n = len;
        }
    } else if (i == 0) {
        const int64_t ppb = len / tile_bytes + (len % tile_bytes != 0);
        const int64_t j = t / ppb, o = (t - j * ppb) * tile_bytes;
        p.src_off = src_off + j * src_step + o;
        p.dst_off = dst_off + j * dst_step + o;
        p.n = len - o < tile_bytes ? len - o : tile_bytes;
    }
    return p;
}
/* xg_vec_piece_at for callers that cannot inline it, range-checked: 0, or -1 when t is no tile of the
 * row, i no lane of a tile or an argument is out of range (pieces.c). */
int xg_vec_piece(const xg_vrow *row, int64_t tile_bytes, int tile_pieces, int64_t t, int i, int64_t *src_off,
                 int64_t *dst_off, int64_t *n);
/* tile0[k] = the tiles of rows [0, k): n + 1 entries (tile0 may be NULL).  Returns the total, or -1
 * when it passes INT32_MAX (a launch's workgroups are counted in 32 bits) or an argument is bad. */
int64_t xg_vec_rows_tiles(const xg_vrow *rows, int64_t n, int64_t tile_bytes, int tile_pieces, int32_t *tile0);

/* ---------------------------------------------------------------- views (vecs.c)
 * A VIEW is a set of k >= 1 rows of one GPU's xg_vrow list that are one striped file view: the same
 * src_buf and dst_buf, the same len, count, src_step and dst_step, len <= tile_bytes, and offsets on
 * one side -- the STRIPED side -- exactly len apart from row to row (the other, dense, side may sit
 * anywhere).  A tile dealt across the rows of a view (xg_view_piece_at) writes (dst-striped, the a2m
 * scatter) or reads (src-striped, the m2a gather) k x len contiguous bytes per block index where a
 * tile of one row touches len.
 * xg_vrow_views finds them, O(n log n) time and O(n) memory: the row indices sorted by (bufs, len,
 * count, steps, destination offset, source offset, list index) are chained where the destination
 * offsets are len apart; the rows that chained with nothing are sorted once more with the source
 * offset ahead of the destination's and chained by it (a chain that qualifies both ways is
 * dst-striped).  The rows of a view need not be neighbours in the list.  A chain longer than
 * kmax = min(tile_pieces, max(1, tile_bytes / len)) is cut into consecutive views of kmax rows, the
 * last one shorter; a row that chains with nothing, one with len > tile_bytes and one with len <= 0
 * or count <= 0 is a view of k = 1.  Views come in the order of their first rows in the first sort,
 * so two lists that are permutations of each other give the same views.
 * order: n row indices, the views' rows one view behind the other, each in ascending striped offset;
 * view_k: rows per view; view_kind: XG_VIEW_* per view (either may be NULL).  Returns the view count,
 * -1 for bad arguments or no memory. */
enum { XG_VIEW_SINGLE = 0, XG_VIEW_DST_STRIPED = 1, XG_VIEW_SRC_STRIPED = 2 };
int64_t xg_vrow_views(const xg_vrow *rows, int64_t n, int64_t tile_bytes, int tile_pieces, int64_t *order,
                      int32_t *view_k, int32_t *view_kind);
/* Tile arithmetic of a view of k rows, host and device code alike (pieces.c holds the external
 * definitions).  len <= tile_bytes: jb = clamp(tile_bytes / (k x len), 1, tile_pieces / k) blocks per
 * row go to a tile, ceil(count / jb) tiles; lane q of tile t takes row i = q % k (the fastest index:
 * a tile's pieces ascend on the striped side) and block j = t x jb + q / k, and is live when
 * q < k x jb and j < count.  With k = 1 this is xg_vec_piece_at's deal exactly.  len > tile_bytes
 * (k = 1): that function's long-block deal, lane 0 takes piece t.  64-bit throughout but for the
 * division by k; xg_view_tiles is INT64_MAX when it does not fit, 0 for a bad argument. */
inline XG_HD int64_t xg_view_jb(int64_t len, int k, int64_t tile_bytes, int tile_pieces)
{
    const int64_t b = tile_bytes / ((int64_t)k * len), hi = tile_pieces / k;
    return b > hi ? (hi < 1 ? 1 : hi) : b < 1 ? 1 : b;
}
inline XG_HD int64_t xg_view_tiles(int64_t len, int64_t count, int k, int64_t tile_bytes, int tile_pieces)
{
    if (len <= 0 || count <= 0 || k < 1 || tile_bytes < 1 || tile_pieces < 1) return 0;
    if (len <= tile_bytes) {
        const int64_t jb = xg_view_jb(len, k, tile_bytes, tile_pieces);
        return count / jb + (count % jb != 0);
    }
    return xg_vec_row_tiles(len, count, tile_bytes, tile_pieces);
}
/* Lane q of tile t of a view whose rows have blocks of len bytes, count of them, and go jb to a
 * tile: n bytes (0: the lane is idle) at byte `off` of block `block` of the view's row `row`, that is
 * at the row's own offsets + block x step + off on either side. */
typedef struct { int32_t row, pad; int64_t block, off, n; } xg_view_at;
inline XG_HD xg_view_at xg_view_piece_at(int64_t len, int64_t count, int k, int64_t jb, int64_t tile_bytes, int64_t t,
                                         int q)
{
    xg_view_at p;
    p.row = p.pad = 0;
    p.block = p.off = p.n = 0;
    if (len <= tile_bytes) {
        const uint32_t uq = (uint32_t)q, uk = (uint32_t)k, b = uq / uk;       /* 32-bit: k is uniform */
        const int64_t j = t * jb + b;
        if ((int64_t)b < jb && j < count) {
            p.row = (int32_t)(uq - b * uk);
            p.block = j;
            p.n = len;
        }
    } else if (q == 0) {
        const int64_t ppb = len / tile_bytes + (len % tile_bytes != 0);
        p.block = t / ppb;
        p.off = (t - p.block * ppb) * tile_bytes;
        p.n = len - p.off < tile_bytes ? len - p.off : tile_bytes;
    }
    return p;
}
/* xg_view_piece_at over the k rows of a view (rows[0 .. k), in view order), range-checked: 0 and
 * *row, the offsets and *n of lane q of tile t, or -1 when the rows are no view of k (len, count or a
 * step differs, k does not fit a tile), t is no tile of it, q no lane of a tile or an argument is out
 * of range (pieces.c). */
int xg_view_piece(const xg_vrow *rows, int k, int64_t tile_bytes, int tile_pieces, int64_t t, int q, int *row,
                  int64_t *src_off, int64_t *dst_off, int64_t *n);

/* fill: `nsegs` consecutive d-byte segments at `off` in the SEND region,
 * segment i = fingerprint(rank, seed0 + i, iter) (prepare_*_data loops). */
typedef struct { int32_t rank, seed0; int64_t off; int32_t nsegs, pad; } xg_segrun;
/* verify: one d-byte receive slot at `off` in the RECV region that must hold
 * fingerprint(src, seed, iter); dst is the receiving logical rank. */
typedef struct { int32_t src, seed, dst, pad; int64_t off; } xg_slot;

enum { XG_FP_REFERENCE = 0, XG_FP_STRONG = 1 };   /* fingerprint modes */

/* Fill/verify descriptors of GPU g (host side, from the schedule's layout).
 * Return the count; out may be NULL to query it. */
int xg_fill_runs(const xg_sched *s, int ngpus, int g, xg_segrun *out);
int xg_verify_slots(const xg_sched *s, int ngpus, int g, xg_slot *out);

/* Every receive slot of the job and the send segment it must equal after the run (any method
 * 1..20, TAM included: what check_buffer's call sites :139 / :215 pair), whatever the bytes are:
 * slot `slot` of rank dst, at recv_off in dst_gpu's RECV, holds the d bytes at send_off =
 * xg_send_offset(src) + seed * d of src_gpu's SEND.  Ordered by (dst_gpu, xg_verify_slots order).
 * Returns the count; out may be NULL to query it. */
typedef struct { int32_t src, seed, dst, slot, src_gpu, dst_gpu; int64_t send_off, recv_off; } xg_delivery;
int xg_deliveries(const xg_sched *s, int ngpus, xg_delivery *out);
/* The length of every delivery, in xg_deliveries' order (d for a uniform schedule, the pair's own
 * length for a ragged one).  Returns the count; out may be NULL to query it. */
int xg_delivery_lens(const xg_sched *s, int ngpus, int64_t *out);

/* save_all_timing (mpi_test.c:2008-2066): the four per-repetition CSVs of m13,
 * <prefix>send_wait_all_times_<c>.csv, total_times, post_request_time,
 * barrier_time; timers = procs x ntimes, rank-major. */
int xg_save_all_timing(int procs, int ntimes, int comm_size, const xg_timer *timers, const char *prefix);

/* ---------------------------------------------------------------- report
 * summarize_results (mpi_test.c:2068-2118): 8 "| ..." lines on stdout and one
 * appended row (header on first write) in `filename`. */
int xg_summarize_results(int procs, int cb_nodes, int data_size, int comm_size, int ntimes,
                         int type, const char *filename, const char *prefix,
                         xg_timer timer1, xg_timer max_timer1);

/* ---------------------------------------------------------------- plan tables (plan_tables.cc)
 * What xg_plan_load makes of a device plan before it touches the device -- the piece, launch,
 * dispatch-cut, tile and row tables, the displacement fix-ups, the engine segments and the chains --
 * is host arithmetic over the plan, the knobs below and the regions' bases and sizes.  The runtime
 * calls the builder inside xg_plan_load; this group lets a test call it with no GPU.
 * xg_plan_knobs: every context setting the builder reads (the runtime's context holds one, filled
 * by xg_init from the device and the environment). */
typedef struct xg_plan_knobs {
    xg_copy_rules rules;       /* what decides each copy launch's kernel and piece size (xg_copy_launch_choose) */
    int64_t extent_tile;       /* bytes per copy_kernel_x tile */
    int64_t engine_max_step;   /* GPU-local steps of <= this many bytes may be engine steps; 0: no step engine */
    int64_t solo_max;          /* solo segments move <= this many bytes per run */
    int64_t launch_max;        /* copy launches above 1.5 x this many bytes go as dispatches of ~this size; 0: never */
    int64_t split_min;         /* a cross-GPU step's local part of >= this many bytes runs on the side stream */
    int64_t self_max;          /* ... of <= this many bytes goes in the step's RCCL group */
    int32_t variant;           /* copy kernel variant: 0 by size, 1 plain, 6 non-temporal */
    int32_t engine_wmax;       /* at most this many (co-resident) grid-engine workgroups */
    int32_t engine_drain;      /* 1: drain before every barrier arrival */
    int32_t solo;              /* 0: never the solo engine */
    int32_t solo_rails;        /* solo segments deal their pieces over up to this many rails */
    int32_t solo_waves;        /* waves per rail: 16 (a workgroup) or 1 */
    int32_t wave_grid;         /* copy_kernel_w workgroups resident at once */
    int32_t step_chain;        /* 1: chains of one-launch local steps */
    int32_t engine_arm;        /* 1: single-segment plans may be armed */
    int32_t fuse_stage;        /* 1: stage copies join the step's local launch when hazard-free */
    int32_t split_after_pack;  /* 1: a split step's local part forks after its pack launch */
    int32_t rank, nranks;      /* this GPU of how many */
    int32_t virt;              /* 1: one of nranks GPUs emulated on one device */
} xg_plan_knobs;
/* What xg_init sets with an empty environment on a device of `cus` compute units that admits
 * engine_occ co-resident step-engine workgroups and wave_grid copy_kernel_w workgroups; rank 0 of 1. */
void xg_plan_knobs_default(xg_plan_knobs *k, int cus, int engine_occ, int wave_grid);
/* Apply the XG_* plan knobs found in env to k (already filled by xg_plan_knobs_default): the one
 * place that reads them (xg_init calls it).  env: NULL-terminated array of
 * "NAME=value" strings, first match of a name wins, as getenv; NULL: the process environment.
 * Messages go to stderr: a refused XG_COPY_VARIANT, and, once per process, every retired knob
 * still set. */
void xg_plan_knobs_env(xg_plan_knobs *k, const char *const *env);
/* The names it reads, in a fixed order; returns their number (out may be NULL). */
int xg_plan_knob_names(const char **out, int cap);
/* Build the tables of dp for regions of bytes[b] bytes at address base[b].  XG_EARG (with the
 * runtime's message on stderr) for a descriptor outside its region or a tile table that does not
 * cover its pieces; *out is then NULL. */
typedef struct xg_plan_tables xg_plan_tables;
int xg_plan_tables_build(const xg_devplan *dp, const xg_plan_knobs *k, const uint64_t base[XG_NBUF],
                         const int64_t bytes[XG_NBUF], xg_plan_tables **out);
void xg_plan_tables_free(xg_plan_tables *t);
/* The introspection of a loaded plan (xg.h: xg_plan_nsteps .. xg_plan_engine_steps forward here). */
int xg_plan_tables_nsteps(const xg_plan_tables *t);
int xg_plan_tables_launches(const xg_plan_tables *t);
int xg_plan_tables_step_form(const xg_plan_tables *t, int s);
int xg_plan_tables_kind_launches(const xg_plan_tables *t, int kind);
int xg_plan_tables_wave_launches(const xg_plan_tables *t, int *grid, int *max_pieces_per_wave);
int xg_plan_tables_small_launches(const xg_plan_tables *t, int *kib);
int xg_plan_tables_shift_launches(const xg_plan_tables *t);
int xg_plan_tables_extent_launches(const xg_plan_tables *t);
int xg_plan_tables_engine(const xg_plan_tables *t);
int xg_plan_tables_engine_rails(const xg_plan_tables *t);
int xg_plan_tables_engine_steps(const xg_plan_tables *t, int *nseg, int *nhaz);
/* Every table as text, one record per line in a fixed order, every pointer as region+offset.
 * Returns the length (without the final NUL); at most cap bytes are written; buf may be NULL. */
int64_t xg_plan_tables_dump(const xg_plan_tables *t, char *buf, int64_t cap);

/* ---------------------------------------------------------------- row launch tables (vec_tables.cc)
 * What xg_vecplace_load (xg.h) makes of GPU g's xg_vrow list before it touches the device: everything
 * one copy_kernel_v launch reads, as host arithmetic over the rows and the regions' bases and sizes.
 *   device rows  {src, dst, src_step, dst_step, len, count} per row, the pointers absolute;
 *   tile0        rows + 1 entries, the prefix of xg_vec_row_tiles (xg_vec_rows_tiles);
 *   cuts         the launch's dispatches, as tile indices from 0: dispatch k runs tiles
 *                [cut k, cut k + 1).  A launch of more than 1.5 x launch_max bytes goes as dispatches
 *                of about launch_max bytes of whole tiles (launch_max <= each < launch_max + its last
 *                tile's bytes; a cut may fall inside a row), and no runt closes it: a remainder of
 *                fewer than 16 tiles or less than launch_max / 2 bytes joins the dispatch before it.
 *                launch_max == 0: one dispatch.  O(rows + cuts) time, whatever the rows' counts.
 * XG_EARG with a message on stderr (*out is then NULL) for a row with len <= 0 or count <= 0, a row
 * whose first or last block leaves its region on either side (in 64 bits; an offset or a byte total
 * that overflows int64 is refused as such), a region index out of range, more than INT32_MAX tiles,
 * tile_bytes < 1, tile_pieces outside 1 .. 256 or launch_max < 0.  n == 0 is XG_OK: no tile, no
 * dispatch.  XG_ENOMEM. */
typedef struct xg_vec_tables xg_vec_tables;
int xg_vec_tables_build(const xg_vrow *rows, int64_t n, const uint64_t base[XG_NBUF], const int64_t bytes[XG_NBUF],
                        int64_t tile_bytes, int tile_pieces, int64_t launch_max, xg_vec_tables **out);
void xg_vec_tables_free(xg_vec_tables *t);
int64_t xg_vec_tables_rows(const xg_vec_tables *t);
int64_t xg_vec_tables_tiles(const xg_vec_tables *t);
int xg_vec_tables_dispatches(const xg_vec_tables *t);
int64_t xg_vec_tables_bytes(const xg_vec_tables *t);                    /* the launch's bytes */
int64_t xg_vec_tables_cut(const xg_vec_tables *t, int k);               /* k in 0 .. dispatches; -1 outside */
int64_t xg_vec_tables_dispatch_bytes(const xg_vec_tables *t, int k);    /* k in 0 .. dispatches - 1; -1 outside */
/* Every table as text, one record per line, every pointer as region+offset, in the manner of
 * xg_plan_tables_dump: "vec rows .. tiles .. dispatches .. bytes .. tile_bytes .. tile_pieces ..
 * launch_max ..", then "row i src dst src_step dst_step len count", "tile0 i v", "cut i v",
 * "dbytes i v".  Returns the length (without the final NUL); at most cap bytes are written. */
int64_t xg_vec_tables_dump(const xg_vec_tables *t, char *buf, int64_t cap);

/* ---------------------------------------------------------------- view launch tables (vec_tables.cc)
 * What xg_vecplace_load_views (xg.h) makes of the same list: everything one copy_kernel_vv launch
 * reads, one workgroup per tile of one VIEW (xg_vrow_views, xg_view_piece_at).
 *   device rows  as above, permuted into view order (xg_vrow_views' order);
 *   views        {first device row, k, jb} per view;
 *   tile0        views + 1 entries, the prefix of xg_view_tiles;
 *   cuts         by the row tables' rule, word for word, over the views' tiles (a view's tile bytes
 *                are those of a row of blocks of k x len bytes, jb to a tile).  O(views + cuts) time.
 * The refusals are xg_vec_tables_build's (the row named is the list's), with more than INT32_MAX
 * tiles counted over the views.  n == 0 is XG_OK. */
typedef struct xg_view_tables xg_view_tables;
int xg_view_tables_build(const xg_vrow *rows, int64_t n, const uint64_t base[XG_NBUF], const int64_t bytes[XG_NBUF],
                         int64_t tile_bytes, int tile_pieces, int64_t launch_max, xg_view_tables **out);
void xg_view_tables_free(xg_view_tables *t);
int64_t xg_view_tables_rows(const xg_view_tables *t);
int64_t xg_view_tables_views(const xg_view_tables *t);                   /* all views */
int64_t xg_view_tables_multi(const xg_view_tables *t);                   /* ... those of k > 1 */
int64_t xg_view_tables_tiles(const xg_view_tables *t);
int xg_view_tables_dispatches(const xg_view_tables *t);
int64_t xg_view_tables_bytes(const xg_view_tables *t);
int64_t xg_view_tables_cut(const xg_view_tables *t, int k);              /* k in 0 .. dispatches; -1 outside */
int64_t xg_view_tables_dispatch_bytes(const xg_view_tables *t, int k);   /* k in 0 .. dispatches - 1; -1 outside */
int64_t xg_view_tables_order(const xg_view_tables *t, int64_t i);        /* the list index of device row i; -1 outside */
/* "views rows .. views .. multi .. tiles .. dispatches .. bytes .. tile_bytes .. tile_pieces ..
 * launch_max ..", then "row i src dst src_step dst_step len count" (device order), "order i list_index",
 * "view i row0 k jb kind", "tile0 i v", "cut i v", "dbytes i v", as xg_vec_tables_dump. */
int64_t xg_view_tables_dump(const xg_view_tables *t, char *buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
