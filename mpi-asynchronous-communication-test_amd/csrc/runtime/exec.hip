// exec.hip -- execution of a loaded plan: each step's entries of the plan's launch table and its
// RCCL groups, chains of stamped launches, engine segments, graph replay, armed (doorbell)
// runs, step marks.  Nothing here decides how a step's copies launch: xg_plan_load did.
#include "rt.h"

extern "C" const char *xg_debug_where(void)
{
    static char buf[160];
    snprintf(buf, sizeof buf, "%s: step %d of %d: %s", g_where.fn, g_where.step, g_where.nsteps, g_where.phase);
    return buf;
}

// Execution of one step on GPU g (xg_devplan, built by libxghost):
//   1. the step's launch-table entries up to its RCCL group: stage copies, local
//      gather/scatter, packs into the per-peer staging region (pre copies)
//   2. one ncclGroupStart .. ncclSend/ncclRecv .. ncclGroupEnd with the <= 7
//      peer GPUs this step talks to (xGMI)                  (p2p)
//   3. the entries behind it: staging unpacked into the receive slots (post)
//   4. a clock_kernel stamp (step mark) -- the reference's Waitall boundary
// All on one HIP stream per context, so step s+1 starts after step s; the
// cross-GPU order comes from RCCL send/recv matching.

// step boundary i of a run (-1: its start) on `stream`: a clock stamp (d_gstamp)
int mark(xg_plan *p, int i, hipStream_t stream)
{
    hipLaunchKernelGGL(xgk::clock_kernel, dim3(1), dim3(64), 0, stream, p->d_gstamp + i + 1);
    HIPCHK(hipGetLastError());
    return XG_OK;
}

// the run's step marks, after it: gs[i + 1] = boundary i's stamp, gs[0] the start's
int read_marks(const xg_plan *p, std::vector<unsigned long long> &gs)
{
    gs.resize((size_t)p->nsteps + 1);
    HIPCHK(hipMemcpy(gs.data(), p->d_gstamp, 8 * gs.size(), hipMemcpyDeviceToHost));
    return XG_OK;
}

// seconds from the run's start to boundary i
double mark_elapsed(const xg_plan *p, int i, const std::vector<unsigned long long> &gs)
{
    return (double)(gs[i + 1] - gs[0]) / p->ctx->wall_hz;
}

// Copy launches.  What a launch is -- its pieces, its ONE kernel kind (PIECE copy_kernel_g<4>,
// WAVE copy_kernel_w<2 / 4 / 8>, SHIFT copy_kernel_s, EXTENT copy_kernel_x, SMALL copy_kernel_q<1 /
// 2>; all but WAVE plain or non-temporal), its dispatches, its stream, the mark behind it -- was
// decided when the plan was loaded (CopyLaunch, host/plan_tables.h); here the table is walked.

// One dispatch of launch l: pieces [b, b + n) (SMALL: workgroups [b, b + n)), on the kernel of its
// kind.  The one exception: only the first dispatch of a cut WAVE launch runs copy_kernel_w; the
// later ones copy their pieces with copy_kernel_g<4>.
static int launch_one(xg_plan *p, const CopyLaunch &l, int b, int n, hipStream_t st, unsigned long long *start)
{
    const xgk::DCopy *pc = p->d_pieces + b;
    switch (l.kind) {
    case XG_COPY_SMALL: {
        // each workgroup finds its piece of the launch's rows
        const auto k = l.kib == 4 ? (l.nt ? xgk::copy_kernel_q<1, true> : xgk::copy_kernel_q<1, false>)
                                  : (l.nt ? xgk::copy_kernel_q<2, true> : xgk::copy_kernel_q<2, false>);
        hipLaunchKernelGGL(k, dim3(n), dim3(xgk::kThreads), 0, st, p->d_rows + l.q_row, (uint32_t)b,
                           (uint32_t)l.q_copies, l.q_len, (uint32_t)l.q_k, start);
        break;
    }
    case XG_COPY_EXTENT: {
        // one workgroup per tile of the dispatch (which one: by its first piece)
        int k = 0;
        while (k + 1 < l.ndisp && p->cuts[l.cut + k + 1] <= b) ++k;
        const auto kx = l.nt ? xgk::copy_kernel_x<true> : xgk::copy_kernel_x<false>;
        hipLaunchKernelGGL(kx, dim3(p->xt_n[l.xt + k]), dim3(xgk::kThreads), 0, st, pc, p->d_xt + p->xt_off[l.xt + k],
                           start);
        break;
    }
    case XG_COPY_SHIFT: {
        const auto k = l.nt ? xgk::copy_kernel_s<true> : xgk::copy_kernel_s<false>;
        hipLaunchKernelGGL(k, dim3(n), dim3(xgk::kThreads), 0, st, pc, start);
        break;
    }
    case XG_COPY_WAVE:
        if (b == l.b) {
            const auto k = l.kib == 2   ? xgk::copy_kernel_w<2>
                           : l.kib == 4 ? xgk::copy_kernel_w<4>
                                        : xgk::copy_kernel_w<xgk::kWaveKiB>;
            hipLaunchKernelGGL(k, dim3(wave_wgs(p, n)), dim3(xgk::kThreads), 0, st, pc, n, start);
            break;
        }
        [[fallthrough]];        // a later dispatch (nt is false)
    case XG_COPY_PIECE: {
        const auto k = l.nt ? xgk::copy_kernel_g<4, true> : xgk::copy_kernel_g<4>;
        hipLaunchKernelGGL(k, dim3(n), dim3(xgk::kThreads), 0, st, pc, start);
        break;
    }
    default:
        return XG_EARG;
    }
    HIPCHK(hipGetLastError());
    return XG_OK;
}

// kernel-timing session bookkeeping around one kernel dispatch of `bytes` copied bytes
static int kt_before(xg_ctx *c, hipStream_t stream, bool *kt)
{
    *kt = c->kt_mode == 1 && 2 * (size_t)c->nk + 1 < c->kev.size();
    if (*kt) HIPCHK(hipEventRecord(c->kev[2 * c->nk], stream));
    return XG_OK;
}

static int kt_after(xg_ctx *c, hipStream_t stream, bool kt, int64_t bytes)
{
    if (kt) {
        HIPCHK(hipEventRecord(c->kev[2 * c->nk + 1], stream));
        c->kbytes[c->nk] = 2 * bytes;      // algorithmic HBM bytes: read + write
    }
    if (kt || c->kt_mode == 2) {
        c->nk++;
        c->kt_bytes += 2 * bytes;
    }
    return XG_OK;
}

// One copy launch as its dispatches, each bracketed by kernel-timing events when a per-launch
// session is on.  start: the first dispatch stamps its start there (see copy_kernel_g).
static int launch_copy(xg_plan *p, const CopyLaunch &l, hipStream_t st, unsigned long long *start)
{
    const int *cut = p->cuts.data() + l.cut;
    int rc;
    for (int k = 0; k < l.ndisp; ++k) {
        const int64_t nb = l.kind == XG_COPY_SMALL ? p->qbytes[l.q_bytes + k]
                           : l.ndisp == 1          ? l.bytes
                                                   : p->plen[cut[k + 1]] - p->plen[cut[k]];
        bool kt;
        if ((rc = kt_before(p->ctx, st, &kt))) return rc;
        if ((rc = launch_one(p, l, cut[k], cut[k + 1] - cut[k], st, k == 0 ? start : nullptr))) return rc;
        if ((rc = kt_after(p->ctx, st, kt, nb))) return rc;
    }
    return XG_OK;
}

// step part 1: the step's launches up to its RCCL group.  A side-stream launch (a split
// step's local part) forks off `stream` and runs beside the packs and the RCCL group;
// enqueue_post joins it back before the step ends.  A launch that holds the previous
// step's unpacks ends that step: its mark, when marking, goes right behind it, and nothing
// of this step comes before it, so no message of this step lands before one of the previous.
// start: the step's first launch stamps its start there (chains).
int enqueue_pre(xg_plan *p, int s, hipStream_t stream, hipStream_t side, unsigned long long *start)
{
    const StepR &st = p->steps[s];
    int rc;
    for (int i = st.l_b; i < st.l_rccl; ++i) {
        const CopyLaunch &l = p->launches[i];
        if (l.side) {
            HIPCHK(hipEventRecord(p->fork[s], stream));
            HIPCHK(hipStreamWaitEvent(side, p->fork[s], 0));
        }
        if ((rc = launch_copy(p, l, l.side ? side : stream, i == st.l_b ? start : nullptr))) return rc;
        if (l.side) HIPCHK(hipEventRecord(p->join[s], side));
        if (l.mark_prev && p->rec_ev && p->need_mark[s - 1] && (rc = mark(p, s - 1, stream))) return rc;
    }
    return XG_OK;
}

// step part 3: the launches behind the RCCL group (the unpacks, unless deferred into the
// next step's launch), then wait for the forked local part
int enqueue_post(xg_plan *p, int s, hipStream_t stream)
{
    const StepR &st = p->steps[s];
    int rc;
    for (int i = st.l_rccl; i < st.l_e; ++i)
        if ((rc = launch_copy(p, p->launches[i], stream, nullptr))) return rc;
    for (int i = st.l_b; i < st.l_rccl; ++i)
        if (p->launches[i].side) HIPCHK(hipStreamWaitEvent(stream, p->join[s], 0));
    return XG_OK;
}

static int enqueue_step(xg_plan *p, int s)
{
    xg_ctx *c = p->ctx;
    const StepR &st = p->steps[s];
    int rc;
    if (c->virt && (st.p2p_n || st.sync_after) && !p->local_only) {
        fprintf(stderr, "xg: a virtual GPU's cross-GPU step runs only through xg_vplans_run\n");
        return XG_EARG;
    }
    if ((rc = enqueue_pre(p, s, c->stream, c->side))) return rc;
    if (p->local_only) return enqueue_post(p, s, c->stream);
    // the step's send/recv calls, in the order libxghost lists them (xg_devplan_step_calls), one
    // group per run of them between fences (a relay step: two, the second forwarding what the
    // first delivered to this GPU's staging -- stream order puts it behind the first); the
    // barrier call, if any, is the step's last and follows the unpacks
    const xg_call *cl = p->calls.data() + st.call_b;
    for (int i = 0; i < st.call_n && st.p2p_n;) {
        int e = i;
        while (e < st.call_n && (cl[e].kind == XG_CALL_SEND || cl[e].kind == XG_CALL_RECV)) ++e;
        if (e > i && (rc = rccl_group(
                          e - i,
                          [&](int k) {
                              const xg_call &o = cl[i + k];
                              uint8_t *ptr = p->reg->ptr[o.buf] + o.off;
                              return o.kind == XG_CALL_SEND
                                         ? ncclSend(ptr, (size_t)o.len, ncclUint8, o.peer, c->comm, c->stream)
                                         : ncclRecv(ptr, (size_t)o.len, ncclUint8, o.peer, c->comm, c->stream);
                          },
                          st.groups > 1 ? "relay step exchange" : "step exchange")))
            return rc;
        i = e + 1;            // past the fence (or the barrier, which ends the list)
    }
    if ((rc = enqueue_post(p, s, c->stream))) return rc;
    if (st.sync_after)   /* in-loop MPI_Barrier: every GPU finishes this step before any goes on */
        NCCLCHK(ncclAllReduce(c->d_red, c->d_red, 1, ncclFloat64, ncclMax, c->comm, c->stream));
    return XG_OK;
}

// one launch of the step engine over segment g (armed: waits for the doorbell `epoch`)
int launch_seg(xg_plan *p, const EngSeg &g, hipStream_t stream, bool armed)
{
    xg_ctx *c = p->ctx;
    int rc;
    if (p->engine_reset) {
        HIPCHK(hipMemsetAsync(p->d_engine, 0, sizeof(xgk::EngineState), stream));
        p->engine_base = p->solo_base = 0;
        p->engine_reset = false;
    }
    const int n = g.s1 - g.s0;
    xgk::Doorbell *db = armed ? p->db : nullptr;
    const unsigned epoch = armed ? ++p->epoch : 0;
    // what the launches before this one added to the state's counters (xg_sched.h xg_eng_*)
    const unsigned base = g.solo ? p->solo_base : p->engine_base;
    if (!g.solo) p->engine_base += xg_eng_grid_tickets((unsigned)g.w, (unsigned)n, db != nullptr);
    else if (db) ++p->solo_base;
    bool kt;
    if ((rc = kt_before(c, stream, &kt))) return rc;
    unsigned long long *stamps = reinterpret_cast<unsigned long long *>(p->d_engine + 1) + g.s0;
    const int *sb = p->d_sb + g.sb_off;
    if (g.solo) {
        // one-wave rails by granule (granule 1: 16 registers per piece and lane, half the rows
        // per chunk), or workgroup rails
        const auto k = g.wv != 1     ? xgk::solo_engine_kernel<xgk::kSoloK, xgk::kSoloWaves>
                       : g.gran == 16 ? xgk::solo_engine_kernel<xgk::kSoloK, 1>
                       : g.gran == 4  ? xgk::solo_engine_kernel<xgk::kSoloK, 1, 4>
                                      : xgk::solo_engine_kernel<xgk::kSoloK / 2, 1, 1>;
        hipLaunchKernelGGL(k, dim3(g.w), dim3(g.wv != 1 ? xgk::kSoloThreads : 64), 0, stream, p->d_solo + g.u0,
                           g.npieces, g.sbase, g.dbase, sb, n, p->d_engine, stamps, p->nsteps, db, epoch, base);
    } else {
        const auto k = g.b == 1   ? xgk::step_engine_kernel<1>
                       : g.b == 4 ? xgk::step_engine_kernel<4>
                                  : xgk::step_engine_kernel<16>;
        hipLaunchKernelGGL(k, dim3(g.w), dim3(xgk::kThreads), 0, stream, p->d_epieces, sb, n, p->d_engine, stamps,
                           base, db, epoch);
    }
    HIPCHK(hipGetLastError());
    return kt_after(c, stream, kt, g.bytes);
}

// every engine step's stamp (wall-clock ticks), after a synchronised run: grid
// segments stamp once per step; a solo segment's rails each stamp the steps they
// closed (0 elsewhere), so a rail's stamp of step t is its latest at or before t
// and the step's is the MAX over rails
int read_stamps(const xg_plan *p, std::vector<unsigned long long> &st)
{
    const size_t n = (size_t)p->nsteps;
    std::vector<unsigned long long> all(n * p->stamp_rails);
    HIPCHK(hipMemcpy(all.data(), p->d_engine + 1, 8 * all.size(), hipMemcpyDeviceToHost));
    st.assign(all.begin(), all.begin() + n);
    for (const EngSeg &g : p->segs)
        if (g.solo) {
            // a rail's closing stamp stands in every step behind its last barrier: not its time
            // for the steps it sat out before its last one with pieces (xg_solo_carry_tail)
            const int *cstep = p->sb.data() + g.sb_off + (size_t)g.w * (g.npieces / g.wv + 1);
            xg_solo_carry_tail(reinterpret_cast<uint64_t *>(all.data()), g.w, (int64_t)n, g.s0, g.s1 - g.s0, cstep,
                               g.rail_last.data());
            xg_solo_reduce_stamps(reinterpret_cast<const uint64_t *>(all.data()), g.w, (int64_t)n, g.s0, g.s1,
                                  reinterpret_cast<uint64_t *>(st.data()));
        }
    return XG_OK;
}

// step_done[] of a run of p from the stamps read back after it (libxghost, xg_step_times): the
// marks gs, the chain stamps cst and the engine stamps st (each null when the run has none),
// under p's segments, chains and step marks; host_total >= 0: an armed run's host-measured time
int step_times(const xg_plan *p, const std::vector<unsigned long long> *gs, const std::vector<unsigned long long> *cst,
               const std::vector<unsigned long long> *st, double wall_hz, double host_total, double *step_done)
{
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "stamps are 64-bit");
    auto u64 = [](const std::vector<unsigned long long> *v) {
        return v ? reinterpret_cast<const uint64_t *>(v->data()) : nullptr;
    };
    std::vector<int32_t> seg_end;
    for (const EngSeg &g : p->segs) seg_end.push_back(g.s1);
    return xg_step_times(p->nsteps, u64(gs), u64(cst), u64(st), p->seg_of.data(), seg_end.data(), p->chain_end.data(),
                         reinterpret_cast<const uint8_t *>(p->need_mark.data()), wall_hz, host_total, step_done)
               ? XG_EARG
               : XG_OK;
}

// after a synchronised run: did an engine workgroup give up at a grid barrier?
// Then the tickets are inconsistent: zero the state before the next launch.
extern "C" int xg_plan_check(xg_plan *p)
{
    if (p->segs.empty()) return XG_OK;
    xgk::EngineState es;
    HIPCHK(hipSetDevice(p->ctx->device));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    HIPCHK(hipMemcpy(&es, p->d_engine, sizeof es, hipMemcpyDeviceToHost));
    if (es.tmo) {
        p->engine_reset = true;
        fprintf(stderr, "xg: step engine: a workgroup timed out at a grid barrier (workgroups not co-resident?)\n");
        return XG_EHIP;
    }
    return XG_OK;
}

// step s of this plan as enqueued on (stream, side): an engine segment is one
// launch at its first step and nothing at the others
static int enqueue_unit(xg_plan *p, int s)
{
    const int gi = p->seg_of[s];
    if (gi < 0) return enqueue_step(p, s);
    if (p->segs[gi].s0 != s) return XG_OK;
    return launch_seg(p, p->segs[gi], p->ctx->stream);
}

// Armed run of a one-segment plan: the engine is launched, announces itself
// through the doorbell, and waits; the timed region starts when the host rings
// and ends when the engine reports its last step delivered (system-scope store
// to host memory).  The launch and dispatch latency (several us from an idle
// stream) thus stays outside, like the setup of a persistent MPI request before
// MPI_Start; every byte still moves inside.  Step times: the wall-clock stamps,
// anchored at the host-measured end.
static int run_armed(xg_plan *p, double *step_done, double *step_post, double *wall)
{
    xg_ctx *c = p->ctx;
    const EngSeg &g = p->segs[0];
    int rc;
    if ((rc = launch_seg(p, g, c->stream, true))) return rc;
    const unsigned epoch = p->epoch;
    const double tl = xg_now();
    bool ready;
    while (!(ready = __atomic_load_n(&p->db->ready, __ATOMIC_ACQUIRE) == epoch) && xg_now() - tl < 5.0) {
    }
    const double t0 = xg_now();
    __atomic_store_n(&p->db->ring, epoch, __ATOMIC_RELEASE);
    const double tp = xg_now();
    bool done;
    while (!(done = __atomic_load_n(&p->db->done, __ATOMIC_ACQUIRE) == epoch) && xg_now() - t0 < 10.0) {
    }
    const double t1 = xg_now();
    HIPCHK(hipStreamSynchronize(c->stream));
    if (wall) *wall = xg_now() - t0;
    if ((rc = xg_plan_check(p))) return rc;
    if (!ready || !done) {
        fprintf(stderr, "xg: armed step engine: no %s from the device\n", ready ? "completion" : "ready signal");
        return XG_EHIP;
    }
    if (step_post) {
        step_post[0] = tp - t0;
        for (int s = 1; s < p->nsteps; ++s) step_post[s] = 0;
    }
    if (step_done) {
        std::vector<unsigned long long> st;
        if ((rc = read_stamps(p, st))) return rc;
        return step_times(p, nullptr, nullptr, &st, c->wall_hz, t1 - t0, step_done);
    }
    return XG_OK;
}

// The timed run's launches: ev0, then every step (a chain's launches stamp the steps'
// completions, an engine segment is one launch), each followed by its step event.
// step_post (may be null): host seconds spent enqueueing each step.
static int enqueue_run(xg_plan *p, double *step_post)
{
    xg_ctx *c = p->ctx;
    int rc;
    if ((rc = mark(p, -1, c->stream))) return rc;
    p->rec_ev = true;
    const bool chains = p->d_cstamp && !c->kt_mode;
    for (int s = 0; s < p->nsteps;) {
        const double tp = xg_now();
        const int gi = p->seg_of[s];
        if (chains && p->chain_end[s]) {
            // a chain: launch t + 1 stamps step t's completion at its start; a clock
            // kernel stamps the last one's, one event after it anchors them all
            const int ce = p->chain_end[s];
            for (int t = s; t < ce; ++t) {
                const double tq = xg_now();
                // the step's first launch stamps the previous step's completion
                if ((rc = enqueue_pre(p, t, c->stream, c->side, t > s ? p->d_cstamp + t - 1 : nullptr))) {
                    p->rec_ev = false;
                    return rc;
                }
                if (step_post) step_post[t] = xg_now() - tq;
            }
            hipLaunchKernelGGL(xgk::clock_kernel, dim3(1), dim3(64), 0, c->stream, p->d_cstamp + ce - 1);
            HIPCHK(hipGetLastError());
            if ((rc = mark(p, ce - 1, c->stream))) {
                p->rec_ev = false;
                return rc;
            }
            s = ce;
            continue;
        }
        const int e = gi >= 0 ? p->segs[gi].s1 : s + 1;     // one launch posts a whole segment
        if ((rc = enqueue_unit(p, s))) {
            p->rec_ev = false;
            return rc;
        }
        // a deferred step's unpacks run in the next step's fused launch, which records its event
        if ((gi >= 0 || (!p->steps[s].deferred && p->need_mark[s])) && (rc = mark(p, e - 1, c->stream))) {
            p->rec_ev = false;
            return rc;
        }
        if (step_post) {
            step_post[s] = xg_now() - tp;
            for (int t = s + 1; t < e; ++t) step_post[t] = 0;
        }
        s = e;
    }
    p->rec_ev = false;
    return XG_OK;
}

// graph replay applies: asked for, not inside a kernel-timing session (its per-launch
// events are host bookkeeping), and a plan of more than one launch
static bool use_graph(const xg_plan *p)
{
    const int g = p->ctx->graph;
    return (g == 1 || (g < 0 && p->graph_auto)) && !p->ctx->kt_mode && p->nlaunch > 1 && p->d_gstamp;
}

extern "C" int xg_plan_run(xg_plan *p, double *step_done, double *step_post, double *wall)
{
    xg_ctx *c = p->ctx;
    int rc;
    HIPCHK(hipSetDevice(c->device));
    if (p->db && !c->kt_mode) return run_armed(p, step_done, step_post, wall);
    const bool chains = p->d_cstamp && !c->kt_mode;
    if (use_graph(p) && !p->g_run) {
        // captured once: the grid engine's ticket counter restarts from zero in every replay,
        // the step boundaries are stamps (mark)
        p->engine_reset = true;
        rc = capture(c->stream, &p->g_run, [&] { return enqueue_run(p, nullptr); });
        if (rc) {
            p->engine_reset = true;      // the host's ticket base moved for launches that never ran
            return rc;
        }
    }
    const bool graph = p->g_run && use_graph(p);
    const double t0 = xg_now();
    where("xg_plan_run", 0, p->nsteps, "posting the steps");
    if (graph) {
        HIPCHK(hipGraphLaunch(p->g_run, c->stream));
        // a replay restarts the device ticket counter from zero (the memset captured in the
        // graph) and leaves it at the captured run's count, which the host base does not track:
        // the next eager launch must zero the state again
        p->engine_reset = true;
        if (step_post && p->nsteps > 0) {
            // the whole run is posted by one graph launch: its host time is shared out over the
            // steps in proportion to the request posts this GPU's ranks make in each
            // (xg_stepplan.posts), so xg_sched_rank_timer credits all of it to the ranks that post
            // -- no share lands on a step without posts, where no Timer would read it -- and the
            // shares sum to the launch time (evenly over the steps if nothing is posted)
            const double tl = xg_now() - t0;
            int64_t tot = 0;
            for (int s = 0; s < p->nsteps; ++s) tot += p->steps[s].posts;
            for (int s = 0; s < p->nsteps; ++s)
                step_post[s] = tot > 0 ? tl * p->steps[s].posts / (double)tot : tl / p->nsteps;
        }
    } else if ((rc = enqueue_run(p, step_post))) {
        return rc;
    }
    where("xg_plan_run", p->nsteps, p->nsteps, "waiting for the device (hipStreamSynchronize)");
    HIPCHK(hipStreamSynchronize(c->stream));
    where("idle", -1, 0, "");
    if (wall) *wall = xg_now() - t0;
    if ((rc = xg_plan_check(p))) return rc;
    if (!step_done) return XG_OK;
    std::vector<unsigned long long> st;
    if (!p->segs.empty() && (rc = read_stamps(p, st))) return rc;
    std::vector<unsigned long long> cst, gs;
    if (chains) {
        cst.resize(p->nsteps);
        HIPCHK(hipMemcpy(cst.data(), p->d_cstamp, 8 * (size_t)p->nsteps, hipMemcpyDeviceToHost));
    }
    if ((rc = read_marks(p, gs))) return rc;
    // chains and segments anchored backwards at the mark behind them, unmarked steps filled in
    return step_times(p, &gs, chains ? &cst : nullptr, p->segs.empty() ? nullptr : &st, c->wall_hz, -1.0, step_done);
}

// Which steps an eager or captured run marks with a clock stamp (need[s] != 0; null: all).
// The last step is always marked; captured graphs hold the old marks and are dropped.
extern "C" int xg_plan_set_step_marks(xg_plan *p, const uint8_t *need)
{
    if (!p) return XG_EARG;
    for (int s = 0; s < p->nsteps; ++s) p->need_mark[s] = !need || need[s] || s == p->nsteps - 1;
    for (hipGraphExec_t *g : {&p->g_run, &p->vg.exec})   // captured runs hold the old marks: capture again
        if (*g) {
            HIPCHK(hipGraphExecDestroy(*g));
            *g = nullptr;
        }
    return XG_OK;
}

// Test hook: GPU g of a G-GPU job (a virtual context) runs its own share alone -- every copy
// launch of its plan (stage, local gather/scatter, packs, unpacks) with its RCCL calls and
// in-loop barriers left out, so a share too large to put all G GPUs on one device (configs[4]
// at its stated size: 256 GiB per GPU) still executes, its local slots verifiable.  Refused
// (XG_EARG) for a plan whose local copies travel as self send/recv in an RCCL group
// (XG_SELF_MAX): leaving the group out would drop them.
extern "C" int xg_plan_set_local_only(xg_plan *p, int on)
{
    if (!p || !p->ctx->virt) return XG_EARG;
    for (const StepR &st : p->steps)
        if (on && st.self_local) return XG_EARG;
    p->local_only = on != 0;
    return XG_OK;
}

// Test hook: the engine state of p as earlier launches would have left it -- `tickets` grid tickets
// taken in all, `armed` armed launches of the plan's (solo) segment -- so a test starts a plan's
// cumulative counters next to 2^31 or 2^32 instead of launching it a billion times.  The whole
// state is written (stamps untouched) and the host's bases and epoch follow; the doorbell's words
// hold the last epoch, as an armed run leaves them.
extern "C" int xg_plan_engine_preset(xg_plan *p, unsigned tickets, unsigned armed)
{
    if (!p || p->segs.empty()) return XG_EARG;
    const EngSeg &g = p->segs[0];
    if (armed && (!p->db || !g.solo)) return XG_EARG;
    HIPCHK(hipSetDevice(p->ctx->device));
    HIPCHK(hipStreamSynchronize(p->ctx->stream));
    xg_eng_solo_state ss;
    xg_eng_solo_state_after(g.solo ? (uint32_t)g.w : 0u, armed, &ss);
    xgk::EngineState es;
    memset(&es, 0, sizeof es);
    es.count = tickets;
    es.arrive = ss.arrive;
    es.rails = ss.rails;
    for (int l = 0; l < xgk::kGoLines; ++l) {
        es.go[l][0] = ss.go;
        es.fin[l][0] = ss.fin[l];
    }
    HIPCHK(hipMemcpy(p->d_engine, &es, sizeof es, hipMemcpyHostToDevice));
    p->engine_base = tickets;
    p->solo_base = armed;
    p->epoch = armed;
    p->engine_reset = false;
    if (p->db) {
        __atomic_store_n(&p->db->ring, armed, __ATOMIC_RELEASE);
        __atomic_store_n(&p->db->ready, armed, __ATOMIC_RELEASE);
        __atomic_store_n(&p->db->done, armed, __ATOMIC_RELEASE);
    }
    return XG_OK;
}

extern "C" int xg_plan_enqueue(xg_plan *p)
{
    int rc;
    auto body = [&] {
        int r;
        for (int s = 0; s < p->nsteps; ++s)
            if ((r = enqueue_unit(p, s))) return r;
        return XG_OK;
    };
    if (!use_graph(p)) return body();
    if (!p->g_enq) {
        p->engine_reset = true;
        if ((rc = capture(p->ctx->stream, &p->g_enq, body))) {
            p->engine_reset = true;      // the host's ticket base moved for launches that never ran
            return rc;
        }
    }
    HIPCHK(hipGraphLaunch(p->g_enq, p->ctx->stream));
    p->engine_reset = true;          // the replay moved the device counter, not the host base
    return XG_OK;
}

