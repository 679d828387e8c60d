// rt.h -- internal header of libxg's device half (include/xg.h is the C-ABI): the
// context, region and plan structures every runtime translation unit shares, the error
// macros, and the helpers more than one of them calls.  gfx950 only.
//
//   ctx.hip        context (streams, communicator), HBM regions, fill / verify / span checksums
//   plan_load.hip  xg_plan_load: uploads the tables host/plan_tables.cc built, displacement scan
//   exec.hip       execution: walks each step's launch-table entries, RCCL groups, chains, engine,
//                  graph, armed runs
//   virtual.hip    a whole G-GPU job on one device (test hook)
//   measure.hip    kernel-timing sessions and the RCCL p2p microbenchmark
//   vecplace.hip   xg_vecplace_*: a strided placement as one copy_kernel_v launch (host/vec_tables.cc's tables)
#pragma once

#include <hip/hip_runtime.h>
#include <unistd.h>
#include <rccl/rccl.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <vector>

#include "../kernels.h"
#include "../host/plan_tables.h"     // the host tables of a plan and their builder (no HIP)
#include "xg.h"

// On an error, hipGetLastError() is read once more: HIP keeps the last failing call's error
// for it, and a later launch check (hipGetLastError right after a launch) would otherwise
// report this old error as its own.
#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "xg: HIP error %s at %s:%d: %s\n", hipGetErrorString(e_), __FILE__,   \
                    __LINE__, #x);                                                                 \
            (void)hipGetLastError();                                                               \
            return XG_EHIP;                                                                        \
        }                                                                                          \
    } while (0)

#define NCCLCHK(x)                                                                                 \
    do {                                                                                           \
        ncclResult_t r_ = (x);                                                                     \
        if (r_ != ncclSuccess) {                                                                   \
            fprintf(stderr, "xg: RCCL error %s at %s:%d: %s\n", ncclGetErrorString(r_), __FILE__, \
                    __LINE__, #x);                                                                 \
            return XG_ERCCL;                                                                       \
        }                                                                                          \
    } while (0)

// Device scratch freed on every return path (error returns of HIPCHK included).
struct DevMem {
    void *p = nullptr;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem()
    {
        if (p) (void)hipFree(p);
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair()
    {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// Where the host thread is (diagnostics for a run that does not return: xg_debug_where): the
// entry point, the step it is posting and whether it is waiting for the device.  Plain stores,
// read only by a watchdog after the fact.
struct WhereState {
    const char *fn = "idle";
    int step = -1, nsteps = 0;
    const char *phase = "";
};
inline WhereState g_where;         // one for the library (C++17 inline variable)
static inline void where(const char *fn, int step, int nsteps, const char *phase)
{
    g_where.fn = fn; g_where.step = step; g_where.nsteps = nsteps; g_where.phase = phase;
}

// One RCCL group whose calls come from `post`, a callable returning ncclResult_t for
// call i (i = 0..n-1): the group is closed (ncclGroupEnd) on every path, so an error
// never leaves this rank inside an open group.  Returns XG_OK or XG_ERCCL.
template <class F>
static int rccl_group(int n, F post, const char *what)
{
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess) {
        fprintf(stderr, "xg: RCCL error %s: ncclGroupStart (%s)\n", ncclGetErrorString(r), what);
        return XG_ERCCL;
    }
    int rc = XG_OK;
    for (int i = 0; i < n && rc == XG_OK; ++i) {
        r = post(i);
        if (r != ncclSuccess) {
            fprintf(stderr, "xg: RCCL error %s: call %d of %d in a group (%s)\n", ncclGetErrorString(r), i, n, what);
            rc = XG_ERCCL;
        }
    }
    r = ncclGroupEnd();
    if (r != ncclSuccess) {
        fprintf(stderr, "xg: RCCL error %s: ncclGroupEnd (%s)\n", ncclGetErrorString(r), what);
        rc = XG_ERCCL;
    }
    return rc;
}

// The plan-table knobs (xg_plan_knobs, xg_sched.h: rank, nranks, virt, rules, the engine, solo, launch
// and step-form settings) are the context's base: xg_init fills them from the device and the
// environment, xg_plan_load hands them to the builder.
struct xg_ctx : xg_plan_knobs {
    int device;
    hipStream_t stream;
    hipStream_t side;       // local gather/scatter of a step that also talks to other GPUs (overlaps RCCL)
    ncclComm_t comm;
    double *d_red;          // device scratch for barrier / MAX reductions
    int graph;                 // hipGraph replay of multi-launch runs: 1 always, 0 never, -1 latency-bound one-GPU runs
    double wall_hz;            // wall_clock64() rate
    int engine_occ;            // co-resident step-engine workgroups the device admits (caps engine_wmax)
    // kernel timing session (xg_ktime_begin/end): 1 = an event pair around every
    // copy launch, 2 = one pair around the whole session on the main stream
    int kt_mode;
    int nk;
    std::vector<hipEvent_t> kev;   // start/end pairs per copy launch (mode 1), or the region pair
    std::vector<int64_t> kbytes;   // algorithmic bytes (read + write) per launch (mode 1)
    int64_t kt_bytes;              // their sum (both modes)
};

struct xg_regions {
    xg_ctx *ctx;
    uint8_t *ptr[XG_NBUF];
    int64_t bytes[XG_NBUF];
    bool owned[XG_NBUF];    // hipMalloc'd here (freed, poisoned at creation); false: the caller's memory (xg_regions_adopt)
};

// A loaded plan: the host tables (PlanTables, host/plan_tables.h) and their device copies.
struct xg_plan : PlanTables {
    xg_ctx *ctx = nullptr;
    xg_regions *reg = nullptr;
    xgk::DCopy *d_pieces = nullptr;         // pieces, patched by the displacement scan
    int *d_xt = nullptr;                    // xt_begin
    xgk::DCopy *d_rows = nullptr;           // rows
    std::vector<hipEvent_t> fork, join;     // per step with a side-stream launch: main -> side, side -> main
    int *d_sb = nullptr;                    // sb
    xgk::DCopy *d_epieces = nullptr;        // ep
    xgk::EngineState *d_engine = nullptr;   // state (16 B, zeroed at load) followed by stamps: rail r's of step
                                            // s at [r * nsteps + s] (grid segments: rail 0)
    unsigned engine_base = 0;               // barrier tickets taken by earlier launches (wraps)
    unsigned solo_base = 0;                 // armed solo launches since the state was last zeroed (wraps; not
                                            // `epoch`, which outlives an engine_reset)
    bool engine_reset = false;              // zero the state before the next launch
    xgk::Doorbell *db = nullptr;            // host-pinned doorbell of armed runs (may_arm), or null
    unsigned long long *d_solo = nullptr;   // solo_desc
    unsigned epoch = 0;                     // armed launches so far
    // staging displacements of the packed segments, computed on the device at load
    int64_t *d_disp = nullptr;
    int ndisp = 0;
    bool rec_ev = false;                    // xg_plan_run is marking steps (fused launches mark the previous step's end)
    unsigned long long *d_cstamp = nullptr;  // nsteps wall-clock stamps of chained steps (chain_end)
    // hipGraph replay (XG_GRAPH=1): the launches of one xg_plan_enqueue / one timed xg_plan_run,
    // captured at first use and replayed after (a launch-bound multi-step run then costs one
    // graph launch of host time instead of a launch, an event and an RCCL group per step)
    hipGraphExec_t g_enq = nullptr, g_run = nullptr;
    // step marks: mark(i) has a one-lane clock_kernel write the wall clock to d_gstamp[i + 1]
    // (i = -1: the start) once everything before it on the stream is done.  Not timing events:
    // an event record left the device idle ~4.7 us per step against ~2.1 us for the stamp
    // (profiles/r04/stamp_marks/), and captured events are not re-recorded by a graph replay on
    // this stack (tools/graph_probe.hip), so eager runs, graph replays and virtual jobs all stamp
    unsigned long long *d_gstamp = nullptr;
    std::vector<char> need_mark;            // per step: an eager or captured run marks it (xg_plan_set_step_marks;
                                            // default all) -- engine segments and chains mark their last step always
    bool local_only = false;                // test hook (xg_plan_set_local_only): a virtual GPU runs its share alone,
                                            // its RCCL calls and in-loop barriers left out
    uint64_t id = 0;                        // unique per loaded plan (keys the virtual runner's graphs)
    struct VGraph {
        std::vector<uint64_t> ids;
        bool rccl = false;
        hipGraphExec_t exec = nullptr;
    } vg;                                   // plans[0] of a virtual job: the job's captured run
};

// Capture what `body` enqueues on `stream` into a graph and instantiate it.  The stream
// leaves capture mode on every path; on failure nothing is kept.
template <class F>
static int capture(hipStream_t stream, hipGraphExec_t *out, F body)
{
    *out = nullptr;
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(stream, &g);
    if (rc || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        if (!rc) fprintf(stderr, "xg: hipStreamEndCapture: %s\n", hipGetErrorString(e));
        return rc ? rc : XG_EHIP;
    }
    const hipError_t ie = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) {
        *out = nullptr;
        fprintf(stderr, "xg: hipGraphInstantiate: %s\n", hipGetErrorString(ie));
        return XG_EHIP;
    }
    return XG_OK;
}

// RCCL writes its log -- and, under NCCL_DEBUG=WARN/VERSION, a version banner at
// communicator creation -- to stdout unless NCCL_DEBUG_FILE says otherwise; stdout
// here carries the reference's report (bin/test, bin/pt2pt_test) and bench.py's JSON
// line, so send RCCL's output to stderr unless the user chose a file.  Called before
// every first RCCL call (RCCL reads the variable when it first logs).
static inline void rccl_log_to_stderr()
{
    if (!getenv("NCCL_DEBUG_FILE")) setenv("NCCL_DEBUG_FILE", "/dev/stderr", 0);
}

// RCCL 2.27 also prints a version banner (RCCL/HIP/ROCm version, host, library path)
// straight to stdout when it creates a communicator: fd 1 points at fd 2 for that call.
struct StdoutToStderr {
    int saved;
    StdoutToStderr() : saved(-1)
    {
        fflush(stdout);
        saved = dup(1);
        if (saved >= 0) dup2(2, 1);
    }
    ~StdoutToStderr()
    {
        fflush(stdout);
        if (saved >= 0) {
            dup2(saved, 1);
            close(saved);
        }
    }
};


// ---- shared between the runtime's translation units
// exec.hip
int mark(xg_plan *p, int i, hipStream_t stream);
int read_marks(const xg_plan *p, std::vector<unsigned long long> &gs);
double mark_elapsed(const xg_plan *p, int i, const std::vector<unsigned long long> &gs);
int read_stamps(const xg_plan *p, std::vector<unsigned long long> &st);
int step_times(const xg_plan *p, const std::vector<unsigned long long> *gs, const std::vector<unsigned long long> *cst,
               const std::vector<unsigned long long> *st, double wall_hz, double host_total, double *step_done);
int enqueue_pre(xg_plan *p, int s, hipStream_t stream, hipStream_t side, unsigned long long *start = nullptr);
int enqueue_post(xg_plan *p, int s, hipStream_t stream);
int launch_seg(xg_plan *p, const EngSeg &g, hipStream_t stream, bool armed = false);
