// rt.h -- internal header of libxg's device half (include/xg.h is the C-ABI): the
// context, region and plan structures every runtime translation unit shares, the error
// macros, and the helpers more than one of them calls.  gfx950 only.
//
//   ctx.hip        context (streams, communicator), HBM regions, fill / verify / span checksums
//   plan_load.hip  xg_plan_load: piece table, copy-launch table, engine segments, displacement scan
//   exec.hip       execution: walks each step's launch-table entries, RCCL groups, chains, engine,
//                  graph, armed runs
//   virtual.hip    a whole G-GPU job on one device (test hook)
//   measure.hip    kernel-timing sessions and the RCCL p2p microbenchmark
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

struct xg_ctx {
    int rank, nranks, device;
    bool virt;              // xg_init_virtual: one of nranks GPUs emulated on one device, no RCCL
    hipStream_t stream;
    hipStream_t side;       // local gather/scatter of a step that also talks to other GPUs (overlaps RCCL)
    ncclComm_t comm;
    double *d_red;          // device scratch for barrier / MAX reductions
    xg_copy_rules rules;    // what decides each copy launch's kernel and piece size (xg_copy_launch_choose,
                            // xg_sched.h): chunk, cus, the wave / ragged / extent / small-piece knobs
    int64_t engine_max_step;   // GPU-local plans whose largest step moves <= this many bytes use the step engine
    int engine_wmax;           // at most this many (co-resident) engine workgroups
    int engine_drain;          // 1: always drain before each barrier arrival (XG_ENGINE_DRAIN=1)
    int solo;                  // 0: never use the solo engine
    int64_t solo_max;          // solo segments move <= this many bytes per run
    int solo_rails;            // solo segments deal their pieces over up to this many rails
    int solo_waves;            // waves per rail: 16 (a workgroup) or 1
    int64_t launch_max;        // copy launches above this many bytes go as back-to-back launches of ~this size
    int wave_grid;             // copy_kernel_w workgroups resident at once (occupancy x CUs)
    int step_chain;            // 1: time runs of one-launch local steps by in-kernel stamps (xg_plan_run)
    int engine_arm;            // 1: xg_plan_run arms single-segment plans (doorbell)
    int64_t split_min;         // a cross-GPU step's local gather of >= this many bytes runs on the side stream
                               // (smaller: in the pack / fused launch)
    int64_t self_max;          // a cross-GPU step's local part of <= this many bytes goes in its RCCL group
    int fuse_stage;            // 1: a step's stage copies launch with its local copies when hazard-free
    int split_after_pack;      // 1: a split step's local part forks after its pack launch
    int graph;                 // hipGraph replay of multi-launch runs: 1 always, 0 never, -1 latency-bound one-GPU runs
    double wall_hz;            // wall_clock64() rate
    int variant;            // copy kernel variant (copy_variant in plan_load.hip)
    int64_t extent_tile;       // bytes per copy_kernel_x tile (kExtTileBytes)
    int engine_occ;            // co-resident step-engine workgroups the device admits (plan load caps W)
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

// One copy launch of a run, decided once by xg_plan_load (build_tables in plan_load.hip: the only
// place that turns a step's form -- split, fused, fused_local, stage_fused, deferred, self_local --
// into launches) and never changed after: execution, the launch counts and chain eligibility all
// read the table.
struct CopyLaunch {
    int b = 0, n = 0;                // pieces [b, b + n) of the plan's piece table
    int64_t bytes = 0;               // bytes they copy (read + written once)
    int kind = XG_COPY_PIECE;        // its ONE kernel (xg_copy_launch_choose, xg_sched.h): PIECE copy_kernel_g<4, nt>,
                                     // WAVE copy_kernel_w<kib>, SHIFT copy_kernel_s<nt>, EXTENT copy_kernel_x<nt>,
                                     // SMALL copy_kernel_q<kib / 4, nt>; every one can stamp its start (chains)
    bool nt = false;                 // non-temporal loads and stores (never WAVE)
    int kib = 0;                     // piece KiB of a WAVE (2 / 4 / 8) or SMALL (4 / 8) launch, else 0
    // EXTENT only: one workgroup per TILE of pieces -- dispatch k's tiles are
    // xg_plan::xt_begin[xt_off[xt + k] ..], xt_n[xt + k] of them (tile_launches)
    int xt = 0;
    // SMALL only: the launch has NO pieces (n = 0); its copies are rows [q_row, q_row + q_copies) of
    // xg_plan::d_rows, each q_len bytes, taken q_k to a group (xg_small_index); its cuts are workgroup
    // indices from 0, and dispatch k copies xg_plan::qbytes[q_bytes + k] bytes
    int q_row = 0, q_copies = 0, q_k = 1, q_bytes = 0;
    int64_t q_len = 0;
    bool side = false;               // runs on the side stream: fork event before it, join event after it
    bool mark_prev = false;          // holds the previous step's unpacks: that step's mark goes right behind it
    int cut = 0, ndisp = 1;          // its dispatches (launches above 1.5 x launch_max go as several):
                                     // dispatch k = pieces [cuts[cut + k], cuts[cut + k + 1]) of xg_plan::cuts
};

struct StepR {
    // Piece ranges of one step's parts in the plan's piece table: stage (TAM rank-local
    // copies), local gather/scatter, packs into staging, unpacks out of it.  How the parts
    // launch is the step's run of the launch table (below).
    //   split: a step with cross-GPU ops runs its local part on the side stream beside the
    //   packs and the RCCL group.
    //   fused: this step's packs go in ONE launch with the previous step's unpacks
    //   (deferred there); a pack only fills staging and delivers nothing, so every
    //   message of this step is still delivered after every one of the previous step.
    //   Never when a pack reads bytes those unpacks write (xg_step_packs_meet_unpacks).
    // call_b / call_n: the step's RCCL calls in the plan's call list (xg_devplan_step_calls);
    // p2p_n of them are send/recv (one group), sync_after: the last is the in-loop barrier
    int stage_b = 0, stage_n = 0, local_b = 0, local_n = 0, pack_b = 0, pack_n = 0, post_b = 0, post_n = 0;
    int call_b = 0, call_n = 0, p2p_n = 0, sync_after = 0;
    int groups = 1;                  // RCCL groups of the step: 1, or 2 for a relay step (XG_CALL_FENCE between)
    int posts = 0;                   // request posts of this GPU's ranks in the step (xg_stepplan.posts)
    int pre_n = 0;                   // local_n + pack_n
    int64_t stage_bytes = 0, local_bytes = 0, pack_bytes = 0, post_bytes = 0;   // bytes copied by each part (read + written once)
    bool split = false, fused = false, deferred = false;
    bool small = false;              // its local launch runs copy_kernel_q: it has rows, no pieces (local_n = 0),
                                     // and is never an engine step
    bool self_local = false;         // the local copies travel in the RCCL group as self send/recv (XG_SELF_MAX)
    bool fused_local = false;        // fused, and the local copies join that launch (small, hazard-free)
    bool stage_fused = false;        // the stage copies join the step's local (+ pack) launch: none of the
                                     // other pre copies meets their bytes (xg_step_stage_meets_rest)
    // The step's launches: entries [l_b, l_e) of xg_plan::launches, in issue order -- the stage
    // launch, the fused launch (previous unpacks + packs), then the packs and the forked local
    // part (XG_SPLIT_AFTER_PACK decides which goes first) or the one local + pack launch; the
    // RCCL group goes before entry l_rccl; the unpacks follow it, unless deferred into the next
    // step's fused launch.  (An engine segment's steps never run theirs.)
    int l_b = 0, l_rccl = 0, l_e = 0;
};

// A run of >= 2 consecutive GPU-local steps (no RCCL op, no in-loop barrier, no
// TAM stage copy, no unpack, each <= engine_max_step bytes) executed by ONE
// step_engine_kernel launch; every other step is its own launches.
struct EngSeg {
    int s0, s1;                    // steps [s0, s1)
    int w, b;                      // workgroups; 16-B loads per lane per unit (1, 4, 16)
    int sb_off;                    // its block in d_sb: (n + 1) unit offsets, then n flags
                                   // (solo: per rail nrows + 1 row barrier counts, then per rail
                                   // n closed-step indices)
    int nhaz;                      // hazard points (xg_engine_hazards flag 2)
    bool solo;                     // solo engine (solo_engine_kernel), pieces from u0
    int wv;                        // solo: waves per rail (16 or 1)
    int gran;                      // solo: descriptor granule in bytes (16, or 4 / 1 for segments not 16-B aligned)
    int u0;                        // first unit / piece of the segment in d_epieces
    int npieces;                   // solo: pieces per rail (whole chunks of rows), rail r's from u0 + r * npieces
                                   // in d_solo; w = rails
    const uint8_t *sbase;          // solo: base pointers of the descriptors' offsets
    uint8_t *dbase;
    int64_t bytes;                 // bytes copied per run
};

struct xg_plan {
    xg_ctx *ctx = nullptr;
    xg_regions *reg = nullptr;
    int nsteps = 0;
    xgk::DCopy *d_pieces = nullptr;
    int npieces = 0;
    std::vector<StepR> steps;
    std::vector<xg_call> calls;             // every step's RCCL calls, as xg_devplan_step_calls lists them
    std::vector<int32_t> call_begin;        // nsteps + 1: where each step's calls start
    std::vector<CopyLaunch> launches;       // every step's copy launches (StepR::l_b .. l_e), fixed at load
    std::vector<int> cuts;                  // their dispatches' piece boundaries (CopyLaunch::cut)
    // copy_kernel_x tile tables, one per dispatch of every EXTENT launch (xg_extent_tiles over the
    // dispatch's ordered pieces): xt_n[i] tiles, tile t = pieces [xt_begin[xt_off[i] + t], .. + t + 1])
    // of the dispatch (indices relative to its first piece); d_xt: xt_begin on the device
    std::vector<int> xt_begin, xt_off, xt_n;
    int *d_xt = nullptr;
    // copy_kernel_q launches: one row {src, dst, len} per positive copy, in destination order
    // (CopyLaunch::q_row), and the bytes of each of their dispatches (CopyLaunch::q_bytes)
    std::vector<xgk::DCopy> rows;
    xgk::DCopy *d_rows = nullptr;
    std::vector<int64_t> qbytes;
    std::vector<hipEvent_t> fork, join;     // per step with a side-stream launch: main -> side, side -> main
    int variant = 0;
    bool streaming = false;                 // one run copies more than the Infinity Cache holds (read + write)
    // step engine segments
    std::vector<int> seg_of;                // per step: index into segs, or -1
    std::vector<EngSeg> segs;
    int *d_sb = nullptr;
    xgk::DCopy *d_epieces = nullptr;        // every segment's work units, step-major
    xgk::EngineState *d_engine = nullptr;   // state (16 B, zeroed at load) followed by stamps: rail r's of step
                                            // s at [r * nsteps + s] (grid segments: rail 0)
    int stamp_rails = 1;                    // rails the stamp area holds
    unsigned engine_base = 0;               // barrier tickets taken by earlier launches (wraps)
    bool engine_reset = false;              // zero the state before the next launch
    xgk::Doorbell *db = nullptr;            // host-pinned doorbell of armed runs (single-segment plans), or null
    std::vector<unsigned long long> solo_desc;  // solo segments' packed pieces (host copy)
    unsigned long long *d_solo = nullptr;
    unsigned epoch = 0;                     // armed launches so far
    // staging displacements of the packed segments, computed on the device at load
    int64_t *d_disp = nullptr;
    int ndisp = 0;
    int nlaunch = 0;                        // kernel launches per run (copies + engine), RCCL's aside
    bool rec_ev = false;                    // xg_plan_run is marking steps (fused launches mark the previous step's end)
    // chains: runs of >= 2 consecutive steps that are each ONE local copy launch, or a TAM
    // stage launch and/or a local launch (outside engine segments, no RCCL, no barrier).  xg_plan_run times them with no
    // mark between launches: launch t+1 stamps its start = step t's completion, a clock kernel
    // closes the chain, the chain's mark after it anchors the stamps.  chain_end[s] = end of s's chain (s = its
    // first step), 0 elsewhere.
    std::vector<int> chain_end;
    unsigned long long *d_cstamp = nullptr;  // nsteps wall-clock stamps of chained steps
    std::vector<int64_t> plen;              // prefix sums of the piece lengths (npieces + 1), host side
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
    bool graph_auto = false;                // XG_GRAPH unset: this plan replays as a graph (latency-bound, one GPU)
    bool local_only = false;                // test hook (xg_plan_set_local_only): a virtual GPU runs its share alone,
                                            // its RCCL calls and in-loop barriers left out
    uint64_t id = 0;                        // unique per loaded plan (keys the virtual runner's graphs)
    struct VGraph {
        std::vector<uint64_t> ids;
        bool rccl = false;
        hipGraphExec_t exec = nullptr;
    } vg;                                   // plans[0] of a virtual job: the job's captured run
};

// Every copy launch one run issues, in issue order (an engine segment's steps issue none).
template <class F>
static void each_launch(const xg_plan *p, F f)
{
    for (int s = 0; s < p->nsteps; ++s)
        if (p->seg_of[s] < 0)
            for (int i = p->steps[s].l_b; i < p->steps[s].l_e; ++i) f(p->launches[i]);
}

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

// Settled tuning, fixed since round 4 (DESIGN.md "Knobs" lists what each was measured against).
constexpr int64_t kNtMin = 128 << 20;      // launches of >= this many bytes stream past the MALL:
                                           // non-temporal (profiles/r02/copy_nt_sizes.txt, copy_ab_nt/)
constexpr int64_t kNtStream = 4 << 20;     // ... and, in a streaming plan, launches of >= this many
constexpr int64_t kGridCacheMax = 256 << 20;   // grid_pays: a run of <= this many bytes stays in the MALL
constexpr int64_t kWgCost = 2048;          // a copy workgroup's fixed start, bytes-equivalent (xg_piece_size)
// copy_kernel_x (placement plans): tile caps (a workgroup takes at most kExtTilePieces pieces --
// one descriptor per lane -- and about kExtTileBytes bytes), the mean copy length up to which a
// launch runs it, and whether it runs at all without XG_EXTENT_COPY (copy_kernel_x)
constexpr int64_t kExtTileBytes = 32 << 10;
constexpr int kExtTilePieces = xgk::kThreads;
constexpr int64_t kExtMeanMax = 1024;
constexpr int kExtDefault = 1;
// copy_kernel_q: the launch size from which a uniform launch runs it, its piece KiB, the copies
// per group of its piece order (xg_small_index's k: with 8, the eight workgroups that start
// together walk eight consecutive destination copies side by side, one piece each per round) and
// whether it runs at all without XG_SMALL_PIECES.  Chosen by bench.py's CHOICE_RULE over the arms of
// profiles/r10/small_pieces/ab.txt: 8 KiB x 8 copies -5 % against the
// parent's 32 KiB pieces; 8 KiB in plain destination order (k = 1) a tie, 4 KiB slower.  The
// threshold is the smallest launch of the size sweep (size_sweep.txt: 28 MiB - 896 MiB) that won by
// the rule: 112 MiB -7 %, 224 MiB -5 %, 896 MiB -4 %; 56 MiB -3 % (inside the spread), 28 MiB +1 %.
constexpr int64_t kSmallMin = 112 << 20;
constexpr int kSmallKiB = 8;
constexpr int kSmallOrder = 8;
constexpr int kSmallDefault = 1;
constexpr int64_t kWaveMax = 32 << 20;     // copy_kernel_w up to this launch size (profiles/r03/wave_local/)

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
int enqueue_pre(xg_plan *p, int s, hipStream_t stream, hipStream_t side, unsigned long long *start = nullptr);
int enqueue_post(xg_plan *p, int s, hipStream_t stream);
int launch_seg(xg_plan *p, const EngSeg &g, hipStream_t stream, bool armed = false);
