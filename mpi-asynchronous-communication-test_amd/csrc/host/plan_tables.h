// plan_tables.h -- internal header of the plan-table builder (plan_tables.cc, libxghost): the tables
// a loaded plan runs from, and the one function that builds them.  Plain C++17, no HIP: the runtime
// (csrc/runtime/) includes it and uploads what the builder made; a CPU test builds the same tables
// through the xg_plan_tables_* group of xg_sched.h.  Not part of the public ABI.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../dcopy.h"
#include "xg.h"

typedef xg_plan_knobs PlanKnobs;

// One copy launch of a run, decided once by the builder (TableBuilder in plan_tables.cc: the only
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
    // PlanTables::xt_begin[xt_off[xt + k] ..], xt_n[xt + k] of them (tile_launches)
    int xt = 0;
    // SMALL only: the launch has NO pieces (n = 0); its copies are rows [q_row, q_row + q_copies) of
    // PlanTables::rows, each q_len bytes, taken q_k to a group (xg_small_index); its cuts are workgroup
    // indices from 0, and dispatch k copies PlanTables::qbytes[q_bytes + k] bytes
    int q_row = 0, q_copies = 0, q_k = 1, q_bytes = 0;
    int64_t q_len = 0;
    bool side = false;               // runs on the side stream: fork event before it, join event after it
    bool mark_prev = false;          // holds the previous step's unpacks: that step's mark goes right behind it
    int cut = 0, ndisp = 1;          // its dispatches (launches above 1.5 x launch_max go as several):
                                     // dispatch k = pieces [cuts[cut + k], cuts[cut + k + 1]) of PlanTables::cuts
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
    // The step's launches: entries [l_b, l_e) of PlanTables::launches, in issue order -- the stage
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
    int sb_off;                    // its block in sb: (n + 1) unit offsets, then n flags
                                   // (solo: per rail nrows + 1 row barrier counts, then per rail
                                   // n closed-step indices)
    int nhaz;                      // hazard points (xg_engine_hazards flag 2)
    bool solo;                     // solo engine (solo_engine_kernel), pieces from u0
    int wv;                        // solo: waves per rail (16 or 1)
    int gran;                      // solo: descriptor granule in bytes (16, or 4 / 1 for segments not 16-B aligned)
    int u0;                        // first unit / piece of the segment in ep
    int npieces;                   // solo: pieces per rail (whole chunks of rows), rail r's from u0 + r * npieces
                                   // in solo_desc; w = rails
    const uint8_t *sbase;          // solo: base pointers of the descriptors' offsets
    uint8_t *dbase;
    int64_t bytes;                 // bytes copied per run
    std::vector<int32_t> rail_last;   // solo: per rail, its last step with pieces (from s0; xg_solo_rail_last)
};

// The staging displacements of the packed segments (alltoallw translate,
// mpi_test.c:233-302) are scanned on the device at load: one scan group per step and
// direction, then the pack pieces' destinations / unpack pieces' sources are patched.
// These are the scan's inputs; the host's own layout (xg_devplan_build) is its cross-check.
struct DisplScan {
    std::vector<int64_t> len, host;   // per packed copy (in group order): length, host displacement
    std::vector<int> groups{0};
    std::vector<xgk::DFix> fix;
    void close_group()
    {
        if ((int)len.size() > groups.back()) groups.push_back((int)len.size());
    }
};

// Everything a run reads that is decided at load, as host tables; the runtime's xg_plan derives
// from it and adds the device copies.
struct xg_plan_tables {
    int nsteps = 0;
    int npieces = 0;
    uint64_t base[XG_NBUF] = {};            // the regions the tables' pointers lie in
    int64_t bytes[XG_NBUF] = {};
    int wave_grid = 1;                      // PlanKnobs::wave_grid (wave_wgs)
    std::vector<StepR> steps;
    std::vector<xg_call> calls;             // every step's RCCL calls, as xg_devplan_step_calls lists them
    std::vector<int32_t> call_begin;        // nsteps + 1: where each step's calls start
    std::vector<CopyLaunch> launches;       // every step's copy launches (StepR::l_b .. l_e), fixed at load
    std::vector<int> cuts;                  // their dispatches' piece boundaries (CopyLaunch::cut)
    // copy_kernel_x tile tables, one per dispatch of every EXTENT launch (xg_extent_tiles over the
    // dispatch's ordered pieces): xt_n[i] tiles, tile t = pieces [xt_begin[xt_off[i] + t], .. + t + 1])
    // of the dispatch (indices relative to its first piece)
    std::vector<int> xt_begin, xt_off, xt_n;
    // copy_kernel_q launches: one row {src, dst, len} per positive copy, in destination order
    // (CopyLaunch::q_row), and the bytes of each of their dispatches (CopyLaunch::q_bytes)
    std::vector<xgk::DCopy> rows;
    std::vector<int64_t> qbytes;
    std::vector<xgk::DCopy> pieces;         // the piece table, ordered (order_pieces); staging sides at
                                            // displacement 0 until the device scan patches its copy
    std::vector<int64_t> plen;              // prefix sums of the piece lengths (npieces + 1)
    DisplScan ds;
    int variant = 0;
    bool streaming = false;                 // one run copies more than the Infinity Cache holds (read + write)
    // step engine segments
    std::vector<int> seg_of;                // per step: index into segs, or -1
    std::vector<EngSeg> segs;
    std::vector<xgk::DCopy> ep;             // every grid segment's work units, step-major
    std::vector<int> sb;                    // every segment's block table (EngSeg::sb_off)
    std::vector<unsigned long long> solo_desc;  // solo segments' packed pieces
    int stamp_rails = 1;                    // rails the stamp area holds
    bool may_arm = false;                   // ONE segment that is the whole plan, arming on: xg_plan_run may arm it
    // chains: runs of >= 2 consecutive steps that are each ONE local copy launch, or a TAM
    // stage launch and/or a local launch (outside engine segments, no RCCL, no barrier).  xg_plan_run times them with no
    // mark between launches: launch t+1 stamps its start = step t's completion, a clock kernel
    // closes the chain, the chain's mark after it anchors the stamps.  chain_end[s] = end of s's chain (s = its
    // first step), 0 elsewhere.
    std::vector<int> chain_end;
    bool any_chain = false;
    int nlaunch = 0;                        // kernel launches per run (copies + engine), RCCL's aside
    bool graph_auto = false;                // XG_GRAPH unset: this plan replays as a graph (latency-bound, one GPU)
};
typedef xg_plan_tables PlanTables;

// Fills *t (freshly constructed) from dp.  XG_EARG after the message on stderr: a descriptor outside
// its region, or a tile table that does not cover its pieces.
int plan_tables_build(PlanTables *t, const xg_devplan *dp, const PlanKnobs *k, const uint64_t base[XG_NBUF],
                      const int64_t bytes[XG_NBUF]);

// Every copy launch one run issues, in issue order (an engine segment's steps issue none).
template <class F>
static void each_launch(const PlanTables *p, F f)
{
    for (int s = 0; s < p->nsteps; ++s)
        if (p->seg_of[s] < 0)
            for (int i = p->steps[s].l_b; i < p->steps[s].l_e; ++i) f(p->launches[i]);
}

// workgroups (4 waves each) of a copy_kernel_w dispatch over n pieces
static inline int wave_wgs(const PlanTables *p, int n) { return std::max(1, std::min(p->wave_grid, (n + 3) / 4)); }

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
