// plan_tables.cc -- the host half of xg_plan_load: a device plan (devplan.c) becomes the piece table,
// the table of copy launches (each step's launches, decided here once: TableBuilder), their dispatch
// cuts and tile tables, the displacement-scan inputs, the engine segments and the chains.  Host
// arithmetic only: the runtime (csrc/runtime/plan_load.hip) uploads what this file made, and the
// xg_plan_tables_* group of xg_sched.h builds the same tables with no GPU.
#include "plan_tables.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

// ------------------------------------------------------------------ engine segments
// Engine eligibility of one step: GPU-local copies only, small enough that the
// per-launch boundary dominates (profiles/r01_engine_sweep.txt: crossover ~16 MiB).
static bool engine_step(const PlanKnobs *c, const StepR &st)
{
    return !st.p2p_n && !st.sync_after && !st.stage_n && !st.stage_fused && !st.post_n && !st.pack_n && !st.fused &&
           !st.deferred && !st.small && st.local_bytes <= c->engine_max_step;
}

// Solo or grid engine for a hazard-free segment of n steps (`busy` of them move
// bytes) moving `bytes`: the cheaper by a model of the measured costs (MI355X,
// profiles/r02/rails/solo_probe*.txt): a workgroup rail (one CU) moves ~120 GB/s of
// load + store traffic and closes a step in ~0.2 us, a one-wave rail ~15 GB/s (up to
// the ~6 TB/s HBM copy rate) and ~0.05 us; the grid engine moves at the copy kernels'
// ~5 TB/s but pays >= 1 us of device-scope barrier per step; a lone busy step outside
// the engine is a copy launch inside the timed region (~8 us).
static bool solo_pays(int64_t bytes, int n, int rails, int wv, int busy, int gran = 16)
{
    const double traffic = 2.0 * (double)bytes;
    // one-wave rails on 4-B / 1-B accesses move a quarter / a sixteenth of the 16-B rate
    const double rail = 15e9 * gran / 16.0;
    const double solo = wv == 1 ? traffic / std::min(rails * rail, 6e12 * gran / 16.0) + n * 0.05e-6
                                : traffic / (rails * 120e9) + n * 0.2e-6;
    const double grid = traffic / 5e12 + n * 1.0e-6 + (busy < 2 ? 8e-6 : 0.0);
    return solo < grid;
}

// The source and destination hull of a list of transfers (empty ones aside): lo = UINTPTR_MAX,
// hi = 0 when none holds bytes.
struct Hull {
    uintptr_t slo = UINTPTR_MAX, shi = 0, dlo = UINTPTR_MAX, dhi = 0;
    void add(uintptr_t src, uintptr_t dst, uint64_t len)
    {
        if (len == 0) return;
        slo = std::min(slo, src); shi = std::max<uintptr_t>(shi, src + len);
        dlo = std::min(dlo, dst); dhi = std::max<uintptr_t>(dhi, dst + len);
    }
    void add(const Hull &h)
    {
        slo = std::min(slo, h.slo); shi = std::max(shi, h.shi);
        dlo = std::min(dlo, h.dlo); dhi = std::max(dhi, h.dhi);
    }
};

static Hull hull_of(const std::vector<xgk::DCopy> &xfer)
{
    Hull h;
    for (const xgk::DCopy &x : xfer)
        if (x.len > 0) h.add((uintptr_t)x.src, (uintptr_t)x.dst, (uint64_t)x.len);
    return h;
}

// 16-B loads per lane per grid unit (1, 4, 16): grows with the segment's largest step so a step
// spreads over up to one workgroup per CU with bytes enough in flight (profiles/r01_engine_sweep.txt:
// small units starve big steps, big units leave small steps on a handful of workgroups).
static int grid_burst(int64_t maxstep) { return maxstep <= (1 << 20) ? 1 : (maxstep <= (4 << 20) ? 4 : 16); }

// One engine segment candidate: steps [s0, s1) with their transfers (chunk-sized pieces
// re-joined), hazard flags, solo granule and shape.  Nothing is committed to the plan.
struct SegCand {
    int s0, s1, n;
    std::vector<std::vector<xgk::DCopy>> xfer;
    std::vector<xg_span> spans;
    std::vector<int> tb, fl;
    int64_t bytes, maxstep;
    int nhaz, gran;
    uintptr_t slo, shi, dlo, dhi;
    xg_solo_shape sh;
    bool fits;                     // the solo tables can be built (limits, alignment, window)
    bool rail_safe;                // no step reads what another writes (xg_engine_rail_safe)
};

static SegCand seg_candidate(const PlanTables *p, const PlanKnobs *c, int s0, int s1)
{
    const std::vector<xgk::DCopy> &pieces = p->pieces;
    SegCand k{};
    k.s0 = s0; k.s1 = s1; k.n = s1 - s0;
    k.xfer.resize(k.n);
    for (int t = s0; t < s1; ++t) {
        const StepR &st = p->steps[t];
        for (int i = st.local_b; i < st.local_b + st.local_n;) {     // eligible steps hold no packs
            const uint8_t *src = pieces[i].src;
            uint8_t *dst = pieces[i].dst;
            int64_t len = pieces[i].len;
            for (++i; i < st.local_b + st.local_n && pieces[i].src == src + len && pieces[i].dst == dst + len; ++i)
                len += pieces[i].len;
            k.xfer[t - s0].push_back({src, dst, len});
        }
        k.bytes += st.local_bytes + st.pack_bytes;
        k.maxstep = std::max(k.maxstep, st.local_bytes + st.pack_bytes);
    }
    k.tb.assign(k.n + 1, 0);
    for (int t = 0; t < k.n; ++t) {
        k.tb[t + 1] = k.tb[t] + (int)k.xfer[t].size();
        for (const xgk::DCopy &x : k.xfer[t])
            k.spans.push_back({(uint64_t)(uintptr_t)x.src, (uint64_t)(uintptr_t)x.dst, (uint64_t)x.len});
    }
    // hazards over whole transfers (host scan)
    k.fl.assign(k.n, 0);
    k.nhaz = xg_engine_hazards(k.spans.data(), k.tb.data(), k.n, c->engine_drain, k.fl.data());
    // solo granule: the largest of 16 / 4 / 1 every transfer is aligned to (segment sizes
    // that are not multiples of 16 move on 4-B or 1-B accesses, one-wave rails only)
    uint64_t bits = 0;
    for (const xg_span &x : k.spans) bits |= x.src | x.dst | x.len;
    k.gran = (bits & 15) == 0 ? 16 : (bits & 3) == 0 ? 4 : 1;
    // solo: each step's 1 KiB pieces dealt round-robin over up to solo_rails rails, per
    // rail rows of XG_SOLO_WAVES pieces (xg_solo_tables_g, host/solo.c)
    Hull h;
    for (const std::vector<xgk::DCopy> &x : k.xfer) h.add(hull_of(x));
    k.slo = h.slo; k.shi = h.shi; k.dlo = h.dlo; k.dhi = h.dhi;
    // Rails never wait for each other, so a segment runs on them only if no step reads what
    // another step writes, in either order: a write-after-read gets no hazard flag (the grid
    // barrier orders it) but races on rails.  Disjoint source and destination hulls (every
    // SEND -> RECV plan) prove it without a scan.
    k.rail_safe = k.shi <= k.dlo || k.dhi <= k.slo ||
                  xg_engine_rail_safe(k.spans.data(), k.tb.data(), k.n) != 0;
    k.fits = (k.gran == 16 || c->solo_waves == 1) && k.shi > k.slo && k.dhi > k.dlo && k.n <= XG_SOLO_MAX_STEPS &&
             k.bytes <= c->solo_max &&
             xg_solo_tables_g(k.spans.data(), k.tb.data(), k.n, c->solo_rails, c->solo_waves, k.gran, k.slo, k.dlo,
                              &k.sh, nullptr, nullptr) == XG_OK;
    return k;
}

// Cut a hazard-free run [s0, s1) that is too long for one solo launch (steps, bytes, pieces
// per rail, the descriptors' offset window) into consecutive sub-runs that each fit, greedily
// from per-step totals; empty if some single step does not fit on its own.
static std::vector<std::pair<int, int>> solo_split(const PlanKnobs *c, const SegCand &k)
{
    std::vector<std::pair<int, int>> out;
    const int64_t rows_cap = XG_SOLO_MAX_PIECES - 3 * XG_SOLO_K * c->solo_waves;   // padding headroom
    const int64_t pieces_cap = (int64_t)c->solo_rails * rows_cap;
    const uint64_t window = (c->solo_waves == 1 ? XG_SOLO_WIDE_OFF_MAX : XG_SOLO_OFF_MAX) * (uint64_t)k.gran;
    int a = k.s0;
    int64_t bytes = 0, np = 0;
    Hull run;
    for (int t = k.s0; t < k.s1; ++t) {
        int64_t tb = 0, tp = 0;
        for (const xgk::DCopy &x : k.xfer[t - k.s0]) {
            if (x.len <= 0) continue;
            tb += x.len;
            tp += (x.len + XG_SOLO_PIECE - 1) / XG_SOLO_PIECE;
        }
        const Hull step = hull_of(k.xfer[t - k.s0]);
        auto ok = [&](int steps, int64_t b, int64_t q, const Hull &h) {
            return steps <= XG_SOLO_MAX_STEPS && b <= c->solo_max && q <= pieces_cap &&
                   (h.shi <= h.slo || h.shi - h.slo <= window) && (h.dhi <= h.dlo || h.dhi - h.dlo <= window);
        };
        if (!ok(1, tb, tp, step)) return {};
        Hull both = run;
        both.add(step);
        if (!ok(t + 1 - a, bytes + tb, np + tp, both)) {
            out.push_back({a, t});
            a = t;
            bytes = np = 0;
            run = Hull();
        }
        bytes += tb;
        np += tp;
        run.add(step);
    }
    out.push_back({a, k.s1});
    return out;
}

// Grid engine vs the same steps as chained copy launches, for a run larger than the
// Infinity Cache (bytes > kGridCacheMax = 256 MiB, the MALL: every
// round of units pays HBM latency and address translation of fresh pages).  Per step, the grid's workgroups take ceil(units / W)
// dependent load -> store rounds of ~2 us each behind a ~0.9 us barrier; a chained
// launch costs a ~2.3 us boundary and moves the step at the copy kernel's rate.  Measured
// (profiles/r02/theta/): P16384 A256 d2048 m1 -c 8 (2048 steps of 2048 two-KiB
// transfers) grid 30.0 ms vs chains 7.0 ms; -c 1 (16384 steps of 256) 60.6 vs 47.3 ms.
static bool grid_pays(const PlanTables *p, const PlanKnobs *c, const SegCand &k)
{
    if (k.bytes <= kGridCacheMax) return true;
    const int64_t unit = (int64_t)grid_burst(k.maxstep) * xgk::kThreads * 16;
    std::vector<int64_t> units(k.n, 0);
    int64_t maxu = 0;
    for (int t = 0; t < k.n; ++t) {
        for (const xgk::DCopy &x : k.xfer[t]) units[t] += (x.len + unit - 1) / unit;
        maxu = std::max(maxu, units[t]);
    }
    const int64_t W = std::max<int64_t>(1, std::min<int64_t>(maxu, c->engine_wmax));
    double grid = 0, chain = 0;
    for (int t = 0; t < k.n; ++t) {
        const StepR &st = p->steps[k.s0 + t];
        const double traffic = 2.0 * (double)(st.local_bytes + st.pack_bytes);
        grid += 0.9e-6 + std::max((double)((units[t] + W - 1) / W) * 2e-6, traffic / 5e12);
        chain += 2.3e-6 + traffic / 5.5e12;
    }
    return grid < chain;
}

// Commit a candidate as an engine segment (solo tables or grid units) to the plan.  Units: the
// step's transfers (chunk-sized pieces re-joined) cut to B * 4 KiB, one burst of B 16-B loads per
// lane per workgroup visit (grid_burst).  Barrier flags: xg_engine_hazards.
static int commit_seg(PlanTables *p, const PlanKnobs *c, SegCand &k, bool solo)
{
    std::vector<xgk::DCopy> &ep = p->ep;
    std::vector<int> &sb = p->sb;
    EngSeg g;
    g.s0 = k.s0; g.s1 = k.s1; g.bytes = k.bytes; g.nhaz = k.nhaz;
    g.solo = solo;
    g.wv = c->solo_waves;
    g.gran = k.gran;
    g.b = grid_burst(k.maxstep);
    g.sb_off = (int)sb.size();
    g.sbase = nullptr;
    g.dbase = nullptr;
    const int n = k.n;
    if (solo) {
        g.sbase = (const uint8_t *)k.slo;
        g.dbase = (uint8_t *)k.dlo;
        g.u0 = (int)p->solo_desc.size();
        g.w = k.sh.rails;
        g.npieces = k.sh.npieces;
        std::vector<int> meta(k.sh.nmeta);
        p->solo_desc.resize(g.u0 + (size_t)k.sh.rails * k.sh.npieces);
        if (xg_solo_tables_g(k.spans.data(), k.tb.data(), n, c->solo_rails, c->solo_waves, k.gran, k.slo, k.dlo, &k.sh,
                             reinterpret_cast<uint64_t *>(p->solo_desc.data()) + g.u0, meta.data()) != XG_OK)
            return XG_EARG;
        sb.insert(sb.end(), meta.begin(), meta.end());
        g.rail_last.resize(k.sh.rails);
        if (xg_solo_rail_last(k.spans.data(), k.tb.data(), n, k.sh.rails, g.rail_last.data()) != XG_OK) return XG_EARG;
    } else {
        // grid units: the step's transfers cut to B * 4 KiB, one burst of B 16-B loads per lane
        const int64_t unit = (int64_t)g.b * xgk::kThreads * 16;
        const int u0 = (int)ep.size();
        std::vector<int> beg(n + 1);
        int maxu = 0;
        for (int t = 0; t < n; ++t) {
            beg[t] = (int)ep.size() - u0;
            for (const xgk::DCopy &x : k.xfer[t])
                for (int64_t o = 0; o < x.len; o += unit)
                    ep.push_back({x.src + o, x.dst + o, x.len - o < unit ? x.len - o : unit});
            maxu = std::max(maxu, (int)ep.size() - u0 - beg[t]);
        }
        beg[n] = (int)ep.size() - u0;
        g.w = std::max(1, std::min(maxu, c->engine_wmax));
        g.npieces = 0;
        g.u0 = 0;
        for (int t = 0; t <= n; ++t) sb.push_back(u0 + beg[t]);
        sb.insert(sb.end(), k.fl.begin(), k.fl.end());
    }
    for (int t = k.s0; t < k.s1; ++t) p->seg_of[t] = (int)p->segs.size();
    p->segs.push_back(g);
    return XG_OK;
}

// The engine segments of a plan from its piece table: every maximal run of >= 2 eligible steps.
static int build_segments(PlanTables *p, const PlanKnobs *c)
{
    p->seg_of.assign(p->nsteps, -1);
    if (c->engine_max_step <= 0) return XG_OK;
    int rc;
    for (int s = 0; s < p->nsteps;) {
        int e = s;
        const int s_run = s;
        while (e < p->nsteps && engine_step(c, p->steps[e])) ++e;
        // steps where this GPU copies nothing cost nothing as their own "launches": trim
        // them off both ends, and keep the run only if >= 2 steps copy something
        const int run_end = e;
        int busy = 0;
        while (s < e && !p->steps[s].pre_n) ++s;
        while (e > s && !p->steps[e - 1].pre_n) --e;
        for (int t = s; t < e; ++t) busy += p->steps[t].pre_n > 0;
        // one busy step is worth an engine launch only as the whole plan: a small one-step
        // plan on rails takes 5 us armed against 6 us (10-24 us cold) as an event-timed copy
        // launch (profiles/r02/one_step/)
        const bool whole = s_run == 0 && run_end == p->nsteps && !c->virt;
        if (busy < (whole ? 1 : 2)) {
            s = run_end > s ? run_end : s + 1;
            continue;
        }
        SegCand k = seg_candidate(p, c, s, e);
        const bool solo = k.nhaz == 0 && k.rail_safe && k.fits && c->solo &&
                          solo_pays(k.bytes, k.n, k.sh.rails, c->solo_waves, busy, k.gran);
        if (!solo && k.nhaz == 0 && k.rail_safe && c->solo && !k.fits && k.n >= 2) {
            // too long for one solo launch (more than XG_SOLO_MAX_STEPS steps -- e.g. a large -k --,
            // more bytes or pieces per rail than one launch holds): consecutive solo launches,
            // each a kernel boundary, when that beats one grid launch's barrier per step
            std::vector<std::pair<int, int>> cut = solo_split(c, k);
            std::vector<SegCand> parts;
            bool all = !cut.empty() && cut.size() > 1;
            for (size_t i = 0; all && i < cut.size(); ++i) {
                parts.push_back(seg_candidate(p, c, cut[i].first, cut[i].second));
                all = parts.back().fits && parts.back().nhaz == 0 && parts.back().rail_safe;
            }
            const double traffic = 2.0 * (double)k.bytes;
            const double grid = traffic / 5e12 + k.n * 1.0e-6;
            const double split = (double)cut.size() * 6e-6 + traffic / (6e12 * k.gran / 16.0) + k.n * 0.05e-6;
            if (all && split < grid) {
                for (SegCand &q : parts)
                    if ((rc = commit_seg(p, c, q, true))) return rc;
                s = e;
                continue;
            }
        }
        if (!solo && busy < 2) {      // one busy step: an engine launch only if it runs solo
            s = run_end;
            continue;
        }
        if (!solo && !grid_pays(p, c, k)) {   // streaming-size run of many small transfers per step
            s = e;
            continue;
        }
        if ((rc = commit_seg(p, c, k, solo))) return rc;
        s = e;
    }
    if (p->segs.empty()) return XG_OK;
    p->stamp_rails = 1;
    for (const EngSeg &g : p->segs)
        if (g.solo) p->stamp_rails = std::max(p->stamp_rails, g.w);
    // a plan that is ONE segment can be armed by xg_plan_run (doorbell in host memory)
    p->may_arm = c->engine_arm && !c->virt && p->segs.size() == 1 && p->segs[0].s0 == 0 && p->segs[0].s1 == p->nsteps;
    return XG_OK;
}

// ------------------------------------------------------------------ steps, pieces, launches
// Pass 1 of a load: per step, what it holds, its RCCL calls and its form (split, fused,
// fused_local, stage_fused, deferred, self_local).  false: a descriptor outside its region.
static bool step_forms(PlanTables *p, const PlanKnobs *c, const xg_devplan *dp)
{
    p->steps.resize(dp->nsteps);
    for (int s = 0; s < dp->nsteps; ++s) {
        const xg_stepplan &sp = dp->steps[s];
        StepR &st = p->steps[s];
        if (sp.stage_count < 0 || sp.stage_count > sp.pre_count || sp.post_count < 0) return false;
        int nloc = 0, npack = 0;
        for (int i = sp.stage_count; i < sp.pre_count; ++i) {
            const bool pack = dp->copies[sp.pre_begin + i].dst_buf == XG_BUF_STAGE_SEND;
            if (!pack && npack) return false;                   // the plan lists local copies, then packs
            (pack ? npack : nloc) += dp->copies[sp.pre_begin + i].len > 0;
        }
        for (int i = 0; i < sp.post_count; ++i)
            if (dp->copies[sp.post_begin + i].src_buf != XG_BUF_STAGE_RECV) return false;   // post copies unpack
        // the step's RCCL calls: exactly what libxghost says this GPU posts (calls.c)
        const int nc = xg_devplan_step_calls(dp, s, c->self_max, nullptr);
        if (nc < 0) return false;
        st.self_local = xg_devplan_step_self_calls(dp, s, c->self_max) > 0;
        st.call_b = (int)p->calls.size();
        st.call_n = nc;
        p->call_begin.push_back(st.call_b);
        p->calls.resize(st.call_b + nc);
        xg_devplan_step_calls(dp, s, c->self_max, p->calls.data() + st.call_b);
        st.posts = sp.posts;
        for (int i = 0; i < nc; ++i) {
            const xg_call &o = p->calls[st.call_b + i];
            if (o.kind == XG_CALL_BARRIER) {
                st.sync_after = c->nranks > 1;
                continue;
            }
            if (o.kind == XG_CALL_FENCE) {        // a relay step's second RCCL group follows
                st.groups++;
                continue;
            }
            if ((o.kind != XG_CALL_SEND && o.kind != XG_CALL_RECV) || o.peer < 0 || o.peer >= c->nranks ||
                (o.peer == c->rank && !st.self_local) || o.buf < 0 || o.buf >= XG_NBUF || o.off < 0 ||
                o.len < 0 || o.off + o.len > p->bytes[o.buf])
                return false;
            st.p2p_n++;
        }
        if (st.self_local) nloc = 0;        // the local copies travel in the step's RCCL group
        int64_t b_loc = 0;
        for (int i = sp.stage_count; i < sp.pre_count; ++i)
            if (dp->copies[sp.pre_begin + i].dst_buf != XG_BUF_STAGE_SEND && !st.self_local)
                b_loc += std::max<int64_t>(0, dp->copies[sp.pre_begin + i].len);
        // a cross-GPU step's local part runs on the side stream beside the packs and the RCCL
        // group (split) when it is large enough to pay for the fork / join; a smaller one joins
        // the step's first launch -- the fused one too, if it touches none of the bytes the
        // previous step's unpacks write (then the step is ONE copy launch + its RCCL group).
        // The fused launch itself holds step s-1's unpacks and this step's packs, its workgroups
        // in any order: never when a pack reads (forwards) bytes those unpacks write, whatever
        // becomes of the local part.  A split local part forks behind that launch.
        st.split = st.p2p_n > 0 && nloc > 0 && b_loc >= c->split_min;
        const bool prev_ok = s > 0 && npack > 0 && sp.stage_count == 0 &&
                             !p->steps[s - 1].sync_after && dp->steps[s - 1].post_count > 0;
        st.fused = prev_ok && xg_step_packs_meet_unpacks(dp, s) == 0 &&
                   (st.split || nloc == 0 || !xg_step_local_meets_unpacks(dp, s));
        st.fused_local = st.fused && !st.split && nloc > 0;
        // TAM: a step's stage copies share the local (+ pack) launch when none of those meets
        // their bytes -- README m15 / m16 step 3: 6 -> 5 launches per run
        st.stage_fused = c->fuse_stage && sp.stage_count > 0 && (nloc > 0 || npack > 0) && !st.split &&
                         !st.fused && !st.self_local && xg_step_stage_meets_rest(dp, s) == 0;
        if (st.fused) p->steps[s - 1].deferred = true;
    }
    p->call_begin.push_back((int32_t)p->calls.size());
    return true;
}

// Whether one run copies more than the Infinity Cache holds: decides each launch's variant
// (copy_variant).
static bool plan_streams(const PlanTables *p, const xg_devplan *dp)
{
    // the bytes one run copies (as the StepR totals add them up)
    int64_t run = 0;
    for (int s = 0; s < dp->nsteps; ++s) {
        const xg_stepplan &sp = dp->steps[s];
        for (int i = 0; i < sp.pre_count; ++i) {
            const xg_copy &cp = dp->copies[sp.pre_begin + i];
            const bool local = i >= sp.stage_count && cp.dst_buf != XG_BUF_STAGE_SEND;
            if (!(local && p->steps[s].self_local)) run += std::max<int64_t>(0, cp.len);
        }
        for (int i = 0; i < sp.post_count; ++i) run += std::max<int64_t>(0, dp->copies[sp.post_begin + i].len);
    }
    // ... and whether its regions could hold in it at all: -k repetitions re-copy the same
    // bytes, so a run of many small repetitions (P32 A14 -d 64 KiB -k 50: 56 MiB of
    // regions, 2.8 GB copied) stays cache-resident and copies with plain stores
    int64_t foot = 0;
    for (int i = 0; i < XG_NBUF; ++i) foot += std::max<int64_t>(0, dp->region_bytes[i]);
    return std::min(2 * run, foot) > ((int64_t)256 << 20);
}

// The copy kernel variant of a launch moving `bytes`.  Variant 0 picks non-temporal
// loads/stores (6) when the bytes cannot come back from the 256 MiB Infinity Cache: a
// launch whose own source + destination exceed it, or a launch of >= kNtStream bytes in a
// plan whose run copies more than it (every step then finds its bytes evicted by the steps
// before) -- unless what it writes is read again at once (`reread`: packs feeding RCCL, TAM
// stage copies), which then may still find it in the cache; plain (1) otherwise.
static int copy_variant(const PlanTables *p, int64_t bytes, bool reread)
{
    if (p->variant) return p->variant;
    return bytes >= kNtMin || (!reread && p->streaming && bytes >= kNtStream) ? 6 : 1;
}

// Pass 2 of a load: the piece table and the launch table together, launch by launch -- a
// launch's pieces are contiguous and cut for that launch's bytes, and its table entry (kernel
// form, stream, mark) is decided where its pieces are cut.  Host work only.
struct TableBuilder {
    typedef std::pair<int, int> Range;      // copies [first, first + second) of dp->copies
    PlanTables *p;
    const PlanKnobs *c;
    const xg_devplan *dp;
    std::vector<xgk::DCopy> &pieces;
    DisplScan &ds;
    int64_t chunk = 0;                      // bytes per piece of the open launch
    CopyLaunch *cur = nullptr;              // the open launch

    int64_t bytes_of(Range rg) const
    {
        int64_t n = 0;
        for (int i = 0; i < rg.second; ++i) n += std::max<int64_t>(0, dp->copies[rg.first + i].len);
        return n;
    }

    // Open launch `l` over the copies of `ranges`: its first piece, its bytes, its kernel kind and
    // the size its pieces are cut to.  Three steps: the facts of the launch, gathered in one pass
    // over its copies; the choice, by xg_copy_launch_choose (libxghost, pieces.c -- the precedence
    // of the five kinds is written there, in xg_sched.h, and nowhere else); the choice recorded.
    // One piece per workgroup.  Bytes per piece (xg_piece_size): rules.chunk (32 KiB:
    // profiles/r01_copy_ab.txt) or chunk / 2, / 4, / 8 (>= 4 KiB; a halving keeps dividing the
    // power-of-two segment sizes: no ragged tail piece per segment, profiles/r01_min_pieces_ab.txt),
    // whichever gives the least work to the busiest CU: a launch of w pieces of c bytes puts
    // ceil(w / CUs) pieces on some CU, each costing c bytes plus a fixed per-workgroup start (kWgCost
    // = 2 KiB bytes-equivalent); ties keep the larger piece.  A 28 MiB pack of 256 KiB segments: 896
    // pieces of 32 KiB = 3.5 per CU (the busiest 4 x 32 KiB) -> 1792 of 16 KiB = exactly 7
    // (7 x 16 KiB).  The bench's 448 MiB launches stay 32 KiB (56 per CU).  (A rule forcing
    // >= 2 x CUs pieces on small launches was measured 3-7 % slower and dropped:
    // profiles/r03/min_wg/summary.txt.)
    // `cross`: a launch of a cross-GPU step (packs, unpacks, its local part), or of a GPU-local
    // step too large for the step engine: a WAVE launch when plain, aligned and of wave_min ..
    // kWaveMax bytes (profiles/r03/wave_copy/).
    // `reread` (copy_variant) comes twice: for the cut of the pieces and for the kernel.  They
    // differ in one launch only (step(), the local + pack launch); where the cut says plain and
    // the kernel non-temporal, the wave-sized pieces run copy_kernel_g<4, true>.
    // `may_small`: a step's own local (+ pack) launch, SMALL when it is uniform, aligned, holds no
    // pack and moves >= small_piece_min bytes: its copies are listed as rows (add), no piece is cut
    // at all.  The bench's 448 MiB launches: 114,688 / 57,344 workgroups from 448 rows.
    void open(CopyLaunch &l, std::initializer_list<Range> ranges, bool cross, bool reread_cut, bool reread_run,
              bool may_small = false)
    {
        const xg_copy_rules &r = c->rules;
        cur = &l;
        l.b = (int)pieces.size();
        chunk = r.chunk;
        xg_launch_facts f{};
        std::vector<int64_t> lens;
        for (const Range &rg : ranges)
            for (int i = 0; i < rg.second; ++i) {
                lens.push_back(dp->copies[rg.first + i].len);
                xg_launch_facts_add(&f, &dp->copies[rg.first + i]);
            }
        l.bytes = f.bytes;
        if (l.bytes <= 0) return;
        f.lens = lens.data();
        f.nlens = (int)lens.size();
        f.dp_flags = dp->flags;
        f.cross = cross;
        f.may_small = may_small;
        f.nt_cut = copy_variant(p, l.bytes, reread_cut) == 6;
        f.nt_run = copy_variant(p, l.bytes, reread_run) == 6;
        xg_copy_choice ch;
        xg_copy_launch_choose(&f, &r, &ch);         // bytes > 0: it cannot refuse
        l.kind = ch.kind;
        l.nt = ch.nt;
        l.kib = ch.kib;
        chunk = ch.piece;
        if (l.kind == XG_COPY_SMALL) {
            l.q_len = f.uniform_len;
            l.q_k = ch.order;
            l.q_row = (int)p->rows.size();
        }
    }
    // a copy_kernel_q launch: its rows in destination order (order_pieces, for a launch without pieces)
    void close()
    {
        cur->n = (int)pieces.size() - cur->b;
        if (cur->kind != XG_COPY_SMALL) return;
        cur->q_copies = (int)p->rows.size() - cur->q_row;
        std::stable_sort(p->rows.begin() + cur->q_row, p->rows.end(),
                         [](const xgk::DCopy &x, const xgk::DCopy &y) { return x.dst < y.dst; });
    }

    const uint8_t *at(int buf, int64_t off) const { return (const uint8_t *)(uintptr_t)(p->base[buf] + (uint64_t)off); }

    // side: -1 plain copy; 0 pack (destination in STAGE_SEND, displacement from the
    // device scan); 1 unpack (source in STAGE_RECV, likewise)
    bool add(const xg_copy &cp, int side)
    {
        if (cp.len <= 0) return true;
        if (cp.src_buf < 0 || cp.src_buf >= XG_NBUF || cp.dst_buf < 0 || cp.dst_buf >= XG_NBUF) return false;
        if (cp.src_off < 0 || cp.dst_off < 0 || cp.src_off + cp.len > p->bytes[cp.src_buf] ||
            cp.dst_off + cp.len > p->bytes[cp.dst_buf])
            return false;
        if (cur->kind == XG_COPY_SMALL) {        // one row per copy; the kernel cuts it (open() let no pack or unpack in)
            p->rows.push_back({at(cp.src_buf, cp.src_off), (uint8_t *)at(cp.dst_buf, cp.dst_off), cp.len});
            return side < 0;
        }
        const int ci = (int)ds.len.size();
        if (side >= 0) {
            ds.len.push_back(cp.len);
            ds.host.push_back(side == 0 ? cp.dst_off : cp.src_off);
        }
        for (int64_t o = 0; o < cp.len; o += chunk) {
            xgk::DCopy d;
            // staging side of a packed copy: displacement 0 until the device scan patches it
            d.src = at(cp.src_buf, (side == 1 ? 0 : cp.src_off) + o);
            d.dst = (uint8_t *)at(cp.dst_buf, (side == 0 ? 0 : cp.dst_off) + o);
            d.len = cp.len - o < chunk ? cp.len - o : chunk;
            if (side >= 0) ds.fix.push_back({(int)pieces.size(), ci, o, side, 0});
            pieces.push_back(d);
        }
        return true;
    }
    bool add_range(Range rg, int side)
    {
        for (int i = 0; i < rg.second; ++i)
            if (!add(dp->copies[rg.first + i], side)) return false;
        return true;
    }
    int64_t span(int b) const
    {
        int64_t n = 0;
        for (int i = b; i < (int)pieces.size(); ++i) n += pieces[i].len;
        return n;
    }
    // step t's unpacks, into the open launch (t's own, or the fused launch of step t + 1)
    bool add_post(int t)
    {
        const xg_stepplan &tp = dp->steps[t];
        StepR &tt = p->steps[t];
        tt.post_b = (int)pieces.size();
        if (!add_range({tp.post_begin, tp.post_count}, 1)) return false;
        ds.close_group();
        tt.post_n = (int)pieces.size() - tt.post_b;
        tt.post_bytes = span(tt.post_b);
        return true;
    }

    // One step: at most four launches -- stage | local | packs | unpacks, in piece order.
    //   stage_fused: stage, local and packs are ONE launch (`local`; the stage pieces count as
    //   local ones); fused_local: the previous step's unpacks, local and packs are ONE launch
    //   (`local`); split: `local` alone on the side stream, `pack` (fused: with the previous
    //   unpacks in front) on the main one; fused with no local copies: `pack` alone; else local
    //   and packs are ONE launch (`local`).
    bool step(int s)
    {
        const xg_stepplan &sp = dp->steps[s];
        StepR &st = p->steps[s];
        int first_pack = sp.pre_count;
        for (int i = sp.stage_count; i < sp.pre_count; ++i)
            if (dp->copies[sp.pre_begin + i].dst_buf == XG_BUF_STAGE_SEND) {
                first_pack = i;
                break;
            }
        const Range r_stage{sp.pre_begin, sp.stage_count},
            r_local{sp.pre_begin + sp.stage_count, st.self_local ? 0 : first_pack - sp.stage_count},
            r_pack{sp.pre_begin + first_pack, sp.pre_count - first_pack},
            r_prev{st.fused ? dp->steps[s - 1].post_begin : 0, st.fused ? dp->steps[s - 1].post_count : 0},
            r_post{sp.post_begin, sp.post_count};
        // a GPU-local step's launch counts as cross too when it cannot be an engine step (larger
        // than engine_max_step, or the engine off): one large one-off launch
        const bool cross = st.p2p_n > 0 || r_pack.second > 0 || c->engine_max_step <= 0 ||
                           bytes_of(r_local) > c->engine_max_step;
        CopyLaunch stage, local, pack, post;        // n stays 0: the step has no such launch
        st.stage_b = (int)pieces.size();
        if (st.stage_fused) {
            open(local, {r_stage, r_local, r_pack}, cross, true, true);
            if (!add_range(r_stage, -1)) return false;
        } else {
            open(stage, {r_stage}, false, true, true);      // read again at once by the step's own copies
            if (!add_range(r_stage, -1)) return false;
            close();
            st.stage_n = stage.n;
            st.stage_bytes = stage.bytes;
            if (st.fused_local) {
                open(local, {r_prev, r_local, r_pack}, true, true, true);
                local.mark_prev = true;
                if (!add_post(s - 1)) return false;
            } else if (st.split) {
                open(local, {r_local}, true, false, false, true);
                local.side = true;
            } else if (!st.fused) {
                // the cut asks whether the step lists packs, the kernel whether any holds bytes:
                // they part for a step whose packs are all empty
                open(local, {r_local, r_pack}, cross, r_pack.second > 0, bytes_of(r_pack) > 0, true);
            }
        }
        st.local_b = st.stage_fused ? st.stage_b : (int)pieces.size();
        if (!add_range(r_local, -1)) return false;
        st.local_n = (int)pieces.size() - st.local_b;
        st.local_bytes = span(st.local_b);
        if (local.kind == XG_COPY_SMALL) {       // rows, not pieces
            st.small = true;
            st.local_bytes = local.bytes;
        }
        if (st.split || (st.fused && !st.fused_local)) {
            if (st.split) close();
            open(pack, {r_prev, r_pack}, true, true, true);
            pack.mark_prev = st.fused;
            if (st.fused && !add_post(s - 1)) return false;
        }
        st.pack_b = (int)pieces.size();
        if (!add_range(r_pack, 0)) return false;
        ds.close_group();
        st.pack_n = (int)pieces.size() - st.pack_b;
        st.pack_bytes = span(st.pack_b);
        st.pre_n = st.local_n + st.pack_n;
        close();
        st.post_b = (int)pieces.size();
        if (!st.deferred) {
            open(post, {r_post}, true, false, false);
            if (!add_post(s)) return false;
            close();
        }
        // issue order.  A fused launch ends the previous step, so it goes before anything of this
        // one.  The packs feed the RCCL group (the critical path), the local part does not: by
        // default the local part forks after the pack launch, so it overlaps the transfer instead
        // of sharing HBM with the packs (XG_SPLIT_AFTER_PACK=0: both at once, as in round 2)
        std::vector<CopyLaunch> &tab = p->launches;
        auto push = [&](const CopyLaunch &l) {
            if (l.n > 0 || l.kind == XG_COPY_SMALL) tab.push_back(l);
        };
        const bool pack_first = st.fused || c->split_after_pack;
        st.l_b = (int)tab.size();
        push(stage);
        if (pack_first) push(pack);
        push(local);
        if (!pack_first) push(pack);
        st.l_rccl = (int)tab.size();
        push(post);
        st.l_e = (int)tab.size();
        return true;
    }
};

static bool build_tables(PlanTables *p, const PlanKnobs *c, const xg_devplan *dp)
{
    TableBuilder tb{p, c, dp, p->pieces, p->ds};
    for (int s = 0; s < dp->nsteps; ++s)
        if (!tb.step(s)) return false;
    return true;
}

// Order of a launch's local pieces (workgroup i copies piece i): by destination address.
// The workgroups in flight at any moment then write a few consecutive segments instead of
// one piece in each of dozens of scattered slots -- 7-10 % shorter all-to-many launches
// (DRAM row locality of the write stream; message or source order measured slower,
// profiles/r02/piece_order/; so did dealing each XCD its own eighth, 3-8 %,
// profiles/r04/xcd_order/).  Local pieces carry no displacement fix-ups and a launch's
// pieces are independent, so any order is valid.
// Unpack pieces (source in staging, patched by the device scan) are ordered by their
// destination too, with their fix-ups renumbered.
static void order_pieces(PlanTables *p)
{
    std::vector<xgk::DCopy> &pieces = p->pieces;
    DisplScan &ds = p->ds;
    auto key_less = [](const xgk::DCopy &x, const xgk::DCopy &y) { return x.dst < y.dst; };
    for (const StepR &st : p->steps)
        std::stable_sort(pieces.begin() + st.local_b, pieces.begin() + st.local_b + st.local_n, key_less);
    std::vector<int> where(pieces.size(), -1);      // old index -> its fix-up
    for (size_t f = 0; f < ds.fix.size(); ++f) where[ds.fix[f].piece] = (int)f;
    for (const StepR &st : p->steps) {
        if (st.post_n < 2) continue;
        std::vector<int> idx(st.post_n);
        for (int i = 0; i < st.post_n; ++i) idx[i] = st.post_b + i;
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return pieces[x].dst < pieces[y].dst; });
        std::vector<xgk::DCopy> sorted(st.post_n);
        for (int i = 0; i < st.post_n; ++i) sorted[i] = pieces[idx[i]];
        for (int i = 0; i < st.post_n; ++i) {
            const int f = where[idx[i]];
            if (f >= 0) ds.fix[f].piece = st.post_b + i;
        }
        std::copy(sorted.begin(), sorted.end(), pieces.begin() + st.post_b);
    }
}

// The dispatches of a copy_kernel_q launch: its cuts are workgroup indices (0 .. its workgroups), a
// dispatch is about launch_max bytes of whole pieces -- a cut may fall inside a copy, the kernel
// takes the dispatch's first workgroup as `base` -- and no runt dispatch closes the launch.  The
// bytes of each dispatch (kernel-timing sessions) are summed here once, through the index function.
static void cut_small(PlanTables *p, const PlanKnobs *c, CopyLaunch &l)
{
    const int64_t cap = c->launch_max, piece = (int64_t)l.kib << 10;
    const int64_t W = (int64_t)l.q_copies * xg_small_ppc(l.q_len, piece);
    l.cut = (int)p->cuts.size();
    p->cuts.push_back(0);
    if (cap > 0 && l.bytes > cap + cap / 2) {
        const int64_t per = std::max<int64_t>(1, cap / piece);
        for (int64_t o = per; o < W && (W - o) * piece >= cap / 2 && W - o >= 16; o += per) p->cuts.push_back((int)o);
    }
    p->cuts.push_back((int)W);
    l.ndisp = (int)p->cuts.size() - 1 - l.cut;
    l.q_bytes = (int)p->qbytes.size();
    for (int k = 0; k < l.ndisp; ++k) {
        int64_t nb = 0;
        for (int64_t b = p->cuts[l.cut + k]; b < p->cuts[l.cut + k + 1]; ++b)
            nb += xg_small_index((uint32_t)b, (uint32_t)l.q_copies, l.q_len, piece, (uint32_t)l.q_k).n;
        p->qbytes.push_back(nb);
    }
}

// Each launch's dispatches.  A launch of more than 1.5 x launch_max bytes goes as back-to-back
// kernel dispatches of about launch_max bytes each (its pieces are independent: the same step,
// a few more kernel boundaries).  P256 A32 -d 4 MiB m1 / m2 (one 32 GiB step, 1 M pieces):
// 12.6 -> 11.0 ms at 512 MiB per dispatch, 11.5 at 128 MiB; cutting by piece count instead
// hurt steps of small pieces (profiles/r02/launch_split/).  Every count of launches
// (xg_plan_launches, the kernel-timing sessions) counts these dispatches, as rocprofv3 does.
static void cut_launches(PlanTables *p, const PlanKnobs *c)
{
    const int64_t cap = c->launch_max;
    const int64_t *pre = p->plen.data();        // prefix sums of the piece lengths
    for (CopyLaunch &l : p->launches) {
        if (l.kind == XG_COPY_SMALL) {
            cut_small(p, c, l);
            continue;
        }
        const int end = l.b + l.n;
        l.cut = (int)p->cuts.size();
        p->cuts.push_back(l.b);
        for (int o = l.b; cap > 0 && l.bytes > cap + cap / 2 && o < end;) {
            // the first piece boundary at least cap bytes past o (lower_bound may return end + 1
            // when fewer than cap bytes remain: clamp), then no runt dispatch at the end
            int e = (int)(std::lower_bound(pre + o + 1, pre + end + 1, pre[o] + cap) - pre);
            if (e > end) e = end;
            if (end - e < 16 || pre[end] - pre[e] < cap / 2) e = end;
            if (e < end) p->cuts.push_back(e);
            o = e;
        }
        p->cuts.push_back(end);
        l.ndisp = (int)p->cuts.size() - 1 - l.cut;
    }
}

// The tile table of every dispatch of every copy_kernel_x launch: xg_extent_tiles (libxghost) over the
// dispatch's pieces as they are ordered and cut, so a dispatch's tiles cover exactly its pieces.
static bool tile_launches(PlanTables *p, const PlanKnobs *c)
{
    std::vector<int64_t> lens;
    std::vector<int32_t> begin;
    for (CopyLaunch &l : p->launches) {
        if (l.kind != XG_COPY_EXTENT) continue;
        l.xt = (int)p->xt_off.size();
        for (int k = 0; k < l.ndisp; ++k) {
            const int b = p->cuts[l.cut + k], n = p->cuts[l.cut + k + 1] - b;
            lens.resize(n);
            for (int i = 0; i < n; ++i) lens[i] = p->plen[b + i + 1] - p->plen[b + i];
            begin.resize((size_t)n + 1);
            const int nt = xg_extent_tiles(lens.data(), n, c->extent_tile, kExtTilePieces, begin.data());
            if (nt < 0 || (n > 0 && (nt == 0 || begin[0] != 0 || begin[nt] != n))) return false;
            p->xt_off.push_back((int)p->xt_begin.size());
            p->xt_n.push_back(nt);
            p->xt_begin.insert(p->xt_begin.end(), begin.begin(), begin.begin() + nt + 1);
        }
    }
    return true;
}

// Chains (PlanTables::chain_end).  A chain step: no engine segment's, no RCCL, no unpack, no
// barrier, and every launch of it on the main stream (every copy kernel can stamp its start).
static bool find_chains(PlanTables *p)
{
    auto chain_step = [&](int s) {
        const StepR &st = p->steps[s];
        if (p->seg_of[s] >= 0 || st.l_e == st.l_b || st.l_rccl != st.l_e || st.p2p_n || st.sync_after ||
            st.pack_n || st.deferred)
            return false;
        for (int i = st.l_b; i < st.l_e; ++i) {
            const CopyLaunch &l = p->launches[i];
            if (l.side || l.mark_prev) return false;
        }
        return true;
    };
    bool any = false;
    for (int s = 0; s < p->nsteps;) {
        int e = s;
        while (e < p->nsteps && chain_step(e)) ++e;
        if (e - s >= 2) {
            p->chain_end[s] = e;
            any = true;
        }
        s = e > s ? e : s + 1;
    }
    return any;
}

int plan_tables_build(PlanTables *p, const xg_devplan *dp, const PlanKnobs *c, const uint64_t base[XG_NBUF],
                      const int64_t bytes[XG_NBUF])
{
    p->nsteps = dp->nsteps;
    p->variant = c->variant;
    p->wave_grid = c->wave_grid;
    memcpy(p->base, base, sizeof p->base);
    memcpy(p->bytes, bytes, sizeof p->bytes);
    if (!step_forms(p, c, dp) || (p->streaming = plan_streams(p, dp), !build_tables(p, c, dp))) {
        fprintf(stderr, "xg_plan_load: copy or p2p descriptor outside its region\n");
        return XG_EARG;
    }
    order_pieces(p);
    const std::vector<xgk::DCopy> &pieces = p->pieces;
    p->npieces = (int)pieces.size();
    p->plen.assign(pieces.size() + 1, 0);
    for (size_t i = 0; i < pieces.size(); ++i) p->plen[i + 1] = p->plen[i] + pieces[i].len;
    cut_launches(p, c);
    if (!tile_launches(p, c)) {
        fprintf(stderr, "xg_plan_load: the tiles of a copy_kernel_x dispatch do not cover its pieces\n");
        return XG_EARG;
    }
    if (const int rc = build_segments(p, c)) return rc;
    p->chain_end.assign(p->nsteps, 0);
    p->any_chain = c->step_chain && find_chains(p);
    // kernel dispatches per run: an engine segment is one, every other step its table entries'
    p->nlaunch = (int)p->segs.size();
    each_launch(p, [&](const CopyLaunch &l) { p->nlaunch += l.ndisp; });
    int64_t run = 0;
    for (const StepR &st : p->steps) run += st.stage_bytes + st.local_bytes + st.pack_bytes + st.post_bytes;
    // a one-GPU run of several small launches is bound by launching them, not by their
    // bytes: replayed as one graph (README TAM chains 17-19 -> 15-16 us,
    // profiles/r03/readme_cli/summary.txt).  Multi-GPU and virtual runs stay launched:
    // graphs of RCCL and cross-stream nodes replayed 1.1-5x slower (profiles/r03/hybrid/)
    p->graph_auto = c->nranks == 1 && !c->virt && run <= ((int64_t)16 << 20);
    return XG_OK;
}

// ------------------------------------------------------------------ the C surface (xg_sched.h)
extern "C" void xg_plan_knobs_default(xg_plan_knobs *k, int cus, int engine_occ, int wave_grid)
{
    memset(k, 0, sizeof *k);
    k->rules.chunk = 32768;                   // profiles/r01_copy_ab.txt
    k->rules.wg_cost = kWgCost;
    k->rules.wave_min = (int64_t)1 << 20;
    k->rules.wave_max = kWaveMax;
    k->rules.extent_mean_max = kExtMeanMax;
    k->rules.small_piece_min = kSmallMin;
    k->rules.cus = cus > 0 ? cus : 256;
    k->rules.wave_kib = 0;
    k->rules.ragged_copy = 1;
    k->rules.extent_copy = kExtDefault;
    k->rules.small_pieces = kSmallDefault;
    k->rules.small_kib = kSmallKiB;
    k->rules.small_order = kSmallOrder;
    k->extent_tile = kExtTileBytes;
    k->engine_max_step = 16 << 20;            // crossover vs one launch per step: profiles/r01_engine_sweep.txt
    // the engine's grid barrier needs every workgroup resident at once: at most one
    // per CU by design, never more than the device admits (a partitioned device has
    // fewer CUs; several ranks per GPU share them)
    k->engine_wmax = std::max(1, std::min(cus, engine_occ));
    k->solo = 1;
    // one solo launch moves <= 1 GiB (2048 pieces per one-wave rail of 512; the wide
    // descriptors have no window below that): the Theta-scale runs split into 8 launches
    // instead of 32, 5-6 % faster (profiles/r02/theta/theta_probe_solo_max.txt)
    k->solo_max = (int64_t)1 << 30;
    k->solo_waves = 1;
    k->solo_rails = 512;                      // 512 one-wave rails: 2 per CU by LDS
    k->launch_max = (int64_t)512 << 20;
    k->wave_grid = wave_grid;
    k->step_chain = 1;
    k->split_min = (int64_t)1 << 20;
    k->self_max = (int64_t)256 << 10;
    k->fuse_stage = 1;
    k->split_after_pack = 1;
    k->nranks = 1;
}

// ---- the knobs' environment: the rules several variables share, then one row per variable.  v is
// the variable's value, NULL when unset (atoi / atoll read "" and "abc" as 0, "1x" as 1).
static void off_if_0(int32_t *f, const char *v) { *f = !(v && !strcmp(v, "0")); }     // off for exactly "0"; written even unset
static void on_if_1(int32_t *f, const char *v) { *f = v && !strcmp(v, "1"); }         // on for exactly "1"; written even unset
static void flag(int32_t *f, const char *v) { if (v) *f = atoi(v) != 0; }             // a set variable always writes
static void number(int64_t *f, const char *v, int64_t lo = INT64_MIN) { if (v && atoll(v) >= lo) *f = atoll(v); }
// a positive value lowers the field, never raises it
static void cap(int32_t *f, const char *v) { if (v && atoi(v) > 0) *f = std::max(1, std::min(*f, atoi(v))); }

struct Knob {
    const char *name;
    void (*apply)(xg_plan_knobs *k, const char *v);
};
#define KNOB(name, ...) {name, [](xg_plan_knobs *k, const char *v) { __VA_ARGS__; }}
static const Knob kKnobs[] = {
    KNOB("XG_COPY_VARIANT",                  // 0 by size (default), 1 plain, 6 non-temporal
         if (v && (atoi(v) == 1 || atoi(v) == 6)) k->variant = atoi(v);
         else if (v && atoi(v) != 0) fprintf(stderr, "xg: XG_COPY_VARIANT=%s ignored (0, 1 or 6)\n", v)),
    // "0": a ragged plan's misaligned launches stay on copy_kernel_g (A/B)
    KNOB("XG_RAGGED_COPY", if (v && atoi(v) == 0) k->rules.ragged_copy = 0),
    // copy_kernel_x for a placement plan's launches of short extents (xg_copy_launch_choose): "0" keeps
    // them on copy_kernel_s.  XG_EXTENT_MEAN_MAX / XG_EXTENT_TILE_KIB: the routing threshold and the
    // tile's byte cap, for the A/B of profiles/extent_copy_ab.py
    KNOB("XG_EXTENT_COPY", flag(&k->rules.extent_copy, v)),
    KNOB("XG_EXTENT_MEAN_MAX", number(&k->rules.extent_mean_max, v, 1)),
    KNOB("XG_EXTENT_TILE_KIB", if (v && atoi(v) > 0 && atoi(v) <= 1024) k->extent_tile = (int64_t)atoi(v) << 10),
    // copy_kernel_q for large uniform launches (xg_copy_launch_choose): "0" restores copy_kernel_g's
    // 32 KiB pieces.  XG_SMALL_PIECE_MIN: test hook, the launch size it starts at;
    // XG_SMALL_PIECE_KIB (4 / 8) and XG_SMALL_PIECE_ORDER (copies per group of the piece order):
    // for the A/B of profiles/small_pieces_ab.sh
    KNOB("XG_SMALL_PIECES", flag(&k->rules.small_pieces, v)),
    KNOB("XG_SMALL_PIECE_MIN", number(&k->rules.small_piece_min, v, 0)),
    KNOB("XG_SMALL_PIECE_KIB", if (v && (atoi(v) == 4 || atoi(v) == 8)) k->rules.small_kib = atoi(v)),
    KNOB("XG_SMALL_PIECE_ORDER", if (v && atoi(v) >= 1 && atoi(v) <= 1024) k->rules.small_order = atoi(v)),
    KNOB("XG_ENGINE_MAX_STEP", number(&k->engine_max_step, v)),      // 0: never use the step engine
    // test hook: a positive value caps the grid engine's workgroups (never raises them), so that a
    // step's bytes are confined to a known number of CUs
    KNOB("XG_ENGINE_WG", cap(&k->engine_wmax, v)),
    KNOB("XG_ENGINE_DRAIN", on_if_1(&k->engine_drain, v)),           // "1": drain every step even without a hazard
    KNOB("XG_ENGINE_SOLO", off_if_0(&k->solo, v)),                   // "0": never solo (the grid engine runs every segment)
    KNOB("XG_ENGINE_SOLO_MAX", number(&k->solo_max, v)),
    // waves per rail: 1 (default) or 16.  The rails' default follows the waves, so this row stands
    // before XG_SOLO_RAILS'.  See DESIGN.md (solo engine): profiles/r02/rails/solo_probe.txt
    KNOB("XG_SOLO_WAVES", k->solo_waves = v && atoi(v) == XG_SOLO_WAVES ? XG_SOLO_WAVES : 1;
         k->solo_rails = k->solo_waves == 1 ? 512 : 16),             // 512 one-wave rails: 2 per CU by LDS
    KNOB("XG_SOLO_RAILS", if (v && atoi(v) > 0) k->solo_rails = std::min(atoi(v), XG_SOLO_MAX_RAILS)),
    KNOB("XG_COPY_LAUNCH_MAX", number(&k->launch_max, v)),           // bytes; 0 = one launch however large
    // the wave-persistent copy for the launches of cross-GPU steps (packs, unpacks, the
    // local part): profiles/r03/wave_copy/ -- one GPU's configs[2] pack launch 5.8 ->
    // 6.25 TB/s; the 448 MiB non-temporal launches stay copy_kernel_g (6.0 vs 5.5-5.8);
    // above kWaveMax the one-piece-per-workgroup launch is as fast or faster
    // (profiles/r03/wave_local/: 28 MiB 9.3 vs 9.9 us, 56 MiB 18.7 vs 18.2, 112 MiB equal)
    KNOB("XG_COPY_WAVE_MIN", number(&k->rules.wave_min, v)),         // test hook: 0 puts every cross-GPU launch on the wave copy
    // test hook: a positive value caps the grid (never raises it), so that a wave gets several
    // pieces -- on a whole device every launch of <= kWaveMax bytes has one piece per wave
    KNOB("XG_WAVE_GRID", cap(&k->wave_grid, v)),
    // piece KiB of a wave-copy launch: 0 = by its bytes (pieces.c), 2 / 4 / 8 forced (A/B)
    KNOB("XG_WAVE_KIB", k->rules.wave_kib = v && (atoi(v) == 2 || atoi(v) == 4 || atoi(v) == 8) ? atoi(v) : 0),
    KNOB("XG_STEP_CHAIN", off_if_0(&k->step_chain, v)),              // "0": a step mark after every step launch
    // "1": arm single-segment plans (launched before the timed region, started by the host's
    // doorbell ring).  Off by default: the reference's total_time brackets its request posts
    // (mpi_test.c:1444, :1763), so the like-for-like time includes the kernel launch
    KNOB("XG_ENGINE_ARM", on_if_1(&k->engine_arm, v)),
    // a cross-GPU step's local part: <= self_max bytes travels in the step's RCCL group as self
    // send/recv (one RCCL launch carries a latency-bound step), < split_min bytes joins the
    // step's pack / fused launch, larger runs on the side stream beside the exchange (split).
    // README configuration as a virtual 8-GPU job (profiles/r03/hybrid/): m6 direct 49 -> 2
    // launches per run, m12 46 -> 6; configs[1..4]'s bulk local parts (MiBs) stay split
    KNOB("XG_SPLIT_MIN", number(&k->split_min, v)),                  // bytes: a smaller local part is not split off
    KNOB("XG_SELF_MAX", number(&k->self_max, v)),                    // bytes: local part posted as self send/recv (0: never)
    KNOB("XG_FUSE_STAGE", off_if_0(&k->fuse_stage, v)),              // "0": stage copies always in a launch of their own
    KNOB("XG_SPLIT_AFTER_PACK", off_if_0(&k->split_after_pack, v)),  // "0": a split step's local part and its packs start together
};

// name's value in env ("NAME=value" strings, the first match); env NULL: the process environment
static const char *env_get(const char *const *env, const char *name)
{
    if (!env) return getenv(name);
    const size_t n = strlen(name);
    for (; *env; ++env)
        if (!strncmp(*env, name, n) && (*env)[n] == '=') return *env + n + 1;
    return nullptr;
}

// Knobs that are constants now (Knobs): a setting left in the environment -- an A/B
// recipe under profiles/ from the round that measured it -- changes nothing, so say so once
static void warn_folded_knobs(const char *const *env)
{
    static bool done = false;
    if (done) return;
    done = true;
    static const char *const folded[] = {
        // round 4: settled tuning
        "XG_COPY_BALANCE", "XG_COPY_CHUNK", "XG_COPY_NT_MIN", "XG_COPY_NT_STREAM", "XG_COPY_WAVE",
        "XG_COPY_WAVE_MAX", "XG_COPY_WG_COST", "XG_FUSE_UNPACK", "XG_GRID_CACHE_MAX",
        "XG_PIECE_ORDER", "XG_SOLO_MIN_STEPS", "XG_SOLO_RELAY", "XG_SPLIT_LOCAL",
        // round 5: environment twins of bin/test options (--fingerprint, --eager-limit, ...)
        "XG_FINGERPRINT", "XG_EAGER_LIMIT", "XG_PACK_MAX_SEG", "XG_PACK_MIN", "XG_PACK_FORM"};
    for (const char *k : folded)
        if (env_get(env, k)) fprintf(stderr, "xg: %s is set but no longer read (folded into a constant or an option)\n", k);
}

extern "C" void xg_plan_knobs_env(xg_plan_knobs *k, const char *const *env)
{
    warn_folded_knobs(env);
    for (const Knob &r : kKnobs) r.apply(k, env_get(env, r.name));
}

extern "C" int xg_plan_knob_names(const char **out, int cap)
{
    const int n = (int)(sizeof kKnobs / sizeof *kKnobs);
    for (int i = 0; out && i < n && i < cap; ++i) out[i] = kKnobs[i].name;
    return n;
}

extern "C" int xg_plan_tables_build(const xg_devplan *dp, const xg_plan_knobs *k, const uint64_t base[XG_NBUF],
                                    const int64_t bytes[XG_NBUF], xg_plan_tables **out)
{
    if (!dp || !k || !base || !bytes || !out) return XG_EARG;
    *out = nullptr;
    PlanTables *t = new PlanTables();
    if (const int rc = plan_tables_build(t, dp, k, base, bytes)) {
        delete t;
        return rc;
    }
    *out = t;
    return XG_OK;
}

extern "C" void xg_plan_tables_free(xg_plan_tables *t) { delete t; }

extern "C" int xg_plan_tables_nsteps(const xg_plan_tables *p) { return p->nsteps; }
extern "C" int xg_plan_tables_engine(const xg_plan_tables *p) { return p->segs.empty() ? 0 : p->segs[0].w; }
extern "C" int xg_plan_tables_engine_rails(const xg_plan_tables *p)
{
    for (const EngSeg &g : p->segs)
        if (g.solo) return g.w;
    return 0;
}
extern "C" int xg_plan_tables_launches(const xg_plan_tables *p) { return p->nlaunch; }

extern "C" int xg_plan_tables_step_form(const xg_plan_tables *p, int s)
{
    if (!p || s < 0 || s >= p->nsteps) return -1;
    const StepR &st = p->steps[s];
    return (st.split ? XG_FORM_SPLIT : 0) | (st.fused ? XG_FORM_FUSED : 0) | (st.fused_local ? XG_FORM_FUSED_LOCAL : 0) |
           (st.stage_fused ? XG_FORM_STAGE_FUSED : 0) | (st.deferred ? XG_FORM_DEFERRED : 0) |
           (st.self_local ? XG_FORM_SELF_LOCAL : 0) | (p->seg_of[s] >= 0 ? XG_FORM_ENGINE : 0);
}

extern "C" int xg_plan_tables_engine_steps(const xg_plan_tables *p, int *nseg, int *nhaz)
{
    int n = 0, h = 0;
    for (const EngSeg &g : p->segs) {
        n += g.s1 - g.s0;
        h += g.nhaz;
    }
    if (nseg) *nseg = (int)p->segs.size();
    if (nhaz) *nhaz = h;
    return n;
}

// The launch-table entries one run issues (a launch of several dispatches counts once) of one
// kind, XG_COPY_PIECE .. XG_COPY_SMALL.
extern "C" int xg_plan_tables_kind_launches(const xg_plan_tables *p, int kind)
{
    int count = 0;
    each_launch(p, [&](const CopyLaunch &l) { count += l.kind == kind; });
    return count;
}

// The WAVE launches and the geometry the runtime gives their copy_kernel_w dispatch: w workgroups
// of 4 waves over n pieces.
extern "C" int xg_plan_tables_wave_launches(const xg_plan_tables *p, int *grid, int *max_pieces_per_wave)
{
    int most = 0;
    each_launch(p, [&](const CopyLaunch &l) {
        if (l.kind != XG_COPY_WAVE) return;
        const int m = p->cuts[l.cut + 1] - l.b, w = wave_wgs(p, m);
        most = std::max(most, (m + 4 * w - 1) / (4 * w));
    });
    if (grid) *grid = p->wave_grid;
    if (max_pieces_per_wave) *max_pieces_per_wave = most;
    return xg_plan_tables_kind_launches(p, XG_COPY_WAVE);
}

extern "C" int xg_plan_tables_shift_launches(const xg_plan_tables *p) { return xg_plan_tables_kind_launches(p, XG_COPY_SHIFT); }
extern "C" int xg_plan_tables_extent_launches(const xg_plan_tables *p) { return xg_plan_tables_kind_launches(p, XG_COPY_EXTENT); }

// *kib: the SMALL launches' piece size, 0 when there is none; may be NULL
extern "C" int xg_plan_tables_small_launches(const xg_plan_tables *p, int *kib)
{
    if (kib) *kib = 0;
    each_launch(p, [&](const CopyLaunch &l) {
        if (kib && l.kind == XG_COPY_SMALL) *kib = l.kib;
    });
    return xg_plan_tables_kind_launches(p, XG_COPY_SMALL);
}

// ------------------------------------------------------------------ the text dump
namespace {
struct Dump {
    const PlanTables *p;
    std::string s;
    void f(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        char line[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(line, sizeof line, fmt, ap);
        va_end(ap);
        s += line;
    }
    // region+offset of an address: the first region that holds it (its end included, for an
    // empty range's pointer); "-" for null
    std::string at(const void *q) const
    {
        const uint64_t a = (uint64_t)(uintptr_t)q;
        char out[64];
        if (!a) return "-";
        for (int pass = 0; pass < 2; ++pass)
            for (int b = 0; b < XG_NBUF; ++b)
                if (p->bytes[b] > 0 && a >= p->base[b] &&
                    (pass ? a == p->base[b] + (uint64_t)p->bytes[b] : a < p->base[b] + (uint64_t)p->bytes[b])) {
                    snprintf(out, sizeof out, "%d+%llu", b, (unsigned long long)(a - p->base[b]));
                    return out;
                }
        snprintf(out, sizeof out, "?+%llx", (unsigned long long)a);
        return out;
    }
    void copies(const char *tag, const std::vector<xgk::DCopy> &v)
    {
        for (size_t i = 0; i < v.size(); ++i)
            f("%s %zu %s %s %lld\n", tag, i, at(v[i].src).c_str(), at(v[i].dst).c_str(), (long long)v[i].len);
    }
    template <class T> void ints(const char *tag, const std::vector<T> &v)
    {
        for (size_t i = 0; i < v.size(); ++i) f("%s %zu %lld\n", tag, i, (long long)v[i]);
    }
};
}  // namespace

extern "C" int64_t xg_plan_tables_dump(const xg_plan_tables *p, char *buf, int64_t cap)
{
    Dump d{p, {}};
    d.f("plan nsteps %d npieces %d variant %d streaming %d nlaunch %d graph_auto %d may_arm %d stamp_rails %d\n",
        p->nsteps, p->npieces, p->variant, (int)p->streaming, p->nlaunch, (int)p->graph_auto, (int)p->may_arm,
        p->stamp_rails);
    for (size_t i = 0; i < p->steps.size(); ++i) {
        const StepR &t = p->steps[i];
        d.f("step %zu stage %d %d local %d %d pack %d %d post %d %d calls %d %d p2p %d sync %d groups %d posts %d pre %d "
            "bytes %lld %lld %lld %lld form %d small %d l %d %d %d seg %d chain %d\n",
            i, t.stage_b, t.stage_n, t.local_b, t.local_n, t.pack_b, t.pack_n, t.post_b, t.post_n, t.call_b, t.call_n,
            t.p2p_n, t.sync_after, t.groups, t.posts, t.pre_n, (long long)t.stage_bytes, (long long)t.local_bytes,
            (long long)t.pack_bytes, (long long)t.post_bytes, xg_plan_tables_step_form(p, (int)i), (int)t.small, t.l_b,
            t.l_rccl, t.l_e, p->seg_of[i], p->chain_end[i]);
    }
    for (size_t i = 0; i < p->calls.size(); ++i) {
        const xg_call &o = p->calls[i];
        d.f("call %zu kind %d peer %d buf %d off %lld len %lld\n", i, o.kind, o.peer, o.buf, (long long)o.off,
            (long long)o.len);
    }
    d.ints("call_begin", p->call_begin);
    for (size_t i = 0; i < p->launches.size(); ++i) {
        const CopyLaunch &l = p->launches[i];
        d.f("launch %zu b %d n %d bytes %lld kind %d nt %d kib %d xt %d q %d %d %d %d %lld side %d mark_prev %d cut %d "
            "ndisp %d\n",
            i, l.b, l.n, (long long)l.bytes, l.kind, (int)l.nt, l.kib, l.xt, l.q_row, l.q_copies, l.q_k, l.q_bytes,
            (long long)l.q_len, (int)l.side, (int)l.mark_prev, l.cut, l.ndisp);
    }
    d.ints("cut", p->cuts);
    d.ints("xt_begin", p->xt_begin);
    d.ints("xt_off", p->xt_off);
    d.ints("xt_n", p->xt_n);
    d.copies("row", p->rows);
    d.ints("qbytes", p->qbytes);
    d.copies("piece", p->pieces);
    d.ints("disp_len", p->ds.len);
    d.ints("disp_host", p->ds.host);
    d.ints("disp_group", p->ds.groups);
    for (size_t i = 0; i < p->ds.fix.size(); ++i) {
        const xgk::DFix &x = p->ds.fix[i];
        d.f("fix %zu piece %d copy %d off %lld side %d\n", i, x.piece, x.copy, (long long)x.off, x.side);
    }
    for (size_t i = 0; i < p->segs.size(); ++i) {
        const EngSeg &g = p->segs[i];
        d.f("seg %zu steps %d %d w %d b %d sb_off %d nhaz %d solo %d wv %d gran %d u0 %d npieces %d sbase %s dbase %s "
            "bytes %lld\n",
            i, g.s0, g.s1, g.w, g.b, g.sb_off, g.nhaz, (int)g.solo, g.wv, g.gran, g.u0, g.npieces, d.at(g.sbase).c_str(),
            d.at(g.dbase).c_str(), (long long)g.bytes);
    }
    d.copies("unit", p->ep);
    d.ints("sb", p->sb);
    for (size_t i = 0; i < p->solo_desc.size(); ++i) d.f("solo_desc %zu 0x%llx\n", i, p->solo_desc[i]);
    const int64_t n = (int64_t)d.s.size();
    if (buf && cap > 0) {
        const int64_t m = std::min(n, cap - 1);
        memcpy(buf, d.s.data(), (size_t)m);
        buf[m] = 0;
    }
    return n;
}
