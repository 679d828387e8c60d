"""Plans with ONE heavy step, and lower bounds on the time that step can take (TEST HELPER for
test_time_plan.py and test_gpu_step_times.py; plain Python, no GPU).

A test of step times cannot compare with numpy.  It compares with three things that are not the
code under test: the bytes the plan says each step moves, the rates no memory level of the device
can exceed, and the test's own host clock.  Every plan is a run of light SEND -> RECV steps (LIGHT
bytes in LIGHT_COPIES copies) with one heavy step of H >= 256 x LIGHT bytes at position p, so

    d[s] = step_done[s] - step_done[s - 1]     (d[0] = step_done[0])

must peak at p, and d[p] cannot be shorter than the device needs for H bytes.

The bounds.  lower_chip(H): a step that loads H bytes and stores H bytes on the whole device; its
2 H bytes of traffic less what the caches can keep from HBM move at HBM_PEAK at best, and no
global load is served faster than L2_RATE.  lower_cus(H, n): a step confined to n workgroups or
rails, each on one CU at best.  CU_RATE is the aggregate L2 rate shared out over 256 CUs, ~144 GB/s;
DESIGN.md puts one CU's load + store traffic at ~120 GB/s, i.e. ~60 GB/s of reads, so the engine
bounds sit ~2.4 x under what the engines do.  That is the margin they have; it is not tuned.

The discount.  Every engine stamp before a segment's last is an ISSUE time: only the step's reads
are sure to be over, which is why the engine bounds count H once.  And an engine may have loaded
part of the heavy step BEFORE the previous step's stamp: the grid engine loads one unit per
workgroup while the barrier is pending, the solo engine two chunks of K rows per rail ahead of its
stores.  discount() takes those bytes -- from the plan's own segment record -- off H before the
bound is applied, and every engine plan keeps discount <= H / 4 by capping the workgroups
(XG_ENGINE_WG) and the rails (XG_SOLO_RAILS), so the bound stays meaningful.
"""
from synth_plan import K, PIECE, _layout, _solo_pays

# ------------------------------------------------------------------ the constants, each with its source
HBM_PEAK = 8.0e12                   # B/s: the HBM3E specification (the micro-architecture guide)
L2_RATE = 36.9e12                   # B/s: the highest aggregate L2 figure of the guide -- the fastest level a
                                    # global load can be served from
CU_RATE = L2_RATE / 256             # B/s per CU (~144 GB/s)
CACHE = (256 << 20) + 8 * (4 << 20)    # Infinity Cache + 8 XCD L2s: the bytes that can avoid HBM inside one step
WALL_HZ = 1e8                       # the 100 MHz wall clock the stamps count
MIN_TICKS = 20                      # every engine bound is longer than this many ticks

LIGHT = 16 << 10                    # bytes of a light step ...
LIGHT_COPIES = 4                    # ... in this many copies
HEAVY_COPIES = 4
UNIT = 4096                         # grid engine: a unit is b x 4 KiB (kernels.h step_engine_kernel<B>)


def lower_chip(H):
    return max(H / L2_RATE, (2 * H - CACHE) / HBM_PEAK)


def lower_cus(H, n):
    return H / (min(n, 256) * CU_RATE)


def discount(seg):
    """bytes of the heavy step an engine may have loaded before the previous step's stamp, from the
    segment's record (form()["segs"]): grid -- one unit per workgroup; solo -- two chunks of K rows
    of `wv` pieces per rail"""
    if seg["solo"]:
        return seg["w"] * 2 * K * seg["wv"] * PIECE
    return seg["w"] * seg["b"] * UNIT


POSITIONS = ("first", "middle", "last")


def position(pos, n):
    return {"first": 0, "middle": n // 2, "last": n - 1}[pos]


def heavy_steps(n, p, H, light=LIGHT, tail=0):
    """n steps, step p of H bytes in HEAVY_COPIES copies, the others of `light` bytes in
    LIGHT_COPIES copies; tail > 0: one more step of `tail` bytes in one copy behind them.  Every
    offset and length a multiple of 16, destinations disjoint between poisoned gaps, sources
    disjoint: no step depends on another -> (steps, send_bytes, recv_bytes)"""
    assert H >= 256 * light and H % (16 * HEAVY_COPIES) == 0 and light % (16 * LIGHT_COPIES) == 0 and 0 <= p < n
    specs, cuts = [], [0]
    for s in range(n):
        k, each = (HEAVY_COPIES, H // HEAVY_COPIES) if s == p else (LIGHT_COPIES, light // LIGHT_COPIES)
        specs += [(each, 0, 0)] * k
        cuts.append(len(specs))
    if tail:
        assert tail % 16 == 0
        specs.append((tail, 0, 0))
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    return [copies[a:b] for a, b in zip(cuts, cuts[1:])], send_bytes, recv_bytes


# ------------------------------------------------------------------ the routes
# env: the context's knobs.  H: the heavy step.  kind: what a step of the plan is -- "launch" (a
# launch and a mark per step), "chain" (stamped launches), "grid" / "solo" (one engine segment).
# n: the plan's steps ("solo": the fewest at which the cost model takes rails, sized()).  w: the
# workgroups / rails the segment must have.  tail: a last step above XG_ENGINE_MAX_STEP, which keeps
# the plan at two launches so that XG_GRAPH=1 captures it (as ROUTES["graph"] of
# test_gpu_dep_plans.py; the positions are then those of the segment).
GRID_WG = 8                         # discount 8 x 64 KiB = H / 32
_GRID = dict(XG_ENGINE_SOLO=0, XG_ENGINE_WG=GRID_WG)
TAIL = (16 << 20) + 4096
ROUTES = {
    # the one case with a footprint past the caches: lower_chip ~ 96 us, the check on wall_hz
    "launches": dict(env=dict(XG_ENGINE_MAX_STEP=0, XG_STEP_CHAIN=0), H=512 << 20, kind="launch", n=7),
    "chains": dict(env=dict(XG_ENGINE_MAX_STEP=0), H=64 << 20, kind="chain", n=7),
    "chains_graph": dict(env=dict(XG_ENGINE_MAX_STEP=0, XG_GRAPH=1), H=64 << 20, kind="chain", n=7),
    "grid": dict(env=dict(_GRID, XG_ENGINE_ARM=0), H=16 << 20, kind="grid", n=7, w=GRID_WG),
    "grid_armed": dict(env=dict(_GRID, XG_ENGINE_ARM=1), H=16 << 20, kind="grid", n=7, w=GRID_WG),
    "grid_graph": dict(env=dict(_GRID, XG_GRAPH=1), H=16 << 20, kind="grid", n=7, w=GRID_WG, tail=TAIL),
    "solo16": dict(env=dict(XG_SOLO_WAVES=16, XG_SOLO_RAILS=16, XG_ENGINE_ARM=0), H=16 << 20, kind="solo", w=16),
    "solo16_armed": dict(env=dict(XG_SOLO_WAVES=16, XG_SOLO_RAILS=16, XG_ENGINE_ARM=1), H=16 << 20, kind="solo", w=16),
    # 16 pieces per light step on 64 rails: most rails have nothing in the step behind the heavy
    # one and carry their stamp of the heavy step (xg_solo_reduce_stamps)
    "solo1x64": dict(env=dict(XG_SOLO_RAILS=64, XG_ENGINE_ARM=0), H=8 << 20, kind="solo", w=64),
    "solo1x64_armed": dict(env=dict(XG_SOLO_RAILS=64, XG_ENGINE_ARM=1), H=8 << 20, kind="solo", w=64),
    # one rail: MAX over rails is the identity, so this checks the stamps themselves.  H = 2 MiB
    # keeps the run short; the light steps are 8 KiB, so that H is still 256 of them
    "solo16x1": dict(env=dict(XG_SOLO_WAVES=16, XG_SOLO_RAILS=1, XG_ENGINE_ARM=0), H=2 << 20, kind="solo", w=1,
                     light=8 << 10),
}
CASES = [(r, pos) for r in ROUTES for pos in POSITIONS]


def sized(route, pos):
    """the route's plan with the heavy step at `pos` -> (steps, send_bytes, recv_bytes, p)"""
    r = ROUTES[route]
    light = r.get("light", LIGHT)
    if r["kind"] != "solo":
        p = position(pos, r["n"])
        return heavy_steps(r["n"], p, r["H"], light, r.get("tail", 0)) + (p,)
    waves = r["env"].get("XG_SOLO_WAVES", 1)
    for n in range(8, 400, 2):          # _solo_pays keeps 10 % in hand on the rail side
        if _solo_pays(r["H"] + (n - 1) * light, n, r["w"], waves, n, 16):
            p = position(pos, n)
            return heavy_steps(n, p, r["H"], light) + (p,)
    raise AssertionError("no rail routing at this size")


# ------------------------------------------------------------------ the form of a plan
def form(records):
    """what a plan's tables (xg.parse_tables) say of its routing: the launches of a run, the
    engine segments with their step ranges, workgroups or rails, unit (b x 4 KiB) or waves per
    rail, the chains' ends, and whether a run is armed"""
    plan = records["plan"]
    segs = [dict(steps=tuple(g["steps"]), w=g["w"], solo=g["solo"], **({"wv": g["wv"]} if g["solo"] else {"b": g["b"]}))
            for g in records.get("seg", [])]
    return dict(nsteps=plan["nsteps"], launches=plan["nlaunch"], segs=segs,
                chains=[(s, st["chain"]) for s, st in enumerate(records.get("step", [])) if st["chain"]],
                armed=plan["may_arm"])


def expected_form(route, nsteps):
    """the form the route's plan must take, stated by hand: what the GPU test asserts of the loaded
    plan and test_time_plan.py of xg.PlanTables under env"""
    r = ROUTES[route]
    n = nsteps - (1 if r.get("tail") else 0)          # the segment's steps
    kind, env = r["kind"], r["env"]
    f = dict(nsteps=nsteps, launches=nsteps, segs=[], chains=[], armed=0)
    if kind == "chain":
        f["chains"] = [(0, nsteps)]
    elif kind in ("grid", "solo"):
        seg = dict(steps=(0, n), w=r["w"], solo=int(kind == "solo"))
        if kind == "solo":
            seg["wv"] = env.get("XG_SOLO_WAVES", 1)
        else:
            seg["b"] = 16               # a step above 4 MiB: 64 KiB units
        f["segs"] = [seg]
        f["launches"] = 1 + (1 if r.get("tail") else 0)
        f["armed"] = int(env.get("XG_ENGINE_ARM", 0) == 1)
    return f


def bound(route, f):
    """the least d[p] of the route's heavy step, seconds, from the form f of its plan"""
    r = ROUTES[route]
    if not f["segs"]:
        return lower_chip(r["H"])
    seg = f["segs"][0]
    return lower_cus(r["H"] - discount(seg), seg["w"])


# ------------------------------------------------------------------ a reference for xg_step_times
M64 = (1 << 64) - 1


def step_times_ref(marks, seg_of, seg_end, wall_hz, chain_stamps=None, engine_stamps=None, chain_end=None,
                   need_mark=None, host_total=-1.0):
    """xg_step_times in a dozen lines -> (step_done, the steps whose time was clamped to 0)"""
    n = len(seg_of)
    done, clamped = [None] * n, []
    s = 0
    while s < n:
        chain = chain_stamps is not None and chain_end is not None and chain_end[s]
        e = n if host_total >= 0 else chain_end[s] if chain else seg_end[seg_of[s]] if seg_of[s] >= 0 else s + 1
        st = chain_stamps if chain else engine_stamps if (host_total >= 0 or seg_of[s] >= 0) else None
        if st is None and need_mark is not None and not need_mark[s]:
            s = e
            continue
        end = host_total if host_total >= 0 else float((marks[e] - marks[0]) & M64) / wall_hz
        for t in range(s, e):
            x = end - (float((st[e - 1] - st[t]) & M64) / wall_hz if st is not None else 0.0)
            done[t] = end if t == e - 1 else max(x, 0.0)
            if t != e - 1 and x < 0:
                clamped.append(t)
        s = e
    for t in range(n - 2, -1, -1):
        if done[t] is None:
            done[t] = done[t + 1]
    return done, clamped


# ------------------------------------------------------------------ the tables of a plan, with no GPU
def devplan(xg, steps, send_bytes, recv_bytes):
    """synth_plan.Synth._load's xg_devplan: one GPU, steps of (src_buf, src_off, dst_buf, dst_off, len)"""
    import ctypes as C
    copies = [c for st in steps for c in st]
    arr = (xg.Copy * max(1, len(copies)))(*[xg.Copy(so, do, ln, sb, db) for (sb, so, db, do, ln) in copies])
    sp, b = [], 0
    for st in steps:
        sp.append(xg.StepPlan(b, len(st), 0, 0, 0, 0, 0, 0))
        b += len(st)
    spa = (xg.StepPlan * max(1, len(sp)))(*sp)
    p2p = (xg.P2P * 1)()
    dp = xg.DevPlan()
    dp.gpu, dp.ngpus, dp.nsteps = 0, 1, len(steps)
    for i, v in enumerate((send_bytes, recv_bytes, 0, 0, 0)):
        dp.region_bytes[i] = v
    dp.ncopy, dp.np2p = len(copies), 0
    dp.copies = C.cast(arr, C.POINTER(xg.Copy))
    dp.p2p = C.cast(p2p, C.POINTER(xg.P2P))
    dp.steps = C.cast(spa, C.POINTER(xg.StepPlan))
    dp._keep = (arr, spa, p2p)
    return dp


def tables_form(xg, dp, env, **more):
    """form() of the tables xg.PlanTables builds for dp under env on a 256-CU device"""
    pt = xg.PlanTables(dp, env=env, **more)
    try:
        return form(pt.records())
    finally:
        pt.close()


# ------------------------------------------------------------------ further plans
# Two engine segments round a launch: 4 light steps, one step above XG_ENGINE_MAX_STEP (16 MiB), 4
# light steps.  Each segment is one grid launch of 4 workgroups (a light step is 4 units of 4 KiB),
# anchored at its own mark.
TWO_SEG = dict(env=dict(XG_ENGINE_SOLO=0), H=64 << 20, n=9, p=4)
TWO_SEG_FORM = dict(nsteps=9, launches=3, chains=[], armed=0,
                    segs=[dict(steps=(0, 4), w=4, solo=0, b=1), dict(steps=(5, 9), w=4, solo=0, b=1)])

# The heavy step's mark off, on the launches route (eager, and captured again under XG_GRAPH=1)
UNMARKED = dict(H=64 << 20, n=7, p=3,
                envs={"eager": dict(XG_ENGINE_MAX_STEP=0, XG_STEP_CHAIN=0),
                      "graph": dict(XG_ENGINE_MAX_STEP=0, XG_STEP_CHAIN=0, XG_GRAPH=1)})

# Virtual two-GPU jobs (dep_plan.Job).  The local part stays in the step's first launch.
V_LOCAL = dict(XG_SELF_MAX=0, XG_SPLIT_MIN=1 << 40)
V_CROSS = dict(env=dict(V_LOCAL, XG_ENGINE_MAX_STEP=0), E=32 << 20, n=7, p=3)
V_SEG = dict(env=dict(V_LOCAL, XG_ENGINE_SOLO=0, XG_ENGINE_WG=GRID_WG), H=16 << 20, n=8, p=3)
# each GPU's form: (a) three launches, packs and unpacks, three launches; (b) the engine, packs and unpacks
V_CROSS_FORM = dict(nsteps=7, launches=8, segs=[], armed=0)
V_SEG_FORM = dict(nsteps=8, launches=3, segs=[dict(steps=(0, 7), w=GRID_WG, solo=0, b=16)], armed=0)


def _v_light(k, base_s, base_r):
    """light step k's local copies: LIGHT bytes SEND -> RECV in LIGHT_COPIES copies"""
    each = LIGHT // LIGHT_COPIES
    return [(0, base_s + (k * LIGHT_COPIES + i) * each, 1, base_r + (k * LIGHT_COPIES + i) * (each + 32), each)
            for i in range(LIGHT_COPIES)]


def job_cross():
    """(a) three light local steps, a step in which each GPU packs E bytes, sends them to the other
    and unpacks what it receives, three light local steps"""
    from dep_plan import Job, Part, _cut
    E, n, p = V_CROSS["E"], V_CROSS["n"], V_CROSS["p"]
    steps = []
    for s in range(n):
        if s == p:
            steps.append([Part(packs=[(1 - g, 0, o, m) for (o, m) in _cut(0, E, 4 << 20)],
                               unpacks=[(1 - g, 1, 64 + o, m) for (o, m) in _cut(0, E, 4 << 20)]) for g in range(2)])
        else:
            steps.append([Part(local=_v_light(s, E, 64 + E + 64)) for _g in range(2)])
    nb = (E + n * LIGHT, 64 + E + 64 + n * (LIGHT + 32 * LIGHT_COPIES) + 64, 0)
    return Job(2, [nb, nb], steps, "heavy_cross_step")


def job_segment():
    """(b) seven local steps on both GPUs -- one engine segment each -- with the heavy one (H bytes
    in HEAVY_COPIES copies) in the middle, then a small cross-GPU step"""
    from dep_plan import Job, Part, _cut
    H, n, p = V_SEG["H"], V_SEG["n"], V_SEG["p"]
    X = 512 << 10
    each = H // HEAVY_COPIES
    steps = []
    for s in range(n - 1):
        if s == p:
            local = [(0, X + i * each, 1, 64 + X + 64 + i * (each + 64), each) for i in range(HEAVY_COPIES)]
        else:
            local = _v_light(s, X + H, 64 + X + 64 + HEAVY_COPIES * (each + 64))
        steps.append([Part(local=local) for _g in range(2)])
    steps.append([Part(packs=[(1 - g, 0, o, m) for (o, m) in _cut(0, X, 128 << 10)],
                       unpacks=[(1 - g, 1, 64 + o, m) for (o, m) in _cut(0, X, 128 << 10)]) for g in range(2)])
    nb = (X + H + n * LIGHT, 64 + X + 64 + HEAVY_COPIES * (each + 64) + n * (LIGHT + 32 * LIGHT_COPIES) + 64, 0)
    return Job(2, [nb, nb], steps, "heavy_step_in_a_segment")
