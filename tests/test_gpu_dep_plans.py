"""GPU: plans whose steps DEPEND on each other, through every form a step can take.

Every schedule the product builds reads SEND and writes disjoint RECV slots, so no reordering of
its copies shows in the bytes -- and the runtime reorders a great deal, each time on a host
predicate: the grid engine loads the next step early (xg_engine_hazards), rails never wait
(xg_engine_rail_safe), a step's packs and local copies join the launch of the previous step's
unpacks (xg_step_packs_meet_unpacks, xg_step_local_meets_unpacks), stage copies join the local
launch (xg_step_stage_meets_rest), the local part runs on the side stream or inside the RCCL group.
The jobs of dep_plan.py carry read-after-write chains, delayed and partly overlapping reads,
rewrites and write-after-read between steps and phases; each case asserts (i) every region of every
GPU against the in-order numpy execution on 3 runs, each from a freshly written random image,
(ii) the routing -- the bytes would also be right on a slower form -- and (iii) xg_plan_check.
Their host side is checked in test_dep_plan.py.
"""
import os

import pytest

import dep_plan as D
from synth_plan import _ctx_env, _rails, _sized

pytestmark = pytest.mark.gpu

PER = 580               # copies per step: >= 2 x 256 workgroups, (PER - NDEP) a multiple of the length cycle
UNIT = 4096


def _virtual(xg, G, **env):
    """the G contexts of a virtual job, created under these knobs (read at init)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return [xg.Context.virtual(g, G, device=0) for g in range(G)]
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _units(steps, unit):
    """per step: {copy: the engine units it is cut to}, units numbered in destination order"""
    out = []
    for st in steps:
        at, m = 0, {}
        for c in sorted(st, key=lambda c: c[3]):
            k = -(-c[4] // unit)
            m[c] = range(at, at + k)
            at += k
        out.append((m, at))
    return out


def _assert_other_workgroups(steps, unit, W, ndep):
    """every dependent copy (the first ndep of a step) and each copy of an earlier step it meets run
    on different workgroups (unit i of a step is workgroup i % W's)"""
    units = _units(steps, unit)
    pairs = 0
    for j in range(1, len(steps)):
        for c in steps[j][:ndep]:
            for i in range(j):
                for w in steps[i]:
                    if (D._meet(c[0], c[1], c[4], w[2], w[3], w[4]) or D._meet(c[2], c[3], c[4], w[2], w[3], w[4]) or
                            D._meet(c[2], c[3], c[4], w[0], w[1], w[4])):
                        assert not ({u % W for u in units[j][0][c]} & {u % W for u in units[i][0][w]}), (j, c, i, w)
                        pairs += 1
    return pairs


def _solo_case(xg, steps, send_bytes, recv_bytes, name, env, routing, seed):
    job = D.solo_job(steps, send_bytes, recv_bytes, name)
    assert max(job.bytes[0]) < 8 << 20
    cx = _ctx_env(xg, **env)
    try:
        D.run_job(xg, [cx], job, seed=seed, routing=routing)
    finally:
        cx.close()


def _nhaz(xg, job):
    spans, size = job.spans()
    walk = D.hazard_walk(spans, size)
    assert xg.engine_hazards(spans)[0] == walk
    return walk.count(2)


# ------------------------------------------------------------------ one GPU, every kind per route
ROUTES = {
    "grid": dict(XG_ENGINE_SOLO=0),                                     # step_engine_kernel<1>, launched
    "armed": dict(XG_ENGINE_SOLO=0, XG_ENGINE_ARM=1),                   # ... waiting for the doorbell
    "graph": dict(XG_ENGINE_SOLO=0, XG_GRAPH=1, XG_ENGINE_MAX_STEP=1 << 20),   # ... in a replayed graph
    "chains": dict(XG_ENGINE_MAX_STEP=0),                               # a launch per step, chained stamps
    "launches": dict(XG_ENGINE_MAX_STEP=0, XG_STEP_CHAIN=0),            # a launch and an event per step
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", D.KINDS)
def test_one_gpu_kinds(xg, kind, route):
    """Every dependency kind as one plan per route.  On the grid engine every step has more than two
    units per workgroup, each dependent copy is a workgroup's FIRST unit of its step (the one loaded
    while the barrier is pending, or -- off the 16-B grid -- the unprefetched byte path) and runs on
    another workgroup than the copies it depends on; the hazard points are the byte walk's.  graph:
    a last step above XG_ENGINE_MAX_STEP keeps the plan at two launches, so XG_GRAPH=1 captures it:
    3 replays, the ticket counter restarting in each."""
    steps, sb, rb = D.solo_kind(kind, PER)
    if route == "graph":
        big = (1 << 20) + 4096
        steps = steps + [[(D.S, sb, D.R, rb, big)]]
        sb, rb = sb + big + 16, rb + big + 32
    job = D.solo_job(steps, sb, rb, kind)
    nhaz = _nhaz(xg, job)
    engine = route in ("grid", "armed", "graph")
    nseg = len(steps) - (route == "graph")

    def routing(loaded):
        ld, d = loaded[0], xg.device()
        W = d.xg_plan_engine(ld.p)
        if not engine:
            assert W == 0 and d.xg_plan_launches(ld.p) == len(steps)
            return
        assert W > 0 and d.xg_plan_engine_rails(ld.p) == 0
        assert ld.engine_steps() == (nseg, 1, nhaz), (ld.engine_steps(), nseg, nhaz)
        assert d.xg_plan_launches(ld.p) == (2 if route == "graph" else 1)
        seg = steps[:nseg]
        assert all(n >= 2 * W for (_m, n) in _units(seg, UNIT)), (W, [n for (_m, n) in _units(seg, UNIT)])
        assert _assert_other_workgroups(seg, UNIT, W, D.NDEP) >= D.NDEP
        for st in seg[1:]:                        # among a step's first units some are off the 16-B grid
            off = [((so | do | n) & 15) != 0 for (_sb, so, _db, do, n) in st[:W]]
            assert any(off) and not all(off)

    _solo_case(xg, steps, sb, rb, "%s/%s" % (kind, route), ROUTES[route], routing, seed=D.KINDS.index(kind))


def test_grid_engine_64k_units_raw_chain(xg):
    """step_engine_kernel<16>: the read-after-write chain with transfers of one 64 KiB unit less 16 B,
    one unit, one unit and 16 B, three units and 4080 B; a workgroup per unit of the largest step"""
    steps, sb, rb = D.unit64_chain()
    big = max(sum(c[4] for c in st) for st in steps)
    assert 4 << 20 < big and rb < 8 << 20 and sb < 8 << 20
    job = D.solo_job(steps, sb, rb, "unit64_chain")
    nhaz = _nhaz(xg, job)
    assert nhaz == 3

    def routing(loaded):
        ld, d = loaded[0], xg.device()
        units = max(n for (_m, n) in _units(steps, 64 << 10))
        assert d.xg_plan_engine(ld.p) == units and d.xg_plan_engine_rails(ld.p) == 0
        assert ld.engine_steps() == (4, 1, 3)
        assert _assert_other_workgroups(steps, 64 << 10, units, 12) >= 12

    _solo_case(xg, steps, sb, rb, "unit64_chain", dict(XG_ENGINE_SOLO=0), routing, seed=64)


@pytest.mark.parametrize("kind", ["raw_chain", "war", "waw_other"])
def test_rails_refused(xg, kind):
    """The plan is sized (steps that move nothing, until the cost model prefers rails) so that its
    hazard-free twin -- the same copies, the dependent sources moved to SEND, the rewrite made
    identical -- DOES run on rails: that is the control.  The dependent plan itself must not."""
    base, sb, rb = D.solo_kind(kind, 2 * D.NDEP)

    def pad(steps, n):
        return steps[:1] + [[] for _ in range(n)] + steps[1:]

    tw, tsb = D.twin(base, sb, rb)
    bits = 0
    for st in tw:
        for (_sb, so, _db, do, n) in st:
            bits |= so | do | n
    gran = 16 if bits % 16 == 0 else 4 if bits % 4 == 0 else 1
    tsteps, _s, _r = _sized(lambda n: (pad(tw, n), tsb, rb), 512, 1, gran)
    npad = len(tsteps) - len(tw)
    want_rails = _rails(tsteps, 512, 1)

    def on_rails(loaded):
        d = xg.device()
        assert d.xg_plan_engine_rails(loaded[0].p) == want_rails > 0, (d.xg_plan_engine_rails(loaded[0].p), want_rails)
        assert loaded[0].engine_steps() == (len(tsteps), 1, 0)

    def off_rails(loaded):
        d = xg.device()
        assert d.xg_plan_engine_rails(loaded[0].p) == 0, "a dependent segment on unsynchronised rails"
        assert d.xg_plan_engine(loaded[0].p) > 0
        n, nseg, _nhaz_ = loaded[0].engine_steps()
        assert (n, nseg) == (len(tsteps), 1)

    _solo_case(xg, tsteps, tsb, rb, kind + "/twin", {}, on_rails, seed=7)
    _solo_case(xg, pad(base, npad), sb, rb, kind + "/rails", {}, off_rails, seed=8)


def test_mixed_plan(xg):
    """12 hazard-free steps, then the 4 of the read-after-write chain: whatever segments the loader
    cuts and whichever engine takes them, the image is right"""
    steps, sb, rb = D.solo_kind("raw_chain", 2 * D.NDEP, lead=12)
    assert len(steps) == 16 and rb < 8 << 20
    job = D.solo_job(steps, sb, rb, "mixed")
    nhaz = _nhaz(xg, job)
    assert nhaz == 3

    def routing(loaded):
        n, nseg, nh = loaded[0].engine_steps()
        assert n == 16 and nseg >= 1 and nh == nhaz, (n, nseg, nh)
        if nseg == 1:
            assert xg.device().xg_plan_engine_rails(loaded[0].p) == 0

    _solo_case(xg, steps, sb, rb, "mixed", {}, routing, seed=12)


# ------------------------------------------------------------------ two (three) virtual GPUs
def _pair_case(xg, name, env, routing, rccl=False, seed=0):
    job, _want = D.PAIR_JOBS[name]()
    assert all(max(job.bytes[g]) < 8 << 20 for g in range(job.G))
    ctxs = _virtual(xg, job.G, **env)
    try:
        D.run_job(xg, ctxs, job, seed=seed, rccl=rccl, routing=routing)
    finally:
        for cx in ctxs:
            cx.close()


def _forms(ld):
    return [ld.form(s) for s in range(ld.job.nsteps)]


def _launches(xg, loaded):
    return [xg.device().xg_plan_launches(ld.p) for ld in loaded]


NO_LOCAL_FORMS = dict(XG_SELF_MAX=0, XG_SPLIT_MIN=1 << 40)       # the local part stays in the step's first launch
VARIANTS = {"copies": ({}, False), "rccl": ({}, True), "graph": (dict(XG_GRAPH=1), False)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_pack_reads_the_previous_unpacks(xg, variant):
    """(a) step 0 delivers 3 MiB into the peer's RECV; step 1 packs the LAST bytes those unpacks
    wrote and sends them back.  One launch for step 0's unpacks and step 1's packs would read them
    in any order: step 1 must not be fused (xg_step_packs_meet_unpacks)."""
    env, rccl = VARIANTS[variant]

    def routing(loaded):
        for ld in loaded:
            f = _forms(ld)
            assert not f[1] & xg.FORM_FUSED and not f[0] & xg.FORM_DEFERRED, f
        assert _launches(xg, loaded) == [4, 4]             # packs, unpacks, packs, unpacks

    _pair_case(xg, "a_pack_reads_unpacks", dict(NO_LOCAL_FORMS, **env), routing, rccl, seed=1)


def test_barrier_between_the_two_steps(xg):
    """(h) the same with an in-loop barrier after step 0 (through RCCL: an all-reduce)"""
    def routing(loaded):
        for ld in loaded:
            assert not _forms(ld)[1] & xg.FORM_FUSED
    _pair_case(xg, "h_barrier", NO_LOCAL_FORMS, routing, rccl=False, seed=2)
    _pair_case(xg, "h_barrier", NO_LOCAL_FORMS, routing, rccl=True, seed=3)


def test_local_reads_the_previous_unpacks(xg):
    """(b) step 1's local copies read the last bytes step 0 unpacked, with every knob set so that
    they would join the fused launch: refused, bytes right.  Control, the local copies reading SEND:
    fused_local taken, one launch fewer."""
    seen = {}

    def dep(loaded):
        for ld in loaded:
            f = _forms(ld)[1]
            assert not f & (xg.FORM_FUSED_LOCAL | xg.FORM_FUSED | xg.FORM_SPLIT | xg.FORM_SELF_LOCAL), f
        seen["dep"] = _launches(xg, loaded)

    def control(loaded):
        for ld in loaded:
            f = _forms(ld)[1]
            assert f & xg.FORM_FUSED_LOCAL and f & xg.FORM_FUSED and _forms(ld)[0] & xg.FORM_DEFERRED, f
        seen["control"] = _launches(xg, loaded)

    _pair_case(xg, "b_local_reads_unpacks", NO_LOCAL_FORMS, dep, seed=4)
    _pair_case(xg, "b_control", NO_LOCAL_FORMS, control, seed=5)
    assert seen["dep"] == [4, 4] and seen["control"] == [3, 3], seen


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("after_pack", [1, 0])
def test_local_reads_the_previous_unpacks_on_the_side_stream(xg, after_pack, variant):
    """(c) the same local copies split off to the side stream (XG_SPLIT_MIN=0): the step is fused and
    split, and the fork stands behind the fused launch whichever XG_SPLIT_AFTER_PACK is asked for"""
    env, rccl = VARIANTS[variant]

    def routing(loaded):
        for ld in loaded:
            f = _forms(ld)[1]
            assert f & xg.FORM_SPLIT and f & xg.FORM_FUSED and not f & xg.FORM_FUSED_LOCAL, f

    _pair_case(xg, "b_local_reads_unpacks", dict(env, XG_SELF_MAX=0, XG_SPLIT_MIN=0, XG_SPLIT_AFTER_PACK=after_pack),
               routing, rccl, seed=6 + after_pack)


def test_local_overwrites_the_previous_unpacks(xg):
    """(d) step 1's local copies write over bytes step 0 unpacked: the local copies' bytes win"""
    def routing(loaded):
        for ld in loaded:
            assert not _forms(ld)[1] & (xg.FORM_FUSED_LOCAL | xg.FORM_FUSED)
    _pair_case(xg, "d_local_overwrites_unpacks", NO_LOCAL_FORMS, routing, seed=8)


def test_write_after_read_through_the_exchange(xg):
    """(e) step 0's packs read RECV[x], its unpacks overwrite RECV[x]; step 1's packs read the new
    bytes: not fused"""
    def routing(loaded):
        for ld in loaded:
            assert not _forms(ld)[1] & xg.FORM_FUSED
    _pair_case(xg, "e_war_exchange", NO_LOCAL_FORMS, routing, seed=9)


def test_stage_copies(xg):
    """(f) a stage copy SEND -> SCRATCH and a local copy SCRATCH -> RECV of the same step: the stage
    copies keep a launch of their own.  Control, the local copy reading SEND: one launch for both."""
    seen = {}

    def dep(loaded):
        for ld in loaded:
            assert not _forms(ld)[0] & xg.FORM_STAGE_FUSED
        seen["dep"] = _launches(xg, loaded)

    def control(loaded):
        for ld in loaded:
            assert _forms(ld)[0] & xg.FORM_STAGE_FUSED
        seen["control"] = _launches(xg, loaded)

    env = dict(NO_LOCAL_FORMS, XG_FUSE_STAGE=1)
    _pair_case(xg, "f_stage_dep", env, dep, seed=10)
    _pair_case(xg, "f_stage_control", env, control, seed=11)
    assert [a - b for a, b in zip(seen["dep"], seen["control"])] == [1, 1], seen


@pytest.mark.parametrize("rccl", [False, True])
def test_local_reads_the_previous_unpacks_in_the_group(xg, rccl):
    """(g) the local copies of (b) as self send / receive pairs inside step 1's RCCL group, which
    follows the fused launch"""
    def routing(loaded):
        for ld in loaded:
            f = _forms(ld)[1]
            assert f & xg.FORM_SELF_LOCAL and f & xg.FORM_FUSED and not f & xg.FORM_FUSED_LOCAL, f
    _pair_case(xg, "b_local_reads_unpacks", dict(XG_SELF_MAX=1 << 30), routing, rccl, seed=12)


def test_ring_forwarding(xg):
    """(i) three GPUs, each forwarding in step t + 1 what it received in step t: no step fused"""
    def routing(loaded):
        for ld in loaded:
            assert not any(f & xg.FORM_FUSED for f in _forms(ld)), _forms(ld)
    _pair_case(xg, "i_ring", NO_LOCAL_FORMS, routing, seed=13)


def test_engine_segment_inside_a_two_gpu_plan(xg):
    """(k) a cross-GPU step, then three GPU-local steps that read what it unpacked, each the step
    before: one engine launch, a hazard point at both of its inner boundaries"""
    def routing(loaded):
        for ld in loaded:
            assert ld.engine_steps() == (3, 1, 2), ld.engine_steps()
            f = _forms(ld)
            assert not f[0] & xg.FORM_ENGINE and all(x & xg.FORM_ENGINE for x in f[1:]), f
        assert _launches(xg, loaded) == [3, 3]             # packs, unpacks, the engine
    _pair_case(xg, "k_engine_inside", NO_LOCAL_FORMS, routing, seed=14)
