"""GPU: step times land on the steps that took them.

The product's output is times, and every Timer field is read from step_done[], which xg_plan_run
and xg_vplans_run* return.  A run that reported [0, 0, ..., wall] would be ordered and inside its
wall time; so would one that credited every step's time to its neighbour or counted the wall clock
at the wrong rate.  Here every plan has ONE heavy step among light ones (time_plan.py): with

    d[s] = step_done[s] - step_done[s - 1]      (d[0] = step_done[0])

every run asserts (1) the largest d is the heavy step's, (2) it is no shorter than the device needs
for the step's bytes (time_plan.lower_chip / lower_cus: HBM and L2 rates, the bytes an engine may
have loaded early taken off), (3) step_done[-1] <= 1.01 x the host's own clock around the call (the
device interval lies inside the host call; 1 % covers the two clocks' rate tolerance, which is in
the ppm range), and (4) the bytes, whole RECV against numpy.  The routing of every plan is asserted
from the loaded plan's own tables against the form test_time_plan.py proves with no GPU.

Through every source of step_done[]: marks (a launch per step), chain stamps, chains in a replayed
graph, the grid engine launched, armed and inside a graph, the solo engine on 16-wave and one-wave
rails (MAX over rails, carried stamps) and on ONE rail (the stamps themselves), two segments round
a launch (each anchored at its own mark), an unmarked step (the back-fill), and virtual two-GPU
jobs, where a segment's time is shared out by GPU 0's engine stamps.

Every run also asserts that no step time is 0 (xg_step_times clamps a time that would fall before
the start to 0: a stamp that was never taken, or is another step's, shows there).  Eager runs are
posted behind a cover copy (Cover) and every plan runs once before its asserted runs (_warm_up),
so that the host's own launch latency does not pose as step 0's time.

Every figure is printed before it is asserted (pytest -s shows d[p] / bound per run).
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import time_plan as T
from synth_plan import Synth, _ctx_env

pytestmark = pytest.mark.gpu

RUNS = 3
TILE = (16 << 20) - 4080            # the large case's SEND: this random block, tiled (copies 128 MiB apart differ)


class TiledSynth(Synth):
    """Synth for a plan of hundreds of MiB: SEND is a tiled random block, the regions are written
    and read in place, the expectation is the in-order numpy execution of the SEND -> RECV copies"""

    def __init__(self, xg, ctx, send_bytes, recv_bytes, steps, seed=0):
        d = xg.device()
        self.xg, self.d = xg, d
        rb = (C.c_int64 * xg.NBUF)(send_bytes, recv_bytes, 0, 0, 0)
        self.r = C.c_void_p()
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(self.r)) == 0
        block = np.random.default_rng(seed).integers(0, 256, TILE, dtype=np.uint8)
        self.send = np.tile(block, -(-send_bytes // TILE))[:send_bytes]
        self.recv = np.full(recv_bytes, 0xA5, np.uint8)
        assert d.xg_regions_write(self.r, xg.BUF_SEND, 0, self.send.ctypes.data_as(C.c_void_p), send_bytes) == 0
        self._load(ctx, send_bytes, recv_bytes, steps)

    def expected(self, recv=None):
        want = self.recv.copy()
        for st in self.steps:
            for (sb, so, db, do, ln) in st:
                assert (sb, db) == (0, 1)
                want[do:do + ln] = self.send[so:so + ln]
        return want


def _read_recv(sy):
    out = np.empty(len(sy.recv), np.uint8)
    assert sy.d.xg_regions_read(sy.r, 1, 0, out.ctypes.data_as(C.c_void_p), len(out)) == 0
    return out


def _timed(run, n):
    """run(step_done) between two readings of the host clock -> (step_done, host seconds)"""
    done = (C.c_double * n)()
    t0 = time.perf_counter()
    rc = run(done)
    t_host = time.perf_counter() - t0
    assert rc == 0
    return list(done), t_host


class Cover(Synth):
    """A plan of one 256 MiB copy in regions of its own, on the context of the plan under test.
    Enqueued (xg_plan_enqueue: no marks, no wait) right before an EAGER timed run, it keeps the
    device busy for ~100 us on the stream the run is posted to, so the run's start mark and its
    first launches are all queued when the device reaches them.  Otherwise the device idles behind
    the start mark for as long as the host needs to post the first launch, 10-25 us that land in
    d[0] and are as long as the heavy steps here -- a light first step then often beats the heavy
    one, by the host's doing.  A run inside an application is posted behind other work in just this
    way.  Armed runs and graph replays have no such gap; the 512 MiB case does not need a cover
    and runs without one, which keeps its host-clock check tight."""
    BYTES = 256 << 20

    def __init__(self, xg, ctx):
        d = xg.device()
        self.xg, self.d = xg, d
        rb = (C.c_int64 * xg.NBUF)(self.BYTES, self.BYTES, 0, 0, 0)
        self.r = C.c_void_p()
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(self.r)) == 0
        self.recv = np.zeros(0, np.uint8)
        self._load(ctx, self.BYTES, self.BYTES, [[(0, 0, 1, 0, self.BYTES)]])

    def enqueue(self):
        assert self.d.xg_plan_enqueue(self.p) == 0


def _eager(env):
    """a run under these knobs is posted launch by launch inside the timed region"""
    return env.get("XG_GRAPH", 0) != 1 and env.get("XG_ENGINE_ARM", 0) != 1


def _plan_run(sy, cover=None):
    post, wall = (C.c_double * len(sy.steps))(), C.c_double()
    if cover is not None:
        cover.enqueue()
    return _timed(lambda done: sy.d.xg_plan_run(sy.p, done, post, C.byref(wall)), len(sy.steps))


def _warm_up(sy, cover=None):
    """One run that asserts nothing about times.  An eager run's d[0] holds whatever the host needs
    between the start mark and the first launch (the device waits behind the mark): on a process's
    first launch of a kernel that includes loading its code, tens to hundreds of us that are no
    step's time.  Without this run the first asserted one would depend on which test ran before."""
    sy.poison()
    _plan_run(sy, cover)


def _diffs(done):
    return [done[0]] + [b - a for a, b in zip(done, done[1:])]


def _check_times(what, done, t_host, p, bound, over=None):
    """(1)-(3) of the module's docstring; over: the steps among which d[p] must be the largest (default all)"""
    d = _diffs(done)
    over = list(over if over is not None else range(len(d)))
    top = max(over, key=lambda s: d[s])
    print("%s: d[p=%d] = %.2f us, bound %.2f us, ratio %.2f; largest other %.2f us; done[-1] %.1f us, host %.1f us"
          % (what, p, d[p] * 1e6, bound * 1e6, d[p] / bound, max([d[s] for s in over if s != p] + [0]) * 1e6,
             done[-1] * 1e6, t_host * 1e6))
    assert all(x >= 0 for x in d), (what, done)
    # no step is done at the instant of the start mark: a 0 is a time clamped by xg_step_times, i.e.
    # a stamp that was never taken or is not the step's (consistent stamps clamp nothing, test_time_plan.py)
    assert all(x > 0 for x in done), (what, done)
    assert top == p, (what, "the largest step time is step %d's, the heavy step is %d" % (top, p), d)
    assert d[p] >= bound, (what, "the heavy step took %.3g s, the device needs %.3g s" % (d[p], bound), d)
    assert done[-1] <= 1.01 * t_host, (what, done[-1], t_host)


def _loaded_form(xg, plan):
    d = xg.device()
    d.xg_plan_tables_of.restype = C.c_void_p
    d.xg_plan_tables_of.argtypes = [C.c_void_p]
    return T.form(xg.parse_tables(xg.dump_tables(C.c_void_p(d.xg_plan_tables_of(plan)))))


def _loaded(xg, cx, steps, send_bytes, recv_bytes, seed):
    cls = TiledSynth if recv_bytes > 256 << 20 else Synth
    return cls(xg, cx, send_bytes, recv_bytes, steps, seed=seed)


def _runs(what, sy, p, bound, cover=None):
    """RUNS runs from a poisoned RECV each: the times, then the whole image"""
    want = sy.expected()
    _warm_up(sy, cover)
    for rep in range(RUNS):
        sy.poison()
        done, t_host = _plan_run(sy, cover)
        got = _read_recv(sy)
        _check_times("%s run %d" % (what, rep), done, t_host, p, bound)
        assert np.array_equal(got, want), (what, rep, int(np.flatnonzero(got != want)[0]))


# ------------------------------------------------------------------ every route, the heavy step first, in the middle, last
@pytest.mark.parametrize("route,pos", T.CASES)
def test_heavy_step_on_every_route(xg, route, pos):
    """time_plan.ROUTES: the route's knobs, its heavy step, the form its plan must take"""
    r = T.ROUTES[route]
    steps, send_bytes, recv_bytes, p = T.sized(route, pos)
    cx = _ctx_env(xg, **r["env"])
    cover = None
    try:
        sy = _loaded(xg, cx, steps, send_bytes, recv_bytes, seed=len(route) + p)
        try:
            if _eager(r["env"]) and route != "launches":
                cover = Cover(xg, cx)
            f = _loaded_form(xg, sy.p)
            assert f == T.expected_form(route, len(steps)), (f, T.expected_form(route, len(steps)))
            if f["segs"]:
                assert T.discount(f["segs"][0]) <= r["H"] // 4
            _runs("%s/%s" % (route, pos), sy, p, T.bound(route, f), cover)
        finally:
            if cover is not None:
                cover.close()
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ two segments round a launch
def test_two_segments_round_a_launch(xg):
    """4 light steps (an engine segment), a 64 MiB step above XG_ENGINE_MAX_STEP (a launch), 4 light
    steps (a second segment): each segment's stamps are anchored at its own mark, so neither
    segment's steps reach into the launch's time and each segment as a whole is shorter than it"""
    spec = T.TWO_SEG
    steps, send_bytes, recv_bytes = T.heavy_steps(spec["n"], spec["p"], spec["H"])
    low = T.lower_chip(spec["H"])
    cx = _ctx_env(xg, **spec["env"])
    try:
        sy = _loaded(xg, cx, steps, send_bytes, recv_bytes, seed=2)
        try:
            assert _loaded_form(xg, sy.p) == T.TWO_SEG_FORM
            cover = Cover(xg, cx)
            want = sy.expected()
            _warm_up(sy, cover)
            for rep in range(RUNS):
                sy.poison()
                done, t_host = _plan_run(sy, cover)
                got = _read_recv(sy)
                _check_times("two segments run %d" % rep, done, t_host, 4, low)
                d = _diffs(done)
                print("two segments run %d: segment A %.2f us, launch %.2f us, segment B %.2f us"
                      % (rep, sum(d[:4]) * 1e6, d[4] * 1e6, sum(d[5:]) * 1e6))
                assert done[3] <= done[4] - low, (rep, done)
                assert sum(d[:4]) < d[4] and sum(d[5:]) < d[4], (rep, d)
                assert np.array_equal(got, want), rep
            cover.close()
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ an unmarked heavy step
@pytest.mark.parametrize("mode", list(T.UNMARKED["envs"]))
def test_unmarked_heavy_step(xg, mode):
    """a launch per step, the heavy step's mark off: it is reported done when the next marked step
    is, and that step's time then holds the heavy step.  graph: the first run captures with every
    mark on, xg_plan_set_step_marks drops that graph, and the next run captures again."""
    spec = T.UNMARKED
    n, p, H = spec["n"], spec["p"], spec["H"]
    q = p + 1
    steps, send_bytes, recv_bytes = T.heavy_steps(n, p, H)
    cx = _ctx_env(xg, **spec["envs"][mode])
    try:
        sy = _loaded(xg, cx, steps, send_bytes, recv_bytes, seed=3)
        try:
            assert _loaded_form(xg, sy.p) == dict(nsteps=n, launches=n, segs=[], chains=[], armed=0)
            cover = Cover(xg, cx) if _eager(spec["envs"][mode]) else None
            want = sy.expected()
            _warm_up(sy, cover)
            sy.poison()
            done, t_host = _plan_run(sy, cover)          # every step marked
            _check_times("unmarked/%s, all marks" % mode, done, t_host, p, T.lower_chip(H))
            need = [1] * n
            need[p] = 0
            assert sy.d.xg_plan_set_step_marks(sy.p, (C.c_uint8 * n)(*need)) == 0
            for rep in range(RUNS):
                sy.poison()
                done, t_host = _plan_run(sy, cover)
                got = _read_recv(sy)
                print("unmarked/%s run %d: done[p-1 .. q] = %s us" % (mode, rep, [round(x * 1e6, 2) for x in done[p - 1:q + 1]]))
                assert done[p] == done[q], (rep, done)
                assert done[q] - done[p - 1] >= T.lower_chip(H), (rep, done)
                assert all(0 <= a <= b for a, b in zip(done, done[1:])) and done[-1] <= 1.01 * t_host, (rep, done, t_host)
                d = _diffs(done)
                assert max(range(n), key=lambda s: d[s]) == p, (rep, d)      # the back-filled time of p
                assert np.array_equal(got, want), rep
            if cover is not None:
                cover.close()
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ virtual two-GPU jobs
def _virtual(xg, G, **env):
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


def _virtual_runs(xg, job, spec, want_form, rccl, check):
    """the job on two virtual GPUs: each GPU's form, then RUNS runs from the same seeded image --
    check(run, step_done, host seconds), every region of both GPUs against Job.execute"""
    import dep_plan as D
    job.check()
    ctxs = _virtual(xg, job.G, **spec["env"])
    loaded = []
    try:
        for g, cx in enumerate(ctxs):
            loaded.append(D.Loaded(xg, cx, job, g))
        for ld in loaded:
            f = _loaded_form(xg, ld.p)
            f.pop("chains")
            assert f == want_form, (job.name, ld.g, f)
        init = job.initial(17)
        want = job.execute([[a.copy() for a in regs] for regs in init])
        arr = (C.c_void_p * job.G)(*[ld.p for ld in loaded])
        fn = xg.device().xg_vplans_run_rccl if rccl else xg.device().xg_vplans_run
        for rep in range(RUNS):
            for g, ld in enumerate(loaded):
                for b in D.USER_BUFS:
                    ld.write(b, init[g][b])
            done, t_host = _timed(lambda out: fn(arr, job.G, out), job.nsteps)
            got = [[ld.read(b) if b in D.USER_BUFS else None for b in range(5)] for ld in loaded]
            check(rep, done, t_host)
            job.compare(got, want, "run %d" % rep)
            for ld in loaded:
                assert xg.device().xg_plan_check(ld.p) == 0
    finally:
        for ld in loaded:
            ld.close()
        for cx in ctxs:
            cx.close()


@pytest.mark.parametrize("rccl", [False, True], ids=["copies", "rccl"])
def test_virtual_heavy_cross_gpu_step(xg, rccl):
    """(a) light local steps round a step in which each GPU packs 32 MiB, sends them to the other
    and unpacks what it receives: six copies of 32 MiB on the one device, none put off into the next
    step (test_time_plan.py).  The staging bytes are written and read again inside the step and
    the 256 MiB it touches fit the caches, so only the L2 term of lower_chip is sure: every one of
    the 192 MiB moved is loaded once, and no load is served faster than the L2s serve."""
    spec = T.V_CROSS
    low = 6 * spec["E"] / T.L2_RATE
    _virtual_runs(xg, T.job_cross(), spec, T.V_CROSS_FORM, rccl,
                  lambda rep, done, t_host: _check_times("virtual cross run %d" % rep, done, t_host, spec["p"], low))


@pytest.mark.parametrize("rccl", [False, True], ids=["copies", "rccl"])
def test_virtual_heavy_step_inside_a_segment(xg, rccl):
    """(b) steps 0..6 are one grid-engine segment on both GPUs, the heavy step (16 MiB) in its
    middle.  Each GPU's segment is ONE launch at step 0 and every mark of steps 0..6 is enqueued
    behind both launches, so the marks alone put every step of the segment at the segment's end;
    xg_vplans_run shares the segment's time out by GPU 0's engine stamps, anchored at the mark
    behind step 6.  d[0] then also holds GPU 1's launch, which runs behind GPU 0's; among the steps
    whose d is a difference of two engine stamps (1..6) the heavy step's is the largest and no
    shorter than 8 workgroups need for its bytes."""
    spec = T.V_SEG
    seg = T.V_SEG_FORM["segs"][0]
    s0, s1 = seg["steps"]
    low = T.lower_cus(spec["H"] - T.discount(seg), seg["w"])

    def check(rep, done, t_host):
        _check_times("virtual segment run %d" % rep, done, t_host, spec["p"], low, over=range(s0 + 1, s1))
        assert done[spec["p"] - 1] <= done[s1 - 1] - low, (rep, done)        # not everything at the segment's end

    _virtual_runs(xg, T.job_segment(), spec, T.V_SEG_FORM, rccl, check)
