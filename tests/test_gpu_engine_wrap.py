"""GPU: the step engines' cumulative counters across 2^31 and 2^32.

EngineState's counters (kernels.h) are never reset between launches: the grid engine's barriers
wait on `count`, an armed solo launch reads `arrive`, `fin[line]` and `rails`.  A long-lived plan
takes them past 2^32 -- `count` after some 65,000 launches of a 256-workgroup plan -- and no other
test starts them anywhere but zero.  xg_plan_engine_preset (a test hook) makes a plan's state what
earlier launches would have left; every case here computes its preset from the LOADED plan (W or R,
the step count, the hazard flags), so the wrap falls where the case says, and is bit-exact against
the in-order numpy execution of the harness it borrows: dep_plan.py (a barrier that opens early
gives wrong bytes: the dependent copy is another workgroup's first unit), pingpong.py (a lost or
repeated run gives another image).  What the kernels decide on these words is xg_sched.h's
xg_eng_* functions; tests/test_engine_counters.py walks those on the CPU.

(a) grid engine, dependent steps, 2^32 and 2^31 at the end of run 1, inside its first barrier,
    inside the hazard barrier and the last barrier of run 2; launched and armed; B = 1, 4, 16
(b) 19 rounds posted with no wait, the wrap inside round 9's launch
(c) preset, then replay -> eager -> replay: the replay's zeroing wins
(d) armed solo launches on 48, 3, 7, 37 and 64 rails, from two launches before each counter whose
    divisor does not divide 2^32 wraps; the doorbell epoch through 0
(e) the hook's refusals, and (0, 0) on a fresh plan
"""
import ctypes as C
import time
import types

import pytest

import dep_plan as D
import pingpong as PP
from synth_plan import (Synth, _assert_gaps, _compare, _ctx_env, _granule_steps, _rails, _round_steps, _segment,
                        _sized)
from test_gpu_back_to_back import _assert_times, _begin, _check, _loaded_records, _post, ld  # noqa: F401 (ld: a fixture)
from test_gpu_dep_plans import PER, ROUTES, UNIT, _assert_other_workgroups, _nhaz, _solo_case, _units

pytestmark = pytest.mark.gpu

M = 1 << 32
LINES = 16
EARG = 3


def _preset(xg, plan, tickets, armed=0):
    assert xg.device().xg_plan_engine_preset(plan, tickets % M, armed % M) == 0, (tickets, armed)


# ------------------------------------------------------------------ (a) grid engine, dependent steps
def _tickets(place, point, W, n, armed, haz):
    """the tickets taken before run 1 so that `point` falls at `place`; a run takes T = W * (n + armed)
    (armed: the pre-barrier comes first); inside a barrier = behind W // 2 of its W tickets"""
    T, j = W * (n + armed), max(1, W // 2)
    return {"end1": point - T,                                          # run 1's last arrival takes the counter to point
            "first1": point - j,                                        # armed: the pre-barrier
            "behind_pre1": point - W - j,                               # armed: the barrier behind it
            "haz2": point - T - (armed * W + haz * W + j),              # run 2: the barrier in front of the dependent step
            "last2": point - T - (armed * W + (n - 1) * W + j)}[place] % M


KIND_STEPS = {"raw_chain": (4, [2, 2, 2, 1]), "war": (3, [0, 0, 1])}        # flag-2 barriers / all flag 0
GRID_CASES = [(route, kind, bits, place)
              for route in ("grid", "armed") for kind in KIND_STEPS
              for bits, places in ((32, ["end1", "first1", "behind_pre1", "haz2", "last2"]), (31, ["first1", "last2"]))
              for place in places if route == "armed" or place != "behind_pre1"]


@pytest.mark.parametrize("route,kind,bits,place", GRID_CASES, ids=["%s-%s-%d-%s" % c for c in GRID_CASES])
def test_grid_dependent_steps_across_the_wrap(xg, route, kind, bits, place):
    """test_gpu_dep_plans.test_one_gpu_kinds' plan and routing (step_engine_kernel<1>, 256 workgroups,
    every dependent copy another workgroup's first unit), its ticket counter preset after the load:
    3 runs, each from a fresh random image, xg_plan_check clean.  raw_chain: every barrier a hazard
    barrier; war: all flags 0, and an early barrier would overwrite what step 0 still reads."""
    steps, sb, rb = D.solo_kind(kind, PER)
    n, flags = KIND_STEPS[kind]
    job = D.solo_job(steps, sb, rb, kind)
    spans, _size = job.spans()
    assert len(steps) == n and xg.engine_hazards(spans)[0] == flags and _nhaz(xg, job) == flags.count(2)
    armed = int(route == "armed")
    haz = flags.index(2) if 2 in flags else 0       # the dependent step is step 1 in both kinds

    def routing(loaded):
        ld_, d = loaded[0], xg.device()
        W = d.xg_plan_engine(ld_.p)
        assert W > 0 and d.xg_plan_engine_rails(ld_.p) == 0 and d.xg_plan_launches(ld_.p) == 1
        assert ld_.engine_steps() == (n, 1, flags.count(2))
        rec = _loaded_records(xg, ld_.p)
        assert rec["plan"]["may_arm"] == armed and rec["seg"][0]["b"] == 1 and rec["seg"][0]["w"] == W
        assert all(u >= 2 * W for (_m, u) in _units(steps, UNIT))
        assert _assert_other_workgroups(steps, UNIT, W, D.NDEP) >= D.NDEP
        _preset(xg, ld_.p, _tickets(place, 1 << bits, W, n, armed, haz))

    _solo_case(xg, steps, sb, rb, "%s/%s/%d/%s" % (kind, route, bits, place), ROUTES[route], routing,
               seed=100 + GRID_CASES.index((route, kind, bits, place)))


@pytest.mark.parametrize("B", [4, 16])
def test_grid_wider_units_across_the_wrap(xg, B):
    """step_engine_kernel<4> (the read-after-write chain at 4 x the lengths, 220 copies a step: above
    1 MiB) and <16> (dep_plan.unit64_chain): 2^32 inside run 2's first hazard barrier"""
    steps, sb, rb = D.solo_kind("raw_chain", 220, unit=4) if B == 4 else D.unit64_chain()
    job = D.solo_job(steps, sb, rb, "raw_chain_b%d" % B)
    assert _nhaz(xg, job) == 3 and len(steps) == 4

    def routing(loaded):
        ld_, d = loaded[0], xg.device()
        W = d.xg_plan_engine(ld_.p)
        assert W > 0 and d.xg_plan_engine_rails(ld_.p) == 0 and ld_.engine_steps() == (4, 1, 3)
        assert _loaded_records(xg, ld_.p)["seg"][0]["b"] == B
        ndep = D.NDEP if B == 4 else 12
        assert _assert_other_workgroups(steps, B * UNIT, W, ndep) >= ndep
        _preset(xg, ld_.p, _tickets("haz2", M, W, 4, 0, 0))

    _solo_case(xg, steps, sb, rb, job.name, dict(XG_ENGINE_SOLO=0), routing, seed=200 + B)


# ------------------------------------------------------------------ (b) back to back across the wrap
@pytest.mark.parametrize("ld", ["grid", "solo"], indirect=True)
def test_rounds_with_no_wait_across_the_wrap(xg, ld):
    """19 rounds posted with xg_plan_enqueue and one sync, plan a's counter preset so that 2^32 falls
    inside round 9's launch: the host's base runs up to ten launches ahead of the device word.
    "solo" launches unarmed and touches no counter: the preset itself must disturb nothing."""
    n, nseg, _nh = _engine_steps(ld.a)
    W = ld.d.xg_plan_engine(ld.a.p)
    assert (n, nseg) == (12, 1) and W == ld.c["a"]["segs"][0]["w"]
    T = W * n
    _begin(ld)
    _preset(xg, ld.a.p, M - 8 * T - T // 2)
    _post(ld, 19)
    _check(ld, 19, "19 rounds across the wrap")


def _engine_steps(sy):
    ns, nh = C.c_int(), C.c_int()
    n = sy.d.xg_plan_engine_steps(sy.p, C.byref(ns), C.byref(nh))
    return n, ns.value, nh.value


# ------------------------------------------------------------------ (c) preset, replay, eager, replay
@pytest.mark.parametrize("ld", ["grid_launch_graph"], indirect=True)
def test_replay_zeroes_a_preset_state(xg, ld):
    """a segment and a launch in one graph: the preset puts the counter next to 2^32, the replay's
    captured memset restarts it from zero all the same, the eager round inside a kernel-timing
    session re-zeroes after the replay, and the next replay again"""
    n, nseg, _nh = _engine_steps(ld.a)
    W = ld.d.xg_plan_engine(ld.a.p)
    assert (n, nseg, W) == (11, 1, 3)
    _begin(ld)
    _preset(xg, ld.a.p, M - W * n // 2)
    _post(ld, 1)
    ld.cx.ktime_begin(per_launch=False)
    _post(ld, 1)
    _ms, launches, _bytes = ld.cx.ktime_end()
    assert launches == ld.d.xg_plan_launches(ld.a.p) + ld.d.xg_plan_launches(ld.b.p)
    _post(ld, 1)
    _check(ld, 3, "preset, replay, eager, replay")


# ------------------------------------------------------------------ (d) armed solo launches
def _lines(R):
    return min(R, LINES)


def _armed_starts(R):
    """{counter: armed launches before the walk}: two launches before each counter whose divisor (R
    for arrive, the rails of a line for fin, the lines for rails) does not divide 2^32 passes 2^32"""
    divs = [("arrive", R), ("rails", _lines(R))]
    divs += [("fin/%d" % q, q) for q in sorted({len(range(l, R, _lines(R))) for l in range(_lines(R))})]
    return {name: -(-M // d) - 3 for name, d in divs if M % d}


def _run_under_a_second(sy):
    """one timed (armed) run -> (RECV, step times, wall), rc 0 asserted; host time and the run's own
    wall time under 1 s: a launch that fell into the ring's ~2 s timeout or the host's 10 s wait breaks it"""
    t0 = time.perf_counter()
    got, done, wall = sy.run_timed()
    host = time.perf_counter() - t0
    assert host < 1.0 and wall < 1.0, (host, wall)
    return got, done, wall


@pytest.mark.parametrize("ld", ["armed"], indirect=True)
@pytest.mark.parametrize("counter", ["arrive", "fin/3"])
def test_armed_pingpong_across_the_wrap(xg, ld, counter):
    """48 one-wave rails (16 lines of 3), both plans armed through xg_plan_run: six rounds from two
    launches before `arrive` (fin) passes 2^32; the image after every run, a's and b's"""
    R = ld.d.xg_plan_engine_rails(ld.a.p)
    assert R == 48 == ld.d.xg_plan_engine_rails(ld.b.p)
    starts = _armed_starts(R)
    assert set(starts) == {"arrive", "fin/3"}
    _begin(ld)
    for sy in (ld.a, ld.b):                 # the kernel's first launch loads its code: not under the 1 s bound
        sy.run_timed()
    _check(ld, 1, "the first round")
    for sy in (ld.a, ld.b):
        _preset(xg, sy.p, 0, starts[counter])
    for k in range(2, 8):
        half = Synth.expected(types.SimpleNamespace(send=ld.a.send, recv=ld.images[k - 1], steps=ld.pp.steps_a),
                              ld.images[k - 1])
        for sy, want in ((ld.a, half), (ld.b, ld.images[k])):
            got, done, wall = _run_under_a_second(sy)
            _compare(ld.steps, got, want)
            _assert_times(done, wall)
    _check(ld, 7, "six armed rounds across %s's wrap" % counter)


@pytest.mark.parametrize("rails", [3, 7, 37, 64])
def test_armed_rails_across_the_wrap(xg, rails):
    """test_gpu_solo_synth's granule-16 plan (its one segment, so that it arms) on 3, 7, 37 and 64
    one-wave rails: per counter that can misread the wrap at that R, six runs from two launches before
    it; 64 rails (every divisor a power of two) is the control, and takes the doorbell epoch through 0"""
    steps, send_bytes, recv_bytes = _sized(lambda pad: _granule_steps(16, pad), rails, 1, 16)
    plan = _segment(steps)
    _assert_gaps(plan, recv_bytes)
    assert _rails(steps, rails, 1) == rails
    starts = _armed_starts(rails)
    assert set(starts) == {3: {"arrive", "rails"}, 7: {"arrive", "rails"}, 37: {"arrive", "fin/3"}, 64: set()}[rails]
    if rails == 64:
        starts = {"epoch": M - 3}
    cx = _ctx_env(xg, XG_SOLO_RAILS=rails, XG_ENGINE_ARM=1)
    try:
        sy = Synth(xg, cx, send_bytes, recv_bytes, plan, seed=rails)
        try:
            d = xg.device()
            assert d.xg_plan_engine_rails(sy.p) == rails == d.xg_plan_engine(sy.p)
            assert _engine_steps(sy) == (len(plan), 1, 0)
            assert _loaded_records(xg, sy.p)["plan"]["may_arm"] == 1
            want = sy.expected()
            _compare(plan, sy.run(), want)          # the kernel's first launch loads its code: not under the 1 s bound
            for name, armed in starts.items():
                _preset(xg, sy.p, 0, armed)
                for rep in range(6):
                    sy.poison()
                    got, done, wall = _run_under_a_second(sy)
                    _compare(plan, got, want)
                    _assert_times(done, wall)
                    assert d.xg_plan_check(sy.p) == 0, (name, rep)
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ (e) the hook itself
def test_preset_refusals(xg):
    """XG_EARG: no plan; a plan with no engine segment; armed launches of a plan that is not armed;
    ... of an armed plan whose segment runs on the grid engine"""
    d = xg.device()
    assert d.xg_plan_engine_preset(None, 0, 0) == EARG
    steps, send_bytes, recv_bytes = _sized(lambda pad: _granule_steps(16, pad), 7, 1, 16)
    plan = _segment(steps)
    for env, engine, solo, armed_ok in ((dict(XG_ENGINE_MAX_STEP=0), False, False, False),
                                        (dict(XG_SOLO_RAILS=7, XG_ENGINE_ARM=0), True, True, False),
                                        (dict(XG_ENGINE_SOLO=0, XG_ENGINE_ARM=1), True, False, False),
                                        (dict(XG_SOLO_RAILS=7, XG_ENGINE_ARM=1), True, True, True)):
        cx = _ctx_env(xg, **env)
        try:
            sy = Synth(xg, cx, send_bytes, recv_bytes, plan, seed=3)
            try:
                assert (d.xg_plan_engine(sy.p) > 0) == engine and (d.xg_plan_engine_rails(sy.p) > 0) == solo, env
                assert d.xg_plan_engine_preset(sy.p, 0, 0) == (0 if engine else EARG), env
                assert d.xg_plan_engine_preset(sy.p, 5, 0) == (0 if engine else EARG), env
                assert d.xg_plan_engine_preset(sy.p, 0, 1) == (0 if armed_ok else EARG), env
                if engine:                          # back to a state a run can start from, and one run
                    assert d.xg_plan_engine_preset(sy.p, 0, 0) == 0
                    _compare(plan, sy.run(), sy.expected())
                    assert d.xg_plan_check(sy.p) == 0
            finally:
                sy.close()
        finally:
            cx.close()


@pytest.mark.parametrize("engine", ["grid", "solo_armed"])
def test_preset_of_nothing_changes_nothing(xg, engine):
    """(0, 0) on a fresh plan: the run's bytes and xg_plan_check as on a plan never preset"""
    if engine == "grid":
        steps, send_bytes, recv_bytes = _round_steps(3, 700, False)
        env = dict(XG_ENGINE_SOLO=0)
    else:
        full, send_bytes, recv_bytes = _sized(lambda pad: _granule_steps(16, pad), 7, 1, 16)
        steps, env = _segment(full), dict(XG_SOLO_RAILS=7, XG_ENGINE_ARM=1)
    cx = _ctx_env(xg, **env)
    try:
        images = []
        for preset in (False, True):
            sy = Synth(xg, cx, send_bytes, recv_bytes, steps, seed=9)
            try:
                d = xg.device()
                assert d.xg_plan_engine(sy.p) > 0 and (d.xg_plan_engine_rails(sy.p) > 0) == (engine != "grid")
                if preset:
                    _preset(xg, sy.p, 0, 0)
                for _rep in range(2):
                    sy.poison()
                    got = sy.run()
                    _compare(steps, got, sy.expected())
                    assert d.xg_plan_check(sy.p) == 0
                images.append(got.copy())
            finally:
                sy.close()
        assert (images[0] == images[1]).all()
    finally:
        cx.close()
