"""GPU: runs posted back to back with no wait between them, as bench.py posts them.

bench.py posts --steps repetitions of every plan with xg_plan_enqueue and synchronises once;
warm-up replays graphs where the plan allows, the timed region runs inside a kernel-timing session
(which turns replay off) and only xg_plan_check follows it.  Every other test waits for the device
after each run, and no schedule of the product could show a lost, repeated or reordered run anyway:
it reads SEND and writes fixed RECV slots.  The two plans of pingpong.py share one xg_regions on one
context and leave a different image after every number of rounds (a round: plan a, then plan b),
so here

    k rounds posted without a wait == k in-order rounds of the numpy execution,

bit for bit over the whole RECV, gaps included, through every form a run can take: pingpong.CASES
(host side: test_pingpong.py) puts plan a on the solo engine (one-wave rails, workgroup rails,
granule 1), the grid engine, chained copy_kernel_g launches posted or replayed as a graph, a
segment and a launch in one graph (asked for, and by default), copy_kernel_s, copy_kernel_x,
copy_kernel_q, an armed segment, and launches cut into dispatches.  Each case asserts its routing on
the loaded plans first: a case that fell to another kernel fails.

The sequences: (1) K rounds, one sync; (2) the benchmark's -- rounds, a whole-session kernel timing
around more rounds, rounds again, with no wait anywhere: in the graph cases replay -> eager -> replay;
(3) a per-launch session, every dispatch's bytes against the plan's tables; (4) timed (or armed)
xg_plan_run calls behind queued work; (5) step marks changed between rounds.

Out of scope: copy_kernel_w is a cross-GPU launch kind, and copy_kernel_v has a runtime object of
its own (xg_vecplace) that takes no xg_plan_enqueue.
"""
import ctypes as C
import time
import types

import numpy as np
import pytest

import pingpong as PP
from synth_plan import _compare, _ctx_env
from time_plan import devplan

pytestmark = pytest.mark.gpu

SEED = 5


def _loaded_records(xg, plan):
    d = xg.device()
    d.xg_plan_tables_of.restype = C.c_void_p
    d.xg_plan_tables_of.argtypes = [C.c_void_p]
    return xg.parse_tables(xg.dump_tables(C.c_void_p(d.xg_plan_tables_of(plan))))


def _assert_routing(xg, case, which, sy, pp):
    """the loaded plan took the form the case states (and test_pingpong.py proved of the host tables)"""
    c, d = PP.CASES[case], xg.device()
    want = c[which]
    rec = _loaded_records(xg, sy.p)
    kinds = xg.plan_kind_launches(sy.p)
    f = PP.form(rec, kinds)
    assert f == want, (case, which, f, want)
    seg = want["segs"][0] if want["segs"] else None
    assert d.xg_plan_engine(sy.p) == (seg["w"] if seg else 0)
    assert d.xg_plan_engine_rails(sy.p) == (seg["w"] if seg and seg["solo"] else 0)
    assert d.xg_plan_launches(sy.p) == want["launches"]
    nsmall = C.c_int()
    assert (d.xg_plan_shift_launches(sy.p), d.xg_plan_extent_launches(sy.p),
            d.xg_plan_small_launches(sy.p, C.byref(nsmall))) == tuple(want["kinds"][2:5]), (case, which)
    # the dispatches of a run and their bytes: the loaded tables and the host's own build agree
    dp = devplan(xg, sy.steps, pp.send_bytes, pp.recv_bytes)
    dp.flags = pp.flags
    pt = xg.PlanTables(dp, env=c["env"])
    try:
        disp = PP.dispatch_bytes(pt.records())
    finally:
        pt.close()
    assert disp == PP.dispatch_bytes(rec) and len(disp) == want["launches"] and sum(disp) == pp.bytes_a()
    return disp


@pytest.fixture(scope="module")
def ld(request, xg):
    """one context under the case's knobs, both plans over one xg_regions, the routing asserted, and
    the images after 0 .. kmax rounds from one seeded random RECV (computed once, never written to)"""
    case = request.param
    c = PP.CASES[case]
    pp = PP.pingpong(**c["gen"])
    cx = _ctx_env(xg, **c["env"])
    try:
        a = PP.FlagSynth(xg, cx, pp.send_bytes, pp.recv_bytes, pp.steps_a, seed=SEED, flags=pp.flags)
        try:
            b = PP.FlagSynth.over(a, cx, pp.steps_b, flags=pp.flags)
            try:
                disp_a = _assert_routing(xg, case, "a", a, pp)
                disp_b = _assert_routing(xg, case, "b", b, pp)
                recv0 = np.random.default_rng(SEED + 1).integers(0, 256, pp.recv_bytes, dtype=np.uint8)
                images = pp.images(c["kmax"], a.send, recv0)
                for im in images:
                    im.setflags(write=False)
                yield types.SimpleNamespace(case=case, c=c, pp=pp, cx=cx, a=a, b=b, d=xg.device(), images=images,
                                            disp=disp_a + disp_b, nbytes=pp.bytes_a() + pp.bytes_b(),
                                            steps=pp.steps_a + pp.steps_b)
            finally:
                b.close()
        finally:
            a.close()
    finally:
        cx.close()


every_case = pytest.mark.parametrize("ld", PP.BACK_TO_BACK, indirect=True)


def _begin(ld):
    """RECV := the seeded image (SEND holds its seeded bytes since the load)"""
    ld.a.write_recv(ld.images[0])


def _post(ld, rounds):
    for _ in range(rounds):
        assert ld.d.xg_plan_enqueue(ld.a.p) == 0
        assert ld.d.xg_plan_enqueue(ld.b.p) == 0


def _check(ld, k, what):
    """after a sync: the whole RECV is the k-round image, SEND is untouched, no engine barrier timed out"""
    ld.cx.sync()
    got = ld.a.read(1)
    if not (got == ld.images[k]).all():
        same = [j for j, im in enumerate(ld.images) if (got == im).all()]
        print("%s %s: expected the image after %d rounds; RECV equals the image after %s"
              % (ld.case, what, k, ("%d rounds" % same[0]) if same else "no number of rounds"))
    _compare(ld.steps, got, ld.images[k])
    assert (ld.a.read(0) == ld.a.send).all(), "SEND changed"
    assert ld.d.xg_plan_check(ld.a.p) == 0 and ld.d.xg_plan_check(ld.b.p) == 0


def _timed_run(ld, sy):
    """xg_plan_run -> (step_done, wall), rc 0 asserted"""
    n = len(sy.steps)
    done, post, wall = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
    assert ld.d.xg_plan_run(sy.p, done, post, C.byref(wall)) == 0
    return list(done), wall.value


def _assert_times(done, wall):
    assert all(0 <= x <= y for x, y in zip(done, done[1:])) and done[0] >= 0, done
    assert done[-1] <= wall + 1e-4, (done[-1], wall)


# ------------------------------------------------------------------ 1. rounds with no wait
@every_case
@pytest.mark.parametrize("K", [1, 2, 19])
def test_rounds_with_no_wait(ld, K):
    _begin(ld)
    _post(ld, K)
    _check(ld, K, "%d rounds" % K)


# ------------------------------------------------------------------ 2. the benchmark's sequence
@every_case
def test_benchmark_sequence(ld):
    """3 rounds, a whole-session kernel timing around 7 rounds, 5 rounds: one sync at the end (and
    the one inside xg_ktime_end).  A graph case replays, runs eager inside the session, and replays."""
    W, K, T = 3, 7, 5
    la, lb = ld.d.xg_plan_launches(ld.a.p), ld.d.xg_plan_launches(ld.b.p)
    _begin(ld)
    _post(ld, W)
    t0 = time.perf_counter()
    ld.cx.ktime_begin(per_launch=False)
    _post(ld, K)
    ms, n, nbytes = ld.cx.ktime_end()
    _post(ld, T)
    ld.cx.sync()
    host = time.perf_counter() - t0
    print("%s: session of %d rounds: %d launches, %d B, %.1f us on the device, %.1f us on the host clock"
          % (ld.case, K, n, nbytes, ms * 1e3, host * 1e6))
    _check(ld, W + K + T, "benchmark sequence")
    assert n == K * (la + lb), (n, K, la, lb)
    assert nbytes == 2 * K * ld.nbytes, (nbytes, K, ld.nbytes)
    assert 0 < ms * 1e-3 <= host, (ms, host)


# ------------------------------------------------------------------ 3. per-launch session
@pytest.mark.parametrize("ld", list(PP.CASES), indirect=True)
def test_per_launch_session(ld):
    """every dispatch of 3 rounds, in order: 2 x the bytes the plan's tables say it moves, a time of its own"""
    R = 3
    n = R * len(ld.disp)
    _begin(ld)
    t0 = time.perf_counter()
    ld.cx.ktime_begin(n, per_launch=True)
    _post(ld, R)
    ms, got_n, nbytes = ld.cx.ktime_end()
    ld.cx.sync()
    host = time.perf_counter() - t0
    assert got_n == n, (got_n, n)
    per = ld.cx.ktime_launches(got_n)
    print("%s: %d launches, %.1f us in all, %.1f us on the host clock; bytes %s"
          % (ld.case, got_n, ms * 1e3, host * 1e6, [b for _t, b in per[:len(ld.disp)]]))
    assert [b for _t, b in per] == [2 * x for x in ld.disp] * R
    assert sum(b for _t, b in per) == nbytes == 2 * R * ld.nbytes
    assert all(t > 0 for t, _b in per), [t for t, _b in per]
    assert sum(t for t, _b in per) * 1e-3 <= host, (sum(t for t, _b in per), host)
    _check(ld, R, "per-launch session")


# ------------------------------------------------------------------ 4. a timed run behind queued work
@every_case
def test_timed_run_behind_queued_work(ld):
    """5 rounds posted, then xg_plan_run of a and of b (armed case: armed launches that start behind
    the queue and must meet their own deadlines): the 6-round image, step times in order and inside
    the run's wall time"""
    _begin(ld)
    _post(ld, 5)
    done_a, wall_a = _timed_run(ld, ld.a)
    done_b, wall_b = _timed_run(ld, ld.b)
    print("%s: a done %.1f us of %.1f us, b done %.1f us of %.1f us"
          % (ld.case, done_a[-1] * 1e6, wall_a * 1e6, done_b[-1] * 1e6, wall_b * 1e6))
    _assert_times(done_a, wall_a)
    _assert_times(done_b, wall_b)
    _check(ld, 6, "timed run behind 5 rounds")


# ------------------------------------------------------------------ 5. marks changed between rounds
@every_case
def test_marks_changed_between_rounds(ld):
    """2 rounds, xg_plan_set_step_marks (only a's last step; captured graphs are dropped), 2 rounds:
    the 4-round image.  Then a timed round under the new marks: the 5-round image."""
    _begin(ld)
    _post(ld, 2)
    n = len(ld.a.steps)
    try:
        assert ld.d.xg_plan_set_step_marks(ld.a.p, (C.c_uint8 * n)(*([0] * (n - 1) + [1]))) == 0
        _post(ld, 2)
        _check(ld, 4, "marks changed after 2 of 4 rounds")
        done, wall = _timed_run(ld, ld.a)
        _assert_times(done, wall)
        done, wall = _timed_run(ld, ld.b)
        _assert_times(done, wall)
        _check(ld, 5, "a timed round under the new marks")
    finally:
        assert ld.d.xg_plan_set_step_marks(ld.a.p, None) == 0
