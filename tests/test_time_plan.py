"""CPU: the host side of the step-time tests (time_plan.py, test_gpu_step_times.py).

(1) Every plan of test_gpu_step_times.py takes, under the GPU test's knobs on a 256-CU device, the
form the GPU test asserts of the loaded plan (time_plan.expected_form and the forms stated beside
the further plans): engine segments and their step ranges, workgroups or rails, launches, chain
ends.  (2) Every engine plan keeps the bytes an engine may load early under a quarter of its heavy
step, and its bound is longer than 20 ticks of the wall clock.  (3) xg_step_times -- the one place
where stamps become step times -- against a dozen-line Python reference on seeded random stamp
sets: launches, chains and segments mixed, marks off on some steps, stamps above 2^63, wall_hz
other than 1e8, armed runs; for consistent stamps no time is clamped to 0.  (4) The solo rails'
closing stamp: a rail writes it to every step behind its last barrier, the host takes it back off
the steps the rail sat out before its last one with pieces (xg_solo_carry_tail) -- found by
test_gpu_step_times.py, where a heavy LAST step's time landed on an earlier step.
"""
import random

import pytest

import time_plan as T


# ------------------------------------------------------------------ (1) the plans' forms
@pytest.mark.parametrize("route,pos", T.CASES)
def test_route_plans_take_the_expected_form(xg, route, pos):
    steps, send_bytes, recv_bytes, p = T.sized(route, pos)
    r = T.ROUTES[route]
    H, light = r["H"], r.get("light", T.LIGHT)
    n = len(steps) - (1 if r.get("tail") else 0)
    assert p == T.position(pos, n) and sum(c[4] for c in steps[p]) == H
    assert all(sum(c[4] for c in st) == light and len(st) == T.LIGHT_COPIES for s, st in enumerate(steps[:n]) if s != p)
    assert H >= 256 * light
    assert all((so | do | ln) % 16 == 0 and (sb, db) == (0, 1) for st in steps for (sb, so, db, do, ln) in st)
    f = T.tables_form(xg, T.devplan(xg, steps, send_bytes, recv_bytes), r["env"])
    assert f == T.expected_form(route, len(steps)), (f, T.expected_form(route, len(steps)))
    if r.get("tail"):                   # the step behind the segment is no engine step
        assert sum(c[4] for c in steps[-1]) > 16 << 20 and f["segs"][0]["steps"][1] == len(steps) - 1


@pytest.mark.parametrize("route", [r for r in T.ROUTES if T.ROUTES[r]["kind"] in ("grid", "solo")])
def test_engine_plans_keep_their_discount_and_a_measurable_bound(xg, route):
    r = T.ROUTES[route]
    for pos in T.POSITIONS:
        steps, send_bytes, recv_bytes, _p = T.sized(route, pos)
        f = T.tables_form(xg, T.devplan(xg, steps, send_bytes, recv_bytes), r["env"])
        seg = f["segs"][0]
        assert 0 < T.discount(seg) <= r["H"] // 4, (T.discount(seg), r["H"])
        assert T.bound(route, f) == T.lower_cus(r["H"] - T.discount(seg), r["w"])
        assert T.bound(route, f) * T.WALL_HZ > T.MIN_TICKS
    if route.startswith("solo1x64"):    # rails with nothing in the step behind the heavy one
        assert r["w"] > T.LIGHT // T.PIECE


def test_bounds():
    assert T.CACHE == 288 << 20 and abs(T.CU_RATE - 144.1e9) < 0.1e9
    assert T.lower_chip(16 << 20) == (16 << 20) / T.L2_RATE                     # inside the caches: the L2 rate
    assert abs(T.lower_chip(512 << 20) - 96.5e-6) < 0.1e-6                      # past them: HBM
    assert T.lower_cus(1 << 20, 8) == (1 << 20) / (8 * T.CU_RATE) and T.lower_cus(1 << 20, 300) == T.lower_cus(1 << 20, 256)
    assert T.discount(dict(solo=0, w=8, b=16)) == 8 * 65536
    assert T.discount(dict(solo=1, w=16, wv=16)) == 16 * 2 * 8 * 16 * 1024 and T.discount(dict(solo=1, w=64, wv=1)) == 1 << 20


def test_further_plans_take_the_expected_form(xg):
    """two segments round a launch; the launches route of the unmarked step; the virtual jobs"""
    steps, sb, rb = T.heavy_steps(T.TWO_SEG["n"], T.TWO_SEG["p"], T.TWO_SEG["H"])
    assert T.tables_form(xg, T.devplan(xg, steps, sb, rb), T.TWO_SEG["env"]) == T.TWO_SEG_FORM
    steps, sb, rb = T.heavy_steps(T.UNMARKED["n"], T.UNMARKED["p"], T.UNMARKED["H"])
    for env in T.UNMARKED["envs"].values():
        f = T.tables_form(xg, T.devplan(xg, steps, sb, rb), env)
        assert f == dict(nsteps=7, launches=7, segs=[], chains=[], armed=0)
    for job, spec, want in ((T.job_cross(), T.V_CROSS, T.V_CROSS_FORM), (T.job_segment(), T.V_SEG, T.V_SEG_FORM)):
        job.check()
        for g in range(2):
            pt = xg.PlanTables(job.devplan(xg, g), env=spec["env"], rank=g, nranks=2, virt=1)
            try:
                rec = pt.records()
            finally:
                pt.close()
            f = T.form(rec)
            f.pop("chains")             # a virtual job stamps no chains (xg_vplans_run marks every step)
            assert f == want, (job.name, g, f)
            # nothing of the heavy step is put off into the next step's launch, nothing joins the one before
            assert not rec["step"][spec["p"]]["form"] & (xg.FORM_DEFERRED | xg.FORM_FUSED | xg.FORM_FUSED_LOCAL)
            assert not rec["step"][spec["p"] + 1]["form"] & (xg.FORM_FUSED | xg.FORM_FUSED_LOCAL)
    seg = T.V_SEG_FORM["segs"][0]
    assert T.discount(seg) <= T.V_SEG["H"] // 4
    assert T.lower_cus(T.V_SEG["H"] - T.discount(seg), seg["w"]) * T.WALL_HZ > T.MIN_TICKS


# ------------------------------------------------------------------ (3) xg_step_times
def _random_run(rng, hz, base):
    """a plan of launches, chains and segments mixed with consistent stamps: device ticks rise
    along the run; -> the arguments of xg_step_times and the true tick of every step's end"""
    n = rng.randint(1, 40)
    seg_of, seg_end, chain_end = [-1] * n, [], [0] * n
    s = 0
    while s < n:
        kind = rng.choice(("launch", "launch", "chain", "seg"))
        e = min(n, s + rng.randint(2, 9)) if kind != "launch" else s + 1
        if kind == "chain" and e - s >= 2:
            chain_end[s] = e
        elif kind == "seg" and e - s >= 1:
            for t in range(s, e):
                seg_of[t] = len(seg_end)
            seg_end.append(e)
        else:
            e = s + 1
        s = e
    need = [1 if rng.random() < 0.7 else 0 for _ in range(n)]
    need[-1] = 1
    t = base
    marks, cst, est, true = [t] + [0] * n, [0] * n, [0] * n, [0] * n
    s = 0
    while s < n:
        if chain_end[s]:
            e = chain_end[s]
        elif seg_of[s] >= 0:
            e = seg_end[seg_of[s]]
        else:
            e = s + 1
        t += rng.randint(100, 800)                       # the launch
        tick = {}
        for u in range(s, e):
            t += rng.randint(1, 100000)
            tick[u] = t
            if chain_end[s]:
                cst[u] = t & T.M64
            elif seg_of[s] >= 0:
                est[u] = t & T.M64
        t += rng.randint(50, 400)                        # the mark behind the unit
        marks[e] = t & T.M64
        for u in range(s, e):                            # anchored at the mark: every stamp later by the mark's delay
            true[u] = tick[u] + (t - tick[e - 1])
        s = e
    marks[0] = base & T.M64
    return dict(marks=marks, seg_of=seg_of, seg_end=seg_end, wall_hz=hz, chain_stamps=cst, engine_stamps=est,
                chain_end=chain_end, need_mark=need), true


@pytest.mark.parametrize("seed", range(12))
def test_step_times_against_the_reference(xg, seed):
    rng = random.Random(seed)
    for rep in range(40):
        hz = rng.choice((1e8, 1e8, 2.5e7, 1e9, 99999871.0))
        base = rng.choice((0, 12345, (1 << 63) + rng.randrange(1 << 62), (1 << 64) - rng.randrange(1, 200000)))
        a, true = _random_run(rng, hz, base)
        if rep % 4 == 3:                # no marks off
            a["need_mark"] = None
        rc, got = xg.step_times(**a)
        want, clamped = T.step_times_ref(**a)
        assert rc == 0 and got == pytest.approx(want, rel=1e-12, abs=1e-12), (seed, rep)
        assert clamped == [], (seed, rep, clamped)
        n = len(got)
        assert all(x <= y for x, y in zip(got, got[1:]))
        for s in range(n):              # a step that has a time of its own: its true end after the start
            own = a["seg_of"][s] >= 0 or any(b <= s < e for b, e in enumerate(a["chain_end"]) if e) or \
                a["need_mark"] is None or a["need_mark"][s]
            if own:
                assert got[s] == pytest.approx((true[s] - base) / hz, rel=1e-9), (seed, rep, s)
            else:
                nxt = min(t for t in range(s + 1, n) if a["seg_of"][t] >= 0 or a["chain_end"][t] or a["need_mark"][t])
                assert got[s] == got[nxt]


@pytest.mark.parametrize("seed", range(4))
def test_step_times_of_an_armed_run(xg, seed):
    rng = random.Random(100 + seed)
    for _rep in range(40):
        n = rng.randint(1, 50)
        hz = rng.choice((1e8, 2.5e7))
        t = rng.choice((5000, (1 << 63) + 17, (1 << 64) - 1000))
        est = []
        for _s in range(n):
            t += rng.randint(1, 50000)
            est.append(t & T.M64)
        total = (est[-1] - est[0] & T.M64) / hz + rng.random() * 1e-5 + 1e-9
        a = dict(marks=None, seg_of=[0] * n, seg_end=[n], wall_hz=hz, engine_stamps=est, host_total=total)
        rc, got = xg.step_times(**a)
        want, clamped = T.step_times_ref(**a)
        assert rc == 0 and got == pytest.approx(want, rel=1e-12, abs=1e-15) and clamped == []
        assert got[-1] == total and all(0 < x <= y for x, y in zip(got, got[1:]))


def test_step_times_clamp_and_errors(xg):
    """an inconsistent stamp (later than its segment's last) is clamped to 0 and the reference names
    it; bad arguments are refused"""
    a = dict(marks=[1000, 0, 0, 5000], seg_of=[0, 0, 0], seg_end=[3], wall_hz=1e8, engine_stamps=[2000, 9000, 3000])
    rc, got = xg.step_times(**a)
    want, clamped = T.step_times_ref(**a)
    assert rc == 0 and got == want and clamped == [1] and got[1] == 0.0 and got[0] == pytest.approx(3e-5)
    a = dict(marks=[0, 10, 20], seg_of=[-1, -1], seg_end=[], wall_hz=1e8)
    assert xg.step_times(**a) == (0, [1e-7, 2e-7])
    assert xg.step_times(**dict(a, wall_hz=0.0))[0] == xg.EARG
    assert xg.step_times(**dict(a, seg_of=[0, 0], seg_end=[2]))[0] == xg.EARG          # a segment without engine stamps
    assert xg.step_times(**dict(a, seg_of=[0, 0], seg_end=[3], engine_stamps=[1, 2]))[0] == xg.EARG    # its end past the plan
    assert xg.step_times(**dict(a, chain_stamps=[1, 2], chain_end=[5, 0]))[0] == xg.EARG
    # the back-fill: the unmarked first step is done when the second is
    assert xg.step_times(**dict(a, need_mark=[0, 1])) == (0, [2e-7, 2e-7])


# ------------------------------------------------------------------ the solo rails' closing stamp
def _rail_steps(xg, steps, rails_max, waves):
    """per rail, the steps it has pieces in, in order -- read back from the tables' descriptors
    (each real piece's source address names its transfer, so its step), not from the deal"""
    from synth_plan import DBASE, PIECE, SBASE, _spans
    sp = _spans(steps)
    step_of = {src + o: t for t, st in enumerate(sp) for (src, _dst, n) in st for o in range(0, n, PIECE)}
    rc, shape, descs, close, csteps, rows = xg.solo_tables(sp, rails_max, SBASE, DBASE, waves=waves)
    assert rc == 0
    busy = []
    for r in range(shape["rails"]):
        if waves == 1:
            srcs = [SBASE + 16 * (d & 0xFFFFFFFF) for d in descs[r][:rows[r]]]
        else:
            srcs = [SBASE + 16 * (d & 0xFFFFFF) for d in descs[r] if (d >> 48) & 0x7F]
        busy.append([step_of[s] for s in srcs])
        assert busy[-1] == sorted(busy[-1])
    return sp, shape["rails"], csteps, busy


def _kernel_stamps(n, csteps, busy, rng):
    """solo_engine_kernel's stamps of one run: every rail on a clock of its own stamps the steps its
    barriers close, and writes its closing stamp to every step behind its last barrier -> (stamps
    [rail][step], when each rail finished each step it has pieces in)"""
    stamps, fin = [], []
    for cs, b in zip(csteps, busy):
        t, f = rng.randint(1, 1000), {}
        for s in b:
            t += rng.randint(1, 50)
            f[s] = t                    # the rail's last piece of step s so far
        closed = [c for c in cs if c >= 0]
        assert closed == sorted(set(b))[:-1]            # every busy step but the last has a barrier
        s_end = closed[-1] + 1 if closed else 0
        stamps.append([t if i >= s_end else f.get(i, 0) if i in closed else 0 for i in range(n)])
        fin.append(f)
    return stamps, fin


@pytest.mark.parametrize("waves,rails", [(1, 64), (1, 7), (16, 16), (16, 3)])
def test_solo_stamps_put_a_rails_last_step_where_it_is(xg, waves, rails):
    """Step times of a solo segment = MAX over rails of each rail's finish of its latest step with
    pieces at or before t.  Plans whose steps often hold fewer pieces than there are rails, so that
    rails sit steps out -- also just before their last step: there the kernel's closing stamp must
    not stand for the steps sat out (xg_solo_carry_tail), and left in it does differ."""
    rng = random.Random(waves * 100 + rails)
    differs = 0
    for _rep in range(20):
        n = rng.randint(2, 24)
        counts = [rng.choice((0, 1, 2, 5, waves, 3 * waves, rails * waves + 3)) for _ in range(n)]
        counts[rng.randrange(n)] = 4 * rails * waves          # every rail has pieces
        specs = [(1024 * c, 0, 0) if c else None for c in counts]
        copies, _sb, _rb = T._layout([x for x in specs if x])
        it = iter(copies)
        steps = [[next(it)] if x else [] for x in specs]
        sp, R, csteps, busy = _rail_steps(xg, steps, rails, waves)
        assert R == rails
        last = xg.solo_rail_last(sp, R)
        assert last == [b[-1] for b in busy]
        stamps, fin = _kernel_stamps(n, csteps, busy, rng)
        want = [max(max([f[s] for s in f if s <= t] + [0]) for f in fin) for t in range(n)]
        got = xg.solo_reduce_stamps(xg.solo_carry_tail(stamps, csteps, last), 0, n)
        assert got == want, (counts, got, want)
        differs += xg.solo_reduce_stamps(stamps, 0, n) != want
    assert differs > 0


def test_step_times_under_sanitizers(tmp_path):
    """tests/step_times_san.c (its own main) runs xg_step_times and the solo stamp functions over
    2000 seeded plans with every array at exactly its stated size, compiled with csrc/host/solo.c
    under AddressSanitizer and UBSan and run as an executable"""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    solo = os.path.join(repo, "mpi-asynchronous-communication-test_amd", "csrc", "host", "solo.c")
    exe = str(tmp_path / "step_times_san")
    subprocess.run(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(repo, "include"),
                    os.path.join(here, "step_times_san.c"), solo, "-o", exe, "-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    assert "2000 plans timed" in out.stdout, out.stdout
