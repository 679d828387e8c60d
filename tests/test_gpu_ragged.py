"""GPU: ragged exchanges (xg_sched_build_v, xg_exchange_v) and copy_kernel_s, the shifted piece
copy their misaligned launches run (csrc/kernels.h).

The kernel is driven through synthetic one-GPU plans with XG_DP_RAGGED set (synth_plan's layout:
seeded random SEND, poisoned RECV, a poisoned gap of >= 16 B around every destination) and judged
bit for bit over the whole RECV region against the in-order numpy execution, so an overrun, a
dropped or a shifted store all show.  The schedules run over a caller's buffers (random payload,
guards) and are judged by the numpy delivery over xg_deliveries / xg_delivery_lens and by the span
checksums (xg.payload_check).
"""
import ctypes as C
import json
import pathlib
import sys
import tempfile

import numpy as np
import pytest

from conftest import REPO
from synth_plan import CHUNK_A, PHASE_PAIRS, Synth, _assert_gaps, _compare, _ctx_env, _layout, realign_edge_lens
from test_gpu_payload import PACKINGS, Caller, _rand, _read, _virtual_job, _write

pytestmark = pytest.mark.gpu

NEVER = 1 << 40
RAGGED_METHODS = list(range(1, 15)) + [17, 18, 19, 20]
SWEEP_LENS = [1, 15, 16, 17, 33, 4097]


class RaggedSynth(Synth):
    """synth_plan.Synth with the device plan's flags word set before the plan is loaded"""

    def __init__(self, xg, ctx, send_bytes, recv_bytes, steps, seed=0, flags=0):
        d = xg.device()
        self.xg, self.d = xg, d
        rb = (C.c_int64 * xg.NBUF)(send_bytes, recv_bytes, 0, 0, 0)
        self.r = C.c_void_p()
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(self.r)) == 0
        self.send = np.random.default_rng(seed).integers(0, 256, send_bytes, dtype=np.uint8)
        self.recv = np.full(recv_bytes, 0xA5, np.uint8)
        buf = self.send.tobytes()
        assert d.xg_regions_write(self.r, xg.BUF_SEND, 0, buf, len(buf)) == 0
        copies = [c for st in steps for c in st]
        self.copies = (xg.Copy * max(1, len(copies)))(*[xg.Copy(so, do, ln, sb, db) for (sb, so, db, do, ln) in copies])
        sp, b = [], 0
        for st in steps:
            sp.append(xg.StepPlan(b, len(st), 0, 0, 0, 0, 0, 0))
            b += len(st)
        self.sp = (xg.StepPlan * len(sp))(*sp)
        self.p2p = (xg.P2P * 1)()
        dp = xg.DevPlan()
        dp.gpu, dp.ngpus, dp.nsteps, dp.flags = 0, 1, len(steps), flags
        for i, v in enumerate((send_bytes, recv_bytes, 0, 0, 0)):
            dp.region_bytes[i] = v
        dp.ncopy, dp.np2p = len(copies), 0
        dp.copies = C.cast(self.copies, C.POINTER(xg.Copy))
        dp.p2p = C.cast(self.p2p, C.POINTER(xg.P2P))
        dp.steps = C.cast(self.sp, C.POINTER(xg.StepPlan))
        self.dp = dp
        self.p = C.c_void_p()
        assert d.xg_plan_load(ctx.handle, self.r, C.byref(dp), C.byref(self.p)) == 0
        self.steps = steps

    def read_send(self):
        out = C.create_string_buffer(len(self.send))
        assert self.d.xg_regions_read(self.r, 0, 0, out, len(self.send)) == 0
        return np.frombuffer(out.raw, np.uint8)


def _edge_steps():
    """step 0: synth_plan's phase pairs x realign_edge_lens (the byte path either side of its
    threshold, bodies around 4 KiB multiples with tails 0 / 1 / 15, a full piece, two and three
    pieces at the pinned CHUNK_A) plus CHUNK_A - 1 and CHUNK_A; steps 1..6: all 256 (source phase,
    destination phase) pairs at one of SWEEP_LENS each"""
    specs, cuts = [], [0]
    for (sp, dp) in PHASE_PAIRS:
        specs += [(n, sp, dp) for n in realign_edge_lens(dp) + [CHUNK_A - 1, CHUNK_A]]
    cuts.append(len(specs))
    for n in SWEEP_LENS:
        specs += [(n, sp, dp) for sp in range(16) for dp in range(16)]
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[a:b] for a, b in zip(cuts, cuts[1:])]
    assert all((so % 16, do % 16) == (sp, dp) for (_a, so, _b, do, _n), (_m, sp, dp) in zip(copies, specs))
    return steps, send_bytes, recv_bytes


def _run_synth(xg, cx, flags, want_shift, seed):
    steps, send_bytes, recv_bytes = _edge_steps()
    assert send_bytes + recv_bytes < 16 << 20
    _assert_gaps(steps, recv_bytes)
    cx.set_copy_params(CHUNK_A, -1)
    assert xg.piece_size([c[4] for c in steps[0]], CHUNK_A, cx.info()[1], 2048) == CHUNK_A
    sy = RaggedSynth(xg, cx, send_bytes, recv_bytes, steps, seed=seed, flags=flags)
    try:
        d = xg.device()
        assert d.xg_plan_engine(sy.p) == 0
        assert d.xg_plan_launches(sy.p) == len(steps)
        assert sum(xg.plan_kind_launches(sy.p)) == len(steps) - xg.plan_engine_segments(sy.p)
        assert xg.plan_wave_launches(sy.p)[0] == 0
        assert d.xg_plan_shift_launches(sy.p) == (len(steps) if want_shift else 0)
        want = sy.expected()
        got = sy.run()
        _compare(steps, got, want)                          # RECV over its whole length, gaps still 0xA5
        assert np.array_equal(sy.read_send(), sy.send), "SEND was written"
    finally:
        sy.close()


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("variant", [1, 6])
def test_shifted_copy_edges(xg, variant):
    """copy_kernel_s<NT> (plain: XG_COPY_VARIANT=1, non-temporal: 6), one launch per step
    (XG_ENGINE_MAX_STEP=0) of a synthetic plan with XG_DP_RAGGED: every step runs it
    (xg_plan_shift_launches == steps), RECV equals the numpy execution bit for bit over its whole
    length -- head, body, tail, the byte path, the one-load path where the phases agree, pieces
    cut at CHUNK_A -- and SEND is unchanged"""
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=NEVER, XG_COPY_VARIANT=variant)
    try:
        _run_synth(xg, cx, xg.DP_RAGGED, True, seed=variant)
    finally:
        cx.close()


@pytest.mark.parametrize("how", ["no flag", "XG_RAGGED_COPY=0"])
def test_shifted_copy_routing_off(xg, how):
    """the same plan without XG_DP_RAGGED, and with the flag under XG_RAGGED_COPY=0: no launch
    runs copy_kernel_s (copy_kernel_g's realign path carries them) and it still delivers"""
    env = dict(XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=NEVER, XG_COPY_VARIANT=1)
    if how != "no flag":
        env["XG_RAGGED_COPY"] = 0
    cx = _ctx_env(xg, **env)
    try:
        _run_synth(xg, cx, 0 if how == "no flag" else xg.DP_RAGGED, False, seed=11)
    finally:
        cx.close()


def test_aligned_launch_of_a_ragged_plan_keeps_its_kernel(xg):
    """in a plan with XG_DP_RAGGED a launch whose copies are all on the 16-B grid keeps today's
    kernel: step 0 (aligned) is not a shift launch, step 1 (one odd length) is"""
    copies, send_bytes, recv_bytes = _layout([(4096, 0, 0), (8192, 0, 0), (4097, 0, 0)])
    steps = [copies[:2], copies[2:]]
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=NEVER, XG_COPY_VARIANT=1)
    try:
        sy = RaggedSynth(xg, cx, send_bytes, recv_bytes, steps, seed=5, flags=xg.DP_RAGGED)
        try:
            assert xg.device().xg_plan_shift_launches(sy.p) == 1
            _compare(steps, sy.run(), sy.expected())
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ 2. ragged exchange, one GPU
P, A = 8, 3


def _ragged_lens():
    rng = np.random.default_rng(83)
    lens = [int(x) for x in rng.integers(0, 3 * 32768 + 101, P * A)]
    for k, v in ((0, 0), (2, 1), (5, 15), (7, 16), (10, 17), (13, 3 * 32768), (16, 0), (23, 3 * 32768 + 100)):
        lens[k] = v
    return lens


def _deliver_v(image, caller, s):
    send = image[caller.send_off:caller.send_off + caller.send_bytes].copy()
    for q, n in zip(s.deliveries(1), s.delivery_lens(1)):
        image[caller.recv_off + q.recv_off:caller.recv_off + q.recv_off + n] = send[q.send_off:q.send_off + n]


@pytest.mark.parametrize("engine", ["per-step launches", "engines"])
def test_ragged_exchange_on_one_gpu(xg, engine):
    """P 8, A 3, seeded lengths in 0 .. 3 x 32768 + 100 (0, 1, 15, 16, 17 and a multiple of 16 among
    them), methods 1-14 and 17-20 over a caller's arena (+48 B skew, 64 guard bytes), with one
    launch per step (XG_ENGINE_MAX_STEP=0: copy_kernel_s carries the steps) and with the step
    engines: the whole arena equals the numpy delivery -- every slot its own length of its source
    segment, guards and SEND intact -- payload_check finds nothing, slot_chk() equals the oracle's
    checksum of every slot, and one flipped byte is reported as exactly that slot"""
    import xg_oracle as O
    lens = _ragged_lens()
    rl = xg.aggregator_list(P, A)
    env = {"XG_ENGINE_MAX_STEP": 0} if engine == "per-step launches" else {}
    cx = _ctx_env(xg, **env)
    try:
        shift, in_engine = 0, 0
        for method in RAGGED_METHODS:
            s = xg.Schedule(method, P, A, 0, 3, rl, lens=lens)
            assert s.ragged
            with pytest.raises(xg.XGError, match="ragged"):
                xg.MethodRun(cx, s)                                   # the fingerprint fill knows one d
            rb = s.devplan(1, 0).region_bytes
            assert rb[0] == sum(lens) == rb[1]
            cal = Caller(xg, cx, rb[0], rb[1], seed=300 + method)
            try:
                reg = xg.Regions.adopt(cx, rb, send=cal.send, recv=cal.recv)
                run = xg.MethodRun(cx, s, regions=reg, fill=False)
                try:
                    cal.image[cal.recv_off:cal.recv_off + rb[1]] = 0xA5
                    shift += run.shift_launches()
                    in_engine += run.engine_steps()[0]
                    if engine == "per-step launches":
                        assert run.engine_workgroups == 0 and run.shift_launches() >= 1
                    run.run_timed()
                    _deliver_v(cal.image, cal, s)
                    got = cal.read()
                    diff = np.flatnonzero(got != cal.image)
                    assert diff.size == 0, (method, "first differing arena byte", int(diff[0]), cal.send_off, cal.recv_off)
                    assert xg.payload_check(run) == []
                    recv = cal.image[cal.recv_off:cal.recv_off + rb[1]]
                    dl, dn = s.deliveries(1), s.delivery_lens(1)
                    assert run.slot_chk() == [O.chk64(recv[q.recv_off:q.recv_off + n]) for q, n in zip(dl, dn)]
                    # the last byte of the longest slot: inside the span only because the span has its length
                    k = max(range(len(dl)), key=lambda i: dn[i])
                    at = dl[k].recv_off + dn[k] - 1
                    _write(run, xg.BUF_RECV, at, _read(run, xg.BUF_RECV, at, 1) ^ np.uint8(0x40))
                    assert xg.payload_check(run) == [(dl[k].dst, dl[k].slot)], method
                finally:
                    run.close()
                reg.close()
            finally:
                cal.close()
        if engine == "per-step launches":
            assert in_engine == 0 and shift >= len(RAGGED_METHODS)
        else:
            assert in_engine > 0, "no engine segment carried a ragged step"
    finally:
        cx.close()


@pytest.fixture(scope="module")
def ctx(xg):
    c = xg.Context(rank=0, nranks=1, device=0)
    yield c
    c.close()


@pytest.mark.parametrize("method", [1, 2, 5, 9])
def test_exchange_v_on_one_gpu(xg, ctx, method):
    """xg_exchange_v (verify on) over a caller's buffers: 0, no bad slot, a timer per rank, the
    arena equals the numpy delivery; a uniform matrix runs as xg_exchange does; a negative entry is
    XG_ESCHED with the builder's words"""
    lens = _ragged_lens()
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, 3, rl, lens=lens)
    rb = s.devplan(1, 0).region_bytes
    cal = Caller(xg, ctx, rb[0], rb[1], seed=500 + method)
    try:
        rc, bad, timers, err = xg.exchange_v(ctx, method, P, A, lens, rl, 3, cal.send, cal.recv)
        assert (rc, bad, err) == (0, 0, "")
        assert len(timers) == P and all(t.total_time > 0 for t in timers)
        _deliver_v(cal.image, cal, s)
        diff = np.flatnonzero(cal.read() != cal.image)
        assert diff.size == 0, (method, "first differing arena byte", int(diff[0]))
        assert xg.exchange_v(ctx, method, P, A, [64] * (P * A), rl, 3, cal.send, None)[:2] == (0, 0)
        neg = list(lens)
        neg[3] = -5
        rc, _bad, _t, err = xg.exchange_v(ctx, method, P, A, neg, rl, 3, cal.send, cal.recv)
        assert rc != 0 and "negative length" in err
    finally:
        cal.close()


# ------------------------------------------------------------------ 3. virtual jobs
@pytest.fixture(scope="module")
def worlds(xg):
    w = {G: [xg.Context.virtual(g, G, device=0) for g in range(G)] for G in (2, 3)}
    yield w
    for ctxs in w.values():
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("method", [1, 5, 9, 11])
def test_ragged_virtual_jobs(xg, worlds, G, method):
    """the same ragged shape as a G-GPU job on this device, direct, one-sided and two-sided (packs
    and unpacks at every phase: copy_kernel_s on both sides of the staging buffers), a random
    payload per GPU: payload_check is empty on every GPU; once more through RCCL"""
    s = xg.Schedule(method, P, A, 0, 3, xg.aggregator_list(P, A), lens=_ragged_lens())
    for pack, form in PACKINGS:
        _virtual_job(xg, worlds[G], s, pack, form, rccl=False, corrupt=False)
    _virtual_job(xg, worlds[G], s, 1 << 30, 0, rccl=True, corrupt=False)


# ------------------------------------------------------------------ 4. real 2-rank jobs
def _ragged_job(tmp_path, case, timeout=100):
    """two ragged_worker.py processes over one RCCL communicator, started as test_gpu_multirank
    starts its jobs (XG_SHARE_GPU=1, one hardware queue per rank), each under a timeout of its
    own; -> every rank's result line"""
    from test_gpu_multirank import _env, _spawn, _wait_all
    import os
    G = 2
    tmp_path = pathlib.Path(tempfile.mkdtemp(prefix="job", dir=str(tmp_path)))
    worker = os.path.join(REPO, "tests", "ragged_worker.py")
    procs = [_spawn(["timeout", "-k", "10", str(timeout - 5), sys.executable, "-u", worker, json.dumps(case)],
                    _env(tmp_path, RANK=r, WORLD_SIZE=G, LOCAL_RANK=r, XG_MR_DEADLINE=timeout - 15), None,
                    "rank%d" % r, tmp_path)
             for r in range(G)]
    outs = _wait_all(procs, timeout)
    failed = ["rank %d exit %d: %s" % (r, p.returncode, " | ".join(err.strip().splitlines()[-3:]))
              for r, ((p, _o, _e), (out, err)) in enumerate(zip(procs, outs)) if p.returncode]
    assert not failed, "\n".join(failed)
    rows = [json.loads([x for x in out.splitlines() if x.startswith("{")][-1]) for out, _err in outs]
    assert [r["rank"] for r in rows] == list(range(G))
    return rows


def test_exchange_v_as_two_rank_job(tmp_path):
    """xg_exchange_v (m1, verify on) between two real ranks: both return 0 with 0 bad slots, and
    each rank's whole RECV equals the numpy delivery of both ranks' payloads"""
    rows = _ragged_job(tmp_path, {"method": 1, "P": P, "A": A, "c": 3, "lens": _ragged_lens()})
    for r in rows:
        assert (r["rc"], r["bad"], r["err"], r["exact"]) == (0, 0, "", True), r
        assert r["timers"] == P // 2


def test_exchange_v_refuses_mismatched_matrices(tmp_path):
    """two ranks whose matrices differ in one entry: XG_EARG on both, before the exchange posts
    anything (the matrix is part of what the ranks compare first)"""
    rows = _ragged_job(tmp_path, {"method": 1, "P": P, "A": A, "c": 3, "lens": _ragged_lens(),
                                  "perturb": {"1": [9, 1]}})
    for r in rows:
        assert r["rc"] == 3 and "different inputs" in r["err"], r
        assert r["bad"] == 0 and r["exact"] is None
