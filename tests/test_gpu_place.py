"""GPU: placement by offset-length lists -- copy_kernel_x (the extent copy of csrc/kernels.h), its
routing and tile tables (host/plan_tables.cc), and xg_exchange_w.

The kernel is driven through synthetic one-step plans with XG_DP_RAGGED | XG_DP_EXTENTS
(synth_plan's layout: seeded random SEND, poisoned RECV, a poisoned gap around every destination
unless the test packs them on purpose) and judged over EVERY byte of RECV against the in-order
numpy execution, so an overrun, a dropped store or a disturbed neighbour all show.  The read bound
(nothing outside the granules of a piece's first and last source byte) cannot be tested without
provoking a fault; it is argued from the code."""
import ctypes as C
import json
import os
import pathlib
import sys
import tempfile

import numpy as np
import pytest

from conftest import REPO
from place_cases import make_exts, payload, placed
from synth_plan import CHUNK_A, Synth, _assert_gaps, _compare, _ctx_env, _layout

pytestmark = pytest.mark.gpu

MEAN_MAX = 1024                 # kExtMeanMax (host/plan_tables.h): the routing threshold
PHASE_LENS = list(range(1, 50)) + [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


class ExtSynth(Synth):
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

    def counts(self):
        d = self.d
        return d.xg_plan_launches(self.p), d.xg_plan_extent_launches(self.p), d.xg_plan_shift_launches(self.p)

    def read_send(self):
        out = C.create_string_buffer(len(self.send))
        assert self.d.xg_regions_read(self.r, 0, 0, out, len(self.send)) == 0
        return np.frombuffer(out.raw, np.uint8)


def _flags(xg):
    return xg.DP_RAGGED | xg.DP_EXTENTS


def _run(xg, cx, steps, send_bytes, recv_bytes, seed, flags, want_counts=None):
    """load, check the launch counts (launches, extent launches, shift launches; None = any), run,
    compare every RECV byte with the numpy execution, SEND untouched"""
    sy = ExtSynth(xg, cx, send_bytes, recv_bytes, steps, seed=seed, flags=flags)
    try:
        assert xg.device().xg_plan_engine(sy.p) == 0
        got_counts = sy.counts()
        if want_counts is not None:
            for g, w in zip(got_counts, want_counts):
                assert w is None or g == w, (got_counts, want_counts)
            if want_counts[0] == len(steps):        # single-dispatch launches: every one has exactly one kind
                assert sum(xg.plan_kind_launches(sy.p)) == len(steps) - xg.plan_engine_segments(sy.p)
        want = sy.expected()
        got = sy.run()
        _compare(steps, got, want)
        assert np.array_equal(sy.read_send(), sy.send), "SEND was written"
        return got, got_counts
    finally:
        sy.close()


def _phase_specs():
    return [(n, sp, dp) for n in PHASE_LENS for sp in range(16) for dp in range(16)]


# ------------------------------------------------------------------ 1. phases x lengths
@pytest.mark.parametrize("variant", [0, 6])
def test_extent_copy_phases_and_lengths(xg, variant):
    """all 16 x 16 (source, destination) phase pairs at lengths 1..49, 63..65, 255..257, 1023..1025,
    4095..4097 (~4.5 MB) in ONE launch on copy_kernel_x, plain and non-temporal: every RECV byte
    equals the numpy execution, every gap keeps its poison"""
    specs = _phase_specs()
    copies, send_bytes, recv_bytes = _layout(specs)
    assert all((so % 16, do % 16) == (sp, dp) for (_a, so, _b, do, _n), (_m, sp, dp) in zip(copies, specs))
    assert sum(n for n, _s, _d in specs) <= MEAN_MAX * len(specs)
    steps = [copies]
    _assert_gaps(steps, recv_bytes)
    env = {"XG_ENGINE_MAX_STEP": 0}
    if variant:
        env["XG_COPY_VARIANT"] = variant
    cx = _ctx_env(xg, **env)
    try:
        _run(xg, cx, steps, send_bytes, recv_bytes, 20 + variant, _flags(xg), (1, 1, 0))
    finally:
        cx.close()


# ------------------------------------------------------------------ 2. shared cells
@pytest.mark.parametrize("sources", ["spaced", "packed"])
def test_extent_copy_neighbours_share_cells(xg, sources):
    """4000 pieces of seeded random length 1..40 back to back in the destination with no gap (most
    16-B cells belong to two or more pieces), sources spaced at random phases / back to back as
    well: every destination byte matches, the poison before the first piece and after the last is
    intact"""
    rng = np.random.default_rng(7)
    lens = [int(x) for x in rng.integers(1, 41, 4000)]
    copies, so, do = [], 5, 37
    for n in lens:
        if sources == "spaced":
            so = ((so + 15) & ~15) + 16 + int(rng.integers(0, 16))
        copies.append((0, so, 1, do, n))
        so += n
        do += n
    send_bytes, recv_bytes = ((so + 15) & ~15) + 16, ((do + 15) & ~15) + 48
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0)
    try:
        got, _ = _run(xg, cx, [copies], send_bytes, recv_bytes, 31, _flags(xg), (1, 1, 0))
        assert (got[:37] == 0xA5).all() and (got[do:] == 0xA5).all()
    finally:
        cx.close()


# ------------------------------------------------------------------ 3. tile and batch edges
def _rand_phase_specs(lens, seed):
    rng = np.random.default_rng(seed)
    return [(n, int(rng.integers(0, 16)), int(rng.integers(0, 16))) for n in lens]


def test_extent_copy_tile_edges(xg):
    """one launch each (a step each) of exactly 1, 63, 64, 65, 255, 256, 257 and 513 pieces of 16 B
    (the wave batches of the scan and the 256-piece tile cap); 40 pieces of 1000 B (tiles close by
    bytes, 32 KiB, before they close by count); one full-size piece (CHUNK_A, 32 KiB + 16 B: one
    piece by the pinned chunk, and longer than the tile's byte cap, so a tile of its own) in the
    middle of 16-B pieces; and zero-length copies interleaved"""
    groups = [[16] * n for n in (1, 63, 64, 65, 255, 256, 257, 513)]
    groups.append([1000] * 40)
    groups.append([16] * 60 + [CHUNK_A] + [16] * 60)
    groups.append([n for k in range(90) for n in (0, 17 + k % 5)] + [0])
    specs, cuts = [], [0]
    for gi, lens in enumerate(groups):
        specs += _rand_phase_specs(lens, 100 + gi)
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[a:b] for a, b in zip(cuts, cuts[1:])]
    for lens in groups:
        assert sum(lens) <= MEAN_MAX * sum(1 for n in lens if n > 0)
    assert xg.extent_tiles([1000] * 40) == [0, 32, 40]
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_STEP_CHAIN=0)
    try:
        cx.set_copy_params(CHUNK_A, -1)
        assert xg.piece_size(groups[9], CHUNK_A, cx.info()[1], 2048) == CHUNK_A
        _run(xg, cx, steps, send_bytes, recv_bytes, 41, _flags(xg), (len(steps), len(steps), 0))
    finally:
        cx.close()


def test_extent_copy_in_a_chain(xg):
    """the same kind of steps as a chain of stamped launches (the default): copy_kernel_x stamps its
    start like the other copy kernels, step times ascend"""
    groups = [[16] * 300, [40] * 500, [250] * 100]
    specs, cuts = [], [0]
    for gi, lens in enumerate(groups):
        specs += _rand_phase_specs(lens, 200 + gi)
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[a:b] for a, b in zip(cuts, cuts[1:])]
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0)
    try:
        sy = ExtSynth(xg, cx, send_bytes, recv_bytes, steps, seed=43, flags=_flags(xg))
        try:
            assert sy.counts() == (3, 3, 0)
            assert sum(xg.plan_kind_launches(sy.p)) == len(steps) - xg.plan_engine_segments(sy.p)
            n = len(steps)
            done, post, wall = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
            assert sy.d.xg_plan_run(sy.p, done, post, C.byref(wall)) == 0
            assert all(0 < a <= b for a, b in zip(done, list(done)[1:])), list(done)
            _compare(steps, sy.run(), sy.expected())
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ 4. dispatch cuts
def test_extent_copy_dispatch_cuts(xg):
    """a ~1 MiB launch with XG_COPY_LAUNCH_MAX = 256 KiB goes as several dispatches of one
    copy_kernel_x launch: every dispatch's tiles cover exactly its pieces (every byte delivered
    once, nothing else written)"""
    rng = np.random.default_rng(9)
    specs = _rand_phase_specs([int(x) for x in rng.integers(1, 420, 5000)], 10)
    copies, send_bytes, recv_bytes = _layout(specs)
    assert 900 << 10 < sum(n for n, _s, _d in specs) < 1200 << 10
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_COPY_LAUNCH_MAX=256 << 10)
    try:
        _got, (launches, ext, shift) = _run(xg, cx, [copies], send_bytes, recv_bytes, 51, _flags(xg))
        assert launches >= 3 and (ext, shift) == (1, 0), (launches, ext, shift)
    finally:
        cx.close()


# ------------------------------------------------------------------ 5. routing
def _short_steps():
    copies, send_bytes, recv_bytes = _layout(_rand_phase_specs([16, 1, 33, 700, 64] * 200, 12))
    return [copies], send_bytes, recv_bytes


def test_extent_copy_off_is_the_shifted_copy(xg):
    """XG_EXTENT_COPY=0: no launch on copy_kernel_x, the launch runs copy_kernel_s, and RECV holds
    the identical bytes"""
    steps, send_bytes, recv_bytes = _short_steps()
    got = []
    for env, want in (({}, (1, 1, 0)), ({"XG_EXTENT_COPY": 0}, (1, 0, 1))):
        cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, **env)
        try:
            got.append(_run(xg, cx, steps, send_bytes, recv_bytes, 61, _flags(xg), want)[0])
        finally:
            cx.close()
    assert np.array_equal(got[0], got[1])


def test_extent_copy_routing_by_mean_length_and_flag(xg):
    """a launch whose mean length is above the threshold stays on copy_kernel_s (one byte above it,
    and one at it); the same short pieces in a plan with only XG_DP_RAGGED never reach
    copy_kernel_x: existing behaviour is untouched"""
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0)
    try:
        for lens, want in (([MEAN_MAX + 1] * 50 + [MEAN_MAX] * 49 + [MEAN_MAX + 49], (1, 0, 1)),
                           ([MEAN_MAX] * 100, (1, 1, 0)),
                           ([4096 + 7] * 30, (1, 0, 1))):
            copies, send_bytes, recv_bytes = _layout(_rand_phase_specs(lens, 13))
            _run(xg, cx, [copies], send_bytes, recv_bytes, 71, _flags(xg), want)
        steps, send_bytes, recv_bytes = _short_steps()
        _run(xg, cx, steps, send_bytes, recv_bytes, 72, xg.DP_RAGGED, (1, 0, 1))
        _run(xg, cx, steps, send_bytes, recv_bytes, 73, 0, (1, 0, 0))
    finally:
        cx.close()


# ------------------------------------------------------------------ 6. exchange_w on one GPU
P, A = 8, 3


@pytest.fixture(scope="module")
def ctx(xg):
    c = xg.Context(rank=0, nranks=1, device=0)
    yield c
    c.close()


def _np(raw):
    return np.frombuffer(raw, np.uint8)


@pytest.mark.parametrize("method", [1, 2, 3, 5])
def test_exchange_w_on_one_gpu(xg, ctx, method):
    """P 8, A 3, per pair 0..6 extents of 0..3000 B at seeded random non-overlapping domain offsets
    with gaps, verify on: rc 0, no bad slot, no bad extent; a2m (m1, m3): the whole domain buffer
    equals the numpy placement, every byte outside the extents keeps the caller's pattern, SEND is
    untouched; m2a (m2, m5): the whole dense RECV equals the numpy gather and the domain is
    untouched.  Then the placement step alone (PlaceRun): place_check finds nothing, and names
    exactly the extent whose placed byte was corrupted"""
    exts, dom = make_exts(P, A, seed=600 + method)
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, 3, rl, lens=xg.exts_lens(exts, P, A))
    a2m = s.direction == xg.A2M
    ndom = s.domain_bytes(1, 0, dom)
    ndense = s.region_bytes(1, 0, xg.BUF_SEND if a2m else xg.BUF_RECV)
    assert xg.exts_check(exts, P, A, dom, scatter=a2m) == (0, "")
    nsend, nrecv = (ndense, ndom) if a2m else (ndom, ndense)
    reg = xg.Regions(ctx, [nsend, nrecv, 0, 0, 0])
    try:
        src, preset = payload(0, nsend, salt=method), payload(1, nrecv, salt=method)
        reg.write(xg.BUF_SEND, 0, src.tobytes())
        reg.write(xg.BUF_RECV, 0, preset.tobytes())
        rc, bad, bad_e, place_s, timers, err = xg.exchange_w(ctx, method, P, A, exts, dom, rl, 3,
                                                             reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
        assert (rc, bad, bad_e, err) == (0, 0, 0, ""), (rc, bad, bad_e, err)
        assert place_s > 0 and len(timers) == P and all(t.total_time > 0 for t in timers)
        want = placed(s, 1, 0, exts, dom, lambda h: src, preset)
        got = _np(reg.read(xg.BUF_RECV, 0, nrecv))
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (method, "first differing byte of recv", int(diff[0]), len(diff))
        assert np.array_equal(_np(reg.read(xg.BUF_SEND, 0, nsend)), src), "send was written"
    finally:
        reg.close()
    # the placement step on its own, over a dense side of random bytes
    run = xg.PlaceRun(ctx, s, exts, dom)
    try:
        rb = run.view.region_bytes
        assert run.view.flags == xg.DP_RAGGED | xg.DP_EXTENTS and rb[2:] == [0, 0, 0]
        assert (rb[0], rb[1]) == ((ndense, ndom) if a2m else (ndom, ndense))
        side = payload(2, rb[0], salt=method)
        run.regions.write(xg.BUF_SEND, 0, side.tobytes())
        assert run.run() > 0
        assert xg.place_check(run) == []
        k = max(range(len(run.view.copies)), key=lambda i: run.view.copies[i][4])
        _sb, _so, _db, do, n = run.view.copies[k]
        at = do + n - 1
        byte = _np(run.regions.read(xg.BUF_RECV, at, 1))[0] ^ np.uint8(0x40)
        run.regions.write(xg.BUF_RECV, at, bytes([int(byte)]))
        assert xg.place_check(run) == [run.ext_index[k]]
    finally:
        run.close()


def test_exchange_w_refuses_a_bad_list(xg, ctx):
    """a scatter overlap, an extent past its domain and a rank out of range: XG_EARG with the
    checker's words, nothing run; the overlapping list is accepted for a collective read"""
    rl = xg.aggregator_list(P, A)
    dom = [4096] * A
    reg = xg.Regions(ctx, [8192, 3 * 4096, 0, 0, 0])
    try:
        for exts, word in (([(0, 0, 0, 100), (1, 0, 99, 10)], "overlap"),
                           ([(0, 1, 4000, 97)], "past the domain end"),
                           ([(P, 0, 0, 1)], "out of range")):
            rc, _b, _e, _t, _tm, err = xg.exchange_w(ctx, 1, P, A, exts, dom, rl, 3, reg.ptr(0), reg.ptr(1))
            assert rc == xg.EARG and word in err, (rc, err)
        rc, bad, bad_e, _t, _tm, err = xg.exchange_w(ctx, 2, P, A, [(0, 0, 0, 100), (1, 0, 99, 10)], dom, rl, 3,
                                                     reg.ptr(1), reg.ptr(0))
        assert (rc, bad, bad_e, err) == (0, 0, 0, "")
    finally:
        reg.close()


# ------------------------------------------------------------------ 7. two real ranks
def _place_job(tmp_path, case, timeout=100):
    """two place_worker.py processes over one RCCL communicator, started as test_gpu_multirank
    starts its jobs (XG_SHARE_GPU=1), each under a time limit of its own -> every rank's result lines"""
    from test_gpu_multirank import _env, _spawn, _wait_all
    G = 2
    tmp_path = pathlib.Path(tempfile.mkdtemp(prefix="job", dir=str(tmp_path)))
    worker = os.path.join(REPO, "tests", "place_worker.py")
    procs = [_spawn(["timeout", "-k", "10", str(timeout - 5), sys.executable, "-u", worker, json.dumps(case)],
                    _env(tmp_path, RANK=r, WORLD_SIZE=G, LOCAL_RANK=r, XG_MR_DEADLINE=timeout - 15), None,
                    "rank%d" % r, tmp_path)
             for r in range(G)]
    outs = _wait_all(procs, timeout)
    failed = ["rank %d exit %d: %s" % (r, p.returncode, " | ".join(err.strip().splitlines()[-3:]))
              for r, ((p, _o, _e), (out, err)) in enumerate(zip(procs, outs)) if p.returncode]
    assert not failed, "\n".join(failed)
    rows = [[json.loads(x) for x in out.splitlines() if x.startswith("{")] for out, _err in outs]
    assert [r[0]["rank"] for r in rows] == list(range(G))
    return rows


@pytest.mark.parametrize("method", [1, 2])
def test_exchange_w_as_two_rank_job(tmp_path, method):
    """the shape of the one-GPU test between two real ranks: both return 0 with no bad slot and no
    bad extent, and each rank's whole destination (a2m: its domain buffer, m2a: its dense RECV)
    equals the numpy execution over both ranks' payloads.  Then a call where rank 1's list differs
    by one offset, and a call with a scatter overlap: both ranks return XG_EARG with their own
    messages and the job ends normally"""
    rows = _place_job(tmp_path, {"method": method, "P": P, "A": A, "c": 3, "seed": 700 + method})
    for r in rows:
        good, differ, overlap = r
        assert (good["rc"], good["bad"], good["bad_exts"], good["err"], good["exact"]) == (0, 0, 0, "", True), good
        assert differ["rc"] == 3 and "different inputs" in differ["err"], differ
        if method == 1:
            assert overlap["rc"] == 3 and ("overlap" in overlap["err"] or "another GPU" in overlap["err"]), overlap
        else:
            assert overlap["rc"] == 0, overlap            # a gather may read a byte twice
    if method == 1:
        assert any("overlap" in r[2]["err"] for r in rows)
