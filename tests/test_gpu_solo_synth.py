"""GPU: the two persistent step engines at their own edges, under synthetic plans.

solo_engine_kernel<K, WV, G> (the rails) and step_engine_kernel<B> (the grid barrier) otherwise
run only under the methods' schedules: one uniform -d per plan and regular step shapes.  Here the
plans are built copy by copy (synth_plan.py): SEND -> RECV copies whose destinations are each
written once in the whole plan and stand between poisoned gaps of >= 16 B, so a piece stored a
granule too long, a row stored twice or a rail that moves nothing shows in the RECV image, which
is compared WHOLE with the numpy in-order execution (Synth.expected).  RECV is poisoned again
before every run, so a run cannot pass on the bytes of the one before.  Every test asserts its
routing as well -- the rail count, the segment count, units above workgroups -- since the bytes
alone would also be right on the other engine, and the step stamps of every run (ordered, inside
the wall time: a rail with nothing in a step carries its previous stamp, xg_solo_reduce_stamps).

Which engine a segment takes is decided at plan load by a cost model (plan_tables.cc solo_pays);
synth_plan._solo_pays mirrors it only to SIZE the plans -- steps that move nothing are added until
the model prefers rails -- and the asserted rail count is the check that it did.  What the plans
are (granules, row counts, flags) is checked without a GPU in test_synth_plan.py.
"""
import ctypes as C

import numpy as np
import pytest

from synth_plan import (GRANULE_CTX, K, SBASE, DBASE, UNIT64, Synth, _assert_gaps, _capacity_steps, _compare,
                        _ctx_env, _granule_steps, _pieces, _rails, _round_steps, _row_pieces, _row_steps, _segment,
                        _sized, _spans, _tables, _unit64_steps)

pytestmark = pytest.mark.gpu


def _check_plan(steps, send_bytes, recv_bytes):
    """the common rules of the solo plans"""
    assert all(sb == 0 and db == 1 for st in steps for (sb, _so, db, _do, _n) in st)     # SEND -> RECV only
    _assert_gaps(steps, recv_bytes)     # >= 16 poisoned bytes on both sides, so every destination written once
    assert recv_bytes < 8 << 20 and send_bytes < 8 << 20


def _engine_steps(xg, sy):
    ns, nh = C.c_int(), C.c_int()
    n = xg.device().xg_plan_engine_steps(sy.p, C.byref(ns), C.byref(nh))
    return n, ns.value, nh.value


def _run3(sy, steps, runs=3):
    """`runs` runs from a poisoned RECV each: the whole image against numpy, the stamps ordered"""
    want = sy.expected()
    for rep in range(runs):
        sy.poison()
        got, done, wall = sy.run_timed()
        _compare(steps, got, want)
        assert len(done) == len(steps)
        assert all(0 <= a <= b for a, b in zip(done, done[1:])), (rep, done)
        assert done[-1] <= wall + 1e-4, (rep, done[-1], wall)


def _solo_env(waves, rails, arm):
    env = {"XG_ENGINE_ARM": arm}
    if waves != 1:
        env["XG_SOLO_WAVES"] = waves
    if rails:
        env["XG_SOLO_RAILS"] = rails
    return env


# ------------------------------------------------------------------ (a) lengths and granules
@pytest.mark.parametrize("arm", [1, 0])
@pytest.mark.parametrize("G,waves,rails", GRANULE_CTX)
def test_solo_lengths_and_granules(xg, G, waves, rails, arm):
    """solo_engine_kernel<8, 1, 16>, <8, 1, 4>, <4, 1, 1> and <8, 16, 16> on 1, a few and the
    default number of rails (rails = 0: XG_SOLO_RAILS unset), launched in the timed region or
    armed; lengths that end inside, at and past a 64-lane access (synth_plan.SOLO_LENS), empty
    steps at both ends and inside, runs of one-copy steps, steps of 5-40 copies.  A plan is armed
    only when ONE segment covers all its steps, and build_segments trims the steps that move
    nothing off a segment's ends, so under XG_ENGINE_ARM=1 the plan runs twice: as stated
    (a launched segment between steps that do nothing) and without those end steps (the doorbell
    path).  The one-rail and fine-granule plans hold more than 24 steps: the cost model takes
    one 15 GB/s rail only for < 445 x steps x G bytes, so steps that move nothing are added in
    the middle (up to 180 steps for G = 1 on one rail)."""
    rails_max = rails or (512 if waves == 1 else 16)
    steps, send_bytes, recv_bytes = _sized(lambda pad: _granule_steps(G, pad), rails_max, waves, G)
    _check_plan(steps, send_bytes, recv_bytes)
    want_rails = _rails(steps, rails_max, waves)
    if rails:
        assert want_rails == rails          # enough pieces to fill the rails asked for
    cx = _ctx_env(xg, **_solo_env(waves, rails, arm))
    try:
        for plan in ([steps, _segment(steps)] if arm else [steps]):
            sy = Synth(xg, cx, send_bytes, recv_bytes, plan, seed=G + waves)
            try:
                d = xg.device()
                assert d.xg_plan_engine_rails(sy.p) == want_rails, (d.xg_plan_engine_rails(sy.p), want_rails)
                assert d.xg_plan_engine(sy.p) == want_rails
                assert _engine_steps(xg, sy) == (len(_segment(steps)), 1, 0)
                _run3(sy, plan)
            finally:
                sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ (b) row and chunk edges
@pytest.mark.parametrize("arm", [1, 0])
@pytest.mark.parametrize("rows", [1, K, K + 1, 2 * K, 2 * K + 1, 3 * K + 1])
@pytest.mark.parametrize("waves", [16, 1])
def test_solo_row_and_chunk_edges(xg, waves, rows, arm):
    """ONE rail whose table holds exactly `rows` real rows (a row = one piece per wave): the
    double-buffer loop of solo_engine_kernel stores ceil(rows / K) chunks, leaving by its
    `break` after an odd number of them (1, K, 2K + 1 rows) and by its loop condition after an
    even number (K + 1, 2K, 3K + 1), and solo_store stops inside a chunk at the first padding
    row.  The row count is confirmed from the tables the host builds for the same steps
    (xg.solo_tables); on a 16-wave rail the last row is partly filled (full for rows = 1) and
    a stretch of one-piece steps puts >= 8 step barriers into one row."""
    npieces = _row_pieces(rows, waves)
    steps, send_bytes, recv_bytes = _sized(lambda pad: _row_steps(npieces, waves, pad), 1, waves, 16)
    _check_plan(steps, send_bytes, recv_bytes)
    shape, close, real = _tables(xg, steps, 1, waves, 16)
    assert shape["rails"] == 1 and real == [rows], (shape, real)
    assert shape["nrows"] >= ((rows + K - 1) // K + 1) * K           # the spare chunk the loop loads unasked
    if waves == 16:
        assert max(close[0]) >= 8, close[0]
    cx = _ctx_env(xg, **_solo_env(waves, 1, arm))
    try:
        sy = Synth(xg, cx, send_bytes, recv_bytes, steps, seed=rows)
        try:
            d = xg.device()
            assert d.xg_plan_engine(sy.p) == 1 and d.xg_plan_engine_rails(sy.p) == 1
            assert _engine_steps(xg, sy) == (len(_segment(steps)), 1, 0)
            _run3(sy, steps)
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ (c) pieces-per-rail capacity
@pytest.mark.parametrize("rails,per_step", [(1, 150), (2, 240)])
def test_solo_splits_at_the_piece_capacity(xg, rails, per_step):
    """40 steps of `per_step` copies of 16-48 B: more pieces per rail than one launch's tables hold
    (rows_cap = 4608 - 3 * 8 per one-wave rail), far below the step and byte caps -- solo_split
    cuts the run into consecutive solo launches at a step boundary."""
    steps, send_bytes, recv_bytes = _capacity_steps(per_step)
    _check_plan(steps, send_bytes, recv_bytes)
    assert _pieces(steps) > rails * (4608 - 3 * K)
    rc, shape, *_ = xg.solo_tables(_spans(steps), rails, SBASE, DBASE, waves=1)
    assert rc == 3 and shape["npieces"] > 4608                       # one table cannot hold it
    cx = _ctx_env(xg, XG_SOLO_RAILS=rails, XG_ENGINE_ARM=0)
    try:
        sy = Synth(xg, cx, send_bytes, recv_bytes, steps, seed=rails)
        try:
            n_eng, nseg, nhaz = _engine_steps(xg, sy)
            assert n_eng == 40 and nseg >= 2 and nhaz == 0, (n_eng, nseg, nhaz)
            assert xg.device().xg_plan_engine_rails(sy.p) == rails
            _run3(sy, steps)
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ the grid engine
@pytest.mark.parametrize("reader", [False, True])
def test_grid_engine_rounds(xg, reader):
    """step_engine_kernel<1> with 700 units per step on (at most) 256 workgroups: every workgroup
    takes a second and a third round of its `i += W` loop, continuing behind the unit it loaded
    while the barrier was pending, or -- where that unit is off the 16-B grid -- from the step's
    first unit.  Three SEND -> RECV steps in a row (flags 0, 0, 1); the variant puts a step that
    reads step 0's output between them (flag 2 after step 0: drain, release / acquire, no early
    load)."""
    per = 700
    steps, send_bytes, recv_bytes = _round_steps(4 if reader else 3, per, reader)
    _assert_gaps(steps, recv_bytes)
    assert recv_bytes < 8 << 20 and max(sum(c[4] for c in st) for st in steps) <= 1 << 20     # B = 1: 4 KiB units
    base = {0: 1 << 40, 1: 2 << 40}
    flags, nhaz = xg.engine_hazards([[(base[sb] + so, base[db] + do, n) for (sb, so, db, do, n) in st] for st in steps])
    assert (flags, nhaz) == (([2, 0, 0, 1], 1) if reader else ([0, 0, 1], 0))
    cx = _ctx_env(xg, XG_ENGINE_SOLO=0)
    try:
        sy = Synth(xg, cx, send_bytes, recv_bytes, steps, seed=5)
        try:
            d = xg.device()
            W = d.xg_plan_engine(sy.p)
            assert W > 0 and d.xg_plan_engine_rails(sy.p) == 0
            assert all(len(st) > W and len(st) >= 2.5 * W for st in steps), (per, W)
            assert _engine_steps(xg, sy) == (len(steps), 1, nhaz)
            # among the units a workgroup prefetches (the first W of steps 1..) some are off the grid
            for st in steps[1:]:
                off = [((so | do | n) & 15) != 0 for (_sb, so, _db, do, n) in st[:W]]
                assert any(off) and not all(off)
            _run3(sy, steps)
        finally:
            sy.close()
    finally:
        cx.close()


def test_grid_engine_64k_units(xg):
    """step_engine_kernel<16> (a step above 4 MiB: 64 KiB units, 16 loads per lane in flight):
    transfers of unit - 16, unit, unit + 16 and 3 * unit + 4080 bytes -- a last unit 16 B short
    of full, exactly full, of 16 B, of 4080 B -- transfers of a few KiB at odd phases, and a
    step that moves nothing between two that do."""
    steps, send_bytes, recv_bytes = _unit64_steps()
    _assert_gaps(steps, recv_bytes)
    big = max(sum(c[4] for c in st) for st in steps)
    assert 4 << 20 < big < (4 << 20) + (256 << 10) and recv_bytes < 8 << 20 and send_bytes < 8 << 20
    assert any(not st for st in steps[1:-1])
    cx = _ctx_env(xg, XG_ENGINE_SOLO=0)
    try:
        sy = Synth(xg, cx, send_bytes, recv_bytes, steps, seed=16)
        try:
            d = xg.device()
            units = max(sum(-(-c[4] // UNIT64) for c in st) for st in steps)
            assert d.xg_plan_engine(sy.p) == units and d.xg_plan_engine_rails(sy.p) == 0      # a workgroup per unit
            assert _engine_steps(xg, sy) == (len(steps), 1, 0)
            _run3(sy, steps)
        finally:
            sy.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ write-after-read keeps off the rails
def test_write_after_read_runs_on_the_grid_engine(xg):
    """Step 0 copies RECV[X] on to RECV[Y], step 1 overwrites RECV[X] from SEND: no hazard flag
    (the grid barrier orders a write after a read) -- and on rails, which never wait for each
    other, a rail already in step 1 could overwrite X before another has loaded it for step 0.
    The segment must take the grid engine (xg_engine_rail_safe); X is rewritten with fresh known
    bytes before each of 5 runs, the whole RECV image compared."""
    L = 64 << 10
    X, Y = 64, 64 + L + 64
    recv_bytes = Y + L + 64
    steps = [[(1, X, 1, Y, L)], [(0, 0, 1, X, L)]]
    _assert_gaps(steps, recv_bytes)
    cx = xg.Context(rank=0, nranks=1, device=0)
    try:
        sy = Synth(xg, cx, L, recv_bytes, steps, seed=3)
        try:
            d = xg.device()
            assert d.xg_plan_engine(sy.p) > 0
            assert _engine_steps(xg, sy) == (2, 1, 0)
            assert d.xg_plan_engine_rails(sy.p) == 0, "a write-after-read segment on unsynchronised rails"
            rng = np.random.default_rng(11)
            for _rep in range(5):
                image = np.full(recv_bytes, 0xA5, np.uint8)
                image[X:X + L] = rng.integers(0, 256, L, dtype=np.uint8)
                sy.write_recv(image)
                got, done, wall = sy.run_timed()
                _compare(steps, got, sy.expected(image))
                assert 0 <= done[0] <= done[1] <= wall + 1e-4
        finally:
            sy.close()
    finally:
        cx.close()
