"""GPU: copy_kernel_q, the small-piece copy of large uniform launches (csrc/kernels.h), and its
routing (xg_copy_launch_choose in csrc/host/pieces.c, called by TableBuilder::open).

The kernel is driven through synthetic one-GPU plans (synth_plan: seeded random SEND, poisoned
RECV, sources laid out against the destinations' order, a poisoned gap of >= 16 B around every
destination) with XG_SMALL_PIECE_MIN=0, so launches of a few KiB take the form the 448 MiB launches
of bench.py take by default, and judged bit for bit over the whole RECV region against the in-order
numpy execution: an overrun into a gap, a dropped tail and a piece at the wrong offset all show.
Every test moves under 64 MiB (which is why the 1 MiB copies come 1, 2 and 7 to a launch, not 449).
"""
import ctypes as C

import numpy as np
import pytest

from synth_plan import Synth, _assert_gaps, _compare, _ctx_env, _layout

pytestmark = pytest.mark.gpu

NEVER = 1 << 40
LENS = [16, 4080, 4096, 4112, 8208, 3 * 4096, 5 * 4096 + 48, 1 << 20]
COPIES = [1, 2, 7, 449]
ENV = dict(XG_SMALL_PIECE_MIN=0, XG_SMALL_PIECE_KIB=8, XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=NEVER)


def _uniform_steps(shapes):
    """one step (= one launch) per (length, copies): `copies` aligned copies of `length` bytes"""
    specs, cuts = [], [0]
    for n, k in shapes:
        specs += [(n, 0, 0)] * k
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[a:b] for a, b in zip(cuts, cuts[1:])]
    assert sum(n * k for n, k in shapes) < 64 << 20
    _assert_gaps(steps, recv_bytes)
    # sources run against the destinations: the launch's rows are in destination order, not source order
    assert all(a[1] > b[1] for st in steps for a, b in zip(st, st[1:]))
    return steps, send_bytes, recv_bytes


def _small(xg, sy):
    kib = C.c_int(-1)
    return xg.device().xg_plan_small_launches(sy.p, C.byref(kib)), kib.value


def _run(xg, env, steps, send_bytes, recv_bytes, want_small, kib=None, seed=3, launches=None):
    cx = _ctx_env(xg, **env)
    try:
        sy = Synth(xg, cx, send_bytes, recv_bytes, steps, seed=seed)
        try:
            d = xg.device()
            assert d.xg_plan_engine(sy.p) == 0
            assert _small(xg, sy) == (want_small, (kib or 0) if want_small else 0)
            if launches is not None:
                assert d.xg_plan_launches(sy.p) == launches
                if launches == len(steps):          # single-dispatch launches: every one has exactly one kind
                    assert sum(xg.plan_kind_launches(sy.p)) == launches - xg.plan_engine_segments(sy.p)
            want = sy.expected()
            got = sy.run()
            _compare(steps, got, want)                      # RECV over its whole length, gaps still 0xA5
            _compare(steps, sy.run(), want)                 # and again: a second run writes the same bytes
            return got
        finally:
            sy.close()
    finally:
        cx.close()


ALL_SHAPES = [(n, k) for n in LENS for k in COPIES if n * k < 16 << 20]


@pytest.mark.parametrize("order", [1, 8, 32])
@pytest.mark.parametrize("variant", [1, 6])
@pytest.mark.parametrize("kib", [4, 8])
def test_lengths_and_copy_counts(xg, kib, variant, order):
    """copy_kernel_q<1 | 2, plain | NT> over every length (one piece short of, at and past the piece
    sizes, several pieces with a 48-B tail, 1 MiB) x 1, 2, 7 and 449 copies, one launch per step:
    every launch takes the small form and RECV is the numpy execution bit for bit; in plain
    destination order (1) and in groups of 8 (the default) and 32 copies, whose last group is short
    for 1, 2, 7 and 449 copies"""
    steps, sb, rb = _uniform_steps(ALL_SHAPES)
    env = dict(ENV, XG_SMALL_PIECE_KIB=kib, XG_COPY_VARIANT=variant, XG_SMALL_PIECE_ORDER=order)
    _run(xg, env, steps, sb, rb, len(steps), kib, seed=kib + variant, launches=len(steps))


@pytest.mark.parametrize("kib", [4, 8])
def test_beside_the_step_engine(xg, kib):
    """with the step engine on (its default), small-form steps stay launches of their own: none of
    them joins an engine segment, where its rows would never be copied"""
    steps, sb, rb = _uniform_steps([(4112, 7), (8208, 2), (16, 449), (5 * 4096 + 48, 7)])
    env = {k: v for k, v in ENV.items() if k != "XG_ENGINE_MAX_STEP"}
    _run(xg, dict(env, XG_SMALL_PIECE_KIB=kib), steps, sb, rb, len(steps), kib, launches=len(steps))


@pytest.mark.parametrize("variant", [1, 6])
@pytest.mark.parametrize("kib", [4, 8])
def test_dispatches_cut_inside_a_copy(xg, kib, variant):
    """XG_COPY_LAUNCH_MAX = 20 KiB: dispatches of 5 (4 KiB pieces) or 2 (8 KiB) workgroups against
    copies of 6 or 3 pieces, so the cuts fall inside copies and each dispatch starts at a base
    workgroup; 449 copies of 4112 B (two pieces each, the second 16 B) likewise"""
    shapes = [(5 * 4096 + 48, 7), (4112, 449), (3 * 4096, 14)]
    steps, sb, rb = _uniform_steps(shapes)
    cx_env = dict(ENV, XG_SMALL_PIECE_KIB=kib, XG_COPY_VARIANT=variant, XG_COPY_LAUNCH_MAX=20480)
    piece, per = kib << 10, 20480 // (kib << 10)
    want, inside = 0, False
    for n, k in shapes:              # the cut rule of cut_small: no runt of < 16 workgroups or < half a dispatch
        W = k * -(-n // piece)
        cuts = [o for o in range(per, W, per)]
        keep = 0
        for o in cuts:
            if (W - o) * piece < 10240 or W - o < 16:
                break
            keep += 1
        assert keep >= 2                                                       # really cut
        inside = inside or any(o % -(-n // piece) for o in cuts[:keep])
        want += keep + 1
    assert inside                                                              # ... somewhere inside a copy
    _run(xg, cx_env, steps, sb, rb, len(steps), kib, launches=want)


@pytest.mark.parametrize("kib", [4, 8])
def test_zero_length_copies_among_the_uniform(xg, kib):
    """empty copies in a launch do not break its uniformity and get no row"""
    specs = []
    for i in range(23):
        specs += [(8208, 0, 0)] + ([(0, 0, 0)] if i % 3 == 0 else [])
    specs = [(0, 0, 0)] + specs + [(0, 0, 0)]
    copies, sb, rb = _layout(specs)
    steps = [copies]
    _assert_gaps(steps, rb)
    _run(xg, dict(ENV, XG_SMALL_PIECE_KIB=kib), steps, sb, rb, 1, kib)


@pytest.mark.parametrize("variant", [1, 6])
def test_other_launches_keep_their_kernels(xg, variant):
    """a launch of mixed lengths and a launch with one copy at offset 8 are not small-form launches
    (counter 0) and deliver the right bytes on today's kernels; the uniform launch between them is"""
    mixed = [(4096, 0, 0)] * 5 + [(4112, 0, 0)] + [(4096, 0, 0)] * 5
    uniform = [(4096, 0, 0)] * 11
    off8 = [(4096, 0, 0)] * 5 + [(4096, 8, 8)] + [(4096, 0, 0)] * 5
    copies, sb, rb = _layout(mixed + uniform + off8)
    steps = [copies[:11], copies[11:22], copies[22:]]
    _assert_gaps(steps, rb)
    assert copies[27][1] % 16 == 8 and copies[27][3] % 16 == 8
    env = dict(ENV, XG_COPY_VARIANT=variant)
    _run(xg, env, steps, sb, rb, 1, 8, launches=3)
    _run(xg, env, [steps[0], steps[2]], sb, rb, 0, launches=2)


def test_small_pieces_off(xg):
    """XG_SMALL_PIECES=0: no launch takes the small form and the bytes are the same"""
    steps, sb, rb = _uniform_steps([(4112, 7), (5 * 4096 + 48, 449), (1 << 20, 2)])
    on = _run(xg, ENV, steps, sb, rb, len(steps), 8)
    off = _run(xg, dict(ENV, XG_SMALL_PIECES=0), steps, sb, rb, 0)
    assert np.array_equal(on, off)


def test_default_threshold(xg):
    """without the test hook a launch below the 112 MiB threshold keeps its kernel"""
    steps, sb, rb = _uniform_steps([(1 << 20, 7)])
    env = {k: v for k, v in ENV.items() if k != "XG_SMALL_PIECE_MIN"}
    _run(xg, env, steps, sb, rb, 0)
