"""GPU: solo_engine_kernel's descriptors at the ends of their offset windows.

A solo piece is two offsets in granules from the segment's lowest source and destination: 24 bits
each beside the length and `before` in the packed form (16-wave rails), 32 bits each in the wide
form (one-wave rails, the length in the row's barrier word).  Everything else in the suite that
runs on rails stays below bit 18 of those fields; the plans here (sparse_synth.py) reach their
tops -- hulls of exactly 2^28 B packed and 2^32 B wide at granule 1, just over 8 and 32 GiB at
granules 4 and 16 (bit 31 of a granule offset, scaled by 4 and 16 in 64 bits) -- with 1 KiB
pieces, the length field's own top bit, behind step barriers, and split_steps goes one granule
past the window, where plan_tables.cc solo_split must cut the run and give each part bases of
its own.  The regions are address space: a few hundred KiB move.  SparseSynth judges every byte
of RECV all the same: the destinations with 4 KiB on both sides byte for byte against numpy, the
rest by device checksums of 1 MiB spans against the poison's, SEND by checksums before and
after; 3 runs from fresh poison, the stamps ordered.  The routing is asserted as in
test_gpu_solo_synth.py.  That a wrong mask, shift or 32-bit intermediate would fail this
comparison is shown on the CPU (test_solo_tables.py::test_window_plans_reject_a_broken_decode)."""
import ctypes as C

import pytest

from sparse_synth import FORMS, SparseSynth, bases, split_steps, window_plan
from synth_plan import _assert_gaps, _ctx_env, _rails, _segment

pytestmark = pytest.mark.gpu

CASES = ([("P", r, a) for r in (1, 3, 16) for a in (1, 0)] +
         [(fm, r, a) for fm in ("W1", "W4", "W16") for r in (1, 7, 0) for a in (1, 0)])


def _engine_steps(xg, sy):
    ns, nh = C.c_int(), C.c_int()
    n = xg.device().xg_plan_engine_steps(sy.p, C.byref(ns), C.byref(nh))
    return n, ns.value, nh.value


def _env(form, rails, arm):
    env = {"XG_ENGINE_ARM": arm}
    if FORMS[form]["waves"] != 1:
        env["XG_SOLO_WAVES"] = FORMS[form]["waves"]
    if rails:
        env["XG_SOLO_RAILS"] = rails
    return env


def _fits_hbm(cx, send_bytes, recv_bytes):
    _arch, _cus, hbm = cx.info()
    assert send_bytes + recv_bytes < hbm, (send_bytes, recv_bytes, hbm)


@pytest.mark.parametrize("form,rails,arm", CASES)
def test_solo_descriptors_at_the_window_ends(xg, form, rails, arm):
    """(P) solo_engine_kernel<8, 16, 16> on 1, 3 and 16 rails; (W1) <4, 1, 1>, (W4) <8, 1, 4> and
    (W16) <8, 1, 16> on 1, 7 and the default number of rails (rails = 0: XG_SOLO_RAILS unset);
    launched in the timed region (the plan as stated: its segment stands between steps that move
    nothing) or armed (the plan without those steps, one segment over all of it: the doorbell
    path; (P) armed runs the stated plan as well)."""
    waves = FORMS[form]["waves"]
    rails_max = rails or (512 if waves == 1 else 16)
    steps, send_bytes, recv_bytes = window_plan(form, rails_max)
    _assert_gaps(steps, recv_bytes)
    seg = _segment(steps)
    want_rails = _rails(steps, rails_max, waves)
    plans = [steps] if not arm else [steps, seg] if form == "P" else [seg]
    G, (slo, dlo) = FORMS[form]["G"], bases(steps)
    print("%s: %d rails, largest source / destination field 0x%x / 0x%x, %d B moved"
          % (form, want_rails, max(c[1] - slo for st in steps for c in st) // G,
             max(c[3] - dlo for st in steps for c in st) // G, sum(c[4] for st in steps for c in st)))
    cx = _ctx_env(xg, **_env(form, rails, arm))
    try:
        _fits_hbm(cx, send_bytes, recv_bytes)
        for plan in plans:
            sy = SparseSynth(xg, cx, send_bytes, recv_bytes, plan, seed=rails + 2 * arm)
            try:
                d = xg.device()
                assert d.xg_plan_engine_rails(sy.p) == want_rails, (d.xg_plan_engine_rails(sy.p), want_rails)
                assert d.xg_plan_engine(sy.p) == want_rails
                assert _engine_steps(xg, sy) == (len(seg), 1, 0)
                sy.run_checked()
            finally:
                sy.close()
    finally:
        cx.close()


@pytest.mark.parametrize("form", ["P", "W1"])
def test_solo_splits_at_the_offset_window(xg, form):
    """both hulls one granule wider than the descriptors' window, the low and the far copies in
    different steps: solo_split cuts the run into consecutive solo launches, and the second
    decodes against its own lowest source and destination, not the first's"""
    waves = FORMS[form]["waves"]
    rails_max = 512 if waves == 1 else 16
    steps, send_bytes, recv_bytes, cut = split_steps(form, "steps")
    _assert_gaps(steps, recv_bytes)
    first, second = bases(steps[:cut]), bases(steps[cut:])
    assert first[0] != second[0] and first[1] != second[1]
    cx = _ctx_env(xg, **_env(form, 0, 0))
    try:
        _fits_hbm(cx, send_bytes, recv_bytes)
        sy = SparseSynth(xg, cx, send_bytes, recv_bytes, steps, seed=7)
        try:
            n_eng, nseg, nhaz = _engine_steps(xg, sy)
            print("%s split: %d steps in %d segments, cut expected at step %d" % (form, n_eng, nseg, cut))
            assert n_eng == len(steps) and nseg >= 2 and nhaz == 0, (n_eng, nseg, nhaz)
            assert xg.device().xg_plan_engine_rails(sy.p) == _rails(steps[:cut], rails_max, waves) > 0
            sy.run_checked()
        finally:
            sy.close()
    finally:
        cx.close()


@pytest.mark.parametrize("form", ["P", "W1"])
def test_one_step_wider_than_the_window_keeps_off_the_rails(xg, form):
    """one step alone spans the window plus a granule on both sides: no cut between steps helps,
    the run must take another engine or the copy launches, and still deliver every byte"""
    steps, send_bytes, recv_bytes, _none = split_steps(form, "one_step")
    _assert_gaps(steps, recv_bytes)
    cx = _ctx_env(xg, **_env(form, 0, 0))
    try:
        _fits_hbm(cx, send_bytes, recv_bytes)
        sy = SparseSynth(xg, cx, send_bytes, recv_bytes, steps, seed=8)
        try:
            assert xg.device().xg_plan_engine_rails(sy.p) == 0
            sy.run_checked()
        finally:
            sy.close()
    finally:
        cx.close()
