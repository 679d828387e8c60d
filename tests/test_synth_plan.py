"""The host side of the copy-kernel edge tests (synth_plan.py, test_gpu_copy_edges.py): the
layouts keep what the GPU tests lean on, and a wrong receive region is reported with the copy
that holds the first differing byte -- checked here, where no GPU is needed, because a passing
GPU suite never runs the reporting path.  Likewise the plans of the step-engine tests
(test_gpu_solo_synth.py): their granules, row counts, table capacity and barrier flags."""
import numpy as np
import pytest

from sparse_synth import EDGE, FORMS, GUARD, SPAN, SparsePlan, split_steps, window_plan
from synth_plan import (DBASE, GRANULE_CTX, K, PHASE_PAIRS, SBASE, SOLO_LENS, UNIT64, WAVE_NP, _assert_gaps,
                        _capacity_steps, _compare, _granule_steps, _layout, _pieces, _rails, _round_steps, _row_pieces,
                        _row_steps, _segment, _sized, _spans, _tables, _unit64_steps, realign_edge_lens,
                        wave_edge_steps)


def _numpy_run(steps, send, recv_bytes):
    recv = np.full(recv_bytes, 0xA5, np.uint8)
    for st in steps:
        for (_sb, so, _db, do, n) in st:
            recv[do:do + n] = send[so:so + n]
    return recv


def test_layouts_keep_phases_gaps_and_disjoint_sources():
    specs = [(n, sp, dp) for (sp, dp) in PHASE_PAIRS for n in realign_edge_lens(dp)]
    for rev in (False, True):
        copies, send_bytes, recv_bytes = _layout(specs, reverse_sources=rev)
        _assert_gaps([copies], recv_bytes)
        assert send_bytes % 16 == 0 and recv_bytes % 16 == 0
        for (n, sp, dp), (sb, so, db, do, ln) in zip(specs, copies):
            assert (sb, db, ln, so % 16, do % 16) == (0, 1, n, sp, dp)
            assert so + ln <= send_bytes and do + ln <= recv_bytes
        src = sorted((so, so + n) for (_sb, so, _db, _do, n) in copies)
        assert all(b[0] >= a[1] for a, b in zip(src, src[1:]))
    with pytest.raises(AssertionError):
        _assert_gaps([[(0, 0, 1, 16, 32), (0, 0, 1, 63, 8)]], 128)       # a gap of 15 bytes


@pytest.mark.parametrize("kib", [2, 4, 8])
def test_wave_launches_have_the_intended_piece_counts(kib):
    steps, _send_bytes, recv_bytes = wave_edge_steps(kib)
    _assert_gaps(steps, recv_bytes)
    full = kib << 10
    assert [sum(-(-c[4] // full) for c in st) for st in steps] == WAVE_NP
    assert all((c[1] | c[3] | c[4]) % 16 == 0 for st in steps for c in st)
    # four waves of one workgroup, pieces dealt round-robin: the counts the kernel's loop sees
    per_wave = sorted({(n - 1 - w) // 4 + 1 for n in WAVE_NP for w in range(4) if w < n})
    assert per_wave == [1, 2, 63, 64, 65, 66, 129, 130]
    assert recv_bytes < 14 << 20


def test_compare_names_the_copy_of_the_first_wrong_byte():
    specs = [(100, 0, 0), (4099, 5, 12), (33, 15, 1)]
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[:1], copies[1:]]
    send = np.random.default_rng(0).integers(0, 256, send_bytes, dtype=np.uint8)
    want = _numpy_run(steps, send, recv_bytes)
    _compare(steps, want.copy(), want)                                   # equal: passes
    do = copies[1][3]
    for at, text in ((do + 4098, "byte 4098 of the copy of 4099 B, source phase 5, destination phase 12, step 1"),
                     (do + 4099, "in the gap 1 B from the copy of 4099 B"),      # an overrun by one byte
                     (copies[0][3] - 1, "in the gap 1 B from the copy of 100 B, source phase 0, destination phase 0, step 0"),
                     (copies[2][3], "byte 0 of the copy of 33 B, source phase 15, destination phase 1, step 1")):
        got = want.copy()
        got[at] ^= 0x01
        with pytest.raises(pytest.fail.Exception) as e:
            _compare(steps, got, want)
        assert text in str(e.value) and "RECV[%d]" % at in str(e.value), str(e.value)
    got = want.copy()                                                    # a store shifted by 16 bytes
    got[do + 16:do + 32] = want[do:do + 16]
    with pytest.raises(pytest.fail.Exception):
        _compare(steps, got, want)


# ------------------------------------------------------------------ step-engine plans (test_gpu_solo_synth.py)
@pytest.mark.parametrize("G,waves,rails", GRANULE_CTX)
def test_granule_plans_are_what_they_claim(xg, G, waves, rails):
    """each plan's granule is exactly G, it holds empty steps at both ends and inside, one-copy
    runs and 5-40-copy steps, every length of its set, SEND -> RECV copies between gaps, and
    pieces enough to fill the rails asked for"""
    rails_max = rails or (512 if waves == 1 else 16)
    steps, send_bytes, recv_bytes = _sized(lambda pad: _granule_steps(G, pad), rails_max, waves, G)
    _assert_gaps(steps, recv_bytes)
    assert all(sb == 0 and db == 1 for st in steps for (sb, _so, db, _do, _n) in st)
    bits = 0
    for st in steps:
        for (_sb, so, _db, do, n) in st:
            bits |= so | do | n
    assert bits % G == 0 and (G == 16 or bits % (4 * G) != 0)
    assert not steps[0] and not steps[-1] and any(not st for st in _segment(steps))
    sizes = sorted({len(st) for st in steps})
    assert sizes[:3] == [0, 1, 5] and sizes[-1] == 40
    ends = {n % (64 * G) for st in steps for (_sb, _so, _db, _do, n) in st}
    assert 0 in ends and G in ends and 64 * G - G in ends          # at, past and inside a 64-lane access
    assert set(SOLO_LENS[G]) == {n for st in steps for (_sb, _so, _db, _do, n) in st}
    shape, _close, _rows = _tables(xg, steps, rails_max, waves, G)
    assert shape["rails"] == _rails(steps, rails_max, waves) and (not rails or shape["rails"] == rails)
    assert len(steps) >= 24 and recv_bytes < 1 << 20


@pytest.mark.parametrize("waves", [16, 1])
def test_row_plans_fill_the_intended_rows(xg, waves):
    for rows in (1, K, K + 1, 2 * K, 2 * K + 1, 3 * K + 1):
        steps, _send_bytes, recv_bytes = _sized(lambda pad: _row_steps(_row_pieces(rows, waves), waves, pad), 1, waves, 16)
        _assert_gaps(steps, recv_bytes)
        shape, close, real = _tables(xg, steps, 1, waves, 16)
        assert shape["rails"] == 1 and real == [rows]
        assert waves == 1 or max(close[0]) >= 8                     # one row holds the ends of many steps


def test_capacity_and_grid_plans(xg):
    for rails, per_step in ((1, 150), (2, 240)):
        steps, _send_bytes, recv_bytes = _capacity_steps(per_step)
        _assert_gaps(steps, recv_bytes)
        assert _pieces(steps) > rails * (4608 - 3 * K)
        rc, shape, *_ = xg.solo_tables(_spans(steps), rails, SBASE, DBASE, waves=1)
        assert rc == 3 and shape["npieces"] > 4608
    base = {0: 1 << 40, 1: 2 << 40}
    for reader in (False, True):
        steps, _send_bytes, recv_bytes = _round_steps(4 if reader else 3, 700, reader)
        _assert_gaps(steps, recv_bytes)
        assert all(len(st) == 700 and max(c[4] for c in st) <= 4096 for st in steps)
        flags, nhaz = xg.engine_hazards([[(base[a] + so, base[b] + do, n) for (a, so, b, do, n) in st] for st in steps])
        assert (flags, nhaz) == (([2, 0, 0, 1], 1) if reader else ([0, 0, 1], 0))
    steps, _send_bytes, recv_bytes = _unit64_steps()
    _assert_gaps(steps, recv_bytes)
    assert {c[4] % UNIT64 for st in steps for c in st} >= {UNIT64 - 16, 0, 16, 4080}
    assert max(sum(c[4] for c in st) for st in steps) > 4 << 20 and recv_bytes < 8 << 20


# ------------------------------------------------------------------ window plans (test_gpu_solo_windows.py)
def _hulls(steps):
    cs = [c for st in steps for c in st]
    return (min(c[1] for c in cs), max(c[1] + c[4] for c in cs)), (min(c[3] for c in cs), max(c[3] + c[4] for c in cs))


@pytest.mark.parametrize("form", list(FORMS))
def test_window_plans_are_what_they_claim(form):
    """both hulls start EDGE bytes into their regions, end EDGE before their ends and are exactly
    the window (P, W1) or the smallest that sets bit 31 of a granule offset (W4, W16); the copies
    stand at the corners, the alternating patterns and every single high bit on each side alone;
    granule, lengths and phases are the form's; steps that move nothing stand at both ends"""
    f = FORMS[form]
    G = f["G"]
    for rails in (1, 3 if form == "P" else 7, 16 if form == "P" else 512):
        steps, send_bytes, recv_bytes = window_plan(form, rails)
        _assert_gaps(steps, recv_bytes)
        assert not steps[0] and not steps[-1] and all(_segment(steps)[i] for i in (0, -1))
        (slo, shi), (dlo, dhi) = _hulls(steps)
        hull = {"P": 1 << 28, "W1": 1 << 32, "W4": (1 << 33) + 1024, "W16": (1 << 35) + 1024}[form]
        assert (slo, shi, dlo, dhi) == (EDGE, EDGE + hull, EDGE, EDGE + hull)
        assert send_bytes == recv_bytes == hull + 2 * EDGE
        assert _rails(steps, rails, f["waves"]) == min(rails, _pieces(steps))     # the rails asked for are filled
        rel = [((so - EDGE) // G, (do - EDGE) // G, n) for st in steps for (_a, so, _b, do, n) in st]
        bits = 0
        for st in steps:
            for (_a, so, _b, do, n) in st:
                bits |= so | do | n
        assert bits % G == 0 and (G == 16 or bits % (4 * G) != 0)
        top, (p0, p1) = f["top"], f["pats"]
        pairs = {(s, d) for (s, d, _n) in rel}
        assert {(0, top), (top, 0), (p0, p1), (p1, p0)} <= pairs
        assert any(s == top and d > top - 2 * (1040 + G) // G for (s, d) in pairs - {(top, 0)})     # (top, top')
        assert any(s == 0 and 0 < d < 2 * (1040 + G) // G for (s, d) in pairs)                      # (0, 0')
        low = 1 << min(f["bits"])
        for b in list(f["bits"]) + ([31] if form in ("W4", "W16") else []):
            assert any(s == 1 << b and d < low for (s, d) in pairs) or (b == 31 and (1 << b, 0) in pairs)
            assert any(d == 1 << b and s < low for (s, d) in pairs) or (b == 31 and (0, 1 << b) in pairs)
        lens = {n for (_s, _d, n) in rel}
        assert lens >= set(f["lens"]) and (form != "W1" or lens >= {1023, 1024, 1025})
        if G < 16:                          # odd phases (multiples of G) on both sides
            assert all({x[side] * G % 16 for x in rel} >= ({1, 5, 15} if G == 1 else {4, 8, 12}) for side in (0, 1))
        assert sum(n for (_s, _d, n) in rel) < 512 << 10
    if form == "P":                         # the stretch: 17 one-piece steps, all high on both sides but the first
        st = _segment(steps)[:17]
        assert all(len(x) == 1 and x[0][4] == 1024 and x[0][3] - EDGE >= 1 << 27 for x in st)


@pytest.mark.parametrize("form", ["P", "W1"])
def test_split_plans_exceed_the_window_by_one_granule(form):
    f = FORMS[form]
    G, window = f["G"], f["window"] * f["G"]
    steps, _send_bytes, recv_bytes, cut = split_steps(form, "steps")
    _assert_gaps(steps, recv_bytes)
    (slo, shi), (dlo, dhi) = _hulls(steps)
    assert shi - slo == dhi - dlo == window + G and recv_bytes == window + G + 2 * EDGE
    for part in (steps[:cut], steps[cut:]):
        (a, b), (c, d) = _hulls(part)
        assert b - a <= window and d - c <= window and sum(1 for st in part if st) >= 2
    (a, b), (c, d) = _hulls(steps[:cut + 1])
    assert b - a > window and d - c > window
    for st in steps:                        # no step alone exceeds it, so a cut between steps is enough
        if st:
            (a, b), (c, d) = _hulls([st])
            assert b - a <= window and d - c <= window
    assert _hulls(steps[:cut])[0][0] != _hulls(steps[cut:])[0][0] and _hulls(steps[:cut])[1][0] != _hulls(steps[cut:])[1][0]
    assert len(steps) >= 13
    steps, _send_bytes, recv_bytes, _none = split_steps(form, "one_step")
    _assert_gaps(steps, recv_bytes)
    (a, b), (c, d) = _hulls(steps[:1])
    assert b - a == d - c == window + G and sum(1 for st in steps if st) >= 2


def test_sparse_plan_covers_every_byte_of_recv():
    """the windows (destination + GUARD on both sides, clipped, merged) and the spans of the rest
    tile RECV exactly; a CPU execution's stores pass, a wrong byte names its copy, a store a GiB
    away from every destination is found through its span, and a store into a guard as a gap"""
    recv_bytes = (3 << 30) + 77
    steps = [[(0, 0, 1, 100, 50), (0, 64, 1, 5000, 1000)], [], [(0, 2000, 1, 3 << 30, 60), (0, 0, 1, 1 << 30, 17)]]
    plan = SparsePlan(steps, 4096, recv_bytes, seed=9)
    assert plan.windows == [(0, 5000 + 1000 + GUARD), ((1 << 30) - GUARD, (1 << 30) + 17 + GUARD),
                            ((3 << 30) - GUARD, recv_bytes)]
    tiles = sorted(plan.windows + [(o, o + n) for o, n in plan.rest])
    assert tiles[0][0] == 0 and tiles[-1][1] == recv_bytes and all(a[1] == b[0] for a, b in zip(tiles, tiles[1:]))
    assert all(0 < n <= SPAN for _o, n in plan.rest) and sum(1 for _o, n in plan.rest if n < SPAN) <= len(plan.windows)
    assert sum(n for _o, n in plan.send_spans) == 4096
    good = [(do, plan.src(so, n)) for st in steps for (_a, so, _b, do, n) in st]
    plan.judge_stores(good)
    for stores, text in (
            (good[:1] + [(5000, plan.src(64, 1000)[::-1].copy())] + good[2:], "byte 0 of the copy of 1000 B, source phase 0, destination phase 8, step 0"),
            (good + [(5000 + 1000, np.zeros(16, np.uint8))], "in the gap 1 B from the copy of 1000 B"),
            (good + [((2 << 30) + 5, np.full(1, 0xA4, np.uint8))], "1 spans of RECV outside every destination's guard were written"),
            (good[:3], "byte 0 of the copy of 17 B")):
        with pytest.raises(pytest.fail.Exception) as e:
            plan.judge_stores(stores)
        assert text in str(e.value), str(e.value)
