"""The host side of the copy-kernel edge tests (synth_plan.py, test_gpu_copy_edges.py): the
layouts keep what the GPU tests lean on, and a wrong receive region is reported with the copy
that holds the first differing byte -- checked here, where no GPU is needed, because a passing
GPU suite never runs the reporting path.  Likewise the plans of the step-engine tests
(test_gpu_solo_synth.py): their granules, row counts, table capacity and barrier flags."""
import numpy as np
import pytest

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
