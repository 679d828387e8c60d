"""The host side of the copy-kernel edge tests (synth_plan.py, test_gpu_copy_edges.py): the
layouts keep what the GPU tests lean on, and a wrong receive region is reported with the copy
that holds the first differing byte -- checked here, where no GPU is needed, because a passing
GPU suite never runs the reporting path."""
import numpy as np
import pytest

from synth_plan import (PHASE_PAIRS, WAVE_NP, _assert_gaps, _compare, _layout, realign_edge_lens,
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
