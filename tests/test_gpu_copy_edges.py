"""GPU: the copy kernels (csrc/kernels.h) at the edges the schedules never produce --
pipelined_copy16<4>'s lane-divergent pipeline boundaries, copy_kernel_w with many pieces per
wave, realign_copy at its tile and piece edges -- and fill_kernel / verify_kernel on ragged
segments longer than their 64 KiB chunk.

The copy tests fill SEND with seeded random bytes, run ONE synthetic plan (synth_plan.Synth,
every step one copy launch: XG_ENGINE_MAX_STEP=0), read the WHOLE receive region back and
compare it with the in-order numpy execution.  Destinations are separated by poisoned gaps of
16 to 48 bytes, so an overrun, a dropped store and a shifted store all show; a mismatch names
the copy that holds (or is nearest to) the first differing byte.  The comparison is bit-exact.
"""
import numpy as np
import pytest

from synth_plan import (CHUNK_A, CHUNK_B, PHASE_PAIRS, WAVE_NP, Synth, _assert_gaps, _compare, _ctx_env, _layout,
                        _up16, pipeline_edge_lens, realign_edge_lens, wave_edge_steps)

pytestmark = pytest.mark.gpu

NEVER = 1 << 40          # XG_COPY_WAVE_MIN: no launch is large enough for copy_kernel_w


def _run_and_compare(xg, cx, steps, send_bytes, recv_bytes, seed, wave=None):
    """load, check how the plan launches (wave: None = no copy_kernel_w launch, else a function
    of (launches, grid, max pieces per wave)), run once, compare the whole receive region"""
    _assert_gaps(steps, recv_bytes)
    sy = Synth(xg, cx, send_bytes, recv_bytes, steps, seed=seed)
    try:
        d = xg.device()
        assert d.xg_plan_engine(sy.p) == 0
        assert d.xg_plan_launches(sy.p) == len(steps)
        assert sum(xg.plan_kind_launches(sy.p)) == len(steps) - xg.plan_engine_segments(sy.p)
        got_wave = xg.plan_wave_launches(sy.p)
        if wave is None:
            assert got_wave[0] == 0, got_wave
        else:
            wave(*got_wave)
        want = sy.expected()
        got = sy.run()
        _compare(steps, got, want)
    finally:
        sy.close()


# ------------------------------------------------------------------ B.1 copy_kernel_g
@pytest.mark.parametrize("chunk", [CHUNK_A, CHUNK_B])
@pytest.mark.parametrize("variant", [1, 6])
def test_pipelined_copy_boundaries(xg, variant, chunk):
    """copy_kernel_g<4, NT> (plain and non-temporal) on one-piece aligned copies of n4 16-B units
    at every boundary of the 4-deep pipeline: 768 (a lane enters it if i + 768 < n4: 768 / 769 /
    770, and 1023 / 1024 / 1025 where the last lane does), 1792 (a second loop trip: 1792 / 1793,
    2047 / 2048 / 2049), 255 / 256 / 257 (remainder loop only), up to 7 trips (8191), and a copy
    of two full pieces and a tail."""
    lens = pipeline_edge_lens(chunk)
    assert sum(lens) < 1 << 20
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=NEVER, XG_COPY_VARIANT=variant)
    try:
        cx.set_copy_params(chunk, -1)
        assert xg.piece_size(lens, chunk, cx.info()[1], 2048) == chunk
        copies, send_bytes, recv_bytes = _layout([(n, 0, 0) for n in lens])
        _run_and_compare(xg, cx, [copies], send_bytes, recv_bytes, seed=variant)
    finally:
        cx.close()


# ------------------------------------------------------------------ B.2 copy_kernel_w
@pytest.mark.parametrize("grid,kib", [(1, 2), (1, 4), (1, 8), (2, 8)])
def test_wave_copy_many_pieces_per_wave(xg, grid, kib):
    """copy_kernel_w<2 / 4 / 8> on a grid capped at one workgroup (XG_WAVE_GRID=1; and at two):
    its four waves copy 1, 2, 63 .. 66 and 129 / 130 pieces each, unequal counts in one launch --
    the double-buffered k -> k + 1 loop, both of its exits, and the refetch of 64 descriptors at
    pieces 64 and 128.  On a whole device (wave grid 1536 workgroups = 6144 waves) a launch of
    segments no shorter than its piece has at most 4096 pieces: one per wave, the loop never turns."""
    steps, send_bytes, recv_bytes = wave_edge_steps(kib)
    assert recv_bytes < 14 << 20
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=0, XG_COPY_VARIANT=1, XG_WAVE_GRID=grid,
                  XG_WAVE_KIB=kib)
    try:
        def wave(launches, got_grid, most):
            assert launches == len(steps)            # every step is a copy_kernel_w launch
            assert got_grid == grid
            assert most == -(-max(WAVE_NP) // (4 * grid))
            if grid == 1:
                assert most >= 130
        _run_and_compare(xg, cx, steps, send_bytes, recv_bytes, seed=10 * grid + kib, wave=wave)
    finally:
        cx.close()


def test_wave_grid_hook_only_lowers(xg):
    """XG_WAVE_GRID caps copy_kernel_w's grid and cannot raise it above occupancy x CUs; the
    device's own figure is printed (copy_kernel_w, quotes it)."""
    copies, send_bytes, recv_bytes = _layout([(4096, 0, 0)])
    grids = {}
    for name, env in (("device", {}), ("huge", {"XG_WAVE_GRID": 1 << 30}), ("zero", {"XG_WAVE_GRID": 0}),
                      ("three", {"XG_WAVE_GRID": 3})):
        cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=0, XG_COPY_VARIANT=1, **env)
        try:
            cus = cx.info()[1]
            sy = Synth(xg, cx, send_bytes, recv_bytes, [copies])
            try:
                launches, grids[name], most = xg.plan_wave_launches(sy.p)
                assert (launches, most) == (1, 1)
            finally:
                sy.close()
        finally:
            cx.close()
    print("copy_kernel_w<8>: wave_grid %d = %d CUs x %d workgroups" % (grids["device"], cus, grids["device"] // cus))
    assert grids["device"] >= cus and grids["device"] % cus == 0
    assert grids["huge"] == grids["device"] and grids["zero"] == grids["device"] and grids["three"] == 3


# ------------------------------------------------------------------ B.3 realign_copy
def test_realign_copy_tile_and_piece_edges(xg):
    """realign_copy at ten (source, destination) phase pairs: the byte path (n < head + 16) on
    both sides of its threshold, bodies of exactly 1, 2 and 3 tiles and one 16-B store either
    side of a tile edge, each with a tail of 0, 1 and 15 bytes, the 8-tile ring of a full piece,
    and transfers longer than a piece (a second piece of one byte; three pieces) whose pieces
    all run at the same phase pair.  One source starts at SEND's first byte and one ends at its
    last, so the aligned 16-B window reads touch the region's first and last chunk."""
    specs = [(4099, 0, 1)]                                     # its source lands at SEND offset 0
    for (sp, dp) in PHASE_PAIRS:
        specs += [(n, sp, dp) for n in realign_edge_lens(dp)]
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0, XG_COPY_WAVE_MIN=NEVER)
    try:
        cx.set_copy_params(CHUNK_A, -1)
        copies, send_bytes, recv_bytes = _layout(specs, reverse_sources=False)
        assert copies[0][1] == 0
        # ... and one whose source ends with the region: phase 5 -> 12, 4107 B (5 + 4107 = 257 x 16)
        send_bytes += _up16(4107) + 16
        last = (0, send_bytes - 4107, 1, recv_bytes + 12, 4107)
        assert last[1] % 16 == 5 and send_bytes % 16 == 0
        recv_bytes = _up16(last[3] + 4107) + 32
        copies.append(last)
        lens = [c[4] for c in copies]
        assert xg.piece_size(lens, CHUNK_A, cx.info()[1], 2048) == CHUNK_A
        assert 2 << 20 < sum(lens) < 3 << 20
        _run_and_compare(xg, cx, [copies], send_bytes, recv_bytes, seed=3)
    finally:
        cx.close()


# ------------------------------------------------------------------ B.4 fill / verify
@pytest.fixture(scope="module")
def ctx(xg):
    c = xg.Context(rank=0, nranks=1, device=0)
    yield c
    c.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [65535, 65544, 65552, 131077])
@pytest.mark.parametrize("method", [1, 2])
def test_fill_and_verify_past_one_chunk(xg, ctx, method, d, mode):
    """fill_kernel and verify_kernel on segments of more than their 64 KiB chunk that are not
    multiples of it (65535 stays inside one; 131077 puts slots on odd addresses): the byte-wise
    fill across a chunk boundary, the unaligned verify path at c0 > 0, and the atomicAdd /
    atomicMin merge of chk / bad / first_bad across a slot's chunks.  The receive region is read
    back and compared with the oracle byte for byte; then single flipped bytes at and around the
    chunk boundary, and two in different chunks, are reported exactly."""
    import xg_oracle as O
    P, A, it = 3, 2, 1
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, d, 3, rl, ntimes=1)
    run = xg.MethodRun(ctx, s, it=it, mode=mode)
    try:
        run.run_timed()
        exp = O.expected_recv(method, P, A, d, rl, it, mode=mode)
        nrecv = run.view.region_bytes[xg.BUF_RECV]
        want = np.full(nrecv, 0xA5, np.uint8)
        for r, buf in exp.items():
            if buf is not None and buf.size:
                want[s.recv_offset(1, r): s.recv_offset(1, r) + buf.size] = buf
        got = np.frombuffer(run.read(xg.BUF_RECV, 0, nrecv), dtype=np.uint8)
        assert (got == want).all(), "RECV differs from the oracle first at byte %d" % int(np.flatnonzero(got != want)[0])
        nslots = len(run.slots)
        assert nslots == 6
        clean = [O.chk64(want[off: off + d]) for (_src, _seed, _dst, off) in run.slots]
        chk, bad, first = run.verify()
        assert bad == [0] * nslots and first == [-1] * nslots and chk == clean

        def flipped(victim, offsets):
            """verify() with these bytes of the victim slot flipped; the bytes are restored"""
            base = run.slots[victim][3]
            buf = want[base: base + d].copy()
            for at in offsets:
                buf[at] ^= 0x5A
                run.write(xg.BUF_RECV, base + at, bytes([int(buf[at])]))
            out = run.verify()
            for at in offsets:
                run.write(xg.BUF_RECV, base + at, bytes([int(want[base + at])]))
            return out, O.chk64(buf)

        for i, at in enumerate(a for a in (0, 65535, 65536, 65537, d - 1) if a < d):
            victim = (i + d) % nslots
            (chk, bad, first), want_chk = flipped(victim, [at])
            assert bad == [int(k == victim) for k in range(nslots)], (at, bad)
            assert first == [at if k == victim else -1 for k in range(nslots)], (at, first)
            assert chk[victim] != clean[victim] and chk[victim] == want_chk
            assert all(chk[k] == clean[k] for k in range(nslots) if k != victim)
        # two bytes of one slot, in different chunks wherever the slot has two (d > 65536 + 1)
        lo, hi = 65533 if d > 65536 else 3, d - 2
        assert d <= 65536 or lo // 65536 != hi // 65536
        victim = nslots - 1
        (chk, bad, first), want_chk = flipped(victim, [hi, lo])
        assert bad == [2 * int(k == victim) for k in range(nslots)], bad
        assert first == [lo if k == victim else -1 for k in range(nslots)], first
        assert chk[victim] == want_chk and chk[:victim] == clean[:victim]
        chk, bad, first = run.verify()
        assert bad == [0] * nslots and first == [-1] * nslots and chk == clean
    finally:
        run.close()
