"""Synthetic one-GPU plans for the GPU tests: xg_devplan structures (include/xg_sched.h) built
directly from lists of copies and executed through the C-ABI (xg_plan_load / xg_plan_run); the
expected bytes come from executing the same steps in order with numpy."""
import ctypes as C
import os

import numpy as np
import pytest


# Piece sizes pinned for the copy-kernel edge tests (test_gpu_copy_edges.py): 16 x an odd number,
# so xg_piece_size can take no halving (chunk / 2 is no multiple of 16) and every copy of at most
# `chunk` bytes is exactly one piece.  Lengths in 16-B units around pipelined_copy16<4>'s
# boundaries: a lane enters the pipeline if i + 768 < n4 and repeats its loop if i + 1792 < n4.
CHUNK_A = 16 * 2049
CHUNK_B = 16 * 8191
N4_A = [1, 255, 256, 257, 767, 768, 769, 770, 1023, 1024, 1025, 1791, 1792, 1793, 2047, 2048, 2049]
N4_A_LONG = 2 * 2049 + 769              # two full pieces and a tail that enters the pipeline
N4_B = [2816, 2817, 3839, 3840, 3841, 4864, 4865, 8190, 8191]      # up to 7 trips of the main loop


def pipeline_edge_lens(chunk):
    """byte lengths of the copies of the copy_kernel_g launch at this pinned chunk"""
    if chunk == CHUNK_A:
        return [16 * n for n in N4_A] + [16 * N4_A_LONG]
    assert chunk == CHUNK_B
    return [16 * n for n in N4_B]


# (source mod 16, destination mod 16) of the realign_copy edge test; the first two agree mod 16
# and reach realign_copy through a ragged length
PHASE_PAIRS = [(0, 0), (3, 3), (0, 1), (1, 0), (15, 0), (0, 15), (15, 15), (5, 12), (8, 4), (13, 6)]


def realign_edge_lens(dphase):
    """lengths around realign_copy's byte path, its 4 KiB tiles and the CHUNK_A piece cut"""
    head = (16 - dphase) & 15
    lens = [1, 15, 16, 17, 30, 31, 32, 47, 48]
    lens += [head + body + tail for body in (16, 4080, 4096, 4112, 8192, 12304) for tail in (0, 1, 15)]
    lens += [head + 32768,              # eight full tiles in one piece
             CHUNK_A + 1,               # the second piece is one byte
             2 * CHUNK_A + 4099]        # three pieces at one phase pair
    return lens


def _up16(x):
    return (x + 15) & ~15


def _layout(specs, reverse_sources=True):
    """specs: (length, source phase, destination phase) per copy -> SEND -> RECV copies in that
    order, send_bytes, recv_bytes.  Destinations ascend in spec order, each at its phase, behind a
    poisoned gap of 16..48 B (+ the phase); sources are disjoint, laid out in the opposite order."""
    so_of, cur = {}, 0
    order = range(len(specs) - 1, -1, -1) if reverse_sources else range(len(specs))
    for i in order:
        n, sp, _dp = specs[i]
        so_of[i] = _up16(cur) + sp
        cur = so_of[i] + n
    send_bytes = _up16(cur) + 16
    copies, cur = [], 0
    for i, (n, _sp, dp) in enumerate(specs):
        do = _up16(cur) + 16 * (1 + i % 3) + dp
        copies.append((0, so_of[i], 1, do, n))
        cur = do + n
    return copies, send_bytes, _up16(cur) + 32


def _assert_gaps(steps, recv_bytes):
    """the property the tests lean on: every destination has >= 16 poisoned bytes on both sides"""
    iv = sorted((do, do + n) for st in steps for (_sb, _so, _db, do, n) in st)
    assert iv[0][0] >= 16 and recv_bytes - iv[-1][1] >= 16
    assert all(b[0] - a[1] >= 16 for a, b in zip(iv, iv[1:]))


def _compare(steps, got, want):
    if (got == want).all():
        return
    at = int(np.flatnonzero(got != want)[0])
    best = None
    for s, st in enumerate(steps):
        for (_sb, so, _db, do, n) in st:
            dist = 0 if do <= at < do + n else min(abs(at - do), abs(at - (do + n - 1)))
            if best is None or dist < best[0]:
                best = (dist, s, so, do, n)
    dist, s, so, do, n = best
    where = "byte %d of" % (at - do) if dist == 0 else "in the gap %d B from" % dist
    pytest.fail("%d bytes differ; the first, RECV[%d] = 0x%02x (expected 0x%02x), is %s the copy of %d B, "
                "source phase %d, destination phase %d, step %d (RECV[%d..%d))"
                % (int((got != want).sum()), at, got[at], want[at], where, n, so % 16, do % 16, s, do, do + n))


WAVE_NP = [1, 3, 4, 6, 255, 256, 257, 262, 517]


def wave_edge_steps(kib):
    """one launch per entry of WAVE_NP with exactly that many pieces of <= kib KiB, every offset
    and length a multiple of 16: single-piece copies whose lengths cycle over full, 16 B, around
    1 KiB (one access per lane: 1008 / 1024 / 1040) and full - 16, and up to three copies of
    3 * kib KiB + 48 B, each cut into four pieces"""
    full = kib << 10
    cyc = [full, 16, 1008, 1024, 1040, full - 16]
    specs, cuts = [], [0]
    for li, npieces in enumerate(WAVE_NP):
        nbig = min(3, npieces // 4)
        nsingle = npieces - 4 * nbig
        at = {0, nsingle // 2, nsingle} if nbig == 3 else ({nsingle // 2} if nbig else set())
        at = sorted(at)[:nbig]
        assert len(at) == nbig
        for k in range(nsingle + 1):
            if k in at:
                specs.append((3 * full + 48, 0, 0))
            if k < nsingle:
                specs.append((cyc[(k + li) % 6], 0, 0))
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[a:b] for a, b in zip(cuts, cuts[1:])]
    for st, npieces in zip(steps, WAVE_NP):
        assert sum(-(-n // full) for (_a, _b, _c, _d, n) in st) == npieces
    return steps, send_bytes, recv_bytes


def _ctx_env(xg, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return xg.Context(rank=0, nranks=1, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Synth:
    """regions (SEND random bytes, RECV poisoned) + a synthetic one-GPU plan"""

    def __init__(self, xg, ctx, send_bytes, recv_bytes, steps, seed=0):
        d = xg.device()
        self.xg, self.d = xg, d
        rb = (C.c_int64 * xg.NBUF)(send_bytes, recv_bytes, 0, 0, 0)
        self.r = C.c_void_p()
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(self.r)) == 0
        rng = np.random.default_rng(seed)
        self.send = rng.integers(0, 256, send_bytes, dtype=np.uint8)
        self.recv = np.full(recv_bytes, 0xA5, np.uint8)
        buf = self.send.tobytes()
        assert d.xg_regions_write(self.r, xg.BUF_SEND, 0, buf, len(buf)) == 0
        copies = [c for st in steps for c in st]
        self.copies = (xg.Copy * max(1, len(copies)))(
            *[xg.Copy(so, do, ln, sb, db) for (sb, so, db, do, ln) in copies])
        sp, b = [], 0
        for st in steps:
            sp.append(xg.StepPlan(b, len(st), 0, 0, 0, 0, 0, 0))
            b += len(st)
        self.sp = (xg.StepPlan * len(sp))(*sp)
        self.p2p = (xg.P2P * 1)()
        dp = xg.DevPlan()
        dp.gpu, dp.ngpus, dp.nsteps = 0, 1, len(steps)
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

    def expected(self, recv=None):
        """RECV after one run that starts from `recv` (default: the poisoned region)"""
        bufs = {0: self.send.copy(), 1: (self.recv if recv is None else recv).copy()}
        for st in self.steps:
            # one step = simultaneous copies (the generator keeps them independent)
            vals = [bufs[sb][so:so + ln].copy() for (sb, so, db, do, ln) in st]
            for (sb, so, db, do, ln), v in zip(st, vals):
                bufs[db][do:do + ln] = v
        return bufs[1]

    def run(self):
        n = max(1, len(self.steps))
        done, post, wall = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
        assert self.d.xg_plan_run(self.p, done, post, C.byref(wall)) == 0
        out = C.create_string_buffer(len(self.recv))
        assert self.d.xg_regions_read(self.r, 1, 0, out, len(self.recv)) == 0
        return np.frombuffer(out.raw, np.uint8)

    def close(self):
        self.d.xg_plan_free(self.p)
        self.d.xg_regions_free(self.r)
