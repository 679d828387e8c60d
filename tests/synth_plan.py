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


def _compare(steps, got, want, base=0):
    """got and want: RECV[base .. base + len(got))"""
    if (got == want).all():
        return
    first = int(np.flatnonzero(got != want)[0])
    at = base + first
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
                % (int((got != want).sum()), at, got[first], want[first], where, n, so % 16, do % 16, s, do, do + n))


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


# ------------------------------------------------------------------ step-engine plans
# (test_gpu_solo_synth.py; their host side is checked in test_synth_plan.py)
PIECE, K = 1024, 8                      # kernels.h kSoloPiece, kSoloK
SBASE, DBASE = 1 << 32, 3 << 32         # stand-in region addresses for the CPU table builder

# the last access of a piece ends inside, at and past a 64-lane instruction (64 x G bytes)
SOLO_LENS = {
    16: [16, 32, 1008, 1024, 1040, 2048, 3 * 1024 + 16],
    4: [4, 60, 64, 68, 252, 256, 260, 1020, 1024, 1028, 2044],
    1: [1, 15, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049],
}


def _solo_pays(nbytes, n, rails, waves, busy, gran):
    """plan_tables.cc solo_pays, mirrored only to SIZE plans (10 % kept in hand on the rail side):
    the rail count a GPU test asserts is the check that the library's model agreed"""
    traffic = 2.0 * nbytes
    if waves == 1:
        solo = traffic / min(rails * 15e9 * gran / 16.0, 6e12 * gran / 16.0) + n * 0.05e-6
    else:
        solo = traffic / (rails * 120e9) + n * 0.2e-6
    grid = traffic / 5e12 + n * 1.0e-6 + (8e-6 if busy < 2 else 0.0)
    return 1.1 * solo < grid


def _pieces(steps):
    return sum(-(-n // PIECE) for st in steps for (_a, _b, _c, _d, n) in st)


def _rails(steps, rails_max, waves):
    """the rail count xg_solo_tables_g gives (test_solo_tables.py)"""
    return max(1, min(rails_max, _pieces(steps) // waves))


def _segment(steps):
    """the steps build_segments keeps: those that move nothing are trimmed off both ends"""
    busy = [i for i, st in enumerate(steps) if st]
    return steps[busy[0]:busy[-1] + 1]


def _sized(build, rails_max, waves, gran):
    """build(pad) with the fewest extra empty steps at which the cost model takes rails"""
    for pad in range(0, 1500, 4):
        steps, send_bytes, recv_bytes = build(pad)
        seg = _segment(steps)
        nbytes = sum(n for st in seg for (_a, _b, _c, _d, n) in st)
        if _solo_pays(nbytes, len(seg), _rails(steps, rails_max, waves), waves, sum(1 for st in seg if st), gran):
            return steps, send_bytes, recv_bytes
    raise AssertionError("no rail routing at this size")


def _spans(steps):
    return [[(SBASE + so, DBASE + do, n) for (_sb, so, _db, do, n) in st] for st in steps]


def _tables(xg, steps, rails_max, waves, gran):
    """the segment's solo tables, on the CPU: (shape, per-rail row barrier counts, per-rail real rows)"""
    sp = _spans(_segment(steps))
    srcs = [x[0] for st in sp for x in st]
    dsts = [x[1] for st in sp for x in st]
    rc, shape, _descs, close, _csteps, rows = xg.solo_tables(sp, rails_max, min(srcs), min(dsts), waves=waves,
                                                             granule=gran)
    assert rc == 0, (rc, shape)
    if waves == 1:                      # wide form: the row word also carries the piece's length
        close = [[x & 0xFF for x in r] for r in close]
    return shape, close, rows


# (a) copies per step: empty steps at the start, in the middle and at the end, runs of steps
# with one tiny copy each, steps of 5-40 copies; `pad` more empty steps go into the first gap
COUNTS_HEAD = [0, 0, 5, 1, 1, 1, 40, 0, 0]
COUNTS_TAIL = [13, 1, 1, 27, 0, 1, 33, 7, 1, 1, 1, 1, 40, 0, 0]
# (granule, waves per rail, XG_SOLO_RAILS; 0 = unset)
GRANULE_CTX = ([(16, 1, r) for r in (1, 7, 0)] + [(16, 16, r) for r in (1, 3, 16)] +
               [(4, 1, r) for r in (1, 7, 0)] + [(1, 1, r) for r in (1, 7, 0)])


def _granule_steps(G, pad=0):
    """24 + pad steps whose offsets and lengths are all multiples of G and not all of the next
    coarser granule (lengths G and SOLO_LENS[G][1]; for G < 16 source and destination phases too)"""
    lens = SOLO_LENS[G]
    specs, cuts = [], [0]
    for count in COUNTS_HEAD + [0] * pad + COUNTS_TAIL:
        for _ in range(count):
            i = len(specs)
            n = lens[i % 2] if count == 1 else lens[i % len(lens)]
            specs.append((n, (G * (i % 7)) % 16, (G * (i % 5)) % 16))
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    return [copies[a:b] for a, b in zip(cuts, cuts[1:])], send_bytes, recv_bytes


# (b) one piece each / (length, pieces)
SINGLE = [1024, 16, 1008, 32, 1024]
MULTI = [(1040, 2), (1024, 1), (3 * 1024 + 16, 4), (2048, 2), (16, 1), (1008, 1)]


def _row_pieces(rows, waves):
    """pieces that fill exactly `rows` rows of one rail: on a 16-wave rail the last row partly (full for one row)"""
    return rows if waves == 1 else 16 * (rows - 1) + (16 if rows == 1 else 5)


def _row_steps(npieces, waves, pad=0):
    """exactly `npieces` solo pieces: a stretch of one-piece steps (17 for 16-wave rails, so that
    one row of 16 pieces holds the ends of 15 steps), `pad` empty steps, then steps of up to 12
    (one-wave rails: 3) copies of 1, 2 and 4 pieces"""
    specs, cuts, left = [], [0], npieces
    for i in range(min(left, 17 if waves == 16 else 3)):
        specs.append((SINGLE[i % 5], 0, 0))
        cuts.append(len(specs))
        left -= 1
    cuts += [len(specs)] * pad
    i = 0
    while left:
        for _ in range(12 if waves == 16 else 3):
            if not left:
                break
            n, q = MULTI[i % 6]
            i += 1
            if q > left:
                n, q = SINGLE[i % 5], 1
            specs.append((n, 0, 0))
            left -= q
        cuts.append(len(specs))
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[a:b] for a, b in zip(cuts, cuts[1:])]
    assert _pieces(steps) == npieces
    return steps, send_bytes, recv_bytes


def _capacity_steps(per_step):
    """(c) 40 steps of `per_step` copies of 16-48 B, one solo piece each"""
    cyc = [16, 16, 32, 16, 48]
    copies, send_bytes, recv_bytes = _layout([(cyc[i % 5], 0, 0) for i in range(40 * per_step)])
    return [copies[t * per_step:(t + 1) * per_step] for t in range(40)], send_bytes, recv_bytes


ROUND_LENS = [16, 4096, 256, 1024, 33, 2048, 4095, 512, 48, 17]           # <= one 4 KiB unit each


def _round_steps(nsteps, per, reader):
    """grid engine: `nsteps` steps of `per` transfers of 16 B - 4 KiB, each its own unit; lengths
    33, 4095 and 17 and every 7th transfer's phases are off the 16-B grid (the byte path; as a
    workgroup's first unit of a step it is not prefetched).  reader: step 1 instead reads step
    0's destinations, RECV -> RECV, into destinations of its own."""
    specs = []
    for i in range(nsteps * per):
        odd = i % 7 == 3
        specs.append((ROUND_LENS[i % len(ROUND_LENS)], i % 16 if odd else 0, (5 * i) % 16 if odd else 0))
    copies, send_bytes, recv_bytes = _layout(specs)
    steps = [copies[t * per:(t + 1) * per] for t in range(nsteps)]
    if reader:
        assert per % len(ROUND_LENS) == 0          # copy k of step 1 is as long as copy k of step 0
        steps[1] = [(1, a[3], 1, b[3], b[4]) for a, b in zip(steps[0], steps[1])]
        assert all(a[4] == b[4] for a, b in zip(steps[0], steps[1]))
    return steps, send_bytes, recv_bytes


UNIT64 = 64 << 10


def _unit64_steps():
    """grid engine, 64 KiB units: transfers of unit - 16, unit, unit + 16 and 3 * unit + 4080 bytes
    (a last unit 16 B short of full, exactly full, of 16 B, of 4080 B), 11 such groups in the
    step above 4 MiB, transfers of a few KiB at odd phases, and a step that moves nothing"""
    group = [(UNIT64 - 16, 0, 0), (UNIT64, 0, 0), (UNIT64 + 16, 0, 0), (3 * UNIT64 + 4080, 0, 0)]
    spec_steps = [group + [(3 * 1024 + 5, 3, 9)], 11 * group + [(5 * 1024 + 1, 8, 1), (2 * 1024 + 7, 15, 15)], [], group]
    copies, send_bytes, recv_bytes = _layout([x for st in spec_steps for x in st])
    steps, b = [], 0
    for st in spec_steps:
        steps.append(copies[b:b + len(st)])
        b += len(st)
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
        self._load(ctx, send_bytes, recv_bytes, steps)

    def _load(self, ctx, send_bytes, recv_bytes, steps):
        """the steps as an xg_devplan, loaded over self.r"""
        xg, d = self.xg, self.d
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

    def run_timed(self):
        """one run -> (RECV, step completion times, wall time), seconds from the run's start"""
        n = max(1, len(self.steps))
        done, post, wall = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
        assert self.d.xg_plan_run(self.p, done, post, C.byref(wall)) == 0
        out = C.create_string_buffer(len(self.recv))
        assert self.d.xg_regions_read(self.r, 1, 0, out, len(self.recv)) == 0
        return np.frombuffer(out.raw, np.uint8), list(done)[:len(self.steps)], wall.value

    def run(self):
        return self.run_timed()[0]

    def poison(self):
        """RECV back to 0xA5 everywhere (xg_regions_poison)"""
        assert self.d.xg_regions_poison(self.r) == 0

    def write_recv(self, image):
        """the whole RECV region := image"""
        buf = np.ascontiguousarray(image, np.uint8).tobytes()
        assert len(buf) == len(self.recv)
        assert self.d.xg_regions_write(self.r, 1, 0, buf, len(buf)) == 0

    def close(self):
        self.d.xg_plan_free(self.p)
        self.d.xg_regions_free(self.r)
