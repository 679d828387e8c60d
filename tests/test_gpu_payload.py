"""GPU: exchanging caller-owned device buffers, checked by span checksums.

span_chk_kernel (csrc/kernels.h) behind xg_chk_spans, xg_regions_adopt, MethodRun(fill=False),
xg.payload_check and xg_exchange.  The payloads are seeded random bytes the library knows nothing
about; delivery is judged by position-keyed checksums of the source segments and the delivered
slots (xg_deliveries), and where the issue is the bytes themselves (adoption, xg_exchange) the
whole region is read back and compared bit for bit with numpy.
"""
import ctypes as C

import numpy as np
import pytest

from synth_plan import _ctx_env

pytestmark = pytest.mark.gpu

CHUNK = 65536            # kChkChunk: bytes of a span per span_chk_kernel workgroup
CFG0 = (32, 14, 2048, 3)  # BASELINE configs[0]: P, A, d, c
# (pack_max_seg, pack form) of a multi-GPU plan: direct, one-sided, two-sided (test_gpu_virtual.py)
PACKINGS = ((0, -1), (1 << 30, 1), (1 << 30, 0))


@pytest.fixture(scope="module")
def ctx(xg):
    c = xg.Context(rank=0, nranks=1, device=0)
    yield c
    c.close()


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _write(obj, buf, off, arr):
    obj.write(buf, off, arr.tobytes())


def _read(obj, buf, off, n):
    return np.frombuffer(obj.read(buf, off, n), dtype=np.uint8)


# ------------------------------------------------------------------ 1. the kernel against the oracle
def _span_cases(xg):
    """(region, offset, length) of every span, and the region sizes.  Short lengths at all 16
    start phases in SEND / RECV / STAGE_SEND in turn, each in a slot of its own; the chunk-sized
    ones share one window of RECV (spans only read, so they may overlap)."""
    short = [0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 4095, 4096, 4097,
             # 4 KiB is one 16-B piece per lane of the 256-lane workgroup: +- one wave of pieces
             # (1 KiB), +- one piece, +- 64 B -- the trip count of the piece loop differs by lane
             4096 - 1024, 4096 + 1024, 4096 - 16, 4096 + 16, 4096 - 64, 4096 + 64,
             # the 4-deep batch loop: entered by a lane if its piece + 768 exists (synth_plan's edges)
             16 * 769, 16 * 1024 + 3, 16 * 1793 + 9]
    bufs = (xg.BUF_SEND, xg.BUF_RECV, xg.BUF_STAGE_SEND)
    cur = {b: 0 for b in bufs}
    spans = []
    for i, (ph, n) in enumerate((ph, n) for n in short for ph in range(16)):
        b = bufs[i % 3]
        off = cur[b] + 32 + ph          # the first span starts past byte 0: that one comes below
        spans.append((b, off, n))
        cur[b] = (off + n + 15) & ~15
    win = cur[xg.BUF_RECV] + 64
    for ph in range(16):
        for n in (CHUNK - 1, CHUNK, CHUNK + 1):
            spans.append((xg.BUF_RECV, win + ph, n))
    for ph in (0, 1, 8, 15):
        for n in (2 * CHUNK + 5, 3 * CHUNK):
            spans.append((xg.BUF_RECV, win + ph, n))
    cur[xg.BUF_RECV] = win + 3 * CHUNK + 16 + 5     # ends 5 bytes into a granule
    sizes = [cur[xg.BUF_SEND] + 3, cur[xg.BUF_RECV], cur[xg.BUF_STAGE_SEND] + 16, 0, 0]
    spans.append((xg.BUF_SEND, 0, 4097))                                   # begins at a region's first byte
    spans.append((xg.BUF_SEND, sizes[0] - 1001, 1001))                     # ends at a region's last byte
    spans.append((xg.BUF_RECV, sizes[1] - (CHUNK + 77), CHUNK + 77))       # ... across a chunk, misaligned end
    spans.append((xg.BUF_STAGE_SEND, 0, sizes[2]))                         # a whole region
    return spans, sizes


def test_span_checksums_equal_the_oracle(xg, ctx):
    """xg_chk_spans == O.chk64 on seeded random bytes, every span in ONE launch: all 16 start
    phases x lengths 0 .. 4097 and around 4 KiB (one 16-B piece per lane), and lengths c - 1, c,
    c + 1 (all phases), 2c + 5 and 3c (phases 0, 1, 8, 15) for the kernel's chunk c = kChkChunk =
    64 KiB per workgroup; spans in SEND, RECV and STAGE_SEND, one from a region's first byte, two
    up to a region's last.  A span past its region's end is XG_EARG."""
    import xg_oracle as O
    spans, sizes = _span_cases(xg)
    assert sum(sizes) < 8 << 20 and sum(n for _b, _o, n in spans) < 8 << 20
    reg = xg.Regions(ctx, sizes)
    try:
        data = {}
        for b in (xg.BUF_SEND, xg.BUF_RECV, xg.BUF_STAGE_SEND):
            data[b] = _rand(100 + b, sizes[b])
            _write(reg, b, 0, data[b])
        got = xg.chk_spans(reg, spans)
        want = [O.chk64(data[b][o:o + n]) for b, o, n in spans]
        bad = [(b, o, n, hex(g), hex(w)) for (b, o, n), g, w in zip(spans, got, want) if g != w]
        assert not bad, (len(bad), bad[:8])
        assert xg.chk_spans(reg, []) == []
        # the kernel wrote nothing
        for b in data:
            assert np.array_equal(_read(reg, b, 0, sizes[b]), data[b])
        d = xg.device()
        out = (C.c_uint64 * 2)()
        for b, o, n in ((xg.BUF_SEND, sizes[0] - 10, 11), (xg.BUF_RECV, sizes[1], 1), (xg.BUF_SCRATCH, 0, 1),
                        (xg.NBUF, 0, 0), (xg.BUF_SEND, -1, 1), (xg.BUF_SEND, 0, -1)):
            arr = (xg.BufSpan * 2)(xg.BufSpan(xg.BUF_SEND, 0, 0, 16), xg.BufSpan(b, 0, o, n))
            assert d.xg_chk_spans(reg._r, arr, 2, out) == 3, (b, o, n)       # XG_EARG
        assert xg.chk_spans(reg, [(xg.BUF_RECV, sizes[1], 0), (xg.BUF_SCRATCH, 0, 0)]) == [O.chk64(data[0][:0])] * 2
    finally:
        reg.close()


# ------------------------------------------------------------------ 2. against verify_kernel
@pytest.mark.parametrize("d", [1000, 65536 + 8])
def test_slot_checksums_equal_verify(xg, ctx, d):
    """a fingerprint-filled run (P 8, A 3, m1): slot_chk() (span_chk_kernel) equals verify()[0]
    (verify_kernel) slot for slot -- d = 1000 puts the slots on every 8-B phase, 64 KiB + 8 spans
    two chunks"""
    P, A = 8, 3
    s = xg.Schedule(1, P, A, d, 3, xg.aggregator_list(P, A), iteration=2)
    run = xg.MethodRun(ctx, s, it=2, mode=1)
    try:
        run.run_timed()
        chk, bad, _first = run.verify()
        assert len(chk) == P * A and not any(bad)
        assert run.slot_chk() == chk
        assert xg.payload_check(run) == []
    finally:
        run.close()


# ------------------------------------------------------------------ 3. adoption
class Caller:
    """a "caller's" allocation (an ordinary xg.Regions whose SEND region is the arena) of random
    bytes, with a SEND and a RECV buffer inside it at 16-B aligned addresses that are 48 past a
    256-B line, each between two 64-byte guards"""

    def __init__(self, xg, ctx, send_bytes, recv_bytes, seed, skew=48):
        self.xg = xg
        up = lambda x: (x + 255) & ~255
        self.send_off = 256 + skew
        self.recv_off = up(self.send_off + send_bytes + 64) + 256 + skew
        self.total = up(self.recv_off + recv_bytes + 64)
        self.send_bytes, self.recv_bytes = send_bytes, recv_bytes
        self.arena = xg.Regions(ctx, [self.total, 0, 0, 0, 0])
        self.image = _rand(seed, self.total)                 # what the arena must hold
        _write(self.arena, xg.BUF_SEND, 0, self.image)
        base = self.arena.ptr(xg.BUF_SEND)
        assert base % 256 == 0
        self.send, self.recv = base + self.send_off, base + self.recv_off

    def read(self):
        return _read(self.arena, self.xg.BUF_SEND, 0, self.total)

    def close(self):
        self.arena.close()


def _deliver(image, caller, dl, d):
    """numpy execution of the exchange on the arena's image (one GPU)"""
    send = image[caller.send_off:caller.send_off + caller.send_bytes].copy()
    for q in dl:
        image[caller.recv_off + q.recv_off:caller.recv_off + q.recv_off + d] = send[q.send_off:q.send_off + d]


@pytest.mark.parametrize("d", [1000, 4096])
def test_adopted_buffers(xg, ctx, d):
    """m1-m4 at P 8, A 3 over SEND / RECV adopted from inside a caller's allocation (+48 B past a
    line, 64 random guard bytes around each; d = 1000 takes the realign path): adopting writes
    nothing; after each run the whole allocation equals the numpy execution -- every slot its
    source segment, SEND and the four guards untouched -- and payload_check agrees; closing the
    adopted regions leaves the allocation alive and intact; a pointer at +8 B is XG_EARG"""
    P, A = 8, 3
    rl = xg.aggregator_list(P, A)
    for method in (1, 2, 3, 4):
        s = xg.Schedule(method, P, A, d, 3, rl)
        rb = s.devplan(1, 0).region_bytes
        cal = Caller(xg, ctx, rb[0], rb[1], seed=10 * method + d)
        try:
            with pytest.raises(xg.XGError, match="code 3"):
                xg.Regions.adopt(ctx, rb, send=cal.send + 8, recv=cal.recv)
            with pytest.raises(xg.XGError, match="code 3"):
                xg.Regions.adopt(ctx, rb, send=cal.send, recv=cal.recv + 8)
            with pytest.raises(xg.XGError, match="code 3"):       # not inside its allocation
                xg.Regions.adopt(ctx, rb, send=cal.send, recv=cal.arena.ptr(xg.BUF_SEND) + cal.total - 256)
            reg = xg.Regions.adopt(ctx, rb, send=cal.send, recv=cal.recv)
            assert (reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV)) == (cal.send, cal.recv)
            assert np.array_equal(cal.read(), cal.image), "adopting wrote to the caller's memory"
            assert np.array_equal(_read(reg, xg.BUF_RECV, 0, rb[1]), cal.image[cal.recv_off:cal.recv_off + rb[1]])
            run = xg.MethodRun(ctx, s, regions=reg, fill=False)      # poisons RECV (an explicit xg_regions_poison)
            try:
                cal.image[cal.recv_off:cal.recv_off + rb[1]] = 0xA5
                run.run_timed()
                _deliver(cal.image, cal, s.deliveries(1), d)
                got = cal.read()
                diff = np.flatnonzero(got != cal.image)
                assert diff.size == 0, (method, d, "first differing arena byte", int(diff[0]), cal.send_off, cal.recv_off)
                assert xg.payload_check(run) == []
            finally:
                run.close()
            reg.close()
            assert np.array_equal(cal.read(), cal.image), "closing the adopted regions touched the allocation"
        finally:
            cal.close()


# ------------------------------------------------------------------ 4. same plan, same kernels
def _shape(run):
    return (run.launches, run.wave_launches(), run.engine_steps(), run.engine_workgroups, run.engine_rails, run.nsteps)


def _same_plan(xg, cx, s):
    rb = s.devplan(1, 0).region_bytes
    plain = xg.MethodRun(cx, s, mode=1)
    try:
        want = _shape(plain)
    finally:
        plain.close()
    cal = Caller(xg, cx, rb[0], rb[1], seed=s.method, skew=0)      # 256-B aligned, as hipMalloc gives
    try:
        assert cal.send % 256 == 0 and cal.recv % 256 == 0
        reg = xg.Regions.adopt(cx, rb, send=cal.send, recv=cal.recv)
        run = xg.MethodRun(cx, s, regions=reg, fill=False)
        try:
            assert _shape(run) == want, (s.method, _shape(run), want)
            run.run_timed()
            assert xg.payload_check(run) == []
        finally:
            run.close()
            reg.close()
    finally:
        cal.close()
    return want


@pytest.mark.parametrize("method", [1, 3, 9, 15])
def test_payload_path_runs_the_same_plan(xg, ctx, method):
    """over adopted buffers the plan of configs[0] has the launches, wave-copy launches, engine
    segments, workgroups and rails of the ordinary fingerprint run of the same schedule"""
    P, A, d, c = CFG0
    want = _same_plan(xg, ctx, xg.Schedule(method, P, A, d, c, xg.aggregator_list(P, A)))
    assert want[0] >= 1


def test_payload_path_runs_the_same_plan_per_step(xg):
    """... and with one launch per step (XG_ENGINE_MAX_STEP=0) at P 8, A 3, d 2 MiB, m1"""
    cx = _ctx_env(xg, XG_ENGINE_MAX_STEP=0)
    try:
        want = _same_plan(xg, cx, xg.Schedule(1, 8, 3, 2 << 20, 3, xg.aggregator_list(8, 3)))
        assert want[3] == 0 and want[4] == 0 and want[0] >= want[5] >= 1
    finally:
        cx.close()


# ------------------------------------------------------------------ 5. every method
@pytest.fixture(scope="module")
def cfg0_regions(xg, ctx):
    P, A, d, c = CFG0
    rl = xg.aggregator_list(P, A)
    rb = [0] * xg.NBUF
    for m in range(1, 21):
        rb = [max(a, b) for a, b in zip(rb, xg.Schedule(m, P, A, d, c, rl).devplan(1, 0).region_bytes)]
    reg = xg.Regions(ctx, rb)
    payload = _rand(5, rb[0])
    yield reg, payload
    reg.close()


@pytest.mark.parametrize("method", list(range(1, 21)))
def test_every_method_delivers_a_random_payload(xg, ctx, cfg0_regions, method):
    """configs[0], every method, fill=False over a random payload on one GPU (TAM m15 / m16 go
    through SCRATCH): payload_check finds nothing; after one byte of one receive slot is flipped
    it reports exactly that (dst, slot)"""
    P, A, d, c = CFG0
    reg, payload = cfg0_regions
    s = xg.Schedule(method, P, A, d, c, xg.aggregator_list(P, A))
    run = xg.MethodRun(ctx, s, regions=reg, fill=False)
    try:
        _write(run, xg.BUF_SEND, 0, payload)
        run.run_timed()
        assert xg.payload_check(run) == []
        dl = s.deliveries(1)
        assert len(dl) == P * A
        q = dl[(37 * method) % len(dl)]
        at = q.recv_off + (method * 101) % d
        byte = _read(run, xg.BUF_RECV, at, 1)
        assert byte[0] == payload[q.send_off + at - q.recv_off]
        _write(run, xg.BUF_RECV, at, byte ^ np.uint8(0x10))
        assert xg.payload_check(run) == [(q.dst, q.slot)]
    finally:
        run.close()


# ------------------------------------------------------------------ 6. virtual jobs
@pytest.fixture(scope="module")
def worlds(xg):
    w = {G: [xg.Context.virtual(g, G, device=0) for g in range(G)] for G in (2, 3)}
    yield w
    for ctxs in w.values():
        for c in ctxs:
            c.close()


def _virtual_job(xg, ctxs, s, pack, form, rccl, corrupt):
    G = len(ctxs)
    runs = [xg.MethodRun(c, s, pack_max_seg=pack, pack_form=form, fill=False) for c in ctxs]
    try:
        for g, r in enumerate(runs):
            n = r.view.region_bytes[xg.BUF_SEND]
            if n:
                _write(r, xg.BUF_SEND, 0, _rand(1000 * s.method + 10 * G + g, n))
        xg.run_virtual(runs, rccl=rccl)
        assert xg.payload_check(runs) == [], (s.method, G, pack, form, rccl)
        if corrupt:
            # a slot of GPU 1 that another GPU sent: it arrived through the step's exchange
            # (packed forms: out of STAGE_RECV by an unpack)
            q = [q for q in s.deliveries(G) if q.dst_gpu == 1 and q.src_gpu != 1][-1]
            at = q.recv_off + s.d - 1
            _write(runs[1], xg.BUF_RECV, at, _read(runs[1], xg.BUF_RECV, at, 1) ^ np.uint8(1))
            assert xg.payload_check(runs) == [(q.dst, q.slot)], (s.method, G, pack, form)
    finally:
        for r in runs:
            r.close()


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("method", [1, 2, 5, 9])
def test_virtual_jobs_deliver_a_random_payload(xg, worlds, G, method):
    """P 8, A 4, d 4096 as a G-GPU job on this device, direct, one-sided and two-sided, a random
    payload per GPU: every slot's checksum equals its source segment's in the owning GPU's SEND;
    once more through RCCL; a byte flipped in a slot GPU 1 received from another GPU is reported"""
    P, A, d = 8, 4, 4096
    s = xg.Schedule(method, P, A, d, 3, xg.aggregator_list(P, A))
    for pack, form in PACKINGS:
        _virtual_job(xg, worlds[G], s, pack, form, rccl=False, corrupt=(form == 0))
    _virtual_job(xg, worlds[G], s, 1 << 30, 0, rccl=True, corrupt=False)


# ------------------------------------------------------------------ 7. the operator
@pytest.mark.parametrize("method", [1, 2])
def test_exchange_on_one_gpu(xg, ctx, worlds, method):
    """xg_exchange over a caller's buffers (P 8, A 3, d 4096): 0 with no bad slot, timers of every
    rank with total_time > 0, the caller's RECV holds every source segment bit for bit, SEND and
    the guards are as they were; a virtual context is refused (XG_EARG)"""
    P, A, d = 8, 3, 4096
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, d, 3, rl, iteration=1)
    rb = s.devplan(1, 0).region_bytes
    cal = Caller(xg, ctx, rb[0], rb[1], seed=70 + method)
    try:
        rc, bad, timers, err = xg.exchange(ctx, method, P, A, d, rl, 3, cal.send, cal.recv, it=1)
        assert (rc, bad, err) == (0, 0, "")
        assert len(timers) == P and all(t.total_time > 0 for t in timers)
        _deliver(cal.image, cal, s.deliveries(1), d)
        got = cal.read()
        diff = np.flatnonzero(got != cal.image)
        assert diff.size == 0, (method, "first differing arena byte", int(diff[0]))
        # unverified, and with buffers of the library's own
        assert xg.exchange(ctx, method, P, A, d, rl, 3, cal.send, None, verify=False)[:2] == (0, 0)
        rc, _bad, _t, err = xg.exchange(ctx, method, P, A, d, rl, 3, cal.send + 8, cal.recv)
        assert rc == 3 and "refused" in err
        assert np.array_equal(cal.read(), cal.image)
        rc, _bad, _t, err = xg.exchange(worlds[2][0], method, P, A, d, rl, 3, cal.send, cal.recv)
        assert rc == 3 and "virtual" in err
    finally:
        cal.close()
