"""GPU: placement by strided runs on the device -- copy_kernel_v (the row copy of csrc/kernels.h), the
runtime object around it (xg_vecplace_*, csrc/runtime/vecplace.hip) and xg_exchange_wv.

The kernel is driven through VecPlace over synthetic rows (seeded random SEND, poisoned RECV, a
poisoned gap around every destination block unless the test packs them on purpose) and judged over
EVERY byte of RECV against numpy over the rows' blocks, so an overrun, a dropped store or a
disturbed neighbour all show; SEND must come back unchanged.  Every table the GPU sees here is one
the host suite (test_vec_tables.py) builds and walks without a GPU."""
import json
import os
import pathlib
import sys
import tempfile

import numpy as np
import pytest

from conftest import REPO
from place_cases import payload, placed
from synth_plan import _ctx_env
from vec_cases import make_vecs, py_expand

pytestmark = pytest.mark.gpu

S, R = 0, 1
POISON = 0xA5
VEC_LEN_MAX = 1024              # kVecLenMax (host/exchange_w.c): the routing threshold
PHASE_LENS = list(range(1, 50)) + [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


def _odd(n):
    return n | 1


class Layout:
    """rows laid one behind the other: destinations ascend, every block behind a poisoned gap of at
    least 16 B; sources disjoint"""

    def __init__(self):
        self.rows, self.s, self.d = [], 16, 64

    def add(self, n, count, sp=0, dp=0, sgap=1, dgap=17):
        """a row of `count` blocks of n bytes whose first block has phases (sp, dp); the steps are
        odd, so every block of the row has phases of its own"""
        ss, ds = _odd(n + sgap), _odd(n + dgap)
        so = ((self.s + 15) & ~15) + sp
        do = ((self.d + 15) & ~15) + 16 + dp
        self.rows.append((S, R, so, do, ss, ds, n, count))
        self.s = so + (count - 1) * ss + n
        self.d = do + (count - 1) * ds + n
        return self.rows[-1]

    def sizes(self):
        return ((self.s + 15) & ~15) + 16, ((self.d + 15) & ~15) + 64


def _blocks(rows):
    for k, (sb, db, so, do, ss, ds, n, c) in enumerate(rows):
        for j in range(c):
            yield k, j, so + j * (ss if c > 1 else 0), do + j * (ds if c > 1 else 0), n


def _run_rows(xg, cx, rows, send_bytes, recv_bytes, seed, want_dispatches=None):
    """load, run once, compare every RECV byte with numpy over the rows' blocks (the poison between
    them included), SEND untouched -> (RECV, the VecPlace's (tiles, dispatches))"""
    send = np.random.default_rng(seed).integers(0, 256, send_bytes, dtype=np.uint8)
    want = np.full(recv_bytes, POISON, np.uint8)
    for (_sb, _db, so, do, ss, ds, n, c) in rows:
        if c == 1:
            want[do:do + n] = send[so:so + n]
        else:
            j = np.arange(c, dtype=np.int64)[:, None]
            i = np.arange(n, dtype=np.int64)[None, :]
            want[(do + j * ds + i).ravel()] = send[(so + j * ss + i).ravel()]
    run = xg.VecPlace(cx, rows, [send_bytes, recv_bytes, 0, 0, 0])
    try:
        shape = (run.tiles, run.dispatches)
        assert run.tiles == xg.vec_rows_tiles(rows)[-1]
        if want_dispatches is not None:
            assert run.dispatches == want_dispatches
        run.regions.write(xg.BUF_SEND, 0, send.tobytes())
        assert run.run() > 0
        got = np.frombuffer(run.regions.read(xg.BUF_RECV, 0, recv_bytes), np.uint8)
        diff = np.flatnonzero(got != want)
        if diff.size:
            at = int(diff[0])
            near = min(_blocks(rows), key=lambda b: min(abs(at - b[3]), abs(at - b[3] - b[4])))
            pytest.fail("%d bytes of RECV differ; the first is RECV[%d] = %#x, expected %#x; nearest block: row %d "
                        "block %d RECV[%d..%d)" % (diff.size, at, got[at], want[at], near[0], near[1], near[3],
                                                    near[3] + near[4]))
        back = np.frombuffer(run.regions.read(xg.BUF_SEND, 0, send_bytes), np.uint8)
        assert np.array_equal(back, send), "SEND was written"
        return got, shape
    finally:
        run.close()


# ------------------------------------------------------------------ 1. phases x lengths
@pytest.mark.parametrize("variant", [0, 6])
def test_vec_copy_phases_and_lengths(xg, variant):
    """rows of 3 blocks at all 16 x 16 (source, destination) start phases and lengths 1..49, 63..65,
    255..257, 1023..1025, 4095..4097, the steps odd (every block of a row at phases of its own), in ONE
    launch of copy_kernel_v, plain and non-temporal: every RECV byte equals numpy's, every gap keeps
    its poison"""
    lay = Layout()
    for n in PHASE_LENS:
        for sp in range(16):
            for dp in range(16):
                r = lay.add(n, 3, sp, dp)
                assert (r[2] % 16, r[3] % 16, r[4] % 2, r[5] % 2) == (sp, dp, 1, 1)
    send_bytes, recv_bytes = lay.sizes()
    cx = _ctx_env(xg, **({"XG_COPY_VARIANT": variant} if variant else {}))
    try:
        _run_rows(xg, cx, lay.rows, send_bytes, recv_bytes, 20 + variant, want_dispatches=1)
    finally:
        cx.close()


# ------------------------------------------------------------------ 2. tile edges
def test_vec_copy_tile_edges(xg):
    """rows of 16-B blocks of exactly 1, 63, 64, 65, 255, 256, 257 and 513 blocks (the wave batches of
    the scan and the 256-block tile); 40 blocks of 1000 B (bpt = 32: tiles close by bytes); a block of
    exactly the 32 KiB tile; of 32 KiB + 16 (a second piece of 16 B); 3 blocks of 100 000 B (four
    pieces each, the last short) -- at seeded random phases, one launch"""
    rng = np.random.default_rng(3)
    lay = Layout()
    ph = lambda: int(rng.integers(0, 16))
    for c in (1, 63, 64, 65, 255, 256, 257, 513):
        lay.add(16, c, ph(), ph())
    lay.add(1000, 40, ph(), ph())
    lay.add(32768, 2, ph(), ph())
    lay.add(32768 + 16, 2, ph(), ph())
    lay.add(100000, 3, ph(), ph())
    assert xg.vec_row_tiles(1000, 40) == 2 and xg.vec_row_tiles(32784, 2) == 4 and xg.vec_row_tiles(100000, 3) == 12
    send_bytes, recv_bytes = lay.sizes()
    cx = _ctx_env(xg)
    try:
        _run_rows(xg, cx, lay.rows, send_bytes, recv_bytes, 41, want_dispatches=1)
    finally:
        cx.close()


# ------------------------------------------------------------------ 3. shared cells
@pytest.mark.parametrize("n", [1, 7, 15, 17, 40])
def test_vec_copy_packed_row_shares_cells(xg, n):
    """a packed row, stride == len, of 4000 blocks (every 16-B cell belongs to several blocks, and to
    two tiles at a tile's end), sources spaced: every byte matches, the poison before the first block
    and after the last is intact"""
    rows = [(S, R, 5, 37, n + 3, n, n, 4000)]
    send_bytes, recv_bytes = 5 + 4000 * (n + 3) + 32, ((37 + 4000 * n + 15) & ~15) + 48
    cx = _ctx_env(xg)
    try:
        got, _ = _run_rows(xg, cx, rows, send_bytes, recv_bytes, 31 + n)
        assert (got[:37] == POISON).all() and (got[37 + 4000 * n:] == POISON).all()
    finally:
        cx.close()


@pytest.mark.parametrize("lens", [(7, 25), (1, 40, 15), (16, 16), (33, 5, 90)])
def test_vec_copy_striped_rows_share_cells(xg, lens):
    """two and three rows striped into each other with no gap (stride = the sum of their lengths):
    most 16-B cells belong to blocks of different rows, written by different workgroups; the bytes
    before the first block and after the last keep their poison"""
    stride, count = sum(lens), 1500
    rows, so, do = [], 3, 21
    for n in lens:
        rows.append((S, R, so, do, n, stride, n, count))       # the dense side packed, the domain side striped
        so += count * n + 5
        do += n
    end = 21 + count * stride
    send_bytes, recv_bytes = so + 32, ((end + 15) & ~15) + 48
    cx = _ctx_env(xg)
    try:
        got, _ = _run_rows(xg, cx, rows, send_bytes, recv_bytes, 50 + len(lens))
        assert (got[:21] == POISON).all() and (got[end:] == POISON).all()
    finally:
        cx.close()


# ------------------------------------------------------------------ 4. row search
def test_vec_copy_row_search(xg):
    """700 rows through the binary search over tile0 in one launch: one-tile rows mixed with rows of
    hundreds of tiles; the first and the last row are one block of one byte"""
    rng = np.random.default_rng(11)
    lay = Layout()
    lay.add(1, 1, 9, 13)
    for k in range(698):
        if k % 100 == 50:
            lay.add(16, 256 * int(rng.integers(200, 400)) + 7, int(rng.integers(0, 16)), int(rng.integers(0, 16)), dgap=1)
        elif k % 7 == 3:
            lay.add(int(rng.integers(1, 100)), int(rng.integers(257, 900)), int(rng.integers(0, 16)), int(rng.integers(0, 16)))
        else:
            lay.add(int(rng.integers(1, 300)), int(rng.integers(1, 60)), int(rng.integers(0, 16)), int(rng.integers(0, 16)))
    lay.add(1, 1, 15, 15)
    tiles = [xg.vec_row_tiles(r[6], r[7]) for r in lay.rows]
    assert len(tiles) == 700 and tiles[0] == tiles[-1] == 1 and max(tiles) >= 200 and tiles.count(1) > 400
    send_bytes, recv_bytes = lay.sizes()
    cx = _ctx_env(xg)
    try:
        _run_rows(xg, cx, lay.rows, send_bytes, recv_bytes, 61, want_dispatches=1)
    finally:
        cx.close()


# ------------------------------------------------------------------ 5. dispatch cuts
def test_vec_copy_dispatch_cuts(xg):
    """about 1 MiB with XG_COPY_LAUNCH_MAX = 256 KiB: at least 3 dispatches of one launch, a cut
    inside a row, `base` applied in every dispatch (every byte delivered once, nothing else written)"""
    lay = Layout()
    lay.add(64, 8192, 3, 5, dgap=1)
    lay.add(1000, 300, 7, 1)
    lay.add(100000, 3, 0, 9)
    lay.add(33, 700, 2, 2)
    send_bytes, recv_bytes = lay.sizes()
    cap = 256 << 10
    assert 900 << 10 < sum(r[6] * r[7] for r in lay.rows) < 1300 << 10
    host = xg.VecTables(lay.rows, [send_bytes, recv_bytes, 0, 0, 0], launch_max=cap)
    cuts, tile0 = host.cuts(), xg.vec_rows_tiles(lay.rows)
    assert len(cuts) - 1 >= 3 and any(c not in tile0 for c in cuts[1:-1]), cuts
    cx = _ctx_env(xg, XG_COPY_LAUNCH_MAX=cap)
    try:
        _run_rows(xg, cx, lay.rows, send_bytes, recv_bytes, 51, want_dispatches=len(cuts) - 1)
    finally:
        cx.close()


# ------------------------------------------------------------------ 6. 64-bit offsets
def test_vec_copy_offsets_past_2_to_31(xg):
    """one row of 3 blocks of 4 KiB with dst_step = 2^31 + 48 in a RECV region just over 4 GiB, a second
    row with src_step = 2^31 + 48: the destinations and 4 KiB on both sides byte for byte, the rest of
    RECV by device checksum in 1 MiB spans against the poison's, SEND's checksums unchanged"""
    import xg_oracle as O
    from sparse_synth import SPAN, SparsePlan
    far = (1 << 31) + 48
    rows = [(S, R, 4096 + 5, 8192 + 3, 4099, far, 4096, 3),
            (S, R, 65536 + 7, 65536 + 11, far, 4101, 4096, 3)]
    nbytes = 2 * far + 65536 + 4096 + 8192
    assert nbytes > 1 << 32
    plan = SparsePlan([[(S, so, R, do, n) for (_k, _j, so, do, n) in _blocks(rows)]], nbytes, nbytes, seed=5)
    cx = _ctx_env(xg)
    try:
        run = xg.VecPlace(cx, rows, [nbytes, nbytes, 0, 0, 0])
        try:
            for lo, v in plan.sources:
                run.regions.write(xg.BUF_SEND, lo, v.tobytes())
            send_before = xg.chk_spans(run, [(S, o, n) for o, n in plan.send_spans])
            assert run.run() > 0
            for w, (lo, hi) in enumerate(plan.windows):
                plan.check_window(w, np.frombuffer(run.regions.read(xg.BUF_RECV, lo, hi - lo), np.uint8))
            poison = {}
            for _o, n in plan.rest:
                if n not in poison:
                    poison[n] = O.chk64(np.full(n, POISON, np.uint8))
            assert len(plan.rest) > 4000 and SPAN in poison
            plan.check_rest(xg.chk_spans(run, [(R, o, n) for o, n in plan.rest]), lambda n: poison[n])
            assert xg.chk_spans(run, [(S, o, n) for o, n in plan.send_spans]) == send_before, "SEND was written"
        finally:
            run.close()
    finally:
        cx.close()


# ------------------------------------------------------------------ 7. exchange_wv on one GPU
P, A = 8, 3


@pytest.fixture(scope="module")
def ctx(xg):
    c = xg.Context(rank=0, nranks=1, device=0)
    yield c
    c.close()


def _np(raw):
    return np.frombuffer(raw, np.uint8)


class _Env:
    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("method", [1, 2, 3, 5])
def test_exchange_wv_on_one_gpu(xg, ctx, method):
    """P 8, A 3 over a make_vecs list, verify on: rc 0, no bad slot, no bad vec, copy_kernel_v ran; the
    whole destination equals place_cases.placed over the expansion, SEND is untouched, and the
    destination is byte-equal to what xg_exchange_w leaves for vecs_expand of the list; with
    XG_VEC_COPY=0 the same bytes arrive and no vec tile runs.  Then VecPlace alone: vec_check finds
    nothing, and names exactly the row whose placed byte was flipped"""
    vecs, dom = make_vecs(P, A, seed=800 + method)
    exts = py_expand(vecs)
    assert xg.vecs_expand(vecs) == exts
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, 3, rl, lens=xg.vecs_lens(vecs, P, A))
    a2m = s.direction == xg.A2M
    ndom = s.domain_bytes(1, 0, dom)
    ndense = s.region_bytes(1, 0, xg.BUF_SEND if a2m else xg.BUF_RECV)
    assert xg.vecs_check(vecs, P, A, dom, scatter=a2m) == (0, "")
    nsend, nrecv = (ndense, ndom) if a2m else (ndom, ndense)
    src, preset = payload(0, nsend, salt=method), payload(1, nrecv, salt=method)
    want = placed(s, 1, 0, exts, dom, lambda h: src, preset)
    reg = xg.Regions(ctx, [nsend, nrecv, 0, 0, 0])
    try:
        def fresh():
            reg.write(xg.BUF_SEND, 0, src.tobytes())
            reg.write(xg.BUF_RECV, 0, preset.tobytes())

        def judge(what):
            got = _np(reg.read(xg.BUF_RECV, 0, nrecv))
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, (method, what, "first differing byte of recv", int(diff[0]), len(diff))
            assert np.array_equal(_np(reg.read(xg.BUF_SEND, 0, nsend)), src), "send was written"
            return got

        fresh()
        rc, bad, bad_v, place_s, timers, err = xg.exchange_wv(ctx, method, P, A, vecs, dom, rl, 3,
                                                              reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
        assert (rc, bad, bad_v, err) == (0, 0, 0, ""), (rc, bad, bad_v, err)
        assert place_s > 0 and len(timers) == P and all(t.total_time > 0 for t in timers)
        rows, idx, rb = s.vec_rows(1, 0, vecs, dom)
        assert xg.vec_tiles() == xg.vec_rows_tiles(rows)[-1] > 0
        by_vec = judge("exchange_wv")
        fresh()
        rc, bad, bad_e, _ps, _tm, err = xg.exchange_w(ctx, method, P, A, xg.vecs_expand(vecs), dom, rl, 3,
                                                      reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
        assert (rc, bad, bad_e, err) == (0, 0, 0, "")
        assert np.array_equal(judge("exchange_w"), by_vec)
        fresh()
        with _Env(XG_VEC_COPY=0):
            rc, bad, bad_v, _ps, _tm, err = xg.exchange_wv(ctx, method, P, A, vecs, dom, rl, 3,
                                                           reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
        assert (rc, bad, bad_v, err) == (0, 0, 0, "") and xg.vec_tiles() == 0
        assert np.array_equal(judge("XG_VEC_COPY=0"), by_vec)
    finally:
        reg.close()
    # the placement alone, over a dense side of random bytes
    run = xg.VecPlace(ctx, rows, rb, vec_index=idx)
    try:
        assert (rb[0], rb[1]) == ((ndense, ndom) if a2m else (ndom, ndense)) and rb[2:] == [0, 0, 0]
        run.regions.write(xg.BUF_SEND, 0, payload(2, rb[0], salt=method).tobytes())
        assert run.run() > 0 and run.dispatches == 1
        assert xg.vec_check(run) == []
        assert xg.vec_check(run, batch=7) == []
        k = max(range(len(rows)), key=lambda i: rows[i][6] * rows[i][7])
        _sb, _db, _so, do, _ss, ds, n, c = rows[k]
        at = do + (c - 1) * (ds if c > 1 else 0) + n - 1        # the last byte of the row's last block
        byte = _np(run.regions.read(xg.BUF_RECV, at, 1))[0] ^ np.uint8(0x40)
        run.regions.write(xg.BUF_RECV, at, bytes([int(byte)]))
        assert xg.vec_check(run) == [idx[k]]
    finally:
        run.close()


def test_exchange_wv_long_blocks_go_by_the_expansion(xg, ctx):
    """a list whose mean block length is above kVecLenMax reports zero vec tiles (it went through
    xg_vecs_expand into xg_exchange_w) and places the same bytes; one of mean exactly kVecLenMax runs
    copy_kernel_v"""
    rl = xg.aggregator_list(P, A)
    for n, tiles in ((VEC_LEN_MAX + 1, False), (VEC_LEN_MAX, True)):
        vecs = [(r, a, r * 3 * (n + 9), n, n + 9, 3) for r in range(P) for a in range(A)]
        dom = [P * 3 * (n + 9)] * A
        s = xg.Schedule(1, P, A, 0, 3, rl, lens=xg.vecs_lens(vecs, P, A))
        nsend, nrecv = s.region_bytes(1, 0, xg.BUF_SEND), s.domain_bytes(1, 0, dom)
        src, preset = payload(0, nsend, salt=9), payload(1, nrecv, salt=9)
        reg = xg.Regions(ctx, [nsend, nrecv, 0, 0, 0])
        try:
            reg.write(xg.BUF_SEND, 0, src.tobytes())
            reg.write(xg.BUF_RECV, 0, preset.tobytes())
            rc, bad, bad_v, _ps, _tm, err = xg.exchange_wv(ctx, 1, P, A, vecs, dom, rl, 3, reg.ptr(0), reg.ptr(1))
            assert (rc, bad, bad_v, err) == (0, 0, 0, "")
            assert (xg.vec_tiles() > 0) == tiles
            want = placed(s, 1, 0, py_expand(vecs), dom, lambda h: src, preset)
            assert np.array_equal(_np(reg.read(xg.BUF_RECV, 0, nrecv)), want)
        finally:
            reg.close()


# ------------------------------------------------------------------ 8. refusals
def test_exchange_wv_refuses_a_bad_list(xg, ctx):
    """a scatter overlap (inside a vec, and between two), a block past its domain and a rank out of
    range: XG_EARG with the checker's words, nothing run (the destination keeps its bytes); the
    overlapping list is accepted for a collective read"""
    rl = xg.aggregator_list(P, A)
    dom = [4096] * A
    reg = xg.Regions(ctx, [8192, 3 * 4096, 0, 0, 0])
    try:
        before = reg.read(xg.BUF_RECV, 0, 3 * 4096)
        overlap = [(0, 0, 0, 100, 200, 3), (1, 0, 499, 10, 0, 1)]
        for vecs, word in ((overlap, "overlap"),
                           ([(0, 0, 0, 100, 99, 3)], "overlap"),
                           ([(0, 1, 0, 100, 1000, 5)], "past the domain end"),
                           ([(P, 0, 0, 1, 0, 1)], "out of range")):
            rc, _b, _v, _t, _tm, err = xg.exchange_wv(ctx, 1, P, A, vecs, dom, rl, 3, reg.ptr(0), reg.ptr(1))
            assert rc == xg.EARG and word in err, (rc, err)
            assert xg.vec_tiles() == 0
        assert reg.read(xg.BUF_RECV, 0, 3 * 4096) == before
        rc, bad, bad_v, _t, _tm, err = xg.exchange_wv(ctx, 2, P, A, overlap, dom, rl, 3, reg.ptr(1), reg.ptr(0))
        assert (rc, bad, bad_v, err) == (0, 0, 0, "")
    finally:
        reg.close()


def test_vecplace_refuses_rows_outside_their_regions(xg, ctx):
    """xg_vecplace_load hands the rows to the host builder first: a last block one byte past RECV is
    XG_EARG and nothing is launched"""
    with pytest.raises(xg.XGError):
        xg.VecPlace(ctx, [(S, R, 0, 4096 - 100 - 2 * 50 + 1, 100, 50, 100, 3)], [4096, 4096, 0, 0, 0])
    run = xg.VecPlace(ctx, [(S, R, 0, 4096 - 100 - 2 * 50, 100, 50, 100, 3)], [4096, 4096, 0, 0, 0])
    try:
        assert (run.tiles, run.dispatches) == (1, 1) and run.run() > 0
    finally:
        run.close()
    run = xg.VecPlace(ctx, [], [4096, 4096, 0, 0, 0])
    try:
        assert (run.tiles, run.dispatches) == (0, 0) and run.run() >= 0
    finally:
        run.close()


# ------------------------------------------------------------------ 9. two real ranks
def _vec_job(tmp_path, case, timeout=100):
    """two vec_worker.py processes over one RCCL communicator, started as test_gpu_place._place_job
    starts place_worker.py, each under a time limit of its own -> every rank's result lines"""
    from test_gpu_multirank import _env, _spawn, _wait_all
    G = 2
    tmp_path = pathlib.Path(tempfile.mkdtemp(prefix="job", dir=str(tmp_path)))
    worker = os.path.join(REPO, "tests", "vec_worker.py")
    procs = [_spawn(["timeout", "-k", "10", str(timeout - 5), sys.executable, "-u", worker, json.dumps(case)],
                    _env(tmp_path, RANK=r, WORLD_SIZE=G, LOCAL_RANK=r, XG_MR_DEADLINE=timeout - 15), None,
                    "rank%d" % r, tmp_path)
             for r in range(G)]
    outs = _wait_all(procs, timeout)
    failed = ["rank %d exit %d: %s" % (r, p.returncode, " | ".join(err.strip().splitlines()[-3:]))
              for r, ((p, _o, _e), (out, err)) in enumerate(zip(procs, outs)) if p.returncode]
    assert not failed, "\n".join(failed)
    rows = [[json.loads(x) for x in out.splitlines() if x.startswith("{")] for out, _err in outs]
    assert [r[0]["rank"] for r in rows] == list(range(G))
    return rows


@pytest.mark.parametrize("method", [1, 2])
def test_exchange_wv_as_two_rank_job(tmp_path, method):
    """the shape of the one-GPU test between two real ranks: both return 0 with no bad slot and no
    bad vec, each ran copy_kernel_v, and each rank's whole destination equals the numpy execution
    over both ranks' payloads.  Then a call where rank 1's list differs by one stride, and a call
    with a scatter overlap: both ranks return XG_EARG with their own messages and the job ends
    normally -- the outcomes asserted for xg_exchange_w"""
    rows = _vec_job(tmp_path, {"method": method, "P": P, "A": A, "c": 3, "seed": 900 + method})
    for r in rows:
        good, differ, overlap = r
        assert (good["rc"], good["bad"], good["bad_vecs"], good["err"], good["exact"]) == (0, 0, 0, "", True), good
        assert good["tiles"] > 0, good
        assert differ["rc"] == 3 and "different inputs" in differ["err"], differ
        if method == 1:
            assert overlap["rc"] == 3 and ("overlap" in overlap["err"] or "another GPU" in overlap["err"]), overlap
        else:
            assert overlap["rc"] == 0, overlap            # a gather may read a byte twice
    if method == 1:
        assert any("overlap" in r[2]["err"] for r in rows)
