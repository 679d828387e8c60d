"""GPU: placement of striped views in whole lines -- copy_kernel_vv (the view copy of csrc/kernels.h),
xg_vecplace_load_views around it (csrc/runtime/vecplace.hip) and xg_exchange_wv with XG_VEC_VIEWS=1.

The kernel is driven through VecPlace(views=True) over synthetic rows (seeded random SEND, poisoned
RECV) and judged over EVERY byte of RECV against numpy over the rows' blocks, so an overrun, a dropped
store or a disturbed neighbour all show; SEND must come back unchanged.  Every run asserts that views
were in fact formed -- the object's view count is the expected one and its workgroups are the host's
view tile count -- so a fall-back to single rows cannot pass.  Every table the GPU sees here is one
the host suite (test_vec_views.py) builds and walks without a GPU."""
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
from vec_cases import py_expand

pytestmark = pytest.mark.gpu

S, R = 0, 1
POISON = 0xA5
TB, TP = 32768, 256


def _odd(n):
    return n | 1


def jb_of(n, k):
    return max(1, min(TB // (k * n), TP // k))


class Layout:
    """views and rows laid one behind the other on both sides, every view behind a poisoned gap of at
    least 16 B on the striped side, the dense runs of its rows an odd gap of their own apart"""

    def __init__(self):
        self.rows, self.multi, self.a, self.b = [], 0, 16, 64        # a: the dense side's cursor, b: the striped side's

    def view(self, k, n, count, phase=0, gap=0, dst=True, dense_phase=3):
        """k rows of count blocks of n bytes: the striped side starts at `phase` of a 16-B cell, the
        rows n apart, the stride k * n + gap; the dense side packed per row (step n + an odd gap)"""
        step_d = _odd(n + 2)
        stride = k * n + gap
        b0 = ((self.b + 15) & ~15) + 16 + phase
        for i in range(k):
            a0 = ((self.a + 15) & ~15) + dense_phase + 2 * i + 1
            self.rows.append((S, R, a0, b0 + i * n, step_d, stride, n, count) if dst else
                             (S, R, b0 + i * n, a0, stride, step_d, n, count))
            self.a = a0 + (count - 1) * step_d + n
        self.b = b0 + (count - 1) * stride + k * n
        kmax = min(TP, max(1, TB // n))
        self.multi += (k // kmax + (k % kmax > 1)) if n <= TB else 0
        return self.rows[-k:]

    def sizes(self, dst=True):
        a, b = ((self.a + 15) & ~15) + 32, ((self.b + 15) & ~15) + 64
        return (a, b) if dst else (b, a)


def _blocks(rows):
    for k, (sb, db, so, do, ss, ds, n, c) in enumerate(rows):
        for j in range(c):
            yield k, j, so + j * (ss if c > 1 else 0), do + j * (ds if c > 1 else 0), n


def _expected(rows, send, recv_bytes):
    want = np.full(recv_bytes, POISON, np.uint8)
    for (_sb, _db, so, do, ss, ds, n, c) in rows:
        if c == 1:
            want[do:do + n] = send[so:so + n]
        else:
            j = np.arange(c, dtype=np.int64)[:, None]
            i = np.arange(n, dtype=np.int64)[None, :]
            want[(do + j * ds + i).ravel()] = send[(so + j * ss + i).ravel()]
    return want


def _run_views(xg, cx, rows, send_bytes, recv_bytes, seed, want_multi, launch_max=512 << 20, rows_too=False):
    """load by views, run once, compare every RECV byte with numpy over the rows' blocks (the poison
    between them included), SEND untouched; the object's views and tiles are the host's.  rows_too:
    the same rows by the row copy leave the same RECV.  -> (RECV, the host's ViewTables)"""
    send = np.random.default_rng(seed).integers(0, 256, send_bytes, dtype=np.uint8)
    want = _expected(rows, send, recv_bytes)
    host = xg.ViewTables(rows, [send_bytes, recv_bytes, 0, 0, 0], launch_max=launch_max)
    assert host.multi == want_multi > 0, (host.multi, want_multi)
    out = []
    for views in ([True, False] if rows_too else [True]):
        run = xg.VecPlace(cx, rows, [send_bytes, recv_bytes, 0, 0, 0], views=views)
        try:
            if views:
                assert run.views == want_multi, "the rows were not loaded as the expected views"
                assert (run.tiles, run.dispatches) == (host.tiles, host.dispatches)
            else:
                assert (run.views, run.tiles) == (0, xg.vec_rows_tiles(rows)[-1])
            run.regions.write(xg.BUF_SEND, 0, send.tobytes())
            assert run.run() > 0
            got = np.frombuffer(run.regions.read(xg.BUF_RECV, 0, recv_bytes), np.uint8)
            diff = np.flatnonzero(got != want)
            if diff.size:
                at = int(diff[0])
                near = min(_blocks(rows), key=lambda b: min(abs(at - b[3]), abs(at - b[3] - b[4])))
                pytest.fail("views=%s: %d bytes of RECV differ; the first is RECV[%d] = %#x, expected %#x; nearest block: "
                            "row %d block %d RECV[%d..%d)" % (views, diff.size, at, got[at], want[at], near[0], near[1],
                                                              near[3], near[3] + near[4]))
            back = np.frombuffer(run.regions.read(xg.BUF_SEND, 0, send_bytes), np.uint8)
            assert np.array_equal(back, send), "SEND was written"
            out.append(got)
        finally:
            run.close()
    if rows_too:
        assert np.array_equal(out[0], out[1])
    return out[0], host


# ------------------------------------------------------------------ 1. phases x lengths x widths
@pytest.mark.parametrize("striped", ["dst", "src"])
@pytest.mark.parametrize("variant", [0, 6])
def test_view_copy_phases_lengths_and_widths(xg, variant, striped):
    """views of k in 2, 3, 5, 16, 17 rows x blocks of 1, 7, 15, 16, 17, 33, 64, 100, 1000 bytes,
    3 x jb + 1 blocks a row (three full tiles and one of a single block index), the striped side at
    all 16 start phases with strides of k x len + 0, 5 and 10, every row's dense run at an odd offset
    of its own, in ONE launch of copy_kernel_vv, plain and non-temporal, dst-striped and src-striped:
    every RECV byte equals numpy's, every gap keeps its poison"""
    dst = striped == "dst"
    lay = Layout()
    nviews = 0
    for k in (2, 3, 5, 16, 17):
        for n in (1, 7, 15, 16, 17, 33, 64, 100, 1000):
            for ph in range(16):
                rows = lay.view(k, n, 3 * jb_of(n, k) + 1, phase=ph, gap=5 * (ph % 3), dst=dst, dense_phase=ph ^ 5)
                assert rows[0][3 if dst else 2] % 16 == ph
                nviews += 1
    send_bytes, recv_bytes = lay.sizes(dst)
    assert lay.multi == nviews == 720
    cx = _ctx_env(xg, **({"XG_COPY_VARIANT": variant} if variant else {}))
    try:
        _got, host = _run_views(xg, cx, lay.rows, send_bytes, recv_bytes, 20 + variant, nviews)
        assert host.dispatches == 1 and host.tiles == 4 * nviews
        kinds = {v[3] for v in host.records()["view"]}
        assert kinds == {xg.VIEW_DST_STRIPED if dst else xg.VIEW_SRC_STRIPED}
    finally:
        cx.close()


# ------------------------------------------------------------------ 2. tile and split edges
def test_view_copy_tile_and_split_edges(xg):
    """16-B blocks: views of 255 and 256 rows (a tile is one block index of every row), 257 rows
    (256 + 1), 300 rows of 5 blocks (256 + 44), and 4 rows of 1, 63, 64, 65 and 257 blocks (jb = 64:
    the last tile empty but for one block index, exactly full, one over) -- at seeded phases, one
    launch, against numpy and against the row copy"""
    rng = np.random.default_rng(3)
    lay = Layout()
    ph = lambda: int(rng.integers(0, 16))
    lay.view(255, 16, 7, ph(), 3)
    lay.view(256, 16, 8, ph(), 0)
    lay.view(257, 16, 9, ph(), 1)
    lay.view(300, 16, 5, ph(), 7)
    for c in (1, 63, 64, 65, 257):
        lay.view(4, 16, c, ph(), 16 * (c % 2))
    assert lay.multi == 1 + 1 + 1 + 2 + 5 and jb_of(16, 4) == 64
    send_bytes, recv_bytes = lay.sizes()
    cx = _ctx_env(xg)
    try:
        _got, host = _run_views(xg, cx, lay.rows, send_bytes, recv_bytes, 41, lay.multi, rows_too=True)
        ks = sorted(v[1] for v in host.records()["view"])
        assert ks == [1, 4, 4, 4, 4, 4, 44, 255, 256, 256, 256]
    finally:
        cx.close()


# ------------------------------------------------------------------ 3. gaps and no gaps
@pytest.mark.parametrize("gap", [0, 5])
def test_view_copy_shared_cells(xg, gap):
    """4000 blocks of 7 B in each of 3 rows: with stride == k x len the destination is one packed
    interval, every 16-B cell shared between the rows of one tile and, at tile ends, between
    workgroups; with stride == k x len + 5 the 5 bytes keep their poison.  The bytes before the first
    block and after the last are intact"""
    k, n, c = 3, 7, 4000
    stride = k * n + gap
    rows = [(S, R, 5 + i * (c * (n + 2) + 9), 37 + i * n, n + 2, stride, n, c) for i in range(k)]
    end = 37 + (c - 1) * stride + k * n
    send_bytes, recv_bytes = 5 + k * (c * (n + 2) + 9) + 32, ((end + 15) & ~15) + 48
    cx = _ctx_env(xg)
    try:
        got, host = _run_views(xg, cx, rows, send_bytes, recv_bytes, 31 + gap, 1, rows_too=True)
        assert host.tiles == -(-c // jb_of(n, k)) > 40
        assert (got[:37] == POISON).all() and (got[end:] == POISON).all()
        if gap:
            body = got[37:37 + (c - 1) * stride].reshape(c - 1, stride)
            assert (body[:, k * n:] == POISON).all()
        else:
            assert not (got[37:end] == POISON).all()
    finally:
        cx.close()


# ------------------------------------------------------------------ 4. a mixed launch
def test_view_copy_mixed_launch(xg):
    """views, single rows and 3 blocks of 100 000 B in one launch, about 700 views through the
    search over tile0; the list's first and last rows are one block of one byte; against numpy and
    against the row copy"""
    rng = np.random.default_rng(11)
    lay = Layout()
    r = lambda lo, hi: int(rng.integers(lo, hi))
    lay.view(1, 1, 1, 9)
    for i in range(698):
        if i == 350:
            lay.view(1, 100000, 3, r(0, 16))
        elif i % 100 == 50:
            lay.view(r(2, 9), 16, 256 * r(20, 40) + 7, r(0, 16))
        elif i % 3 == 0:
            lay.view(1, r(1, 300), r(1, 60), r(0, 16), gap=r(1, 40))
        else:
            lay.view(r(2, 20), r(1, 120), r(1, 120), r(0, 16), gap=r(0, 3) * 5)
    lay.view(1, 1, 1, 15)
    assert lay.rows[0][6:] == (1, 1) and lay.rows[-1][6:] == (1, 1)
    send_bytes, recv_bytes = lay.sizes()
    cx = _ctx_env(xg)
    try:
        _got, host = _run_views(xg, cx, lay.rows, send_bytes, recv_bytes, 61, lay.multi, rows_too=True)
        assert host.views == 700 and 400 < host.multi < 500 and host.dispatches == 1
        assert xg.view_tiles(100000, 3, 1) == 12
    finally:
        cx.close()


# ------------------------------------------------------------------ 5. dispatch cuts
def test_view_copy_dispatch_cuts(xg):
    """about 1 MiB with XG_COPY_LAUNCH_MAX = 256 KiB: at least 3 dispatches of one launch, a cut
    inside a view of several rows, the runtime's dispatches the host's, `base` applied in every
    dispatch (every byte delivered once, nothing else written)"""
    lay = Layout()
    lay.view(1, 33, 700, 2)
    lay.view(8, 64, 1024, 3)
    lay.view(3, 1000, 100, 7, gap=7)
    lay.view(1, 100000, 3, 9)
    send_bytes, recv_bytes = lay.sizes()
    cap = 256 << 10
    assert 900 << 10 < sum(r[6] * r[7] for r in lay.rows) < 1300 << 10
    cx = _ctx_env(xg, XG_COPY_LAUNCH_MAX=cap)
    try:
        _got, host = _run_views(xg, cx, lay.rows, send_bytes, recv_bytes, 51, 2, launch_max=cap)
        cuts, rec = host.cuts(), host.records()
        inside = [c for c in cuts[1:-1] if c not in rec["tile0"]]
        assert len(cuts) - 1 >= 3 and inside, cuts
        v = max(i for i, t0 in enumerate(rec["tile0"]) if t0 <= inside[0])
        assert rec["view"][v][1] > 1, "the cut lies in a single row"
    finally:
        cx.close()


# ------------------------------------------------------------------ 6. 64-bit offsets
def test_view_copy_offsets_past_2_to_31(xg):
    """a view of 2 rows of 3 blocks of 4 KiB with dst_step = 2^31 + 48 in a RECV region just over
    4 GiB: the destinations and 4 KiB on both sides byte for byte, the rest of RECV by device checksum
    in 1 MiB spans against the poison's, SEND's checksums unchanged"""
    import xg_oracle as O
    from sparse_synth import SPAN, SparsePlan
    far = (1 << 31) + 48
    rows = [(S, R, 4096 + 5, 8192 + 3, 4099, far, 4096, 3),
            (S, R, 65536 + 7, 8192 + 3 + 4096, 4099, far, 4096, 3)]
    nbytes = 2 * far + 65536 + 4096 + 8192
    assert nbytes > 1 << 32
    host = xg.ViewTables(rows, [nbytes, nbytes, 0, 0, 0])
    assert (host.multi, host.views, host.tiles) == (1, 1, 1) and xg.vec_rows_tiles(rows)[-1] == 2
    plan = SparsePlan([[(S, so, R, do, n) for (_k, _j, so, do, n) in _blocks(rows)]], nbytes, nbytes, seed=5)
    cx = _ctx_env(xg)
    try:
        run = xg.VecPlace(cx, rows, [nbytes, nbytes, 0, 0, 0], views=True)
        try:
            assert (run.views, run.tiles) == (1, 1)
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


@pytest.mark.parametrize("L", [64, 100])
@pytest.mark.parametrize("method", [1, 2])
def test_exchange_wv_by_views_on_one_gpu(xg, ctx, method, L):
    """P 8, A 3, every aggregator's domain striped over the ranks in runs of L, rank-major, verify on.
    Without the knob: rc 0, nothing bad, no view, the row tables' tile count, as before.  With
    XG_VEC_VIEWS=1 (and with =0: off): rc 0, no bad slot, no bad vec, one view per aggregator, the
    host's view tile count, the destination byte-equal to the run without the knob and to
    place_cases.placed over the expansion, SEND untouched"""
    count = 61
    vecs = [(r, a, r * L, L, P * L, count) for r in range(P) for a in range(A)]
    dom = [P * L * count] * A
    exts = py_expand(vecs)
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, 3, rl, lens=xg.vecs_lens(vecs, P, A))
    a2m = s.direction == xg.A2M
    assert a2m == (method == 1)
    ndom = s.domain_bytes(1, 0, dom)
    ndense = s.region_bytes(1, 0, xg.BUF_SEND if a2m else xg.BUF_RECV)
    nsend, nrecv = (ndense, ndom) if a2m else (ndom, ndense)
    src, preset = payload(0, nsend, salt=method), payload(1, nrecv, salt=method)
    want = placed(s, 1, 0, exts, dom, lambda h: src, preset)
    rows, _idx, rb = s.vec_rows(1, 0, vecs, dom)
    host = xg.ViewTables(rows, rb)
    assert host.multi == A and host.views == A and host.tiles < xg.vec_rows_tiles(rows)[-1]
    reg = xg.Regions(ctx, [nsend, nrecv, 0, 0, 0])
    try:
        def once(**env):
            reg.write(xg.BUF_SEND, 0, src.tobytes())
            reg.write(xg.BUF_RECV, 0, preset.tobytes())
            with _Env(**env):
                rc, bad, bad_v, place_s, _tm, err = xg.exchange_wv(ctx, method, P, A, vecs, dom, rl, 3,
                                                                   reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
            assert (rc, bad, bad_v, err) == (0, 0, 0, ""), (env, rc, bad, bad_v, err)
            assert place_s > 0
            assert np.array_equal(_np(reg.read(xg.BUF_SEND, 0, nsend)), src), "send was written"
            return _np(reg.read(xg.BUF_RECV, 0, nrecv)).copy(), xg.vec_tiles(), xg.exchange_wv_views()

        plain, tiles, views = once()
        assert (tiles, views) == (xg.vec_rows_tiles(rows)[-1], 0)
        assert np.array_equal(plain, want)
        got, tiles, views = once(XG_VEC_VIEWS=1)
        assert views == A > 0 and tiles == host.tiles
        assert np.array_equal(got, plain)
        off, tiles, views = once(XG_VEC_VIEWS=0)
        assert (tiles, views) == (xg.vec_rows_tiles(rows)[-1], 0) and np.array_equal(off, plain)
    finally:
        reg.close()


# ------------------------------------------------------------------ 8. two real ranks
def test_exchange_wv_by_views_as_two_rank_job(tmp_path):
    """the one-GPU test between two real ranks with XG_VEC_VIEWS=1, started as
    test_gpu_vec.py::test_exchange_wv_as_two_rank_job starts its children (fresh processes, each under
    a time limit of its own): both return 0 with no bad slot and no bad vec, each placed its rows as
    the views and the view tiles the host gives for them, and each rank's whole destination equals the
    numpy execution over both ranks' payloads"""
    from test_gpu_multirank import _env, _spawn, _wait_all
    G, timeout = 2, 100
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="job", dir=str(tmp_path)))
    worker = os.path.join(REPO, "tests", "vec_views_worker.py")
    case = {"method": 1, "P": P, "A": A, "c": 3, "L": 64, "count": 61}
    procs = [_spawn(["timeout", "-k", "10", str(timeout - 5), sys.executable, "-u", worker, json.dumps(case)],
                    _env(tmp, RANK=r, WORLD_SIZE=G, LOCAL_RANK=r, XG_MR_DEADLINE=timeout - 15, XG_VEC_VIEWS=1), None,
                    "rank%d" % r, tmp)
             for r in range(G)]
    outs = _wait_all(procs, timeout)
    failed = ["rank %d exit %d: %s" % (r, p.returncode, " | ".join(err.strip().splitlines()[-3:]))
              for r, ((p, _o, _e), (_out, err)) in enumerate(zip(procs, outs)) if p.returncode]
    assert not failed, "\n".join(failed)
    rows = [[json.loads(x) for x in out.splitlines() if x.startswith("{")] for out, _err in outs]
    assert [r[0]["rank"] for r in rows] == list(range(G))
    for (r,) in rows:
        assert (r["rc"], r["bad"], r["bad_vecs"], r["err"], r["exact"]) == (0, 0, 0, "", True), r
        assert r["views"] == r["host_views"] > 0 and r["tiles"] == r["host_tiles"] < r["row_tiles"], r
    assert sum(r[0]["views"] for r in rows) == A
