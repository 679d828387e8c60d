"""Ragged schedules (xg_sched_build_v, include/xg_sched.h): a length per (rank, aggregator) pair.

CPU only.  A uniform matrix must BE the old schedule (messages byte for byte, steps, traces, layout,
device plans); a ragged one must carry every pair's own length at prefix-sum offsets, deliver
exactly the bytes a numpy loop over xg_deliveries delivers when its device plans are executed on
numpy regions (plan_exec's executor, with a payload of random bytes in place of the fingerprint
fill, which knows one d only), pair its RCCL calls in every pack form, and keep the eager rule per
message.
"""
import ctypes as C

import numpy as np
import pytest

import plan_exec
from conftest import golden_configs, load_golden

CONFIGS = golden_configs()
RAGGED_METHODS = list(range(1, 15)) + [17, 18, 19, 20]
FORMS = (0, 1, 2, 3)          # XG_PACK_TWO_SIDED, XG_PACK_ONE_SIDED, XG_RELAY, XG_RELAY_COALESCED


def _raw_msgs(xg, s):
    h = xg.host()
    n = h.xg_sched_nmsg(s.handle)
    return n, C.string_at(h.xg_sched_msgs(s.handle), n * C.sizeof(xg.Msg))


def _plan_tuple(v):
    return (v.flags, v.region_bytes, v.copies, v.p2p, v.steps, v.sync_after, v.stage_count, v.posts,
            v.local_bytes, v.remote_send_bytes, v.remote_recv_bytes)


# ------------------------------------------------------------------ uniform identity
@pytest.mark.parametrize("cfg", CONFIGS)
def test_uniform_matrix_is_the_old_schedule(xg, cfg):
    """every golden configuration x methods 1..20: xg_sched_build_v with a constant matrix equals
    xg_sched_build_iter -- the xg_msg array byte for byte, nsteps, the traces of the first and the
    last rank, xg_region_bytes, and the device plans (copies, p2p lists, step plans) at G = 1, 2, 3
    with flags == 0; a configuration the old builder refuses is refused with the same words"""
    meta, _, _ = load_golden(cfg)
    P, A, d, c, rl = meta["P"], meta["A"], meta["d"], meta["c"], meta["aggregators"]
    kw = dict(ntimes=meta["ntimes"], proc_node=meta["proc_node"], barrier_type=meta["barrier"], iteration=1)
    for m in range(1, 21):
        try:
            old = xg.Schedule(m, P, A, d, c, rl, **kw)
        except xg.XGError as e:
            with pytest.raises(xg.XGError) as ei:
                xg.Schedule(m, P, A, 0, c, rl, lens=[d] * (P * A), **kw)
            assert str(ei.value) == str(e), (cfg, m)
            continue
        new = xg.Schedule(m, P, A, 0, c, rl, lens=[d] * (P * A), **kw)
        assert not new.ragged and not old.ragged
        assert _raw_msgs(xg, new) == _raw_msgs(xg, old), (cfg, m)
        assert new.nsteps == old.nsteps
        for r in (0, P - 1):
            assert new.trace(r) == old.trace(r), (cfg, m, r)
        for G in (1, 2, 3):
            for g in range(G):
                for buf in range(xg.NBUF):
                    assert new.region_bytes(G, g, buf) == old.region_bytes(G, g, buf), (cfg, m, G, g, buf)
                a, b = new.devplan(G, g), old.devplan(G, g)
                assert a.flags == 0 and b.flags == 0
                assert _plan_tuple(a) == _plan_tuple(b), (cfg, m, G, g)
        assert new.delivery_lens(2) == [d] * len(old.deliveries(2))


# ------------------------------------------------------------------ ragged layout
P7, A3 = 7, 3


def _lens_p7():
    rng = np.random.default_rng(7)
    lens = [int(x) for x in rng.integers(0, 5001, P7 * A3)]
    for k in (0, 4, 11, 20):           # several empty segments, the first and the last pair among them
        lens[k] = 0
    return lens


def _sched(xg, m, lens=None, c=2, ntimes=2, P=P7, A=A3, **kw):
    lens = _lens_p7() if lens is None else lens
    return xg.Schedule(m, P, A, 0, c, xg.aggregator_list(P, A), ntimes=ntimes, lens=lens, **kw)


@pytest.mark.parametrize("method", RAGGED_METHODS)
def test_ragged_layout(xg, method):
    """P 7, A 3, seeded lengths in 0..5000 with several zeros: every data message's len, soff and
    doff are the matrix entry and its prefix sums; xg_deliveries has P x A entries whose receive
    intervals (xg_delivery_lens) are disjoint and tile each GPU's RECV region exactly, whose send
    intervals tile SEND; region bytes are the row and column sums"""
    lens = _lens_p7()
    L = np.array(lens, dtype=np.int64).reshape(P7, A3)
    s = _sched(xg, method, lens)
    assert s.ragged
    rl = s.rank_list
    a2m = s.direction == xg.A2M
    seen = set()
    for (src, sseg, dst, dslot, ln, _step, fl), (sb, so, db, do) in zip(s.messages(), s.locations()):
        if sseg < 0:                   # 0-byte rounds (pairwise) and go-signals (m18)
            assert ln == 0
            continue
        r, a = (src, sseg) if a2m else (dst, dslot)
        assert (rl[a] == dst and dslot == src) if a2m else (rl[a] == src and sseg == dst), (method, src, dst)
        assert ln == L[r, a], (method, r, a)
        assert (sb, db) == (xg.BUF_SEND, xg.BUF_RECV)
        if a2m:
            assert so == L[r, :a].sum() and do == L[:r, a].sum(), (method, r, a)
        else:
            assert so == L[:r, a].sum() and do == L[r, :a].sum(), (method, r, a)
        assert so == s.seg_offset(src, sseg) and do == s.slot_offset(dst, dslot)
        seen.add((r, a))
    # every pair with bytes travels (Alltoallw and the scattered methods post nothing for an empty one)
    assert {(r, a) for r in range(P7) for a in range(A3) if L[r, a]} <= seen
    for G in (1, 2, 3, 4):
        dl, dn = s.deliveries(G), s.delivery_lens(G)
        assert len(dl) == P7 * A3 == len(dn)
        for g in range(G):
            lo, hi = s.block_range(G, g)
            aggs = [a for a in range(A3) if lo <= rl[a] < hi]
            rows, cols = int(L[lo:hi].sum()), int(L[:, aggs].sum())
            assert s.region_bytes(G, g, xg.BUF_SEND) == (rows if a2m else cols)
            assert s.region_bytes(G, g, xg.BUF_RECV) == (cols if a2m else rows)
            for side, buf in (("recv", xg.BUF_RECV), ("send", xg.BUF_SEND)):
                iv = sorted((getattr(q, side + "_off"), n) for q, n in zip(dl, dn)
                            if getattr(q, "dst_gpu" if side == "recv" else "src_gpu") == g and n)
                at = 0
                for off, n in iv:
                    assert off == at, (method, G, g, side, off, at)
                    at += n
                assert at == s.region_bytes(G, g, buf)
        for q, n in zip(dl, dn):
            r, a = (q.src, q.seed) if a2m else (q.dst, q.slot)
            assert n == L[r, a]


# ------------------------------------------------------------------ CPU execution
def _simulate(xg, s, G, pack, form, seed):
    """plan_exec.simulate with a random payload in SEND (make_regions fills d-byte fingerprints)"""
    views = [s.devplan(G, g, pack, 0, form) for g in range(G)]
    regs = []
    for g, v in enumerate(views):
        reg = [np.zeros(max(0, b), np.uint8) for b in v.region_bytes]
        reg[0][:] = np.random.default_rng(seed + g).integers(0, 256, reg[0].size, dtype=np.uint8)
        reg[1][:] = 0xA5
        regs.append(reg)
    sends = [r[0].copy() for r in regs]
    for st in range(views[0].nsteps):
        parts = [plan_exec.step_parts(v, st) for v in views]
        for g in range(G):
            plan_exec.copies(regs[g], parts[g][0], "stage")
            plan_exec.copies(regs[g], parts[g][1], "pre")
        for grp in sorted({o[5] for g in range(G) for o in parts[g][2]}):
            for g in range(G):
                ops = [o for o in parts[g][2] if o[5] == grp]
                plan_exec.check_races([(o[2], o[3], o[2], o[3], o[4]) if o[1] else (-1, 0, o[2], o[3], o[4])
                                       for o in ops], "p2p group %d" % grp)
            for g in range(G):
                for p in range(G):
                    if p == g:
                        continue
                    snd = [o for o in parts[g][2] if o[0] == p and o[1] and o[5] == grp]
                    rcv = [o for o in parts[p][2] if o[0] == g and not o[1] and o[5] == grp]
                    assert len(snd) == len(rcv), (st, grp, g, p)
                    for (_, _, sb, so, sl, _g), (_, _, rb, ro, rlen, _h) in zip(snd, rcv):
                        assert sl == rlen, (st, grp, g, p)
                        regs[p][rb][ro:ro + rlen] = regs[g][sb][so:so + sl]
        for g in range(G):
            plan_exec.copies(regs[g], parts[g][3], "post")
    return views, regs, sends


def _check_delivery(s, G, views, regs, sends, what):
    want = [np.full(v.region_bytes[1], 0xA5, np.uint8) for v in views]
    for q, n in zip(s.deliveries(G), s.delivery_lens(G)):
        want[q.dst_gpu][q.recv_off:q.recv_off + n] = sends[q.src_gpu][q.send_off:q.send_off + n]
    for g in range(G):
        assert np.array_equal(regs[g][0], sends[g]), (what, g, "SEND was written")
        diff = np.flatnonzero(regs[g][1] != want[g])
        assert diff.size == 0, (what, g, "first differing RECV byte", int(diff[0]))


@pytest.mark.parametrize("method", RAGGED_METHODS)
def test_ragged_plans_deliver_on_the_cpu(xg, method):
    """the ragged device plans of P 7, A 3 at G = 1..4, direct and in every pack form, executed
    launch by launch on numpy regions (races inside a launch checked): RECV is exactly what a
    numpy loop over xg_deliveries / xg_delivery_lens delivers, SEND is untouched, every plan has
    XG_DP_RAGGED, and xg_devplans_match accepts the job"""
    s = _sched(xg, method)
    for G in (1, 2, 3, 4):
        for pack, form in [(0, -1)] + [(1 << 20, f) for f in FORMS]:
            views, regs, sends = _simulate(xg, s, G, pack, form, seed=100 * method + G)
            assert all(v.flags == xg.DP_RAGGED for v in views)
            _check_delivery(s, G, views, regs, sends, (method, G, pack, form))
            if G > 1:
                xg.devplans_match(views)


def test_relay_forms_pair_or_refuse_on_large_ragged_messages(xg):
    """P 8, A 8, G 4, m9 with lengths 1 MiB + 1 .. 1 MiB + 4096: every cross-GPU message is above
    XG_RELAY_MIN_BYTES, so the relay forms engage (a second RCCL group appears) -- their 16-B
    aligned cuts are taken inside each message, whatever its phase; the calls pair, and the plans
    executed on numpy deliver every byte"""
    P = A = 8
    rng = np.random.default_rng(9)
    lens = [(1 << 20) + int(x) for x in rng.integers(1, 4097, P * A)]
    s = xg.Schedule(9, P, A, 0, 3, xg.aggregator_list(P, A), lens=lens)
    assert s.ragged
    for form in FORMS:
        views = [s.devplan(4, g, 1 << 20, 0, form) for g in range(4)]
        pairs = xg.devplans_match(views, groups=True)
        assert pairs
        if form in (xg.RELAY, xg.RELAY_COALESCED):
            assert any(p[1] == 1 for p in pairs), "the relay form did not engage at this shape"
    for form in (xg.RELAY, xg.RELAY_COALESCED):
        views, regs, sends = _simulate(xg, s, 4, 1 << 20, form, seed=form)
        _check_delivery(s, 4, views, regs, sends, ("relay", form))


# ------------------------------------------------------------------ eager rule
def _steps(s):
    return sorted((src, sseg, dst, dslot, step) for (src, sseg, dst, dslot, _n, step, _f) in s.messages())


@pytest.mark.parametrize("c", [1, 3])
def test_eager_rule_is_per_message(xg, c):
    """m7 (blocking sends), P 8, A 3, at c = 1 and at c = 3.  The step compiler reads a send's
    length only through `cnt * esz <= eager_limit` (sched.c, post_eager), so a ragged matrix whose
    every length is in 1..65424 (all eager) gives every message the step it has at uniform
    d = 65424, and one whose every length is above 65424 (none eager) the step it has at
    d = 65425.  At c = 1 a rank waits for its receives after every single send and the two
    uniform schedules have the same steps; at c = 3 they differ (2 steps against 6), so there the
    property tells the two apart."""
    P, A, lim = 8, 3, xg.MPICH_EAGER_LIMIT
    rl = xg.aggregator_list(P, A)
    rng = np.random.default_rng(65424)
    small = [int(x) for x in rng.integers(1, lim + 1, P * A)]
    small[0], small[-1] = lim, 1
    large = [int(x) for x in rng.integers(lim + 1, 3 * lim, P * A)]
    large[0] = lim + 1
    at = {d: xg.Schedule(7, P, A, d, c, rl, ntimes=2) for d in (lim, lim + 1)}
    assert (_steps(at[lim]) != _steps(at[lim + 1])) == (c == 3)
    for lens, d in ((small, lim), (large, lim + 1)):
        s = xg.Schedule(7, P, A, 0, c, rl, ntimes=2, lens=lens)
        assert s.ragged
        assert _steps(s) == _steps(at[d])
        assert s.nsteps == at[d].nsteps


# ------------------------------------------------------------------ refusals
def test_refusals(xg):
    """m15 / m16 with a matrix that is not uniform, a negative entry and a NULL matrix each return
    NULL with a message; a uniform matrix is accepted by m15 / m16"""
    P, A = 8, 3
    rl = xg.aggregator_list(P, A)
    lens = _lens_p7() + [5, 6, 7]
    for m in (15, 16):
        with pytest.raises(xg.XGError, match="TAM"):
            xg.Schedule(m, P, A, 0, 2, rl, lens=lens, proc_node=4)
        assert not xg.Schedule(m, P, A, 0, 2, rl, lens=[256] * (P * A), proc_node=4).ragged
    bad = list(lens)
    bad[5] = -1
    with pytest.raises(xg.XGError, match="negative length -1 for rank 1, aggregator index 2"):
        xg.Schedule(1, P, A, 0, 2, rl, lens=bad)
    h = xg.host()
    err = C.create_string_buffer(256)
    rla = (C.c_int * A)(*rl)
    assert not h.xg_sched_build_v(1, P, A, None, 2, rla, 1, 1, 0, xg.MPICH_EAGER_LIMIT, 0, err, 256)
    assert b"NULL" in err.value
    with pytest.raises(xg.XGError, match="entries"):
        xg.Schedule(1, P, A, 0, 2, rl, lens=lens[:-1])
