"""A/B of the placement step of a striped file view: copy_kernel_v over the vec list's rows (VecPlace:
one workgroup per tile of one row, every block by arithmetic) against the same placement through its
expansion (xg_vecs_expand -> xg_place_plan_build -> xg_plan_load: today's path, copy_kernel_x up to a
mean extent of 1 KiB, copy_kernel_s above), on the same build, same box, one MI355X.

Shape: configs[1]'s (P 32, A 14, method 1, one GPU), 1 MiB per (rank, aggregator) pair: 448 MiB per
launch at every L.  The domains are striped over the ranks: block k of rank r sits at (k * P + r) * L
of its aggregator's domain, L in LENS -- 448 vecs (896 where L does not divide the pair) against up
to 7.3 M extents.  Both arms are loaded once over regions of their own; then RUNS timed runs each,
the arms alternating run by run; a run's time is the device time between the clock stamps around
the launch (xg_vecplace_run / xg_plan_run).  Per L: median, p10-p90 and min-max of the device time
and TB/s of read + write for both arms, the verdict by bench.py's CHOICE_RULE (a median must beat
the other by more than the larger min-max spread of the two arms; otherwise a tie), and the wall
time of each arm's whole set-up (check, lens, rows or expansion + plan, load).  Last line: the
largest L of the table up to which the vec arm wins or ties -- what kVecLenMax follows.

usage: python profiles/vec_copy_ab.py [out.txt]      (prints; also written to out.txt)
"""
import ctypes as C
import os
import statistics as S
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as G      # noqa: E402

P, A, C_SIZE, PAIR = 32, 14, 200000000, 1 << 20
LENS = (64, 256, 1000, 1024, 4096, 16384, 65536)
RUNS, WARM = 200, 3


def striped_vecs(xg, L):
    per, vecs = -(-PAIR // L), []
    full, tail = PAIR // L, PAIR % L
    for a in range(A):
        for r in range(P):
            vecs.append(xg.Vec(r, a, r * L, L, P * L, full))
            if tail:
                vecs.append(xg.Vec(r, a, (full * P + r) * L, tail, 0, 1))
    return (xg.Vec * len(vecs))(*vecs), len(vecs), [per * P * L] * A


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def measure(xg, ctx, L):
    """-> ({arm: [device seconds]}, {arm: {set-up stage: wall seconds}}, (vecs, extents, tiles, kinds))"""
    h, d = xg.host(), xg.device()
    rl = xg.aggregator_list(P, A)
    err = C.create_string_buffer(512)
    va, nv, dom = striped_vecs(xg, L)
    dm = (C.c_int64 * A)(*dom)
    setup = {"vec": {}, "ext": {}}
    now = time.perf_counter
    # ---- the vec arm's set-up
    t = now()
    assert h.xg_vecs_check(va, nv, P, A, dm, 1, err, 512) == 0, err.value
    setup["vec"]["check"] = now() - t
    lens = (C.c_int64 * (P * A))()
    t = now()
    assert h.xg_vecs_lens(va, nv, P, A, lens) == 0
    setup["vec"]["lens"] = now() - t
    s = xg.Schedule(1, P, A, 0, C_SIZE, rl, lens=list(lens))
    rows, rb = (xg.VRow * nv)(), (C.c_int64 * xg.NBUF)()
    t = now()
    assert h.xg_vec_rows_build(s.handle, 1, 0, va, nv, dm, rows, None, rb) == nv
    setup["vec"]["rows"] = now() - t
    reg_v, reg_e, vp, plan, dp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), None
    out = {"vec": [], "ext": []}
    try:
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(reg_v)) == 0
        t = now()
        assert d.xg_vecplace_load(ctx.handle, reg_v, rows, nv, C.byref(vp)) == 0
        setup["vec"]["load"] = now() - t
        # ---- the expansion arm's: the caller flattens the view first
        t = now()
        ne = h.xg_vecs_expand(va, nv, None, 0)
        ea = (xg.Ext * ne)()
        assert h.xg_vecs_expand(va, nv, ea, ne) == ne
        setup["ext"]["expand"] = now() - t
        t = now()
        assert h.xg_exts_check(ea, ne, P, A, dm, 1, err, 512) == 0, err.value
        setup["ext"]["check"] = now() - t
        lens_e = (C.c_int64 * (P * A))()
        t = now()
        assert h.xg_exts_lens(ea, ne, P, A, lens_e) == 0
        setup["ext"]["lens"] = now() - t
        assert list(lens_e) == list(lens)
        t = now()
        dp = h.xg_place_plan_build(s.handle, 1, 0, ea, ne, dm)
        setup["ext"]["plan"] = now() - t
        assert dp and list(dp.contents.region_bytes) == list(rb)
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(reg_e)) == 0
        t = now()
        assert d.xg_plan_load(ctx.handle, reg_e, dp, C.byref(plan)) == 0
        setup["ext"]["load"] = now() - t
        kinds = (d.xg_plan_launches(plan), d.xg_plan_extent_launches(plan), d.xg_plan_shift_launches(plan))
        tiles = (d.xg_vecplace_tiles(vp), d.xg_vecplace_dispatches(vp))
        sec, done, post, wall = C.c_double(), (C.c_double * 1)(), (C.c_double * 1)(), C.c_double()
        for i in range(WARM + RUNS):                            # the arms alternate run by run
            assert d.xg_vecplace_run(vp, C.byref(sec)) == 0
            assert d.xg_plan_run(plan, done, post, C.byref(wall)) == 0
            if i >= WARM:
                out["vec"].append(sec.value)
                out["ext"].append(done[0])
    finally:
        if vp:
            d.xg_vecplace_free(vp)
        if plan:
            d.xg_plan_free(plan)
        for r in (reg_v, reg_e):
            if r:
                d.xg_regions_free(r)
        if dp:
            h.xg_devplan_free(dp)
    return out, setup, (nv, ne, tiles, kinds)


def verdict(a, b):
    """CHOICE_RULE between two arms' samples -> 'a', 'b' or 'tie'"""
    spread = max(max(a) - min(a), max(b) - min(b))
    ma, mb = S.median(a), S.median(b)
    return "a" if ma < mb - spread else "b" if mb < ma - spread else "tie"


def main():
    xg = G.load_package().xg
    nbytes = 2 * P * A * PAIR
    lines = ["placement launch, P %d A %d, %d MiB per launch, striped domains; %d runs per arm, alternating; device us"
             % (P, A, (P * A * PAIR) >> 20, RUNS),
             "vec = copy_kernel_v over the rows (VecPlace); ext = the expansion's placement plan (xg_plan_load)"]
    ctx = xg.Context(rank=0, nranks=1, device=0)
    best, open_ = 0, True
    try:
        for L in LENS:
            out, setup, (nv, ne, tiles, kinds) = measure(xg, ctx, L)
            v = verdict(out["vec"], out["ext"])
            word = {"a": "vec wins", "b": "ext wins", "tie": "tie"}[v]
            for arm in ("vec", "ext"):
                us = [x * 1e6 for x in out[arm]]
                what = ("%d vecs, %d tiles, %d dispatch" % (nv, tiles[0], tiles[1]) if arm == "vec" else
                        "%d extents, %d dispatch, copy_kernel_x %d copy_kernel_s %d" % ((ne,) + kinds))
                lines.append("L %6d %s  median %8.1f (p10 %8.1f p90 %8.1f, min %8.1f max %8.1f)  TB/s %.3f  | set-up ms %s "
                             "= %.2f  [%s]"
                             % (L, arm, S.median(us), pct(us, 0.1), pct(us, 0.9), min(us), max(us),
                                nbytes / S.median(out[arm]) / 1e12,
                                " ".join("%s %.2f" % (k, x * 1e3) for k, x in setup[arm].items()),
                                sum(setup[arm].values()) * 1e3, what))
            lines.append("L %6d verdict: %s (vec / ext median %.3f)" % (L, word, S.median(out["vec"]) / S.median(out["ext"])))
            print("\n".join(lines[-3:]), flush=True)
            if open_ and v != "b":
                best = L
            else:
                open_ = False
    finally:
        ctx.close()
    lines.append("the largest L up to which the vec arm wins or ties on device time: %d" % best)
    print(lines[-1])
    text = "\n".join(lines)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
