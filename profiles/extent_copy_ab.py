"""A/B of the placement step's copy: copy_kernel_x, one workgroup per tile of extents
(XG_EXTENT_COPY=1), against copy_kernel_s, one workgroup per extent (XG_EXTENT_COPY=0: what a
placement plan ran before copy_kernel_x existed), on the same plan, same box, one MI355X.

Shape: configs[1]'s (P 32, A 14, method 1, one GPU), PAIR bytes per (rank, aggregator) pair
(1 MiB: 448 MiB per launch).  The domains are striped over the ranks: extent k of rank r sits at
(k * P + r) * L of its aggregator's domain, L in LENS -- 1000 puts every phase in play.  At L = 64
the pair is 256 KiB (112 MiB per launch, 1.8 M extents): the full size is 7.3 M descriptors.
Per setting a fresh context (the knobs are read at xg_init; XG_EXTENT_MEAN_MAX is lifted so that
copy_kernel_x runs at every L); the placement plan runs under a per-launch kernel-timing session
(xg_ktime mode 1) LAUNCHES times; the settings alternate PASSES times.  Reported per (L, setting):
launches, median / p10 / p90 of the launch time (us) and of TB/s of read + write, beside the gather
ceiling (5.96-5.99 TB/s, profiles/r04/gather_ab/summary.txt).  Then the tile's byte cap
(XG_EXTENT_TILE_KIB 8 / 16 / 32) at L = 256 and 1024.

usage: python profiles/extent_copy_ab.py [out.txt]      (prints; also written to out.txt)
"""
import ctypes as C
import os
import statistics as S
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as G      # noqa: E402

P, A, C_SIZE, PAIR = 32, 14, 200000000, 1 << 20
LENS = (64, 256, 1000, 1024, 4096, 16384, 65536)
LAUNCHES, PASSES = 100, 2
CEIL = (5.96, 5.99)


def striped(xg, L, pair):
    """-> (Ext array, n, dom_bytes): per pair ceil(pair / L) extents (the last one short when L does
    not divide the pair), extent k of rank r at (k * P + r) * L of aggregator a's domain"""
    import numpy as np
    per = -(-pair // L)
    k = np.arange(per, dtype=np.int64)
    ln = np.minimum(L, pair - k * L)
    dt = np.dtype([("rank", np.int32), ("agg", np.int32), ("off", np.int64), ("len", np.int64)])
    ex = np.empty(P * A * per, dt)
    i = 0
    for a in range(A):
        for r in range(P):
            v = ex[i:i + per]
            v["rank"], v["agg"], v["off"], v["len"] = r, a, (k * P + r) * L, ln
            i += per
    arr = (xg.Ext * len(ex)).from_buffer_copy(ex.tobytes())
    return arr, len(ex), [per * P * L] * A


def measure(xg, env, L, pair):
    """-> per-launch (us, TB/s) of LAUNCHES placement launches, (extent, shift) launches per run"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        ctx = xg.Context(rank=0, nranks=1, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    h, d = xg.host(), xg.device()
    out = []
    try:
        rl = xg.aggregator_list(P, A)
        arr, n, dom = striped(xg, L, pair)
        s = xg.Schedule(1, P, A, 0, C_SIZE, rl, lens=[pair] * (P * A))
        dp = h.xg_place_plan_build(s.handle, 1, 0, arr, n, (C.c_int64 * A)(*dom))
        assert dp, "xg_place_plan_build"
        reg, plan = C.c_void_p(), C.c_void_p()
        try:
            assert d.xg_regions_alloc(ctx.handle, dp.contents.region_bytes, C.byref(reg)) == 0
            assert d.xg_plan_load(ctx.handle, reg, dp, C.byref(plan)) == 0
            kinds = (d.xg_plan_extent_launches(plan), d.xg_plan_shift_launches(plan))
            assert d.xg_plan_launches(plan) == 1, "the placement step must be one dispatch"
            done, post, wall = (C.c_double * 1)(), (C.c_double * 1)(), C.c_double()
            for _ in range(3):                                       # warm-up: first touch of the regions
                assert d.xg_plan_run(plan, done, post, C.byref(wall)) == 0
            ctx.ktime_begin(LAUNCHES + 8, per_launch=True)
            for _ in range(LAUNCHES):
                assert d.xg_plan_run(plan, done, post, C.byref(wall)) == 0
            _ms, nl, _b = ctx.ktime_end()
            for ms, b in ctx.ktime_launches(nl):
                if ms > 0 and b > 0:
                    out.append((ms * 1e3, b / (ms * 1e-3) / 1e12))
        finally:
            if plan:
                d.xg_plan_free(plan)
            if reg:
                d.xg_regions_free(reg)
            h.xg_devplan_free(dp)
    finally:
        ctx.close()
    return out, kinds


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def row(name, rows, kinds):
    us, tb = [r[0] for r in rows], [r[1] for r in rows]
    return ("%-34s launches %4d  us/launch median %9.1f (p10 %9.1f p90 %9.1f)  TB/s median %.3f (p10 %.3f p90 %.3f)"
            "  = %.1f %% of the %.2f TB/s gather ceiling  [copy_kernel_x %d, copy_kernel_s %d]"
            % (name, len(us), S.median(us), pct(us, 0.1), pct(us, 0.9), S.median(tb), pct(tb, 0.1), pct(tb, 0.9),
               100 * S.median(tb) / CEIL[1], CEIL[1], kinds[0], kinds[1]))


def main():
    xg = G.load_package().xg
    base = {"XG_ENGINE_MAX_STEP": 0, "XG_EXTENT_MEAN_MAX": 1 << 30}
    lines = ["placement launch, P %d A %d, striped domains; XG_EXTENT_COPY=1: copy_kernel_x, =0: copy_kernel_s" % (P, A)]
    lens = [int(x) for x in os.environ.get("EXTENT_AB_LENS", "").split(",") if x] or LENS
    for L in lens:
        pair = PAIR // 4 if L < 256 else PAIR
        got, kinds = {1: [], 0: []}, {}
        for _ in range(PASSES):
            for setting in (1, 0):
                rows, kinds[setting] = measure(xg, dict(base, XG_EXTENT_COPY=setting), L, pair)
                got[setting] += rows
        for setting in (1, 0):
            lines.append(row("L %6d (%3d MiB) XG_EXTENT_COPY=%d" % (L, (P * A * pair) >> 20, setting), got[setting],
                             kinds[setting]))
        print("\n".join(lines[-2:]), flush=True)
    if not os.environ.get("EXTENT_AB_LENS"):
        for L in (256, 1024):
            for kib in (8, 16, 32):
                rows, kinds = [], None
                for _ in range(PASSES):
                    r, kinds = measure(xg, dict(base, XG_EXTENT_COPY=1, XG_EXTENT_TILE_KIB=kib), L, PAIR)
                    rows += r
                lines.append(row("L %6d tile %2d KiB" % (L, kib), rows, kinds))
                print(lines[-1], flush=True)
    text = "\n".join(lines)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
