"""A/B/C of the placement step of a striped file view, three arms on the same build, same box, one
MI355X:
  views  copy_kernel_vv over the vec list's views (VecPlace with views: one workgroup per tile of one
         view, the tile dealt across the rows, k x L contiguous bytes per block index);
  rows   copy_kernel_v over the same rows (one workgroup per tile of one row: what xg_exchange_wv runs
         without XG_VEC_VIEWS);
  ext    the same placement through its expansion (xg_vecs_expand -> xg_place_plan_build ->
         xg_plan_load: copy_kernel_x up to a mean extent of 1 KiB, copy_kernel_s above).

Shape: profiles/vec_copy_ab.py's -- configs[1]'s (P 32, A 14, method 1, one GPU), 1 MiB per (rank,
aggregator) pair: 448 MiB per launch at every L, the domains striped over the ranks in runs of L.
All three arms are loaded once over regions of their own; then RUNS timed runs each, the arms
alternating run by run; a run's time is the device time between the clock stamps around the launch.
Per L: median (p10-p90) [min-max] of the device time and TB/s of read + write per arm, and the
verdict of every pair of arms by bench.py's CHOICE_RULE (a median must beat the other by more than the
larger min-max spread of the two arms; otherwise a tie).

usage: python profiles/vec_views_ab.py [outdir]     (prints; summary.txt and runs_L<L>.txt -- every
       run's device us, one line per run, the arms side by side -- are written to outdir)
"""
import ctypes as C
import os
import statistics as S
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as G      # noqa: E402
from vec_copy_ab import A, C_SIZE, P, PAIR, pct, striped_vecs, verdict      # noqa: E402

LENS = (64, 256, 1000, 1024, 4096)
RUNS, WARM = 200, 3
ARMS = ("views", "rows", "ext")


def measure(xg, ctx, L):
    """-> ({arm: [device seconds]}, {arm: what ran})"""
    h, d = xg.host(), xg.device()
    rl = xg.aggregator_list(P, A)
    err = C.create_string_buffer(512)
    va, nv, dom = striped_vecs(xg, L)
    dm = (C.c_int64 * A)(*dom)
    assert h.xg_vecs_check(va, nv, P, A, dm, 1, err, 512) == 0, err.value
    lens = (C.c_int64 * (P * A))()
    assert h.xg_vecs_lens(va, nv, P, A, lens) == 0
    s = xg.Schedule(1, P, A, 0, C_SIZE, rl, lens=list(lens))
    rows, rb = (xg.VRow * nv)(), (C.c_int64 * xg.NBUF)()
    assert h.xg_vec_rows_build(s.handle, 1, 0, va, nv, dm, rows, None, rb) == nv
    reg = {a: C.c_void_p() for a in ARMS}
    vp = {a: C.c_void_p() for a in ARMS[:2]}
    plan, dp = C.c_void_p(), None
    out = {a: [] for a in ARMS}
    try:
        for a in ARMS:
            assert d.xg_regions_alloc(ctx.handle, rb, C.byref(reg[a])) == 0
        assert d.xg_vecplace_load_views(ctx.handle, reg["views"], rows, nv, C.byref(vp["views"])) == 0
        assert d.xg_vecplace_load(ctx.handle, reg["rows"], rows, nv, C.byref(vp["rows"])) == 0
        ne = h.xg_vecs_expand(va, nv, None, 0)
        ea = (xg.Ext * ne)()
        assert h.xg_vecs_expand(va, nv, ea, ne) == ne
        dp = h.xg_place_plan_build(s.handle, 1, 0, ea, ne, dm)
        assert dp and list(dp.contents.region_bytes) == list(rb)
        assert d.xg_plan_load(ctx.handle, reg["ext"], dp, C.byref(plan)) == 0
        nviews = d.xg_vecplace_views(vp["views"])
        assert nviews > 0 and d.xg_vecplace_views(vp["rows"]) == 0
        what = {"views": "%d vecs, %d views of k > 1, %d tiles, %d dispatch"
                         % (nv, nviews, d.xg_vecplace_tiles(vp["views"]), d.xg_vecplace_dispatches(vp["views"])),
                "rows": "%d vecs, %d tiles, %d dispatch" % (nv, d.xg_vecplace_tiles(vp["rows"]), d.xg_vecplace_dispatches(vp["rows"])),
                "ext": "%d extents, %d dispatch, copy_kernel_x %d copy_kernel_s %d"
                       % (ne, d.xg_plan_launches(plan), d.xg_plan_extent_launches(plan), d.xg_plan_shift_launches(plan))}
        sec, done, post, wall = C.c_double(), (C.c_double * 1)(), (C.c_double * 1)(), C.c_double()
        for i in range(WARM + RUNS):                            # the arms alternate run by run
            t = {}
            for a in ARMS[:2]:
                assert d.xg_vecplace_run(vp[a], C.byref(sec)) == 0
                t[a] = sec.value
            assert d.xg_plan_run(plan, done, post, C.byref(wall)) == 0
            t["ext"] = done[0]
            if i >= WARM:
                for a in ARMS:
                    out[a].append(t[a])
    finally:
        for a in ARMS[:2]:
            if vp[a]:
                d.xg_vecplace_free(vp[a])
        if plan:
            d.xg_plan_free(plan)
        for a in ARMS:
            if reg[a]:
                d.xg_regions_free(reg[a])
        if dp:
            h.xg_devplan_free(dp)
    return out, what


def main():
    xg = G.load_package().xg
    outdir = sys.argv[1] if len(sys.argv) > 1 else None
    if outdir:
        os.makedirs(outdir, exist_ok=True)
    nbytes = 2 * P * A * PAIR
    lines = ["placement launch, P %d A %d, %d MiB per launch, striped domains; %d runs per arm, alternating; device us, "
             "median (p10-p90) [min-max]" % (P, A, (P * A * PAIR) >> 20, RUNS),
             "views = copy_kernel_vv over the views; rows = copy_kernel_v over the rows; ext = the expansion's placement plan"]
    ctx = xg.Context(rank=0, nranks=1, device=0)
    try:
        for L in LENS:
            out, what = measure(xg, ctx, L)
            first = len(lines)
            for arm in ARMS:
                us = [x * 1e6 for x in out[arm]]
                lines.append("L %5d %-5s  %8.1f (%8.1f - %8.1f) [%8.1f - %8.1f]  TB/s %.3f  [%s]"
                             % (L, arm, S.median(us), pct(us, 0.1), pct(us, 0.9), min(us), max(us),
                                nbytes / S.median(out[arm]) / 1e12, what[arm]))
            for a, b in (("views", "rows"), ("views", "ext"), ("rows", "ext")):
                v = verdict(out[a], out[b])
                lines.append("L %5d verdict %s / %s: %s (median ratio %.3f)"
                             % (L, a, b, {"a": a + " wins", "b": b + " wins", "tie": "tie"}[v],
                                S.median(out[a]) / S.median(out[b])))
            print("\n".join(lines[first:]), flush=True)
            if outdir:
                with open(os.path.join(outdir, "runs_L%d.txt" % L), "w") as f:
                    f.write("# device us per run: %s\n" % " ".join(ARMS))
                    for i in range(RUNS):
                        f.write(" ".join("%.2f" % (out[a][i] * 1e6) for a in ARMS) + "\n")
    finally:
        ctx.close()
    if outdir:
        with open(os.path.join(outdir, "summary.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
