"""Host set-up of one placement, the strided-run description against its flattened extent list.

Shape: configs[1]'s (P 32, A 14, method 1, one GPU), 1 MiB per (rank, aggregator) pair, the domains
striped over the ranks in runs of L bytes (profiles/extent_copy_ab.py's view).  Arm A describes it
as 448 vecs (one per pair; 896 when L does not divide the pair: the short last run is a vec of its
own) and times xg_vecs_check + xg_vecs_lens + xg_vec_rows_build; arm B flattens it to one xg_ext
per run and times xg_exts_check + xg_exts_lens + xg_place_plan_build.  Both build the same schedule
in between (not timed).  Host only, no GPU; the arms alternate REPS times, the median is reported,
with the bytes of the list and of the table each arm would upload (24 B per copy, 48 B per row).

usage: python profiles/vec_host_setup.py [out.txt]      (prints; also written to out.txt)
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
REPS = 5


def striped_exts(xg, L):
    import numpy as np
    per = -(-PAIR // L)
    k = np.arange(per, dtype=np.int64)
    ln = np.minimum(L, PAIR - k * L)
    dt = np.dtype([("rank", np.int32), ("agg", np.int32), ("off", np.int64), ("len", np.int64)])
    ex = np.empty(P * A * per, dt)
    i = 0
    for a in range(A):
        for r in range(P):
            v = ex[i:i + per]
            v["rank"], v["agg"], v["off"], v["len"] = r, a, (k * P + r) * L, ln
            i += per
    return (xg.Ext * len(ex)).from_buffer_copy(ex.tobytes()), len(ex), [per * P * L] * A


def striped_vecs(xg, L):
    per, vecs = -(-PAIR // L), []
    full, tail = PAIR // L, PAIR % L
    for a in range(A):
        for r in range(P):
            vecs.append(xg.Vec(r, a, r * L, L, P * L, full))
            if tail:
                vecs.append(xg.Vec(r, a, (full * P + r) * L, tail, 0, 1))
    return (xg.Vec * len(vecs))(*vecs), len(vecs), [per * P * L] * A


def main():
    xg = G.load_package().xg
    h = xg.host()
    rl = xg.aggregator_list(P, A)
    err = C.create_string_buffer(512)
    lines = ["host set-up of one placement, P %d A %d, %d B per pair, striped domains; median of %d, ms" % (P, A, PAIR, REPS),
             "%7s %9s %9s | %10s %10s %10s | %12s %12s" % ("L", "vecs", "extents", "A check", "A lens", "A rows",
                                                           "A list B", "A table B"),
             "%7s %9s %9s | %10s %10s %10s | %12s %12s" % ("", "", "", "B check", "B lens", "B plan", "B list B",
                                                           "B table B")]
    for L in LENS:
        va, nv, dom = striped_vecs(xg, L)
        ea, ne, dom_e = striped_exts(xg, L)
        assert dom == dom_e
        dm = (C.c_int64 * A)(*dom)
        lens_v, lens_e = (C.c_int64 * (P * A))(), (C.c_int64 * (P * A))()
        ta, tb = [[], [], []], [[], [], []]
        nrows = ncopy = 0
        for _ in range(REPS):
            t0 = time.perf_counter()
            assert h.xg_vecs_check(va, nv, P, A, dm, 1, err, 512) == 0, err.value
            t1 = time.perf_counter()
            assert h.xg_vecs_lens(va, nv, P, A, lens_v) == 0
            t2 = time.perf_counter()
            s = xg.Schedule(1, P, A, 0, C_SIZE, rl, lens=list(lens_v))
            rows = (xg.VRow * nv)()
            t3 = time.perf_counter()
            nrows = h.xg_vec_rows_build(s.handle, 1, 0, va, nv, dm, rows, None, None)
            t4 = time.perf_counter()
            for k, d in enumerate((t1 - t0, t2 - t1, t4 - t3)):
                ta[k].append(d * 1e3)
            t0 = time.perf_counter()
            assert h.xg_exts_check(ea, ne, P, A, dm, 1, err, 512) == 0, err.value
            t1 = time.perf_counter()
            assert h.xg_exts_lens(ea, ne, P, A, lens_e) == 0
            t2 = time.perf_counter()
            assert list(lens_e) == list(lens_v)
            t3 = time.perf_counter()
            pd = h.xg_place_plan_build(s.handle, 1, 0, ea, ne, dm)
            t4 = time.perf_counter()
            ncopy = pd.contents.ncopy
            h.xg_devplan_free(pd)
            for k, d in enumerate((t1 - t0, t2 - t1, t4 - t3)):
                tb[k].append(d * 1e3)
        assert nrows == nv and ncopy == ne
        lines.append("%7d %9d %9d | %10.3f %10.3f %10.3f | %12d %12d" % (L, nv, ne, *[S.median(x) for x in ta],
                                                                       nv * C.sizeof(xg.Vec), nrows * 48))
        lines.append("%7s %9s %9s | %10.3f %10.3f %10.3f | %12d %12d" % ("", "", "", *[S.median(x) for x in tb],
                                                                       ne * C.sizeof(xg.Ext), ncopy * 24))
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
