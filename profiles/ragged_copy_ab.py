"""A/B of the ragged exchange's copy: copy_kernel_s (XG_RAGGED_COPY=1) against copy_kernel_g's
realign path (XG_RAGGED_COPY=0) on the same plan, same box, one MI355X.

Shape: configs[1]'s (P 32, A 14, comm_size 200000000, methods 1-4, one GPU) with a ragged matrix
-- 1 MiB + a seeded offset in -65536..65536 at byte granularity -- and, as the side check, the
uniform 1 MiB schedule (no launch of it may change with the setting).  Per setting a fresh context
(XG_RAGGED_COPY is read at xg_init); per method the plan runs under a per-launch kernel-timing
session (xg_ktime mode 1) until it has at least LAUNCHES launches; the settings alternate PASSES
times.  Reported per (matrix, setting): launches, median / p10 / p90 of the kernel time per launch
(us) and of TB/s of read + write, the median's share of the 8 TB/s peak and of the 5.96-5.99 TB/s
gather ceiling (profiles/r04/gather_ab/summary.txt), and the copy_kernel_s launches per run.

usage: python profiles/ragged_copy_ab.py [out.txt]      (prints; also written to out.txt)
"""
import os
import statistics as S
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as G      # noqa: E402

P, A, C_SIZE, D = 32, 14, 200000000, 1 << 20
METHODS = (1, 2, 3, 4)
LAUNCHES, PASSES = 64, 2
PEAK, CEIL = 8.0, (5.96, 5.99)


def lens_ragged():
    import numpy as np
    off = np.random.default_rng(8).integers(-65536, 65537, P * A)
    return [D + int(x) for x in off]


def measure(xg, setting, lens):
    """-> (per-launch (us, TB/s) of every timed launch, copy_kernel_s launches per run of m1..m4)"""
    os.environ["XG_RAGGED_COPY"] = str(setting)
    ctx = xg.Context(rank=0, nranks=1, device=0)
    rl = xg.aggregator_list(P, A)
    out, shift = [], []
    try:
        for m in METHODS:
            s = xg.Schedule(m, P, A, D, C_SIZE, rl, lens=lens)
            run = xg.MethodRun(ctx, s, fill=False)
            try:
                shift.append(run.shift_launches())
                run.run_timed()                                  # warm-up: first touch of the regions
                reps = -(-LAUNCHES // max(1, run.launches))
                ctx.ktime_begin(reps * run.launches + 8, per_launch=True)
                for _ in range(reps):
                    run.run_timed()
                _ms, n, _b = ctx.ktime_end()
                for ms, b in ctx.ktime_launches(n):
                    if ms > 0 and b > 0:
                        out.append((ms * 1e3, b / (ms * 1e-3) / 1e12))
            finally:
                run.close()
    finally:
        ctx.close()
    return out, shift


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def main():
    xg = G.load_package().xg
    lines = []
    for name, lens in (("ragged 1 MiB +- 64 KiB", lens_ragged()), ("uniform 1 MiB", [D] * (P * A))):
        got = {1: [], 0: []}
        shifts = {}
        for _ in range(PASSES):
            for setting in (1, 0):
                rows, shifts[setting] = measure(xg, setting, lens)
                got[setting] += rows
        for setting in (1, 0):
            us, tb = [r[0] for r in got[setting]], [r[1] for r in got[setting]]
            med = S.median(tb)
            lines.append("%-24s XG_RAGGED_COPY=%d  launches %4d  us/launch median %7.1f (p10 %7.1f p90 %7.1f)  "
                         "TB/s median %.3f (p10 %.3f p90 %.3f)  = %.1f %% of %.0f TB/s, %.1f-%.1f %% of the gather "
                         "ceiling  shift launches per run m1-m4 %s"
                         % (name, setting, len(us), S.median(us), pct(us, 0.1), pct(us, 0.9), med, pct(tb, 0.1),
                            pct(tb, 0.9), 100 * med / PEAK, PEAK, 100 * med / CEIL[1], 100 * med / CEIL[0],
                            shifts[setting]))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
