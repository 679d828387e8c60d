"""Span checksum rate against this commit's xg_verify on the same bytes, and xg_exchange's
total_time beside xg_run_method's.  One MI355X, BASELINE configs[1] (P 32, A 14, d 1 MiB: 448
receive slots, 448 MiB read per call).

After a fingerprint-filled m1 run and a warm-up, xg_verify and xg_chk_spans are timed on the
same slots, alternating, REPS times each in one process: host clock around the C call, which
ends in a stream synchronise (so each figure is a CALL time: descriptor upload, the kernel, the
result copy -- the same kind of work in both).  Then the same for spans shifted by one byte
(off + 1, d - 1 bytes: every span starts at phase 1 of a 16-B granule).  Last, m1 through
xg_exchange (caller buffers, verify off) and xg_run_method, alternating: the largest total_time
over the 32 ranks of each call.

usage: python3 profiles/payload_chk_rate.py [out.txt]      (KERNELS_ONLY=1: skip the operators,
for a run under rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as G  # noqa: E402

xg = G.load_package().xg
PEAK = 8e12              # HBM3E peak of the MI355X, bytes/s
REPS = int(os.environ.get("REPS", "20"))
P, A, d, c = 32, 14, 1 << 20, 3
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def stats(ts, nbytes):
    med = statistics.median(ts)
    return "median %.1f us (min %.1f, max %.1f, spread %.1f %%)  %.0f GB/s = %.1f %% of 8 TB/s" % (
        med * 1e6, min(ts) * 1e6, max(ts) * 1e6, 100 * (max(ts) - min(ts)) / med, nbytes / med / 1e9,
        100 * nbytes / med / PEAK)


def main():
    dev = xg.device()
    ctx = xg.Context(rank=0, nranks=1, device=0)
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(1, P, A, d, c, rl)
    run = xg.MethodRun(ctx, s, mode=1)
    run.run_timed()
    ns = run.nslots
    chk, bad, _first = run.verify()
    assert not any(bad) and run.slot_chk() == chk
    say("configs[1]: P %d A %d d %d, m1: %d slots, %d MiB per call; %d repetitions, alternating" % (
        P, A, d, ns, ns * d >> 20, REPS))
    vchk, vbad = (C.c_uint64 * ns)(), (C.c_int64 * ns)()
    out = (C.c_uint64 * ns)()

    def spans(shift):
        return (xg.BufSpan * ns)(*[xg.BufSpan(xg.BUF_RECV, 0, off + shift, d - shift) for _s, _e, _d, off in run.slots])

    def t_verify():
        t0 = xg.now()
        assert dev.xg_verify(run._r, run._slots, ns, d, 0, 1, vchk, vbad, None) == 0
        return xg.now() - t0

    def t_spans(arr):
        t0 = xg.now()
        assert dev.xg_chk_spans(run._r, arr, ns, out) == 0
        return xg.now() - t0

    for shift, name in ((0, "aligned"), (1, "shifted by 1 byte")):
        arr = spans(shift)
        for _ in range(3):
            t_verify(), t_spans(arr)
        tv, tc = [], []
        for _ in range(REPS):
            tv.append(t_verify())
            tc.append(t_spans(arr))
        say("%s:" % name)
        say("  xg_verify    (verify_kernel, slots as they lie) %s" % stats(tv, ns * d))
        say("  xg_chk_spans (span_chk_kernel)                  %s" % stats(tc, ns * (d - shift)))
        say("  xg_chk_spans / xg_verify medians: %.3f" % (statistics.median(tc) / statistics.median(tv)))
    run.close()

    if not os.environ.get("KERNELS_ONLY"):
        dev.xg_run_method.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                      C.POINTER(xg.Timer), C.c_int, C.c_int, C.POINTER(xg.RunOpts),
                                      C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
        rb = s.devplan(1, 0).region_bytes
        arena = xg.Regions(ctx, [rb[0], rb[1], 0, 0, 0])
        o = xg.RunOpts()
        dev.xg_run_opts_default(C.byref(o))
        o.fingerprint = 1
        rla = (C.c_int * A)(*rl)
        timers = (xg.Timer * P)()
        err = C.create_string_buffer(512)

        def t_method():
            assert dev.xg_run_method(ctx.handle, 1, P, A, d, rla, c, timers, 0, 1, C.byref(o), None, err, 512) == 0
            return max(t.total_time for t in timers)

        def t_exchange():
            rc, _bad, tm, e = xg.exchange(ctx, 1, P, A, d, rl, c, arena.ptr(xg.BUF_SEND), arena.ptr(xg.BUF_RECV),
                                          verify=False)
            assert rc == 0, e
            return max(t.total_time for t in tm)

        for _ in range(2):
            t_method(), t_exchange()
        tm, te = [], []
        for _ in range(REPS):
            tm.append(t_method())
            te.append(t_exchange())
        moved = 2 * ns * d
        say("m1 total_time (largest over the ranks; %d MiB read + written):" % (moved >> 20))
        say("  xg_run_method %s" % stats(tm, moved))
        say("  xg_exchange   %s" % stats(te, moved))
        assert xg.exchange(ctx, 1, P, A, d, rl, c, arena.ptr(xg.BUF_SEND), arena.ptr(xg.BUF_RECV))[:2] == (0, 0)
        arena.close()
    ctx.close()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
