#!/usr/bin/env python3
"""The plans whose kernel dispatches pin down how a step's copies launch: every launch form of
the per-plan launch table (host/plan_tables.cc: TableBuilder) -- stage launches alone and
fused, local + pack launches, fused unpack + pack launches, deferred unpacks, split steps in
both fork orders, the local part inside the RCCL group, wave launches, cut launches, chains.
Each plan is loaded and run once and every slot is checked against the oracle.

Run under `rocprofv3 --kernel-trace` (no other tracing, no counters) and reduce the trace
with launch_table_reduce.py; two builds that launch alike give identical reduced traces:

  rocprofv3 --kernel-trace -d OUT -o run --output-format csv -- python3 profiles/launch_table_trace.py
  python3 profiles/launch_table_reduce.py OUT/.../run_kernel_trace.csv > trace.txt

XG_TREE=<checkout> runs another checkout's build (the oracle is this one's)."""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.abspath(os.environ.get("XG_TREE", HERE))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(HERE, "oracle"))
import __graft_entry__ as G  # noqa: E402
import xg_oracle as O  # noqa: E402

xg = G.load_package().xg
P, A, c, k = 32, 14, 3, 2
CUT = {"XG_COPY_LAUNCH_MAX": "65536"}


def cases():
    """(label, virtual GPUs or 0, method, d, environment)"""
    out = []
    for m in (1, 2, 3, 4, 6, 12):                       # chains whose first dispatch stamps, and cuts
        chain = [{}, {"XG_STEP_CHAIN": "0"}] if m in (6, 12) else [{}]
        for ch in chain:
            for cut in ({}, CUT):
                out.append((0, m, 48 << 10, {**ch, **cut}))
    for m in (15, 16):                                  # a stage launch alone / fused into the local launch
        for fuse in ({}, {"XG_FUSE_STAGE": "0"}):
            out.append((0, m, 2048, fuse))
    out.append((0, 1, 1000, {}))                        # misaligned pieces: no wave launch
    for m in (1, 6, 9, 12):                             # fused unpack + pack launches, deferred unpacks
        for cut in ({}, CUT):
            for self_max in ({}, {"XG_SELF_MAX": "0"}):     # the local part in the RCCL group / in the pack launch
                out.append((2, m, 16 << 10, {**cut, **self_max}))
        wave = {"XG_COPY_WAVE_MIN": "0"}                # wave launches
        out.append((2, m, 16 << 10, wave))
        out.append((2, m, 16 << 10, {**wave, "XG_WAVE_KIB": "2"}))
        out.append((2, m, 16 << 10, {**wave, **CUT}))   # a cut wave launch
    for order in ({}, {"XG_SPLIT_AFTER_PACK": "0"}):    # split steps, both fork orders
        out.append((2, 1, 256 << 10, {"XG_SPLIT_MIN": "65536", **order}))
    return out


def contexts(gpus, env):
    env = {"XG_ENGINE_MAX_STEP": "0", **env}           # every step its own launches
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        if gpus:
            return [xg.Context.virtual(g, gpus, device=0) for g in range(gpus)]
        return [xg.Context(rank=0, nranks=1, device=0)]
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v


def check(s, run, exp, d, G_):
    chk, bad, _first = run.verify()
    if any(bad):
        raise SystemExit("bad bytes in a slot")
    for (src, _seed, dst, off), ck in zip(run.slots, chk):
        local = off - s.recv_offset(G_, dst)
        if ck != O.chk64(exp[dst][local: local + d]):
            raise SystemExit("slot %d -> %d differs from the oracle" % (src, dst))


rl = xg.aggregator_list(P, A)
for i, (gpus, m, d, env) in enumerate(cases()):
    it = 2 if gpus else 1
    s = xg.Schedule(m, P, A, d, c, rl, ntimes=k, iteration=it)
    exp = O.expected_recv(m, P, A, d, rl, it, mode=1)
    ctxs = contexts(gpus, env)
    runs = [xg.MethodRun(cx, s, it=it, mode=1, **({"pack_max_seg": 1 << 30} if gpus else {})) for cx in ctxs]
    if gpus:
        xg.run_virtual(runs)
    else:
        runs[0].run_timed()
    for r in runs:                                      # the verify kernels end the plan's stretch of the trace
        check(s, r, exp, d, max(gpus, 1))
    print("plan %2d: %s m%-2d d %-6d %-52s launches %s wave %s" % (
        i, "%d virtual GPUs" % gpus if gpus else "1 GPU         ", m, d,
        " ".join("%s=%s" % e for e in sorted(env.items())) or "-", [r.launches for r in runs],
        [r.wave_launches()[0] for r in runs]), flush=True)
    for r in runs:
        r.close()
    for cx in ctxs:
        cx.close()
print("all plans ok")
