"""One rank of a real multi-rank xg_exchange_w job on the box's GPU (tests/test_gpu_place.py).

Started G times as tests/multirank_worker.py is (RANK / WORLD_SIZE / XG_MR_DIR / XG_SHARE_GPU=1).
argv[1]: JSON {"method", "P", "A", "c", "seed"}.  The extent list is place_cases.make_exts(P, A,
seed) on every rank.  Every rank builds its own source buffer (seeded random bytes: GPU g's is
payload(g, n), so every rank can compute what any other holds) and destination buffer (a pre-set
pattern), and makes three calls with verify on, printing one JSON line each:
  1. the list as it is: return code, bad slots, bad extents, error text and whether its whole
     destination (a2m: the domain buffer, m2a: the dense RECV) equals the numpy execution;
  2. rank 1's list with one offset changed (the ranks' inputs differ);
  3. every rank's list with a one-byte overlap of two extents of one aggregator.
A rank still running at XG_MR_DEADLINE says where and exits 5.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))


def main():
    import numpy as np
    import __graft_entry__ as G
    from multirank_worker import NOW, deadline_watch, rendezvous
    from place_cases import make_exts, payload, placed
    xg = G.load_package().xg
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    deadline_watch(xg, rank, float(os.environ.get("XG_MR_DEADLINE", "100")))
    case = json.loads(sys.argv[1])
    method, P, A, c = case["method"], case["P"], case["A"], case["c"]
    exts, dom = make_exts(P, A, case["seed"])
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, c, rl, lens=xg.exts_lens(exts, P, A))
    a2m = s.direction == xg.A2M

    def sizes(g):
        dense = s.region_bytes(world, g, xg.BUF_SEND if a2m else xg.BUF_RECV)
        d = s.domain_bytes(world, g, dom)
        return (dense, d) if a2m else (d, dense)

    uid = rendezvous(xg, rank, world, os.environ["XG_MR_DIR"])
    ctx = xg.Context(rank=rank, nranks=world, device=0, uid=uid)
    ctx.barrier()
    nsend, nrecv = sizes(rank)
    reg = xg.Regions(ctx, [nsend + 16, nrecv + 16, 0, 0, 0])
    try:
        preset = payload(100 + rank, nrecv)
        reg.write(xg.BUF_SEND, 0, payload(rank, nsend).tobytes())
        reg.write(xg.BUF_RECV, 0, preset.tobytes())

        def call(what, lst):
            NOW[0] = "xg_exchange_w m%d (%s)" % (method, what)
            rc, bad, bad_e, _place_s, timers, err = xg.exchange_w(ctx, method, P, A, lst, dom, rl, c,
                                                                  reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
            return {"rank": rank, "what": what, "rc": rc, "bad": bad, "bad_exts": bad_e, "err": err,
                    "timers": sum(1 for t in timers if t.total_time > 0)}

        row = call("good", exts)
        row["exact"] = None
        if row["rc"] == 0:
            want = placed(s, world, rank, exts, dom, lambda h: payload(h, sizes(h)[0]), preset)
            got = np.frombuffer(reg.read(xg.BUF_RECV, 0, nrecv), dtype=np.uint8)
            row["exact"] = bool(np.array_equal(got, want))
        print(json.dumps(row), flush=True)
        # one offset differs on rank 1 (towards a gap or not: the lists differ either way)
        mine = list(exts)
        if rank == 1:
            k = next(i for i, e in enumerate(mine) if e[3] > 0 and e[2] > 0)
            r, a, off, n = mine[k]
            mine[k] = (r, a, off - 1, n)
        print(json.dumps(call("differ", mine)), flush=True)
        # two extents of aggregator 0 that share one byte, on every rank
        k = max((i for i, e in enumerate(exts) if e[1] == 0 and e[3] > 1), key=lambda i: exts[i][2])
        r, a, off, n = exts[k]
        print(json.dumps(call("overlap", list(exts) + [((r + 1) % P, a, off + n - 1, 1)])), flush=True)
        ctx.barrier()
    finally:
        reg.close()
    ctx.close()


if __name__ == "__main__":
    main()
