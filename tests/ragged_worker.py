"""One rank of a real multi-rank xg_exchange_v job on the box's GPU (tests/test_gpu_ragged.py).

Started G times as tests/multirank_worker.py is (RANK / WORLD_SIZE / XG_MR_DIR / XG_SHARE_GPU=1).
argv[1]: JSON {"method", "P", "A", "c", "lens": [P x A], "perturb": {rank: [index, delta]}}.
Every rank builds its own SEND / RECV (an ordinary allocation, SEND = seeded random bytes: GPU g's
payload is _payload(g, n), so every rank can compute what any other sent), calls xg_exchange_v
with verify on over the matrix -- a rank named in "perturb" with one entry changed -- and prints
one JSON line: its return code, bad slots, error text and whether its whole RECV equals the numpy
delivery.  A rank still running at XG_MR_DEADLINE says where and exits 5.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))


def _payload(g, n):
    import numpy as np
    return np.random.default_rng(4242 + g).integers(0, 256, n, dtype=np.uint8)


def main():
    import numpy as np
    import __graft_entry__ as G
    from multirank_worker import NOW, deadline_watch, rendezvous
    xg = G.load_package().xg
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    deadline_watch(xg, rank, float(os.environ.get("XG_MR_DEADLINE", "100")))
    case = json.loads(sys.argv[1])
    method, P, A, c, lens = case["method"], case["P"], case["A"], case["c"], list(case["lens"])
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, c, rl, lens=lens)           # the job's layout (the unperturbed matrix)
    mine = list(lens)
    if str(rank) in case.get("perturb", {}):
        k, delta = case["perturb"][str(rank)]
        mine[k] += delta
    uid = rendezvous(xg, rank, world, os.environ["XG_MR_DIR"])
    ctx = xg.Context(rank=rank, nranks=world, device=0, uid=uid)
    ctx.barrier()
    nsend, nrecv = s.region_bytes(world, rank, xg.BUF_SEND), s.region_bytes(world, rank, xg.BUF_RECV)
    reg = xg.Regions(ctx, [nsend + 16, nrecv + 16, 0, 0, 0])    # + 16: a perturbed rank's plan may be longer
    try:
        reg.write(xg.BUF_SEND, 0, _payload(rank, nsend).tobytes())
        NOW[0] = "xg_exchange_v m%d" % method
        rc, bad, timers, err = xg.exchange_v(ctx, method, P, A, mine, rl, c, reg.ptr(xg.BUF_SEND),
                                             reg.ptr(xg.BUF_RECV))
        exact = None
        if rc == 0:
            want = np.full(nrecv, 0xA5, np.uint8)
            for q, n in zip(s.deliveries(world), s.delivery_lens(world)):
                if q.dst_gpu == rank:
                    src = _payload(q.src_gpu, s.region_bytes(world, q.src_gpu, xg.BUF_SEND))
                    want[q.recv_off:q.recv_off + n] = src[q.send_off:q.send_off + n]
            got = np.frombuffer(reg.read(xg.BUF_RECV, 0, nrecv), dtype=np.uint8)
            exact = bool(np.array_equal(got, want))
        print(json.dumps({"rank": rank, "rc": rc, "bad": bad, "err": err, "exact": exact,
                          "timers": sum(1 for t in timers if t.total_time > 0)}), flush=True)
        ctx.barrier()
    finally:
        reg.close()
    ctx.close()


if __name__ == "__main__":
    main()
