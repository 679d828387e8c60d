"""One rank of a real multi-rank xg_exchange job on the box's GPU (tests/test_gpu_payload_multirank.py).

Started G times like tests/multirank_worker.py (RANK / WORLD_SIZE / XG_MR_DIR / XG_SHARE_GPU=1):
every rank is its own process and RCCL rank on device 0.  argv[1]: JSON {"shape": [P, A, d, c],
"methods": [...]}.  Every rank owns a "caller's" SEND and RECV buffer of seeded random bytes
(GPU g's SEND is default_rng(seed + g), so every rank can compute what any other holds) and runs
xg_exchange with verify over them; afterwards it reads its whole RECV back and compares it with
the numpy execution of the deliveries.  Then one more call with rank 1's SEND pointer misaligned
by 8 bytes: every rank must get the same non-zero code, and the communicator must still work
(a barrier follows).  Each rank prints one JSON line per call and a last {"done": true}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from multirank_worker import NOW, deadline_watch, rendezvous  # noqa: E402


def main():
    import numpy as np
    import __graft_entry__ as G
    xg = G.load_package().xg
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    deadline_watch(xg, rank, float(os.environ.get("XG_MR_DEADLINE", "100")))
    case = json.loads(sys.argv[1])
    P, A, d, c = case["shape"]
    rl = xg.aggregator_list(P, A)
    uid = rendezvous(xg, rank, world, os.environ["XG_MR_DIR"])
    ctx = xg.Context(rank=rank, nranks=world, device=0, uid=uid)
    ctx.barrier()

    def payload(method, g, n):
        return np.random.default_rng(1000 * method + g).integers(0, 256, n, dtype=np.uint8)

    for method in case["methods"] + [-case["methods"][0]]:
        misalign = method < 0           # the last call: rank 1 hands in a SEND pointer at +8 B
        method = abs(method)
        NOW[0] = "exchange m%d%s" % (method, " misaligned" if misalign else "")
        sys.stderr.write("rank %d: %s\n" % (rank, NOW[0]))
        s = xg.Schedule(method, P, A, d, c, rl, iteration=1)
        sb = [s.region_bytes(world, g, xg.BUF_SEND) for g in range(world)]
        rb = s.region_bytes(world, rank, xg.BUF_RECV)
        arena = xg.Regions(ctx, [sb[rank] + 16, rb, 0, 0, 0])     # RECV: poisoned by the allocation
        try:
            arena.write(xg.BUF_SEND, 0, payload(method, rank, sb[rank] + 16).tobytes())
            send, recv = arena.ptr(xg.BUF_SEND), arena.ptr(xg.BUF_RECV)
            if misalign and rank == 1:
                send += 8
            rc, bad, timers, err = xg.exchange(ctx, method, P, A, d, rl, c, send, recv or None, it=1)
            wrong = -1
            if rc == 0:
                want = np.full(rb, 0xA5, np.uint8)
                sends = [payload(method, g, sb[g] + 16) for g in range(world)]
                for q in s.deliveries(world):
                    if q.dst_gpu == rank:
                        want[q.recv_off:q.recv_off + d] = sends[q.src_gpu][q.send_off:q.send_off + d]
                got = np.frombuffer(arena.read(xg.BUF_RECV, 0, rb), dtype=np.uint8)
                wrong = int(np.count_nonzero(got != want))
            print(json.dumps({"method": method, "misaligned": misalign, "rank": rank, "rc": rc, "bad": bad,
                              "wrong_bytes": wrong, "err": err, "slots": rb // d,
                              "total_time": max((t.total_time for t in timers), default=0.0)}), flush=True)
        finally:
            arena.close()
    NOW[0] = "last barrier"
    ctx.barrier()                        # the refused call left the communicator usable
    ctx.close()
    print(json.dumps({"done": True}), flush=True)


if __name__ == "__main__":
    main()
