"""One rank of a real multi-rank xg_exchange_wv job on the box's GPU (tests/test_gpu_vec.py).

Started G times as tests/place_worker.py is (RANK / WORLD_SIZE / XG_MR_DIR / XG_SHARE_GPU=1).
argv[1]: JSON {"method", "P", "A", "c", "seed"}.  The vec list is vec_cases.make_vecs(P, A, seed) on
every rank.  Every rank builds its own source buffer (GPU g's is payload(g, n)) and destination
buffer (a pre-set pattern), and makes three calls with verify on, printing one JSON line each:
  1. the list as it is: return code, bad slots, bad vecs, error text, the copy_kernel_v workgroups of
     the placement and whether its whole destination (a2m: the domain buffer, m2a: the dense RECV)
     equals the numpy execution over the list's expansion;
  2. rank 1's list with one stride changed (the ranks' inputs differ);
  3. every rank's list with a one-byte overlap of two blocks of one aggregator.
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
    from place_cases import payload, placed
    from vec_cases import make_vecs, py_expand
    xg = G.load_package().xg
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    deadline_watch(xg, rank, float(os.environ.get("XG_MR_DEADLINE", "100")))
    case = json.loads(sys.argv[1])
    method, P, A, c = case["method"], case["P"], case["A"], case["c"]
    vecs, dom = make_vecs(P, A, case["seed"])
    exts = py_expand(vecs)
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, c, rl, lens=xg.vecs_lens(vecs, P, A))
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
            NOW[0] = "xg_exchange_wv m%d (%s)" % (method, what)
            rc, bad, bad_v, _place_s, timers, err = xg.exchange_wv(ctx, method, P, A, lst, dom, rl, c,
                                                                   reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
            return {"rank": rank, "what": what, "rc": rc, "bad": bad, "bad_vecs": bad_v, "err": err,
                    "tiles": xg.vec_tiles(), "timers": sum(1 for t in timers if t.total_time > 0)}

        row = call("good", vecs)
        row["exact"] = None
        if row["rc"] == 0:
            want = placed(s, world, rank, exts, dom, lambda h: payload(h, sizes(h)[0]), preset)
            got = np.frombuffer(reg.read(xg.BUF_RECV, 0, nrecv), dtype=np.uint8)
            row["exact"] = bool(np.array_equal(got, want))
        print(json.dumps(row), flush=True)
        # one stride differs on rank 1 (the lists differ, whatever the checker would say of it)
        mine = list(vecs)
        if rank == 1:
            k = next(i for i, v in enumerate(mine) if v[3] > 0 and v[5] > 1)
            r, a, off, n, st, cnt = mine[k]
            mine[k] = (r, a, off, n, st + 1, cnt)
        print(json.dumps(call("differ", mine)), flush=True)
        # a block of one byte on the last byte of a block of aggregator 0, on every rank
        r, a, off, n, st, cnt = next(v for v in vecs if v[1] == 0 and v[3] > 1 and v[5] > 0)
        print(json.dumps(call("overlap", list(vecs) + [((r + 1) % P, a, off + n - 1, 1, 0, 1)])), flush=True)
        ctx.barrier()
    finally:
        reg.close()
    ctx.close()


if __name__ == "__main__":
    main()
