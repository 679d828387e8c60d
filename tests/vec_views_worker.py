"""One rank of a real multi-rank xg_exchange_wv job placed by views (tests/test_gpu_vec_views.py).

Started G times as tests/vec_worker.py is (RANK / WORLD_SIZE / XG_MR_DIR / XG_SHARE_GPU=1), with
XG_VEC_VIEWS=1 in its environment.  argv[1]: JSON {"method", "P", "A", "c", "L", "count"}.  The vec
list is every aggregator's domain striped over the P ranks in runs of L bytes, rank-major, on every
rank.  Every rank builds its own source buffer (GPU g's is payload(g, n)) and destination buffer (a
pre-set pattern), makes one call with verify on and prints one JSON line: return code, bad slots, bad
vecs, error text, the placement's workgroups and views, the host's view tile count and view count for
this GPU's rows, and whether its whole destination equals the numpy execution over the list's
expansion.  A rank still running at XG_MR_DEADLINE says where and exits 5.
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
    from vec_cases import py_expand
    xg = G.load_package().xg
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    deadline_watch(xg, rank, float(os.environ.get("XG_MR_DEADLINE", "100")))
    case = json.loads(sys.argv[1])
    method, P, A, c, L, count = (case[k] for k in ("method", "P", "A", "c", "L", "count"))
    vecs = [(r, a, r * L, L, P * L, count) for r in range(P) for a in range(A)]
    dom = [P * L * count] * A
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
        NOW[0] = "xg_exchange_wv m%d by views" % method
        rc, bad, bad_v, _place_s, timers, err = xg.exchange_wv(ctx, method, P, A, vecs, dom, rl, c,
                                                               reg.ptr(xg.BUF_SEND), reg.ptr(xg.BUF_RECV))
        rows, _idx, rb = s.vec_rows(world, rank, vecs, dom)
        host = xg.ViewTables(rows, rb)
        row = {"rank": rank, "rc": rc, "bad": bad, "bad_vecs": bad_v, "err": err, "tiles": xg.vec_tiles(),
               "views": xg.exchange_wv_views(), "host_tiles": host.tiles, "host_views": host.multi,
               "row_tiles": xg.vec_rows_tiles(rows)[-1], "exact": None}
        if rc == 0:
            want = placed(s, world, rank, exts, dom, lambda h: payload(h, sizes(h)[0]), preset)
            got = np.frombuffer(reg.read(xg.BUF_RECV, 0, nrecv), dtype=np.uint8)
            row["exact"] = bool(np.array_equal(got, want))
        print(json.dumps(row), flush=True)
        ctx.barrier()
    finally:
        reg.close()
    ctx.close()


if __name__ == "__main__":
    main()
