"""Extent lists for the placement tests (test_place_host.py, test_gpu_place.py, place_worker.py) and
their numpy execution: what every GPU's domain buffer (a2m) or dense RECV (m2a) must hold."""
import numpy as np


def make_exts(P, A, seed, max_per_pair=6, max_len=3000):
    """per (rank, aggregator) pair 0..max_per_pair extents of 0..max_len bytes; every aggregator's
    extents at seeded random, non-overlapping domain offsets with gaps of 0..70 B (a gap of 0 makes
    neighbours share a 16-B cell), the list in seeded random order -> (exts, dom_bytes)"""
    rng = np.random.default_rng(seed)
    per_agg = [[] for _ in range(A)]
    for r in range(P):
        for a in range(A):
            for _ in range(int(rng.integers(0, max_per_pair + 1))):
                per_agg[a].append((r, int(rng.integers(0, max_len + 1))))
    exts, dom = [], []
    for a in range(A):
        order = rng.permutation(len(per_agg[a]))
        cur = int(rng.integers(0, 40))
        for i in order:
            r, n = per_agg[a][i]
            off = cur + int(rng.choice([0, 0, 1, 7, 16, 33, 70]))
            exts.append((r, a, off, n))
            cur = off + n
        dom.append(cur + int(rng.integers(0, 50)))
    exts = [exts[i] for i in rng.permutation(len(exts))]
    return exts, dom


def payload(g, n, salt=0):
    return np.random.default_rng(4242 + 97 * salt + g).integers(0, 256, n, dtype=np.uint8)


def placed(s, G, g, exts, dom, src_of, preset):
    """numpy execution on GPU g of a G-GPU job over schedule s (built from the list's lengths).
    a2m: -> g's domain buffer, starting from `preset`, given src_of(h) = GPU h's dense SEND;
    m2a: -> g's dense RECV, starting from `preset`, given src_of(h) = GPU h's domain buffer."""
    out = preset.copy()
    a2m = s.direction == 0
    done = {}
    srcs = {}
    for (r, a, off, n) in exts:
        at = done.get((r, a), 0)
        done[(r, a)] = at + n
        if n <= 0:
            continue
        ar = s.rank_list[a]
        ag, rg = s.gpu_of(G, ar), s.gpu_of(G, r)
        if (ag if a2m else rg) != g:
            continue
        h = rg if a2m else ag
        if h not in srcs:
            srcs[h] = src_of(h)
        dpos = s.domain_offset(G, a, dom) + off
        if a2m:
            spos = s.send_offset(G, r) + s.seg_offset(r, a) + at
            out[dpos:dpos + n] = srcs[h][spos:spos + n]
        else:
            rpos = s.recv_offset(G, r) + s.slot_offset(r, a) + at
            out[rpos:rpos + n] = srcs[h][dpos:dpos + n]
    return out
