"""Strided-run lists for the vec placement tests (test_vec_host.py): a Python expansion (what a
vec list means), seeded lists whose blocks never overlap, and mutations of them that a checker must judge as it judges their expansion."""
import numpy as np

WORDS = ("out of range", "negative", "overflow", "past the domain end", "overlap")


def py_expand(vecs):
    """one (rank, agg, off, len) per block of every positive vec, in order; the stride of a vec
    with count == 1 is not looked at"""
    out = []
    for (r, a, off, n, st, c) in vecs:
        if n > 0 and c > 0:
            out += [(r, a, off + j * (st if c > 1 else 0), n) for j in range(c)]
    return out


def word(err):
    """the kind of fault a checker's message names ('' for none)"""
    return next((w for w in WORDS if w in err), "")


def make_vecs(P, A, seed, bands=5, max_len=300, max_count=9):
    """Per aggregator `bands` groups of vecs laid one behind the other with gaps of 0..40 B (a gap
    of 0: neighbours touch and share a 16-B cell), every group one of
      striped   2..4 vecs of random pairs with one stride S = the sum of their lengths (+ gaps),
                interleaved block by block -- the view of a global array's rows;
      mixed     a vec of stride S beside two vecs of stride 2 S that alternate in its gaps (unequal
                strides, hulls meeting);
      packed    one vec with stride == len (its blocks back to back);
      spaced    one vec with stride > len;
      single    count == 1 with a stride that means nothing (negative), a count-0 and a len-0 vec;
    the list in seeded random order -> (vecs, dom_bytes).  No two blocks overlap."""
    rng = np.random.default_rng(seed)
    vecs, dom = [], []
    for a in range(A):
        cur = int(rng.integers(0, 40))
        for b in range(bands):
            kind = ("striped", "mixed", "packed", "spaced", "single")[(b + a + seed) % 5]
            cur += int(rng.choice([0, 0, 1, 7, 16, 33]))
            c = int(rng.integers(2, max_count + 1))
            rk = lambda: int(rng.integers(0, P))
            ln = lambda: int(rng.integers(1, max_len + 1))
            if kind == "striped":
                k = int(rng.integers(2, 5))
                lens = [ln() for _ in range(k)]
                gaps = [int(rng.choice([0, 0, 3, 16])) for _ in range(k)]
                S = sum(lens) + sum(gaps)
                o = cur
                for n, g in zip(lens, gaps):
                    vecs.append((rk(), a, o, n, S, c))
                    o += n + g
                cur += c * S
            elif kind == "mixed":
                n0, n1, n2 = ln(), ln(), ln()
                S = n0 + max(n1, n2) + int(rng.choice([0, 5]))
                vecs.append((rk(), a, cur, n0, S, 2 * c))
                vecs.append((rk(), a, cur + n0, n1, 2 * S, c))
                vecs.append((rk(), a, cur + n0 + S, n2, 2 * S, c))
                cur += 2 * c * S
            elif kind == "packed":
                n = int(rng.integers(1, 41))
                vecs.append((rk(), a, cur, n, n, 20 * c))
                cur += 20 * c * n
            elif kind == "spaced":
                n = ln()
                st = n + int(rng.integers(1, 50))
                vecs.append((rk(), a, cur, n, st, c))
                cur += (c - 1) * st + n
            else:
                n = ln()
                vecs.append((rk(), a, cur, n, -5, 1))
                vecs.append((rk(), a, cur, 17, 3, 0))
                vecs.append((rk(), a, cur + 1, 0, 0, 4))
                cur += n
        dom.append(cur + int(rng.integers(0, 50)))
    vecs = [vecs[i] for i in rng.permutation(len(vecs))]
    return vecs, dom


def mutate(vecs, dom, P, A, seed):
    """one seeded mutation of a good list -> (name, vecs, dom): most make it a list a scatter must
    refuse, some keep it good"""
    rng = np.random.default_rng(seed)
    v = [list(x) for x in vecs]
    pos = [i for i, x in enumerate(v) if x[3] > 0 and x[5] > 0]
    multi = [i for i in pos if v[i][5] > 1]
    i, m = int(rng.choice(pos)), int(rng.choice(multi))
    kind = ("none", "shift+1", "shift-1", "stride<len", "stride=len", "past", "rank", "agg", "count0", "len0",
            "dup", "grow", "stride+1")[seed % 13]
    dom = list(dom)
    if kind == "shift+1":
        v[i][2] += 1
    elif kind == "shift-1":
        v[i][2] = max(0, v[i][2] - 1)
    elif kind == "stride<len":
        v[m][4] = v[m][3] - 1
    elif kind == "stride=len":
        v[m][4] = v[m][3]
    elif kind == "past":
        dom[v[i][1]] = v[i][2] + (v[i][5] - 1) * (v[i][4] if v[i][5] > 1 else 0) + v[i][3] - 1
    elif kind == "rank":
        v[i][0] = P
    elif kind == "agg":
        v[i][1] = A
    elif kind == "count0":
        v[i][5] = 0
    elif kind == "len0":
        v[i][3] = 0
    elif kind == "dup":
        v.append([(v[i][0] + 1) % P, v[i][1], v[i][2] + v[i][3] - 1, 1, 0, 1])
    elif kind == "grow":
        v[i][3] += 1
    elif kind == "stride+1":
        v[m][4] += 1
    return kind, [tuple(x) for x in v], dom

