"""Host side of placement by offset-length lists (csrc/host/place.c, xg_extent_tiles in pieces.c):
no GPU.  The list checks, the length matrix, the domain layout, the placement plan executed with
numpy, the tile cut of a copy_kernel_x dispatch, and a fuzz program under ASan + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from place_cases import make_exts, payload, placed

P, A = 8, 3
EARG = 3


# ------------------------------------------------------------------ xg_exts_lens
def test_exts_lens_against_numpy(xg):
    for seed in range(20):
        exts, _dom = make_exts(P, A, seed)
        want = np.zeros((P, A), np.int64)
        for r, a, _off, n in exts:
            want[r, a] += n
        assert xg.exts_lens(exts, P, A) == [int(x) for x in want.reshape(-1)]
    assert xg.exts_lens([], P, A) == [0] * (P * A)
    for bad in ([(P, 0, 0, 1)], [(0, A, 0, 1)], [(-1, 0, 0, 1)], [(0, 0, 0, -1)],
                [(0, 0, 0, 1 << 62), (0, 0, 0, 1 << 62)]):
        with pytest.raises(xg.XGError):
            xg.exts_lens(bad, P, A)


# ------------------------------------------------------------------ xg_exts_check
def test_exts_check_accepts_valid_lists(xg):
    for seed in range(50):
        exts, dom = make_exts(P, A, seed)
        assert xg.exts_check(exts, P, A, dom, scatter=True) == (0, "")
        assert xg.exts_check(exts, P, A, dom, scatter=False) == (0, "")
    assert xg.exts_check([], P, A, [0] * A) == (0, "")
    # len == 0 is ignored wherever it points inside the domain, an extent may end at the domain end
    assert xg.exts_check([(0, 0, 10, 0), (1, 0, 0, 20), (2, 0, 20, 0), (3, 0, 20, 10)], P, A, [30, 0, 0]) == (0, "")


BIG = 1 << 62
BROKEN = [      # (what, extents and domain lengths given a valid case's domain lengths, the reason's words)
    ("rank high", lambda d: ([(P, 0, 0, 1)], d), "rank 8 out of range"),
    ("rank negative", lambda d: ([(-1, 0, 0, 1)], d), "rank -1 out of range"),
    ("aggregator high", lambda d: ([(0, A, 0, 1)], d), "aggregator 3 out of range"),
    ("aggregator negative", lambda d: ([(0, -1, 0, 1)], d), "aggregator -1 out of range"),
    ("negative offset", lambda d: ([(0, 0, -1, 1)], d), "negative offset or length"),
    ("negative length", lambda d: ([(0, 0, 0, -1)], d), "negative offset or length"),
    ("negative domain", lambda d: ([(0, 0, 0, 1)], [d[0], -1, d[2]]), "negative domain length"),
    ("one byte past the end", lambda d: ([(0, 1, d[1] - 5, 6)], d), "past the domain end"),
    ("empty past the end", lambda d: ([(0, 1, d[1] + 1, 0)], d), "past the domain end"),
    ("off + len overflows", lambda d: ([(0, 0, BIG + 5, BIG)], [BIG, d[1], d[2]]), "overflow"),
    ("a pair's lengths overflow", lambda d: ([(0, 0, 0, BIG), (0, 0, BIG - 1, BIG)], [(1 << 63) - 1, d[1], d[2]]),
     "overflow"),
]


@pytest.mark.parametrize("what, make, word", BROKEN, ids=[b[0] for b in BROKEN])
def test_exts_check_refuses_each_broken_kind(xg, what, make, word):
    good, gdom = make_exts(P, A, 3)
    exts, dom = make(gdom)
    for lst in (exts, good + exts):
        for scatter in (True, False):
            rc, err = xg.exts_check(lst, P, A, dom, scatter=scatter)
            assert rc == EARG and word in err, (what, rc, err)


def test_exts_check_overlap_is_a_scatter_error_only(xg):
    """two positive extents of one aggregator that share ONE byte: refused as a scatter, by list
    index; accepted as a gather; the same offsets on different aggregators are no overlap; a
    zero-length extent inside another is none either"""
    exts, dom = make_exts(P, A, 4)
    k = max((i for i, e in enumerate(exts) if e[1] == 1 and e[3] > 1), key=lambda i: exts[i][2])
    r, a, off, n = exts[k]
    bad = exts + [((r + 3) % P, a, off + n - 1, 1)]
    rc, err = xg.exts_check(bad, P, A, dom, scatter=True)
    assert rc == EARG and "overlap" in err and "extents %d and %d" % (k, len(exts)) in err, err
    assert xg.exts_check(bad, P, A, dom, scatter=False) == (0, "")
    assert xg.exts_check(exts + [((r + 3) % P, a, off + n, 0), (0, a, off + 1, 0)], P, A, dom) == (0, "")
    assert xg.exts_check([(0, 0, 0, 8), (0, 1, 0, 8), (1, 2, 4, 8)], P, A, [16] * A) == (0, "")
    assert xg.exts_check([(0, 0, 0, 8), (5, 0, 7, 8)], P, A, [16] * A)[0] == EARG
    assert xg.exts_check([(0, 0, 8, 8), (5, 0, 0, 8)], P, A, [16] * A) == (0, "")      # touching, list order reversed


# ------------------------------------------------------------------ xg_place_plan_build
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("method", [1, 2])
def test_place_plan_executed_with_numpy(xg, G, method):
    """P 8 / A 3: every GPU's plan is one step of pre copies, no p2p, flags RAGGED | EXTENTS,
    only SEND and RECV sized (the dense side as the exchange's region, the domain side as
    xg_domain_bytes); its copies, executed with numpy on a dense side filled per xg_deliveries,
    give every domain (a2m) / every dense slot (m2a) its expected bytes"""
    exts, dom = make_exts(P, A, 40 + method)
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, 3, rl, lens=xg.exts_lens(exts, P, A))
    a2m = s.direction == xg.A2M
    assert sum(s.domain_bytes(G, g, dom) for g in range(G)) == sum(dom)
    # the exchange itself: every GPU's dense RECV from every GPU's dense SEND, per xg_deliveries
    send = [payload(g, s.region_bytes(G, g, xg.BUF_SEND), salt=method) for g in range(G)]
    if not a2m:     # the dense SEND of a collective read is what the gather produced: start from domains
        domain = [payload(g, s.domain_bytes(G, g, dom), salt=9) for g in range(G)]
    recv = [np.full(s.region_bytes(G, g, xg.BUF_RECV), 0xA5, np.uint8) for g in range(G)]
    for g in range(G):
        v = s.place_plan(G, g, exts, dom)
        assert v.flags == xg.DP_RAGGED | xg.DP_EXTENTS and v.nsteps == 1 and v.p2p == []
        hosted = [e for e in exts if e[3] > 0 and s.gpu_of(G, rl[e[1]]) == g]
        assert v.steps == [(0, len(hosted), 0, 0, len(hosted), 0)] and len(v.copies) == len(hosted)
        assert [c[4] for c in v.copies] == [e[3] for e in hosted]
        assert all(c[0] == xg.BUF_SEND and c[2] == xg.BUF_RECV for c in v.copies)
        dense = s.region_bytes(G, g, xg.BUF_RECV if a2m else xg.BUF_SEND)
        nd = s.domain_bytes(G, g, dom)
        assert v.region_bytes == ([dense, nd, 0, 0, 0] if a2m else [nd, dense, 0, 0, 0])
        if a2m:
            for q, n in zip(s.deliveries(G), s.delivery_lens(G)):
                if q.dst_gpu == g:
                    recv[g][q.recv_off:q.recv_off + n] = send[q.src_gpu][q.send_off:q.send_off + n]
            preset = payload(50 + g, nd)
            got = preset.copy()
            for (_sb, so, _db, do, n) in v.copies:
                got[do:do + n] = recv[g][so:so + n]
            want = placed(s, G, g, exts, dom, lambda h: send[h], preset)
            assert np.array_equal(got, want), (method, G, g)
        else:
            got = np.full(dense, 0x5A, np.uint8)
            for (_sb, so, _db, do, n) in v.copies:
                got[do:do + n] = domain[g][so:so + n]
            send[g] = got
    if not a2m:
        for g in range(G):
            for q, n in zip(s.deliveries(G), s.delivery_lens(G)):
                if q.dst_gpu == g:
                    recv[g][q.recv_off:q.recv_off + n] = send[q.src_gpu][q.send_off:q.send_off + n]
            want = placed(s, G, g, exts, dom, lambda h: domain[h], np.full(len(recv[g]), 0xA5, np.uint8))
            assert np.array_equal(recv[g], want), (method, G, g)


def test_domain_offsets_are_prefix_sums_in_rank_order(xg):
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(1, P, A, 64, 3, rl)
    dom = [1000, 37, 5]
    for G in (1, 2, 4):
        for g in range(G):
            mine = sorted((rl[a], a) for a in range(A) if s.gpu_of(G, rl[a]) == g)
            at = 0
            for _r, a in mine:
                assert s.domain_offset(G, a, dom) == at
                at += dom[a]
            assert s.domain_bytes(G, g, dom) == at
    assert s.domain_offset(1, A, dom) == -1 and s.domain_offset(1, -1, dom) == -1


# ------------------------------------------------------------------ xg_extent_tiles
def test_extent_tiles_properties(xg):
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(1, 700))
        hi = int(rng.choice([17, 300, 5000, 40000]))
        lens = [int(x) for x in rng.integers(0, hi, n)]
        tb, tp = int(rng.choice([8192, 16384, 32768])), int(rng.choice([4, 64, 256]))
        b = xg.extent_tiles(lens, tb, tp)
        assert b[0] == 0 and b[-1] == n and all(x < y for x, y in zip(b, b[1:]))     # a partition, in order
        for t, (lo, hi_) in enumerate(zip(b, b[1:])):
            size = sum(lens[lo:hi_])
            assert hi_ - lo <= tp
            assert size <= tb or hi_ - lo == 1, (trial, t)                             # both caps, or one long piece
            if hi_ < n:                                                                # maximal: the next piece breaks a cap
                assert hi_ - lo == tp or size + lens[hi_] > tb, (trial, t)
    assert xg.extent_tiles([], 16384, 256) == [0]
    assert xg.extent_tiles([5], 0, 256) is None and xg.extent_tiles([5], 16384, 0) is None


@pytest.mark.parametrize("n, want", [(255, [0, 255]), (256, [0, 256]), (257, [0, 256, 257])])
def test_extent_tiles_exact_cases(xg, n, want):
    assert xg.extent_tiles([16] * n, 16384, 256) == want


# ------------------------------------------------------------------ fuzz under sanitizers
@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc not found")
def test_place_fuzz_under_sanitizers(tmp_path):
    """tests/place_fuzz.c with place.c, pieces.c and the schedule sources as one standalone
    executable under ASan + UBSan (leaks on), CPU only, nothing preloaded: random valid and broken
    lists through the check, the matrix, the plan builder (every copy inside its regions, the
    lengths summing up) and the tile cut"""
    exe = str(tmp_path / "place_fuzz")
    host = os.path.join(REPO, "mpi-asynchronous-communication-test_amd", "csrc", "host")
    srcs = [os.path.join(host, f) for f in ("programs.c", "sched.c", "devplan.c", "report.c", "hazard.c", "solo.c",
                                            "calls.c", "pieces.c", "place.c")]
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c99",
                    "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), "-I", host,
                    "-o", exe, os.path.join(REPO, "tests", "place_fuzz.c")] + srcs + ["-lm"], check=True)
    p = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ok after 300 lists" in p.stdout, p.stdout
