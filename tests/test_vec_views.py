"""Host: striped views of a row list -- their recognition (xg_vrow_views, csrc/host/vecs.c), the deal
of a tile across a view's rows (xg_view_piece_at, xg_sched.h) and the tables of a view launch
(xg_view_tables_build, csrc/host/vec_tables.cc), what xg_vecplace_load_views uploads -- built and
judged with no GPU:
  recognition  the views of striped lists in any list order, every condition broken alone, the cuts
               of long chains;
  deal         every (tile, lane) of a view through xg_view_piece against the rows' blocks;
  tables       cuts against a cutter written a second time here, by bisection, in a child process
               under a time and an address-space limit; refusals; the dump; xg_vec_tables_dump's text
               derived a second time for inputs of test_vec_tables.py;
  sanitizers   tests/view_tables_san.cc, a program of its own, under ASan and UBSan.
"""
import bisect
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mpi-asynchronous-communication-test_amd")
sys.path.insert(0, HERE)
from test_vec_tables import BIG, HAND, REFUSED, cut_case, regions_of      # noqa: E402
from vec_cases import py_expand      # noqa: E402

S, R = 0, 1
P, A = 8, 3
TB, TP = 32768, 256
SINGLE, DST, SRC = 0, 1, 2


# ------------------------------------------------------------------ the arithmetic, a second time
def kmax_of(n, tb=TB, tp=TP):
    return min(tp, max(1, tb // n))


def jb_of(n, k, tb=TB, tp=TP):
    return max(1, min(tb // (k * n), tp // k))


def view_tiles(n, c, k, tb=TB, tp=TP):
    if n <= tb:
        return -(-c // jb_of(n, k, tb, tp))
    return -(-n // tb) * c


def view_before(n, c, k, t, tb=TB, tp=TP):
    """bytes of tiles [0, t) of a view of k rows"""
    if n <= tb:
        return min(t * jb_of(n, k, tb, tp), c) * k * n
    ppb = -(-n // tb)
    return (t // ppb) * n + min((t % ppb) * tb, n)


class Launch:
    """prefix sums over views (len, count, k): tiles and bytes before any tile, O(log views) each, and
    the cutting rule of xg_sched.h by bisection over the tile index"""

    def __init__(self, views, tb=TB, tp=TP):
        self.views, self.tb, self.tp = views, tb, tp
        self.tile0, self.byte0 = [0], [0]
        for (n, c, k) in views:
            self.tile0.append(self.tile0[-1] + view_tiles(n, c, k, tb, tp))
            self.byte0.append(self.byte0[-1] + n * c * k)
        self.T, self.B = self.tile0[-1], self.byte0[-1]

    def before(self, t):
        if t >= self.T:
            return self.B
        v = bisect.bisect_right(self.tile0, t) - 1
        n, c, k = self.views[v]
        return self.byte0[v] + view_before(n, c, k, t - self.tile0[v], self.tb, self.tp)

    def cuts(self, cap):
        out = [0]
        if self.T == 0:
            return out
        if cap > 0 and self.B > cap + cap // 2:
            o = 0
            while self.B - self.before(o) >= cap:
                lo, hi = o + 1, self.T                      # the first e with bytes [o, e) >= cap
                while lo < hi:
                    mid = (lo + hi) // 2
                    if self.before(mid) - self.before(o) >= cap:
                        hi = mid
                    else:
                        lo = mid + 1
                if lo >= self.T or self.T - lo < 16 or self.B - self.before(lo) < cap // 2:
                    break
                out.append(lo)
                o = lo
        return out + [self.T]


def blocks_of(rows):
    """(row, src_off, dst_off, n) of every block"""
    out = []
    for i, (_sb, _db, so, do, ss, ds, n, c) in enumerate(rows):
        out += [(i, so + j * (ss if c > 1 else 0), do + j * (ds if c > 1 else 0), n) for j in range(c)]
    return out


def as_sets(rows, views):
    """views as a set of (kind, the rows themselves in view order): what does not depend on list order"""
    return {(kind, tuple(rows[i] for i in idx)) for kind, idx in views}


# ------------------------------------------------------------------ recognition
def striped_vecs(L, count, order, seed=0):
    """a domain of every aggregator striped over the P ranks in runs of L bytes"""
    pairs = [(r, a) for a in range(A) for r in range(P)] if order == "agg" else [(r, a) for r in range(P) for a in range(A)]
    if order == "shuffled":
        pairs = [pairs[i] for i in np.random.default_rng(seed).permutation(len(pairs))]
    return [(r, a, r * L, L, P * L, count) for (r, a) in pairs], [P * L * count] * A


@pytest.mark.parametrize("L", [64, 100])
@pytest.mark.parametrize("method", [1, 2])
def test_striped_lists_give_the_same_views_in_any_order(xg, method, L):
    """P 8, A 3, runs of L: as a2m rows every aggregator's 8 rows are one dst-striped view, as m2a rows
    one src-striped view, whether the list is agg-major, rank-major or shuffled; xg_vec_rows_build's
    rows of one aggregator are A apart in a rank-major list"""
    rl = xg.aggregator_list(P, A)
    seen = []
    for order in ("agg", "rank", "shuffled"):
        vecs, dom = striped_vecs(L, 37, order, seed=5)
        assert len(py_expand(vecs)) == P * A * 37
        s = xg.Schedule(method, P, A, 0, 3, rl, lens=xg.vecs_lens(vecs, P, A))
        rows, idx, _rb = s.vec_rows(1, 0, vecs, dom)
        views = xg.vrow_views(rows)
        kind = DST if s.direction == xg.A2M else SRC
        assert [(kd, len(ix)) for kd, ix in views] == [(kind, P)] * A, views
        for _kd, ix in views:
            striped = [rows[i][3 if kind == DST else 2] for i in ix]
            assert [y - x for x, y in zip(striped, striped[1:])] == [L] * (P - 1)
            assert len({vecs[idx[i]][1] for i in ix}) == 1           # one aggregator's rows
            if order == "rank":
                assert sorted(ix) == list(range(min(ix), min(ix) + A * P, A))
        assert sorted(i for _kd, ix in views for i in ix) == list(range(len(rows)))
        seen.append(as_sets(rows, views))
    assert seen[0] == seen[1] == seen[2]


def _chain(k, n=48, count=9, dst=True):
    """k rows of one view, in order: the striped side n apart, the dense side anywhere"""
    if dst:
        return [(S, R, 1000 * i + 7, 64 + n * i, n, k * n + 5, n, count) for i in range(k)]
    return [(S, R, 64 + n * i, 1000 * i + 7, k * n + 5, n, n, count) for i in range(k)]


@pytest.mark.parametrize("dst", [True, False], ids=["dst", "src"])
@pytest.mark.parametrize("what", ["len", "count", "src_step", "dst_step", "src_buf", "dst_buf", "offset"])
def test_every_condition_alone_splits_the_chain(xg, what, dst):
    """six rows of one view; row 3 made different in one field is a view of its own between [0, 1, 2]
    and [4, 5]; a striped offset of len + 1 from row 3 on makes [0, 1, 2] and [3, 4, 5]"""
    rows = [list(r) for r in _chain(6, dst=dst)]
    kind = DST if dst else SRC
    assert xg.vrow_views(rows) == [(kind, [0, 1, 2, 3, 4, 5])]
    field = {"src_buf": 0, "dst_buf": 1, "src_step": 4, "dst_step": 5, "len": 6, "count": 7}
    if what == "offset":
        for r in rows[3:]:
            r[3 if dst else 2] += 1
        want = {(kind, (0, 1, 2)), (kind, (3, 4, 5))}
    else:
        rows[3][field[what]] = 4 if what.endswith("buf") else rows[3][field[what]] + 1
        want = {(kind, (0, 1, 2)), (SINGLE, (3,)), (kind, (4, 5))}
    got = xg.vrow_views(rows)
    assert {(kd, tuple(ix)) for kd, ix in got} == want, got
    rng = np.random.default_rng(3)
    perm = [int(i) for i in rng.permutation(6)]
    shuffled = [rows[i] for i in perm]
    assert as_sets([tuple(r) for r in shuffled], xg.vrow_views(shuffled)) == as_sets([tuple(r) for r in rows], got)


def test_a_chain_that_qualifies_both_ways_is_dst_striped(xg):
    rows = [(S, R, 16 * i, 640 + 16 * i, 64, 64, 16, 3) for i in range(4)]
    assert xg.vrow_views(rows) == [(DST, [0, 1, 2, 3])]


def test_long_chains_are_cut_at_kmax(xg):
    """257 rows of 16 B are 256 + 1; 40 rows of 1000 B (kmax 32) are 32 + 8; rows of 32 KiB + 16 a
    len apart are each alone; count == 1 rows (both steps 0) chain like any others"""
    rows = [(S, R, 100 * i, 16 * i, 16, 16 * 257, 16, 4) for i in range(257)]
    assert [(kd, len(ix)) for kd, ix in xg.vrow_views(rows)] == [(DST, 256), (SINGLE, 1)]
    assert xg.vrow_views(rows)[0][1] == list(range(256))
    rows = [(S, R, 1003 * i, 1000 * i, 1000, 40000, 1000, 4) for i in range(40)]
    assert kmax_of(1000) == 32
    assert [(kd, ix) for kd, ix in xg.vrow_views(rows)] == [(DST, list(range(32))), (DST, list(range(32, 40)))]
    n = 32768 + 16
    rows = [(S, R, 0, n * i, n, 4 * n, n, 2) for i in range(4)]
    assert sorted(xg.vrow_views(rows)) == [(SINGLE, [i]) for i in range(4)]
    rows = [(S, R, 500 * i, 33 * i, 0, 0, 33, 1) for i in range(5)]
    assert xg.vrow_views(rows) == [(DST, [0, 1, 2, 3, 4])]
    assert xg.vrow_views([]) == []
    # smaller tiles: the cut follows tile_bytes and tile_pieces
    rows = _chain(10, n=48)
    assert [len(ix) for _kd, ix in xg.vrow_views(rows, tile_bytes=200, tile_pieces=256)] == [4, 4, 2]
    assert [len(ix) for _kd, ix in xg.vrow_views(rows, tile_bytes=32768, tile_pieces=3)] == [3, 3, 3, 1]


# ------------------------------------------------------------------ the deal
KS = [1, 2, 3, 5, 16, 17, 255, 256]
LENS = [1, 7, 16, 17, 64, 100, 1000]


def _view_rows(k, n, count, gap=0):
    """a dst-striped view: stride == k * n + gap on the destination, the sources dense and apart"""
    return [(S, R, 7 + i * (count * n + 3), 11 + i * n, n, k * n + gap, n, count) for i in range(k)]


def _walk(xg, rows, tiles, tb=TB, tp=TP):
    """[(tile, lane, row, src_off, dst_off, n)] of every live lane; idle lanes only behind live ones"""
    out = []
    arr = (xg.VRow * len(rows))(*[xg.VRow(*r) for r in rows])
    for t in range(tiles):
        live = True
        for q in range(tp):
            p = xg.view_piece(arr, t, q, tb, tp)
            assert p is not None
            if p[3]:
                assert live, "a piece behind an idle lane"
                out.append((t, q) + p)
            else:
                live = False
                assert p == (0, 0, 0, 0)
    return out


@pytest.mark.parametrize("k", KS)
def test_the_deal_covers_every_block_once(xg, k):
    """views of k rows at every len that fits (k <= kmax), a count that leaves the last tile partial:
    walking every (tile, lane) through xg_view_piece yields exactly the blocks of the rows, each
    once; a tile's destination pieces ascend lane by lane and are one interval of the tile's bytes
    (stride == k x len); lane q holds row q % k; k == 1 equals xg_vec_piece at every (tile, lane)"""
    done = 0
    for n in LENS:
        if k > kmax_of(n):
            assert xg.view_piece(_view_rows(k, n, 3), 0, 0) is None       # no view: refused
            continue
        jb = jb_of(n, k)
        count = 2 * jb + (jb + 1) // 2
        tiles = view_tiles(n, count, k)
        assert tiles == 3 and xg.view_tiles(n, count, k) == tiles
        rows = _view_rows(k, n, count)
        got = _walk(xg, rows, tiles)
        assert sorted((r, so, do, m) for (_t, _q, r, so, do, m) in got) == sorted(blocks_of(rows))
        for t in range(tiles):
            mine = [g for g in got if g[0] == t]
            assert [g[2] for g in mine] == [g[1] % k for g in mine]
            assert [y[4] - x[4] for x, y in zip(mine, mine[1:])] == [n] * (len(mine) - 1)
            assert len(mine) == k * min(jb, count - t * jb)
            assert mine[0][4] == 11 + t * jb * k * n
        assert xg.view_piece(rows, tiles, 0) is None and xg.view_piece(rows, 0, TP) is None
        if k == 1:
            for t in range(tiles):
                for q in range(TP):
                    assert xg.view_piece(rows, t, q)[1:] == xg.vec_piece_at(rows[0], t, q)
        done += 1
    assert done >= (2 if k >= 255 else 5)


def test_the_deal_of_a_single_row_is_the_row_deal(xg):
    """k = 1 at small tiles and for long blocks (lane 0 takes piece t): xg_vec_piece everywhere"""
    for row in HAND:
        for tb, tp in ((32768, 256), (64, 1), (64, 256)):
            tiles = xg.vec_row_tiles(row[6], row[7], tb, tp)
            assert xg.view_tiles(row[6], row[7], 1, tb, tp) == tiles
            for t in sorted({0, 1, tiles // 2, tiles - 1} & set(range(tiles))):
                for q in range(tp):
                    assert xg.view_piece([row], t, q, tb, tp)[1:] == xg.vec_piece_at(row, t, q, tb, tp)


def test_the_deal_in_64_bits(xg):
    """steps of 2^31 + 48 and row offsets past 2^32: exact"""
    far, n = (1 << 31) + 48, 4096
    rows = [(S, R, (1 << 32) + 5 + i * (1 << 33), (1 << 32) + 3 + n * i, far + 1, far, n, 5) for i in range(2)]
    assert jb_of(n, 2) == 4
    got = _walk(xg, rows, 2)
    assert sorted(g[2:] for g in got) == sorted(blocks_of(rows))
    assert max(g[4] for g in got) == (1 << 32) + 3 + n + 4 * far > 1 << 33
    assert xg.view_tiles(1, (1 << 62), 2, 2, 2) == 1 << 62 and xg.view_tiles(32769, 1 << 62, 1) == (1 << 63) - 1


# ------------------------------------------------------------------ tables
def _mib_rows():
    """about 1 MiB: a view of 8 rows of 64-B blocks, singles, a view of 3 rows of 1000 B, long blocks"""
    rows = [(S, R, 70000 * i, 64 * i, 64, 512, 64, 1024) for i in range(8)]                   # 512 KiB
    rows += [(S, R, 600000 + 101000 * i, 600000 + 1000 * i, 1000, 3000 + 7, 1000, 100) for i in range(3)]    # 300 KB
    rows += [(S, R, 1000000, 1000000, 100001, 100003, 100000, 3)]                              # 300 KB
    rows += [(S, R, 1400000, 1400000, 33, 35, 33, 700)]
    return rows


def table_case(name):
    """-> (rows, tile_bytes, tile_pieces, launch_max)"""
    if name.startswith("mib_"):
        rows = _mib_rows()
        if name.endswith("_shuffled"):
            rows = [rows[i] for i in np.random.default_rng(9).permutation(len(rows))]
        return rows, TB, TP, {"0": 0, "1": 1, "256k": 256 << 10}[name.split("_")[1]]
    if name == "view_of_2^30_blocks":       # O(views + cuts): two rows of 2^30 blocks, one view
        return [(S, R, 0, 16 * i, 16, 32, 16, 1 << 30) for i in range(2)], TB, TP, 512 << 20
    if name == "runt_inside_a_view":
        return [(S, R, 0, 64 * i, 64, 128, 64, 128 * 148) for i in range(2)], TB, TP, 64 * 16384
    return cut_case(name)                   # rows that are no views: the row tables' cases


TABLE_CASES = ["mib_0", "mib_1", "mib_256k", "mib_256k_shuffled", "view_of_2^30_blocks", "runt_inside_a_view",
               "exactly_1.5", "one_tile_over_1.5", "runt_by_tiles", "blocks_2^30"]


def _regions(rows):
    nb = regions_of(rows)
    return [max(x, 1 << 35) if any(r[7] >= 1 << 30 for r in rows) else x for x in nb]


def _child(name):
    """run as a script: build the case's tables and print them"""
    import resource
    resource.setrlimit(resource.RLIMIT_AS, (4 << 30, 4 << 30))      # a cut loop that only appends ends here
    sys.path.insert(0, os.path.dirname(HERE))
    import __graft_entry__ as G
    xg = G.load_package().xg
    rows, tb, tp, cap = table_case(name)
    xg.ViewTables.lib()
    t0 = time.perf_counter()
    t = xg.ViewTables(rows, _regions(rows), tile_bytes=tb, tile_pieces=tp, launch_max=cap)
    dt = time.perf_counter() - t0
    rec = t.records()
    print(json.dumps(dict(cuts=t.cuts(), dbytes=t.dispatch_bytes(), tiles=t.tiles, bytes=t.bytes, seconds=dt,
                          views=rec.get("view", []), order=t.order(), multi=t.multi, tile0=rec["tile0"])))


@pytest.mark.parametrize("name", TABLE_CASES)
def test_view_dispatch_cuts(xg, name):
    """the view records are those of xg_vrow_views with jb by the rule; tile0 is the prefix of the
    views' tile counts; the cuts ascend strictly from 0 to the tile total, obey the row tables' rule
    and are those of the bisection cutter above; the 2^30 cases return in milliseconds"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=8)
    assert out.returncode == 0, out.stderr[-2000:]
    t = json.loads(out.stdout)
    rows, tb, tp, cap = table_case(name)
    views = xg.vrow_views(rows, tb, tp)
    assert t["order"] == [i for _kd, ix in views for i in ix]
    at, shapes = 0, []
    for (kd, ix), rec in zip(views, t["views"]):
        n, c = rows[ix[0]][6], rows[ix[0]][7]
        assert rec == [at, len(ix), jb_of(n, len(ix), tb, tp) if n <= tb else 1, kd]
        shapes.append((n, c, len(ix)))
        at += len(ix)
    assert len(t["views"]) == len(views) and t["multi"] == sum(len(ix) > 1 for _kd, ix in views)
    L = Launch(shapes, tb, tp)
    c = t["cuts"]
    nb = [L.before(y) - L.before(x) for x, y in zip(c, c[1:])]
    print(name, "views", len(views), "tiles", L.T, "bytes", L.B, "cap", cap, "cuts", c[:6], "...", c[-3:], "seconds", t["seconds"])
    assert (t["tiles"], t["bytes"], t["tile0"]) == (L.T, L.B, L.tile0)
    assert c[0] == 0 and c[-1] == L.T and all(x < y for x, y in zip(c, c[1:]))
    assert nb == t["dbytes"] and sum(nb) == L.B
    if cap == 0 or L.B <= cap + cap // 2:
        assert len(c) == 2
    for k, n in enumerate(nb[:-1]):
        last_tile = L.before(c[k + 1]) - L.before(c[k + 1] - 1)
        assert cap <= n < cap + last_tile, (k, n, last_tile)
    if len(c) > 2:
        assert c[-1] - c[-2] >= 16 and nb[-1] >= cap // 2, (c[-3:], nb[-2:])
    assert c == L.cuts(cap)
    if name.startswith("mib_256k"):
        inside = [x for x in c[1:-1] if x not in L.tile0]
        assert len(c) - 1 >= 3 and inside, "no cut inside a view"
        v = bisect.bisect_right(L.tile0, inside[0]) - 1
        assert shapes[v][2] > 1, "the cut lies in a single row"
        assert 900 << 10 < L.B < 1300 << 10 and t["multi"] == 2
    want = {"mib_0": 1, "exactly_1.5": 1, "one_tile_over_1.5": 2, "runt_by_tiles": 2, "runt_inside_a_view": 2,
            "blocks_2^30": 32, "view_of_2^30_blocks": 64}
    if name in want:
        assert len(c) - 1 == want[name]
    if "2^30" in name:
        assert t["seconds"] < 0.25, "xg_view_tables_build walks tiles or blocks"


def test_an_empty_list_is_no_dispatch(xg):
    t = xg.ViewTables([], [0] * 5)
    assert (t.rows, t.views, t.multi, t.tiles, t.dispatches, t.bytes, t.cuts()) == (0, 0, 0, 0, 0, 0, [0])


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals(xg, capfd, name):
    """every row xg_vec_tables_build refuses, alone and behind a good view: XG_EARG, the same words on
    stderr under this builder's name, the list's row index"""
    rows, word = REFUSED[name]
    with pytest.raises(xg.XGError, match="xg_view_tables_build: 3"):
        xg.ViewTables(rows, [BIG, BIG, 0, 0, 0])
    err = capfd.readouterr().err
    assert word in err and "xg_view_tables_build: row 0:" in err
    with pytest.raises(xg.XGError):
        xg.ViewTables(_chain(4) + list(rows), [BIG, BIG, 0, 0, 0])
    assert "xg_view_tables_build: row 4:" in capfd.readouterr().err


def test_too_many_tiles_and_bad_caps_are_refused(xg, capfd):
    """INT32_MAX tiles pass; one more, in one view or over two, is XG_EARG; so are tile_pieces 257,
    tile_bytes 0 and a negative launch_max"""
    ok = (S, R, 0, 0, 1, 1, 1, (1 << 31) - 1)
    nb = [1 << 32, 1 << 32, 0, 0, 0]
    assert xg.ViewTables([ok], nb, tile_bytes=64, tile_pieces=1, launch_max=0).tiles == (1 << 31) - 1
    two = [(S, R, 0, i, 2, 2, 1, 1 << 31) for i in range(2)]            # one view of two rows: 2^31 tiles at jb 1
    assert xg.vrow_views(two, 2, 2) == [(DST, [0, 1])]
    for rows, tb, tp in (([(S, R, 0, 0, 1, 1, 1, 1 << 31)], 64, 1), ([ok, (S, R, 0, 0, 0, 0, 1, 1)], 64, 1), (two, 2, 2)):
        with pytest.raises(xg.XGError):
            xg.ViewTables(rows, nb, tile_bytes=tb, tile_pieces=tp, launch_max=0)
        assert "tiles" in capfd.readouterr().err
    for kw in (dict(tile_pieces=257), dict(tile_bytes=0), dict(launch_max=-1), dict(tile_pieces=0)):
        with pytest.raises(xg.XGError):
            xg.ViewTables([ok], nb, **kw)
        assert "bad arguments" in capfd.readouterr().err


def test_rows_at_the_very_end_of_their_regions_pass(xg):
    rows = [(S, R, 0, BIG - 100 - 2 * 50, 100, 50, 100, 3), (S, R, BIG - 100, 0, 0, 0, 100, 1),
            (S, R, 0, 200, 100, -100, 100, 3)]
    assert xg.ViewTables(rows, [BIG, BIG, 0, 0, 0]).tiles == 3


def test_the_dump_is_deterministic(xg):
    """built twice: the same text; a permutation of the list: the same rows, views, tile0, cuts and
    bytes, the order records apart; the rows stand in view order with the list's pointers"""
    rows = _mib_rows()
    nb = regions_of(rows)
    a = xg.ViewTables(rows, nb, launch_max=256 << 10)
    text = a.dump()
    assert xg.ViewTables(rows, nb, launch_max=256 << 10).dump() == text == a.dump()
    perm = [int(i) for i in np.random.default_rng(4).permutation(len(rows))]
    b = xg.ViewTables([rows[i] for i in perm], nb, launch_max=256 << 10)
    strip = lambda s: [x for x in s.splitlines() if not x.startswith("order ")]
    assert strip(b.dump()) == strip(text)
    assert [perm[i] for i in b.order()] == a.order()
    rec = a.records()
    assert rec["views"]["views"] == a.views == len(rec["view"]) and rec["views"]["multi"] == a.multi == 2
    for i, d in zip(a.order(), rec["row"]):
        r = rows[i]
        assert d == [(r[0], r[2]), (r[1], r[3]), r[4] if r[7] > 1 else 0, r[5] if r[7] > 1 else 0, r[6], r[7]]


@pytest.mark.parametrize("case", ["hand", "mib_256k", "runt_inside_a_row"])
def test_the_row_tables_dump_is_what_it_was(xg, case):
    """xg_vec_tables_dump for inputs of test_vec_tables.py, its text derived here a second time (a row
    is a view of one row to the arithmetic above): the cutter the two builders now share gives the
    row tables what it gave them"""
    if case == "hand":
        rows, tb, tp, cap = HAND, 32768, 256, 1500
    else:
        rows, tb, tp, cap = cut_case(case)
    nb = regions_of(rows)
    L = Launch([(r[6], r[7], 1) for r in rows], tb, tp)
    cuts = L.cuts(cap)
    want = ["vec rows %d tiles %d dispatches %d bytes %d tile_bytes %d tile_pieces %d launch_max %d"
            % (len(rows), L.T, len(cuts) - 1, L.B, tb, tp, cap)]
    for i, (sb, db, so, do, ss, ds, n, c) in enumerate(rows):
        want.append("row %d %d+%d %d+%d %d %d %d %d" % (i, sb, so, db, do, ss if c > 1 else 0, ds if c > 1 else 0, n, c))
    want += ["tile0 %d %d" % (i, v) for i, v in enumerate(L.tile0)]
    want += ["cut %d %d" % (i, v) for i, v in enumerate(cuts)]
    want += ["dbytes %d %d" % (i, L.before(y) - L.before(x)) for i, (x, y) in enumerate(zip(cuts, cuts[1:]))]
    assert xg.VecTables(rows, nb, tile_bytes=tb, tile_pieces=tp, launch_max=cap).dump().splitlines() == want
    # and the view tables of rows that are no views cut where the row tables cut
    v = xg.ViewTables(rows, nb, tile_bytes=tb, tile_pieces=tp, launch_max=cap)
    if v.multi == 0 and v.order() == list(range(len(rows))):
        assert v.cuts() == cuts


# ------------------------------------------------------------------ sanitizers
def test_view_tables_under_sanitizers(tmp_path):
    """tests/view_tables_san.cc (its own main) drives the recognition, the deal and the table builder
    over the cases above, compiled with vec_tables.cc and the C host sources under AddressSanitizer
    and UBSan and run as an executable: nothing is preloaded"""
    host = os.path.join(PKG, "csrc", "host")
    inc = ["-I" + os.path.join(os.path.dirname(HERE), "include")]
    san = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    csrc = [os.path.join(host, f) for f in ("programs.c", "sched.c", "devplan.c", "report.c", "hazard.c", "solo.c",
                                            "calls.c", "pieces.c", "place.c", "vecs.c")]
    objs = []
    for src in csrc:
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-c", src, "-o", o] + san + inc, check=True)
        objs.append(o)
    exe = str(tmp_path / "view_tables_san")
    subprocess.run(["g++", "-std=c++17", os.path.join(HERE, "view_tables_san.cc"), os.path.join(host, "vec_tables.cc"),
                    "-I" + host, "-o", exe] + objs + san + inc + ["-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    assert "launches covered" in out.stdout, out.stdout


if __name__ == "__main__":
    _child(sys.argv[1])
