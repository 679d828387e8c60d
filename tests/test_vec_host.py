"""Host: placement by strided runs -- xg_vecs_expand / lens / check, xg_vec_rows_build and the tile
arithmetic of a row table (include/xg_sched.h, csrc/host/vecs.c, pieces.c).
The oracle is always the expansion: what xg_exts_* and xg_place_plan_build say of one extent per
block.  No GPU."""
import time

import pytest

from vec_cases import make_vecs, mutate, py_expand, word

P, A = 8, 3
I64 = (1 << 63) - 1


# ------------------------------------------------------------------ 1. expansion, lengths, rows
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_expand_and_lens_equal_the_python_expansion(xg, seed):
    vecs, dom = make_vecs(P, A, seed)
    exts = py_expand(vecs)
    assert xg.vecs_expand(vecs) == exts
    assert len(exts) > len(vecs)
    assert xg.vecs_lens(vecs, P, A) == xg.exts_lens(exts, P, A)
    assert xg.vecs_check(vecs, P, A, dom, scatter=True) == (0, "")
    assert xg.exts_check(exts, P, A, dom, scatter=True) == (0, "")


@pytest.mark.parametrize("method,G", [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2)])
def test_rows_are_the_expansions_copies(xg, method, G):
    """every row's blocks, by the row's own arithmetic, are the copies xg_place_plan_build makes of the
    expansion, in order; vec_index names the hosted positive vecs; the regions are the plan's"""
    vecs, dom = make_vecs(P, A, 10 + method)
    exts = py_expand(vecs)
    rl = xg.aggregator_list(P, A)
    s = xg.Schedule(method, P, A, 0, 3, rl, lens=xg.vecs_lens(vecs, P, A))
    seen = 0
    for g in range(G):
        rows, idx, rb = s.vec_rows(G, g, vecs, dom)
        view = s.place_plan(G, g, exts, dom)
        copies = view.copies
        hosted = [i for i, v in enumerate(vecs) if v[3] > 0 and v[5] > 0 and s.gpu_of(G, rl[v[1]]) == g]
        assert idx == hosted and len(rows) == len(hosted)
        assert rb == list(view.region_bytes)
        mine = []
        for (sb, db, so, do, ss, ds, n, c), i in zip(rows, idx):
            assert (n, c) == (vecs[i][3], vecs[i][5])
            if c == 1:
                assert (ss, ds) == (0, 0)
            mine += [(sb, so + j * ss, db, do + j * ds, n) for j in range(c)]
        assert mine == [tuple(c) for c in copies]
        seen += len(rows)
    assert seen == sum(1 for v in vecs if v[3] > 0 and v[5] > 0)


# ------------------------------------------------------------------ 2. the checker against the expansion's
def _cases():
    out = []
    for seed in range(330):
        vecs, dom = make_vecs(P, A, 1000 + seed % 17, bands=4, max_len=60, max_count=5)
        out.append(mutate(vecs, dom, P, A, seed))
    return out


def test_check_agrees_with_the_expansions_check(xg):
    """330 seeded lists (good ones, a vec shifted one byte either way, stride < len, stride == len,
    stride + 1, a block past the domain end, a rank and an aggregator out of range, count 0, len 0, a
    one-byte duplicate, a vec grown by a byte), as a scatter and as a gather: the same verdict and the
    same kind of fault as xg_exts_check gives the expansion"""
    cases = _cases()
    assert len(cases) >= 300
    verdicts = {}
    for kind, vecs, dom in cases:
        exts = py_expand(vecs)
        for scatter in (True, False):
            rc_v, err_v = xg.vecs_check(vecs, P, A, dom, scatter=scatter)
            rc_e, err_e = xg.exts_check(exts, P, A, dom, scatter=scatter)
            assert (rc_v, word(err_v)) == (rc_e, word(err_e)), (kind, scatter, err_v, err_e, vecs, dom)
            assert (rc_v == 0) == (err_v == "")
            verdicts.setdefault((kind, scatter), set()).add(word(err_v))
    # the mutations do what they are named for
    assert verdicts[("none", True)] == {""} and verdicts[("stride=len", True)] <= {"", "overlap"}
    assert verdicts[("stride<len", True)] == {"overlap"} and verdicts[("stride<len", False)] == {""}
    assert verdicts[("dup", True)] == {"overlap"} and verdicts[("dup", False)] == {""}
    assert "overlap" in verdicts[("shift+1", True)] | verdicts[("shift-1", True)]
    assert verdicts[("past", True)] == {"past the domain end"} == verdicts[("past", False)]
    assert verdicts[("rank", True)] == {"out of range"} == verdicts[("agg", False)]
    assert verdicts[("count0", True)] == {""} == verdicts[("len0", True)]


def test_check_walks_unequal_strides_and_single_blocks(xg):
    """clusters that are no striped view: unequal strides that never collide, the same with one
    collision deep inside, a count-1 block in a gap and on a block"""
    dom = [10000]
    a = (0, 0, 0, 10, 30, 100)              # [0, 10) every 30
    b = (1, 0, 10, 5, 60, 50)               # [10, 15) every 60: in a's gaps
    assert xg.vecs_check([a, b], 2, 1, dom) == (0, "")
    c = (1, 0, 15, 5, 45, 60)               # 15, 60, 105, ...: 15 + 45 k meets a at 60 (k = 1)
    rc, err = xg.vecs_check([a, c], 2, 1, dom)
    assert rc == xg.EARG and "overlap" in err and "vec 0 block 2" in err and "vec 1 block 1" in err, err
    assert xg.vecs_check([a, (1, 0, 2980, 20, 0, 1)], 2, 1, dom) == (0, "")      # behind a's last block
    assert xg.vecs_check([a, (1, 0, 1510, 20, 0, 1)], 2, 1, dom) == (0, "")      # in a gap
    assert xg.vecs_check([a, (1, 0, 1509, 20, 0, 1)], 2, 1, dom)[0] == xg.EARG
    # equal strides whose residues wrap round the circle
    d = (1, 0, 25, 10, 30, 99)              # [25, 35) every 30: wraps onto a's [30, 40)
    assert xg.vecs_check([a, d], 2, 1, dom)[0] == xg.EARG
    e = (1, 0, 25, 5, 30, 99)               # [25, 30): touches
    assert xg.vecs_check([a, e], 2, 1, dom) == (0, "")


def test_negative_fields(xg):
    dom = [1000]
    for vec in ((0, 0, 0, 4, -1, 2), (0, 0, 0, 4, 8, -1), (0, 0, 0, -4, 8, 2), (0, 0, -1, 4, 8, 2)):
        for scatter in (True, False):
            rc, err = xg.vecs_check([vec], 1, 1, dom, scatter=scatter)
            assert rc == xg.EARG and "negative" in err, (vec, err)
    assert xg.vecs_check([(0, 0, 0, 4, -1, 1)], 1, 1, dom) == (0, "")            # count 1: the stride means nothing
    assert xg.vecs_check([(0, 0, 0, 4, 0, 7)], 1, 1, dom, scatter=False) == (0, "")
    assert xg.vecs_expand([(0, 0, 0, 4, -1, 2)]) is None
    with pytest.raises(xg.XGError):
        xg.vecs_lens([(0, 0, 0, -4, 8, 2)], 1, 1)


# ------------------------------------------------------------------ 3. overflow
def test_overflow(xg):
    big = [I64]
    # off + (count - 1) * stride past int64
    for vec in ((0, 0, 1 << 62, 8, 1 << 40, 1 << 23), (0, 0, I64 - 10, 8, 8, 2), (0, 0, 0, 8, 1 << 62, 4)):
        for scatter in (True, False):
            rc, err = xg.vecs_check([vec], 1, 1, big, scatter=scatter)
            assert rc == xg.EARG and "overflow" in err, (vec, err)
        assert xg.vecs_expand([vec]) is None
    # ... + len past int64
    rc, err = xg.vecs_check([(0, 0, I64 - 16, 17, 0, 1)], 1, 1, big)
    assert rc == xg.EARG and "overflow" in err
    # count * len past int64 (a gather may read one block again and again)
    vec = (0, 0, 0, 1 << 30, 0, 1 << 40)
    rc, err = xg.vecs_check([vec], 1, 1, [1 << 30], scatter=False)
    assert rc == xg.EARG and "overflow" in err, err
    with pytest.raises(xg.XGError):
        xg.vecs_lens([vec], 1, 1)
    # ... and the sum of two vecs of one pair
    half = (0, 0, 0, 1 << 31, 0, 1 << 31)
    assert xg.vecs_lens([half], 1, 1) == [1 << 62]
    with pytest.raises(xg.XGError):
        xg.vecs_lens([half, half], 1, 1)
    # a tile total past 2^31 - 1: counted in 64 bits, refused as a launch
    assert xg.vec_row_tiles(16, 1 << 40) == 1 << 32
    assert xg.vec_row_tiles(1 << 50, 1 << 40) == I64
    row = (0, 1, 0, 0, 16, 16, 16, 1 << 40)
    assert xg.vec_rows_tiles([row]) is None
    ok = (0, 1, 0, 0, 16, 16, 16, ((1 << 31) - 1) * 256)
    assert xg.vec_rows_tiles([ok]) == [0, (1 << 31) - 1]
    assert xg.vec_rows_tiles([ok, (0, 1, 0, 0, 0, 0, 1, 1)]) is None


# ------------------------------------------------------------------ 4. O(vecs)
def test_nothing_walks_the_blocks_of_a_regular_view(xg):
    """a gather of 2^40 blocks, and a scatter of 32 interleaved vecs of 2^30 blocks each (2^35
    blocks: half a minute at a billion a second), pass check, lens and tile count in far under 5 s"""
    t0 = time.monotonic()
    g = [(r, 0, 64 * r, 64, 0, 1 << 40) for r in range(4)]
    assert xg.vecs_check(g, 4, 1, [256], scatter=False) == (0, "")
    assert xg.vecs_lens(g, 4, 1) == [1 << 46] * 4
    assert xg.vec_row_tiles(64, 1 << 40) == 1 << 32
    S = 32 * 64
    sc = [(r, 0, 64 * r, 64, S, 1 << 30) for r in range(32)]
    assert xg.vecs_check(sc, 32, 1, [S << 30], scatter=True) == (0, "")
    assert xg.vecs_lens(sc, 32, 1) == [1 << 36] * 32
    # one residue moved onto its neighbour: found at the first period, not after a walk to the end
    bad = sc[:5] + [(5, 0, 64 * 5 - 1, 64, S, 1 << 30)] + sc[6:]
    rc, err = xg.vecs_check(bad, 32, 1, [S << 30], scatter=True)
    assert rc == xg.EARG and "overlap" in err
    assert time.monotonic() - t0 < 5.0


# ------------------------------------------------------------------ 5. the tile arithmetic
TB, TP = 32768, 256


@pytest.mark.parametrize("length", [1, 15, 16, 17, 127, 128, 129, 1000, 32767, 32768, 32769, 65541])
def test_pieces_of_a_row_are_its_blocks_cut_at_the_tile_size(xg, length):
    """every tile and lane of a row, in order, gives exactly the row's blocks cut at 32 KiB; lanes past a
    tile's last piece give nothing; a tile holds at most 256 pieces and (short blocks) 32 KiB"""
    for count in (1, 255, 256, 257, 513):
        so, do, ss, ds = 1000, 5000, length, length + 37
        row = (0, 1, so, do, ss, ds, length, count)
        want = []
        for j in range(count):
            for o in range(0, length, TB):
                want.append((so + j * ss + o, do + j * ds + o, min(TB, length - o)))
        tiles = xg.vec_row_tiles(length, count)
        bpt = max(1, min(TP, TB // length))
        assert tiles == (-(-count // bpt) if length <= TB else count * -(-length // TB))
        got = []
        for t in range(tiles):
            lanes = range(TP) if bpt > 1 or t in (0, tiles - 1) else (0, 1, TP - 1)
            live = [p for p in (xg.vec_piece_at(row, t, i) for i in lanes) if p[2] > 0]
            assert xg.vec_piece_at(row, t, 0)[2] > 0
            assert len(live) <= TP and (length > TB or sum(p[2] for p in live) <= max(TB, length))
            got += live
        assert got == want
        assert xg.vec_piece_at(row, tiles, 0) is None and xg.vec_piece_at(row, 0, TP) is None
        assert xg.vec_rows_tiles([row, (0, 1, 0, 0, 0, 0, 0, 5), row]) == [0, tiles, tiles, 2 * tiles]
