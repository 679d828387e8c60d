"""xg_small_index (include/xg_sched.h; xg_small_piece_at in csrc/host/pieces.c): where workgroup b
of a small-piece launch (copy_kernel_q) copies -- the row, the offset inside the copy and the
byte count, by arithmetic alone.  Checked against enumeration: over all workgroups of a launch
every byte of every copy is covered exactly once, no piece runs past its copy, and the order is
the one the header states (groups of k copies, piece by piece round the group)."""
import pytest

LENS = [16, 4080, 4096, 4112, 8208, 3 * 4096, 5 * 4096 + 48, 1 << 20]
PIECES = [4096, 8192]
COPIES = [1, 2, 7, 449]
ORDERS = [1, 2, 8, 32]


def _pieces(xg, copies, length, piece, k, lo=0, hi=None):
    ppc = -(-length // piece)
    hi = copies * ppc if hi is None else hi
    return [xg.small_piece_at(b, copies, length, piece, k) for b in range(lo, hi)]


def _assert_cover(got, copies, length, piece):
    """every byte of every copy exactly once, pieces inside their copy and at most `piece` long"""
    seen = {}
    for copy, off, n in got:
        assert 0 <= copy < copies and off % piece == 0 and 0 < n <= piece and off + n <= length
        assert n == piece or off + n == length               # only a copy's last piece is short
        assert (copy, off) not in seen
        seen[(copy, off)] = n
    assert len(seen) == copies * -(-length // piece)
    for c in range(copies):
        assert sum(n for (cc, _o), n in seen.items() if cc == c) == length


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("length", LENS)
def test_cover_and_order(xg, length, piece):
    ppc = -(-length // piece)
    for copies in COPIES:
        if length == 1 << 20 and copies == 449:
            copies_k = [(copies, 1), (copies, 32)]          # 115 k workgroups per order: two orders are enough
        else:
            copies_k = [(copies, k) for k in ORDERS]
        for copies, k in copies_k:
            got = _pieces(xg, copies, length, piece, k)
            _assert_cover(got, copies, length, piece)
            # the stated order: full groups of k copies, then a last group of copies % k
            want = []
            for g0 in range(0, copies, k):
                kk = min(k, copies - g0)
                want += [(g0 + i, j * piece, min(piece, length - j * piece)) for j in range(ppc) for i in range(kk)]
            assert got == want, (copies, length, piece, k)
            assert xg.small_piece_at(copies * ppc, copies, length, piece, k) is None    # past the launch


def test_last_group_shorter_than_k(xg):
    """7 copies in groups of 2, 8 and 32: groups of 2 + 2 + 2 + 1, one of 7, one of 7"""
    for k, sizes in ((2, [2, 2, 2, 1]), (8, [7]), (32, [7])):
        got = _pieces(xg, 7, 8208, 4096, k)
        at = 0
        for g, kk in enumerate(sizes):
            grp = got[at: at + 3 * kk]
            assert [c for c, _o, _n in grp] == [g * k + i for _j in range(3) for i in range(kk)]
            assert [o for _c, o, _n in grp] == [j * 4096 for j in range(3) for _i in range(kk)]
            at += 3 * kk
        assert at == len(got)


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("k", ORDERS)
def test_dispatch_cuts_at_every_workgroup(xg, piece, k):
    """a three-copy launch cut into two dispatches at every workgroup boundary (a cut inside a copy
    included): dispatch [0, cut) and dispatch [cut, W), each workgroup at base + its index, cover
    every byte exactly once together"""
    length, copies = 5 * 4096 + 48, 3
    W = copies * -(-length // piece)
    whole = _pieces(xg, copies, length, piece, k)
    for cut in range(W + 1):
        first = _pieces(xg, copies, length, piece, k, 0, cut)
        second = _pieces(xg, copies, length, piece, k, cut, W)
        assert first + second == whole
        _assert_cover(first + second, copies, length, piece)


def test_bad_arguments(xg):
    assert xg.small_piece_at(-1, 3, 4096, 4096) is None
    assert xg.small_piece_at(0, 0, 4096, 4096) is None
    assert xg.small_piece_at(0, 3, 0, 4096) is None
    assert xg.small_piece_at(0, 3, 4096, 4096, 0) is None
    assert xg.small_piece_at(0, 1 << 31, 4096, 4096) is None         # more workgroups than 32 bits index
    assert xg.small_piece_at(0, 3, 4096, 4096) == (0, 0, 4096)
