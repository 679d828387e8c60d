"""The step engines' launch counters across their 32-bit wrap (include/xg_sched.h xg_eng_*), on the CPU.

EngineState's counters (kernels.h) are cumulative 32-bit words that no launch resets.  A long-lived
plan carries them past 2^31 and 2^32: the grid engine's `count` after some 65,000 launches of a
256-workgroup, 255-step plan, the solo engine's `arrive`, `fin[line]` and `rails` after 2^32 / R,
2^32 / per_line and 2^32 / L armed launches.  No run on a device gets there, so the decisions the
kernels take on these words -- which value a barrier waits for, who arrived last, which rail lets
rail 0 announce itself, which finished rail tells the host -- are functions shared by the kernels
and libxghost, and a walker in plain Python integers plays launches around the wrap against them:
the counters are Python's, reduced modulo 2^32 after every increment as the device words are; every
decision is the C function's.

The negative control transcribes the solo engine's earlier formulas, which read the launch boundary
off the raw counter value ((old // R + 1) * R, a % per_line, b % L), and runs them through the same
walker: they hold for every power of two and fail for divisors that do not divide 2^32.
"""
import random

import pytest

M = 1 << 32
LINES = 16


def _lines(R):
    return min(R, LINES)


def _per_line(R, line):
    return len(range(line, R, _lines(R)))          # rails r with r % L == line


def _i32(x):
    x &= M - 1
    return x - M if x >= M >> 1 else x


# ---------------------------------------------------------------------- grid engine
GRID_W = [1, 3, 4, 255, 256, 304]
GRID_STEPS = [1, 2, 12]
PLACES = ["boundary", "pre", "first", "middle", "last", "nowhere"]


def _grid_base(place, point, W, steps, armed):
    """the tickets taken before launch 1 such that `point` (2^32 or 2^31) falls at `place` of it;
    inside a barrier: behind max(1, W // 2) of its W tickets (W = 1: on its one ticket)"""
    T = W * (steps + armed)
    j = max(1, W // 2)
    if place == "boundary":
        return (point - T) % M                     # the launch's last arrival takes the counter to `point`
    if place == "pre":
        return (point - j) % M if armed else None
    if place == "nowhere":
        return 12345
    b = {"first": 0, "middle": steps // 2, "last": steps - 1}[place]
    return (point - (armed * W + b * W + j)) % M


def _grid_barrier(h, rng, W, count, target, has_last):
    """W arrivals in a random order; -> the counter behind them"""
    order = list(range(W))
    rng.shuffle(order)
    lasts = []
    for k, wg in enumerate(order, 1):
        count = (count + 1) % M
        assert bool(h.xg_eng_waiting(count, target)) == (k < W), (W, k, count, target)
        if has_last and h.xg_eng_last(count, target):
            lasts.append(k)
    if has_last:
        assert lasts == [W], (W, count, target, lasts)          # exactly one last arriver: the W-th
    assert count == target                                      # the barrier opens on its own W-th ticket
    # workgroups that went on take up to W - 1 tickets of the next barrier: this one stays open
    for ahead in {1, (W - 1) // 2, W - 1} - {0}:
        assert not h.xg_eng_waiting((count + ahead) % M, target), (W, count, ahead)
    return count


def _grid_launch(h, rng, W, steps, armed, base, count):
    b = base
    if armed:                       # the pre-barrier: nobody is "last", its target is the steps' base
        b = h.xg_eng_grid_pre_target(base, W)
        assert b == (base + W) % M
        count = _grid_barrier(h, rng, W, count, b, False)
    for s in range(steps):
        target = h.xg_eng_grid_target(b, W, s)
        assert target == (base + (armed + s + 1) * W) % M
        count = _grid_barrier(h, rng, W, count, target, True)
    return count


@pytest.mark.parametrize("point", [1 << 32, 1 << 31])
def test_grid_barriers_across_the_wrap(xg, point):
    """W in GRID_W, 1 / 2 / 12 steps, armed and not; 2^32 (2^31) at a launch boundary exactly, inside
    the armed pre-barrier, inside the first, a middle and the last barrier of launch 1, and nowhere;
    two launches each, the host's base advanced by xg_eng_grid_tickets as launch_seg does"""
    h = xg.host()
    rng = random.Random(point % 1000003)
    seen = 0
    for W in GRID_W:
        for steps in GRID_STEPS:
            for armed in (0, 1):
                T = h.xg_eng_grid_tickets(W, steps, armed)
                assert T == W * (steps + armed)
                for place in PLACES:
                    base = _grid_base(place, point, W, steps, armed)
                    if base is None:
                        continue
                    count = base
                    crossed = False
                    for _launch in range(2):
                        before = count
                        count = _grid_launch(h, rng, W, steps, armed, base, count)
                        base = (base + T) % M
                        assert count == base
                        crossed |= any((before + t) % M == point % M for t in range(1, T + 1))
                    assert crossed == (place != "nowhere"), (W, steps, armed, place)
                    seen += 1
    assert seen == len(GRID_W) * len(GRID_STEPS) * (len(PLACES) + len(PLACES) - 1)


# ---------------------------------------------------------------------- solo engine
class Shared:
    """the functions the kernel calls, through libxghost"""

    def __init__(self, h):
        self.h = h

    def arrive_target(self, R, base, old):
        return self.h.xg_eng_solo_arrive_target(base, R)

    def waiting(self, count, target):
        return bool(self.h.xg_eng_waiting(count, target))

    def line_last(self, a, base, R, line):
        return bool(self.h.xg_eng_solo_line_last(a, base, R, line))

    def rails_last(self, b, base, R):
        return bool(self.h.xg_eng_solo_rails_last(b, base, R))


class Earlier:
    """the solo engine's formulas before the host kept a base, transcribed: rail 0's target from
    what its own increment returned, the last of a line and the last line by remainder"""

    def arrive_target(self, R, base, old):
        return (old // R + 1) * R % M

    def waiting(self, count, target):
        return _i32(count - target) < 0

    def line_last(self, a, base, R, line):
        return a % _per_line(R, line) == 0

    def rails_last(self, b, base, R):
        return b % _lines(R) == 0


def _solo_launch(rules, rng, R, base, st):
    """one armed launch of R rails over the words st = [arrive, rails, fin[16]]: the rails become
    resident in a random order, then finish in another.  False if rail 0 is released at any moment
    but the R-th arrival of this launch, or `done` is rung by anyone but the last rail to finish."""
    L = _lines(R)
    order = list(range(R))
    rng.shuffle(order)
    target = None
    for k, rail in enumerate(order, 1):
        old = st[0]
        st[0] = (st[0] + 1) % M
        if rail == 0:
            target = rules.arrive_target(R, base, old)
        if target is not None and (not rules.waiting(st[0], target)) != (k == R):
            return False
    rng.shuffle(order)
    rang = []
    for k, rail in enumerate(order, 1):
        line = rail % L
        st[2][line] = (st[2][line] + 1) % M
        if not rules.line_last(st[2][line], base, R, line):
            continue
        st[1] = (st[1] + 1) % M
        if rules.rails_last(st[1], base, R):
            rang.append(k)
    return rang == [R]


def _solo_starts(R):
    """{counter: the armed launches before the walk}: two launches before `arrive`, a `fin` word
    (one start per distinct per_line) and `rails` pass 2^32"""
    out = {}
    for name, d in ([("arrive", R), ("rails", _lines(R))] +
                    [("fin/%d" % q, q) for q in sorted({_per_line(R, l) for l in range(_lines(R))})]):
        passing = -(-M // d) - 1                   # the launch (by its base) that takes the word to >= 2^32
        out[name] = (passing - 2) % M
    return out


def _walk(rules, R, seed):
    """-> the counters whose walk (six armed launches from two before the wrap) went wrong"""
    bad = []
    for name, start in _solo_starts(R).items():
        rng = random.Random(1000 * R + seed)
        st = [start * R % M, start * _lines(R) % M, [start * _per_line(R, l) % M for l in range(_lines(R))] +
              [0] * (LINES - _lines(R))]
        wrapped = False
        for i in range(6):
            before = (st[0], st[1], list(st[2]))
            ok = _solo_launch(rules, rng, R, (start + i) % M, st)
            wrapped |= st[0] < before[0] or st[1] < before[1] or any(a < b for a, b in zip(st[2], before[2]))
            if not ok:
                bad.append(name)
                break
        else:
            assert wrapped, (R, name)              # the walk did take a counter through 2^32
    return bad


def test_solo_geometry_and_state(xg):
    """lines, rails per line and the words after `armed` launches, against Python integers"""
    h = xg.host()
    for R in range(1, 513):
        assert h.xg_eng_solo_lines(R) == _lines(R)
        per = [h.xg_eng_solo_per_line(R, l) for l in range(_lines(R))]
        assert per == [_per_line(R, l) for l in range(_lines(R))] and sum(per) == R
        for armed in (0, 1, 5, -(-M // R) - 1, -(-M // R) % M, (1 << 28) - 1, 1 << 28, (1 << 31) + 7, M - 3, M - 1):
            s = xg.EngSoloState()
            h.xg_eng_solo_state_after(R, armed, s)
            assert (s.arrive, s.rails, s.go) == (armed * R % M, armed * _lines(R) % M, armed)
            assert list(s.fin) == [armed * _per_line(R, l) % M for l in range(_lines(R))] + [0] * (LINES - _lines(R))


def test_solo_counters_across_the_wrap(xg):
    """every R in 1 .. 512, each counter from two armed launches before it passes 2^32, six launches
    in random arrival and finishing orders: rail 0 released exactly at the R-th arrival of its own
    launch, one ring per launch, from the last rail to finish.  The earlier formulas through the same
    walker: right for every power of two, wrong for some other R -- the walker sees the defect."""
    shared = Shared(xg.host())
    wrong_now = {R: _walk(shared, R, 1) for R in range(1, 513)}
    assert not any(wrong_now.values()), {R: b for R, b in wrong_now.items() if b}
    wrong_then = {R: _walk(Earlier(), R, 1) for R in range(1, 513)}
    pow2 = [R for R in range(1, 513) if R & (R - 1) == 0]
    assert not any(wrong_then[R] for R in pow2), {R: wrong_then[R] for R in pow2 if wrong_then[R]}
    failing = [R for R in range(1, 513) if wrong_then[R]]
    assert failing and all(M % R for R in failing)
    # the cases the device tests take: 3 rails (arrive, rails), 37 and 48 (per_line 3: fin as well)
    assert {"arrive", "rails"} <= set(wrong_then[3]), wrong_then[3]
    assert {"arrive", "fin/3"} <= set(wrong_then[37]) and {"arrive", "fin/3"} <= set(wrong_then[48]), wrong_then
    print("earlier formulas: wrong for %d of 512 rail counts, the first %s" % (len(failing), failing[:8]))
