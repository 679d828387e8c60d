"""Plans that put the solo engine's descriptors at the ends of their offset windows, and a harness
that judges every byte of a RECV region of many GiB without moving it across PCIe.

A solo piece reaches the kernel as offsets in granules from the segment's lowest source and
destination (csrc/host/solo.c): 24 bits each in the PACKED form of 16-wave rails, 32 bits each in
the WIDE form of one-wave rails.  The plans here (window_steps, split_steps) state their copies
relative to those two bases -- the hulls start EDGE bytes into their regions -- and reach the top
of the fields: the regions are 256 MiB to 32 GiB of address space, the bytes moved a few hundred
KiB.  SparsePlan (host only) holds what such a plan reads and must write; SparseSynth runs it:
SEND is written only where copies read, every destination is read back with a guard on both
sides and compared byte for byte with the in-order numpy execution, and the rest of RECV is
checksummed on the device in 1 MiB spans against the checksum of that many poison bytes."""
import bisect
import ctypes as C

import numpy as np
import pytest

from synth_plan import PIECE, SOLO_LENS, Synth, _compare, _rails, _segment, _solo_pays, _up16

EDGE = 4096                             # a hull starts this far into its region and ends this far before its end
GUARD = 4096                            # bytes read back on both sides of every destination
SPAN = 1 << 20                          # the rest of RECV, and all of SEND, is checksummed in spans of this length
POISON = 0xA5

# top: the granule offset of the farthest piece (1 KiB); pats: two granule offsets of alternating
# bits; bits: single-bit granule offsets.  P and W1 end exactly at the window (top + the piece's
# granules = 2^24, 2^32); W4 and W16 are the smallest hulls that set bit 31 of a granule offset
# (just over 8 and 32 GiB), so 0xAAAAAAAA lies outside them and 0x2AAAAAAA stands in for it.
FORMS = {
    "P": dict(G=16, waves=16, top=(1 << 24) - 64, pats=(0x555540, 0xAAAA80), bits=range(19, 24), window=1 << 24,
              lens=[1024, 16, 1040]),
    "W1": dict(G=1, waves=1, top=(1 << 32) - 1024, pats=(0x55555555, 0xAAAAAAAA), bits=range(23, 32),
               window=1 << 32, lens=SOLO_LENS[1]),
    "W4": dict(G=4, waves=1, top=1 << 31, pats=(0x55555555, 0x2AAAAAAA), bits=range(23, 31), window=1 << 32,
               lens=SOLO_LENS[4]),
    "W16": dict(G=16, waves=1, top=1 << 31, pats=(0x55555555, 0x2AAAAAAA), bits=range(23, 31), window=1 << 32,
                lens=SOLO_LENS[16]),
}
P_PIECES = 16 * 16 + 16                 # (P): enough pieces for 16 rails of 16 waves
STEP_SIZES = [5, 1, 12, 1, 1, 40, 3, 27]


class _Bump:
    """low offsets, ascending, each behind a gap of 16..48 B, at a phase that is a multiple of G"""

    def __init__(self, G, mod):
        self.G, self.mod, self.cur, self.i = G, mod, 2 * EDGE, 0

    def take(self, n):
        at = _up16(self.cur) + 16 * (1 + self.i % 3) + (self.G * (self.i % self.mod)) % 16
        self.cur, self.i = at + n, self.i + 1
        return at


def _window_copies(form, far=0):
    """-> (stretch, rest): copies (src, dst, len) in bytes from the hull bases.  `far`: the pieces
    at the top stand that many granules further (split_steps).  A destination is written once, so
    only one copy ends at the top of the destination hull and only one starts at its base: the
    second visit to either corner stands one piece and a gap of 16 B + a granule inside; sources
    are only read, so both visits to a source corner are exact."""
    f = FORMS[form]
    G, lens = f["G"], f["lens"]
    odd = G if G < 16 else 0
    top = (f["top"] + far) * G
    top2 = f["top"] * G - PIECE - 16 - odd
    low2 = PIECE + 16 + odd
    stride = PIECE + 16 + odd
    # one-piece copies high on both sides, one per step (synth_plan._row_steps): on a 16-wave rail
    # a row of 16 of them holds the ends of 15 steps
    stretch = [(0, top, PIECE), (top, top2, PIECE)]
    for i in range(2, 17 if f["waves"] == 16 else 5):
        stretch.append((top2 - (i - 2) * stride, top2 - (i - 1) * stride, PIECE))
    rest = [(top, 0, PIECE), (0, low2, PIECE)]
    p0, p1 = f["pats"]
    for k in range(3):                  # the patterns against each other, and 4 KiB neighbours at other lengths
        n = PIECE if k == 0 else lens[k % len(lens)]
        rest.append((p0 * G + k * 4096, p1 * G + k * 4096, n))
        rest.append((p1 * G + k * 4096, p0 * G + k * 4096, n))
    ls, ld = _Bump(G, 7), _Bump(G, 5)
    for j, b in enumerate(f["bits"]):   # one bit on one side, none of the high bits on the other
        n = lens[(2 * j) % len(lens)]
        rest.append((G << b, ld.take(n), n))
        n = lens[(2 * j + 1) % len(lens)]
        rest.append((ls.take(n), G << b, n))
    assert max(ls.cur, ld.cur) < G << min(f["bits"])
    if form == "P":                     # fill 16 rails: 1 KiB copies scattered over both hulls, one per 4 KiB slot
        nslots = (f["top"] * G + PIECE) // 4096
        have = sum(-(-n // PIECE) for (_s, _d, n) in stretch + rest)
        j = 0
        while have < P_PIECES:
            s, d = (j * 40503 + 77) % nslots, (j * 30011 + 1234) % nslots
            j += 1
            if min(s, d) < 2048 or max(s, d) >= nslots - 8:      # the low offsets and the stretch live there
                continue
            rest.append((s * 4096 + 2560, d * 4096 + 2560, PIECE))
            have += 1
    return stretch, rest


def _cut(copies, sizes=STEP_SIZES):
    steps, b, i = [], 0, 0
    while b < len(copies):
        steps.append(copies[b:b + sizes[i % len(sizes)]])
        b += len(steps[-1])
        i += 1
    return steps


def _place(rel_steps, hull):
    """steps of (src, dst, len) from the hull bases -> SEND -> RECV steps, send_bytes, recv_bytes"""
    steps = [[(0, EDGE + s, 1, EDGE + d, n) for (s, d, n) in st] for st in rel_steps]
    return steps, hull + 2 * EDGE, hull + 2 * EDGE


def _hull(form, far=0):
    f = FORMS[form]
    return (f["top"] + far) * f["G"] + PIECE


def window_steps(form, pad=0):
    """the stretch of one-piece steps, `pad` steps that move nothing, then the other copies in
    steps of 1-40, between two steps that move nothing (build_segments trims those: the plan as
    stated is a launched segment, synth_plan._segment of it can be armed); both hulls are
    _hull(form) bytes"""
    stretch, rest = _window_copies(form)
    return _place([[]] + [[c] for c in stretch] + [[]] * pad + _cut(rest) + [[]], _hull(form))


def window_plan(form, rails_max):
    """window_steps with the fewest empty steps at which the cost model takes rails"""
    f = FORMS[form]
    for pad in range(0, 1900, 4):
        steps, send_bytes, recv_bytes = window_steps(form, pad)
        seg = _segment(steps)
        nbytes = sum(c[4] for st in seg for c in st)
        if _solo_pays(nbytes, len(seg), _rails(steps, rails_max, f["waves"]), f["waves"], sum(1 for st in seg if st),
                      f["G"]):
            return steps, send_bytes, recv_bytes
    raise AssertionError("no rail routing at this size")


def _split_pays(nbytes, n, ncut, gran):
    """plan_tables.cc build_segments' inequality for consecutive solo launches, mirrored only to
    SIZE the plan (10 % kept in hand); the asserted segment and rail counts are the check"""
    traffic = 2.0 * nbytes
    return 1.1 * (ncut * 6e-6 + traffic / (6e12 * gran / 16.0) + n * 0.05e-6) < traffic / 5e12 + n * 1.0e-6


def split_steps(form, variant):
    """window_steps(form) with the pieces at the top one granule further: each hull is the window
    plus one granule, so no single table holds the plan.
    "steps": -> steps, send_bytes, recv_bytes, cut.  Steps [0, cut) read from the source base on
    and write up to the destination top, steps [cut, ..) read up to the source top and write from
    the destination base on; each part fits a window, steps [0, cut] do not, and there are steps
    enough for solo_split's two launches to beat the grid engine.
    "one_step": -> steps, send_bytes, recv_bytes, None.  Step 0 alone holds both ends of both
    hulls, so nothing can be cut."""
    f = FORMS[form]
    G, window = f["G"], f["window"] * f["G"]
    stretch, rest = _window_copies(form, far=1)
    hull = _hull(form, far=1)
    assert hull == window + G
    if variant == "one_step":
        ends = [c for c in stretch + rest if (c[0] == 0 and c[1] + c[2] == hull) or (c[0] + c[2] == hull and c[1] == 0)]
        assert len(ends) == 2
        others = [c for c in stretch + rest if c not in ends]
        steps, send_bytes, recv_bytes = _place([ends] + _cut(others), hull)
        return steps, send_bytes, recv_bytes, None
    assert variant == "steps"

    def part(i, c):
        s, d, n = c
        if s + n > window:
            return 1
        if d + n > window or s < G:
            return 0
        if d < G:
            return 1
        return i % 2
    first = next(c for c in rest if c[0] + c[2] == hull and c[1] == 0)          # the copy that forces the cut
    a = [[c for i, c in enumerate(x) if part(i, c) == 0] for x in (stretch, rest)]
    b = [[c for i, c in enumerate(x) if part(i, c) == 1 and c != first] for x in (stretch, rest)]
    for pad in range(0, 1900, 4):
        head = [[c] for c in a[0]] + [[]] * pad + _cut(a[1])
        rel = head + [[first]] + [[c] for c in b[0]] + _cut(b[1])
        if _split_pays(sum(c[2] for st in rel for c in st), len(rel), 2, G):
            steps, send_bytes, recv_bytes = _place(rel, hull)
            return steps, send_bytes, recv_bytes, len(head)
    raise AssertionError("no split at this size")


def bases(steps):
    """the lowest source and destination offset of the steps' copies: the kernel's bases"""
    return min(c[1] for st in steps for c in st), min(c[3] for st in steps for c in st)


# ------------------------------------------------------------------ what a sparse plan reads and must write
class SparsePlan:
    """host only: the seeded bytes of every source range, the windows of RECV around the
    destinations with their expected bytes, and the spans that cover the rest of RECV"""

    def __init__(self, steps, send_bytes, recv_bytes, seed=0):
        assert all(sb == 0 and db == 1 for st in steps for (sb, _so, db, _do, _n) in st)     # SEND -> RECV only
        self.steps, self.send_bytes, self.recv_bytes = steps, send_bytes, recv_bytes
        copies = [c for st in steps for c in st if c[4] > 0]
        assert all(0 <= so and so + n <= send_bytes and 0 <= do and do + n <= recv_bytes for (_a, so, _b, do, n) in copies)
        rng = np.random.default_rng(seed)
        self.sources = []               # disjoint (offset, bytes), ascending
        for lo, hi in self._merge(sorted((so, so + n) for (_a, so, _b, _do, n) in copies)):
            self.sources.append((lo, rng.integers(0, 256, hi - lo, dtype=np.uint8)))
        self._starts = [lo for lo, _v in self.sources]
        self.windows = self._merge(sorted((max(0, do - GUARD), min(recv_bytes, do + n + GUARD))
                                          for (_a, _so, _b, do, n) in copies))
        self._wlo = [lo for lo, _hi in self.windows]
        self.expected = [np.full(hi - lo, POISON, np.uint8) for lo, hi in self.windows]
        for st in steps:                # in order; one step = simultaneous copies
            for (_a, so, _b, do, n) in st:
                if n:
                    w = self.window_of(do)
                    self.expected[w][do - self.windows[w][0]:do - self.windows[w][0] + n] = self.src(so, n)
        self.rest, at = [], 0           # the complement of the windows, in spans of SPAN and the remainders
        for lo, hi in self.windows + [(recv_bytes, recv_bytes)]:
            while at < lo:
                self.rest.append((at, min(SPAN, lo - at)))
                at += self.rest[-1][1]
            at = hi
        self.send_spans = [(o, min(SPAN, send_bytes - o)) for o in range(0, send_bytes, SPAN)]

    @staticmethod
    def _merge(iv):
        out = []
        for lo, hi in iv:
            if out and lo <= out[-1][1]:
                out[-1] = (out[-1][0], max(out[-1][1], hi))
            else:
                out.append((lo, hi))
        return out

    def src(self, so, n):
        i = bisect.bisect_right(self._starts, so) - 1
        lo, v = self.sources[i]
        assert lo <= so and so + n <= lo + len(v)
        return v[so - lo:so - lo + n]

    def window_of(self, at):
        """index of the window that holds RECV[at], or -1"""
        i = bisect.bisect_right(self._wlo, at) - 1
        return i if i >= 0 and at < self.windows[i][1] else -1

    def check_window(self, w, got):
        """got: RECV[windows[w]) after a run -- against the numpy execution, naming the copy"""
        _compare(self.steps, got, self.expected[w], base=self.windows[w][0])

    def check_rest(self, chks, poison_chk):
        """chks: the device checksums of self.rest; poison_chk(n): that of n poison bytes"""
        bad = [(off, n) for (off, n), c in zip(self.rest, chks) if c != poison_chk(n)]
        if bad:
            off, n = bad[0]
            near = min((min(abs(off - do), abs(off + n - do)), s, do, ln) for s, st in enumerate(self.steps)
                       for (_a, _so, _b, do, ln) in st)
            pytest.fail("%d spans of RECV outside every destination's guard were written; the first is RECV[%d..%d), "
                        "%d B from the copy of %d B of step %d (RECV[%d..%d))"
                        % (len(bad), off, off + n, near[0], near[3], near[1], near[2], near[2] + near[3]))

    def judge_stores(self, stores):
        """stores: (RECV offset, bytes) in execution order, e.g. from interpreting the solo tables
        on the CPU: the same two checks a GPU run gets"""
        got = [np.full(hi - lo, POISON, np.uint8) for lo, hi in self.windows]
        stray = set()
        for do, v in stores:
            at = do
            while at < do + len(v):
                w = self.window_of(at)
                if w < 0:               # outside every window: its span's checksum would change
                    i = bisect.bisect_right(self._wlo, at)
                    end = min(do + len(v), self.windows[i][0] if i < len(self.windows) else do + len(v))
                    stray.add(at)
                else:
                    lo, hi = self.windows[w]
                    end = min(do + len(v), hi)
                    got[w][at - lo:end - lo] = v[at - do:end - do]
                at = end
        for w in range(len(self.windows)):
            self.check_window(w, got[w])
        if stray:                       # the span that holds it no longer sums to poison
            at = min(stray)
            self.check_rest([1 if off <= at < off + n else 0 for off, n in self.rest], lambda n: 0)
            pytest.fail("a store at RECV[%d], outside the region" % at)


# ------------------------------------------------------------------ ... and its run on the device
class SparseSynth(Synth):
    """regions at full size, of which only the source ranges are written and only the windows
    are read back; Synth's plan load and timed run"""

    def __init__(self, xg, ctx, send_bytes, recv_bytes, steps, seed=0):
        import xg_oracle as O
        d = xg.device()
        self.xg, self.d, self.O = xg, d, O
        self.plan = SparsePlan(steps, send_bytes, recv_bytes, seed)
        rb = (C.c_int64 * xg.NBUF)(send_bytes, recv_bytes, 0, 0, 0)
        self.r = C.c_void_p()
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(self.r)) == 0
        try:
            for lo, v in self.plan.sources:
                buf = v.tobytes()
                assert d.xg_regions_write(self.r, xg.BUF_SEND, lo, buf, len(buf)) == 0
            self._rest = self._spans(xg.BUF_RECV, self.plan.rest)
            self._send = self._spans(xg.BUF_SEND, self.plan.send_spans)
            self._poison_chk = {}
            self.send_before = self._chk(self._send)
            self._load(ctx, send_bytes, recv_bytes, steps)
        except BaseException:
            d.xg_regions_free(self.r)
            raise
        self.steps = steps

    def _spans(self, buf, spans):
        return (self.xg.BufSpan * max(1, len(spans)))(*[self.xg.BufSpan(buf, 0, o, n) for o, n in spans]), len(spans)

    def _chk(self, spans):
        """xg_chk_spans of the whole list, one launch"""
        arr, n = spans
        out = (C.c_uint64 * max(1, n))()
        assert self.d.xg_chk_spans(self.r, arr, n, out) == 0
        return list(out)[:n]

    def poison_chk(self, n):
        if n not in self._poison_chk:   # a span's words count from its first byte: the length alone decides
            self._poison_chk[n] = self.O.chk64(np.full(n, POISON, np.uint8))
        return self._poison_chk[n]

    def run_checked(self, runs=3):
        """`runs` runs from a poisoned RECV each: every window against numpy, every other span of
        RECV still poison, the stamps ordered and inside the wall time; then SEND unchanged"""
        n = max(1, len(self.steps))
        for rep in range(runs):
            self.poison()
            done, post, wall = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
            assert self.d.xg_plan_run(self.p, done, post, C.byref(wall)) == 0
            for w, (lo, hi) in enumerate(self.plan.windows):
                out = C.create_string_buffer(hi - lo)
                assert self.d.xg_regions_read(self.r, 1, lo, out, hi - lo) == 0
                self.plan.check_window(w, np.frombuffer(out.raw, np.uint8))
            self.plan.check_rest(self._chk(self._rest), self.poison_chk)
            done = list(done)[:len(self.steps)]
            assert all(0 <= a <= b for a, b in zip(done, done[1:])), (rep, done)
            assert done[-1] <= wall.value + 1e-4, (rep, done[-1], wall.value)
        after = self._chk(self._send)
        bad = [sp for sp, a, b in zip(self.plan.send_spans, self.send_before, after) if a != b]
        assert not bad, ("SEND was written", len(bad), bad[:3])
