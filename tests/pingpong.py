"""Two plans whose image after k rounds is different for every k (TEST HELPER for test_pingpong.py
and test_gpu_back_to_back.py; plain Python, the generator needs no GPU).

Every schedule the product builds reads SEND and writes fixed RECV slots: one correct run leaves the
same image as twenty, so a lost, repeated, reordered or overlapping run cannot show.  Here RECV holds
two areas, A and B, of n slots each, every slot between >= 16 poisoned bytes, and two synthetic
one-GPU plans over ONE xg_regions:

    plan a    A[i] -> B[next(i)] for every i, the copies spread over several steps
    plan b    B[i] -> A[i]       for every i, in one step

Slot i is lens[i % L] bytes long (L = len(lens)) and next(i) = (i + L) mod n is the next slot of
the same length, so with one length (L = 1) next(i) = i + 1.  One ROUND is a then b: it moves every
A slot to the next one of its length.  The slots of one length form a ring of n / L slots, so the
images after 0 .. n / L - 1 rounds are pairwise distinct whenever the slots of some ring hold
pairwise distinct bytes (a random image: test_pingpong.py asserts it), and in a round each plan
reads only what the other plan's previous launch wrote.  Plan a reads A and writes B: no step of it
reads or writes what another step writes, so it stays eligible for every engine, xg_engine_rail_safe
included.  SEND is never touched.

image(k) is the in-order numpy execution, Synth.expected over a's steps then over b's, k times --
never the library.  test_pingpong.py checks it against the closed form (the rotation).
"""
import ctypes as C
import types

import numpy as np

from synth_plan import Synth, _up16
from time_plan import devplan

SEND_BYTES = 4096                   # random bytes no plan reads or writes: they must stay as they are


class PingPong:
    """the generator's result: steps_a / steps_b (lists of steps of (src_buf, src_off, dst_buf,
    dst_off, len)), send_bytes / recv_bytes, flags (the xg_devplan flags of both plans), slots_a /
    slots_b ((offset, length) per slot), L, ring (= n / L: image(k) is distinct for k < ring)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def nxt(self, i):
        return (i + self.L) % len(self.slots_a)

    def round(self, send, recv):
        """RECV after one round from `recv`: Synth.expected of a, then of b"""
        for steps in (self.steps_a, self.steps_b):
            recv = Synth.expected(types.SimpleNamespace(send=send, recv=recv, steps=steps), recv)
        return recv

    def image(self, k, send, recv0):
        """RECV after k rounds from recv0"""
        recv = recv0.copy()
        for _ in range(k):
            recv = self.round(send, recv)
        return recv

    def images(self, kmax, send, recv0):
        """[image(0), ..., image(kmax)], each computed from the one before"""
        out = [recv0.copy()]
        for _ in range(kmax):
            out.append(self.round(send, out[-1]))
        return out

    def bytes_a(self):
        return sum(c[4] for st in self.steps_a for c in st)

    bytes_b = bytes_a               # b moves what a moved


def pingpong(lens, n, counts, phase=(0, 0), flags=0):
    """lens: the slot lengths, slot i lens[i % len(lens)] bytes; n: slots per area, a multiple of
    len(lens); counts: copies per step of plan a (their sum is n); phase: (A's, B's) offset mod 16
    of every slot; flags: both plans' xg_devplan flags."""
    L = len(lens)
    assert n % L == 0 and sum(counts) == n and all(x > 0 for x in lens)
    cur, areas = 0, []
    for ph in phase:
        slots = []
        for i in range(n):
            off = _up16(cur) + 16 * (1 + i % 3) + ph            # a poisoned gap of 16 .. 48 B (+ the phase)
            slots.append((off, lens[i % L]))
            cur = off + lens[i % L]
        areas.append(slots)
        cur = _up16(cur) + 64                                   # between the areas
    A, B = areas
    copies_a = [(1, A[i][0], 1, B[(i + L) % n][0], A[i][1]) for i in range(n)]
    steps_a, b = [], 0
    for k in counts:
        steps_a.append(copies_a[b:b + k])
        b += k
    steps_b = [[(1, B[i][0], 1, A[i][0], B[i][1]) for i in range(n)]]
    return PingPong(steps_a=steps_a, steps_b=steps_b, send_bytes=SEND_BYTES, recv_bytes=_up16(cur) + 32, flags=flags,
                    slots_a=A, slots_b=B, L=L, ring=n // L)


# ------------------------------------------------------------------ the cases
# env: the context's knobs.  gen: pingpong()'s arguments.  a / b: the form each plan must take under
# them, stated by hand (time_plan.form's fields, and `kinds`: the launches per kernel kind [PIECE,
# WAVE, SHIFT, EXTENT, SMALL] of xg_plan_kind_launches -- an engine segment is none of them).
# kmax: the most rounds a test posts on the case (< ring).
RAGGED, EXTENTS = 1, 2              # xg.DP_RAGGED, xg.DP_EXTENTS
N = 48
EVEN = [4] * 12                     # plan a: 12 steps of 4 copies
TAILED = [3] * 11 + [15]            # ... 11 steps of 3 and one of 15, which alone passes a small XG_ENGINE_MAX_STEP
EXT_LENS = [64, 300, 72, 129, 255, 100, 288, 177]
NONE = [0, 0, 0, 0, 0]


def _seg(steps, w, solo, **kw):
    return dict(steps=steps, w=w, solo=solo, **kw)


def _form(nsteps, launches, segs=(), chains=(), armed=0, graph_auto=1, kinds=NONE, gran=None):
    f = dict(nsteps=nsteps, launches=launches, segs=list(segs), chains=list(chains), armed=armed, graph_auto=graph_auto,
             kinds=list(kinds))
    if gran is not None:
        f["gran"] = gran
    return f


CASES = {
    # one solo segment each: 48 pieces of 1 KiB on 48 one-wave rails -- solo_engine_kernel<8, 1>
    "solo": dict(env={}, gen=dict(lens=[1024], n=N, counts=EVEN), kmax=19,
                 a=_form(12, 1, [_seg((0, 12), 48, 1, wv=1)], gran=[16]),
                 b=_form(1, 1, [_seg((0, 1), 48, 1, wv=1)], gran=[16])),
    # ... on 3 workgroup rails of 16 waves -- solo_engine_kernel<8, 16>
    "solo16": dict(env=dict(XG_SOLO_WAVES=16), gen=dict(lens=[1024], n=N, counts=EVEN), kmax=19,
                   a=_form(12, 1, [_seg((0, 12), 3, 1, wv=16)], gran=[16]),
                   b=_form(1, 1, [_seg((0, 1), 3, 1, wv=16)], gran=[16])),
    # slot length and phases odd: byte accesses -- solo_engine_kernel<4, 1, 1>
    "solo_g1": dict(env={}, gen=dict(lens=[1023], n=N, counts=EVEN, phase=(1, 3)), kmax=19,
                    a=_form(12, 1, [_seg((0, 12), 48, 1, wv=1)], gran=[1]),
                    b=_form(1, 1, [_seg((0, 1), 48, 1, wv=1)], gran=[1])),
    # a: one grid segment of 4 workgroups (a step is 4 units of 4 KiB) -- step_engine_kernel<1>; b: one launch
    "grid": dict(env=dict(XG_ENGINE_SOLO=0), gen=dict(lens=[4096], n=N, counts=EVEN), kmax=19,
                 a=_form(12, 1, [_seg((0, 12), 4, 0, b=1)], gran=[16]),
                 b=_form(1, 1, kinds=[1, 0, 0, 0, 0])),
    # a: a chain of 12 copy_kernel_g launches, posted one by one
    "launches": dict(env=dict(XG_ENGINE_MAX_STEP=0, XG_GRAPH=0), gen=dict(lens=[1024], n=N, counts=EVEN), kmax=19,
                     a=_form(12, 12, chains=[(0, 12)], kinds=[12, 0, 0, 0, 0]),
                     b=_form(1, 1, kinds=[1, 0, 0, 0, 0])),
    # ... replayed as one graph (b, a single launch, is never captured: replay, launch, replay, ...)
    "graph": dict(env=dict(XG_ENGINE_MAX_STEP=0, XG_GRAPH=1), gen=dict(lens=[1024], n=N, counts=EVEN), kmax=19,
                  graph=1,
                  a=_form(12, 12, chains=[(0, 12)], kinds=[12, 0, 0, 0, 0]),
                  b=_form(1, 1, kinds=[1, 0, 0, 0, 0])),
    # a: a grid segment of 11 steps of 12 KiB and a launch of 60 KiB, above XG_ENGINE_MAX_STEP, in one graph
    "grid_launch_graph": dict(env=dict(XG_ENGINE_SOLO=0, XG_GRAPH=1, XG_ENGINE_MAX_STEP=32768),
                              gen=dict(lens=[4096], n=N, counts=TAILED), kmax=19, graph=1,
                              a=_form(12, 2, [_seg((0, 11), 3, 0, b=1)], kinds=[1, 0, 0, 0, 0], gran=[16]),
                              b=_form(1, 1, kinds=[1, 0, 0, 0, 0])),
    # no graph knob: a is a solo segment and a launch, two launches of a one-GPU plan under 16 MiB,
    # which the defaults replay as a graph (graph_auto)
    "default_graph": dict(env=dict(XG_ENGINE_MAX_STEP=8192), gen=dict(lens=[1024], n=N, counts=TAILED), kmax=19,
                          graph=1,
                          a=_form(12, 2, [_seg((0, 11), 33, 1, wv=1)], kinds=[1, 0, 0, 0, 0], gran=[16]),
                          b=_form(1, 1, kinds=[1, 0, 0, 0, 0])),
    # ragged plans, source phase != destination phase: every launch copy_kernel_s
    "shifted": dict(env=dict(XG_ENGINE_MAX_STEP=0), gen=dict(lens=[4097, 1000, 33], n=72, counts=[6] * 12, phase=(3, 8),
                                                            flags=RAGGED), kmax=19,
                    a=_form(12, 12, chains=[(0, 12)], kinds=[0, 0, 12, 0, 0]),
                    b=_form(1, 1, kinds=[0, 0, 1, 0, 0])),
    # placement plans of 240 slots of 64-300 B: every launch copy_kernel_x
    "extents": dict(env=dict(XG_ENGINE_MAX_STEP=0), gen=dict(lens=EXT_LENS, n=240, counts=[40] * 6, phase=(5, 12),
                                                            flags=RAGGED | EXTENTS), kmax=19,
                    a=_form(6, 6, chains=[(0, 6)], kinds=[0, 0, 0, 6, 0]),
                    b=_form(1, 1, kinds=[0, 0, 0, 1, 0])),
    # aligned uniform slots of 8208 B (8 KiB + 16 B: two pieces a copy, the second 16 B): every launch copy_kernel_q
    "small": dict(env=dict(XG_ENGINE_MAX_STEP=0, XG_SMALL_PIECE_MIN=0), gen=dict(lens=[8208], n=N, counts=EVEN), kmax=19,
                  a=_form(12, 12, chains=[(0, 12)], kinds=[0, 0, 0, 0, 12]),
                  b=_form(1, 1, kinds=[0, 0, 0, 0, 1])),
    # one solo segment each, which xg_plan_run arms (the doorbell) and xg_plan_enqueue launches plainly
    "armed": dict(env=dict(XG_ENGINE_ARM=1), gen=dict(lens=[1024], n=N, counts=EVEN), kmax=19,
                  a=_form(12, 1, [_seg((0, 12), 48, 1, wv=1)], armed=1, gran=[16]),
                  b=_form(1, 1, [_seg((0, 1), 48, 1, wv=1)], armed=1, gran=[16])),
    # launches cut into dispatches of ~64 KiB (XG_COPY_LAUNCH_MAX): a's first step (144 KiB) goes as
    # two dispatches, b (288 KiB) as four -- the per-launch session must give each dispatch its own bytes
    "cut": dict(env=dict(XG_ENGINE_MAX_STEP=0, XG_COPY_LAUNCH_MAX=65536, XG_GRAPH=0),
                gen=dict(lens=[4096, 8192], n=N, counts=[24, 8, 8, 8]), kmax=3,
                a=_form(4, 5, chains=[(0, 4)], kinds=[4, 0, 0, 0, 0]),
                b=_form(1, 4, kinds=[1, 0, 0, 0, 0])),
}
BACK_TO_BACK = [c for c in CASES if c != "cut"]         # the cases of every sequence; "cut": the per-launch session only


def form(records, kinds):
    """time_plan.form of a plan's tables (xg.parse_tables), with graph_auto, the launches per kernel
    kind (kinds: xg_plan_kind_launches of the loaded plan, PlanTables.kind_launches of a host build:
    the launch table also lists the steps an engine segment runs) and the segments' granules"""
    from time_plan import form as base
    f = base(records)
    f["graph_auto"] = records["plan"]["graph_auto"]
    f["kinds"] = list(kinds)
    if records.get("seg"):
        f["gran"] = [g["gran"] for g in records["seg"]]
    return f


def dispatch_bytes(records):
    """the bytes every kernel dispatch of one run moves, in the order a run posts them, from the
    plan's own tables: an engine segment is one dispatch of its bytes (at its first step), a copy
    launch its dispatches -- pieces [cut[k], cut[k + 1]) of the piece table, or a copy_kernel_q
    launch's qbytes"""
    plen = [p[2] for p in records.get("piece", [])]
    cuts, qbytes = records.get("cut", []), records.get("qbytes", [])
    launches, segs = records.get("launch", []), records.get("seg", [])
    out = []
    for s, st in enumerate(records["step"]):
        if st["seg"] >= 0:
            g = segs[st["seg"]]
            if g["steps"][0] == s:
                out.append(g["bytes"])
            continue
        b, _rccl, e = st["l"]
        for l in launches[b:e]:
            for k in range(l["ndisp"]):
                if l["kind"] == 4:          # XG_COPY_SMALL
                    out.append(qbytes[l["q"][3] + k])
                else:
                    out.append(sum(plen[cuts[l["cut"] + k]:cuts[l["cut"] + k + 1]]))
    return out


# ------------------------------------------------------------------ on the GPU
class FlagSynth(Synth):
    """Synth whose plan carries xg_devplan flags, and -- over() -- a further plan loaded over the
    regions of an existing one, which stay the first one's: close() of the further plan frees only
    its plan.  Synth itself is unchanged."""

    def __init__(self, xg, ctx, send_bytes, recv_bytes, steps, seed=0, flags=0):
        self.flags, self.owner = flags, True
        Synth.__init__(self, xg, ctx, send_bytes, recv_bytes, steps, seed=seed)

    @classmethod
    def over(cls, first, ctx, steps, flags=0):
        self = cls.__new__(cls)
        self.xg, self.d, self.r = first.xg, first.d, first.r
        self.send, self.recv = first.send, first.recv
        self.flags, self.owner = flags, False
        self._load(ctx, len(first.send), len(first.recv), steps)
        return self

    def _load(self, ctx, send_bytes, recv_bytes, steps):
        dp = devplan(self.xg, steps, send_bytes, recv_bytes)
        dp.flags = self.flags
        self.dp = dp
        self.p = C.c_void_p()
        assert self.d.xg_plan_load(ctx.handle, self.r, C.byref(dp), C.byref(self.p)) == 0
        self.steps = steps

    def read(self, buf):
        n = len(self.recv) if buf == 1 else len(self.send)
        out = C.create_string_buffer(n)
        assert self.d.xg_regions_read(self.r, buf, 0, out, n) == 0
        return np.frombuffer(out.raw, np.uint8)

    def close(self):
        self.d.xg_plan_free(self.p)
        if self.owner:
            self.d.xg_regions_free(self.r)
