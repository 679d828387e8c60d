"""Device plans WITH dependencies between their steps, their in-order numpy reference, and a
runner through the C-ABI (TEST HELPER, never part of the product).

What a valid xg_devplan means (include/xg_sched.h, DESIGN.md "what a device plan means"):

  * Steps run in order.
  * Inside a step four phases run in order: the stage copies; the pre copies (local copies, then
    packs); the p2p groups (group 0, then group 1); the post copies (unpacks).
  * The copies of one phase -- and the calls of one p2p group -- are simultaneous: none writes
    bytes another of the same phase reads or writes.
  * Phases and steps may depend on each other in any way: read after write, write after write with
    other bytes, write after read.
  * One limit: a step's LOCAL copies may run beside the step's own p2p groups and unpacks (side
    stream, RCCL group), so they touch no byte those write and write none those read.

Every schedule the product builds reads SEND and writes disjoint RECV slots, so there the order of
steps never shows in the bytes.  The jobs here are built so that it does: a Job is a list of steps,
each a Part per GPU; Job.execute runs exactly the semantics above on numpy regions (check_races per
phase, p2p matched per ordered GPU pair in issue order and per group, as plan_exec.simulate does);
run_job loads the same plans on the device (xg_plan_load), preloads SEND, RECV and SCRATCH with a
seeded random image (a read of not-yet-written bytes then differs from every valid outcome; a
constant poison would equal itself), runs them (xg_plan_run, or xg_vplans_run for a virtual job) and
compares SEND, RECV and SCRATCH whole on every GPU.
"""
import ctypes as C

import numpy as np
import pytest

from plan_exec import check_races
from synth_plan import Synth, _up16
from test_pieces import _plan

S, R, SS, SR, SC = 0, 1, 2, 3, 4            # XG_BUF_SEND, RECV, STAGE_SEND, STAGE_RECV, SCRATCH
BUF_NAME = {S: "SEND", R: "RECV", SS: "STAGE_SEND", SR: "STAGE_RECV", SC: "SCRATCH"}
USER_BUFS = (S, R, SC)


class Part:
    """One GPU's share of one step.  stage / local: copies (src_buf, src_off, dst_buf, dst_off, len).
    packs: (peer, src_buf, src_off, len), grouped by ascending peer; unpacks: (peer, dst_buf,
    dst_off, len), likewise -- the builder lays the staging out.  p2p: direct calls (peer, is_send,
    buf, off, len) out of / into the regions.  sync: an in-loop barrier ends the step."""

    def __init__(self, stage=(), local=(), packs=(), p2p=(), unpacks=(), sync=0):
        self.stage, self.local, self.packs = list(stage), list(local), list(packs)
        self.p2p, self.unpacks, self.sync = list(p2p), list(unpacks), sync


def _lay(part):
    """the staging layout of xg_devplan_build: a step's packs tile STAGE_SEND from 0 in list order,
    its unpacks STAGE_RECV from 0, one send / receive per peer over the peer's packed range (ahead
    of the direct calls) -> (stage, local, pack copies, ops (peer, is_send, buf, off, len, group),
    unpack copies, STAGE_SEND bytes, STAGE_RECV bytes)"""
    packs, unp, sends, recvs = [], [], [], []
    for lst, out, ops, is_send in ((part.packs, packs, sends, 1), (part.unpacks, unp, recvs, 0)):
        assert [x[0] for x in lst] == sorted(x[0] for x in lst), "packs / unpacks are grouped by peer"
        at = 0
        for peer in sorted({x[0] for x in lst}):
            begin = at
            for (_p, buf, off, n) in (x for x in lst if x[0] == peer):
                out.append((buf, off, SS, at, n) if is_send else (SR, at, buf, off, n))
                at += n
            ops.append((peer, is_send, SS if is_send else SR, begin, at - begin, 0))
        if is_send:
            sbytes = at
        else:
            rbytes = at
    sends += [(p, 1, b, o, n, 0) for (p, snd, b, o, n) in part.p2p if snd]
    recvs += [(p, 0, b, o, n, 0) for (p, snd, b, o, n) in part.p2p if not snd]
    return list(part.stage), list(part.local), packs, sends + recvs, unp, sbytes, rbytes


def _op_copies(ops, k0=0):
    """p2p calls as pseudo copies for check_races: a send reads its bytes, a receive writes its
    bytes; the other side is a buffer of the call's own"""
    return [(b, o, -1 - k0 - k, 0, n) if snd else (-1 - k0 - k, 0, b, o, n)
            for k, (_p, snd, b, o, n, _g) in enumerate(ops)]


def _meet(b1, o1, n1, b2, o2, n2):
    return n1 > 0 and n2 > 0 and b1 == b2 and o1 < o2 + n2 and o2 < o1 + n1


class Job:
    """G GPUs, region sizes bytes[g] = (SEND, RECV, SCRATCH), steps[s][g] = Part"""

    def __init__(self, G, nbytes, steps, name=""):
        self.G, self.name, self.parts = G, name, steps
        self.nsteps = len(steps)
        assert all(len(st) == G for st in steps)
        self.laid = [[_lay(p) for p in st] for st in steps]
        self.bytes = []
        for g in range(G):
            rb = [0] * 5
            rb[S], rb[R], rb[SC] = nbytes[g]
            rb[SS] = max([0] + [self.laid[s][g][5] for s in range(self.nsteps)])
            rb[SR] = max([0] + [self.laid[s][g][6] for s in range(self.nsteps)])
            self.bytes.append(rb)

    # ------------------------------------------------------------------ the xg_devplan of GPU g
    def devplan(self, xg, g):
        """test_pieces._plan over the laid-out copies, with the p2p calls, the barriers and the
        region sizes filled in"""
        dp = _plan(xg, [(self.laid[s][g][0], self.laid[s][g][1], self.laid[s][g][2], self.laid[s][g][4])
                        for s in range(self.nsteps)])
        ops = [o for s in range(self.nsteps) for o in self.laid[s][g][3]]
        arr = (xg.P2P * max(1, len(ops)))(*[xg.P2P(o, n, p, b, snd, grp) for (p, snd, b, o, n, grp) in ops])
        at = 0
        for s in range(self.nsteps):
            dp.steps[s].p2p_begin, dp.steps[s].p2p_count = at, len(self.laid[s][g][3])
            dp.steps[s].sync_after = 1 if self.parts[s][g].sync else 0
            at += len(self.laid[s][g][3])
        dp.gpu, dp.ngpus, dp.np2p = g, self.G, len(ops)
        dp.p2p = C.cast(arr, C.POINTER(xg.P2P))
        for i, v in enumerate(self.bytes[g]):
            dp.region_bytes[i] = v
        dp._keep = dp._keep + (arr,)
        return dp

    def calls(self, xg, self_max=0):
        """every GPU's calls per step as xg_devplan_step_calls lists them: [g][s] = [(kind, peer, buf, off, len)]"""
        out = []
        for g in range(self.G):
            dp = self.devplan(xg, g)
            per = []
            for s in range(self.nsteps):
                n = xg.host().xg_devplan_step_calls(C.byref(dp), s, self_max, None)
                arr = (xg.Call * max(1, n))()
                xg.host().xg_devplan_step_calls(C.byref(dp), s, self_max, arr)
                per.append([(c.kind, c.peer, c.buf, c.off, c.len) for c in arr[:n]])
            out.append(per)
        return out

    # ------------------------------------------------------------------ validity
    def check(self):
        """every phase race-free and inside its regions, every send paired with a receive of its
        length, the local copies clear of their own step's exchange (the limit above)"""
        for s in range(self.nsteps):
            for g in range(self.G):
                stage, local, packs, ops, unp, _sb, _rb = self.laid[s][g]
                what = "%s step %d gpu %d" % (self.name, s, g)
                for (sb, so, db, do, n) in stage + local + packs + unp:
                    assert n >= 0 and 0 <= so and so + n <= self.bytes[g][sb], (what, sb, so, n)
                    assert 0 <= do and do + n <= self.bytes[g][db], (what, db, do, n)
                for (_p, _snd, b, o, n, _grp) in ops:
                    assert 0 <= o and o + n <= self.bytes[g][b], (what, b, o, n)
                check_races(stage, what + " stage")
                check_races(local + packs, what + " pre")
                check_races(_op_copies(ops), what + " p2p")
                check_races(unp, what + " post")
                assert all(c[2] == SS for c in packs) and all(c[0] == SR for c in unp)
                assert not any(c[2] == SS for c in local), "a local copy into STAGE_SEND would read as a pack"
                for (lsb, lso, ldb, ldo, ln) in local:
                    for (xsb, xso, xdb, xdo, xn) in _op_copies(ops) + unp:
                        assert not (_meet(ldb, ldo, ln, xdb, xdo, xn) or _meet(ldb, ldo, ln, xsb, xso, xn) or
                                    _meet(lsb, lso, ln, xdb, xdo, xn)), (what, "a local copy meets the step's exchange")
            self._moves(s)

    def _moves(self, s):
        """the p2p transfers of step s: (src gpu, buf, off, dst gpu, buf, off, len), matched per
        ordered GPU pair in issue order"""
        out = []
        for g in range(self.G):
            for p in range(self.G):
                sends = [o for o in self.laid[s][g][3] if o[0] == p and o[1]]
                recvs = [o for o in self.laid[s][p][3] if o[0] == g and not o[1]]
                assert len(sends) == len(recvs), (self.name, s, g, p, len(sends), len(recvs))
                for (_p, _s, sb, so, sn, _g), (_q, _r, rb, ro, rn, _h) in zip(sends, recvs):
                    assert sn == rn, (self.name, s, g, p, sn, rn)
                    out.append((g, sb, so, p, rb, ro, sn))
        return out

    # ------------------------------------------------------------------ the reference
    def initial(self, seed):
        """SEND, RECV and SCRATCH of every GPU as seeded random bytes (staging: zeros, never compared)"""
        rng = np.random.default_rng(seed)
        return [[rng.integers(0, 256, n, dtype=np.uint8) if b in USER_BUFS else np.zeros(n, np.uint8)
                 for b, n in enumerate(self.bytes[g])] for g in range(self.G)]

    @staticmethod
    def _phase(reg, lst):
        """simultaneous copies: every source is read before any destination is written"""
        vals = [reg[sb][so:so + n].copy() for (sb, so, _db, _do, n) in lst]
        for (_sb, _so, db, do, n), v in zip(lst, vals):
            reg[db][do:do + n] = v

    def execute(self, regs):
        """the plan's semantics, in order, on regs[g][buf] (changed in place and returned)"""
        for s in range(self.nsteps):
            for g in range(self.G):
                self._phase(regs[g], self.laid[s][g][0])
                self._phase(regs[g], self.laid[s][g][1] + self.laid[s][g][2])
            moves = self._moves(s)
            vals = [regs[g][sb][so:so + n].copy() for (g, sb, so, _p, _rb, _ro, n) in moves]
            for (_g, _sb, _so, p, rb, ro, n), v in zip(moves, vals):
                regs[p][rb][ro:ro + n] = v
            for g in range(self.G):
                self._phase(regs[g], self.laid[s][g][4])
        return regs

    def owner(self, g, buf, at):
        """the last write of the plan that covers byte `at` of GPU g's region buf, as text"""
        last = None
        for s in range(self.nsteps):
            stage, local, packs, _ops, unp, _sb, _rb = self.laid[s][g]
            for what, lst in (("stage copy", stage), ("local copy", local), ("pack", packs)):
                for (sb, so, db, do, n) in lst:
                    if db == buf and do <= at < do + n:
                        last = "byte %d of the %s %s[%d..%d) -> %s[%d..%d) of step %d" % (
                            at - do, what, BUF_NAME[sb], so, so + n, BUF_NAME[db], do, do + n, s)
            for (src, sb, so, p, rb, ro, n) in self._moves(s):
                if p == g and rb == buf and ro <= at < ro + n:
                    last = "byte %d of the receive from GPU %d's %s[%d..%d) into %s[%d..%d) of step %d" % (
                        at - ro, src, BUF_NAME[sb], so, so + n, BUF_NAME[rb], ro, ro + n, s)
            for (sb, so, db, do, n) in unp:
                if db == buf and do <= at < do + n:
                    last = "byte %d of the unpack STAGE_RECV[%d..%d) -> %s[%d..%d) of step %d" % (
                        at - do, so, so + n, BUF_NAME[db], do, do + n, s)
        return last or "written by no copy of the plan"

    def compare(self, got, want, what=""):
        """got / want: [g][buf] -> fails naming the first differing byte and the copy that owns it"""
        for g in range(self.G):
            for b in USER_BUFS:
                if (got[g][b] == want[g][b]).all():
                    continue
                at = int(np.flatnonzero(got[g][b] != want[g][b])[0])
                pytest.fail("%s %s: GPU %d %s: %d bytes differ; the first, %s[%d] = 0x%02x (expected 0x%02x), is %s"
                            % (self.name, what, g, BUF_NAME[b], int((got[g][b] != want[g][b]).sum()), BUF_NAME[b], at,
                               got[g][b][at], want[g][b][at], self.owner(g, b, at)))

    # ------------------------------------------------------------------ what the plan depends on
    def spans(self, g=0):
        """GPU g's pre copies per step as (src, dst, len) in one address space (the regions back to
        back), for xg_engine_hazards and the walks below"""
        base, at = {}, 0
        for b in range(5):
            base[b] = at
            at += _up16(self.bytes[g][b]) + 64
        return [[(base[sb] + so, base[db] + do, n) for (sb, so, db, do, n) in self.laid[s][g][1]]
                for s in range(self.nsteps)], at


    def phases(self, g):
        """everything that touches GPU g's regions, one list per phase (4 per step: phase 4 s + 0
        stage, + 1 pre, + 2 p2p, + 3 post) as (src, dst, len) in spans()' address space; a send has
        no dst, a receive no src -> (phases, size)"""
        base, at = {}, 0
        for b in range(5):
            base[b] = at
            at += _up16(self.bytes[g][b]) + 64
        def cp(lst):
            return [(base[sb] + so, base[db] + do, n) for (sb, so, db, do, n) in lst]
        out = []
        for s in range(self.nsteps):
            stage, local, packs, ops, unp, _sb, _rb = self.laid[s][g]
            out += [cp(stage), cp(local + packs),
                    [(base[b] + o, None, n) if snd else (None, base[b] + o, n) for (_p, snd, b, o, n, _g) in ops], cp(unp)]
        return out, at


STAGE, PRE, P2P, POST = 0, 1, 2, 3


def hazard_walk(steps, size):
    """xg_engine_hazards' definition, byte by byte: flags[s] = 2 where step s + 1 reads, or rewrites
    with other bytes (another dst - src), a byte written since the last flag 2; else 0 (1 for the
    last step).  steps: [[(src, dst, len)]] inside [0, size)."""
    pend = np.zeros(size, bool)
    delta = np.zeros(size, np.int64)
    flags = [0] * len(steps)
    for s, st in enumerate(steps):
        hit = False
        for (src, dst, n) in st:
            if n and (pend[src:src + n].any() or (pend[dst:dst + n] & (delta[dst:dst + n] != dst - src)).any()):
                hit = True
                break
        if hit:
            flags[s - 1] = 2
            pend[:] = False
        for (src, dst, n) in st:
            pend[dst:dst + n] = True
            delta[dst:dst + n] = dst - src
    if flags:
        flags[-1] = max(flags[-1], 1)
    return flags


def dependencies(steps, size):
    """a direct walk, with no hazard points in it: every (writer step i, reader step j > i, kind) such
    that step j reads ("raw"), rewrites with another dst - src ("waw"), rewrites identically ("same") or
    overwrites after step i read ("war") a byte whose LAST write (for war: last read) before j was step i's"""
    wstep = np.full(size, -1, np.int64)
    rstep = np.full(size, -1, np.int64)
    delta = np.zeros(size, np.int64)
    out = set()
    for j, st in enumerate(steps):
        for k, (src, dst, n) in enumerate(st):
            if not n:
                continue
            if src is not None:                 # (a receive has no source here, a send no destination)
                for i in np.unique(wstep[src:src + n]):
                    if 0 <= i < j:
                        out.add((int(i), j, "raw"))
            if dst is None:
                continue
            dl = dst - src if src is not None else -(1 + j * 1000003 + k)
            w, d = wstep[dst:dst + n], delta[dst:dst + n]
            for i in np.unique(w[(w >= 0) & (w < j) & (d != dl)]):
                out.add((int(i), j, "waw"))
            for i in np.unique(w[(w >= 0) & (w < j) & (d == dl)]):
                out.add((int(i), j, "same"))
            for i in np.unique(rstep[dst:dst + n]):
                if 0 <= i < j:
                    out.add((int(i), j, "war"))
        for (src, dst, n) in st:
            if src is not None:
                rstep[src:src + n] = j
        for k, (src, dst, n) in enumerate(st):
            if dst is not None:
                wstep[dst:dst + n] = j
                delta[dst:dst + n] = dst - src if src is not None else -(1 + j * 1000003 + k)
    return out


# ---------------------------------------------------------------------- one-GPU plans (local copies only)
DEP_LENS = [16, 4096, 256, 1000, 33, 2048, 4097, 512, 48, 17]      # 1000 / 33 / 4097 / 17: off the 16-B grid
KINDS = ("raw_chain", "raw_delayed", "partial", "waw_other", "waw_same", "war")
NDEP = 60               # dependent copies per dependent step
SHIFT = 10              # reader j reads what writer j + SHIFT (mod NDEP) wrote: same length, another workgroup


class _Bump:
    """bump allocators over SEND and RECV: sources back to back, destinations behind gaps of 16-48 B
    that nothing writes, every 7th transfer at odd phases"""

    def __init__(self):
        self.s = self.r = self.k = 0

    def src(self, n, phase=0):
        off = _up16(self.s) + phase
        self.s = off + n
        return off

    def dst(self, n, phase=0):
        off = _up16(self.r) + 16 * (1 + self.k % 3) + phase
        self.r = off + n
        return off

    def fresh(self, n=None):
        """a SEND -> RECV copy of the k-th length"""
        k = self.k
        n = DEP_LENS[k % len(DEP_LENS)] if n is None else n
        odd = k % 7 == 3
        c = (S, self.src(n, k % 16 if odd else 0), R, self.dst(n, (5 * k) % 16 if odd else 0), n)
        self.k += 1
        return c

    def read(self, off, n):
        """a RECV -> RECV copy of RECV[off .. off + n) into a destination of its own"""
        k = self.k
        c = (R, off, R, self.dst(n, (5 * k) % 16 if k % 7 == 3 else 0), n)
        self.k += 1
        return c


def solo_kind(kind, per, unit=1, lead=0):
    """One-GPU plan of `per` copies per step carrying dependency `kind`; the dependent copies are the
    FIRST NDEP of their step (each a workgroup's first unit there, the one the grid engine loads
    early) and meet what the LAST NDEP copies of the writing step moved (the chain's second and third
    hop: what the first NDEP of the step before moved).  unit: every length x unit (unit = 16 with
    16 x DEP_LENS: 64 KiB engine units); lead: that many hazard-free steps in front.
    -> (steps, send_bytes, recv_bytes)"""
    assert per >= 2 * NDEP and (per - NDEP) % len(DEP_LENS) == 0 and NDEP % len(DEP_LENS) == 0
    b = _Bump()

    def fill(count):
        return [b.fresh(unit * DEP_LENS[b.k % len(DEP_LENS)]) for _ in range(count)]

    def readers(writers):
        return [b.read(writers[(j + SHIFT) % NDEP][3], writers[(j + SHIFT) % NDEP][4]) for j in range(NDEP)]

    steps = [fill(per) for _ in range(lead + 1)]
    tail = steps[-1][-NDEP:]
    if kind == "raw_chain":                         # A -> B in step 0, B -> C in 1, C -> D in 2, D -> E in 3
        for _hop in range(3):
            dep = readers(tail)
            steps.append(dep + fill(per - NDEP))
            tail = dep
    elif kind == "raw_delayed":                     # written in step 0, read in step 3
        steps += [fill(per), fill(per)]
        steps.append(readers(tail) + fill(per - NDEP))
        steps.append(fill(per))
    elif kind == "partial":                         # the last byte of one destination, the gap, the first of the next
        tail = steps[-1][-NDEP - 1:]
        dep = [b.read(a[3] + a[4] - 1, c[3] + 1 - (a[3] + a[4] - 1)) for a, c in zip(tail, tail[1:])]
        dep = dep[SHIFT:] + dep[:SHIFT]
        steps.append(dep + fill(per - NDEP))
        steps.append(fill(per))
    elif kind in ("waw_other", "waw_same"):         # half of a destination again, from another source / all of it, identically
        w = [tail[(j + SHIFT) % NDEP] for j in range(NDEP)]
        if kind == "waw_same":
            dep = list(w)
        else:
            dep = [(S, b.src(n // 2, 0), R, do + n - n // 2, n // 2) for (_sb, _so, _db, do, n) in w]
        steps.append(dep + fill(per - NDEP))
        steps.append(fill(per))
    elif kind == "war":                             # step 0 reads RECV[x], step 1 overwrites it
        xs = [(b.dst(n, 3 if j % 7 == 3 else 0), n) for j, (_sb, _so, _db, _do, n) in enumerate(tail)]   # unwritten so far
        steps[-1] = steps[-1][:-NDEP] + [b.read(x, n) for (x, n) in xs]
        dep = [(S, b.src(n, 0), R, x, n) for (x, n) in (xs[(j + SHIFT) % NDEP] for j in range(NDEP))]
        steps.append(dep + fill(per - NDEP))
        steps.append(fill(per))
    else:
        raise AssertionError(kind)
    return steps, _up16(b.s) + 16, _up16(b.r) + 32


def unit64_chain():
    """the RAW chain at the grid engine's 64 KiB units: step 0 moves 11 groups of synth_plan's
    _unit64_steps transfers (above 4 MiB: 16 loads per lane in flight) and two short ones at odd
    phases; step 1 copies on what the last 12 of them wrote, step 2 what step 1 wrote, step 3 the
    first four of step 2 -- each reader first in its step, its writer four transfers further on"""
    u = 64 << 10
    group = [u - 16, u, u + 16, 3 * u + 4080]
    b = _Bump()
    steps = [[b.fresh(n) for n in 11 * group] + [b.fresh(5 * 1024 + 1), b.fresh(2 * 1024 + 7)]]
    tail = steps[0][-14:-2]
    for count in (12, 12, 4):
        tail = [b.read(tail[(j + 4) % len(tail)][3], tail[(j + 4) % len(tail)][4]) for j in range(count)]
        steps.append(tail)
    return steps, _up16(b.s) + 16, _up16(b.r) + 32


def twin(steps, send_bytes, recv_bytes):
    """the hazard-free twin: the same copies with every RECV source moved to fresh SEND bytes, and a
    rewrite of RECV bytes made the identical rewrite (from the SEND bytes their first write took)
    -> (steps, send_bytes)"""
    first = np.full(recv_bytes, -1, np.int64)       # the SEND byte each RECV byte was first written from
    out, at = [], _up16(send_bytes)
    for st in steps:
        new = []
        for (sb, so, db, do, n) in st:
            assert db == R
            if n and first[do] >= 0:
                sb, so = S, int(first[do])
                assert (first[do:do + n] == so + np.arange(n)).all()
            elif sb == R:
                sb, so = S, at
                at = _up16(at + n)
            first[do:do + n] = so + np.arange(n)
            new.append((sb, so, db, do, n))
        out.append(new)
    return out, at + 16


def solo_job(steps, send_bytes, recv_bytes, name=""):
    """a one-GPU Job of local copies only"""
    return Job(1, [(send_bytes, recv_bytes, 0)], [[Part(local=st)] for st in steps], name)


# ---------------------------------------------------------------------- multi-GPU jobs
# Every GPU packs and unpacks in every cross-GPU step (so the loader may fuse each step's packs with
# the unpacks of the step before), and GPU g's share is the same for every g.  Each builder returns
# (job, [(kind, (step, phase) of the writer or first reader, (step, phase) of the dependent access)]).
ODD_LENS = [131072, 4097, 1000, 65536, 16]          # consecutive windows: the later ones at odd offsets


def _cut(off, total, piece):
    return [(off + o, min(piece, total - o)) for o in range(0, total, piece)]


def _windows(off, lens):
    """consecutive windows of these lengths from off"""
    out = []
    for n in lens:
        out.append((off, n))
        off += n
    return out


def _tail_windows(end, lens=ODD_LENS):
    """consecutive windows of these lengths that END at `end`"""
    return _windows(end - sum(lens), lens)


def job_pack_reads_unpacks(sync=0):
    """(a) step 0 delivers SEND -> the peer's RECV[64 .. 64 + 3 MiB); step 1 packs the LAST bytes
    those unpacks wrote and sends them back; no local copies.  sync: (h) a barrier between them."""
    M = 3 << 20
    wins = _tail_windows(64 + M)
    back = _windows(64 + M + 64, [n for (_o, n) in wins])
    steps = []
    for s in range(2):
        parts = []
        for g in range(2):
            p = 1 - g
            if s == 0:
                parts.append(Part(packs=[(p, S, o, n) for (o, n) in _cut(0, M, 128 << 10)],
                                  unpacks=[(p, R, 64 + o, n) for (o, n) in _cut(0, M, 128 << 10)], sync=sync))
            else:
                parts.append(Part(packs=[(p, R, o, n) for (o, n) in wins], unpacks=[(p, R, o, n) for (o, n) in back]))
        steps.append(parts)
    nb = (M, back[-1][0] + back[-1][1] + 64, 0)
    return Job(2, [nb, nb], steps, "pack_reads_unpacks" + ("_sync" if sync else "")), [("raw", (0, POST), (1, PRE))]


def job_local_after_unpacks(kind):
    """(b) (c) (g) kind "reads": step 1's local copies read the last bytes step 0's unpacks wrote (into
    SCRATCH); "control": they read SEND instead; (d) "overwrites": they write over those bytes."""
    N = 1 << 20
    lens = ODD_LENS[1:4]
    wins = _tail_windows(64 + N, lens)
    src = _windows(N + (256 << 10), lens)
    scr = _windows(16, lens)
    steps = []
    for s in range(2):
        parts = []
        for g in range(2):
            p = 1 - g
            if s == 0:
                parts.append(Part(packs=[(p, S, o, n) for (o, n) in _cut(0, N, 128 << 10)],
                                  unpacks=[(p, R, 64 + o, n) for (o, n) in _cut(0, N, 128 << 10)]))
                continue
            if kind == "reads":
                local = [(R, o, SC, d, n) for (o, n), (d, _n) in zip(wins, scr)]
            elif kind == "control":
                local = [(S, o, SC, d, n) for (o, n), (d, _n) in zip(src, scr)]
            else:
                local = [(S, o, R, d, n) for (o, n), (d, _n) in zip(src, wins)]
            parts.append(Part(local=local, packs=[(p, S, o, n) for (o, n) in _cut(N, 256 << 10, 128 << 10)],
                              unpacks=[(p, R, 64 + N + 64 + o - N, n) for (o, n) in _cut(N, 256 << 10, 128 << 10)]))
        steps.append(parts)
    nb = (N + (256 << 10) + sum(lens) + 16, 64 + N + 64 + (256 << 10) + 64, 16 + sum(lens) + 16)
    want = {"reads": [("raw", (0, POST), (1, PRE))], "control": [], "overwrites": [("waw", (0, POST), (1, PRE))]}[kind]
    return Job(2, [nb, nb], steps, "local_%s_unpacks" % kind), want


def job_war_exchange():
    """(e) step 0's packs read RECV[x] and its unpacks overwrite RECV[x]; step 1's packs then read
    the new bytes of RECV[x]"""
    wins = _windows(64, ODD_LENS)
    L = sum(ODD_LENS)
    ys = _windows(64 + L + 64, ODD_LENS)
    steps = []
    for s in range(2):
        parts = []
        for g in range(2):
            p = 1 - g
            parts.append(Part(packs=[(p, R, o, n) for (o, n) in wins],
                              unpacks=[(p, R, o, n) for (o, n) in (wins if s == 0 else ys)]))
        steps.append(parts)
    nb = (64, 64 + 2 * L + 128, 0)
    return Job(2, [nb, nb], steps, "war_exchange"), [("war", (0, PRE), (0, POST)), ("raw", (0, POST), (1, PRE))]


def job_stage(kind):
    """(f) a stage copy SEND -> SCRATCH; "dep": the step's local copy SCRATCH -> RECV reads it;
    "control": the local copy reads SEND.  Both GPUs also exchange 128 KiB in this and the next step."""
    lens = ODD_LENS[3:0:-1]                    # 65536, 1000, 4097
    L = sum(lens)
    st = _windows(0, lens)
    sc = _windows(16, lens)
    rc = _windows(64, lens)
    E = 128 << 10
    steps = []
    for s in range(2):
        parts = []
        for g in range(2):
            p = 1 - g
            ex = dict(packs=[(p, S, 2 * L + s * E, E)], unpacks=[(p, R, 64 + L + 64 + s * (E + 64), E)])
            if s == 0:
                stage = [(S, o, SC, d, n) for (o, n), (d, _n) in zip(st, sc)]
                if kind == "dep":
                    local = [(SC, o, R, d, n) for (o, n), (d, _n) in zip(sc, rc)]
                else:
                    local = [(S, L + o, R, d, n) for (o, n), (d, _n) in zip(st, rc)]
                parts.append(Part(stage=stage, local=local, **ex))
            else:
                parts.append(Part(**ex))
        steps.append(parts)
    nb = (2 * L + 2 * E, 64 + L + 64 + 2 * (E + 64), 16 + L + 16)
    return Job(2, [nb, nb], steps, "stage_" + kind), ([("raw", (0, STAGE), (0, PRE))] if kind == "dep" else [])


def job_ring(hops=3):
    """(i) three GPUs: in step t + 1 each forwards to its right neighbour what it received from its
    left one in step t (step 0: from SEND), for `hops` forwarding steps"""
    lens = ODD_LENS[:4]
    L = sum(lens)
    slot = [_windows(64 + t * (L + 64), lens) for t in range(hops + 1)]
    steps = []
    for t in range(hops + 1):
        parts = []
        for g in range(3):
            srcs = _windows(0, lens) if t == 0 else slot[t - 1]
            parts.append(Part(packs=[((g + 1) % 3, S if t == 0 else R, o, n) for (o, n) in srcs],
                              unpacks=[((g + 2) % 3, R, o, n) for (o, n) in slot[t]]))
        steps.append(parts)
    nb = (L, 64 + (hops + 1) * (L + 64), 0)
    return Job(3, [nb] * 3, steps, "ring"), [("raw", (t, POST), (t + 1, PRE)) for t in range(hops)]


def job_engine_inside():
    """(k) a cross-GPU step, then three GPU-local steps -- an engine segment -- that read what it
    unpacked: step 1 copies out of the unpacked bytes, step 2 out of step 1's, step 3 out of step 2's"""
    E = 512 << 10
    b = _Bump()
    b.r = 64 + E
    srcs, at = [], 64
    for k in range(40):
        n = DEP_LENS[k % len(DEP_LENS)]
        srcs.append((at, n))
        at += n + 16 * (k % 3)
    chain = [[b.read(o, n) for (o, n) in srcs]]
    for _hop in range(2):
        prev = chain[-1]
        chain.append([b.read(prev[(j + SHIFT) % 40][3], prev[(j + SHIFT) % 40][4]) for j in range(40)])
    steps = [[Part(packs=[(1 - g, S, o, n) for (o, n) in _cut(0, E, 128 << 10)],
                   unpacks=[(1 - g, R, 64 + o, n) for (o, n) in _cut(0, E, 128 << 10)]) for g in range(2)]]
    steps += [[Part(local=st) for _g in range(2)] for st in chain]
    nb = (E, _up16(b.r) + 32, 0)
    return (Job(2, [nb, nb], steps, "engine_inside"),
            [("raw", (0, POST), (1, PRE)), ("raw", (1, PRE), (2, PRE)), ("raw", (2, PRE), (3, PRE))])


PAIR_JOBS = {
    "a_pack_reads_unpacks": lambda: job_pack_reads_unpacks(),
    "b_local_reads_unpacks": lambda: job_local_after_unpacks("reads"),
    "b_control": lambda: job_local_after_unpacks("control"),
    "d_local_overwrites_unpacks": lambda: job_local_after_unpacks("overwrites"),
    "e_war_exchange": job_war_exchange,
    "f_stage_dep": lambda: job_stage("dep"),
    "f_stage_control": lambda: job_stage("control"),
    "h_barrier": lambda: job_pack_reads_unpacks(sync=1),
    "i_ring": job_ring,
    "k_engine_inside": job_engine_inside,
}


# ---------------------------------------------------------------------- the runner
class Loaded(Synth):
    """GPU g's regions and loaded plan of a Job (Synth's handles: run_timed and close are its)"""

    def __init__(self, xg, ctx, job, g):
        d = xg.device()
        self.xg, self.d, self.job, self.g = xg, d, job, g
        rb = (C.c_int64 * xg.NBUF)(*job.bytes[g])
        self.r = C.c_void_p()
        assert d.xg_regions_alloc(ctx.handle, rb, C.byref(self.r)) == 0
        self.dp = job.devplan(xg, g)
        self.p = C.c_void_p()
        assert d.xg_plan_load(ctx.handle, self.r, C.byref(self.dp), C.byref(self.p)) == 0, job.name
        self.steps = [None] * job.nsteps
        self.recv = np.zeros(job.bytes[g][R], np.uint8)

    def write(self, buf, image):
        data = np.ascontiguousarray(image, np.uint8).tobytes()
        assert len(data) == self.job.bytes[self.g][buf]
        if data:
            assert self.d.xg_regions_write(self.r, buf, 0, data, len(data)) == 0

    def read(self, buf):
        n = self.job.bytes[self.g][buf]
        out = C.create_string_buffer(max(1, n))
        if n:
            assert self.d.xg_regions_read(self.r, buf, 0, out, n) == 0
        return np.frombuffer(out.raw, np.uint8)[:n]

    def form(self, s):
        return self.xg.plan_step_form(self.p, s)

    def engine_steps(self):
        ns, nh = C.c_int(), C.c_int()
        n = self.d.xg_plan_engine_steps(self.p, C.byref(ns), C.byref(nh))
        return n, ns.value, nh.value


def run_job(xg, ctxs, job, seed=0, runs=3, rccl=False, routing=None):
    """Load job on ctxs (one context per GPU), assert routing(loaded plans), then `runs` runs, each
    from a freshly written random image of SEND, RECV and SCRATCH: every region of every GPU against
    Job.execute, xg_plan_check clean."""
    job.check()
    loaded = []
    try:
        for g, cx in enumerate(ctxs):
            loaded.append(Loaded(xg, cx, job, g))
        if routing:
            routing(loaded)
        virtual = getattr(ctxs[0], "is_virtual", False)
        for rep in range(runs):
            init = job.initial(1000 * seed + rep)
            want = job.execute([[a.copy() for a in regs] for regs in init])
            for g, ld in enumerate(loaded):
                for b in USER_BUFS:
                    ld.write(b, init[g][b])
            if virtual:
                arr = (C.c_void_p * job.G)(*[ld.p for ld in loaded])
                done = (C.c_double * max(1, job.nsteps))()
                fn = xg.device().xg_vplans_run_rccl if rccl else xg.device().xg_vplans_run
                assert fn(arr, job.G, done) == 0, (job.name, rep)
            else:
                assert job.G == 1
                loaded[0].run_timed()
            got = [[ld.read(b) if b in USER_BUFS else None for b in range(5)] for ld in loaded]
            job.compare(got, want, "run %d" % rep)
            for ld in loaded:
                assert xg.device().xg_plan_check(ld.p) == 0, (job.name, rep)
    finally:
        for ld in loaded:
            ld.close()
