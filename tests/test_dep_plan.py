"""CPU: the dependent-plan generator (dep_plan.py) builds what it says, and the host predicates that
let the runtime reorder steps -- xg_engine_hazards, xg_step_packs_meet_unpacks -- agree with direct
walks over random plans.  The GPU half is test_gpu_dep_plans.py."""
import ctypes as C

import numpy as np
import pytest

import dep_plan as D
from dep_plan import PRE, R, S, SC, SR, SS
from test_pieces import _plan

PER = 2 * D.NDEP


def _solo_jobs():
    for kind in D.KINDS:
        steps, sb, rb = D.solo_kind(kind, PER)
        yield kind, D.solo_job(steps, sb, rb, kind)


# what each one-GPU kind must contain (kind of dependency, writer step, dependent step), and what not
SOLO_WANT = {
    "raw_chain": ([("raw", 0, 1), ("raw", 1, 2), ("raw", 2, 3)], ["waw", "war"]),
    "raw_delayed": ([("raw", 0, 3)], ["waw", "war"]),
    "partial": ([("raw", 0, 1)], ["waw", "war"]),
    "waw_other": ([("waw", 0, 1)], ["raw", "war", "same"]),
    "waw_same": ([("same", 0, 1)], ["raw", "war", "waw"]),
    "war": ([("war", 0, 1)], ["raw", "waw", "same"]),
}


def test_one_gpu_jobs_are_valid_and_hold_their_dependency(xg):
    """every phase race-free; the named dependency is there by a direct interval walk, between the
    named steps and on every one of the NDEP dependent copies, and no other kind is; lengths off the
    16-B grid and odd phases are among the dependent copies; the hazard flags are the byte walk's"""
    for kind, job in _solo_jobs():
        job.check()
        spans, size = job.spans()
        deps = D.dependencies(spans, size)
        want, never = SOLO_WANT[kind]
        assert {(i, j, k) for (k, i, j) in want} <= deps, (kind, sorted(deps))
        assert not [d for d in deps if d[2] in never], (kind, sorted(deps))
        assert deps == {(i, j, k) for (k, i, j) in want}, (kind, sorted(deps))
        for (k, i, j) in want:                     # each dependent copy on its own carries it
            for c in spans[j][:D.NDEP]:
                assert (0, 1, k) in D.dependencies([spans[i], [c]], size), (kind, c)
        dep = [c for (_k, _i, j) in want for c in job.laid[j][0][1][:D.NDEP]]
        if kind != "partial":                      # (its windows are the gaps: 18 - 66 B at any phase)
            assert any(n % 16 and (so % 16 or do % 16) for (_sb, so, _db, do, n) in dep), kind
            assert any((so | do | n) % 16 == 0 for (_sb, so, _db, do, n) in dep), kind
        flags, nhaz = xg.engine_hazards(spans)
        walk = D.hazard_walk(spans, size)
        assert flags == walk and nhaz == walk.count(2), (kind, flags, walk)
        assert nhaz == {"raw_chain": 3, "raw_delayed": 1, "partial": 1, "waw_other": 1, "waw_same": 0, "war": 0}[kind]
        safe = xg.rail_safe(spans)
        assert safe == (kind in ("waw_other", "waw_same")), (kind, safe)      # rails: no read of another step's write


def test_partial_overlap_reads_one_byte_of_each_writer():
    steps, _sb, _rb = D.solo_kind("partial", PER)
    wr = sorted((do, do + n) for (_s, _so, _d, do, n) in steps[0])
    for (_sb, so, _db, _do, n) in steps[1][:D.NDEP]:
        hit = [(lo, hi) for (lo, hi) in wr if lo < so + n and so < hi]
        assert len(hit) == 2 and hit[0][1] - so == 1 and so + n - hit[1][0] == 1, (so, n, hit)
        assert n - 2 >= 16                          # the stretch between them, which nothing wrote


def test_twins_are_hazard_free(xg):
    """the same copies with the dependent sources moved to SEND (a rewrite: made identical): no
    hazard point, rail-safe, no dependency but identical rewrites"""
    for kind in D.KINDS:
        steps, sb, rb = D.solo_kind(kind, PER)
        tw, tsb = D.twin(steps, sb, rb)
        assert [[c[2:] for c in st] for st in tw] == [[c[2:] for c in st] for st in steps]
        job = D.solo_job(tw, tsb, rb, kind + "_twin")
        job.check()
        spans, size = job.spans()
        assert {d[2] for d in D.dependencies(spans, size)} <= {"same"}, kind
        assert xg.engine_hazards(spans)[1] == 0 and xg.rail_safe(spans), kind


CONTROLS = {"b_control": (4 * 0 + D.POST, 4 * 1 + PRE), "f_stage_control": (D.STAGE, PRE)}


def test_multi_gpu_jobs_are_valid_and_hold_their_dependency(xg):
    """every phase of every GPU race-free, xg_calls_match pairs every call (with the local copies in
    the group too), and the named dependency is there between the named phases, on every GPU"""
    for name, build in D.PAIR_JOBS.items():
        job, want = build()
        job.check()
        assert all(max(job.bytes[g]) < 8 << 20 for g in range(job.G)), name
        for self_max in (0, 1 << 30):
            calls = job.calls(xg, self_max)
            pairs = xg.calls_match(calls, job.nsteps)
            sends = sum(1 for g in range(job.G) for st in calls[g] for c in st if c[0] == xg.CALL_SEND)
            recvs = sum(1 for g in range(job.G) for st in calls[g] for c in st if c[0] == xg.CALL_RECV)
            assert len(pairs) == sends == recvs and sends > 0, (name, self_max, len(pairs), sends, recvs)
        for g in range(job.G):
            ph, size = job.phases(g)
            deps = D.dependencies(ph, size)
            for (kind, (si, pi), (sj, pj)) in want:
                assert (4 * si + pi, 4 * sj + pj, kind) in deps, (name, g, kind, sorted(deps))
            if name in CONTROLS:                   # the control lacks exactly what its twin has
                i, j = CONTROLS[name]
                assert not [d for d in deps if d[:2] == (i, j)], (name, sorted(deps))


def test_reference_executor_runs_in_order():
    """Job.execute against bytes worked out by hand: a forward through the exchange, a
    write-after-read in one step, simultaneous copies inside a phase"""
    job, _ = D.job_war_exchange()
    init = job.initial(1)
    out = job.execute([[a.copy() for a in regs] for regs in init])
    L = sum(D.ODD_LENS)
    for g in range(2):
        assert (out[g][R][64:64 + L] == init[1 - g][R][64:64 + L]).all()              # step 0
        assert (out[g][R][64 + L + 64:64 + 2 * L + 64] == init[g][R][64:64 + L]).all()     # there and back
        assert (out[g][S] == init[g][S]).all()
    swap = D.Job(1, [(0, 32, 0)], [[D.Part(local=[(R, 0, R, 16, 16), (R, 16, R, 0, 16)])]], "swap")
    with pytest.raises(AssertionError):
        swap.check()                        # a race inside one phase is no valid plan
    regs = [[np.zeros(0, np.uint8), np.arange(32, dtype=np.uint8)] + [np.zeros(0, np.uint8)] * 3]
    swap.execute(regs)
    assert list(regs[0][R]) == list(range(16, 32)) + list(range(16))                  # sources read first


# ------------------------------------------------------------------ xg_engine_hazards against walks
def _random_steps(rng, size):
    """a few steps of a few copies inside [0, size), no race inside a step"""
    steps = []
    for _s in range(int(rng.integers(2, 7))):
        st = []
        for _try in range(int(rng.integers(1, 5))):
            n = int(rng.choice([1, 3, 8, 16, 17, 40]))
            src, dst = int(rng.integers(0, size - n)), int(rng.integers(0, size - n))
            if rng.random() < 0.3 and steps and steps[-1]:           # an identical rewrite of an earlier copy
                src, dst, n = steps[-1][int(rng.integers(len(steps[-1])))]
            c = (src, dst, n)
            ok = not (src < dst + n and dst < src + n)
            for (s2, d2, n2) in st:
                ok = ok and not (dst < d2 + n2 and d2 < dst + n) and not (dst < s2 + n2 and s2 < dst + n) \
                    and not (d2 < src + n and src < d2 + n2)
            if ok:
                st.append(c)
        steps.append(st)
    return steps


def test_engine_hazards_match_a_direct_walk(xg):
    """300 seeded random step lists in a 256-B region.  Wherever step j reads, or rewrites with other
    bytes, a byte last written by step i < j, some flag in [i, j - 1] is 2; no flag is 2 where no
    such pair begins after the last 2 (together: exactly the byte walk's flags)"""
    rng = np.random.default_rng(20)
    seen2 = seen0 = 0
    for case in range(300):
        steps = _random_steps(rng, 256)
        spans = [[(1 << 20 | s, 1 << 20 | d, n) for (s, d, n) in st] for st in steps]     # any base address
        flags, nhaz = xg.engine_hazards(spans)
        assert nhaz == flags.count(2) and flags[-1] >= 1 and set(flags[:-1]) <= {0, 2}, (case, flags)
        for (i, j, kind) in D.dependencies(steps, 256):
            if kind in ("raw", "waw"):
                assert 2 in flags[i:j], (case, steps, flags, (i, j, kind))
        walk = D.hazard_walk(steps, 256)
        assert [f == 2 for f in flags] == [f == 2 for f in walk], (case, steps, flags, walk)
        seen2 += nhaz > 0
        seen0 += nhaz == 0
    assert seen2 > 50 and seen0 > 50, (seen2, seen0)


# ------------------------------------------------------------------ xg_step_packs_meet_unpacks
def _meet(xg, unp, local, packs, step=1):
    dp = _plan(xg, [([], [], [(S, 0, SS, 0, 150)], unp), ([], local, packs, [])])
    return xg.host().xg_step_packs_meet_unpacks(C.byref(dp), step)


def test_packs_meet_unpacks(xg):
    """a pack of step s that reads a byte step s - 1's unpacks write keeps out of their launch: the
    first and the last byte of an unpack, a longer unpack that starts lower, empty copies, another
    region, and local copies (xg_step_local_meets_unpacks' business) never count"""
    unp = [(SR, 0, R, 1000, 100), (SR, 100, R, 1010, 20), (SR, 120, SC, 5000, 50)]   # RECV [1000,1100) over [1010,1030); SCRATCH [5000,5050)
    cases = [
        ([(S, 0, SS, 0, 64)], 0),                    # out of SEND
        ([(R, 2000, SS, 0, 64)], 0),                 # RECV, elsewhere
        ([(R, 936, SS, 0, 64)], 0),                  # ends where the unpack starts
        ([(R, 937, SS, 0, 64)], 1),                  # reads its first byte
        ([(R, 1000, SS, 0, 1)], 1),
        ([(R, 1099, SS, 0, 1)], 1),                  # its last byte (the longer unpack that starts lower ends there)
        ([(R, 1099, SS, 0, 64)], 1),
        ([(R, 1100, SS, 0, 64)], 0),                 # the byte after
        ([(R, 1030, SS, 0, 8)], 1),                  # past the short unpack, inside the long one
        ([(SC, 1050, SS, 0, 8)], 0),                 # the same offsets in another region
        ([(SC, 5049, SS, 0, 8)], 1),
        ([(S, 1050, SS, 0, 8)], 0),
        ([(R, 1050, SS, 0, 0)], 0),                  # an empty pack
        ([(S, 0, SS, 0, 16), (R, 1100, SS, 16, 16), (R, 1029, SS, 32, 4)], 1),     # the third of three
    ]
    for packs, want in cases:
        assert _meet(xg, unp, [], packs) == want, (packs, want)
        assert _meet(xg, unp, [(R, 1050, SC, 0, 8)], packs) == want, (packs, want)      # a local copy that does meet them
    for empty in ([], [(SR, 0, R, 1000, 0), (SR, 0, R, 5000, 0)]):                      # no unpacks, or only empty ones
        assert _meet(xg, empty, [], [(R, 1000, SS, 0, 64)]) == 0
    assert _meet(xg, unp, [(R, 1050, SC, 0, 8)], []) == 0                               # no packs
    assert xg.host().xg_step_local_meets_unpacks(
        C.byref(_plan(xg, [([], [], [(S, 0, SS, 0, 150)], unp), ([], [], [(R, 1050, SS, 0, 8)], [])])), 1) == 0
    assert _meet(xg, unp, [], [(R, 1000, SS, 0, 8)], step=0) == -1
    assert _meet(xg, unp, [], [(R, 1000, SS, 0, 8)], step=2) == -1


def test_packs_meet_unpacks_matches_its_definition(xg):
    """300 seeded random cases: the C test equals a brute-force overlap check; both answers occur"""
    rng = np.random.default_rng(4)
    seen = [0, 0]
    for case in range(300):
        unp, at = [], 0
        for _ in range(int(rng.integers(0, 5))):
            n = int(rng.choice([0, 1, 7, 16, 60]))
            unp.append((SR, at, int(rng.choice([R, SC])), int(rng.integers(0, 100)), n))
            at += n
        packs, at = [], 0
        for _ in range(int(rng.integers(0, 4))):
            n = int(rng.choice([0, 1, 5, 16, 33]))
            packs.append((int(rng.choice([S, R, SC])), int(rng.integers(0, 100)), SS, at, n))
            at += n
        local = [(R, int(rng.integers(0, 300)), SC, 400, 8)] if case % 3 == 0 else []
        want = int(any(n > 0 and un > 0 and sb == ub and so < uo + un and uo < so + n
                       for (sb, so, _db, _do, n) in packs for (_s, _o, ub, uo, un) in unp))
        assert _meet(xg, unp, local, packs) == want, (case, unp, packs)
        seen[want] += 1
    assert min(seen) > 40, seen


def test_real_plans_never_forward_their_unpacks(xg):
    """every golden-shape plan on 2 and 8 GPUs in every pack form: no pack reads a byte the step
    before unpacked (so the fused unpack + pack launch loses no step to the new test), and steps with
    packs right behind a step with unpacks exist"""
    from conftest import golden_configs, load_golden
    behind = 0
    for cfg in golden_configs():
        meta, _, _ = load_golden(cfg)
        for m in meta["method_list"]:
            s = xg.Schedule(m, meta["P"], meta["A"], meta["d"], meta["c"], meta["aggregators"], ntimes=meta["ntimes"],
                            proc_node=meta["proc_node"], barrier_type=meta["barrier"])
            for G in (2, 8):
                if G > meta["P"]:
                    continue
                for form in (-1, 0, 1):
                    for g in range(G):
                        v = s.devplan(G, g, 1 << 30, 0, form)
                        for st in range(1, v.nsteps):
                            assert v.packs_meet_unpacks(st) == 0, (cfg, m, G, form, g, st)
                            pb, pc, _qb, _qc, _ob, _oc = v.steps[st]
                            behind += v.steps[st - 1][5] > 0 and any(c[2] == SS for c in v.copies[pb:pb + pc])
    assert behind > 100, behind
