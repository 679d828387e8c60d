"""Host side of the ping-pong plans (pingpong.py) that test_gpu_back_to_back.py posts back to back:
what a GPU test leans on is proven here, without a GPU.

  * the image after k rounds -- the in-order numpy execution -- equals the closed form (every A
    slot moved k slots on along the ring of its length, B a copy of A), and the images after
    0 .. kmax rounds are pairwise distinct: a lost, repeated or reordered run changes the image;
  * every slot lies between >= 16 poisoned bytes (_assert_gaps over both plans' destinations, which
    are all slots of both areas), every region stays under 2 MiB, both plans are rail-safe;
  * under each case's knobs xg.PlanTables gives exactly the stated form: launches, segments with
    their kind, rails or workgroups and granule, chains, launches per kernel kind, graph_auto,
    arming -- and the dispatches' bytes (dispatch_bytes) add up to the plan's.
"""
import numpy as np
import pytest

import pingpong as PP
from synth_plan import DBASE, Synth, _assert_gaps
from time_plan import devplan


def _pp(case):
    return PP.pingpong(**PP.CASES[case]["gen"])


def _random(pp, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, pp.send_bytes, dtype=np.uint8), rng.integers(0, 256, pp.recv_bytes, dtype=np.uint8)


def _closed_form(pp, k, recv0):
    """RECV after k rounds, by the rotation: not computed from the step lists"""
    out = recv0.copy()
    n = len(pp.slots_a)
    for i, (off, ln) in enumerate(pp.slots_a if k else []):
        j = (i + k * pp.L) % n
        for slots in (pp.slots_a, pp.slots_b):
            assert slots[j][1] == ln
            out[slots[j][0]:slots[j][0] + ln] = recv0[off:off + ln]
    return out


@pytest.mark.parametrize("case", list(PP.CASES))
def test_images_after_k_rounds(case):
    """in-order execution == closed form for every k <= kmax, and the images are pairwise distinct"""
    pp, kmax = _pp(case), PP.CASES[case]["kmax"]
    assert kmax < pp.ring
    send, recv0 = _random(pp, 11)
    keep = send.copy()
    imgs = pp.images(kmax, send, recv0)
    assert (send == keep).all()
    for k, img in enumerate(imgs):
        want = _closed_form(pp, k, recv0)
        assert (img == want).all(), (case, k, "in-order execution and the rotation differ first at RECV[%d]"
                                     % int(np.flatnonzero(img != want)[0]))
        assert (img == pp.image(k, send, recv0)).all()
    for i in range(len(imgs)):
        for j in range(i + 1, len(imgs)):
            assert (imgs[i] != imgs[j]).any(), (case, "the images after %d and %d rounds are the same" % (i, j))


@pytest.mark.parametrize("case", list(PP.CASES))
def test_round_is_synth_expected(case):
    """round() is Synth.expected of a, then of b, on an object that holds what a loaded Synth holds"""
    import types
    pp = _pp(case)
    send, recv0 = _random(pp, 12)
    sa = types.SimpleNamespace(send=send, recv=recv0, steps=pp.steps_a)
    mid = Synth.expected(sa)
    sb = types.SimpleNamespace(send=send, recv=mid, steps=pp.steps_b)
    assert (Synth.expected(sb) == pp.round(send, recv0)).all()
    # a changes B only, b changes A only
    a_lo, a_hi = pp.slots_a[0][0], pp.slots_a[-1][0] + pp.slots_a[-1][1]
    b_lo = pp.slots_b[0][0]
    assert a_hi < b_lo and (mid[:b_lo] == recv0[:b_lo]).all() and (Synth.expected(sb)[b_lo:] == mid[b_lo:]).all()
    assert a_lo >= 16


@pytest.mark.parametrize("case", list(PP.CASES))
def test_layout(xg, case):
    pp = _pp(case)
    assert (PP.RAGGED, PP.EXTENTS) == (xg.DP_RAGGED, xg.DP_EXTENTS)
    _assert_gaps(pp.steps_a, pp.recv_bytes)
    _assert_gaps(pp.steps_b, pp.recv_bytes)
    _assert_gaps(pp.steps_a + pp.steps_b, pp.recv_bytes)           # A's and B's slots together
    assert pp.recv_bytes < 2 << 20 and pp.send_bytes < 2 << 20
    ph = PP.CASES[case]["gen"].get("phase", (0, 0))
    assert all(off % 16 == ph[0] for off, _n in pp.slots_a) and all(off % 16 == ph[1] for off, _n in pp.slots_b)
    assert [c for st in pp.steps_a for c in st] == [(1, pp.slots_a[i][0], 1, pp.slots_b[pp.nxt(i)][0], pp.slots_a[i][1])
                                                    for i in range(len(pp.slots_a))]
    assert pp.steps_b == [[(1, b[0], 1, a[0], a[1]) for a, b in zip(pp.slots_a, pp.slots_b)]]
    for steps in (pp.steps_a, pp.steps_b):
        assert xg.rail_safe([[(DBASE + so, DBASE + do, n) for (_sb, so, _db, do, n) in st] for st in steps])
        assert xg.engine_hazards([[(DBASE + so, DBASE + do, n) for (_sb, so, _db, do, n) in st] for st in steps])[1] == 0


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("case", list(PP.CASES))
def test_routing(xg, case, which):
    """the form of each plan under the case's knobs, on a 256-CU device"""
    c, pp = PP.CASES[case], _pp(case)
    steps = pp.steps_a if which == "a" else pp.steps_b
    dp = devplan(xg, steps, pp.send_bytes, pp.recv_bytes)
    dp.flags = pp.flags
    pt = xg.PlanTables(dp, env=c["env"])
    try:
        rec = pt.records()
        f = PP.form(rec, pt.kind_launches())
        assert f == c[which], (f, c[which])
        disp = PP.dispatch_bytes(rec)
        assert len(disp) == pt.launches() == f["launches"]
        assert sum(disp) == pp.bytes_a() and all(x > 0 for x in disp)
        assert pt.engine_rails() == (f["segs"][0]["w"] if f["segs"] and f["segs"][0]["solo"] else 0)
        assert pt.engine() == (f["segs"][0]["w"] if f["segs"] else 0)
        if c.get("graph"):          # a run of a is replayed as a graph: asked for, or by default
            assert (f["launches"] > 1 and (c["env"].get("XG_GRAPH") == 1 or
                                           ("XG_GRAPH" not in c["env"] and f["graph_auto"]))) == (which == "a")
    finally:
        pt.close()


def test_cut_case_has_unequal_dispatches(xg):
    """the case that checks a cut launch's per-dispatch bytes: both plans hold a launch of several
    dispatches, none of them as long as its launch and not all equally long"""
    c, pp = PP.CASES["cut"], _pp("cut")
    for steps in (pp.steps_a, pp.steps_b):
        dp = devplan(xg, steps, pp.send_bytes, pp.recv_bytes)
        pt = xg.PlanTables(dp, env=c["env"])
        try:
            rec = pt.records()
            cutl = [l for l in rec["launch"] if l["ndisp"] > 1]
            assert cutl
            disp = PP.dispatch_bytes(rec)
            for l in cutl:
                assert all(x < l["bytes"] for x in disp[:l["ndisp"]])      # the cut launch is each plan's first
                assert len(set(disp[:l["ndisp"]])) > 1
        finally:
            pt.close()
