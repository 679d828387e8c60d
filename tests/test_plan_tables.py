"""CPU: the tables a plan load builds (csrc/host/plan_tables.cc), built with no GPU.

xg.PlanTables builds what xg_plan_load builds -- pieces, copy launches, dispatch cuts, tile tables,
copy_kernel_q rows, displacement fix-ups, engine segments -- from a device plan, a set of knobs and
fake region addresses (2 MiB-aligned unless a test says otherwise), and writes them as text; the
tests read that text.  The device plans come from the real host library (devplan.c, place.c) or are
hand-made as in synth_plan.py / dep_plan.py.

The dispatch-cut cases run in a child process each (this file, run as a script) under a time limit
and an address-space limit: a cut loop that stops advancing fails its test and does not stall the
suite."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mpi-asynchronous-communication-test_amd")
S, R, SS, SR = 0, 1, 2, 3       # XG_BUF_SEND, RECV, STAGE_SEND, STAGE_RECV


# ------------------------------------------------------------------ the cover property
def patched_pieces(t):
    """the piece table with every fix-up applied as the device scan applies it: the staging side of
    piece f.piece = staging base + the host displacement of copy f.copy + f.off"""
    pieces = [list(p) for p in t.get("piece", [])]
    lens, host = t.get("disp_len", []), t.get("disp_host", [])
    seen = set()
    for f in t.get("fix", []):
        p = pieces[f["piece"]]
        assert f["piece"] not in seen, ("two fix-ups for one piece", f)
        seen.add(f["piece"])
        assert 0 <= f["off"] and f["off"] + p[2] <= lens[f["copy"]], ("a fix-up past its copy", f, p)
        side = 1 if f["side"] == 0 else 0                    # side 0 patches dst (pack), 1 src (unpack)
        assert p[side] == (SS if f["side"] == 0 else SR, f["off"]), ("unpatched staging side", f, p)
        p[side] = (p[side][0], host[f["copy"]] + f["off"])
    return pieces


def check_cover(xg, t, view_copies, view_steps, stage_count):
    """every positive copy of the device plan is covered exactly once, byte for byte, by the pieces
    and rows of ONE launch of its own step -- or of the next step's launch that holds the previous
    unpacks, when the step is deferred; nothing else is in the tables; local and unpack ranges in
    destination order; the launch table tiled by the steps"""
    pieces = patched_pieces(t)
    rows = t.get("row", [])
    launches, steps = t.get("launch", []), t.get("step", [])
    at = 0
    for st in steps:
        lb, lr, le = st["l"]
        assert lb == at and lb <= lr <= le, ("launch ranges", st)
        at = le
    assert at == len(launches)
    # what each launch offers: (src, dst) -> [len] of its pieces / rows
    offer = []
    for l in launches:
        d = {}
        for p in pieces[l["b"]:l["b"] + l["n"]]:
            d.setdefault((p[0], p[1]), []).append(p[2])
        if l["kind"] == xg.COPY_SMALL:
            qr, qc = l["q"][0], l["q"][1]
            for r in rows[qr:qr + qc]:
                d.setdefault((r[0], r[1]), []).append(r[2])
        offer.append(d)
    used = 0
    for s, (pre_b, pre_n, _pb, _pn, post_b, post_n) in enumerate(view_steps):
        form = steps[s]["form"]
        own = list(range(*steps[s]["l"][::2]))
        nxt = list(range(*steps[s + 1]["l"][::2])) if s + 1 < len(steps) else []
        for i in list(range(pre_b, pre_b + pre_n)) + list(range(post_b, post_b + post_n)):
            sb, so, db, do, n = view_copies[i]
            if n <= 0:
                continue
            post = i >= post_b and i < post_b + post_n
            local = not post and i - pre_b >= stage_count[s] and db != SS
            if local and form & xg.FORM_SELF_LOCAL:
                continue                                   # travels in the step's RCCL group
            where = [j for j in nxt if launches[j]["mark_prev"]] if post and form & xg.FORM_DEFERRED else own
            took = None
            o = 0
            while o < n:
                key = ((sb, so + o), (db, do + o))
                cand = [j for j in where if offer[j].get(key)]
                assert len(cand) == 1, ("copy %d of step %d at byte %d: launches %s hold it" % (i, s, o, cand), key)
                assert took in (None, cand[0]), ("copy %d of step %d lies in two launches" % (i, s))
                took = cand[0]
                ln = offer[took][key].pop()
                assert 0 < ln <= n - o, ("a piece longer than the rest of its copy", i, s, o, ln)
                o += ln
                used += 1
    assert used == len(pieces) + len(rows), ("pieces or rows that belong to no copy", used, len(pieces), len(rows))
    for st in steps:
        for name in ("local", "post"):
            b, n = st[name]
            dst = [pieces[i][1] for i in range(b, b + n)]
            assert dst == sorted(dst), (name, "pieces out of destination order", st)
    for l in launches:
        if l["kind"] == xg.COPY_SMALL:
            dst = [r[1] for r in rows[l["q"][0]:l["q"][0] + l["q"][1]]]
            assert dst == sorted(dst)


def view_tables(xg, v, **knobs):
    """the tables of a DevicePlanView as GPU v.gpu of v.ngpus"""
    kn = dict(rank=v.gpu, nranks=v.ngpus, virt=int(v.ngpus > 1))
    kn.update(knobs)
    return xg.PlanTables(v.ptr, **kn)


def check_view(xg, v, **knobs):
    pt = view_tables(xg, v, **knobs)
    try:
        t = pt.records()
        check_cover(xg, t, v.copies, v.steps, v.stage_count)
        return t
    finally:
        pt.close()


from conftest import golden_configs, load_golden      # noqa: E402

PACKS = ((0, -1), (4 << 20, 0), (4 << 20, 1), (0, 2), (0, 3))       # direct and every pack form (xg_sched.h)


@pytest.mark.parametrize("G", [1, 2, 8])
@pytest.mark.parametrize("cfg", golden_configs())
def test_cover_golden(xg, cfg, G):
    """every golden config x method x G in {1, 2, 8} x {direct, every pack form}; of 8 GPUs the
    first, one in the middle and the last"""
    meta, _, _ = load_golden(cfg)
    for m in meta["method_list"]:
        s = xg.Schedule(m, meta["P"], meta["A"], meta["d"], meta["c"], meta["aggregators"], ntimes=meta["ntimes"],
                        proc_node=meta["proc_node"], barrier_type=meta["barrier"])
        for pack, form in (PACKS if G > 1 else PACKS[:1]):
            for g in sorted({0, G // 2 - (G > 2), G - 1}):
                try:
                    v = s.devplan(G, g, pack, 0, form)
                except xg.XGError:
                    continue
                check_view(xg, v)


def test_cover_ragged(xg):
    """the ragged cases of test_ragged_sched.py: P 7, A 3, seeded lengths, G = 1..4, every form"""
    import test_ragged_sched as RS
    for method in RS.RAGGED_METHODS:
        s = RS._sched(xg, method)
        for G in (1, 2, 3, 4):
            for pack, form in [(0, -1)] + [(1 << 20, f) for f in RS.FORMS]:
                for g in range(G):
                    check_view(xg, s.devplan(G, g, pack, 0, form))


# test_gpu_place.py's lists (extents of 0..3000 B: their mean is above the EXTENT routing threshold) and
# the same with extents of 0..1500 B, which run copy_kernel_x
PLACE = [(8, 3, 600 + m, m, G, ml) for m in (1, 2, 3, 5) for G in (1, 2) for ml in (3000, 1500)]


def _place_views(xg, P, A, seed, method, G, max_len):
    from place_cases import make_exts
    exts, dom = make_exts(P, A, seed=seed, max_len=max_len)
    s = xg.Schedule(method, P, A, 0, 3, xg.aggregator_list(P, A), lens=xg.exts_lens(exts, P, A))
    return [s.place_plan(G, g, exts, dom) for g in range(G)]


@pytest.mark.parametrize("case", PLACE, ids=lambda c: "P%d_A%d_s%d_m%d_G%d_len%d" % c)
@pytest.mark.parametrize("launch_max", [512 << 20, 4096])
def test_cover_and_tiles_of_placement_plans(xg, case, launch_max):
    """the placement cases of place_cases.py: the cover property, and every dispatch of every EXTENT
    launch has a tile table that starts at 0, ends at its piece count and respects both caps (a
    tile holds at most 256 pieces and, unless it is one piece, at most extent_tile bytes)"""
    tile_bytes, tile_pieces = 32 << 10, 256
    for v in _place_views(xg, *case):
        t = check_view(xg, v, launch_max=launch_max)
        ext = [l for l in t.get("launch", []) if l["kind"] == xg.COPY_EXTENT]
        assert ext or case[5] > 1024 or not any(c[4] > 0 for c in v.copies)
        plen = [p[2] for p in t.get("piece", [])]
        for l in ext:
            for k in range(l["ndisp"]):
                b, e = t["cut"][l["cut"] + k], t["cut"][l["cut"] + k + 1]
                off, nt = t["xt_off"][l["xt"] + k], t["xt_n"][l["xt"] + k]
                begin = t["xt_begin"][off:off + nt + 1]
                assert begin[0] == 0 and begin[-1] == e - b and nt >= 1, (l, k, begin[:3], begin[-1], e - b)
                for x, y in zip(begin, begin[1:]):
                    assert 0 < y - x <= tile_pieces
                    assert y - x == 1 or sum(plen[b + x:b + y]) <= tile_bytes, (l, k, x, y)


# ------------------------------------------------------------------ dispatch cuts (child processes)
CUT_CAPS = [1, 4096, 65536, 512 << 20, 0]


def _synth_devplan(xg, steps, send_bytes, recv_bytes):
    """synth_plan.Synth._load's xg_devplan: one GPU, steps of (src_buf, src_off, dst_buf, dst_off, len)"""
    copies = [c for st in steps for c in st]
    arr = (xg.Copy * max(1, len(copies)))(*[xg.Copy(so, do, ln, sb, db) for (sb, so, db, do, ln) in copies])
    sp, b = [], 0
    for st in steps:
        sp.append(xg.StepPlan(b, len(st), 0, 0, 0, 0, 0, 0))
        b += len(st)
    spa = (xg.StepPlan * max(1, len(sp)))(*sp)
    p2p = (xg.P2P * 1)()
    dp = xg.DevPlan()
    dp.gpu, dp.ngpus, dp.nsteps = 0, 1, len(steps)
    for i, v in enumerate((send_bytes, recv_bytes, 0, 0, 0)):
        dp.region_bytes[i] = v
    dp.ncopy, dp.np2p = len(copies), 0
    dp.copies = C.cast(arr, C.POINTER(xg.Copy))
    dp.p2p = C.cast(p2p, C.POINTER(xg.P2P))
    dp.steps = C.cast(spa, C.POINTER(xg.StepPlan))
    dp._keep = (arr, spa, p2p)
    return dp


def _one_step(lens):
    """one step of SEND -> RECV copies of these lengths, back to back on the 16-B grid"""
    st, at = [], 0
    for n in lens:
        st.append((S, at, R, at, n))
        at += (n + 15) & ~15
    return [st], at, at


def _only_chunk(n):
    """a chunk of at least n bytes that is the only piece size xg_piece_size may take: it halves its
    candidates while they are multiples of 16, and half of 16 x an odd number is none"""
    return ((n + 15) // 16 | 1) * 16


def cut_case(name, cap):
    """-> (steps, send_bytes, recv_bytes, knobs): the pieces are the copies (each at most one chunk)
    unless the case says otherwise.  `unit` scales the lengths to the cap so that a launch of a few
    thousand pieces is cut at every cap."""
    unit = 1 << 20 if cap >= 1 << 29 else 1024
    chunk = 1 << 20 if cap >= 1 << 29 else 32768
    # no WAVE launch (its pieces are 2 - 8 KiB whatever the chunk), no engine: PIECE launches cut by xg_piece_size
    kn = dict(launch_max=cap, chunk=chunk, engine_max_step=0, small_pieces=0, wave_min=1 << 60)
    rng = np.random.default_rng(5)
    if name == "random":        # a few thousand pieces of random lengths, three launches (steps)
        steps, at = [], 0
        for n in (3000, 1, 700):
            st = []
            for ln in rng.integers(1, unit + 1, n):
                st.append((S, at, R, at, int(ln)))
                at += (int(ln) + 15) & ~15
            steps.append(st)
        return steps, at, at, kn
    if name == "one_large":     # one piece larger than the cap among small ones (the chunk admits it)
        big = max(4096, cap + cap // 3)
        kn.update(chunk=_only_chunk(big))
        return _one_step([64] * 40 + [big] + [64] * 40) + (kn,)
    if name == "equal_cap":     # every piece equal to the cap (at least 16 B; cap 0: 4 KiB)
        ln = max(cap, 16) if cap else 4096
        kn.update(chunk=_only_chunk(ln))
        return _one_step([ln] * 100) + (kn,)
    if name == "one_piece":     # one-piece launches
        steps, at = [], 0
        for ln in (1, 16, 4096, chunk):
            steps.append([(S, at, R, at, ln)])
            at += (ln + 15) & ~15
        return steps, at, at, kn
    if name == "small":         # uniform copy_kernel_q launches: 13 pieces of 8 KiB per copy, so a cut of
        kn.update(small_pieces=1, small_piece_min=0, chunk=32768)      # cap / 8 KiB pieces falls inside a copy
        ncopy = 40 if cap < 1 << 29 else 3 * (cap >> 20) // 2 * 10 + 7
        return _one_step([13 * 8192] * ncopy) + (kn,)
    if name == "small_tail":    # the same with a last piece of 4 KiB per copy
        kn.update(small_pieces=1, small_piece_min=0, chunk=32768)
        return _one_step([12 * 8192 + 4096] * 40) + (kn,)
    raise KeyError(name)


CUT_CASES = ["random", "one_large", "equal_cap", "one_piece", "small", "small_tail"]


def _child(name, cap):
    """run as a script: build the case's tables and print the dump's launch, cut and piece records"""
    import resource
    resource.setrlimit(resource.RLIMIT_AS, (4 << 30, 4 << 30))      # a cut loop that only appends ends here
    sys.path.insert(0, os.path.dirname(HERE))
    import __graft_entry__ as G
    xg = G.load_package().xg
    steps, sb, rb, kn = cut_case(name, cap)
    pt = xg.PlanTables(_synth_devplan(xg, steps, sb, rb), **kn)
    t = pt.records()
    out = dict(launch=t.get("launch", []), cut=t.get("cut", []), plen=[p[2] for p in t.get("piece", [])],
               qbytes=t.get("qbytes", []), nlaunch=t["plan"]["nlaunch"])
    print(json.dumps(out))


@pytest.mark.parametrize("cap", CUT_CAPS)
@pytest.mark.parametrize("name", CUT_CASES)
def test_dispatch_cuts(xg, name, cap):
    """cuts strictly increase from the launch's first piece to its last; every dispatch but the last
    holds at least launch_max bytes; the last is no runt by the code's rule (>= 16 pieces and >= half
    the cap, unless it is the only one); qbytes sums to the launch's bytes; a launch of at most
    1.5 x the cap is one dispatch (and so is every launch at cap 0).
    small_tail: a copy_kernel_q dispatch is cap / piece whole pieces (cut_small counts pieces, not
    bytes), so where copies end in a short piece -- and the piece order puts eight copies' last
    pieces side by side -- a dispatch may hold less than the cap: there the piece count and the bytes
    xg_small_piece_at gives those pieces are asserted, the bound in bytes only for `small`."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(cap)], capture_output=True, text=True,
                         timeout=8)
    assert out.returncode == 0, out.stderr[-2000:]
    t = json.loads(out.stdout)
    plen, cuts = t["plen"], t["cut"]
    steps, _sb, _rb, _kn = cut_case(name, cap)
    want = [sum(c[4] for c in st) for st in steps]
    assert [l["bytes"] for l in t["launch"]] == want
    if name == "equal_cap":
        assert plen == [max(cap, 16) if cap else 4096] * 100
    if name == "one_large":
        assert sorted(plen) == [64] * 80 + [max(4096, cap + cap // 3)]
    ndisp = 0
    for l in t["launch"]:
        c = cuts[l["cut"]:l["cut"] + l["ndisp"] + 1]
        small = l["kind"] == xg.COPY_SMALL
        assert (name.startswith("small")) == small
        if small:
            piece = l["kib"] << 10
            q_copies, q_len = l["q"][1], l["q"][4]
            ppc = -(-q_len // piece)
            first, last = 0, q_copies * ppc
            nb = t["qbytes"][l["q"][3]:l["q"][3] + l["ndisp"]]
            assert sum(nb) == l["bytes"] == q_copies * q_len
        else:
            first, last = l["b"], l["b"] + l["n"]
            nb = [sum(plen[x:y]) for x, y in zip(c, c[1:])]
            assert sum(nb) == l["bytes"]
        assert c[0] == first and c[-1] == last and all(x < y for x, y in zip(c, c[1:])), (l, c[:4], c[-2:])
        if cap == 0 or l["bytes"] <= cap + cap // 2:
            assert l["ndisp"] == 1, l
        for k, n in enumerate(nb[:-1]):
            if small:
                assert c[k + 1] - c[k] == max(1, cap // piece), (l, k)
                assert n == sum(xg.small_piece_at(w, q_copies, q_len, piece, l["q"][2])[2] for w in range(c[k], c[k + 1]))
                if name == "small":
                    assert n >= cap, (l, k, n)
            else:
                assert n >= cap, (l, k, n)
        if l["ndisp"] > 1:
            assert c[-1] - c[-2] >= 16 and (nb[-1] if not small else (c[-1] - c[-2]) * piece) >= cap // 2, (l, nb[-1])
        ndisp += l["ndisp"]
    assert ndisp == t["nlaunch"]
    if name in ("random", "small") and cap:
        assert max(l["ndisp"] for l in t["launch"]) > 1, "the case cuts nothing at this cap"
    if name == "small" and cap == 65536:
        l = t["launch"][0]
        ppc = -(-l["q"][4] // (l["kib"] << 10))
        assert any(x % ppc for x in cuts[l["cut"] + 1:l["cut"] + l["ndisp"]]), "no cut inside a copy"


# ------------------------------------------------------------------ engine segments
def _seg_tables(xg, steps, send_bytes, recv_bytes, base=None, **knobs):
    pt = xg.PlanTables(_synth_devplan(xg, steps, send_bytes, recv_bytes), base=base, **knobs)
    try:
        t = pt.records()
        return t, pt.engine_steps(), pt.engine_rails()
    finally:
        pt.close()


def _check_seg_of(t):
    """seg_of and the segments agree: the segments are disjoint ascending step ranges, and step s
    names segment i exactly when s lies in it"""
    segs = t.get("seg", [])
    want = [-1] * len(t.get("step", []))
    end = 0
    for i, g in enumerate(segs):
        s0, s1 = g["steps"]
        assert end <= s0 < s1 <= len(want)
        end = s1
        want[s0:s1] = [i] * (s1 - s0)
    assert [st["seg"] for st in t["step"]] == want


@pytest.mark.parametrize("form", ["P", "W1", "W4", "W16"])
def test_window_plans_are_one_solo_segment(xg, form):
    """sparse_synth.window_plan: hulls of exactly 2^28 B (P) and 2^32 B (W1), bit 31 of a granule
    offset at granules 4 and 16 -- one solo segment over the plan's busy steps, on the rails
    test_gpu_solo_windows.py reads on the device; the bases are the hull's lowest addresses"""
    from sparse_synth import FORMS, bases, window_plan
    from synth_plan import _rails, _segment
    f = FORMS[form]
    rails_max = 512 if f["waves"] == 1 else 16
    steps, sb, rb = window_plan(form, rails_max)
    t, eng, rails = _seg_tables(xg, steps, sb, rb, solo_waves=f["waves"], solo_rails=rails_max)
    assert eng == (len(_segment(steps)), 1, 0), eng
    assert rails == _rails(steps, rails_max, f["waves"])
    g = t["seg"][0]
    assert g["solo"] == 1 and g["gran"] == f["G"] and g["wv"] == f["waves"]
    assert (g["sbase"], g["dbase"]) == ((S, bases(steps)[0]), (R, bases(steps)[1]))
    _check_seg_of(t)


@pytest.mark.parametrize("form", ["P", "W1"])
def test_one_granule_past_the_window_is_two_solo_segments(xg, form):
    """sparse_synth.split_steps: both hulls the window plus one granule.  "steps": solo_split cuts
    exactly once, at the step that forces it, and each part has bases of its own; "one_step": no
    cut helps, no rails"""
    from sparse_synth import FORMS, bases, split_steps
    from synth_plan import _rails
    f = FORMS[form]
    rails_max = 512 if f["waves"] == 1 else 16
    kn = dict(solo_waves=f["waves"], solo_rails=rails_max)
    steps, sb, rb, cut = split_steps(form, "steps")
    t, eng, rails = _seg_tables(xg, steps, sb, rb, **kn)
    assert eng == (len(steps), 2, 0), eng
    assert [g["steps"] for g in t["seg"]] == [[0, cut], [cut, len(steps)]]
    assert rails == _rails(steps[:cut], rails_max, f["waves"]) > 0
    for g, part in zip(t["seg"], (steps[:cut], steps[cut:])):
        assert g["solo"] == 1 and (g["sbase"], g["dbase"]) == ((S, bases(part)[0]), (R, bases(part)[1]))
    _check_seg_of(t)
    steps, sb, rb, _none = split_steps(form, "one_step")
    t, eng, rails = _seg_tables(xg, steps, sb, rb, **kn)
    assert rails == 0
    _check_seg_of(t)


@pytest.mark.parametrize("form", ["P", "W1"])
def test_a_part_of_exactly_the_window_is_kept_whole(xg, form):
    """sparse_synth.window_plan (both hulls exactly the window) and, behind it, one step whose copy
    reads one granule past the source hull and writes below the destination hull: the run no longer
    fits one table, and solo_split cuts it in exactly two -- the window plan's steps, whose hulls
    equal the window (a part may fill it: <=), and the added step"""
    from sparse_synth import EDGE, FORMS, window_plan
    from synth_plan import PIECE
    f = FORMS[form]
    rails_max = 512 if f["waves"] == 1 else 16
    steps, sb, rb = window_plan(form, rails_max)
    hull = sb - 2 * EDGE
    assert hull == f["window"] * f["G"]
    steps = steps[:-1] + [[]] * 24 + [[(S, EDGE + hull - PIECE + f["G"], R, 0, PIECE)], []]     # the empty steps: the split pays
    t, eng, _rails = _seg_tables(xg, steps, sb + f["G"], rb, solo_waves=f["waves"], solo_rails=rails_max)
    busy = [i for i, st in enumerate(steps) if st]
    assert eng == (busy[-1] + 1 - busy[0], 2, 0), eng
    assert [g["steps"] for g in t["seg"]] == [[busy[0], busy[-1]], [busy[-1], busy[-1] + 1]]
    assert all(g["solo"] for g in t["seg"])
    _check_seg_of(t)


def test_write_after_read_takes_the_grid_engine(xg):
    """the plan of test_gpu_solo_synth.py: step 0 copies RECV[X] on to RECV[Y], step 1 overwrites
    RECV[X] from SEND -- no hazard flag, but no rails (xg_engine_rail_safe): one grid segment.  The
    same for dep_plan's war kind; synth_plan._round_steps(reader) reads what step 0 wrote: a hazard"""
    import dep_plan as D
    from synth_plan import _round_steps
    L = 64 << 10
    X, Y = 64, 64 + L + 64
    t, eng, rails = _seg_tables(xg, [[(1, X, 1, Y, L)], [(0, 0, 1, X, L)]], L, Y + L + 64)
    assert eng == (2, 1, 0) and rails == 0 and t["seg"][0]["solo"] == 0 and t["seg"][0]["w"] > 0, (eng, rails)
    _check_seg_of(t)
    steps, sb, rb = D.solo_kind("war", 2 * D.NDEP)
    t, eng, rails = _seg_tables(xg, steps, sb, rb)
    assert eng == (len(steps), 1, 0) and rails == 0 and t["seg"][0]["solo"] == 0, (eng, rails)
    _check_seg_of(t)
    steps, sb, rb = _round_steps(4, 20, reader=True)
    t, eng, rails = _seg_tables(xg, steps, sb, rb)
    assert eng[:2] == (4, 1) and eng[2] >= 1 and rails == 0 and t["seg"][0]["solo"] == 0, (eng, rails)
    _check_seg_of(t)


@pytest.mark.parametrize("align,gran", [(4, 4), (1, 1), (16, 16)])
def test_region_bases_set_the_solo_granule(xg, align, gran):
    """16-B aligned offsets and lengths in regions whose bases are only 4-B / 1-B aligned: the
    descriptors' granule is the bases' alignment"""
    from synth_plan import _capacity_steps
    steps, sb, rb = _capacity_steps(4)
    base = [((b + 1) << 40) + (align if align < 16 else 0) for b in range(5)]
    t, eng, rails = _seg_tables(xg, steps, sb, rb, base=base)
    assert eng[1] == 1 and rails > 0, (eng, rails)
    assert t["seg"][0]["gran"] == gran and t["seg"][0]["solo"] == 1
    _check_seg_of(t)


# ------------------------------------------------------------------ step forms
NO_LOCAL_FORMS = dict(self_max=0, split_min=1 << 40)


def _job_forms(xg, name, **knobs):
    import dep_plan as D
    job, _want = D.PAIR_JOBS[name]()
    out = []
    for g in range(job.G):
        pt = xg.PlanTables(job.devplan(xg, g), rank=g, nranks=job.G, virt=1, **knobs)
        out.append(([pt.step_form(s) for s in range(job.nsteps)], pt.launches(), pt.engine_steps()))
        pt.close()
    return out


def test_dependent_step_forms(xg):
    """the forms test_gpu_dep_plans.py expects of dep_plan.PAIR_JOBS, from the CPU handle"""
    F = xg
    for f, n, _e in _job_forms(xg, "a_pack_reads_unpacks", **NO_LOCAL_FORMS):
        assert not f[1] & F.FORM_FUSED and not f[0] & F.FORM_DEFERRED and n == 4, (f, n)
    for f, _n, _e in _job_forms(xg, "h_barrier", **NO_LOCAL_FORMS):
        assert not f[1] & F.FORM_FUSED
    for f, n, _e in _job_forms(xg, "b_local_reads_unpacks", **NO_LOCAL_FORMS):
        assert not f[1] & (F.FORM_FUSED_LOCAL | F.FORM_FUSED | F.FORM_SPLIT | F.FORM_SELF_LOCAL) and n == 4, (f, n)
    for f, n, _e in _job_forms(xg, "b_control", **NO_LOCAL_FORMS):
        assert f[1] & F.FORM_FUSED_LOCAL and f[1] & F.FORM_FUSED and f[0] & F.FORM_DEFERRED and n == 3, (f, n)
    for after_pack in (1, 0):
        for f, _n, _e in _job_forms(xg, "b_local_reads_unpacks", self_max=0, split_min=0, split_after_pack=after_pack):
            assert f[1] & F.FORM_SPLIT and f[1] & F.FORM_FUSED and not f[1] & F.FORM_FUSED_LOCAL, f
    for f, _n, _e in _job_forms(xg, "d_local_overwrites_unpacks", **NO_LOCAL_FORMS):
        assert not f[1] & (F.FORM_FUSED_LOCAL | F.FORM_FUSED)
    for f, _n, _e in _job_forms(xg, "e_war_exchange", **NO_LOCAL_FORMS):
        assert not f[1] & F.FORM_FUSED
    dep = _job_forms(xg, "f_stage_dep", fuse_stage=1, **NO_LOCAL_FORMS)
    ctl = _job_forms(xg, "f_stage_control", fuse_stage=1, **NO_LOCAL_FORMS)
    assert all(not f[0] & F.FORM_STAGE_FUSED for f, _n, _e in dep) and all(f[0] & F.FORM_STAGE_FUSED for f, _n, _e in ctl)
    assert [a[1] - b[1] for a, b in zip(dep, ctl)] == [1, 1]
    for f, _n, _e in _job_forms(xg, "b_local_reads_unpacks", self_max=1 << 30):
        assert f[1] & F.FORM_SELF_LOCAL and f[1] & F.FORM_FUSED and not f[1] & F.FORM_FUSED_LOCAL, f
    for f, _n, _e in _job_forms(xg, "i_ring", **NO_LOCAL_FORMS):
        assert not any(x & F.FORM_FUSED for x in f), f
    for f, n, e in _job_forms(xg, "k_engine_inside"):
        assert e == (3, 1, 2) and not f[0] & F.FORM_ENGINE and all(x & F.FORM_ENGINE for x in f[1:]) and n == 3, (f, n, e)


def test_dependent_step_plans_are_covered(xg):
    """the cover property over the hand-made two- and three-GPU plans (packs that forward, fused and
    deferred steps, stage copies)"""
    import dep_plan as D
    for name in D.PAIR_JOBS:
        job, _want = D.PAIR_JOBS[name]()
        for kn in (NO_LOCAL_FORMS, dict(self_max=0, split_min=0), dict(self_max=1 << 30)):
            for g in range(job.G):
                dp = job.devplan(xg, g)
                pt = xg.PlanTables(dp, rank=g, nranks=job.G, virt=1, **kn)
                try:
                    copies = [(c.src_buf, c.src_off, c.dst_buf, c.dst_off, c.len) for c in dp.copies[:dp.ncopy]]
                    steps = [(s.pre_begin, s.pre_count, 0, 0, s.post_begin, s.post_count) for s in dp.steps[:dp.nsteps]]
                    check_cover(xg, pt.records(), copies, steps, [s.stage_count for s in dp.steps[:dp.nsteps]])
                finally:
                    pt.close()


# ------------------------------------------------------------------ knobs, sanitizers
def test_default_knobs_are_the_rules_defaults(xg):
    """xg_plan_knobs_default gives the copy rules xg.CopyRules.DEFAULTS states for a 256-CU device"""
    k = xg.PlanTables.knobs()
    assert {n: getattr(k.rules, n) for n in xg.CopyRules.DEFAULTS} == xg.CopyRules.DEFAULTS
    assert (k.nranks, k.rank, k.virt, k.launch_max, k.engine_wmax, k.solo_rails) == (1, 0, 0, 512 << 20, 256, 512)


def test_plan_tables_under_sanitizers(tmp_path):
    """tests/plan_tables_san.cc (its own main) builds the tables of a handful of plans -- golden-like
    schedules on 1, 2 and 8 GPUs in every pack form, a ragged one, a placement plan, cut at several
    launch_max -- and checks the cover property in C++, then reads scripted knob environments (empty,
    very long values, digits past int, entries without '=', an empty name, every variable at once),
    compiled with plan_tables.cc and the C host sources under AddressSanitizer and UBSan and run as
    an executable"""
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
    exe = str(tmp_path / "plan_tables_san")
    subprocess.run(["g++", "-std=c++17", os.path.join(HERE, "plan_tables_san.cc"), os.path.join(host, "plan_tables.cc"),
                    "-I" + host, "-o", exe] + objs + san + inc + ["-lm"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    assert "plans covered" in out.stdout, out.stdout
    assert "knob environments: 8 read" in out.stdout, out.stdout         # its xg_plan_knobs_env section


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]))
