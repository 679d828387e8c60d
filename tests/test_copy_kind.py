"""xg_copy_launch_choose (csrc/host/pieces.c): the ONE kernel kind of a copy launch -- PIECE, WAVE,
SHIFT, EXTENT or SMALL --, its non-temporal flag, piece KiB, piece order and piece size, from the
launch's facts (gathered by xg_launch_facts_add as plan load gathers them) and the context's knobs.
No device: the rule is plain C in libxghost.

Two checks: a decision table, one row per line of the precedence and per boundary, and a
differential test against `_flag_rule`, a restatement of the clauses TableBuilder::open had when
the kernel was five overlapping flags (kib, nt, shift, ext, q) read back by launch_one in another
order -- which also shows that those flags excluded each other."""
import random

K, M = 1 << 10, 1 << 20
INT32_MAX = (1 << 31) - 1
S, R, SS, SR = 0, 1, 2, 3            # XG_BUF_SEND, RECV, STAGE_SEND, STAGE_RECV


def _copies(lens, src_phase=0, dst_phase=0, src_buf=S, dst_buf=R):
    """copies of these lengths, back to back on the 16-B grid (plus the phases) in both regions"""
    out, off = [], 0
    for n in lens:
        out.append((src_buf, off + src_phase, dst_buf, off + dst_phase, n))
        off += (max(n, 0) + 15) // 16 * 16 + 16
    return out


def _choose(xg, copies, flags=0, cross=False, may_small=False, nt_cut=False, nt_run=False, **rules):
    return xg.copy_launch_choose(xg.launch_facts(copies, flags, cross, may_small, nt_cut, nt_run), **rules)


def _piece(xg, copies, **rules):
    r = dict(xg.CopyRules.DEFAULTS, **rules)
    return xg.piece_size([c[4] for c in copies], r["chunk"], r["cus"], r["wg_cost"])


# ------------------------------------------------------------------ the facts
def test_facts_are_gathered_over_the_positive_copies(xg):
    f = xg.launch_facts([(S, 16, R, 32, 4096), (S, 0, R, 0, 0), (S, 8192, R, 8200, 4096), (S, 5, R, 5, -3)])
    assert (f.bytes, f.npos, f.bits & 15, f.uniform_len, f.nlens) == (8192, 2, 8, 4096, 4)
    assert xg.launch_facts([(S, 0, R, 0, 4096), (S, 4096, R, 4096, 4112)]).uniform_len == -1
    assert xg.launch_facts([(S, 0, R, 0, 4096), (S, 4096, R, 4096, 4112), (S, 0, R, 0, 4112)]).uniform_len == -1
    assert xg.launch_facts([(S, 0, SS, 0, 4096), (S, 4096, SS, 4096, 4096)]).uniform_len == -1      # packs
    assert xg.launch_facts([(SR, 0, R, 0, 4096)]).uniform_len == -1                                 # an unpack
    assert xg.launch_facts([(SS, 0, SR, 0, 4096)]).uniform_len == 4096     # staging on the other side: a plain copy
    f = xg.launch_facts([(S, 0, R, 0, 0)])
    assert (f.bytes, f.npos, f.uniform_len) == (0, 0, 0) and xg.copy_launch_choose(f) is None


# ------------------------------------------------------------------ the decision table
def test_wave_range(xg):
    """bytes = wave_min - 1, wave_min, wave_max, wave_max + 1 (the rule moves, the launch stays)"""
    c = _copies([64 * K] * 16)                                              # 1 MiB, aligned
    P, W = (xg.COPY_PIECE, 0, 0, 0, _piece(xg, c)), (xg.COPY_WAVE, 0, 2, 0, 2 * K)
    assert _choose(xg, c, cross=True, wave_min=M + 1) == P
    assert _choose(xg, c, cross=True, wave_min=M) == W
    assert _choose(xg, c, cross=True, wave_min=0, wave_max=M) == W
    assert _choose(xg, c, cross=True, wave_min=0, wave_max=M - 1) == P
    assert _choose(xg, c, cross=False, wave_min=M) == P                       # not a cross launch
    assert _choose(xg, c, cross=True, nt_cut=True, nt_run=True) == (xg.COPY_PIECE, 1, 0, 0, _piece(xg, c))
    assert _choose(xg, _copies([64 * K] * 16, dst_phase=8), cross=True)[0] == xg.COPY_PIECE   # off the grid


def test_wave_piece_kib(xg):
    """cus = 256: 8 KiB pieces from 8 MiB, 4 KiB from 4 MiB, 2 KiB below; XG_WAVE_KIB forces one"""
    for nbytes, kib in ((8 * M, 8), (8 * M - 16, 4), (4 * M, 4), (4 * M - 16, 2), (M, 2), (32 * M, 8)):
        assert _choose(xg, _copies([nbytes]), cross=True, cus=256) == (xg.COPY_WAVE, 0, kib, 0, kib * K), nbytes
    assert _choose(xg, _copies([4 * M]), cross=True, cus=64)[2] == 8
    for forced in (2, 4, 8):
        assert _choose(xg, _copies([8 * M]), cross=True, wave_kib=forced) == (xg.COPY_WAVE, 0, forced, 0, forced * K)


def test_cut_plain_run_non_temporal(xg):
    """inside the wave range, the cut plain and the run non-temporal: PIECE, nt, over wave-sized
    pieces -- and SMALL once small_piece_min is below it and the copies are uniform"""
    c = _copies([256 * K] * 16)                                             # 4 MiB
    assert _choose(xg, c, cross=True, may_small=True, nt_run=True) == (xg.COPY_PIECE, 1, 0, 0, 4 * K)
    assert _choose(xg, c, cross=True, may_small=True, nt_run=True, small_piece_min=4 * M) == (xg.COPY_SMALL, 1, 8, 8, 8 * K)
    c = _copies([256 * K] * 15 + [256 * K + 16])
    assert _choose(xg, c, cross=True, may_small=True, nt_run=True, small_piece_min=0) == (xg.COPY_PIECE, 1, 0, 0, 4 * K)
    # a plain run of the same launch is WAVE, which SMALL never replaces
    assert _choose(xg, _copies([256 * K] * 16), cross=True, may_small=True, small_piece_min=0) == (xg.COPY_WAVE, 0, 4, 0, 4 * K)


def test_extent_threshold_and_flags(xg):
    """bytes = npos * extent_mean_max and one more; both flags with extent_copy 1 and 0: EXTENT,
    else SHIFT; EXTENT comes before WAVE and is never SMALL"""
    both = xg.DP_RAGGED | xg.DP_EXTENTS
    at = _copies([1024] * 9 + [0, 1024], src_phase=3)
    over = _copies([1024] * 9 + [0, 1025], src_phase=3)
    assert _choose(xg, at, both) == (xg.COPY_EXTENT, 0, 0, 0, _piece(xg, at))
    assert _choose(xg, over, both) == (xg.COPY_SHIFT, 0, 0, 0, _piece(xg, over))
    assert _choose(xg, at, both, extent_copy=0) == (xg.COPY_SHIFT, 0, 0, 0, _piece(xg, at))
    assert _choose(xg, at, both, nt_run=True, nt_cut=True)[:2] == (xg.COPY_EXTENT, 1)
    assert _choose(xg, at, xg.DP_RAGGED)[0] == xg.COPY_SHIFT                  # no placement plan
    assert _choose(xg, at, both, extent_mean_max=1023)[0] == xg.COPY_SHIFT
    assert _choose(xg, at, both, chunk=(1 << 24) + 16)[0] == xg.COPY_SHIFT    # chunk past the tile indices
    assert _choose(xg, at, both, chunk=1 << 24)[0] == xg.COPY_EXTENT
    short = _copies([1024] * 1024)                                            # 1 MiB of short aligned copies
    assert _choose(xg, short, both, cross=True, may_small=True, small_piece_min=0)[0] == xg.COPY_EXTENT
    assert _choose(xg, short, xg.DP_RAGGED, cross=True)[0] == xg.COPY_WAVE


def test_shift_needs_the_flag_the_knob_and_a_misaligned_bit(xg):
    for copies in (_copies([4096, 4097]), _copies([4096] * 2, src_phase=1), _copies([4096] * 2, dst_phase=15)):
        assert _choose(xg, copies, xg.DP_RAGGED) == (xg.COPY_SHIFT, 0, 0, 0, _piece(xg, copies))
        assert _choose(xg, copies, xg.DP_RAGGED, nt_cut=True, nt_run=True)[:2] == (xg.COPY_SHIFT, 1)
        assert _choose(xg, copies, 0)[0] == xg.COPY_PIECE                     # without XG_DP_RAGGED
        assert _choose(xg, copies, xg.DP_RAGGED, ragged_copy=0)[0] == xg.COPY_PIECE
        assert _choose(xg, copies, xg.DP_RAGGED, may_small=True, small_piece_min=0)[0] == xg.COPY_SHIFT
    assert _choose(xg, _copies([4096, 8192]), xg.DP_RAGGED)[0] == xg.COPY_PIECE   # all on the grid


def test_small_replaces_piece_only(xg):
    c = _copies([M] * 7)
    nbytes = 7 * M
    assert _choose(xg, c, may_small=True, small_piece_min=nbytes) == (xg.COPY_SMALL, 0, 8, 8, 8 * K)
    assert _choose(xg, c, may_small=True, small_piece_min=nbytes + 1) == (xg.COPY_PIECE, 0, 0, 0, _piece(xg, c))
    assert _choose(xg, c, may_small=True, nt_cut=True, nt_run=True, small_piece_min=0, small_kib=4, small_order=1) == \
        (xg.COPY_SMALL, 1, 4, 1, 4 * K)
    assert _choose(xg, c, may_small=False, small_piece_min=0)[0] == xg.COPY_PIECE
    assert _choose(xg, c, may_small=True, small_piece_min=0, small_pieces=0)[0] == xg.COPY_PIECE
    assert _choose(xg, c, may_small=True)[0] == xg.COPY_PIECE                 # below the default 112 MiB
    assert _choose(xg, _copies([M] * 112), may_small=True) == (xg.COPY_SMALL, 0, 8, 8, 8 * K)
    # non-uniform, off the grid, or touching staging: no SMALL
    assert _choose(xg, _copies([M] * 6 + [M + 16]), may_small=True, small_piece_min=0)[0] == xg.COPY_PIECE
    assert _choose(xg, _copies([M] * 7, src_phase=8, dst_phase=8), may_small=True, small_piece_min=0)[0] == xg.COPY_PIECE
    assert _choose(xg, _copies([M] * 7, dst_buf=SS), may_small=True, small_piece_min=0)[0] == xg.COPY_PIECE
    assert _choose(xg, _copies([M] * 6) + [(SR, 0, R, 1 << 30, M)], may_small=True, small_piece_min=0)[0] == xg.COPY_PIECE
    assert _choose(xg, _copies([M, 0] * 7), may_small=True, small_piece_min=0)[0] == xg.COPY_SMALL   # empty copies aside


def test_small_index_guards(xg):
    """npos * ppc and small_order * ppc stay within INT32_MAX (xg_small_index works in 32 bits)"""
    ppc = 1 << 22
    n = 8 * K * ppc                                                           # 32 GiB copies
    assert _choose(xg, _copies([n] * 511), may_small=True, small_order=1)[0] == xg.COPY_SMALL        # 511 * 2^22 < 2^31
    assert _choose(xg, _copies([n] * 512), may_small=True, small_order=1)[0] == xg.COPY_PIECE        # = 2^31
    assert _choose(xg, _copies([n - 8 * K] * 512), may_small=True, small_order=1)[0] == xg.COPY_SMALL
    assert _choose(xg, _copies([n]), may_small=True, small_order=511)[0] == xg.COPY_SMALL
    assert _choose(xg, _copies([n]), may_small=True, small_order=512)[0] == xg.COPY_PIECE
    assert _choose(xg, _copies([n]), may_small=True, small_order=1024, small_kib=4)[0] == xg.COPY_PIECE


# ------------------------------------------------------------------ the differential test
def _wave_kib_for(nbytes, cus):
    for kib in (8, 4):
        if nbytes // (kib << 10) >= 4 * cus:
            return kib
    return 2


def _flag_rule(xg, copies, flags, cross, may_small, v_cut, v_run, r, note):
    """TableBuilder::open as it was with one flag per kernel, clause by clause (v_cut, v_run:
    copy_variant's 1 or 6 for the cut and for the run), then launch_one's order of reading the
    flags back -> (kind, nt, kib, order, piece), or None for a launch without bytes; note["wave_cut"]:
    the pieces were cut to the wave size"""
    bits, nbytes, lens = 0, 0, []
    for _sb, so, _db, do, n in copies:
        lens.append(n)
        if n <= 0:
            continue
        nbytes += n
        bits |= so | do | n
    if nbytes <= 0:
        return None
    nt = v_run == 6
    stamps = v_run in (1, 6)
    shift = bool(flags & xg.DP_RAGGED) and bool(r["ragged_copy"]) and (bits & 15) != 0
    npos = sum(n > 0 for n in lens)
    ext = (bool(flags & xg.DP_EXTENTS) and bool(r["extent_copy"]) and stamps and r["chunk"] <= (1 << 24)
           and nbytes <= npos * r["extent_mean_max"])
    if ext:
        shift = False
    kib = 0
    if not ext and cross and r["wave_min"] <= nbytes <= r["wave_max"] and (bits & 15) == 0 and v_cut == 1:
        k = r["wave_kib"] or _wave_kib_for(nbytes, r["cus"])
        chunk = k << 10
        note["wave_cut"] = True
        if v_run == 1:
            kib = k
    else:
        chunk = xg.piece_size(lens, r["chunk"], r["cus"], r["wg_cost"])
    q = 0
    if not (not may_small or not r["small_pieces"] or ext or shift or kib or not stamps or (bits & 15) != 0
            or nbytes < r["small_piece_min"]):
        length, uniform = 0, True
        for sb, _so, db, _do, n in copies:
            if n <= 0:
                continue
            uniform = uniform and (length == 0 or n == length) and db != SS and sb != SR
            length = n
        piece = r["small_kib"] << 10
        ppc = (length + piece - 1) // piece
        if uniform and npos * ppc <= INT32_MAX and r["small_order"] * ppc <= INT32_MAX:
            q = r["small_kib"] // 4
    assert (q != 0) + (kib != 0) + ext + shift <= 1, "two kernels flagged for one launch"
    if q:
        return xg.COPY_SMALL, int(nt), 4 * q, r["small_order"], r["small_kib"] << 10
    kind = xg.COPY_WAVE if kib else xg.COPY_EXTENT if ext else xg.COPY_SHIFT if shift else xg.COPY_PIECE
    return kind, int(nt), kib, 0, chunk


def _random_case(rng):
    r = dict(chunk=rng.choice([32768, 32784, 16384, 65536, (1 << 24) + 16]), cus=rng.choice([1, 64, 256, 304]),
             wave_min=rng.choice([0, 64 * K, M]), wave_max=rng.choice([256 * K, 4 * M, 32 * M]),
             wave_kib=rng.choice([0, 0, 2, 4, 8]), wg_cost=rng.choice([0, 2048]), ragged_copy=rng.randint(0, 3) > 0,
             extent_copy=rng.randint(0, 3) > 0, extent_mean_max=rng.choice([256, 1024, 4096]),
             small_pieces=rng.randint(0, 3) > 0, small_piece_min=rng.choice([0, 64 * K, M, 112 * M]),
             small_kib=rng.choice([4, 8]), small_order=rng.choice([1, 8, 32, 1024]))
    n = rng.choice([1, 2, 7, 40])
    base = rng.choice([16, 256, 1024, 4096, 8 * K + 16, 64 * K, 256 * K, M])
    how = rng.choice(["uniform", "uniform", "mixed", "short"])
    lens = [base if how == "uniform" else rng.choice([base, base, base + 16, 1024, 1025, 16, 4097]) if how == "mixed"
            else rng.randint(1, 2048) // rng.choice([1, 16]) * rng.choice([1, 16]) for _ in range(n)]
    lens = [0 if rng.random() < 0.05 else x for x in lens]
    phase = rng.choice([0, 0, 0, 8, 1])
    copies = _copies(lens, src_phase=phase, dst_phase=rng.choice([0, phase]))
    if rng.random() < 0.15:
        i = rng.randrange(n)
        sb, so, db, do, ln = copies[i]
        copies[i] = (SR, so, db, do, ln) if rng.random() < 0.5 else (sb, so, SS, do, ln)
    flags = rng.choice([0, 0, xg_flags[0], xg_flags[0] | xg_flags[1], xg_flags[1]])
    return copies, flags, rng.random() < 0.6, rng.random() < 0.7, rng.choice([1, 1, 6]), rng.choice([1, 1, 6]), r


xg_flags = (1, 2)       # XG_DP_RAGGED, XG_DP_EXTENTS


def test_the_flag_rule_and_the_function_agree(xg):
    assert (xg.DP_RAGGED, xg.DP_EXTENTS) == xg_flags
    rng = random.Random(20)
    seen = {}
    for _ in range(4000):
        copies, flags, cross, may_small, v_cut, v_run, r = _random_case(rng)
        note = {}
        want = _flag_rule(xg, copies, flags, cross, may_small, v_cut, v_run, r, note)
        got = _choose(xg, copies, flags, cross, may_small, v_cut == 6, v_run == 6, **r)
        assert got == want, (copies, flags, cross, may_small, v_cut, v_run, r)
        if want:
            key = (want[0], want[1], "wave_cut" in note)
            seen[key] = seen.get(key, 0) + 1
    # every kind, plain and non-temporal (WAVE plain only), and PIECE-nt over wave-sized pieces
    for kind in (xg.COPY_PIECE, xg.COPY_SHIFT, xg.COPY_EXTENT, xg.COPY_SMALL):
        for nt in (0, 1):
            assert sum(v for k, v in seen.items() if k[:2] == (kind, nt)) >= 20, (kind, nt, seen)
    assert sum(v for k, v in seen.items() if k[0] == xg.COPY_WAVE) >= 100 and not any(k[:2] == (xg.COPY_WAVE, 1) for k in seen)
    assert sum(v for k, v in seen.items() if k == (xg.COPY_PIECE, 1, True)) >= 10, seen


# ------------------------------------------------------------------ under sanitizers
def test_copy_kind_under_sanitizers(tmp_path):
    """tests/copy_kind_san.c with pieces.c as one standalone executable under ASan + UBSan (leaks
    on), CPU only, nothing preloaded: the table cases of xg_copy_launch_choose and
    xg_step_local_meets_unpacks and seeded random launches"""
    import os
    import shutil
    import subprocess

    import pytest

    from conftest import REPO
    if not shutil.which("gcc"):
        pytest.skip("gcc not found")
    exe = str(tmp_path / "copy_kind_san")
    host = os.path.join(REPO, "mpi-asynchronous-communication-test_amd", "csrc", "host")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c99",
                    "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"),
                    "-o", exe, os.path.join(REPO, "tests", "copy_kind_san.c"), os.path.join(host, "pieces.c")],
                   check=True)
    p = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ok after 2000 launches" in p.stdout, p.stdout
