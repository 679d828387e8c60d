"""xg_plan_knobs_env (csrc/host/plan_tables.cc): the one place that reads the XG_* plan knobs.

Every expected value here is written out by hand from the stanzas xg_init held before the parser
moved to the host library: for each variable an accepted value, every class of value it rejects
(out of range, not in its set, non-numeric, empty) and its quirks.  A case is (entries, changes):
the environment as "NAME=value" strings and the fields that differ from xg_plan_knobs_default
afterwards; every other byte of the structure must equal the default's.  `pre` sets fields before
the call, which tells a rule that always writes its field from one that writes only when set.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

DEV = (256, 256, 2048)          # cus, co-resident engine workgroups, wave grid


def _set(k, name, v):
    setattr(k.rules if hasattr(k.rules, name) else k, name, v)


def apply_env(xg, entries, dev=DEV, pre=None):
    """-> (the knobs after xg_plan_knobs_env over `entries`, the default knobs with `pre`)"""
    h = xg.PlanTables.lib()
    k, base = xg.PlanKnobs(), xg.PlanKnobs()
    for s in (k, base):
        h.xg_plan_knobs_default(C.byref(s), *dev)
        for name, v in (pre or {}).items():
            _set(s, name, v)
    arr = [e.encode() for e in entries] + [None]
    h.xg_plan_knobs_env(C.byref(k), (C.c_char_p * len(arr))(*arr))
    return k, base


def check(xg, entries, changes, dev=DEV, pre=None):
    k, want = apply_env(xg, entries, dev, pre)
    for name, v in changes.items():
        _set(want, name, v)
    if bytes(k) != bytes(want):
        fields = [f[0] for f in xg.CopyRules._fields_] + [f[0] for f in xg.PlanKnobs._fields_[1:]]
        get = lambda s, n: getattr(s.rules if hasattr(s.rules, n) else s, n)
        diff = {n: (get(k, n), get(want, n)) for n in fields if get(k, n) != get(want, n)}
        raise AssertionError("%s dev %s pre %s: (got, want) %s" % (entries, dev, pre, diff))


def test_empty_environment_is_the_default(xg):
    h = xg.PlanTables.lib()
    for dev in (DEV, (256, 100, 1536), (0, 0, 0)):
        k = xg.PlanKnobs()
        C.memset(C.byref(k), 0xFF, C.sizeof(k))         # the default clears padding too
        h.xg_plan_knobs_default(C.byref(k), *dev)
        want = bytes(k)
        h.xg_plan_knobs_env(C.byref(k), (C.c_char_p * 1)(None))
        assert bytes(k) == want
    k = xg.PlanTables.knobs()
    assert bytes(k) == bytes(xg.PlanTables.knobs(env={})) and C.sizeof(k) == 184


# ------------------------------------------------------------------ one variable at a time
NOT_NUMBERS = ["abc", ""]

# off only for the exact string "0"; written whether set or not
OFF_IF_0 = dict(XG_ENGINE_SOLO="solo", XG_STEP_CHAIN="step_chain", XG_FUSE_STAGE="fuse_stage",
                XG_SPLIT_AFTER_PACK="split_after_pack")
# on only for the exact string "1"; written whether set or not
ON_IF_1 = dict(XG_ENGINE_DRAIN="engine_drain", XG_ENGINE_ARM="engine_arm")
# a set variable always writes atoi != 0
FLAGS = dict(XG_EXTENT_COPY="extent_copy", XG_SMALL_PIECES="small_pieces")
# any number as atol / atoll reads it
NUMBERS = dict(XG_ENGINE_MAX_STEP="engine_max_step", XG_ENGINE_SOLO_MAX="solo_max", XG_COPY_LAUNCH_MAX="launch_max",
               XG_COPY_WAVE_MIN="wave_min", XG_SPLIT_MIN="split_min", XG_SELF_MAX="self_max")


@pytest.mark.parametrize("name", list(OFF_IF_0))
def test_off_only_for_the_string_0(xg, name):
    f = OFF_IF_0[name]
    check(xg, [name + "=0"], {f: 0})
    for v in ["1", "00", " 0", "0 ", "0x", "-0", "2"] + NOT_NUMBERS:
        check(xg, ["%s=%s" % (name, v)], {})
        check(xg, ["%s=%s" % (name, v)], {f: 1}, pre={f: 0})
    check(xg, [], {f: 1}, pre={f: 0})                   # unset: written all the same


@pytest.mark.parametrize("name", list(ON_IF_1))
def test_on_only_for_the_string_1(xg, name):
    f = ON_IF_1[name]
    check(xg, [name + "=1"], {f: 1})
    for v in ["0", "01", " 1", "1 ", "1x", "+1", "2"] + NOT_NUMBERS:
        check(xg, ["%s=%s" % (name, v)], {})
        check(xg, ["%s=%s" % (name, v)], {f: 0}, pre={f: 1})
    check(xg, [], {f: 0}, pre={f: 1})


@pytest.mark.parametrize("name", list(FLAGS))
def test_a_set_flag_always_writes(xg, name):
    f = FLAGS[name]
    for v in ["0", "00"] + NOT_NUMBERS:
        check(xg, ["%s=%s" % (name, v)], {f: 0})
    for v in ["1", "5", "-1", "1x"]:
        check(xg, ["%s=%s" % (name, v)], {})
        check(xg, ["%s=%s" % (name, v)], {f: 1}, pre={f: 7})
    check(xg, [], {}, pre={f: 7})                       # unset: left alone


@pytest.mark.parametrize("name", list(NUMBERS))
def test_any_number(xg, name):
    f = NUMBERS[name]
    for v, want in (("0", 0), ("4096", 4096), ("-5", -5), ("99999999999", 99999999999), ("12x", 12), (" 7", 7),
                    ("abc", 0), ("", 0)):
        check(xg, ["%s=%s" % (name, v)], {f: want})
    check(xg, [], {}, pre={f: 77})


def test_copy_variant(xg):
    for v, want in (("1", 1), ("6", 6), ("1x", 1), ("6 ", 6)):
        check(xg, ["XG_COPY_VARIANT=" + v], {"variant": want})
    for v in ["0", "2", "7", "-1", "16"] + NOT_NUMBERS:         # 2, 7, -1, 16 with a message (test_messages)
        check(xg, ["XG_COPY_VARIANT=" + v], {})
        check(xg, ["XG_COPY_VARIANT=" + v], {}, pre={"variant": 6})


def test_ragged_copy_is_off_for_whatever_reads_as_zero(xg):
    for v in ["0", "00", "x1"] + NOT_NUMBERS:
        check(xg, ["XG_RAGGED_COPY=" + v], {"ragged_copy": 0})
    for v in ["1", "2", "-1", "1x"]:
        check(xg, ["XG_RAGGED_COPY=" + v], {})
        check(xg, ["XG_RAGGED_COPY=" + v], {}, pre={"ragged_copy": 0})     # never switched on


def test_extent_knobs(xg):
    for v, want in (("1", 1), ("4096", 4096), ("99999999999", 99999999999)):
        check(xg, ["XG_EXTENT_MEAN_MAX=" + v], {"extent_mean_max": want})
    for v in ["0", "-1"] + NOT_NUMBERS:
        check(xg, ["XG_EXTENT_MEAN_MAX=" + v], {})
    for v, want in (("1", 1 << 10), ("16", 16 << 10), ("1024", 1 << 20)):           # stored as bytes
        check(xg, ["XG_EXTENT_TILE_KIB=" + v], {"extent_tile": want})
    for v in ["0", "1025", "65536", "-1"] + NOT_NUMBERS:
        check(xg, ["XG_EXTENT_TILE_KIB=" + v], {})


def test_small_piece_knobs(xg):
    for v, want in (("0", 0), ("4096", 4096), ("99999999999", 99999999999), ("abc", 0), ("", 0)):
        check(xg, ["XG_SMALL_PIECE_MIN=" + v], {"small_piece_min": want})
    check(xg, ["XG_SMALL_PIECE_MIN=-1"], {})
    check(xg, ["XG_SMALL_PIECE_KIB=4"], {"small_kib": 4})
    check(xg, ["XG_SMALL_PIECE_KIB=8"], {"small_kib": 8}, pre={"small_kib": 4})
    for v in ["0", "2", "6", "16", "-4"] + NOT_NUMBERS:
        check(xg, ["XG_SMALL_PIECE_KIB=" + v], {})
    for v, want in (("1", 1), ("3", 3), ("1024", 1024)):
        check(xg, ["XG_SMALL_PIECE_ORDER=" + v], {"small_order": want})
    for v in ["0", "1025", "-1"] + NOT_NUMBERS:
        check(xg, ["XG_SMALL_PIECE_ORDER=" + v], {})


def test_engine_max_step_takes_negative_numbers(xg):
    check(xg, ["XG_ENGINE_MAX_STEP=-1"], {"engine_max_step": -1})


def test_wave_kib_is_written_even_when_unset(xg):
    for v in ("2", "4", "8"):
        check(xg, ["XG_WAVE_KIB=" + v], {"wave_kib": int(v)})
    for v in ["0", "1", "3", "6", "16", "-2"] + NOT_NUMBERS:
        check(xg, ["XG_WAVE_KIB=" + v], {"wave_kib": 0}, pre={"wave_kib": 4})
    check(xg, [], {"wave_kib": 0}, pre={"wave_kib": 4})


# ------------------------------------------------------------------ waves and rails, the caps
def test_solo_waves_and_rails(xg):
    check(xg, ["XG_SOLO_WAVES=16"], {"solo_waves": 16, "solo_rails": 16})
    check(xg, ["XG_SOLO_WAVES=16x"], {"solo_waves": 16, "solo_rails": 16})
    for v in ["8", "1", "0", "160", "-16"] + NOT_NUMBERS:
        check(xg, ["XG_SOLO_WAVES=" + v], {})
        check(xg, ["XG_SOLO_WAVES=" + v], {"solo_waves": 1, "solo_rails": 512}, pre={"solo_waves": 16, "solo_rails": 5})
    check(xg, [], {"solo_waves": 1, "solo_rails": 512}, pre={"solo_waves": 16, "solo_rails": 5})
    for v, want in (("1", 1), ("4", 4), ("512", 512), ("513", 512), ("100000", 512)):
        check(xg, ["XG_SOLO_RAILS=" + v], {"solo_rails": want})
    for v in ["0", "-1"] + NOT_NUMBERS:
        check(xg, ["XG_SOLO_RAILS=" + v], {})
        check(xg, ["XG_SOLO_WAVES=16", "XG_SOLO_RAILS=" + v], {"solo_waves": 16, "solo_rails": 16})
    # the rails' default follows the waves before XG_SOLO_RAILS applies, in whatever order they are listed
    for entries in (["XG_SOLO_WAVES=16", "XG_SOLO_RAILS=4"], ["XG_SOLO_RAILS=4", "XG_SOLO_WAVES=16"]):
        check(xg, entries, {"solo_waves": 16, "solo_rails": 4})
    check(xg, ["XG_SOLO_WAVES=16", "XG_SOLO_RAILS=100000"], {"solo_waves": 16, "solo_rails": 512})
    check(xg, ["XG_SOLO_WAVES=8", "XG_SOLO_RAILS=4"], {"solo_rails": 4})
    check(xg, ["XG_SOLO_WAVES=8"], {})                                              # 1 wave, 512 rails


@pytest.mark.parametrize("name,field,slot", [("XG_ENGINE_WG", "engine_wmax", 1), ("XG_WAVE_GRID", "wave_grid", 2)])
def test_caps_only_lower(xg, name, field, slot):
    cur = DEV[slot]
    for v, want in (("1", 1), ("8", 8), (str(cur - 1), cur - 1), (str(cur), cur), (str(cur + 1), cur), ("65536", cur)):
        check(xg, ["%s=%s" % (name, v)], {field: want})
    for v in ["0", "-1", "-8"] + NOT_NUMBERS:
        check(xg, ["%s=%s" % (name, v)], {})


def test_engine_cap_on_a_device_that_admits_fewer_workgroups_than_cus(xg):
    dev = (256, 100, 1536)                      # the default is then min(cus, engine_occ) = 100
    assert apply_env(xg, [], dev)[0].engine_wmax == 100
    check(xg, ["XG_ENGINE_WG=50"], {"engine_wmax": 50}, dev=dev)
    check(xg, ["XG_ENGINE_WG=200"], {"engine_wmax": 100}, dev=dev)
    check(xg, ["XG_ENGINE_WG=256"], {"engine_wmax": 100}, dev=dev)
    check(xg, ["XG_WAVE_GRID=1535"], {"wave_grid": 1535}, dev=dev)
    check(xg, ["XG_WAVE_GRID=2048"], {"wave_grid": 1536}, dev=dev)
    # a current value below 1 (no such device; the stanza's max(1, ...)) comes out as 1
    check(xg, ["XG_WAVE_GRID=5"], {"wave_grid": 1}, dev=(256, 256, 0))


# ------------------------------------------------------------------ the array
def test_first_match_wins_and_strays_are_ignored(xg):
    check(xg, ["XG_SELF_MAX=1", "XG_SELF_MAX=2"], {"self_max": 1})
    check(xg, ["XG_ENGINE_SOLO=1", "XG_ENGINE_SOLO=0"], {})
    check(xg, ["XG_SELF_MAX", "XG_SELF_MAX=3"], {"self_max": 3})                   # an entry without '='
    check(xg, ["XG_SELF_MAXIMUM=4", "XXG_SELF_MAX=4", "=5", "", "XG_SELF_MA=6", "xg_self_max=7"], {})
    check(xg, ["XG_NO_SUCH_KNOB=1", "XG_GRAPH=1", "XG_SELF_COMM=1", "XG_SHARE_GPU=1", "RANK=3"], {})
    check(xg, ["XG_SELF_MAX=8=9"], {"self_max": 8})


def test_every_variable_at_once(xg):
    entries = ["XG_COPY_VARIANT=6", "XG_RAGGED_COPY=0", "XG_EXTENT_COPY=0", "XG_EXTENT_MEAN_MAX=2048",
               "XG_EXTENT_TILE_KIB=64", "XG_SMALL_PIECES=0", "XG_SMALL_PIECE_MIN=4096", "XG_SMALL_PIECE_KIB=4",
               "XG_SMALL_PIECE_ORDER=3", "XG_ENGINE_MAX_STEP=32768", "XG_ENGINE_WG=8", "XG_ENGINE_DRAIN=1",
               "XG_ENGINE_SOLO=0", "XG_ENGINE_SOLO_MAX=1048576", "XG_SOLO_WAVES=16", "XG_SOLO_RAILS=7",
               "XG_COPY_LAUNCH_MAX=65536", "XG_COPY_WAVE_MIN=0", "XG_WAVE_GRID=64", "XG_WAVE_KIB=2", "XG_STEP_CHAIN=0",
               "XG_ENGINE_ARM=1", "XG_SPLIT_MIN=123", "XG_SELF_MAX=456", "XG_FUSE_STAGE=0", "XG_SPLIT_AFTER_PACK=0"]
    want = dict(variant=6, ragged_copy=0, extent_copy=0, extent_mean_max=2048, extent_tile=65536, small_pieces=0,
                small_piece_min=4096, small_kib=4, small_order=3, engine_max_step=32768, engine_wmax=8, engine_drain=1,
                solo=0, solo_max=1 << 20, solo_waves=16, solo_rails=7, launch_max=65536, wave_min=0, wave_grid=64,
                wave_kib=2, step_chain=0, engine_arm=1, split_min=123, self_max=456, fuse_stage=0, split_after_pack=0)
    assert sorted(e.split("=")[0] for e in entries) == sorted(xg.PlanTables.knob_names())
    check(xg, entries, want)
    check(xg, entries[::-1], want)


def test_names(xg):
    names = xg.PlanTables.knob_names()
    assert len(names) == len(set(names)) == 26
    assert set(names) == set(OFF_IF_0) | set(ON_IF_1) | set(FLAGS) | set(NUMBERS) | {
        "XG_COPY_VARIANT", "XG_RAGGED_COPY", "XG_EXTENT_MEAN_MAX", "XG_EXTENT_TILE_KIB", "XG_SMALL_PIECE_MIN",
        "XG_SMALL_PIECE_KIB", "XG_SMALL_PIECE_ORDER", "XG_ENGINE_WG", "XG_SOLO_WAVES", "XG_SOLO_RAILS", "XG_WAVE_GRID",
        "XG_WAVE_KIB"}
    h = xg.PlanTables.lib()
    out = (C.c_char_p * 3)()
    assert h.xg_plan_knob_names(out, 2) == 26 and [out[0], out[1], out[2]] == [names[0].encode(), names[1].encode(), None]
    # DESIGN.md section 10 lists every one
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    sec = text[text.index("## 10. Knobs"):text.index("## 11.")]
    listed = set(re.findall(r"`(XG_[A-Z_]+)`", sec))
    assert not set(names) - listed, sorted(set(names) - listed)
    assert "xg_plan_knobs_env" in sec


def test_python_env_argument(xg):
    """xg.PlanTables.knobs(env=): values through str, explicit fields after it, XG_GRAPH passes, a
    name that is no plan knob raises, the process environment is neither read nor written"""
    before = dict(os.environ)
    k = xg.PlanTables.knobs(env=dict(XG_SOLO_WAVES=16, XG_ENGINE_WG=300, XG_GRAPH=1, XG_SELF_MAX="77"), solo_rails=3,
                            wave_min=5)
    assert (k.solo_waves, k.solo_rails, k.engine_wmax, k.self_max, k.rules.wave_min) == (16, 3, 256, 77, 5)
    assert xg.PlanTables.knobs(100, 50, 64, env=dict(XG_ENGINE_WG=60, XG_WAVE_GRID=70)).engine_wmax == 50
    for bad in ("XG_SOLO_WAVE", "XG_SELF_COMM", "XG_COPY_CHUNK", "HOME"):
        with pytest.raises(xg.XGError):
            xg.PlanTables.knobs(env={bad: 1})
    assert dict(os.environ) == before


# ------------------------------------------------------------------ the process environment, the messages
CHILD = """
import ctypes as C, sys
sys.path.insert(0, %r)
import __graft_entry__ as G
xg = G.load_package().xg
h = xg.PlanTables.lib()
def run(arr):
    k = xg.PlanKnobs()
    h.xg_plan_knobs_default(C.byref(k), 256, 256, 2048)
    h.xg_plan_knobs_env(C.byref(k), arr)
    return k
"""


def _child(code, env):
    for name in env:
        assert name not in os.environ, name
    out = subprocess.run([sys.executable, "-c", CHILD % REPO + code], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, **env))
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def test_null_reads_the_process_environment():
    out = _child("k = run(None)\nprint(k.engine_max_step, k.solo_waves, k.solo_rails, k.variant)\n"
                 "k = run((C.c_char_p * 1)(None))\nprint(k.engine_max_step, k.solo_waves, k.solo_rails)\n",
                 dict(XG_ENGINE_MAX_STEP="12345", XG_SOLO_WAVES="16", XG_COPY_VARIANT="3", XG_COPY_WAVE="1"))
    assert out.stdout.split("\n")[:2] == ["12345 16 16 0", "%d 1 512" % (16 << 20)]
    assert out.stderr == ("xg: XG_COPY_WAVE is set but no longer read (folded into a constant or an option)\n"
                          "xg: XG_COPY_VARIANT=3 ignored (0, 1 or 6)\n")


def test_messages():
    """the two texts, verbatim; the retired-knob warning once per process, in the list's order"""
    out = _child("arr = (C.c_char_p * 5)(b'XG_COPY_VARIANT=-1', b'XG_PACK_FORM=2', b'XG_COPY_CHUNK=65536', b'XG_ENGINE_WG=4', None)\n"
                 "run(arr)\nrun(arr)\nrun((C.c_char_p * 2)(b'XG_COPY_VARIANT=abc', None))\n", {})
    fold = "xg: %s is set but no longer read (folded into a constant or an option)\n"
    bad = "xg: XG_COPY_VARIANT=-1 ignored (0, 1 or 6)\n"
    assert out.stderr == fold % "XG_COPY_CHUNK" + fold % "XG_PACK_FORM" + bad + bad
