"""A context's plan knobs are what the host parser gives for its device and its environment.

xg_init queries the device (compute units, co-resident engine workgroups, the wave grid), fills the
defaults and applies the environment through xg_plan_knobs_env; xg.PlanTables.knobs(env=) does the
same with no GPU.  For one environment per rule family, the waves and rails pair and each cap below
and above the device's value, every field of Context.knobs() (xg_ctx_knobs) equals the host's.  No
kernel runs.
"""
import pytest

from synth_plan import _ctx_env

pytestmark = pytest.mark.gpu


def _fields(xg, k):
    out = {f[0]: getattr(k.rules, f[0]) for f in xg.CopyRules._fields_}
    out.update({f[0]: getattr(k, f[0]) for f in xg.PlanKnobs._fields_[1:]})
    return out


@pytest.fixture(scope="module")
def facts(xg):
    """(cus, engine_wmax, wave_grid) of a context under an empty environment: with no XG_ENGINE_WG
    engine_wmax is min(cus, co-resident workgroups), which as engine_occ gives itself again"""
    cx = _ctx_env(xg)
    try:
        k = cx.knobs()
        assert k.rules.cus == cx.info()[1] and 1 <= k.engine_wmax <= k.rules.cus and k.wave_grid >= k.rules.cus
        return k.rules.cus, k.engine_wmax, k.wave_grid
    finally:
        cx.close()


def _envs(wmax, grid):
    return [
        {},
        dict(XG_ENGINE_SOLO=0, XG_STEP_CHAIN=0, XG_ENGINE_ARM=1, XG_ENGINE_DRAIN=1),         # exact "0" / exact "1"
        dict(XG_ENGINE_SOLO="00", XG_FUSE_STAGE="", XG_ENGINE_ARM="01", XG_RAGGED_COPY="abc"),
        dict(XG_EXTENT_COPY=0, XG_SMALL_PIECES=5, XG_COPY_VARIANT=6, XG_WAVE_KIB=4),         # flags and sets
        dict(XG_ENGINE_MAX_STEP=-1, XG_SELF_MAX=0, XG_SPLIT_MIN=12345, XG_COPY_LAUNCH_MAX=65536, XG_COPY_WAVE_MIN=0,
             XG_SMALL_PIECE_MIN=4096, XG_EXTENT_MEAN_MAX=0),                                 # numbers
        dict(XG_EXTENT_TILE_KIB=64, XG_SMALL_PIECE_KIB=4, XG_SMALL_PIECE_ORDER=1025),        # ranges
        dict(XG_SOLO_WAVES=16),
        dict(XG_SOLO_WAVES=16, XG_SOLO_RAILS=4),
        dict(XG_SOLO_RAILS=100000),
        dict(XG_ENGINE_WG=max(1, wmax - 1), XG_WAVE_GRID=max(1, grid - 1)),                  # the caps, below ...
        dict(XG_ENGINE_WG=wmax + 1, XG_WAVE_GRID=grid + 1),                                  # ... and above
    ]


def test_context_knobs_are_the_host_parsers(xg, facts):
    cus, wmax, grid = facts
    for env in _envs(wmax, grid):
        cx = _ctx_env(xg, **env)
        try:
            got = _fields(xg, cx.knobs())
        finally:
            cx.close()
        want = _fields(xg, xg.PlanTables.knobs(cus, wmax, grid, env=env))
        assert got == want, (env, {n: (got[n], want[n]) for n in got if got[n] != want[n]})
    low = _fields(xg, xg.PlanTables.knobs(cus, wmax, grid, env=_envs(wmax, grid)[-2]))
    assert (low["engine_wmax"], low["wave_grid"]) == (max(1, wmax - 1), max(1, grid - 1))


def test_virtual_context_knobs(xg, facts):
    cus, wmax, grid = facts
    cx = xg.Context.virtual(3, 8, device=0)
    try:
        got = _fields(xg, cx.knobs())
    finally:
        cx.close()
    assert got == _fields(xg, xg.PlanTables.knobs(cus, wmax, grid, rank=3, nranks=8, virt=1))
