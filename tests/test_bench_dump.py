"""bench.py --dump-outputs: what the timed path's last step delivered, as .npy files two builds
can be compared by -- the sample is fixed by the arguments, its size bounded, and on the GPU every
sampled byte is the one the reference's fingerprint puts there."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO


def test_dump_sample_is_fixed_and_bounded():
    """the sample depends on the method and the sizes alone; every slot while they fit, a sorted
    subset without repeats when they do not; every chunk inside its slot; the default workload's
    dump (4 methods, 448 slots of 1 MiB each) stays far below 64 MB"""
    import bench
    per = bench.DUMP_ELEMS // 4
    s = bench.dump_sample(1, 448, 1 << 20, per)
    assert s == bench.dump_sample(1, 448, 1 << 20, per) != bench.dump_sample(2, 448, 1 << 20, per)
    assert [i for i, _o, _n in s] == list(range(448))
    assert all(n == bench.DUMP_CHUNK and 0 <= o <= (1 << 20) - n for _i, o, n in s)
    assert len({o for _i, o, _n in s}) > 400                       # offsets differ from slot to slot
    assert 4 * sum(n for _i, _o, n in s) * 4 < 64e6               # float32, all four methods
    # configs[4]'s 16384 slots under a 20-method budget: a subset within it
    per = bench.DUMP_ELEMS // 20
    s = bench.dump_sample(7, 256 * 64, 64 << 20, per)
    idx = [i for i, _o, _n in s]
    assert idx == sorted(set(idx)) and 0 <= idx[0] and idx[-1] < 256 * 64
    assert len(s) == per // bench.DUMP_CHUNK and sum(n for _i, _o, n in s) <= per
    assert 4 * bench.DUMP_ELEMS < 64e6                             # whatever the methods: 48 MiB of float32
    # segments shorter than a chunk are dumped whole
    assert bench.dump_sample(1, 3, 100, per) == [(0, 0, 100), (1, 0, 100), (2, 0, 100)]


@pytest.mark.gpu
def test_dump_outputs_hold_the_delivered_bytes(xg, tmp_path):
    """a small plain run (P12 A5, odd -d, methods 1-4) twice with the same arguments: the same files,
    byte for byte, float32, one row per sampled slot -- and every row the fingerprint of the slot's
    source (MAP_DATA: byte o = src + seed + o mod 256) at the sampled offset"""
    import bench
    import xg_oracle as O
    P, A, d, methods = 12, 5, 4099, (1, 2, 3, 4)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for dd in dirs:
        p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--procs", str(P), "--aggs", str(A), "--size", str(d), "--dump-outputs", str(dd)],
                           capture_output=True, text=True, timeout=100, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-2000:]
        line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) == ["method%d_recv.npy" % m for m in methods]
    rl = xg.aggregator_list(P, A)
    for m in methods:
        got = np.load(dirs[0] / ("method%d_recv.npy" % m))
        assert got.dtype == np.float32 and np.array_equal(got, np.load(dirs[1] / ("method%d_recv.npy" % m)))
        slots = xg.Schedule(m, P, A, d, 200000000, rl, ntimes=1).verify_slots(1, 0)
        sample = bench.dump_sample(m, len(slots), d, bench.DUMP_ELEMS // len(methods))
        assert len(slots) == P * A and got.shape == (len(sample), bench.DUMP_CHUNK)
        want = np.stack([O.map_data(slots[i][0], slots[i][1], 0, d)[o:o + n] for i, o, n in sample])
        assert np.array_equal(got, want.astype(np.float32)), m
