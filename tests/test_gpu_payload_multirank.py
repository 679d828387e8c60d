"""xg_exchange between real ranks: one 2-rank job on the box's one MI355X (XG_SHARE_GPU=1, as
tests/test_gpu_multirank.py runs its jobs: every process under its own time limit, a failed or
late rank ends the job).  Each rank exchanges seeded random bytes in buffers of its own; the
source checksums travel over the job's MAX reduction and every slot is compared with its
segment's -- and, in the worker, the whole RECV region with the numpy execution.  The last call
hands rank 1 a SEND pointer misaligned by 8 bytes: both ranks must return the same error and
the job must end normally (nobody waits in RCCL for the rank that refused)."""
import json
import pathlib
import sys
import tempfile

import pytest

from conftest import REPO
from test_gpu_multirank import _env, _spawn, _wait_all

pytestmark = pytest.mark.gpu

WORKER = str(pathlib.Path(REPO) / "tests" / "payload_worker.py")


def test_exchange_as_two_rank_job(tmp_path):
    G, P, A, d, methods, timeout = 2, 8, 4, 4096, [1, 2, 5], 120
    case = {"shape": [P, A, d, 3], "methods": methods}
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="job", dir=str(tmp_path)))
    procs = [_spawn([sys.executable, "-u", WORKER, json.dumps(case)],
                    _env(tmp, RANK=r, WORLD_SIZE=G, LOCAL_RANK=r, XG_MR_DEADLINE=timeout - 10), None, "rank%d" % r, tmp)
             for r in range(G)]
    outs = _wait_all(procs, timeout)
    failed = ["rank %d exit %d: %s" % (r, p.returncode, " | ".join(err.strip().splitlines()[-3:]))
              for r, ((p, _o, _e), (_out, err)) in enumerate(zip(procs, outs)) if p.returncode]
    assert not failed, "\n".join(failed)
    rows = [[json.loads(x) for x in out.splitlines() if x.startswith("{")] for out, _err in outs]
    for r in range(G):
        assert rows[r][-1] == {"done": True} and len(rows[r]) == len(methods) + 2, rows[r]
        for row, m in zip(rows[r], methods):
            assert (row["method"], row["rc"], row["bad"], row["wrong_bytes"], row["err"]) == (m, 0, 0, 0, ""), row
            assert row["slots"] > 0 and row["total_time"] > 0, row
    assert sum(rows[r][0]["slots"] for r in range(G)) == P * A
    last = [rows[r][len(methods)] for r in range(G)]
    assert all(x["misaligned"] for x in last)
    assert last[0]["rc"] == last[1]["rc"] == 3, last                # XG_EARG on the rank that refused and its peer
    assert "refused" in last[1]["err"] and "another GPU" in last[0]["err"], last
