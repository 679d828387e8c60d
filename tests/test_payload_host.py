"""xg_deliveries (devplan.c): every receive slot of a job paired with the send segment it must
equal -- the pairing of check_buffer's call sites (mpi_test.c:139, :215) in a form that needs no
fingerprint, which xg_exchange and xg.payload_check compare by span checksums.  CPU only.

Every golden configuration x its methods x G in {1, 2, 3, 8}: the list is xg_verify_slots of
every GPU in order, the send side lies inside the owning GPU's SEND region, every (dst, slot)
appears once, and -- independently of the library -- the oracle's closed form of the receive
buffers holds exactly the named segment in the named slot."""
import pytest

from conftest import golden_configs, load_golden

GPUS = (1, 2, 3, 8)


def _sched(xg, meta, method, d=None):
    P, A = meta["P"], meta["A"]
    rl = xg.aggregator_list(P, A, meta["proc_node"], meta["type"])
    it = meta["iters"] - 1
    return rl, it, xg.Schedule(method, P, A, meta["d"] if d is None else d, meta["c"], rl, ntimes=meta["ntimes"],
                               proc_node=meta["proc_node"], barrier_type=meta.get("barrier", 0), iteration=it)


@pytest.mark.parametrize("G", GPUS)
@pytest.mark.parametrize("cfg", golden_configs())
def test_deliveries_are_the_verify_slots_of_every_gpu(xg, cfg, G):
    meta = load_golden(cfg)[0]
    if G > meta["P"]:
        pytest.skip("more GPUs than ranks")
    for method in meta["method_list"]:
        _rl, _it, s = _sched(xg, meta, method)
        dl = s.deliveries(G)
        slots = [(g, x) for g in range(G) for x in s.verify_slots(G, g)]
        assert len(dl) == len(slots), (cfg, method, G)
        for q, (g, (src, seed, dst, off)) in zip(dl, slots):
            assert (q.src, q.seed, q.dst, q.recv_off, q.dst_gpu) == (src, seed, dst, off, g), (cfg, method, G)
            assert q.dst_gpu == s.gpu_of(G, q.dst) and q.src_gpu == s.gpu_of(G, q.src)
            assert q.recv_off == s.recv_offset(G, q.dst) + q.slot * s.d
            assert q.send_off == s.send_offset(G, q.src) + q.seed * s.d
            assert q.send_off >= 0 and q.send_off + s.d <= s.region_bytes(G, q.src_gpu, xg.BUF_SEND)
            assert q.recv_off >= 0 and q.recv_off + s.d <= s.region_bytes(G, q.dst_gpu, xg.BUF_RECV)
        assert len({(q.dst, q.slot) for q in dl}) == len(dl), (cfg, method, G)
        # no send segment is delivered twice, and each lies where xg_fill_runs puts (src, seed)
        assert len({(q.src, q.seed) for q in dl}) == len(dl), (cfg, method, G)
        segs = {(r, seed0 + i): off + i * s.d
                for g in range(G) for r, seed0, off, n in s.fill_runs(G, g) for i in range(n)}
        assert all(segs[(q.src, q.seed)] == q.send_off for q in dl), (cfg, method, G)


@pytest.mark.parametrize("cfg", golden_configs())
def test_deliveries_match_the_oracle_receive_buffers(xg, cfg):
    """the independent tie: at d = 64 on the collision-free fingerprint the oracle's expected
    receive buffer of dst holds fingerprint(src, seed) in slot `slot`, for every delivery"""
    import numpy as np
    import xg_oracle as O
    meta = load_golden(cfg)[0]
    d = 64
    for method in meta["method_list"]:
        rl, it, s = _sched(xg, meta, method, d=d)
        exp = O.expected_recv(method, meta["P"], meta["A"], d, rl, it, mode=1)
        dl = s.deliveries(1)
        assert dl or meta["A"] == 0
        for q in dl:
            got = exp[q.dst][q.slot * d:(q.slot + 1) * d]
            assert np.array_equal(got, O.fingerprint(1, q.src, q.seed, it, d)), (cfg, method, q.src, q.seed, q.dst)
        assert sum(len(v) for v in exp.values() if v is not None) == len(dl) * d, (cfg, method)


def test_deliveries_count_query_needs_no_buffer(xg):
    s = xg.Schedule(2, 8, 3, 1000, 3, xg.aggregator_list(8, 3))
    for G in (1, 2, 3, 8):
        assert xg.host().xg_deliveries(s.handle, G, None) == 24
        assert sorted((q.dst, q.slot) for q in s.deliveries(G)) == [(r, i) for r in range(8) for i in range(3)]
