"""Per-launch timing of the tier chain (include/gjkepa.h gjkepa_launch_timing), the basis of bench.py's
dominant-kernel roofline: every launch of an overlapped chain is reported once, on the stream it ran
on, with start <= end inside the chain (launches of one stream in order); timing never changes a
record, and the records match the oracle.  test_schedule pins the shipped schedule launch by launch."""
import os
import sys

import numpy as np
import pytest

import gjkepa

pytestmark = pytest.mark.gpu
SEED = 0x6A4B5C1D


def _device_run(pool, timing: bool, precision=gjkepa.PREC_F64):
    import torch
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(pool.verts).to(dev)
    o = torch.from_numpy(pool.hull_off).to(dev)
    c = torch.from_numpy(pool.hull_cnt).to(dev)
    p = torch.from_numpy(pool.pairs.reshape(-1).copy()).to(dev)
    n = pool.n_pairs
    out = torch.zeros(n * gjkepa.record_dtype(precision).itemsize, dtype=torch.uint8, device=dev)
    wsb = gjkepa.workspace_bytes_for(n, gjkepa.large_pairs(pool))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    gjkepa.launch_timing(timing)
    for _ in range(2):
        gjkepa.gjkepa_batch_device(2, 1.0, gjkepa.DTYPE_F32, precision, v.data_ptr(), o.data_ptr(), c.data_ptr(),
                                   p.data_ptr(), n, out.data_ptr(), ws.data_ptr(), wsb, s.cuda_stream)
    gjkepa.launch_timing(False)
    lt = gjkepa.launch_timing_read()
    torch.cuda.synchronize(dev)
    return np.frombuffer(out.cpu().numpy().tobytes(), gjkepa.record_dtype(precision)), lt


@pytest.mark.parametrize("lo,hi", [(32, 32), (8, 256)])
def test_launch_timing_covers_the_chain(orc, lo, hi):
    n = 70000                                         # >= 64K pairs: the overlapped (multi-stream) chain
    pool = gjkepa.synth_pairs(SEED, n, lo, hi, 2.5)
    plain, lt0 = _device_run(pool, False)
    timed, lt = _device_run(pool, True)
    assert len(lt0) == 0
    assert plain.tobytes() == timed.tobytes()
    assert sorted(set(lt["chain"].tolist())) == [0, 1]
    one = lt[lt["chain"] == 1]
    kinds = [(k.decode(), int(t)) for k, t in zip(one["kernel"], one["tier"])]
    assert kinds[0] == ("reset", 0) and kinds[1] == ("gjk", 0) and kinds[2] == ("gjk", 1)
    assert sum(1 for k in kinds if k == ("epa", 0)) == 2           # EPA tier 0 in two parts
    assert {("epa", t) for t in range(6)} <= set(kinds) and ("contact", 0) in kinds
    assert (one["start_ms"] >= 0).all() and (one["end_ms"] >= one["start_ms"]).all()
    assert one["stream"].max() >= 1                                # internal streams reported
    e0 = one[(one["kernel"] == b"epa") & (one["tier"] == 0)]
    assert e0["first_pair"][0] == 0 and e0["first_pair"][1] + e0["n_pairs"][1] == n
    e2 = one[(one["kernel"] == b"epa") & (one["tier"] == 2)]
    e3 = one[(one["kernel"] == b"epa") & (one["tier"] == 3)]
    assert e2["stream"][0] == e3["stream"][0]                       # EPA tiers 2 and 3 in sequence
    assert e3["start_ms"][0] >= e2["end_ms"][0]
    sub = np.arange(0, n, 7)
    ref = orc.gjkepa_batch(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[sub]), 2, 1.0)
    assert timed[sub].tobytes() == ref.tobytes()


def _single_stream(n):
    """The chain of 65 <= n < 64K pairs: every launch on the caller's stream over the whole range."""
    return ([("reset", 0, 0, -1, 0, 0, 0),
             ("gjk", 0, 0, -1, 0, 0, n), ("gjk", 1, 0, 1, 0, 0, n), ("gjk", 2, 0, 2, 0, 0, n)]
            + [("epa", t, 0, 0x10 + t, 0, 0, n) for t in range(6)]
            + [("contact", 0, 0, 0x20, 0, 0, n), ("contact", 1, 0, 0x21, 0, 0, n)])


N_OV = 65536 + 37        # the smallest overlapped batch with a partial last chunk: 1025 chunks, cut at 666
# streams in order of first use: 0 the caller's, 1 the pass of fork point 0, 2 EPA tier 0's second part,
# 3 the pass of fork point 2
_OVERLAPPED = [
    ("reset", 0, 0, -1, 0, 0, 0),
    ("gjk", 0, 0, -1, 0, 0, N_OV), ("gjk", 1, 0, 1, 0, 0, N_OV), ("gjk", 2, 0, 2, 0, 0, N_OV),
    ("epa", 0, 0, 0x10, 0, 0, 42624), ("contact", 0, 0, 0x20, 1, 0, 42624),
    ("epa", 0, 1, 0x10, 2, 42624, 22949), ("contact", 0, 1, 0x20, 1, 42624, 22949),
    ("epa", 1, 0, 0x11, 0, 0, N_OV), ("epa", 2, 0, 0x12, 0, 0, N_OV),
    ("contact", 0, 0, 0x24, 3, 0, N_OV), ("contact", 1, 0, 0x25, 3, 0, N_OV),
    ("epa", 3, 0, 0x13, 0, 0, N_OV), ("epa", 4, 0, 0x14, 0, 0, N_OV), ("epa", 5, 0, 0x15, 0, 0, N_OV),
    ("contact", 0, 0, 0x2A, 0, 0, N_OV), ("contact", 1, 0, 0x2B, 0, 0, N_OV),
]
_F64, _F32 = gjkepa.PREC_F64, gjkepa.PREC_F32
SCHEDULES = {
    (64, _F64): [("query", 0, 0, -1, 0, 0, 64)],
    (65, _F64): _single_stream(65),
    (65, _F32): _single_stream(65) + [("redo", 0, 0, 0x2E, 0, 0, 65)],
    (N_OV, _F64): _OVERLAPPED,
    (N_OV, _F32): _OVERLAPPED + [("redo", 0, 0, 0x2E, 0, 0, N_OV)],
}
assert [len(v) for v in SCHEDULES.values()] == [1, 12, 13, 17, 18]


def schedule_of(lt, chain=1):
    """(kernel, tier, part, route_code, stream, first_pair, n_pairs) of every launch of one chain."""
    one = lt[lt["chain"] == chain]
    return [(r["kernel"].decode(), int(r["tier"]), int(r["part"]), int(r["route_code"]), int(r["stream"]),
             int(r["first_pair"]), int(r["n_pairs"])) for r in one]


@pytest.mark.parametrize("n,precision", list(SCHEDULES), ids=lambda v: str(v))
def test_schedule(orc, n, precision):
    """The launches gjkepa_batch_device enqueues, in order, with the stream each goes to and the pair
    range it covers: one fused launch up to 64 pairs, the single-stream chain above, the overlapped
    chain from 64K pairs (EPA tier 0 in parts of 650 and 350 per mille of the 64-pair chunks)."""
    pool = gjkepa.synth_pairs(SEED, n, 4, 32, 2.5)
    rec, lt = _device_run(pool, True, precision)
    got = schedule_of(lt)
    print(f"n={n} precision={precision}")
    for row in got:
        print(row)
    assert got == SCHEDULES[(n, precision)]
    if n == N_OV:
        sub = np.arange(0, n, 7)
        ref = orc.gjkepa_batch(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[sub]), 2, 1.0)
        if precision == _F32:                         # the oracle's model of the fp32 path (test_gpu_parity.py)
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
            from fp32_check import model_fp32
            ref, _ = model_fp32(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[sub]), ref, 16)
        assert rec[sub].tobytes() == ref.tobytes()
