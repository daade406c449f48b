"""CPU tests of bench.py's roofline logic (no GPU): the dominant kernel is the one with the most launch
time per chain; its wall span is the union of its launches' intervals (two concurrent parts count
once); the pairs a parted launch serves are its route code's tally split by the hits in its range;
achieved = pairs per launch x bytes per pair / mean launch duration."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import gjkepa  # noqa: E402


def _rec(kernel, tier, chain, start, end, first=0, n=0, code=-1, part=0, stream=0):
    r = np.zeros(1, gjkepa.LAUNCH_TIME)
    r["kernel"], r["tier"], r["chain"], r["start_ms"], r["end_ms"] = kernel, tier, chain, start, end
    r["first_pair"], r["n_pairs"], r["route_code"], r["part"], r["stream"] = first, n, code, part, stream
    return r


def _chain(c, n):
    return [
        _rec(b"gjk", 0, c, 0.0, 1.0, 0, n),
        _rec(b"epa", 0, c, 1.0, 4.0, 0, n // 2, bench.ROUTE_EPA0, 0, 0),
        _rec(b"epa", 0, c, 1.1, 5.5, n // 2, n - n // 2, bench.ROUTE_EPA0, 1, 1),
        _rec(b"contact", 0, c, 4.0, 6.0, 0, n // 2, bench.ROUTE_CT0, 0, 2),   # 2.0 ms, but less than EPA's 7.4
        _rec(b"contact", 0, c, 6.0, 6.5, n // 2, n - n // 2, bench.ROUTE_CT0, 1, 2),
    ]


def test_busy_span_is_the_union_of_intervals():
    rs = np.concatenate([_rec(b"epa", 0, 0, 1.0, 4.0), _rec(b"epa", 0, 0, 1.1, 5.5), _rec(b"epa", 0, 0, 7.0, 8.0)])
    assert abs(bench.busy_span(rs) - (4.5 + 1.0)) < 1e-6


def test_dump_outputs_writes_every_field_of_a_fixed_sample(tmp_path):
    """--dump-outputs: one float .npy per record field; a batch above DUMP_MAX_PAIRS is cut to the same
    seeded sample every time, named by pair_index, and the whole dump stays under the byte limit."""
    n = bench.DUMP_MAX_PAIRS + 1000
    rng = np.random.default_rng(1)
    recs = np.zeros(n, gjkepa.REC64)
    recs["penetration_depth"] = rng.random(n)
    recs["collision_normal"] = rng.random((n, 3))
    recs["nearest_points"] = rng.random((n, 6))
    recs["collision"] = rng.integers(0, 2, n)
    recs["diag"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    info = bench.dump_outputs(str(tmp_path / "a"), recs)
    bench.dump_outputs(str(tmp_path / "b"), recs)
    idx = np.load(tmp_path / "a" / "pair_index.npy")
    assert len(idx) == bench.DUMP_MAX_PAIRS == info["records"] and info["of"] == n
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
    ii = idx.astype(np.int64)
    total = 0
    for name in ("pair_index",) + bench.DUMP_FIELDS:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float64 and a.tobytes() == b.tobytes(), name
        total += a.nbytes
        if name != "pair_index":
            assert (a == recs[name][ii]).all(), name
    assert total == info["bytes"] <= bench.DUMP_MAX_BYTES
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(x + ".npy" for x in info["arrays"])
    # a small batch is written whole; fp32 records keep their float fields in float32
    small = np.zeros(100, gjkepa.REC32)
    small["penetration_depth"] = np.arange(100)
    bench.dump_outputs(str(tmp_path / "c"), small)
    d = np.load(tmp_path / "c" / "penetration_depth.npy")
    assert d.dtype == np.float32 and (d == np.arange(100)).all()
    assert np.load(tmp_path / "c" / "status.npy").dtype == np.float64
    assert (np.load(tmp_path / "c" / "pair_index.npy") == np.arange(100)).all()


def test_dominant_kernel_parts_and_pairs():
    n = 1000
    lt = np.concatenate(_chain(0, n) + _chain(1, n))
    tally = np.zeros(bench.WS_TALLY, np.uint32)
    tally[bench.ROUTE_EPA0] = 600
    recs = np.zeros(n, gjkepa.REC64)
    recs["collision"][:400] = 1           # 400 hits in the first half, 200 in the second
    recs["collision"][500:700] = 1
    d = bench.dominant_kernel(lt, tally, recs, 928.0, None)
    assert d["kernel"] == "epa tier 0" and d["launches_per_step"] == 2.0
    assert abs(d["wall_span_ms"] - 4.5) < 1e-6                        # union of [1, 4] and [1.1, 5.5]
    assert abs(d["pairs_per_step"] - 600) < 1e-6 and abs(d["pairs_per_launch"] - 300) < 1e-6
    launch_ms = (3.0 + 4.4) / 2
    assert abs(d["launch_ms"] - launch_ms) < 1e-4
    assert abs(d["achieved"] - 300 * 928.0 / (launch_ms * 1e-3) / 1e9) < 1e-3
    assert abs(d["span_achieved"] - 600 * 928.0 / 4.5e-3 / 1e9) < 1e-3
    assert d["frac"] == round(d["achieved"] / bench.PEAK_HBM_GBS, 6)
