"""CPU tests of the separation-distance entries of the C-ABI (include/gjkepa.h gjkepa_distance_*): the
record layout, the workspace size and the argument checks, all of which run before any device work."""
import math

import numpy as np
import pytest

import gjkepa

INF = float("inf")


def test_record_size(lib):
    assert lib.gjkepa_distance_record_bytes() == 128 == gjkepa.DIST64.itemsize
    # the int8 fields sit behind lambda[3] and code[3], iters behind them
    assert gjkepa.DIST64.fields["code"][1] == 104 and gjkepa.DIST64.fields["n_simplex"][1] == 116
    assert gjkepa.DIST64.fields["flags"][1] == 118 and gjkepa.DIST64.fields["iters"][1] == 120


def test_workspace_bytes(lib):
    sizes = [gjkepa.distance_workspace_bytes(n) for n in (0, 1, 64, 1000, 1 << 20)]
    assert all(b > 0 for b in sizes) and sizes == sorted(sizes)
    assert lib.gjkepa_distance_workspace_bytes(-1) < 0
    with pytest.raises(gjkepa.GjkEpaError):
        gjkepa.distance_workspace_bytes(-5)


def test_exports_are_bound():
    for f in ("gjkepa_distance_record_bytes", "gjkepa_distance_workspace_bytes", "gjkepa_distance_batch_device",
              "gjkepa_distance_batch"):
        assert f in gjkepa.EXPORTS


def test_device_entry_argument_checks_without_gpu(lib):
    p = 0x1000     # never dereferenced: every call below is answered before any device work
    dev = lib.gjkepa_distance_batch_device
    assert dev(7, p, p, p, p, 1, None, 0, INF, p, p, 256, None) == -1                  # bad dtype
    assert dev(0, p, p, p, p, 1, p, 9, INF, p, p, 256, None) == -1                     # bad records_precision
    assert dev(0, p, p, p, p, -1, None, 0, INF, p, p, 256, None) == -1                 # negative n_pairs
    for hole in range(6):                                                             # null pointers
        a = [p] * 6
        a[hole] = None
        assert dev(0, a[0], a[1], a[2], a[3], 1, None, 0, INF, a[4], a[5], 256, None) == -1, hole
    assert dev(0, p, p, p, p, 1, None, 0, math.nan, p, p, 256, None) == -1             # NaN max_distance
    assert dev(0, p, p, p, p, 1, None, 0, -1.0, p, p, 256, None) == -1                 # negative max_distance
    assert b"max_distance" in lib.gjkepa_last_error()
    assert dev(0, p, p, p, p, 1, None, 0, INF, p, p, 8, None) == -4                    # workspace too small
    # a bad records_precision is not looked at without records
    assert dev(0, None, None, None, None, 0, None, 9, INF, None, None, 0, None) == 0


def test_empty_batch_returns_ok(lib):
    assert lib.gjkepa_distance_batch_device(0, None, None, None, None, 0, None, 0, INF, None, None, 0, None) == 0
    assert lib.gjkepa_distance_batch_device(1, None, None, None, None, 0, None, 0, 0.0, None, None, 0, None) == 0
    assert lib.gjkepa_distance_batch(0, None, 0, None, None, 0, None, 0, None, 0, INF, None, 0) == 0
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0)
    empty = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, np.zeros((0, 2), np.int32))
    assert len(gjkepa.distance_batch(empty)) == 0


def test_host_entry_argument_checks_without_gpu(lib):
    host = lib.gjkepa_distance_batch
    assert host(7, None, 0, None, None, 0, None, 1, None, 0, INF, None, 0) == -1       # bad dtype
    assert host(0, None, 0, None, None, 0, None, 1, None, 0, math.nan, None, 0) == -1  # NaN max_distance
    assert host(0, None, 0, None, None, 0, None, 1, None, 0, INF, None, 0) == -1       # null pointers
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0, dtype=np.float64)
    bad = pool.pairs.copy()
    bad[0, 0] = 99
    with pytest.raises(gjkepa.GjkEpaError, match="missing hull"):
        gjkepa.distance_batch(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, bad))
    off = pool.hull_off.copy()
    off[3] = pool.verts.size - 3                                                      # hull 3 runs past the pool
    with pytest.raises(gjkepa.GjkEpaError, match="outside the vertex pool"):
        gjkepa.distance_batch(gjkepa.HullPool(pool.verts, off, pool.hull_cnt, pool.pairs))
    with pytest.raises(gjkepa.GjkEpaError, match="records"):
        gjkepa.distance_batch(pool, records=np.zeros(3, gjkepa.REC64))
    with pytest.raises(gjkepa.GjkEpaError, match="max_distance"):
        gjkepa.distance_batch(pool, max_distance=-0.5)
