"""CPU tests of the rigid-motion cast and pool pose entries of the C-ABI (include/gjkepa.h gjkepa_cast_rigid_*,
gjkepa_pose_pool*): the workspace size and the argument checks, all of which run before any device work."""
import math

import numpy as np
import pytest

import gjkepa

INF = float("inf")
TAU = 1e-6


def test_constants_and_workspace_bytes(lib):
    assert gjkepa.MOTION_DOUBLES == 9
    sizes = [gjkepa.cast_rigid_workspace_bytes(n) for n in (0, 1, 64, 1000, 1 << 20)]
    assert all(b == 256 for b in sizes)
    assert sizes == [gjkepa.cast_workspace_bytes(n) for n in (0, 1, 64, 1000, 1 << 20)]
    assert lib.gjkepa_cast_rigid_workspace_bytes(-1) < 0
    with pytest.raises(gjkepa.GjkEpaError):
        gjkepa.cast_rigid_workspace_bytes(-5)


def test_exports_are_bound():
    for f in ("gjkepa_cast_rigid_workspace_bytes", "gjkepa_cast_rigid_batch_device", "gjkepa_cast_rigid_batch",
              "gjkepa_pose_pool_device", "gjkepa_pose_pool"):
        assert f in gjkepa.EXPORTS


def test_cast_device_entry_argument_checks_without_gpu(lib):
    p = 0x1000     # never dereferenced: every call below is answered before any device work
    dev = lib.gjkepa_cast_rigid_batch_device
    ws = gjkepa.cast_rigid_workspace_bytes(1)
    assert dev(7, p, p, p, p, 1, p, TAU, None, 0, p, p, ws, None) == -1                # bad dtype
    assert dev(0, p, p, p, p, 1, p, TAU, p, 9, p, p, ws, None) == -1                   # bad records_precision
    assert dev(0, p, p, p, p, -1, p, TAU, None, 0, p, p, ws, None) == -1               # negative n_pairs
    for hole in range(7):                                                             # null pointers
        a = [p] * 7
        a[hole] = None
        assert dev(0, a[0], a[1], a[2], a[3], 1, a[4], TAU, None, 0, a[5], a[6], ws, None) == -1, hole
    for bad in (math.nan, INF, -INF, 0.0, -1e-6):                                     # tolerance
        assert dev(0, p, p, p, p, 1, p, bad, None, 0, p, p, ws, None) == -1, bad
        assert b"tolerance" in lib.gjkepa_last_error()
    assert dev(0, p, p, p, p, 1, p, TAU, None, 0, p, p, ws - 1, None) == -4            # workspace too small
    assert dev(0, p, p, p, p, 1, p, TAU, None, 0, p, p, 8, None) == -4
    # a bad records_precision is not looked at without records; an empty batch is answered at once
    assert dev(0, None, None, None, None, 0, None, TAU, None, 9, None, None, 0, None) == 0
    assert dev(1, None, None, None, None, 0, None, 1.0, None, 0, None, None, 0, None) == 0


def test_cast_host_entry_argument_checks_without_gpu(lib):
    host = lib.gjkepa_cast_rigid_batch
    assert host(0, None, 0, None, None, 0, None, 0, None, TAU, None, 0, None, 0) == 0         # empty batch
    assert host(7, None, 0, None, None, 0, None, 1, None, TAU, None, 0, None, 0) == -1        # bad dtype
    assert host(0, None, 0, None, None, 0, None, 1, None, math.nan, None, 0, None, 0) == -1   # NaN tolerance
    assert host(0, None, 0, None, None, 0, None, 1, None, TAU, None, 0, None, 0) == -1        # null pointers
    assert host(0, None, -1, None, None, 0, None, 1, None, TAU, None, 0, None, 0) == -1       # bad sizes
    p = 0x1000
    assert host(0, p, 8, p, p, 2, p, 1, p, TAU, p, 9, p, 0) == -1                             # bad records_precision
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0, dtype=np.float64)
    bm = np.zeros((8, 9))
    empty = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, np.zeros((0, 2), np.int32))
    assert len(gjkepa.cast_rigid_batch(empty, bm, TAU)) == 0
    bad = pool.pairs.copy()
    bad[0, 0] = 99
    with pytest.raises(gjkepa.GjkEpaError, match="missing hull"):
        gjkepa.cast_rigid_batch(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, bad), bm, TAU)
    off = pool.hull_off.copy()
    off[3] = pool.verts.size - 3                                                      # hull 3 runs past the pool
    with pytest.raises(gjkepa.GjkEpaError, match="outside the vertex pool"):
        gjkepa.cast_rigid_batch(gjkepa.HullPool(pool.verts, off, pool.hull_cnt, pool.pairs), bm, TAU)
    with pytest.raises(gjkepa.GjkEpaError, match="records"):
        gjkepa.cast_rigid_batch(pool, bm, TAU, records=np.zeros(3, gjkepa.REC64))
    with pytest.raises(gjkepa.GjkEpaError, match="body_motion"):
        gjkepa.cast_rigid_batch(pool, np.zeros((4, 9)), TAU)                          # per pair, not per hull
    for tol in (0.0, -0.5, INF, math.nan):
        with pytest.raises(gjkepa.GjkEpaError, match="tolerance"):
            gjkepa.cast_rigid_batch(pool, bm, tol)


def test_pose_entries_argument_checks_without_gpu(lib):
    p, q = 0x1000, 0x2000
    dev, host = lib.gjkepa_pose_pool_device, lib.gjkepa_pose_pool
    assert dev(7, p, p, p, 1, p, None, 0, q, None, None) == -1                        # bad in_dtype
    assert dev(0, p, p, p, 1, p, None, 7, q, None, None) == -1                        # bad out_dtype
    assert dev(0, p, p, p, -1, p, None, 0, q, None, None) == -1                       # negative n_hulls
    for hole in range(5):                                                            # null pointers (time, status may be)
        a = [p, p, p, p, q]
        a[hole] = None
        assert dev(0, a[0], a[1], a[2], 1, a[3], None, 0, a[4], None, None) == -1, hole
    assert dev(0, p, p, p, 1, p, None, 1, p, None, None) == -1                        # in place with different dtypes
    assert b"in place" in lib.gjkepa_last_error()
    assert dev(0, None, None, None, 0, None, None, 0, None, None, None) == 0          # no hulls
    assert host(0, None, 0, None, None, 0, None, None, 0, None, None, 0) == 0
    assert host(7, p, 8, p, p, 1, p, None, 0, q, None, 0) == -1
    assert host(0, p, -1, p, p, 1, p, None, 0, q, None, 0) == -1                      # bad sizes
    assert host(0, None, 8, p, p, 1, p, None, 0, q, None, 0) == -1                    # null pointer
    assert host(1, p, 8, p, p, 1, p, None, 0, p, None, 0) == -1                       # in place with different dtypes
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0)
    bm = np.zeros((8, 9))
    off = pool.hull_off.copy()
    off[3] = pool.verts.size - 3
    with pytest.raises(gjkepa.GjkEpaError, match="outside the vertex pool"):
        gjkepa.pose_pool(gjkepa.HullPool(pool.verts, off, pool.hull_cnt, pool.pairs), bm)
    with pytest.raises(gjkepa.GjkEpaError, match="body_motion"):
        gjkepa.pose_pool(pool, np.zeros((4, 9)))
    with pytest.raises(gjkepa.GjkEpaError, match="time"):
        gjkepa.pose_pool(pool, bm, time=np.zeros(3))
