"""CPU tests of the linear-cast entries of the C-ABI (include/gjkepa.h gjkepa_cast_*): the record
layout, the workspace size and the argument checks, all of which run before any device work."""
import math

import numpy as np
import pytest

import gjkepa

INF = float("inf")
TAU = 1e-6


def test_record_size(lib):
    assert lib.gjkepa_cast_record_bytes() == 128 == gjkepa.CAST64.itemsize
    # the distance record's layout: toi where the distance is, steps in its pad word
    for name, other in (("toi", "distance"), ("point_a", "point_a"), ("normal", "normal"), ("lambda", "lambda"),
                        ("code", "code"), ("n_simplex", "n_simplex"), ("status", "status"), ("flags", "flags"),
                        ("iters", "iters"), ("steps", "pad")):
        assert gjkepa.CAST64.fields[name][1] == gjkepa.DIST64.fields[other][1], name
    assert (gjkepa.CAST_IMPACT, gjkepa.CAST_START, gjkepa.CAST_SKIPPED, gjkepa.STATUS_CAST_MAXITER) == (1, 2, 4, 6)


def test_workspace_bytes(lib):
    sizes = [gjkepa.cast_workspace_bytes(n) for n in (0, 1, 64, 1000, 1 << 20)]
    assert all(b > 0 and b % 256 == 0 for b in sizes) and sizes == sorted(sizes)
    assert lib.gjkepa_cast_workspace_bytes(-1) < 0
    with pytest.raises(gjkepa.GjkEpaError):
        gjkepa.cast_workspace_bytes(-5)


def test_exports_are_bound():
    for f in ("gjkepa_cast_record_bytes", "gjkepa_cast_workspace_bytes", "gjkepa_cast_batch_device", "gjkepa_cast_batch"):
        assert f in gjkepa.EXPORTS


def test_device_entry_argument_checks_without_gpu(lib):
    p = 0x1000     # never dereferenced: every call below is answered before any device work
    dev = lib.gjkepa_cast_batch_device
    ws = gjkepa.cast_workspace_bytes(1)
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
    # a bad records_precision is not looked at without records
    assert dev(0, None, None, None, None, 0, None, TAU, None, 9, None, None, 0, None) == 0


def test_empty_batch_returns_ok(lib):
    assert lib.gjkepa_cast_batch_device(0, None, None, None, None, 0, None, TAU, None, 0, None, None, 0, None) == 0
    assert lib.gjkepa_cast_batch_device(1, None, None, None, None, 0, None, 1.0, None, 0, None, None, 0, None) == 0
    assert lib.gjkepa_cast_batch(0, None, 0, None, None, 0, None, 0, None, TAU, None, 0, None, 0) == 0
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0)
    empty = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, np.zeros((0, 2), np.int32))
    assert len(gjkepa.cast_batch(empty, np.zeros((0, 3)), TAU)) == 0


def test_host_entry_argument_checks_without_gpu(lib):
    host = lib.gjkepa_cast_batch
    assert host(7, None, 0, None, None, 0, None, 1, None, TAU, None, 0, None, 0) == -1        # bad dtype
    assert host(0, None, 0, None, None, 0, None, 1, None, math.nan, None, 0, None, 0) == -1   # NaN tolerance
    assert host(0, None, 0, None, None, 0, None, 1, None, TAU, None, 0, None, 0) == -1        # null pointers
    assert host(0, None, -1, None, None, 0, None, 1, None, TAU, None, 0, None, 0) == -1       # bad sizes
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0, dtype=np.float64)
    motion = np.zeros((4, 3))
    bad = pool.pairs.copy()
    bad[0, 0] = 99
    with pytest.raises(gjkepa.GjkEpaError, match="missing hull"):
        gjkepa.cast_batch(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, bad), motion, TAU)
    off = pool.hull_off.copy()
    off[3] = pool.verts.size - 3                                                      # hull 3 runs past the pool
    with pytest.raises(gjkepa.GjkEpaError, match="outside the vertex pool"):
        gjkepa.cast_batch(gjkepa.HullPool(pool.verts, off, pool.hull_cnt, pool.pairs), motion, TAU)
    with pytest.raises(gjkepa.GjkEpaError, match="records"):
        gjkepa.cast_batch(pool, motion, TAU, records=np.zeros(3, gjkepa.REC64))
    with pytest.raises(gjkepa.GjkEpaError, match="motion"):
        gjkepa.cast_batch(pool, np.zeros((3, 3)), TAU)
    for tol in (0.0, -0.5, INF, math.nan):
        with pytest.raises(gjkepa.GjkEpaError, match="tolerance"):
            gjkepa.cast_batch(pool, motion, tol)
