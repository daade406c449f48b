"""The swept broad phase's definition (include/gjkepa.h gjkepa_broadphase_swept, csrc/swept_sphere.h) without
a GPU: the header's text, compiled for the host (tests/sweep_host.cpp), gives the bits of the numpy
restatement (tests/sweep_ref.py); the list is a superset of what the rigid cast's host program reports as
IMPACT or START over every pair of a scene, at both tolerances, and closes the gap the static list leaves;
every branch of the parameter s is met by passing and failing pairs and agrees with a sampled closest
approach; invalid hulls and motions take part in no pair; the three entries check their arguments.

Measured (the scene of 96 hulls below, 4 560 pairs, either tolerance): 283 swept pairs against 432 static ones
(whose reach has the reference's + 1.0); the cast flags 59 IMPACT and 59 START, none undecided; all 118 are in
the swept list, and 16 of the IMPACT pairs are not in the static list."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cast_rigid_ref as rr
import gjkepa
import sweep_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

CAST_SEED = 6
N_CAST, BOX_CAST, VMAX_CAST = 96, 10.0, 3.0


@pytest.fixture(scope="module")
def sweep_host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sweep_host")), "libsweep_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    os.path.join(ROOT, "tests", "sweep_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.sweep_host.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_int64, vp, ctypes.c_double, vp, vp]

    def run(pool, bm, tolerance):
        n = len(pool.hull_cnt)
        verts = np.ascontiguousarray(pool.verts)
        off = np.ascontiguousarray(pool.hull_off, np.int64)
        cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
        mot = np.ascontiguousarray(bm, np.float64).reshape(-1)
        rho, ok = np.zeros(n), np.zeros((n, n), np.uint8)
        assert lib.sweep_host(pool.dtype_code, verts.ctypes.data, off.ctypes.data, cnt.ctypes.data, n, mot.ctypes.data,
                              float(tolerance), rho.ctypes.data, ok.ctypes.data) == 0
        return rho, ok != 0
    return run


@needs_gxx
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_header_text_gives_the_restatements_bits(sweep_host, dtype):
    pool, bm = sr.branch_scene()
    pool = pool.as_dtype(dtype)
    pool, bm, bad = sr.with_invalid(pool, bm)
    for tol in (1.0, 1e-3, 1e-6):
        _, ok, _, valid = sr.reference(pool, bm, tol, with_branch=True)
        vrho = sr.balls(pool, bm)[1]
        rho, got = sweep_host(pool, bm, tol)
        assert np.array_equal(np.isnan(rho), ~valid) and not valid[bad].any()
        assert rho[valid].tobytes() == vrho[valid].tobytes()
        assert np.array_equal(got, ok)


def test_every_branch_of_s_is_exercised_and_agrees_with_a_sampled_approach():
    pool, bm = sr.branch_scene()
    tol = 1e-3
    _, ok, branch, valid = sr.reference(pool, bm, tol, with_branch=True)
    assert valid.all()
    a, b = np.triu_indices(len(bm), 1)
    ok, branch = ok[a, b], branch[a, b]
    for k, name in sr.BRANCHES.items():
        n_pass, n_fail = int((ok & (branch == k)).sum()), int((~ok & (branch == k)).sum())
        print(f"{name}: {n_pass} passing, {n_fail} failing pairs")
        assert n_pass >= 5 and n_fail >= 5, (name, n_pass, n_fail)
    assert (branch[(a < 60) & (b < 60)] == sr.S_EE0).all()
    # the closest approach over 2001 sampled times, computed without s
    rho = sr.balls(pool, bm)[1]
    d, e = bm[a, 6:9] - bm[b, 6:9], bm[a, 0:3] - bm[b, 0:3]
    t = np.linspace(0.0, 1.0, 2001)
    low = np.linalg.norm(d[:, None, :] + t[None, :, None] * e[:, None, :], axis=2).min(1)
    reach = rho[a] + rho[b] + tol
    step = np.linalg.norm(e, axis=1) / 2000.0         # the true minimum lies within half a sample's travel below `low`
    assert (low[~ok] > reach[~ok]).all()
    assert (low[ok] - 0.5 * step[ok] <= reach[ok] * (1.0 + 1e-8)).all()


@needs_gxx
def test_list_is_a_superset_of_the_cast(orc, sweep_host, tmp_path_factory):
    """Every pair of 96 hulls cast by the host program at 1e-3 and 1e-6: what it flags IMPACT or START is in
    the reference list; the scene is one where that matters (IMPACT pairs the static list misses)."""
    cast = rr.build_host(tmp_path_factory.mktemp("sweep_cast"))[0]
    pool, bm = sr.scene(CAST_SEED, N_CAST, 8, 32, BOX_CAST, VMAX_CAST)
    pairs = sr.all_pairs(N_CAST)
    every = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pairs)
    static = set(sr.keys(orc.broadphase(pool.verts, pool.hull_off, pool.hull_cnt)[0]).tolist())
    for tol in (1e-3, 1e-6):
        ref = sr.reference(pool, bm, tol)
        assert np.array_equal(np.argwhere(sweep_host(pool, bm, tol)[1]), ref)   # the header's text gives this list
        listed = set(sr.keys(ref).tolist())
        rec = cast(every, bm, tol)
        impact, _, start, _, stopped = rr.kinds(rec)
        flagged = sr.keys(pairs[impact | start])
        gap = [k for k in sr.keys(pairs[impact]).tolist() if k not in static]
        print(f"tolerance {tol:g}: {len(ref)} swept pairs, {len(static)} static pairs of {len(pairs)}; cast: {impact.sum()} "
              f"impacts, {start.sum()} starts, {stopped.sum()} undecided; {len(gap)} impacts outside the static list")
        assert 0.01 * len(pairs) <= len(ref) <= 0.30 * len(pairs)
        assert stopped.sum() <= 0.02 * len(pairs)
        assert len(gap) >= 10
        missing = [k for k in flagged.tolist() if k not in listed]
        assert not missing, [(k >> 32, k & 0xFFFFFFFF) for k in missing]


def test_invalid_hulls_and_motions_take_part_in_no_pair():
    pool, bm = sr.scene(5, 120, 4, 64, 6.0, 2.0, dtype=np.float64)
    clean = sr.reference(pool, bm, 1e-3)
    bad_pool, bad_bm, bad = sr.with_invalid(pool, bm)
    ref = sr.reference(bad_pool, bad_bm, 1e-3)
    assert np.isin(clean, bad).any(axis=1).sum() >= len(bad)          # they were in pairs before
    assert not np.isin(ref, bad).any()
    keep = ~np.isin(clean, bad).any(axis=1)
    assert np.array_equal(ref, clean[keep])                            # and nobody else's pairs changed


def test_swept_api_validation_without_gpu(lib):
    inf, nan = float("inf"), float("nan")
    assert lib.gjkepa_broadphase_swept_workspace_bytes(-1, 0) < 0
    assert lib.gjkepa_broadphase_swept_workspace_bytes(0, -1) < 0
    n = np.full(1, 77, np.int64)
    host = lambda dtype, nh, tol, lr, count: lib.gjkepa_broadphase_swept(dtype, None, 0, None, None, nh, None, tol, lr, None, 0,
                                                                         count, 0)
    assert host(7, 1, 1e-3, inf, n.ctypes.data) == -1                  # dtype
    for tol in (0.0, -1.0, nan, inf):
        assert host(0, 0, tol, inf, n.ctypes.data) == -1
    for lr in (nan, -1.0, -inf):
        assert host(0, 0, 1e-3, lr, n.ctypes.data) == -1
    assert host(0, 0, 1e-3, inf, None) == -1                           # null count
    assert host(0, 1, 1e-3, inf, n.ctypes.data) == -1                  # null pool
    n[0] = 77
    assert host(0, 0, 1e-3, inf, n.ctypes.data) == 0 and n[0] == 0     # no hulls: no pairs
    assert host(1, 0, 1e-6, 0.0, n.ctypes.data) == 0 and n[0] == 0
    dev = lambda dtype, nh, tol, lr: lib.gjkepa_broadphase_swept_device(dtype, None, None, None, nh, None, tol, lr, None, 0,
                                                                        None, None, 0, None)
    assert dev(0, 5, 1e-3, inf) == -1                                  # null pointers
    assert dev(7, 5, 1e-3, inf) == -1 and dev(0, -1, 1e-3, inf) == -1
    assert dev(0, 5, 0.0, inf) == -1 and dev(0, 5, nan, inf) == -1 and dev(0, 5, 1e-3, nan) == -1 and dev(0, 5, 1e-3, -2.0) == -1
    assert b"long_radius" in lib.gjkepa_last_error()


def test_python_wrapper_checks_the_motion_shape():
    pool = gjkepa.synth_scene(1, 4, 8, 8, 2.0)
    with pytest.raises(gjkepa.GjkEpaError):
        gjkepa.broadphase_swept(pool, np.zeros((3, 9)), 1e-3)
