"""The distance GJK's simplex arithmetic (csrc/dist_simplex.h, shared by the distance kernel) on the
host: tests/distance_host.cpp runs it over a plain support scan, and its records are checked here the
way tests/test_distance.py checks the GPU's, without a GPU: self-certifying bounds, brute force, the
oracle's hit / miss verdicts, the max_distance early-out and the degenerate hulls."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import gjkepa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("disthost") / "libdistance_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    os.path.join(ROOT, "tests", "distance_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.distance_host_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_double, ctypes.c_void_p]

    def run(pool, max_distance=float("inf")):
        out = np.zeros(pool.n_pairs, gjkepa.DIST64)
        verts = np.ascontiguousarray(pool.verts)
        off = np.ascontiguousarray(pool.hull_off, np.int64)
        cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
        prs = np.ascontiguousarray(pool.pairs, np.int32).reshape(-1)
        assert lib.distance_host_batch(pool.dtype_code, verts.ctypes.data, off.ctypes.data, cnt.ctypes.data,
                                       prs.ctypes.data, pool.n_pairs, max_distance, out.ctypes.data) == 0
        return out
    return run


@pytest.mark.parametrize("lo,hi,n", [(8, 32, 1500), (1, 4, 600), (33, 256, 300)])
def test_host_records_certify_and_agree_with_the_oracle(host, orc, lo, hi, n):
    pool = gjkepa.synth_pairs(0xD157, n, lo, hi, 4.0)
    rec = host(pool)
    hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
    assert (~hit).mean() >= 0.30
    assert np.array_equal((rec["flags"] & gjkepa.DIST_OVERLAP) != 0, hit)
    assert (rec["status"] == gjkepa.STATUS_OK).all() and ((rec["flags"] & ~gjkepa.DIST_OVERLAP) == 0).all()
    assert (rec["distance"][hit] == 0).all() and (rec["n_simplex"][hit] == 0).all()
    miss = np.nonzero(~hit)[0]
    dr.check_certificate(pool, rec, miss)
    print(f"host distance GJK ({lo}, {hi}): largest iteration count {rec['iters'].max()}")
    assert rec["iters"].max() <= 64
    assert host(pool.as_dtype(np.float64)).tobytes() == rec.tobytes()


@pytest.mark.parametrize("lo,hi,n", [(1, 4, 600), (8, 12, 200)])
def test_host_distance_matches_brute_force(host, orc, lo, hi, n):
    pool = gjkepa.synth_pairs(0xD157, n, lo, hi, 4.0)
    rec = host(pool)
    miss = np.nonzero(orc.gjkepa_batch(pool, 2, 1.0)["collision"] == 0)[0]
    ref = dr.pool_distances(pool, miss)
    err = np.abs(rec["distance"][miss] - ref)
    print(f"host vs brute force ({lo}, {hi}): {len(miss)} pairs, worst relative error {(err / ref).max():.2e}")
    assert (err <= dr.tol(ref)).all()


def test_host_max_distance(host):
    pool = gjkepa.synth_pairs(0xD157, 1500, 8, 32, 4.0)
    full, cut = host(pool), host(pool, 0.5)
    far = (cut["flags"] & gjkepa.DIST_FAR) != 0
    sep = (full["flags"] & gjkepa.DIST_OVERLAP) == 0
    assert far.any() and not (far & ~sep).any()
    assert (full["distance"][far] > 0.5).all() and (cut["distance"][far] > 0.5).all()
    assert cut[~far].tobytes() == full[~far].tobytes()
    assert (cut["distance"][~far & sep] <= 0.5 + dr.tol(0.5)).all()
    assert (cut["distance"][far] <= full["distance"][far] + dr.tol(full["distance"][far])).all()
    dr.check_certificate(pool, cut, np.nonzero(far)[0], far=True)


def test_host_degenerate_hulls(host):
    """points, segments, a flat square against a parallel square, touching and overlapping boxes"""
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], float)
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], float)
    cases = [
        (np.zeros((1, 3)), np.array([[3.0, 4.0, 0.0]]), 5.0),
        (np.array([[0, 0, 0], [1, 0, 0]], float), np.array([[0, 2, -1], [0, 2, 1]], float), 2.0),
        (np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0]], float), np.array([[1, 1, 0], [1, 3, 0]], float), 1.0),   # collinear
        (sq, sq + [0.25, 0.25, 0.75], 0.75),
        (sq, sq + [3, 0, 0], 2.0),
        (cube, cube + [1.5, 0, 0], 0.5),
        (cube, cube + [2, 2, 2], np.sqrt(3.0)),
        (cube, cube + [1, 0, 0], 0.0),            # touching faces
        (cube, cube + [0.5, 0.2, 0.1], 0.0),      # overlapping
        (sq, sq + [0.5, 0.5, 0], 0.0),            # coplanar, overlapping
        (cube, cube, 0.0),
    ]
    pool = gjkepa.HullPool.from_pairs([(a, b) for a, b, _ in cases])
    rec = host(pool)
    want = np.array([d for _, _, d in cases])
    assert (np.abs(rec["distance"] - want) <= dr.tol(want)).all(), (rec["distance"], want)
    assert np.array_equal((rec["flags"] & gjkepa.DIST_OVERLAP) != 0, want == 0)
    dr.check_certificate(pool, rec, np.nonzero(want > 0)[0])
    bad = gjkepa.HullPool(pool.verts.copy(), pool.hull_off, pool.hull_cnt.copy(), pool.pairs)
    bad.verts[int(bad.hull_off[2])] = np.nan
    bad.hull_cnt[6] = 0
    rb = host(bad)
    assert rb["status"][1] == rb["status"][3] == gjkepa.STATUS_BAD_INPUT
    keep = np.ones(len(cases), bool)
    keep[[1, 3]] = False
    assert rb[keep].tobytes() == rec[keep].tobytes()
