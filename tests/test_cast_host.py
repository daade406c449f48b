"""The linear cast's advancement and simplex arithmetic (csrc/cast_advance.h, shared by the cast kernel)
on the host: tests/cast_host.cpp runs it over a plain support scan, and its records are checked here the
way tests/test_cast.py checks the GPU's, without a GPU (tests/cast_ref.py): the IMPACT certificate, the
reference distance at the time of impact, the first time the reference comes within the tolerance, the
swept hull for the misses, the oracle's verdicts for the overlapping starts, brute force, and known
answers."""
import shutil

import numpy as np
import pytest

import cast_ref as cr
import distance_ref as dr
import gjkepa
from test_distance import boundary_pool

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

SEED = 0xD157
MOTION_SEED = 0xCA57


@pytest.fixture(scope="module")
def dist_host(tmp_path_factory):
    return cr.build_distance_host(tmp_path_factory.mktemp("casthost_dist"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cr.build_cast_host(tmp_path_factory.mktemp("casthost"))


@pytest.mark.parametrize("lo,hi,n,tau", [(8, 32, 1500, 1e-6), (8, 32, 1500, 1e-3), (1, 4, 600, 1e-6), (33, 256, 300, 1e-6)])
def test_host_casts_certify_and_agree_with_the_reference(host, dist_host, orc, lo, hi, n, tau):
    pool = gjkepa.synth_pairs(SEED, n, lo, hi, 4.0)
    motion = cr.motions(pool, MOTION_SEED)
    rec = host(pool, motion, tau)
    hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
    ref = cr.Reference(dist_host, pool, motion)
    cr.check_pool(pool, motion, rec, tau, ref, hit, cr.swept_distance(dist_host, ref))
    # fp32 and fp64 storage of the same values: the same bytes
    assert host(pool.as_dtype(np.float64), motion, tau).tobytes() == rec.tobytes()


def test_host_tier_boundary_pool(host, dist_host):
    """hulls of 1 .. 256 vertices about two centres, hull B moved onto hull A's centre"""
    pool = boundary_pool()
    motion = np.tile([-3.0, -0.5, -0.25], (pool.n_pairs, 1))
    rec = host(pool, motion, 1e-6)
    cr.check_boundary(pool, motion, rec, cr.Reference(dist_host, pool, motion), 1e-6)


@pytest.mark.parametrize("lo,hi,n", [(1, 4, 600), (8, 12, 200)])
def test_host_distance_at_toi_matches_brute_force(host, lo, hi, n):
    tau = 1e-6
    pool = gjkepa.synth_pairs(SEED, n, lo, hi, 4.0)
    motion = cr.motions(pool, MOTION_SEED)
    rec = host(pool, motion, tau)
    ii = np.nonzero(cr.kinds(rec)[0])[0]
    assert len(ii) >= 30
    d = np.array([dr.pair_distance(pool.hull(int(pool.pairs[k, 0])),
                                   pool.hull(int(pool.pairs[k, 1])) + rec["toi"][k] * motion[k]) for k in ii])
    print(f"brute force at toi ({lo}, {hi}): {len(ii)} impacts, distance / tau in [{(d / tau).min():.6f}, {(d / tau).max():.6f}]")
    assert (d <= tau + dr.tol(tau)).all() and (d >= 0.5 * tau - dr.tol(tau)).all()


CUBE = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], float)
# (hull A, hull B, motion, analytic time of contact or None for a miss, approach speed)
KNOWN = {
    "cube face to face": (CUBE, CUBE + [3, 0, 0], [-4, 0, 0], 0.5, 4.0),
    "ray against a cube face": (np.array([[0.3, 0.4, 2.0]]), CUBE, [0, 0, 2], 0.5, 2.0),
    "crossing segments": (np.array([[-1, 0, 0], [1, 0, 0]], float), np.array([[0, -1, 1], [0, 1, 1]], float), [0, 0, -2], 0.5, 2.0),
    "corner to corner": (CUBE, CUBE + [2, 2, 2], [-2, -2, -2], 0.5, 2.0 * np.sqrt(3.0)),
    "sliding past a face": (CUBE, CUBE + [1.5, -3, 0], [0, 6, 0], None, 0.0),
    "moving away": (CUBE, CUBE + [3, 0, 0], [1, 0, 0], None, 0.0),
}


@pytest.mark.parametrize("tau", [1e-3, 1e-6, 1e-9])
def test_host_known_answers(host, tau):
    names = list(KNOWN)
    pool = gjkepa.HullPool.from_pairs([(KNOWN[k][0], KNOWN[k][1]) for k in names])
    motion = np.array([KNOWN[k][2] for k in names], float)
    rec = host(pool, motion, tau)
    assert (rec["status"] == gjkepa.STATUS_OK).all()
    for k, name in enumerate(names):
        t_hit, speed = KNOWN[name][3], KNOWN[name][4]
        r = rec[k]
        if t_hit is None:
            assert r["flags"] == 0 and r["toi"] == 1.0, (name, r)
            continue
        # contact at t_hit; the gap is tau at t_hit - tau / speed and tau / 2 at t_hit - tau / (2 speed)
        assert r["flags"] == cr.IMPACT, (name, r)
        lo, hi = t_hit - tau / speed, t_hit - 0.5 * tau / speed
        assert lo - 1e-12 <= r["toi"] <= hi + 1e-12, (name, r["toi"], lo, hi)
    # The certificate's normal is the direction of point_a - point_b, a vector of length ~tau between
    # points known to eps * scale each (eps = 2^-53): it is off by about eps * scale / tau radians, which
    # moves the gap along it by eps * scale * extent / tau.  That stays below the gap of tau / 2 only for
    # tau^2 > 2 eps * scale * extent, tau above about 3e-8 at the unit scale of these cases: the times of
    # impact hold at 1e-9 (above), the plane certificate is checked at 1e-3 and 1e-6.
    if tau >= 1e-6:
        cr.check_cast_certificate(pool, motion, rec, [k for k, n in enumerate(names) if KNOWN[n][3] is not None], tau)
    cr.check_miss_certificate(pool, motion, rec, [k for k, n in enumerate(names) if KNOWN[n][3] is None])
    first = rec[0]["toi"]
    assert (2 - tau) / 4 - 1e-12 <= first <= (2 - tau / 2) / 4 + 1e-12


def test_host_start_and_bad_input(host):
    tau = 1e-6
    cases = [
        (CUBE, CUBE + [1, 0, 0], [-1, 0, 0]),                # touching at t = 0
        (CUBE, CUBE + [3, 0, 0], [-4, 0, 0]),
        (CUBE, CUBE + [1 + 5e-7, 0, 0], [-1, 0, 0]),         # separated by less than tau at t = 0
        (CUBE, CUBE + [0.5, 0.2, 0.1], [1, 0, 0]),           # overlapping at t = 0
        (CUBE, CUBE + [0, 3, 0], [0, -4, 0]),
        (CUBE, CUBE + [0, 0, 3], [0, 0, -4]),
    ]
    pool = gjkepa.HullPool.from_pairs([(a, b) for a, b, _ in cases])
    motion = np.array([d for _, _, d in cases], float)
    rec = host(pool, motion, tau)
    assert (rec["status"] == gjkepa.STATUS_OK).all()
    assert rec["flags"].tolist() == [cr.START, cr.IMPACT, cr.START, cr.START, cr.IMPACT, cr.IMPACT]
    assert (rec["toi"][[0, 2, 3]] == 0).all() and (rec["steps"][[0, 2, 3]] == 0).all()
    assert rec["n_simplex"][3] == 0 and (rec["normal"][3] == 0).all() and (rec["point_a"][3] == 0).all()
    assert rec["n_simplex"][2] >= 1 and abs(np.linalg.norm(rec["point_a"][2] - rec["point_b"][2]) - 5e-7) <= 1e-12
    assert np.allclose(rec["normal"][2], [-1, 0, 0], atol=1e-9)
    # NaN vertex, zero count, NaN motion: BAD_INPUT, every other record unchanged
    bad = gjkepa.HullPool(pool.verts.copy(), pool.hull_off, pool.hull_cnt.copy(), pool.pairs)
    bad.verts[int(bad.hull_off[2])] = np.nan          # hull A of pair 1
    bad.hull_cnt[9] = 0                               # hull B of pair 4
    bmotion = motion.copy()
    bmotion[5, 1] = np.nan
    rb = host(bad, bmotion, tau)
    assert (rb["status"][[1, 4, 5]] == gjkepa.STATUS_BAD_INPUT).all()
    assert (rb["flags"][[1, 4, 5]] == 0).all() and (rb["toi"][[1, 4, 5]] == 0).all() and (rb["n_simplex"][[1, 4, 5]] == 0).all()
    assert rb[[0, 2, 3]].tobytes() == rec[[0, 2, 3]].tobytes()
