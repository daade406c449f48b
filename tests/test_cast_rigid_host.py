"""The rigid-motion cast's advancement, pose and simplex arithmetic (csrc/cast_advance.h cast_advance_rigid,
csrc/rigid_pose.h; shared by the rigid cast kernel and the pose kernel) on the host: tests/cast_rigid_host.cpp
runs it over a plain support scan, and its records are checked here the way tests/test_cast_rigid.py checks
the GPU's, without a GPU (tests/cast_rigid_ref.py): the IMPACT certificate against an independent numpy pose,
the reference distance at and before the time of impact, the misses' planes, the oracle's verdicts for the
overlapping starts, the linear cast's whole check at zero rotation, known answers, and the pose itself.

Measured on the host program (seeds below): CAST_MAXITER on 1 of 300 pairs of the 8-32 pool at tau 1e-6, on 1 of
300 of the 1-4 pool and on no pair of the other two; steps per impact mean 13.5 / p99 50 (8-32, 1e-6), 7.3 (8-32,
1e-3), 12.7 (1-4), 13.5 (33-256); 398 impacts and 279 misses over the four pools; the host pose within 0.45 of its
bound against the numpy pose.
"""
import shutil

import numpy as np
import pytest

import cast_ref as cr
import cast_rigid_ref as rr
import gjkepa

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

SEED = 0xD157
MOTION_SEED = 0xCA57
# name -> lo, hi, pairs, tau
POOLS = {"8-32": (8, 32, 300, 1e-6), "8-32 coarse": (8, 32, 300, 1e-3), "1-4": (1, 4, 300, 1e-6), "33-256": (33, 256, 150, 1e-6)}


@pytest.fixture(scope="module")
def dist_host(tmp_path_factory):
    return cr.build_distance_host(tmp_path_factory.mktemp("rigidhost_dist"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return rr.build_host(tmp_path_factory.mktemp("rigidhost"))


@pytest.fixture(scope="module")
def casts(host):
    """the four pools, their motions and the host program's records, computed once"""
    out = {}
    for name, (lo, hi, n, tau) in POOLS.items():
        pool = gjkepa.synth_pairs(SEED, n, lo, hi, 4.0)
        bm = rr.motions(pool, MOTION_SEED)
        out[name] = (pool, bm, tau, host[0](pool, bm, tau))
    return out


@pytest.mark.parametrize("name", list(POOLS))
def test_host_casts_certify_and_agree_with_the_reference(casts, host, dist_host, orc, name):
    pool, bm, tau, rec = casts[name]
    hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
    rr.check_pool(pool, rec, tau, rr.Reference(dist_host, pool, bm), hit, min_impacts=30, min_misses=5 if name == "33-256" else 0)
    # fp32 and fp64 storage of the same values: the same bytes
    assert host[0](pool.as_dtype(np.float64), bm, tau).tobytes() == rec.tobytes()


def test_host_outcome_counts_over_the_pools(casts):
    impacts = sum(int(rr.kinds(rec)[0].sum()) for _, _, _, rec in casts.values())
    misses = sum(int(rr.kinds(rec)[1].sum()) for _, _, _, rec in casts.values())
    assert impacts >= 150 and misses >= 60, (impacts, misses)


def test_host_zero_rotation_passes_the_linear_casts_checks(host, dist_host, orc):
    """w = 0 for both bodies, v_A = 0, v_B = d: the rigid records pass the linear cast's check unchanged"""
    lo, hi, n, tau = POOLS["8-32"]
    pool = gjkepa.synth_pairs(SEED, n, lo, hi, 4.0)
    d = cr.motions(pool, MOTION_SEED)
    rec = host[0](pool, rr.linear_motions(pool, d), tau)
    hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
    ref = cr.Reference(dist_host, pool, d)
    cr.check_pool(pool, d, rec, tau, ref, hit, cr.swept_distance(dist_host, ref))


@pytest.mark.parametrize("tau", [1e-3, 1e-6])
def test_host_known_answers(host, dist_host, tau):
    cases, pool, bm = rr.known_pool(tau)
    rec = host[0](pool, bm, tau)
    rr.check_known(rec, tau, rr.Reference(dist_host, pool, bm), cases)


def test_host_start_and_bad_input(host):
    tau = 1e-6
    pool, bm, flags = rr.start_and_bad_cases()
    rec = host[0](pool, bm, tau)
    assert (rec["status"] == gjkepa.STATUS_OK).all()
    assert rec["flags"].tolist() == flags
    assert (rec["toi"][[0, 2, 3]] == 0).all() and (rec["steps"][[0, 2, 3]] == 0).all()
    assert rec["n_simplex"][3] == 0 and (rec["normal"][3] == 0).all() and (rec["point_a"][3] == 0).all()
    assert rec["n_simplex"][2] >= 1 and abs(np.linalg.norm(rec["point_a"][2] - rec["point_b"][2]) - 5e-7) <= 1e-12
    assert np.allclose(rec["normal"][2], [-1, 0, 0], atol=1e-9)
    # a NaN in v, w and c, a zero count and a NaN vertex: BAD_INPUT, every other record unchanged
    bad = gjkepa.HullPool(pool.verts.copy(), pool.hull_off, pool.hull_cnt.copy(), pool.pairs)
    bbm = bm.copy()
    bbm[2 * 1 + 1, 1] = np.nan                        # v of hull B of pair 1
    bbm[2 * 4, 4] = np.nan                            # w of hull A of pair 4
    bbm[2 * 5 + 1, 8] = np.nan                        # c of hull B of pair 5
    bad.hull_cnt[2 * 6 + 1] = 0                       # hull B of pair 6
    bad.verts[int(bad.hull_off[2 * 7]) + 3] = np.nan  # hull A of pair 7
    rb = host[0](bad, bbm, tau)
    b = [1, 4, 5, 6, 7]
    assert (rb["status"][b] == gjkepa.STATUS_BAD_INPUT).all()
    assert (rb["flags"][b] == 0).all() and (rb["toi"][b] == 0).all() and (rb["n_simplex"][b] == 0).all()
    assert rb[[0, 2, 3]].tobytes() == rec[[0, 2, 3]].tobytes()


def test_host_pose_against_numpy(host):
    """the header's rational pose against the rotation matrix of the normalised quaternion: equal to
    4e-16 x (largest coordinate or pivot distance) x (1 + |w|)"""
    pool = gjkepa.synth_pairs(SEED, 200, 1, 64, 4.0, dtype=np.float64)
    bm = rr.motions(pool, MOTION_SEED)
    rng = np.random.default_rng(7)
    time = rng.uniform(0.0, 1.0, len(pool.hull_cnt))
    worst = 0.0
    for tm in (None, time):
        out, status = host[1](pool, bm, tm)
        assert (status == gjkepa.STATUS_OK).all()
        posed = gjkepa.HullPool(out, pool.hull_off, pool.hull_cnt, pool.pairs)
        for h in range(len(pool.hull_cnt)):
            P, t = pool.hull(h), 1.0 if tm is None else tm[h]
            # the reference in extended precision, so that the difference is the host function's error alone
            X = rr.pose(P, bm[h], t, np.longdouble)
            scale = max(np.abs(P).max(), float(np.abs(X).max()), np.linalg.norm(P - bm[h, 6:9], axis=1).max())
            bound = 4e-16 * scale * (1.0 + np.linalg.norm(bm[h, 3:6]))
            worst = max(worst, float(np.abs(posed.hull(h) - X).max()) / bound)
    print(f"host pose against the numpy pose: largest difference / bound {worst:.3f}")
    assert worst <= 1.0


def test_host_pose_exact_limits_and_status(host):
    pool = gjkepa.synth_pairs(SEED, 50, 1, 40, 4.0)
    bm = rr.motions(pool, MOTION_SEED)
    nh = len(pool.hull_cnt)
    # t = 0 returns the input bytes, for both output types
    out, _ = host[1](pool, bm, np.zeros(nh))
    assert out.dtype == np.float32 and out.tobytes() == pool.verts.tobytes()
    out64, _ = host[1](pool, bm, np.zeros(nh), np.float64)
    assert out64.tobytes() == pool.verts.astype(np.float64).tobytes()
    # w = 0 returns p + t v bit for bit
    lin = bm.copy()
    lin[:, 3:6] = 0.0
    time = np.random.default_rng(3).uniform(0.0, 1.0, nh)
    out64, _ = host[1](pool, lin, time, np.float64)
    posed = gjkepa.HullPool(out64, pool.hull_off, pool.hull_cnt, pool.pairs)
    for h in range(nh):
        assert np.array_equal(posed.hull(h), pool.hull(h) + time[h] * lin[h, 0:3])
    # fp32 out is the fp64 result rounded once; in place equals out of place
    full64, _ = host[1](pool, bm, time, np.float64)
    full32, _ = host[1](pool, bm, time, np.float32)
    assert full32.tobytes() == full64.astype(np.float32).tobytes()
    inplace = pool.verts.copy()
    host[1](gjkepa.HullPool(inplace, pool.hull_off, pool.hull_cnt, pool.pairs), bm, time, out=inplace)
    assert inplace.tobytes() == full32.tobytes()
    # status: bad count, non-finite motion, time and vertex; nothing written for those hulls
    bad = gjkepa.HullPool(pool.verts.copy(), pool.hull_off, pool.hull_cnt.copy(), pool.pairs)
    bbm, btime = bm.copy(), time.copy()
    bad.hull_cnt[3] = 0
    bbm[10, 5] = np.inf
    btime[20] = np.nan
    bad.verts[int(bad.hull_off[30])] = np.nan
    sentinel = np.full(pool.verts.size, 123.0)
    out, status = host[1](bad, bbm, btime, out=sentinel.copy())
    badh = [3, 10, 20, 30]
    assert (status[badh] == gjkepa.STATUS_BAD_INPUT).all() and (np.delete(status, badh) == gjkepa.STATUS_OK).all()
    for h in range(nh):
        o, n = int(pool.hull_off[h]), int(pool.hull_cnt[h])
        if h in badh:
            assert (out[o:o + 3 * n] == 123.0).all()
        else:
            assert out[o:o + 3 * n].tobytes() == full64[o:o + 3 * n].tobytes()
