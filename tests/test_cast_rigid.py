"""gjkepa_cast_rigid_batch(_device) and gjkepa_pose_pool(_device) on the GPU: the cast (time of impact) of
convex pairs with both bodies in rigid motion, and the pose that moves a pool along the same path.

The records are checked as tests/test_cast_rigid_host.py checks the host program's (tests/cast_rigid_ref.py):
every IMPACT certifies itself against an independent numpy pose, the reference distance at the time of impact
lies in [tau / 2, tau] and stays above tau / 2 before it, a MISS carries a plane that separates at t = 1,
overlapping starts agree with the oracle, CAST_MAXITER stays below 2% of a pool; and the kernel's records
equal the host program's byte for byte, for pools of every tier and a pool of hulls at every tier edge.

Measured on an MI355X (fp32 storage) over the pools below: every record equal to the host program's byte for
byte, so the figures are those of tests/test_cast_rigid_host.py (CAST_MAXITER on 1 pair each of the 8-32 pool
at tau 1e-6 and the 1-4 pool; 13.5 steps per impact, at most 64); 82 impacts of 100 on the tier-boundary pool
in at most 28 steps; distance of the pools posed at toi by pose_pool 0.549 to 0.9985 tau.
"""
import shutil

import numpy as np
import pytest

import cast_ref as cr
import cast_rigid_ref as rr
import distance_ref as dr
import gjkepa
from test_distance import boundary_pool

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")]

SEED = 0xD157
MOTION_SEED = 0xCA57
POOLS = {"8-32": (8, 32, 300, 1e-6), "8-32 coarse": (8, 32, 300, 1e-3), "1-4": (1, 4, 300, 1e-6), "33-256": (33, 256, 150, 1e-6)}


@pytest.fixture(scope="module")
def dist_host(tmp_path_factory):
    return cr.build_distance_host(tmp_path_factory.mktemp("rigid_dist"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return rr.build_host(tmp_path_factory.mktemp("rigid_host"))


class Case:
    def __init__(self, pool, bm, tau, orc, dist_host):
        self.pool, self.bm, self.tau = pool, bm, tau
        self.hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
        self.rec = gjkepa.cast_rigid_batch(pool, bm, tau)            # records=None
        assert self.rec.dtype == gjkepa.CAST64 and self.rec.shape == (pool.n_pairs,)
        self.ref = rr.Reference(dist_host, pool, bm)


@pytest.fixture(scope="module")
def cases(orc, dist_host):
    c = {}
    for k, (lo, hi, n, tau) in POOLS.items():
        pool = gjkepa.synth_pairs(SEED, n, lo, hi, 4.0)
        c[k] = Case(pool, rr.motions(pool, MOTION_SEED), tau, orc, dist_host)
    return c


@pytest.mark.parametrize("name", list(POOLS))
def test_casts_certify_and_agree_with_the_reference(cases, name):
    c = cases[name]
    rr.check_pool(c.pool, c.rec, c.tau, c.ref, c.hit, min_impacts=30, min_misses=5 if name == "33-256" else 0)


def test_outcome_counts_over_the_pools(cases):
    impacts = sum(int(rr.kinds(c.rec)[0].sum()) for c in cases.values())
    misses = sum(int(rr.kinds(c.rec)[1].sum()) for c in cases.values())
    assert impacts >= 150 and misses >= 60, (impacts, misses)


@pytest.mark.parametrize("name", list(POOLS))
def test_kernel_and_host_program_give_the_same_bytes(cases, host, name):
    """csrc/cast_advance.h and csrc/rigid_pose.h are one text for the kernel and for tests/cast_rigid_host.cpp,
    and the kernel's two-direction support scans return the plain scans' first maxima: the records agree
    byte for byte, for fp32 and fp64 storage."""
    c = cases[name]
    expect = host[0](c.pool, c.bm, c.tau).tobytes()
    assert c.rec.tobytes() == expect
    assert gjkepa.cast_rigid_batch(c.pool.as_dtype(np.float64), c.bm, c.tau).tobytes() == expect


def test_zero_rotation_passes_the_linear_casts_checks(cases, dist_host):
    c = cases["8-32"]
    d = cr.motions(c.pool, MOTION_SEED)
    rec = gjkepa.cast_rigid_batch(c.pool, rr.linear_motions(c.pool, d), c.tau)
    ref = cr.Reference(dist_host, c.pool, d)
    cr.check_pool(c.pool, d, rec, c.tau, ref, c.hit, cr.swept_distance(dist_host, ref))


@pytest.mark.parametrize("tau", [1e-3, 1e-6])
def test_known_answers(dist_host, host, tau):
    known, pool, bm = rr.known_pool(tau)
    rec = gjkepa.cast_rigid_batch(pool, bm, tau)
    rr.check_known(rec, tau, rr.Reference(dist_host, pool, bm), known)
    assert rec.tobytes() == host[0](pool, bm, tau).tobytes()


def test_prefixes_and_a_repeated_call(cases):
    c = cases["8-32"]
    p = c.pool
    assert gjkepa.cast_rigid_batch(p, c.bm, c.tau).tobytes() == c.rec.tobytes()
    for n in (1, 63, 64, 65):
        r = gjkepa.cast_rigid_batch(gjkepa.HullPool(p.verts, p.hull_off, p.hull_cnt, p.pairs[:n]), c.bm, c.tau)
        assert r.tobytes() == c.rec[:n].tobytes()


@pytest.mark.parametrize("name", ["8-32", "1-4", "33-256"])
def test_records_skip_the_hits(cases, name):
    c = cases[name]
    for prec in (gjkepa.PREC_F64, gjkepa.PREC_F32):
        contact = gjkepa.gjkepa_batch(c.pool, 2, 1.0, precision=prec)
        assert np.array_equal(contact["collision"] != 0, c.hit)
        r = gjkepa.cast_rigid_batch(c.pool, c.bm, c.tau, records=contact)
        assert np.array_equal((r["flags"] & rr.SKIPPED) != 0, c.hit)
        sk = r[c.hit]
        assert (sk["flags"] == rr.SKIPPED).all() and (sk["toi"] == 0).all() and (sk["iters"] == 0).all()
        assert (sk["steps"] == 0).all() and (sk["n_simplex"] == 0).all() and (sk["status"] == gjkepa.STATUS_OK).all()
        assert r[~c.hit].tobytes() == c.rec[~c.hit].tobytes()


def test_bad_input_leaves_neighbours_alone(cases):
    c = cases["8-32"]
    p = c.pool
    verts, cnt, bm = p.verts.copy(), p.hull_cnt.copy(), c.bm.copy()
    nan_pair, zero_pair, big_pair, nan_v, inf_w, nan_c = 10, 70, 131, 200, 201, 270
    verts[int(p.hull_off[p.pairs[nan_pair, 1]]) + 2] = np.nan
    cnt[p.pairs[zero_pair, 0]] = 0
    cnt[p.pairs[big_pair, 1]] = 257
    bm[p.pairs[nan_v, 0], 2] = np.nan
    bm[p.pairs[inf_w, 1], 3] = np.inf
    bm[p.pairs[nan_c, 1], 7] = np.nan
    r = gjkepa.cast_rigid_batch(gjkepa.HullPool(verts, p.hull_off, cnt, p.pairs), bm, c.tau)
    bad = [nan_pair, zero_pair, big_pair, nan_v, inf_w, nan_c]
    assert (r["status"][bad] == gjkepa.STATUS_BAD_INPUT).all()
    assert (r["toi"][bad] == 0).all() and (r["flags"][bad] == 0).all() and (r["n_simplex"][bad] == 0).all()
    keep = np.ones(p.n_pairs, bool)
    keep[bad] = False
    assert r[keep].tobytes() == c.rec[keep].tobytes()


def test_start_cases(host):
    pool, bm, flags = rr.start_and_bad_cases()
    rec = gjkepa.cast_rigid_batch(pool, bm, 1e-6)
    assert rec["flags"].tolist() == flags and (rec["status"] == gjkepa.STATUS_OK).all()
    assert rec.tobytes() == host[0](pool, bm, 1e-6).tobytes()


def test_tier_boundaries(orc, dist_host, host):
    """Hulls of 1 .. 256 vertices about two centres, every hull B moved onto hull A's centre, every body
    spinning with |w| = 0.5: the pool checks without the count thresholds, and every pair of two hulls of
    at least 32 vertices (both enclose their centre) is an IMPACT."""
    pool = boundary_pool()
    bm = rr.boundary_motions(pool)
    tau = 1e-6
    rec = gjkepa.cast_rigid_batch(pool, bm, tau)
    hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
    assert not hit.any()
    impact = rr.check_pool(pool, rec, tau, rr.Reference(dist_host, pool, bm), hit, min_impacts=0)[0]
    cnt = pool.hull_cnt[pool.pairs]
    assert impact[(cnt >= 32).all(axis=1)].all()
    assert rec.tobytes() == host[0](pool, bm, tau).tobytes()


def _device_pool(pool, bm, dev):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(pool.verts)).to(dev), torch.from_numpy(pool.hull_off).to(dev),
            torch.from_numpy(pool.hull_cnt).to(dev), torch.from_numpy(pool.pairs.reshape(-1).copy()).to(dev),
            torch.from_numpy(np.ascontiguousarray(bm, np.float64).reshape(-1)).to(dev))


def test_device_entry_chained_after_the_batch_and_captured(cases):
    """gjkepa_batch_device then gjkepa_cast_rigid_batch_device on one stream, eager and as a captured graph
    replayed twice: the bytes of the host entry with the batch's records (and, without records, the host
    entry's without)."""
    import torch
    c = cases["33-256"]
    pool, n = c.pool, c.pool.n_pairs
    dev = torch.device("cuda", 0)
    verts, off, cnt, prs, mot = _device_pool(pool, c.bm, dev)
    wsb, cwsb = gjkepa.workspace_bytes(n), gjkepa.cast_rigid_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    cws = torch.zeros(cwsb, dtype=torch.uint8, device=dev)
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)

    def run(out, stream, records=True):
        if records:
            gjkepa.gjkepa_batch_device(2, 1.0, pool.dtype_code, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(),
                                       cnt.data_ptr(), prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb, stream)
        gjkepa.cast_rigid_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                       mot.data_ptr(), c.tau, contact.data_ptr() if records else 0, gjkepa.PREC_F64,
                                       out.data_ptr(), cws.data_ptr(), cwsb, stream)

    expect = gjkepa.cast_rigid_batch(pool, c.bm, c.tau, records=gjkepa.gjkepa_batch(pool, 2, 1.0))
    work = torch.cuda.Stream(dev)
    eager = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    plain = torch.zeros_like(eager)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(work):
        run(eager, work.cuda_stream)
        run(plain, work.cuda_stream, records=False)
    torch.cuda.synchronize(dev)
    assert eager.cpu().numpy().tobytes() == expect.tobytes()
    assert plain.cpu().numpy().tobytes() == c.rec.tobytes()             # the host entry equals the device entry
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    with torch.cuda.graph(g, stream=side):
        run(out, side.cuda_stream)
    torch.cuda.synchronize(dev)
    for _ in range(2):
        with torch.cuda.stream(work):
            out.zero_()
            g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager)
    del g


def test_pose_pool_equals_the_host_function(cases, host):
    """device bytes (fp64 out) equal the host function's, fp32 out is np.float32 of those, time per hull and
    NULL both work, in place equals out of place, and the device entry equals the host entry"""
    import torch
    c = cases["33-256"]
    pool, bm = c.pool, c.bm
    nh = len(pool.hull_cnt)
    time = np.random.default_rng(11).uniform(0.0, 1.0, nh)
    for tm in (None, time):
        want64, _ = host[1](pool, bm, tm, np.float64)
        got64 = gjkepa.pose_pool(pool, bm, tm, np.float64)
        assert got64.verts.dtype == np.float64 and got64.verts.tobytes() == want64.tobytes()
        got32 = gjkepa.pose_pool(pool, bm, tm)
        assert got32.verts.dtype == np.float32 and got32.verts.tobytes() == want64.astype(np.float32).tobytes()
        p64 = pool.as_dtype(np.float64)
        assert gjkepa.pose_pool(p64, bm, tm).verts.tobytes() == want64.tobytes()
        assert gjkepa.pose_pool(p64, bm, tm, np.float32).verts.tobytes() == want64.astype(np.float32).tobytes()
    # the device entry, out of place and in place
    dev = torch.device("cuda", 0)
    verts, off, cnt, _, mot = _device_pool(pool, bm, dev)
    tdev = torch.from_numpy(time).to(dev)
    out = torch.zeros_like(verts)
    status = torch.full((nh,), -1, dtype=torch.int8, device=dev)
    want32 = host[1](pool, bm, time)[0]
    gjkepa.pose_pool_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), nh, mot.data_ptr(),
                            tdev.data_ptr(), gjkepa.DTYPE_F32, out.data_ptr(), status.data_ptr())
    torch.cuda.synchronize(dev)
    assert out.cpu().numpy().tobytes() == want32.tobytes() and (status.cpu().numpy() == gjkepa.STATUS_OK).all()
    gjkepa.pose_pool_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), nh, mot.data_ptr(),
                            tdev.data_ptr(), gjkepa.DTYPE_F32, verts.data_ptr())
    torch.cuda.synchronize(dev)
    assert verts.cpu().numpy().tobytes() == want32.tobytes()


def test_pose_pool_status_and_untouched_regions(cases):
    c = cases["8-32"]
    pool = c.pool
    nh = len(pool.hull_cnt)
    time = np.random.default_rng(5).uniform(0.0, 1.0, nh)
    good, st = gjkepa.pose_pool(pool, c.bm, time, np.float64, return_status=True)
    assert (st == gjkepa.STATUS_OK).all()
    bad = gjkepa.HullPool(pool.verts.copy(), pool.hull_off, pool.hull_cnt.copy(), pool.pairs)
    bm, btime = c.bm.copy(), time.copy()
    bad.hull_cnt[3] = 0
    bad.hull_cnt[5] = 257
    bm[10, 5] = np.inf
    btime[20] = np.nan
    bad.verts[int(bad.hull_off[30]) + 1] = np.nan
    badh = [3, 5, 10, 20, 30]
    posed, st = gjkepa.pose_pool(bad, bm, btime, np.float64, return_status=True)
    assert (st[badh] == gjkepa.STATUS_BAD_INPUT).all() and (np.delete(st, badh) == gjkepa.STATUS_OK).all()
    for h in range(nh):
        o, n = int(pool.hull_off[h]), int(pool.hull_cnt[h])
        want = bad.verts[o:o + 3 * n].astype(np.float64) if h in badh else good.verts[o:o + 3 * n]
        assert posed.verts[o:o + 3 * n].tobytes() == want.tobytes(), h


@pytest.mark.parametrize("name", ["8-32", "8-32 coarse", "33-256"])
def test_posing_at_toi_and_measuring_the_distance_is_consistent(cases, name):
    """for each impact: both hulls posed at toi by pose_pool (fp64 out), then gjkepa_distance_batch: a
    distance in [tau / 2, tau]"""
    c = cases[name]
    impact = rr.kinds(c.rec)[0]
    time = np.zeros(len(c.pool.hull_cnt))
    time[c.pool.pairs[:, 0]] = c.rec["toi"]
    time[c.pool.pairs[:, 1]] = c.rec["toi"]
    posed = gjkepa.pose_pool(c.pool, c.bm, time, np.float64)
    d = gjkepa.distance_batch(posed)
    dist = d["distance"][impact]
    assert (d["status"][impact] == gjkepa.STATUS_OK).all() and (d["flags"][impact] == 0).all()
    print(f"{name}: distance of the pools posed at toi / tau in [{(dist / c.tau).min():.6f}, {(dist / c.tau).max():.6f}]")
    assert (dist >= 0.5 * c.tau).all() and (dist <= c.tau).all()
