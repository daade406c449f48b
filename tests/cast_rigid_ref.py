"""Shared helpers of the rigid-motion cast tests (tests/test_cast_rigid_host.py on the CPU,
tests/test_cast_rigid.py on the GPU): an independent pose in numpy (the rotation matrix of the normalised
quaternion, not the header's rational formula), the reference distance f(t) of the hulls posed by it (the
host distance program of tests/distance_host.cpp on fp64 pools), seeded body motions, and the checks a
pool's records have to pass.

f is not convex in t under rotation, so `free before toi` is sampled (64 uniform times in [0, toi) and
toi (1 - 2^-k), k = 1 .. 20) where the linear cast's tests search."""
import ctypes
import os
import subprocess

import numpy as np

import cast_ref as cr
import distance_ref as dr
import gjkepa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPACT, START, SKIPPED = gjkepa.CAST_IMPACT, gjkepa.CAST_START, gjkepa.CAST_SKIPPED
OK, MAXITER, BAD = gjkepa.STATUS_OK, gjkepa.STATUS_CAST_MAXITER, gjkepa.STATUS_BAD_INPUT
MAX_STEPS = 64
MAXITER_SHARE = 0.02


def rotation(w, t, dtype=np.float64):
    """R(t) for rotation vectors w (n, 3) at times t (n,): the matrix of the unit quaternion
    (1, t w / 2) / |(1, t w / 2)|"""
    w = np.asarray(w, dtype).reshape(-1, 3)
    t = np.broadcast_to(np.asarray(t, dtype), (len(w),))
    q = np.concatenate([np.ones((len(w), 1), dtype), 0.5 * t[:, None] * w], axis=1)
    q = q / np.sqrt((q * q).sum(1))[:, None]
    a, b, c, d = q.T
    return np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], 1),
                     np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], 1),
                     np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], 1)], 1)


def pose(P, m, t, dtype=np.float64):
    """the (n, 3) vertices P of a body with motion m = (v, w, c) at time t"""
    P, m = np.asarray(P, dtype).reshape(-1, 3), np.asarray(m, dtype)
    v, w, c = m[0:3], m[3:6], m[6:9]
    return c + dtype(t) * v + (P - c) @ rotation(w, t, dtype)[0].T


def build_host(tmpdir):
    """tests/cast_rigid_host.cpp; returns (cast, pose): cast(pool, body_motion, tolerance) -> CAST64 records,
    pose(pool, body_motion, time=None, out_dtype=None, out=None) -> (verts_out, int8 status per hull)."""
    so = os.path.join(str(tmpdir), "libcast_rigid_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    os.path.join(ROOT, "tests", "cast_rigid_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.cast_rigid_host_batch.argtypes = [ctypes.c_int, vp, vp, vp, vp, ctypes.c_int64, vp, ctypes.c_double, vp]
    lib.pose_host_batch.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int, vp, vp]

    def cast(pool, body_motion, tolerance):
        out = np.zeros(pool.n_pairs, gjkepa.CAST64)
        verts = np.ascontiguousarray(pool.verts)
        off = np.ascontiguousarray(pool.hull_off, np.int64)
        cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
        prs = np.ascontiguousarray(pool.pairs, np.int32).reshape(-1)
        mot = np.ascontiguousarray(body_motion, np.float64).reshape(-1)
        assert mot.size == 9 * cnt.size
        assert lib.cast_rigid_host_batch(pool.dtype_code, verts.ctypes.data, off.ctypes.data, cnt.ctypes.data, prs.ctypes.data,
                                         pool.n_pairs, mot.ctypes.data, float(tolerance), out.ctypes.data) == 0
        return out

    def pose_pool(pool, body_motion, time=None, out_dtype=None, out=None):
        verts = np.ascontiguousarray(pool.verts)
        off = np.ascontiguousarray(pool.hull_off, np.int64)
        cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
        mot = np.ascontiguousarray(body_motion, np.float64).reshape(-1)
        assert mot.size == 9 * cnt.size
        tm = None if time is None else np.ascontiguousarray(time, np.float64)
        if out is None:
            out = np.zeros(verts.size, out_dtype or verts.dtype)
        status = np.full(cnt.size, -1, np.int8)
        assert lib.pose_host_batch(pool.dtype_code, verts.ctypes.data, off.ctypes.data, cnt.ctypes.data, cnt.size, mot.ctypes.data,
                                   None if tm is None else tm.ctypes.data, gjkepa.DTYPE_F32 if out.dtype == np.float32 else
                                   gjkepa.DTYPE_F64, out.ctypes.data, status.ctypes.data) == 0
        return out, status
    return cast, pose_pool


def centres(pool):
    return np.array([pool.hull(h).mean(0) for h in range(len(pool.hull_cnt))])


def motions(pool, seed, wmax=1.0):
    """Body motions (n_hulls, 9) of a pool whose hulls belong to one pair each: the linear part of
    cast_ref.motions, d per pair, split -0.3 d for hull A and +0.7 d for hull B; a rotation vector of
    uniformly random direction and length U[0, wmax] per body; the pivot at the hull's vertex mean."""
    d = cr.motions(pool, seed)
    rng = np.random.default_rng(seed ^ 0x5A17)
    nh = len(pool.hull_cnt)
    assert len(np.unique(pool.pairs)) == pool.pairs.size
    m = np.zeros((nh, 9))
    m[pool.pairs[:, 0], 0:3] = -0.3 * d
    m[pool.pairs[:, 1], 0:3] = 0.7 * d
    u = rng.normal(size=(nh, 3))
    m[:, 3:6] = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.0, wmax, size=(nh, 1))
    m[:, 6:9] = centres(pool)
    return m


def linear_motions(pool, d):
    """w = 0 for both bodies, v_A = 0, v_B = d per pair"""
    m = np.zeros((len(pool.hull_cnt), 9))
    m[pool.pairs[:, 1], 0:3] = d
    m[:, 6:9] = centres(pool)
    return m


class Reference:
    """f(t) = distance of A(t) and B(t) for every pair of a pool at once: the pairs as an fp64 pool of
    their own (hull 2k = A of pair k, 2k + 1 = its B) posed by the numpy pose, through the host distance
    program."""

    def __init__(self, dist_host, pool, body_motion):
        self.dist_host = dist_host
        self.n = pool.n_pairs
        bm = np.asarray(body_motion, np.float64).reshape(-1, 9)
        hulls = [pool.hull(int(h)) for h in pool.pairs.reshape(-1)]
        self.base = gjkepa.HullPool.from_pairs(list(zip(hulls[0::2], hulls[1::2])))
        self.P = np.concatenate(hulls)
        self.body = np.repeat(np.arange(2 * self.n), [len(h) for h in hulls])
        self.m = bm[pool.pairs.reshape(-1)]
        # where vertex i of the concatenation goes in the pool: x, y, z columns of its hull
        cnt, off = self.base.hull_cnt.astype(np.int64), self.base.hull_off
        local = np.arange(len(self.P)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        self.pos = off[self.body][:, None] + np.arange(3)[None] * cnt[self.body][:, None] + local[:, None]

    def at(self, t):
        """the pairs' pool with both hulls of pair k posed at t[k]"""
        t = np.repeat(np.broadcast_to(np.asarray(t, np.float64), (self.n,)), 2)
        R = rotation(self.m[:, 3:6], t)[self.body]
        c, v = self.m[self.body, 6:9], self.m[self.body, 0:3]
        X = c + t[self.body, None] * v + np.einsum("nij,nj->ni", R, self.P - c)
        verts = np.zeros_like(self.base.verts)
        verts[self.pos] = X
        return gjkepa.HullPool(verts, self.base.hull_off, self.base.hull_cnt, self.base.pairs)

    def hulls_at(self, k, t):
        p = self.at(np.full(self.n, t))
        return p.hull(2 * k), p.hull(2 * k + 1)

    def f(self, t):
        r = self.dist_host(self.at(t))
        assert (r["status"] == OK).all()
        return np.where((r["flags"] & gjkepa.DIST_OVERLAP) != 0, 0.0, r["distance"])


def kinds(rec):
    """masks of a batch's records: impact, miss, start, overlapping start, undecided (CAST_MAXITER)"""
    ok = rec["status"] == OK
    impact = ok & (rec["flags"] == IMPACT)
    miss = ok & (rec["flags"] == 0)
    start = ok & (rec["flags"] == START)
    return impact, miss, start, start & (rec["n_simplex"] == 0), rec["status"] == MAXITER


def check_impacts(pool, ref, rec, idx, tau):
    """An IMPACT record certifies itself: the witness points rebuilt from lambda / code with the numpy pose
    at toi are the record's to 1e-12 of the coordinates and lie at most tau apart; the normal is unit and
    min n.a(toi) - max n.b(toi) > 0 over the posed hulls.  Returns (width, gap) per pair."""
    width, gap = np.zeros(len(idx)), np.zeros(len(idx))
    for j, k in enumerate(idx):
        r = rec[k]
        toi = float(r["toi"])
        assert r["flags"] == IMPACT and r["status"] == OK and 0.0 < toi < 1.0, (k, r)
        A, B = (pose(ref.P[ref.body == 2 * k + s], ref.m[2 * k + s], toi) for s in (0, 1))
        n = int(r["n_simplex"])
        assert 1 <= n <= 3, (k, n)
        lam, code = r["lambda"], r["code"]
        assert (lam >= 0).all() and (lam[n:] == 0).all() and (code[n:] == 0xFFFFFFFF).all(), (k, lam, code)
        assert abs(lam.sum() - 1.0) <= 1e-12, (k, lam)
        ia, ib = (code[:n] & 0xFFFF).astype(np.int64), (code[:n] >> 16).astype(np.int64)
        assert (ia < len(A)).all() and (ib < len(B)).all(), (k, code)
        pa, pb = lam[:n] @ A[ia], lam[:n] @ B[ib]
        ptol = 1e-12 * (1.0 + max(np.abs(A).max(), np.abs(B).max()))
        assert np.abs(pa - r["point_a"]).max() <= ptol and np.abs(pb - r["point_b"]).max() <= ptol, (k, pa, pb, r)
        width[j] = float(np.linalg.norm(r["point_a"] - r["point_b"]))
        assert width[j] <= tau + dr.tol(tau), (k, width[j], tau)
        nrm = r["normal"]
        assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-12, (k, nrm)
        gap[j] = float((A @ nrm).min() - (B @ nrm).max())
        assert gap[j] > 0.0, (k, gap[j])
    return width, gap


def check_free_before(ref, rec, mask, tau, include_end=None):
    """f >= tau / 2 at 64 uniform times in [0, toi) and at toi (1 - 2^-k), k = 1 .. 20, for the records of
    `mask`; include_end: the records checked at toi itself as well (the misses, at t = 1).  Returns the
    smallest f / tau seen."""
    toi = np.where(mask, rec["toi"], 0.0)
    fracs = [j / 64.0 for j in range(64)] + [1.0 - 2.0 ** -k for k in range(1, 21)]
    low = np.inf
    for fr in fracs + ([1.0] if include_end is not None else []):
        m = mask if fr < 1.0 else include_end
        if not m.any():
            continue
        f = ref.f(toi * fr)
        bad = m & ~(f >= 0.5 * tau - dr.tol(tau))
        assert not bad.any(), (fr, np.nonzero(bad)[0][:8], f[bad][:8], toi[bad][:8])
        low = min(low, float((f[m] / tau).min()))
    return low


def check_miss_normals(ref, rec, idx):
    """a MISS record's normal separates the hulls posed at t = 1"""
    for k in idx:
        r = rec[k]
        assert r["flags"] == 0 and r["status"] == OK and r["toi"] == 1.0 and r["n_simplex"] == 0, (k, r)
        A, B = (pose(ref.P[ref.body == 2 * k + s], ref.m[2 * k + s], 1.0) for s in (0, 1))
        nrm = r["normal"]
        assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-12, (k, nrm)
        assert (A @ nrm).min() - (B @ nrm).max() > 0.0, (k, r)


def check_pool(pool, rec, tau, ref, hit, min_impacts=30, min_misses=0):
    """Every check the pools' records have to pass, for the host program and the GPU alike.  ref: Reference
    of (pool, body_motion); hit: the oracle's collision flags on the unposed pool.  Returns kinds()."""
    impact, miss, start, start_overlap, stopped = kinds(rec)
    assert np.isin(rec["status"], (OK, MAXITER)).all(), np.unique(rec["status"])
    assert (impact | miss | start | stopped).all()
    assert rec["steps"].max() <= MAX_STEPS and (rec["reserved"] == 0).all()
    assert (rec["flags"][stopped] == 0).all()
    print(f"{pool.n_pairs} pairs at tau {tau:g}: {impact.sum()} impacts, {miss.sum()} misses, {start.sum()} starts "
          f"({start_overlap.sum()} overlapping), {stopped.sum()} undecided; steps per impact mean "
          f"{rec['steps'][impact].mean() if impact.any() else 0:.2f} p99 "
          f"{np.percentile(rec['steps'][impact], 99) if impact.any() else 0:.0f} max {rec['steps'].max()}, iters per impact mean "
          f"{rec['iters'][impact].mean() if impact.any() else 0:.1f} max {rec['iters'].max()}")
    assert stopped.sum() <= MAXITER_SHARE * pool.n_pairs, (stopped.sum(), pool.n_pairs)
    assert impact.sum() >= min_impacts and miss.sum() >= min_misses, (impact.sum(), miss.sum())
    ii = np.nonzero(impact)[0]
    width, gap = check_impacts(pool, ref, rec, ii, tau)
    f_toi = ref.f(np.where(impact, rec["toi"], 0.0))[ii]
    if len(ii):
        print(f"  impacts: width / tau in [{(width / tau).min():.4f}, {(width / tau).max():.4f}], smallest gap / tau "
              f"{(gap / tau).min():.4f}, reference distance at toi / tau in [{(f_toi / tau).min():.6f}, {(f_toi / tau).max():.6f}]")
    assert (f_toi <= tau + dr.tol(tau)).all() and (f_toi >= 0.5 * tau - dr.tol(tau)).all()
    low = check_free_before(ref, rec, impact | stopped | miss, tau, include_end=miss)
    print(f"  free before toi: smallest reference distance / tau over the samples {low:.6f}")
    check_miss_normals(ref, rec, np.nonzero(miss)[0])
    assert np.array_equal(start_overlap, hit)
    ss = np.nonzero(start & ~start_overlap)[0]
    if len(ss):
        assert (ref.f(np.zeros(pool.n_pairs))[ss] <= tau + dr.tol(tau)).all()
    return impact, miss, start, start_overlap, stopped


def boundary_motions(pool, seed=0xB0D1):
    """tests/test_distance.py boundary_pool: every hull B (the second set) moved onto the first set's
    centre, every body spinning with |w| = 0.5 about its vertex mean"""
    nh = len(pool.hull_cnt)
    rng = np.random.default_rng(seed)
    m = np.zeros((nh, 9))
    m[np.unique(pool.pairs[:, 1]), 0:3] = [-3.0, -0.5, -0.25]
    u = rng.normal(size=(nh, 3))
    m[:, 3:6] = 0.5 * u / np.linalg.norm(u, axis=1, keepdims=True)
    m[:, 6:9] = centres(pool)
    return m


CUBE = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], float)
SLAB = CUBE * [20, 20, 1] + [-10, -10, -1]                    # the resting box [-10, 10]^2 x [-1, 0]
BAR = np.array([[-1, 0, 0.5], [1, 0, 0.5]], float)
STILL = [0.0] * 6


def band(gap_to_time, tau):
    """the analytic band of toi: from the time the gap is tau to the time it is tau / 2"""
    return gap_to_time(tau), gap_to_time(0.5 * tau)


def known_cases(tau):
    """name -> (hull A, motion A, hull B, motion B, (lo, hi) band of toi or None for a miss with 0 steps,
    outcomes allowed)"""
    bar_t = lambda gap: (2 / 1.2) * np.tan(0.5 * np.arcsin(0.5 - gap))
    cube_t = lambda gap: (2 / 1.5) * np.tan(0.5 * (np.arcsin((0.65 - gap) * np.sqrt(2.0)) - np.pi / 4))
    tumbling = CUBE + [0.0, -0.5, 0.15]                        # unit cube centred (0.5, 0, 0.65)
    spinning = CUBE + [0.0, 0.0, 1.25]
    return {
        "swinging bar": (BAR, STILL[:3] + [0, 1.2, 0, 0, 0, 0.5], SLAB, STILL + [0, 0, -0.5], band(bar_t, tau), "impact"),
        "tumbling cube": (tumbling, STILL[:3] + [1.5, 0, 0, 0.5, 0, 0.65], SLAB, STILL + [0, 0, -0.5], band(cube_t, tau), "impact"),
        "spin about the normal": (spinning, STILL[:3] + [0, 0, 2, 0.5, 0.5, 1.75], CUBE, STILL + [0.5, 0.5, 0.5], None, "miss"),
        "spin about the normal, falling": (spinning, [0, 0, -1, 0, 0, 2, 0.5, 0.5, 1.75], CUBE, STILL + [0.5, 0.5, 0.5],
                                           (0.25 - tau, 0.25 - 0.5 * tau), "impact"),
        "plate about a distant pivot": (BAR, STILL + [0, 0, 0.5], SLAB, STILL[:3] + [0, -1.2, 0, 0, 0, 0.5], band(bar_t, tau),
                                        "impact or undecided"),
    }


def known_pool(tau):
    cases = known_cases(tau)
    pool = gjkepa.HullPool.from_pairs([(c[0], c[2]) for c in cases.values()])
    bm = np.array([m for c in cases.values() for m in (c[1], c[3])], float)
    return cases, pool, bm


def check_known(rec, tau, ref, cases):
    for k, (name, case) in enumerate(cases.items()):
        r, bnd, allowed = rec[k], case[4], case[5]
        impact, stopped = r["status"] == OK and r["flags"] == IMPACT, r["status"] == MAXITER
        print(f"{name} at tau {tau:g}: status {r['status']} flags {r['flags']} toi {r['toi']:.9f} steps {r['steps']} band {bnd}")
        if allowed == "miss":
            assert r["status"] == OK and r["flags"] == 0 and r["toi"] == 1.0 and r["steps"] == 0, (name, r)
            continue
        assert impact or (stopped and allowed == "impact or undecided"), (name, r)
        assert r["toi"] <= bnd[1] + 1e-12, (name, r["toi"], bnd)
        if impact:
            assert bnd[0] - 1e-12 <= r["toi"], (name, r["toi"], bnd)
    impact, miss, _, _, stopped = kinds(rec)
    check_impacts(None, ref, rec, np.nonzero(impact)[0], tau)
    check_free_before(ref, rec, impact | stopped | miss, tau, include_end=miss)
    check_miss_normals(ref, rec, np.nonzero(miss)[0])


def start_and_bad_cases():
    """(pool, body motions, expected flags) of the START cases, and the edits that make pairs bad"""
    spin = [0, 0, 0, 0.3, -0.2, 0.4]
    cases = [
        (CUBE, CUBE + [1, 0, 0], [-1, 0, 0]),                # touching at t = 0
        (CUBE, CUBE + [3, 0, 0], [-4, 0, 0]),
        (CUBE, CUBE + [1 + 5e-7, 0, 0], [-1, 0, 0]),         # separated by less than tau = 1e-6 at t = 0
        (CUBE, CUBE + [0.5, 0.2, 0.1], [1, 0, 0]),           # overlapping at t = 0
        (CUBE, CUBE + [0, 3, 0], [0, -4, 0]),
        (CUBE, CUBE + [0, 0, 3], [0, 0, -4]),
        (CUBE, CUBE + [-3, 0, 0], [4, 0, 0]),
        (CUBE, CUBE + [0, -3, 0], [0, 4, 0]),
    ]
    pool = gjkepa.HullPool.from_pairs([(a, b) for a, b, _ in cases])
    bm = np.zeros((2 * len(cases), 9))
    bm[:, 3:6] = spin[3:]
    bm[1::2, 0:3] = [d for _, _, d in cases]
    bm[:, 6:9] = centres(pool)
    return pool, bm, [START, IMPACT, START, START, IMPACT, IMPACT, IMPACT, IMPACT]
