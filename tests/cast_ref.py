"""Shared helpers of the linear-cast tests (tests/test_cast_host.py on the CPU, tests/test_cast.py on the
GPU): seeded motions for a pool, the certificate an IMPACT (and a MISS) record carries, and a reference
for the distance f(t) of hull A and hull B + t d built on the host distance program of
tests/distance_host.cpp (itself checked against brute force by tests/test_distance_host.py).

f is convex in t (the distance of two convex sets under a linear motion), so its minimum over [0, 1] is
found by a golden-section search and the first time it falls to tau by bisection on [0, argmin]."""
import ctypes
import os
import subprocess

import numpy as np

import distance_ref as dr
import gjkepa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPACT, START, SKIPPED = gjkepa.CAST_IMPACT, gjkepa.CAST_START, gjkepa.CAST_SKIPPED


def build_distance_host(tmpdir):
    """tests/distance_host.cpp, built exactly as tests/test_distance_host.py builds it; returns
    run(pool, max_distance=inf) -> DIST64 records."""
    so = os.path.join(str(tmpdir), "libdistance_host.so")
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


def build_cast_host(tmpdir):
    """tests/cast_host.cpp (csrc/cast_advance.h over a naive support scan); returns
    run(pool, motion, tolerance) -> CAST64 records."""
    so = os.path.join(str(tmpdir), "libcast_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    os.path.join(ROOT, "tests", "cast_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.cast_host_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]

    def run(pool, motion, tolerance):
        out = np.zeros(pool.n_pairs, gjkepa.CAST64)
        verts = np.ascontiguousarray(pool.verts)
        off = np.ascontiguousarray(pool.hull_off, np.int64)
        cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
        prs = np.ascontiguousarray(pool.pairs, np.int32).reshape(-1)
        mot = np.ascontiguousarray(motion, np.float64).reshape(-1)
        assert mot.size == 3 * pool.n_pairs
        assert lib.cast_host_batch(pool.dtype_code, verts.ctypes.data, off.ctypes.data, cnt.ctypes.data, prs.ctypes.data,
                                   pool.n_pairs, mot.ctypes.data, float(tolerance), out.ctypes.data) == 0
        return out
    return run


def motions(pool, seed):
    """d = -c U[0, 1.5] + w U[0, 1] per pair: c = hull B's centroid minus hull A's, w a random unit
    vector; aimed roughly at A, from a seeded numpy generator."""
    rng = np.random.default_rng(seed)
    n = pool.n_pairs
    c = np.array([pool.hull(int(b)).mean(0) - pool.hull(int(a)).mean(0) for a, b in pool.pairs])
    w = rng.normal(size=(n, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    return -c * rng.uniform(0.0, 1.5, size=(n, 1)) + w * rng.uniform(0.0, 1.0, size=(n, 1))


class Moved:
    """The pairs of a pool as an fp64 pool of their own (hull 2k = A of pair k, 2k + 1 = its B), whose B
    hulls can be translated per pair and doubled into the swept hull conv(B, B + d)."""

    def __init__(self, pool, motion):
        self.n = pool.n_pairs
        self.d = np.asarray(motion, np.float64).reshape(self.n, 3)
        self.A = [pool.hull(int(a)) for a, _ in pool.pairs]
        self.B = [pool.hull(int(b)) for _, b in pool.pairs]
        self.base = gjkepa.HullPool.from_pairs(list(zip(self.A, self.B)))
        # per vertex scalar of the pool: its pair and axis if it belongs to a hull B, else pair -1
        self.pair_of = np.full(self.base.verts.size, -1, np.int64)
        self.axis_of = np.zeros(self.base.verts.size, np.int64)
        for k in range(self.n):
            o, m = int(self.base.hull_off[2 * k + 1]), int(self.base.hull_cnt[2 * k + 1])
            self.pair_of[o:o + 3 * m] = k
            self.axis_of[o:o + 3 * m] = np.repeat(np.arange(3), m)
        self.isb = self.pair_of >= 0

    def at(self, t):
        """the pool with every hull B of pair k moved by t[k] d[k]"""
        t = np.broadcast_to(np.asarray(t, np.float64), (self.n,))
        v = self.base.verts.copy()
        k, ax = self.pair_of[self.isb], self.axis_of[self.isb]
        v[self.isb] += t[k] * self.d[k, ax]
        return gjkepa.HullPool(v, self.base.hull_off, self.base.hull_cnt, self.base.pairs)

    def swept(self, idx):
        """pairs idx with hull B replaced by the vertices of B and B + d (their hull is what B sweeps)"""
        return gjkepa.HullPool.from_pairs([(self.A[k], np.concatenate([self.B[k], self.B[k] + self.d[k]])) for k in idx])


class Reference:
    """f(t) = distance of A and B + t d for every pair of a pool at once, from the host distance program"""

    def __init__(self, dist_host, pool, motion):
        self.dist_host = dist_host
        self.mv = Moved(pool, motion)

    def f(self, t):
        r = self.dist_host(self.mv.at(t))
        assert (r["status"] == gjkepa.STATUS_OK).all()
        return np.where((r["flags"] & gjkepa.DIST_OVERLAP) != 0, 0.0, r["distance"])

    def argmin(self, iters=44):
        """golden-section search of the convex f over [0, 1]: bracket width 0.618^44 = 6e-10"""
        n = self.mv.n
        g = (np.sqrt(5.0) - 1.0) / 2.0
        lo, hi = np.zeros(n), np.ones(n)
        x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
        f1, f2 = self.f(x1), self.f(x2)
        for _ in range(iters):
            left = f1 <= f2                      # the minimum lies in [lo, x2]; else in [x1, hi]
            hi = np.where(left, x2, hi)
            lo = np.where(left, lo, x1)
            nx1, nx2 = hi - g * (hi - lo), lo + g * (hi - lo)
            fn1, fn2 = self.f(nx1), self.f(nx2)
            x1, x2, f1, f2 = nx1, nx2, fn1, fn2
        cand = np.stack([np.zeros(n), lo, x1, x2, hi, np.ones(n)])
        vals = np.stack([self.f(c) for c in cand])
        best = vals.argmin(0)
        return cand[best, np.arange(n)], vals[best, np.arange(n)]

    def first_within(self, tau, hint=None, iters=52):
        """per pair a time `before` with f(before) > tau such that f <= tau is first reached within 2^-52
        after it (0 when f(0) <= tau; +inf when the search finds no time with f <= tau).  hint: times to
        try beside the golden-section minimum (the records' toi)."""
        n = self.mv.n
        tm, fm = self.argmin()
        if hint is not None:
            fh = self.f(hint)
            better = fh < fm
            tm, fm = np.where(better, hint, tm), np.where(better, fh, fm)
        f0 = self.f(np.zeros(n))
        lo, hi = np.zeros(n), tm.copy()
        for _ in range(iters):
            mid = 0.5 * (lo + hi)
            below = self.f(mid) <= tau
            hi = np.where(below, mid, hi)
            lo = np.where(below, lo, mid)
        out = lo
        out = np.where(f0 <= tau, 0.0, out)
        return np.where(fm <= tau, out, np.inf), fm


def check_cast_certificate(pool, motion, rec, idx, tau):
    """Assert that the IMPACT records rec[idx] certify themselves and return (width, gap, speed) per
    pair: |point_a - point_b|, the gap min_i n.a_i - max_j n.b_j - toi n.d along the record's normal,
    and n.d.  (1) the witness points rebuilt from lambda / code (plus toi d for B) are the record's
    and lie at most tau apart; (2) the gap is positive; (3) n.d > 0, so with (2) the plane separates
    the hulls at every earlier time."""
    motion = np.asarray(motion, np.float64).reshape(-1, 3)
    width, gap, speed = np.zeros(len(idx)), np.zeros(len(idx)), np.zeros(len(idx))
    for t, k in enumerate(idx):
        r, d = rec[k], motion[k]
        A, B = pool.hull(int(pool.pairs[k, 0])), pool.hull(int(pool.pairs[k, 1]))
        toi = float(r["toi"])
        assert r["flags"] == IMPACT and r["status"] == gjkepa.STATUS_OK and 0.0 < toi < 1.0, (k, r)
        n = int(r["n_simplex"])
        assert 1 <= n <= 3, (k, n)
        lam, code = r["lambda"], r["code"]
        assert (lam >= 0).all() and (lam[n:] == 0).all() and (code[n:] == 0xFFFFFFFF).all(), (k, lam, code)
        assert abs(lam.sum() - 1.0) <= 1e-12, (k, lam)
        ia, ib = (code[:n] & 0xFFFF).astype(np.int64), (code[:n] >> 16).astype(np.int64)
        assert (ia < len(A)).all() and (ib < len(B)).all(), (k, code)
        pa, pb = lam[:n] @ A[ia], lam[:n] @ B[ib] + toi * d
        ptol = 1e-12 * (1.0 + max(np.abs(A).max(), np.abs(B).max() + np.abs(d).max()))
        assert np.abs(pa - r["point_a"]).max() <= ptol and np.abs(pb - r["point_b"]).max() <= ptol, (k, pa, pb, r)
        width[t] = float(np.linalg.norm(r["point_a"] - r["point_b"]))
        assert width[t] <= tau + dr.tol(tau), (k, width[t], tau)
        nrm = r["normal"]
        assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-12, (k, nrm)
        speed[t] = float(nrm @ d)
        gap[t] = float((A @ nrm).min() - (B @ nrm).max() - toi * speed[t])
        assert gap[t] > 0.0, (k, gap[t])
        assert speed[t] > 0.0, (k, speed[t])
    if len(idx):
        print(f"cast certificate over {len(idx)} impacts at tau {tau:g}: width / tau in [{(width / tau).min():.4f}, "
              f"{(width / tau).max():.4f}], smallest gap / tau {(gap / tau).min():.4f}, smallest n.d {speed.min():.3e}")
    return width, gap, speed


def check_miss_certificate(pool, motion, rec, idx):
    """a MISS record's normal is that of a plane which still separates the hulls at t = 1"""
    motion = np.asarray(motion, np.float64).reshape(-1, 3)
    for k in idx:
        r, d = rec[k], motion[k]
        A, B = pool.hull(int(pool.pairs[k, 0])), pool.hull(int(pool.pairs[k, 1]))
        assert r["flags"] == 0 and r["status"] == gjkepa.STATUS_OK and r["toi"] == 1.0 and r["n_simplex"] == 0, (k, r)
        nrm = r["normal"]
        assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-12, (k, nrm)
        assert (A @ nrm).min() - (B @ nrm).max() - nrm @ d > 0.0, (k, r)


def kinds(rec):
    """boolean masks of a batch's records: impact, miss, start, overlapping start"""
    ok = rec["status"] == gjkepa.STATUS_OK
    impact = ok & (rec["flags"] == IMPACT)
    miss = ok & (rec["flags"] == 0)
    start = ok & (rec["flags"] == START)
    return impact, miss, start, start & (rec["n_simplex"] == 0)


def check_pool(pool, motion, rec, tau, ref, hit, swept_dist_of):
    """Every check the issue sets for a pool's records, for the host program and the GPU alike.
    ref: Reference of (pool, motion); hit: the oracle's collision flags; swept_dist_of(idx): distance of
    hull A and the swept hull of B for the pairs idx.  Returns the masks of kinds()."""
    impact, miss, start, start_overlap = kinds(rec)
    assert (rec["status"] == gjkepa.STATUS_OK).all(), np.unique(rec["status"])      # no CAST_MAXITER, no bad input
    assert (impact | miss | start).all()
    assert rec["steps"].max() <= 32 and (rec["reserved"] == 0).all()
    assert impact.sum() >= 30 and miss.sum() >= 15, (impact.sum(), miss.sum())
    assert np.array_equal(start_overlap, hit)
    ii = np.nonzero(impact)[0]
    check_cast_certificate(pool, motion, rec, ii, tau)
    check_miss_certificate(pool, motion, rec, np.nonzero(miss)[0])
    # the reference distance at toi lies in [tau / 2, tau]
    f_toi = ref.f(np.where(impact, rec["toi"], 0.0))[ii]
    print(f"reference distance at toi / tau in [{(f_toi / tau).min():.6f}, {(f_toi / tau).max():.6f}]")
    assert (f_toi <= tau + dr.tol(tau)).all() and (f_toi >= 0.5 * tau - dr.tol(tau)).all()
    # the reference first comes within tau no later than toi
    before, fmin = ref.first_within(tau, hint=np.where(impact, rec["toi"], 0.5))
    assert np.isfinite(before[ii]).all()
    assert (before[ii] <= rec["toi"][ii] + dr.tol(rec["toi"][ii])).all()
    # a separated START is within tau at t = 0
    ss = np.nonzero(start & ~start_overlap)[0]
    if len(ss):
        assert (ref.f(np.zeros(pool.n_pairs))[ss] <= tau + dr.tol(tau)).all()
    # MISS against the swept hull of B, where that hull fits (2 n_b <= 256)
    nb = pool.hull_cnt[pool.pairs[:, 1]]
    sw = np.nonzero(2 * nb <= gjkepa.MAX_HULL_VERTS)[0]
    sd = swept_dist_of(sw)
    clear = sd > tau * (1 + 1e-6) + 1e-9
    close = sd < 0.5 * tau * (1 - 1e-6) - 1e-9
    assert miss[sw][clear].all(), np.nonzero(~miss[sw] & clear)
    assert not miss[sw][close].any(), np.nonzero(miss[sw] & close)
    print(f"{pool.n_pairs} pairs at tau {tau:g}: {impact.sum()} impacts, {miss.sum()} misses, {start.sum()} starts "
          f"({start_overlap.sum()} overlapping); steps mean {rec['steps'][impact].mean():.2f} max {rec['steps'].max()}, "
          f"iters mean {rec['iters'][impact].mean():.2f} max {rec['iters'].max()}; swept check on {len(sw)} pairs "
          f"({clear.sum()} clear, {close.sum()} close)")
    return impact, miss, start, start_overlap


def check_boundary(pool, motion, rec, ref, tau):
    """the checks of the tier-boundary pool (tests/test_distance.py boundary_pool) with hull B moved onto
    hull A's centre"""
    impact, miss, start, _ = kinds(rec)
    assert (rec["status"] == gjkepa.STATUS_OK).all() and (impact | miss).all()
    _, fmin = ref.argmin()
    assert impact[fmin < 0.5 * tau * (1 - 1e-6) - 1e-9].all() and miss[fmin > tau * (1 + 1e-6) + 1e-9].all()
    cnt = pool.hull_cnt[pool.pairs]
    assert impact[(cnt >= 32).all(axis=1)].all()                    # both hulls enclose their centre
    assert impact[(cnt == [8, 256]).all(axis=1)].all() and (cnt == [8, 256]).all(axis=1).any()
    ii = np.nonzero(impact)[0]
    assert len(ii) >= 60
    check_cast_certificate(pool, motion, rec, ii, tau)
    check_miss_certificate(pool, motion, rec, np.nonzero(miss)[0])
    f_toi = ref.f(np.where(impact, rec["toi"], 0.0))[ii]
    assert (f_toi <= tau + dr.tol(tau)).all() and (f_toi >= 0.5 * tau - dr.tol(tau)).all()
    print(f"boundary pool: {len(ii)} impacts of {pool.n_pairs}, steps max {rec['steps'].max()}, iters max {rec['iters'].max()}")


def swept_distance(dist_host, ref):
    def of(idx):
        if len(idx) == 0:
            return np.zeros(0)
        r = dist_host(ref.mv.swept(idx))
        assert (r["status"] == gjkepa.STATUS_OK).all()
        return np.where((r["flags"] & gjkepa.DIST_OVERLAP) != 0, 0.0, r["distance"])
    return of
