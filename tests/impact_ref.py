"""Shared helpers of the tests of the contact manifold at the time of impact
(tests/test_manifold_cast_host.py on the CPU, tests/test_manifold_cast.py on the GPU): the builder of the host
program tests/impact_host.cpp, the pools with their motions, the known answers, and a numpy reference for a
computed record that is independent of csrc/manifold_clip.h and csrc/rigid_pose.h: the hulls posed by
cast_rigid_ref.pose (the rotation matrix of the normalised quaternion), then manifold_ref's features by the
rule, monotone-chain footprints, Sutherland-Hodgman clip and shoelace (manifold_ref.PairRef)."""
import ctypes
import os
import subprocess

import numpy as np

import cast_rigid_ref as rr
import gjkepa
import manifold_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 1e-3
MARGIN = mr.MARGIN
AT_TOI, NO_HIT, FALLBACK = gjkepa.MANIFOLD_AT_TOI, gjkepa.MANIFOLD_NO_HIT, gjkepa.MANIFOLD_FALLBACK
# The largest distance, over the known answers, between a reported point and the vertex the numpy pose puts
# there (projected onto z = hA), measured on the host program; the tests bound it at 16 times this.
POSITION_MEASURED = 7.1e-12
POSITION_BOUND = 16 * POSITION_MEASURED


# ---------------------------------------------------------------- the host program
def build_impact_host(tmpdir, extra_flags=()):
    """tests/impact_host.cpp as a shared library; returns run(pool, body_motion, cast, margin, records=None)
    -> MANIFOLD64 records."""
    so = os.path.join(str(tmpdir), "libimpact_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", *extra_flags,
                    os.path.join(ROOT, "tests", "impact_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.impact_host_batch.argtypes = [ctypes.c_int, vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int, ctypes.c_double, vp]

    def run(pool, body_motion, cast, margin, records=None):
        out = np.zeros(pool.n_pairs, gjkepa.MANIFOLD64)
        verts = np.ascontiguousarray(pool.verts)
        off = np.ascontiguousarray(pool.hull_off, np.int64)
        cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
        prs = np.ascontiguousarray(pool.pairs, np.int32).reshape(-1)
        mot = np.ascontiguousarray(body_motion, np.float64).reshape(-1)
        cast = np.ascontiguousarray(cast)
        assert mot.size == 9 * cnt.size and cast.dtype == gjkepa.CAST64 and cast.shape == (pool.n_pairs,)
        prec = gjkepa.PREC_F64
        if records is not None:
            records = np.ascontiguousarray(records)
            assert records.dtype in (gjkepa.REC64, gjkepa.REC32) and records.shape == (pool.n_pairs,)
            prec = gjkepa.PREC_F64 if records.dtype == gjkepa.REC64 else gjkepa.PREC_F32
        assert lib.impact_host_batch(pool.dtype_code, verts.ctypes.data, off.ctypes.data, cnt.ctypes.data, prs.ctypes.data,
                                     pool.n_pairs, mot.ctypes.data, cast.ctypes.data,
                                     None if records is None else records.ctypes.data, prec, float(margin),
                                     out.ctypes.data) == 0
        return out
    return run


def skipped(n=1):
    """the record a cast leaves for a pair it skipped as a hit"""
    r = np.zeros(n, gjkepa.CAST64)
    r["code"] = 0xFFFFFFFF
    r["flags"] = gjkepa.CAST_SKIPPED
    return r


def skip_hits(cast, contact):
    """the cast records a cast given `contact` as its records leaves: the pairs with the collision byte SKIPPED"""
    out = cast.copy()
    hit = contact["collision"] != 0
    out[hit] = skipped(int(hit.sum()))
    return out


# ---------------------------------------------------------------- pools
def lifted_box_pool(n=320, seed=0x1A9D):
    """manifold_ref.stack's rotated box stacks with the upper box lifted off the lower one along the stack's
    axis to a gap of 2 tau to 0.3, and body motions from cast_rigid_ref.motions (closing, with spin).  Every
    second pair lands flat: its linear motion is kept along the axis only and both spins are turned onto the
    axis (a yaw about the contact normal), so the stacks of manifold_ref's small tilts meet face to face.
    Returns (pool, body_motion)."""
    rng = np.random.default_rng(seed)
    prs, axes = [], []
    for _ in range(n):
        a, b = mr.stack(rng, mr.box(*rng.uniform(0.5, 1.0, 3)), mr.box(*rng.uniform(0.5, 1.0, 3)))
        axis = a[4:].mean(0) - a[:4].mean(0)              # manifold_ref.box lists the z = -hz face first
        axis /= np.linalg.norm(axis)
        gap = (b @ axis).min() - (a @ axis).max()         # negative: the stack's penetration
        prs.append((a, b + (rng.uniform(2 * TAU, 0.3) - gap) * axis))
        axes.append(axis)
    pool = gjkepa.HullPool.from_pairs(prs)
    bm = rr.motions(pool, seed ^ 0xC105)
    for k in range(0, n, 2):
        ha, hb = pool.pairs[k]
        for h in (ha, hb):
            bm[h, 0:3] = (bm[h, 0:3] @ axes[k]) * axes[k]
            bm[h, 3:6] = (bm[h, 3:6] @ axes[k]) * axes[k]
    return pool, bm


def boundary_pool():
    """manifold_ref.tier_boundary_pool's hulls (sizes 1, 4, 32, 33, 128, 129, 256, fp32 storage), the second set
    moved out to (3, 0.5, 0.25) where cast_rigid_ref.boundary_motions expects it.  Returns (pool, body_motion)."""
    src = mr.tier_boundary_pool()
    shift = np.array([3.0, 0.5, 0.25]) - np.array([0.2, 0.1, 0.05])
    prs = [(src.hull(int(a)), (src.hull(int(b)) + shift).astype(np.float32).astype(np.float64)) for a, b in src.pairs]
    pool = gjkepa.HullPool.from_pairs(prs, dtype=np.float32)
    return pool, rr.boundary_motions(pool)


FALL = [0.0, 0.0, -1.0]


def known_cases():
    """name -> (hull B, motion of B, expected number of points, expected area or None, indices of the vertices
    of B that touch).  Hull A is cast_rigid_ref.SLAB at rest, its top face z = 0; every B starts 0.3 above it."""
    cube = rr.CUBE + [-0.5, -0.5, 0.3]
    edge = (rr.CUBE - 0.5) @ mr.rot([0, 1, 0], np.pi / 4).T + [0, 0, np.sqrt(0.5) + 0.3]
    corner = (rr.CUBE - 0.5) @ mr.rot([1, -1, 0], np.arccos(1 / np.sqrt(3.0))).T + [0, 0, np.sqrt(0.75) + 0.3]
    bar = rr.BAR + [0, 0, -0.2]                                # both ends at z = 0.3

    def lowest(h, tol=1e-9):
        return np.nonzero(h[:, 2] <= h[:, 2].min() + tol)[0]
    return {
        "cube falling flat": (cube, FALL + [0, 0, 0] + [0, 0, 0.8], 4, 1.0, lowest(cube)),
        "cube falling while yawing": (cube, FALL + [0, 0, 0.8] + [0, 0, 0.8], 4, 1.0, lowest(cube)),
        "cube on an edge": (edge, FALL + [0, 0, 0] + list(edge.mean(0)), 2, None, lowest(edge)),
        "cube on a corner": (corner, FALL + [0, 0, 0] + list(corner.mean(0)), 1, None, lowest(corner)),
        "bar falling": (bar, FALL + [0, 0, 0] + [0, 0, 0.3], 2, None, np.array([0, 1])),
        # the end at x = +1 comes down as the bar turns about +y through its centre, 0.5 above the slab
        "bar cartwheeling": (rr.BAR, [0, 0, 0, 0, 1.2, 0, 0, 0, 0.5], 1, None, np.array([1])),
    }


def known_pool():
    cases = known_cases()
    pool = gjkepa.HullPool.from_pairs([(rr.SLAB, c[0]) for c in cases.values()])
    bm = np.array([m for c in cases.values() for m in (rr.STILL + [0, 0, -0.5], c[1])], float)
    return cases, pool, bm


def check_known(rec, cast, cases, bm):
    """the known answers; returns the largest position error: reported point against the touching vertex as the
    numpy pose gives it at toi, projected onto z = hA"""
    worst = 0.0
    for k, (name, (hull, _, npt, area, touch)) in enumerate(cases.items()):
        r, c = rec[k], cast[k]
        assert c["flags"] == gjkepa.CAST_IMPACT and c["status"] == gjkepa.STATUS_OK, (name, c)
        assert r["status"] == gjkepa.STATUS_OK and r["flags"] == AT_TOI and r["n_points"] == npt, (name, r)
        assert -TAU <= r["depth"] < 0.0, (name, r["depth"])
        assert (r["normal"] == -c["normal"]).all(), (name, r["normal"], c["normal"])
        if area is not None:
            assert abs(r["area"] - area) <= 1e-12, (name, r["area"])
        posed = rr.pose(hull, bm[2 * k + 1], float(c["toi"]))[touch]
        assert len(posed) == npt, (name, touch)
        hA = 0.0
        want = np.c_[posed[:, :2], np.full(npt, hA)]
        got = r["point"][:npt]
        err = max(float(np.linalg.norm(got - w, axis=1).min()) for w in want)
        codes = sorted(int(x) for x in r["code"][:npt])
        assert codes == sorted(0xFFFF | (int(i) << 16) for i in touch), (name, [hex(x) for x in codes])
        print(f"{name}: toi {c['toi']:.9f} depth {r['depth']:.3e} points {npt} position error {err:.3e}")
        worst = max(worst, err)
    return worst


# ---------------------------------------------------------------- the reference and the checks
def computed_mask(cast):
    """rule 5 on records with valid hulls, motions and times"""
    n = cast["normal"]
    return ((cast["flags"] & gjkepa.CAST_SKIPPED) == 0) & (cast["status"] == gjkepa.STATUS_OK) & \
        ((cast["flags"] & (gjkepa.CAST_IMPACT | gjkepa.CAST_START)) != 0) & np.isfinite(n).all(1) & (n != 0).any(1)


def check_empty(rec, status, flags):
    assert (rec["status"] == status).all() and (rec["flags"] == flags).all() and (rec["n_points"] == 0).all(), rec
    assert (rec["point"] == 0).all() and (rec["depth"] == 0).all() and (rec["normal"] == 0).all() and (rec["area"] == 0).all()
    assert (rec["code"] == 0xFFFFFFFF).all() and (rec["n_feat_a"] == 0).all() and (rec["n_feat_b"] == 0).all()
    assert (rec["reserved"] == 0).all()


def check_pool(pool, bm, cast, rec, margin=MARGIN, name="pool"):
    """Every check on the records of a pool whose cast records hold no SKIPPED pair: NO_HIT exactly where rule 5
    does not compute, and for every computed record, against the hulls posed by the numpy pose at its toi: points
    on A's support plane and inside both footprints within 1e-9 s, counter-clockwise and convex, codes naming
    feature vertices, depth = hA - hB, and an area of at least a quarter of the reference polygon's
    (manifold_ref.check_record and the area rule of manifold_ref.check_pool).  Returns (computed mask, n_points
    histogram of the computed IMPACT records)."""
    bm = np.asarray(bm, float).reshape(-1, 9)
    comp = computed_mask(cast)
    assert rec.dtype == gjkepa.MANIFOLD64 and rec.shape == (pool.n_pairs,)
    assert not (cast["flags"] & gjkepa.CAST_SKIPPED).any()
    check_empty(rec[~comp], gjkepa.STATUS_OK, NO_HIT)
    assert (rec["status"] == gjkepa.STATUS_OK).all()
    assert ((rec["flags"][comp] & AT_TOI) != 0).all() and ((rec["flags"][comp] & NO_HIT) == 0).all()
    excluded, fallback, ratio = 0, 0, np.inf
    for k in np.nonzero(comp)[0]:
        r, c = rec[k], cast[k]
        ha, hb = (int(x) for x in pool.pairs[k])
        A, B = rr.pose(pool.hull(ha), bm[ha], float(c["toi"])), rr.pose(pool.hull(hb), bm[hb], float(c["toi"]))
        ref = mr.PairRef(A, B, -c["normal"], margin)
        assert (r["normal"] == ref.n).all(), (k, r["normal"], c["normal"])
        if r["flags"] & FALLBACK:
            fallback += 1
        # every in-plane tolerance is relative to s: two features that are one point each (two single-vertex hulls
        # passing within tau) have an s that is the rounding of their coordinates, and nothing in-plane to check
        if ref.near_threshold or ref.short_edge or ref.s <= 1e-9 * ref.mag:
            excluded += 1
            npt = int(r["n_points"])
            assert 1 <= npt <= 4 and np.abs(r["point"][:npt] @ ref.n - ref.hA).max() <= 1e-12 * ref.mag, (k, r)
            continue
        area = mr.check_record(r, ref, k)              # plane, depth, orientation, footprints (2e-9 s), codes
        if r["flags"] & FALLBACK:
            continue
        for p in ref.to2(r["point"][:int(r["n_points"])]):
            assert mr.outside(ref.foot_a, p) <= mr.EPS * ref.s and mr.outside(ref.foot_b, p) <= mr.EPS * ref.s, \
                (k, p, mr.outside(ref.foot_a, p) / ref.s, mr.outside(ref.foot_b, p) / ref.s)
        nv, npt = len(ref.verts), int(r["n_points"])
        assert nv >= 1, (k, "the reference finds no intersection", r)
        if nv <= 4:
            assert npt == nv, (k, npt, nv, ref.verts, r)
            assert area >= ref.area - 4 * mr.EPS * ref.s * ref.perimeter, (k, area, ref.area)
        else:
            assert npt == 4, (k, npt, nv)
        assert area >= 0.25 * ref.area, (k, area, ref.area)
        if ref.area > 0 and nv >= 3:
            ratio = min(ratio, area / ref.area)
    impact = comp & ((cast["flags"] & gjkepa.CAST_IMPACT) != 0)
    hist = np.bincount(rec["n_points"][impact], minlength=5)
    stopped = int((cast["status"] == gjkepa.STATUS_CAST_MAXITER).sum())
    print(f"{name}: {int(comp.sum())} computed of {pool.n_pairs} ({int(impact.sum())} impacts), n_points 1/2/3/4 = "
          f"{hist[1]}/{hist[2]}/{hist[3]}/{hist[4]}, excluded {excluded}, fallback {fallback}, undecided {stopped}, "
          f"smallest area / reference area {ratio:.6f}")
    assert excluded <= 0.02 * max(int(comp.sum()), 50), (name, excluded)
    assert fallback <= 0.01 * max(int(comp.sum()), 100), (name, fallback)
    assert stopped <= rr.MAXITER_SHARE * pool.n_pairs, (name, stopped)
    return comp, hist


def check_brackets(pool, comp):
    """the computed pairs take in every tier bracket of the larger hull: up to 32, 33 to 128, above"""
    nmax = pool.hull_cnt[pool.pairs].max(1)
    for lo, hi in ((0, 32), (32, 128), (128, 256)):
        assert comp[(nmax > lo) & (nmax <= hi)].any(), (lo, hi)
    for n in mr.BOUNDARY_SIZES[1:]:
        assert comp[nmax == n].any(), n
