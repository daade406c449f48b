"""Shared helpers of the contact-manifold tests (tests/test_manifold_host.py on the CPU,
tests/test_manifold.py on the GPU): the pools, a numpy reference that is independent of
csrc/manifold_clip.h (features recomputed from the record's normal, monotone-chain hulls, float
Sutherland-Hodgman clipping), the checks every computed record must pass, and the builder of the host
program tests/manifold_host.cpp.

The reference shares with the definition (include/gjkepa.h) only what is part of it: the feature rule
with its margin and decimation, and the plane frame, because the scale s of every tolerance is the
largest 2-D coordinate in that frame."""
import os
import subprocess

import numpy as np

import gjkepa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_HIT, DECIMATED, FALLBACK = gjkepa.MANIFOLD_NO_HIT, gjkepa.MANIFOLD_DECIMATED, gjkepa.MANIFOLD_FALLBACK
MARGIN = 1e-6
EPS = 1e-9          # the definition's tolerance, in units of s


# ---------------------------------------------------------------- the host program
def build_manifold_host(tmpdir, extra_flags=()):
    """tests/manifold_host.cpp (csrc/manifold_clip.h over a plain scan) as a program of its own; returns
    run(pool, records, margin) -> MANIFOLD64 records."""
    exe = os.path.join(str(tmpdir), "manifold_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra_flags,
                    os.path.join(ROOT, "tests", "manifold_host.cpp"), "-o", exe], check=True)
    count = [0]

    def run(pool, records, margin):
        count[0] += 1
        fin = os.path.join(str(tmpdir), f"in{count[0]}.bin")
        fout = os.path.join(str(tmpdir), f"out{count[0]}.bin")
        verts = np.ascontiguousarray(pool.verts)
        records = np.ascontiguousarray(records)
        assert records.dtype in (gjkepa.REC64, gjkepa.REC32) and records.shape == (pool.n_pairs,)
        prec = gjkepa.PREC_F64 if records.dtype == gjkepa.REC64 else gjkepa.PREC_F32
        with open(fin, "wb") as f:
            f.write(np.array([pool.dtype_code, verts.size, len(pool.hull_cnt), pool.n_pairs, prec], np.int64).tobytes())
            f.write(np.array([margin], np.float64).tobytes())
            f.write(verts.tobytes())
            f.write(np.ascontiguousarray(pool.hull_off, np.int64).tobytes())
            f.write(np.ascontiguousarray(pool.hull_cnt, np.int32).tobytes())
            f.write(np.ascontiguousarray(pool.pairs, np.int32).tobytes())
            f.write(records.tobytes())
        subprocess.run([exe, fin, fout], check=True)
        out = np.fromfile(fout, gjkepa.MANIFOLD64)
        os.remove(fin)
        os.remove(fout)
        assert out.shape == (pool.n_pairs,)
        return out
    return run


# ---------------------------------------------------------------- pools
def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def box(hx, hy, hz):
    return np.array([[x * hx, y * hy, z * hz] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], float)


def prism(k, radius=1.0, half=0.5):
    a = 2 * np.pi * np.arange(k) / k
    ring = np.stack([radius * np.cos(a), radius * np.sin(a)], 1)
    return np.concatenate([np.c_[ring, np.full(k, -half)], np.c_[ring, np.full(k, half)]])


def yaw_angle(rng):
    """uniform, but not within 1e-3 rad of a multiple of 90 degrees"""
    while True:
        y = rng.uniform(0, 2 * np.pi)
        if abs((y + np.pi / 4) % (np.pi / 2) - np.pi / 4) > 1e-3:
            return y


def stack(rng, lower, upper, yaw=None, tilt=None):
    """`upper` (centred on its own origin) yawed, tilted and set on top of `lower` with an offset of up to
    0.4 and a penetration of 0.001 to 0.02, the pair then turned by a random rotation"""
    yaw = yaw_angle(rng) if yaw is None else yaw
    if tilt is None:
        tilt = rng.uniform(0, 2e-7) if rng.random() < 0.5 else rng.uniform(0, 0.05)
    t_axis = rot([0, 0, 1], rng.uniform(0, 2 * np.pi)) @ [1, 0, 0]
    up = upper @ rot([0, 0, 1], yaw).T @ rot(t_axis, tilt).T
    up = up + [rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 0]
    up[:, 2] += lower[:, 2].max() - rng.uniform(0.001, 0.02) - up[:, 2].min()
    r, shift = random_rotation(rng), rng.uniform(-1, 1, 3)
    return lower @ r.T + shift, up @ r.T + shift


def box_pool(n=260, seed=0xB0C5):
    """rotated box stacks"""
    rng = np.random.default_rng(seed)
    return gjkepa.HullPool.from_pairs(
        [stack(rng, box(*rng.uniform(0.5, 1.0, 3)), box(*rng.uniform(0.5, 1.0, 3))) for _ in range(n)])


PRISM_K = (3, 16, 32, 33, 64, 128)


def prism_pool(seed=0x9215, reps=4):
    """k-gon prisms (2 k vertices: the 32 / 33 cap of a feature, DECIMATED, tiers 1 and 2), each on a box
    and on a slightly yawed copy of itself"""
    rng = np.random.default_rng(seed)
    prs = []
    for k in PRISM_K:
        for _ in range(reps):
            prs.append(stack(rng, box(0.8, 0.8, 0.5), prism(k)))
            prs.append(stack(rng, prism(k), prism(k), yaw=rng.uniform(0.01, 0.05)))
    return gjkepa.HullPool.from_pairs(prs)


BOUNDARY_SIZES = (1, 4, 32, 33, 128, 129, 256)


def tier_boundary_pool(seed=0x71E2):
    """hulls of every tier-edge size, one set about the origin and one about (0.2, 0.1, 0.05), in every
    combination: all but the pair of two points overlap.  Values are fp32-exact."""
    rng = np.random.default_rng(seed)
    tetra = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float) / np.sqrt(3.0)
    sets = []
    for centre in ((0.0, 0.0, 0.0), (0.2, 0.1, 0.05)):
        hulls = []
        for n in BOUNDARY_SIZES:
            if n == 1:
                h = np.zeros((1, 3))
            elif n == 4:
                h = tetra @ random_rotation(rng).T
            else:
                u = rng.normal(size=(n, 3))
                h = u / np.linalg.norm(u, axis=1, keepdims=True)
            hulls.append((h + centre).astype(np.float32).astype(np.float64))
        sets.append(hulls)
    return gjkepa.HullPool.from_pairs([(a, b) for a in sets[0] for b in sets[1]], dtype=np.float32)


SPHERE_POOLS = {"1-4": (1, 4, 6000, 0.6), "8-32": (8, 32, 300, 2.5), "33-256": (33, 256, 200, 2.5)}


def sphere_pool(name, seed=0x5EED):
    lo, hi, n, rmax = SPHERE_POOLS[name]
    return gjkepa.synth_pairs(seed, n, lo, hi, rmax)


CUBE = box(0.5, 0.5, 0.5) + 0.5          # the unit cube [0, 1]^3
D = 0.01                                 # penetration of the known answers


def known_answers():
    """name -> (hull A, hull B, expected number of points, expected points or None)"""
    rz45 = rot([0, 0, 1], np.pi / 4)
    c = CUBE - [0.5, 0.5, 0.0]            # unit cube centred on the z axis
    edge_down = (CUBE - 0.5) @ rot([0, 1, 0], np.pi / 4).T           # an edge along y lowest
    corner_down = (CUBE - 0.5) @ rot([1, -1, 0], np.arccos(1 / np.sqrt(3.0))).T   # a corner lowest
    rect = [[0.5, 0.25, 1], [1, 0.25, 1], [1, 1, 1], [0.5, 1, 1]]
    return {
        "offset cubes": (CUBE, CUBE + [0.5, 0.25, 1 - D], 4, rect),
        "aligned cubes": (CUBE, CUBE + [0, 0, 1 - D], 4, [[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]]),
        "45 degree yaw": (c, c @ rz45.T + [0, 0, 1 - D], 4, None),
        "edge on face": (box(2, 2, 0.5), edge_down + [0, 0, 0.5 + np.sqrt(0.5) - D], 2,
                         [[0, -0.5, 0.5], [0, 0.5, 0.5]]),
        "vertex on face": (box(2, 2, 0.5), corner_down + [0, 0, 0.5 + np.sqrt(0.75) - D], 1, [[0, 0, 0.5]]),
        "crossed edges": (edge_down @ rot([0, 0, 1], np.pi / 2).T @ rot([1, 0, 0], np.pi).T,
                          edge_down + [0, 0, 2 * np.sqrt(0.5) - D], 1, [[0, 0, np.sqrt(0.5)]]),
        "point in a box": (box(1, 1, 1), np.array([[0.2, 0.1, 0.97]]), 1, [[0.2, 0.1, 1.0]]),
    }


# ---------------------------------------------------------------- the reference
def cross2(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def monotone_chain(pts):
    """strict convex hull of 2-D points, counter-clockwise; returns indices into pts (1, 2 or >= 3)"""
    order = sorted(range(len(pts)), key=lambda i: (pts[i][0], pts[i][1], i))
    uniq = [order[0]]
    for i in order[1:]:
        if (pts[i] != pts[uniq[-1]]).any():
            uniq.append(i)
    if len(uniq) <= 2:
        return uniq

    def half(seq):
        h = []
        for i in seq:
            while len(h) >= 2 and cross2(pts[h[-1]] - pts[h[-2]], pts[i] - pts[h[-2]]) <= 0:
                h.pop()
            h.append(i)
        return h
    lower, upper = half(uniq), half(uniq[::-1])
    return lower[:-1] + upper[:-1]


def outside(poly, p):
    """how far the point p lies outside the convex footprint poly (1, 2 or >= 3 points, ccw): <= 0 inside"""
    poly = np.asarray(poly, float)
    if len(poly) == 1:
        return float(np.linalg.norm(p - poly[0]))
    if len(poly) == 2:
        e = poly[1] - poly[0]
        t = np.clip((p - poly[0]) @ e / (e @ e), 0, 1)
        return float(np.linalg.norm(p - (poly[0] + t * e)))
    e = np.roll(poly, -1, 0) - poly
    return float((-cross2(e, p - poly) / np.linalg.norm(e, axis=1)).max())


def clip(subject, clipper, eps):
    """Sutherland-Hodgman: the part of the convex `subject` (1, 2 or >= 3 points) inside the polygon
    `clipper` (>= 3 points, ccw), a point counting as inside up to eps beyond an edge"""
    out = [np.asarray(p, float) for p in subject]
    m = len(clipper)
    for i in range(m):
        c0, c1 = clipper[i], clipper[(i + 1) % m]
        e = c1 - c0
        le = np.linalg.norm(e)
        src, out = out, []
        if not src:
            break
        dist = [cross2(e, p - c0) / le for p in src]
        for j, cur in enumerate(src):
            prev, dp, dc = src[j - 1], dist[j - 1], dist[j]
            if dc >= -eps:
                if dp < -eps:
                    out.append(prev + (cur - prev) * (dp / (dp - dc)))
                out.append(cur)
            elif dp >= -eps and len(src) > 1:
                out.append(prev + (cur - prev) * (dp / (dp - dc)))
    return out


def intersect(pa, pb, eps):
    """the intersection of two convex footprints as a list of 2-D points (its polygon, segment or point)"""
    if len(pb) >= 3:
        return clip(pa, pb, eps)
    if len(pa) >= 3:
        return clip(pb, pa, eps)
    if len(pa) == 1:
        return [pa[0]] if outside(pb, pa[0]) <= eps else []
    if len(pb) == 1:
        return [pb[0]] if outside(pa, pb[0]) <= eps else []
    r, q = pa[1] - pa[0], pb[1] - pb[0]
    den = cross2(r, q)
    if abs(den) > EPS * np.linalg.norm(r) * np.linalg.norm(q):
        t = cross2(pb[0] - pa[0], q) / den
        p = pa[0] + t * r
        return [p] if outside(pa, p) <= eps and outside(pb, p) <= eps else []
    ends = [p for p in pb if outside(pa, p) <= eps] + [p for p in pa if outside(pb, p) <= eps]
    return ends


def merged(poly, tol):
    """the polygon's vertices with runs closer than tol (cyclically) merged into their first"""
    keep = []
    for p in poly:
        if not any(np.linalg.norm(p - q) < tol for q in keep):
            keep.append(p)
    return keep


def shoelace(poly):
    if len(poly) < 3:
        return 0.0
    p = np.asarray(poly, float)
    return 0.5 * float(np.sum(cross2(p, np.roll(p, -1, 0))))


def plane_frame(n):
    e = np.zeros(3)
    e[int(np.argmin(np.abs(n)))] = 1.0            # argmin: the first of equals
    u = np.cross(e, n)
    u /= np.linalg.norm(u)
    return u, np.cross(n, u)


def decimate(idx):
    step = -(-len(idx) // gjkepa.MANIFOLD_MAX_FEATURE) if len(idx) > gjkepa.MANIFOLD_MAX_FEATURE else 1
    return idx[::step]


class PairRef:
    """the reference for one computed pair"""

    def __init__(self, A, B, n, margin):
        self.A, self.B, self.n = A, B, n
        ha, hb = A @ n, B @ n
        self.hA, self.hB = float(ha.max()), float(hb.min())
        self.FA = np.nonzero(ha >= self.hA - margin)[0]
        self.FB = np.nonzero(hb <= self.hB + margin)[0]
        self.near_threshold = bool((np.abs(ha - (self.hA - margin)) < 1e-9).any() or
                                   (np.abs(hb - (self.hB + margin)) < 1e-9).any())
        self.u, self.w = plane_frame(n)
        self.o = A[self.FA[0]]
        self.mag = 1.0 + max(np.abs(A).max(), np.abs(B).max())
        pa, pb = self.to2(A[self.FA]), self.to2(B[self.FB])
        self.s = float(max(np.abs(pa).max(), np.abs(pb).max()))
        # the footprints of the whole features (what a reported point must lie in) ...
        self.foot_a = pa[monotone_chain(pa)]
        self.foot_b = pb[monotone_chain(pb)]
        # ... and of the vertices the definition uses, as vertex indices (what a code refers to)
        ua, ub = decimate(self.FA), decimate(self.FB)
        self.used_a = ua[monotone_chain(self.to2(A[ua]))]
        self.used_b = ub[monotone_chain(self.to2(B[ub]))]
        self.poly = intersect(list(self.foot_a), list(self.foot_b), EPS * self.s)
        tiny = merged(self.poly, 1e-12 * self.s)
        edges = [np.linalg.norm(tiny[i] - tiny[i - 1]) for i in range(len(tiny))] if len(tiny) > 1 else []
        self.short_edge = any(e < 1e-6 * self.s for e in edges)
        self.verts = merged(self.poly, 1e-6 * self.s)
        self.area = shoelace(self.poly)
        self.perimeter = float(sum(np.linalg.norm(self.poly[i] - self.poly[i - 1]) for i in range(len(self.poly)))) \
            if len(self.poly) > 1 else 0.0

    def to2(self, p):
        d = np.asarray(p, float) - self.o
        return np.stack([d @ self.u, d @ self.w], -1)

    def project(self, v):
        """v moved along n onto hull A's support plane"""
        return v + (self.hA - v @ self.n) / (self.n @ self.n) * self.n


def is_computed(contact):
    n = contact["collision_normal"].astype(np.float64)
    return (contact["collision"] != 0) & (contact["status"] == gjkepa.STATUS_OK) & np.isfinite(n).all(1) & (n != 0).any(1)


def check_record(r, ref, k):
    """checks 1 to 6 on one computed record against its reference; returns its area"""
    npt = int(r["n_points"])
    assert 1 <= npt <= 4, (k, npt)                                                           # 1
    pts, code = r["point"][:npt], r["code"]
    assert (r["point"][npt:] == 0).all() and (code[npt:] == 0xFFFFFFFF).all(), (k, r)
    ptol = 1e-12 * ref.mag
    assert np.abs(pts @ ref.n - ref.hA).max() <= ptol, (k, pts @ ref.n - ref.hA)              # 2
    assert abs(r["depth"] - (ref.hA - ref.hB)) <= ptol, (k, r["depth"], ref.hA - ref.hB)     # 3
    assert (r["normal"] == ref.n).all()
    assert r["n_feat_a"] == len(ref.FA) and r["n_feat_b"] == len(ref.FB), (k, r, len(ref.FA), len(ref.FB))
    assert bool(r["flags"] & DECIMATED) == (max(len(ref.FA), len(ref.FB)) > gjkepa.MANIFOLD_MAX_FEATURE), (k, r)
    p2 = ref.to2(pts)
    area = shoelace(p2)                                                                      # 4
    # eps = 1.1e-16 over the ~100 operations from the record's coordinates to a 2-D area
    assert abs(r["area"] - area) <= 1e-13 * ref.mag ** 2, (k, r["area"], area)
    if npt >= 3:
        e = np.roll(p2, -1, 0) - p2
        assert (cross2(e, np.roll(e, -1, 0)) > 0).all(), (k, p2)
    else:
        assert r["area"] == 0
    if r["flags"] & FALLBACK:
        assert npt == 1 and code[0] == 0xFFFFFFFF, (k, r)
        return area
    s = ref.s
    for p in p2:                                                                             # 5
        assert outside(ref.foot_a, p) <= 2 * EPS * s and outside(ref.foot_b, p) <= 2 * EPS * s, \
            (k, p, outside(ref.foot_a, p) / s, outside(ref.foot_b, p) / s)
    for p, q, c in zip(pts, p2, code[:npt]):                                                 # 6
        ia, ib = int(c & 0xFFFF), int(c >> 16)
        assert (ia != 0xFFFF or ib != 0xFFFF), (k, c)
        if ib == 0xFFFF:
            assert ia in ref.used_a and np.abs(ref.project(ref.A[ia]) - p).max() <= ptol, (k, c, p)
        elif ia == 0xFFFF:
            assert ib in ref.used_b and np.abs(ref.project(ref.B[ib]) - p).max() <= ptol, (k, c, p)
        else:
            for hull, used, i in ((ref.A, ref.used_a, ia), (ref.B, ref.used_b, ib)):
                assert i in used and len(used) >= 2, (k, c)
                at = list(used).index(i)
                e0, e1 = ref.to2(hull[i]), ref.to2(hull[used[(at + 1) % len(used)]])
                off = abs(cross2(e1 - e0, q - e0)) / np.linalg.norm(e1 - e0)
                assert off <= 2 * EPS * s, (k, c, off / s)
    return area


def check_pool(pool, contact, rec, margin=MARGIN, name="pool", min_hits=30, oracle_depth=True):
    """Every check the definition sets for a pool's records (host program and GPU alike).  contact: the
    pool's contact records; rec: its manifold records.  Returns (computed mask, n_points histogram)."""
    comp = is_computed(contact)
    assert rec.dtype == gjkepa.MANIFOLD64 and rec.shape == (pool.n_pairs,)
    assert np.array_equal((rec["flags"] & NO_HIT) != 0, ~comp)                 # NO_HIT <=> not a usable collision
    no = rec[~comp]
    assert (no["status"] == gjkepa.STATUS_OK).all() and (no["n_points"] == 0).all() and (no["flags"] == NO_HIT).all()
    assert (no["point"] == 0).all() and (no["depth"] == 0).all() and (no["normal"] == 0).all() and (no["area"] == 0).all()
    assert (no["code"] == 0xFFFFFFFF).all() and (no["n_feat_a"] == 0).all() and (no["n_feat_b"] == 0).all()
    assert (rec["status"] == gjkepa.STATUS_OK).all() and (rec["reserved"] == 0).all()
    hits = np.nonzero(comp)[0]
    assert len(hits) >= min_hits, (name, len(hits))
    excluded, fallback, ratio, depth_err = 0, 0, np.inf, 0.0
    for k in hits:
        r = rec[k]
        A, B = pool.hull(int(pool.pairs[k, 0])), pool.hull(int(pool.pairs[k, 1]))
        ref = PairRef(A, B, contact["collision_normal"][k].astype(np.float64), margin)
        depth_err = max(depth_err, abs(float(r["depth"]) - float(contact["penetration_depth"][k])))      # 8: reported
        if r["flags"] & FALLBACK:
            fallback += 1
        if ref.near_threshold or ref.short_edge:
            excluded += 1
            npt = int(r["n_points"])
            assert 1 <= npt <= 4 and np.abs(r["point"][:npt] @ ref.n - ref.hA).max() <= 1e-12 * ref.mag, (k, r)
            continue
        area = check_record(r, ref, k)
        if r["flags"] & FALLBACK:
            continue
        nv, npt = len(ref.verts), int(r["n_points"])                                                     # 7
        assert nv >= 1, (k, "the reference finds no intersection", r)
        if nv <= 4:
            assert npt == nv, (k, npt, nv, ref.verts, r)
            assert area >= ref.area - 4 * EPS * ref.s * ref.perimeter, (k, area, ref.area)
        else:
            assert npt == 4, (k, npt, nv)
            assert area >= 0.25 * ref.area, (k, area, ref.area)
        if ref.area > 0 and nv >= 3:
            ratio = min(ratio, area / ref.area)
    hist = np.bincount(rec["n_points"][comp], minlength=5)
    print(f"{name}: {len(hits)} computed of {pool.n_pairs}, n_points 1/2/3/4 = {hist[1]}/{hist[2]}/{hist[3]}/{hist[4]}, "
          f"excluded {excluded}, fallback {fallback}, decimated {int(((rec['flags'] & DECIMATED) != 0).sum())}, "
          f"smallest area / reference area {ratio:.6f}, largest |depth - penetration_depth| {depth_err:.3e}")
    assert excluded <= 0.02 * len(hits), (name, excluded, len(hits))
    assert fallback <= 0.01 * len(hits), (name, fallback, len(hits))
    return comp, hist


def check_boundary_cover(pool, comp):
    """the tier-boundary pool's computed pairs take in every hull size on either side (two points never
    collide, and a point inside a tetrahedron may be called a miss)"""
    cnt = pool.hull_cnt[pool.pairs]
    assert not comp[(cnt == 1).all(1)].any()
    for n in BOUNDARY_SIZES:
        assert comp[cnt[:, 0] == n].any() and comp[cnt[:, 1] == n].any(), n
    assert comp[(cnt >= 32).all(1)].all()


def check_known(rec, names, answers):
    """the known answers: the number of points, and the points themselves where they are listed"""
    for r, name in zip(rec, names):
        _, _, npt, want = answers[name]
        assert r["flags"] == 0 and r["status"] == gjkepa.STATUS_OK and r["n_points"] == npt, (name, r)
        if want is not None:
            got = r["point"][:npt]
            want = np.asarray(want, float)
            for w in want:
                assert np.abs(got - w).max(1).min() <= 1e-9, (name, w, got)
    r = rec[names.index("45 degree yaw")]
    rad = np.linalg.norm(r["point"][:4, :2], axis=1)                # the octagon's vertices: 0.5 / cos(22.5 deg) from the axis
    assert np.abs(rad - 0.5 / np.cos(np.pi / 8)).max() <= 1e-9 and abs(r["area"] - 2 * rad[0] ** 2) <= 1e-9, r
