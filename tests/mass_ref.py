"""Shared helpers of the mass-property tests (tests/test_mass_host.py on the CPU, tests/test_mass.py on the GPU):
the definition of include/gjkepa.h (gjkepa_mass_batch; csrc/mass_props.h) restated in numpy from the header's
text -- the same 64 strided partials, the same xor butterfly, the same operation order, so its records are the
device's bit for bit -- and an exact reference in fractions.Fraction (the inputs are fp32-representable, so they
convert exactly; its results are formed from exact sums and rounded once).

dot(a, b) is (a.x b.x + a.y b.y) + a.z b.z throughout, as gkd::dot evaluates it; numpy contracts nothing."""
from fractions import Fraction

import numpy as np

import gjkepa

OK, DEGENERATE, BAD_INPUT = gjkepa.STATUS_OK, gjkepa.STATUS_DEGENERATE, gjkepa.STATUS_BAD_INPUT
PARTIALS, TERMS = 64, 14
MOMENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))       # xx, yy, zz, xy, xz, yz


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def face_terms(o, pa, pb, pc):
    """the 14 terms of every face: (F, 14)"""
    A, B, C = pa - o, pb - o, pc - o
    N = cross(B - A, C - B)
    d = dot(A, cross(B, C))
    S = (A + B) + C
    t = np.empty((len(A), TERMS))
    t[:, 0] = d
    for k in range(3):
        t[:, 1 + k] = d * S[:, k]
    for m, (i, j) in enumerate(MOMENTS):
        t[:, 4 + m] = d * (((S[:, i] * S[:, j] + A[:, i] * A[:, j]) + B[:, i] * B[:, j]) + C[:, i] * C[:, j])
    t[:, 10] = np.sqrt(dot(N, N))
    t[:, 11:14] = N
    return t


def totals(terms):
    """64 strided partials in ascending face order from +0.0, then P[l] = P[l] + P[l ^ s], s = 1 .. 32"""
    P = np.zeros((PARTIALS, TERMS))
    for base in range(0, len(terms), PARTIALS):
        chunk = terms[base:base + PARTIALS]
        P[:len(chunk)] = P[:len(chunk)] + chunk
    lanes = np.arange(PARTIALS)
    s = 1
    while s < PARTIALS:
        P = P + P[lanes ^ s]
        s *= 2
    assert (P.view(np.uint64) == P[0].view(np.uint64)).all() or np.isnan(P).any()
    return P[0]


def blank(status):
    r = np.zeros((), gjkepa.MASS64)
    r["status"] = status
    return r


def cloud(p, faces, hull_status=None):
    """The record of one cloud.  p: (n, 3) float64 (the stored points widened); faces: (F, 3) int32."""
    p, faces = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    n, F = len(p), len(faces)
    if n < 4 or n > gjkepa.HULL_MAX_POINTS:
        return blank(BAD_INPUT)
    if hull_status is not None and hull_status != OK:
        return blank(hull_status)
    if F < 4 or F > 2 * n - 4:
        return blank(BAD_INPUT)
    if (faces < 0).any() or (faces >= n).any() or not np.isfinite(p).all():
        return blank(BAD_INPUT)
    with np.errstate(all="ignore"):
        o = p[faces[0, 0]]
        T = totals(face_terms(o, p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]))
        r = blank(OK)
        T0 = T[0]
        vol = T0 / 6.0
        m = T[1:4] / (4.0 * T0)
        r["volume"] = vol
        r["com"] = o + m
        M = [T[4 + k] / 120.0 - (vol * m[i]) * m[j] for k, (i, j) in enumerate(MOMENTS)]
        r["inertia"] = [M[1] + M[2], M[0] + M[2], M[0] + M[1], -M[3], -M[4], -M[5]]
        r["area"] = 0.5 * T[10]
        r["closure"] = np.abs(T[11:14]).max() / T[10] if not np.isnan(T[11:14]).any() else np.nan
        q = p - r["com"]
        qq = dot(q, q)
        r["radius"] = np.sqrt(max(0.0, qq.max())) if not np.isnan(qq).any() else np.nan
        r["n_faces"] = F
        vals = np.concatenate([[T0, r["volume"], r["area"], r["radius"], r["closure"]], r["com"], r["inertia"]])
    if not (np.isfinite(vals).all() and T0 > 0.0):
        return blank(DEGENERATE)
    return r


def reference(pool, hull, use_status=True):
    """MASS64 records of a CloudPool from the dict hull_batch returned (or a caller's own faces)"""
    out = np.zeros(pool.n_clouds, gjkepa.MASS64)
    for c in range(pool.n_clouds):
        n = int(pool.cloud_cnt[c])
        if n < 4 or n > gjkepa.HULL_MAX_POINTS:
            out[c] = blank(BAD_INPUT)
            continue
        nf, fo = int(hull["n_faces"][c]), int(hull["face_off"][c])
        hs = int(hull["status"][c]) if use_status else None
        if hs is not None and hs != OK:
            out[c] = blank(hs)
            continue
        if nf < 4 or nf > 2 * n - 4:
            out[c] = blank(BAD_INPUT)
            continue
        out[c] = cloud(pool.cloud(c), np.asarray(hull["faces"]).reshape(-1, 3)[fo:fo + nf], hs)
    return out


def with_pivots(records, body_motion):
    """the motion blocks the entries hand back: c = com for every OK record, everything else untouched"""
    bm = np.array(body_motion, np.float64).reshape(-1, 9)
    ok = records["status"] == OK
    bm[ok, 6:9] = records["com"][ok]
    return bm


# ---------------------------------------------------------------- exact reference
def exact(p, faces):
    """volume, com[3], inertia[6] (about com) and radius of an outward mesh: exact rationals, rounded once"""
    P = [[Fraction(float(v)) for v in row] for row in np.asarray(p, np.float64)]
    o = P[int(faces[0][0])]
    T0, T1, T2 = Fraction(0), [Fraction(0)] * 3, [Fraction(0)] * 6
    for a, b, c in np.asarray(faces).tolist():
        A, B, C = ([P[i][k] - o[k] for k in range(3)] for i in (a, b, c))
        d = (A[0] * (B[1] * C[2] - B[2] * C[1]) + A[1] * (B[2] * C[0] - B[0] * C[2]) + A[2] * (B[0] * C[1] - B[1] * C[0]))
        S = [A[k] + B[k] + C[k] for k in range(3)]
        T0 += d
        T1 = [T1[k] + d * S[k] for k in range(3)]
        T2 = [T2[m] + d * (S[i] * S[j] + A[i] * A[j] + B[i] * B[j] + C[i] * C[j]) for m, (i, j) in enumerate(MOMENTS)]
    vol = T0 / 6
    m = [T1[k] / (4 * T0) for k in range(3)]
    com = [o[k] + m[k] for k in range(3)]
    M = [T2[k] / 120 - vol * m[i] * m[j] for k, (i, j) in enumerate(MOMENTS)]
    inertia = [M[1] + M[2], M[0] + M[2], M[0] + M[1], -M[3], -M[4], -M[5]]
    r2 = max(sum((x[k] - com[k]) ** 2 for k in range(3)) for x in P)
    return dict(volume=float(vol), com=np.array([float(x) for x in com]), inertia=np.array([float(x) for x in inertia]),
                radius=float(np.sqrt(np.float64(float(r2)))))


# ---------------------------------------------------------------- seeded clouds
def unit_cloud(seed, n, shape, centre=(0.0, 0.0, 0.0)):
    """n fp32-representable points (float64 array): on the unit sphere (shape 1: every point a hull vertex) or in
    the unit ball (shape 0), about a centre"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if shape == 0:
        u *= rng.uniform(0.0, 1.0, size=(n, 1)) ** (1.0 / 3.0)
        u[:4] /= np.linalg.norm(u[:4], axis=1, keepdims=True)     # never flat: four points on the sphere
    return (u + np.asarray(centre)).astype(np.float32).astype(np.float64)


def flat_cloud(n):
    """n points in the plane z = 0.5: the hull module answers DEGENERATE"""
    k = np.arange(n, dtype=np.float64)
    return np.stack([np.cos(k), np.sin(2.0 * k), np.full(n, 0.5)], 1).astype(np.float32).astype(np.float64)


SIZES = (4, 5, 16, 17, 34, 35, 64, 65, 255, 256)


def mixed_clouds(n_clouds, seed=1, first=0):
    """A list of n_clouds (n, 3) clouds cycling, from kind `first`, through every size of SIZES as a sphere and as
    a ball cloud, centred within 9 of the origin, with a BAD_INPUT cloud (n = 3, n = 257 in turn) after every 5th
    and a DEGENERATE (flat) cloud after every 7th; and what each cloud is"""
    kinds = [(n, s) for n in SIZES for s in (1, 0)]
    out, what = [], []
    rng = np.random.default_rng(seed)
    good = 0
    while len(out) < n_clouds:
        n, s = kinds[(first + good) % len(kinds)]
        out.append(unit_cloud(seed * 100003 + good, n, s, rng.uniform(-9.0, 9.0, 3)))
        what.append((n, s))
        good += 1
        if good % 5 == 0:
            out.append(unit_cloud(seed, 3 if good % 10 else 257, 1)); what.append("bad")
        if good % 7 == 0:
            out.append(flat_cloud(4 + good % 60)); what.append("flat")
    return out[:n_clouds], what[:n_clouds]
