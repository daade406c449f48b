"""Brute-force separation distance of two small convex hulls given by their vertices (numpy only).

The distance of two disjoint convex polytopes is attained between a vertex, an edge or a face of one
and a vertex, an edge or a face of the other, and the closest pair of features is vertex-vertex,
vertex-edge, edge-edge or vertex-face.  Every edge is a segment between two vertices and every point of
a face lies in a triangle of three of its vertices, so the minimum over ALL vertex pairs, vertex-segment
pairs, segment-segment pairs and vertex-triangle pairs (any two / three vertices of a hull; both
directions; zero-area triangles skipped) is exact: each candidate is a distance between two points of
the hulls (never below the true distance), and the closest features are among them.  Works for 1-, 2-
and 3-vertex and coplanar hulls.  Cost grows as n^4: use it for hulls of at most 12 vertices and a few
hundred pairs.  For overlapping hulls the result is meaningless (some positive number or 0)."""
import numpy as np


def _vertex_segment(P, Q):
    """min distance from the points P to every segment between two points of Q"""
    if len(Q) < 2:
        return np.inf
    i, j = np.triu_indices(len(Q), 1)
    q0, e = Q[i], Q[j] - Q[i]
    ee = (e * e).sum(1)
    t = ((P[:, None, :] - q0[None]) * e[None]).sum(2) / np.where(ee > 0, ee, 1.0)
    t = np.clip(np.where(ee > 0, t, 0.0), 0.0, 1.0)
    d = P[:, None, :] - (q0[None] + t[..., None] * e[None])
    return float(np.sqrt((d * d).sum(2)).min())


def _segment_segment(A, B):
    """min over segment pairs of the distance at the (clipped) closest parameters of the two lines"""
    if len(A) < 2 or len(B) < 2:
        return np.inf
    i, j = np.triu_indices(len(A), 1)
    k, l = np.triu_indices(len(B), 1)
    p0, u = A[i][:, None, :], (A[j] - A[i])[:, None, :]
    q0, w = B[k][None, :, :], (B[l] - B[k])[None, :, :]
    r = p0 - q0
    a, b, c = (u * u).sum(2), (u * w).sum(2), (w * w).sum(2)
    d, e = (u * r).sum(2), (w * r).sum(2)
    den = a * c - b * b
    ok = den > 1e-14 * a * c
    den = np.where(ok, den, 1.0)
    s = np.clip(np.where(ok, (b * e - c * d) / den, 0.0), 0.0, 1.0)
    t = np.clip(np.where(ok, (a * e - b * d) / den, 0.0), 0.0, 1.0)
    g = r + s[..., None] * u - t[..., None] * w
    return float(np.sqrt((g * g).sum(2)).min())


def _vertex_triangle(P, Q):
    """min distance from the points P to the triangles of Q their projection falls inside"""
    n = len(Q)
    if n < 3:
        return np.inf
    tri = np.array([(i, j, k) for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n)])
    a, ab, ac = Q[tri[:, 0]], Q[tri[:, 1]] - Q[tri[:, 0]], Q[tri[:, 2]] - Q[tri[:, 0]]
    bb, cc, bc = (ab * ab).sum(1), (ac * ac).sum(1), (ab * ac).sum(1)
    det = bb * cc - bc * bc
    ok = det > 1e-14 * bb * cc                      # zero-area triangles are skipped
    det = np.where(ok, det, 1.0)
    ap = P[:, None, :] - a[None]
    d1, d2 = (ap * ab[None]).sum(2), (ap * ac[None]).sum(2)
    v = (d1 * cc - d2 * bc) / det
    w = (d2 * bb - d1 * bc) / det
    inside = ok[None] & (v >= 0) & (w >= 0) & (v + w <= 1)
    g = ap - v[..., None] * ab[None] - w[..., None] * ac[None]
    dist = np.where(inside, np.sqrt((g * g).sum(2)), np.inf)
    return float(dist.min())


def pair_distance(A, B):
    """Exact distance between conv(A) and conv(B) for disjoint hulls; A, B: (n, 3) float64 vertices."""
    A = np.asarray(A, np.float64).reshape(-1, 3)
    B = np.asarray(B, np.float64).reshape(-1, 3)
    d = A[:, None, :] - B[None]
    best = float(np.sqrt((d * d).sum(2)).min())
    return min(best, _vertex_segment(A, B), _vertex_segment(B, A), _segment_segment(A, B),
               _vertex_triangle(A, B), _vertex_triangle(B, A))


def pool_distances(pool, idx=None):
    """pair_distance for the pairs `idx` (default: all) of a gjkepa.HullPool"""
    idx = range(pool.n_pairs) if idx is None else idx
    return np.array([pair_distance(pool.hull(int(pool.pairs[k, 0])), pool.hull(int(pool.pairs[k, 1]))) for k in idx])


def tol(ref):
    """the distance tests' tolerance: 1e-6 relative (the project's north-star bar) + 1e-9 absolute
    (tests/test_warm.py's floor)"""
    return 1e-6 * np.asarray(ref, np.float64) + 1e-9


def check_certificate(pool, rec, idx, far=False):
    """Assert that the distance records rec[idx] certify themselves as separated pairs and return
    (upper, lower): per pair |point_a - point_b| recomputed from lambda / code, and the support gap
    min_i n.a_i - max_j n.b_j along the record's normal; the true distance lies between them.
    far: FAR records, whose `distance` is the lower bound only (it may sit below the upper bound)."""
    upper, lower = np.zeros(len(idx)), np.zeros(len(idx))
    worst = dict(lam_sum=0.0, point=0.0, up=0.0, low=0.0)
    for t, k in enumerate(idx):
        r = rec[k]
        A, B = pool.hull(int(pool.pairs[k, 0])), pool.hull(int(pool.pairs[k, 1]))
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
        up = float(np.linalg.norm(r["point_a"] - r["point_b"]))
        nrm = r["normal"]
        assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-12, (k, nrm)
        low = float((A @ nrm).min() - (B @ nrm).max())
        d = float(r["distance"])
        if far:
            assert d <= up + tol(up), (k, d, up)
        else:
            assert abs(up - d) <= tol(d), (k, up, d)
        assert low >= d - tol(d), (k, low, d)
        upper[t], lower[t] = up, low
        worst["lam_sum"] = max(worst["lam_sum"], abs(lam.sum() - 1.0))
        worst["point"] = max(worst["point"], np.abs(pa - r["point_a"]).max(), np.abs(pb - r["point_b"]).max())
        worst["up"] = max(worst["up"], 0.0 if far else abs(up - d) / d)
        worst["low"] = max(worst["low"], (d - low) / d)
    print(f"certificate over {len(idx)} pairs: worst |sum lambda - 1| {worst['lam_sum']:.2e}, point {worst['point']:.2e}, "
          f"relative (upper - distance) {worst['up']:.2e}, (distance - lower) {worst['low']:.2e}")
    return upper, lower
