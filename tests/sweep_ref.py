"""Shared helpers of the swept broad phase's tests (tests/test_sweep_host.py on the CPU, tests/test_sweep.py
on the GPU): the definition of include/gjkepa.h (gjkepa_broadphase_swept; csrc/swept_sphere.h) restated in
numpy, O(N^2), in the header's operation order, so its list is the device's bit for bit as brute() of
tests/test_broadphase.py is the static broad phase's; and seeded scenes over gjkepa.synth_scene.

dot(a, b) is (a.x b.x + a.y b.y) + a.z b.z throughout, as gkd::dot evaluates it; numpy contracts nothing."""
import numpy as np

import gjkepa

S_EE0, S_RECEDE, S_CLAMP1, S_INTERIOR = 0, 1, 2, 3
BRANCHES = {S_EE0: "ee == 0", S_RECEDE: "de >= 0", S_CLAMP1: "clamp to 1", S_INTERIOR: "interior"}


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def balls(pool, body_motion):
    """(valid [n] bool, rho [n]) of a pool's hulls: valid = count in 1 .. MAX_HULL_VERTS, every vertex finite,
    every motion double finite; rho = sqrt(max_i q_i.q_i), q_i = x_i - c."""
    bm = np.asarray(body_motion, np.float64).reshape(-1, 9)
    n = len(pool.hull_cnt)
    assert len(bm) == n
    valid = np.zeros(n, bool)
    rho = np.full(n, np.nan)
    with np.errstate(all="ignore"):
        for h in range(n):
            cnt = int(pool.hull_cnt[h])
            if not 1 <= cnt <= gjkepa.MAX_HULL_VERTS:
                continue
            x = pool.hull(h)
            if not (np.isfinite(x).all() and np.isfinite(bm[h]).all()):
                continue
            q = x - bm[h, 6:9]
            valid[h] = True
            rho[h] = np.sqrt(max(0.0, dot(q, q).max()))
    return valid, rho


def pair_terms(ca, va, cb, vb):
    """d, e, s and the branch of s for arrays of pairs (a the lower index)"""
    with np.errstate(all="ignore"):
        d, e = ca - cb, va - vb
        ee, de = dot(e, e), dot(d, e)
        first = (ee == 0.0) | (de >= 0.0)
        clamp = ~first & (-de >= ee)
        s = np.where(first, 0.0, np.where(clamp, 1.0, (-de) / ee))
        branch = np.where(ee == 0.0, S_EE0, np.where(first, S_RECEDE, np.where(clamp, S_CLAMP1, S_INTERIOR)))
    return d, e, s, branch


def pair_pass(ca, va, rho_a, cb, vb, rho_b, tolerance):
    """the definition's test for arrays of pairs; returns (pass, branch of s)"""
    d, e, s, branch = pair_terms(ca, va, cb, vb)
    with np.errstate(all="ignore"):
        m = d + s[..., None] * e
        dist = np.sqrt(dot(m, m))
        reach = (rho_a + rho_b) + tolerance
        lim = reach + 1e-9 * ((reach + np.abs(d).max(-1)) + np.abs(e).max(-1))
        return dist <= lim, branch


def reference(pool, body_motion, tolerance, with_branch=False, rows=256):
    """The swept list: int32 [n, 2], ascending (a, b), `rows` rows of the pair matrix at a time; with_branch:
    also the full (n, n) pass and branch matrices and the valid mask."""
    bm = np.asarray(body_motion, np.float64).reshape(-1, 9)
    valid, rho = balls(pool, bm)
    c, v = bm[:, 6:9], bm[:, 0:3]
    n = len(bm)
    oks, branches = [], []
    for r in range(0, n, rows):
        a = slice(r, min(r + rows, n))
        ok, branch = pair_pass(c[a, None, :], v[a, None, :], rho[a, None], c[None, :, :], v[None, :, :], rho[None, :], tolerance)
        oks.append(ok & valid[a, None] & valid[None, :])
        if with_branch:
            branches.append(branch)
    ok = np.triu(np.concatenate(oks), 1) if oks else np.zeros((0, 0), bool)
    pairs = np.argwhere(ok).astype(np.int32)
    return (pairs, ok, np.concatenate(branches), valid) if with_branch else pairs


def centres(pool):
    """the vertex means; 0 for a hull whose count is out of range"""
    c = np.zeros((len(pool.hull_cnt), 3))
    for h, n in enumerate(pool.hull_cnt):
        if 1 <= n <= gjkepa.MAX_HULL_VERTS:
            c[h] = pool.hull(h).mean(0)
    return c


def unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def motions(pool, seed, vmax, wmax=1.0):
    """Body motions (n_hulls, 9): v of uniformly random direction and length U[0, vmax], w as in
    cast_rigid_ref.motions (random direction, length U[0, wmax]), the pivot at the hull's vertex mean."""
    rng = np.random.default_rng(seed)
    n = len(pool.hull_cnt)
    m = np.zeros((n, 9))
    m[:, 0:3] = unit(rng, n) * rng.uniform(0.0, vmax, size=(n, 1))
    m[:, 3:6] = unit(rng, n) * rng.uniform(0.0, wmax, size=(n, 1))
    m[:, 6:9] = centres(pool)
    return m


def scene(seed, n_hulls, n_min, n_max, box, vmax, dtype=np.float32, shift=0.0):
    """(pool, body motions): gjkepa.synth_scene with seeded motions; shift moves every vertex (and pivot) by
    -shift along each axis (a scene centred on the origin for shift = box / 2)"""
    pool = gjkepa.synth_scene(seed, n_hulls, n_min, n_max, box, dtype=dtype)
    if shift:
        pool = gjkepa.HullPool((pool.verts - dtype(shift)).astype(dtype), pool.hull_off, pool.hull_cnt, pool.pairs)
    return pool, motions(pool, seed ^ 0x5EE9, vmax)


def branch_scene():
    """160 hulls in a box of 12, v up to 4; the first 60 share one velocity (the ee == 0 branch)"""
    pool, bm = scene(21, 160, 8, 32, 12.0, 4.0)
    bm[:60, 0:3] = [0.7, -1.1, 0.4]
    return pool, bm


def with_invalid(pool, bm):
    """hulls 3, 7, 11, 13, 17 made invalid: count 0, count 300, a NaN vertex, an infinite v, a NaN c"""
    cnt, verts, bm = pool.hull_cnt.copy(), pool.verts.copy(), bm.copy()
    cnt[3] = 0
    cnt[7] = 300
    verts[pool.hull_off[11] + 1] = np.nan
    bm[13, 1] = np.inf
    bm[17, 8] = np.nan
    return gjkepa.HullPool(verts, pool.hull_off, cnt, pool.pairs), bm, [3, 7, 11, 13, 17]


def all_pairs(n):
    a, b = np.triu_indices(n, 1)
    return np.stack([a, b], 1).astype(np.int32)


def keys(pairs):
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return p[:, 0] * (1 << 32) + p[:, 1]
