"""gjkepa_broadphase_swept(_device) on the GPU: the pair list of the casts.

The list equals the numpy restatement of the definition (tests/sweep_ref.py): same pairs, same order, same
count, over dense, sparse, mixed-size, fp64, origin-centred and invalid scenes, tiny pools, bodies at rest
and bodies sharing one velocity; long_radius never changes a byte of it; a cut list still counts and stays
an ascending subset; the device entry repeats itself on one workspace and replays as a captured graph on
rewritten motions; and swept list -> gjkepa_batch -> gjkepa_cast_rigid_batch with records gives the host
cast program's bytes, with every IMPACT or START of the static list's pairs present in the swept list.

The full-size scene S1 (2^20 hulls) is not checked here: a numpy reference over a grid takes far longer than
a few seconds at that size.  tools/bench_sweep.py checks a sample of it against the restatement instead."""
import functools
import shutil

import numpy as np
import pytest

import cast_rigid_ref as rr
import gjkepa
import sweep_ref as sr

pytestmark = pytest.mark.gpu
INF = float("inf")


def _rest(pool, bm):
    bm = bm.copy()
    bm[:, 0:3] = 0.0
    return pool, bm


def _shared(pool, bm):
    bm = bm.copy()
    bm[:, 0:3] = [1.5, -0.25, 2.0]
    return pool, bm


def _invalid():
    pool, bm, _ = sr.with_invalid(*sr.scene(5, 600, 4, 64, 12.0, 2.0, dtype=np.float64))
    return pool, bm


# name -> (scene, tolerance)
SCENES = {
    "dense": (lambda: sr.scene(1, 2000, 32, 32, 15.0, 2.0), 1e-3),
    "sparse": (lambda: sr.scene(2, 3000, 8, 40, 60.0, 3.0), 1e-3),
    "mixed": (lambda: sr.scene(3, 1500, 8, 256, 20.0, 2.0), 1e-6),
    "f64": (lambda: sr.scene(4, 1000, 16, 16, 10.0, 2.0, dtype=np.float64), 1e-6),
    "origin": (lambda: sr.scene(8, 1200, 16, 32, 16.0, 2.0, shift=8.0), 1e-3),
    "invalid": (_invalid, 1e-3),
    "branches": (sr.branch_scene, 1e-3),
    "at rest": (lambda: _rest(*sr.scene(9, 1000, 16, 16, 12.0, 2.0)), 1.0),
    "one velocity": (lambda: _shared(*sr.scene(10, 1000, 16, 16, 12.0, 2.0)), 1e-3),
    **{f"n={n}": ((lambda n=n: sr.scene(6, n, 8, 8, 3.0, 1.0)), 1e-3) for n in (1, 2, 63, 64, 65)},
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(pool, body motions, tolerance, reference list) of a scene, built once"""
    build, tol = SCENES[name]
    pool, bm = build()
    return pool, bm, tol, sr.reference(pool, bm, tol)


@pytest.mark.parametrize("name", list(SCENES))
def test_list_equals_the_reference(name):
    pool, bm, tol, ref = case(name)
    got, n = gjkepa.broadphase_swept(pool, bm, tol)
    print(f"{name}: {len(pool.hull_cnt)} hulls, {len(ref)} pairs in the reference, {n} found")
    assert n == len(ref)
    assert got.tobytes() == ref.tobytes()
    if name == "invalid":
        assert len(ref) > 0 and not np.isin(got, [3, 7, 11, 13, 17]).any()
    if name in ("dense", "sparse", "mixed", "origin", "at rest", "one velocity", "n=65"):
        assert len(ref) > 0


def bullet_scene():
    """the dense scene with three bullets travelling about 20 cell edges (the cell is 2 (1 + 1) = 4 without
    them); bullets 0 and 1 pass through the same point at t = 0.5"""
    pool, bm = sr.scene(1, 2000, 32, 32, 15.0, 2.0)
    bm = bm.copy()
    bm[0, 0:3] = [80.0, 0.0, 0.0]
    bm[1, 0:3] = 2.0 * (bm[0, 6:9] + 0.5 * bm[0, 0:3] - bm[1, 6:9])
    bm[2, 0:3] = [-30.0, 60.0, 40.0]
    return pool, bm


def test_long_radius_does_not_change_the_list():
    pool, bm = bullet_scene()
    tol = 1e-3
    ref = sr.reference(pool, bm, tol)
    assert (ref == [0, 1]).all(axis=1).any()                                  # the bullets that cross
    big = sr.balls(pool, bm)[1] + 0.5 * np.linalg.norm(bm[:, 0:3], axis=1)
    half = float(np.median(big))
    assert (big > 10.0).sum() == 3 and 800 < (big > half).sum() < 1200
    for lr in (INF, 10.0, half, 0.0):
        got, n = gjkepa.broadphase_swept(pool, bm, tol, long_radius=lr)
        print(f"long_radius {lr:g}: {(big > lr).sum()} long bodies, {n} pairs")
        assert n == len(ref), lr
        assert got.tobytes() == ref.tobytes(), lr


def test_truncated_list_still_counts():
    pool, bm, tol, ref = case("dense")
    m = len(ref)
    for lr in (INF, 1.5):
        got, n = gjkepa.broadphase_swept(pool, bm, tol, long_radius=lr, max_pairs=m // 3)
        assert n == m and len(got) == m // 3
        assert np.all(np.diff(sr.keys(got)) > 0)                              # still ascending, distinct
        assert set(sr.keys(got).tolist()) <= set(sr.keys(ref).tolist())


def test_device_entry_repeats_and_replays_as_a_graph():
    import torch
    pool, bm, tol, ref = case("dense")
    pool2, bm2 = bullet_scene()
    ref2 = sr.reference(pool2, bm2, tol)
    nh = len(pool.hull_cnt)
    dev = torch.device("cuda", 0)
    verts, off, cnt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pool.verts, pool.hull_off, pool.hull_cnt))
    mot = torch.from_numpy(np.ascontiguousarray(bm).reshape(-1)).to(dev)
    cap = 2 * max(len(ref), len(ref2))
    wsb = gjkepa.broadphase_swept_workspace_bytes(nh, cap)
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)

    def run(pairs, count, stream, long_radius=4.0):
        gjkepa.broadphase_swept_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), nh, mot.data_ptr(),
                                       tol, long_radius, pairs.data_ptr(), cap, count.data_ptr(), ws.data_ptr(), wsb, stream)

    def fresh():
        return torch.full((cap, 2), -1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)

    (p0, c0) = fresh()                                                        # a short workspace enqueues nothing
    rc = gjkepa.load().gjkepa_broadphase_swept_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), nh,
                                                      mot.data_ptr(), tol, INF, p0.data_ptr(), cap, c0.data_ptr(),
                                                      ws.data_ptr(), wsb - 1, None)
    assert rc == -4                                                           # GJKEPA_E_WORKSPACE
    torch.cuda.synchronize(dev)
    assert (p0 == -1).all() and int(c0.item()) == 0
    work = torch.cuda.Stream(dev)
    (p1, c1), (p2, c2), (pg, cg) = fresh(), fresh(), fresh()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(work):
        run(p1, c1, work.cuda_stream)
        run(p2, c2, work.cuda_stream)
    torch.cuda.synchronize(dev)
    assert int(c1.item()) == len(ref) == int(c2.item())
    assert p1[:len(ref)].cpu().numpy().tobytes() == ref.tobytes()
    assert (p1[len(ref):] == -1).all()                                        # nothing written past the list
    assert torch.equal(p1, p2)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    with torch.cuda.graph(g, stream=side):
        run(pg, cg, side.cuda_stream)
    torch.cuda.synchronize(dev)
    for motion, want in ((bm, ref), (bm2, ref2), (bm, ref)):
        with torch.cuda.stream(work):
            mot.copy_(torch.from_numpy(np.ascontiguousarray(motion).reshape(-1)), non_blocking=False)
            g.replay()
        torch.cuda.synchronize(dev)
        assert int(cg.item()) == len(want)
        assert pg[:len(want)].cpu().numpy().tobytes() == want.tobytes()
    del g


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_swept_list_through_the_batch_and_the_cast(tmp_path_factory):
    """20 000 hulls: swept list -> gjkepa_batch -> gjkepa_cast_rigid_batch with records"""
    host_cast = rr.build_host(tmp_path_factory.mktemp("sweep_chain"))[0]
    tol = 1e-6
    pool, bm = sr.scene(12, 20000, 16, 48, 80.0, 3.0)
    swept, n = gjkepa.broadphase_swept(pool, bm, tol, long_radius=4.0)
    assert n == len(swept) > 10000
    cand = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, swept)
    contact = gjkepa.gjkepa_batch(cand, 2, 1.0)
    hit = contact["collision"] != 0
    rec = gjkepa.cast_rigid_batch(cand, bm, tol, records=contact)
    assert np.array_equal((rec["flags"] & rr.SKIPPED) != 0, hit)
    impact = rr.kinds(rec)[0]
    print(f"{n} swept pairs: {hit.sum()} hits skipped, {impact.sum()} impacts ({impact.mean():.3f})")
    assert 0.0 < impact.mean() < 1.0
    # a sample of the list through the host cast program: the same bytes where the cast ran
    pick = np.arange(0, n, max(1, n // 1500))
    sample = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, swept[pick])
    want = host_cast(sample, bm, tol)
    ran = ~hit[pick]
    assert ran.sum() > 500
    assert rec[pick][ran].tobytes() == want[ran].tobytes()
    # what the cast finds on the static list is in the swept list
    static, _ = gjkepa.broadphase(pool)
    srec = gjkepa.cast_rigid_batch(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, static), bm, tol)
    s_impact, _, s_start, _, _ = rr.kinds(srec)
    flagged = sr.keys(static[s_impact | s_start])
    print(f"{len(static)} static pairs: {s_impact.sum()} impacts, {s_start.sum()} starts")
    assert len(flagged) > 100
    assert np.isin(flagged, sr.keys(swept)).all()
