"""Batched mass properties on the GPU (include/gjkepa.h gjkepa_mass_batch(_device), gjkepa_mass_pool): the
records are the numpy restatement's (tests/mass_ref.py) byte for byte in both storage dtypes, on pools that mix
every shape at which the kernel takes another path (fewer faces than lanes, 64 and 66 faces where the partials
wrap, the tier boundary at 64 / 65 points, 508 faces) with BAD_INPUT and DEGENERATE clouds between them, in pools
of 1, 3, 5 and about 1,500 clouds; the pivots land in the motion blocks and the radius is the swept broad phase's
rho; gjkepa_mass_pool gives the bytes of the two entries it chains; the device entry runs on a stream and in a
captured hull -> mass chain; and faces of the caller's own with an index out of range are answered BAD_INPUT."""
import numpy as np
import pytest

import gjkepa
import mass_ref as mr
import sweep_ref as sr

pytestmark = pytest.mark.gpu
OK, DEGENERATE, BAD_INPUT = mr.OK, mr.DEGENERATE, mr.BAD_INPUT


def device_pool(pool, dev):
    """the device buffers of gjkepa_hull_batch_device / gjkepa_mass_batch_device for a CloudPool"""
    import torch
    n = pool.n_clouds
    foff = gjkepa.hull_face_offsets(pool.cloud_cnt)
    slots = int(foff[-1] + max(2 * int(pool.cloud_cnt[-1]) - 4, 0))
    t = dict(p=torch.from_numpy(np.ascontiguousarray(pool.verts)).to(dev), off=torch.from_numpy(pool.cloud_off).to(dev),
             cnt=torch.from_numpy(pool.cloud_cnt).to(dev), foff=torch.from_numpy(foff).to(dev),
             faces=torch.full((max(slots, 1) * 3,), -1, dtype=torch.int32, device=dev),
             nf=torch.zeros(n, dtype=torch.int32, device=dev), nv=torch.zeros(n, dtype=torch.int32, device=dev),
             st=torch.zeros(n, dtype=torch.int8, device=dev), out=torch.zeros(n * 128, dtype=torch.uint8, device=dev))
    return t


def enqueue_hull(pool, t, stream):
    gjkepa.hull_batch_device(pool.dtype_code, t["p"].data_ptr(), t["off"].data_ptr(), t["cnt"].data_ptr(), pool.n_clouds,
                             t["foff"].data_ptr(), t["faces"].data_ptr(), t["nf"].data_ptr(), t["nv"].data_ptr(),
                             t["st"].data_ptr(), 0, 0, stream)


def enqueue_mass(pool, t, stream, out=None, motion=0, status=True):
    gjkepa.mass_batch_device(pool.dtype_code, t["p"].data_ptr(), t["off"].data_ptr(), t["cnt"].data_ptr(), pool.n_clouds,
                             t["foff"].data_ptr(), t["faces"].data_ptr(), t["nf"].data_ptr(), t["st"].data_ptr() if status else 0,
                             (t["out"] if out is None else out).data_ptr(), motion, stream)


def records(t):
    return t.cpu().numpy().view(gjkepa.MASS64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_clouds,first", [(1, 14), (3, 12), (5, 16), (1500, 0)])
def test_records_are_the_restatements_bytes(n_clouds, first, dtype):
    """first: where the small pools start in mass_ref's cycle of shapes: one 65-point sphere cloud; 64 sphere, 64
    ball, 65 sphere (both tiers in one pool); 255, 255, 256, 256, 4"""
    clouds, what = mr.mixed_clouds(n_clouds, seed=7, first=first)
    pool = gjkepa.CloudPool.from_list(clouds, dtype=dtype)
    hull = gjkepa.hull_batch(pool)
    got = gjkepa.mass_batch(pool, hull)
    want = mr.reference(pool, hull)
    assert got.dtype == gjkepa.MASS64 and got.tobytes() == want.tobytes()
    for c, w in enumerate(what):
        assert want["status"][c] == {"bad": BAD_INPUT, "flat": DEGENERATE}.get(w, OK), (c, w)
    bad = want["status"] != OK
    assert (want[bad].view(np.uint8).reshape(-1, 128)[:, :108] == 0).all() and (want[bad]["n_faces"] == 0).all()
    if n_clouds == 1500:
        assert {w for w in what if isinstance(w, tuple)} == {(n, s) for n in mr.SIZES for s in (0, 1)}
        assert bad.sum() > 300 and (want["status"] == DEGENERATE).sum() > 100
        nf = dict(zip(what, hull["n_faces"]))
        assert nf[(4, 1)] == 4 and nf[(34, 1)] == 64 and nf[(35, 1)] == 66 and nf[(256, 1)] == 508 and nf[(256, 0)] < 508
        # without the hull's status the flat clouds have no faces: rule 3
        loose = gjkepa.mass_batch(pool, hull, use_status=False)
        assert loose.tobytes() == mr.reference(pool, hull, use_status=False).tobytes()
        assert (loose["status"][want["status"] == DEGENERATE] == BAD_INPUT).all()


def test_pivots_land_in_the_motion_blocks_and_radius_is_rho():
    clouds, what = mr.mixed_clouds(300, seed=11)
    pool = gjkepa.CloudPool.from_list(clouds, dtype=np.float32)
    hull = gjkepa.hull_batch(pool)
    rng = np.random.default_rng(5)
    bm = rng.normal(size=(pool.n_clouds, 9))
    rec, out = gjkepa.mass_batch(pool, hull, body_motion=bm)
    assert rec.tobytes() == mr.reference(pool, hull).tobytes()
    ok = rec["status"] == OK
    assert ok.sum() > 200 and (~ok).sum() > 50
    assert out[ok, 6:9].tobytes() == rec["com"][ok].tobytes()
    assert out[:, 0:6].tobytes() == bm[:, 0:6].tobytes() and out[~ok].tobytes() == bm[~ok].tobytes()
    assert out.tobytes() == mr.with_pivots(rec, bm).tobytes()
    # the swept broad phase's rho for these pivots (tests/sweep_ref.py balls), on the clouds as a hull pool
    as_hulls = gjkepa.HullPool(pool.verts, pool.cloud_off, pool.cloud_cnt, np.zeros((0, 2), np.int32))
    valid, rho = sr.balls(as_hulls, out)
    assert valid[ok].all()
    assert rho[ok].tobytes() == rec["radius"][ok].tobytes()


def test_mass_pool_is_hull_then_mass():
    pool = gjkepa.synth_scene(31, 200, 8, 64, 20.0)
    cnt, verts = pool.hull_cnt.copy(), pool.verts.copy()
    cnt[17] = 1                                                          # a one-vertex hull
    o, n = int(pool.hull_off[40]), int(cnt[40])
    verts[o + 2 * n:o + 3 * n] = 0.25                                    # a flat one
    pool = gjkepa.HullPool(verts, pool.hull_off, cnt, pool.pairs)
    bm = np.random.default_rng(6).normal(size=(200, 9))
    rec, out = gjkepa.mass_pool(pool, bm)
    clouds = gjkepa.CloudPool(pool.verts, pool.hull_off, pool.hull_cnt)
    hull = gjkepa.hull_batch(clouds)
    rec2, out2 = gjkepa.mass_batch(clouds, hull, body_motion=bm)
    assert rec.tobytes() == rec2.tobytes() and out.tobytes() == out2.tobytes()
    assert rec.tobytes() == mr.reference(clouds, hull).tobytes()
    assert rec["status"][17] == BAD_INPUT and rec["status"][40] == DEGENERATE and (np.delete(rec["status"], [17, 40]) == OK).all()
    assert out[17].tobytes() == bm[17].tobytes() and out[40].tobytes() == bm[40].tobytes()
    assert gjkepa.mass_pool(pool).tobytes() == rec.tobytes()
    # unit-sphere hulls: the centre of mass lies inside the sphere, so no vertex is further than its diameter
    ok = rec["status"] == OK
    assert (rec["radius"][ok] > 0).all() and (rec["radius"][ok] < 2.0).all() and (rec["volume"][ok] > 0).all()


def test_device_entry_on_a_stream_and_in_a_captured_chain():
    import torch
    dev = torch.device("cuda", 0)
    clouds, _ = mr.mixed_clouds(400, seed=13)
    pool = gjkepa.CloudPool.from_list(clouds, dtype=np.float32)
    other = gjkepa.CloudPool.from_list([c[::-1] * 1.5 for c in clouds], dtype=np.float32)   # the same counts, other points
    t = device_pool(pool, dev)
    bm0 = np.random.default_rng(8).normal(size=(pool.n_clouds, 9))
    mot = torch.from_numpy(bm0.reshape(-1)).to(dev)

    def expect(p):
        h = gjkepa.hull_batch(p)
        return mr.reference(p, h)

    want, want_other = expect(pool), expect(other)
    work = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(work):
        enqueue_hull(pool, t, work.cuda_stream)
        enqueue_mass(pool, t, work.cuda_stream, motion=mot.data_ptr())
    torch.cuda.synchronize(dev)
    assert records(t["out"]).tobytes() == want.tobytes()
    assert mot.cpu().numpy().tobytes() == mr.with_pivots(want, bm0).tobytes()
    # the linear chain hull -> mass, captured on one stream and replayed with the points rewritten in place
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    out = torch.zeros_like(t["out"])
    with torch.cuda.graph(g, stream=side):
        enqueue_hull(pool, t, side.cuda_stream)
        enqueue_mass(pool, t, side.cuda_stream, out=out)
    torch.cuda.synchronize(dev)
    for p, w in ((other, want_other), (pool, want)):
        with torch.cuda.stream(work):
            t["p"].copy_(torch.from_numpy(np.ascontiguousarray(p.verts)))
            out.zero_()
            g.replay()
        torch.cuda.synchronize(dev)
        assert records(out).tobytes() == w.tobytes()
    del g


def test_callers_faces_with_an_index_out_of_range():
    """The guard of rule 4: the bad index is compared with n and never used as an address."""
    import torch
    dev = torch.device("cuda", 0)
    clouds, _ = mr.mixed_clouds(40, seed=17)
    pool = gjkepa.CloudPool.from_list(clouds, dtype=np.float32)
    hull = gjkepa.hull_batch(pool)
    want = mr.reference(pool, hull, use_status=False)
    faces = hull["faces"].copy()
    okc = np.nonzero(want["status"] == OK)[0]
    hit = {int(okc[1]): (0, 0, 1 << 30), int(okc[4]): (3, 2, -1), int(okc[9]): (1, 1, int(pool.cloud_cnt[okc[9]])),
           int(okc[12]): (int(hull["n_faces"][okc[12]]) - 1, 0, -(1 << 31))}
    for c, (f, k, v) in hit.items():
        faces[int(hull["face_off"][c]) + f, k] = v
    t = device_pool(pool, dev)
    t["faces"][:faces.size] = torch.from_numpy(faces.reshape(-1)).to(dev)
    t["nf"].copy_(torch.from_numpy(hull["n_faces"]))
    enqueue_mass(pool, t, 0, status=False)
    torch.cuda.synchronize(dev)
    got = records(t["out"])
    for c in hit:
        want[c] = mr.blank(BAD_INPUT)
    assert got["status"][list(hit)].tolist() == [BAD_INPUT] * 4
    assert got.tobytes() == want.tobytes()
