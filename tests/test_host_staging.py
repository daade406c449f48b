"""The host-buffer entries share one set of per-device staging buffers (csrc/gjkepa_capi.cpp Stage):
verts / off / cnt by every entry, d_rec / d_out / d_ws by the distance and the cast entry.  Run one
after the other in one process, on pools of different sizes and storage types, each entry must give
the bytes it gives alone, and the bytes of the device entries, which use no staging.  Two threads on one
device must not see each other's buffers (the lock spans upload to copy back)."""
import threading

import numpy as np
import pytest

import gjkepa
from test_collide import expected, scene_with_invalid
from test_hull import assert_same

pytestmark = pytest.mark.gpu

TAU = 1e-6
SIZES = (1, 4, 32, 33, 128, 129, 256)        # both sides of the tier brackets 1-32 / 33-128 / 129-256
BAD_PAIR = 10


def pair_list(shift):
    """65 pairs over every (size, size) combination of SIZES, overlapping to well separated, pair
    BAD_PAIR with an empty hull; every hull moved by `shift`.  Returns the pairs and hull B's motion."""
    rng = np.random.default_rng(7)

    def sphere(n, centre):
        p = rng.normal(size=(n, 3))
        return p / np.linalg.norm(p, axis=1, keepdims=True) + centre + shift

    pairs, motion = [], []
    for k in range(64):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        gap = (0.5, 1.9, 2.5, 4.0)[k % 4]
        pairs.append((sphere(SIZES[k % 7], 0.0), sphere(SIZES[(k // 7 + k) % 7], gap * d)))
        motion.append(-3.0 * d)
    pairs.insert(BAD_PAIR, (np.zeros((0, 3)), sphere(32, 0.0)))
    motion.insert(BAD_PAIR, np.zeros(3))
    return pairs, np.array(motion)


def device_entries(pool, motion, precision):
    """Contact, distance and cast records of the pool through the device entries on torch tensors, with
    workspaces sized by the *_workspace_bytes functions."""
    import torch
    dev = torch.device("cuda", 0)
    n = pool.n_pairs
    verts, off, cnt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pool.verts, pool.hull_off, pool.hull_cnt))
    prs = torch.from_numpy(pool.pairs.reshape(-1).copy()).to(dev)
    mot = torch.from_numpy(np.ascontiguousarray(motion, np.float64).reshape(-1)).to(dev)
    rb = gjkepa.record_dtype(precision).itemsize
    sizes = (gjkepa.workspace_bytes(n), gjkepa.distance_workspace_bytes(n), gjkepa.cast_workspace_bytes(n))
    ws, dws, cws = (torch.zeros(b, dtype=torch.uint8, device=dev) for b in sizes)
    contact = torch.zeros(n * rb, dtype=torch.uint8, device=dev)
    dist = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    cast = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    work = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(work):
        s = work.cuda_stream
        gjkepa.gjkepa_batch_device(2, 1.0, pool.dtype_code, precision, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(),
                                   prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), sizes[0], s)
        gjkepa.distance_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                     contact.data_ptr(), precision, float("inf"), dist.data_ptr(), dws.data_ptr(),
                                     sizes[1], s)
        gjkepa.cast_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                 mot.data_ptr(), TAU, contact.data_ptr(), precision, cast.data_ptr(), cws.data_ptr(),
                                 sizes[2], s)
    torch.cuda.synchronize(dev)
    return tuple(t.cpu().numpy().tobytes() for t in (contact, dist, cast))


@pytest.mark.parametrize("dtype,precision", [(np.float64, gjkepa.PREC_F64), (np.float32, gjkepa.PREC_F32)],
                         ids=["f64", "f32"])
def test_entries_share_staging(orc, dtype, precision):
    pairs_a, motion_a = pair_list(0.0)
    a = gjkepa.HullPool.from_pairs(pairs_a, dtype)
    pairs_b, motion_b = pairs_a, [motion_a]
    for i in range(1, 4):                                   # pool B: A four times, the copies moved apart
        more, m = pair_list(np.array([10.0 * i, 0.0, 0.0]))
        pairs_b = pairs_b + more
        motion_b.append(m)
    b = gjkepa.HullPool.from_pairs(pairs_b, dtype)
    motion_b = np.concatenate(motion_b)
    assert a.n_pairs == 65 and b.n_pairs == 260 and b.verts.size == 4 * a.verts.size
    clouds = gjkepa.synth_clouds(21, 300, 4, 256, 0)
    scene = scene_with_invalid()                            # holds an empty hull and one of 300 vertices

    rec1 = gjkepa.gjkepa_batch(a, precision=precision)                       # 1
    dist1 = gjkepa.distance_batch(a, rec1)                                   # 2
    cast1 = gjkepa.cast_batch(a, motion_a, TAU, rec1)                        # 3
    hulls = gjkepa.hull_batch(clouds)                                        # 4
    cand, n_cand = gjkepa.broadphase(scene)                                  # 5
    hit_pairs, hit_recs, n_cand2 = gjkepa.collide(scene)                     # 6
    rec_b = gjkepa.gjkepa_batch(b, precision=precision)                      # 7
    dist_b = gjkepa.distance_batch(b)                                        # 8
    cast_b = gjkepa.cast_batch(b, motion_b, TAU)                             # 9
    rec2 = gjkepa.gjkepa_batch(a, precision=precision)                       # 10
    dist2 = gjkepa.distance_batch(a, rec2)                                   # 11
    cast2 = gjkepa.cast_batch(a, motion_a, TAU, rec2)                        # 12

    assert rec2.tobytes() == rec1.tobytes()
    assert dist2.tobytes() == dist1.tobytes()
    assert cast2.tobytes() == cast1.tobytes()
    want = device_entries(a, motion_a, precision)
    assert rec1.tobytes() == want[0]
    assert dist1.tobytes() == want[1]
    assert cast1.tobytes() == want[2]
    # the pool does what it was built for: hits and misses, the bad pair, impacts, every tier bracket
    hit = rec1["collision"] != 0
    assert 10 < hit.sum() < 55 and rec1["status"][BAD_PAIR] == gjkepa.STATUS_BAD_INPUT
    assert dist1["status"][BAD_PAIR] == gjkepa.STATUS_BAD_INPUT and cast1["status"][BAD_PAIR] == gjkepa.STATUS_BAD_INPUT
    assert ((dist1["flags"] & gjkepa.DIST_HIT) != 0).tolist() == hit.tolist()
    assert ((cast1["flags"] & gjkepa.CAST_SKIPPED) != 0).tolist() == hit.tolist()
    assert ((cast1["flags"] & gjkepa.CAST_IMPACT) != 0).sum() > 10
    big = a.hull_cnt[a.pairs].max(axis=1)
    assert all(((big > lo) & (big <= hi)).any() for lo, hi in ((0, 32), (32, 128), (128, 256)))
    # pool B's first copy is pool A: pairs are independent, so its records are A's (without contact
    # records the hits are answered too, so only the other pairs compare)
    assert rec_b[:65].tobytes() == rec1.tobytes()
    assert dist_b[:65][~hit].tobytes() == dist1[~hit].tobytes()
    assert cast_b[:65][~hit].tobytes() == cast1[~hit].tobytes()
    # hulls, broad phase and collide against the oracle, as their own tests compare them
    assert_same(hulls, orc.hull_batch(clouds.verts, clouds.cloud_off, clouds.cloud_cnt), clouds, "after the pair entries")
    want_cand, want_n = orc.broadphase(scene.verts, scene.hull_off, scene.hull_cnt)
    assert n_cand == want_n == n_cand2
    np.testing.assert_array_equal(cand.reshape(-1, 2), want_cand.reshape(-1, 2))
    want_p, want_r, _ = expected(orc, scene)
    np.testing.assert_array_equal(hit_pairs, want_p)
    assert hit_recs.tobytes() == want_r.tobytes()


def test_two_threads_on_one_device():
    """distance_batch and cast_batch share d_rec / d_out / d_ws: called from two host threads at once,
    every result is the single-threaded one."""
    pairs, motion = pair_list(0.0)
    pool = gjkepa.HullPool.from_pairs(pairs, np.float64)
    rec = gjkepa.gjkepa_batch(pool)
    want_dist = gjkepa.distance_batch(pool, rec).tobytes()
    want_cast = gjkepa.cast_batch(pool, motion, TAU, rec).tobytes()
    got = {"dist": [], "cast": []}
    start = threading.Barrier(2)

    def run(key, fn):
        start.wait()
        for _ in range(8):
            got[key].append(fn().tobytes())

    threads = [threading.Thread(target=run, args=("dist", lambda: gjkepa.distance_batch(pool, rec))),
               threading.Thread(target=run, args=("cast", lambda: gjkepa.cast_batch(pool, motion, TAU, rec)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got["dist"] == [want_dist] * 8
    assert got["cast"] == [want_cast] * 8
