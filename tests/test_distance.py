"""gjkepa_distance_batch(_device) on the GPU: the separation distance and closest points of the pairs
the narrow phase calls a miss.

Every separated record certifies itself (distance_ref.check_certificate): the witness points rebuilt
from lambda / code lie in the hulls and bound the distance from above, the support gap along the
record's normal bounds it from below, and the two must agree within 1e-6 relative + 1e-9 — for hulls
of any size, with no reference implementation.  Small hulls are also compared with brute force.

Measured on an MI355X (fp32 storage): the largest iteration count over all pools below is 12 (cap 64);
worst relative gap between the certified bounds 1.9e-9; worst relative error against brute force 1.4e-14.
"""
import numpy as np
import pytest

import distance_ref as dr
import gjkepa

pytestmark = pytest.mark.gpu

SEED = 0xD157
POOLS = {"8-32": (8, 32, 1500), "1-4": (1, 4, 600), "33-256": (33, 256, 300)}
OVERLAP, HIT, FAR = gjkepa.DIST_OVERLAP, gjkepa.DIST_HIT, gjkepa.DIST_FAR


def boundary_pool():
    """Hulls of 1, 2, 3, 4, 8, 32, 33, 128, 129 and 256 unit-sphere vertices (every tier edge), one set
    about the origin and one about (3, 0.5, 0.25), and every pair of one from each set: all separated
    by more than 1.  Values are fp32-exact."""
    sizes = [1, 2, 3, 4, 8, 32, 33, 128, 129, 256]
    rng = np.random.default_rng(SEED)
    chunks, off, cnt, o = [], [], [], 0
    for centre in ((0.0, 0.0, 0.0), (3.0, 0.5, 0.25)):
        for n in sizes:
            u = rng.normal(size=(n, 3))
            h = (u / np.linalg.norm(u, axis=1, keepdims=True) + centre).astype(np.float32)
            chunks.append(h.T.reshape(-1))
            off.append(o)
            cnt.append(n)
            o += 3 * n
    m = len(sizes)
    pairs = np.array([(i, m + j) for i in range(m) for j in range(m)], np.int32)
    return gjkepa.HullPool(np.concatenate(chunks), np.asarray(off, np.int64), np.asarray(cnt, np.int32), pairs)


class Case:
    def __init__(self, pool, orc):
        self.pool = pool
        self.hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
        self.miss = np.nonzero(~self.hit)[0]
        self.rec = gjkepa.distance_batch(pool)              # records=None, max_distance=inf
        assert self.rec.dtype == gjkepa.DIST64 and self.rec.shape == (pool.n_pairs,)
        assert (~self.hit).mean() >= 0.30, "the pool has too few misses to test anything"


@pytest.fixture(scope="module")
def cases(orc):
    c = {k: Case(gjkepa.synth_pairs(SEED, n, lo, hi, 4.0), orc) for k, (lo, hi, n) in POOLS.items()}
    c["boundary"] = Case(boundary_pool(), orc)
    c["8-12"] = Case(gjkepa.synth_pairs(SEED, 200, 8, 12, 4.0), orc)
    return c


@pytest.mark.parametrize("name", ["8-32", "1-4", "33-256", "boundary"])
def test_certificate(cases, name):
    c = cases[name]
    r = c.rec[c.miss]
    assert (r["status"] == gjkepa.STATUS_OK).all() and (r["flags"] == 0).all()
    if name == "boundary":
        assert len(c.miss) == c.pool.n_pairs
        assert ([8, 256] == c.pool.hull_cnt[c.pool.pairs]).all(axis=1).any()
    upper, lower = dr.check_certificate(c.pool, c.rec, c.miss)
    assert (np.abs(upper - lower) <= 2 * dr.tol(upper)).all()
    print(f"{name}: {len(c.miss)} separated pairs, smallest distance {r['distance'].min():.3e}, "
          f"largest iteration count {c.rec['iters'].max()}")
    assert 1 <= c.rec["iters"][c.miss].min() and c.rec["iters"].max() <= 64
    assert (c.rec["pad"] == 0).all() and (c.rec["reserved"] == 0).all()


@pytest.mark.parametrize("name", ["1-4", "8-12"])
def test_brute_force(cases, name):
    c = cases[name]
    ref = dr.pool_distances(c.pool, c.miss)
    err = np.abs(c.rec["distance"][c.miss] - ref)
    print(f"{name}: {len(c.miss)} pairs against brute force, worst relative error {(err / ref).max():.2e}")
    assert (err <= dr.tol(ref)).all()


@pytest.mark.parametrize("name", ["8-32", "1-4", "33-256"])
def test_agrees_with_the_narrow_phase(cases, name):
    c = cases[name]
    assert np.array_equal((c.rec["flags"] & OVERLAP) != 0, c.hit)
    ov = c.rec[c.hit]
    assert (ov["distance"] == 0).all() and (ov["n_simplex"] == 0).all() and (ov["code"] == 0xFFFFFFFF).all()
    assert (ov["point_a"] == 0).all() and (ov["normal"] == 0).all() and (ov["lambda"] == 0).all()
    for prec in (gjkepa.PREC_F64, gjkepa.PREC_F32):
        contact = gjkepa.gjkepa_batch(c.pool, 2, 1.0, precision=prec)
        assert np.array_equal(contact["collision"] != 0, c.hit)
        r = gjkepa.distance_batch(c.pool, records=contact)
        assert np.array_equal((r["flags"] & HIT) != 0, c.hit)
        skipped = r[c.hit]
        assert (skipped["flags"] == HIT).all() and (skipped["distance"] == 0).all() and (skipped["iters"] == 0).all()
        assert r[c.miss].tobytes() == c.rec[c.miss].tobytes()


@pytest.mark.parametrize("name", ["8-32", "1-4", "33-256", "8-12"])
def test_max_distance(cases, name):
    c = cases[name]
    cut = gjkepa.distance_batch(c.pool, max_distance=0.5)
    far = (cut["flags"] & FAR) != 0
    assert far.any() and not (far & c.hit).any()
    assert (cut["flags"][far] == FAR).all() and (cut["status"][far] == gjkepa.STATUS_OK).all()
    # FAR is a proof: the record's own lower bound, and the full run's certified distance, exceed 0.5
    idx = np.nonzero(far)[0]
    assert (cut["distance"][idx] > 0.5).all()
    dr.check_certificate(c.pool, cut, idx, far=True)
    assert (c.rec["distance"][idx] > 0.5).all()
    if name in ("1-4", "8-12"):
        ref = dr.pool_distances(c.pool, idx)
        assert (ref + dr.tol(ref) > 0.5).all()
    full = c.rec["distance"][idx]
    assert (cut["distance"][idx] <= full + dr.tol(full)).all()
    # everything that did not stop early is the +inf run's record, and within the bound
    assert cut[~far].tobytes() == c.rec[~far].tobytes()
    near = ~far & ~c.hit
    assert (cut["distance"][near] <= 0.5 + dr.tol(0.5)).all()
    print(f"{name}: {far.sum()} of {len(c.miss)} separated pairs FAR at 0.5; iterations {cut['iters'][far].mean():.2f} "
          f"against {c.rec['iters'][far].mean():.2f} without the bound")


def test_storage_dtype_and_determinism(cases):
    c = cases["8-32"]
    assert gjkepa.distance_batch(c.pool.as_dtype(np.float64)).tobytes() == c.rec.tobytes()
    assert gjkepa.distance_batch(c.pool).tobytes() == c.rec.tobytes()
    big = cases["33-256"]
    assert gjkepa.distance_batch(big.pool.as_dtype(np.float64)).tobytes() == big.rec.tobytes()
    assert gjkepa.distance_batch(big.pool).tobytes() == big.rec.tobytes()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_prefix_batches_agree(cases, n):
    c = cases["8-32"]
    p = c.pool
    r = gjkepa.distance_batch(gjkepa.HullPool(p.verts, p.hull_off, p.hull_cnt, p.pairs[:n]))
    assert r.tobytes() == c.rec[:n].tobytes()


def test_bad_input_leaves_neighbours_alone(cases):
    c = cases["8-32"]
    p = c.pool
    verts, cnt = p.verts.copy(), p.hull_cnt.copy()
    nan_pair, zero_pair, big_pair = 10, 70, 131                # three different 64-pair chunks
    verts[int(p.hull_off[p.pairs[nan_pair, 1]]) + 2] = np.nan
    cnt[p.pairs[zero_pair, 0]] = 0
    cnt[p.pairs[big_pair, 1]] = 257
    r = gjkepa.distance_batch(gjkepa.HullPool(verts, p.hull_off, cnt, p.pairs))
    bad = [nan_pair, zero_pair, big_pair]
    assert (r["status"][bad] == gjkepa.STATUS_BAD_INPUT).all()
    assert (r["distance"][bad] == 0).all() and (r["flags"][bad] == 0).all() and (r["n_simplex"][bad] == 0).all()
    keep = np.ones(p.n_pairs, bool)
    keep[bad] = False
    assert r[keep].tobytes() == c.rec[keep].tobytes()


def test_device_entry_chained_after_the_batch_and_captured(cases):
    """gjkepa_batch_device then gjkepa_distance_batch_device on one stream, eager and as a captured
    graph replayed twice: the bytes of the host entry with the batch's records."""
    import torch
    c = cases["33-256"]
    pool, n = c.pool, c.pool.n_pairs
    dev = torch.device("cuda", 0)
    verts = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.hull_off).to(dev)
    cnt = torch.from_numpy(pool.hull_cnt).to(dev)
    prs = torch.from_numpy(pool.pairs.reshape(-1).copy()).to(dev)
    wsb, dwsb = gjkepa.workspace_bytes(n), gjkepa.distance_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    dws = torch.zeros(dwsb, dtype=torch.uint8, device=dev)
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)

    def run(out, stream):
        gjkepa.gjkepa_batch_device(2, 1.0, pool.dtype_code, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(),
                                   cnt.data_ptr(), prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb, stream)
        gjkepa.distance_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(),
                                     n, contact.data_ptr(), gjkepa.PREC_F64, float("inf"), out.data_ptr(),
                                     dws.data_ptr(), dwsb, stream)

    expect = gjkepa.distance_batch(pool, records=gjkepa.gjkepa_batch(pool, 2, 1.0))
    work = torch.cuda.Stream(dev)
    eager = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(work):
        run(eager, work.cuda_stream)
    torch.cuda.synchronize(dev)
    assert eager.cpu().numpy().tobytes() == expect.tobytes()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    with torch.cuda.graph(g, stream=side):
        run(out, side.cuda_stream)
    torch.cuda.synchronize(dev)
    for _ in range(2):
        with torch.cuda.stream(work):
            out.zero_()
            g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager)
    del g
