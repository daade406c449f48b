"""gjkepa_manifold_batch(_device) on the GPU: the contact manifold (up to 4 points) of colliding pairs.

The records are checked as tests/test_manifold_host.py checks the host program's (tests/manifold_ref.py),
with contact records from gjkepa_batch, on the box, sphere, prism and tier-boundary pools and the known
answers; and they equal the host program's bytes on every pool, for fp32 and fp64 storage, for batch
prefixes around a 64-pair chunk, from run to run, from the device entry and from a captured graph.

Measured on an MI355X over the pools below: no pair excluded, none with FALLBACK; box pool 233 hits of
260 with 126 four-point and 107 one-point patches, smallest area against the reference polygon 0.6235
(prism pool 0.6323 with 18 decimated records, the 45-degree octagon 0.7071; the bound is 0.25); every
hit of the sphere and tier-boundary pools is one point; largest |depth - penetration_depth| 6.7e-16 but
for the prism pool's 9.0e-11 (EPA's convergence on a 128-gon; reported, not asserted).
"""
import shutil

import numpy as np
import pytest

import gjkepa
import manifold_ref as mr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")]


class Case:
    def __init__(self, pool):
        self.pool = pool
        self.contact = gjkepa.gjkepa_batch(pool, 2, 1.0)
        self.rec = gjkepa.manifold_batch(pool, self.contact, mr.MARGIN)
        assert self.rec.dtype == gjkepa.MANIFOLD64 and self.rec.shape == (pool.n_pairs,)


@pytest.fixture(scope="module")
def cases():
    c = {"box": Case(mr.box_pool()), "prism": Case(mr.prism_pool()), "boundary": Case(mr.tier_boundary_pool())}
    for name in mr.SPHERE_POOLS:
        c["sphere " + name] = Case(mr.sphere_pool(name))
    answers = mr.known_answers()
    c["known"] = Case(gjkepa.HullPool.from_pairs([(answers[k][0], answers[k][1]) for k in answers]))
    return c


POOLS = ["box", "sphere 1-4", "sphere 8-32", "sphere 33-256", "prism", "boundary", "known"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return mr.build_manifold_host(tmp_path_factory.mktemp("manifold_host_gpu"))


@pytest.mark.parametrize("name", POOLS)
def test_records_pass_the_checks(cases, name):
    c = cases[name]
    comp, hist = mr.check_pool(c.pool, c.contact, c.rec, name=name + " pool",
                               min_hits=100 if name == "box" else 7 if name == "known" else 30)
    # NO_HIT <=> the batch's collision byte is clear or its status is not OK
    assert np.array_equal((c.rec["flags"] & mr.NO_HIT) != 0, (c.contact["collision"] == 0) | (c.contact["status"] != 0))
    if name == "box":
        assert hist[4] >= 100, hist
    if name == "boundary":
        mr.check_boundary_cover(c.pool, comp)
    if name == "prism":
        k = np.repeat(mr.PRISM_K, len(c.rec) // len(mr.PRISM_K))
        dec = (c.rec["flags"] & mr.DECIMATED) != 0
        assert not dec[comp & (k <= 32)].any() and dec[comp & (k >= 33)].any()


def test_known_answers(cases):
    answers = mr.known_answers()
    c = cases["known"]
    assert (c.contact["collision"] != 0).all() and (c.contact["status"] == 0).all()
    mr.check_known(c.rec, list(answers), answers)


@pytest.mark.parametrize("name", POOLS)
def test_kernel_and_host_program_give_the_same_bytes(cases, host, name):
    """csrc/manifold_clip.h is one text for the kernel and for tests/manifold_host.cpp, and the kernel's
    lane-parallel heights, membership and ranks are the plain scan's"""
    c = cases[name]
    assert host(c.pool, c.contact, mr.MARGIN).tobytes() == c.rec.tobytes()


def test_storage_dtype_determinism_and_prefixes(cases):
    for name in ("sphere 8-32", "sphere 33-256", "boundary"):           # fp32-exact values
        c = cases[name]
        assert c.pool.verts.dtype == np.float32
        assert gjkepa.manifold_batch(c.pool.as_dtype(np.float64), c.contact, mr.MARGIN).tobytes() == c.rec.tobytes()
    for name in ("box", "prism"):                                        # repeated runs
        c = cases[name]
        for _ in range(2):
            assert gjkepa.manifold_batch(c.pool, c.contact, mr.MARGIN).tobytes() == c.rec.tobytes()
    c = cases["box"]
    p = c.pool
    for n in (1, 63, 64, 65):
        r = gjkepa.manifold_batch(gjkepa.HullPool(p.verts, p.hull_off, p.hull_cnt, p.pairs[:n]), c.contact[:n], mr.MARGIN)
        assert r.tobytes() == c.rec[:n].tobytes()


def test_f32_records_and_bad_input(cases, host):
    c = cases["sphere 8-32"]
    p = c.pool
    c32 = gjkepa.gjkepa_batch(p, 2, 1.0, precision=gjkepa.PREC_F32)
    r32 = gjkepa.manifold_batch(p, c32, mr.MARGIN)
    assert r32.tobytes() == host(p, c32, mr.MARGIN).tobytes()
    assert (r32["normal"] == c32["collision_normal"].astype(np.float64)).all()
    assert np.array_equal((r32["flags"] & mr.NO_HIT) != 0, ~mr.is_computed(c32))
    # bad counts first, NaN vertices where a pair is computed, unusable records: the neighbours keep their bytes
    hits, miss = np.nonzero(mr.is_computed(c.contact))[0], np.nonzero(~mr.is_computed(c.contact))[0]
    verts, cnt, contact = p.verts.copy(), p.hull_cnt.copy(), c.contact.copy()
    cnt[p.pairs[miss[0], 0]] = 0
    cnt[p.pairs[hits[3], 1]] = 257
    verts[int(p.hull_off[p.pairs[hits[4], 1]]) + 1] = np.nan
    verts[int(p.hull_off[p.pairs[miss[1], 0]])] = np.nan
    contact["status"][hits[0]] = gjkepa.STATUS_EPA_MAXITER
    contact["collision_normal"][hits[1]] = 0
    contact["collision_normal"][hits[2], 1] = np.nan
    bad_pool = gjkepa.HullPool(verts, p.hull_off, cnt, p.pairs)
    r = gjkepa.manifold_batch(bad_pool, contact, mr.MARGIN)
    assert r.tobytes() == host(bad_pool, contact, mr.MARGIN).tobytes()
    bad = [miss[0], hits[3], hits[4]]
    assert (r["status"][bad] == gjkepa.STATUS_BAD_INPUT).all() and (r["flags"][bad] == 0).all() and (r["n_points"][bad] == 0).all()
    assert (r["flags"][hits[:3]] == mr.NO_HIT).all() and r["flags"][miss[1]] == mr.NO_HIT
    keep = np.ones(p.n_pairs, bool)
    keep[bad + list(hits[:3])] = False
    assert r[keep].tobytes() == c.rec[keep].tobytes()


def test_device_entry_chained_after_the_batch_and_captured(cases):
    """gjkepa_batch_device then gjkepa_manifold_batch_device on one stream, eager and as a captured graph
    replayed twice: the bytes of the host entry."""
    import torch
    c = cases["box"]
    pool, n = c.pool, c.pool.n_pairs
    dev = torch.device("cuda", 0)
    verts = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.hull_off).to(dev)
    cnt = torch.from_numpy(pool.hull_cnt).to(dev)
    prs = torch.from_numpy(pool.pairs.reshape(-1).copy()).to(dev)
    wsb, mwsb = gjkepa.workspace_bytes(n), gjkepa.manifold_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    mws = torch.zeros(mwsb, dtype=torch.uint8, device=dev)
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)

    def run(out, stream):
        gjkepa.gjkepa_batch_device(2, 1.0, pool.dtype_code, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(),
                                   cnt.data_ptr(), prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb, stream)
        gjkepa.manifold_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                     contact.data_ptr(), gjkepa.PREC_F64, mr.MARGIN, out.data_ptr(), mws.data_ptr(), mwsb,
                                     stream)

    work = torch.cuda.Stream(dev)
    eager = torch.zeros(n * 160, dtype=torch.uint8, device=dev)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(work):
        run(eager, work.cuda_stream)
    torch.cuda.synchronize(dev)
    assert eager.cpu().numpy().tobytes() == c.rec.tobytes()
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
