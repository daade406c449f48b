"""gjkepa_cast_batch(_device) on the GPU: the linear cast (time of impact) of moving convex pairs.

The records are checked as tests/test_cast_host.py checks the host program's (tests/cast_ref.py): every
IMPACT certifies itself, the reference distance at the time of impact lies in [tau / 2, tau], the
reference first comes within tau no later than that time, misses agree with the swept hull and
overlapping starts with the oracle, for pools of every tier and a pool of hulls at every tier edge.

Measured on an MI355X (fp32 storage) over the pools below: at most 4 advancement steps (mean 1.66 to
1.79 per impact) and 25 GJK iterations per pair; |point_a - point_b| / tau 0.5000 to 0.5001 at tau 1e-6
and up to 0.987 at 1e-3; smallest gap along the normal 0.463 tau; every record equal to the host
program's byte for byte.
"""
import shutil

import numpy as np
import pytest

import cast_ref as cr
import distance_ref as dr
import gjkepa
from test_distance import boundary_pool

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")]

SEED = 0xD157
MOTION_SEED = 0xCA57
TAU = 1e-6
POOLS = {"8-32": (8, 32, 1500), "1-4": (1, 4, 600), "33-256": (33, 256, 300)}


@pytest.fixture(scope="module")
def dist_host(tmp_path_factory):
    return cr.build_distance_host(tmp_path_factory.mktemp("cast_dist"))


class Case:
    def __init__(self, pool, motion, tau, orc, dist_host):
        self.pool, self.motion, self.tau = pool, motion, tau
        self.hit = orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0
        self.rec = gjkepa.cast_batch(pool, motion, tau)            # records=None
        assert self.rec.dtype == gjkepa.CAST64 and self.rec.shape == (pool.n_pairs,)
        self.ref = cr.Reference(dist_host, pool, motion)


@pytest.fixture(scope="module")
def cases(orc, dist_host):
    c = {}
    for k, (lo, hi, n) in POOLS.items():
        pool = gjkepa.synth_pairs(SEED, n, lo, hi, 4.0)
        c[k] = Case(pool, cr.motions(pool, MOTION_SEED), TAU, orc, dist_host)
    c["8-32 coarse"] = Case(c["8-32"].pool, c["8-32"].motion, 1e-3, orc, dist_host)
    return c


@pytest.mark.parametrize("name", ["8-32", "8-32 coarse", "1-4", "33-256"])
def test_casts_certify_and_agree_with_the_reference(cases, dist_host, name):
    c = cases[name]
    cr.check_pool(c.pool, c.motion, c.rec, c.tau, c.ref, c.hit, cr.swept_distance(dist_host, c.ref))
    assert (c.rec["iters"][cr.kinds(c.rec)[0]] >= 2).all()


def test_tier_boundaries(orc, dist_host):
    """Hulls of 1 .. 256 vertices about two centres, hull B moved onto hull A's centre.  Every pair the
    reference sees come within tau / 2 is an IMPACT and certifies, (8, 256) among them; the pairs of
    hulls too small to enclose their centre (points, segments, triangles) may pass each other."""
    pool = boundary_pool()
    motion = np.tile([-3.0, -0.5, -0.25], (pool.n_pairs, 1))
    c = Case(pool, motion, TAU, orc, dist_host)
    assert not c.hit.any()
    cr.check_boundary(pool, motion, c.rec, c.ref, TAU)


@pytest.mark.parametrize("name", ["8-32", "8-32 coarse", "1-4", "33-256"])
def test_kernel_and_host_program_give_the_same_bytes(cases, tmp_path_factory, name):
    """csrc/cast_advance.h is one text for the kernel and for tests/cast_host.cpp, and the kernel's
    support scans return the plain scan's first maximum: the records agree byte for byte."""
    c = cases[name]
    host = cr.build_cast_host(tmp_path_factory.mktemp("cast_host"))
    assert host(c.pool, c.motion, c.tau).tobytes() == c.rec.tobytes()


@pytest.mark.parametrize("name", ["1-4"])
def test_brute_force_at_toi(cases, name):
    c = cases[name]
    ii = np.nonzero(cr.kinds(c.rec)[0])[0]
    d = np.array([dr.pair_distance(c.pool.hull(int(c.pool.pairs[k, 0])),
                                   c.pool.hull(int(c.pool.pairs[k, 1])) + c.rec["toi"][k] * c.motion[k]) for k in ii])
    assert (d <= TAU + dr.tol(TAU)).all() and (d >= 0.5 * TAU - dr.tol(TAU)).all()


@pytest.mark.parametrize("name", ["8-32", "1-4", "33-256"])
def test_records_skip_the_hits(cases, name):
    c = cases[name]
    for prec in (gjkepa.PREC_F64, gjkepa.PREC_F32):
        contact = gjkepa.gjkepa_batch(c.pool, 2, 1.0, precision=prec)
        assert np.array_equal(contact["collision"] != 0, c.hit)
        r = gjkepa.cast_batch(c.pool, c.motion, TAU, records=contact)
        assert np.array_equal((r["flags"] & cr.SKIPPED) != 0, c.hit)
        sk = r[c.hit]
        assert (sk["flags"] == cr.SKIPPED).all() and (sk["toi"] == 0).all() and (sk["iters"] == 0).all()
        assert (sk["steps"] == 0).all() and (sk["n_simplex"] == 0).all() and (sk["status"] == gjkepa.STATUS_OK).all()
        assert r[~c.hit].tobytes() == c.rec[~c.hit].tobytes()


def test_storage_dtype_determinism_and_prefixes(cases):
    for name in ("8-32", "33-256"):
        c = cases[name]
        assert gjkepa.cast_batch(c.pool.as_dtype(np.float64), c.motion, TAU).tobytes() == c.rec.tobytes()
        assert gjkepa.cast_batch(c.pool, c.motion, TAU).tobytes() == c.rec.tobytes()
    c = cases["8-32"]
    p = c.pool
    for n in (1, 63, 65):
        r = gjkepa.cast_batch(gjkepa.HullPool(p.verts, p.hull_off, p.hull_cnt, p.pairs[:n]), c.motion[:n], TAU)
        assert r.tobytes() == c.rec[:n].tobytes()


def test_bad_input_leaves_neighbours_alone(cases):
    c = cases["8-32"]
    p = c.pool
    verts, cnt, motion = p.verts.copy(), p.hull_cnt.copy(), c.motion.copy()
    nan_pair, zero_pair, big_pair, nan_motion = 10, 70, 131, 200        # four different 64-pair chunks
    verts[int(p.hull_off[p.pairs[nan_pair, 1]]) + 2] = np.nan
    cnt[p.pairs[zero_pair, 0]] = 0
    cnt[p.pairs[big_pair, 1]] = 257
    motion[nan_motion, 2] = np.inf
    r = gjkepa.cast_batch(gjkepa.HullPool(verts, p.hull_off, cnt, p.pairs), motion, TAU)
    bad = [nan_pair, zero_pair, big_pair, nan_motion]
    assert (r["status"][bad] == gjkepa.STATUS_BAD_INPUT).all()
    assert (r["toi"][bad] == 0).all() and (r["flags"][bad] == 0).all() and (r["n_simplex"][bad] == 0).all()
    keep = np.ones(p.n_pairs, bool)
    keep[bad] = False
    assert r[keep].tobytes() == c.rec[keep].tobytes()


def test_device_entry_chained_after_the_batch_and_captured(cases):
    """gjkepa_batch_device then gjkepa_cast_batch_device on one stream, eager and as a captured graph
    replayed twice: the bytes of the host entry with the batch's records."""
    import torch
    c = cases["33-256"]
    pool, n = c.pool, c.pool.n_pairs
    dev = torch.device("cuda", 0)
    verts = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.hull_off).to(dev)
    cnt = torch.from_numpy(pool.hull_cnt).to(dev)
    prs = torch.from_numpy(pool.pairs.reshape(-1).copy()).to(dev)
    mot = torch.from_numpy(np.ascontiguousarray(c.motion, np.float64).reshape(-1)).to(dev)
    wsb, cwsb = gjkepa.workspace_bytes(n), gjkepa.cast_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    cws = torch.zeros(cwsb, dtype=torch.uint8, device=dev)
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)

    def run(out, stream):
        gjkepa.gjkepa_batch_device(2, 1.0, pool.dtype_code, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(),
                                   cnt.data_ptr(), prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb, stream)
        gjkepa.cast_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                 mot.data_ptr(), TAU, contact.data_ptr(), gjkepa.PREC_F64, out.data_ptr(),
                                 cws.data_ptr(), cwsb, stream)

    expect = gjkepa.cast_batch(pool, c.motion, TAU, records=gjkepa.gjkepa_batch(pool, 2, 1.0))
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
