"""gjkepa_manifold_cast_batch(_device), gjkepa_event_manifolds_device and gjkepa_collide_moving_patches on the
GPU: the contact manifold at the time of impact and the patches of a moving step's events.

Cast records come from gjkepa.cast_rigid_batch and contact records from gjkepa.gjkepa_batch.  The kernel's bytes
equal the host program's (tests/impact_host.cpp) on the pools of tests/test_manifold_cast_host.py and on the known
answers, in both storage dtypes, for prefixes around a 64-pair chunk and from run to run; the pairs the cast
skipped get gjkepa.manifold_batch's bytes; the points agree with gjkepa.pose_pool's vertices at the pair's toi;
canaries stay intact; the device entry runs on a stream and in a captured chain that is replayed on rewritten
motions; the gather and the one-call step equal the composition."""
import shutil

import numpy as np
import pytest

import cast_rigid_ref as rr
import events_ref as er
import gjkepa
import impact_ref as ir
import manifold_ref as mr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")]
CANARY = 0xA5
SKIPPED = gjkepa.CAST_SKIPPED


class Case:
    """a pool with its motions, the batch's contact records, the rigid cast's records with them, and the
    manifolds at the time of impact with them"""

    def __init__(self, pool, bm):
        self.pool, self.bm = pool, np.asarray(bm, float).reshape(-1, 9)
        self.contact = gjkepa.gjkepa_batch(pool, 2, 1.0)
        self.cast = gjkepa.cast_rigid_batch(pool, self.bm, ir.TAU, records=self.contact)
        self.rec = gjkepa.manifold_cast_batch(pool, self.bm, self.cast, ir.MARGIN, records=self.contact)
        assert self.rec.dtype == gjkepa.MANIFOLD64 and self.rec.shape == (pool.n_pairs,)


def mixed_pool():
    """stacks in contact (the cast skips them) and lifted stacks (the cast finds their impacts) in one list"""
    stacks = mr.box_pool(n=60)
    lifted, bm_l = ir.lifted_box_pool(n=60, seed=0x5C1D)
    hulls = [(stacks.hull(int(a)), stacks.hull(int(b))) for a, b in stacks.pairs] + \
            [(lifted.hull(int(a)), lifted.hull(int(b))) for a, b in lifted.pairs]
    return gjkepa.HullPool.from_pairs(hulls), np.concatenate([rr.motions(stacks, 0x77), bm_l])


@pytest.fixture(scope="module")
def cases():
    known = ir.known_pool()
    return {"box": Case(*ir.lifted_box_pool()), "boundary": Case(*ir.boundary_pool()), "mixed": Case(*mixed_pool()),
            "known": Case(known[1], known[2])}


POOLS = ["box", "boundary", "mixed", "known"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ir.build_impact_host(tmp_path_factory.mktemp("impact_host_gpu"))


@pytest.mark.parametrize("name", POOLS)
def test_kernel_and_host_program_give_the_same_bytes(cases, host, name):
    """csrc/manifold_clip.h and csrc/rigid_pose.h are one text for the kernel and for tests/impact_host.cpp"""
    c = cases[name]
    assert host(c.pool, c.bm, c.cast, ir.MARGIN, c.contact).tobytes() == c.rec.tobytes()
    bare = gjkepa.manifold_cast_batch(c.pool, c.bm, c.cast, ir.MARGIN)
    assert host(c.pool, c.bm, c.cast, ir.MARGIN).tobytes() == bare.tobytes()
    # the other storage dtype of the same values (fp32-exact for the boundary pool, rounded for the others)
    other = c.pool.as_dtype(np.float32 if c.pool.verts.dtype == np.float64 else np.float64)
    con = gjkepa.gjkepa_batch(other, 2, 1.0)
    cast = gjkepa.cast_rigid_batch(other, c.bm, ir.TAU, records=con)
    got = gjkepa.manifold_cast_batch(other, c.bm, cast, ir.MARGIN, records=con)
    assert host(other, c.bm, cast, ir.MARGIN, con).tobytes() == got.tobytes()
    if name == "boundary":
        assert got.tobytes() == c.rec.tobytes()


def test_records_pass_the_checks(cases):
    c = cases["box"]
    assert not (c.cast["flags"] & SKIPPED).any()
    comp, hist = ir.check_pool(c.pool, c.bm, c.cast, c.rec, name="box pool")
    assert hist.sum() >= 100 and hist[4] >= 30, hist
    c = cases["boundary"]
    comp, _ = ir.check_pool(c.pool, c.bm, c.cast, c.rec, name="tier-boundary pool")
    ir.check_brackets(c.pool, comp)
    c = cases["known"]
    worst = ir.check_known(c.rec, c.cast, ir.known_cases(), c.bm)
    assert worst <= ir.POSITION_BOUND and worst <= 0.1 * ir.POSITION_BOUND, worst


def test_prefixes_and_repeated_runs(cases):
    c = cases["mixed"]
    p = c.pool
    for _ in range(2):
        assert gjkepa.manifold_cast_batch(p, c.bm, c.cast, ir.MARGIN, records=c.contact).tobytes() == c.rec.tobytes()
    for n in (1, 63, 64, 65):
        r = gjkepa.manifold_cast_batch(gjkepa.HullPool(p.verts, p.hull_off, p.hull_cnt, p.pairs[:n]), c.bm, c.cast[:n],
                                       ir.MARGIN, records=c.contact[:n])
        assert r.tobytes() == c.rec[:n].tobytes()
    b = cases["box"]
    q = b.pool
    for n in (1, 63, 64, 65):
        r = gjkepa.manifold_cast_batch(gjkepa.HullPool(q.verts, q.hull_off, q.hull_cnt, q.pairs[:n]), b.bm, b.cast[:n], ir.MARGIN)
        assert r.tobytes() == b.rec[:n].tobytes()


def test_skipped_pairs_equal_the_contact_manifold(cases):
    c = cases["mixed"]
    sk = (c.cast["flags"] & SKIPPED) != 0
    assert sk.sum() >= 50 and (~sk).sum() >= 50
    want = gjkepa.manifold_batch(c.pool, c.contact, ir.MARGIN)
    assert c.rec[sk].tobytes() == want[sk].tobytes()
    assert ((c.rec["flags"][~sk] & ir.NO_HIT) == 0).sum() >= 30
    c32 = gjkepa.gjkepa_batch(c.pool, 2, 1.0, precision=gjkepa.PREC_F32)
    cast32 = gjkepa.cast_rigid_batch(c.pool, c.bm, ir.TAU, records=c32)
    sk32 = (cast32["flags"] & SKIPPED) != 0
    got = gjkepa.manifold_cast_batch(c.pool, c.bm, cast32, ir.MARGIN, records=c32)
    assert got[sk32].tobytes() == gjkepa.manifold_batch(c.pool, c32, ir.MARGIN)[sk32].tobytes()
    # a SKIPPED pair does not read its motion blocks
    nan_bm = c.bm.copy()
    nan_bm[c.pool.pairs[sk].reshape(-1)] = np.nan
    again = gjkepa.manifold_cast_batch(c.pool, nan_bm, c.cast, ir.MARGIN, records=c.contact)
    assert again.tobytes() == c.rec.tobytes()


def test_points_are_pose_pool_vertices_at_the_time_of_impact(cases):
    """a point whose code names one vertex of one hull is that vertex where gjkepa_pose_pool (fp64 out) puts it at
    the pair's toi, moved along n onto A's support plane: the two in-plane coordinates agree within the bound
    measured on the host program"""
    checked = 0
    for name in ("box", "known"):
        c = cases[name]
        time = np.zeros(len(c.pool.hull_cnt))
        time[c.pool.pairs[:, 0]] = c.cast["toi"]
        time[c.pool.pairs[:, 1]] = c.cast["toi"]
        posed = gjkepa.pose_pool(c.pool, c.bm, time, np.float64)
        for k in np.nonzero(ir.computed_mask(c.cast))[0]:
            r = c.rec[k]
            n = r["normal"]
            u, w = mr.plane_frame(n)
            for p, code in zip(r["point"][:r["n_points"]], r["code"]):
                ia, ib = int(code & 0xFFFF), int(code >> 16)
                if (ia == 0xFFFF) == (ib == 0xFFFF):
                    continue
                v = posed.hull(int(c.pool.pairs[k, 0]))[ia] if ib == 0xFFFF else posed.hull(int(c.pool.pairs[k, 1]))[ib]
                d = p - v
                assert abs(d @ u) <= ir.POSITION_BOUND and abs(d @ w) <= ir.POSITION_BOUND, (name, k, d @ u, d @ w)
                checked += 1
    assert checked >= 200


def _up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def test_device_entry_on_a_stream_with_canaries(cases):
    import torch
    c = cases["mixed"]
    pool, n = c.pool, c.pool.n_pairs
    dev = torch.device("cuda", 0)
    verts, off, cnt, prs = _up(pool.verts, dev), _up(pool.hull_off, dev), _up(pool.hull_cnt, dev), _up(pool.pairs, dev)
    mot, cast, con = _up(c.bm, dev), _up(c.cast, dev), _up(c.contact, dev)
    wsb = gjkepa.manifold_cast_workspace_bytes(n)
    ws = torch.full((wsb + 256,), CANARY, dtype=torch.uint8, device=dev)
    out = torch.full(((n + 1) * 160,), CANARY, dtype=torch.uint8, device=dev)
    work = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(work):
        gjkepa.manifold_cast_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                          mot.data_ptr(), cast.data_ptr(), con.data_ptr(), gjkepa.PREC_F64, ir.MARGIN,
                                          out.data_ptr(), ws.data_ptr(), wsb, work.cuda_stream)
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    assert got[:n * 160].tobytes() == c.rec.tobytes()
    assert (got[n * 160:] == CANARY).all() and (ws[wsb:] == CANARY).all()


def test_captured_chain_replayed_on_rewritten_motions(cases):
    """gjkepa_batch_device -> gjkepa_cast_rigid_batch_device -> gjkepa_manifold_cast_batch_device on one stream as a
    captured graph, replayed once after the motions are rewritten in place: the host entries' bytes for them"""
    import torch
    c = cases["mixed"]
    pool, n = c.pool, c.pool.n_pairs
    dev = torch.device("cuda", 0)
    verts, off, cnt, prs = _up(pool.verts, dev), _up(pool.hull_off, dev), _up(pool.hull_cnt, dev), _up(pool.pairs, dev)
    mot = _up(c.bm, dev)
    wsb, cwsb, mwsb = gjkepa.workspace_bytes(n), gjkepa.cast_rigid_workspace_bytes(n), gjkepa.manifold_cast_workspace_bytes(n)
    ws, cws, mws = (torch.zeros(b, dtype=torch.uint8, device=dev) for b in (wsb, cwsb, mwsb))
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    cast = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 160, dtype=torch.uint8, device=dev)

    def run(stream):
        gjkepa.gjkepa_batch_device(2, 1.0, pool.dtype_code, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(),
                                   prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb, stream)
        gjkepa.cast_rigid_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                       mot.data_ptr(), ir.TAU, contact.data_ptr(), gjkepa.PREC_F64, cast.data_ptr(),
                                       cws.data_ptr(), cwsb, stream)
        gjkepa.manifold_cast_batch_device(pool.dtype_code, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                          mot.data_ptr(), cast.data_ptr(), contact.data_ptr(), gjkepa.PREC_F64, ir.MARGIN,
                                          out.data_ptr(), mws.data_ptr(), mwsb, stream)

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(g, stream=side):
        run(side.cuda_stream)
    torch.cuda.synchronize(dev)
    bm2 = c.bm.copy()
    bm2[:, 0:3] *= 0.8
    bm2[:, 3:6] *= -0.5
    mot.copy_(_up(bm2, dev))
    out.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    cast2 = gjkepa.cast_rigid_batch(pool, bm2, ir.TAU, records=c.contact)
    want = gjkepa.manifold_cast_batch(pool, bm2, cast2, ir.MARGIN, records=c.contact)
    assert cast.cpu().numpy().tobytes() == cast2.tobytes()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert want.tobytes() != c.rec.tobytes()
    del g


def test_event_manifolds_gather(cases):
    import torch
    c = cases["mixed"]
    n, nh = c.pool.n_pairs, len(c.pool.hull_cnt)
    ev, n_events, _, _, _ = gjkepa.events(c.pool.pairs, c.cast, nh, records=c.contact)
    assert n_events == len(ev) >= 100
    dev = torch.device("cuda", 0)
    d_ev, d_mf = _up(ev, dev), _up(c.rec, dev)
    d_n = torch.tensor([n_events], dtype=torch.int64, device=dev)
    for cap in (n_events, n_events + 5, 0, 1, n_events - 1):
        out = torch.full(((max(cap, n_events) + 1) * 160,), CANARY, dtype=torch.uint8, device=dev)
        gjkepa.event_manifolds_device(d_ev.data_ptr(), d_n.data_ptr(), cap, d_mf.data_ptr(), out.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        got = out.cpu().numpy()
        m = min(cap, n_events)
        assert got[:m * 160].tobytes() == c.rec[ev["pair"][:m]].tobytes(), cap
        assert (got[m * 160:] == CANARY).all(), cap


def test_collide_moving_patches_equals_the_composition():
    pool, bm, _ = er.pipeline_scene(41, 300, 5.0)
    tol = ir.TAU
    res = gjkepa.collide_moving_patches(pool, bm, tol, ir.MARGIN, pose=True)
    ref = gjkepa.collide_moving(pool, bm, tol, pose=True)
    assert res["n_events"] == ref["n_events"] and res["n_candidates"] == ref["n_candidates"]
    assert res["counts"].tolist() == ref["counts"].tolist() and res["events"].tobytes() == ref["events"].tobytes()
    assert res["body_time"].tobytes() == ref["body_time"].tobytes()
    assert res["posed"].verts.tobytes() == ref["posed"].verts.tobytes()
    # entry by entry
    swept, n = gjkepa.broadphase_swept(pool, bm, tol)
    cand = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, swept)
    contact = gjkepa.gjkepa_batch(cand, 2, 1.0)
    cast = gjkepa.cast_rigid_batch(cand, bm, tol, records=contact)
    mf = gjkepa.manifold_cast_batch(cand, bm, cast, ir.MARGIN, records=contact)
    ev = res["events"]
    assert len(ev) == res["n_events"] >= 100
    assert res["patches"].tobytes() == mf[ev["pair"]].tobytes()
    kind, p = ev["kind"], res["patches"]
    hit, at = kind == gjkepa.EVENT_HIT, (kind == gjkepa.EVENT_START) | (kind == gjkepa.EVENT_IMPACT)
    und = kind == gjkepa.EVENT_UNDECIDED
    assert hit.any() and at.any()
    assert ((p["flags"][hit] & ir.AT_TOI) == 0).all() and (p["n_points"][hit & (p["flags"] == 0)] >= 1).all()
    moving = at & (p["status"] == gjkepa.STATUS_OK) & ((p["flags"] & ir.NO_HIT) == 0)
    assert moving.sum() >= 30 and ((p["flags"][moving] & ir.AT_TOI) != 0).all() and (p["n_points"][moving] >= 1).all()
    assert (p["flags"][und] == ir.NO_HIT).all()
    cut = gjkepa.collide_moving_patches(pool, bm, tol, ir.MARGIN, max_events=100)
    assert cut["n_events"] == res["n_events"] and cut["events"].tobytes() == ev[:100].tobytes()
    assert cut["patches"].tobytes() == res["patches"][:100].tobytes()
