"""gjkepa_events_device and gjkepa_collide_moving on the GPU: the event list and the per-body clamp of a moving step.

Synthetic cast and contact records (no upstream kernel) at every size around the key pass's tile: events,
n_events, counts, body_time and body_event equal the numpy restatement of the definition (tests/events_ref.py)
byte for byte, with many events at time 0, IMPACT events sharing one toi, batches of only misses and only events,
a hub body named by 2 000 pairs, a body with only HIT / START events and an unsorted pair list; a cut list keeps
the full counts and body outputs and leaves a canary alone; contact records absent, F64 and F32; two calls on one
workspace agree and the captured chain swept broad phase -> batch -> rigid cast -> events -> pose replays on
rewritten motions; the pipeline scene holds the clamp's guarantee against the distance query; collide_moving
equals the composition.

Pipeline scene (events_ref.pipeline_scene: 2 000 hulls of 8 .. 32 vertices in a box of 16, every fourth at rest,
three bullets, tau = 1e-3), counted on the CPU with the host cast program and the oracle's collision flags and
found again on the GPU: 30 210 swept pairs; 8 773 HIT, 26 START, 4 527 IMPACT (1 466 of them with a resting
partner), 13 UNDECIDED, 0 BAD."""
import functools

import numpy as np
import pytest

import distance_ref as dr
import events_ref as er
import gjkepa

pytestmark = pytest.mark.gpu
T = gjkepa.EVENTS_TILE
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
PIPELINE_COUNTS = [8773, 26, 4527, 13, 0]          # HIT, START, IMPACT, UNDECIDED, BAD
PIPELINE_PAIRS, PIPELINE_RESTING_IMPACTS = 30210, 1466
CANARY = 0xA5


def run(pairs, cast, n_hulls, records=None, max_events=None, bodies=True):
    """gjkepa_events_device over host arrays with a canary record behind events[max_events]; returns
    (events, n_events, counts, body_time, body_event) as gjkepa.events does"""
    import torch
    dev = torch.device("cuda", 0)
    prs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n = len(prs)
    cap = n if max_events is None else max_events
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_prs, d_cast = up(prs), up(cast)
    d_rec = None if records is None else up(records)
    prec = gjkepa.PREC_F32 if records is not None and records.dtype == gjkepa.REC32 else gjkepa.PREC_F64
    d_ev = torch.full(((cap + 1) * 128,), CANARY, dtype=torch.uint8, device=dev)
    d_n = torch.full((6,), -7, dtype=torch.int64, device=dev)
    d_time = torch.full((n_hulls + 1,), -7.0, dtype=torch.float64, device=dev)
    d_rank = torch.full((n_hulls + 1,), -7, dtype=torch.int32, device=dev)
    wsb = gjkepa.events_workspace_bytes(n, n_hulls)
    ws = torch.full((wsb + 256,), CANARY, dtype=torch.uint8, device=dev)
    gjkepa.events_device(d_prs.data_ptr() if n else 0, n, n_hulls, d_cast.data_ptr() if n else 0,
                         0 if d_rec is None else d_rec.data_ptr(), prec, d_ev.data_ptr(), cap, d_n.data_ptr(), d_n.data_ptr() + 8,
                         d_time.data_ptr() if bodies else 0, d_rank.data_ptr() if bodies else 0, ws.data_ptr(), wsb,
                         torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    host_n = d_n.cpu().numpy()
    m = min(int(host_n[0]), cap)
    ev = d_ev.cpu().numpy()
    assert (ev[m * 128:] == CANARY).all(), "written at or past events[min(n_events, max_events)]"
    assert (ws[wsb:] == CANARY).all() and float(d_time[n_hulls]) == -7.0 and int(d_rank[n_hulls]) == -7
    if not bodies:
        assert (d_time == -7.0).all() and (d_rank == -7).all()
        return ev[:m * 128].view(gjkepa.EVENT64).copy(), int(host_n[0]), host_n[1:].copy(), None, None
    return (ev[:m * 128].view(gjkepa.EVENT64).copy(), int(host_n[0]), host_n[1:].copy(), d_time.cpu().numpy()[:n_hulls].copy(),
            d_rank.cpu().numpy()[:n_hulls].copy())


@functools.lru_cache(maxsize=None)
def synthetic(n, only=None):
    """(pairs, cast records, F64 contact records, n_hulls, hub, quiet) of n pairs: an unsorted list over n / 4 + 4
    hulls with every kind (only: one kind for all).  From 3 000 pairs on also 60 IMPACT records sharing one toi, a hub
    body in 1 000 pairs as a and 1 000 as b, all of them IMPACT or UNDECIDED.  The body `quiet` is named by HIT and
    START records alone."""
    rng = np.random.default_rng(1000 + n)
    nh = n // 4 + 6
    hub, quiet = nh - 1, nh - 2
    kind = rng.choice([er.NONE, er.HIT, er.START, er.IMPACT, er.UNDECIDED, er.BAD], size=n, p=[0.4, 0.1, 0.1, 0.25, 0.1, 0.05])
    if only is not None:
        kind[:] = only
    pairs = rng.integers(0, nh - 2, size=(n, 2)).astype(np.int32)
    toi = None
    if n >= 3000 and only is None:
        toi = rng.uniform(1e-6, 1.0, size=n)
        where = rng.permutation(n)
        tied, hub_a, hub_b, still = where[:60], where[60:1060], where[1060:2060], where[2060:2100]
        kind[tied], toi[tied] = er.IMPACT, 0.375
        kind[hub_a] = rng.choice([er.IMPACT, er.UNDECIDED], size=1000)
        kind[hub_b] = rng.choice([er.IMPACT, er.UNDECIDED], size=1000)
        pairs[hub_a, 0], pairs[hub_b, 1] = hub, hub
        kind[still] = rng.choice([er.HIT, er.START], size=40)
        pairs[still, 0] = quiet
        toi = np.where((kind == er.IMPACT) | (kind == er.UNDECIDED), toi, np.where(kind == er.NONE, 1.0, 0.0))
    cast = er.synth_cast(rng, kind, toi)
    return pairs, cast, er.synth_contacts(rng, n), nh, hub, quiet


def check(got, want, what=""):
    ev, n, counts, bt, be = got
    w_ev, w_n, w_counts, w_bt, w_be = want
    assert n == w_n and counts.tolist() == w_counts.tolist(), (what, n, w_n, counts, w_counts)
    assert n == counts[:4].sum()
    assert ev.tobytes() == w_ev[:len(ev)].tobytes(), what
    if bt is not None:
        assert be.tobytes() == w_be.tobytes() and bt.tobytes() == w_bt.tobytes(), what


@pytest.mark.parametrize("n", SIZES)
def test_synthetic_records_equal_the_restatement(n):
    pairs, cast, rec, nh, hub, quiet = synthetic(n)
    want = er.reference(pairs, cast, nh, rec)
    got = run(pairs, cast, nh, rec)
    print(f"n = {n}: {want[1]} events, counts {want[2].tolist()}")
    check(got, want, n)
    assert len(got[0]) == want[1]
    if n >= 3000:
        ev, _, counts, bt, be = got
        zero = ev["time"] == 0.0
        assert ((ev["kind"] == er.HIT) & zero).sum() >= 100 and ((ev["kind"] == er.START) & zero).sum() >= 100
        tied = ev[(ev["time"] == 0.375) & (ev["kind"] == er.IMPACT)]
        assert len(tied) >= 50 and (np.diff(tied["pair"]) > 0).all()              # ties go by pair index
        assert ((ev["a"] == hub).sum(), (ev["b"] == hub).sum()) == (1000, 1000)
        first = np.nonzero((ev["a"] == hub) | (ev["b"] == hub))[0][0]
        assert be[hub] == first and bt[hub] == ev["time"][first]
        named = (ev["a"] == quiet) | (ev["b"] == quiet)
        assert named.sum() == 40 and np.isin(ev["kind"][named], (er.HIT, er.START)).all()
        assert bt[quiet] == 1.0 and be[quiet] == -1
        assert (np.diff(pairs[:, 0].astype(np.int64)) < 0).any()                   # the list is unsorted
        assert (np.diff(ev["time"]) >= 0).all() and len(np.unique(ev["pair"])) == len(ev)
    if n == 0:
        assert got[1] == 0 and (got[3] == 1.0).all() and (got[4] == -1).all() and len(got[3]) == nh


def test_only_misses_and_only_events():
    n = T + 1
    pairs, cast, rec, nh, _, _ = synthetic(n, only=er.NONE)
    got = run(pairs, cast, nh, rec)
    check(got, er.reference(pairs, cast, nh, rec), "misses")
    assert got[1] == 0 and (got[2] == 0).all() and (got[3] == 1.0).all() and (got[4] == -1).all()
    for only in (er.IMPACT, er.HIT):
        pairs, cast, rec, nh, _, _ = synthetic(n, only=only)
        got = run(pairs, cast, nh, rec)
        check(got, er.reference(pairs, cast, nh, rec), only)
        assert got[1] == n == len(got[0])
    pairs, cast = er.edge_records(np.random.default_rng(5))                         # every clash and special toi
    check(run(pairs, cast, 2 * len(cast)), er.reference(pairs, cast, 2 * len(cast)), "edge")


def test_cut_list_keeps_counts_and_body_outputs():
    n = 3 * T + 17
    pairs, cast, rec, nh, _, _ = synthetic(n)
    full = run(pairs, cast, nh, rec)
    assert full[1] > 1000
    for cap in (0, 1, full[1] - 1):
        got = run(pairs, cast, nh, rec, max_events=cap)                             # run() holds the canary
        assert got[1] == full[1] and got[2].tolist() == full[2].tolist()
        assert len(got[0]) == cap and got[0].tobytes() == full[0][:cap].tobytes()
        assert got[3].tobytes() == full[3].tobytes() and got[4].tobytes() == full[4].tobytes()
    got = run(pairs, cast, nh, rec, bodies=False)                                   # the list without the body pass
    assert got[0].tobytes() == full[0].tobytes() and got[1] == full[1]


@pytest.mark.parametrize("records", ["none", "f64", "f32"])
def test_contact_records_give_the_hit_geometry(records):
    n = T + 65
    pairs, cast, rec64, nh, _, _ = synthetic(n)
    rec = {"none": None, "f64": rec64, "f32": er.synth_contacts(np.random.default_rng(9), n, gjkepa.PREC_F32)}[records]
    got = gjkepa.events(pairs, cast, nh, records=rec)                               # the binding's own staging
    check(got, er.reference(pairs, cast, nh, rec), records)
    ev = got[0]
    hit = ev["kind"] == er.HIT
    assert hit.sum() >= 100
    if rec is None:
        assert (ev["point_a"][hit] == 0).all() and (ev["normal"][hit] == 0).all() and (ev["depth"][hit] == 0).all()
    else:
        src = rec[ev["pair"][hit]]
        assert np.array_equal(ev["point_a"][hit], src["nearest_points"][:, 0:3].astype(np.float64))
        assert np.array_equal(ev["point_b"][hit], src["nearest_points"][:, 3:6].astype(np.float64))
        assert np.array_equal(ev["normal"][hit], src["collision_normal"].astype(np.float64))
        assert np.array_equal(ev["depth"][hit], src["penetration_depth"].astype(np.float64))
        assert np.array_equal(ev["status"][hit], src["status"])
    other = ~hit
    assert ev["point_a"][other].tobytes() == cast["point_a"][ev["pair"][other]].tobytes() and (ev["depth"][other] == 0).all()


class Chain:
    """swept broad phase -> batch -> rigid cast -> events -> pose on device buffers.  The pool ends in two resting
    hulls far from everything and from each other: the pair list is filled with that pair before the broad phase
    writes its n_found pairs, so the later entries run over all `cap` pairs whatever n_found is, and the padding
    pairs are misses that give no event."""

    def __init__(self, pool, bm, tol, cap):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        far = np.array([[1e3, 0, 0], [1e3, 1, 0], [1e3, 0, 1], [1e3 + 1, 0, 0]])
        pad = gjkepa.HullPool.from_pairs([(far, far + [0, 1e3, 0])], dtype=pool.verts.dtype)
        self.nh = len(pool.hull_cnt) + 2
        verts = np.concatenate([pool.verts, pad.verts])
        off = np.concatenate([pool.hull_off, pad.hull_off + pool.verts.size])
        cnt = np.concatenate([pool.hull_cnt, pad.hull_cnt])
        self.pool = gjkepa.HullPool(verts, off, cnt, np.zeros((0, 2), np.int32))
        self.tol, self.cap, self.dtype = tol, cap, self.pool.dtype_code
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.verts, self.off, self.cnt = t(verts), t(off), t(cnt)
        self.mot = t(self.motion(bm).reshape(-1))
        self.pad = t(np.array([[self.nh - 2, self.nh - 1]], np.int32))
        z = lambda count, dt: torch.zeros(count, dtype=dt, device=self.dev)
        self.ws_sweep = z(gjkepa.broadphase_swept_workspace_bytes(self.nh, cap), torch.uint8)
        self.ws_batch = z(gjkepa.workspace_bytes(cap), torch.uint8)
        self.ws_cast = z(gjkepa.cast_rigid_workspace_bytes(cap), torch.uint8)
        self.ws_ev = z(gjkepa.events_workspace_bytes(cap, self.nh), torch.uint8)

    def motion(self, bm):
        m = np.zeros((self.nh, 9))
        m[:len(bm)] = bm
        m[len(bm):, 6:9] = [[1e3, 0, 0], [1e3, 1e3, 0]]
        return m

    def buffers(self):
        torch = self.torch
        z = lambda count, dt: torch.zeros(count, dtype=dt, device=self.dev)
        return dict(pairs=z((self.cap, 2), torch.int32), count=z(1, torch.int64), contact=z(self.cap * 128, torch.uint8),
                    cast=z(self.cap * 128, torch.uint8), events=z(self.cap * 128, torch.uint8), n=z(6, torch.int64),
                    time=z(self.nh, torch.float64), rank=z(self.nh, torch.int32), posed=z(self.verts.numel(), self.verts.dtype))

    def enqueue(self, b, stream):
        p = lambda x: x.data_ptr()
        b["pairs"].copy_(self.pad.expand(self.cap, 2))
        gjkepa.broadphase_swept_device(self.dtype, p(self.verts), p(self.off), p(self.cnt), self.nh, p(self.mot), self.tol,
                                       er.PIPELINE_LONG, p(b["pairs"]), self.cap, p(b["count"]), p(self.ws_sweep),
                                       self.ws_sweep.numel(), stream)
        gjkepa.gjkepa_batch_device(2, 1.0, self.dtype, gjkepa.PREC_F64, p(self.verts), p(self.off), p(self.cnt), p(b["pairs"]),
                                   self.cap, p(b["contact"]), p(self.ws_batch), self.ws_batch.numel(), stream)
        gjkepa.cast_rigid_batch_device(self.dtype, p(self.verts), p(self.off), p(self.cnt), p(b["pairs"]), self.cap, p(self.mot),
                                       self.tol, p(b["contact"]), gjkepa.PREC_F64, p(b["cast"]), p(self.ws_cast),
                                       self.ws_cast.numel(), stream)
        gjkepa.events_device(p(b["pairs"]), self.cap, self.nh, p(b["cast"]), p(b["contact"]), gjkepa.PREC_F64, p(b["events"]),
                             self.cap, p(b["n"]), p(b["n"]) + 8, p(b["time"]), p(b["rank"]), p(self.ws_ev), self.ws_ev.numel(),
                             stream)
        b["posed"].copy_(self.verts)
        gjkepa.pose_pool_device(self.dtype, p(self.verts), p(self.off), p(self.cnt), self.nh, p(self.mot), p(b["time"]),
                                self.dtype, p(b["posed"]), 0, stream)

    def eager(self, bm):
        torch = self.torch
        work = torch.cuda.Stream(self.dev)
        b = self.buffers()
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(work):
            self.mot.copy_(torch.from_numpy(self.motion(bm).reshape(-1)))
            self.enqueue(b, work.cuda_stream)
        torch.cuda.synchronize(self.dev)
        return b


def test_repeat_and_graph_replay():
    import torch
    tol = er.PIPELINE_TAU
    pool, bm, _ = er.pipeline_scene(31, 600, 10.0)
    bm2 = bm.copy()
    bm2[:, 0:3] = -1.5 * bm[:, 0:3]
    chain = Chain(pool, bm, tol, 32768)
    dev = chain.dev
    first, again = chain.eager(bm), chain.eager(bm)                                 # two calls on one workspace
    n_found, n_events = int(first["count"].item()), int(first["n"][0].item())
    print(f"{n_found} pairs of {chain.cap}, {n_events} events, counts {first['n'][1:].tolist()}")
    assert 1000 < n_found <= chain.cap and n_events > 100 and int(first["n"][3].item()) > 50
    for k in first:
        assert torch.equal(first[k], again[k]), k
    # the events are the restatement's on the chain's own records, the padding pairs giving none
    pairs, cast = first["pairs"].cpu().numpy(), first["cast"].cpu().numpy().view(gjkepa.CAST64)
    contact = first["contact"].cpu().numpy().view(gjkepa.REC64)
    want = er.reference(pairs, cast, chain.nh, contact)
    assert want[1] == n_events and first["events"].cpu().numpy()[:n_events * 128].tobytes() == want[0].tobytes()
    assert (want[0]["pair"] < n_found).all()
    assert first["time"].cpu().numpy().tobytes() == want[3].tobytes()
    second = chain.eager(bm2)
    assert not torch.equal(first["events"], second["events"])
    g, side, work = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    bg = chain.buffers()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(g, stream=side):
        chain.enqueue(bg, side.cuda_stream)
    torch.cuda.synchronize(dev)
    for motion, want_b in ((bm, first), (bm2, second), (bm, first)):
        with torch.cuda.stream(work):
            chain.mot.copy_(torch.from_numpy(chain.motion(motion).reshape(-1)))     # body_motion rewritten in place
            g.replay()
        torch.cuda.synchronize(dev)
        m = int(want_b["n"][0].item()) * 128                                        # the list's tail keeps the replay before
        for k in bg:
            assert torch.equal(bg[k][:m], want_b[k][:m]) if k == "events" else torch.equal(bg[k], want_b[k]), k
    del g


@functools.lru_cache(maxsize=None)
def pipeline():
    """the pipeline scene through the library's own entries, one after the other"""
    tol = er.PIPELINE_TAU
    pool, bm, rest = er.pipeline_scene()
    swept, n = gjkepa.broadphase_swept(pool, bm, tol, long_radius=er.PIPELINE_LONG)
    cand = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, swept)
    contact = gjkepa.gjkepa_batch(cand, 2, 1.0)
    cast = gjkepa.cast_rigid_batch(cand, bm, tol, records=contact)
    got = gjkepa.events(swept, cast, len(pool.hull_cnt), records=contact)
    posed = gjkepa.pose_pool(pool, bm, time=got[3])
    posed64 = gjkepa.pose_pool(pool, bm, time=got[3], out_dtype=np.float64)         # the cast's arithmetic exactly
    return dict(pool=pool, bm=bm, rest=rest, tol=tol, swept=swept, n=n, contact=contact, cast=cast, got=got, posed=posed,
                posed64=posed64)


def test_pipeline_scene_events_and_the_clamps_guarantee():
    s = pipeline()
    pool, rest, tol, swept, contact, cast = s["pool"], s["rest"], s["tol"], s["swept"], s["contact"], s["cast"]
    ev, n_events, counts, body_time, body_event = s["got"]
    print(f"{s['n']} swept pairs, {n_events} events, counts {counts.tolist()}")
    assert s["n"] == len(swept) == PIPELINE_PAIRS
    check(s["got"], er.reference(swept, cast, len(pool.hull_cnt), contact), "pipeline")
    resting_partner = rest[ev["a"]] | rest[ev["b"]]
    n_rest = int(((ev["kind"] == er.IMPACT) & resting_partner).sum())
    print(f"{n_rest} IMPACT events with a resting partner")
    assert counts[0] >= 5 and counts[1] >= 5 and n_rest >= 20
    assert counts.tolist() == PIPELINE_COUNTS and n_rest == PIPELINE_RESTING_IMPACTS
    assert np.array_equal(ev["kind"] == er.HIT, contact["collision"][ev["pair"]] != 0)
    assert (body_time <= 1.0).all() and (body_time >= 0.0).all() and (body_time < 1.0).sum() > 500
    # every listed pair with a member at rest whose event is not HIT or START: posed at body_time the mover is at or
    # before the pair's time of impact and its partner has not moved, so the cast's certificate holds
    kind = er.kinds(cast)
    sel = (rest[swept[:, 0]] | rest[swept[:, 1]]) & np.isin(kind, (er.IMPACT, er.UNDECIDED))
    assert sel.sum() >= n_rest >= 20 and (kind[sel] == er.IMPACT).sum() == n_rest
    mover_time = np.where(rest[swept[:, 0]], body_time[swept[:, 1]], body_time[swept[:, 0]])
    assert (mover_time[sel] <= cast["toi"][sel]).all()
    assert (body_time[rest] == 1.0).sum() < rest.sum()                              # resting bodies are clamped too: posing leaves them
    posed = s["posed64"]
    dist = gjkepa.distance_batch(gjkepa.HullPool(posed.verts, posed.hull_off, posed.hull_cnt, swept[sel]))
    print(f"distance status values {np.unique(dist['status']).tolist()}")
    assert ((dist["flags"] & gjkepa.DIST_OVERLAP) == 0).all()
    low = float(dist["distance"].min())
    print(f"{sel.sum()} pairs with a resting member: smallest distance / tau at body_time {low / tol:.6f}")
    assert low >= 0.5 * tol - dr.tol(tol)


def test_collide_moving_equals_the_composition(lib):
    s = pipeline()
    pool, bm, tol = s["pool"], s["bm"], s["tol"]
    ev, n_events, counts, body_time, _ = s["got"]
    res = gjkepa.collide_moving(pool, bm, tol, long_radius=er.PIPELINE_LONG, pose=True)
    assert res["n_events"] == n_events and res["n_candidates"] == s["n"] and res["counts"].tolist() == counts.tolist()
    assert res["events"].tobytes() == ev.tobytes()
    assert res["body_time"].tobytes() == body_time.tobytes()
    assert res["posed"].verts.tobytes() == s["posed"].verts.tobytes()
    cut = gjkepa.collide_moving(pool, bm, tol, long_radius=er.PIPELINE_LONG, max_events=100)    # a cut event list
    assert cut["n_events"] == n_events and cut["events"].tobytes() == ev[:100].tobytes() and cut["posed"] is None
    assert cut["body_time"].tobytes() == body_time.tobytes()
    # a first candidate list that is cut: 8 per hull is too few for 300 hulls in a box of 5
    dense, dbm, _ = er.pipeline_scene(41, 300, 5.0)
    swept, n = gjkepa.broadphase_swept(dense, dbm, tol)
    assert n > 8 * 300 and n > 1024
    cand = gjkepa.HullPool(dense.verts, dense.hull_off, dense.hull_cnt, swept)
    contact = gjkepa.gjkepa_batch(cand, 2, 1.0)
    cast = gjkepa.cast_rigid_batch(cand, dbm, tol, records=contact)
    want = gjkepa.events(swept, cast, 300, records=contact)
    res = gjkepa.collide_moving(dense, dbm, tol, pose=True)
    assert res["n_candidates"] == n and res["n_events"] == want[1] and res["counts"].tolist() == want[2].tolist()
    assert res["events"].tobytes() == want[0].tobytes() and res["body_time"].tobytes() == want[3].tobytes()
    assert res["posed"].verts.tobytes() == gjkepa.pose_pool(dense, dbm, time=want[3]).verts.tobytes()
