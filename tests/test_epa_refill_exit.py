"""The refill EPA tiers (EPA tiers 0-2, epa_kernel_refill) close an iteration in the pass that ran it: a
pass is refill, epa_grow, epa_close, park / finish, so a pair leaves its group in the pass of its last
iteration and the group is idle at the very next refill (DESIGN.md §4.2 "Refill").  Per pair the calls
are unchanged, so every record must be what it was: each case below runs fp64 compute through
gjkepa_batch_device into an output buffer pre-filled with 0xFF bytes, with fp32 and with fp64 vertex
storage, and compares byte for byte against the oracle.

The shapes are the smallest at which the pass order can go wrong (every batch has more than 64 pairs:
up to 64 go to the one-wave query path and never reach a refill kernel):
- the shortest lifetimes: pairs of tests/golden/branch_cov.npz that stop at the close of iteration 1
  leave in the pass they entered, four at a time (a wave whose groups all empty at once), next to the
  fixture's longest tier-0 pairs, at the end of the batch (the queue runs dry with groups idle), and a
  pair whose iteration 1 is run whole by epa_begin (a hit on the initial triangle: three simplex
  points) fresh in the same pass as a pair epa_seed set up;
- order independence on the C2 fixture: in order, reversed and sorted by iteration count both ways;
- the parking tier on the C5 fixture with park slots for every pair, none, and five;
- one batch on the forked schedule (70,000 pairs) and one on the single stream (3,000).
"""
import os

import numpy as np
import pytest

import gjkepa

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARK_BYTES = 2880                                           # GJKEPA_PARK_BYTES
HANDED, OWN = 0x2F, 0x2D                                    # GJKEPA_TALLY_SEED_HANDED / GJKEPA_TALLY_SEED_OWN
STORAGE = [np.float32, np.float64]
SEED = 0x5EED4E0D


def ws_min(n):
    return (512 + n + 255) // 256 * 256                     # header + route bytes: no park slots


def run(pool, version=2, ws_bytes=None):
    """Records of one gjkepa_batch_device call into a 0xFF-filled buffer, and the workspace header."""
    import torch
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev)
         for x in (pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs.reshape(-1))]
    n = pool.n_pairs
    wsb = gjkepa.workspace_bytes(n) if ws_bytes is None else ws_bytes
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    out = torch.full((n * 128,), 0xFF, dtype=torch.uint8, device=dev)
    gjkepa.gjkepa_batch_device(version, 1.0, pool.dtype_code, gjkepa.PREC_F64, t[0].data_ptr(), t[1].data_ptr(),
                               t[2].data_ptr(), t[3].data_ptr(), n, out.data_ptr(), ws.data_ptr(), wsb, 0)
    torch.cuda.synchronize()
    hdr = ws[:512].cpu().numpy().view(np.uint32)
    return np.frombuffer(out.cpu().numpy().tobytes(), gjkepa.REC64), hdr


def differing(g, ref):
    n = len(ref)
    bad = (g.view(np.uint8).reshape(n, -1) != ref.view(np.uint8).reshape(n, -1)).any(axis=1)
    return f"{int(bad.sum())} of {n} records differ, first {np.nonzero(bad)[0][:8].tolist()}"


def load_pool(name):
    z = np.load(os.path.join(GOLDEN, name))
    return z, gjkepa.HullPool(z["verts"], z["hull_off"], z["hull_cnt"], z["pairs"])


def subset(pool, idx, dtype):
    """The pool's pairs `idx` in that order (pairs are hull indices: the hulls stay where they are)."""
    return gjkepa.HullPool(pool.verts.astype(dtype), pool.hull_off, pool.hull_cnt,
                           np.ascontiguousarray(pool.pairs[np.asarray(idx, np.int64)]))


def epa_iters(rec):
    return ((rec["diag"] >> 8) & 0xFF).astype(np.int64)


# ---------------------------------------------------------------- shortest lifetimes

def short_layout(n):
    """n indices into branch_cov.npz's pair list.  From the fixture's own records (version 2): `one`
    stops at the close of iteration 1, `long_` are the longest pairs of hulls up to 32 vertices (EPA
    tier 0), `begin` are status-0 hits on the initial triangle (ORC_BR_INIT_TRI_HIT: a three-point
    simplex, so iteration 1 is epa_begin's), `seed` are hits with four distinct simplex points."""
    z, pool = load_pool("branch_cov.npz")
    rec = z["rec_v2"].reshape(-1).view(gjkepa.REC64)
    it = epa_iters(rec)
    hit0 = (rec["collision"] != 0) & (rec["status"] == 0)
    small = pool.hull_cnt[pool.pairs].max(axis=1) <= 32
    tri = ((z["cov"] >> np.uint64(4)) & np.uint64(1)).astype(bool)
    one = np.nonzero(hit0 & (it == 1))[0]
    two = np.nonzero(hit0 & (it == 2))[0]
    assert len(one) == 9 and len(two) == 33, (len(one), len(two))
    cand = np.nonzero(hit0 & small & ~tri)[0]
    long_ = cand[np.argsort(-it[cand], kind="stable")][:7]
    assert it[long_].min() >= 4 and it[long_].max() >= 7, it[long_]
    begin = np.nonzero(hit0 & tri)[0]
    seed = np.nonzero(hit0 & ~tri & (it == 2))[0]
    assert len(begin) >= 8 and len(seed) >= 8
    head = list(one[:4])                                    # a whole wave's groups leave in the pass they entered
    for a, b in zip(one[4:].tolist() + one[:3].tolist(), long_.tolist()):
        head += [a, b]                                      # iteration-1 pairs between the longest ones
    for a, b in zip(begin[:8].tolist(), seed[:8].tolist()):
        head += [a, b]                                      # epa_begin's and epa_seed's pairs fresh together
    tail = list(one[:6])                                    # the queue runs dry on iteration-1 pairs
    rng = np.random.default_rng(n)
    fill = []
    while len(head) + len(fill) + len(tail) < n:            # the whole fixture, permuted, as often as it takes
        fill += rng.permutation(pool.n_pairs).tolist()
    fill = fill[:n - len(head) - len(tail)]
    idx = head + fill + tail
    assert len(idx) == n
    return pool, idx


@pytest.fixture(scope="module")
def short_cases(orc):
    """(n, storage) -> (pool, {version: oracle records}), each computed once."""
    cases = {}
    for n in (65, 130, 257):
        base, idx = short_layout(n)
        for dt in STORAGE:
            pool = subset(base, idx, dt)
            cases[n, dt] = (pool, {v: orc.gjkepa_batch(pool, v, 1.0) for v in (1, 2, 3)})
    return cases


@pytest.mark.parametrize("storage", STORAGE, ids=["f32", "f64"])
@pytest.mark.parametrize("version", [1, 2, 3])
@pytest.mark.parametrize("n", [65, 130, 257])
def test_shortest_lifetimes(short_cases, n, version, storage):
    pool, refs = short_cases[n, storage]
    ref = refs[version]
    g, hdr = run(pool, version)
    print(f"n {n} v{version} {np.dtype(storage).name}: {int((ref['collision'] != 0).sum())} hits, "
          f"{int(((ref['status'] == 0) & (epa_iters(ref) == 1)).sum())} stop at iteration 1, "
          f"{int((ref['status'] != 0).sum())} with an error status")
    assert g.tobytes() == ref.tobytes(), differing(g, ref)
    tally = hdr[gjkepa.WS_COUNTERS:gjkepa.WS_COUNTERS + gjkepa.WS_TALLY]
    assert tally[OWN] > 0, (int(tally[OWN]), int(tally[HANDED]))   # pairs seeded without handed normals ran


# ---------------------------------------------------------------- order independence

@pytest.fixture(scope="module")
def c2(orc):
    z, pool = load_pool("c2_32v.npz")
    assert pool.n_pairs == 1024 and pool.verts.dtype == np.float32
    # fp64 storage holds the same values (fp32 widened exactly), so the oracle's records are the same
    ref = orc.gjkepa_batch(pool, 2, 1.0)
    it = epa_iters(ref)
    orders = {
        "in_order": np.arange(1024),
        "reversed": np.arange(1024)[::-1],
        "ascending": np.argsort(it, kind="stable"),
        "descending": np.argsort(-it, kind="stable"),
    }
    return pool, ref, orders


@pytest.mark.parametrize("storage", STORAGE, ids=["f32", "f64"])
@pytest.mark.parametrize("order", ["in_order", "reversed", "ascending", "descending"])
def test_order_independence(c2, order, storage):
    pool, ref, orders = c2
    idx = orders[order]
    g, _ = run(subset(pool, idx, storage))
    want = ref[idx]
    assert g.tobytes() == want.tobytes(), differing(g, want)


# ---------------------------------------------------------------- the parking tier

@pytest.fixture(scope="module")
def c5(orc):
    z, pool = load_pool("c5_deep.npz")
    assert pool.n_pairs == 256 and pool.verts.dtype == np.float32
    return pool, orc.gjkepa_batch(pool, 2, 1.0)             # fp64 storage: the same values, the same records


@pytest.mark.parametrize("storage", STORAGE, ids=["f32", "f64"])
@pytest.mark.parametrize("slots", ["every_pair", "none", "five"])
def test_parking_tier(c5, slots, storage):
    base, ref = c5
    n = base.n_pairs
    pool = subset(base, np.arange(n), storage)
    wsb = ws_min(n) + {"every_pair": n, "none": 0, "five": 5}[slots] * PARK_BYTES
    g, hdr = run(pool, 2, wsb)
    parked = int(hdr[gjkepa.WS_PARK_WORD])                  # park attempts
    print(f"park slots {slots}, {np.dtype(storage).name}: {parked} park attempts, "
          f"up to {int(epa_iters(ref).max())} iterations")
    assert g.tobytes() == ref.tobytes(), differing(g, ref)
    if slots == "none":
        assert parked == 0
    else:
        assert parked > 0                                   # park_now ran after a close


# ---------------------------------------------------------------- both schedules

@pytest.fixture(scope="module")
def c2_generated(orc):
    out = {}
    for n in (70000, 3000):                                 # forked schedule (from 64K pairs) / single stream
        pool = gjkepa.synth_pairs(SEED, n, 32, 32, 2.5)
        out[n] = (pool, orc.gjkepa_batch(pool, 2, 1.0))     # fp32 values; fp64 storage widens them exactly
    return out


@pytest.mark.parametrize("storage", STORAGE, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [70000, 3000])
def test_both_schedules(c2_generated, n, storage):
    base, ref = c2_generated[n]
    g, _ = run(base.as_dtype(storage))
    assert g.tobytes() == ref.tobytes(), differing(g, ref)
