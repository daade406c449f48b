"""The refill EPA tiers' queue hands a group its pair's metadata from LDS (gjkepa_kernel.hip, PairQueue /
MetaTab; DESIGN.md §4.2 "Pair metadata once per chunk").

When the queue's table has run out, the lanes of the wave load the hull counts and vertex offsets of the
next routed pairs of the 64-pair chunk at once and store them behind the groups' images; a refilled group
reads its entry and issues only the vertex and slot-word loads.  The table holds what the wave's last LDS
block leaves beside the queue's own state (23 pairs for EPA tier 0 with fp32 storage and fp64 compute, one
with fp64 storage and fp64 compute), so a chunk takes one to many fills, and the entries are overwritten while groups still run earlier pairs.  Per pair
the calls are unchanged, so every record must be what it was: each case runs the device entry into an
output buffer of 0xFF bytes and compares byte for byte with the oracle's records (for the pair lists over
tests/golden/c2_32v.npz the fixture's own, picked by pair: a record depends only on its pair's hulls).

How a launch cuts a list into units (Units): the first half or more goes out as 64-pair units, the rest
as 8-pair units, further units from the launch's counter once there are more units than workgroups.
- chunk occupancy: 64-pair units with 0, 1, 2, 3, 4, 5, 63 and 64 pairs routed to EPA tier 0 (hits) among
  misses: an empty table, fewer pairs than groups, exactly the four groups, one more, more than one fill;
- partial last chunks: 65, 127 and 4,097 pairs (the hull tables end with the last pair's hulls, so a lane
  past n_pairs would read a pair index outside the list);
- table reuse: 400,000 pairs (a wave claims several units, the table is refilled while groups run pairs of
  the fill before), and one such batch whose hits all lie in the 64-pair units claimed last;
- hull shapes: consecutive routed pairs whose hulls differ in size (4 to 32 vertices) and lie far apart in
  the vertex pool, and pairs of one chunk that share a hull;
- tier 1: the fixture's pairs whose polytope outgrows tier 0; tier 2: tests/golden/c5_deep.npz with a park
  slot for every pair and with the minimum workspace;
- both compute precisions, fp64 vertex storage, gjkepa_batch_warm_device, a batch under 65,536 pairs (one
  stream) and one above (the forked chain);
- tallies: the route tallies of every EPA tier, contact pass and the fp64 redo, and the two seed tallies
  (GJKEPA_TALLY_SEED_HANDED / _OWN), word for word the counts the library gave for the same batch before
  the table existed (tests/golden/epa_refill_meta_tallies.json, written by tools/refill_meta_tallies.py
  from that build), next to what the oracle's records say directly: every hit is routed to the EPA tier
  of its larger hull once, and every fresh EPA entry is seeded once.
A pair whose hulls do not fit the tier that receives it (ST_DEFER from `fits`) cannot be made through the
entries: gjk_finish and the tiers' own finish route a pair with epa_tier_for, which returns only a tier
whose hull capacity holds the pair's larger hull, and the C interface launches no tier by itself.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

import gjkepa

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPA0, EPA_TIERS = 0x10, 6                          # GJKEPA_ROUTE_EPA0, GJKEPA_EPA_TIERS
HANDED, OWN = 0x2F, 0x2D                           # GJKEPA_TALLY_SEED_HANDED / GJKEPA_TALLY_SEED_OWN
PARK_BYTES = 2880                                  # GJKEPA_PARK_BYTES
KS = (0, 1, 2, 3, 4, 5, 63, 64)                    # pairs routed to EPA tier 0 per 64-pair chunk
SEED = 0x5EED3E7A
BIG = 400_000
# tally words held to the recorded counts: EPA tiers, contact passes, redo, the two seed tallies (not the GJK
# queue's count, which depends on how a launch's waves share the units)
TALLY_WORDS = list(range(0x10, 0x16)) + list(range(0x20, 0x2C)) + [0x2D, 0x2E, 0x2F]
TALLY_GOLDEN = os.path.join(HERE, "golden", "epa_refill_meta_tallies.json")


def expect_tallies(key, tally, park):
    """The selected tally words and the park word of case `key` equal the recorded ones."""
    with open(TALLY_GOLDEN) as f:
        want = json.load(f)[key]
    got = {"tally": [int(tally[i]) for i in TALLY_WORDS], "park": int(park)}
    assert got == want, (key, dict(zip([hex(i) for i in TALLY_WORDS], zip(got["tally"], want["tally"]))), got["park"], want["park"])


def ws_min(n):
    return (512 + n + 255) // 256 * 256            # header + route bytes: no park slots


@functools.lru_cache(maxsize=None)
def base():
    """The C2 fixture's pool, its oracle records (version 2), and the pair indices of its misses, of its hits
    that stop at EPA iteration 1, of its other hits that stay in tier 0, and of the hits tier 0 passes on
    to tier 1 for certain (more than 37 iterations: over 40 polytope vertices; or over 64 faces at the end)."""
    z = np.load(os.path.join(HERE, "golden", "c2_32v.npz"))
    pool = gjkepa.HullPool(z["verts"], z["hull_off"], z["hull_cnt"], z["pairs"])
    rec = np.ascontiguousarray(z["rec_v2"]).reshape(-1).view(gjkepa.REC64)
    assert (rec["status"] == 0).all()
    hit = rec["collision"] != 0
    it, nf = (rec["diag"] >> 8) & 0xFF, rec["diag"] >> 16
    grown = hit & ((it > 37) | (nf > 64))
    return (pool, rec, np.nonzero(~hit)[0], np.nonzero(hit & (it == 1))[0], np.nonzero(hit & (it > 1) & ~grown)[0],
            np.nonzero(grown)[0])


def hits_in_turn():
    """Tier 0's hits, one-iteration and longer ones alternating while both last."""
    _, _, _, one, multi, _ = base()
    out = []
    for i in range(max(len(one), len(multi))):
        out += [one[i]] if i < len(one) else []
        out += [multi[i]] if i < len(multi) else []
    return np.asarray(out)


def chunk(k, size, a, b, ia, ib):
    """`size` pair indices: k of class `a` spread evenly among class `b`, both taken in turn from ia / ib on."""
    at = set(np.linspace(0, size - 1, k).round().astype(int).tolist()) if k else set()
    assert len(at) == k
    out = []
    for j in range(size):
        if j in at:
            out.append(a[ia % len(a)])
            ia += 1
        else:
            out.append(b[ib % len(b)])
            ib += 1
    return out, ia, ib


def chunks(ks, tail=None):
    """64-pair chunks with ks[i] hits among misses; tail = (size, k): a last partial chunk."""
    miss, hits = base()[2], hits_in_turn()
    idx, ih, im = [], 0, 0
    for k, size in [(k, 64) for k in ks] + ([(tail[1], tail[0])] if tail else []):
        c, ih, im = chunk(k, size, hits, miss, ih, im)
        idx += c
    return np.asarray(idx)


def batch(idx, dtype=np.float32):
    pool, rec = base()[:2]
    return gjkepa.HullPool(pool.verts.astype(dtype), pool.hull_off, pool.hull_cnt, pool.pairs[idx].copy()), rec[idx]


def run(pool, precision=gjkepa.PREC_F64, warm=False, ws_bytes=None, storage=None):
    """One device-entry call of `pool` into an output buffer of 0xFF bytes: the records, the route tallies and
    the park word.  The hull tables on the device end with the last hull, the pair list with the last pair."""
    import torch
    dev = torch.device("cuda", 0)
    n = pool.n_pairs
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
         (pool.verts, pool.hull_off.astype(np.int64), pool.hull_cnt.astype(np.int32), pool.pairs.astype(np.int32).reshape(-1))]
    dt = gjkepa.record_dtype(precision)
    wsb = gjkepa.workspace_bytes(n) if ws_bytes is None else ws_bytes
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    out = torch.full((n * dt.itemsize,), 0xFF, dtype=torch.uint8, device=dev)
    args = (2, 1.0, pool.dtype_code, precision, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n,
            out.data_ptr(), ws.data_ptr(), wsb)
    if warm:
        w = torch.full((4 * n,), -1, dtype=torch.int32, device=dev)          # a first call: every code 0xFFFFFFFF
        gjkepa.gjkepa_batch_warm_device(*args, w.data_ptr())
    else:
        gjkepa.gjkepa_batch_device(*args, 0)
    torch.cuda.synchronize()
    h = ws[:512].cpu().numpy().view(np.uint32)
    return out.cpu().numpy().view(dt), h[gjkepa.WS_COUNTERS:gjkepa.WS_COUNTERS + gjkepa.WS_TALLY], int(h[gjkepa.WS_PARK_WORD])


def assert_records(g, want, what):
    same = (g.view(np.uint8).reshape(len(g), -1) == want.view(np.uint8).reshape(len(want), -1)).all(axis=1)
    assert same.all(), (what, f"{int((~same).sum())} of {len(g)} records differ", np.nonzero(~same)[0][:10].tolist())


def assert_tallies(tally, park_word, want, nmax, slots, what):
    """From the oracle's records: every hit is routed to the EPA tier of its larger hull once (a tier passes a
    polytope that outgrows it on: the later tiers count those too), and every fresh EPA entry (not resumed
    from a park slot) is seeded once, from handed normals or by its own arithmetic."""
    hit = want["collision"] != 0
    epa = tally[EPA0:EPA0 + EPA_TIERS].astype(np.int64)
    assert int(epa[0]) == int((hit & (nmax <= 32)).sum()), (what, epa.tolist())
    assert int(epa.sum()) >= int(hit.sum()), (what, epa.tolist())
    resumed = min(park_word, slots)
    assert int(tally[HANDED]) + int(tally[OWN]) == int(epa.sum()) - resumed, (what, int(tally[HANDED]), int(tally[OWN]), epa.tolist())
    assert int(tally[HANDED]) > 0, what


def nmax_of(pool):
    return pool.hull_cnt[pool.pairs].max(axis=1)


def check(pool, want, what, **kw):
    g, tally, park = run(pool, **kw)
    assert_records(g, want, what)
    expect_tallies(what + "".join(f", {k} {np.dtype(v).name if k == 'storage' else v}" for k, v in sorted(kw.items())), tally, park)
    kw.pop("storage", None)
    slots = max(0, ((kw.get("ws_bytes") or gjkepa.workspace_bytes(pool.n_pairs)) - ws_min(pool.n_pairs)) // PARK_BYTES)
    assert_tallies(tally, park, want, nmax_of(pool), slots, what)
    return tally


# ---------------------------------------------------------------- chunk occupancy, partial chunks

@pytest.mark.parametrize("storage", [np.float32, np.float64], ids=["f32", "f64"])
def test_chunk_occupancy(storage):
    """1,024 pairs: the eight chunks of KS as the batch's 64-pair units, then the same list as 8-pair units."""
    idx = chunks(KS + KS)
    rec = base()[1]
    assert [int((rec["collision"][idx[64 * c:64 * c + 64]] != 0).sum()) for c in range(8)] == list(KS)
    pool, want = batch(idx, storage)
    check(pool, want, "chunk occupancy", storage=storage)


@pytest.mark.parametrize("n,tail_hits", [(65, 1), (127, 40), (4097, 1)])
def test_partial_last_chunk(n, tail_hits):
    """The list ends inside a chunk; its last pair is a hit, so the last routed lane is the last pair."""
    full = (n - 1) // 64
    idx = chunks((KS * (full // 8 + 1))[:full], tail=(n - 64 * full, tail_hits))
    assert len(idx) == n and base()[1]["collision"][idx[-1]] != 0
    pool, want = batch(idx)
    check(pool, want, f"{n} pairs")


# ---------------------------------------------------------------- table reuse

def test_waves_claim_several_units():
    """400,000 pairs: chunks of 3, 64, 0, 17, 5, 40, 1 and 63 hits in turn, taken from the counter by waves whose
    groups still run pairs of the chunk (and of the table fill) before."""
    pool, want = batch(np.resize(chunks((3, 64, 0, 17, 5, 40, 1, 63)), BIG))
    check(pool, want, "several units per wave")


def test_hits_only_in_the_units_claimed_last():
    """400,000 pairs, misses but for the last 512 of the 64-pair units (just before the list's 8-pair tail), which
    hold hits only: the waves that claim them have scanned other units, with empty tables, before."""
    n_tail = min(BIG // 2, 2048 * 64)                       # Units: at most 64 pairs per workgroup, 2,048 workgroups at most
    nbig = (BIG - n_tail) // 64
    idx = np.resize(base()[2], BIG)
    late = np.arange(64 * (nbig - 512), 64 * nbig)
    idx[late] = np.resize(hits_in_turn(), len(late))
    pool, want = batch(idx)
    check(pool, want, "late hits")


# ---------------------------------------------------------------- hull shapes

@functools.lru_cache(maxsize=None)
def shapes_pool():
    """Hulls of 4 to 32 vertices.  The pair list takes the generated pairs in a shuffled order (consecutive
    routed pairs: hulls of different sizes, far apart in the pool), then pairs that chain through shared
    hulls (pair j: hull A of pair j, hull B of pair j + 1; and every fourth pair once more)."""
    p = gjkepa.synth_pairs(SEED, 1024, 4, 32, 2.5)
    rng = np.random.default_rng(7)
    shuffled = p.pairs[rng.permutation(p.n_pairs)]
    a, b = p.pairs[:256, 0], p.pairs[1:257, 1]
    chained = np.stack([a, b], axis=1)
    again = shuffled[:256:4]
    pairs = np.ascontiguousarray(np.concatenate([shuffled, chained, again, chained[::-1]]).astype(np.int32))
    return gjkepa.HullPool(p.verts, p.hull_off, p.hull_cnt, pairs)


@pytest.fixture(scope="module")
def shapes(orc):
    pool = shapes_pool()
    return pool, orc.gjkepa_batch(pool, 2, 1.0)


@pytest.mark.parametrize("storage", [np.float32, np.float64], ids=["f32", "f64"])
def test_hull_shapes(shapes, storage):
    pool, want = shapes
    cnt = pool.hull_cnt[pool.pairs]
    hit = want["collision"] != 0
    assert cnt.min() == 4 and cnt.max() == 32 and int(hit[:1024].sum()) > 300 and int(hit[1024:].sum()) > 100
    routed = np.nonzero(hit[:1024])[0]
    assert (np.abs(np.diff(pool.hull_off[pool.pairs[routed, 0]])) > 3 * 64).mean() > 0.9      # far apart in the pool
    assert len(np.unique(cnt[routed])) > 20
    check(pool.as_dtype(storage), want, "hull shapes", storage=storage)


# ---------------------------------------------------------------- tiers 1 and 2

def test_tier1_takes_what_outgrows_tier0():
    """The fixture's pairs that tier 0 passes on, several to a chunk and between tier-0 hits."""
    grown = base()[5]
    assert len(grown) >= 3
    idx = chunks(KS)
    idx[np.linspace(200, 500, 3 * len(grown)).astype(int)] = np.tile(grown, 3)
    idx = np.concatenate([idx, np.resize(grown, 64), chunks((5, 64))])
    pool, want = batch(idx)
    tally = check(pool, want, "tier 1")
    print(f"tier 1: {int(tally[EPA0 + 1])} pairs, {int(np.isin(idx, grown).sum())} of them by the records' final sizes")
    assert int(tally[EPA0 + 1]) >= int(np.isin(idx, grown).sum()), tally[EPA0:EPA0 + EPA_TIERS].tolist()


def c5_case(orc):
    z = np.load(os.path.join(HERE, "golden", "c5_deep.npz"))
    pool = gjkepa.HullPool(z["verts"], z["hull_off"], z["hull_cnt"], z["pairs"])
    assert pool.n_pairs == 256 and pool.hull_cnt.min() >= 32 and pool.hull_cnt.max() <= 128
    return pool, orc.gjkepa_batch(pool, 2, 1.0)


@pytest.fixture(scope="module")
def c5(orc):
    return c5_case(orc)


@pytest.mark.parametrize("slots", ["every_pair", "none"])
def test_tier2(c5, slots):
    """33-128-vertex hulls: EPA tier 2 (parks with slots; with none a polytope that outgrows it restarts)."""
    pool, want = c5
    n = pool.n_pairs
    wsb = ws_min(n) + (n * PARK_BYTES if slots == "every_pair" else 0)
    g, tally, park = run(pool, ws_bytes=wsb)
    assert_records(g, want, f"tier 2, park slots {slots}")
    expect_tallies(f"tier 2, park slots {slots}", tally, park)
    assert int(tally[EPA0 + 2]) == int((nmax_of(pool) > 32).sum()) and int(tally[EPA0]) == int((nmax_of(pool) <= 32).sum())
    assert (park > 0) == (slots == "every_pair")
    assert int(tally[HANDED]) + int(tally[OWN]) == int(tally[EPA0:EPA0 + EPA_TIERS].sum()) - (park if slots == "every_pair" else 0)


# ---------------------------------------------------------------- precisions, entries, schedules

def test_fp32_compute_equals_cpu_model():
    """fp32 compute on the occupancy chunks and a partial one: the records of the fp32 path's CPU model (the
    fp32 oracle, its uncertified or failed pairs recomputed in fp64)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle
    from fp32_check import model_fp32
    pool, _ = batch(chunks(KS, tail=(37, 5)))
    model, _ = model_fp32(pool, oracle.gjkepa_batch(pool, 2, 1.0, 16), 16)
    g, tally, park = run(pool, precision=gjkepa.PREC_F32)
    assert_records(g, model, "fp32 compute")
    expect_tallies("fp32 compute", tally, park)


def test_warm_entry_cold_call():
    """gjkepa_batch_warm_device with fresh warm slots: the plain call's bytes."""
    pool, want = batch(np.resize(chunks(KS, tail=(37, 5)), 3000))
    check(pool, want, "warm entry, cold call", warm=True)


@pytest.mark.parametrize("n", [3000, 70000])
def test_batch_sizes(n):
    """One stream with small work units (under 65,536 pairs) and the forked chain."""
    pool, want = batch(np.resize(chunks(KS, tail=(37, 5)), n))
    check(pool, want, f"{n} pairs")
