"""Contact tier 0's pending case_04 queue (gjkepa_kernel.hip, contact_kernel; GJKEPA_CT_QUEUE04).

A pair whose contact point takes get_collisionPoint_02's case_04 leaves that branch to a per-wave
queue, and a round of its own runs it once 8 entries are pending (or the wave has no unit left).  The
batches below are laid out so that 64-pair chunks hold chosen numbers of such pairs (none, one, one
short of / exactly / one over a deferred round, the same around two rounds, and a whole chunk), on
every scheduling form of the contact pass: counter-claimed units with the small tail units (one
stream), one workgroup per chunk (the forked pass of a large batch) and the sparse 16-chunk claim.
The layouts are steered by a CPU classification of the oracle's records (the band counts of
contact_v2 along the oracle's normal); the check itself is byte equality with the oracle on the same
pool.  Every batch runs twice into an output buffer filled with 0xFF bytes, so a record word, contact
point or route byte the queue leaves unwritten shows.
"""
import functools
import os
import sys

import numpy as np
import pytest

import gjkepa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
C2 = (32, 32, 2.5)                            # bench.py's flagship config: 32-vertex hulls
COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 64)      # likely-case_04 hits per 64-pair chunk, cycled over the chunks
CT20, CT50 = 0x24, 0x2A                       # route codes GJKEPA_ROUTE_CT(2) / CT(5) + contact tier 0


def over_tier0(ref):
    """Hits EPA tier 0 cannot finish: more final polytope faces (the diag word) than its 64 face slots."""
    return (ref["collision"] != 0) & ((ref["diag"] >> 16) > 64)


def likely_case04(pool, ref):
    """Per pair: a hit whose band sets along the oracle's normal are (2, >= 3) or (>= 3, 2)."""
    c = int(pool.hull_cnt[0])
    assert (pool.hull_cnt == c).all()                     # C2: every hull has 32 vertices
    n = ref["collision_normal"]
    cnt = []
    for side in (0, 1):
        o = pool.hull_off[pool.pairs[:, side]][:, None] + np.arange(c)[None, :]
        x, y, z = (pool.verts[o + a * c].astype(np.float64) for a in range(3))
        t = x * n[:, :1] + y * n[:, 1:2] + z * n[:, 2:]
        t = -t if side else t
        cnt.append((t > t.max(axis=1, keepdims=True) - 0.1).sum(axis=1))
    return (ref["collision"] != 0) & (((cnt[0] == 2) & (cnt[1] >= 3)) | ((cnt[0] >= 3) & (cnt[1] == 2)))


@functools.lru_cache(maxsize=None)
def base():
    """The C2 pool the layouts draw from, its oracle records and the classification (computed once)."""
    import oracle
    pool = gjkepa.synth_pairs(0xC0DE04, 24000, *C2)
    ref = oracle.gjkepa_batch(pool, 2, 1.0)
    return pool, ref, likely_case04(pool, ref)


def layout(n_pairs):
    """A pair list over base()'s hulls: chunk i holds COUNTS[i % 9] likely-case_04 hits (first in the
    chunk), the rest other pairs in pool order; both kinds are reused in turn when they run out."""
    pool, _, likely = base()
    yes, no = np.nonzero(likely)[0], np.nonzero(~likely)[0]
    idx, iy, ino = [], 0, 0
    for c in range((n_pairs + 63) // 64):
        size = min(64, n_pairs - 64 * c)
        k = min(COUNTS[c % len(COUNTS)], size)
        idx += [yes[(iy + j) % len(yes)] for j in range(k)] + [no[(ino + j) % len(no)] for j in range(size - k)]
        iy, ino = iy + k, ino + size - k
    idx = np.asarray(idx)
    # the layout holds what it claims, by the same classification
    per_chunk = [int(likely[idx[64 * c:64 * c + 64]].sum()) for c in range((n_pairs + 63) // 64)]
    full = n_pairs // 64
    assert all(per_chunk[c] >= COUNTS[c % len(COUNTS)] for c in range(full)), per_chunk[:18]
    assert full >= len(COUNTS)
    return gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[idx].copy())


def run_poisoned(pool, version=2, precision=gjkepa.PREC_F64):
    """Two device-API runs of `pool`, each into an output buffer of 0xFF bytes: their records and the
    second run's route tallies."""
    import torch
    dev = torch.device("cuda", 0)
    n = pool.n_pairs
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
         (pool.verts, pool.hull_off.astype(np.int64), pool.hull_cnt.astype(np.int32), pool.pairs.astype(np.int32).reshape(-1))]
    dt = gjkepa.record_dtype(precision)
    wsb = gjkepa.workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        out = torch.full((n * dt.itemsize,), 0xFF, dtype=torch.uint8, device=dev)
        gjkepa.gjkepa_batch_device(version, 1.0, pool.dtype_code, precision, t[0].data_ptr(), t[1].data_ptr(),
                                   t[2].data_ptr(), t[3].data_ptr(), n, out.data_ptr(), ws.data_ptr(), wsb, 0)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy().view(dt))
    h = ws[:512].cpu().numpy().view(np.uint32)
    return runs, h[gjkepa.WS_COUNTERS:gjkepa.WS_COUNTERS + gjkepa.WS_TALLY]


def assert_records(runs, want, what):
    w = want.view(np.uint8).reshape(len(want), -1)
    for i, g in enumerate(runs):
        same = (g.view(np.uint8).reshape(len(g), -1) == w).all(axis=1)
        assert same.all(), (what, f"run {i}", int((~same).sum()), np.nonzero(~same)[0][:10].tolist())


def test_classification_finds_case04_pairs():
    """CPU: the classification that steers the layouts marks about 28% of C2's hits."""
    _, ref, likely = base()
    hits = int((ref["collision"] != 0).sum())
    assert 0.2 * hits < likely.sum() < 0.36 * hits, (int(likely.sum()), hits)


def test_classification_agrees_with_oracle_branch_bits(orc):
    """CPU: on the pool's first pairs the classification is the oracle's own case_04 branch bit."""
    pool, _, likely = base()
    n = 2000
    head = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[:n])
    _, cov = orc.gjkepa_batch_cov(head, 2, 1.0)
    took = ((cov >> np.uint64(orc.BR["V2_CASE04"])) | (cov >> np.uint64(orc.BR["V2_CASE04B"]))) & np.uint64(1)
    assert (took.astype(bool) == likely[:n]).mean() > 0.99


@pytest.mark.gpu
def test_one_stream_units_and_tail(orc):
    """2,048 pairs: one stream, counter-claimed 64-pair units and the small tail units."""
    pool = layout(2048)
    runs, _ = run_poisoned(pool)
    assert_records(runs, orc.gjkepa_batch(pool, 2, 1.0), "one stream")


@pytest.mark.gpu
def test_forked_pass_one_chunk_per_workgroup(orc):
    """70,000 pairs: the forked passes, whose tier-0 pass gives each workgroup one chunk, so every
    workgroup ends on a partial round; EPA tier 1's few pairs take the sparse claim."""
    pool = layout(70000)
    want = orc.gjkepa_batch(pool, 2, 1.0)
    late = int(over_tier0(want).sum())
    assert late > 0
    runs, tally = run_poisoned(pool)
    assert_records(runs, want, "forked passes")
    assert late <= int(tally[CT20]) + int(tally[CT50]) and int(tally[CT20]) * 16 < pool.n_pairs, (late, int(tally[CT20]))


@pytest.mark.gpu
def test_sparse_claim_queue_persists_across_chunks(orc):
    """Contact tier 0's pairs under 1/16 of the batch: case_04 pairs EPA tier 0 must hand to tier 1 (more
    than 64 polytope faces by the oracle's diag word), repeated and spread one or two to a chunk among
    far-apart pairs, so the sparse 16-chunk claim serves them and a wave's queue fills over many chunks."""
    pool, ref, likely = base()
    long04 = np.nonzero(likely & over_tier0(ref))[0]
    assert len(long04) >= 8, len(long04)
    n = 70000
    cube = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], float)
    far = gjkepa.HullPool.from_pairs([(cube, cube + 50.0)], dtype=np.float32)
    verts = np.concatenate([pool.verts, far.verts])
    off = np.concatenate([pool.hull_off, far.hull_off + len(pool.verts)])
    cnt = np.concatenate([pool.hull_cnt, far.hull_cnt])
    pairs = np.tile(np.asarray(far.pairs[0] + len(pool.hull_cnt), np.int32), (n, 1))
    at = np.arange(0, n, 41)[:1500]                      # one or two per 64-pair chunk
    pairs[at] = pool.pairs[long04[np.arange(len(at)) % len(long04)]]
    batch = gjkepa.HullPool(verts, off, cnt, pairs)
    runs, tally = run_poisoned(batch)
    want = orc.gjkepa_batch(batch, 2, 1.0)
    assert int((want["collision"] != 0).sum()) == len(at)
    assert_records(runs, want, "sparse claim")
    # every one of them reached contact tier 0 through a later fork point's pass (EPA tiers 1-2: CT20,
    # tiers 3-5: CT50), and those passes choose the sparse claim below 1/16 of the batch
    assert int(tally[CT20]) + int(tally[CT50]) == len(at) and len(at) * 16 < n, (int(tally[CT20]), int(tally[CT50]))


@pytest.mark.gpu
def test_mixed_sizes_beside_contact_tier1(orc):
    """Hulls of 8-256 vertices: contact tier 1 (no queue) serves the large ones beside tier 0."""
    pool = gjkepa.synth_pairs(0xC0DE05, 3000, 8, 256, 2.5)
    runs, _ = run_poisoned(pool)
    assert_records(runs, orc.gjkepa_batch(pool, 2, 1.0), "mixed sizes")


@pytest.mark.gpu
def test_branch_fixture_case04_pairs_fill_rounds(orc):
    """tests/golden/branch_cov.npz's case_04 pairs (both argument orders, sub-branches _1 / _2 / _3),
    repeated to fill several deferred rounds, between its other small-hull pairs."""
    z = np.load(os.path.join(GOLDEN, "branch_cov.npz"))
    bit = lambda name: ((z["cov"] >> np.uint64(orc.BR[name])) & np.uint64(1)).astype(bool)  # noqa: E731
    small = z["hull_cnt"][z["pairs"]].max(axis=1) <= 32
    c04 = (bit("V2_CASE04") | bit("V2_CASE04B")) & small
    for name in ("V2_CASE04", "V2_CASE04B", "V2_CASE04_1", "V2_CASE04_2", "V2_CASE04_3"):
        assert (bit(name) & c04).any(), name
    yes, no = np.nonzero(c04)[0], np.nonzero(small & ~c04)[0]
    idx = np.concatenate([np.resize(yes, 150), no, np.resize(yes, 75), no[:40], np.resize(yes, 9)])
    pool = gjkepa.HullPool(z["verts"], z["hull_off"], z["hull_cnt"], z["pairs"][idx].copy())
    runs, _ = run_poisoned(pool)
    assert_records(runs, z["rec_v2"].reshape(-1).view(gjkepa.REC64)[idx], "branch fixture")


@pytest.mark.gpu
def test_fp32_compute_equals_cpu_model():
    """fp32 compute on the 2,048-pair layout: the records of the fp32 path's CPU model (the fp32 oracle,
    its uncertified or failed pairs recomputed in fp64), so a queued pair that fails is rerouted."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle
    from fp32_check import model_fp32
    pool = layout(2048)
    model, redo = model_fp32(pool, oracle.gjkepa_batch(pool, 2, 1.0, 16), 16)
    runs, _ = run_poisoned(pool, precision=gjkepa.PREC_F32)
    assert 0 < int(redo.sum()) < pool.n_pairs
    assert_records(runs, model, "fp32 compute")


@pytest.mark.gpu
@pytest.mark.parametrize("version", [1, 3])
def test_versions_without_case04(orc, version):
    """Versions 1 and 3 have no case_04: nothing is queued and the records are the oracle's."""
    pool = layout(2048)
    runs, _ = run_poisoned(pool, version=version)
    assert_records(runs, orc.gjkepa_batch(pool, version, 1.0), f"version {version}")
