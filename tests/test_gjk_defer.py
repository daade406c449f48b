"""GJK tier 0's pending loop queue (gjkepa_kernel.hip, gjk_kernel; GJKEPA_G0_DEFER_AT).

Once at most GJKEPA_G0_DEFER_AT of a wave's 16 groups are still in GJK's tetrahedron loop, they leave it
undecided for a per-wave queue, and a round of their own continues them once 16 entries are pending (or
the wave has no unit left).  The batches below are pair lists over the hulls of tests/golden/c2_32v.npz,
steered by its oracle records: *long* pairs are the misses (the reference has no separating-axis exit, so a
miss stays in the loop for at least 4 iterations), *short* pairs the hits that leave after one iteration,
*medium* pairs the hits that take three or more.  64-pair chunks hold chosen numbers of long pairs among
short ones (none, around one queued round, around two, a whole chunk).  How a launch cuts a list into units
(gjkepa_kernel.hip, Units): the first half or more goes out as 64-pair units, the rest as 16-pair units, one
unit per workgroup while there are no more units than workgroups (every batch here below 16,384 pairs; its
waves end on a partial round each), further units from the launch's counter otherwise.  So the small
batches check the stop, the push and the partial rounds at a wave's end on both unit sizes; the 70,000-pair
batch and the two of 400,000 pairs, where a wave claims several units, check full queued rounds from the
round hook, the ring living across units and its wrap.  A record depends only on its pair's two hulls, so the
expected records are the fixture's own, picked by pair; the check is byte equality, twice, into output
buffers filled with 0xFF bytes, so a word, route byte or warm slot a queued pair leaves unwritten shows.
"""
import functools
import os
import sys

import numpy as np
import pytest

import gjkepa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64)    # long pairs per 64-pair chunk
QUEUED = 0x2C                                     # gjkepa_kernel.h GJKEPA_TALLY_GJK_QUEUED


@functools.lru_cache(maxsize=None)
def base():
    """The fixture's pool, its oracle records (version 2) and the three classes' pair indices."""
    z = np.load(os.path.join(HERE, "golden", "c2_32v.npz"))
    pool = gjkepa.HullPool(z["verts"], z["hull_off"], z["hull_cnt"], z["pairs"])
    rec = np.ascontiguousarray(z["rec_v2"]).reshape(-1).view(gjkepa.REC64)
    hit, it = rec["collision"] != 0, rec["diag"] & 0xFF
    assert (rec["status"] == 0).all()
    return pool, rec, np.nonzero(~hit)[0], np.nonzero(hit & (it == 1))[0], np.nonzero(hit & (it >= 3))[0]


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
    """Pair indices of 64-pair chunks with ks[i] long pairs among short ones; tail = (size, k): a last partial chunk."""
    _, _, long_, short, _ = base()
    idx, il, is_ = [], 0, 0
    for k, size in [(k, 64) for k in ks] + ([(tail[1], tail[0])] if tail else []):
        c, il, is_ = chunk(k, size, long_, short, il, is_)
        idx += c
    return np.asarray(idx)


def tiled(idx, n):
    return np.resize(idx, n)


def batch(idx):
    pool, rec, *_ = base()
    return gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[idx].copy()), rec[idx]


def run_poisoned(pool, precision=gjkepa.PREC_F64, warm=False):
    """Two device-API runs of `pool`, each into an output buffer of 0xFF bytes (warm: the warm entry with
    fresh slots): their records, the second run's route tallies and its warm slots."""
    import torch
    dev = torch.device("cuda", 0)
    n = pool.n_pairs
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
         (pool.verts, pool.hull_off.astype(np.int64), pool.hull_cnt.astype(np.int32), pool.pairs.astype(np.int32).reshape(-1))]
    dt = gjkepa.record_dtype(precision)
    wsb = gjkepa.workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    runs, w = [], None
    for _ in range(2):
        out = torch.full((n * dt.itemsize,), 0xFF, dtype=torch.uint8, device=dev)
        args = (2, 1.0, pool.dtype_code, precision, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n,
                out.data_ptr(), ws.data_ptr(), wsb)
        if warm:
            w = torch.full((4 * n,), -1, dtype=torch.int32, device=dev)      # a first call: every code 0xFFFFFFFF
            gjkepa.gjkepa_batch_warm_device(*args, w.data_ptr())
        else:
            gjkepa.gjkepa_batch_device(*args, 0)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy().view(dt))
    h = ws[:512].cpu().numpy().view(np.uint32)
    codes = w.cpu().numpy().view(np.uint32).reshape(-1, 4) if warm else None
    return runs, h[gjkepa.WS_COUNTERS:gjkepa.WS_COUNTERS + gjkepa.WS_TALLY], codes


def assert_records(runs, want, what):
    w = want.view(np.uint8).reshape(len(want), -1)
    for i, g in enumerate(runs):
        same = (g.view(np.uint8).reshape(len(g), -1) == w).all(axis=1)
        assert same.all(), (what, f"run {i}", int((~same).sum()), np.nonzero(~same)[0][:10].tolist())
    assert runs[0].tobytes() == runs[1].tobytes(), what          # and one batch twice is the same bytes


def test_fixture_classes_fill_the_layouts():
    """CPU: the fixture's misses, one-iteration hits and hits of three or more iterations, and that each
    class fills a whole chunk with distinct pairs (larger layouts take them in turn again)."""
    _, rec, long_, short, medium = base()
    assert (len(long_), len(short), len(medium)) == (276, 360, 154)
    assert min(len(long_), len(short), len(medium)) >= 64
    idx = chunks(KS, tail=(37, 5))
    assert len(idx) == 704 + 37
    is_long = rec["collision"][idx] == 0
    assert [int(is_long[64 * c:64 * c + 64].sum()) for c in range(12)] == list(KS) + [5]
    assert ((rec["diag"][idx] & 0xFF)[~is_long] == 1).all()


@pytest.mark.gpu
def test_chunk_layouts_one_stream():
    """704 pairs: eleven chunks of 0 .. 64 long pairs, one stream (the chunks up to k = 16 as 64-pair units, the
    later ones cut into 16-pair units, a wave each); the queue's tally counts only long pairs."""
    pool, want = batch(chunks(KS))
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, "eleven chunks")
    assert 0 < int(tally[QUEUED]) <= int((want["collision"] == 0).sum()), int(tally[QUEUED])


@pytest.mark.gpu
def test_chunk_layouts_with_partial_chunk():
    """The same list and a last chunk of 37 pairs with 5 long ones."""
    pool, want = batch(chunks(KS, tail=(37, 5)))
    runs, _, _ = run_poisoned(pool)
    assert_records(runs, want, "eleven chunks and a partial one")


@pytest.mark.gpu
def test_no_long_pair_queues_nothing():
    """Short pairs only: every pair leaves the loop after one iteration, so no group is ever stopped."""
    pool, want = batch(chunks((0, 0, 0)))
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, "short pairs only")
    assert int(tally[QUEUED]) == 0


@pytest.mark.gpu
def test_below_one_round_only_the_last_partial_round():
    """200 pairs with 15 long ones: no wave ever holds 16 entries, so only the rounds at the waves' ends run."""
    _, _, long_, short, _ = base()
    idx, _, _ = chunk(15, 200, long_, short, 0, 0)
    pool, want = batch(np.asarray(idx))
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, "below one round")
    assert int(tally[QUEUED]) <= 15


BIG = 400_000            # more 64-pair units (about 4,200) than the launch has workgroups: a wave claims several


@pytest.mark.gpu
def test_waves_claim_several_units():
    """400,000 pairs: a wave takes 64-pair units from the counter one after another, each holding a few long
    pairs (3, 0, 9, 1, 17, 5, 0, 33 in turn), so its ring fills over several units, wraps, and full queued
    rounds run from the round hook between main rounds; then 16-pair units of the same list."""
    idx = tiled(chunks((3, 0, 9, 1, 17, 5, 0, 33)), BIG)
    pool, want = batch(idx)
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, "several units per wave")
    assert 0 < int(tally[QUEUED]) <= int((want["collision"] == 0).sum())


@pytest.mark.gpu
def test_late_stragglers():
    """400,000 pairs, short ones but for the last 1,024 of the 64-pair units (the units just before the list's
    16-pair tail), which hold long pairs only: the waves that claim them have run other units before, and
    their last 64-pair units fill the ring four times over."""
    n_tail = BIG // 2 if BIG // 2 < 2048 * 64 else 2048 * 64          # Units: at most 64 pairs per workgroup
    nbig = (BIG - n_tail) // 64
    _, _, long_, short, _ = base()
    idx = np.resize(short, BIG)
    late = np.arange(64 * (nbig - 1024), 64 * nbig)
    idx[late] = np.resize(long_, len(late))
    pool, want = batch(idx)
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, "late stragglers")
    assert 0 < int(tally[QUEUED]) <= len(late)


@pytest.mark.gpu
def test_medium_and_long_pairs_mixed():
    """Medium and long pairs together, no short ones: queued rounds hold pairs that finish at different
    iterations, so a round that pushes its slowest groups back (GJKEPA_G0_REPUSH) does."""
    _, _, long_, _, medium = base()
    idx = []
    for k in (8, 24, 32, 40, 56, 64, 0, 12):
        c, _, _ = chunk(k, 64, long_, medium, len(idx), len(idx))
        idx += c
    pool, want = batch(np.asarray(idx))
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, "medium and long")
    assert int(tally[QUEUED]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3000, 70000])
def test_batch_sizes(n):
    """The chunk layouts tiled to 3,000 pairs (one stream, small tail units) and 70,000 (the forked chain)."""
    pool, want = batch(tiled(chunks(KS, tail=(37, 5)), n))
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, f"{n} pairs")
    assert 0 < int(tally[QUEUED]) <= int((want["collision"] == 0).sum())


@pytest.mark.gpu
def test_fp32_compute_equals_cpu_model():
    """fp32 compute on the eleven chunks and the partial one: the records of the fp32 path's CPU model (the
    fp32 oracle, its uncertified or failed pairs recomputed in fp64)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle
    from fp32_check import model_fp32
    pool, _ = batch(chunks(KS, tail=(37, 5)))
    model, _ = model_fp32(pool, oracle.gjkepa_batch(pool, 2, 1.0, 16), 16)
    runs, _, _ = run_poisoned(pool, precision=gjkepa.PREC_F32)
    assert_records(runs, model, "fp32 compute")


@pytest.mark.gpu
def test_warm_entry_cold_call():
    """gjkepa_batch_warm_device with fresh warm slots: the plain call's bytes, and the queued pairs' warm
    slots are written by their queued round (a miss mark for a miss, the simplex codes for a hit)."""
    pool, want = batch(tiled(chunks(KS, tail=(37, 5)), 3000))
    runs, tally, codes = run_poisoned(pool, warm=True)
    assert_records(runs, want, "warm entry, cold call")
    assert int(tally[QUEUED]) > 0
    hit = want["collision"] != 0
    assert np.all(codes[~hit, 0] == 0xFFFFFFFE) and np.all(codes[~hit, 1:] == 0xFFFFFFFF)
    assert np.all(codes[hit] != 0xFFFFFFFF)


@pytest.mark.gpu
def test_fp64_vertex_storage_keeps_the_plain_path():
    """The same vertices stored as fp64: that instantiation has no room for the queue (gjk_queue), so nothing is
    queued and the records are the same."""
    pool, want = batch(chunks(KS, tail=(37, 5)))
    pool = gjkepa.HullPool(pool.verts.astype(np.float64), pool.hull_off, pool.hull_cnt, pool.pairs)
    runs, tally, _ = run_poisoned(pool)
    assert_records(runs, want, "fp64 storage")
    assert int(tally[QUEUED]) == 0
