#!/usr/bin/env python3
"""Benchmark of the contact-manifold query (gjkepa_manifold_batch_device), one MI355X.

A step is one gjkepa_manifold_batch_device call over the whole pair batch (pool, pair list, the batch's
contact records and the output resident in HBM), with `records` = the output of one gjkepa_batch_device
call on the same pairs: every hit is computed, every miss answered NO_HIT by the filter.  Workloads are
bench.py's C2 and C4 pools (gjkepa_synth_pairs, seed 0x6A4B5C1D):
  C2: 2^20 pairs of 32-vertex hulls (tier 0)
  C4: 2^22 pairs of 8-256-vertex hulls (all three tiers)
Random sphere hulls touch in a vertex, an edge crossing or a vertex on a face: nearly every hit of C2 and
C4 is a one-point manifold.  A third workload times the patch arithmetic itself:
  BOX: 2^18 pairs, the tests' rotated box stacks (tests/manifold_ref.py box_pool, 4096 distinct stacks,
       each listed 64 times: the hulls stay in cache, so this is the clip's time, not HBM's)
Prints one JSON line: value = M pairs/s of the whole batch (HIP events on the launch stream, median of
the steps), the share of hits, the hits by n_points, and beside it, measured in the same process on the
same batch, gjkepa_distance_batch_device with records = NULL: the project's yardstick for a kernel
that makes one pass over the hulls of every pair.  A sample of the hits is checked against the
reference of tests/manifold_ref.py.

    python tools/bench_manifold.py [--config C2|C4|BOX] [--steps K] [--warmup W] [--pairs N] [--margin M]
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "collision-detect-gjk-epa_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import gjkepa  # noqa: E402

SEED = 0x6A4B5C1D
CONFIGS = {   # n_min, n_max, r_max, pairs, description
    "C2": (32, 32, 2.5, 1 << 20, "1M random 32-vertex convex-hull pairs"),
    "C4": (8, 256, 2.5, 4 << 20, "4M pairs, mixed hull sizes 8-256 vertices"),
    "BOX": (8, 8, 0.0, 1 << 18, "256K pairs: 4096 rotated box stacks listed 64 times"),
}
BOX_STACKS = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="C2")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--margin", type=float, default=1e-6)
    args = ap.parse_args()
    import torch

    lo, hi, rmax, n, desc = CONFIGS[args.config]
    n = args.pairs or n
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = gjkepa.load()
    if args.config == "BOX":
        import manifold_ref as mr
        base = mr.box_pool(n=min(BOX_STACKS, n), seed=SEED).as_dtype(np.float32)
        pool = gjkepa.HullPool(base.verts, base.hull_off, base.hull_cnt, np.tile(base.pairs, (-(-n // base.n_pairs), 1))[:n])
    else:
        pool = gjkepa.synth_pairs(SEED, n, lo, hi, rmax, dtype=np.float32)
    verts = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.hull_off).to(dev)
    cnt = torch.from_numpy(pool.hull_cnt).to(dev)
    prs = torch.from_numpy(pool.pairs.reshape(-1)).to(dev)
    wsb, mwsb, dwsb = gjkepa.workspace_bytes(n), gjkepa.manifold_workspace_bytes(n), gjkepa.distance_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    mws = torch.zeros(mwsb, dtype=torch.uint8, device=dev)
    dws = torch.zeros(dwsb, dtype=torch.uint8, device=dev)
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 160, dtype=torch.uint8, device=dev)
    dout = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    for _ in range(2):          # the batch whose records feed the manifold (the first call warms up)
        gjkepa.gjkepa_batch_device(2, 1.0, gjkepa.DTYPE_F32, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(),
                                   cnt.data_ptr(), prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb,
                                   stream.cuda_stream)
        torch.cuda.synchronize(dev)

    def manifold():
        gjkepa.manifold_batch_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                     contact.data_ptr(), gjkepa.PREC_F64, args.margin, out.data_ptr(), mws.data_ptr(), mwsb,
                                     stream.cuda_stream)

    def distance():             # the yardstick: every pair computed (records = NULL)
        gjkepa.distance_batch_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                     0, gjkepa.PREC_F64, float("inf"), dout.data_ptr(), dws.data_ptr(), dwsb,
                                     stream.cuda_stream)

    def timed(launch):
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record(stream)
            launch()
            b.record(stream)
        torch.cuda.synchronize(dev)
        return sorted(a.elapsed_time(b) for a, b in ev)

    ms = timed(manifold)
    dms = timed(distance)
    med, dmed = ms[len(ms) // 2], dms[len(dms) // 2]

    rec = out.cpu().numpy().view(gjkepa.MANIFOLD64)
    crec = contact.cpu().numpy().view(gjkepa.REC64)
    computed = ((rec["flags"] & gjkepa.MANIFOLD_NO_HIT) == 0) & (rec["status"] == gjkepa.STATUS_OK)
    hist = np.bincount(rec["n_points"][computed], minlength=5)
    result = {
        "metric": "M pairs/sec (contact manifold after a batch, misses answered NO_HIT)", "value": round(n / med / 1e3, 4),
        "unit": "M pairs/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(med, 4),
        "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "higher_is_better": True, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{args.config}: {desc}, fp32 storage, fp64 compute", "pairs": n, "seed": SEED,
                   "margin": args.margin},
        "hit_share": round(float(computed.mean()), 4),
        "computed_pairs_per_s_M": round(float(computed.sum()) / med / 1e3, 4),
        "n_points_share": {str(k): round(float(hist[k]) / max(1, int(computed.sum())), 6) for k in range(1, 5)},
        "flag_counts": {"no_hit": int(((rec["flags"] & gjkepa.MANIFOLD_NO_HIT) != 0).sum()),
                        "decimated": int(((rec["flags"] & gjkepa.MANIFOLD_DECIMATED) != 0).sum()),
                        "fallback": int(((rec["flags"] & gjkepa.MANIFOLD_FALLBACK) != 0).sum())},
        "status_counts": {int(k): int(v) for k, v in zip(*np.unique(rec["status"], return_counts=True))},
        "feature_size_max": [int(rec["n_feat_a"].max()), int(rec["n_feat_b"].max())],
        "distance_no_records_same_batch_ms": round(dmed, 4), "distance_ms_min": round(dms[0], 4),
        "distance_ms_max": round(dms[-1], 4), "manifold_over_distance": round(med / dmed, 4),
        "version": lib.gjkepa_version_string().decode(),
    }
    import manifold_ref as mr
    idx = np.nonzero(computed)[0][:256]
    sub = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[idx])
    with contextlib.redirect_stdout(sys.stderr):        # the checker's own report line
        mr.check_pool(sub, crec[idx], rec[idx], margin=args.margin, name="bench sample", min_hits=1)
    result["checked_sample"] = int(len(idx))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
