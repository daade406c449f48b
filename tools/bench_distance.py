#!/usr/bin/env python3
"""Benchmark of the separation-distance query (gjkepa_distance_batch_device), one MI355X.

A step is one gjkepa_distance_batch_device call over the whole pair batch (pool, pair list, the
batch's contact records and the output resident in HBM), with `records` = the output of one
gjkepa_batch_device call on the same pairs: hits are skipped, every miss is computed.  Workloads are
bench.py's C2 and C4 pools (gjkepa_synth_pairs, seed 0x6A4B5C1D):
  C2: 2^20 pairs of 32-vertex hulls (distance tier 0)
  C4: 2^22 pairs of 8-256-vertex hulls (all three tiers)
Prints one JSON line: value = M pairs/s of the whole batch (HIP events on the launch stream), the
share of misses, the largest iteration count, and beside it the GJK kernels' launch times for the same
batch from gjkepa_launch_timing, the closest existing yardstick (the same support scans, a similar
iteration count).  A sample of the misses is checked with the records' own certificate.

    python tools/bench_distance.py [--config C2|C4] [--steps K] [--warmup W] [--pairs N] [--max-distance D]
                                   [--no-records]
"""
from __future__ import annotations

import argparse
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
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="C2")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--max-distance", type=float, default=float("inf"))
    ap.add_argument("--no-records", action="store_true", help="records = NULL: every pair computed, overlaps found here")
    args = ap.parse_args()
    import torch

    lo, hi, rmax, n, desc = CONFIGS[args.config]
    n = args.pairs or n
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = gjkepa.load()
    pool = gjkepa.synth_pairs(SEED, n, lo, hi, rmax, dtype=np.float32)
    verts = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.hull_off).to(dev)
    cnt = torch.from_numpy(pool.hull_cnt).to(dev)
    prs = torch.from_numpy(pool.pairs.reshape(-1)).to(dev)
    wsb, dwsb = gjkepa.workspace_bytes(n), gjkepa.distance_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    dws = torch.zeros(dwsb, dtype=torch.uint8, device=dev)
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    # the batch whose records feed the distance query: once to warm up, once with its per-launch timing
    for timed in (False, True):
        gjkepa.launch_timing(timed)
        gjkepa.gjkepa_batch_device(2, 1.0, gjkepa.DTYPE_F32, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(),
                                   cnt.data_ptr(), prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb,
                                   stream.cuda_stream)
        torch.cuda.synchronize(dev)
    gjkepa.launch_timing(False)
    lt = gjkepa.launch_timing_read()
    gjk = [{"tier": int(t["tier"]), "ms": round(float(t["end_ms"] - t["start_ms"]), 4)} for t in lt if t["kernel"] == b"gjk"]

    def launch():
        gjkepa.distance_batch_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                     0 if args.no_records else contact.data_ptr(), gjkepa.PREC_F64, args.max_distance,
                                     out.data_ptr(),
                                     dws.data_ptr(), dwsb, stream.cuda_stream)

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in ev:
        a.record(stream)
        launch()
        b.record(stream)
    torch.cuda.synchronize(dev)
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    med = ms[len(ms) // 2]

    rec = out.cpu().numpy().view(gjkepa.DIST64)
    hit = (rec["flags"] & gjkepa.DIST_HIT) != 0
    computed = ~hit & (rec["status"] != gjkepa.STATUS_BAD_INPUT)
    sep = computed & ((rec["flags"] & gjkepa.DIST_OVERLAP) == 0)
    result = {
        "metric": "M pairs/sec (separation distance after a batch, hits skipped)", "value": round(n / med / 1e3, 4),
        "unit": "M pairs/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(med, 4),
        "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "higher_is_better": True, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{args.config}: {desc}, fp32 storage, fp64 compute", "pairs": n, "seed": SEED,
                   "max_distance": None if np.isinf(args.max_distance) else args.max_distance,
                   "records": not args.no_records},
        "miss_share": round(float(computed.mean()), 4),
        "computed_pairs_per_s_M": round(float(computed.sum()) / med / 1e3, 4),
        "iters_max": int(rec["iters"].max()), "iters_mean_computed": round(float(rec["iters"][computed].mean()), 3),
        "flag_counts": {"hit": int(hit.sum()), "overlap": int(((rec["flags"] & gjkepa.DIST_OVERLAP) != 0).sum()),
                        "far": int(((rec["flags"] & gjkepa.DIST_FAR) != 0).sum())},
        "status_counts": {int(k): int(v) for k, v in zip(*np.unique(rec["status"], return_counts=True))},
        "gjk_launches_same_batch_ms": gjk, "gjk_launches_total_ms": round(sum(g["ms"] for g in gjk), 4),
        "version": lib.gjkepa_version_string().decode(),
    }
    import contextlib

    import distance_ref as dr
    idx = np.nonzero(sep & ((rec["flags"] & gjkepa.DIST_FAR) == 0))[0][:512]
    with contextlib.redirect_stdout(sys.stderr):        # the checker's own report line
        upper, lower = dr.check_certificate(pool, rec, idx)
    result["certificate_sample"] = {"pairs": int(len(idx)), "worst_relative_gap": float(((upper - lower) / upper).max())}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
