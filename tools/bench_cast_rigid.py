#!/usr/bin/env python3
"""Benchmark of the rigid-motion cast (gjkepa_cast_rigid_batch_device) and the pool pose
(gjkepa_pose_pool_device), one MI355X.

A step is one gjkepa_cast_rigid_batch_device call over the whole pair batch (pool, pair list, body motions,
the batch's contact records and the output resident in HBM), with `records` = the output of one
gjkepa_batch_device call on the same pairs: hits are skipped, every miss is cast.  Workloads are bench.py's C2
and C4 pools (gjkepa_synth_pairs, seed 0x6A4B5C1D) with tools/bench_cast.py's motions d per pair:
  C2: 2^20 pairs of 32-vertex hulls (cast tier 0)
  C4: 2^22 pairs of 8-256-vertex hulls (all three tiers)
Two legs, each beside the yardstick gjkepa_cast_batch_device (the linear cast) on the same batch, records and
motion d, measured the same way in the same process:
  w0:   w = 0 for both bodies, v_A = 0, v_B = d.  The rigid entry must produce the linear cast's flags; its
        cost over the linear cast is the price of the pose arithmetic and the two-direction support scan.
  spin: v_A = -0.3 d, v_B = 0.7 d, rotation vectors of random direction and length U[0, 1], pivots at the
        hulls' vertex means (tests/cast_rigid_ref.py motions): time, steps and iterations per cast pair and
        the CAST_MAXITER share.
Prints one JSON line per run: value = M pairs/s of the whole batch (HIP events on the launch stream, median
after warm-up).

    python tools/bench_cast_rigid.py [--config C2|C4] [--steps K] [--warmup W] [--pairs N] [--tolerance T]
    python tools/bench_cast_rigid.py --pose [--hulls N]     # the pose kernel: 2^21 hulls of 32, fp32 in and out
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "collision-detect-gjk-epa_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import gjkepa  # noqa: E402
from bench_cast import CONFIGS, MOTION_SEED, SEED, motions  # noqa: E402

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E peak, the figure DESIGN.md §5 uses


def centroids(pool):
    cnt = pool.hull_cnt.astype(np.int64)
    starts = (pool.hull_off[:, None] + cnt[:, None] * np.arange(3)[None]).reshape(-1)
    return np.add.reduceat(pool.verts, starts, dtype=np.float64).reshape(-1, 3) / cnt[:, None]


def body_motions(pool, d, seed, spin):
    """(n_hulls, 9): spin False: w = 0, v_A = 0, v_B = d; True: tests/cast_rigid_ref.py motions()"""
    nh = len(pool.hull_cnt)
    m = np.zeros((nh, 9))
    m[:, 6:9] = centroids(pool)
    if not spin:
        m[pool.pairs[:, 1], 0:3] = d
        return m
    rng = np.random.default_rng(seed ^ 0x5A17)
    m[pool.pairs[:, 0], 0:3] = -0.3 * d
    m[pool.pairs[:, 1], 0:3] = 0.7 * d
    u = rng.normal(size=(nh, 3))
    m[:, 3:6] = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, size=(nh, 1))
    return m


def timed(torch, dev, stream, launch, steps, warmup):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record(stream)
        launch()
        b.record(stream)
    torch.cuda.synchronize(dev)
    return sorted(a.elapsed_time(b) for a, b in ev)


def summary(rec):
    ok = rec["status"] == gjkepa.STATUS_OK
    skipped = (rec["flags"] & gjkepa.CAST_SKIPPED) != 0
    impact = ok & (rec["flags"] == gjkepa.CAST_IMPACT)
    computed = ~skipped & (rec["status"] != gjkepa.STATUS_BAD_INPUT)
    stopped = rec["status"] == gjkepa.STATUS_CAST_MAXITER
    return {
        "flag_counts": {"impact": int(impact.sum()), "miss": int((ok & (rec["flags"] == 0)).sum()),
                        "start": int((ok & (rec["flags"] == gjkepa.CAST_START)).sum()), "skipped": int(skipped.sum())},
        "status_counts": {int(k): int(v) for k, v in zip(*np.unique(rec["status"], return_counts=True))},
        "computed_pairs": int(computed.sum()),
        "cast_maxiter_share_of_computed": round(float(stopped.sum()) / max(1, int(computed.sum())), 6),
        "steps_mean_computed": round(float(rec["steps"][computed].mean()), 3),
        "steps_mean_impact": round(float(rec["steps"][impact].mean()), 3) if impact.any() else 0.0,
        "steps_p99_impact": float(np.percentile(rec["steps"][impact], 99)) if impact.any() else 0.0,
        "steps_max": int(rec["steps"].max()),
        "iters_mean_computed": round(float(rec["iters"][computed].mean()), 3), "iters_max": int(rec["iters"].max()),
    }


def bench_cast(args, torch, dev, lib):
    lo, hi, rmax, n, desc = CONFIGS[args.config]
    n = args.pairs or n
    pool = gjkepa.synth_pairs(SEED, n, lo, hi, rmax, dtype=np.float32)
    d = motions(pool, MOTION_SEED)
    verts = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.hull_off).to(dev)
    cnt = torch.from_numpy(pool.hull_cnt).to(dev)
    prs = torch.from_numpy(pool.pairs.reshape(-1)).to(dev)
    mot = torch.from_numpy(d.reshape(-1)).to(dev)
    wsb, cwsb = gjkepa.workspace_bytes(n), gjkepa.cast_rigid_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    cws = torch.zeros(cwsb, dtype=torch.uint8, device=dev)
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    lout = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    for _ in range(2):            # the batch whose records feed the casts
        gjkepa.gjkepa_batch_device(2, 1.0, gjkepa.DTYPE_F32, gjkepa.PREC_F64, verts.data_ptr(), off.data_ptr(),
                                   cnt.data_ptr(), prs.data_ptr(), n, contact.data_ptr(), ws.data_ptr(), wsb,
                                   stream.cuda_stream)
        torch.cuda.synchronize(dev)

    def linear():
        gjkepa.cast_batch_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n,
                                 mot.data_ptr(), args.tolerance, contact.data_ptr(), gjkepa.PREC_F64, lout.data_ptr(),
                                 cws.data_ptr(), cwsb, stream.cuda_stream)

    lms = timed(torch, dev, stream, linear, args.steps, args.warmup)
    lrec = lout.cpu().numpy().view(gjkepa.CAST64).copy()
    lmed = lms[len(lms) // 2]
    base = {"unit": "M pairs/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
            "dtype": "f64", "data": "synthetic", "version": lib.gjkepa_version_string().decode(),
            "config": {"workload": f"{args.config}: {desc}, fp32 storage, fp64 compute", "pairs": n, "seed": SEED,
                       "motion_seed": MOTION_SEED, "tolerance": args.tolerance, "records": True},
            "linear_cast_same_batch": {"ms_per_step": round(lmed, 4), "ms_min": round(lms[0], 4), "ms_max": round(lms[-1], 4),
                                       **summary(lrec)}}
    for leg in ("w0", "spin"):
        bm = torch.from_numpy(body_motions(pool, d, MOTION_SEED, leg == "spin").reshape(-1)).to(dev)

        def rigid():
            gjkepa.cast_rigid_batch_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(),
                                           n, bm.data_ptr(), args.tolerance, contact.data_ptr(), gjkepa.PREC_F64,
                                           out.data_ptr(), cws.data_ptr(), cwsb, stream.cuda_stream)

        ms = timed(torch, dev, stream, rigid, args.steps, args.warmup)
        rec = out.cpu().numpy().view(gjkepa.CAST64)
        med = ms[len(ms) // 2]
        result = dict(base)
        result.update({"metric": f"M pairs/sec (rigid-motion cast after a batch, hits skipped; leg {leg})", "leg": leg,
                       "value": round(n / med / 1e3, 4), "ms_per_step": round(med, 4), "ms_min": round(ms[0], 4),
                       "ms_max": round(ms[-1], 4), "rigid_over_linear": round(med / lmed, 3), **summary(rec)})
        if leg == "w0":
            same = (rec["flags"] == lrec["flags"]) & (rec["status"] == lrec["status"])
            result["flags_equal_linear_cast"] = bool(same.all())
            result["flags_differing_pairs"] = int((~same).sum())
            both = (rec["flags"] == gjkepa.CAST_IMPACT) & same
            result["toi_max_abs_difference_to_linear"] = float(np.abs(rec["toi"][both] - lrec["toi"][both]).max()) if both.any() else 0.0
        print(json.dumps(result), flush=True)
        del bm


def bench_pose(args, torch, dev, lib):
    nh = args.hulls or (1 << 21)
    pool = gjkepa.synth_pairs(SEED, nh // 2, 32, 32, 2.5, dtype=np.float32)
    d = motions(pool, MOTION_SEED)
    bm = torch.from_numpy(body_motions(pool, d, MOTION_SEED, True).reshape(-1)).to(dev)
    verts = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.hull_off).to(dev)
    cnt = torch.from_numpy(pool.hull_cnt).to(dev)
    out = torch.zeros_like(verts)
    status = torch.zeros(nh, dtype=torch.int8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def pose():
        gjkepa.pose_pool_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), nh, bm.data_ptr(), 0,
                                gjkepa.DTYPE_F32, out.data_ptr(), status.data_ptr(), stream.cuda_stream)

    ms = timed(torch, dev, stream, pose, args.steps, args.warmup)
    med = ms[len(ms) // 2]
    # bytes moved per hull: vertices in and out, offset, count, motion block, status
    moved = nh * (2 * 32 * 3 * 4 + 8 + 4 + 72 + 1)
    ok = bool((status.cpu().numpy() == gjkepa.STATUS_OK).all())
    print(json.dumps({"metric": "G vertices/sec (pool pose, fp32 in and out, t = 1)", "value": round(nh * 32 / med / 1e6, 4),
                      "unit": "G vertices/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(med, 4),
                      "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "higher_is_better": True, "hulls": nh,
                      "bytes_moved": moved, "achieved_GBs": round(moved / med / 1e6, 1), "hbm_peak_GBs": HBM_PEAK_GBS,
                      "share_of_hbm_peak": round(moved / med / 1e6 / HBM_PEAK_GBS, 4), "all_status_ok": ok,
                      "version": lib.gjkepa_version_string().decode()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="C2")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--pose", action="store_true", help="benchmark the pose kernel instead")
    ap.add_argument("--hulls", type=int, default=0)
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = gjkepa.load()
    (bench_pose if args.pose else bench_cast)(args, torch, dev, lib)


if __name__ == "__main__":
    main()
