#!/usr/bin/env python3
"""Benchmark of the batched mass properties (gjkepa_mass_batch_device), one MI355X.

A step is one gjkepa_mass_batch_device call over the whole cloud batch (points, offsets, the faces
gjkepa_hull_batch_device wrote, the records and the motion blocks resident in HBM).  Workloads are
tools/bench_hull.py's pools (gjkepa_synth_clouds, seed 0x6A4B5C1D):
  M1: 2^20 clouds of 64 points uniform in the unit ball (bench_hull's H1)
  M3: 2^16 clouds of 256 points on the unit sphere (508 faces each; bench_hull's H3)
Prints one JSON line per config: value = M hulls/s of the mass pass (HIP events on the launch stream, median
step), and beside it gjkepa_hull_batch_device over the same pool, measured the same way in the same process,
with the ratio of the two times.  The first clouds' records are held against the numpy restatement
(tests/mass_ref.py), byte for byte.

    python tools/bench_mass.py [--config M1|M3|all] [--steps K] [--warmup W] [--clouds N]
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
CONFIGS = {   # n_clouds, points, shape, description
    "M1": (1 << 20, 64, 0, "2^20 clouds x 64 points uniform in the unit ball"),
    "M3": (1 << 16, 256, 1, "2^16 clouds x 256 points on the unit sphere (508 faces each)"),
}


def run(name, args, torch, dev):
    n, pts, shape, desc = CONFIGS[name]
    n = args.clouds or n
    lib = gjkepa.load()
    pool = gjkepa.synth_clouds(SEED, n, pts, pts, shape, dtype=np.float32)
    foff = gjkepa.hull_face_offsets(pool.cloud_cnt)
    nslots = int(foff[-1] + 2 * int(pool.cloud_cnt[-1]) - 4)
    p = torch.from_numpy(pool.verts).to(dev)
    off = torch.from_numpy(pool.cloud_off).to(dev)
    cnt = torch.from_numpy(pool.cloud_cnt).to(dev)
    fo = torch.from_numpy(foff).to(dev)
    faces = torch.empty((nslots, 3), dtype=torch.int32, device=dev)
    nf = torch.empty(n, dtype=torch.int32, device=dev)
    nv = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int8, device=dev)
    hv = torch.empty_like(p)
    vi = torch.empty(pool.verts.size, dtype=torch.int32, device=dev)
    out = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    mot = torch.zeros(n * gjkepa.MOTION_DOUBLES, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)

    def hull():
        gjkepa.hull_batch_device(gjkepa.DTYPE_F32, p.data_ptr(), off.data_ptr(), cnt.data_ptr(), n, fo.data_ptr(),
                                 faces.data_ptr(), nf.data_ptr(), nv.data_ptr(), st.data_ptr(), hv.data_ptr(),
                                 vi.data_ptr(), stream.cuda_stream)

    def mass():
        gjkepa.mass_batch_device(gjkepa.DTYPE_F32, p.data_ptr(), off.data_ptr(), cnt.data_ptr(), n, fo.data_ptr(),
                                 faces.data_ptr(), nf.data_ptr(), st.data_ptr(), out.data_ptr(), mot.data_ptr(),
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

    hms = timed(hull)          # leaves the faces the mass pass reads
    ms = timed(mass)
    med, hmed = ms[len(ms) // 2], hms[len(hms) // 2]
    rec = out.cpu().numpy().view(gjkepa.MASS64)
    nfh = nf.cpu().numpy()
    # what the pass has to move: points (fp32), offset / count / face offset / face count / status, the faces, the
    # record and the pivot
    alg = 12.0 * pool.cloud_cnt.astype(np.float64).sum() + n * (8 + 4 + 8 + 4 + 1) + 12.0 * nfh.sum() + n * (128 + 24)
    result = {
        "metric": "M hulls/sec (mass properties of hulls)", "value": round(n / med / 1e3, 4), "unit": "M hulls/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(med, 4), "ms_min": round(ms[0], 4),
        "ms_max": round(ms[-1], 4), "higher_is_better": True, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{name}: {desc}, fp32 storage, fp64 compute", "clouds": n, "seed": SEED},
        "faces_mean": round(float(nfh.mean()), 2), "bytes_per_hull": round(alg / n, 1),
        "achieved_GBs": round(alg / (med * 1e-3) / 1e9, 1),
        "status_counts": {int(k): int(v) for k, v in zip(*np.unique(rec["status"], return_counts=True))},
        "hull_same_pool": {"value": round(n / hmed / 1e3, 4), "unit": "M hulls/s", "ms_per_step": round(hmed, 4),
                           "ms_min": round(hms[0], 4), "ms_max": round(hms[-1], 4)},
        "mass_over_hull_time": round(med / hmed, 4),
        "version": lib.gjkepa_version_string().decode(),
    }
    import mass_ref as mr
    k = min(n, 256)
    sub = gjkepa.CloudPool(pool.verts, pool.cloud_off[:k], pool.cloud_cnt[:k])
    fg = faces.cpu().numpy()
    want = mr.reference(sub, dict(faces=fg, face_off=foff[:k], n_faces=nfh[:k], status=st.cpu().numpy()[:k]))
    pivots = mot.cpu().numpy().reshape(-1, 9)[:k, 6:9]
    result["parity_sample"] = {"clouds": k, "bitexact": bool(rec[:k].tobytes() == want.tobytes()),
                               "pivots": bool(pivots.tobytes() == want["com"].tobytes())}
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS) + ["all"], default="all")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clouds", type=int, default=0)
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in (sorted(CONFIGS) if args.config == "all" else [args.config]):
        run(name, args, torch, dev)


if __name__ == "__main__":
    main()
