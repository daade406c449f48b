#!/usr/bin/env python3
"""Benchmark of the contact manifold at the time of impact (gjkepa_manifold_cast_batch_device), one MI355X.

A step is one gjkepa_manifold_cast_batch_device call over the whole pair batch (pool, pair list, motion blocks,
cast records and the output resident in HBM).  Workloads are bench.py's pools (gjkepa_synth_pairs, seed
0x6A4B5C1D), every hull a body of its own:
  C2: 2^18 pairs of 32-vertex hulls (tier 0)
  C4: 2^18 pairs of 8-256-vertex hulls (all three tiers)
Hull B of every pair moves onto hull A's centre while both bodies spin (|w| up to 0.5 about their vertex means),
and the cast records come from one gjkepa_cast_rigid_batch_device call without contact records at tau = 1e-3:
every pair that does not overlap at t = 0 is an IMPACT and is computed, every overlapping pair is a START with a
zero normal and is answered NO_HIT by the filter.
Prints one JSON line per config: ms per call (HIP events on the launch stream, median step), the computed
pairs and the time per computed pair, and beside it, measured the same way in the same process on the same
pool, gjkepa_manifold_batch_device with the records of one gjkepa_batch_device call (its computed pairs are the
overlapping ones), with its time per computed pair and the ratio of the two.  On the whole list the two kernels
compute different shares of it and answer the rest in the filter, so both are timed again on a list of their
own on which every pair is computed: the first M pairs each computes, M the same for both ("dense").  The first
computed records are held against the numpy reference of tests/impact_ref.py.

    python tools/bench_impact.py [--config C2|C4|all] [--steps K] [--warmup W] [--pairs N] [--margin M]
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
TAU = 1e-3
CONFIGS = {   # n_min, n_max, r_max, pairs, description
    "C2": (32, 32, 2.5, 1 << 18, "256K random 32-vertex convex-hull pairs"),
    "C4": (8, 256, 2.5, 1 << 18, "256K pairs, mixed hull sizes 8-256 vertices"),
}


def motions(pool):
    """hull B onto hull A's centre, both spinning about their vertex means"""
    nh = len(pool.hull_cnt)
    c = centres(pool)
    rng = np.random.default_rng(SEED)
    m = np.zeros((nh, 9))
    a, b = pool.pairs[:, 0], pool.pairs[:, 1]
    m[b, 0:3] = c[a] - c[b]
    u = rng.normal(size=(nh, 3))
    m[:, 3:6] = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.0, 0.5, size=(nh, 1))
    m[:, 6:9] = c
    return m


def centres(pool):
    """vertex means of every hull of a pool whose hulls are stored as x, y, z columns at hull_off"""
    v = pool.verts.astype(np.float64)
    cnt, off = pool.hull_cnt.astype(np.int64), pool.hull_off.astype(np.int64)
    out = np.zeros((len(cnt), 3))
    for n in np.unique(cnt):
        sel = np.nonzero(cnt == n)[0]
        idx = off[sel][:, None] + np.arange(3 * n)[None]
        out[sel] = v[idx].reshape(len(sel), 3, n).mean(2)
    return out


def run(name, args, torch, dev):
    lo, hi, rmax, n, desc = CONFIGS[name]
    n = args.pairs or n
    lib = gjkepa.load()
    pool = gjkepa.synth_pairs(SEED, n, lo, hi, rmax, dtype=np.float32)
    bm = motions(pool)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    verts, off, cnt, prs, mot = up(pool.verts), up(pool.hull_off), up(pool.hull_cnt), up(pool.pairs.reshape(-1)), up(bm.reshape(-1))
    wsb, cwsb, mwsb = gjkepa.workspace_bytes(n), gjkepa.cast_rigid_workspace_bytes(n), gjkepa.manifold_cast_workspace_bytes(n)
    ws, cws, mws = (torch.zeros(b, dtype=torch.uint8, device=dev) for b in (wsb, cwsb, mwsb))
    contact = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    cast = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 160, dtype=torch.uint8, device=dev)
    cout = torch.zeros(n * 160, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    pool_args = (gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs.data_ptr(), n)

    for _ in range(2):          # the records both manifolds read (the first calls warm up)
        gjkepa.gjkepa_batch_device(2, 1.0, gjkepa.DTYPE_F32, gjkepa.PREC_F64, *pool_args[1:], contact.data_ptr(), ws.data_ptr(),
                                   wsb, stream.cuda_stream)
        gjkepa.cast_rigid_batch_device(*pool_args, mot.data_ptr(), TAU, 0, gjkepa.PREC_F64, cast.data_ptr(), cws.data_ptr(),
                                       cwsb, stream.cuda_stream)
        torch.cuda.synchronize(dev)

    def at_toi():
        gjkepa.manifold_cast_batch_device(*pool_args, mot.data_ptr(), cast.data_ptr(), 0, gjkepa.PREC_F64, args.margin,
                                          out.data_ptr(), mws.data_ptr(), mwsb, stream.cuda_stream)

    def contact_manifold():
        gjkepa.manifold_batch_device(*pool_args, contact.data_ptr(), gjkepa.PREC_F64, args.margin, cout.data_ptr(),
                                     mws.data_ptr(), mwsb, stream.cuda_stream)

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

    ms, cms = timed(at_toi), timed(contact_manifold)
    med, cmed = ms[len(ms) // 2], cms[len(cms) // 2]
    rec = out.cpu().numpy().view(gjkepa.MANIFOLD64).copy()
    crec = cout.cpu().numpy().view(gjkepa.MANIFOLD64).copy()
    castr = cast.cpu().numpy().view(gjkepa.CAST64)
    computed = ((rec["flags"] & gjkepa.MANIFOLD_NO_HIT) == 0) & (rec["status"] == gjkepa.STATUS_OK)
    ccomputed = ((crec["flags"] & gjkepa.MANIFOLD_NO_HIT) == 0) & (crec["status"] == gjkepa.STATUS_OK)
    # the dense lists: M pairs each, every one computed
    m = int(min(computed.sum(), ccomputed.sum()))
    ia, ic = np.nonzero(computed)[0][:m], np.nonzero(ccomputed)[0][:m]
    prs_a, prs_c = up(pool.pairs[ia].reshape(-1)), up(pool.pairs[ic].reshape(-1))
    cast_a = up(castr[ia].view(np.uint8).reshape(-1))
    con_c = up(contact.cpu().numpy().view(gjkepa.REC64)[ic].view(np.uint8).reshape(-1))

    def at_toi_dense():
        gjkepa.manifold_cast_batch_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs_a.data_ptr(), m,
                                          mot.data_ptr(), cast_a.data_ptr(), 0, gjkepa.PREC_F64, args.margin, out.data_ptr(),
                                          mws.data_ptr(), mwsb, stream.cuda_stream)

    def contact_dense():
        gjkepa.manifold_batch_device(gjkepa.DTYPE_F32, verts.data_ptr(), off.data_ptr(), cnt.data_ptr(), prs_c.data_ptr(), m,
                                     con_c.data_ptr(), gjkepa.PREC_F64, args.margin, cout.data_ptr(), mws.data_ptr(), mwsb,
                                     stream.cuda_stream)

    dms, dcms = timed(at_toi_dense), timed(contact_dense)
    dmed, dcmed = dms[len(dms) // 2], dcms[len(dcms) // 2]
    assert out.cpu().numpy().view(gjkepa.MANIFOLD64)[:m].tobytes() == rec[ia].tobytes()
    assert cout.cpu().numpy().view(gjkepa.MANIFOLD64)[:m].tobytes() == crec[ic].tobytes()
    assert ((rec["flags"][computed] & gjkepa.MANIFOLD_AT_TOI) != 0).all()
    hist = np.bincount(rec["n_points"][computed], minlength=5)
    ns, cns = med * 1e6 / max(1, int(computed.sum())), cmed * 1e6 / max(1, int(ccomputed.sum()))
    result = {
        "metric": "ms per call (contact manifold at the time of impact after a rigid cast)", "value": round(med, 4),
        "unit": "ms", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_min": round(ms[0], 4),
        "ms_max": round(ms[-1], 4), "higher_is_better": False, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{name}: {desc}, fp32 storage, fp64 compute", "pairs": n, "seed": SEED, "margin": args.margin,
                   "tolerance": TAU},
        "computed_pairs": int(computed.sum()), "ns_per_computed_pair": round(ns, 3),
        "undecided_casts": int((castr["status"] == gjkepa.STATUS_CAST_MAXITER).sum()),
        "n_points_share": {str(k): round(float(hist[k]) / max(1, int(computed.sum())), 6) for k in range(1, 5)},
        "contact_manifold_same_pool_ms": round(cmed, 4), "contact_manifold_ms_min": round(cms[0], 4),
        "contact_manifold_ms_max": round(cms[-1], 4), "contact_manifold_computed_pairs": int(ccomputed.sum()),
        "contact_manifold_ns_per_computed_pair": round(cns, 3), "per_pair_over_contact_manifold": round(ns / cns, 4),
        "dense": {"pairs": m, "ms": round(dmed, 4), "ms_min": round(dms[0], 4), "ms_max": round(dms[-1], 4),
                  "ns_per_pair": round(dmed * 1e6 / max(1, m), 3), "contact_manifold_ms": round(dcmed, 4),
                  "contact_manifold_ms_min": round(dcms[0], 4), "contact_manifold_ms_max": round(dcms[-1], 4),
                  "contact_manifold_ns_per_pair": round(dcmed * 1e6 / max(1, m), 3),
                  "over_contact_manifold": round(dmed / dcmed, 4)},
        "version": lib.gjkepa_version_string().decode(),
    }
    import impact_ref as ir
    idx = np.nonzero(computed)[0][:128]
    sub = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, pool.pairs[idx])
    with contextlib.redirect_stdout(sys.stderr):        # the checker's own report line
        ir.check_pool(sub, bm, castr[idx], rec[idx], margin=args.margin, name="bench sample")
    result["checked_sample"] = int(len(idx))
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS) + ["all"], default="all")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--margin", type=float, default=1e-6)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in (sorted(CONFIGS) if args.config == "all" else [args.config]):
        run(name, args, torch, dev)


if __name__ == "__main__":
    main()
