#!/usr/bin/env python3
"""Benchmark of the swept broad phase (gjkepa_broadphase_swept_device), one MI355X.

Scene S1 (tools/bench_scene.py: 2^20 hulls x 32 unit-sphere vertices, ~4 static candidate pairs per hull)
with seeded body motions (pivots at the vertex means, v of random direction and length U[0, vmax], w of
random direction and length U[0, 1]).  A step is one device call with the pool, the motions, the list and
the workspace resident in HBM.  Legs, all in one process:
  static      gjkepa_broadphase_device on the scene: the yardstick
  rest        the swept entry with v = 0 and tolerance 1: comparable work to the static entry
  moving      the swept entry with the seeded motions at --tolerance
  bullets     the moving scene plus --bullets bodies with |v| = --bullet-edges cell edges, once with
              long_radius = +inf (the bullets set the cell edge) and once with --long-radius
Prints one JSON line per leg: value = M hulls/s (HIP events on the launch stream, median after warm-up).  The
moving and bullet legs hold the pairs of --check sampled bodies against the numpy restatement of the
definition (tests/sweep_ref.py), and the two bullet legs' lists against each other.

    python tools/bench_sweep.py [--hulls N] [--steps K] [--warmup W] [--legs static,rest,moving,bullets]
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
import sweep_ref as sr  # noqa: E402

SEED = 0x6A4B5C1D
MOTION_SEED = 0x5EE9


def motions(pool, vmax):
    """sweep_ref.motions for a pool of equal hull sizes, vectorised"""
    n, k = len(pool.hull_cnt), int(pool.hull_cnt[0])
    assert (pool.hull_cnt == k).all() and (np.diff(pool.hull_off) == 3 * k).all()
    rng = np.random.default_rng(MOTION_SEED)
    m = np.zeros((n, 9))
    m[:, 0:3] = sr.unit(rng, n) * rng.uniform(0.0, vmax, size=(n, 1))
    m[:, 3:6] = sr.unit(rng, n) * rng.uniform(0.0, 1.0, size=(n, 1))
    m[:, 6:9] = pool.verts.reshape(n, 3, k).astype(np.float64).mean(2)
    return m


def radii(pool, bm):
    n, k = len(pool.hull_cnt), int(pool.hull_cnt[0])
    q = pool.verts.reshape(n, 3, k).astype(np.float64).transpose(0, 2, 1) - bm[:, None, 6:9]
    return np.sqrt(sr.dot(q, q).max(1))


def check_sample(pairs, bm, rho, tolerance, bodies):
    """the list's pairs of the sampled bodies against the restatement over every other body"""
    n = len(bm)
    key = sr.keys(pairs)
    bad = 0
    for a in bodies:
        ok, _ = sr.pair_pass(bm[a, 6:9], bm[a, 0:3], rho[a], bm[:, 6:9], bm[:, 0:3], rho, tolerance)
        hi = np.nonzero(ok & (np.arange(n) > a))[0]
        # as the lower index a the definition's operands are in this order; as the higher one the test is
        # symmetric bit for bit (d, e and m change sign only)
        lo = np.nonzero(ok & (np.arange(n) < a))[0]
        want = np.sort(np.concatenate([lo * (1 << 32) + a, a * (1 << 32) + hi]))
        got = np.sort(key[(pairs[:, 0] == a) | (pairs[:, 1] == a)])
        bad += int(not np.array_equal(want, got))
    return {"bodies": len(bodies), "bodies_whose_pairs_differ": bad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hulls", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tolerance", type=float, default=1e-3)
    ap.add_argument("--vmax", type=float, default=1.0)
    ap.add_argument("--bullets", type=int, default=8)
    ap.add_argument("--bullet-edges", type=float, default=5.0)
    ap.add_argument("--long-radius", type=float, default=6.0)
    ap.add_argument("--check", type=int, default=32)
    ap.add_argument("--legs", default="static,rest,moving,bullets")
    args = ap.parse_args()
    import torch

    n = args.hulls
    box = (n * 113 / 6) ** (1 / 3)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = gjkepa.load()
    pool = gjkepa.synth_scene(SEED, n, 32, 32, box)
    bm = motions(pool, args.vmax)
    rho = radii(pool, bm)
    v, off, cnt = (torch.from_numpy(x).to(dev) for x in (pool.verts, pool.hull_off, pool.hull_cnt))
    mot = torch.zeros(9 * n, dtype=torch.float64, device=dev)
    cap = 16 * n
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    npair = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = max(gjkepa.broadphase_workspace_bytes(n, cap), gjkepa.broadphase_swept_workspace_bytes(n, cap))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    sample = np.random.default_rng(3).choice(n, size=min(args.check, n), replace=False)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize(dev)
        return sorted(a.elapsed_time(b) for a, b in ev)

    def report(leg, ms, extra):
        med = ms[len(ms) // 2]
        found = int(npair.item())
        assert found <= cap, (found, cap)
        print(json.dumps({"metric": f"M hulls/sec through the swept broad phase (leg {leg})", "leg": leg,
                          "value": round(n / med / 1e3, 3), "unit": "M hulls/s", "ms_per_step": round(med, 4),
                          "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "n_gpus": 1, "steps": args.steps,
                          "warmup": args.warmup, "higher_is_better": True, "hulls": n, "pairs": found, "list_capacity": cap,
                          "version": lib.gjkepa_version_string().decode(), **extra}), flush=True)
        return med

    def static():
        gjkepa.broadphase_device(gjkepa.DTYPE_F32, v.data_ptr(), off.data_ptr(), cnt.data_ptr(), n, pairs.data_ptr(), cap,
                                 npair.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream)

    def swept(tolerance, long_radius):
        return lambda: gjkepa.broadphase_swept_device(gjkepa.DTYPE_F32, v.data_ptr(), off.data_ptr(), cnt.data_ptr(), n,
                                                      mot.data_ptr(), tolerance, long_radius, pairs.data_ptr(), cap,
                                                      npair.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream)

    def the_list():
        return pairs[:int(npair.item())].cpu().numpy()

    legs = args.legs.split(",")
    base = None
    if "static" in legs:
        base = report("static", timed(static), {})
    if "rest" in legs:
        rest = bm.copy()
        rest[:, 0:3] = 0.0
        mot.copy_(torch.from_numpy(rest.reshape(-1)))
        med = report("rest", timed(swept(1.0, float("inf"))), {"tolerance": 1.0, "long_radius": "inf"})
        if base:
            print(json.dumps({"leg": "rest", "swept_over_static": round(med / base, 3)}), flush=True)
    if "moving" in legs:
        mot.copy_(torch.from_numpy(bm.reshape(-1)))
        ms = timed(swept(args.tolerance, float("inf")))
        report("moving", ms, {"tolerance": args.tolerance, "vmax": args.vmax, "long_radius": "inf",
                              "swept_over_static": round(ms[len(ms) // 2] / base, 3) if base else None,
                              "parity_sample": check_sample(the_list(), bm, rho, args.tolerance, sample)})
    if "bullets" in legs:
        edge = 2.0 * float((rho + 0.5 * np.linalg.norm(bm[:, 0:3], axis=1)).max()) + args.tolerance
        shot = bm.copy()
        who = np.random.default_rng(4).choice(n, size=args.bullets, replace=False)
        shot[who, 0:3] = sr.unit(np.random.default_rng(5), args.bullets) * args.bullet_edges * edge
        mot.copy_(torch.from_numpy(shot.reshape(-1)))
        lists = []
        for lr in (float("inf"), args.long_radius):
            ms = timed(swept(args.tolerance, lr))
            lists.append(the_list())
            report("bullets", ms, {"tolerance": args.tolerance, "vmax": args.vmax, "bullets": args.bullets,
                                   "bullet_travel": round(args.bullet_edges * edge, 3), "cell_edge_without_bullets": round(edge, 3),
                                   "long_radius": "inf" if lr == float("inf") else lr,
                                   "parity_sample": check_sample(lists[-1], shot, rho, args.tolerance,
                                                                 np.concatenate([who, sample[:8]]))})
        print(json.dumps({"leg": "bullets", "lists_identical": bool(np.array_equal(lists[0], lists[1]))}), flush=True)


if __name__ == "__main__":
    main()
