#!/usr/bin/env python3
"""Benchmark of the event pass (gjkepa_events_device), one MI355X.

The pair list and the records of tools/bench_sweep.py's moving leg (scene S1, 2^20 hulls x 32
unit-sphere vertices with seeded motions, about 1.75 M swept pairs at tolerance 1e-3), built once on the device:
swept broad phase -> gjkepa_batch_device -> gjkepa_cast_rigid_batch_device with the batch's records.  A step is
one device call with every buffer resident in HBM.  Legs, all in one process:
  events        the event pass with the body outputs
  events_list   the event pass without them (body_time = body_event = NULL)
  compact       gjkepa_compact_hits_device over the same number of records: the yardstick for one pass over
                record lines
  cast          the rigid cast over the same list: the step the pass follows
Prints one JSON line per leg (HIP events on the launch stream, median after warm-up) and a summary line with
the event pass's share of the cast and its ratio to the compaction.  --check holds the events and body outputs
of the first call against the numpy restatement (tests/events_ref.py) on the downloaded records.

    python tools/bench_events.py [--hulls N] [--steps K] [--warmup W] [--legs events,events_list,compact,cast]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "collision-detect-gjk-epa_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import bench_sweep  # noqa: E402
import events_ref as er  # noqa: E402
import gjkepa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hulls", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tolerance", type=float, default=1e-3)
    ap.add_argument("--vmax", type=float, default=1.0)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--legs", default="events,events_list,compact,cast")
    args = ap.parse_args()
    import torch

    n = args.hulls
    box = (n * 113 / 6) ** (1 / 3)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = gjkepa.load()
    pool = gjkepa.synth_scene(bench_sweep.SEED, n, 32, 32, box)
    bm = bench_sweep.motions(pool, args.vmax)
    v, off, cnt = (torch.from_numpy(x).to(dev) for x in (pool.verts, pool.hull_off, pool.hull_cnt))
    mot = torch.from_numpy(bm.reshape(-1)).to(dev)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    z = lambda count, dt: torch.zeros(count, dtype=dt, device=dev)
    p = lambda t: t.data_ptr()

    # the list and its records, once
    cap = 4 * n
    pairs, npair = z((cap, 2), torch.int32), z(1, torch.int64)
    ws = z(gjkepa.broadphase_swept_workspace_bytes(n, cap), torch.uint8)
    gjkepa.broadphase_swept_device(gjkepa.DTYPE_F32, p(v), p(off), p(cnt), n, p(mot), args.tolerance, float("inf"), p(pairs),
                                   cap, p(npair), p(ws), ws.numel(), s)
    m = int(npair.item())
    assert 0 < m <= cap, (m, cap)
    del ws
    contact, cast = z(m * 128, torch.uint8), z(m * 128, torch.uint8)
    ws_batch = z(gjkepa.workspace_bytes_for(m, 0), torch.uint8)
    ws_cast = z(gjkepa.cast_rigid_workspace_bytes(m), torch.uint8)
    gjkepa.gjkepa_batch_device(2, 1.0, gjkepa.DTYPE_F32, gjkepa.PREC_F64, p(v), p(off), p(cnt), p(pairs), m, p(contact),
                               p(ws_batch), ws_batch.numel(), s)

    def run_cast():
        gjkepa.cast_rigid_batch_device(gjkepa.DTYPE_F32, p(v), p(off), p(cnt), p(pairs), m, p(mot), args.tolerance, p(contact),
                                       gjkepa.PREC_F64, p(cast), p(ws_cast), ws_cast.numel(), s)

    run_cast()
    torch.cuda.synchronize(dev)
    events, counts = z(m * 128, torch.uint8), z(6, torch.int64)
    btime, brank = z(n, torch.float64), z(n, torch.int32)
    ws_ev = z(gjkepa.events_workspace_bytes(m, n), torch.uint8)
    hit_idx, hits, nhit = z(m, torch.int32), z(m * 128, torch.uint8), z(1, torch.int64)
    ws_c = z(gjkepa.compact_workspace_bytes(m), torch.uint8)

    def run_events(bodies):
        return lambda: gjkepa.events_device(p(pairs), m, n, p(cast), p(contact), gjkepa.PREC_F64, p(events), m, p(counts),
                                            p(counts) + 8, p(btime) if bodies else 0, p(brank) if bodies else 0, p(ws_ev),
                                            ws_ev.numel(), s)

    def run_compact():
        gjkepa.compact_hits_device(gjkepa.PREC_F64, p(contact), m, p(hit_idx), p(hits), p(nhit), p(ws_c), ws_c.numel(), s)

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

    med = {}

    def report(leg, ms, extra):
        med[leg] = ms[len(ms) // 2]
        print(json.dumps({"metric": f"M pairs/sec (leg {leg})", "leg": leg, "value": round(m / med[leg] / 1e3, 3),
                          "unit": "M pairs/s", "ms_per_step": round(med[leg], 4), "ms_min": round(ms[0], 4),
                          "ms_max": round(ms[-1], 4), "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                          "higher_is_better": True, "hulls": n, "pairs": m, "version": lib.gjkepa_version_string().decode(),
                          **extra}), flush=True)

    legs = args.legs.split(",")
    if args.check:
        run_events(True)()
        torch.cuda.synchronize(dev)
        host = counts.cpu().numpy()
        want = er.reference(pairs[:m].cpu().numpy(), cast.cpu().numpy().view(gjkepa.CAST64), n,
                            contact.cpu().numpy().view(gjkepa.REC64))
        ne = int(host[0])
        same = (ne == want[1] and host[1:].tolist() == want[2].tolist() and
                events.cpu().numpy()[:ne * 128].tobytes() == want[0].tobytes() and
                btime.cpu().numpy().tobytes() == want[3].tobytes() and brank.cpu().numpy().tobytes() == want[4].tobytes())
        print(json.dumps({"leg": "check", "equals_restatement": bool(same), "n_events": ne, "counts": host[1:].tolist()}), flush=True)
    if "events" in legs:
        ms = timed(run_events(True))
        host = counts.cpu().numpy()
        report("events", ms, {"n_events": int(host[0]), "counts": host[1:].tolist(),
                              "bodies_clamped": int((btime < 1.0).sum().item())})
    if "events_list" in legs:
        report("events_list", timed(run_events(False)), {})
    if "compact" in legs:
        report("compact", timed(run_compact), {"hits": int(nhit.item())})
    if "cast" in legs:
        report("cast", timed(run_cast), {"tolerance": args.tolerance})
    if "events" in med and "cast" in med and "compact" in med:
        print(json.dumps({"leg": "summary", "events_ms": round(med["events"], 4), "events_list_ms": round(med.get("events_list", 0.0), 4),
                          "compact_ms": round(med["compact"], 4), "cast_ms": round(med["cast"], 4),
                          "events_share_of_cast": round(med["events"] / med["cast"], 4),
                          "events_over_compact": round(med["events"] / med["compact"], 3)}), flush=True)


if __name__ == "__main__":
    main()
