#!/usr/bin/env python3
"""Pass model of the refill EPA tiers (epa_kernel_refill, DESIGN.md §4.2 "Refill"), numpy only: no GPU and
no library.  One wave of NG groups takes the pairs of a fixture in order; at the top of a pass the idle
groups are refilled once at least REFILL of them are idle (or all are); every pass costs the same.  A pair
of k EPA iterations (the oracle records' diag word) holds its group for k + 1 passes under the old exit
rule (the close of iteration k ran alone in the pass after it) and for k under the shipped one (the close
runs in the pass of its iteration).  Prints group-passes per pair (NG x wave passes / pairs: occupancy plus
the passes a group waits idle for the refill threshold) under both rules.
--refill-cost adds a fixed cost per pass that begins with a refill (the wave waits for the fresh pairs'
loads), in passes, and prints where two REFILL values of one wave shape cross over.
usage: python tools/refill_model.py [fixture.npz] [--tile 16] [--seed 0] [--cases 4/2,4/1,2/1] [--refill-cost 0,0.1,0.2]"""
import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wave_passes(life, ng, refill, events=False):
    """Passes one wave of `ng` groups needs for pairs that hold a group for life[i] passes each (events: and
    the number of passes that began with a refill, each of which stalls the whole wave once)."""
    left = np.zeros(ng, np.int64)                           # passes the group's pair still needs
    nxt, n, passes, refills = 0, len(life), 0, 0
    while True:
        idle = left == 0
        if nxt < n and (idle.sum() >= refill or idle.all()):
            refills += 1
            for g in np.nonzero(idle)[0]:
                if nxt < n:
                    left[g] = life[nxt]
                    nxt += 1
        if not left.any():
            return (passes, refills) if events else passes
        passes += 1
        left[left > 0] -= 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fixture", nargs="?", default=os.path.join(ROOT, "tests", "golden", "c2_32v.npz"))
    ap.add_argument("--tile", type=int, default=16, help="repeat the fixture's pairs this many times")
    ap.add_argument("--seed", type=int, default=0, help="shuffle seed")
    ap.add_argument("--cases", default="4/2,4/1,2/1", help="groups per wave / REFILL, comma list")
    ap.add_argument("--refill-cost", default="", help="fixed cost of a refill in passes, comma list (e.g. 0,0.1,0.2,0.4)")
    a = ap.parse_args()
    rec = np.load(a.fixture)["rec_v2"]                      # REC64 bytes: collision at 104, diag word at 108
    hit = rec[:, 104] != 0
    iters = ((rec[:, 108:112].copy().view("<u4")[:, 0] >> 8) & 0xFF)[hit].astype(np.int64)
    iters = iters[iters > 0]                                # pairs that ran EPA
    print(f"{os.path.basename(a.fixture)}: {len(iters)} EPA pairs, mean {iters.mean():.2f} iterations, max {iters.max()}; "
          f"tiled {a.tile}x, shuffled (seed {a.seed})")
    life = np.random.default_rng(a.seed).permutation(np.tile(iters, a.tile))
    print("groups/REFILL  group-passes per pair: close in the next pass | in the iteration's pass   wave passes")
    for case in a.cases.split(","):
        ng, refill = (int(x) for x in case.split("/"))
        old, new = wave_passes(life + 1, ng, refill), wave_passes(life, ng, refill)
        print(f"{ng} / {refill}          {ng * old / len(life):26.2f} | {ng * new / len(life):<26.2f} {100.0 * (new - old) / old:+.1f}%")
    if a.refill_cost:
        # a refill stalls the whole wave for the fresh pairs' loads: c passes' worth per pass that begins with one
        costs = [float(x) for x in a.refill_cost.split(",")]
        print("fixed cost per refill (passes) -> group-passes per pair, shipped exit rule; refills per pair")
        print("groups/REFILL  refills/pair  " + "  ".join(f"c={c:<5g}" for c in costs))
        rows = {}
        for case in a.cases.split(","):
            ng, refill = (int(x) for x in case.split("/"))
            p, r = wave_passes(life, ng, refill, events=True)
            rows[ng, refill] = (p, r)
            print(f"{ng} / {refill}          {r / len(life):12.3f}  " + "  ".join(f"{ng * (p + c * r) / len(life):7.2f}" for c in costs))
        for ng in sorted({k[0] for k in rows}):
            rs = sorted(k[1] for k in rows if k[0] == ng)
            for lo, hi in zip(rs, rs[1:]):                  # REFILL lo refills more often and idles less than hi
                (pl, rl), (ph, rh) = rows[ng, lo], rows[ng, hi]
                if rl > rh and ph > pl:
                    print(f"{ng} groups: REFILL {lo} and {hi} cross over at {(ph - pl) / (rl - rh):.3f} passes per refill "
                          f"(REFILL {lo} is ahead below it)")


if __name__ == "__main__":
    main()
