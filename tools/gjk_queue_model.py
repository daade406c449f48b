#!/usr/bin/env python3
"""Pass model of GJK tier 0's pending loop queue (gjk_kernel, DESIGN.md §4.1 "GJK tier 0's loop queue"),
numpy only: no GPU and no library.  One wave of 16 groups takes the pairs of a fixture in order, 16 to a
main round.  A pair that needs k iterations of the tetrahedron loop leaves it in iteration k; the wave runs
an iteration for as long as any of its groups is in the loop.  A round costs its fixed work plus the
iterations the wave runs, in units of one iteration: a main round's fixed work (load, sphere test, initial
simplex, store) is FIXED_SHARE of today's round, a queued round's (hull reload from L2, decode, finish) is
`--straggler` times today's round.  With DEFER_AT = d the main round stops once at most d groups are still
in the loop and those wait on the queue; a queued round runs when 16 are pending and, with repush, stops
the same way.  Prints the modelled GJK tier 0 time relative to today's for d = 0..8 and, given the measured
ratio, the queued round's fixed cost that explains it.
usage: python tools/gjk_queue_model.py [fixture.npz] [--straggler 0.2,0.25,0.3] [--measured D:REPUSH:RATIO]
fixture: `iters` (loop iterations per pair, uint8; tests/golden/c2_gjk_iters.npz: the first 131,072 pairs of
the bench's C2 batch, counted with a copy of the oracle that also reports the count of a miss)."""
import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG = 16                 # groups per wave
FIXED_SHARE = 0.39      # of today's round outside the loop (profiles/r14/stamps_C2: the loop is 61% of the wave time)


def wave_iterations(need, d, repush):
    """(main rounds, iterations run in them, queued rounds, iterations run in those) for one wave."""
    it_main = it_q = nq = 0
    pend = []                                           # iterations the queued pairs still need
    n = len(need) // NG * NG
    for r in range(0, n, NG):
        k = np.sort(need[r:r + NG])[::-1]               # descending: k[d] is the (d + 1)-th slowest group
        t = int(k[0]) if d == 0 else max(1, int(k[d]))  # first iteration after which at most d groups remain
        t = min(t, int(k[0]))
        it_main += t
        pend += [int(x) - t for x in k if x > t]
        while len(pend) >= NG:
            q, pend = np.sort(pend[:NG])[::-1], pend[NG:]
            u = int(q[0]) if not (repush and d) else min(int(q[0]), max(1, int(q[d])))
            it_q += u
            nq += 1
            pend += [int(x) - u for x in q if x > u]
    return n // NG, it_main, nq, it_q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fixture", nargs="?", default=os.path.join(ROOT, "tests", "golden", "c2_gjk_iters.npz"))
    ap.add_argument("--straggler", default="0.2,0.25,0.3", help="queued round's fixed work, as shares of today's round")
    ap.add_argument("--measured", default="", help="D:REPUSH:RATIO[,..]: measured GJK tier 0 time over the parent's")
    a = ap.parse_args()
    z = np.load(a.fixture)
    need, hit = z["iters"].astype(np.int64), z["hit"].astype(bool)
    mx = need[:len(need) // NG * NG].reshape(-1, NG).max(axis=1).mean()
    print(f"{os.path.basename(a.fixture)}: {len(need)} pairs, {100 * hit.mean():.1f}% hits; loop iterations: hits mean "
          f"{need[hit].mean():.2f}, misses mean {need[~hit].mean():.2f} ({need[~hit].min()}-{need[~hit].max()}), all "
          f"{need.mean():.2f}, mean of the maximum over {NG} consecutive pairs {mx:.2f}")
    fixed = FIXED_SHARE / (1 - FIXED_SHARE) * mx         # in iterations
    today = fixed + mx
    print(f"today's round: {fixed:.2f} fixed + {mx:.2f} iterations = {today:.2f}; lane use in the loop {100 * need.mean() / mx:.0f}%")
    shares = [float(x) for x in a.straggler.split(",")]
    print("DEFER_AT repush  queued pairs  iterations per main / queued round   time over today's at queued-round fixed share "
          + " ".join(f"{s:.2f}" for s in shares))
    rows = {}
    for d in range(0, 9):
        for rp in ((0,) if d == 0 else (0, 1)):
            nm, im, nq, iq = wave_iterations(need, d, rp)
            rows[(d, rp)] = (nm, im, nq, iq)
            rel = [(nm * fixed + im + nq * s * today + iq) / (nm * today) for s in shares]
            print(f"{d:8d} {rp:6d} {100 * nq * NG / (nm * NG):12.1f}% {im / nm:12.2f} / {iq / max(nq, 1):<12.2f}"
                  + " " * 46 + " ".join(f"{x:.3f}" for x in rel))
    for m in filter(None, a.measured.split(",")):
        d, rp, ratio = m.split(":")
        nm, im, nq, iq = rows[(int(d), int(rp))]
        s = (float(ratio) * nm * today - nm * fixed - im - iq) / (nq * today)
        print(f"measured {ratio} at DEFER_AT {d}, repush {rp}: explained by a queued round whose fixed work is "
              f"{s:.2f} of today's round ({s * today:.1f} iterations' worth)")


if __name__ == "__main__":
    main()
