"""Shared helpers of the event pass's tests (tests/test_events_host.py on the CPU, tests/test_events.py on the
GPU): the definition of include/gjkepa.h (gjkepa_events_device) restated in numpy from the header's text --
which kind of event a cast record stands for, its time, its 128-byte record, the (time, pair) order, the counts
and the per-body clamp -- and builders of synthetic cast and contact records whose every field is distinct."""
import numpy as np

import gjkepa

HIT, START, IMPACT, UNDECIDED = 1, 2, 3, 4
NONE, BAD = 0, -1
F_IMPACT, F_START, F_SKIPPED = gjkepa.CAST_IMPACT, gjkepa.CAST_START, gjkepa.CAST_SKIPPED
S_OK, S_BAD, S_MAXITER = gjkepa.STATUS_OK, gjkepa.STATUS_BAD_INPUT, gjkepa.STATUS_CAST_MAXITER


def kinds(cast):
    """kind per cast record: the first rule that applies wins"""
    status, flags = cast["status"].astype(np.int64), cast["flags"].astype(np.int64)
    kind = np.full(len(cast), NONE, np.int64)
    kind[(flags & F_IMPACT) != 0] = IMPACT
    kind[(flags & F_START) != 0] = START
    kind[status == S_MAXITER] = UNDECIDED
    kind[(flags & F_SKIPPED) != 0] = HIT
    kind[status == S_BAD] = BAD
    return kind


def times(kind, toi):
    """0 for HIT / START; toi for IMPACT / UNDECIDED when toi > 0, else +0.0 (NaN gives 0)"""
    with np.errstate(invalid="ignore"):
        t = np.where(toi > 0.0, toi, 0.0)
    return np.where((kind == IMPACT) | (kind == UNDECIDED), t, 0.0)


def fill(pairs, cast, records=None):
    """(kind per pair, one EVENT64 record per pair in pair order; the records of pairs without an event are
    zero)"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    kind = kinds(cast)
    ev = np.zeros(len(cast), gjkepa.EVENT64)
    on = kind > 0
    ev["time"] = np.where(on, times(kind, cast["toi"]), 0.0)
    ev["a"], ev["b"] = pairs[:, 0], pairs[:, 1]
    ev["pair"] = np.arange(len(cast))
    ev["kind"] = kind
    ev["status"] = cast["status"]
    for f in ("point_a", "point_b", "normal"):
        ev[f] = cast[f]
    hit = kind == HIT
    ev["point_a"][hit] = ev["point_b"][hit] = ev["normal"][hit] = 0.0
    ev["status"][hit] = 0
    if records is not None:
        ev["point_a"][hit] = records["nearest_points"][hit, 0:3].astype(np.float64)
        ev["point_b"][hit] = records["nearest_points"][hit, 3:6].astype(np.float64)
        ev["normal"][hit] = records["collision_normal"][hit].astype(np.float64)
        ev["depth"][hit] = records["penetration_depth"][hit].astype(np.float64)
        ev["status"][hit] = records["status"][hit]
    ev[~on] = np.zeros(1, gjkepa.EVENT64)
    return kind, ev


def reference(pairs, cast, n_hulls, records=None):
    """(events in (time, pair) order, n_events, counts [5], body_time [n_hulls], body_event [n_hulls])"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    kind, ev = fill(pairs, cast, records)
    idx = np.nonzero(kind > 0)[0]
    bits = ev["time"][idx].view(np.uint64)
    order = idx[np.lexsort((idx, bits))]                   # by the time's bits, ties by pair index
    events = ev[order]
    counts = np.array([(kind == k).sum() for k in (HIT, START, IMPACT, UNDECIDED, BAD)], np.int64)
    body_time, body_event = np.ones(n_hulls), np.full(n_hulls, -1, np.int32)
    for rank in range(len(events) - 1, -1, -1):            # backwards: the smallest rank is written last
        e = events[rank]
        if e["kind"] in (IMPACT, UNDECIDED):
            for h in (int(e["a"]), int(e["b"])):
                body_time[h], body_event[h] = e["time"], rank
    return events, len(events), counts, body_time, body_event


def synth_cast(rng, kind_of_pair, toi=None):
    """CAST64 records of the given kinds (MISS for NONE) with every field distinct: witness fields, lambda and
    code random, toi U(0, 1) for IMPACT / UNDECIDED unless given, 1 for a MISS, 0 otherwise.  Plain records: the
    flag / status a cast writes for that outcome."""
    kind_of_pair = np.asarray(kind_of_pair)
    n = len(kind_of_pair)
    c = np.zeros(n, gjkepa.CAST64)
    for f in ("point_a", "point_b", "normal", "lambda"):
        c[f] = rng.normal(size=(n, 3))
    c["code"] = rng.integers(0, 1 << 32, size=(n, 3), dtype=np.uint64).astype(np.uint32)
    c["n_simplex"] = rng.integers(0, 4, size=n)
    c["iters"] = rng.integers(0, 1000, size=n)
    c["steps"] = rng.integers(0, 65, size=n)
    clamp = (kind_of_pair == IMPACT) | (kind_of_pair == UNDECIDED)
    c["toi"] = np.where(clamp, rng.uniform(1e-6, 1.0, size=n), np.where(kind_of_pair == NONE, 1.0, 0.0))
    if toi is not None:
        c["toi"] = toi
    c["flags"] = np.select([kind_of_pair == HIT, kind_of_pair == START, kind_of_pair == IMPACT], [F_SKIPPED, F_START, F_IMPACT], 0)
    c["status"] = np.select([kind_of_pair == UNDECIDED, kind_of_pair == BAD], [S_MAXITER, S_BAD], S_OK)
    return c


def synth_contacts(rng, n, precision=gjkepa.PREC_F64):
    """contact records with every geometry field distinct and a status in 0 .. 3"""
    r = np.zeros(n, gjkepa.record_dtype(precision))
    r["penetration_depth"] = rng.uniform(0.0, 1.0, size=n)
    r["collision_normal"] = rng.normal(size=(n, 3))
    r["collision_point"] = rng.normal(size=(n, 3))
    r["nearest_points"] = rng.normal(size=(n, 6))
    r["collision"] = rng.integers(0, 2, size=n)
    r["colli_type"] = rng.integers(0, 3, size=n)
    r["status"] = rng.integers(0, 4, size=n)
    r["diag"] = rng.integers(0, 1 << 24, size=n)
    return r


PIPELINE_SEED, PIPELINE_HULLS, PIPELINE_BOX, PIPELINE_TAU, PIPELINE_LONG = 3, 2000, 16.0, 1e-3, 4.0


def pipeline_scene(seed=PIPELINE_SEED, n_hulls=PIPELINE_HULLS, box=PIPELINE_BOX):
    """(pool, body motions, resting mask): hulls of 8 .. 32 vertices in a box, seeded motions (v up to 2, |w| up
    to 1, pivots at the vertex means), every fourth body at rest (v = w = 0), and three bullets crossing the box"""
    import sweep_ref as sr
    pool, bm = sr.scene(seed, n_hulls, 8, 32, box, 2.0)
    bm = bm.copy()
    rest = np.arange(n_hulls) % 4 == 0
    bm[rest, 0:6] = 0.0
    bm[1, 0:3] = [5.0 * box, 0.0, 0.0]
    bm[2, 0:3] = [-2.0 * box, 4.0 * box, 2.5 * box]
    bm[3, 0:3] = [0.0, -3.0 * box, 3.0 * box]
    return pool, bm, rest


# every kind, every precedence clash and the special values of toi: (status, flags, toi)
DENORMAL = 5e-324
EDGE_RECORDS = [
    (S_OK, 0, 1.0),                                  # MISS
    (S_OK, F_IMPACT, 0.25),
    (S_OK, F_START, 0.0),
    (S_OK, F_SKIPPED, 0.0),
    (S_MAXITER, 0, 0.5),
    (S_BAD, 0, 0.0),
    (S_BAD, F_SKIPPED, 0.0),                         # BAD_INPUT wins over SKIPPED
    (S_BAD, F_IMPACT | F_START | F_SKIPPED, 0.3),
    (S_MAXITER, F_SKIPPED, 0.4),                     # SKIPPED wins over MAXITER: time 0
    (S_MAXITER, F_START, 0.6),                       # MAXITER wins over START: time toi
    (S_MAXITER, F_IMPACT, 0.7),
    (S_OK, F_START | F_IMPACT, 0.8),                 # START wins over IMPACT: time 0
    (S_OK, F_SKIPPED | F_START | F_IMPACT, 0.9),
    (S_OK, F_IMPACT, -0.0),
    (S_OK, F_IMPACT, 0.0),
    (S_OK, F_IMPACT, DENORMAL),
    (S_OK, F_IMPACT, float("nan")),
    (S_OK, F_IMPACT, -1.0),
    (S_OK, F_IMPACT, float("inf")),
    (S_MAXITER, 0, -0.0),
    (S_MAXITER, 0, float("nan")),
    (S_MAXITER, 0, DENORMAL),
    (S_OK, F_START, 0.75),                           # a START's toi is not its time
    (S_OK, F_SKIPPED, float("nan")),
    (3, 8, 0.5),                                     # an unknown status and flag: a MISS
]
EDGE_KINDS = [NONE, IMPACT, START, HIT, UNDECIDED, BAD, BAD, BAD, HIT, UNDECIDED, UNDECIDED, START, HIT, IMPACT, IMPACT,
              IMPACT, IMPACT, IMPACT, IMPACT, UNDECIDED, UNDECIDED, UNDECIDED, START, HIT, NONE]


def edge_records(rng):
    """(pairs, cast records) of EDGE_RECORDS"""
    n = len(EDGE_RECORDS)
    c = synth_cast(rng, np.full(n, NONE))
    c["status"] = [e[0] for e in EDGE_RECORDS]
    c["flags"] = [e[1] for e in EDGE_RECORDS]
    c["toi"] = [e[2] for e in EDGE_RECORDS]
    pairs = np.stack([rng.permutation(n), rng.permutation(n) + n], 1).astype(np.int32)
    return pairs, c
