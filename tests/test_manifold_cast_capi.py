"""CPU tests of the C-ABI entries of the contact manifold at the time of impact (include/gjkepa.h
gjkepa_manifold_cast_*, gjkepa_event_manifolds_device, gjkepa_collide_moving_patches): the flag value, the
workspace size, and the argument contract of the four entries as tests/test_manifold_capi.py states it for
the contact manifold's: the return code and the exact gjkepa_last_error() text of each call, doubly-bad calls
pinning the order of the checks.  Everything here is answered before any device work."""
import os
import re

import numpy as np
import pytest

import gjkepa

E_ARG, E_NODEVICE, E_WORKSPACE = -1, -3, -4
F32, F64 = gjkepa.DTYPE_F32, gjkepa.DTYPE_F64
P = 0x1000                      # a pointer no row dereferences
OVER = (1 << 31)                # n_pairs above INT32_MAX
NAN, INF = float("nan"), float("inf")
PAST_CHECKS = {(E_ARG, "device index out of range"), (E_NODEVICE, "no HIP device")}

NULL = "null pointer"
MISSING = "pair references a missing hull"
OUTSIDE = "hull outside the vertex pool"
TOO_MANY = "n_pairs above 2^31-1"
MARGIN = "margin is NaN, infinite or negative"
NDT = "bad n_pairs/dtype"
RPREC = "bad records_precision"
WS = "workspace too small"
SDP = "bad sizes/dtype/precision"

VERTS = np.zeros(48)
OFF = np.array([0, 12, 24, 36], np.int64)
CNT = np.array([4, 4, 4, 4], np.int32)
PAIRS = np.array([0, 1, 2, 3], np.int32)
BAD_PAIRS = np.array([0, 1, 2, 4], np.int32)            # hull 4 does not exist
OFF_PAST = np.array([0, 12, 24, 37], np.int64)          # hull 3 ends one scalar past the pool
RECS = np.zeros(2, gjkepa.REC64)
CAST = np.zeros(2, gjkepa.CAST64)
MOTION = np.zeros(36)
NEV = np.zeros(1, np.int64)
EVENTS = np.zeros(4, gjkepa.EVENT64)
PATCHES = np.zeros(4, gjkepa.MANIFOLD64)
NEW = ("gjkepa_manifold_cast_workspace_bytes", "gjkepa_manifold_cast_batch_device", "gjkepa_manifold_cast_batch",
       "gjkepa_event_manifolds_device", "gjkepa_collide_moving_patches")


def test_flag_value_and_header_declarations(lib):
    assert gjkepa.MANIFOLD_AT_TOI == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gjkepa.h")).read()
    line = [ln for ln in hdr.splitlines() if ln.startswith("#define GJKEPA_MANIFOLD_AT_TOI")][0]
    assert int(line.split()[2]) == 8, line
    for f in NEW:
        assert f in gjkepa.EXPORTS
        assert len(re.findall(r"^int(?:64_t)? " + f + r"\(", hdr, re.M)) == 1, f
        assert getattr(lib, f).restype is not None
    for f in ("manifold_cast_workspace_bytes", "manifold_cast_batch", "manifold_cast_batch_device", "event_manifolds_device",
              "collide_moving_patches"):
        assert callable(getattr(gjkepa, f))


def test_workspace_bytes(lib):
    for n in (0, 1, 64, 1000, 1 << 20):
        assert gjkepa.manifold_cast_workspace_bytes(n) == gjkepa.manifold_workspace_bytes(n)
    assert lib.gjkepa_manifold_cast_workspace_bytes(-1) < 0
    with pytest.raises(gjkepa.GjkEpaError):
        gjkepa.manifold_cast_workspace_bytes(-5)


def call(entry, order, defaults, **kw):
    a = dict(defaults, **kw)
    assert not set(kw) - set(defaults)
    return entry, [a[k] for k in order]


def host(**kw):
    return call("gjkepa_manifold_cast_batch",
                "vd verts nvs off cnt nh pairs n motion cast rec rprec margin out device".split(),
                dict(vd=F64, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, pairs=PAIRS, n=2, motion=MOTION, cast=CAST, rec=RECS,
                     rprec=1, margin=1e-6, out=P, device=-1), **kw)


def dev(**kw):
    return call("gjkepa_manifold_cast_batch_device",
                "vd verts off cnt pairs n motion cast rec rprec margin out ws wsb stream".split(),
                dict(vd=F64, verts=P, off=P, cnt=P, pairs=P, n=2, motion=P, cast=P, rec=P, rprec=1, margin=1e-6, out=P, ws=P,
                     wsb=256, stream=None), **kw)


def gather(**kw):
    return call("gjkepa_event_manifolds_device", "events nev maxev manifolds out stream".split(),
                dict(events=P, nev=P, maxev=4, manifolds=P, out=P, stream=None), **kw)


def step(**kw):
    return call("gjkepa_collide_moving_patches",
                "version tol vd prec verts nvs off cnt nh motion tau radius events maxev nev counts ncand btime vout margin "
                "patches device".split(),
                dict(version=2, tol=1.0, vd=F64, prec=1, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, motion=MOTION, tau=1e-3,
                     radius=INF, events=EVENTS, maxev=4, nev=NEV, counts=None, ncand=None, btime=None, vout=None, margin=1e-6,
                     patches=PATCHES, device=-1), **kw)


def nulls(make, names, **kw):
    return [(make(**{k: None}, **kw), E_ARG, NULL) for k in names]


POOL_PTRS = ("verts", "off", "cnt", "pairs")
ROWS = [
    # ---- gjkepa_manifold_cast_batch: sizes -> dtype / n_pairs -> records_precision with records -> margin ->
    #      n_pairs > 2^31-1 -> n_pairs == 0 -> null (body_motion and the cast records among them) -> pool check
    (host(nh=-1), E_ARG, "bad sizes"), (host(nvs=-1), E_ARG, "bad sizes"), (host(nvs=-1, margin=NAN), E_ARG, "bad sizes"),
    (host(n=-1), E_ARG, NDT), (host(vd=7), E_ARG, NDT), (host(vd=-1), E_ARG, NDT),
    (host(vd=7, verts=None), E_ARG, NDT), (host(vd=7, rprec=9), E_ARG, NDT),
    (host(rprec=9), E_ARG, RPREC), (host(rprec=-1), E_ARG, RPREC),
    (host(rprec=9, margin=NAN), E_ARG, RPREC),
    (host(rprec=9, rec=None), PAST_CHECKS, None),                          # the records are optional: not judged without them
    (host(margin=NAN), E_ARG, MARGIN), (host(margin=INF), E_ARG, MARGIN), (host(margin=-INF), E_ARG, MARGIN),
    (host(margin=-1e-300), E_ARG, MARGIN), (host(margin=NAN, n=OVER), E_ARG, MARGIN), (host(margin=-1.0, n=0), E_ARG, MARGIN),
    (host(n=OVER), E_ARG, TOO_MANY), (host(n=OVER, cast=None), E_ARG, TOO_MANY),
    (host(n=0, verts=None, off=None, cnt=None, pairs=None, motion=None, cast=None, rec=None, out=None), 0, None),
    *nulls(host, POOL_PTRS + ("motion", "cast", "out")),
    (host(cast=None, pairs=BAD_PAIRS), E_ARG, NULL), (host(motion=None, off=OFF_PAST), E_ARG, NULL),
    (host(pairs=BAD_PAIRS), E_ARG, MISSING), (host(off=OFF_PAST), E_ARG, OUTSIDE), (host(nvs=47), E_ARG, OUTSIDE),
    (host(), PAST_CHECKS, None), (host(rec=None), PAST_CHECKS, None), (host(margin=0.0, vd=F32, rprec=0), PAST_CHECKS, None),
    # ---- gjkepa_manifold_cast_batch_device: the same order without the sizes and the pool check, then the workspace
    (dev(n=-1), E_ARG, NDT), (dev(vd=7, verts=None), E_ARG, NDT), (dev(vd=7, rprec=9), E_ARG, NDT),
    (dev(rprec=9), E_ARG, RPREC), (dev(rprec=9, margin=-1.0), E_ARG, RPREC),
    (dev(rprec=9, rec=None, wsb=0), E_WORKSPACE, WS),                      # not judged without records
    (dev(margin=NAN), E_ARG, MARGIN), (dev(margin=INF), E_ARG, MARGIN), (dev(margin=-1e-9), E_ARG, MARGIN),
    (dev(margin=NAN, n=OVER), E_ARG, MARGIN), (dev(margin=NAN, n=0), E_ARG, MARGIN),
    (dev(n=OVER), E_ARG, TOO_MANY), (dev(n=OVER, cast=None), E_ARG, TOO_MANY),
    (dev(n=0, verts=None, off=None, cnt=None, pairs=None, motion=None, cast=None, rec=None, out=None, ws=None, wsb=0), 0, None),
    *nulls(dev, POOL_PTRS + ("motion", "cast", "out", "ws")),
    (dev(ws=None, wsb=0), E_ARG, NULL), (dev(cast=None, wsb=0), E_ARG, NULL), (dev(motion=None, wsb=0), E_ARG, NULL),
    (dev(wsb=255), E_WORKSPACE, WS), (dev(wsb=0), E_WORKSPACE, WS), (dev(wsb=-1), E_WORKSPACE, WS),
    (dev(rec=None, wsb=255), E_WORKSPACE, WS),
    # ---- gjkepa_event_manifolds_device: max_events -> null -> max_events == 0
    (gather(maxev=-1), E_ARG, "bad max_events"), (gather(maxev=-1, nev=None), E_ARG, "bad max_events"),
    (gather(maxev=OVER), E_ARG, "bad max_events"),
    *nulls(gather, ("events", "nev", "manifolds", "out")),
    (gather(maxev=0, nev=None), E_ARG, NULL),
    (gather(maxev=0, events=None, manifolds=None, out=None), 0, None),
    # ---- gjkepa_collide_moving_patches: gjkepa_collide_moving's order, the margin after the sweep's scalars, patches
    #      with events
    (step(maxev=-1), E_ARG, SDP), (step(nvs=-1), E_ARG, SDP), (step(vd=7), E_ARG, SDP), (step(prec=9), E_ARG, SDP),
    (step(vd=7, margin=NAN), E_ARG, SDP),
    (step(tau=0.0, margin=NAN), E_ARG, "tolerance is NaN, infinite, zero or negative"),
    (step(margin=NAN), E_ARG, MARGIN), (step(margin=INF), E_ARG, MARGIN), (step(margin=-1e-300), E_ARG, MARGIN),
    (step(margin=NAN, nev=None), E_ARG, MARGIN), (step(margin=-1.0, nh=0), E_ARG, MARGIN),
    *nulls(step, ("nev", "events", "patches")),
    (step(patches=None, nh=0), E_ARG, NULL),
    (step(maxev=0, events=None, patches=None, nh=0), 0, None),
    (step(nh=0, verts=None, off=None, cnt=None, motion=None), 0, None),
    *nulls(step, ("verts", "off", "cnt", "motion")),
    (step(off=OFF_PAST), E_ARG, OUTSIDE),
    (step(), PAST_CHECKS, None), (step(margin=0.0), PAST_CHECKS, None),
]


def row_id(row):
    (entry, args), rc, _ = row
    return entry.replace("gjkepa_", "") + ("-ok" if rc == 0 else "-past" if rc is PAST_CHECKS else "")


@pytest.mark.parametrize("row", ROWS, ids=[f"{i:03d}-{row_id(r)}" for i, r in enumerate(ROWS)])
def test_return_code_and_error_text(lib, row):
    (entry, args), want_rc, want_text = row
    args = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
    rc = getattr(lib, entry)(*args)
    text = lib.gjkepa_last_error().decode()
    if want_rc is PAST_CHECKS:
        assert (rc, text) in PAST_CHECKS
    elif want_rc == 0:
        assert rc == 0
    else:
        assert (rc, text) == (want_rc, want_text)


def test_empty_batch_returns_ok(lib):
    assert lib.gjkepa_manifold_cast_batch_device(0, None, None, None, None, 0, None, None, None, 1, 0.0, None, None, 0, None) == 0
    assert lib.gjkepa_manifold_cast_batch(1, None, 0, None, None, 0, None, 0, None, None, None, 0, 1e-6, None, 0) == 0
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0)
    empty = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, np.zeros((0, 2), np.int32))
    out = gjkepa.manifold_cast_batch(empty, np.zeros((8, 9)), np.zeros(0, gjkepa.CAST64), 1e-6)
    assert len(out) == 0 and out.dtype == gjkepa.MANIFOLD64
    ne = np.zeros(1, np.int64)
    ev, pt = np.zeros(1, gjkepa.EVENT64), np.full(1, 7, np.uint8).repeat(160).view(gjkepa.MANIFOLD64)
    keep = pt.tobytes()
    assert lib.gjkepa_collide_moving_patches(2, 1.0, 1, 1, None, 0, None, None, 0, None, 1e-3, INF, ev.ctypes.data, 1,
                                             ne.ctypes.data, None, None, None, None, 1e-6, pt.ctypes.data, 0) == 0
    assert ne[0] == 0 and pt.tobytes() == keep


def test_python_wrapper_argument_checks(lib):
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0, dtype=np.float64)
    cast, bm = np.zeros(4, gjkepa.CAST64), np.zeros((8, 9))
    with pytest.raises(gjkepa.GjkEpaError, match="cast_records"):
        gjkepa.manifold_cast_batch(pool, bm, np.zeros(3, gjkepa.CAST64), 1e-6)
    with pytest.raises(gjkepa.GjkEpaError, match="cast_records"):
        gjkepa.manifold_cast_batch(pool, bm, np.zeros(4, gjkepa.DIST64), 1e-6)
    with pytest.raises(gjkepa.GjkEpaError, match="body_motion"):
        gjkepa.manifold_cast_batch(pool, np.zeros((7, 9)), cast, 1e-6)
    with pytest.raises(gjkepa.GjkEpaError, match="records"):
        gjkepa.manifold_cast_batch(pool, bm, cast, 1e-6, records=np.zeros(3, gjkepa.REC64))
    for margin in (-0.5, INF, NAN):
        with pytest.raises(gjkepa.GjkEpaError, match="margin"):
            gjkepa.manifold_cast_batch(pool, bm, cast, margin)
        with pytest.raises(gjkepa.GjkEpaError, match="margin"):
            gjkepa.collide_moving_patches(pool, bm, 1e-3, margin)
