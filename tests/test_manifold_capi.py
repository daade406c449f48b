"""CPU tests of the contact-manifold entries of the C-ABI (include/gjkepa.h gjkepa_manifold_*): the
record layout, the flag values, the workspace size, and the argument contract of both entries as
tests/test_capi_contract.py states it for the others: the return code and the exact gjkepa_last_error()
text of each call, doubly-bad calls pinning the order of the checks.  Everything here is answered
before any device work."""
import os

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

VERTS = np.zeros(48)
OFF = np.array([0, 12, 24, 36], np.int64)
CNT = np.array([4, 4, 4, 4], np.int32)
PAIRS = np.array([0, 1, 2, 3], np.int32)
BAD_PAIRS = np.array([0, 1, 2, 4], np.int32)            # hull 4 does not exist
OFF_PAST = np.array([0, 12, 24, 37], np.int64)          # hull 3 ends one scalar past the pool
CNT_300 = np.array([4, 4, 4, 300], np.int32)
CNT_0 = np.array([4, 4, 4, 0], np.int32)                # an empty hull is never read: any offset passes
OFF_WILD = np.array([0, 12, 24, 1 << 40], np.int64)
RECS = np.zeros(2, gjkepa.REC64)


def test_record_size_and_layout(lib):
    m = gjkepa.MANIFOLD64
    assert lib.gjkepa_manifold_record_bytes() == 160 == m.itemsize
    want = {"depth": 0, "normal": 8, "point": 32, "code": 128, "n_feat_a": 144, "n_feat_b": 146, "n_points": 148,
            "status": 149, "flags": 150, "reserved": 151, "area": 152}
    assert {k: m.fields[k][1] for k in m.names} == want
    assert m["point"].shape == (4, 3) and m["code"].shape == (4,) and m["normal"].shape == (3,)
    assert m["n_feat_a"].base == np.dtype("<u2") and m["code"].base == np.dtype("<u4")


def test_flag_values():
    assert (gjkepa.MANIFOLD_NO_HIT, gjkepa.MANIFOLD_DECIMATED, gjkepa.MANIFOLD_FALLBACK) == (1, 2, 4)
    assert gjkepa.MANIFOLD_MAX_FEATURE == 32
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gjkepa.h")).read()
    for name, value in (("NO_HIT", 1), ("DECIMATED", 2), ("FALLBACK", 4), ("MAX_FEATURE", 32)):
        line = [ln for ln in hdr.splitlines() if ln.startswith(f"#define GJKEPA_MANIFOLD_{name}")][0]
        assert int(line.split()[2]) == value, line


def test_workspace_bytes(lib):
    sizes = [gjkepa.manifold_workspace_bytes(n) for n in (0, 1, 64, 1000, 1 << 20)]
    assert all(b > 0 and b % 256 == 0 for b in sizes) and sizes == sorted(sizes)
    assert lib.gjkepa_manifold_workspace_bytes(-1) < 0
    with pytest.raises(gjkepa.GjkEpaError):
        gjkepa.manifold_workspace_bytes(-5)


def test_exports_are_bound(lib):
    for f in ("gjkepa_manifold_record_bytes", "gjkepa_manifold_workspace_bytes", "gjkepa_manifold_batch_device",
              "gjkepa_manifold_batch"):
        assert f in gjkepa.EXPORTS
        assert getattr(lib, f).restype is not None
    assert callable(gjkepa.manifold_batch) and callable(gjkepa.manifold_batch_device)


def call(entry, order, defaults, **kw):
    a = dict(defaults, **kw)
    assert not set(kw) - set(defaults)
    return entry, [a[k] for k in order]


def host(**kw):
    return call("gjkepa_manifold_batch", "vd verts nvs off cnt nh pairs n rec rprec margin out device".split(),
                dict(vd=F64, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, pairs=PAIRS, n=2, rec=RECS, rprec=1, margin=1e-6,
                     out=P, device=-1), **kw)


def dev(**kw):
    return call("gjkepa_manifold_batch_device", "vd verts off cnt pairs n rec rprec margin out ws wsb stream".split(),
                dict(vd=F64, verts=P, off=P, cnt=P, pairs=P, n=2, rec=P, rprec=1, margin=1e-6, out=P, ws=P, wsb=256,
                     stream=None), **kw)


def nulls(make, names, **kw):
    return [(make(**{k: None}, **kw), E_ARG, NULL) for k in names]


POOL_PTRS = ("verts", "off", "cnt", "pairs")
ROWS = [
    # ---- gjkepa_manifold_batch: sizes -> dtype / n_pairs / records_precision -> margin -> n_pairs > 2^31-1 ->
    #      n_pairs == 0 -> null (records among them) -> pool check
    (host(nh=-1), E_ARG, "bad sizes"), (host(nvs=-1), E_ARG, "bad sizes"),
    (host(nh=-1, vd=7), E_ARG, "bad sizes"), (host(nvs=-1, margin=NAN), E_ARG, "bad sizes"),
    (host(n=-1), E_ARG, NDT), (host(vd=7), E_ARG, NDT), (host(vd=-1), E_ARG, NDT),
    (host(vd=7, verts=None), E_ARG, NDT),                                  # bad dtype + null pointer
    (host(vd=7, rprec=9), E_ARG, NDT),                                     # bad dtype + bad records_precision
    (host(rprec=9), E_ARG, RPREC), (host(rprec=-1), E_ARG, RPREC),
    (host(rprec=9, rec=None), E_ARG, RPREC),                               # the records are required: judged without them too
    (host(rprec=9, margin=NAN), E_ARG, RPREC),                             # bad records_precision + bad margin
    (host(margin=NAN), E_ARG, MARGIN), (host(margin=INF), E_ARG, MARGIN), (host(margin=-INF), E_ARG, MARGIN),
    (host(margin=-1e-300), E_ARG, MARGIN),
    (host(margin=NAN, n=OVER), E_ARG, MARGIN),                             # bad margin + n_pairs > INT32_MAX
    (host(margin=-1.0, n=0), E_ARG, MARGIN),                               # bad margin + empty batch
    (host(n=OVER), E_ARG, TOO_MANY), (host(n=OVER, verts=None), E_ARG, TOO_MANY),
    (host(n=0, verts=None, off=None, cnt=None, pairs=None, rec=None, out=None), 0, None),
    *nulls(host, POOL_PTRS + ("rec", "out")),
    (host(rec=None, pairs=BAD_PAIRS), E_ARG, NULL),                        # null before the pool check
    (host(pairs=BAD_PAIRS), E_ARG, MISSING), (host(pairs=BAD_PAIRS, off=OFF_PAST), E_ARG, MISSING),
    (host(off=OFF_PAST), E_ARG, OUTSIDE), (host(nvs=47), E_ARG, OUTSIDE), (host(cnt=CNT_300), E_ARG, OUTSIDE),
    (host(cnt=CNT_0, off=OFF_WILD), PAST_CHECKS, None),
    (host(), PAST_CHECKS, None), (host(margin=0.0, vd=F32, rprec=0), PAST_CHECKS, None),
    # ---- gjkepa_manifold_batch_device: the same order without the sizes and the pool check, then the workspace
    (dev(n=-1), E_ARG, NDT), (dev(vd=7, verts=None), E_ARG, NDT), (dev(vd=7, rprec=9), E_ARG, NDT),
    (dev(rprec=9), E_ARG, RPREC), (dev(rprec=9, rec=None), E_ARG, RPREC), (dev(rprec=9, margin=-1.0), E_ARG, RPREC),
    (dev(margin=NAN), E_ARG, MARGIN), (dev(margin=INF), E_ARG, MARGIN), (dev(margin=-1e-9), E_ARG, MARGIN),
    (dev(margin=NAN, n=OVER), E_ARG, MARGIN), (dev(margin=NAN, n=0), E_ARG, MARGIN),
    (dev(n=OVER), E_ARG, TOO_MANY), (dev(n=OVER, rec=None), E_ARG, TOO_MANY),
    (dev(n=0, verts=None, off=None, cnt=None, pairs=None, rec=None, out=None, ws=None, wsb=0), 0, None),
    *nulls(dev, POOL_PTRS + ("rec", "out", "ws")),
    (dev(ws=None, wsb=0), E_ARG, NULL), (dev(rec=None, wsb=0), E_ARG, NULL),       # null before the workspace
    (dev(wsb=255), E_WORKSPACE, WS), (dev(wsb=0), E_WORKSPACE, WS), (dev(wsb=-1), E_WORKSPACE, WS),
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
    assert lib.gjkepa_manifold_batch_device(0, None, None, None, None, 0, None, 1, 0.0, None, None, 0, None) == 0
    assert lib.gjkepa_manifold_batch(1, None, 0, None, None, 0, None, 0, None, 0, 1e-6, None, 0) == 0
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0)
    empty = gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, np.zeros((0, 2), np.int32))
    out = gjkepa.manifold_batch(empty, np.zeros(0, gjkepa.REC64), 1e-6)
    assert len(out) == 0 and out.dtype == gjkepa.MANIFOLD64


def test_python_wrapper_argument_checks(lib):
    pool = gjkepa.synth_pairs(1, 4, 8, 8, 1.0, dtype=np.float64)
    recs = np.zeros(4, gjkepa.REC64)
    with pytest.raises(gjkepa.GjkEpaError, match="records"):
        gjkepa.manifold_batch(pool, None, 1e-6)
    with pytest.raises(gjkepa.GjkEpaError, match="records"):
        gjkepa.manifold_batch(pool, np.zeros(3, gjkepa.REC64), 1e-6)
    for margin in (-0.5, INF, NAN):
        with pytest.raises(gjkepa.GjkEpaError, match="margin"):
            gjkepa.manifold_batch(pool, recs, margin)
    bad = pool.pairs.copy()
    bad[0, 0] = 99
    with pytest.raises(gjkepa.GjkEpaError, match="missing hull"):
        gjkepa.manifold_batch(gjkepa.HullPool(pool.verts, pool.hull_off, pool.hull_cnt, bad), recs, 1e-6)
