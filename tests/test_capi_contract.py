"""The argument contract of the C-ABI entries that take host buffers, and of the device entries that
answer before any device work: for each call of the table, the return code and the exact
gjkepa_last_error() text.  The order of an entry's checks decides which error a doubly-bad call
reports, so the table pins that order row by row (include/gjkepa.h; csrc/gjkepa_capi.cpp check_pool and
the entries' leading checks).

A call that passes every argument check goes on to look up its device.  Such rows ask for device -1 and
expect what the lookup answers: "device index out of range" with a GPU, "no HIP device" without one.
Nothing is ever enqueued."""
import ctypes

import numpy as np
import pytest

import gjkepa

E_ARG, E_NODEVICE, E_WORKSPACE = -1, -3, -4
F32, F64 = gjkepa.DTYPE_F32, gjkepa.DTYPE_F64
P = 0x1000                      # a pointer no row dereferences
OVER = (1 << 31)                # n_pairs above INT32_MAX
NAN, INF = float("nan"), float("inf")
PAST_CHECKS = {(E_ARG, "device index out of range"), (E_NODEVICE, "no HIP device")}

SIZES = "bad sizes/dtype/precision"
NULL = "null pointer"
MISSING = "pair references a missing hull"
OUTSIDE = "hull outside the vertex pool"
TOO_MANY = "n_pairs above 2^31-1"
MAXD = "max_distance is NaN or negative"
TOL = "tolerance is NaN, infinite, zero or negative"
WS = "workspace too small"

# a pool of four 4-vertex hulls and two pairs; the entries read these buffers in their pool check
VERTS = np.zeros(48)
OFF = np.array([0, 12, 24, 36], np.int64)
CNT = np.array([4, 4, 4, 4], np.int32)
PAIRS = np.array([0, 1, 2, 3], np.int32)
BAD_PAIRS = np.array([0, 1, 2, 4], np.int32)            # hull 4 does not exist
NEG_PAIRS = np.array([-1, 1, 2, 3], np.int32)
OFF_PAST = np.array([0, 12, 24, 37], np.int64)          # hull 3 ends one scalar past the pool
OFF_NEG = np.array([0, -3, 24, 36], np.int64)
CNT_300 = np.array([4, 4, 4, 300], np.int32)            # above GJKEPA_MAX_HULL_VERTS, and past the pool
CNT_0 = np.array([4, 4, 4, 0], np.int32)                # an empty hull is never read: any offset passes
OFF_WILD = np.array([0, 12, 24, 1 << 40], np.int64)
MOTION = np.zeros(6)
# two 4-point clouds with a 4-triangle face block each
POINTS = np.zeros(24)
COFF = np.array([0, 12], np.int64)
CCNT = np.array([4, 4], np.int32)
FOFF = np.array([0, 4], np.int64)


def call(entry, order, defaults, **kw):
    a = dict(defaults, **kw)
    unknown = set(kw) - set(defaults)
    assert not unknown, unknown
    return entry, [a[k] for k in order]


def batch(**kw):
    return call("gjkepa_batch", "version tol vd prec verts nvs off cnt nh pairs n out device".split(),
                dict(version=2, tol=1.0, vd=F64, prec=1, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, pairs=PAIRS, n=2, out=P,
                     device=-1), **kw)


def dist(**kw):
    return call("gjkepa_distance_batch", "vd verts nvs off cnt nh pairs n rec rprec maxd out device".split(),
                dict(vd=F64, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, pairs=PAIRS, n=2, rec=None, rprec=1, maxd=INF, out=P,
                     device=-1), **kw)


def cast(**kw):
    return call("gjkepa_cast_batch", "vd verts nvs off cnt nh pairs n motion tol rec rprec out device".split(),
                dict(vd=F64, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, pairs=PAIRS, n=2, motion=MOTION, tol=1e-6, rec=None,
                     rprec=1, out=P, device=-1), **kw)


def hull(**kw):
    return call("gjkepa_hull_batch",
                "vd points nps coff ccnt nc foff nfs faces nf nv st hv vi device".split(),
                dict(vd=F64, points=POINTS, nps=24, coff=COFF, ccnt=CCNT, nc=2, foff=FOFF, nfs=8, faces=P, nf=P, nv=P, st=P,
                     hv=None, vi=None, device=-1), **kw)


def broad(**kw):
    return call("gjkepa_broadphase", "vd verts nvs off cnt nh pairs maxp n device".split(),
                dict(vd=F64, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, pairs=P, maxp=8, n="count", device=-1), **kw)


def collide(**kw):
    return call("gjkepa_collide", "version tol vd prec verts nvs off cnt nh pairs out maxc nc ncand device".split(),
                dict(version=2, tol=1.0, vd=F64, prec=1, verts=VERTS, nvs=48, off=OFF, cnt=CNT, nh=4, pairs=P, out=P, maxc=8,
                     nc="count", ncand="count2", device=-1), **kw)


def batch_dev(**kw):
    return call("gjkepa_batch_device", "version tol vd prec verts off cnt pairs n out ws wsb stream".split(),
                dict(version=2, tol=1.0, vd=F64, prec=1, verts=P, off=P, cnt=P, pairs=P, n=2, out=P, ws=P, wsb=1 << 20,
                     stream=None), **kw)


def warm_dev(**kw):
    return call("gjkepa_batch_warm_device", "version tol vd prec verts off cnt pairs n out ws wsb warm stream".split(),
                dict(version=2, tol=1.0, vd=F64, prec=1, verts=P, off=P, cnt=P, pairs=P, n=2, out=P, ws=P, wsb=1 << 20, warm=P,
                     stream=None), **kw)


def dist_dev(**kw):
    return call("gjkepa_distance_batch_device", "vd verts off cnt pairs n rec rprec maxd out ws wsb stream".split(),
                dict(vd=F64, verts=P, off=P, cnt=P, pairs=P, n=2, rec=None, rprec=1, maxd=INF, out=P, ws=P, wsb=256,
                     stream=None), **kw)


def cast_dev(**kw):
    return call("gjkepa_cast_batch_device", "vd verts off cnt pairs n motion tol rec rprec out ws wsb stream".split(),
                dict(vd=F64, verts=P, off=P, cnt=P, pairs=P, n=2, motion=P, tol=1e-6, rec=None, rprec=1, out=P, ws=P, wsb=256,
                     stream=None), **kw)


def hull_dev(**kw):
    return call("gjkepa_hull_batch_device", "vd points coff ccnt nc foff faces nf nv st hv vi stream".split(),
                dict(vd=F64, points=P, coff=P, ccnt=P, nc=2, foff=P, faces=P, nf=P, nv=P, st=P, hv=None, vi=None, stream=None),
                **kw)


def nulls(make, names, text=NULL, **kw):
    return [(make(**{k: None}, **kw), E_ARG, text) for k in names]


POOL_PTRS = ("verts", "off", "cnt", "pairs")
ROWS = [
    # ---- gjkepa_batch: sizes/enums -> n_pairs == 0 -> null -> n_pairs > INT32_MAX -> pool check
    (batch(n=-1), E_ARG, SIZES), (batch(nh=-1), E_ARG, SIZES), (batch(nvs=-1), E_ARG, SIZES),
    (batch(vd=7), E_ARG, SIZES), (batch(prec=-1), E_ARG, SIZES),
    (batch(vd=7, verts=None), E_ARG, SIZES),                               # bad dtype + null pointer
    (batch(prec=2, n=0), E_ARG, SIZES),
    (batch(n=0, verts=None, off=None, cnt=None, pairs=None, out=None), 0, None),   # n_pairs == 0 + null pointer
    *nulls(batch, POOL_PTRS + ("out",)),
    (batch(n=OVER, out=None), E_ARG, NULL),                                # null before the 2^31 bound
    (batch(n=OVER), E_ARG, TOO_MANY),
    (batch(pairs=BAD_PAIRS), E_ARG, MISSING), (batch(pairs=NEG_PAIRS), E_ARG, MISSING),
    (batch(pairs=BAD_PAIRS, off=OFF_PAST), E_ARG, MISSING),                # bad pair index + hull outside the pool
    (batch(off=OFF_PAST), E_ARG, OUTSIDE), (batch(off=OFF_NEG), E_ARG, OUTSIDE), (batch(nvs=47), E_ARG, OUTSIDE),
    (batch(cnt=CNT_300), E_ARG, OUTSIDE),                                  # every positive count is checked here
    (batch(cnt=CNT_0, off=OFF_WILD), PAST_CHECKS, None),
    (batch(), PAST_CHECKS, None), (batch(vd=F32, prec=0), PAST_CHECKS, None),
    # ---- gjkepa_distance_batch: n_hulls / n_vert_scalars sign -> args_ok -> n_pairs == 0 -> null -> pool check
    (dist(nh=-1), E_ARG, "bad sizes"), (dist(nvs=-1), E_ARG, "bad sizes"),
    (dist(nh=-1, vd=7), E_ARG, "bad sizes"),
    (dist(n=-1), E_ARG, "bad n_pairs/dtype"), (dist(vd=7), E_ARG, "bad n_pairs/dtype"),
    (dist(vd=7, verts=None), E_ARG, "bad n_pairs/dtype"),                  # bad dtype + null pointer
    (dist(vd=7, rec=P, rprec=9), E_ARG, "bad n_pairs/dtype"),
    (dist(rec=P, rprec=9), E_ARG, "bad records_precision"),
    (dist(rec=P, rprec=9, maxd=NAN), E_ARG, "bad records_precision"),
    (dist(rprec=9), PAST_CHECKS, None),                                    # not looked at without records
    (dist(maxd=NAN), E_ARG, MAXD), (dist(maxd=-1e-300), E_ARG, MAXD), (dist(maxd=-INF), E_ARG, MAXD),
    (dist(maxd=NAN, n=OVER), E_ARG, MAXD),
    (dist(n=OVER), E_ARG, TOO_MANY), (dist(n=OVER, verts=None), E_ARG, TOO_MANY),
    (dist(n=0, maxd=NAN), E_ARG, MAXD),
    (dist(n=0, verts=None, off=None, cnt=None, pairs=None, out=None), 0, None),    # n_pairs == 0 + null pointer
    *nulls(dist, POOL_PTRS + ("out",)),
    (dist(out=None, pairs=BAD_PAIRS), E_ARG, NULL),
    (dist(pairs=BAD_PAIRS), E_ARG, MISSING), (dist(pairs=BAD_PAIRS, off=OFF_PAST), E_ARG, MISSING),
    (dist(off=OFF_PAST), E_ARG, OUTSIDE), (dist(off=OFF_NEG), E_ARG, OUTSIDE), (dist(cnt=CNT_300), E_ARG, OUTSIDE),
    (dist(cnt=CNT_0, off=OFF_WILD), PAST_CHECKS, None),
    (dist(), PAST_CHECKS, None), (dist(maxd=0.0, vd=F32), PAST_CHECKS, None),
    # ---- gjkepa_cast_batch: as the distance entry, with the tolerance for max_distance and motion among the pointers
    (cast(nh=-1), E_ARG, "bad sizes"), (cast(nvs=-1, tol=0.0), E_ARG, "bad sizes"),
    (cast(n=-1), E_ARG, "bad n_pairs/dtype"), (cast(vd=-1), E_ARG, "bad n_pairs/dtype"),
    (cast(vd=7, motion=None), E_ARG, "bad n_pairs/dtype"),                 # bad dtype + null pointer
    (cast(rec=P, rprec=9), E_ARG, "bad records_precision"), (cast(rec=P, rprec=9, tol=0.0), E_ARG, "bad records_precision"),
    (cast(rprec=9), PAST_CHECKS, None),
    (cast(tol=0.0), E_ARG, TOL), (cast(tol=-1.0), E_ARG, TOL), (cast(tol=NAN), E_ARG, TOL), (cast(tol=INF), E_ARG, TOL),
    (cast(tol=0.0, n=OVER), E_ARG, TOL),                                   # bad tolerance + n_pairs > INT32_MAX
    (cast(n=OVER), E_ARG, TOO_MANY),
    (cast(n=0, tol=NAN), E_ARG, TOL),
    (cast(n=0, verts=None, off=None, cnt=None, pairs=None, motion=None, out=None), 0, None),
    *nulls(cast, POOL_PTRS + ("motion", "out")),
    (cast(pairs=BAD_PAIRS), E_ARG, MISSING), (cast(pairs=BAD_PAIRS, off=OFF_PAST), E_ARG, MISSING),
    (cast(off=OFF_PAST), E_ARG, OUTSIDE), (cast(cnt=CNT_300), E_ARG, OUTSIDE),
    (cast(cnt=CNT_0, off=OFF_WILD), PAST_CHECKS, None),
    (cast(), PAST_CHECKS, None),
    # ---- gjkepa_hull_batch: sizes/dtype -> n_clouds == 0 -> null -> cloud check
    (hull(nc=-1), E_ARG, "bad sizes/dtype"), (hull(nps=-1), E_ARG, "bad sizes/dtype"), (hull(nfs=-1), E_ARG, "bad sizes/dtype"),
    (hull(vd=7), E_ARG, "bad sizes/dtype"), (hull(vd=7, points=None), E_ARG, "bad sizes/dtype"),
    (hull(nc=0, points=None, coff=None, ccnt=None, foff=None, faces=None, nf=None, nv=None, st=None), 0, None),
    *nulls(hull, ("points", "coff", "ccnt", "foff", "faces", "nf", "nv", "st")),
    (hull(nps=23), E_ARG, "cloud outside the point pool"),
    (hull(coff=np.array([0, -12], np.int64)), E_ARG, "cloud outside the point pool"),
    (hull(nfs=7), E_ARG, "cloud's face block outside the face buffer"),
    (hull(foff=np.array([-1, 4], np.int64)), E_ARG, "cloud's face block outside the face buffer"),
    (hull(nps=23, nfs=7), E_ARG, "cloud outside the point pool"),
    (hull(ccnt=np.array([4, 3], np.int32), nps=12, nfs=4), PAST_CHECKS, None),      # too few / too many points: not read
    (hull(ccnt=np.array([4, 257], np.int32), nps=12, nfs=4), PAST_CHECKS, None),
    (hull(), PAST_CHECKS, None), (hull(hv=P, vi=P), PAST_CHECKS, None),
    # ---- gjkepa_broadphase: sizes -> output nulls -> (outputs zeroed) -> n_hulls == 0 -> input nulls -> pool check
    (broad(nh=-1), E_ARG, "bad sizes/dtype"), (broad(maxp=-1), E_ARG, "bad sizes/dtype"), (broad(nvs=-1), E_ARG, "bad sizes/dtype"),
    (broad(nh=OVER - 1), E_ARG, "bad sizes/dtype"), (broad(maxp=OVER), E_ARG, "bad sizes/dtype"),
    (broad(vd=7), E_ARG, "bad sizes/dtype"), (broad(vd=7, n=None), E_ARG, "bad sizes/dtype"),
    (broad(n=None), E_ARG, NULL), (broad(pairs=None), E_ARG, NULL),
    (broad(nh=0, n=None), E_ARG, NULL),
    (broad(nh=0, verts=None, off=None, cnt=None), 0, None), (broad(maxp=0, pairs=None), PAST_CHECKS, None),
    *nulls(broad, ("verts", "off", "cnt")),
    (broad(off=OFF_PAST), E_ARG, OUTSIDE), (broad(off=OFF_NEG), E_ARG, OUTSIDE),
    (broad(cnt=CNT_300), PAST_CHECKS, None),                               # a hull above 256 is skipped, not checked
    (broad(cnt=CNT_300, off=OFF_NEG), E_ARG, OUTSIDE),
    (broad(cnt=CNT_0, off=OFF_WILD), PAST_CHECKS, None),
    (broad(), PAST_CHECKS, None),
    # ---- gjkepa_collide: the same order
    (collide(nh=-1), E_ARG, SIZES), (collide(maxc=-1), E_ARG, SIZES), (collide(nvs=-1), E_ARG, SIZES),
    (collide(nh=OVER - 1), E_ARG, SIZES), (collide(vd=7), E_ARG, SIZES), (collide(prec=7), E_ARG, SIZES),
    (collide(prec=7, nc=None), E_ARG, SIZES),                              # bad precision + null pointer
    (collide(nc=None), E_ARG, NULL), (collide(pairs=None), E_ARG, NULL), (collide(out=None), E_ARG, NULL),
    (collide(nh=0, nc=None), E_ARG, NULL),
    (collide(nh=0, verts=None, off=None, cnt=None, ncand=None), 0, None),
    (collide(maxc=0, pairs=None, out=None, ncand=None), PAST_CHECKS, None),
    *nulls(collide, ("verts", "off", "cnt")),
    (collide(off=OFF_PAST), E_ARG, OUTSIDE),
    (collide(cnt=CNT_300), PAST_CHECKS, None), (collide(cnt=CNT_300, off=OFF_NEG), E_ARG, OUTSIDE),
    (collide(), PAST_CHECKS, None),
    # ---- gjkepa_batch_device / gjkepa_batch_warm_device: n_pairs/enums -> null (n_pairs > 0) -> n_pairs > INT32_MAX
    (batch_dev(n=-1), E_ARG, "bad n_pairs/dtype/precision"), (batch_dev(vd=7), E_ARG, "bad n_pairs/dtype/precision"),
    (batch_dev(prec=7, out=None), E_ARG, "bad n_pairs/dtype/precision"),
    *nulls(batch_dev, POOL_PTRS + ("out", "ws")),
    (batch_dev(n=OVER, ws=None), E_ARG, NULL), (batch_dev(n=OVER), E_ARG, TOO_MANY),
    (warm_dev(n=-1), E_ARG, "bad n_pairs/dtype/precision"), (warm_dev(prec=7, warm=None), E_ARG, "bad n_pairs/dtype/precision"),
    *nulls(warm_dev, POOL_PTRS + ("out", "ws", "warm")),
    (warm_dev(n=OVER), E_ARG, TOO_MANY),
    # ---- gjkepa_distance_batch_device / gjkepa_cast_batch_device: args_ok -> null (n_pairs > 0) -> n_pairs == 0 -> workspace
    (dist_dev(n=-1), E_ARG, "bad n_pairs/dtype"), (dist_dev(vd=7, verts=None), E_ARG, "bad n_pairs/dtype"),
    (dist_dev(rec=P, rprec=9), E_ARG, "bad records_precision"), (dist_dev(maxd=NAN), E_ARG, MAXD),
    (dist_dev(maxd=-1.0, n=OVER), E_ARG, MAXD), (dist_dev(n=OVER, verts=None), E_ARG, TOO_MANY),
    *nulls(dist_dev, POOL_PTRS + ("out", "ws")),
    (dist_dev(ws=None, wsb=0), E_ARG, NULL),
    (dist_dev(n=0, verts=None, off=None, cnt=None, pairs=None, out=None, ws=None, wsb=0, rprec=9), 0, None),
    (dist_dev(wsb=255), E_WORKSPACE, WS), (dist_dev(wsb=0, rec=P), E_WORKSPACE, WS),
    (cast_dev(n=-1), E_ARG, "bad n_pairs/dtype"), (cast_dev(vd=7, motion=None), E_ARG, "bad n_pairs/dtype"),
    (cast_dev(rec=P, rprec=9), E_ARG, "bad records_precision"), (cast_dev(tol=0.0), E_ARG, TOL),
    (cast_dev(tol=NAN, n=OVER), E_ARG, TOL), (cast_dev(n=OVER, verts=None), E_ARG, TOO_MANY),
    *nulls(cast_dev, POOL_PTRS + ("motion", "out", "ws")),
    (cast_dev(ws=None, wsb=0), E_ARG, NULL),
    (cast_dev(n=0, verts=None, off=None, cnt=None, pairs=None, motion=None, out=None, ws=None, wsb=0, rprec=9), 0, None),
    (cast_dev(wsb=255), E_WORKSPACE, WS), (cast_dev(wsb=-1), E_WORKSPACE, WS),
    # ---- gjkepa_hull_batch_device: n_clouds/dtype -> n_clouds == 0 -> null
    (hull_dev(nc=-1), E_ARG, "bad n_clouds/dtype"), (hull_dev(vd=7, points=None), E_ARG, "bad n_clouds/dtype"),
    (hull_dev(nc=0, points=None, coff=None, ccnt=None, foff=None, faces=None, nf=None, nv=None, st=None), 0, None),
    *nulls(hull_dev, ("points", "coff", "ccnt", "foff", "faces", "nf", "nv", "st")),
]


def row_id(row):
    (entry, args), rc, _ = row
    return entry.replace("gjkepa_", "") + ("-ok" if rc == 0 else "-past" if rc is PAST_CHECKS else "")


@pytest.mark.parametrize("row", ROWS, ids=[f"{i:03d}-{row_id(r)}" for i, r in enumerate(ROWS)])
def test_return_code_and_error_text(lib, row):
    (entry, args), want_rc, want_text = row
    counts = {"count": ctypes.c_int64(-7), "count2": ctypes.c_int64(-7)}
    args = [a.ctypes.data if isinstance(a, np.ndarray) else ctypes.addressof(counts[a]) if isinstance(a, str) else a
            for a in args]
    rc =getattr(lib, entry)(*args)
    text = lib.gjkepa_last_error().decode()
    if want_rc is PAST_CHECKS:
        assert (rc, text) in PAST_CHECKS
    elif want_rc == 0:
        assert rc == 0                      # a call that succeeds leaves the last error alone
    else:
        assert (rc, text) == (want_rc, want_text)


def test_counts_are_zeroed_before_the_input_checks(lib):
    """gjkepa_broadphase and gjkepa_collide zero their output counts after the size and output-pointer
    checks and before everything else."""
    n, m = ctypes.c_int64(-7), ctypes.c_int64(-7)
    pn, pm = ctypes.addressof(n), ctypes.addressof(m)
    v, o, c, bad = VERTS.ctypes.data, OFF.ctypes.data, CNT.ctypes.data, OFF_PAST.ctypes.data
    assert lib.gjkepa_broadphase(7, v, 48, o, c, 4, P, 8, pn, -1) == E_ARG and n.value == -7        # sizes: untouched
    assert lib.gjkepa_broadphase(F64, v, 48, o, c, 4, None, 8, pn, -1) == E_ARG and n.value == -7   # output null: untouched
    assert lib.gjkepa_broadphase(F64, None, 48, o, c, 4, P, 8, pn, -1) == E_ARG and n.value == 0
    n.value = -7
    assert lib.gjkepa_broadphase(F64, v, 48, bad, c, 4, P, 8, pn, -1) == E_ARG and n.value == 0
    n.value = -7
    assert lib.gjkepa_broadphase(F64, None, 0, None, None, 0, None, 0, pn, -1) == 0 and n.value == 0
    n.value = -7
    assert lib.gjkepa_collide(2, 1.0, F64, 7, v, 48, o, c, 4, P, P, 8, pn, pm, -1) == E_ARG and (n.value, m.value) == (-7, -7)
    assert lib.gjkepa_collide(2, 1.0, F64, 1, v, 48, o, c, 4, None, P, 8, pn, pm, -1) == E_ARG and (n.value, m.value) == (-7, -7)
    assert lib.gjkepa_collide(2, 1.0, F64, 1, v, 48, bad, c, 4, P, P, 8, pn, pm, -1) == E_ARG and (n.value, m.value) == (0, 0)
    n.value = m.value = -7
    assert lib.gjkepa_collide(2, 1.0, F64, 1, None, 0, None, None, 0, None, None, 0, pn, None, -1) == 0 and n.value == 0


def test_multi_shares_the_pool_check(lib):
    """gjkepa_batch_multi validates the whole job as one gjkepa_batch call would, before any shard runs."""
    dev = np.zeros(1, np.int32)

    def multi(pairs=PAIRS, off=OFF, cnt=CNT):
        rc = lib.gjkepa_batch_multi(2, 1.0, F64, 1, VERTS.ctypes.data, 48, off.ctypes.data, cnt.ctypes.data, 4,
                                    pairs.ctypes.data, 2, P, dev.ctypes.data, 1)
        return rc, lib.gjkepa_last_error().decode()

    assert multi(pairs=BAD_PAIRS, off=OFF_PAST) == (E_ARG, MISSING)
    assert multi(off=OFF_PAST) == (E_ARG, OUTSIDE)
    assert multi(cnt=CNT_300) == (E_ARG, OUTSIDE)
