"""The event pass and the one-call moving step at the C-ABI (include/gjkepa.h gjkepa_events_device,
gjkepa_collide_moving): the argument checks, all answered before any device work; the counts zeroed before the
input checks; n_hulls == 0; and, on the GPU, the workspace bound at its exact size and the empty pair list."""
import math

import numpy as np
import pytest

import gjkepa

INF = float("inf")
P = 0x1000          # never dereferenced: the calls that take it are answered before any device work


def events_call(lib, pairs=P, n_pairs=1, n_hulls=4, cast=P, records=None, prec=gjkepa.PREC_F64, events=P, max_events=1,
                n_events=P, counts=P, body_time=P, body_event=P, ws=P, ws_bytes=0):
    return lib.gjkepa_events_device(pairs, n_pairs, n_hulls, cast, records, prec, events, max_events, n_events, counts,
                                    body_time, body_event, ws, ws_bytes, None)


def test_exports_and_sizes(lib):
    for f in ("gjkepa_event_record_bytes", "gjkepa_events_workspace_bytes", "gjkepa_events_device", "gjkepa_collide_moving"):
        assert f in gjkepa.EXPORTS and hasattr(lib, f)
    assert lib.gjkepa_event_record_bytes() == 128
    assert lib.gjkepa_events_workspace_bytes(-1, 0) == -1 and lib.gjkepa_events_workspace_bytes(0, -1) == -1
    assert lib.gjkepa_events_workspace_bytes(1 << 31, 0) == -1
    with pytest.raises(gjkepa.GjkEpaError):
        gjkepa.events_workspace_bytes(-5, 1)


def test_events_device_argument_checks_without_gpu(lib):
    assert events_call(lib, n_pairs=-1) == -1                                          # negative sizes
    assert events_call(lib, n_hulls=-1) == -1
    assert events_call(lib, max_events=-1) == -1
    assert events_call(lib, n_pairs=1 << 31) == -1
    assert events_call(lib, records=P, prec=9) == -1                                   # bad records_precision with records
    assert b"records_precision" in lib.gjkepa_last_error()
    assert events_call(lib, body_time=None) == -1                                      # exactly one body pointer
    assert events_call(lib, body_event=None) == -1
    assert b"both or neither" in lib.gjkepa_last_error()
    for hole in ("pairs", "cast", "events", "n_events", "counts", "ws"):               # null required pointers
        assert events_call(lib, **{hole: None}) == -1, hole
        assert b"null pointer" in lib.gjkepa_last_error()
    assert events_call(lib, n_pairs=0, n_events=None) == -1                            # the counts are always required
    assert events_call(lib, n_pairs=0, counts=None) == -1
    # what is not an argument error reaches the workspace check: a bad precision without records, no body outputs, no list
    assert events_call(lib, prec=9) == -4
    assert events_call(lib, body_time=None, body_event=None) == -4
    assert events_call(lib, events=None, max_events=0) == -4
    assert events_call(lib, ws_bytes=511) == -4                                        # keys and indices alone need more
    assert events_call(lib, n_pairs=5000, ws_bytes=5000 * 24) == -4
    assert b"workspace" in lib.gjkepa_last_error()


def moving_call(lib, version=2, dtype=0, prec=1, verts=P, n_scalars=24, off=P, cnt=P, n_hulls=1, motion=P, tol=1e-3, lr=INF,
                events=P, max_events=1, n_events=P, counts=None, n_cand=None):
    return lib.gjkepa_collide_moving(version, 1.0, dtype, prec, verts, n_scalars, off, cnt, n_hulls, motion, tol, lr, events,
                                     max_events, n_events, counts, n_cand, None, None, 0)


def test_collide_moving_argument_checks_without_gpu(lib):
    assert moving_call(lib, dtype=7) == -1 and moving_call(lib, prec=7) == -1
    assert moving_call(lib, n_scalars=-1) == -1 and moving_call(lib, n_hulls=-1) == -1 and moving_call(lib, max_events=-1) == -1
    for tol in (0.0, -1.0, math.nan, INF):
        assert moving_call(lib, tol=tol) == -1
        assert b"tolerance" in lib.gjkepa_last_error()
    for lr in (math.nan, -1.0):
        assert moving_call(lib, lr=lr) == -1
    assert moving_call(lib, n_events=None) == -1 and moving_call(lib, events=None) == -1
    n, counts, cand = np.full(1, 77, np.int64), np.full(5, 77, np.int64), np.full(1, 77, np.int64)
    out = dict(n_events=n.ctypes.data, counts=counts.ctypes.data, n_cand=cand.ctypes.data)
    # no hulls: an empty step, answered at once
    assert moving_call(lib, n_hulls=0, verts=None, off=None, cnt=None, motion=None, **out) == 0
    assert n[0] == 0 and cand[0] == 0 and (counts == 0).all()
    # the counts are zeroed before the input checks: a null pool, a hull outside the pool
    for a in (n, counts, cand):
        a[:] = 77
    assert moving_call(lib, verts=None, **out) == -1
    assert n[0] == 0 and cand[0] == 0 and (counts == 0).all()
    for a in (n, counts, cand):
        a[:] = 77
    off, cnt = np.array([23], np.int64), np.array([8], np.int32)
    assert moving_call(lib, off=off.ctypes.data, cnt=cnt.ctypes.data, **out) == -1
    assert b"outside the vertex pool" in lib.gjkepa_last_error()
    assert n[0] == 0 and cand[0] == 0 and (counts == 0).all()
    # an argument error leaves them alone
    n[0] = 77
    assert moving_call(lib, tol=0.0, **out) == -1 and n[0] == 77


def test_python_wrappers_check_their_arrays():
    pool = gjkepa.synth_scene(1, 4, 8, 8, 2.0)
    with pytest.raises(gjkepa.GjkEpaError, match="body_motion"):
        gjkepa.collide_moving(pool, np.zeros((3, 9)), 1e-3)
    with pytest.raises(gjkepa.GjkEpaError, match="tolerance"):
        gjkepa.collide_moving(pool, np.zeros((4, 9)), 0.0)
    res = gjkepa.collide_moving(gjkepa.HullPool(pool.verts[:0], pool.hull_off[:0], pool.hull_cnt[:0], pool.pairs),
                                np.zeros((0, 9)), 1e-3)
    assert res["n_events"] == 0 and res["n_candidates"] == 0 and len(res["events"]) == 0 and len(res["body_time"]) == 0


@pytest.mark.gpu
def test_workspace_bound_and_empty_list_on_the_gpu(lib):
    import torch
    dev = torch.device("cuda", 0)
    n, nh = 1000, 50
    need = gjkepa.events_workspace_bytes(n, nh)
    assert need % 256 == 0 and need >= n * 24
    assert gjkepa.events_workspace_bytes(0, 0) >= 256
    z = lambda count, dt: torch.zeros(count, dtype=dt, device=dev)
    pairs, cast, ev, ws = z(2 * n, torch.int32), z(n * 128, torch.uint8), z(n * 128, torch.uint8), z(need, torch.uint8)
    cnt, bt, be = torch.full((6,), 77, dtype=torch.int64, device=dev), z(nh, torch.float64), z(nh, torch.int32)
    call = lambda n_pairs, bytes_: lib.gjkepa_events_device(pairs.data_ptr(), n_pairs, nh, cast.data_ptr(), None, 0, ev.data_ptr(), n,
                                                            cnt.data_ptr(), cnt.data_ptr() + 8, bt.data_ptr(), be.data_ptr(),
                                                            ws.data_ptr(), bytes_, None)
    assert call(n, need - 1) == -4                                                     # one byte short: nothing enqueued
    torch.cuda.synchronize(dev)
    assert (cnt == 77).all()
    assert call(n, need) == 0                                                          # all-zero cast records are misses
    torch.cuda.synchronize(dev)
    assert (cnt == 0).all() and (bt == 1.0).all() and (be == -1).all()
    cnt.fill_(77); bt.fill_(0.5); be.fill_(7)
    assert call(0, 0) == 0                                                             # an empty list needs no workspace
    torch.cuda.synchronize(dev)
    assert (cnt == 0).all() and (bt == 1.0).all() and (be == -1).all() and (ev == 0).all()
