"""The mass-property entries at the C-ABI (include/gjkepa.h gjkepa_mass_record_bytes, gjkepa_mass_batch_device,
gjkepa_mass_batch, gjkepa_mass_pool): the record size and the argument checks, all answered before any device
work, as test_hull_api_validation_without_gpu does it for the hull entries."""
import numpy as np
import pytest

import gjkepa

P = 0x1000          # never dereferenced: the calls that take it are answered before any device work


def device_call(lib, dtype=0, points=P, off=P, cnt=P, n=1, foff=P, faces=P, nf=P, hs=None, out=P, motion=None):
    return lib.gjkepa_mass_batch_device(dtype, points, off, cnt, n, foff, faces, nf, hs, out, motion, None)


def host_call(lib, dtype=1, points=P, n_scalars=24, off=P, cnt=P, n=1, foff=P, slots=12, faces=P, nf=P, hs=None, out=P, motion=None):
    return lib.gjkepa_mass_batch(dtype, points, n_scalars, off, cnt, n, foff, slots, faces, nf, hs, out, motion, 0)


def pool_call(lib, dtype=1, verts=P, n_scalars=24, off=P, cnt=P, n=1, out=P, motion=None):
    return lib.gjkepa_mass_pool(dtype, verts, n_scalars, off, cnt, n, out, motion, 0)


def test_exports_and_record_size(lib):
    for f in ("gjkepa_mass_record_bytes", "gjkepa_mass_batch_device", "gjkepa_mass_batch", "gjkepa_mass_pool"):
        assert f in gjkepa.EXPORTS and hasattr(lib, f)
    assert lib.gjkepa_mass_record_bytes() == 128 == gjkepa.MASS64.itemsize


def test_device_entry_argument_checks_without_gpu(lib):
    assert device_call(lib, dtype=7) == -1 and b"dtype" in lib.gjkepa_last_error()
    assert device_call(lib, n=-1) == -1
    for hole in ("points", "off", "cnt", "foff", "faces", "nf", "out"):
        assert device_call(lib, **{hole: None}) == -1, hole
        assert b"null pointer" in lib.gjkepa_last_error()
    # no clouds: answered at once, nothing touched
    assert device_call(lib, n=0) == 0
    assert device_call(lib, n=0, points=None, off=None, cnt=None, foff=None, faces=None, nf=None, out=None) == 0


def test_host_entry_argument_checks_without_gpu(lib):
    assert host_call(lib, dtype=7) == -1 and b"dtype" in lib.gjkepa_last_error()
    assert host_call(lib, n=-1) == -1 and host_call(lib, n_scalars=-1) == -1 and host_call(lib, slots=-1) == -1
    assert b"sizes" in lib.gjkepa_last_error()
    for hole in ("points", "off", "cnt", "foff", "faces", "nf", "out"):
        assert host_call(lib, **{hole: None}) == -1, hole
        assert b"null pointer" in lib.gjkepa_last_error()
    out = np.full(2, 7, gjkepa.MASS64)
    assert host_call(lib, n=0, out=out.ctypes.data) == 0 and (out["status"] == 7).all()
    assert host_call(lib, n=0, points=None, off=None, cnt=None, foff=None, faces=None, nf=None, out=None) == 0
    # the pool and face-buffer checks of gjkepa_hull_batch
    cnt, foff = np.array([8, 8], np.int32), np.array([0, 12], np.int64)
    args = dict(cnt=cnt.ctypes.data, foff=foff.ctypes.data, n=2, n_scalars=48, slots=24, out=out.ctypes.data)
    for off in ([0, 25], [-1, 24]):
        o = np.array(off, np.int64)
        assert host_call(lib, off=o.ctypes.data, **args) == -1
        assert b"cloud outside the point pool" in lib.gjkepa_last_error()
    o = np.array([0, 24], np.int64)
    for bad in ([0, 13], [-1, 12]):
        f = np.array(bad, np.int64)
        assert host_call(lib, off=o.ctypes.data, **{**args, "foff": f.ctypes.data}) == -1
        assert b"face block outside the face buffer" in lib.gjkepa_last_error()
    assert host_call(lib, off=o.ctypes.data, **{**args, "slots": 23}) == -1
    assert (out["status"] == 7).all()


def test_pool_entry_argument_checks_without_gpu(lib):
    assert pool_call(lib, dtype=7) == -1 and pool_call(lib, n=-1) == -1 and pool_call(lib, n_scalars=-1) == -1
    for hole in ("verts", "off", "cnt", "out"):
        assert pool_call(lib, **{hole: None}) == -1, hole
        assert b"null pointer" in lib.gjkepa_last_error()
    assert pool_call(lib, n=0, verts=None, off=None, cnt=None, out=None) == 0
    off, cnt = np.array([23], np.int64), np.array([8], np.int32)
    assert pool_call(lib, off=off.ctypes.data, cnt=cnt.ctypes.data) == -1
    assert b"outside the vertex pool" in lib.gjkepa_last_error()


def test_python_wrappers_check_their_arrays():
    pool = gjkepa.synth_scene(1, 4, 8, 8, 2.0)
    with pytest.raises(gjkepa.GjkEpaError, match="body_motion"):
        gjkepa.mass_pool(pool, np.zeros((3, 9)))
    clouds = gjkepa.synth_clouds(1, 3, 8, 8)
    hull = dict(faces=np.zeros((36, 3), np.int32), face_off=np.array([0, 12], np.int64), n_faces=np.zeros(3, np.int32),
                status=np.zeros(3, np.int8))
    with pytest.raises(gjkepa.GjkEpaError, match="per cloud"):
        gjkepa.mass_batch(clouds, hull)
    empty = gjkepa.HullPool(pool.verts[:0], pool.hull_off[:0], pool.hull_cnt[:0], pool.pairs)
    rec, bm = gjkepa.mass_pool(empty, np.zeros((0, 9)))
    assert len(rec) == 0 and bm.shape == (0, 9) and rec.dtype == gjkepa.MASS64
