"""The mass properties' definition (include/gjkepa.h gjkepa_mass_batch, csrc/mass_props.h) without a GPU: the
header's text, compiled for the host (tests/mass_host.cpp), gives the bytes of the numpy restatement
(tests/mass_ref.py) on every shape the GPU test uses; the restatement is exact on a box and a tetrahedron, stays
within 1e-13 of an exact rational reference, reports a closed surface as closed and an open one as open, follows
the five status rules in their order, and moves with a translation.  Faces come from the oracle's hull, which is
the device's bit for bit.

Measured with the seeds below (sphere clouds of 4, 8, 32, 64 and 256 points, six each, centred within 10 of the
origin): volume 3.4e-16 relative, centre of mass 1.7e-16 of the largest |coordinate|, inertia 4.2e-16 of
volume x radius^2, closure 1.1e-17 at most, with the clouds as they are, shifted by 1e3 in fp64, or shifted and
rounded to fp32."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import gjkepa
import mass_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
OK, DEGENERATE, BAD_INPUT = mr.OK, mr.DEGENERATE, mr.BAD_INPUT

ACC_SIZES, ACC_SEEDS = (4, 8, 32, 64, 256), range(6)
TOL = 1e-13                                  # volume relative; com of max|coordinate|; inertia of volume radius^2
CLOSURE_MEASURED = 1.1e-17                   # the largest closure of the accuracy clouds, shifted or not
CLOSURE_BOUND = 16 * CLOSURE_MEASURED
OPEN_BOUND = 1e-3                            # a mesh without its last face
# the seed per size whose last face is at least a thousandth of the surface (a 256-point sphere cloud's mean
# face is 1 / 508 of it, so not every seed's is)
DROP_SEED = {8: 0, 32: 0, 64: 0, 256: 5}


@pytest.fixture(scope="module")
def mass_host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("mass_host")), "libmass_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    os.path.join(ROOT, "tests", "mass_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.mass_host.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_int64, vp, vp, vp, vp, vp]

    def run(pool, hull, use_status=True):
        verts = np.ascontiguousarray(pool.verts)
        off, cnt = np.ascontiguousarray(pool.cloud_off, np.int64), np.ascontiguousarray(pool.cloud_cnt, np.int32)
        foff, nf = np.ascontiguousarray(hull["face_off"], np.int64), np.ascontiguousarray(hull["n_faces"], np.int32)
        faces = np.ascontiguousarray(hull["faces"], np.int32)
        hs = np.ascontiguousarray(hull["status"], np.int8) if use_status else None
        out = np.zeros(cnt.size, gjkepa.MASS64)
        assert lib.mass_host(pool.dtype_code, verts.ctypes.data, off.ctypes.data, cnt.ctypes.data, cnt.size, foff.ctypes.data,
                             faces.ctypes.data, nf.ctypes.data, None if hs is None else hs.ctypes.data, out.ctypes.data) == 0
        return out
    return run


def hull_of(orc, pool):
    return orc.hull_batch(pool.verts, pool.cloud_off, pool.cloud_cnt)


def one(orc, p):
    """(faces, record of the restatement) of one (n, 3) cloud with the oracle's hull"""
    pool = gjkepa.CloudPool.from_list([p])
    h = hull_of(orc, pool)
    assert h["status"][0] == OK
    f = h["faces"][:h["n_faces"][0]]
    return f, mr.cloud(p, f)


def acc_cloud(n, seed):
    rng = np.random.default_rng(1000 * n + seed)
    return mr.unit_cloud(1000 * n + seed, n, 1, rng.uniform(-5.7, 5.7, 3))      # |centre| < 10


def nonzero_only_status(r):
    z = np.zeros((), gjkepa.MASS64)
    z["status"] = r["status"]
    return r.tobytes() == z.tobytes()


# ---------------------------------------------------------------- the header's text
@needs_gxx
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_header_text_gives_the_restatements_bytes(mass_host, orc, dtype):
    clouds, what = mr.mixed_clouds(60, seed=3)
    pool = gjkepa.CloudPool.from_list(clouds, dtype=dtype)
    h = hull_of(orc, pool)
    assert {w for w in what if isinstance(w, tuple)} == {(n, s) for n in mr.SIZES for s in (0, 1)}
    assert "bad" in what and "flat" in what
    for use_status in (True, False):
        got, want = mass_host(pool, h, use_status), mr.reference(pool, h, use_status)
        assert got.tobytes() == want.tobytes()
    st = want["status"]
    for c, w in enumerate(what):
        if w == "bad":
            assert st[c] == BAD_INPUT
        elif w == "flat":
            assert st[c] == BAD_INPUT and mr.reference(pool, h)[c]["status"] == DEGENERATE   # no faces / the hull's status
        else:
            assert st[c] == OK and want["n_faces"][c] == h["n_faces"][c]
            if w[1] == 1:
                assert h["n_faces"][c] == 2 * w[0] - 4
            elif w[0] >= 16:
                assert h["n_faces"][c] < 2 * w[0] - 4
    assert all(nonzero_only_status(r) for r in want[st != OK])


# ---------------------------------------------------------------- closed forms
def test_restatement_is_exact_on_a_box_and_a_tetrahedron(orc):
    box = np.array([[x, y, z] for x in (5, 6) for y in (-3, -1) for z in (2, 5)], float)
    _, r = one(orc, box)
    assert r["status"] == OK and r["volume"] == 6.0 and r["area"] == 22.0 and r["n_faces"] == 12
    assert r["com"].tolist() == [5.5, -2.0, 3.5]
    assert (r["inertia"] == [6.5, 5.0, 2.5, 0.0, 0.0, 0.0]).all()
    assert r["closure"] == 0.0 and r["radius"] == np.sqrt(0.25 + 1.0 + 2.25)
    _, t = one(orc, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float))
    assert t["status"] == OK and t["volume"] == 1.0 / 6.0 and t["com"].tolist() == [0.25, 0.25, 0.25] and t["n_faces"] == 4


# ---------------------------------------------------------------- accuracy, closure
def test_restatement_against_the_exact_reference(orc):
    worst = dict(volume=0.0, com=0.0, inertia=0.0)
    for n in ACC_SIZES:
        for seed in ACC_SEEDS:
            p = acc_cloud(n, seed)
            f, r = one(orc, p)
            ex = mr.exact(p, f)
            worst["volume"] = max(worst["volume"], abs(r["volume"] - ex["volume"]) / ex["volume"])
            worst["com"] = max(worst["com"], np.abs(r["com"] - ex["com"]).max() / np.abs(p).max())
            worst["inertia"] = max(worst["inertia"], np.abs(r["inertia"] - ex["inertia"]).max() / (ex["volume"] * ex["radius"] ** 2))
            assert abs(r["radius"] - ex["radius"]) <= 1e-13 * ex["radius"]
    print("worst errors against exact rationals, as multiples of the bound's unit:", worst)
    assert worst["volume"] <= TOL and worst["com"] <= TOL and worst["inertia"] <= TOL
    assert max(worst.values()) <= 0.1 * TOL          # a tenth of the bound: anything above wants an explanation


def test_closure_of_closed_and_open_meshes(orc):
    assert CLOSURE_BOUND < 1e-9
    worst = 0.0
    for n in ACC_SIZES:
        for seed in ACC_SEEDS:
            p = acc_cloud(n, seed)
            f, r = one(orc, p)
            far = mr.cloud(p + 1e3, f)                                   # exact in fp64: the same hull
            _, far32 = one(orc, (p + 1e3).astype(np.float32).astype(np.float64))
            worst = max(worst, r["closure"], far["closure"], far32["closure"])
            assert far["status"] == OK and far32["status"] == OK
    print("largest closure of a closed mesh:", worst)
    assert worst <= CLOSURE_MEASURED and worst <= CLOSURE_BOUND
    for n, seed in DROP_SEED.items():
        p = acc_cloud(n, seed)
        f, r = one(orc, p)
        cut = mr.cloud(p, f[:-1])
        assert r["closure"] <= CLOSURE_BOUND
        assert cut["status"] == OK and cut["closure"] >= OPEN_BOUND


# ---------------------------------------------------------------- status rules
def test_status_rules_and_their_order(orc):
    p = acc_cloud(8, 1)
    f, good = one(orc, p)
    n, F = len(p), len(f)
    assert good["status"] == OK and F == 12 == 2 * n - 4
    nan_p = np.vstack([p, [[np.nan, 0.0, 0.0]]])                        # a point no face references
    bad_hi, bad_lo = f.copy(), f.copy()
    bad_hi[5, 1], bad_lo[11, 2] = n, -1
    inward = f[:, [0, 2, 1]]
    cases = [
        (p[:3], f[:4] % 3, None, BAD_INPUT),                               # rule 1: n = 3
        (p, f, DEGENERATE, DEGENERATE),                                  # rule 2: the hull's status, valid faces
        (p, f[:3], None, BAD_INPUT),                                     # rule 3: F = 3
        (p, np.vstack([f, f[:1]]), None, BAD_INPUT),                     # rule 3: F = 2n - 3
        (p, bad_hi, None, BAD_INPUT),                                    # rule 4: an index of n
        (p, bad_lo, None, BAD_INPUT),                                    # rule 4: an index of -1
        (nan_p, f, None, BAD_INPUT),                                     # rule 4: a NaN point no face references
        (p, inward, None, DEGENERATE),                                   # rule 5: T0 < 0
        # the order: 1 before 2, 2 before 3 and 4, 3 before 4, 4 before 5
        (p[:3], f[:4] % 3, DEGENERATE, BAD_INPUT),
        (p, f[:3], DEGENERATE, DEGENERATE),
        (p, bad_hi, mr.DEGENERATE, DEGENERATE),
        (p, np.vstack([bad_hi, f[:1]]), None, BAD_INPUT),
        (nan_p, inward, None, BAD_INPUT),
    ]
    for k, (pts, faces, hs, want) in enumerate(cases):
        r = mr.cloud(pts, faces, hs)
        assert r["status"] == want, k
        assert nonzero_only_status(r), k
    assert mr.cloud(p, f, OK).tobytes() == good.tobytes()


@needs_gxx
def test_header_text_follows_the_status_rules(mass_host, orc):
    """the same hand-written clouds through the header's text: caller-supplied faces, a status array of the caller's"""
    p = acc_cloud(8, 1)
    f, _ = one(orc, p)
    bad_hi, bad_lo, inward = f.copy(), f.copy(), f[:, [0, 2, 1]]
    bad_hi[5, 1], bad_lo[11, 2] = 8, -1
    nan_p = np.vstack([p, [[np.nan, 0.0, 0.0]]])
    rows = [(p, f, OK), (p[:3], f[:4] % 3, OK), (p, f, DEGENERATE), (p, f[:3], OK), (p, np.vstack([f, f[:1]]), OK), (p, bad_hi, OK),
            (p, bad_lo, OK), (nan_p, f, OK), (p, inward, OK), (p, f[:3], DEGENERATE), (nan_p, inward, OK), (p, f, OK)]
    pool = gjkepa.CloudPool.from_list([r[0] for r in rows])
    foff = np.cumsum([0] + [len(r[1]) + 2 for r in rows[:-1]]).astype(np.int64)      # blocks of the caller's own
    faces = np.full((foff[-1] + len(rows[-1][1]) + 2, 3), 1 << 30, np.int32)
    for o, r in zip(foff, rows):
        faces[o:o + len(r[1])] = r[1]
    hull = dict(faces=faces, face_off=foff, n_faces=np.array([len(r[1]) for r in rows], np.int32),
                status=np.array([r[2] for r in rows], np.int8))
    got = mass_host(pool, hull)
    want = np.array([mr.cloud(r[0], r[1], r[2]) for r in rows])
    assert got.tobytes() == want.tobytes()
    assert got["status"].tolist() == [OK, BAD_INPUT, DEGENERATE, BAD_INPUT, BAD_INPUT, BAD_INPUT, BAD_INPUT, BAD_INPUT, DEGENERATE,
                                      DEGENERATE, BAD_INPUT, OK]
    assert got[0].tobytes() == got[-1].tobytes()


# ---------------------------------------------------------------- translation
def test_translation_moves_the_centre_and_nothing_else(orc):
    shift = np.array([1000.0, -1000.0, 500.0])
    for n in (8, 64, 256):
        p = np.round(acc_cloud(n, 2) * 8192.0) / 8192.0                 # on the 2^-13 grid: the shift is exact in fp32
        q = p + shift
        assert (q.astype(np.float32).astype(np.float64) == q).all() and (p.astype(np.float32) == p).all()
        f, r = one(orc, p)
        g, s = one(orc, q)
        scale = np.abs(q).max()
        assert np.abs((s["com"] - r["com"]) - shift).max() <= TOL * scale
        assert abs(s["volume"] - r["volume"]) <= TOL * r["volume"]
        assert np.abs(s["inertia"] - r["inertia"]).max() <= TOL * r["volume"] * r["radius"] ** 2
        assert abs(s["radius"] - r["radius"]) <= TOL * scale


def test_record_size(lib):
    assert gjkepa.MASS64.itemsize == 128 == lib.gjkepa_mass_record_bytes()
    assert gjkepa.MASS64.fields["n_faces"][1] == 104 and gjkepa.MASS64.fields["status"][1] == 108
