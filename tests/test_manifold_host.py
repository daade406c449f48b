"""The contact manifold's plane geometry (csrc/manifold_clip.h, shared by the manifold kernel) on the
host: tests/manifold_host.cpp runs it over a plain scan with contact records from the oracle, and its
records are checked here the way tests/test_manifold.py checks the GPU's, without a GPU
(tests/manifold_ref.py): the support plane, the depth, orientation and convexity, containment in the
reference's footprints, the codes, and coverage of the reference's clipped polygon."""
import shutil

import numpy as np
import pytest

import gjkepa
import manifold_ref as mr

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return mr.build_manifold_host(tmp_path_factory.mktemp("manifold_host"))


def test_host_box_pool(host, orc):
    pool = mr.box_pool()
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    rec = host(pool, contact, mr.MARGIN)
    comp, hist = mr.check_pool(pool, contact, rec, name="box pool (host)", min_hits=100)
    assert hist[4] >= 100, hist


@pytest.mark.parametrize("name", list(mr.SPHERE_POOLS))
def test_host_sphere_pool(host, orc, name):
    pool = mr.sphere_pool(name)
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    rec = host(pool, contact, mr.MARGIN)
    mr.check_pool(pool, contact, rec, name=f"sphere pool {name} (host)")
    # fp32 and fp64 storage of the same values: the same bytes
    assert host(pool.as_dtype(np.float64), contact, mr.MARGIN).tobytes() == rec.tobytes()


def test_host_prism_pool(host, orc):
    pool = mr.prism_pool()
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    rec = host(pool, contact, mr.MARGIN)
    comp, _ = mr.check_pool(pool, contact, rec, name="prism pool (host)")
    k = np.repeat(mr.PRISM_K, len(rec) // len(mr.PRISM_K))
    dec = (rec["flags"] & mr.DECIMATED) != 0
    assert not dec[comp & (k <= 32)].any() and dec[comp & (k >= 33)].any()
    # a 33-gon's face is the smallest feature over the cap: every second vertex is used
    on_self = comp & (k == 33) & (rec["n_feat_a"] == 33)
    assert on_self.any() and dec[on_self].all()


def test_host_tier_boundary_pool(host, orc):
    pool = mr.tier_boundary_pool()
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    rec = host(pool, contact, mr.MARGIN)
    comp, _ = mr.check_pool(pool, contact, rec, name="tier-boundary pool (host)")
    mr.check_boundary_cover(pool, comp)


def test_host_known_answers(host, orc):
    answers = mr.known_answers()
    names = list(answers)
    pool = gjkepa.HullPool.from_pairs([(answers[k][0], answers[k][1]) for k in names])
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    assert (contact["collision"] != 0).all() and (contact["status"] == 0).all(), contact
    rec = host(pool, contact, mr.MARGIN)
    mr.check_known(rec, names, answers)
    mr.check_pool(pool, contact, rec, name="known answers (host)", min_hits=len(names))


def test_host_no_hit_bad_input_and_f32_records(host, orc):
    pool = mr.sphere_pool("8-32")
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    rec = host(pool, contact, mr.MARGIN)
    hits = np.nonzero(mr.is_computed(contact))[0]
    # a record with a status, a zero or a NaN normal is no usable collision
    c2 = contact.copy()
    c2["status"][hits[0]] = gjkepa.STATUS_EPA_MAXITER
    c2["collision_normal"][hits[1]] = 0
    c2["collision_normal"][hits[2], 1] = np.nan
    r2 = host(pool, c2, mr.MARGIN)
    assert (r2["flags"][hits[:3]] == mr.NO_HIT).all() and (r2["n_points"][hits[:3]] == 0).all()
    keep = np.ones(len(rec), bool)
    keep[hits[:3]] = False
    assert r2[keep].tobytes() == rec[keep].tobytes()
    # bad counts come first (whatever the record says), non-finite vertices only where a pair is computed
    miss = np.nonzero(~mr.is_computed(contact))[0]
    verts, cnt = pool.verts.copy(), pool.hull_cnt.copy()
    cnt[pool.pairs[miss[0], 0]] = 0
    cnt[pool.pairs[hits[3], 1]] = 257
    verts[int(pool.hull_off[pool.pairs[hits[4], 1]]) + 1] = np.nan
    verts[int(pool.hull_off[pool.pairs[miss[1], 0]])] = np.nan
    r3 = host(gjkepa.HullPool(verts, pool.hull_off, cnt, pool.pairs), contact, mr.MARGIN)
    bad = [miss[0], hits[3], hits[4]]
    assert (r3["status"][bad] == gjkepa.STATUS_BAD_INPUT).all() and (r3["flags"][bad] == 0).all()
    assert (r3["n_points"][bad] == 0).all() and (r3["point"][bad] == 0).all() and (r3["code"][bad] == 0xFFFFFFFF).all()
    assert r3["flags"][miss[1]] == mr.NO_HIT and r3["status"][miss[1]] == gjkepa.STATUS_OK
    keep = np.ones(len(rec), bool)
    keep[bad] = False
    assert r3[keep].tobytes() == rec[keep].tobytes()
    # fp32 contact records: the widened normal is the record's, and the checks hold for it
    c32 = np.zeros(len(contact), gjkepa.REC32)
    for f in contact.dtype.names:
        if f != "pad":
            c32[f] = contact[f]
    r32 = host(pool, c32, mr.MARGIN)
    assert (r32["normal"] == c32["collision_normal"].astype(np.float64)).all()
    assert np.array_equal((r32["flags"] & mr.NO_HIT) != 0, ~mr.is_computed(c32))


def test_host_margin_widens_the_features(host, orc):
    """margin 0 keeps only the extreme vertices; a margin above the tilt takes the whole face"""
    rng = np.random.default_rng(7)
    a, b = mr.stack(rng, mr.box(1, 1, 0.5), mr.box(0.6, 0.6, 0.5), tilt=1e-4)
    pool = gjkepa.HullPool.from_pairs([(a, b)])
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    assert contact["collision"][0] != 0
    wide = host(pool, contact, 1e-3)[0]
    assert wide["n_feat_a"] == 4 and wide["n_feat_b"] == 4 and wide["n_points"] == 4
    thin = host(pool, contact, 0.0)[0]
    assert thin["n_feat_b"] < 4 and thin["n_points"] < 4
