"""The contact manifold at the time of impact on the host: tests/impact_host.cpp runs the header texts
(csrc/manifold_clip.h, csrc/rigid_pose.h) over a plain scan, with cast records from the host cast program
(tests/cast_rigid_host.cpp) and contact records from the oracle, and its records are checked here without a GPU
the way tests/test_manifold_cast.py checks the kernel's (tests/impact_ref.py).

Measured on the host program (g++ -O2 -ffp-contract=off):
  known answers: the largest position error is 7.0e-12 (impact_ref.POSITION_MEASURED; the bound is 16 times it).
  box pool (320 stacks, seed 0x1A9D): 300 computed, all impacts, n_points 1/2/3/4 = 216/0/0/84, no undecided pair.
  tier-boundary pool (49 pairs): 49 computed impacts of one point each, every bracket covered, no undecided pair."""
import shutil

import numpy as np
import pytest

import cast_rigid_ref as rr
import gjkepa
import impact_ref as ir
import manifold_ref as mr

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
IMPACT, START, SKIPPED = gjkepa.CAST_IMPACT, gjkepa.CAST_START, gjkepa.CAST_SKIPPED
OK, BAD, MAXITER = gjkepa.STATUS_OK, gjkepa.STATUS_BAD_INPUT, gjkepa.STATUS_CAST_MAXITER


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ir.build_impact_host(tmp_path_factory.mktemp("impact_host"))


@pytest.fixture(scope="module")
def cast_host(tmp_path_factory):
    return rr.build_host(tmp_path_factory.mktemp("cast_rigid_host"))[0]


@pytest.fixture(scope="module")
def manifold_host(tmp_path_factory):
    return mr.build_manifold_host(tmp_path_factory.mktemp("manifold_host"))


def test_record_layout_and_flag():
    assert gjkepa.MANIFOLD_AT_TOI == 8 and gjkepa.MANIFOLD64.itemsize == 160
    f = gjkepa.MANIFOLD64.fields
    assert [f[k][1] for k in ("depth", "normal", "point", "code", "n_feat_a", "n_feat_b", "n_points", "status", "flags",
                              "reserved", "area")] == [0, 8, 32, 128, 144, 146, 148, 149, 150, 151, 152]
    with open(ir.ROOT + "/include/gjkepa.h") as fh:
        assert "#define GJKEPA_MANIFOLD_AT_TOI    8" in fh.read()


def test_host_known_answers(host, cast_host):
    """The largest position error measured here is 7.0e-12 (a reported point against the touching vertex as the
    numpy pose puts it at toi, projected onto z = 0); bounded at 16 times that, and a tenth of the bound is the
    most a run may show without an explanation."""
    cases, pool, bm = ir.known_pool()
    cast = cast_host(pool, bm, ir.TAU)
    rec = host(pool, bm, cast, ir.MARGIN)
    worst = ir.check_known(rec, cast, cases, bm)
    print(f"largest position error {worst:.3e}, bound {ir.POSITION_BOUND:.3e}")
    assert worst <= ir.POSITION_BOUND
    assert worst <= 0.1 * ir.POSITION_BOUND
    ir.check_pool(pool, bm, cast, rec, name="known answers (host)")


def test_host_box_pool(host, cast_host, orc):
    """320 lifted stacks: 300 computed, all impacts, n_points 1/2/3/4 = 216/0/0/84, none undecided."""
    pool, bm = ir.lifted_box_pool()
    assert not (orc.gjkepa_batch(pool, 2, 1.0)["collision"] != 0).any()       # lifted apart: nothing to skip
    cast = cast_host(pool, bm, ir.TAU)
    rec = host(pool, bm, cast, ir.MARGIN)
    comp, hist = ir.check_pool(pool, bm, cast, rec, name="box pool (host)")
    assert hist.sum() >= 100 and hist[4] >= 30, hist
    # fp32 storage of values that fp32 holds exactly, and fp64 storage of the same values: the same bytes
    p32 = pool.as_dtype(np.float32)
    c32 = cast_host(p32, bm, ir.TAU)
    assert host(p32, bm, c32, ir.MARGIN).tobytes() == host(p32.as_dtype(np.float64), bm, c32, ir.MARGIN).tobytes()


def test_host_tier_boundary_pool(host, cast_host):
    """49 pairs of sizes 1, 4, 32, 33, 128, 129, 256: 49 computed impacts, every bracket covered."""
    pool, bm = ir.boundary_pool()
    cast = cast_host(pool, bm, ir.TAU)
    rec = host(pool, bm, cast, ir.MARGIN)
    comp, _ = ir.check_pool(pool, bm, cast, rec, name="tier-boundary pool (host)")
    ir.check_brackets(pool, comp)
    assert host(pool.as_dtype(np.float64), bm, cast, ir.MARGIN).tobytes() == rec.tobytes()


def hand_records():
    """two unit cubes, B 0.5 above A, and an IMPACT record for them as a cast would leave it at toi 0.25"""
    pool = gjkepa.HullPool.from_pairs([(rr.CUBE, rr.CUBE + [0.25, 0.25, 1.5])])
    bm = np.array([rr.STILL + [0.5, 0.5, 0.5], [0, 0, -2.0, 0, 0, 0.3, 0.75, 0.75, 2.0]], float)
    c = np.zeros(1, gjkepa.CAST64)
    c["toi"], c["normal"], c["flags"], c["code"] = 0.25 - 2.5e-4, [0, 0, -1.0], IMPACT, 0xFFFFFFFF
    c["point_a"], c["point_b"] = [0.5, 0.5, 1.0], [0.5, 0.5, 1.0005]
    return pool, bm, c


def edit(c, **kw):
    c = c.copy()
    for k, v in kw.items():
        c[k] = v
    return c


def test_host_rule_order(host, orc):
    pool, bm, c = hand_records()
    good = host(pool, bm, c, ir.MARGIN)[0]
    assert good["status"] == OK and good["flags"] == ir.AT_TOI and good["n_points"] == 4, good
    assert 0.5 < good["area"] < 0.6 and -ir.TAU <= good["depth"] < 0
    nan_bm = bm.copy()
    nan_bm[1, 4] = np.nan
    # 2. a SKIPPED pair: computed from its contact record, NaN motion or not; NO_HIT without records
    touching = gjkepa.HullPool.from_pairs([(rr.CUBE, rr.CUBE + [0.25, 0.25, 0.99])])
    contact = orc.gjkepa_batch(touching, 2, 1.0)
    assert contact["collision"][0] != 0
    r = host(touching, nan_bm, ir.skipped(), ir.MARGIN, contact)[0]
    assert r["status"] == OK and r["flags"] == 0 and r["n_points"] == 4, r
    ir.check_empty(host(touching, nan_bm, ir.skipped(), ir.MARGIN), OK, ir.NO_HIT)
    # SKIPPED wins over a BAD_INPUT or CAST_MAXITER status in the same record
    sk = edit(ir.skipped(), status=BAD)
    assert host(touching, nan_bm, sk, ir.MARGIN, contact).tobytes() == r.tobytes()
    # 3., 4., 6.
    ir.check_empty(host(pool, bm, edit(c, status=BAD), ir.MARGIN), BAD, 0)
    ir.check_empty(host(pool, bm, edit(c, status=MAXITER, flags=0), ir.MARGIN), OK, ir.NO_HIT)
    ir.check_empty(host(pool, bm, edit(c, status=MAXITER), ir.MARGIN), OK, ir.NO_HIT)
    ir.check_empty(host(pool, bm, edit(c, flags=0, toi=1.0), ir.MARGIN), OK, ir.NO_HIT)                 # a MISS
    ir.check_empty(host(pool, bm, edit(c, flags=START, toi=0.0, normal=[0, 0, 0]), ir.MARGIN), OK, ir.NO_HIT)   # overlapping
    ir.check_empty(host(pool, bm, edit(c, normal=[0, np.nan, -1]), ir.MARGIN), OK, ir.NO_HIT)
    # a separated START is computed at t = 0
    s = host(pool, bm, edit(c, flags=START, toi=0.0), ir.MARGIN)[0]
    assert s["status"] == OK and s["flags"] == ir.AT_TOI and abs(s["depth"] + 0.5) <= 1e-15, s
    # 5. the values of a computed pair
    for toi in (np.nan, 1.5, -0.1):
        ir.check_empty(host(pool, bm, edit(c, toi=toi), ir.MARGIN), BAD, 0)
    ir.check_empty(host(pool, nan_bm, c, ir.MARGIN), BAD, 0)
    inf_bm = bm.copy()
    inf_bm[0, 8] = np.inf
    ir.check_empty(host(pool, inf_bm, c, ir.MARGIN), BAD, 0)
    verts = pool.verts.copy()
    verts[int(pool.hull_off[1]) + 5] = np.nan
    ir.check_empty(host(gjkepa.HullPool(verts, pool.hull_off, pool.hull_cnt, pool.pairs), bm, c, ir.MARGIN), BAD, 0)
    # 1. a bad count beats all of these
    for cnt in (0, 257):
        bad = gjkepa.HullPool(pool.verts, pool.hull_off, np.array([8, cnt], np.int32), pool.pairs)
        for rec, mot, con in ((c, bm, None), (ir.skipped(), nan_bm, contact), (edit(c, status=MAXITER), bm, None),
                              (edit(c, flags=0), bm, None), (edit(c, toi=np.nan), nan_bm, None)):
            ir.check_empty(host(bad, mot, rec, ir.MARGIN, con), BAD, 0)


def test_host_skipped_pairs_equal_the_contact_manifold(host, cast_host, manifold_host, orc):
    """a pool of stacks in contact and lifted stacks together: with the batch's records the SKIPPED pairs get the
    bytes tests/manifold_host.cpp gives for the same contact records, in both record precisions"""
    stacks = mr.box_pool(n=60)
    lifted, bm_l = ir.lifted_box_pool(n=60, seed=0x5C1D)
    hulls = [(stacks.hull(int(a)), stacks.hull(int(b))) for a, b in stacks.pairs] + \
            [(lifted.hull(int(a)), lifted.hull(int(b))) for a, b in lifted.pairs]
    pool = gjkepa.HullPool.from_pairs(hulls)
    bm = np.concatenate([rr.motions(stacks, 0x77), bm_l])
    contact = orc.gjkepa_batch(pool, 2, 1.0)
    cast = ir.skip_hits(cast_host(pool, bm, ir.TAU), contact)
    sk = (cast["flags"] & SKIPPED) != 0
    assert sk.sum() >= 50 and (~sk).sum() >= 50
    c32 = np.zeros(len(contact), gjkepa.REC32)
    for f in contact.dtype.names:
        if f != "pad":
            c32[f] = contact[f]
    for con in (contact, c32):
        rec = host(pool, bm, cast, ir.MARGIN, con)
        want = manifold_host(pool, con, ir.MARGIN)
        assert rec[sk].tobytes() == want[sk].tobytes()
        assert ((rec["flags"][sk] & ir.AT_TOI) == 0).all() and (rec["n_points"][sk] >= 1).sum() >= 50
        assert (want["flags"][~sk] == ir.NO_HIT).all()
    # without the records the same pairs are NO_HIT, and the others do not change
    bare = host(pool, bm, cast, ir.MARGIN)
    ir.check_empty(bare[sk], OK, ir.NO_HIT)
    assert bare[~sk].tobytes() == rec[~sk].tobytes()
