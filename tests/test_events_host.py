"""The event record's definition (include/gjkepa.h gjkepa_events_device, csrc/event_record.h) without a GPU: the
header's text, compiled for the host (tests/events_host.cpp), gives the bytes of the numpy restatement
(tests/events_ref.py) on synthetic records that hold every kind, every precedence clash (BAD_INPUT with SKIPPED,
SKIPPED with MAXITER, MAXITER with START, START with IMPACT), a toi of -0.0, 0, a denormal, NaN, a negative and
an infinite one, and contact records F64, F32 and absent; the restatement's order and clamp hold on a
hand-written case; the record type is 128 bytes in the binding and in the library."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import events_ref as er
import gjkepa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def events_host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("events_host")), "libevents_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    os.path.join(ROOT, "tests", "events_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.events_host.argtypes = [vp, ctypes.c_int64, vp, vp, ctypes.c_int, vp, vp, vp, vp]

    def run(pairs, cast, records=None):
        n = len(cast)
        prs = np.ascontiguousarray(pairs, np.int32).reshape(-1)
        cast = np.ascontiguousarray(cast)
        rec = None if records is None else np.ascontiguousarray(records)
        prec = gjkepa.PREC_F32 if rec is not None and rec.dtype == gjkepa.REC32 else gjkepa.PREC_F64
        kind, key = np.zeros(n, np.int8), np.zeros(n, np.uint64)
        out, counts = np.zeros(n, gjkepa.EVENT64), np.zeros(5, np.int64)
        assert lib.events_host(prs.ctypes.data, n, cast.ctypes.data, None if rec is None else rec.ctypes.data, prec,
                               kind.ctypes.data, key.ctypes.data, out.ctypes.data, counts.ctypes.data) == 0
        return kind, key, out, counts
    return run


def batch(seed):
    """the edge records followed by 3 000 random ones of every kind, with an unsorted pair list"""
    rng = np.random.default_rng(seed)
    pairs, cast = er.edge_records(rng)
    more = er.synth_cast(rng, rng.choice([er.NONE, er.HIT, er.START, er.IMPACT, er.UNDECIDED, er.BAD], size=3000))
    more_pairs = rng.integers(0, 500, size=(3000, 2)).astype(np.int32)
    return np.concatenate([pairs, more_pairs]), np.concatenate([cast, more])


def test_restatement_classifies_the_edge_records_as_the_issue_lists_them():
    pairs, cast = er.edge_records(np.random.default_rng(1))
    kind, ev = er.fill(pairs, cast)
    assert kind.tolist() == er.EDGE_KINDS
    t = dict(zip(range(len(cast)), ev["time"]))
    assert t[8] == 0.0 and t[9] == 0.6 and t[10] == 0.7 and t[11] == 0.0 and t[12] == 0.0      # the clashes
    assert t[15] == er.DENORMAL and t[18] == np.inf and t[21] == er.DENORMAL and t[22] == 0.0
    zero = [13, 14, 16, 17, 19, 20, 23]
    assert (ev["time"][zero].view(np.uint64) == 0).all()                                       # +0.0, never -0.0 or NaN
    assert (ev["time"].view(np.uint64)[kind > 0] <= np.float64(np.inf).view(np.uint64)).all()


def test_restatement_orders_and_clamps_a_hand_written_case():
    """five pairs over four hulls: IMPACT at 0.5 (0, 1), START (1, 2), IMPACT at 0.25 (2, 1), MISS (0, 3), HIT (3, 0)"""
    cast = er.synth_cast(np.random.default_rng(2), [er.IMPACT, er.START, er.IMPACT, er.NONE, er.HIT],
                         toi=[0.5, 0.0, 0.25, 1.0, 0.0])
    pairs = np.array([[0, 1], [1, 2], [2, 1], [0, 3], [3, 0]], np.int32)
    events, n, counts, body_time, body_event = er.reference(pairs, cast, 5)
    assert n == 4 and counts.tolist() == [1, 1, 2, 0, 0]
    assert events["pair"].tolist() == [1, 4, 2, 0] and events["kind"].tolist() == [er.START, er.HIT, er.IMPACT, er.IMPACT]
    assert body_event.tolist() == [3, 2, 2, -1, -1] and body_time.tolist() == [0.5, 0.25, 0.25, 1.0, 1.0]


@needs_gxx
@pytest.mark.parametrize("records", ["none", "f64", "f32"])
def test_header_text_gives_the_restatements_bytes(events_host, records):
    pairs, cast = batch(7)
    rng = np.random.default_rng(8)
    rec = {"none": None, "f64": er.synth_contacts(rng, len(cast), gjkepa.PREC_F64),
           "f32": er.synth_contacts(rng, len(cast), gjkepa.PREC_F32)}[records]
    kind, key, out, counts = events_host(pairs, cast, rec)
    want_kind, want = er.fill(pairs, cast, rec)
    assert np.array_equal(kind, want_kind)
    assert kind[:len(er.EDGE_KINDS)].tolist() == er.EDGE_KINDS
    for k in (er.HIT, er.START, er.IMPACT, er.UNDECIDED, er.BAD, er.NONE):
        assert (kind == k).sum() >= 100
    assert out.tobytes() == want.tobytes()
    on = kind > 0
    assert np.array_equal(key[on], want["time"][on].view(np.uint64)) and (key[~on] == 0xFFFFFFFFFFFFFFFF).all()
    assert counts.tolist() == er.reference(pairs, cast, 1000, rec)[2].tolist()
    hit = kind == er.HIT
    if rec is None:
        assert (out["normal"][hit] == 0).all() and (out["depth"][hit] == 0).all() and (out["status"][hit] == 0).all()
    else:
        assert np.array_equal(out["depth"][hit], rec["penetration_depth"][hit].astype(np.float64)) and (out["depth"][~hit] == 0).all()
        assert np.array_equal(out["point_b"][hit], rec["nearest_points"][hit, 3:6].astype(np.float64))
    assert out["point_a"][kind == er.IMPACT].tobytes() == cast["point_a"][kind == er.IMPACT].tobytes()


def test_record_sizes(lib):
    assert gjkepa.EVENT64.itemsize == 128 == lib.gjkepa_event_record_bytes()
    assert gjkepa.event_dtype is gjkepa.EVENT64
    assert gjkepa.EVENT64.fields["a"][1] == 88 and gjkepa.EVENT64.fields["kind"][1] == 100
