"""Python host binding of the MI355X GJK/EPA C-ABI (include/gjkepa.h) via ctypes.

Mirrors the reference's operator interface: ``gjkepa(version, tol_ff, p1, p2)`` answers one
pair exactly like ``CALL GJKEPA(version_, TOL_FF_, p1_, p2_, ...)`` in
src/GCLIB_GJKEPA.f90:39-52 (same argument meaning; p1/p2 are (n, 3) vertex arrays) and returns
the reference's INTENT(OUT) arguments.  ``gjkepa_batch`` runs a pooled hull set; the
``*_device`` form takes device pointers (e.g. torch tensors on cuda) and an optional stream.

There is no CPU fallback: importing works without a GPU (so the library can be inspected),
but every compute call goes to libgjkepa_hip.so and fails loudly if it cannot run.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "build", "libgjkepa_hip.so")
FLIB_PATH = os.path.join(_HERE, "build", "libgclib_gjkepa.so")

STATUS_OK, STATUS_EPA_MAXITER, STATUS_DEGENERATE, STATUS_BAD_VERSION, STATUS_BAD_INPUT = 0, 1, 2, 3, 4
STATUS_DIST_MAXITER = 5                      # distance records only (gjkepa_distance_batch)
DIST_OVERLAP, DIST_HIT, DIST_FAR = 1, 2, 4   # distance record flag bits
STATUS_CAST_MAXITER = 6                      # cast records only (gjkepa_cast_batch)
CAST_IMPACT, CAST_START, CAST_SKIPPED = 1, 2, 4   # cast record flag bits (a miss has none)
MANIFOLD_NO_HIT, MANIFOLD_DECIMATED, MANIFOLD_FALLBACK = 1, 2, 4   # manifold record flag bits
MANIFOLD_AT_TOI = 8                          # built from a cast record, on the hulls posed at its toi (manifold_cast_batch)
MANIFOLD_MAX_FEATURE = 32                    # feature vertices used per hull (gjkepa_manifold_batch)
DTYPE_F32, DTYPE_F64 = 0, 1
PREC_F32, PREC_F64 = 0, 1
MAX_HULL_VERTS = 256
MOTION_DOUBLES = 9                           # a body's motion over the step: v[3], w[3], c[3] (gjkepa_cast_rigid_batch)

# exported symbols declared in include/gjkepa.h
EXPORTS = (
    "gjkepa_record_bytes", "gjkepa_query", "gjkepa_batch", "gjkepa_workspace_bytes",
    "gjkepa_batch_device", "gjkepa_last_error", "gjkepa_version_string", "gjkepa_synth_pairs",
    "gjkepa_hull_face_capacity", "gjkepa_hull_batch", "gjkepa_hull_batch_device", "gjkepa_synth_clouds",
    "gjkepa_broadphase_workspace_bytes", "gjkepa_broadphase", "gjkepa_broadphase_device", "gjkepa_synth_scene",
    "gjkepa_compact_workspace_bytes", "gjkepa_compact_hits_device", "gjkepa_batch_warm_device",
    "gjkepa_collide", "gjkepa_shard_range", "gjkepa_batch_multi", "gjkepa_comm_unique_id", "gjkepa_comm_init",
    "gjkepa_comm_destroy", "gjkepa_comm_backend", "gjkepa_allgather_records_device",
    "gjkepa_query_service_stop", "gjkepa_query_service_set", "gjkepa_query_service_resident", "gjkepa_workspace_bytes_for",
    "gjkepa_launch_timing", "gjkepa_launch_timing_read",
    "gjkepa_distance_record_bytes", "gjkepa_distance_workspace_bytes", "gjkepa_distance_batch_device",
    "gjkepa_distance_batch",
    "gjkepa_cast_record_bytes", "gjkepa_cast_workspace_bytes", "gjkepa_cast_batch_device", "gjkepa_cast_batch",
    "gjkepa_cast_rigid_workspace_bytes", "gjkepa_cast_rigid_batch_device", "gjkepa_cast_rigid_batch",
    "gjkepa_pose_pool_device", "gjkepa_pose_pool",
    "gjkepa_manifold_record_bytes", "gjkepa_manifold_workspace_bytes", "gjkepa_manifold_batch_device",
    "gjkepa_manifold_batch",
    "gjkepa_broadphase_swept_workspace_bytes", "gjkepa_broadphase_swept_device", "gjkepa_broadphase_swept",
    "gjkepa_event_record_bytes", "gjkepa_events_workspace_bytes", "gjkepa_events_device", "gjkepa_collide_moving",
    "gjkepa_mass_record_bytes", "gjkepa_mass_batch_device", "gjkepa_mass_batch", "gjkepa_mass_pool",
    "gjkepa_manifold_cast_workspace_bytes", "gjkepa_manifold_cast_batch_device", "gjkepa_manifold_cast_batch",
    "gjkepa_event_manifolds_device", "gjkepa_collide_moving_patches",
)
COMM_ID_BYTES = 128
# workspace header word counting the park slots a gjkepa_batch_device call took (diagnostics; csrc/
# gjkepa_capi.cpp kWsParkWord = GJKEPA_WS_COUNTERS + GJKEPA_WS_TALLY)
WS_COUNTERS, WS_TALLY = 40, 48   # gjkepa_kernel.h GJKEPA_WS_COUNTERS / GJKEPA_WS_TALLY (uint32 words)
WS_PARK_WORD = WS_COUNTERS + WS_TALLY
HULL_MAX_POINTS = 256

REC64 = np.dtype([
    ("penetration_depth", "<f8"), ("collision_normal", "<f8", (3,)), ("collision_point", "<f8", (3,)),
    ("nearest_points", "<f8", (6,)), ("collision", "i1"), ("colli_type", "i1"), ("status", "i1"),
    ("reserved", "i1"), ("diag", "<u4"), ("pad", "<u4", (4,)),
])
REC32 = np.dtype([
    ("penetration_depth", "<f4"), ("collision_normal", "<f4", (3,)), ("collision_point", "<f4", (3,)),
    ("nearest_points", "<f4", (6,)), ("collision", "i1"), ("colli_type", "i1"), ("status", "i1"),
    ("reserved", "i1"), ("diag", "<u4"), ("pad", "<u4"),
])
assert REC64.itemsize == 128 and REC32.itemsize == 64
# gjkepa_distance_f64 (include/gjkepa.h): one per pair from distance_batch / distance_batch_device
DIST64 = np.dtype([
    ("distance", "<f8"), ("point_a", "<f8", (3,)), ("point_b", "<f8", (3,)), ("normal", "<f8", (3,)),
    ("lambda", "<f8", (3,)), ("code", "<u4", (3,)), ("n_simplex", "i1"), ("status", "i1"), ("flags", "i1"),
    ("reserved", "i1"), ("iters", "<u4"), ("pad", "<u4"),
])
assert DIST64.itemsize == 128
# gjkepa_cast_f64 (include/gjkepa.h): one per pair from cast_batch / cast_batch_device; the distance
# record's layout with toi for the distance and steps for the pad
CAST64 = np.dtype([
    ("toi", "<f8"), ("point_a", "<f8", (3,)), ("point_b", "<f8", (3,)), ("normal", "<f8", (3,)),
    ("lambda", "<f8", (3,)), ("code", "<u4", (3,)), ("n_simplex", "i1"), ("status", "i1"), ("flags", "i1"),
    ("reserved", "i1"), ("iters", "<u4"), ("steps", "<u4"),
])
assert CAST64.itemsize == 128
# gjkepa_manifold_f64 (include/gjkepa.h): one per pair from manifold_batch / manifold_batch_device
MANIFOLD64 = np.dtype([
    ("depth", "<f8"), ("normal", "<f8", (3,)), ("point", "<f8", (4, 3)), ("code", "<u4", (4,)),
    ("n_feat_a", "<u2"), ("n_feat_b", "<u2"), ("n_points", "i1"), ("status", "i1"), ("flags", "i1"),
    ("reserved", "i1"), ("area", "<f8"),
])
assert MANIFOLD64.itemsize == 160
# gjkepa_event_f64 (include/gjkepa.h): one per event from events / events_device / collide_moving
EVENT_HIT, EVENT_START, EVENT_IMPACT, EVENT_UNDECIDED = 1, 2, 3, 4
EVENT64 = np.dtype([
    ("time", "<f8"), ("point_a", "<f8", (3,)), ("point_b", "<f8", (3,)), ("normal", "<f8", (3,)), ("depth", "<f8"),
    ("a", "<i4"), ("b", "<i4"), ("pair", "<i4"), ("kind", "i1"), ("status", "i1"), ("reserved", "i1", (2,)),
    ("pad", "<u4", (6,)),
])
assert EVENT64.itemsize == 128
event_dtype = EVENT64
# gjkepa_mass_f64 (include/gjkepa.h): one per cloud from mass_batch / mass_batch_device / mass_pool; inertia is
# (Ixx, Iyy, Izz, Ixy, Ixz, Iyz) about com, in world axes, at unit density
MASS64 = np.dtype([
    ("volume", "<f8"), ("area", "<f8"), ("com", "<f8", (3,)), ("inertia", "<f8", (6,)), ("radius", "<f8"),
    ("closure", "<f8"), ("n_faces", "<i4"), ("status", "i1"), ("flags", "i1"), ("reserved", "i1", (2,)),
    ("pad", "<u4", (4,)),
])
assert MASS64.itemsize == 128
EVENTS_TILE = 4096                         # records per block of the event pass's key pass (csrc/events_kernel.h)


def record_dtype(precision: int) -> np.dtype:
    return REC64 if precision == PREC_F64 else REC32


_lib = None


class GjkEpaError(RuntimeError):
    pass


def load(path: str | None = None) -> ctypes.CDLL:
    """Load libgjkepa_hip.so (built in-tree by ``make`` / __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("GJKEPA_LIB") or LIB_PATH
    try:
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 (same soname as
        # /opt/rocm's).  Whichever loads first serves both, and torch's device init fails when it
        # finds the system runtime already mapped, so bring torch's in first when torch is present.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise GjkEpaError(f"{p} not built; run `make -C collision-detect-gjk-epa_amd`")
    lib = ctypes.CDLL(p)
    c_i32, c_i64, c_dbl, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    # the size queries: *_workspace_bytes(n_pairs) -> int64, *_record_bytes(void) -> int
    for q in ("gjkepa", "gjkepa_distance", "gjkepa_cast", "gjkepa_cast_rigid", "gjkepa_manifold", "gjkepa_manifold_cast",
              "gjkepa_compact"):
        fn = getattr(lib, q + "_workspace_bytes")
        fn.argtypes, fn.restype = [c_i64], c_i64
    for q in ("gjkepa_distance", "gjkepa_cast", "gjkepa_manifold"):
        fn = getattr(lib, q + "_record_bytes")
        fn.argtypes, fn.restype = [], ctypes.c_int
    lib.gjkepa_record_bytes.argtypes = [c_i32]
    lib.gjkepa_record_bytes.restype = ctypes.c_int
    lib.gjkepa_last_error.restype = ctypes.c_char_p
    lib.gjkepa_version_string.restype = ctypes.c_char_p
    lib.gjkepa_query.argtypes = [c_i32, c_dbl, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32]
    lib.gjkepa_query.restype = ctypes.c_int
    lib.gjkepa_batch.argtypes = [c_i32, c_dbl, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i32]
    lib.gjkepa_batch.restype = ctypes.c_int
    lib.gjkepa_batch_device.argtypes = [c_i32, c_dbl, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]
    lib.gjkepa_batch_device.restype = ctypes.c_int
    lib.gjkepa_synth_pairs.argtypes = [ctypes.c_uint64, c_i64, c_i64, c_i32, c_i32, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp]
    lib.gjkepa_synth_pairs.restype = c_i64
    lib.gjkepa_hull_face_capacity.argtypes = [c_i32]
    lib.gjkepa_hull_face_capacity.restype = c_i64
    lib.gjkepa_hull_batch.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                      c_vp, c_i32]
    lib.gjkepa_hull_batch.restype = ctypes.c_int
    lib.gjkepa_hull_batch_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                             c_vp]
    lib.gjkepa_hull_batch_device.restype = ctypes.c_int
    lib.gjkepa_synth_clouds.argtypes = [ctypes.c_uint64, c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]
    lib.gjkepa_synth_clouds.restype = c_i64
    lib.gjkepa_broadphase_workspace_bytes.argtypes = [c_i64, c_i64]
    lib.gjkepa_broadphase_workspace_bytes.restype = c_i64
    lib.gjkepa_broadphase.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i32]
    lib.gjkepa_broadphase.restype = ctypes.c_int
    lib.gjkepa_broadphase_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]
    lib.gjkepa_broadphase_device.restype = ctypes.c_int
    lib.gjkepa_broadphase_swept_workspace_bytes.argtypes = [c_i64, c_i64]
    lib.gjkepa_broadphase_swept_workspace_bytes.restype = c_i64
    lib.gjkepa_broadphase_swept.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_dbl, c_dbl, c_vp, c_i64, c_vp, c_i32]
    lib.gjkepa_broadphase_swept.restype = ctypes.c_int
    lib.gjkepa_broadphase_swept_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_dbl, c_dbl, c_vp, c_i64, c_vp, c_vp,
                                                   c_i64, c_vp]
    lib.gjkepa_broadphase_swept_device.restype = ctypes.c_int
    lib.gjkepa_synth_scene.argtypes = [ctypes.c_uint64, c_i64, c_i64, c_i32, c_i32, c_dbl, c_i32, c_vp, c_vp, c_vp]
    lib.gjkepa_synth_scene.restype = c_i64
    lib.gjkepa_compact_hits_device.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]
    lib.gjkepa_compact_hits_device.restype = ctypes.c_int
    lib.gjkepa_batch_warm_device.argtypes = [c_i32, c_dbl, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64,
                                             c_vp, c_vp]
    lib.gjkepa_batch_warm_device.restype = ctypes.c_int
    lib.gjkepa_collide.argtypes = [c_i32, c_dbl, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp,
                                   c_vp, c_i32]
    lib.gjkepa_collide.restype = ctypes.c_int
    lib.gjkepa_shard_range.argtypes = [c_i64, c_i32, c_i32, c_vp, c_vp]
    lib.gjkepa_shard_range.restype = ctypes.c_int
    lib.gjkepa_batch_multi.argtypes = [c_i32, c_dbl, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp,
                                       c_vp, c_i32]
    lib.gjkepa_batch_multi.restype = ctypes.c_int
    lib.gjkepa_comm_unique_id.argtypes = [c_vp]
    lib.gjkepa_comm_unique_id.restype = ctypes.c_int
    lib.gjkepa_comm_init.argtypes = [c_vp, c_i32, c_i32, c_vp, c_i32]
    lib.gjkepa_comm_init.restype = ctypes.c_int
    lib.gjkepa_comm_destroy.argtypes = [c_vp]
    lib.gjkepa_comm_destroy.restype = ctypes.c_int
    lib.gjkepa_comm_backend.restype = ctypes.c_char_p
    lib.gjkepa_allgather_records_device.argtypes = [c_vp, c_i32, c_vp, c_vp, c_i64, c_vp]
    lib.gjkepa_allgather_records_device.restype = ctypes.c_int
    lib.gjkepa_query_service_stop.argtypes = [c_i32]
    lib.gjkepa_query_service_stop.restype = ctypes.c_int
    lib.gjkepa_query_service_set.argtypes = [c_i32]
    lib.gjkepa_query_service_set.restype = ctypes.c_int
    lib.gjkepa_query_service_resident.argtypes = [c_i32]
    lib.gjkepa_query_service_resident.restype = ctypes.c_int
    lib.gjkepa_workspace_bytes_for.argtypes = [c_i64, c_i64]
    lib.gjkepa_workspace_bytes_for.restype = c_i64
    lib.gjkepa_launch_timing.argtypes = [c_i32]
    lib.gjkepa_launch_timing.restype = ctypes.c_int
    lib.gjkepa_launch_timing_read.argtypes = [c_vp, c_i32]
    lib.gjkepa_launch_timing_read.restype = ctypes.c_int
    lib.gjkepa_distance_batch_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i32, c_dbl, c_vp, c_vp,
                                                 c_i64, c_vp]
    lib.gjkepa_distance_batch_device.restype = ctypes.c_int
    lib.gjkepa_distance_batch.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i32, c_dbl, c_vp,
                                          c_i32]
    lib.gjkepa_distance_batch.restype = ctypes.c_int
    lib.gjkepa_cast_batch_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_dbl, c_vp, c_i32, c_vp, c_vp,
                                             c_i64, c_vp]
    lib.gjkepa_cast_batch_device.restype = ctypes.c_int
    lib.gjkepa_cast_batch.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_dbl, c_vp, c_i32, c_vp,
                                      c_i32]
    lib.gjkepa_cast_batch.restype = ctypes.c_int
    lib.gjkepa_cast_rigid_batch_device.argtypes = lib.gjkepa_cast_batch_device.argtypes      # body_motion for motion
    lib.gjkepa_cast_rigid_batch_device.restype = ctypes.c_int
    lib.gjkepa_cast_rigid_batch.argtypes = lib.gjkepa_cast_batch.argtypes
    lib.gjkepa_cast_rigid_batch.restype = ctypes.c_int
    lib.gjkepa_pose_pool_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]
    lib.gjkepa_pose_pool_device.restype = ctypes.c_int
    lib.gjkepa_pose_pool.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32]
    lib.gjkepa_pose_pool.restype = ctypes.c_int
    lib.gjkepa_manifold_batch_device.argtypes = lib.gjkepa_distance_batch_device.argtypes    # margin for max_distance
    lib.gjkepa_manifold_batch_device.restype = ctypes.c_int
    lib.gjkepa_manifold_batch.argtypes = lib.gjkepa_distance_batch.argtypes
    lib.gjkepa_manifold_batch.restype = ctypes.c_int
    lib.gjkepa_manifold_cast_batch_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_dbl,
                                                      c_vp, c_vp, c_i64, c_vp]
    lib.gjkepa_manifold_cast_batch_device.restype = ctypes.c_int
    lib.gjkepa_manifold_cast_batch.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32,
                                               c_dbl, c_vp, c_i32]
    lib.gjkepa_manifold_cast_batch.restype = ctypes.c_int
    lib.gjkepa_event_manifolds_device.argtypes = [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]
    lib.gjkepa_event_manifolds_device.restype = ctypes.c_int
    lib.gjkepa_collide_moving_patches.argtypes = [c_i32, c_dbl, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_dbl,
                                                  c_dbl, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_i32]
    lib.gjkepa_collide_moving_patches.restype = ctypes.c_int
    lib.gjkepa_event_record_bytes.argtypes, lib.gjkepa_event_record_bytes.restype = [], ctypes.c_int
    lib.gjkepa_events_workspace_bytes.argtypes, lib.gjkepa_events_workspace_bytes.restype = [c_i64, c_i64], c_i64
    lib.gjkepa_events_device.argtypes = [c_vp, c_i64, c_i64, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                         c_i64, c_vp]
    lib.gjkepa_events_device.restype = ctypes.c_int
    lib.gjkepa_collide_moving.argtypes = [c_i32, c_dbl, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_dbl, c_dbl,
                                          c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32]
    lib.gjkepa_collide_moving.restype = ctypes.c_int
    lib.gjkepa_mass_record_bytes.argtypes, lib.gjkepa_mass_record_bytes.restype = [], ctypes.c_int
    lib.gjkepa_mass_batch_device.argtypes = [c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
    lib.gjkepa_mass_batch_device.restype = ctypes.c_int
    lib.gjkepa_mass_batch.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32]
    lib.gjkepa_mass_batch.restype = ctypes.c_int
    lib.gjkepa_mass_pool.argtypes = [c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i32]
    lib.gjkepa_mass_pool.restype = ctypes.c_int
    if path is None:
        _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gjkepa_last_error().decode(errors="replace")
        raise GjkEpaError(f"{what} failed ({rc}): {msg}")


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


@dataclass
class Contact:
    """GJKEPA's INTENT(OUT) arguments (GCLIB_GJKEPA.f90:47-52) plus the status code."""
    collision: bool
    colli_type: int
    nearest_points: np.ndarray     # (2, 3): row 0 on p1, row 1 on p2
    collision_normal: np.ndarray   # (3,)
    collision_point: np.ndarray    # (3,)
    penetration_depth: float
    status: int


def gjkepa(version: int, tol_ff: float, p1, p2, device: int = 0) -> Contact:
    """One pair on the GPU; same arguments as the reference GJKEPA (p1, p2: (n, 3))."""
    lib = load()
    a = np.ascontiguousarray(np.asarray(p1, dtype=np.float64).T)   # column-major (n,3) = x[], y[], z[]
    b = np.ascontiguousarray(np.asarray(p2, dtype=np.float64).T)
    hit = np.zeros(1, np.int8)
    typ = np.zeros(1, np.int32)
    st = np.zeros(1, np.int32)
    npf = np.zeros(6)
    nrm = np.zeros(3)
    pt = np.zeros(3)
    dep = np.zeros(1)
    rc = lib.gjkepa_query(int(version), float(tol_ff), _ptr(a), a.shape[1], _ptr(b), b.shape[1],
                          _ptr(hit), _ptr(typ), _ptr(npf), _ptr(nrm), _ptr(pt), _ptr(dep), _ptr(st), int(device))
    _check(rc, "gjkepa_query")
    return Contact(bool(hit[0]), int(typ[0]), npf.reshape(3, 2).T.copy(), nrm, pt, float(dep[0]), int(st[0]))


def query_service_stop(device: int = -1) -> None:
    """Drain the resident grid behind gjkepa() (include/gjkepa.h): call before a device-wide
    synchronisation such as torch.cuda.synchronize() while single-pair calls may have run."""
    _check(load().gjkepa_query_service_stop(int(device)), "gjkepa_query_service_stop")


def query_service_resident(device: int = -1) -> bool:
    """Whether a resident service grid is still on the GPU (gjkepa_query_service_resident)."""
    rc = load().gjkepa_query_service_resident(int(device))
    _check(min(rc, 0), "gjkepa_query_service_resident")
    return rc == 1


def query_service_set(enabled: bool) -> bool:
    """Turn the resident query service on/off for later gjkepa() calls; returns the previous setting."""
    rc = load().gjkepa_query_service_set(1 if enabled else 0)
    if rc < 0:
        _check(rc, "gjkepa_query_service_set")
    return bool(rc)


@dataclass
class HullPool:
    """Pooled hulls: hull h = verts[off[h] : off[h] + 3*cnt[h]] as x[], y[], z[]."""
    verts: np.ndarray    # float32 or float64
    hull_off: np.ndarray  # int64
    hull_cnt: np.ndarray  # int32
    pairs: np.ndarray     # int32 (n_pairs, 2)

    @property
    def n_pairs(self) -> int:
        return int(self.pairs.shape[0])

    @property
    def dtype_code(self) -> int:
        return DTYPE_F32 if self.verts.dtype == np.float32 else DTYPE_F64

    def hull(self, h: int) -> np.ndarray:
        o, n = int(self.hull_off[h]), int(self.hull_cnt[h])
        return self.verts[o:o + 3 * n].reshape(3, n).T.astype(np.float64)

    def as_dtype(self, dt) -> "HullPool":
        return HullPool(self.verts.astype(dt), self.hull_off, self.hull_cnt, self.pairs)

    @staticmethod
    def from_pairs(pairs_list, dtype=np.float64) -> "HullPool":
        """Build a pool from a list of (p1, p2) (n,3) arrays."""
        chunks, off, cnt, pr = [], [], [], []
        o = 0
        for k, (a, b) in enumerate(pairs_list):
            for h in (a, b):
                h = np.asarray(h, dtype=np.float64).reshape(-1, 3)
                chunks.append(h.T.reshape(-1))
                off.append(o)
                cnt.append(h.shape[0])
                o += 3 * h.shape[0]
            pr.append((2 * k, 2 * k + 1))
        verts = np.concatenate(chunks).astype(dtype) if chunks else np.zeros(0, dtype)
        return HullPool(verts, np.asarray(off, np.int64), np.asarray(cnt, np.int32),
                        np.asarray(pr, np.int32).reshape(-1, 2))


def synth_pairs(seed: int, n_pairs: int, n_min: int = 32, n_max: int = 32, r_max: float = 2.5,
                first_pair: int = 0, dtype=np.float32) -> HullPool:
    """Deterministic synthetic workload: C2 = (32, 32, 2.5), C4 = (8, 256, 2.5),
    C5 = (32..128, 0.3)."""
    lib = load()
    code = DTYPE_F32 if np.dtype(dtype) == np.float32 else DTYPE_F64
    total = lib.gjkepa_synth_pairs(seed, first_pair, n_pairs, n_min, n_max, r_max, code, None, None, None, None)
    if total < 0:
        raise GjkEpaError("gjkepa_synth_pairs: bad arguments")
    verts = np.empty(total, dtype=dtype)
    off = np.empty(2 * n_pairs, np.int64)
    cnt = np.empty(2 * n_pairs, np.int32)
    prs = np.empty(2 * n_pairs, np.int32)
    lib.gjkepa_synth_pairs(seed, first_pair, n_pairs, n_min, n_max, r_max, code, _ptr(verts), _ptr(off), _ptr(cnt), _ptr(prs))
    return HullPool(verts, off, cnt, prs.reshape(-1, 2))


def _pool_args(pool: HullPool):
    """The pool's contiguous arrays (to be kept alive over the call) and the argument run the pair-list
    host entries share: verts, n_vert_scalars, hull_off, hull_cnt, n_hulls, pairs, n_pairs."""
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    prs = np.ascontiguousarray(pool.pairs, np.int32).reshape(-1)
    return (verts, off, cnt, prs), (_ptr(verts), verts.size, _ptr(off), _ptr(cnt), cnt.size, _ptr(prs), pool.n_pairs)


def _records_arg(records, n_pairs: int):
    """Optional contact records of a pair list: (contiguous array or None, its pointer, its precision)."""
    if records is None:
        return None, None, PREC_F64
    records = np.ascontiguousarray(records)
    if records.dtype not in (REC64, REC32) or records.shape != (n_pairs,):
        raise GjkEpaError("records: one REC64 / REC32 contact record per pair")
    return records, _ptr(records), (PREC_F64 if records.dtype == REC64 else PREC_F32)


def gjkepa_batch(pool: HullPool, version: int = 2, tol_ff: float = 1.0, precision: int = PREC_F64,
                 device: int = 0) -> np.ndarray:
    """Host-buffer batch on the GPU; returns a structured array of contact records."""
    out = np.zeros(pool.n_pairs, dtype=record_dtype(precision))
    keep, pool_args = _pool_args(pool)
    rc = load().gjkepa_batch(int(version), float(tol_ff), pool.dtype_code, int(precision), *pool_args, _ptr(out),
                             int(device))
    _check(rc, "gjkepa_batch")
    return out


def workspace_bytes(n_pairs: int) -> int:
    return int(load().gjkepa_workspace_bytes(n_pairs))


PARK_MIN_HULL = 32   # pairs with a hull above this many vertices can reach the parking EPA tiers


def large_pairs(pool: HullPool) -> int:
    """Pairs of the pool with a hull above PARK_MIN_HULL vertices (gjkepa_workspace_bytes_for)."""
    c = pool.hull_cnt[pool.pairs.astype(np.int64)]
    return int((c.max(axis=1) > PARK_MIN_HULL).sum()) if pool.n_pairs else 0


def workspace_bytes_for(n_pairs: int, n_large_pairs: int) -> int:
    """Workspace with park slots only for the pairs that can park (include/gjkepa.h)."""
    b = int(load().gjkepa_workspace_bytes_for(int(n_pairs), int(n_large_pairs)))
    if b < 0:
        raise GjkEpaError("gjkepa_workspace_bytes_for: bad arguments")
    return b


# per-launch timing of the tier chain (include/gjkepa.h gjkepa_launch_time)
LAUNCH_TIME = np.dtype([
    ("kernel", "S16"), ("tier", "<i4"), ("part", "<i4"), ("route_code", "<i4"), ("chain", "<i4"),
    ("stream", "<i4"), ("pad", "<i4"), ("first_pair", "<i8"), ("n_pairs", "<i8"), ("start_ms", "<f4"),
    ("end_ms", "<f4"),
])
assert LAUNCH_TIME.itemsize == 64


def launch_timing(enable: bool) -> bool:
    """Record HIP events around every kernel launch of the chains this thread enqueues from now on;
    returns the previous setting."""
    return bool(load().gjkepa_launch_timing(1 if enable else 0))


def launch_timing_read(max_launches: int = 1 << 16) -> np.ndarray:
    """Wait for the recorded launches and return them (LAUNCH_TIME records, enqueue order)."""
    buf = np.zeros(max_launches, LAUNCH_TIME)
    n = load().gjkepa_launch_timing_read(_ptr(buf), max_launches)
    if n < 0:
        _check(n, "gjkepa_launch_timing_read")
    return buf[:n]


def gjkepa_batch_device(version: int, tol_ff: float, vert_dtype: int, precision: int, verts_ptr: int,
                        hull_off_ptr: int, hull_cnt_ptr: int, pairs_ptr: int, n_pairs: int, out_ptr: int,
                        ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Device-resident batch (raw device pointers), asynchronous on `stream`."""
    rc = load().gjkepa_batch_device(int(version), float(tol_ff), int(vert_dtype), int(precision), verts_ptr,
                                    hull_off_ptr, hull_cnt_ptr, pairs_ptr, int(n_pairs), out_ptr, ws_ptr,
                                    int(ws_bytes), stream or None)
    _check(rc, "gjkepa_batch_device")


def gjkepa_batch_warm_device(version: int, tol_ff: float, vert_dtype: int, precision: int, verts_ptr: int,
                             hull_off_ptr: int, hull_cnt_ptr: int, pairs_ptr: int, n_pairs: int, out_ptr: int,
                             ws_ptr: int, ws_bytes: int, warm_ptr: int, stream: int = 0) -> None:
    """gjkepa_batch_device with a per-pair warm-start slot array (device uint32[4 * n_pairs], in/out;
    0xFFFFFFFF = none): persistent pairs whose last simplex still encloses the origin skip GJK."""
    rc = load().gjkepa_batch_warm_device(int(version), float(tol_ff), int(vert_dtype), int(precision), verts_ptr,
                                         hull_off_ptr, hull_cnt_ptr, pairs_ptr, int(n_pairs), out_ptr, ws_ptr,
                                         int(ws_bytes), warm_ptr, stream or None)
    _check(rc, "gjkepa_batch_warm_device")


# ---- separation distance of non-colliding pairs (include/gjkepa.h gjkepa_distance_*) -------------------
def distance_workspace_bytes(n_pairs: int) -> int:
    b = int(load().gjkepa_distance_workspace_bytes(int(n_pairs)))
    if b < 0:
        raise GjkEpaError("gjkepa_distance_workspace_bytes: bad arguments")
    return b


def distance_batch(pool: HullPool, records: np.ndarray | None = None, max_distance: float = float("inf"),
                   device: int = 0) -> np.ndarray:
    """Separation distance and closest points of every pair of the pool (host buffers, blocking);
    returns DIST64 records.  records: the pool's contact records (gjkepa_batch output, REC64 or REC32):
    pairs they call a collision are skipped (flag DIST_HIT); None: overlaps are found here (DIST_OVERLAP).
    max_distance: pairs proven farther apart stop early (flag DIST_FAR, distance = the lower bound)."""
    out = np.zeros(pool.n_pairs, dtype=DIST64)
    keep, pool_args = _pool_args(pool)
    records, rec_ptr, rec_prec = _records_arg(records, pool.n_pairs)
    rc = load().gjkepa_distance_batch(pool.dtype_code, *pool_args, rec_ptr, rec_prec, float(max_distance), _ptr(out),
                                      int(device))
    _check(rc, "gjkepa_distance_batch")
    return out


def distance_batch_device(vert_dtype: int, verts_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, pairs_ptr: int,
                          n_pairs: int, records_ptr: int, records_precision: int, max_distance: float, out_ptr: int,
                          ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Device-resident distance query (raw device pointers), asynchronous on `stream`; records_ptr 0 /
    None: no contact records.  Chain it after gjkepa_batch_device on the same stream with that call's
    output as the records."""
    rc = load().gjkepa_distance_batch_device(int(vert_dtype), verts_ptr, hull_off_ptr, hull_cnt_ptr, pairs_ptr,
                                             int(n_pairs), records_ptr or None, int(records_precision),
                                             float(max_distance), out_ptr, ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_distance_batch_device")


# ---- linear cast / time of impact of moving pairs (include/gjkepa.h gjkepa_cast_*) ---------------------
def cast_workspace_bytes(n_pairs: int) -> int:
    b = int(load().gjkepa_cast_workspace_bytes(int(n_pairs)))
    if b < 0:
        raise GjkEpaError("gjkepa_cast_workspace_bytes: bad arguments")
    return b


def cast_batch(pool: HullPool, motion, tolerance: float, records: np.ndarray | None = None,
               device: int = 0) -> np.ndarray:
    """Linear cast of every pair of the pool (host buffers, blocking); returns CAST64 records.
    motion: (n_pairs, 3) float64, hull B's displacement relative to hull A over the step.  tolerance:
    the absolute distance at which the hulls count as meeting (finite, > 0).  Flags: CAST_IMPACT (toi in
    (0, 1)), CAST_START (within tolerance or overlapping at t = 0), none for a miss (toi = 1).
    records: the pool's contact records (gjkepa_batch output): pairs they call a collision are skipped
    (CAST_SKIPPED)."""
    out = np.zeros(pool.n_pairs, dtype=CAST64)
    keep, pool_args = _pool_args(pool)
    mot = np.ascontiguousarray(motion, np.float64).reshape(-1)
    if mot.size != 3 * pool.n_pairs:
        raise GjkEpaError("motion: 3 float64 per pair")
    records, rec_ptr, rec_prec = _records_arg(records, pool.n_pairs)
    rc = load().gjkepa_cast_batch(pool.dtype_code, *pool_args, _ptr(mot), float(tolerance), rec_ptr, rec_prec, _ptr(out),
                                  int(device))
    _check(rc, "gjkepa_cast_batch")
    return out


def cast_batch_device(vert_dtype: int, verts_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, pairs_ptr: int,
                      n_pairs: int, motion_ptr: int, tolerance: float, records_ptr: int, records_precision: int,
                      out_ptr: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Device-resident linear cast (raw device pointers), asynchronous on `stream`; records_ptr 0 /
    None: no contact records.  Chain it after gjkepa_batch_device on the same stream with that call's
    output as the records."""
    rc = load().gjkepa_cast_batch_device(int(vert_dtype), verts_ptr, hull_off_ptr, hull_cnt_ptr, pairs_ptr,
                                         int(n_pairs), motion_ptr, float(tolerance), records_ptr or None,
                                         int(records_precision), out_ptr, ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_cast_batch_device")


# ---- rigid-motion cast and the pose that goes with it (include/gjkepa.h gjkepa_cast_rigid_*, gjkepa_pose_pool*) ----
def cast_rigid_workspace_bytes(n_pairs: int) -> int:
    b = int(load().gjkepa_cast_rigid_workspace_bytes(int(n_pairs)))
    if b < 0:
        raise GjkEpaError("gjkepa_cast_rigid_workspace_bytes: bad arguments")
    return b


def _motion_arg(pool: HullPool, body_motion) -> np.ndarray:
    mot = np.ascontiguousarray(body_motion, np.float64).reshape(-1)
    if mot.size != MOTION_DOUBLES * len(pool.hull_cnt):
        raise GjkEpaError("body_motion: 9 float64 (v, w, c) per hull of the pool")
    return mot


def cast_rigid_batch(pool: HullPool, body_motion, tolerance: float, records: np.ndarray | None = None,
                     device: int = 0) -> np.ndarray:
    """Cast of every pair of the pool with both bodies in rigid motion (host buffers, blocking); returns
    CAST64 records.  body_motion: (n_hulls, 9) float64 per hull of the pool: v, the pivot's displacement
    over the step; w, the rotation vector (angular velocity times the step; |w| = 2 tan(theta / 2) for a
    turn by theta); c, the pivot at t = 0.  tolerance, flags and records as for cast_batch; status
    STATUS_CAST_MAXITER: undecided, toi = the last time certified free.  Move the bodies with pose_pool."""
    out = np.zeros(pool.n_pairs, dtype=CAST64)
    keep, pool_args = _pool_args(pool)
    mot = _motion_arg(pool, body_motion)
    records, rec_ptr, rec_prec = _records_arg(records, pool.n_pairs)
    rc = load().gjkepa_cast_rigid_batch(pool.dtype_code, *pool_args, _ptr(mot), float(tolerance), rec_ptr, rec_prec,
                                        _ptr(out), int(device))
    _check(rc, "gjkepa_cast_rigid_batch")
    return out


def cast_rigid_batch_device(vert_dtype: int, verts_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, pairs_ptr: int,
                            n_pairs: int, body_motion_ptr: int, tolerance: float, records_ptr: int,
                            records_precision: int, out_ptr: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Device-resident rigid-motion cast (raw device pointers; body_motion: 9 doubles per hull),
    asynchronous on `stream`; records_ptr 0 / None: no contact records."""
    rc = load().gjkepa_cast_rigid_batch_device(int(vert_dtype), verts_ptr, hull_off_ptr, hull_cnt_ptr, pairs_ptr,
                                               int(n_pairs), body_motion_ptr, float(tolerance), records_ptr or None,
                                               int(records_precision), out_ptr, ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_cast_rigid_batch_device")


def pose_pool(pool: HullPool, body_motion, time=None, out_dtype=None, device: int = 0, return_status: bool = False):
    """The pool with every hull h moved along its body's path to time[h] (None: t = 1): the pose the
    rigid-motion cast certifies (host buffers, blocking).  out_dtype: float32 / float64 (default: the
    pool's); float64 is the cast's arithmetic exactly.  Hulls with a bad count or a non-finite motion, time
    or vertex keep their vertices; return_status: also return the int8 status per hull."""
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    mot = _motion_arg(pool, body_motion)
    tm = None if time is None else np.ascontiguousarray(time, np.float64).reshape(-1)
    if tm is not None and tm.size != cnt.size:
        raise GjkEpaError("time: one float64 per hull of the pool")
    out = verts.astype(np.dtype(out_dtype or verts.dtype))     # a copy: untouched scalars keep the input's values
    if out.dtype not in (np.float32, np.float64):
        raise GjkEpaError("out_dtype: float32 or float64")
    status = np.zeros(cnt.size, np.int8)
    rc = load().gjkepa_pose_pool(pool.dtype_code, _ptr(verts), verts.size, _ptr(off), _ptr(cnt), cnt.size, _ptr(mot),
                                 None if tm is None else _ptr(tm), DTYPE_F32 if out.dtype == np.float32 else DTYPE_F64,
                                 _ptr(out), _ptr(status), int(device))
    _check(rc, "gjkepa_pose_pool")
    posed = HullPool(out, pool.hull_off, pool.hull_cnt, pool.pairs)
    return (posed, status) if return_status else posed


def pose_pool_device(in_dtype: int, verts_in_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, n_hulls: int,
                     body_motion_ptr: int, time_ptr: int, out_dtype: int, verts_out_ptr: int, status_ptr: int = 0,
                     stream: int = 0) -> None:
    """Device-resident pose (raw device pointers), asynchronous on `stream`; time_ptr 0 / None: t = 1;
    status_ptr 0 / None: no status; verts_out_ptr may be verts_in_ptr when the dtypes are equal."""
    rc = load().gjkepa_pose_pool_device(int(in_dtype), verts_in_ptr, hull_off_ptr, hull_cnt_ptr, int(n_hulls),
                                        body_motion_ptr, time_ptr or None, int(out_dtype), verts_out_ptr,
                                        status_ptr or None, stream or None)
    _check(rc, "gjkepa_pose_pool_device")


# ---- contact manifold of colliding pairs (include/gjkepa.h gjkepa_manifold_*) --------------------------
def manifold_workspace_bytes(n_pairs: int) -> int:
    b = int(load().gjkepa_manifold_workspace_bytes(int(n_pairs)))
    if b < 0:
        raise GjkEpaError("gjkepa_manifold_workspace_bytes: bad arguments")
    return b


def manifold_batch(pool: HullPool, records: np.ndarray, margin: float, device: int = 0) -> np.ndarray:
    """Contact manifold (up to 4 points on hull A's support plane, with feature codes) of every pair of
    the pool its contact records call a collision (host buffers, blocking); returns MANIFOLD64 records.
    records: the pool's contact records (gjkepa_batch output, REC64 or REC32), required.  margin: the
    thickness of the two features, an absolute length (finite, >= 0).  Every other pair: MANIFOLD_NO_HIT."""
    if records is None:
        raise GjkEpaError("records: one REC64 / REC32 contact record per pair")
    out = np.zeros(pool.n_pairs, dtype=MANIFOLD64)
    keep, pool_args = _pool_args(pool)
    records, rec_ptr, rec_prec = _records_arg(records, pool.n_pairs)
    rc = load().gjkepa_manifold_batch(pool.dtype_code, *pool_args, rec_ptr, rec_prec, float(margin), _ptr(out),
                                      int(device))
    _check(rc, "gjkepa_manifold_batch")
    return out


def manifold_batch_device(vert_dtype: int, verts_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, pairs_ptr: int,
                          n_pairs: int, records_ptr: int, records_precision: int, margin: float, out_ptr: int,
                          ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Device-resident contact manifold (raw device pointers), asynchronous on `stream`.  Chain it after
    gjkepa_batch_device on the same stream with that call's output as the records."""
    rc = load().gjkepa_manifold_batch_device(int(vert_dtype), verts_ptr, hull_off_ptr, hull_cnt_ptr, pairs_ptr,
                                             int(n_pairs), records_ptr or None, int(records_precision),
                                             float(margin), out_ptr, ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_manifold_batch_device")


# ---- contact manifold at the time of impact (include/gjkepa.h gjkepa_manifold_cast_*) -------------------
def manifold_cast_workspace_bytes(n_pairs: int) -> int:
    b = int(load().gjkepa_manifold_cast_workspace_bytes(int(n_pairs)))
    if b < 0:
        raise GjkEpaError("gjkepa_manifold_cast_workspace_bytes: bad arguments")
    return b


def _cast_records_arg(cast_records, n_pairs: int) -> np.ndarray:
    cast = np.ascontiguousarray(cast_records)
    if cast.dtype != CAST64 or cast.shape != (n_pairs,):
        raise GjkEpaError("cast_records: one CAST64 record per pair")
    return cast


def manifold_cast_batch(pool: HullPool, body_motion, cast_records, margin: float, records: np.ndarray | None = None,
                        device: int = 0) -> np.ndarray:
    """Contact manifold of every pair of the pool at its own time of impact (host buffers, blocking); returns
    MANIFOLD64 records.  cast_records: the pool's CAST64 records from cast_rigid_batch; body_motion: the
    (n_hulls, 9) blocks that cast ran with.  An IMPACT or START pair gets the manifold of the two hulls posed at
    its toi along the cast's normal, with flag MANIFOLD_AT_TOI; a pair the cast skipped as a hit gets what
    manifold_batch gives it from `records` (MANIFOLD_NO_HIT without records); a miss or an undecided pair
    MANIFOLD_NO_HIT.  margin as for manifold_batch."""
    out = np.zeros(pool.n_pairs, dtype=MANIFOLD64)
    keep, pool_args = _pool_args(pool)
    mot = _motion_arg(pool, body_motion)
    cast = _cast_records_arg(cast_records, pool.n_pairs)
    records, rec_ptr, rec_prec = _records_arg(records, pool.n_pairs)
    rc = load().gjkepa_manifold_cast_batch(pool.dtype_code, *pool_args, _ptr(mot), _ptr(cast), rec_ptr, rec_prec,
                                           float(margin), _ptr(out), int(device))
    _check(rc, "gjkepa_manifold_cast_batch")
    return out


def manifold_cast_batch_device(vert_dtype: int, verts_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, pairs_ptr: int,
                               n_pairs: int, body_motion_ptr: int, cast_records_ptr: int, records_ptr: int,
                               records_precision: int, margin: float, out_ptr: int, ws_ptr: int, ws_bytes: int,
                               stream: int = 0) -> None:
    """Device-resident manifold at the time of impact (raw device pointers), asynchronous on `stream`.  Chain it
    after cast_rigid_batch_device with that call's output as the cast records; records_ptr 0 / None: no contact
    records."""
    rc = load().gjkepa_manifold_cast_batch_device(int(vert_dtype), verts_ptr, hull_off_ptr, hull_cnt_ptr, pairs_ptr,
                                                  int(n_pairs), body_motion_ptr or None, cast_records_ptr or None,
                                                  records_ptr or None, int(records_precision), float(margin), out_ptr,
                                                  ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_manifold_cast_batch_device")


# ---- multi-GPU (SURVEY.md §8 row e; include/gjkepa.h gjkepa_shard_range / _batch_multi / _comm_*) ------
def shard_range(n_pairs: int, world: int, rank: int) -> tuple[int, int]:
    """(first, count): the contiguous shard of pairs `rank` of `world` owns (the library's rule)."""
    first, count = ctypes.c_int64(), ctypes.c_int64()
    _check(load().gjkepa_shard_range(int(n_pairs), int(world), int(rank), ctypes.byref(first), ctypes.byref(count)),
           "gjkepa_shard_range")
    return first.value, count.value


def gjkepa_batch_multi(pool: HullPool, devices, version: int = 2, tol_ff: float = 1.0,
                       precision: int = PREC_F64) -> np.ndarray:
    """One process driving several devices: pool's pairs in contiguous shards, shard s on devices[s];
    returns every record in pair order (bit-identical to gjkepa_batch)."""
    out = np.zeros(pool.n_pairs, dtype=record_dtype(precision))
    keep, pool_args = _pool_args(pool)
    dev = np.ascontiguousarray(devices, np.int32)
    rc = load().gjkepa_batch_multi(int(version), float(tol_ff), pool.dtype_code, int(precision), *pool_args, _ptr(out),
                                   _ptr(dev), dev.size)
    _check(rc, "gjkepa_batch_multi")
    return out


class Comm:
    """RCCL communicator of the contact-record exchange, one process per device (config C3).
    Rank 0 calls ``Comm.unique_id()``; the caller broadcasts those bytes (e.g. torch.distributed);
    every rank then builds ``Comm(world, rank, uid, device)``."""

    def __init__(self, world: int, rank: int, uid: bytes, device: int):
        if len(uid) != COMM_ID_BYTES:
            raise GjkEpaError("unique id must be COMM_ID_BYTES bytes")
        self.world, self.rank, self.device = world, rank, device
        self._h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        _check(load().gjkepa_comm_init(ctypes.byref(self._h), int(world), int(rank), buf, int(device)),
               "gjkepa_comm_init")

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        _check(load().gjkepa_comm_unique_id(buf), "gjkepa_comm_unique_id")
        return buf.raw

    @staticmethod
    def backend() -> str:
        return load().gjkepa_comm_backend().decode()

    def allgather_records(self, precision: int, shard_ptr: int, all_ptr: int, count: int, stream: int = 0) -> None:
        """Every rank's `count` records (device pointer) into all_ptr[world * count], rank order; async."""
        _check(load().gjkepa_allgather_records_device(self._h, int(precision), shard_ptr, all_ptr, int(count),
                                                      stream or None), "gjkepa_allgather_records_device")

    def close(self) -> None:
        if self._h:
            _check(load().gjkepa_comm_destroy(self._h), "gjkepa_comm_destroy")
            self._h = ctypes.c_void_p()


def version_string() -> str:
    return load().gjkepa_version_string().decode()


def source_hash() -> str:
    """The hash of the sources the loaded library was built from (Makefile SRCHASH)."""
    return version_string().rsplit("src ", 1)[-1].strip()


# ---- batched convex hulls (include/gjkepa.h gjkepa_hull_batch) ----------------
@dataclass
class CloudPool:
    """Pooled point clouds: cloud c = verts[off[c] : off[c] + 3*cnt[c]] as x[], y[], z[]."""
    verts: np.ndarray      # float32 or float64
    cloud_off: np.ndarray  # int64
    cloud_cnt: np.ndarray  # int32

    @property
    def n_clouds(self) -> int:
        return int(self.cloud_cnt.shape[0])

    @property
    def dtype_code(self) -> int:
        return DTYPE_F32 if self.verts.dtype == np.float32 else DTYPE_F64

    def cloud(self, c: int) -> np.ndarray:
        o, n = int(self.cloud_off[c]), int(self.cloud_cnt[c])
        return self.verts[o:o + 3 * n].reshape(3, n).T.astype(np.float64)

    @staticmethod
    def from_list(clouds, dtype=np.float64) -> "CloudPool":
        chunks, off, cnt, o = [], [], [], 0
        for p in clouds:
            p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
            chunks.append(p.T.reshape(-1))
            off.append(o)
            cnt.append(p.shape[0])
            o += 3 * p.shape[0]
        verts = np.concatenate(chunks).astype(dtype) if chunks else np.zeros(0, dtype)
        return CloudPool(verts, np.asarray(off, np.int64), np.asarray(cnt, np.int32))


def hull_face_offsets(cloud_cnt) -> np.ndarray:
    """Triangle offset of each cloud's face block (exclusive prefix sum of 2n - 4, 0 for n < 4)."""
    cnt = np.asarray(cloud_cnt, np.int64)
    cap = np.where(cnt >= 4, 2 * cnt - 4, 0)
    off = np.zeros(len(cap), np.int64)
    if len(cap) > 1:
        off[1:] = np.cumsum(cap)[:-1]
    return off


def synth_clouds(seed: int, n_clouds: int, n_min: int = 64, n_max: int = 64, shape: int = 0,
                 first_cloud: int = 0, dtype=np.float32) -> CloudPool:
    """Deterministic synthetic clouds: uniform in the unit ball (shape 0) or on the sphere (shape 1)."""
    lib = load()
    code = DTYPE_F32 if np.dtype(dtype) == np.float32 else DTYPE_F64
    total = lib.gjkepa_synth_clouds(seed, first_cloud, n_clouds, n_min, n_max, shape, code, None, None, None)
    if total < 0:
        raise GjkEpaError("gjkepa_synth_clouds: bad arguments")
    verts = np.empty(total, dtype=dtype)
    off = np.empty(n_clouds, np.int64)
    cnt = np.empty(n_clouds, np.int32)
    lib.gjkepa_synth_clouds(seed, first_cloud, n_clouds, n_min, n_max, shape, code, _ptr(verts), _ptr(off), _ptr(cnt))
    return CloudPool(verts, off, cnt)


def hull_batch(pool: CloudPool, device: int = 0) -> dict:
    """Convex hull of every cloud on the GPU (host buffers, blocking).  Returns faces (int32
    [sum(2n-4), 3], cloud c's n_faces[c] triangles at face_off[c]), face_off, n_faces, n_verts,
    status, hull_verts (pool layout: cloud c's hull at cloud_off[c], stride n_verts[c]) and
    vert_idx (cloud c's hull vertex indices at cloud_off[c])."""
    lib = load()
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.cloud_off, np.int64)
    cnt = np.ascontiguousarray(pool.cloud_cnt, np.int32)
    n = cnt.size
    foff = hull_face_offsets(cnt)
    nslots = int(foff[-1] + max(2 * int(cnt[-1]) - 4, 0)) if n else 0
    faces = np.full((max(nslots, 1), 3), -1, np.int32)
    nf = np.zeros(n, np.int32)
    nv = np.zeros(n, np.int32)
    st = np.zeros(n, np.int8)
    hv = np.zeros_like(verts)
    vi = np.full(verts.size, -1, np.int32)
    rc = lib.gjkepa_hull_batch(pool.dtype_code, _ptr(verts), verts.size, _ptr(off), _ptr(cnt), n, _ptr(foff), nslots,
                               _ptr(faces), _ptr(nf), _ptr(nv), _ptr(st), _ptr(hv), _ptr(vi), int(device))
    _check(rc, "gjkepa_hull_batch")
    return dict(faces=faces[:nslots], face_off=foff, n_faces=nf, n_verts=nv, status=st, hull_verts=hv, vert_idx=vi)


def hull_batch_device(vert_dtype: int, points_ptr: int, cloud_off_ptr: int, cloud_cnt_ptr: int, n_clouds: int,
                      face_off_ptr: int, faces_ptr: int, n_faces_ptr: int, n_verts_ptr: int, status_ptr: int,
                      hull_verts_ptr: int = 0, vert_idx_ptr: int = 0, stream: int = 0) -> None:
    """Device-resident hull batch (raw device pointers), asynchronous on `stream`."""
    rc = load().gjkepa_hull_batch_device(int(vert_dtype), points_ptr, cloud_off_ptr, cloud_cnt_ptr, int(n_clouds),
                                         face_off_ptr, faces_ptr, n_faces_ptr, n_verts_ptr, status_ptr,
                                         hull_verts_ptr or None, vert_idx_ptr or None, stream or None)
    _check(rc, "gjkepa_hull_batch_device")


# ---- mass properties of hulls (include/gjkepa.h gjkepa_mass_*; csrc/mass_props.h) -----------------------
def _mass_motion(body_motion, n: int):
    if body_motion is None:
        return None
    mot = np.array(body_motion, np.float64).reshape(-1)       # a copy: the call writes the pivots into it
    if mot.size != MOTION_DOUBLES * n:
        raise GjkEpaError("body_motion: 9 float64 (v, w, c) per hull of the pool")
    return mot


def mass_batch(pool: CloudPool, hull: dict, body_motion=None, use_status: bool = True, device: int = 0):
    """Volume, area, centre of mass, inertia (about com, world axes, unit density), bounding radius and closure
    of every cloud's hull (host buffers, blocking): MASS64 records from the dict hull_batch returned for the
    same pool (or faces, face_off, n_faces and status of the caller's own).  use_status False passes no hull
    status.  body_motion: (n_clouds, 9) float64; returns (records, a copy with c = com for every OK cloud)."""
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.cloud_off, np.int64)
    cnt = np.ascontiguousarray(pool.cloud_cnt, np.int32)
    foff = np.ascontiguousarray(hull["face_off"], np.int64)
    faces = np.ascontiguousarray(hull["faces"], np.int32).reshape(-1, 3)
    nf = np.ascontiguousarray(hull["n_faces"], np.int32)
    hs = np.ascontiguousarray(hull["status"], np.int8) if use_status else None
    if foff.size != cnt.size or nf.size != cnt.size or (hs is not None and hs.size != cnt.size):
        raise GjkEpaError("hull: face_off, n_faces and status per cloud of the pool")
    out = np.zeros(cnt.size, MASS64)
    mot = _mass_motion(body_motion, cnt.size)
    rc = load().gjkepa_mass_batch(pool.dtype_code, _ptr(verts), verts.size, _ptr(off), _ptr(cnt), cnt.size, _ptr(foff),
                                  len(faces), _ptr(faces), _ptr(nf), None if hs is None else _ptr(hs), _ptr(out),
                                  None if mot is None else _ptr(mot), int(device))
    _check(rc, "gjkepa_mass_batch")
    return out if mot is None else (out, mot.reshape(-1, MOTION_DOUBLES))


def mass_batch_device(vert_dtype: int, points_ptr: int, cloud_off_ptr: int, cloud_cnt_ptr: int, n_clouds: int,
                      face_off_ptr: int, faces_ptr: int, n_faces_ptr: int, hull_status_ptr: int, out_ptr: int,
                      body_motion_ptr: int = 0, stream: int = 0) -> None:
    """Device-resident mass properties (raw device pointers: what hull_batch_device read and wrote),
    asynchronous on `stream`; hull_status_ptr / body_motion_ptr 0 / None: not given."""
    rc = load().gjkepa_mass_batch_device(int(vert_dtype), points_ptr, cloud_off_ptr, cloud_cnt_ptr, int(n_clouds),
                                         face_off_ptr, faces_ptr, n_faces_ptr, hull_status_ptr or None, out_ptr,
                                         body_motion_ptr or None, stream or None)
    _check(rc, "gjkepa_mass_batch_device")


def mass_pool(pool: HullPool, body_motion=None, device: int = 0):
    """From a narrow-phase hull pool to pivots in one call: the hull of every hull's vertices, then its mass
    properties (MASS64 records).  body_motion: (n_hulls, 9) float64; returns (records, a copy with c = com for
    every OK hull).  Hulls of fewer than four vertices and flat hulls come back STATUS_BAD_INPUT / _DEGENERATE."""
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    out = np.zeros(cnt.size, MASS64)
    mot = _mass_motion(body_motion, cnt.size)
    rc = load().gjkepa_mass_pool(pool.dtype_code, _ptr(verts), verts.size, _ptr(off), _ptr(cnt), cnt.size, _ptr(out),
                                 None if mot is None else _ptr(mot), int(device))
    _check(rc, "gjkepa_mass_pool")
    return out if mot is None else (out, mot.reshape(-1, MOTION_DOUBLES))


def quickhull(points, device: int = 0):
    """GCLIB_QuickHull::QuickHull(points, polytope, info) as called at GCLIB_GJKEPA.f90:950:
    the hull of an (n, 3) cloud as a triangle soup polytope(F, 3, 3) (face, vertex, xyz), outward
    wound; info = the GJKEPA_STATUS_* code (0 = OK)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    r = hull_batch(CloudPool.from_list([p]), device)
    nf = int(r["n_faces"][0])
    return p[r["faces"][:nf]], int(r["status"][0])


def hull_mesh_vertices(polytope) -> np.ndarray:
    """GCLIB_DeHull::getHullMeshesVertex(polytope, points, info) (GCLIB_GJKEPA.f90:920): the
    distinct vertices of a triangle soup, in order of first appearance (host-side; exact equality)."""
    v = np.asarray(polytope, np.float64).reshape(-1, 3)
    _, first = np.unique(v, axis=0, return_index=True)
    return v[np.sort(first)]


# ---- device broad phase (include/gjkepa.h gjkepa_broadphase) -----------------
def synth_scene(seed: int, n_hulls: int, n_min: int = 32, n_max: int = 32, box: float = 10.0,
                first_hull: int = 0, dtype=np.float32) -> HullPool:
    """Deterministic scene: unit-sphere hulls centred uniformly in [0, box)^3 (pairs left empty)."""
    lib = load()
    code = DTYPE_F32 if np.dtype(dtype) == np.float32 else DTYPE_F64
    total = lib.gjkepa_synth_scene(seed, first_hull, n_hulls, n_min, n_max, box, code, None, None, None)
    if total < 0:
        raise GjkEpaError("gjkepa_synth_scene: bad arguments")
    verts = np.empty(total, dtype=dtype)
    off = np.empty(n_hulls, np.int64)
    cnt = np.empty(n_hulls, np.int32)
    lib.gjkepa_synth_scene(seed, first_hull, n_hulls, n_min, n_max, box, code, _ptr(verts), _ptr(off), _ptr(cnt))
    return HullPool(verts, off, cnt, np.zeros((0, 2), np.int32))


def broadphase(pool: HullPool, max_pairs: int | None = None, device: int = 0):
    """Candidate pairs (a < b, ascending) passing the reference's sphere test, on the GPU.
    Returns (pairs int32 [n, 2], n_found); with max_pairs None the list is grown until it fits."""
    lib = load()
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    cap = max_pairs if max_pairs is not None else max(16 * cnt.size, 1024)
    while True:
        out = np.zeros((max(cap, 1), 2), np.int32)
        nf = np.zeros(1, np.int64)
        rc = lib.gjkepa_broadphase(pool.dtype_code, _ptr(verts), verts.size, _ptr(off), _ptr(cnt), cnt.size, _ptr(out),
                                   cap, _ptr(nf), int(device))
        _check(rc, "gjkepa_broadphase")
        n = int(nf[0])
        if n <= cap or max_pairs is not None:
            return out[:min(n, cap)], n
        cap = n


def broadphase_workspace_bytes(n_hulls: int, max_pairs: int) -> int:
    return int(load().gjkepa_broadphase_workspace_bytes(n_hulls, max_pairs))


def broadphase_device(vert_dtype: int, verts_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, n_hulls: int,
                      pairs_ptr: int, max_pairs: int, n_pairs_ptr: int, ws_ptr: int, ws_bytes: int,
                      stream: int = 0) -> None:
    """Device-resident broad phase (raw device pointers), asynchronous on `stream`."""
    rc = load().gjkepa_broadphase_device(int(vert_dtype), verts_ptr, hull_off_ptr, hull_cnt_ptr, int(n_hulls),
                                         pairs_ptr, int(max_pairs), n_pairs_ptr, ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_broadphase_device")


# ---- swept broad phase: the pair list of the casts (include/gjkepa.h gjkepa_broadphase_swept) ---
def broadphase_swept(pool: HullPool, body_motion, tolerance: float, long_radius: float = float("inf"),
                     max_pairs: int | None = None, device: int = 0):
    """Candidate pairs (a < b, ascending) whose swept bounding balls can come within `tolerance` during the
    step, on the GPU: the pair list of cast_rigid_batch.  body_motion as for cast_rigid_batch; long_radius
    is tuning only (bodies with rho + |v| / 2 above it are tested against every body instead of through the
    grid) and never changes the list.  Returns (pairs int32 [n, 2], n_found); with max_pairs None the list
    is grown until it fits."""
    lib = load()
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    mot = _motion_arg(pool, body_motion)
    cap = max_pairs if max_pairs is not None else max(16 * cnt.size, 1024)
    while True:
        out = np.zeros((max(cap, 1), 2), np.int32)
        nf = np.zeros(1, np.int64)
        rc = lib.gjkepa_broadphase_swept(pool.dtype_code, _ptr(verts), verts.size, _ptr(off), _ptr(cnt), cnt.size,
                                         _ptr(mot), float(tolerance), float(long_radius), _ptr(out), cap, _ptr(nf),
                                         int(device))
        _check(rc, "gjkepa_broadphase_swept")
        n = int(nf[0])
        if n <= cap or max_pairs is not None:
            return out[:min(n, cap)], n
        cap = n


def broadphase_swept_workspace_bytes(n_hulls: int, max_pairs: int) -> int:
    return int(load().gjkepa_broadphase_swept_workspace_bytes(n_hulls, max_pairs))


def broadphase_swept_device(vert_dtype: int, verts_ptr: int, hull_off_ptr: int, hull_cnt_ptr: int, n_hulls: int,
                            body_motion_ptr: int, tolerance: float, long_radius: float, pairs_ptr: int,
                            max_pairs: int, n_pairs_ptr: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Device-resident swept broad phase (raw device pointers; body_motion: 9 doubles per hull), asynchronous
    on `stream`."""
    rc = load().gjkepa_broadphase_swept_device(int(vert_dtype), verts_ptr, hull_off_ptr, hull_cnt_ptr, int(n_hulls),
                                               body_motion_ptr, float(tolerance), float(long_radius), pairs_ptr,
                                               int(max_pairs), n_pairs_ptr, ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_broadphase_swept_device")


# ---- event list and per-body clamp of a moving step (include/gjkepa.h gjkepa_events_device) ------
def events_workspace_bytes(n_pairs: int, n_hulls: int) -> int:
    b = int(load().gjkepa_events_workspace_bytes(int(n_pairs), int(n_hulls)))
    if b < 0:
        raise GjkEpaError(f"gjkepa_events_workspace_bytes failed ({b})")
    return b


def events_device(pairs_ptr: int, n_pairs: int, n_hulls: int, cast_records_ptr: int, records_ptr: int,
                  records_precision: int, events_ptr: int, max_events: int, n_events_ptr: int, counts_ptr: int,
                  body_time_ptr: int, body_event_ptr: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Device-resident event pass (raw device pointers), asynchronous on `stream`: the events of a pair list's
    cast records in (time, pair) order, *n_events and counts[5] (device int64), and per hull the first IMPACT
    or UNDECIDED event's time and rank.  records_ptr 0 / None: no contact records; body_time_ptr and
    body_event_ptr both 0 / None: no body outputs."""
    rc = load().gjkepa_events_device(pairs_ptr or None, int(n_pairs), int(n_hulls), cast_records_ptr or None,
                                     records_ptr or None, int(records_precision), events_ptr or None, int(max_events),
                                     n_events_ptr, counts_ptr, body_time_ptr or None, body_event_ptr or None,
                                     ws_ptr or None, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_events_device")


def events(pairs, cast_records, n_hulls: int, records: np.ndarray | None = None, max_events: int | None = None,
           bodies: bool = True, device: int = 0):
    """The event pass over host arrays, staged through torch (for tests and tools; a pipeline keeps its records
    on the device and calls events_device).  pairs: int32 (n, 2); cast_records: CAST64 (n,); records: None or
    the list's REC64 / REC32 contact records; max_events None: room for every event.
    Returns (events EVENT64 [min(n_events, max_events)], n_events, counts int64 [5], body_time float64
    [n_hulls] or None, body_event int32 [n_hulls] or None)."""
    import torch
    prs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n = prs.shape[0]
    cast = np.ascontiguousarray(cast_records)
    if cast.dtype != CAST64 or cast.shape != (n,):
        raise GjkEpaError("cast_records: one CAST64 record per pair")
    records, _, rec_prec = _records_arg(records, n)
    cap = n if max_events is None else int(max_events)
    dev = torch.device("cuda", int(device))

    def to_dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)

    with torch.cuda.device(dev):
        d_prs, d_cast = to_dev(prs), to_dev(cast)
        d_rec = None if records is None else to_dev(records)
        d_ev = torch.zeros(max(cap, 1) * EVENT64.itemsize, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(6, dtype=torch.int64, device=dev)
        d_time = torch.zeros(max(n_hulls, 1), dtype=torch.float64, device=dev) if bodies else None
        d_rank = torch.zeros(max(n_hulls, 1), dtype=torch.int32, device=dev) if bodies else None
        wsb = events_workspace_bytes(n, n_hulls)
        ws = torch.zeros(max(wsb, 256), dtype=torch.uint8, device=dev)
        events_device(d_prs.data_ptr() if n else 0, n, n_hulls, d_cast.data_ptr() if n else 0,
                      0 if d_rec is None else d_rec.data_ptr(), rec_prec, d_ev.data_ptr(), cap, d_n.data_ptr(),
                      d_n.data_ptr() + 8, d_time.data_ptr() if bodies else 0, d_rank.data_ptr() if bodies else 0,
                      ws.data_ptr(), wsb, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.current_stream(dev).synchronize()
    host_n = d_n.cpu().numpy()
    m = min(int(host_n[0]), cap)
    ev = d_ev.cpu().numpy()[:m * EVENT64.itemsize].view(EVENT64).copy()
    if not bodies:
        return ev, int(host_n[0]), host_n[1:6].copy(), None, None
    return ev, int(host_n[0]), host_n[1:6].copy(), d_time.cpu().numpy()[:n_hulls], d_rank.cpu().numpy()[:n_hulls]


def collide_moving(pool: HullPool, body_motion, tolerance: float, long_radius: float = float("inf"), version: int = 2,
                   tol_ff: float = 1.0, precision: int = PREC_F64, max_events: int | None = None, pose: bool = False,
                   device: int = 0):
    """A whole moving step over a hull pool in one call (host buffers, blocking): swept broad phase, narrow
    phase on its list, rigid cast with the batch's records, event pass, and with pose=True the pool posed at
    body_time.  body_motion, tolerance and long_radius as for broadphase_swept.  With max_events None the list
    is grown until it fits.  Returns a dict: events (EVENT64), n_events, counts (int64 [5]: HIT, START, IMPACT,
    UNDECIDED, BAD), n_candidates, body_time (float64 [n_hulls]) and posed (a HullPool, or None)."""
    lib = load()
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    mot = _motion_arg(pool, body_motion)
    cap = max_events if max_events is not None else max(4 * cnt.size, 1024)
    while True:
        ev = np.zeros(max(cap, 1), EVENT64)
        ne, ncand, counts = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(5, np.int64)
        btime = np.zeros(cnt.size)
        posed = verts.copy() if pose else None
        rc = lib.gjkepa_collide_moving(int(version), float(tol_ff), pool.dtype_code, int(precision), _ptr(verts), verts.size,
                                       _ptr(off), _ptr(cnt), cnt.size, _ptr(mot), float(tolerance), float(long_radius),
                                       _ptr(ev), cap, _ptr(ne), _ptr(counts), _ptr(ncand), _ptr(btime),
                                       _ptr(posed) if pose else None, int(device))
        _check(rc, "gjkepa_collide_moving")
        n = int(ne[0])
        if n <= cap or max_events is not None:
            return {"events": ev[:min(n, cap)], "n_events": n, "counts": counts, "n_candidates": int(ncand[0]),
                    "body_time": btime, "posed": HullPool(posed, pool.hull_off, pool.hull_cnt, pool.pairs) if pose else None}
        cap = n


def event_manifolds_device(events_ptr: int, n_events_ptr: int, max_events: int, manifolds_ptr: int, out_ptr: int,
                           stream: int = 0) -> None:
    """out[k] = manifolds[events[k].pair] for k < min(*n_events, max_events) (raw device pointers; n_events a
    device int64), asynchronous on `stream`: the patches of an event list from the pair list's manifold records."""
    rc = load().gjkepa_event_manifolds_device(events_ptr or None, n_events_ptr or None, int(max_events),
                                              manifolds_ptr or None, out_ptr or None, stream or None)
    _check(rc, "gjkepa_event_manifolds_device")


def collide_moving_patches(pool: HullPool, body_motion, tolerance: float, margin: float, long_radius: float = float("inf"),
                           version: int = 2, tol_ff: float = 1.0, precision: int = PREC_F64,
                           max_events: int | None = None, pose: bool = False, device: int = 0):
    """collide_moving with a contact patch per event: the dict of collide_moving plus patches (MANIFOLD64, one per
    listed event): a HIT event's contact manifold, a START or IMPACT event's manifold at its time
    (MANIFOLD_AT_TOI), MANIFOLD_NO_HIT for an UNDECIDED event.  margin as for manifold_batch."""
    lib = load()
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    mot = _motion_arg(pool, body_motion)
    cap = max_events if max_events is not None else max(4 * cnt.size, 1024)
    while True:
        ev = np.zeros(max(cap, 1), EVENT64)
        patches = np.zeros(max(cap, 1), MANIFOLD64)
        ne, ncand, counts = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(5, np.int64)
        btime = np.zeros(cnt.size)
        posed = verts.copy() if pose else None
        rc = lib.gjkepa_collide_moving_patches(int(version), float(tol_ff), pool.dtype_code, int(precision), _ptr(verts),
                                               verts.size, _ptr(off), _ptr(cnt), cnt.size, _ptr(mot), float(tolerance),
                                               float(long_radius), _ptr(ev), cap, _ptr(ne), _ptr(counts), _ptr(ncand),
                                               _ptr(btime), _ptr(posed) if pose else None, float(margin), _ptr(patches),
                                               int(device))
        _check(rc, "gjkepa_collide_moving_patches")
        n = int(ne[0])
        if n <= cap or max_events is not None:
            m = min(n, cap)
            return {"events": ev[:m], "patches": patches[:m], "n_events": n, "counts": counts,
                    "n_candidates": int(ncand[0]), "body_time": btime,
                    "posed": HullPool(posed, pool.hull_off, pool.hull_cnt, pool.pairs) if pose else None}
        cap = n


# ---- contact-list compaction ----------------------------------------
def compact_workspace_bytes(n_pairs: int) -> int:
    return int(load().gjkepa_compact_workspace_bytes(n_pairs))


def compact_hits_device(precision: int, records_ptr: int, n_pairs: int, hit_idx_ptr: int, hits_ptr: int,
                        n_hits_ptr: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
    """Dense, order-preserving list of the hit pairs of a device-resident batch (indices, and the
    records when hits_ptr is non-zero); *n_hits is a device int64."""
    rc = load().gjkepa_compact_hits_device(int(precision), records_ptr, int(n_pairs), hit_idx_ptr, hits_ptr or None,
                                           n_hits_ptr, ws_ptr, int(ws_bytes), stream or None)
    _check(rc, "gjkepa_compact_hits_device")


def collide(pool: HullPool, version: int = 2, tol_ff: float = 1.0, precision: int = PREC_F64,
            max_contacts: int | None = None, device: int = 0):
    """The all-pairs GJKEPA loop over a hull pool in one call (broad phase, narrow phase, hit list).
    Returns (pairs int32 [n, 2] with a < b ascending, records of those hits, n_candidates)."""
    lib = load()
    verts = np.ascontiguousarray(pool.verts)
    off = np.ascontiguousarray(pool.hull_off, np.int64)
    cnt = np.ascontiguousarray(pool.hull_cnt, np.int32)
    cap = max_contacts if max_contacts is not None else max(4 * cnt.size, 1024)
    while True:
        prs = np.zeros((max(cap, 1), 2), np.int32)
        out = np.zeros(max(cap, 1), dtype=record_dtype(precision))
        nc = np.zeros(1, np.int64)
        ncand = np.zeros(1, np.int64)
        rc = lib.gjkepa_collide(int(version), float(tol_ff), pool.dtype_code, int(precision), _ptr(verts), verts.size,
                                _ptr(off), _ptr(cnt), cnt.size, _ptr(prs), _ptr(out), cap, _ptr(nc), _ptr(ncand),
                                int(device))
        _check(rc, "gjkepa_collide")
        n = int(nc[0])
        if n <= cap or max_contacts is not None:
            m = min(n, cap)
            return prs[:m], out[:m], int(ncand[0])
        cap = n
