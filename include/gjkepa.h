/*
 * gjkepa.h — C-ABI drop-in boundary of the MI355X batched GJK/EPA narrow phase.
 *
 * The reference (xiejihong0306/collision-detect-GJK-EPA) exposes exactly one public entry,
 * SUBROUTINE GJKEPA in MODULE GCLIB_GJKEPA (src/GCLIB_GJKEPA.f90:12, :39-52).  It answers one
 * convex-pair query: hit flag, contact type, nearest points, normal, contact point and
 * penetration depth.  The entries below are what an ISO_C_BINDING interface for that path binds:
 *
 *   gjkepa_query         one pair, same arguments / meaning as GJKEPA (GCLIB_GJKEPA.f90:39-52);
 *                        host buffers, blocking.  The Fortran drop-in module
 *                        (collision-detect-gjk-epa_amd/fortran/gclib_gjkepa.f90) wraps it
 *                        under the unchanged GJKEPA signature.
 *   gjkepa_batch         N pairs over a pooled hull set, host buffers, blocking.  This replaces
 *                        the caller-side `!$OMP PARALLEL DO ... CALL GJKEPA` loop implied by the
 *                        THREADPRIVATE design (GCLIB_GJKEPA.f90:9, :16, :55-60).
 *   gjkepa_batch_device  the same with every buffer already resident in device memory (HBM),
 *                        asynchronous on a caller stream; no allocation, no synchronisation,
 *                        so it can be captured into a hipGraph.
 *
 * Error behaviour.  The reference has no return codes: it writes to unit 6 and then PAUSEs or
 * STOPs (GCLIB_GJKEPA.f90:300-301, :337-339, :499-501, :635-637, :1370-1372).  Here every
 * pair carries a status code instead (GJKEPA_STATUS_*), outputs are left at the values the
 * reference would have returned (EPA cap: all zero with collision = 1, :299-302) or zeroed
 * where the reference would have aborted, and the process never blocks.  Functions return
 * 0 on success or a negative GJKEPA_E_* code.
 *
 * Data layout.  A hull is stored exactly like the reference's REAL*8 p(n,3) argument: column
 * major, i.e. x[0..n-1], y[0..n-1], z[0..n-1] (structure of arrays per hull).  Hulls are pooled:
 * hull h starts at scalar offset hull_off[h] of `verts` and has hull_cnt[h] vertices.  A pair
 * is two hull indices (pairs[2k], pairs[2k+1]) = (p1_, p2_).
 *
 * Plain pointers and sizes only; no torch or HIP types in any signature.
 */
#ifndef GJKEPA_H
#define GJKEPA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-pair status (replaces PAUSE / STOP) ---------------------------------------------- */
#define GJKEPA_STATUS_OK          0  /* normal return */
#define GJKEPA_STATUS_EPA_MAXITER 1  /* EPA hit its 99-iteration cap (:299-302): outputs 0, colli_type 0 */
#define GJKEPA_STATUS_DEGENERATE  2  /* reference would STOP: degenerate plane (:1369-1373) etc. */
#define GJKEPA_STATUS_BAD_VERSION 3  /* version_ not in {1,2,3} on a hit (:336-339) */
#define GJKEPA_STATUS_BAD_INPUT   4  /* hull with < 1 vertex or above GJKEPA_MAX_HULL_VERTS */

/* ---- API return codes ---------------------------------------------------------------------- */
#define GJKEPA_E_OK          0
#define GJKEPA_E_ARG        -1  /* invalid argument (null pointer, bad enum, bad size) */
#define GJKEPA_E_HIP        -2  /* HIP runtime error (see gjkepa_last_error) */
#define GJKEPA_E_NODEVICE   -3  /* no usable gfx950 device */
#define GJKEPA_E_WORKSPACE  -4  /* device workspace too small */
#define GJKEPA_E_COMM       -5  /* RCCL unavailable or a collective failed (see gjkepa_last_error) */

/* ---- enums --------------------------------------------------------------------------------- */
#define GJKEPA_DTYPE_F32 0      /* vertex storage dtype */
#define GJKEPA_DTYPE_F64 1
#define GJKEPA_PREC_F64  1      /* compute precision: fp64 = the reference's REAL*8 semantics */
#define GJKEPA_PREC_F32  0      /* compute precision: fp32, opt-in; an fp32 answer is kept only when certified to
                                   1e-6 relative depth (else recomputed in fp64), which makes it slower than F64 */

#define GJKEPA_MAX_HULL_VERTS 256   /* largest hull the kernels accept (config C4: 8..256) */

/* ---- contact records (one per pair) ---------------------------------------------------------
 * Field meaning follows GJKEPA's INTENT(OUT) arguments (GCLIB_GJKEPA.f90:47-52):
 *   penetration_depth  <- penetration_depth_
 *   collision_normal   <- collision_normal_(3)
 *   collision_point    <- collision_point_(3)
 *   nearest_points     <- nearest_points_(2,3), stored row-wise: p1 xyz then p2 xyz
 *   collision          <- collision_ (LOGICAL*1)
 *   colli_type         <- colliType_ (0 no hit / 1 other / 2 face-face)
 *   status             <- GJKEPA_STATUS_*
 *   diag               <- (gjk_iters) | (epa_iters << 8) | (final_faces << 16); diagnostics only
 */
typedef struct gjkepa_contact_f64 {
    double   penetration_depth;
    double   collision_normal[3];
    double   collision_point[3];
    double   nearest_points[6];
    int8_t   collision;
    int8_t   colli_type;
    int8_t   status;
    int8_t   reserved;
    uint32_t diag;
    uint32_t pad[4];
} gjkepa_contact_f64;            /* 128 bytes */

typedef struct gjkepa_contact_f32 {
    float    penetration_depth;
    float    collision_normal[3];
    float    collision_point[3];
    float    nearest_points[6];
    int8_t   collision;
    int8_t   colli_type;
    int8_t   status;
    int8_t   reserved;
    uint32_t diag;
    uint32_t pad;
} gjkepa_contact_f32;            /* 64 bytes */

/* Size in bytes of one contact record for a compute precision (128 for F64, 64 for F32). */
int gjkepa_record_bytes(int32_t precision);

/* ---- single pair: the GJKEPA drop-in (GCLIB_GJKEPA.f90:39-52) ---------------------------------
 * p1, p2: REAL*8 (n,3) column-major, exactly the memory of the Fortran assumed-shape actuals.
 * nearest_points: REAL*8 (2,3) column-major (Fortran layout: p1x p2x p1y p2y p1z p2z).
 * status may be NULL.  Runs on device `device` (batch of one); blocking; thread-safe. */
int gjkepa_query(int32_t version, double tol_ff,
                 const double* p1, int32_t n1,
                 const double* p2, int32_t n2,
                 int8_t* collision, int32_t* colli_type,
                 double* nearest_points, double* collision_normal,
                 double* collision_point, double* penetration_depth,
                 int32_t* status, int32_t device);

/* ---- the resident query service behind gjkepa_query ------------------------------------------
 * gjkepa_query posts each pair to a persistent grid of 64 one-wave workgroups (one per request slot
 * in host-mapped memory) instead of launching kernels per call.  The grid runs on the library's own
 * stream and leaves by itself once no call arrived for 2 ms, or after 20 ms of residency even under
 * steady traffic (the next call relaunches it at once).  While it is resident:
 *   - a device-wide synchronisation in the caller's process (hipDeviceSynchronize,
 *     torch.cuda.synchronize() without a stream, a legacy default-stream sync) waits for the grid
 *     to leave, i.e. up to 2 ms after the last call, or up to 20 ms while other threads keep calling;
 *   - work the process enqueues on a stream that shares the grid's hardware queue (streams are
 *     spread over GPU_MAX_HW_QUEUES queues) starts only after the grid leaves, within those bounds.
 * Callers that synchronise the whole device, or want it idle, drain the grid first: */
/* Drain the service grid of `device` (device < 0: every device) now; returns after it has left.
 * Calls that arrive later relaunch it.  Returns 0 or GJKEPA_E_HIP. */
int gjkepa_query_service_stop(int32_t device);
/* Turn the service on (1) or off (0) for later gjkepa_query calls; off also drains every grid.  Off,
 * single-pair calls of concurrent threads are combined into one batch launch (no resident grid).
 * The initial setting is on unless the environment sets GJKEPA_QUERY_SERVICE=0.  Returns the
 * previous setting (0/1) or a negative GJKEPA_E_* code. */
int gjkepa_query_service_set(int32_t enabled);
/* Diagnostic: 1 while a service grid of `device` (device < 0: any device) is still on the GPU, 0 when
 * none is, or a negative GJKEPA_E_* code.  Non-blocking. */
int gjkepa_query_service_resident(int32_t device);

/* ---- batch over host buffers (blocking) ------------------------------------------------------
 * verts:     hull vertex pool, dtype `vert_dtype`, n_vert_scalars scalars in total.
 * hull_off:  [n_hulls] scalar offset of each hull's x[0] in `verts`.
 * hull_cnt:  [n_hulls] vertex count of each hull (1..GJKEPA_MAX_HULL_VERTS).
 * pairs:     [2*n_pairs] hull indices (p1_, p2_) per pair.
 * out:       [n_pairs] records, gjkepa_contact_f64 (precision F64) or _f32 (precision F32). */
int gjkepa_batch(int32_t version, double tol_ff, int32_t vert_dtype, int32_t precision,
                 const void* verts, int64_t n_vert_scalars,
                 const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                 const int32_t* pairs, int64_t n_pairs,
                 void* out, int32_t device);

/* ---- batch over device buffers (asynchronous on `stream`, a hipStream_t or NULL) -------------
 * All pointers are device pointers on the current device.  `workspace` (256-byte aligned) should hold
 * gjkepa_workspace_bytes(n_pairs) bytes: a 512-byte header of per-kernel work counters and route
 * tallies (reset by the call itself), one routing byte per pair (which GJK / EPA / contact kernel
 * tier owns the pair next), and park slots of 2880 bytes for one pair in 8: an EPA tier whose
 * polytope is about to outgrow it parks the polytope there and the next tier resumes it instead of
 * restarting from the GJK simplex (results identical either way).  The minimum is the header plus
 * the route bytes rounded up to 256; park slots are used as far as the workspace provides them.  It
 * may be reused between calls on the same stream. */
int64_t gjkepa_workspace_bytes(int64_t n_pairs);
/* The same with park slots for one in 8 of `n_large_pairs`: the pairs with a hull above 32 vertices,
 * the only ones that can reach the parking EPA tiers (0 for a batch of small hulls such as config C2:
 * header and route bytes only).  gjkepa_workspace_bytes(n) = gjkepa_workspace_bytes_for(n, n). */
int64_t gjkepa_workspace_bytes_for(int64_t n_pairs, int64_t n_large_pairs);

/* ---- per-launch timing (diagnostics; bench.py's dominant-kernel roofline) ---------------------
 * gjkepa_launch_timing(1): every later chain the calling thread enqueues (gjkepa_batch_device and the
 * entries built on it) records a timing event at its head on the caller's stream and one before and
 * after each kernel launch, on the stream that launch goes to (the caller's or an internal one).
 * gjkepa_launch_timing_read waits for those events and writes up to `max` entries, one per launch in
 * enqueue order; it returns the number written and forgets every recorded launch.  Returns the
 * previous setting / a GJKEPA_E_* code.  Not for graph capture. */
typedef struct gjkepa_launch_time {
    char     kernel[16];    /* "reset", "gjk", "epa", "contact", "redo" or "query" */
    int32_t  tier;          /* kernel tier (contact tier for "contact") */
    int32_t  part;          /* part index of a tier launched over consecutive pair ranges, else 0 */
    int32_t  route_code;    /* the pairs it serves (-1: every pair) */
    int32_t  chain;         /* enqueue call, counted from 0 since the last read */
    int32_t  stream;        /* 0: the caller's stream; 1..: the chain's internal streams, by first use */
    int32_t  pad;
    int64_t  first_pair;    /* pair range the launch scans */
    int64_t  n_pairs;
    float    start_ms;      /* events before / after the launch, ms after the chain's head event */
    float    end_ms;
} gjkepa_launch_time;
int gjkepa_launch_timing(int32_t enable);
int gjkepa_launch_timing_read(gjkepa_launch_time* out, int32_t max);
int gjkepa_batch_device(int32_t version, double tol_ff, int32_t vert_dtype, int32_t precision,
                        const void* verts, const int64_t* hull_off, const int32_t* hull_cnt,
                        const int32_t* pairs, int64_t n_pairs,
                        void* out, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* ---- batched convex hulls ----------------------------------------------
 * The reference rebuilds a convex hull every EPA iteration with
 *   CALL QuickHull(scatPoints, polytope_2_, info)           (GCLIB_GJKEPA.f90:950)
 *   CALL getHullMeshesVertex(polytope_1_, scatPoints, info) (GCLIB_GJKEPA.f90:920)
 * from the unvendored modules GCLIB_QuickHull / GCLIB_DeHull (:14-15, no version pin).  These
 * entries expose the same two operations as a first-class batched device module: the hull of
 * every point cloud of a pool as outward triangles (QuickHull) plus the hull's vertex set
 * (getHullMeshesVertex), so callers can reduce raw point clouds to hulls before the narrow phase.
 *
 * Algorithm (restated bit for bit by oracle/gjkepa_oracle.c: oracle_hull_batch): QuickHull with a
 * global furthest-point order, fp64 arithmetic, absolute epsilon GJKEPA_HULL_EPS.
 *   1. initial tetrahedron: i0 = first argmin x; i1 = first argmax |p - p_i0|^2;
 *      i2 = first argmax |(p_i1 - p_i0) x (p - p_i0)|^2; i3 = first argmax |(p - p_i0).n|,
 *      n = (p_i1 - p_i0) x (p_i2 - p_i0).  Collinear / coplanar / coincident clouds (distance
 *      <= eps at any step) are GJKEPA_STATUS_DEGENERATE.
 *   2. every other point is assigned to the face it is furthest above (first face on ties) when
 *      that distance exceeds eps, otherwise discarded as interior.
 *   3. repeat: the eye is the assigned point furthest above its face (lowest index on ties); every
 *      face the eye is more than eps above is removed; each horizon edge (u, w) is coned to the
 *      eye as face (u, w, eye); points of removed faces are re-assigned among the new faces only.
 * Face slots: new faces take the removed faces' slots in slot order, then append; faces are
 * reported in slot order.  Outward winding: normal = (b - a) x (c - b) points out of the hull.
 * Vertex set (getHullMeshesVertex): the points the faces reference, in ascending point index.
 *
 * Layout.  Input clouds use the hull-pool layout above (cloud c: cloud_cnt[c] points, SoA at
 * scalar offset cloud_off[c]).  Cloud c's faces are written as int32 (a, b, c) point-index
 * triples at triangle offset face_off[c] of `faces`, with room for gjkepa_hull_face_capacity(
 * cloud_cnt[c]) = 2n - 4 triangles.  Optional outputs (NULL to skip), both at cloud_off[c]:
 * `hull_verts` (same dtype as the input) receives the hull as a pool entry of n_verts[c] points,
 * SoA with stride n_verts[c], directly usable as a gjkepa_batch hull with hull_cnt = n_verts;
 * `vert_idx` (int32) receives the hull vertices' point indices.
 * status[c]: GJKEPA_STATUS_OK, _DEGENERATE (flat cloud, zero-area cone face or a non-manifold
 * horizon that overflows 2n - 4 face slots) or _BAD_INPUT (n < 4, n > GJKEPA_HULL_MAX_POINTS,
 * non-finite coordinates); n_faces = n_verts = 0 unless OK. */
#define GJKEPA_HULL_MAX_POINTS 256
#define GJKEPA_HULL_EPS 1.0e-10

/* Triangle slots cloud c needs in `faces`: 2n - 4 (0 for n < 4). */
int64_t gjkepa_hull_face_capacity(int32_t n_points);

/* Host buffers, blocking.  n_point_scalars / n_face_slots bound the pool and face buffers. */
int gjkepa_hull_batch(int32_t vert_dtype, const void* points, int64_t n_point_scalars,
                      const int64_t* cloud_off, const int32_t* cloud_cnt, int64_t n_clouds,
                      const int64_t* face_off, int64_t n_face_slots, int32_t* faces,
                      int32_t* n_faces, int32_t* n_verts, int8_t* status,
                      void* hull_verts, int32_t* vert_idx, int32_t device);

/* Device buffers, asynchronous on `stream` (hipStream_t or NULL); no allocation, no sync. */
int gjkepa_hull_batch_device(int32_t vert_dtype, const void* points,
                             const int64_t* cloud_off, const int32_t* cloud_cnt, int64_t n_clouds,
                             const int64_t* face_off, int32_t* faces,
                             int32_t* n_faces, int32_t* n_verts, int8_t* status,
                             void* hull_verts, int32_t* vert_idx, void* stream);

/* ---- mass properties of hulls (volume, centre of mass, inertia) ---------------------------------
 * What a body needs besides its hull: the pivot of its motion block (the casts, the pose and the swept broad
 * phase want c at the body's own centre, where rho is smallest), and the volume and inertia tensor a caller
 * needs to act on an IMPACT event.  These entries reduce what gjkepa_hull_batch(_device) wrote (outward
 * triangles over a cloud) to one record per cloud.
 * Definition (csrc/mass_props.h is its text, for host and device; plain fp64 in the order written there).
 * o is the point named by the first index of the cloud's first face.  It lies on the hull, so every
 * tetrahedron (o, a, b, c) of an outward convex mesh has a signed volume >= 0 and the sums do not cancel.  Per
 * face, with A = p_a - o, B = p_b - o, C = p_c - o:  N = (B - A) x (C - B);  d = A . (B x C);  S = (A + B) + C;
 * the face adds d, d S_k, d (((S_i S_j + A_i A_j) + B_i B_j) + C_i C_j) for ij = xx, yy, zz, xy, xz, yz, |N| and
 * N_k to 14 totals T.  The sum has one shape whatever the launch: 64 strided partials (partial l takes faces
 * l, l + 64, .. in ascending order from +0.0), then P[l] = P[l] + P[l ^ s] for s = 1, 2, 4, 8, 16, 32.
 *   volume     T0 / 6
 *   com        o + m,  m = T[1..3] / (4 T0)
 *   inertia    (Myy + Mzz, Mxx + Mzz, Mxx + Myy, -Mxy, -Mxz, -Myz) with M_ij = T[4..9] / 120 - volume m_i m_j:
 *              Ixx, Iyy, Izz, Ixy, Ixz, Iyz about com, in world axes, at unit density (multiply by the density)
 *   area       0.5 T10
 *   closure    max|T[11..13]| / T10: 0 for a closed surface; faces of the caller's own that do not close show here
 *   radius     sqrt(max_i |x_i - com|^2) over all points of the cloud (the maximum is attained at a hull
 *              vertex): bit for bit the rho the swept broad phase and the rigid cast compute for the pivot c = com
 *   n_faces    the cloud's face count
 * status, the first rule that applies wins:
 *   1. n outside 4 .. GJKEPA_HULL_MAX_POINTS                              GJKEPA_STATUS_BAD_INPUT
 *   2. hull_status given and not GJKEPA_STATUS_OK                         that status, copied
 *   3. n_faces outside 4 .. 2n - 4                                        GJKEPA_STATUS_BAD_INPUT
 *   4. a face index outside [0, n), or a non-finite coordinate in the cloud   GJKEPA_STATUS_BAD_INPUT
 *   5. T0 not finite or not > 0 (an inward mesh), or a result not finite  GJKEPA_STATUS_DEGENERATE
 * A record that is not OK is zero apart from status.  Every face index is checked before a point is read
 * through it: nothing outside the cloud is read, whatever the face buffer holds.
 * Method: one launch, one wave per cloud (lane l holds partial l), the cloud held in LDS; no atomics, no
 * workspace.  Deterministic. */
typedef struct gjkepa_mass_f64 {
    double   volume;
    double   area;
    double   com[3];
    double   inertia[6];
    double   radius;
    double   closure;
    int32_t  n_faces;
    int8_t   status;
    int8_t   flags;              /* 0 today */
    int8_t   reserved[2];
    uint32_t pad[4];
} gjkepa_mass_f64;               /* 128 bytes */

/* Size in bytes of one mass record (128). */
int gjkepa_mass_record_bytes(void);
/* Device buffers, asynchronous on `stream` (hipStream_t or NULL): no allocation, no synchronisation, every
 * launch on that stream only (a captured graph is a linear chain); records nothing for gjkepa_launch_timing.
 * points .. n_faces are what gjkepa_hull_batch_device read and wrote, so the two chain on one stream;
 * hull_status (may be NULL): its status array.  out: n_clouds records.  body_motion (may be NULL): 9 doubles
 * per cloud; an OK cloud's com is written to body_motion[9 c + 6 .. 9 c + 8] and nothing else of the block.
 * n_clouds == 0 returns 0.  GJKEPA_E_ARG for a bad dtype, a negative count or a null required pointer. */
int gjkepa_mass_batch_device(int32_t vert_dtype, const void* points,
                             const int64_t* cloud_off, const int32_t* cloud_cnt, int64_t n_clouds,
                             const int64_t* face_off, const int32_t* faces, const int32_t* n_faces,
                             const int8_t* hull_status, void* out, double* body_motion, void* stream);
/* Host buffers, blocking; the pool and face-buffer checks of gjkepa_hull_batch (n_point_scalars,
 * n_face_slots).  body_motion: NULL, or 9 n_clouds doubles, in and out. */
int gjkepa_mass_batch(int32_t vert_dtype, const void* points, int64_t n_point_scalars,
                      const int64_t* cloud_off, const int32_t* cloud_cnt, int64_t n_clouds,
                      const int64_t* face_off, int64_t n_face_slots, const int32_t* faces,
                      const int32_t* n_faces, const int8_t* hull_status,
                      void* out, double* body_motion, int32_t device);
/* From a narrow-phase hull pool to pivots in one call (host buffers, blocking): gjkepa_hull_batch_device on
 * the pool into face scratch of the library's, then gjkepa_mass_batch_device with the hull's status: the bytes
 * those two give when called one after the other.  The pool arguments and checks of gjkepa_pose_pool.  Hulls of
 * fewer than four vertices and flat hulls come back BAD_INPUT or DEGENERATE and their motion blocks are left
 * alone.  body_motion: NULL, or 9 n_hulls doubles, in and out. */
int gjkepa_mass_pool(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                     const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                     void* out, double* body_motion, int32_t device);

/* ---- device broad phase -------------------------------------------------
 * Emits the candidate pair list a narrow-phase batch consumes: every pair of hulls (a < b) of a
 * pool whose bounding spheres pass the reference's own rough test,
 * RoughCollisionDetection_SphericalEnvelope (GCLIB_GJKEPA.f90:1165-1188):
 *   m = SUM(p(:,k)) / n (sequential sums), r = MAXVAL(NORM2(p_i - m)),
 *   pair iff NORM2(m_a - m_b) <= r_a + r_b + 1.0      (fp64, the oracle's arithmetic, bit-exact)
 * i.e. exactly the pairs whose GJKEPA call would get past its first test (:76-77); a caller's
 * double loop over all pairs collapses to this list.  Hulls with a bad vertex count or non-finite
 * coordinates take part in no pair.
 *
 * Method (MI355X): per-hull sphere kernel; uniform grid of cell edge 2 r_max + 1 with a radix
 * sort of the cell keys (rocPRIM) and a hash table from cell to first sorted hull; count / scan /
 * emit kernels test each hull against the later-indexed hulls of its 27 neighbouring cells; a final
 * radix sort of the emitted (a << 32 | b) keys leaves the list in ascending (a, b) order — the
 * order of `DO a = 1, N; DO b = a+1, N`.
 * Output: pairs[2k], pairs[2k+1] = (a, b) for k < min(n_found, max_pairs); *n_pairs = n_found
 * (device int64 for the device entry).  n_found > max_pairs means the list was cut: enlarge it and
 * call again.  The device entry never synchronises (graph-capturable): the final sort runs over
 * max_pairs keys padded with all-ones, so size max_pairs near the expected count. */
int64_t gjkepa_broadphase_workspace_bytes(int64_t n_hulls, int64_t max_pairs);

/* Host buffers, blocking.  *n_pairs = pairs found (the list holds the first max_pairs of them). */
int gjkepa_broadphase(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                      const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                      int32_t* pairs, int64_t max_pairs, int64_t* n_pairs, int32_t device);

/* Device buffers, asynchronous on `stream`; n_pairs is a device int64. */
int gjkepa_broadphase_device(int32_t vert_dtype, const void* verts, const int64_t* hull_off,
                             const int32_t* hull_cnt, int64_t n_hulls,
                             int32_t* pairs, int64_t max_pairs, int64_t* n_pairs,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---- contact-list compaction -------------------------------------
 * Turns a batch's records (gjkepa_batch_device output, one per pair) into the dense list a device
 * consumer needs: hit_idx[k] = index of the k-th pair whose collision flag is set (ascending), and,
 * when `hits` is not NULL, that pair's record copied to hits[k].  *n_hits (device int64) = count.
 * Deterministic (no atomics), asynchronous on `stream`, graph-capturable; records stay in HBM.
 * workspace: gjkepa_compact_workspace_bytes(n_pairs) bytes (tile counts, offsets, scan scratch). */
int64_t gjkepa_compact_workspace_bytes(int64_t n_pairs);
int gjkepa_compact_hits_device(int32_t precision, const void* records, int64_t n_pairs,
                               int32_t* hit_idx, void* hits, int64_t* n_hits,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* ---- warm start for persistent pairs -------------------------------------
 * gjkepa_batch_device plus `warm`: a device uint32[4 * n_pairs] array, one slot per pair, carried
 * from call to call (e.g. simulation frames; the same pair at the same index).  On entry a slot holds
 * the support codes (ia | ib << 16) of the simplex the pair's previous call ended GJK with, or
 * 0xFFFFFFFF (fill the array with 0xFF bytes for a first call).  When that simplex, rebuilt from the
 * current vertices, holds the origin strictly inside (every face more than 1e-6 from it), the pair
 * is a hit and EPA starts from it, skipping GJK; otherwise the reference GJK runs.  A pair that
 * missed is marked 0xFFFFFFFE (first word) and runs the reference GJK on its next call.  On exit
 * every slot holds this call's simplex (hits), the miss mark, or 0xFFFFFFFF (errors).  Pairs that
 * are not warm-started are bit-exact with gjkepa_batch_device (hit flags always are); warm-started
 * hits agree with a cold call within EPA's own tolerance (a different start polytope), not bit for
 * bit. */
int gjkepa_batch_warm_device(int32_t version, double tol_ff, int32_t vert_dtype, int32_t precision,
                             const void* verts, const int64_t* hull_off, const int32_t* hull_cnt,
                             const int32_t* pairs, int64_t n_pairs,
                             void* out, void* workspace, int64_t workspace_bytes,
                             uint32_t* warm, void* stream);

/* ---- separation distance of non-colliding pairs -----------------------------------------------
 * The other half of the narrow phase: for every pair of a batch that does not collide, how far apart
 * the two hulls are and which two points are closest (speculative contacts, contact margins, step
 * control, clearance).  The reference has no such query: GJKEPA leaves nearest_points_ at 0 for a miss
 * (GCLIB_GJKEPA.f90:66-77, :87, :125).  This is a distance GJK in fp64 (vertices stored as fp32 or
 * fp64) on the GJK tiers' group shapes, independent of the contact records' bit-exact recipe:
 *   v = a_0 - b_0; each iteration takes the support point w of A - B along -v (first maximum on ties),
 *   stops when the gap v.v - v.w is within 1e-10 v.v or w is already a simplex vertex, and otherwise
 *   replaces the simplex by its sub-simplex closest to the origin (at most 3 vertices).  A tetrahedron
 *   around the origin, or |v| below 1e-12 of the simplex's scale, is an overlap.  There is no sphere
 *   pre-test exit, and at most 64 iterations (then GJKEPA_STATUS_DIST_MAXITER with the bounds so far).
 * max_distance: every iteration has the lower bound lb = v.w / |v|; a pair stops as soon as
 *   lb > max_distance, flagged FAR with distance = lb (so FAR means exactly that the last lower bound
 *   exceeds max_distance, also for a pair that would have converged in that iteration).  +inf: none.
 * records: NULL, or the contact records gjkepa_batch_device wrote for the same pair list (precision
 *   records_precision).  Pairs whose collision byte is set are not computed: flag HIT, distance 0.
 *   With NULL the kernel finds overlapping pairs itself and flags them OVERLAP.
 *
 * One record per pair.  A separated pair's record certifies itself: point_a = sum_k lambda[k] a[ia_k]
 * and point_b = sum_k lambda[k] b[ib_k] (ia_k | ib_k << 16 = code[k], lambda >= 0, sum 1) lie in the
 * hulls, so |point_a - point_b| bounds the distance from above, and min_i normal.a_i - max_j normal.b_j
 * bounds it from below.
 *   distance   separation; 0 for OVERLAP / HIT; the lower bound lb for FAR
 *   point_a/b  closest points on hull A / hull B (FAR: of the simplex so far; 0 for OVERLAP / HIT)
 *   normal     (point_a - point_b) / |point_a - point_b|, unit; 0 when distance is 0
 *   lambda     barycentric weights of the final simplex (unused entries 0)
 *   code       ia | ib << 16 per simplex vertex, the warm-start convention (unused 0xFFFFFFFF)
 *   n_simplex  1..3 (0 when not separated)
 *   status     GJKEPA_STATUS_OK, _BAD_INPUT (the batch's rules) or _DIST_MAXITER
 *   flags      GJKEPA_DIST_OVERLAP | _HIT | _FAR
 *   iters      GJK iterations */
#define GJKEPA_STATUS_DIST_MAXITER 5  /* distance GJK hit its 64-iteration cap: best bounds so far */
#define GJKEPA_DIST_OVERLAP 1   /* the hulls overlap or touch (found by the distance kernel itself) */
#define GJKEPA_DIST_HIT     2   /* skipped: the pair's contact record says collision */
#define GJKEPA_DIST_FAR     4   /* stopped early: the lower bound in `distance` exceeds max_distance */
typedef struct gjkepa_distance_f64 {
    double   distance;
    double   point_a[3];
    double   point_b[3];
    double   normal[3];
    double   lambda[3];
    uint32_t code[3];
    int8_t   n_simplex;
    int8_t   status;
    int8_t   flags;
    int8_t   reserved;
    uint32_t iters;
    uint32_t pad;
} gjkepa_distance_f64;           /* 128 bytes */

/* Size in bytes of one distance record (128). */
int gjkepa_distance_record_bytes(void);
/* Bytes of device workspace for n_pairs pairs (the tier launches' work counters, reset by the call
 * itself; 256-byte aligned); negative for n_pairs < 0. */
int64_t gjkepa_distance_workspace_bytes(int64_t n_pairs);
/* Device buffers, asynchronous on `stream` (hipStream_t or NULL): no allocation, no synchronisation,
 * every launch on that stream only (a captured graph is a linear chain).  The natural pipeline is
 * gjkepa_batch_device followed by this call on the same stream with `records` = the batch's `out`.
 * Deterministic: no atomics touch results.  Records nothing for gjkepa_launch_timing.
 * GJKEPA_E_ARG for a bad dtype, a bad records_precision with records != NULL, a null pointer, or a NaN
 * or negative max_distance; GJKEPA_E_WORKSPACE for a workspace below gjkepa_distance_workspace_bytes. */
int gjkepa_distance_batch_device(int32_t vert_dtype, const void* verts, const int64_t* hull_off,
                                 const int32_t* hull_cnt, const int32_t* pairs, int64_t n_pairs,
                                 const void* records, int32_t records_precision,
                                 double max_distance, void* out, void* workspace, int64_t workspace_bytes,
                                 void* stream);
/* Host buffers, blocking; the pool arguments and checks of gjkepa_batch.  records: NULL or n_pairs
 * contact records (host memory) of precision records_precision. */
int gjkepa_distance_batch(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                          const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                          const int32_t* pairs, int64_t n_pairs,
                          const void* records, int32_t records_precision, double max_distance,
                          void* out, int32_t device);

/* ---- linear cast (time of impact) of moving pairs ---------------------------------------------
 * The third question about a pair: hull B translates relative to hull A by d = motion[3k .. 3k+2]
 * (B's displacement minus A's over the step; fp64, always 3 doubles per pair), B(t) = B + t d for t in
 * [0, 1]: do the hulls come within `tolerance` (an absolute distance tau, finite and > 0) of each
 * other, when first, and where?  A ray cast is the case of a one-vertex hull A.  Linear motion only:
 * angular motion is out of scope (of this entry: gjkepa_cast_rigid_batch below casts spinning bodies).
 * Conservative advancement in fp64 over the distance GJK above, on the same group shapes:
 *   t = 0; at each step the distance GJK runs on A and B + t d (Minkowski points a - b - t d), the
 *   simplex carried from the step before by its codes.  OVERLAP at t = 0: START.  A separation
 *   |point_a - point_b| <= tau: START at step 0, IMPACT with toi = t later.  Otherwise, with n the unit
 *   normal from B to A, s = n.d and lb the GJK's support gap along n: s <= 0 is a MISS (the plane keeps
 *   separating); else dt = (lb - tau / 2) / s, t + dt >= 1 is a MISS, and t += dt leaves a gap of
 *   tau / 2 along n, so every visited time is certified free of contact.
 *   GJKEPA_STATUS_CAST_MAXITER (no flag, toi = the last time certified free) after 32 advancement
 *   steps, a step without progress, an OVERLAP after the first step (tau at the resolution of fp64 for
 *   the pair) or an inner distance run at its 64-iteration cap.
 * A caller can always advance by toi d: toi = 1 for a MISS.  A pair whose closest approach lies between
 * tau / 2 and tau may be reported either way.  The time of impact holds for any tau; the record's
 * normal is the direction between two witness points about tau apart, so the plane certificate below
 * needs tau above about 1e-7 of the coordinates' magnitude (tau^2 > 2^-52 * magnitude * hull extent).
 * records: as for gjkepa_distance_batch_device; pairs whose collision byte is set are not computed:
 *   flag SKIPPED, toi 0.  Bad hull counts, non-finite vertices and a non-finite motion component give
 *   GJKEPA_STATUS_BAD_INPUT for that pair (bad counts first, then SKIPPED, then the values).
 *
 * One record per pair, in the distance record's layout.  An IMPACT record certifies itself: point_a =
 * sum_k lambda[k] a[ia_k] and point_b = sum_k lambda[k] b[ib_k] + toi d lie in A and B(toi) and are at
 * most tau apart; min_i normal.a_i - max_j normal.b_j - toi normal.d > 0; and normal.d > 0, so the same
 * plane separates the hulls at every earlier t.  A MISS record's normal is that of a plane which still
 * separates at t = 1: min_i normal.a_i - max_j normal.b_j - normal.d > 0.
 *   toi        time of impact; 1 for a MISS; 0 for START / SKIPPED / bad input
 *   point_a/b  witness points at time toi in world coordinates (IMPACT, separated START; else 0)
 *   normal     unit, from B to A (IMPACT, separated START, MISS; else 0)
 *   lambda, code, n_simplex   the witness points' simplex, as in the distance record (else 0 /
 *              0xFFFFFFFF / 0)
 *   status     GJKEPA_STATUS_OK, _BAD_INPUT or _CAST_MAXITER
 *   flags      GJKEPA_CAST_IMPACT, _START or _SKIPPED; a MISS has none
 *   iters      GJK iterations over all steps;  steps: advancement steps taken */
#define GJKEPA_STATUS_CAST_MAXITER 6  /* the cast stopped undecided: toi = the last time certified free */
#define GJKEPA_CAST_IMPACT  1   /* the hulls come within tolerance at toi, 0 < toi < 1 */
#define GJKEPA_CAST_START   2   /* within tolerance, or overlapping, at t = 0 */
#define GJKEPA_CAST_SKIPPED 4   /* skipped: the pair's contact record says collision */
typedef struct gjkepa_cast_f64 {
    double   toi;
    double   point_a[3];
    double   point_b[3];
    double   normal[3];
    double   lambda[3];
    uint32_t code[3];
    int8_t   n_simplex;
    int8_t   status;
    int8_t   flags;
    int8_t   reserved;
    uint32_t iters;
    uint32_t steps;
} gjkepa_cast_f64;               /* 128 bytes */

/* Size in bytes of one cast record (128). */
int gjkepa_cast_record_bytes(void);
/* Bytes of device workspace for n_pairs pairs (work counters, reset by the call itself; 256-byte
 * aligned); negative for n_pairs < 0. */
int64_t gjkepa_cast_workspace_bytes(int64_t n_pairs);
/* Device buffers, asynchronous on `stream` (hipStream_t or NULL): no allocation, no synchronisation,
 * every launch on that stream only (a captured graph is a linear chain).  Deterministic.  Records
 * nothing for gjkepa_launch_timing.  n_pairs == 0 returns 0.
 * GJKEPA_E_ARG for a bad dtype, a null pointer, a bad records_precision with records != NULL, or a
 * tolerance that is NaN, infinite or <= 0; GJKEPA_E_WORKSPACE for a workspace below
 * gjkepa_cast_workspace_bytes. */
int gjkepa_cast_batch_device(int32_t vert_dtype, const void* verts, const int64_t* hull_off,
                             const int32_t* hull_cnt, const int32_t* pairs, int64_t n_pairs,
                             const double* motion, double tolerance,
                             const void* records, int32_t records_precision,
                             void* out, void* workspace, int64_t workspace_bytes, void* stream);
/* Host buffers, blocking; the pool arguments and checks of gjkepa_distance_batch.  motion: 3 n_pairs
 * doubles.  records: NULL or n_pairs contact records (host memory) of precision records_precision. */
int gjkepa_cast_batch(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                      const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                      const int32_t* pairs, int64_t n_pairs, const double* motion, double tolerance,
                      const void* records, int32_t records_precision, void* out, int32_t device);

/* ---- rigid-motion cast (time of impact under rotation) and the pose that goes with it ----------
 * The linear cast above with both bodies in full rigid motion.  A body is a hull of the pool; its motion
 * over the step is GJKEPA_MOTION_DOUBLES = 9 doubles at body_motion[9 h] (per hull, not per pair: pair
 * (a, b) reads blocks a and b):
 *   v[3]  displacement of the pivot over the step
 *   w[3]  rotation vector: angular velocity times the step
 *   c[3]  pivot in world coordinates at t = 0, normally the centre of mass
 * Path.  For t in [0, 1] a vertex p of the body is at
 *   h = (0.5 t) w;  q = p - c;  u = h x q;  g = u + h x u;  f = 2 / (1 + h.h)
 *   p(t) = (p + t v) + f g
 * in fp64 without FMA contraction, exactly as written (csrc/rigid_pose.h): the rotation of the
 * unnormalised quaternion (1, h) about the pivot, the pose the first-order update q <- normalize(q +
 * 1/2 t w q) produces.  One division, no sin or cos: host and device give the same bytes.  t = 0 gives p
 * exactly; w = 0 gives p + t v exactly.  The axis is w / |w| throughout and the angle is theta(t) =
 * 2 atan(t |w| / 2), below half a turn, with theta'(t) = |w| / (1 + t^2 |w|^2 / 4) <= |w|.  A caller who
 * integrates with the exponential map by an angle theta passes |w| = 2 tan(theta / 2).
 * Cast.  Conservative advancement in fp64 over the distance GJK on A(t) and B(t).  At a visited time the
 * GJK runs on the Minkowski points a_ia(t) - b_ib(t), the simplex carried by its codes (a valid start,
 * reduced from scratch).  The support of a posed hull along dir is taken on the unposed vertices along
 * R(t)^T dir (the same formula with -h applied to dir).  With n the unit normal from B to A, lb the
 * support gap along n and rho_X = max_i |x_i - c_X|, the closing rate is
 *   s = n.(v_B - v_A) + |n x w_A| rho_A + |n x w_B| rho_B
 * (the velocity of a vertex along the fixed n is theta' r(t).(n x k) <= |w| |n x k| |r|: a spin about
 * the contact normal costs nothing).  OVERLAP at t = 0: START.  Separation <= tau: START at step 0,
 * IMPACT with toi = t later.  s <= 0: MISS (the plane n keeps separating).  Otherwise dt = (lb - tau / 2)
 * / s; t + dt >= 1 is a MISS, n still separating the posed hulls at t = 1 by at least tau / 2; else
 * t += dt.  GJKEPA_STATUS_CAST_MAXITER with toi = the last time certified free after 64 advancement
 * steps, a step without progress, an OVERLAP after the first step or an inner run at its 64-iteration
 * cap.  A pair whose closest approach lies between tau / 2 and tau may be reported either way.
 * Record: gjkepa_cast_f64.  point_a / point_b are the witness points at toi in world coordinates, both
 * posed; normal points from B to A (IMPACT, separated START) or is the normal of the plane separating at
 * t = 1 (MISS); lambda, code, n_simplex as before (codes hold unposed vertex indices); steps <= 64.
 * records and SKIPPED as for the linear cast.  GJKEPA_STATUS_BAD_INPUT for a pair with a hull count
 * outside 1 .. GJKEPA_MAX_HULL_VERTS, a non-finite vertex or a non-finite value among its 18 motion
 * doubles (bad counts first, then SKIPPED, then the values).
 * Limit.  The bound sees a body's spin through rho, its farthest vertex from the pivot: a large body
 * turning about a distant pivot converges slowly and may end as CAST_MAXITER, toi still certified free.
 * Pivots belong at each body's own centre.
 * After the cast, move the bodies with gjkepa_pose_pool: a different rotation formula voids the
 * certificate. */
#define GJKEPA_MOTION_DOUBLES 9
/* Bytes of device workspace (as gjkepa_cast_workspace_bytes); negative for n_pairs < 0. */
int64_t gjkepa_cast_rigid_workspace_bytes(int64_t n_pairs);
/* Device buffers, asynchronous on `stream`: the contract of gjkepa_cast_batch_device (three tier launches
 * after the counter reset, nothing recorded for gjkepa_launch_timing, deterministic, a captured graph is
 * a linear chain; the same error rules).  body_motion: device, 9 doubles per hull of the pool. */
int gjkepa_cast_rigid_batch_device(int32_t vert_dtype, const void* verts, const int64_t* hull_off,
                                   const int32_t* hull_cnt, const int32_t* pairs, int64_t n_pairs,
                                   const double* body_motion, double tolerance,
                                   const void* records, int32_t records_precision,
                                   void* out, void* workspace, int64_t workspace_bytes, void* stream);
/* Host buffers, blocking; the pool arguments and checks of gjkepa_cast_batch.  body_motion: 9 n_hulls
 * doubles. */
int gjkepa_cast_rigid_batch(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                            const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                            const int32_t* pairs, int64_t n_pairs, const double* body_motion, double tolerance,
                            const void* records, int32_t records_precision, void* out, int32_t device);
/* Pose a hull pool along the same path: verts_out = every vertex of every hull h at time[h] (time ==
 * NULL: t = 1), at the input pool's offsets.  out_dtype GJKEPA_DTYPE_F64 is exactly the cast's arithmetic,
 * GJKEPA_DTYPE_F32 that rounded once.  verts_out == verts_in is allowed when the dtypes are equal.
 * status: NULL or one int8 per hull, GJKEPA_STATUS_OK or _BAD_INPUT (a count outside 1 ..
 * GJKEPA_MAX_HULL_VERTS, or a non-finite motion, time or vertex); nothing is written for a BAD_INPUT hull.
 * Asynchronous on `stream`, one launch, no allocation.  n_hulls == 0 returns 0.  GJKEPA_E_ARG for a bad
 * dtype, a null pointer, or in place with different dtypes. */
int gjkepa_pose_pool_device(int32_t in_dtype, const void* verts_in, const int64_t* hull_off,
                            const int32_t* hull_cnt, int64_t n_hulls, const double* body_motion,
                            const double* time, int32_t out_dtype, void* verts_out, int8_t* status, void* stream);
/* Host buffers, blocking; the pool checks of gjkepa_cast_batch without a pair list.  verts_out holds
 * n_vert_scalars scalars of out_dtype; the scalars of no hull, and of BAD_INPUT hulls, keep what the caller
 * put there. */
int gjkepa_pose_pool(int32_t in_dtype, const void* verts_in, int64_t n_vert_scalars,
                     const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                     const double* body_motion, const double* time, int32_t out_dtype, void* verts_out,
                     int8_t* status, int32_t device);

/* ---- swept broad phase: the pair list of the casts ------------------------------------------------
 * gjkepa_broadphase lists the pairs that are close at t = 0; a cast exists for the pair that is far apart
 * now and meets during the step.  This entry lists, from the pool and the per-hull motion blocks of the
 * rigid cast (v, w, c), exactly the pairs whose swept bounding balls can come within `tolerance` during
 * t in [0, 1]: the pair list of gjkepa_cast_rigid_batch (and, with w = 0, of the linear cast).
 * Definition (csrc/swept_sphere.h; fp64, no FMA contraction, dot(a, b) = a.x b.x + a.y b.y + a.z b.z, the
 * operation order written here, so a restatement gives the same bits).  Hull h with motion block
 * m = body_motion + 9 h is valid when its count is in 1 .. GJKEPA_MAX_HULL_VERTS, every vertex is finite
 * and every double of m is finite; an invalid hull takes part in no pair.
 *   rho_h = sqrt(max_i dot(q_i, q_i)), q_i = x_i - c, the vertices widened to double (the rigid cast's
 *   pivot radius: an order-free maximum, then one square root).  Under the cast's path the pivot moves on
 *   c + t v and every vertex stays within rho_h of it, so w does not enter.
 * A pair (a < b) of valid hulls passes when
 *   d = c_a - c_b;  e = v_a - v_b;  ee = dot(e, e);  de = dot(d, e)
 *   s = 0            if ee == 0 or de >= 0
 *       1            else if -de >= ee
 *       (-de) / ee   otherwise
 *   m = (d.x + s e.x, d.y + s e.y, d.z + s e.z);   dist = sqrt(dot(m, m))
 *   reach = (rho_a + rho_b) + tolerance
 *   lim = reach + 1e-9 * ((reach + max|d_k|) + max|e_k|)
 *   pass iff dist <= lim
 * dist is the closest approach of the two ball centres over the step.  The 1e-9 term is part of the
 * definition: it makes the list a superset of the pairs the casts can report as IMPACT or START at this
 * tolerance despite rounding in either place.  Both that and the independence from
 * long_radius below hold while coordinates stay below about 1e5 times (reach + |d| + |e|), i.e. bodies of
 * size 1 out to coordinates of 1e5: beyond that the cast's own posed vertices are coarser than the slack, and
 * past about 2^28 grid cells from the origin the grid (not the long path) may miss a passing pair.
 * Output: the contract of gjkepa_broadphase_device.  The passing pairs in ascending (a, b) order;
 * *n_pairs = n_found (device int64 for the device entry); the list holds min(n_found, max_pairs) of them,
 * distinct and ascending, a subset when cut; the final sort runs over max_pairs padded keys.
 * long_radius (>= 0, +inf for none) is tuning only and never changes the list: the grid's cell edge follows
 * the largest enclosing radius R = rho + 0.5 |v|, so one bullet would turn the grid into an all-pairs test.
 * A valid body with R > long_radius leaves the grid and is tested against every valid body instead; choose a
 * few typical body diameters.  0 tests all pairs.
 * Limit.  The test sees a body through rho about its pivot: a pivot far from the body inflates the list, as
 * it slows the cast.  Pivots belong at each body's own centre.
 * Errors: GJKEPA_E_ARG for a bad dtype, a null pointer, a tolerance that is NaN, infinite or <= 0, a
 * long_radius that is NaN or negative; GJKEPA_E_WORKSPACE for a short workspace.  n_hulls == 0 gives
 * *n_pairs = 0 and returns 0. */
int64_t gjkepa_broadphase_swept_workspace_bytes(int64_t n_hulls, int64_t max_pairs);
/* Device buffers, asynchronous on `stream`: no allocation, no synchronisation, no result that depends on an
 * atomic (graph-capturable; replay after rewriting body_motion in place).  n_pairs is a device int64. */
int gjkepa_broadphase_swept_device(int32_t vert_dtype, const void* verts, const int64_t* hull_off,
                                   const int32_t* hull_cnt, int64_t n_hulls, const double* body_motion,
                                   double tolerance, double long_radius,
                                   int32_t* pairs, int64_t max_pairs, int64_t* n_pairs,
                                   void* workspace, int64_t workspace_bytes, void* stream);
/* Host buffers, blocking: the pool arguments and checks of gjkepa_broadphase.  body_motion: 9 n_hulls
 * doubles. */
int gjkepa_broadphase_swept(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                            const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                            const double* body_motion, double tolerance, double long_radius,
                            int32_t* pairs, int64_t max_pairs, int64_t* n_pairs, int32_t device);

/* ---- event list and per-body clamp of a moving step -------------------------------------------------
 * The casts leave one record per candidate pair, MISS or not, in pair order.  This pass turns the cast
 * records of a pair list (and, for the pairs already in contact, the batch's contact records) into what
 * happened during the step, in the order it happened: a dense list of events sorted by time, and for every
 * body the earliest event that stops it, as the time gjkepa_pose_pool takes per hull.
 * Definition (csrc/event_record.h is its text, for host and device).  The kind of a pair comes from its cast
 * record alone (gjkepa_cast_f64 of the linear or the rigid cast); the first rule that applies wins:
 *   1. status GJKEPA_STATUS_BAD_INPUT     no event, counted as BAD
 *   2. flag GJKEPA_CAST_SKIPPED           GJKEPA_EVENT_HIT, time 0
 *   3. status GJKEPA_STATUS_CAST_MAXITER  GJKEPA_EVENT_UNDECIDED, time = toi, the last time certified free
 *   4. flag GJKEPA_CAST_START             GJKEPA_EVENT_START, time 0
 *   5. flag GJKEPA_CAST_IMPACT            GJKEPA_EVENT_IMPACT, time = toi
 *   6. otherwise (a MISS)                 no event
 * time is toi when toi > 0, else +0.0 (a NaN toi gives 0), so the bits of time, read as uint64, order like
 * the value.
 *   time       0 for HIT / START; toi for IMPACT / UNDECIDED
 *   point_a/b, normal   START, IMPACT, UNDECIDED: the cast record's, bit for bit.  HIT: the contact record's
 *              two nearest_points and its collision_normal (an F32 record's widened)
 *   depth      HIT: the contact record's penetration_depth, else 0
 *   a, b       the pair's hull indices;  pair: its index in the input list
 *   kind       GJKEPA_EVENT_*
 *   status     the status of the record the geometry came from (the cast's; HIT: the contact's)
 * With records == NULL a HIT event's point_a, point_b, normal, depth and status are zero.
 * The list.  events[k] for k < min(*n_events, max_events) holds the events in ascending (time, pair) order.
 * *n_events is the full count, also when the list is cut, and equals counts[0] + .. + counts[3]; counts[5] =
 * HIT, START, IMPACT, UNDECIDED, BAD.  Nothing is written at or past events[max_events].  An event's rank is
 * its position in the full order, whether or not it fits in the list.
 * The clamp.  body_event[h] is the smallest rank among the IMPACT and UNDECIDED events that name hull h as a
 * or b, or -1 if there is none; body_time[h] is that event's time, or 1.0 if there is none.  Both come from
 * the full order and do not depend on max_events.  Contact at t = 0 does not clamp: HIT and START events are
 * the contact solver's matter (gjkepa_manifold_batch), and a resting box would otherwise never move.
 * What the clamp guarantees, and what it does not.  Body h posed at body_time[h] is at or before the time of
 * impact of every listed pair it is in.  Against a partner that does not move (v = w = 0) the cast's
 * certificate therefore holds and the two are at least tolerance / 2 apart.  Two moving bodies clamped to
 * different times are not certified against each other: that policy is the caller's.
 * Method: a key pass (each pair's flag, status and toi are read once; per-tile counts of the five classes,
 * summed in a fixed order), a stable radix sort of (time bits, pair) (rocPRIM), and an emit pass in which rank
 * k gathers its pair's records, writes the event, and, for an IMPACT or UNDECIDED, takes the minimum of k
 * into body_event[a] and body_event[b]: the pass's only atomic, and a minimum does not depend on the order of
 * arrival.  Deterministic. */
#define GJKEPA_EVENT_HIT       1   /* in contact at t = 0 by the batch's collision byte (the cast skipped the pair) */
#define GJKEPA_EVENT_START     2   /* within tolerance, or overlapping, at t = 0 by the cast itself */
#define GJKEPA_EVENT_IMPACT    3   /* the hulls come within tolerance at time */
#define GJKEPA_EVENT_UNDECIDED 4   /* the cast stopped undecided: free up to time */
typedef struct gjkepa_event_f64 {
    double   time;
    double   point_a[3];
    double   point_b[3];
    double   normal[3];
    double   depth;
    int32_t  a, b;
    int32_t  pair;
    int8_t   kind;
    int8_t   status;
    int8_t   reserved[2];
    uint32_t pad[6];
} gjkepa_event_f64;              /* 128 bytes */

/* Size in bytes of one event record (128). */
int gjkepa_event_record_bytes(void);
/* Bytes of device workspace for n_pairs pairs (keys, pair indices, tile counts, sort scratch; 256-byte
 * aligned; n_hulls does not enter today); negative for a negative size or n_pairs above 2^31 - 1. */
int64_t gjkepa_events_workspace_bytes(int64_t n_pairs, int64_t n_hulls);
/* Device buffers, asynchronous on `stream` (hipStream_t or NULL): no allocation, no synchronisation, every
 * launch on that stream only (a captured graph is a linear chain).
 * pairs, cast_records: the pair list and its n_pairs cast records.  records: NULL, or the list's contact
 * records of precision records_precision.  events: room for max_events records.  n_events, counts[5]: device
 * int64.  body_time (double), body_event (int32): n_hulls each, both NULL to skip.  Hull indices are trusted.
 * n_pairs == 0 gives *n_events = 0, zero counts, body_time = 1 and body_event = -1 for all n_hulls.
 * GJKEPA_E_ARG for a null required pointer, a bad records_precision with records != NULL, a negative size, a
 * size above 2^31 - 1 or exactly one of the two body pointers; GJKEPA_E_WORKSPACE for a workspace below
 * gjkepa_events_workspace_bytes. */
int gjkepa_events_device(const int32_t* pairs, int64_t n_pairs, int64_t n_hulls,
                         const void* cast_records,
                         const void* records, int32_t records_precision,
                         void* events, int64_t max_events,
                         int64_t* n_events, int64_t* counts,
                         double* body_time, int32_t* body_event,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- whole moving step (host buffers, blocking) -------------------------------------------------
 * gjkepa_broadphase_swept_device -> gjkepa_batch_device on the candidate list -> gjkepa_cast_rigid_batch_device
 * with the batch's records -> gjkepa_events_device, and, when verts_out is given, gjkepa_pose_pool_device with
 * time = body_time: the bytes those entries give when called one after the other.  The pool arguments and
 * checks of gjkepa_broadphase_swept; body_motion, tolerance, long_radius as there; version, tol_ff, precision
 * as for gjkepa_batch.  events: room for max_events records (the first of the list); *n_events the full count;
 * counts (5, may be NULL) as above; *n_candidates (may be NULL) = pairs of the swept list; body_time (n_hulls,
 * may be NULL); verts_out (may be NULL): n_vert_scalars scalars of vert_dtype, the pool posed at body_time
 * (the scalars of no hull, and of BAD_INPUT hulls, hold the input's values). */
int gjkepa_collide_moving(int32_t version, double tol_ff, int32_t vert_dtype, int32_t precision,
                          const void* verts, int64_t n_vert_scalars,
                          const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                          const double* body_motion, double tolerance, double long_radius,
                          void* events, int64_t max_events, int64_t* n_events,
                          int64_t* counts, int64_t* n_candidates,
                          double* body_time, void* verts_out, int32_t device);

/* ---- contact manifold (up to 4 points) of colliding pairs --------------------------------------
 * The fourth question about a pair, for the pairs a batch calls a collision: a contact patch instead of
 * the reference's one collision_point, as a solver needs for two boxes resting face to face.  It is
 * built from the pair's contact record and the two hulls, in fp64 (vertices stored as fp32 or fp64),
 * with n = the record's collision_normal as doubles, unmodified (an F32 record's is widened):
 *   1. heights   hA = max_i n.a_i, hB = min_j n.b_j (a height of -0 counts as +0), depth = hA - hB.
 *   2. features  FA = { i : n.a_i >= hA - margin }, FB = { j : n.b_j <= hB + margin }, each in ascending
 *      vertex index; margin is an absolute length, finite and >= 0.  At most
 *      GJKEPA_MANIFOLD_MAX_FEATURE = 32 vertices per hull are used: of a feature of m > 32 vertices the
 *      vertices of rank r (in index order) with r % ceil(m / 32) == 0, with flag DECIMATED.  A subset of
 *      a hull's vertices lies inside the hull, so the manifold stays conservative, and a ring (a prism's
 *      face) thins out evenly.
 *   3. frame     e = the coordinate axis of the smallest |n| component (the first of equals),
 *      u = (e x n) / |e x n|, w = n x u; 2-D coordinates (x, y) = ((p - o).u, (p - o).w) about
 *      o = a[FA[0]]; s = the largest |x| or |y| over the vertices used of both features, the scale of
 *      every tolerance below.
 *   4. footprints  the strict 2-D convex hull of each feature, counter-clockwise seen from +n, from the
 *      lexicographically smallest (x, y, index); collinear points are dropped, the farthest kept.  A
 *      footprint is a point, a segment or a polygon.
 *   5. candidates  A's footprint vertices no more than 1e-9 s outside every edge line of B's footprint
 *      (a segment footprint: within 1e-9 s across it and along its length; a point footprint: within
 *      1e-9 s of it), then B's against A's footprint, then every proper crossing (both parameters strictly
 *      inside (0, 1)) of an edge of A with an edge of B in edge order; edges r, q with
 *      |r x q| <= 1e-9 |r| |q| count as parallel and do not cross.  A segment footprint has one edge.
 *   6. reduction to at most four points, each an argmax over the candidates in that order, the first of
 *      equals: p0 = the lexicographically smallest (x, y); p1 = the farthest from p0, kept if farther
 *      than 1e-9 s; pL / pR = the candidates of the largest triangle (p0, p1, c) to the left / right of
 *      p0 -> p1, each kept if the triangle's area exceeds 1e-9 s^2.  Reported counter-clockwise:
 *      p0, pR, p1, pL.  Without any candidate the record holds one point, the contact record's
 *      collision_point projected onto A's support plane, with flag FALLBACK and no code.
 *   7. lifting   every point is moved along n onto A's support plane n.x = hA; its partner on B is
 *      point - depth n.  depth is uniform over the patch: within 2 margin of the depth measured at any
 *      one of the points (the features are margin thick each).
 *   8. code per point  ia | ib << 16 as for the warm start and the distance record: a footprint vertex
 *      of A ia | 0xFFFF << 16, of B 0xFFFF | ib << 16, a crossing the start vertices (in counter-clockwise
 *      order) of its two edges.  Stable from frame to frame while the features are.  Unused: 0xFFFFFFFF.
 * The constants 1e-9 and 32 and the pick rule are part of the definition (csrc/manifold_clip.h is its
 * text, for host and device).
 * Computed for the pairs whose contact record has the collision byte set, status GJKEPA_STATUS_OK and a
 * finite, non-zero normal; every other pair gets flag NO_HIT, no points and zeroed fields (codes
 * 0xFFFFFFFF).  A hull count outside 1 .. GJKEPA_MAX_HULL_VERTS gives GJKEPA_STATUS_BAD_INPUT (zeroed
 * fields, no flag) whatever the record says; a non-finite vertex gives it for a pair that would be
 * computed.
 *   depth      hA - hB along normal
 *   normal     n, as read from the contact record
 *   point      n_points points on A's support plane, counter-clockwise seen from +normal; the rest 0
 *   code       per point, as in step 8
 *   n_feat_a/b vertices of the two features before decimation
 *   area       shoelace area of the reported polygon in the plane; 0 below three points */
#define GJKEPA_MANIFOLD_MAX_FEATURE 32
#define GJKEPA_MANIFOLD_NO_HIT    1   /* not computed: the contact record is no usable collision */
#define GJKEPA_MANIFOLD_DECIMATED 2   /* a feature had more than GJKEPA_MANIFOLD_MAX_FEATURE vertices */
#define GJKEPA_MANIFOLD_FALLBACK  4   /* no candidate: the one point is the projected collision_point */
#define GJKEPA_MANIFOLD_AT_TOI    8   /* built from a cast record, on the hulls posed at its toi (gjkepa_manifold_cast_batch) */
typedef struct gjkepa_manifold_f64 {
    double   depth;
    double   normal[3];
    double   point[4][3];
    uint32_t code[4];
    uint16_t n_feat_a;
    uint16_t n_feat_b;
    int8_t   n_points;
    int8_t   status;
    int8_t   flags;
    int8_t   reserved;
    double   area;
} gjkepa_manifold_f64;           /* 160 bytes */

/* Size in bytes of one manifold record (160). */
int gjkepa_manifold_record_bytes(void);
/* Bytes of device workspace for n_pairs pairs (work counters, reset by the call itself; 256-byte
 * aligned); negative for n_pairs < 0. */
int64_t gjkepa_manifold_workspace_bytes(int64_t n_pairs);
/* Device buffers, asynchronous on `stream` (hipStream_t or NULL): no allocation, no synchronisation,
 * every launch on that stream only (a captured graph is a linear chain; chain it after
 * gjkepa_batch_device with that call's output as `records`).  Deterministic.  Records nothing for
 * gjkepa_launch_timing.  n_pairs == 0 returns 0.
 * records: required, the n_pairs contact records (gjkepa_contact_f64 / _f32 by records_precision) of
 *   the same pair list.
 * GJKEPA_E_ARG for a bad dtype or records_precision, a margin that is NaN, infinite or negative, or a
 * null pointer (records among them); GJKEPA_E_WORKSPACE for a workspace below
 * gjkepa_manifold_workspace_bytes. */
int gjkepa_manifold_batch_device(int32_t vert_dtype, const void* verts, const int64_t* hull_off,
                                 const int32_t* hull_cnt, const int32_t* pairs, int64_t n_pairs,
                                 const void* records, int32_t records_precision, double margin,
                                 void* out, void* workspace, int64_t workspace_bytes, void* stream);
/* Host buffers, blocking; the pool arguments and checks of gjkepa_distance_batch.  records: n_pairs
 * contact records in host memory. */
int gjkepa_manifold_batch(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                          const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                          const int32_t* pairs, int64_t n_pairs,
                          const void* records, int32_t records_precision, double margin,
                          void* out, int32_t device);

/* ---- contact manifold at the time of impact: the patch of a moving step's events -----------------
 * The manifold above for the pairs a cast found: the patch of the two hulls posed at the pair's own time of
 * impact, along the cast record's normal, so a box that lands flat on a floor during the step reaches the
 * solver as four points and not as one witness point.  Inputs: the pool, a pair list, its n_pairs cast
 * records (gjkepa_cast_f64 of gjkepa_cast_rigid_batch), body_motion (9 doubles per hull: the blocks the cast
 * ran with), margin as above, and optionally the batch's contact records of the same list.  Output: one
 * gjkepa_manifold_f64 per pair, in pair order.  Per pair the first rule that applies wins:
 *   1. a hull count outside 1 .. GJKEPA_MAX_HULL_VERTS: GJKEPA_STATUS_BAD_INPUT (zeroed fields, codes
 *      0xFFFFFFFF, no flag).
 *   2. cast flag GJKEPA_CAST_SKIPPED: with records given, the pair is answered exactly as
 *      gjkepa_manifold_batch_device answers it from that contact record (n = collision_normal, the unposed
 *      hulls, fallback point collision_point): the same bytes; the motion blocks are not read.  With
 *      records == NULL: GJKEPA_MANIFOLD_NO_HIT.
 *   3. cast status GJKEPA_STATUS_BAD_INPUT: BAD_INPUT as in rule 1.
 *   4. cast status GJKEPA_STATUS_CAST_MAXITER: NO_HIT.
 *   5. flag GJKEPA_CAST_IMPACT or _START with a finite normal that is not zero: computed.  A non-finite vertex
 *      of either hull, a non-finite value among the pair's 18 motion doubles, or a toi that is NaN or outside
 *      [0, 1] gives BAD_INPUT.  (An overlapping START has a zero normal: rule 6.)
 *   6. anything else (a MISS): NO_HIT.
 * A computed pair runs steps 1 to 8 of the definition above unchanged, on these inputs:
 *   vertices   vertex i of hull X is pose_point(pose_state(v_X, w_X, t), c_X, p_i) with t = the record's toi
 *              (a START has toi 0), the arithmetic of csrc/rigid_pose.h as written: bit for bit what
 *              gjkepa_pose_pool with out_dtype GJKEPA_DTYPE_F64 gives for that hull at that time.
 *   normal     n = (-normal.x, -normal.y, -normal.z) of the cast record, negated exactly: the cast's normal
 *              points from B to A, the manifold's from A into B (depth = hA - hB).
 *   fallback   step 6's point is the cast record's point_a.
 * depth is then minus the support gap along the normal: <= 0, and at least -tolerance for a record the cast
 * certified.  The points lie on A's support plane at the time of impact, the partner on B is point - depth n,
 * and the codes hold unposed vertex indices, so they stay stable from frame to frame.  Flags are the
 * manifold's, plus GJKEPA_MANIFOLD_AT_TOI on every record computed from a cast record (rule 5); the records
 * of rule 2 carry what gjkepa_manifold_batch gives them.
 * A linear cast's records (gjkepa_cast_batch) are served by motion blocks with w = 0, v_A = 0 and v_B = the
 * pair's relative motion; a body that is in several linear-cast pairs with different relative motions has no
 * single block and is out of scope.
 * Limit.  Two bodies that the per-body clamp (gjkepa_events_device) stops at different times are not at
 * their pair's toi when posed at body_time; the patch describes the pair at its own toi, and what to do about
 * the difference is the caller's policy. */
/* Bytes of device workspace (as gjkepa_manifold_workspace_bytes); negative for n_pairs < 0. */
int64_t gjkepa_manifold_cast_workspace_bytes(int64_t n_pairs);
/* Device buffers, asynchronous on `stream`: the contract of gjkepa_manifold_batch_device (no allocation, no
 * synchronisation, one stream, three tier launches after the counter reset, deterministic, nothing recorded
 * for gjkepa_launch_timing; n_pairs == 0 returns 0).  body_motion (device, 9 doubles per hull of the pool) and
 * cast_records (device, n_pairs gjkepa_cast_f64) are required; records: NULL, or the list's contact records.
 * GJKEPA_E_ARG for a bad dtype, a bad records_precision with records != NULL, a margin that is NaN, infinite
 * or negative, or a null required pointer; GJKEPA_E_WORKSPACE for a workspace below
 * gjkepa_manifold_cast_workspace_bytes. */
int gjkepa_manifold_cast_batch_device(int32_t vert_dtype, const void* verts, const int64_t* hull_off,
                                      const int32_t* hull_cnt, const int32_t* pairs, int64_t n_pairs,
                                      const double* body_motion, const void* cast_records,
                                      const void* records, int32_t records_precision, double margin,
                                      void* out, void* workspace, int64_t workspace_bytes, void* stream);
/* Host buffers, blocking; the pool arguments and checks of gjkepa_cast_rigid_batch.  body_motion: 9 n_hulls
 * doubles; cast_records: n_pairs records; records: NULL or n_pairs contact records (host memory). */
int gjkepa_manifold_cast_batch(int32_t vert_dtype, const void* verts, int64_t n_vert_scalars,
                               const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                               const int32_t* pairs, int64_t n_pairs,
                               const double* body_motion, const void* cast_records,
                               const void* records, int32_t records_precision, double margin,
                               void* out, int32_t device);
/* The manifolds of an event list: out[k] = manifolds[events[k].pair] for k < min(*n_events, max_events);
 * nothing is written at or past that bound.  events, n_events (device int64), max_events: what
 * gjkepa_events_device left; manifolds: the gjkepa_manifold_f64 records of the same pair list; out: room for
 * max_events records.  Asynchronous on `stream`, one launch, no allocation (graph-capturable).  max_events == 0
 * returns 0.  GJKEPA_E_ARG for a negative max_events or a null pointer. */
int gjkepa_event_manifolds_device(const void* events, const int64_t* n_events, int64_t max_events,
                                  const void* manifolds, void* out, void* stream);
/* gjkepa_collide_moving with a patch per event (host buffers, blocking): after the event pass,
 * gjkepa_manifold_cast_batch_device on the candidate list with the batch's records, then
 * gjkepa_event_manifolds_device.  Every output it shares with gjkepa_collide_moving holds that call's bytes;
 * patches (room for max_events gjkepa_manifold_f64) [k] belongs to events[k]: a HIT event gets its contact
 * manifold, a START or IMPACT event the manifold at its time, an UNDECIDED event NO_HIT.  margin as for
 * gjkepa_manifold_batch.  GJKEPA_E_ARG also for a bad margin or, with max_events > 0, patches == NULL. */
int gjkepa_collide_moving_patches(int32_t version, double tol_ff, int32_t vert_dtype, int32_t precision,
                                  const void* verts, int64_t n_vert_scalars,
                                  const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                                  const double* body_motion, double tolerance, double long_radius,
                                  void* events, int64_t max_events, int64_t* n_events,
                                  int64_t* counts, int64_t* n_candidates,
                                  double* body_time, void* verts_out, double margin, void* patches,
                                  int32_t device);

/* ---- whole collision step (host buffers, blocking) ---------------------------------------------
 * The reference caller's `DO a; DO b = a+1; CALL GJKEPA(...)` over a pooled hull set in one call:
 * gjkepa_broadphase_device -> gjkepa_batch_device on the candidate list -> gjkepa_compact_hits_device.
 * Writes the first min(n, max_contacts) hits: pairs[2k], pairs[2k+1] = (a, b) (a < b, ascending)
 * and out[k] = that pair's record (gjkepa_contact_f64 / _f32 by precision), bit-exact with GJKEPA
 * on (p_a, p_b).  *n_contacts = hits found; *n_candidates (may be NULL) = pairs past the sphere test. */
int gjkepa_collide(int32_t version, double tol_ff, int32_t vert_dtype, int32_t precision,
                   const void* verts, int64_t n_vert_scalars,
                   const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                   int32_t* pairs, void* out, int64_t max_contacts,
                   int64_t* n_contacts, int64_t* n_candidates, int32_t device);

/* ---- multi-GPU (SURVEY.md §8 row e) ---------------------------------------------------------------
 * Pairs are independent: a job splits into contiguous shards of pairs, one per device, with no
 * exchange during compute.  The reference's own parallelism is the caller's OpenMP loop over GJKEPA
 * (GCLIB_GJKEPA.f90:9, :16, :55-60); these entries replace it across the GPUs of a node.
 *
 * gjkepa_shard_range: rank r of `world` owns pairs [first, first + count); shards differ by at most
 * one pair (the first n_pairs % world ranks get one more). */
int gjkepa_shard_range(int64_t n_pairs, int32_t world, int32_t rank, int64_t* first, int64_t* count);

/* One process, several devices (host buffers, blocking): gjkepa_batch's arguments plus a device list.
 * Shard s (gjkepa_shard_range over ndev) runs on devices[s] from its own host thread; only the hulls
 * the shard references are copied to that device; its records land at out[first .. first + count),
 * so `out` holds every record in pair order — bit-identical to one gjkepa_batch call.  The argument
 * checks are gjkepa_batch's, over the whole job, before any shard runs.  A device may appear more
 * than once: its shards then run one after the other. */
int gjkepa_batch_multi(int32_t version, double tol_ff, int32_t vert_dtype, int32_t precision,
                       const void* verts, int64_t n_vert_scalars,
                       const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
                       const int32_t* pairs, int64_t n_pairs,
                       void* out, const int32_t* devices, int32_t ndev);

/* One process per device (config C3): an RCCL communicator for the contact-record exchange.
 * Rank 0 creates the id (gjkepa_comm_unique_id), the caller broadcasts its GJKEPA_COMM_ID_BYTES bytes
 * (MPI_Bcast, torch.distributed, a file ...), every rank calls gjkepa_comm_init.  RCCL is bound at
 * run time (the copy already in the process, else librccl.so.1); GJKEPA_E_COMM if it is absent. */
#define GJKEPA_COMM_ID_BYTES 128
typedef struct gjkepa_comm gjkepa_comm;
int gjkepa_comm_unique_id(void* id);
int gjkepa_comm_init(gjkepa_comm** comm, int32_t world, int32_t rank, const void* id, int32_t device);
int gjkepa_comm_destroy(gjkepa_comm* comm);
/* Which RCCL the library bound ("process (...)", "librccl.so.1", or "unavailable"). */
const char* gjkepa_comm_backend(void);

/* All-gather of every rank's `count` contact records (device buffers; equal shards) into
 * all_records[world * count] in rank order: one ncclAllGather on `stream` (asynchronous; xGMI).
 * In place when shard_records == all_records + rank * count records. */
int gjkepa_allgather_records_device(gjkepa_comm* comm, int32_t precision, const void* shard_records,
                                    void* all_records, int64_t count, void* stream);

/* Last error message of the calling thread ("" if none). */
const char* gjkepa_last_error(void);

/* Library build string (kernels' target, caps, compile flags). */
const char* gjkepa_version_string(void);

/* ---- synthetic workload generator (deterministic, counter-based SplitMix64) ----
 * Fills a hull pool for `n_pairs` pairs with two private hulls per pair (hull 2k = p1_, 2k+1 = p2_):
 * vertices are unit vectors about the hull centre (all extreme), hull A centred at 0, hull B at
 * u*r with u uniform on S^2 and r ~ U[0, r_max].  Hull sizes are n_min..n_max (uniform integer;
 * n_min == n_max for fixed-size configs).  Values are rounded to fp32 so the fp32 and fp64 pools
 * hold identical numbers.  `first_pair` offsets the counter so shards of one logical job agree.
 * hull_off/hull_cnt/pairs are written for the generated pool (pairs are global hull indices of
 * this pool, i.e. 2k, 2k+1).  Pass verts == NULL to only compute sizes: returns the number of
 * vertex scalars the pool needs. */
int64_t gjkepa_synth_pairs(uint64_t seed, int64_t first_pair, int64_t n_pairs,
                           int32_t n_min, int32_t n_max, double r_max,
                           int32_t vert_dtype, void* verts,
                           int64_t* hull_off, int32_t* hull_cnt, int32_t* pairs);

/* Synthetic point clouds for the hull module: n ~ U{n_min..n_max} points per cloud, uniform in the
 * unit ball (shape 0) or on the unit sphere (shape 1); same conventions as gjkepa_synth_pairs
 * (counter-based per global cloud index, fp32-rounded; verts == NULL returns the scalar count). */
int64_t gjkepa_synth_clouds(uint64_t seed, int64_t first_cloud, int64_t n_clouds,
                            int32_t n_min, int32_t n_max, int32_t shape,
                            int32_t vert_dtype, void* verts,
                            int64_t* cloud_off, int32_t* cloud_cnt);

/* Synthetic scene for the broad phase: n_hulls hulls of n ~ U{n_min..n_max} unit-sphere vertices
 * (as gjkepa_synth_pairs' hull A) centred uniformly in the cube [0, box)^3; counter-based per
 * global hull index, fp32-rounded; verts == NULL returns the scalar count. */
int64_t gjkepa_synth_scene(uint64_t seed, int64_t first_hull, int64_t n_hulls,
                           int32_t n_min, int32_t n_max, double box,
                           int32_t vert_dtype, void* verts, int64_t* hull_off, int32_t* hull_cnt);

#ifdef __cplusplus
}
#endif
#endif /* GJKEPA_H */
