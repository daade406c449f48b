// mass_props.h — the mass properties of gjkepa_mass_batch(_device) and gjkepa_mass_pool: volume, centre of
// mass, inertia tensor, surface area and bounding radius of a convex hull given as outward triangles over a
// point cloud (include/gjkepa.h).
//
// A cloud has n points (widened to double) and F faces, int32 triples (a, b, c) in slot order with the hull
// module's outward winding.  o is the point named by the first index of the first face: it lies on the hull,
// so every tetrahedron (o, a, b, c) has a signed volume >= 0 and the sums below do not cancel.
// Per face, with A = p_a - o, B = p_b - o, C = p_c - o:
//     N = cross(sub(B, A), sub(C, B));  d = dot(A, cross(B, C));  S = (A + B) + C
// and the face's 14 terms are
//     t0      d
//     t1..3   d S_k                                                    k = x, y, z
//     t4..9   d (((S_i S_j + A_i A_j) + B_i B_j) + C_i C_j)            ij = xx, yy, zz, xy, xz, yz
//     t10     sqrt(dot(N, N))
//     t11..13 N_k
// Summation, the same whatever the launch: 64 strided partials, partial l adding faces
// l, l + 64, l + 128, .. in ascending order from +0.0; then an xor butterfly, P[l] = P[l] + P[l ^ s] for all
// l at once, s = 1, 2, 4, 8, 16, 32; the total T is P[0] (every partial holds the same value: a + b is b + a
// bit for bit).  Results:
//     volume = T0 / 6;  m = T[1..3] / (4 T0);  com = o + m
//     M_ij = T[4..9] / 120 - (volume m_i) m_j            second moments about com
//     inertia = (Myy + Mzz, Mxx + Mzz, Mxx + Myy, -Mxy, -Mxz, -Myz)   about com, world axes, unit density
//     area = 0.5 T10;  closure = max|T[11..13]| / T10    0 for a closed surface
//     radius = sqrt(max_i swept_q2(x_i, com)) over all n points: the rho of swept_sphere.h and of the rigid
//              cast for the pivot c = com, bit for bit
// Status, the first rule that applies wins: n outside 4 .. GJKEPA_HULL_MAX_POINTS -> BAD_INPUT; a hull status
// that is given and not OK -> that status; F outside 4 .. 2n - 4 -> BAD_INPUT; a face index outside [0, n) or a
// non-finite coordinate among the n points -> BAD_INPUT; T0 not finite or not > 0, or a result that is not
// finite -> DEGENERATE.  A record that is not OK is zero apart from its status.  No point is read through an
// index that has not been checked.
//
// Host and device code like swept_sphere.h, event_record.h and manifold_clip.h (plain fp64, no FMA
// contraction, the operation order written here): mass_kernel.hip runs the per-face and result text with the
// sums spread over lanes, mass_cloud below is the same definition in sequence (tests/mass_host.cpp), and
// tests/mass_ref.py restates it in numpy with the same bits.
#pragma once
#include <cstdint>

#include "../../include/gjkepa.h"
#include "swept_sphere.h"

namespace gkm {

using gkd::D3;

constexpr int kTerms = 14;
constexpr int kPartials = 64;

DS_HD bool finite_d(double x) { return x - x == 0.0; }      // false for NaN and +-inf

// rules 1 to 3: what the counts and the hull's status say before a face or a point is read
DS_HD int mass_precheck(int n, bool has_hull_status, int hull_status, int n_faces) {
    if (n < 4 || n > GJKEPA_HULL_MAX_POINTS) return GJKEPA_STATUS_BAD_INPUT;
    if (has_hull_status && hull_status != GJKEPA_STATUS_OK) return hull_status;
    if (n_faces < 4 || n_faces > 2 * n - 4) return GJKEPA_STATUS_BAD_INPUT;
    return GJKEPA_STATUS_OK;
}

// the 14 terms of the face (pa, pb, pc) about o, added to acc
template <typename Sqrt>
DS_HD void face_add(D3 o, D3 pa, D3 pb, D3 pc, Sqrt&& sqrt_, double* acc) {
    const D3 A = gkd::sub(pa, o), B = gkd::sub(pb, o), C = gkd::sub(pc, o);
    const D3 N = gkd::cross(gkd::sub(B, A), gkd::sub(C, B));
    const double d = gkd::dot(A, gkd::cross(B, C));
    const D3 S = gkd::mk((A.x + B.x) + C.x, (A.y + B.y) + C.y, (A.z + B.z) + C.z);
    acc[0] = acc[0] + d;
    acc[1] = acc[1] + d * S.x;
    acc[2] = acc[2] + d * S.y;
    acc[3] = acc[3] + d * S.z;
    acc[4] = acc[4] + d * (((S.x * S.x + A.x * A.x) + B.x * B.x) + C.x * C.x);
    acc[5] = acc[5] + d * (((S.y * S.y + A.y * A.y) + B.y * B.y) + C.y * C.y);
    acc[6] = acc[6] + d * (((S.z * S.z + A.z * A.z) + B.z * B.z) + C.z * C.z);
    acc[7] = acc[7] + d * (((S.x * S.y + A.x * A.y) + B.x * B.y) + C.x * C.y);
    acc[8] = acc[8] + d * (((S.x * S.z + A.x * A.z) + B.x * B.z) + C.x * C.z);
    acc[9] = acc[9] + d * (((S.y * S.z + A.y * A.z) + B.y * B.z) + C.y * C.z);
    acc[10] = acc[10] + sqrt_(gkd::dot(N, N));
    acc[11] = acc[11] + N.x;
    acc[12] = acc[12] + N.y;
    acc[13] = acc[13] + N.z;
}

DS_HD gjkepa_mass_f64 mass_blank(int status) {
    gjkepa_mass_f64 r;
    r.volume = r.area = r.radius = r.closure = 0.0;
    for (int k = 0; k < 3; ++k) r.com[k] = 0.0;
    for (int k = 0; k < 6; ++k) r.inertia[k] = 0.0;
    r.n_faces = 0;
    r.status = (int8_t)status;
    r.flags = 0;
    r.reserved[0] = r.reserved[1] = 0;
    for (int k = 0; k < 4; ++k) r.pad[k] = 0u;
    return r;
}

// everything but the radius from the totals; radius = 0, status = OK
DS_HD gjkepa_mass_f64 mass_results(const double* T, D3 o, int n_faces) {
    gjkepa_mass_f64 r = mass_blank(GJKEPA_STATUS_OK);
    const double T0 = T[0], q = 4.0 * T0;
    const double vol = T0 / 6.0;
    const D3 m = gkd::mk(T[1] / q, T[2] / q, T[3] / q);
    r.volume = vol;
    r.com[0] = o.x + m.x; r.com[1] = o.y + m.y; r.com[2] = o.z + m.z;
    const double Mxx = T[4] / 120.0 - (vol * m.x) * m.x, Myy = T[5] / 120.0 - (vol * m.y) * m.y;
    const double Mzz = T[6] / 120.0 - (vol * m.z) * m.z, Mxy = T[7] / 120.0 - (vol * m.x) * m.y;
    const double Mxz = T[8] / 120.0 - (vol * m.x) * m.z, Myz = T[9] / 120.0 - (vol * m.y) * m.z;
    r.inertia[0] = Myy + Mzz; r.inertia[1] = Mxx + Mzz; r.inertia[2] = Mxx + Myy;
    r.inertia[3] = -Mxy; r.inertia[4] = -Mxz; r.inertia[5] = -Myz;
    r.area = 0.5 * T[10];
    r.closure = gkd::swept_max_abs(gkd::mk(T[11], T[12], T[13])) / T[10];
    r.n_faces = n_faces;
    return r;
}

// rule 5, once the radius is in the record
DS_HD int mass_status(double T0, const gjkepa_mass_f64& r) {
    bool ok = finite_d(T0) && T0 > 0.0;
    ok = ok && finite_d(r.volume) && finite_d(r.area) && finite_d(r.radius) && finite_d(r.closure);
    for (int k = 0; k < 3; ++k) ok = ok && finite_d(r.com[k]);
    for (int k = 0; k < 6; ++k) ok = ok && finite_d(r.inertia[k]);
    return ok ? GJKEPA_STATUS_OK : GJKEPA_STATUS_DEGENERATE;
}

// The definition in sequence for one cloud.  TP: the storage type of the points, SoA with stride n at p;
// faces: the cloud's n_faces triples; hull_status: NULL or the hull's status.
template <typename TP, typename Sqrt>
inline gjkepa_mass_f64 mass_cloud(const TP* p, int n, const int32_t* faces, int n_faces, const int8_t* hull_status,
                                  Sqrt&& sqrt_) {
    int st = mass_precheck(n, hull_status != nullptr, hull_status ? *hull_status : 0, n_faces);
    if (st != GJKEPA_STATUS_OK) return mass_blank(st);
    auto P = [&](int i) { return gkd::mk((double)p[i], (double)p[n + i], (double)p[2 * n + i]); };
    bool good = true;
    for (int i = 0; i < n; ++i) {
        const D3 x = P(i);
        good = good && finite_d(x.x) && finite_d(x.y) && finite_d(x.z);
    }
    for (int k = 0; k < 3 * n_faces; ++k) good = good && faces[k] >= 0 && faces[k] < n;
    if (!good) return mass_blank(GJKEPA_STATUS_BAD_INPUT);
    const D3 o = P(faces[0]);
    double part[kPartials][kTerms];
    for (int l = 0; l < kPartials; ++l) {
        for (int t = 0; t < kTerms; ++t) part[l][t] = 0.0;
        for (int f = l; f < n_faces; f += kPartials)
            face_add(o, P(faces[3 * f]), P(faces[3 * f + 1]), P(faces[3 * f + 2]), sqrt_, part[l]);
    }
    for (int s = 1; s < kPartials; s *= 2) {
        double next[kPartials][kTerms];
        for (int l = 0; l < kPartials; ++l)
            for (int t = 0; t < kTerms; ++t) next[l][t] = part[l][t] + part[l ^ s][t];
        for (int l = 0; l < kPartials; ++l)
            for (int t = 0; t < kTerms; ++t) part[l][t] = next[l][t];
    }
    gjkepa_mass_f64 r = mass_results(part[0], o, n_faces);
    const D3 c = gkd::mk(r.com[0], r.com[1], r.com[2]);
    double qq = 0.0;
    for (int i = 0; i < n; ++i) {
        const double t = gkd::swept_q2(P(i), c);
        qq = t > qq ? t : qq;
    }
    r.radius = sqrt_(qq);
    st = mass_status(part[0][0], r);
    return st == GJKEPA_STATUS_OK ? r : mass_blank(st);
}

}  // namespace gkm
