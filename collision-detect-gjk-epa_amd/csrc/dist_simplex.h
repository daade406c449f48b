// dist_simplex.h — the distance GJK of gjkepa_distance_batch(_device): the closest point of a simplex
// of up to four Minkowski points to the origin, and the iteration around it.
//
// Host and device code (plain fp64, no FMA contraction in either build), so the same text runs in
// the distance kernel (gjkepa_kernel.hip, part 12: one group of lanes per pair, every lane of the
// group holding the same values) and in a host program over a naive support scan
// (tests/distance_host.cpp), where it is checked against brute force without a GPU.
//
// Unlike the contact path's gjk_phase (the reference's containment test, bit for bit), this is a
// textbook GJK: it has no counterpart in the reference, which leaves nearest_points_ at 0 for a miss.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DS_HD inline __attribute__((always_inline))
#endif

namespace gkd {

struct D3 { double x, y, z; };
DS_HD D3 mk(double x, double y, double z) { D3 r; r.x = x; r.y = y; r.z = z; return r; }
DS_HD D3 sub(D3 a, D3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DS_HD D3 neg(D3 a) { return mk(-a.x, -a.y, -a.z); }
DS_HD double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DS_HD D3 cross(D3 a, D3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

constexpr int kDistMaxIter = 64;         // iteration cap: GJKEPA_STATUS_DIST_MAXITER past it
constexpr double kDistEps = 1.0e-10;     // relative gap (v.v - v.w) / v.v at which the distance is final
// v.v at or below this fraction of the largest |simplex point|^2 is a distance of zero: 1e-12 of the
// simplex's scale, four orders above the rounding of v itself (a sum of three products)
constexpr double kDistZero2 = 1.0e-24;
// a tetrahedron whose fourth point is within this fraction (squared) of the scale of a face's plane is
// flat: it encloses nothing, and its faces and edges give the closest point
constexpr double kDistFlat2 = 1.0e-20;

constexpr uint32_t kDistNoCode = 0xFFFFFFFFu;
enum { DIST_SEPARATED = 0, DIST_OVERLAP = 1, DIST_FAR = 2, DIST_MAXITER = 3 };

// The simplex: up to four support points y_k = a[ia_k] - b[ib_k], their codes ia | ib << 16 and their
// barycentric weights for v, the simplex's point closest to the origin.
struct Simplex {
    D3 y[4];
    double lam[4];
    uint32_t code[4];
    int n;
};

struct Best {
    double vv;
    double lam[4];
};

// a candidate point sum lam_k y_k of the simplex: taken when strictly closer than the best so far
DS_HD void offer(const Simplex& s, Best& b, double l0, double l1, double l2, double l3) {
    const double l[4] = {l0, l1, l2, l3};
    D3 p = mk(0.0, 0.0, 0.0);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (l[k] != 0.0) { p.x += l[k] * s.y[k].x; p.y += l[k] * s.y[k].y; p.z += l[k] * s.y[k].z; }
    const double vv = dot(p, p);
    if (vv < b.vv) {
        b.vv = vv;
#pragma unroll
        for (int k = 0; k < 4; ++k) b.lam[k] = l[k];
    }
}

// closest point of segment (i, j), clamped to its ends
template <int I, int J> DS_HD void offer_edge(const Simplex& s, Best& b) {
    const D3 ab = sub(s.y[J], s.y[I]);
    const double bb = dot(ab, ab);
    double t = bb > 0.0 ? -dot(s.y[I], ab) / bb : 0.0;
    t = t > 0.0 ? (t < 1.0 ? t : 1.0) : 0.0;         // a NaN gives 0
    double l[4] = {0.0, 0.0, 0.0, 0.0};
    l[I] = 1.0 - t;
    l[J] = t;
    offer(s, b, l[0], l[1], l[2], l[3]);
}

// the origin's projection onto the plane of triangle (i, j, k), when it falls inside the triangle: the
// 2 x 2 Gram system over the edge vectors, so only differences of the points enter
template <int I, int J, int K> DS_HD void offer_face(const Simplex& s, Best& b) {
    const D3 ab = sub(s.y[J], s.y[I]), ac = sub(s.y[K], s.y[I]);
    const double bb = dot(ab, ab), cc = dot(ac, ac), bc = dot(ab, ac);
    const double d1 = -dot(s.y[I], ab), d2 = -dot(s.y[I], ac);
    const double det = bb * cc - bc * bc;
    if (!(det > 1.0e-24 * bb * cc)) return;          // no area: the edges answer
    const double v = (d1 * cc - d2 * bc) / det, w = (d2 * bb - d1 * bc) / det;
    const double u = (1.0 - v) - w;
    if (!(u >= 0.0 && v >= 0.0 && w >= 0.0)) return;
    double l[4] = {0.0, 0.0, 0.0, 0.0};
    l[I] = u;
    l[J] = v;
    l[K] = w;
    offer(s, b, l[0], l[1], l[2], l[3]);
}

// face (i, j, k) of the tetrahedron with the fourth point l: is the origin strictly on l's side, and is
// l off the face's plane at all
template <int I, int J, int K, int L> DS_HD void face_side(const Simplex& s, double scale2, bool& inside, bool& flat) {
    const D3 n = cross(sub(s.y[J], s.y[I]), sub(s.y[K], s.y[I]));
    const double so = -dot(n, s.y[I]), sl = dot(n, sub(s.y[L], s.y[I]));
    if (!(sl * sl > kDistFlat2 * dot(n, n) * scale2)) flat = true;
    if (!(so * sl > 0.0)) inside = false;
}

// The point of the simplex closest to the origin: the nearest of every edge's and every face's closest
// point (each a point of the simplex, so the smallest is the answer whatever the rounding of the others),
// starting from the previous closest point (weights lam[0 .. n-2], new point weight 0) so v never grows.
// Returns true when the simplex is a tetrahedron that holds the origin.  On return the points with a
// zero weight are dropped and s.n <= 3.
DS_HD bool reduce(Simplex& s, double scale2, double& vv) {
    Best b;
    b.vv = 1.0e300;
    if (s.n == 1) {
        offer(s, b, 1.0, 0.0, 0.0, 0.0);
    } else if (s.n == 2) {
        offer(s, b, s.lam[0], 0.0, 0.0, 0.0);
        offer_edge<0, 1>(s, b);
    } else if (s.n == 3) {
        offer(s, b, s.lam[0], s.lam[1], 0.0, 0.0);
        offer_edge<0, 2>(s, b);
        offer_edge<1, 2>(s, b);
        offer_edge<0, 1>(s, b);
        offer_face<0, 1, 2>(s, b);
    } else {
        bool inside = true, flat = false;
        face_side<0, 1, 2, 3>(s, scale2, inside, flat);
        face_side<0, 1, 3, 2>(s, scale2, inside, flat);
        face_side<0, 2, 3, 1>(s, scale2, inside, flat);
        face_side<1, 2, 3, 0>(s, scale2, inside, flat);
        if (inside && !flat) return true;
        offer(s, b, s.lam[0], s.lam[1], s.lam[2], 0.0);
        offer_edge<0, 3>(s, b);
        offer_edge<1, 3>(s, b);
        offer_edge<2, 3>(s, b);
        offer_edge<0, 1>(s, b);
        offer_edge<0, 2>(s, b);
        offer_edge<1, 2>(s, b);
        offer_face<0, 1, 3>(s, b);
        offer_face<0, 2, 3>(s, b);
        offer_face<1, 2, 3>(s, b);
        offer_face<0, 1, 2>(s, b);
    }
    vv = b.vv;
    // keep the points with a weight, in order (static indices only: the simplex stays in registers)
    Simplex o;
    int m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { o.y[j] = mk(0.0, 0.0, 0.0); o.lam[j] = 0.0; o.code[j] = kDistNoCode; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool keep = k < s.n && b.lam[k] > 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (keep && m == j) { o.y[j] = s.y[k]; o.lam[j] = b.lam[k]; o.code[j] = s.code[k]; }
        m += keep ? 1 : 0;
    }
    o.n = m;
    s = o;
    return false;
}

DS_HD D3 closest(const Simplex& s) {
    D3 p = mk(0.0, 0.0, 0.0);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < s.n) { p.x += s.lam[k] * s.y[k].x; p.y += s.lam[k] * s.y[k].y; p.z += s.lam[k] * s.y[k].z; }
    return p;
}

struct Result {
    int outcome;          // DIST_*
    int iters;
    double lower;         // the last iteration's lower bound v.w / |v| (0 if it had none)
    D3 v;                 // closest point of the final simplex: the separation vector a - b
};

// The iteration.  sup(d, ia, ib): first-maximum supports argmax_i d.a_i, argmax_j (-d).b_j;
// pt(ia, ib) = a_ia - b_ib.  Every iteration: w = support along -v; the lower bound v.w / |v| (FAR as
// soon as it exceeds max_distance, before any other test, so FAR is exactly `the final lower bound is
// above max_distance`); stop when the gap v.v - v.w closes to kDistEps v.v or w is already a simplex
// point; else add w and reduce, and stop as well when that brings v no closer (the gap is then below
// what fp64 resolves for this pair).  sqrt_(x): the caller's square root.
template <typename Sup, typename Pt, typename Sqrt>
DS_HD Result dist_gjk(Simplex& s, double max_distance, Sup&& sup, Pt&& pt, Sqrt&& sqrt_) {
    Result r;
    r.outcome = DIST_MAXITER;
    r.iters = 0;
    r.lower = 0.0;
    s.n = 1;
    s.y[0] = pt(0, 0);
    s.code[0] = 0u;
    s.lam[0] = 1.0;
#pragma unroll
    for (int k = 1; k < 4; ++k) { s.y[k] = mk(0.0, 0.0, 0.0); s.lam[k] = 0.0; s.code[k] = kDistNoCode; }
    D3 v = s.y[0];
    double vv = dot(v, v);
    double scale2 = vv;
    for (int it = 1; it <= kDistMaxIter; ++it) {
        if (!(vv > kDistZero2 * scale2)) { r.outcome = DIST_OVERLAP; break; }
        r.iters = it;
        int ia, ib;
        sup(neg(v), ia, ib);
        const D3 w = pt(ia, ib);
        const double vw = dot(v, w);
        r.lower = vw > 0.0 ? vw / sqrt_(vv) : 0.0;
        if (r.lower > max_distance) { r.outcome = DIST_FAR; break; }
        if (vv - vw <= kDistEps * vv) { r.outcome = DIST_SEPARATED; break; }
        const uint32_t code = (uint32_t)ia | ((uint32_t)ib << 16);
        bool seen = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) seen = seen || (k < s.n && s.code[k] == code);
        if (seen) { r.outcome = DIST_SEPARATED; break; }
        // s.n <= 3 here; static slots only
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (s.n == k) { s.y[k] = w; s.code[k] = code; s.lam[k] = 0.0; }
        s.n += 1;
        const double ww = dot(w, w);
        scale2 = ww > scale2 ? ww : scale2;
        double bvv;
        if (reduce(s, scale2, bvv)) { r.outcome = DIST_OVERLAP; break; }
        v = closest(s);
        const double nvv = dot(v, v);
        // no candidate beat the previous closest point: rounding has closed the gap as far as it goes
        if (!(nvv < vv)) { r.outcome = DIST_SEPARATED; break; }
        vv = nvv;
    }
    r.v = v;
    return r;
}

// dist_gjk with a resume entry, for a caller that runs the iteration again after every Minkowski point
// has moved by the same vector (cast_advance.h).  carried = false: dist_gjk's start, pt(0, 0).
// carried = true: s holds n <= 3 codes of an earlier run; the points are rebuilt from the codes with
// pt, the simplex is reduced once from scratch (its closest point has moved with the points; vertex 0
// is reduce's starting candidate, so every feature is offered), and the iteration goes on from there.
// Same tests and exits as dist_gjk, with two differences in what comes back: iters counts the support
// evaluations of this run only, and after the exit `reduce brought v no closer` v is the point the
// last support was taken along, so that lower = min over A - B of x.v / |v| holds for the v returned
// (the simplex and its weights are the reduced ones, as in dist_gjk).
template <typename Sup, typename Pt, typename Sqrt>
DS_HD Result dist_gjk_from(Simplex& s, bool carried, double max_distance, Sup&& sup, Pt&& pt, Sqrt&& sqrt_) {
    Result r;
    r.outcome = DIST_MAXITER;
    r.iters = 0;
    r.lower = 0.0;
    if (!carried) {
        s.n = 1;
        s.code[0] = 0u;
#pragma unroll
        for (int k = 1; k < 4; ++k) s.code[k] = kDistNoCode;
    }
    double scale2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s.y[k] = mk(0.0, 0.0, 0.0);
        s.lam[k] = k == 0 ? 1.0 : 0.0;
        if (k < 3 && k < s.n) {
            s.y[k] = pt((int)(s.code[k] & 0xffffu), (int)(s.code[k] >> 16));
            const double ww = dot(s.y[k], s.y[k]);
            scale2 = ww > scale2 ? ww : scale2;
        }
    }
    bool fresh = s.n > 1;                   // a carried simplex: reduce before the first support
    D3 v = s.y[0];
    double vv = fresh ? 1.0e300 : dot(v, v);
    for (;;) {
        if (!fresh) {
            if (!(vv > kDistZero2 * scale2)) { r.outcome = DIST_OVERLAP; break; }
            if (r.iters >= kDistMaxIter) break;
            r.iters += 1;
            int ia, ib;
            sup(neg(v), ia, ib);
            const D3 w = pt(ia, ib);
            const double vw = dot(v, w);
            r.lower = vw > 0.0 ? vw / sqrt_(vv) : 0.0;
            if (r.lower > max_distance) { r.outcome = DIST_FAR; break; }
            if (vv - vw <= kDistEps * vv) { r.outcome = DIST_SEPARATED; break; }
            const uint32_t code = (uint32_t)ia | ((uint32_t)ib << 16);
            bool seen = false;
#pragma unroll
            for (int k = 0; k < 3; ++k) seen = seen || (k < s.n && s.code[k] == code);
            if (seen) { r.outcome = DIST_SEPARATED; break; }
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (s.n == k) { s.y[k] = w; s.code[k] = code; s.lam[k] = 0.0; }
            s.n += 1;
            const double ww = dot(w, w);
            scale2 = ww > scale2 ? ww : scale2;
        }
        fresh = false;
        double bvv;
        if (reduce(s, scale2, bvv)) { r.outcome = DIST_OVERLAP; break; }
        const D3 nv = closest(s);
        const double nvv = dot(nv, nv);
        if (!(nvv < vv)) { r.outcome = DIST_SEPARATED; break; }
        v = nv;
        vv = nvv;
    }
    r.v = v;
    return r;
}

}  // namespace gkd
