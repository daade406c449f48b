// cast_advance.h — the linear cast of gjkepa_cast_batch(_device): conservative advancement over the
// distance GJK of dist_simplex.h, and the record it leaves.
//
// Hull B translates relative to hull A by t d, t in [0, 1]; the cast finds the first time the hulls
// come within tau of each other.  At every visited time the distance GJK runs on A and B + t d
// (Minkowski points a_ia - b_ib - t d).  It returns a point v of A - B(t) and the support gap
// lb = min over A - B(t) of x.n along n = v / |v|.  The gap along n shrinks at the rate s = n.d, so
// after dt = (lb - tau / 2) / s it is still tau / 2: every time in between is free of contact, and so
// is the new one.  s <= 0, or a step that reaches t = 1, proves a miss with n as the separating plane's
// normal at t = 1.  The simplex is carried from step to step by its codes (dist_gjk_from): a
// translation moves every point of it alike.
//
// Host and device code like dist_simplex.h (plain fp64, no FMA contraction): the cast kernel
// (gjkepa_kernel.hip, part 13) and tests/cast_host.cpp run this text.  Linear motion only; the cast under
// a rigid motion of both hulls (cast_advance_rigid, below) is gjkepa_cast_rigid_batch's.
#pragma once
#include "dist_simplex.h"
#include "rigid_pose.h"

namespace gkd {

constexpr int kCastMaxSteps = 32;        // advancement steps: GJKEPA_STATUS_CAST_MAXITER past them
enum { CAST_MISS = 0, CAST_IMPACT = 1, CAST_START = 2, CAST_START_OVERLAP = 3, CAST_STOPPED = 4 };
// the record's flag bits and the stopped status (include/gjkepa.h GJKEPA_CAST_*, GJKEPA_STATUS_CAST_MAXITER)
constexpr int kCastFlagImpact = 1, kCastFlagStart = 2, kCastStatusMaxIter = 6;

struct CastResult {
    int outcome;          // CAST_*
    int steps;            // advancement steps taken
    uint32_t iters;       // GJK iterations over all steps
    double toi;           // IMPACT: the time found; MISS: 1; START: 0; STOPPED: the last time certified free
    D3 n;                 // MISS: unit normal (from B to A) of the plane that still separates at t = 1
};

// sup(dir, ia, ib) as for dist_gjk; pt0(ia, ib) = a_ia - b_ib at t = 0.  On IMPACT and a separated
// START s holds the final simplex (codes and weights of the witness points at toi).
template <typename Sup, typename Pt0, typename Sqrt>
DS_HD CastResult cast_advance(Simplex& s, D3 d, double tau, Sup&& sup, Pt0&& pt0, Sqrt&& sqrt_) {
    CastResult c;
    c.outcome = CAST_STOPPED;
    c.steps = 0;
    c.iters = 0u;
    c.n = mk(0.0, 0.0, 0.0);
    double t = 0.0;
    for (;;) {
        const D3 td = mk(t * d.x, t * d.y, t * d.z);
        const Result r = dist_gjk_from(
            s, c.steps > 0, __builtin_huge_val(), sup, [&](int ia, int ib) { return sub(pt0(ia, ib), td); }, sqrt_);
        c.iters += (uint32_t)r.iters;
        // an overlap after the first step: tau is at the resolution of fp64 for this pair
        if (r.outcome == DIST_OVERLAP) { if (c.steps == 0) c.outcome = CAST_START_OVERLAP; break; }
        if (r.outcome != DIST_SEPARATED) break;
        const D3 w = closest(s);
        if (sqrt_(dot(w, w)) <= tau) { c.outcome = c.steps == 0 ? CAST_START : CAST_IMPACT; break; }
        const double vn = sqrt_(dot(r.v, r.v));
        const D3 n = mk(r.v.x / vn, r.v.y / vn, r.v.z / vn);
        const double sd = dot(n, d);
        if (!(sd > 0.0)) { c.outcome = CAST_MISS; c.n = n; break; }
        const double dt = (r.lower - 0.5 * tau) / sd;
        if (!(t + dt > t)) break;                      // no progress
        if (t + dt >= 1.0) { c.outcome = CAST_MISS; c.n = n; break; }
        t += dt;
        c.steps += 1;
        if (c.steps >= kCastMaxSteps) break;
    }
    c.toi = c.outcome == CAST_MISS ? 1.0 : t;
    return c;
}

// The 13 doubles of a gjkepa_cast_f64 (toi, point_a, point_b, normal, lambda), its codes, n_simplex,
// status and flags.  at(i), bt(i): vertex i of hull A / hull B at t = 0.  The witness points are summed
// term by term in simplex order, point_b then moved by toi d; the normal is their difference's.
template <typename At, typename Bt, typename Sqrt>
DS_HD void cast_record(const CastResult& c, const Simplex& s, D3 d, At&& at, Bt&& bt, Sqrt&& sqrt_, double* o13,
                       uint32_t* code, int& n, int& status, int& flags) {
#pragma unroll
    for (int i = 0; i < 13; ++i) o13[i] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) code[k] = kDistNoCode;
    n = 0;
    status = c.outcome == CAST_STOPPED ? kCastStatusMaxIter : 0;
    flags = c.outcome == CAST_IMPACT ? kCastFlagImpact
          : (c.outcome == CAST_START || c.outcome == CAST_START_OVERLAP) ? kCastFlagStart : 0;
    o13[0] = c.toi;
    if (c.outcome == CAST_MISS) { o13[7] = c.n.x; o13[8] = c.n.y; o13[9] = c.n.z; }
    if (c.outcome != CAST_IMPACT && c.outcome != CAST_START) return;
    D3 pa = mk(0.0, 0.0, 0.0), pb = mk(0.0, 0.0, 0.0);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < s.n) {
            const D3 ak = at((int)(s.code[k] & 0xffffu)), bk = bt((int)(s.code[k] >> 16));
            pa = mk(pa.x + s.lam[k] * ak.x, pa.y + s.lam[k] * ak.y, pa.z + s.lam[k] * ak.z);
            pb = mk(pb.x + s.lam[k] * bk.x, pb.y + s.lam[k] * bk.y, pb.z + s.lam[k] * bk.z);
            o13[10 + k] = s.lam[k];
            code[k] = s.code[k];
        }
    n = s.n;
    pb = mk(pb.x + c.toi * d.x, pb.y + c.toi * d.y, pb.z + c.toi * d.z);
    const D3 e = sub(pa, pb);
    const double len = sqrt_(dot(e, e));
    o13[1] = pa.x; o13[2] = pa.y; o13[3] = pa.z;
    o13[4] = pb.x; o13[5] = pb.y; o13[6] = pb.z;
    if (len > 0.0) { o13[7] = e.x / len; o13[8] = e.y / len; o13[9] = e.z / len; }
}

// ---- the cast under a rigid motion of both hulls (gjkepa_cast_rigid_batch, rigid_pose.h) ---------------
// Hull A moves by ma and hull B by mb, each about its own pivot.  At every visited time the distance GJK
// runs on the posed hulls A(t), B(t); the simplex is carried by its codes, and since the points of a
// carried simplex move apart under rotation it is only a valid start: dist_gjk_from reduces it from
// scratch.  Along the fixed unit normal n (from B to A) a vertex x of body X moves at
// n.v_X + theta'(t) (x(t) - c_X(t)).(n x k_X), k_X = w_X / |w_X|, and theta' <= |w_X|, so with
// rho_X = max_i |x_i - c_X| the support gap lb along n shrinks at most at the rate
//     s = n.(v_B - v_A) + |n x w_A| rho_A + |n x w_B| rho_B
// (a spin about n costs nothing).  After dt = (lb - tau / 2) / s the gap is still tau / 2.  s <= 0, or a
// step that reaches t = 1, proves a miss with n the normal of a plane that separates the posed hulls at
// t = 1.  Convergence under spin is linear, so the step cap is flat.
constexpr int kCastRigidMaxSteps = 64;

// sup(dir, ia, ib): first-maximum supports of the posed hulls along dir / -dir, as indices of the unposed
// vertices; pt(ia, ib) = a_ia(t) - b_ib(t) at the time on_t was last called with; on_t(t): t has changed
// (called with 0 before the first distance run).  On IMPACT and a separated START s holds the final
// simplex, and the last time given to on_t is toi.
template <typename Sup, typename Pt, typename OnT, typename Sqrt>
DS_HD CastResult cast_advance_rigid(Simplex& s, const Motion& ma, const Motion& mb, double rho_a, double rho_b, double tau,
                                    Sup&& sup, Pt&& pt, OnT&& on_t, Sqrt&& sqrt_) {
    CastResult c;
    c.outcome = CAST_STOPPED;
    c.steps = 0;
    c.iters = 0u;
    c.n = mk(0.0, 0.0, 0.0);
    double t = 0.0;
    on_t(t);
    for (;;) {
        const Result r = dist_gjk_from(s, c.steps > 0, __builtin_huge_val(), sup, pt, sqrt_);
        c.iters += (uint32_t)r.iters;
        if (r.outcome == DIST_OVERLAP) { if (c.steps == 0) c.outcome = CAST_START_OVERLAP; break; }
        if (r.outcome != DIST_SEPARATED) break;
        const D3 w = closest(s);
        if (sqrt_(dot(w, w)) <= tau) { c.outcome = c.steps == 0 ? CAST_START : CAST_IMPACT; break; }
        const double vn = sqrt_(dot(r.v, r.v));
        const D3 n = mk(r.v.x / vn, r.v.y / vn, r.v.z / vn);
        const D3 xa = cross(n, ma.w), xb = cross(n, mb.w);
        const double sd = dot(n, sub(mb.v, ma.v)) + sqrt_(dot(xa, xa)) * rho_a + sqrt_(dot(xb, xb)) * rho_b;
        if (!(sd > 0.0)) { c.outcome = CAST_MISS; c.n = n; break; }
        const double dt = (r.lower - 0.5 * tau) / sd;
        if (!(t + dt > t)) break;                      // no progress
        if (t + dt >= 1.0) { c.outcome = CAST_MISS; c.n = n; break; }
        t += dt;
        on_t(t);
        c.steps += 1;
        if (c.steps >= kCastRigidMaxSteps) break;
    }
    c.toi = c.outcome == CAST_MISS ? 1.0 : t;
    return c;
}

// cast_record for the rigid cast.  at(i), bt(i): vertex i of hull A / hull B posed at toi; both witness
// points are sums of posed vertices, so nothing is moved afterwards.
template <typename At, typename Bt, typename Sqrt>
DS_HD void cast_record_rigid(const CastResult& c, const Simplex& s, At&& at, Bt&& bt, Sqrt&& sqrt_, double* o13,
                             uint32_t* code, int& n, int& status, int& flags) {
    cast_record(c, s, mk(0.0, 0.0, 0.0), at, bt, sqrt_, o13, code, n, status, flags);
}

}  // namespace gkd
