// swept_sphere.h — the pair test of gjkepa_broadphase_swept(_device): can the bounding balls of two bodies
// in rigid motion (rigid_pose.h) come within the cast's tolerance of each other during the step.
//
// A body is seen through its pivot c, the pivot's displacement v and rho = max_i |x_i - c|, the rigid
// cast's pivot_radius (an order-free maximum of q.q, then one square root).  Under the path of rigid_pose.h
// the pivot moves on c + t v and every vertex stays within rho of it (the path is a rotation about the
// pivot), so the rotation vector w does not enter.  The pair (a < b) passes when
//     d = c_a - c_b;  e = v_a - v_b;  ee = e.e;  de = d.e
//     s = 0 if ee == 0 or de >= 0;  1 if -de >= ee;  (-de) / ee otherwise
//     m = d + s e;  dist = sqrt(m.m)
//     reach = (rho_a + rho_b) + tolerance
//     lim = reach + 1e-9 ((reach + max|d_k|) + max|e_k|)
//     dist <= lim
// dist is the closest approach of the two ball centres over t in [0, 1]; the 1e-9 term covers the rounding
// of d, e, s and of the cast's posed vertices, so the list is a superset of what the casts
// can report.
//
// Host and device code like rigid_pose.h (plain fp64, no FMA contraction, the operation order written
// here): sweep_kernel.hip runs this text, and tests/sweep_ref.py restates it in numpy with the same bits.
#pragma once
#include "rigid_pose.h"

namespace gkd {

constexpr double kSweptSlack = 1.0e-9;

// q.q of a vertex about the pivot: rho = sqrt of the largest
DS_HD double swept_q2(D3 x, D3 c) {
    const D3 q = sub(x, c);
    return dot(q, q);
}

DS_HD double swept_max_abs(D3 a) {
    const double x = a.x < 0.0 ? -a.x : a.x, y = a.y < 0.0 ? -a.y : a.y, z = a.z < 0.0 ? -a.z : a.z;
    const double m = x > y ? x : y;
    return m > z ? m : z;
}

// the pair test above, a the lower hull index; any NaN on the way fails the pair
template <typename Sqrt>
DS_HD bool swept_pair(D3 ca, D3 va, double rho_a, D3 cb, D3 vb, double rho_b, double tolerance, Sqrt&& sqrt_) {
    const D3 d = sub(ca, cb), e = sub(va, vb);
    const double ee = dot(e, e), de = dot(d, e);
    double s;
    if (ee == 0.0 || de >= 0.0) s = 0.0;
    else if (-de >= ee) s = 1.0;
    else s = (-de) / ee;
    const D3 m = mk(d.x + s * e.x, d.y + s * e.y, d.z + s * e.z);
    const double dist = sqrt_(dot(m, m));
    const double reach = (rho_a + rho_b) + tolerance;
    const double lim = reach + kSweptSlack * ((reach + swept_max_abs(d)) + swept_max_abs(e));
    return dist <= lim;
}

// the ball enclosing the swept ball, for the grid only: centre g = c + 0.5 v, radius R = rho + 0.5 |v|
DS_HD D3 swept_centre(D3 c, D3 v) { return mk(c.x + 0.5 * v.x, c.y + 0.5 * v.y, c.z + 0.5 * v.z); }
template <typename Sqrt>
DS_HD double swept_radius(double rho, D3 v, Sqrt&& sqrt_) { return rho + 0.5 * sqrt_(dot(v, v)); }

}  // namespace gkd
