// rigid_pose.h — the rigid motion of gjkepa_cast_rigid_batch(_device) and gjkepa_pose_pool(_device): where a
// vertex of a moving body is at time t of the step, and a direction turned back into the body's frame.
//
// A body's motion is 9 doubles (include/gjkepa.h GJKEPA_MOTION_DOUBLES): v, the displacement of its pivot
// over the step; w, its rotation vector (angular velocity times the step); c, the pivot at t = 0.  At
// t in [0, 1] the vertex p is at
//     h = (0.5 t) w;  q = p - c;  u = h x q;  g = u + h x u;  f = 2 / (1 + h.h)
//     p(t) = (p + t v) + f g
// the rotation of the unnormalised quaternion (1, h) about the pivot: one division, no sin or cos, so the
// host and the device produce the same bytes.  t = 0 gives p and w = 0 gives p + t v, both exactly.  The
// axis is w / |w| for every t and the angle 2 atan(t |w| / 2), whose rate |w| / (1 + t^2 |w|^2 / 4) never
// exceeds |w|: cast_advance_rigid's bound rests on that.
//
// Host and device code like dist_simplex.h (plain fp64, no FMA contraction): the rigid cast kernel
// (gjkepa_kernel.hip, part 15), the pose kernel (pose_kernel.hip), gjkepa_capi.cpp and
// tests/cast_rigid_host.cpp run this text.
#pragma once
#include "dist_simplex.h"

namespace gkd {

constexpr int kMotionDoubles = 9;

struct Motion { D3 v, w, c; };
DS_HD Motion motion_of(const double* m) {
    Motion r;
    r.v = mk(m[0], m[1], m[2]);
    r.w = mk(m[3], m[4], m[5]);
    r.c = mk(m[6], m[7], m[8]);
    return r;
}

// what a body's pose at one time shares between its vertices
struct PoseState {
    D3 h;                 // (0.5 t) w
    double f;             // 2 / (1 + h.h)
    D3 tv;                // t v
};
DS_HD PoseState pose_state(D3 v, D3 w, double t) {
    PoseState s;
    const double ht = 0.5 * t;
    s.h = mk(ht * w.x, ht * w.y, ht * w.z);
    s.f = 2.0 / (1.0 + dot(s.h, s.h));
    s.tv = mk(t * v.x, t * v.y, t * v.z);
    return s;
}

// p(t): vertex p of the body with pivot c in the pose s
DS_HD D3 pose_point(const PoseState& s, D3 c, D3 p) {
    const D3 u = cross(s.h, sub(p, c));
    const D3 hu = cross(s.h, u);
    const D3 g = mk(u.x + hu.x, u.y + hu.y, u.z + hu.z);
    return mk((p.x + s.tv.x) + s.f * g.x, (p.y + s.tv.y) + s.f * g.y, (p.z + s.tv.z) + s.f * g.z);
}

// R(t)^T dir: the world direction dir in the body's frame (the rotation of (1, -h)), so that the support
// of the posed body along dir is the unposed vertices' along this
DS_HD D3 pose_dir(const PoseState& s, D3 dir) {
    const D3 mh = neg(s.h);
    const D3 u = cross(mh, dir);
    const D3 hu = cross(mh, u);
    const D3 g = mk(u.x + hu.x, u.y + hu.y, u.z + hu.z);
    return mk(dir.x + s.f * g.x, dir.y + s.f * g.y, dir.z + s.f * g.z);
}

DS_HD bool motion_finite(const double* m) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kMotionDoubles; ++i) ok = ok && (m[i] - m[i] == 0.0);      // false for NaN and +-inf
    return ok;
}

}  // namespace gkd
