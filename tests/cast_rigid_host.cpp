// cast_rigid_host.cpp — the rigid-motion cast of csrc/cast_advance.h (cast_advance_rigid over the pose of
// csrc/rigid_pose.h) on the host, over a plain first-maximum support scan: the same advancement, pose and
// simplex arithmetic the rigid cast kernel runs, so tests/test_cast_rigid_host.py can check it without a
// GPU.  pose_host_batch is the pose kernel's arithmetic the same way.  Built by that test
// (g++ -ffp-contract=off); -DCAST_RIGID_HOST_MAIN adds a main for a stand-alone run under sanitizers.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../collision-detect-gjk-epa_amd/csrc/cast_advance.h"
#include "../include/gjkepa.h"

namespace {

static_assert(gkd::kCastFlagImpact == GJKEPA_CAST_IMPACT && gkd::kCastFlagStart == GJKEPA_CAST_START &&
              gkd::kCastStatusMaxIter == GJKEPA_STATUS_CAST_MAXITER && gkd::kMotionDoubles == GJKEPA_MOTION_DOUBLES,
              "cast_advance.h and rigid_pose.h against gjkepa.h");

template <typename TIn> struct Hull {
    const TIn* p;
    int n;
    gkd::D3 at(int i) const { return gkd::mk((double)p[i], (double)p[n + i], (double)p[2 * n + i]); }
    bool finite() const {
        for (int i = 0; i < 3 * n; ++i)
            if (!std::isfinite((double)p[i])) return false;
        return true;
    }
    // the farthest vertex from the pivot: the largest |p - c|^2, then one square root
    double rho(gkd::D3 c) const {
        double m = 0.0;
        for (int i = 0; i < n; ++i) {
            const gkd::D3 q = gkd::sub(at(i), c);
            const double qq = gkd::dot(q, q);
            m = qq > m ? qq : m;
        }
        return std::sqrt(m);
    }
};

template <typename TIn>
void one_pair(const Hull<TIn>& A, const Hull<TIn>& B, const double* ma_, const double* mb_, double tau, gjkepa_cast_f64* o) {
    std::memset(o, 0, sizeof(*o));
    for (int k = 0; k < 3; ++k) o->code[k] = gkd::kDistNoCode;
    if (A.n < 1 || B.n < 1 || A.n > GJKEPA_MAX_HULL_VERTS || B.n > GJKEPA_MAX_HULL_VERTS || !A.finite() || !B.finite() ||
        !gkd::motion_finite(ma_) || !gkd::motion_finite(mb_)) {
        o->status = GJKEPA_STATUS_BAD_INPUT;
        return;
    }
    const gkd::Motion ma = gkd::motion_of(ma_), mb = gkd::motion_of(mb_);
    auto sqrt_ = [](double x) { return std::sqrt(x); };
    gkd::PoseState sa, sb;
    gkd::Simplex s;
    const gkd::CastResult r = gkd::cast_advance_rigid(
        s, ma, mb, A.rho(ma.c), B.rho(mb.c), tau,
        [&](gkd::D3 dir, int& ia, int& ib) {
            const gkd::D3 da = gkd::pose_dir(sa, dir), db = gkd::pose_dir(sb, dir);
            double va = -1.7976931348623157e308, vb = va;
            ia = ib = 0;
            for (int i = 0; i < A.n; ++i) {
                const gkd::D3 a = A.at(i);
                const double t = da.x * a.x + da.y * a.y + da.z * a.z;
                if (t > va) { va = t; ia = i; }
            }
            for (int j = 0; j < B.n; ++j) {
                const gkd::D3 b = B.at(j);
                const double t = -(db.x * b.x + db.y * b.y + db.z * b.z);
                if (t > vb) { vb = t; ib = j; }
            }
        },
        [&](int ia, int ib) { return gkd::sub(gkd::pose_point(sa, ma.c, A.at(ia)), gkd::pose_point(sb, mb.c, B.at(ib))); },
        [&](double t) {
            sa = gkd::pose_state(ma.v, ma.w, t);
            sb = gkd::pose_state(mb.v, mb.w, t);
        },
        sqrt_);
    double o13[13];
    int n, status, flags;
    gkd::cast_record_rigid(
        r, s, [&](int i) { return gkd::pose_point(sa, ma.c, A.at(i)); }, [&](int i) { return gkd::pose_point(sb, mb.c, B.at(i)); },
        sqrt_, o13, o->code, n, status, flags);
    o->toi = o13[0];
    for (int i = 0; i < 3; ++i) {
        o->point_a[i] = o13[1 + i];
        o->point_b[i] = o13[4 + i];
        o->normal[i] = o13[7 + i];
        o->lambda[i] = o13[10 + i];
    }
    o->n_simplex = (int8_t)n;
    o->status = (int8_t)status;
    o->flags = (int8_t)flags;
    o->iters = r.iters;
    o->steps = (uint32_t)r.steps;
}

template <typename TIn, typename TOut>
void pose_pool(const TIn* in, const int64_t* off, const int32_t* cnt, int64_t n_hulls, const double* motion, const double* time,
               TOut* out, int8_t* status) {
    for (int64_t h = 0; h < n_hulls; ++h) {
        const int n = cnt[h];
        const double t = time ? time[h] : 1.0;
        bool ok = n >= 1 && n <= GJKEPA_MAX_HULL_VERTS && gkd::motion_finite(motion + 9 * h) && std::isfinite(t);
        if (ok) ok = Hull<TIn>{in + off[h], n}.finite();
        if (status) status[h] = ok ? GJKEPA_STATUS_OK : GJKEPA_STATUS_BAD_INPUT;
        if (!ok) continue;
        const Hull<TIn> H{in + off[h], n};
        const gkd::Motion m = gkd::motion_of(motion + 9 * h);
        const gkd::PoseState s = gkd::pose_state(m.v, m.w, t);
        TOut* o = out + off[h];
        for (int i = 0; i < n; ++i) {
            const gkd::D3 p = gkd::pose_point(s, m.c, H.at(i));
            o[i] = (TOut)p.x;
            o[n + i] = (TOut)p.y;
            o[2 * n + i] = (TOut)p.z;
        }
    }
}

}  // namespace

extern "C" int cast_rigid_host_batch(int vert_dtype, const void* verts, const int64_t* hull_off, const int32_t* hull_cnt,
                                     const int32_t* pairs, int64_t n_pairs, const double* body_motion, double tolerance,
                                     void* out) {
    static_assert(sizeof(gjkepa_cast_f64) == 128, "record layout");
    gjkepa_cast_f64* o = (gjkepa_cast_f64*)out;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t ha = pairs[2 * p], hb = pairs[2 * p + 1];
        const double *ma = body_motion + 9 * (int64_t)ha, *mb = body_motion + 9 * (int64_t)hb;
        if (vert_dtype == GJKEPA_DTYPE_F32) {
            const float* v = (const float*)verts;
            one_pair(Hull<float>{v + hull_off[ha], hull_cnt[ha]}, Hull<float>{v + hull_off[hb], hull_cnt[hb]}, ma, mb, tolerance,
                     o + p);
        } else {
            const double* v = (const double*)verts;
            one_pair(Hull<double>{v + hull_off[ha], hull_cnt[ha]}, Hull<double>{v + hull_off[hb], hull_cnt[hb]}, ma, mb,
                     tolerance, o + p);
        }
    }
    return 0;
}

// verts_out: the input pool's offsets, out_dtype scalars; in place when the dtypes are equal
extern "C" int pose_host_batch(int in_dtype, const void* verts_in, const int64_t* hull_off, const int32_t* hull_cnt,
                               int64_t n_hulls, const double* body_motion, const double* time, int out_dtype, void* verts_out,
                               int8_t* status) {
    if (in_dtype == GJKEPA_DTYPE_F32 && out_dtype == GJKEPA_DTYPE_F32)
        pose_pool((const float*)verts_in, hull_off, hull_cnt, n_hulls, body_motion, time, (float*)verts_out, status);
    else if (in_dtype == GJKEPA_DTYPE_F32)
        pose_pool((const float*)verts_in, hull_off, hull_cnt, n_hulls, body_motion, time, (double*)verts_out, status);
    else if (out_dtype == GJKEPA_DTYPE_F32)
        pose_pool((const double*)verts_in, hull_off, hull_cnt, n_hulls, body_motion, time, (float*)verts_out, status);
    else
        pose_pool((const double*)verts_in, hull_off, hull_cnt, n_hulls, body_motion, time, (double*)verts_out, status);
    return 0;
}

#ifdef CAST_RIGID_HOST_MAIN
// Two seeded pools (small hulls in fp32, large hulls in fp64, spinning towards each other) through the
// cast and the pose, for a stand-alone run under -fsanitize=address,undefined.  Prints the outcome counts.
#include <cstdio>
#include <vector>
namespace {
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double uni() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}
template <typename T> int run_pool(int dtype, int n_pairs, int lo, int hi) {
    std::vector<T> verts;
    std::vector<int64_t> off;
    std::vector<int32_t> cnt, pairs;
    std::vector<double> motion;
    for (int h = 0; h < 2 * n_pairs; ++h) {
        const int n = lo + (int)(uni() * (hi - lo + 1));
        const double cx = (h & 1) ? 3.0 : 0.0;
        off.push_back((int64_t)verts.size());
        cnt.push_back(n);
        std::vector<double> x(3 * n);
        for (int i = 0; i < n; ++i) {
            double p[3] = {uni() - 0.5, uni() - 0.5, uni() - 0.5};
            const double len = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + 1e-3;
            for (int a = 0; a < 3; ++a) x[a * n + i] = p[a] / len + (a == 0 ? cx : 0.0);
        }
        for (double v : x) verts.push_back((T)v);
        const double m[9] = {(h & 1) ? -4.0 * uni() : 0.0, uni() - 0.5, uni() - 0.5, uni() - 0.5, uni() - 0.5, uni() - 0.5, cx, 0.0, 0.0};
        motion.insert(motion.end(), m, m + 9);
        pairs.push_back(h);
    }
    std::vector<gjkepa_cast_f64> rec(n_pairs);
    cast_rigid_host_batch(dtype, verts.data(), off.data(), cnt.data(), pairs.data(), n_pairs, motion.data(), 1e-6, rec.data());
    std::vector<double> posed(verts.size());
    std::vector<int8_t> status(2 * n_pairs);
    pose_host_batch(dtype, verts.data(), off.data(), cnt.data(), 2 * n_pairs, motion.data(), nullptr, GJKEPA_DTYPE_F64, posed.data(),
                    status.data());
    int impact = 0, miss = 0, start = 0, stopped = 0;
    for (const auto& r : rec) {
        if (r.status == GJKEPA_STATUS_CAST_MAXITER) ++stopped;
        else if (r.flags == GJKEPA_CAST_IMPACT) ++impact;
        else if (r.flags == GJKEPA_CAST_START) ++start;
        else ++miss;
    }
    std::printf("%d pairs of %d-%d: %d impacts, %d misses, %d starts, %d undecided\n", n_pairs, lo, hi, impact, miss, start, stopped);
    return impact > 0 ? 0 : 1;
}
}  // namespace
int main() { return run_pool<float>(GJKEPA_DTYPE_F32, 200, 8, 32) | run_pool<double>(GJKEPA_DTYPE_F64, 60, 33, 256); }
#endif
