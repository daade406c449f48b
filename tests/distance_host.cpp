// distance_host.cpp — the distance GJK of csrc/dist_simplex.h on the host, over a plain first-maximum
// support scan: the same simplex arithmetic the distance kernel runs, so tests/test_distance_host.py
// can check it against brute force without a GPU.  Built by that test (g++ -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../collision-detect-gjk-epa_amd/csrc/dist_simplex.h"
#include "../include/gjkepa.h"

namespace {

template <typename TIn> struct Hull {
    const TIn* p;
    int n;
    gkd::D3 at(int i) const { return gkd::mk((double)p[i], (double)p[n + i], (double)p[2 * n + i]); }
    bool finite() const {
        for (int i = 0; i < 3 * n; ++i)
            if (!std::isfinite((double)p[i])) return false;
        return true;
    }
};

template <typename TIn>
void one_pair(const Hull<TIn>& A, const Hull<TIn>& B, double max_distance, gjkepa_distance_f64* o) {
    std::memset(o, 0, sizeof(*o));
    for (int k = 0; k < 3; ++k) o->code[k] = gkd::kDistNoCode;
    if (A.n < 1 || B.n < 1 || A.n > GJKEPA_MAX_HULL_VERTS || B.n > GJKEPA_MAX_HULL_VERTS || !A.finite() || !B.finite()) {
        o->status = GJKEPA_STATUS_BAD_INPUT;
        return;
    }
    gkd::Simplex s;
    const gkd::Result r = gkd::dist_gjk(
        s, max_distance,
        [&](gkd::D3 d, int& ia, int& ib) {
            double va = -1.7976931348623157e308, vb = va;
            ia = ib = 0;
            for (int i = 0; i < A.n; ++i) {
                const gkd::D3 a = A.at(i);
                const double t = d.x * a.x + d.y * a.y + d.z * a.z;
                if (t > va) { va = t; ia = i; }
            }
            for (int j = 0; j < B.n; ++j) {
                const gkd::D3 b = B.at(j);
                const double t = -(d.x * b.x + d.y * b.y + d.z * b.z);
                if (t > vb) { vb = t; ib = j; }
            }
        },
        [&](int ia, int ib) { return gkd::sub(A.at(ia), B.at(ib)); }, [](double x) { return std::sqrt(x); });
    o->iters = (uint32_t)r.iters;
    if (r.outcome == gkd::DIST_OVERLAP) {
        o->flags = GJKEPA_DIST_OVERLAP;
        return;
    }
    double pa[3] = {0, 0, 0}, pb[3] = {0, 0, 0};
    for (int k = 0; k < s.n; ++k) {
        const gkd::D3 a = A.at((int)(s.code[k] & 0xffffu)), b = B.at((int)(s.code[k] >> 16));
        pa[0] += s.lam[k] * a.x; pa[1] += s.lam[k] * a.y; pa[2] += s.lam[k] * a.z;
        pb[0] += s.lam[k] * b.x; pb[1] += s.lam[k] * b.y; pb[2] += s.lam[k] * b.z;
        o->lambda[k] = s.lam[k];
        o->code[k] = s.code[k];
    }
    o->n_simplex = (int8_t)s.n;
    const double d[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
    const double dist = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    o->distance = dist;
    for (int i = 0; i < 3; ++i) {
        o->point_a[i] = pa[i];
        o->point_b[i] = pb[i];
        if (dist > 0.0) o->normal[i] = d[i] / dist;
    }
    if (r.outcome == gkd::DIST_FAR) { o->flags = GJKEPA_DIST_FAR; o->distance = r.lower; }
    if (r.outcome == gkd::DIST_MAXITER) o->status = GJKEPA_STATUS_DIST_MAXITER;
}

}  // namespace

extern "C" int distance_host_batch(int vert_dtype, const void* verts, const int64_t* hull_off, const int32_t* hull_cnt,
                                   const int32_t* pairs, int64_t n_pairs, double max_distance, void* out) {
    static_assert(sizeof(gjkepa_distance_f64) == 128, "record layout");
    gjkepa_distance_f64* o = (gjkepa_distance_f64*)out;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t ha = pairs[2 * p], hb = pairs[2 * p + 1];
        if (vert_dtype == GJKEPA_DTYPE_F32) {
            const float* v = (const float*)verts;
            one_pair(Hull<float>{v + hull_off[ha], hull_cnt[ha]}, Hull<float>{v + hull_off[hb], hull_cnt[hb]}, max_distance, o + p);
        } else {
            const double* v = (const double*)verts;
            one_pair(Hull<double>{v + hull_off[ha], hull_cnt[ha]}, Hull<double>{v + hull_off[hb], hull_cnt[hb]}, max_distance, o + p);
        }
    }
    return 0;
}
