// cast_host.cpp — the linear cast of csrc/cast_advance.h on the host, over a plain first-maximum
// support scan: the same advancement and simplex arithmetic the cast kernel runs, so
// tests/test_cast_host.py can check it without a GPU.  Built by that test (g++ -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../collision-detect-gjk-epa_amd/csrc/cast_advance.h"
#include "../include/gjkepa.h"

namespace {

static_assert(gkd::kCastFlagImpact == GJKEPA_CAST_IMPACT && gkd::kCastFlagStart == GJKEPA_CAST_START &&
              gkd::kCastStatusMaxIter == GJKEPA_STATUS_CAST_MAXITER, "cast_advance.h against gjkepa.h");

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
void one_pair(const Hull<TIn>& A, const Hull<TIn>& B, const double* motion, double tau, gjkepa_cast_f64* o) {
    std::memset(o, 0, sizeof(*o));
    for (int k = 0; k < 3; ++k) o->code[k] = gkd::kDistNoCode;
    if (A.n < 1 || B.n < 1 || A.n > GJKEPA_MAX_HULL_VERTS || B.n > GJKEPA_MAX_HULL_VERTS || !A.finite() || !B.finite() ||
        !std::isfinite(motion[0]) || !std::isfinite(motion[1]) || !std::isfinite(motion[2])) {
        o->status = GJKEPA_STATUS_BAD_INPUT;
        return;
    }
    const gkd::D3 d = gkd::mk(motion[0], motion[1], motion[2]);
    auto sqrt_ = [](double x) { return std::sqrt(x); };
    gkd::Simplex s;
    const gkd::CastResult r = gkd::cast_advance(
        s, d, tau,
        [&](gkd::D3 dir, int& ia, int& ib) {
            double va = -1.7976931348623157e308, vb = va;
            ia = ib = 0;
            for (int i = 0; i < A.n; ++i) {
                const gkd::D3 a = A.at(i);
                const double t = dir.x * a.x + dir.y * a.y + dir.z * a.z;
                if (t > va) { va = t; ia = i; }
            }
            for (int j = 0; j < B.n; ++j) {
                const gkd::D3 b = B.at(j);
                const double t = -(dir.x * b.x + dir.y * b.y + dir.z * b.z);
                if (t > vb) { vb = t; ib = j; }
            }
        },
        [&](int ia, int ib) { return gkd::sub(A.at(ia), B.at(ib)); }, sqrt_);
    double o13[13];
    int n, status, flags;
    gkd::cast_record(r, s, d, [&](int i) { return A.at(i); }, [&](int i) { return B.at(i); }, sqrt_, o13, o->code, n, status, flags);
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

}  // namespace

extern "C" int cast_host_batch(int vert_dtype, const void* verts, const int64_t* hull_off, const int32_t* hull_cnt,
                               const int32_t* pairs, int64_t n_pairs, const double* motion, double tolerance, void* out) {
    static_assert(sizeof(gjkepa_cast_f64) == 128, "record layout");
    gjkepa_cast_f64* o = (gjkepa_cast_f64*)out;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t ha = pairs[2 * p], hb = pairs[2 * p + 1];
        if (vert_dtype == GJKEPA_DTYPE_F32) {
            const float* v = (const float*)verts;
            one_pair(Hull<float>{v + hull_off[ha], hull_cnt[ha]}, Hull<float>{v + hull_off[hb], hull_cnt[hb]}, motion + 3 * p,
                     tolerance, o + p);
        } else {
            const double* v = (const double*)verts;
            one_pair(Hull<double>{v + hull_off[ha], hull_cnt[ha]}, Hull<double>{v + hull_off[hb], hull_cnt[hb]}, motion + 3 * p,
                     tolerance, o + p);
        }
    }
    return 0;
}
