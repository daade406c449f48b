// mass_kernel.hip — CDNA4 (gfx950) batched mass properties of hulls: volume, centre of mass, inertia tensor,
// area, closure and bounding radius per cloud (include/gjkepa.h gjkepa_mass_batch_device).
// mass_props.h is the definition's text; this file spreads its sums over the lanes of a wave without changing
// their shape.
//
// Mapping onto the wavefront.  One wave owns one cloud, whatever its size; wave w of the grid takes clouds
// w, w + waves, ..: static assignment, no atomics, no workspace, one launch.  (The hull module's second shape,
// 16 lanes per cloud of at most 64 points with four partials per lane, was built and measured: 0.78 of this
// shape's rate on 64-point clouds, at 256 registers against 112. A 64-point hull has up to 124 faces, so a
// wave is not short of work on it.  DESIGN.md §20 has the numbers.)
//   * points: lane l widens points l, l + 64, .. into the wave's LDS image and checks that they are finite.
//     Gathering the faces' points from the image instead of from HBM measured 1.12x / 1.34x faster (64 / 256 points).
//   * faces: lane l holds the definition's partial l: faces l, l + 64, .. in ascending order.  Each face's
//     three indices are read once and checked against n before a point is read through them; a face with an
//     index out of range reads nothing and the cloud is BAD_INPUT.
//   * the butterfly: the steps 1 .. 32 of gk_common.h xchg (DPP inside a row of 16, permlane swaps above);
//     every lane ends with the same 14 totals.
//   * radius: a second pass over the LDS image, a wave maximum, one square root.
//   * lane 0 stores the record (eight 16-byte stores) and, for an OK cloud, com into the motion block.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gjkepa.h"
#include "gk_common.h"
#include "mass_kernel.h"
#include "mass_props.h"

namespace gk {
namespace mp {

constexpr int kWaves = 4;                          // waves per block, each on clouds of its own
constexpr int NP = GJKEPA_HULL_MAX_POINTS;

static_assert(sizeof(gjkepa_mass_f64) == 128, "record size");
static_assert(gkm::kPartials == 64, "one partial per lane of a wave");

DEV double dsqrt(double x) { return ::sqrt(x); }

// wave-scope ordering point between LDS writes of some lanes and reads of others
DEV void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct MassLds {
    double x[NP], y[NP], z[NP];
};

// v = v + partner(v), step after step: P[l] = P[l] + P[l ^ s] for s = 1 .. 32
template <int S> DEV void sum_steps(double& v) {
    if constexpr (S < 6) {
        v = v + xchg<S>(v);
        sum_steps<S + 1>(v);
    }
}

template <typename TIn> DEV gjkepa_mass_f64 run_cloud(MassLds& L, int lane, const gjkepa_mass_args& a, int64_t ci) {
    const int n = a.cloud_cnt[ci];
    const int hs = a.hull_status ? (int)a.hull_status[ci] : 0;
    const bool n_ok = n >= 4 && n <= NP;
    const int F = n_ok ? a.n_faces[ci] : 0;
    int st = n_ok ? gkm::mass_precheck(n, a.hull_status != nullptr, hs, F) : GJKEPA_STATUS_BAD_INPUT;
    if (st != GJKEPA_STATUS_OK) return gkm::mass_blank(st);
    auto P = [&](int i) { return gkd::mk(L.x[i], L.y[i], L.z[i]); };
    const TIn* src = (const TIn*)a.points + a.cloud_off[ci];
    bool good = true;
    for (int i = lane; i < n; i += 64) {
        const double x = (double)src[i], y = (double)src[n + i], z = (double)src[2 * n + i];
        good &= gkm::finite_d(x) && gkm::finite_d(y) && gkm::finite_d(z);
        L.x[i] = x; L.y[i] = y; L.z[i] = z;
    }
    lds_sync();
    const int32_t* fc = a.faces + 3 * a.face_off[ci];
    const int i0 = fc[0];
    const bool i0_ok = i0 >= 0 && i0 < n;
    good &= i0_ok;
    const gkd::D3 o = P(i0_ok ? i0 : 0);
    double T[gkm::kTerms];
#pragma unroll
    for (int t = 0; t < gkm::kTerms; ++t) T[t] = 0.0;
    for (int f = lane; f < F; f += gkm::kPartials) {
        const int ia = fc[3 * f], ib = fc[3 * f + 1], ic = fc[3 * f + 2];
        const bool in = ia >= 0 && ia < n && ib >= 0 && ib < n && ic >= 0 && ic < n;
        good &= in;
        if (in) gkm::face_add(o, P(ia), P(ib), P(ic), dsqrt, T);
    }
#pragma unroll
    for (int t = 0; t < gkm::kTerms; ++t) sum_steps<0>(T[t]);
    gjkepa_mass_f64 r = gkm::mass_blank(GJKEPA_STATUS_BAD_INPUT);
    if (__ballot(!good) == 0) {
        r = gkm::mass_results(T, o, F);
        const gkd::D3 c = gkd::mk(r.com[0], r.com[1], r.com[2]);
        double qq = 0.0;
        for (int i = lane; i < n; i += 64) {
            const double t = gkd::swept_q2(P(i), c);
            qq = t > qq ? t : qq;
        }
        r.radius = dsqrt(gmax<64>(qq));
        st = gkm::mass_status(T[0], r);
        if (st != GJKEPA_STATUS_OK) r = gkm::mass_blank(st);
    }
    lds_sync();   // the image is free for the wave's next cloud
    return r;
}

template <typename TIn> __global__ __launch_bounds__(64 * kWaves) void mass_kernel(const gjkepa_mass_args a) {
    __shared__ MassLds Ls[kWaves];
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    for (int64_t ci = (int64_t)blockIdx.x * kWaves + wave; ci < a.n_clouds; ci += waves) {
        union {
            gjkepa_mass_f64 m;
            uint4 q[8];
        } u;
        u.m = run_cloud<TIn>(Ls[wave], lane, a, ci);
        if (lane == 0) {
            uint4* dst = (uint4*)a.out + ci * 8;
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[q] = u.q[q];
            if (a.body_motion && u.m.status == GJKEPA_STATUS_OK) {
                double* m = a.body_motion + GJKEPA_MOTION_DOUBLES * ci;
                m[6] = u.m.com[0]; m[7] = u.m.com[1]; m[8] = u.m.com[2];
            }
        }
    }
}

template <typename TIn> hipError_t launch(const gjkepa_mass_args& a, hipStream_t s) {
    const int64_t blocks = (a.n_clouds + kWaves - 1) / kWaves, cap = (int64_t)(a.num_cus > 0 ? a.num_cus : 256) * 8;
    hipLaunchKernelGGL(mass_kernel<TIn>, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(64 * kWaves), 0, s, a);
    return hipGetLastError();
}

}  // namespace mp
}  // namespace gk

hipError_t gjkepa_launch_mass(int vert_dtype, const gjkepa_mass_args& a, hipStream_t s) {
    if (a.n_clouds < 1) return hipSuccess;
    return vert_dtype == GJKEPA_DTYPE_F32 ? gk::mp::launch<float>(a, s) : gk::mp::launch<double>(a, s);
}
