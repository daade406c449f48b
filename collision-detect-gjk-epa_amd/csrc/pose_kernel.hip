// pose_kernel.hip — gjkepa_pose_pool_device: every vertex of every hull of a pool moved along its body's
// path (rigid_pose.h) to the hull's time, the arithmetic of the rigid-motion cast exactly.
//
// A streaming kernel: one wave per hull, grid-stride over the hulls.  Lane l holds vertices l, l + 64, ...
// of the hull (at most kRounds = GJKEPA_MAX_HULL_VERTS / 64 each, three coalesced loads per round), the
// wave agrees on whether every value is finite, and only then are the posed vertices stored: nothing is
// written for a bad hull, and since the whole hull is read before any of it is written the output may be
// the input.  The motion block and the time are wave-uniform.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gjkepa.h"
#include "pose_kernel.h"
#include "rigid_pose.h"

namespace {

constexpr int kWaves = 4;                                    // waves per block
constexpr int kRounds = GJKEPA_MAX_HULL_VERTS / 64;
static_assert(GJKEPA_MAX_HULL_VERTS % 64 == 0, "a hull is a whole number of wave rounds");
static_assert(gkd::kMotionDoubles == GJKEPA_MOTION_DOUBLES, "rigid_pose.h against gjkepa.h");

template <typename TIn, typename TOut>
__global__ __launch_bounds__(64 * kWaves) void pose_kernel(const gjkepa_pose_args a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const TIn* in = (const TIn*)a.verts_in;
    TOut* out = (TOut*)a.verts_out;
    for (int64_t h = (int64_t)blockIdx.x * kWaves + wave; h < a.n_hulls; h += (int64_t)gridDim.x * kWaves) {
        // the hull's count, offset, time and motion block are loaded together, before anything is judged:
        // the vertex loads then wait for one round trip to memory, not for one per test
        const int n = a.hull_cnt[h];
        const int64_t off = a.hull_off[h];
        const double t = a.time ? a.time[h] : 1.0;
        double m[GJKEPA_MOTION_DOUBLES];
#pragma unroll
        for (int j = 0; j < GJKEPA_MOTION_DOUBLES; ++j) m[j] = a.body_motion[GJKEPA_MOTION_DOUBLES * h + j];
        bool ok = n >= 1 && n <= GJKEPA_MAX_HULL_VERTS;
        ok = ok & gkd::motion_finite(m) & std::isfinite(t);
        double x[kRounds], y[kRounds], z[kRounds];
        bool finite = true;
        if (ok) {
#pragma unroll
            for (int k = 0; k < kRounds; ++k) {
                const int i = k * 64 + lane;
                x[k] = y[k] = z[k] = 0.0;
                if (i < n) {
                    x[k] = (double)in[off + i];
                    y[k] = (double)in[off + n + i];
                    z[k] = (double)in[off + 2 * (int64_t)n + i];
                }
                finite = finite && std::isfinite(x[k]) && std::isfinite(y[k]) && std::isfinite(z[k]);
            }
            ok = __ballot(!finite) == 0;
        }
        if (a.status && lane == 0) a.status[h] = ok ? GJKEPA_STATUS_OK : GJKEPA_STATUS_BAD_INPUT;
        if (!ok) continue;
        const gkd::Motion mo = gkd::motion_of(m);
        const gkd::PoseState s = gkd::pose_state(mo.v, mo.w, t);
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            const int i = k * 64 + lane;
            if (i < n) {
                const gkd::D3 p = gkd::pose_point(s, mo.c, gkd::mk(x[k], y[k], z[k]));
                out[off + i] = (TOut)p.x;
                out[off + n + i] = (TOut)p.y;
                out[off + 2 * (int64_t)n + i] = (TOut)p.z;
            }
        }
    }
}

template <typename TIn, typename TOut>
hipError_t launch(const gjkepa_pose_args& a, int num_cus, hipStream_t s) {
    const int64_t blocks = (a.n_hulls + kWaves - 1) / kWaves, cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
    hipLaunchKernelGGL((pose_kernel<TIn, TOut>), dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(64 * kWaves), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t gjkepa_launch_pose(int in_dtype, int out_dtype, const gjkepa_pose_args& a, int num_cus, hipStream_t s) {
    if (in_dtype == GJKEPA_DTYPE_F32)
        return out_dtype == GJKEPA_DTYPE_F32 ? launch<float, float>(a, num_cus, s) : launch<float, double>(a, num_cus, s);
    return out_dtype == GJKEPA_DTYPE_F32 ? launch<double, float>(a, num_cus, s) : launch<double, double>(a, num_cus, s);
}
