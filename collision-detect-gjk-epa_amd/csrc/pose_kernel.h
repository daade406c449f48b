// pose_kernel.h — host-side interface of the pool pose (gjkepa_pose_pool_device; internal, not the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct gjkepa_pose_args {
    const void* verts_in;           // the pool, in_dtype
    const int64_t* hull_off;
    const int32_t* hull_cnt;
    int64_t n_hulls;
    const double* body_motion;      // GJKEPA_MOTION_DOUBLES per hull
    const double* time;             // per hull, or nullptr: t = 1
    void* verts_out;                // the input pool's offsets, out_dtype (may be verts_in when the dtypes are equal)
    int8_t* status;                 // per hull, or nullptr
};
// one launch on `s` (n_hulls >= 1); dtypes: GJKEPA_DTYPE_*
hipError_t gjkepa_launch_pose(int in_dtype, int out_dtype, const gjkepa_pose_args& a, int num_cus, hipStream_t s);
