// mass_kernel.h — host-side interface of the mass-property kernel (internal, not the C-ABI).
//
// One launch over the cloud list, one wave per cloud (mass_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct gjkepa_mass_args {
    const void* points;
    const int64_t* cloud_off;
    const int32_t* cloud_cnt;
    int64_t n_clouds;
    const int64_t* face_off;
    const int32_t* faces;
    const int32_t* n_faces;
    const int8_t* hull_status;  // optional
    void* out;                  // gjkepa_mass_f64 per cloud
    double* body_motion;        // optional
    int num_cus;
};

hipError_t gjkepa_launch_mass(int vert_dtype, const gjkepa_mass_args& a, hipStream_t s);
