// capi_internal.h — helpers shared by the C-ABI translation units (not part of the C-ABI).
#pragma once
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstdint>
#include <string>

namespace gjkepa_internal {
// roctx range over one API call (rocprofv3 --marker-trace shows it beside the kernels it enqueued):
// the chain, the record all-gather, the host-buffer round trips (SURVEY.md §5 tracing)
struct Range {
    explicit Range(const char* what) { roctxRangePushA(what); }
    ~Range() { roctxRangePop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};
// record `msg` as the calling thread's gjkepa_last_error() and return `code`
int set_error(int code, const std::string& msg);

// The host-side validation of a hull pool's index structure (device code trusts it): every index of
// `pairs` (n_pairs x 2; nullptr for the entries without a pair list) names a hull, and every hull of 1 to
// max_checked_cnt vertices lies inside the vertex pool.  Returns 0, or GJKEPA_E_ARG with the error set.
// The bound is the one difference between the entries.  The pair-list entries (gjkepa_batch, _batch_multi,
// _distance_batch, _cast_batch) pass kAnyHullCount: a hull above GJKEPA_MAX_HULL_VERTS outside the pool is
// an argument error there, although the kernels answer its pairs BAD_INPUT without reading it.  The
// all-pairs entries (gjkepa_broadphase, gjkepa_collide) pass GJKEPA_MAX_HULL_VERTS: they skip such a hull
// as their kernels do, whatever its offset.  Both are kept as the entries have always behaved.
constexpr int64_t kAnyHullCount = INT32_MAX;
int check_pool(const int32_t* pairs, int64_t n_pairs, const int64_t* hull_off, const int32_t* hull_cnt, int64_t n_hulls,
               int64_t n_vert_scalars, int64_t max_checked_cnt);
}  // namespace gjkepa_internal
