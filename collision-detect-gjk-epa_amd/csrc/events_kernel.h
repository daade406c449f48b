// events_kernel.h — host-side interface of the event pass (internal, not the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define GJKEPA_EVENTS_TILE 4096   // records per block of the key pass

// workspace bytes for n_pairs pairs (-1 when the device query fails); the floor leaves the sort's scratch out
// and needs no device
int64_t gjkepa_events_ws_bytes(int64_t n_pairs);
int64_t gjkepa_events_ws_floor(int64_t n_pairs);

// enqueue the key / total / sort / emit / time pipeline on `s`; sets *ws_too_small (and enqueues nothing) when
// ws_bytes is below gjkepa_events_ws_bytes(n_pairs).  n_pairs == 0 clears the counts and fills the body outputs.
// body_time / body_event: both or neither.
hipError_t gjkepa_enqueue_events(const int32_t* pairs, int64_t n_pairs, int64_t n_hulls, const void* cast_records,
                                 const void* records, int rec_prec, int rec_bytes, void* events, int64_t max_events,
                                 int64_t* n_events, int64_t* counts, double* body_time, int32_t* body_event, void* ws,
                                 int64_t ws_bytes, hipStream_t s, bool* ws_too_small);

// enqueue the gather out[k] = manifolds[events[k].pair], k < min(*n_events, max_events), on `s` (max_events > 0)
hipError_t gjkepa_enqueue_event_manifolds(const void* events, const int64_t* n_events, int64_t max_events,
                                          const void* manifolds, void* out, hipStream_t s);
