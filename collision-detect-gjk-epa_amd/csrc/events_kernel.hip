// events_kernel.hip — CDNA4 (gfx950) event list and per-body clamp of a moving step.
//
// The casts leave one 128-byte record per candidate pair, MISS or not, in pair order.  This pass turns them
// into the events of the step in ascending (time, pair) order and, per body, the first event that stops it
// (event_record.h is the definition's text; include/gjkepa.h gjkepa_events_device the contract).
//
// Pipeline on one stream, no host synchronisation (graph-capturable):
//   1. key_kernel    one block per 4096-record tile: each lane reads the status / flags word and toi of its
//                    records (12 bytes of a 128-byte record: the pass is bound by the record lines it touches,
//                    as contacts_kernel.hip's count pass), writes the key (the time's bits, all-ones for no
//                    event) and the value (the pair index), and the block sums the five classes.
//   2. total_kernel  one block sums the tile counts in tile order: counts[5], *n_events.
//   3. stable radix sort of (key, pair index) (rocPRIM via hipCUB): position = rank, ties by pair index.
//   4. emit_kernel   lane k < n_events takes the pair of rank k; for k < max_events it gathers the pair's
//                    records and writes the event, 16 bytes per store; for an IMPACT or UNDECIDED it takes the
//                    minimum of k into body_event[a] and body_event[b] (cleared to 0xFFFFFFFF = -1 before).
//   5. time_kernel   body_time[h] = the sorted key at rank body_event[h], which is that event's time, or 1.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstddef>
#include <cstdint>

#include "../../include/gjkepa.h"
#include "event_record.h"
#include "events_kernel.h"

namespace gk {
namespace ev {

constexpr int BLOCK = 256;
constexpr int PER_THREAD = 16;
constexpr int TILE = BLOCK * PER_THREAD;   // records per tile
static_assert(TILE == GJKEPA_EVENTS_TILE, "events_kernel.h names the tile size");

// n_simplex, status, flags, reserved share one aligned 32-bit word of the cast record
constexpr int kWordOff = (int)offsetof(gjkepa_cast_f64, n_simplex);
static_assert(kWordOff % 4 == 0 && offsetof(gjkepa_cast_f64, status) == kWordOff + 1 &&
              offsetof(gjkepa_cast_f64, flags) == kWordOff + 2, "status / flags word of gjkepa_cast_f64");
static_assert(sizeof(gjkepa_cast_f64) == 128 && sizeof(gjkepa_event_f64) == 128, "record sizes");

__device__ __forceinline__ int kind_of(const gjkepa_cast_f64* __restrict__ cast, int64_t p) {
    const uint32_t w = *(const uint32_t*)((const char*)(cast + p) + kWordOff);
    return gkev::event_kind((int)(int8_t)(w >> 8), (int)((w >> 16) & 0xffu));
}

__global__ __launch_bounds__(BLOCK) void key_kernel(const gjkepa_cast_f64* __restrict__ cast, int64_t n,
                                                    uint64_t* __restrict__ keys, int32_t* __restrict__ vals,
                                                    int32_t* __restrict__ tile_counts) {
    __shared__ int wsum[BLOCK / 64][gkev::kClasses];
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    int c[gkev::kClasses] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const int64_t k = t0 + (int64_t)j * BLOCK + threadIdx.x;
        if (k < n) {
            const int kind = kind_of(cast, k);
            keys[k] = gkev::event_key(kind, cast[k].toi);
            vals[k] = (int32_t)k;
            const int cls = gkev::event_class(kind);
#pragma unroll
            for (int i = 0; i < gkev::kClasses; ++i) c[i] += cls == i;
        }
    }
#pragma unroll
    for (int i = 0; i < gkev::kClasses; ++i) {
        for (int m = 32; m >= 1; m /= 2) c[i] += __shfl_xor(c[i], m, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x / 64][i] = c[i];
    }
    __syncthreads();
    if (threadIdx.x < gkev::kClasses) {
        int s = 0;
        for (int w = 0; w < BLOCK / 64; ++w) s += wsum[w][threadIdx.x];
        tile_counts[(int64_t)blockIdx.x * gkev::kClasses + threadIdx.x] = s;
    }
}

// counts[i] = sum over the tiles, n_events = counts[0] + .. + counts[3]; one block
__global__ __launch_bounds__(BLOCK) void total_kernel(const int32_t* __restrict__ tile_counts, int64_t tiles,
                                                      int64_t* __restrict__ counts, int64_t* __restrict__ n_events) {
    __shared__ long long part[BLOCK][gkev::kClasses];
    long long c[gkev::kClasses] = {0, 0, 0, 0, 0};
    for (int64_t t = threadIdx.x; t < tiles; t += BLOCK)
        for (int i = 0; i < gkev::kClasses; ++i) c[i] += tile_counts[t * gkev::kClasses + i];
    for (int i = 0; i < gkev::kClasses; ++i) part[threadIdx.x][i] = c[i];
    __syncthreads();
    __shared__ long long sum[gkev::kClasses];
    if (threadIdx.x < gkev::kClasses) {
        long long s = 0;
        for (int t = 0; t < BLOCK; ++t) s += part[t][threadIdx.x];
        counts[threadIdx.x] = s;
        sum[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) *n_events = sum[0] + sum[1] + sum[2] + sum[3];
}

__global__ __launch_bounds__(BLOCK) void emit_kernel(const int32_t* __restrict__ pairs, const gjkepa_cast_f64* __restrict__ cast,
                                                     const uint8_t* __restrict__ records, int rec_prec, int rec_bytes,
                                                     const int32_t* __restrict__ order, const int64_t* __restrict__ n_events,
                                                     uint4* __restrict__ events, int64_t max_events,
                                                     uint32_t* __restrict__ body_event) {
    const int64_t ne = *n_events;
    for (int64_t k = blockIdx.x * (int64_t)BLOCK + threadIdx.x; k < ne; k += (int64_t)gridDim.x * BLOCK) {
        const int32_t p = order[k];
        const int kind = kind_of(cast, p);
        const int32_t a = pairs[2 * (int64_t)p], b = pairs[2 * (int64_t)p + 1];
        if (k < max_events) {
            union {
                gjkepa_event_f64 e;
                uint4 q[8];
            } u;
            u.e = gkev::event_fill(kind, cast[p], records ? records + (int64_t)p * rec_bytes : nullptr, rec_prec, a, b, p);
            uint4* dst = events + k * 8;
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[q] = u.q[q];
        }
        // the pass's only atomic: a minimum does not depend on the order of arrival, so the result is
        // deterministic.  Ranks are below 2^31, and 0xFFFFFFFF (no event) reads as -1.
        if (body_event && gkev::event_clamps(kind)) {
            atomicMin(&body_event[a], (uint32_t)k);
            atomicMin(&body_event[b], (uint32_t)k);
        }
    }
}

// the sorted key at an event's rank is its time's bits
__global__ __launch_bounds__(BLOCK) void time_kernel(const int32_t* __restrict__ body_event, const uint64_t* __restrict__ skeys,
                                                     int64_t n_hulls, double* __restrict__ body_time) {
    for (int64_t h = blockIdx.x * (int64_t)BLOCK + threadIdx.x; h < n_hulls; h += (int64_t)gridDim.x * BLOCK) {
        const int32_t e = body_event[h];
        body_time[h] = e < 0 ? 1.0 : __longlong_as_double((long long)skeys[e]);
    }
}

// The manifolds of the listed events: rank k < min(*n_events, max_events) copies the 160-byte record of its
// event's pair as ten 16-byte loads and stores, one of the ten per lane, so ten consecutive lanes read and
// write one record's consecutive lines.
constexpr int kManifoldQuads = (int)(sizeof(gjkepa_manifold_f64) / 16);
static_assert(sizeof(gjkepa_manifold_f64) == 160 && kManifoldQuads == 10, "a manifold record is ten 16-byte words");
__global__ __launch_bounds__(BLOCK) void gather_manifolds_kernel(const gjkepa_event_f64* __restrict__ events,
                                                                 const int64_t* __restrict__ n_events, int64_t max_events,
                                                                 const uint4* __restrict__ manifolds, uint4* __restrict__ out) {
    const int64_t ne = *n_events;
    const int64_t m = (ne < max_events ? ne : max_events) * kManifoldQuads;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t k = i / kManifoldQuads;
        const int q = (int)(i - k * kManifoldQuads);
        out[i] = manifolds[(int64_t)events[k].pair * kManifoldQuads + q];
    }
}

}  // namespace ev
}  // namespace gk

namespace {

size_t up(size_t x) { return (x + 255) / 256 * 256; }

struct Layout {
    size_t keys0, vals0, skeys, svals, tiles, temp, total;
};

Layout layout(int64_t n, size_t sort) {
    Layout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up(bytes); return at; };
    const size_t tiles = (size_t)((n + gk::ev::TILE - 1) / gk::ev::TILE);
    L.keys0 = take((size_t)n * 8); L.vals0 = take((size_t)n * 4);
    L.skeys = take((size_t)n * 8); L.svals = take((size_t)n * 4);
    L.tiles = take(tiles * gkev::kClasses * 4);
    L.temp = take(sort);
    L.total = o > 256 ? o : 256;
    return L;
}

hipError_t sort_bytes(int64_t n, size_t& sort) {
    sort = 0;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, sort, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                              (const int32_t*)nullptr, (int32_t*)nullptr, (int)(n > 0 ? n : 1));
}

template <typename T> T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }

int blocks_for(int64_t n) {
    const int64_t b = (n + gk::ev::BLOCK - 1) / gk::ev::BLOCK;
    return (int)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

}  // namespace

hipError_t gjkepa_enqueue_event_manifolds(const void* events, const int64_t* n_events, int64_t max_events,
                                          const void* manifolds, void* out, hipStream_t s) {
    using namespace gk::ev;
    hipLaunchKernelGGL(gather_manifolds_kernel, dim3(blocks_for(max_events * kManifoldQuads)), dim3(BLOCK), 0, s,
                       (const gjkepa_event_f64*)events, n_events, max_events, (const uint4*)manifolds, (uint4*)out);
    return hipGetLastError();
}

int64_t gjkepa_events_ws_floor(int64_t n_pairs) { return (int64_t)layout(n_pairs, 0).total; }

int64_t gjkepa_events_ws_bytes(int64_t n_pairs) {
    size_t sort;
    if (sort_bytes(n_pairs, sort) != hipSuccess) return -1;
    return (int64_t)layout(n_pairs, sort).total;
}

hipError_t gjkepa_enqueue_events(const int32_t* pairs, int64_t n, int64_t n_hulls, const void* cast_records,
                                 const void* records, int rec_prec, int rec_bytes, void* events, int64_t max_events,
                                 int64_t* n_events, int64_t* counts, double* body_time, int32_t* body_event, void* ws,
                                 int64_t ws_bytes, hipStream_t s, bool* ws_too_small) {
    using namespace gk::ev;
    hipError_t e;
    *ws_too_small = false;
    const bool bodies = body_time && body_event && n_hulls > 0;
    const uint64_t* skeys = nullptr;
    if (n == 0) {
        if ((e = hipMemsetAsync(n_events, 0, 8, s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(counts, 0, gkev::kClasses * 8, s)) != hipSuccess) return e;
        if (bodies && (e = hipMemsetAsync(body_event, 0xFF, (size_t)n_hulls * 4, s)) != hipSuccess) return e;
    } else {
        size_t sort;
        if ((e = sort_bytes(n, sort)) != hipSuccess) return e;
        const Layout L = layout(n, sort);
        *ws_too_small = (int64_t)L.total > ws_bytes;
        if (*ws_too_small) return hipSuccess;
        const int64_t tiles = (n + TILE - 1) / TILE;
        const auto* cast = (const gjkepa_cast_f64*)cast_records;
        skeys = at<uint64_t>(ws, L.skeys);
        hipLaunchKernelGGL(key_kernel, dim3((unsigned)tiles), dim3(BLOCK), 0, s, cast, n, at<uint64_t>(ws, L.keys0),
                           at<int32_t>(ws, L.vals0), at<int32_t>(ws, L.tiles));
        hipLaunchKernelGGL(total_kernel, dim3(1), dim3(BLOCK), 0, s, (const int32_t*)at<int32_t>(ws, L.tiles), tiles, counts,
                           n_events);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipcub::DeviceRadixSort::SortPairs(at<void>(ws, L.temp), sort, at<uint64_t>(ws, L.keys0), at<uint64_t>(ws, L.skeys),
                                                    at<int32_t>(ws, L.vals0), at<int32_t>(ws, L.svals), (int)n, 0, 64, s)) != hipSuccess)
            return e;
        if (bodies && (e = hipMemsetAsync(body_event, 0xFF, (size_t)n_hulls * 4, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(emit_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, s, pairs, cast, (const uint8_t*)records, rec_prec,
                           rec_bytes, (const int32_t*)at<int32_t>(ws, L.svals), (const int64_t*)n_events, (uint4*)events,
                           max_events, bodies ? (uint32_t*)body_event : nullptr);
    }
    if (bodies)
        hipLaunchKernelGGL(time_kernel, dim3(blocks_for(n_hulls)), dim3(BLOCK), 0, s, (const int32_t*)body_event, skeys, n_hulls,
                           body_time);
    return hipGetLastError();
}
