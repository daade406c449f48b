// sweep_kernel.hip — CDNA4 (gfx950) swept broad phase: the pair list of the casts.
//
// What it computes: the pairs (a < b) of valid hulls that pass swept_pair (swept_sphere.h): the bounding
// balls about the pivots, moving on c + t v, can come within the tolerance during t in [0, 1].  The list is
// in ascending (a, b) order and does not depend on long_radius.
//
// Pipeline on one stream, no host synchronisation (graph-capturable), the shape of broadphase_kernel.hip:
//   1. ball_kernel    16 lanes per hull (LDS-staged coalesced loads): validity, rho, R = rho + 0.5 |v|; the
//                     largest R among the bodies that stay in the grid (one atomic per block).
//   2. key_kernel     uniform grid over the enclosing balls (g = c + 0.5 v, R): cell edge 2 R_max + tolerance
//                     widened by a relative margin; 63-bit cell keys; a body with R > long_radius gets kLong,
//                     above every cell key and below the invalid key.
//   3. radix sort of (key, hull); gather of c, v, rho into sorted order.  The long bodies are one contiguous
//      run behind the cells; bounds_kernel writes where it begins and ends.
//   4. cell table; grid_kernel<count>; long_kernel<count> (every valid body against the long run, added to the
//      grid pass's count); exclusive scan; grid_kernel<emit> forwards and long_kernel<emit> backwards in each
//      body's range.
//   5. radix sort of the max_pairs keys (padded with all-ones); unpack to int32 (a, b) pairs.
// The cell table, total and unpack kernels repeat broadphase_kernel.hip's: kernels are not shared between
// translation units, and the static broad phase's code objects stay as they are.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/gjkepa.h"
#include "sweep_kernel.h"
#include "swept_sphere.h"

#define DEV_SW __device__ __forceinline__

namespace gk {
namespace sw {

constexpr uint64_t kMask = (1ull << 21) - 1;
constexpr uint64_t kInvalid = ~0ull;
constexpr uint64_t kLong = ~0ull - 1;      // cell keys are below 2^63

DEV_SW uint64_t cell_key(uint64_t ix, uint64_t iy, uint64_t iz) { return ((iz & kMask) << 42) | ((iy & kMask) << 21) | (ix & kMask); }
DEV_SW double dsqrt(double x) { return ::sqrt(x); }
DEV_SW bool finite_d(double x) { return x - x == 0.0; }      // false for NaN and +-inf

// validity, rho and R of every hull; the largest R of the bodies that stay in the grid.  A group of SG lanes
// owns a hull: it stages the hull's 3n scalars in LDS with coalesced loads, then every lane takes vertices
// gl, gl+SG, ... for max q.q and the finiteness of the coordinates (both order-free); lanes 0 .. 8 check the
// motion block.  rho[h] is NaN for a hull that takes part in no pair.
constexpr int SG = 16;
constexpr int BALL_BLOCK = 128;    // 8 hulls per block
constexpr int BALL_STAGE = 64;     // hulls of up to 64 vertices are staged: 6 KB (fp32) of LDS per block
template <typename TIn>
__global__ __launch_bounds__(BALL_BLOCK) void ball_kernel(const TIn* __restrict__ verts, const int64_t* __restrict__ hull_off,
                                                          const int32_t* __restrict__ hull_cnt, int64_t n_hulls,
                                                          const double* __restrict__ motion, double long_radius,
                                                          double* __restrict__ rho, double* __restrict__ big,
                                                          unsigned long long* __restrict__ rmax_bits) {
    constexpr int GPB = BALL_BLOCK / SG;
    __shared__ TIn stage[GPB][3 * BALL_STAGE];
    __shared__ unsigned long long blk;
    const int gl = threadIdx.x % SG, grp = threadIdx.x / SG;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t base = blockIdx.x * (int64_t)GPB; base < n_hulls; base += (int64_t)gridDim.x * GPB) {
        const int64_t h = base + grp;
        const int n = h < n_hulls ? hull_cnt[h] : 0;
        const bool in = h < n_hulls && n >= 1 && n <= GJKEPA_MAX_HULL_VERTS;
        const TIn* p = in ? verts + hull_off[h] : verts;
        if (in && n <= BALL_STAGE)
            for (int i = gl; i < 3 * n; i += SG) stage[grp][i] = p[i];
        __syncthreads();
        const TIn* q = n <= BALL_STAGE ? stage[grp] : p;   // larger hulls are read in place
        const double* m = motion + (h < n_hulls ? h : 0) * gkd::kMotionDoubles;
        int bad = !in;
        double qq = 0.0;
        if (in) {
            if (gl < gkd::kMotionDoubles) bad |= !finite_d(m[gl]);
            const gkd::D3 c = gkd::mk(m[6], m[7], m[8]);
            for (int i = gl; i < n; i += SG) {
                const gkd::D3 x = gkd::mk((double)q[i], (double)q[n + i], (double)q[2 * n + i]);
                bad |= !(finite_d(x.x) && finite_d(x.y) && finite_d(x.z));
                const double t = gkd::swept_q2(x, c);
                qq = t > qq ? t : qq;
            }
        }
#pragma unroll
        for (int k = SG / 2; k >= 1; k /= 2) {
            const double o = __shfl_xor(qq, k, SG);
            qq = o > qq ? o : qq;
            bad |= __shfl_xor(bad, k, SG);
        }
        if (h < n_hulls && gl == 0) {
            double r = NAN, R = NAN;
            if (!bad) {
                r = dsqrt(qq);
                R = gkd::swept_radius(r, gkd::mk(m[0], m[1], m[2]), dsqrt);
                if (!(R > long_radius)) {   // R >= 0: the bit patterns of non-negative doubles order like the values
                    const unsigned long long b = (unsigned long long)__double_as_longlong(R);
                    mine = b > mine ? b : mine;
                }
            }
            rho[h] = r;
            big[h] = R;
        }
        __syncthreads();
    }
    atomicMax(&blk, mine);
    __syncthreads();
    if (threadIdx.x == 0 && blk) atomicMax(rmax_bits, blk);
}

// Grid cell of every body that stays in the grid, from its enclosing ball (g, R).
// A passing pair lies in neighbouring cells: with s the definition's parameter, the ball centres at s are
// dist <= lim apart and g_x - (c_x + s v_x) = (0.5 - s) v_x is at most 0.5 |v_x| long, so
//     |g_a - g_b| <= lim + 0.5 |v_a| + 0.5 |v_b| = (R_a + R_b + tolerance) + slack,
//     slack = 1e-9 ((reach + max|d_k|) + max|e_k|).
// For a passing pair |d| <= dist + |e| <= lim + |e| and |e| <= |v_a| + |v_b| <= 2 (R_a + R_b), which gives
// slack <= 1e-9 (2 reach + 4 (R_a + R_b)) (1 + 2e-9) < 7e-9 (2 R_max + tolerance).  The edge is widened by
// 1e-6: that covers the slack, the rounding of g and R (2^-52 relative each) and of the quotients g / cell
// (monotone in g; half an ulp each) while they stay below 2^28, far above the 2^21 at which the
// coordinates wrap (aliasing only adds candidates).  So |g_a - g_b| < cell per axis and the floors differ by
// at most one.  An infinite R_max gives an infinite cell and every quotient 0 (a non-finite g has an infinite
// R, so it meets only an infinite cell, and its NaN quotient counts as 0): one cell, still conservative.
DEV_SW uint64_t cell_of(double x, double cell) {
    const double q = floor(x / cell);
    return (uint64_t)(int64_t)(q == q ? q : 0.0);   // inf / inf: an infinite cell holds everything
}

__global__ __launch_bounds__(256) void key_kernel(int64_t n, const double* __restrict__ motion, const double* __restrict__ big,
                                                  double tolerance, double long_radius,
                                                  const unsigned long long* __restrict__ rmax_bits,
                                                  uint64_t* __restrict__ keys, int32_t* __restrict__ idx) {
    const double rmax = __longlong_as_double((long long)*rmax_bits);
    const double cell = (2.0 * rmax + tolerance) * (1.0 + 1e-6);
    for (int64_t h = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; h < n; h += (int64_t)gridDim.x * blockDim.x) {
        const double R = big[h];
        uint64_t k = kInvalid;
        if (R > long_radius) k = kLong;
        else if (!isnan(R)) {
            const double* m = motion + h * gkd::kMotionDoubles;
            const gkd::D3 g = gkd::swept_centre(gkd::mk(m[6], m[7], m[8]), gkd::mk(m[0], m[1], m[2]));
            k = cell_key(cell_of(g.x, cell), cell_of(g.y, cell), cell_of(g.z, cell));
        }
        keys[h] = k;
        idx[h] = (int32_t)h;
    }
}

// c, v, rho in sorted order, so neighbouring threads read neighbouring entries
struct Balls {
    double *cx, *cy, *cz, *vx, *vy, *vz, *rho;
};

__global__ __launch_bounds__(256) void gather_kernel(int64_t n, const int32_t* __restrict__ order,
                                                     const double* __restrict__ motion, const double* __restrict__ rho,
                                                     Balls s) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t h = order[p];
        const double* m = motion + (int64_t)h * gkd::kMotionDoubles;
        s.vx[p] = m[0]; s.vy[p] = m[1]; s.vz[p] = m[2];
        s.cx[p] = m[6]; s.cy[p] = m[7]; s.cz[p] = m[8];
        s.rho[p] = rho[h];
    }
}

// bounds[0], bounds[1]: the sorted positions [begin, end) of the long bodies (both 0 when there are none:
// the caller clears them)
__global__ __launch_bounds__(256) void bounds_kernel(int64_t n, const uint64_t* __restrict__ keys, int64_t* __restrict__ bounds) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[p];
        if (k != kLong) continue;
        if (p == 0 || keys[p - 1] != kLong) bounds[0] = p;
        if (p + 1 == n || keys[p + 1] != kLong) bounds[1] = p + 1;
    }
}

// Cell table: open-addressing hash (linear probing) from a cell key to the first sorted position of that
// cell, built from the segment starts of the sorted keys.
DEV_SW uint64_t mix64(uint64_t x) {
    x ^= x >> 31; x *= 0x7FB5D329728EA185ull; x ^= x >> 27; x *= 0x81DADEF4BC2DD44Dull; x ^= x >> 33;
    return x;
}

__global__ __launch_bounds__(256) void cell_table_kernel(int64_t n, const uint64_t* __restrict__ keys,
                                                         unsigned long long* __restrict__ tkeys,
                                                         int32_t* __restrict__ tstart, uint64_t tmask) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[p];
        if (k >= kLong || (p > 0 && keys[p - 1] == k)) continue;
        for (uint64_t h = mix64(k) & tmask;; h = (h + 1) & tmask) {
            const unsigned long long prev = atomicCAS(&tkeys[h], (unsigned long long)kInvalid, (unsigned long long)k);
            if (prev == (unsigned long long)kInvalid) { tstart[h] = (int32_t)p; break; }
        }
    }
}

// first sorted position of cell k, -1 when the cell is empty
DEV_SW int64_t cell_start(const unsigned long long* __restrict__ tkeys, const int32_t* __restrict__ tstart,
                          uint64_t tmask, uint64_t k) {
    for (uint64_t h = mix64(k) & tmask;; h = (h + 1) & tmask) {
        const uint64_t t = tkeys[h];
        if (t == k) return tstart[h];
        if (t == kInvalid) return -1;
    }
}

struct Ball {
    gkd::D3 c, v;
    double rho;
};
DEV_SW Ball ball_at(const Balls& s, int64_t p) {
    Ball b;
    b.c = gkd::mk(s.cx[p], s.cy[p], s.cz[p]);
    b.v = gkd::mk(s.vx[p], s.vy[p], s.vz[p]);
    b.rho = s.rho[p];
    return b;
}
// the definition's test, lo the ball of the lower hull index
DEV_SW bool pass(const Ball& lo, const Ball& hi, double tolerance) {
    return gkd::swept_pair(lo.c, lo.v, lo.rho, hi.c, hi.v, hi.rho, tolerance, dsqrt);
}

// the bodies q from sorted position q0 on while their cell key is <= kh that form a passing pair with body a
// (larger index); returns how many, writing their keys from out[o] on when EMIT.  kh is a cell key: the run
// ends before the long bodies.
template <bool EMIT>
DEV_SW int64_t visit_range(int64_t q0, uint64_t kh, int64_t n, const uint64_t* __restrict__ keys, const Balls& s,
                           const int32_t* __restrict__ order, int32_t a, const Ball& A, double tolerance,
                           uint64_t* __restrict__ out, int64_t o, int64_t max_pairs) {
    int64_t c = 0;
    for (int64_t q = q0; q < n && keys[q] <= kh; ++q) {
        const int32_t b = order[q];
        if (b <= a) continue;
        if (!pass(A, ball_at(s, q), tolerance)) continue;
        if constexpr (EMIT) {
            if (o + c < max_pairs) out[o + c] = ((uint64_t)(uint32_t)a << 32) | (uint32_t)b;
        }
        ++c;
    }
    return c;
}

// thread p (cell-sorted body): the bodies of the 27 neighbouring cells with a larger index that pass the
// exact test; EMIT = false counts (0 for a long or invalid body), true writes (a << 32 | b) keys at the
// thread's offset
template <bool EMIT>
__global__ __launch_bounds__(256) void grid_kernel(int64_t n, const uint64_t* __restrict__ keys, Balls s,
                                                   const int32_t* __restrict__ order,
                                                   const unsigned long long* __restrict__ tkeys,
                                                   const int32_t* __restrict__ tstart, uint64_t tmask, double tolerance,
                                                   int64_t* __restrict__ counts, const int64_t* __restrict__ offs,
                                                   uint64_t* __restrict__ out, int64_t max_pairs) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[p];
        int64_t c = 0;
        if (k < kLong) {
            const Ball A = ball_at(s, p);
            const int32_t a = order[p];
            const int64_t o = EMIT ? offs[p] : 0;
            const uint64_t ix = k & kMask, iy = (k >> 21) & kMask, iz = k >> 42;
            const bool row = ix >= 1 && ix + 1 <= kMask;          // ix-1..ix+1 contiguous in key order
            for (int t = 0; t < 9; ++t) {
                const uint64_t jy = iy + (uint64_t)(t % 3) - 1, jz = iz + (uint64_t)(t / 3) - 1;
                if (row) {   // the row's first non-empty cell, then forward through the row
                    int64_t q0 = -1;
                    for (uint64_t jx = ix - 1; jx != ix + 2 && q0 < 0; ++jx) q0 = cell_start(tkeys, tstart, tmask, cell_key(jx, jy, jz));
                    if (q0 >= 0)
                        c += visit_range<EMIT>(q0, cell_key(ix + 1, jy, jz), n, keys, s, order, a, A, tolerance, out, o + c,
                                               max_pairs);
                } else {     // the row wraps at 2^21: its three cells separately
                    for (uint64_t jx = ix - 1; jx != ix + 2; ++jx) {
                        const uint64_t kc = cell_key(jx, jy, jz);
                        const int64_t q0 = cell_start(tkeys, tstart, tmask, kc);
                        if (q0 >= 0)
                            c += visit_range<EMIT>(q0, kc, n, keys, s, order, a, A, tolerance, out, o + c, max_pairs);
                    }
                }
            }
        }
        if constexpr (!EMIT) counts[p] = c;
    }
}

// The long bodies (sorted positions [bounds[0], bounds[1])) against every valid body, in a kernel of their
// own: thread p (any valid body) walks the long run, every lane of a wave reading the same entry.  A pair
// of a grid body and a long body is the grid body's thread's; a pair of two long bodies belongs to the
// thread of the lower index.  EMIT = false adds the count to the slot the grid pass filled; true writes the
// keys backwards from the end of the thread's range, offs[p + 1], while the grid pass writes forwards from
// offs[p]: distinct slots without a second offset array, and nothing depends on an atomic.
template <bool EMIT>
__global__ __launch_bounds__(256) void long_kernel(int64_t n, const uint64_t* __restrict__ keys, Balls s,
                                                   const int32_t* __restrict__ order, const int64_t* __restrict__ bounds,
                                                   double tolerance, int64_t* __restrict__ counts,
                                                   const int64_t* __restrict__ offs, uint64_t* __restrict__ out,
                                                   int64_t max_pairs) {
    const int64_t begin = bounds[0], end = bounds[1];
    if (begin == end) return;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[p];
        if (k == kInvalid) continue;
        const Ball A = ball_at(s, p);
        const int32_t a = order[p];
        const int64_t o = EMIT ? offs[p + 1] - 1 : 0;
        int64_t c = 0;
        for (int64_t q = begin; q < end; ++q) {
            const int32_t b = order[q];
            if (k == kLong && b <= a) continue;
            const Ball B = ball_at(s, q);
            if (!(a < b ? pass(A, B, tolerance) : pass(B, A, tolerance))) continue;
            if constexpr (EMIT) {
                const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
                if (o - c < max_pairs) out[o - c] = ((uint64_t)lo << 32) | hi;
            }
            ++c;
        }
        if constexpr (!EMIT) counts[p] += c;
    }
}

__global__ void total_kernel(const int64_t* __restrict__ offs, int64_t n, int64_t* __restrict__ n_pairs) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *n_pairs = offs[n];
}

__global__ __launch_bounds__(256) void unpack_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_pairs,
                                                     int64_t max_pairs, int32_t* __restrict__ pairs) {
    const int64_t m = *n_pairs < max_pairs ? *n_pairs : max_pairs;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t v = keys[k];
        pairs[2 * k] = (int32_t)(v >> 32);
        pairs[2 * k + 1] = (int32_t)(v & 0xffffffffu);
    }
}

}  // namespace sw
}  // namespace gk

namespace {

constexpr size_t kAlign = 256;
size_t up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

struct Layout {
    size_t rho, big, rmax, bounds, keys0, idx, skeys, order, ball[7], counts, offs, tkeys, tstart, pk, pk2, temp, total;
    uint64_t tsize;
    size_t sort1, scan, sort2;
};

hipError_t temp_sizes(int64_t n, int64_t max_pairs, size_t& sort1, size_t& scan, size_t& sort2) {
    hipError_t e;
    sort1 = scan = sort2 = 0;
    if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort1, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                (const int32_t*)nullptr, (int32_t*)nullptr, (int)n)) != hipSuccess)
        return e;
    if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (const int64_t*)nullptr, (int64_t*)nullptr, (int)(n + 1))) != hipSuccess)
        return e;
    return hipcub::DeviceRadixSort::SortKeys(nullptr, sort2, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)max_pairs);
}

Layout layout(int64_t n, int64_t max_pairs, size_t sort1, size_t scan, size_t sort2) {
    Layout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up(bytes); return at; };
    const size_t d = (size_t)n * 8, i = (size_t)n * 4;
    L.rho = take(d); L.big = take(d); L.rmax = take(8); L.bounds = take(16);
    L.keys0 = take(d); L.idx = take(i); L.skeys = take(d); L.order = take(i);
    for (size_t& b : L.ball) b = take(d);
    L.counts = take((size_t)(n + 1) * 8); L.offs = take((size_t)(n + 1) * 8);
    L.tsize = 1024;
    while (L.tsize < 2 * (uint64_t)n) L.tsize *= 2;           // load factor <= 1/2
    L.tkeys = take(L.tsize * 8); L.tstart = take(L.tsize * 4);
    L.pk = take((size_t)max_pairs * 8); L.pk2 = take((size_t)max_pairs * 8);
    L.sort1 = sort1; L.scan = scan; L.sort2 = sort2;
    L.temp = take(std::max(sort1, std::max(scan, sort2)));
    L.total = o;
    return L;
}

template <typename T> T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }

int blocks_for(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

}  // namespace

int64_t gjkepa_sweep_ws_bytes(int64_t n_hulls, int64_t max_pairs) {
    size_t s1, sc, s2;
    if (temp_sizes(n_hulls, max_pairs, s1, sc, s2) != hipSuccess) return -1;
    return (int64_t)layout(n_hulls, max_pairs, s1, sc, s2).total;
}

hipError_t gjkepa_enqueue_sweep(int vert_dtype, const void* verts, const int64_t* hull_off, const int32_t* hull_cnt,
                                int64_t n, const double* body_motion, double tolerance, double long_radius,
                                int32_t* pairs, int64_t max_pairs, int64_t* n_pairs, void* ws, int64_t ws_bytes,
                                hipStream_t s, bool* ws_too_small) {
    using namespace gk::sw;
    size_t s1, sc, s2;
    hipError_t e = temp_sizes(n, max_pairs, s1, sc, s2);
    if (e != hipSuccess) return e;
    const Layout L = layout(n, max_pairs, s1, sc, s2);
    *ws_too_small = (int64_t)L.total > ws_bytes;
    if (*ws_too_small) return hipSuccess;
    const int nb = blocks_for(n);
    // rmax and bounds are neighbours: one clear
    if ((e = hipMemsetAsync(at<void>(ws, L.rmax), 0, L.bounds + 16 - L.rmax, s)) != hipSuccess) return e;
    auto* rmax = at<unsigned long long>(ws, L.rmax);
    auto* bounds = at<int64_t>(ws, L.bounds);
    auto* keys = at<uint64_t>(ws, L.skeys);
    auto* order = at<int32_t>(ws, L.order);
    const Balls balls{at<double>(ws, L.ball[0]), at<double>(ws, L.ball[1]), at<double>(ws, L.ball[2]), at<double>(ws, L.ball[3]),
                      at<double>(ws, L.ball[4]), at<double>(ws, L.ball[5]), at<double>(ws, L.ball[6])};
    const int nbs = blocks_for((n + BALL_BLOCK / SG - 1) / (BALL_BLOCK / SG) * 256);   // one block per BALL_BLOCK / SG hulls
    if (vert_dtype == GJKEPA_DTYPE_F32)
        hipLaunchKernelGGL(ball_kernel<float>, dim3(nbs), dim3(BALL_BLOCK), 0, s, (const float*)verts, hull_off, hull_cnt, n,
                           body_motion, long_radius, at<double>(ws, L.rho), at<double>(ws, L.big), rmax);
    else
        hipLaunchKernelGGL(ball_kernel<double>, dim3(nbs), dim3(BALL_BLOCK), 0, s, (const double*)verts, hull_off, hull_cnt, n,
                           body_motion, long_radius, at<double>(ws, L.rho), at<double>(ws, L.big), rmax);
    hipLaunchKernelGGL(key_kernel, dim3(nb), dim3(256), 0, s, n, body_motion, (const double*)at<double>(ws, L.big), tolerance,
                       long_radius, (const unsigned long long*)rmax, at<uint64_t>(ws, L.keys0), at<int32_t>(ws, L.idx));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = L.sort1;
    if ((e = hipcub::DeviceRadixSort::SortPairs(at<void>(ws, L.temp), tb, at<uint64_t>(ws, L.keys0), keys,
                                                at<int32_t>(ws, L.idx), order, (int)n, 0, 64, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(gather_kernel, dim3(nb), dim3(256), 0, s, n, (const int32_t*)order, body_motion,
                       (const double*)at<double>(ws, L.rho), balls);
    hipLaunchKernelGGL(bounds_kernel, dim3(nb), dim3(256), 0, s, n, (const uint64_t*)keys, bounds);
    if ((e = hipMemsetAsync(at<int64_t>(ws, L.counts) + n, 0, 8, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(at<void>(ws, L.tkeys), 0xFF, L.tsize * 8, s)) != hipSuccess) return e;
    const uint64_t tmask = L.tsize - 1;
    const auto* tkeys = at<unsigned long long>(ws, L.tkeys);
    const auto* tstart = at<int32_t>(ws, L.tstart);
    hipLaunchKernelGGL(cell_table_kernel, dim3(nb), dim3(256), 0, s, n, (const uint64_t*)keys, at<unsigned long long>(ws, L.tkeys),
                       at<int32_t>(ws, L.tstart), tmask);
    hipLaunchKernelGGL(grid_kernel<false>, dim3(nb), dim3(256), 0, s, n, (const uint64_t*)keys, balls, (const int32_t*)order,
                       tkeys, tstart, tmask, tolerance, at<int64_t>(ws, L.counts), (const int64_t*)nullptr, (uint64_t*)nullptr,
                       max_pairs);
    hipLaunchKernelGGL(long_kernel<false>, dim3(nb), dim3(256), 0, s, n, (const uint64_t*)keys, balls, (const int32_t*)order,
                       (const int64_t*)bounds, tolerance, at<int64_t>(ws, L.counts), (const int64_t*)nullptr, (uint64_t*)nullptr,
                       max_pairs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tb = L.scan;
    if ((e = hipcub::DeviceScan::ExclusiveSum(at<void>(ws, L.temp), tb, at<int64_t>(ws, L.counts),
                                              at<int64_t>(ws, L.offs), (int)(n + 1), s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(total_kernel, dim3(1), dim3(64), 0, s, at<int64_t>(ws, L.offs), n, n_pairs);
    if (max_pairs > 0) {
        if ((e = hipMemsetAsync(at<uint64_t>(ws, L.pk), 0xFF, (size_t)max_pairs * 8, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(grid_kernel<true>, dim3(nb), dim3(256), 0, s, n, (const uint64_t*)keys, balls, (const int32_t*)order,
                           tkeys, tstart, tmask, tolerance, (int64_t*)nullptr, (const int64_t*)at<int64_t>(ws, L.offs),
                           at<uint64_t>(ws, L.pk), max_pairs);
        hipLaunchKernelGGL(long_kernel<true>, dim3(nb), dim3(256), 0, s, n, (const uint64_t*)keys, balls,
                           (const int32_t*)order, (const int64_t*)bounds, tolerance, (int64_t*)nullptr,
                           (const int64_t*)at<int64_t>(ws, L.offs), at<uint64_t>(ws, L.pk), max_pairs);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        tb = L.sort2;
        if ((e = hipcub::DeviceRadixSort::SortKeys(at<void>(ws, L.temp), tb, at<uint64_t>(ws, L.pk),
                                                   at<uint64_t>(ws, L.pk2), (int)max_pairs, 0, 64, s)) != hipSuccess)
            return e;
        hipLaunchKernelGGL(unpack_kernel, dim3(blocks_for(max_pairs)), dim3(256), 0, s, at<uint64_t>(ws, L.pk2),
                           (const int64_t*)n_pairs, max_pairs, pairs);
    }
    return hipGetLastError();
}
