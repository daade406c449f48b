// mass_host.cpp — csrc/mass_props.h run on the host: the definition's text (gkm::mass_cloud: the per-face terms,
// the 64 partials and their butterfly, the results and the status rules the kernel runs) over a pool of clouds,
// for tests/test_mass_host.py to hold against the numpy restatement (tests/mass_ref.py) without a GPU.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared; -DMASS_HOST_MAIN adds a main for a stand-alone
// run under sanitizers.
#include <cmath>
#include <cstdint>

#include "../collision-detect-gjk-epa_amd/csrc/mass_props.h"

static_assert(sizeof(gjkepa_mass_f64) == 128, "record size");

// the arguments of gjkepa_mass_batch_device, host pointers; out[c] for every cloud
extern "C" int mass_host(int vert_dtype, const void* points, const int64_t* cloud_off, const int32_t* cloud_cnt,
                         int64_t n_clouds, const int64_t* face_off, const int32_t* faces, const int32_t* n_faces,
                         const int8_t* hull_status, gjkepa_mass_f64* out) {
    auto sq = [](double x) { return std::sqrt(x); };
    for (int64_t c = 0; c < n_clouds; ++c) {
        const int n = cloud_cnt[c];
        const int8_t* hs = hull_status ? hull_status + c : nullptr;
        const int32_t* fc = faces + 3 * face_off[c];
        if (vert_dtype == GJKEPA_DTYPE_F32) out[c] = gkm::mass_cloud((const float*)points + cloud_off[c], n, fc, n_faces[c], hs, sq);
        else out[c] = gkm::mass_cloud((const double*)points + cloud_off[c], n, fc, n_faces[c], hs, sq);
    }
    return 0;
}

#ifdef MASS_HOST_MAIN
// Octahedra of seeded size and place, with face indices out of range, a NaN point, bad counts and an inward
// winding among them, for a stand-alone run under -fsanitize=address,undefined.  Prints the status counts.
#include <cstdio>
#include <vector>
int main() {
    const int64_t nc = 512;
    const int oct[8][3] = {{0, 2, 4}, {2, 1, 4}, {1, 3, 4}, {3, 0, 4}, {2, 0, 5}, {1, 2, 5}, {3, 1, 5}, {0, 3, 5}};
    std::vector<double> pts;
    std::vector<int64_t> off(nc), foff(nc);
    std::vector<int32_t> cnt(nc), nf(nc), faces;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int64_t c = 0; c < nc; ++c) {
        const double r = 0.5 + (double)(next() % 100) / 50.0, cx = (double)(next() % 21) - 10.0;
        const int kind = (int)(c % 8);   // 1: index n, 2: index -1, 3: NaN point, 4: n = 3, 5: F = 3, 6: inward
        const int n = kind == 4 ? 3 : 7;
        off[c] = (int64_t)pts.size();
        foff[c] = (int64_t)faces.size() / 3;
        cnt[c] = n;
        nf[c] = kind == 5 ? 3 : 8;
        const double v[7][3] = {{r, 0, 0}, {-r, 0, 0}, {0, r, 0}, {0, -r, 0}, {0, 0, r}, {0, 0, -r}, {kind == 3 ? NAN : 0.0, 0, 0}};
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < n; ++i) pts.push_back(v[i][k] + (k == 0 ? cx : 0.0));
        for (int f = 0; f < 8; ++f) {
            int t[3] = {oct[f][0], oct[f][kind == 6 ? 2 : 1], oct[f][kind == 6 ? 1 : 2]};
            if (f == 5 && kind == 1) t[1] = n;
            if (f == 7 && kind == 2) t[2] = -1;
            for (int k = 0; k < 3; ++k) faces.push_back(t[k]);
        }
    }
    std::vector<gjkepa_mass_f64> out(nc);
    if (mass_host(GJKEPA_DTYPE_F64, pts.data(), off.data(), cnt.data(), nc, foff.data(), faces.data(), nf.data(), nullptr, out.data()))
        return 1;
    int64_t by[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t c = 0; c < nc; ++c) {
        by[out[c].status & 7] += 1;
        const bool want_ok = c % 8 == 0 || c % 8 == 7;
        if ((out[c].status == GJKEPA_STATUS_OK) != want_ok) return 2;
        if (c % 8 == 6 && out[c].status != GJKEPA_STATUS_DEGENERATE) return 3;
        if (!want_ok && (out[c].volume != 0.0 || out[c].n_faces != 0)) return 4;
    }
    std::printf("OK %lld DEGENERATE %lld BAD_INPUT %lld\n", (long long)by[GJKEPA_STATUS_OK], (long long)by[GJKEPA_STATUS_DEGENERATE],
                (long long)by[GJKEPA_STATUS_BAD_INPUT]);
    std::printf("mass_host clean\n");
    return 0;
}
#endif
