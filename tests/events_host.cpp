// events_host.cpp — csrc/event_record.h run on the host: the text the event pass's kernels run, over a batch of
// cast records, for tests/test_events_host.py to hold against the numpy restatement of the definition
// (tests/events_ref.py) without a GPU.  Build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared;
// -DEVENTS_HOST_MAIN adds a main for a stand-alone run under sanitizers.
#include <cstdint>
#include <cstring>

#include "../collision-detect-gjk-epa_amd/csrc/event_record.h"

// per pair: kind[k] (GJKEPA_EVENT_*, 0 for none, -1 for BAD), key[k] (the sort key) and out[k] (the event
// record; zero for a pair without an event); counts[5] as the device pass counts them.  records: NULL or the
// contact records of records_precision.
extern "C" int events_host(const int32_t* pairs, int64_t n, const gjkepa_cast_f64* cast, const void* records,
                           int records_precision, int8_t* kind, uint64_t* key, gjkepa_event_f64* out, int64_t* counts) {
    const size_t rec = records_precision == GJKEPA_PREC_F64 ? sizeof(gjkepa_contact_f64) : sizeof(gjkepa_contact_f32);
    for (int i = 0; i < gkev::kClasses; ++i) counts[i] = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int kd = gkev::event_kind(cast[k].status, cast[k].flags);
        kind[k] = (int8_t)kd;
        key[k] = gkev::event_key(kd, cast[k].toi);
        const int cls = gkev::event_class(kd);
        if (cls >= 0) counts[cls] += 1;
        if (kd > 0)
            out[k] = gkev::event_fill(kd, cast[k], records ? (const char*)records + (size_t)k * rec : nullptr, records_precision,
                                      pairs[2 * k], pairs[2 * k + 1], (int32_t)k);
        else
            std::memset(&out[k], 0, sizeof out[k]);
    }
    return 0;
}

#ifdef EVENTS_HOST_MAIN
// Seeded records of every status / flag combination and the special values of toi, with F64, F32 and no contact
// records, for a stand-alone run under -fsanitize=address,undefined.  Prints the counts.
#include <cmath>
#include <cstdio>
#include <vector>
int main() {
    const int64_t n = 4096;
    const double tois[] = {0.25, 0.0, -0.0, 5e-324, NAN, -1.0, INFINITY, 1.0};
    std::vector<int32_t> pairs(2 * n);
    std::vector<gjkepa_cast_f64> cast(n);
    std::vector<gjkepa_contact_f64> r64(n);
    std::vector<gjkepa_contact_f32> r32(n);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int64_t k = 0; k < n; ++k) {
        std::memset(&cast[k], 0, sizeof cast[k]);
        std::memset(&r64[k], 0, sizeof r64[k]);
        std::memset(&r32[k], 0, sizeof r32[k]);
        pairs[2 * k] = (int32_t)(next() % 1000);
        pairs[2 * k + 1] = (int32_t)(next() % 1000);
        cast[k].status = (int8_t)(next() % 8);
        cast[k].flags = (int8_t)(next() % 8);
        cast[k].toi = tois[next() % 8];
        for (int i = 0; i < 3; ++i) {
            cast[k].point_a[i] = (double)(next() % 1000) / 7.0;
            cast[k].point_b[i] = (double)(next() % 1000) / 11.0;
            cast[k].normal[i] = (double)(next() % 1000) / 13.0;
            r64[k].collision_normal[i] = (double)(next() % 1000) / 17.0;
            r32[k].collision_normal[i] = (float)(next() % 1000) / 19.0f;
        }
        for (int i = 0; i < 6; ++i) {
            r64[k].nearest_points[i] = (double)(next() % 1000) / 23.0;
            r32[k].nearest_points[i] = (float)(next() % 1000) / 29.0f;
        }
        r64[k].penetration_depth = 0.5;
        r32[k].penetration_depth = 0.25f;
    }
    std::vector<int8_t> kind(n);
    std::vector<uint64_t> key(n);
    std::vector<gjkepa_event_f64> out(n);
    int64_t counts[5];
    const void* recs[3] = {nullptr, r64.data(), r32.data()};
    const int precs[3] = {GJKEPA_PREC_F64, GJKEPA_PREC_F64, GJKEPA_PREC_F32};
    for (int v = 0; v < 3; ++v) {
        if (events_host(pairs.data(), n, cast.data(), recs[v], precs[v], kind.data(), key.data(), out.data(), counts)) return 1;
        int64_t with_key = 0;
        for (int64_t k = 0; k < n; ++k) with_key += key[k] != gkev::kNoKey;
        if (with_key != counts[0] + counts[1] + counts[2] + counts[3]) return 2;
        std::printf("records %d: HIT %lld START %lld IMPACT %lld UNDECIDED %lld BAD %lld\n", v, (long long)counts[0],
                    (long long)counts[1], (long long)counts[2], (long long)counts[3], (long long)counts[4]);
    }
    std::printf("events_host clean\n");
    return 0;
}
#endif
