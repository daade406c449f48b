// event_record.h — the event of a pair of a moving step (include/gjkepa.h gjkepa_events_device, DESIGN.md
// §19): which kind of event a cast record stands for, at what time, and the 128-byte record it becomes.
//
// The kind comes from the cast record's status and flags alone; the first rule that applies wins:
//     status BAD_INPUT -> no event (BAD);  flag SKIPPED -> HIT;  status CAST_MAXITER -> UNDECIDED;
//     flag START -> START;  flag IMPACT -> IMPACT;  otherwise (a MISS) no event.
// time is 0 for HIT / START and toi for IMPACT / UNDECIDED, where a toi that is not > 0 (-0, 0, negative,
// NaN) gives +0.0: the bits of a time, read as uint64, order like the value, so they are the sort key.
// START, IMPACT and UNDECIDED take point_a, point_b and normal from the cast record bit for bit; HIT takes
// the contact record's two nearest_points, its collision_normal, its penetration_depth and its status (an F32
// record's widened), or zeros without contact records.
//
// Host and device code like swept_sphere.h and manifold_clip.h: events_kernel.hip runs this text,
// tests/events_host.cpp runs it on the host, and tests/events_ref.py restates it in numpy with the same bits.
#pragma once
#include <cstdint>

#include "../../include/gjkepa.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EV_HD inline __attribute__((always_inline))
#endif

namespace gkev {

constexpr int kNone = 0;            // a MISS: no event
constexpr int kBad = -1;            // BAD_INPUT: no event, counted
constexpr int kClasses = 5;         // counts: HIT, START, IMPACT, UNDECIDED, BAD
constexpr uint64_t kNoKey = ~0ull;  // the sort key of a pair without an event: behind every time

// kind of a pair: GJKEPA_EVENT_*, kNone or kBad
EV_HD int event_kind(int status, int flags) {
    if (status == GJKEPA_STATUS_BAD_INPUT) return kBad;
    if (flags & GJKEPA_CAST_SKIPPED) return GJKEPA_EVENT_HIT;
    if (status == GJKEPA_STATUS_CAST_MAXITER) return GJKEPA_EVENT_UNDECIDED;
    if (flags & GJKEPA_CAST_START) return GJKEPA_EVENT_START;
    if (flags & GJKEPA_CAST_IMPACT) return GJKEPA_EVENT_IMPACT;
    return kNone;
}

// slot of a kind in counts[5], -1 for kNone
EV_HD int event_class(int kind) { return kind == kBad ? 4 : kind - 1; }

// IMPACT and UNDECIDED stop a body; contact at t = 0 does not
EV_HD bool event_clamps(int kind) { return kind == GJKEPA_EVENT_IMPACT || kind == GJKEPA_EVENT_UNDECIDED; }

EV_HD double event_time(int kind, double toi) {
    if (!event_clamps(kind)) return 0.0;
    return toi > 0.0 ? toi : 0.0;        // false for NaN
}

EV_HD uint64_t time_bits(double t) {
    uint64_t u;
    __builtin_memcpy(&u, &t, 8);
    return u;
}

// the sort key of a pair: its event's time bits, or kNoKey
EV_HD uint64_t event_key(int kind, double toi) { return kind > 0 ? time_bits(event_time(kind, toi)) : kNoKey; }

// the record of pair `pair` = (a, b), kind > 0.  contact: the pair's contact record of contact_precision, or
// nullptr.
EV_HD gjkepa_event_f64 event_fill(int kind, const gjkepa_cast_f64& c, const void* contact, int contact_precision,
                                  int32_t a, int32_t b, int32_t pair) {
    gjkepa_event_f64 e;
    e.time = event_time(kind, c.toi);
    e.depth = 0.0;
    e.status = c.status;
    if (kind != GJKEPA_EVENT_HIT) {
        for (int k = 0; k < 3; ++k) { e.point_a[k] = c.point_a[k]; e.point_b[k] = c.point_b[k]; e.normal[k] = c.normal[k]; }
    } else if (!contact) {
        for (int k = 0; k < 3; ++k) e.point_a[k] = e.point_b[k] = e.normal[k] = 0.0;
        e.status = 0;
    } else if (contact_precision == GJKEPA_PREC_F64) {
        const gjkepa_contact_f64& r = *(const gjkepa_contact_f64*)contact;
        for (int k = 0; k < 3; ++k) { e.point_a[k] = r.nearest_points[k]; e.point_b[k] = r.nearest_points[3 + k]; e.normal[k] = r.collision_normal[k]; }
        e.depth = r.penetration_depth;
        e.status = r.status;
    } else {
        const gjkepa_contact_f32& r = *(const gjkepa_contact_f32*)contact;
        for (int k = 0; k < 3; ++k) {
            e.point_a[k] = (double)r.nearest_points[k];
            e.point_b[k] = (double)r.nearest_points[3 + k];
            e.normal[k] = (double)r.collision_normal[k];
        }
        e.depth = (double)r.penetration_depth;
        e.status = r.status;
    }
    e.a = a;
    e.b = b;
    e.pair = pair;
    e.kind = (int8_t)kind;
    e.reserved[0] = e.reserved[1] = 0;
    for (int k = 0; k < 6; ++k) e.pad[k] = 0u;
    return e;
}

}  // namespace gkev
