// manifold_clip.h — the contact manifold of gjkepa_manifold_batch(_device): steps 3 to 8 of the
// definition in include/gjkepa.h (plane frame, footprints, candidates, the reduction to at most four
// points, lifting and codes) for one pair whose two features are already chosen.
//
// Host and device code like dist_simplex.h (plain fp64, no FMA contraction in either build; sqrt and
// the divisions are correctly rounded on both sides): the manifold kernel (gjkepa_kernel.hip, part 14:
// one group of lanes per pair, every lane of the group holding the same values) and
// tests/manifold_host.cpp run this text and give the same bytes.  The caller supplies the vertices and
// the small index lists through one accessor object M:
//   D3   M.vert(h, i)         vertex i of hull h (0: A, 1: B) as doubles
//   int  M.feat(h, k)         k-th vertex index of hull h's (decimated) feature, ascending
//   int  M.foot(h, k) / void M.set_foot(h, k, i)    hull h's footprint, written here: at most
//                             kMaxFeature indices per hull
//   double M.sqrt(x)
// The footprints are kept as vertex indices and their 2-D coordinates recomputed from the hull at every
// use, and the candidates are enumerated once per reduction pass instead of being stored, so a pair
// needs 2 x 2 x kMaxFeature small indices of memory and nothing else.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MC_HD inline __attribute__((always_inline))
#endif

namespace gkm {

constexpr int kMaxFeature = 32;          // GJKEPA_MANIFOLD_MAX_FEATURE: feature vertices kept per hull
constexpr double kTol = 1.0e-9;          // every geometric tolerance, relative to the scale s (s^2 for areas)
constexpr uint32_t kNoCode = 0xFFFFFFFFu;
constexpr uint32_t kNoVert = 0xFFFFu;    // the absent half of a vertex candidate's code
// record flags (include/gjkepa.h GJKEPA_MANIFOLD_*)
constexpr int kFlagNoHit = 1, kFlagDecimated = 2, kFlagFallback = 4;

struct D3 { double x, y, z; };
struct D2 { double x, y; };
MC_HD D3 mk(double x, double y, double z) { D3 r; r.x = x; r.y = y; r.z = z; return r; }
MC_HD D2 mk2(double x, double y) { D2 r; r.x = x; r.y = y; return r; }
MC_HD D3 sub(D3 a, D3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
MC_HD D2 sub2(D2 a, D2 b) { return mk2(a.x - b.x, a.y - b.y); }
MC_HD double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
MC_HD double dot2(D2 a, D2 b) { return a.x * b.x + a.y * b.y; }
MC_HD double cross2(D2 a, D2 b) { return a.x * b.y - a.y * b.x; }
MC_HD D3 cross(D3 a, D3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
MC_HD double abs_(double x) { return x < 0.0 ? -x : x; }

// Decimation of a feature of m vertices (ranks 0 .. m - 1 in index order): the vertices of rank r with
// r % step == 0 are kept, at position r / step; ceil(m / step) <= kMaxFeature of them.
MC_HD int decimation_step(int m) { return m > kMaxFeature ? (m + kMaxFeature - 1) / kMaxFeature : 1; }
MC_HD int decimated_count(int m) { const int st = decimation_step(m); return (m + st - 1) / st; }

// step 3: u, w span the contact plane; (u, w, n) is right-handed, so counter-clockwise in (x, y) is
// counter-clockwise seen from +n.  o = a[FA[0]].
struct Frame {
    D3 n, u, w, o;
};
template <typename M> MC_HD Frame make_frame(const M& m, D3 n) {
    Frame f;
    f.n = n;
    const double ax = abs_(n.x), ay = abs_(n.y), az = abs_(n.z);
    D3 e = mk(1.0, 0.0, 0.0);             // the axis of the smallest |component|, the first of equals
    double least = ax;
    if (ay < least) { e = mk(0.0, 1.0, 0.0); least = ay; }
    if (az < least) e = mk(0.0, 0.0, 1.0);
    const D3 c = cross(e, n);
    const double len = m.sqrt(dot(c, c));
    f.u = mk(c.x / len, c.y / len, c.z / len);
    f.w = cross(n, f.u);
    f.o = m.vert(0, m.feat(0, 0));
    return f;
}
MC_HD D2 to_plane(const Frame& f, D3 p) {
    const D3 d = sub(p, f.o);
    return mk2(dot(d, f.u), dot(d, f.w));
}
template <typename M> MC_HD D2 feat_pt(const M& m, const Frame& f, int h, int k) { return to_plane(f, m.vert(h, m.feat(h, k))); }
template <typename M> MC_HD D2 foot_pt(const M& m, const Frame& f, int h, int k) { return to_plane(f, m.vert(h, m.foot(h, k))); }

// step 4: hull h's footprint by gift wrapping over its feature of cnt vertices, counter-clockwise from
// the lexicographically smallest (x, y, position); a point to the right of the current edge replaces
// its end, and of collinear points the farthest stays.  Returns the footprint's size: 1 a point, 2 a
// segment, >= 3 a polygon.
template <typename M> MC_HD int wrap_footprint(M& m, const Frame& f, int h, int cnt) {
    int start = 0;
    D2 ps = feat_pt(m, f, h, 0);
    for (int k = 1; k < cnt; ++k) {
        const D2 p = feat_pt(m, f, h, k);
        if (p.x < ps.x || (p.x == ps.x && p.y < ps.y)) { start = k; ps = p; }
    }
    int cur = start, nf = 0;
    D2 pc = ps;
    for (;;) {
        m.set_foot(h, nf, m.feat(h, cur));
        ++nf;
        int nxt = -1;
        D2 dn = mk2(0.0, 0.0);
        double ln = 0.0;
        for (int k = 0; k < cnt; ++k) {
            const D2 d = sub2(feat_pt(m, f, h, k), pc);
            if (d.x == 0.0 && d.y == 0.0) continue;            // the current point, or a copy of it
            const double l = dot2(d, d);
            if (nxt < 0) { nxt = k; dn = d; ln = l; continue; }
            const double cr = cross2(dn, d);
            if (cr < 0.0 || (cr == 0.0 && l > ln)) { nxt = k; dn = d; ln = l; }
        }
        if (nxt < 0 || nxt == start || nf >= cnt || nf >= kMaxFeature) break;
        const D2 pn = feat_pt(m, f, h, nxt);
        if (pn.x == ps.x && pn.y == ps.y) break;               // back at a copy of the start
        cur = nxt;
        pc = pn;
    }
    return nf;
}

// number of edges of a footprint of nf vertices: a polygon's nf, a segment's one, a point's none
MC_HD int edge_count(int nf) { return nf >= 3 ? nf : nf == 2 ? 1 : 0; }

// step 5: is p no more than tol outside the footprint of hull h (nf vertices)?
template <typename M> MC_HD bool inside_footprint(const M& m, const Frame& f, int h, int nf, D2 p, double tol) {
    if (nf == 1) {
        const D2 d = sub2(p, foot_pt(m, f, h, 0));
        return m.sqrt(dot2(d, d)) <= tol;
    }
    if (nf == 2) {          // a segment: across its line and along its length
        const D2 b0 = foot_pt(m, f, h, 0);
        const D2 e = sub2(foot_pt(m, f, h, 1), b0), d = sub2(p, b0);
        const double le = m.sqrt(dot2(e, e));
        const double cr = cross2(e, d), al = dot2(e, d);
        return abs_(cr) <= tol * le && al >= -(tol * le) && al - le * le <= tol * le;
    }
    D2 b0 = foot_pt(m, f, h, nf - 1);
    for (int k = 0; k < nf; ++k) {
        const D2 b1 = foot_pt(m, f, h, k);
        const D2 e = sub2(b1, b0);
        if (cross2(e, sub2(p, b0)) < -(tol * m.sqrt(dot2(e, e)))) return false;
        b0 = b1;
    }
    return true;
}

// The candidates in their order: A's footprint vertices inside B's footprint, B's inside A's, then the
// proper crossings (A's edges in order, B's edges in order within each).  v(point, code) sees each.
template <typename M, typename V>
MC_HD void for_each_candidate(const M& m, const Frame& f, int nfa, int nfb, double s, V&& v) {
    const double tol = kTol * s;
    for (int k = 0; k < nfa; ++k) {
        const D2 p = foot_pt(m, f, 0, k);
        if (inside_footprint(m, f, 1, nfb, p, tol)) v(p, (uint32_t)m.foot(0, k) | (kNoVert << 16));
    }
    for (int k = 0; k < nfb; ++k) {
        const D2 p = foot_pt(m, f, 1, k);
        if (inside_footprint(m, f, 0, nfa, p, tol)) v(p, kNoVert | ((uint32_t)m.foot(1, k) << 16));
    }
    const int ea = edge_count(nfa), eb = edge_count(nfb);
    for (int i = 0; i < ea; ++i) {
        const D2 a0 = foot_pt(m, f, 0, i);
        const D2 r = sub2(foot_pt(m, f, 0, i + 1 < nfa ? i + 1 : 0), a0);
        const double lr = m.sqrt(dot2(r, r));
        for (int j = 0; j < eb; ++j) {
            const D2 b0 = foot_pt(m, f, 1, j);
            const D2 q = sub2(foot_pt(m, f, 1, j + 1 < nfb ? j + 1 : 0), b0);
            const double den = cross2(r, q);
            if (abs_(den) <= kTol * (lr * m.sqrt(dot2(q, q)))) continue;       // parallel
            const D2 d = sub2(b0, a0);
            const double t = cross2(d, q) / den, t2 = cross2(d, r) / den;
            if (t > 0.0 && t < 1.0 && t2 > 0.0 && t2 < 1.0)
                v(mk2(a0.x + t * r.x, a0.y + t * r.y), (uint32_t)m.foot(0, i) | ((uint32_t)m.foot(1, j) << 16));
        }
    }
}

// what steps 3 to 8 leave: the record's points, codes, count, area and flag bits
struct Patch {
    D3 pt[4];
    uint32_t code[4];
    int n;
    double area;
    int flags;
};

// a point of the contact plane lifted onto A's support plane n.x = hA
MC_HD D3 lift(D3 p, D3 n, double hA) {
    const double t = (hA - dot(n, p)) / dot(n, n);
    return mk(p.x + t * n.x, p.y + t * n.y, p.z + t * n.z);
}
MC_HD D3 from_plane(const Frame& f, D2 p, double hA) {
    const D3 q = mk(f.o.x + (p.x * f.u.x + p.y * f.w.x), f.o.y + (p.x * f.u.y + p.y * f.w.y), f.o.z + (p.x * f.u.z + p.y * f.w.z));
    return lift(q, f.n, hA);
}

// Steps 3 to 8.  n: the contact record's normal; hA: hull A's support height along it; ma, mb: the
// (decimated) features' sizes, 1 .. kMaxFeature each; cp: the contact record's collision_point, for the
// fallback.
template <typename M> MC_HD Patch clip_manifold(M& m, D3 n, double hA, int ma, int mb, D3 cp) {
    Patch out;
#pragma unroll
    for (int k = 0; k < 4; ++k) { out.pt[k] = mk(0.0, 0.0, 0.0); out.code[k] = kNoCode; }
    out.n = 0;
    out.area = 0.0;
    out.flags = 0;
    const Frame f = make_frame(m, n);
    double s = 0.0;
    for (int k = 0; k < ma; ++k) {
        const D2 p = feat_pt(m, f, 0, k);
        const double a = abs_(p.x) > abs_(p.y) ? abs_(p.x) : abs_(p.y);
        if (a > s) s = a;
    }
    for (int k = 0; k < mb; ++k) {
        const D2 p = feat_pt(m, f, 1, k);
        const double a = abs_(p.x) > abs_(p.y) ? abs_(p.x) : abs_(p.y);
        if (a > s) s = a;
    }
    const int nfa = wrap_footprint(m, f, 0, ma), nfb = wrap_footprint(m, f, 1, mb);
    // p0: the lexicographically smallest candidate (the first of equals)
    bool any = false;
    D2 p0 = mk2(0.0, 0.0);
    uint32_t c0 = kNoCode;
    for_each_candidate(m, f, nfa, nfb, s, [&](D2 p, uint32_t code) {
        if (!any || p.x < p0.x || (p.x == p0.x && p.y < p0.y)) { p0 = p; c0 = code; }
        any = true;
    });
    if (!any) {
        out.pt[0] = lift(cp, n, hA);
        out.n = 1;
        out.flags = kFlagFallback;
        return out;
    }
    // p1: the candidate farthest from p0
    D2 p1 = p0;
    uint32_t c1 = kNoCode;
    double far2 = 0.0;
    for_each_candidate(m, f, nfa, nfb, s, [&](D2 p, uint32_t code) {
        const D2 d = sub2(p, p0);
        const double l = dot2(d, d);
        if (l > far2) { far2 = l; p1 = p; c1 = code; }
    });
    out.pt[0] = from_plane(f, p0, hA);
    out.code[0] = c0;
    out.n = 1;
    if (!(m.sqrt(far2) > kTol * s)) return out;
    // pL, pR: the largest triangle (p0, p1, candidate) on either side of p0 -> p1
    const D2 e = sub2(p1, p0);
    D2 pl = p0, pr = p0;
    uint32_t cl = kNoCode, cr = kNoCode;
    double al = 0.0, ar = 0.0;
    for_each_candidate(m, f, nfa, nfb, s, [&](D2 p, uint32_t code) {
        const double a = 0.5 * cross2(e, sub2(p, p0));
        if (a > al) { al = a; pl = p; cl = code; }
        if (a < ar) { ar = a; pr = p; cr = code; }
    });
    const double amin = kTol * (s * s);
    const bool hasl = al > amin, hasr = -ar > amin;
    // counter-clockwise: p0, pR, p1, pL (no indexed stores: the slots are chosen by selects)
    const D3 x1 = from_plane(f, p1, hA);
    if (hasr) {
        out.pt[1] = from_plane(f, pr, hA); out.code[1] = cr;
        out.pt[2] = x1; out.code[2] = c1;
        if (hasl) {
            out.pt[3] = from_plane(f, pl, hA); out.code[3] = cl;
            out.n = 4;
            out.area = 0.5 * (((cross2(p0, pr) + cross2(pr, p1)) + cross2(p1, pl)) + cross2(pl, p0));
        } else {
            out.n = 3;
            out.area = 0.5 * ((cross2(p0, pr) + cross2(pr, p1)) + cross2(p1, p0));
        }
    } else {
        out.pt[1] = x1; out.code[1] = c1;
        if (hasl) {
            out.pt[2] = from_plane(f, pl, hA); out.code[2] = cl;
            out.n = 3;
            out.area = 0.5 * ((cross2(p0, p1) + cross2(p1, pl)) + cross2(pl, p0));
        } else {
            out.n = 2;
        }
    }
    return out;
}

}  // namespace gkm
