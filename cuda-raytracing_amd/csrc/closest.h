// closest.h -- the arithmetic of rt_closest_point (include/rt_abi.h spells it out operation by operation), one
// definition for the kernel (rt_closest.hip) and for the brute-force host call (closest_host.cpp): the nearest point
// of a sphere and of a triangle record (a, ab, ac) to a point, the (d2, kind, id) order of candidates, and the
// lower bound on a box's candidates that lets the kernel skip a subtree.  fp32, no contraction (build.py FP_FLAGS),
// only + - * /, sqrt and comparisons; selects instead of fmin / fmax, so that a NaN stays a NaN.
#pragma once

#include "rt_math.h"

namespace rtc {

using rtm::f3;

struct Candidate {
    float d2;  // computed squared distance (may be NaN: never accepted)
    f3 q;      // the nearest point
    uint32_t region;
};

// Sphere (c, rad): the point of the surface on the line from the centre through p (inside or outside alike).
RT_HD Candidate closest_on_sphere(f3 p, f3 c, float rad) {
    const f3 v = rtm::sub(p, c);
    const float len = sqrtf(rtm::dot(v, v));
    const float s = len - rad;
    const float dist = s < 0.0f ? -s : s;
    Candidate r;
    r.d2 = dist * dist;
    const float k = rad / len;
    r.q = len > 0.0f ? rtm::mk(c.x + v.x * k, c.y + v.y * k, c.z + v.z * k) : rtm::mk(c.x + rad, c.y + 0.0f, c.z + 0.0f);
    r.region = 0;
    return r;
}

RT_HD float ratio(float n, float d) { return d > 0.0f ? n / d : 0.0f; }

// Triangle a, a + ab, a + ac (the mirror's record: v0, e1, e2): the Voronoi regions of its vertices (1, 2, 3), edges
// (4: ab, 5: ac, 6: the opposite one) and interior (0), the first rule that holds.  Only the winning rule's quotients
// are formed (two divisions for the interior, one for an edge, none for a vertex), from that rule's own operands.
RT_HD Candidate closest_on_triangle(f3 p, f3 a, f3 ab, f3 ac) {
    const f3 ap = rtm::sub(p, a);
    const float d1 = rtm::dot(ab, ap), d2 = rtm::dot(ac, ap);
    const float aa = rtm::dot(ab, ab), bb = rtm::dot(ab, ac), cc = rtm::dot(ac, ac);
    const float d3 = d1 - aa, d4 = d2 - bb, d5 = d1 - bb, d6 = d2 - cc;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const bool r1 = d1 <= 0.0f && d2 <= 0.0f;
    const bool r2 = d3 >= 0.0f && d4 <= d3;
    const bool r3 = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool r4 = d6 >= 0.0f && d5 <= d6;
    const bool r5 = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool r6 = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
    const uint32_t region = r1 ? 1u : r2 ? 2u : r3 ? 4u : r4 ? 3u : r5 ? 5u : r6 ? 6u : 0u;
    const float den = (va + vb) + vc;
    // quotient A: rule 3's v or rule 7's; quotient B: the w of rule 5, 6 or 7; a vertex region divides nothing
    float qa = 0.0f, qb = 0.0f;
    if (region == 4u) qa = ratio(d1, d1 - d3);
    if (region == 5u) qb = ratio(d2, d2 - d6);
    if (region == 6u) qb = ratio(e43, e43 + e56);
    if (region == 0u) qa = ratio(vb, den), qb = ratio(vc, den);
    float v = qa, w = qb;  // rule 7, clamped by selects
    v = v < 0.0f ? 0.0f : v;
    v = v > 1.0f ? 1.0f : v;
    w = w < 0.0f ? 0.0f : w;
    const float rest = 1.0f - v;
    w = w > rest ? rest : w;
    if (region == 1u) v = 0.0f, w = 0.0f;
    if (region == 2u) v = 1.0f, w = 0.0f;
    if (region == 4u) v = qa, w = 0.0f;
    if (region == 3u) v = 0.0f, w = 1.0f;
    if (region == 5u) v = 0.0f, w = qb;
    if (region == 6u) w = qb, v = 1.0f - qb;
    Candidate r;
    r.q = rtm::mk((a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w);
    const f3 e = rtm::sub(p, r.q);
    r.d2 = rtm::dot(e, e);
    r.region = region;
    return r;
}

// The running answer of one point: the lexicographic minimum of (d2, kind, id) over the candidates with d2 <= r2.
// It starts as (r2, nothing); kind 0 = nothing accepted yet.
struct Best {
    float d2;
    uint32_t kind, id, region;
    f3 q;
};
RT_HD Best best_start(float r2) { return Best{r2, 0u, 0u, 0u, rtm::mk(0.0f, 0.0f, 0.0f)}; }
// kind 1 (spheres) before kind 2 (faces), lower ids first; a NaN d2 fails both comparisons
RT_HD void offer(Best& b, const Candidate& c, uint32_t kind, uint32_t id) {
    const bool tie = c.d2 == b.d2 && (b.kind == 0u || kind < b.kind || (kind == b.kind && id < b.id));
    if (c.d2 < b.d2 || tie) b.d2 = c.d2, b.kind = kind, b.id = id, b.region = c.region, b.q = c.q;
}

// ---------------------------------------------------------------------------------------------------------------
// The cull.  box_bound(p, lo, hi) is a float L such that EVERY face whose three vertices lie in the box [lo, hi] has
// a computed d2 >= L, computed as closest_on_triangle computes it; a subtree under that box is skipped only when
// L > best.d2 -- strictly, so a face that would tie the best (and win by its lower id) is never skipped -- and since
// `offer` accepts nothing above best.d2, and best.d2 only falls, skipping changes no answer.  -1 = no bound.
//
// Premises (the caller's gate, else it does not cull): p and the box are finite, |p|_inf <= 2^60 and |box|_inf <=
// 2^63 (the mirror's `fast` flag bounds every node by 2^62).  With M = max(|p|_inf, |box|_inf), the function itself
// refuses M < 2^-60.  U = 2^-24.
//
// 1. Where the computed q lies.  a = v0 is in the box.  ab = RN(v1 - v0), so |ab_k| <= 2M (1 + U) and a + ab is within
//    2^-23 M of v1, hence of the box, on every axis; ac alike.  (A leaf tree's box holds a + ab and a + ac
//    themselves, rounded outward: leaftree.cpp.)  In every rule v and w are NaN -- then q and d2 are NaN and the face
//    is never accepted, so skipping it is harmless -- or 0 <= v, w <= 1 with v + w <= 1 + U: rule 7's w is cut at
//    RN(1 - v), rule 6's v is RN(1 - w), rules 3, 5, 6 divide a non-negative n by a d >= n.  So the real point
//    a + ab v + ac w is a convex combination of a, a + ab, a + ac up to U |ac| <= 2^-22.9 M: within 2^-21 M of the
//    box.  The four roundings of (a + ab v) + ac w add at most U (2 + 3 + 2 + 5.1) M (1 + 2^-20) + 2^-149 (the two
//    products may underflow) < 2^-20 M, M >= 2^-60.  Together: the computed q is within D = 2^-19 M of the box, on
//    every axis.
// 2. The axis gap.  g = max(RN(lo - p), RN(p - hi)) overstates the real gap by at most one rounding of a value
//    <= 2M: 2^-23 M.  G = RN(g - 2^-18 M) -- the slack is exact, a power of two times M >= 2^-60 -- adds another
//    2^-22.9 M at most, so G <= gap - 2^-18 M + 2^-22 M <= gap - D.  Where G > 0 the gap is real and positive and
//    |p_k - q_k| >= gap - D >= G; where G <= 0 it is taken as 0.
// 3. No factor on the sum.  |p_k - q_k| >= G_k with G_k a float, and rounding to nearest is monotone and keeps a
//    float where it is: the computed e_k = RN(p_k - q_k) has |e_k| >= G_k.  Products and sums of non-negative
//    floats are monotone too, through underflow and overflow alike, so dot(e, e) >= dot(G, G) when both run the
//    same operations in the same order -- rtm::dot here and there.  Hence d2 >= L = dot(G, G): L carries no
//    relative slack, and a point straight above a flat box, where the gap IS the distance, gives L below d2 by the
//    axis slack and never above it (tests/closest_cases.py "above").
RT_HD float box_bound(f3 p, f3 lo, f3 hi) {
    const float pm = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z));
    const float bm = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(hi.x)), fmaxf(fabsf(lo.y), fabsf(hi.y))),
                           fmaxf(fabsf(lo.z), fabsf(hi.z)));
    const float m = fmaxf(pm, bm);
    const float slack = m * 0x1p-18f;
    const float ux = lo.x - p.x, wx = p.x - hi.x, uy = lo.y - p.y, wy = p.y - hi.y, uz = lo.z - p.z, wz = p.z - hi.z;
    const float gx = (ux > wx ? ux : wx) - slack, gy = (uy > wy ? uy : wy) - slack, gz = (uz > wz ? uz : wz) - slack;
    const f3 g = rtm::mk(gx > 0.0f ? gx : 0.0f, gy > 0.0f ? gy : 0.0f, gz > 0.0f ? gz : 0.0f);
    return m >= 0x1p-60f ? rtm::dot(g, g) : -1.0f;
}
// The lane's half of the gate: p finite and inside 2^60 (false for a NaN).
RT_HD bool point_in_cull_range(f3 p) {
    return fabsf(p.x) <= 0x1p60f && fabsf(p.y) <= 0x1p60f && fabsf(p.z) <= 0x1p60f;
}

}  // namespace rtc
