// hit_list.h -- the list of rt_trace_hits (include/rt_abi.h): the K smallest accepted distances of one ray, in order,
// one definition for the kernel (rt_hits.hip) and for the host hook rt_hit_list_host (host_hooks.hip).
//
// An entry is two words: the distance t and a payload p -- a record index of the mirror's `tris` (mirror.h), or
// SPHERE | sphere index.  The list is a pair of arrays of CAP >= K slots that is only ever indexed by constants of
// fully unrolled loops, so on the device every slot is a register and no private array is left to land in scratch.
// A list of K < CAP entries sits in the LAST K slots: the slots before them hold t = -inf, which nothing is ever
// placed in front of, so they never move; an unfilled slot holds t = tmax and p = EMPTY.  The K-th smallest accepted
// distance once K are held, and tmax before that -- rt_abi.h's bound() -- is therefore always the last slot's t, a
// register with a fixed name, whatever K is.
//
// offer() is rt_abi.h's rule: nothing for a NaN, a t < 0 or !(t < bound()); otherwise the entry goes in before the
// first entry whose t is strictly greater -- an equal t goes behind the ones already there, arrival order breaks
// ties -- and the list is cut to K.  One extension serves a walk that visits a leaf's triangles out of leaf order
// (rt_hits.hip, leaf trees): with `leaf_end` = the record index one past the leaf being walked, an entry with an equal
// t whose record lies in (p, leaf_end) also counts as greater.  Such an entry is a later triangle of the same leaf
// (leaves are disjoint runs of records, and p lies in this one).  Candidates of one leaf are then ordered by (t,
// position in the leaf), which is the order the sequential loop leaves them in, whatever order they are offered in;
// leaf_end = 0 is the plain arrival rule.
#pragma once

#include <cmath>
#include <cstdint>

#include "rt_math.h"

namespace rth {

constexpr uint32_t EMPTY = 0xffffffffu;   // payload of a slot that holds no hit
constexpr uint32_t SPHERE = 0x80000000u;  // payload flag: the low bits are a sphere index, not a `tris` record
constexpr int MAX_HITS = 16;              // RT_HITS_MAX

template <int CAP>
struct List {
    float t[CAP];
    uint32_t p[CAP];
    float tmax;      // the ray's tmax: the bound throughout under COUNT_ALL
    uint32_t total;  // offers accepted (under COUNT_ALL: every hit in [0, tmax) of the nodes visited)
};

template <int CAP>
RT_HD void init(List<CAP>& L, int k, float tmax) {
#pragma unroll
    for (int s = 0; s < CAP; s++) {
        L.t[s] = s < CAP - k ? -INFINITY : tmax;
        L.p[s] = EMPTY;
    }
    L.tmax = tmax;
    L.total = 0;
}

// rt_abi.h's bound(): what a distance must lie below to be accepted, and what the slab test culls against.
template <int CAP>
RT_HD float bound(const List<CAP>& L, bool count_all) {
    return count_all ? L.tmax : L.t[CAP - 1];
}

// Whether entry (et, ep) stays behind a new (t, p): strictly greater, or -- inside the leaf that ends at leaf_end --
// equal and later in the leaf.  An EMPTY or SPHERE payload is never below leaf_end (<= 2^31).
RT_HD bool behind(float et, uint32_t ep, float t, uint32_t p, uint32_t leaf_end) {
    return (et > t) | ((et == t) & (ep > p) & (ep < leaf_end));
}

template <int CAP>
RT_HD void offer(List<CAP>& L, bool count_all, float t, uint32_t p, uint32_t leaf_end = 0) {
    if (!(t >= 0.0f)) return;  // a NaN, or t < 0
    // t < bound(), or the bound's own distance ahead of the same leaf's last entry
    const bool fits = behind(L.t[CAP - 1], L.p[CAP - 1], t, p, leaf_end);
    if (count_all ? !(t < L.tmax) : !fits) return;
    L.total++;
    if (!fits) return;  // COUNT_ALL: counted, but beyond the K kept
    bool b[CAP];
#pragma unroll
    for (int s = 0; s < CAP; s++) b[s] = behind(L.t[s], L.p[s], t, p, leaf_end);
    // the list is sorted, so b is false ... false true ... true: the entries behind move up one slot (the last falls
    // off), the new one takes the first slot of theirs
#pragma unroll
    for (int s = CAP - 1; s > 0; s--) {
        L.t[s] = b[s - 1] ? L.t[s - 1] : (b[s] ? t : L.t[s]);
        L.p[s] = b[s - 1] ? L.p[s - 1] : (b[s] ? p : L.p[s]);
    }
    L.t[0] = b[0] ? t : L.t[0];
    L.p[0] = b[0] ? p : L.p[0];
}

// The first slot's entry, the others moved down one: a loop that takes the slots in turn needs no runtime index.
template <int CAP>
RT_HD void rotate(List<CAP>& L, float* t, uint32_t* p) {
    *t = L.t[0], *p = L.p[0];
#pragma unroll
    for (int s = 0; s + 1 < CAP; s++) L.t[s] = L.t[s + 1], L.p[s] = L.p[s + 1];
    L.t[CAP - 1] = 0.0f, L.p[CAP - 1] = EMPTY;
}

}  // namespace rth
