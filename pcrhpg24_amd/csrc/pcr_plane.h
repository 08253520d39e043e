// The host plans of the slab calls (pcr_plane_support, pcr_select_slabs; include/pcr_hip.h has the rules): the checks on a
// pcr_slab, its class against a batch's exact box, and per batch what is skipped, what the box alone decides and which slabs the
// kernel has to test. Plain C++ without a HIP dependency, so a host-only build can call it.
#pragma once
#include <cstdint>
#include <vector>

#include "pcr_types.h"

enum { SLAB_MISS = 0, SLAB_ALL = 1, SLAB_CUT = 2 };
enum { PLANE_SKIPPED = 0, PLANE_WHOLE = 1, PLANE_DECODED = 2 };
enum { SLABS_OUTSIDE = 0, SLABS_INSIDE = 1, SLABS_STRADDLING = 2 };

// nullptr, or what is wrong with the slab.
inline const char *slab_check(const pcr_slab &s)
{
    if (s.reserved != 0) return "pcr_slab::reserved is not 0";
    for (int a = 0; a < 3; ++a)
        if (s.n[a] > PCR_SLAB_MAX_NORMAL || s.n[a] < -PCR_SLAB_MAX_NORMAL) return "a normal component is beyond PCR_SLAB_MAX_NORMAL";
    if (s.lo > PCR_SLAB_MAX_BOUND || s.lo < -PCR_SLAB_MAX_BOUND || s.hi > PCR_SLAB_MAX_BOUND || s.hi < -PCR_SLAB_MAX_BOUND)
        return "a bound is beyond PCR_SLAB_MAX_BOUND";
    return nullptr;
}

// s(S, p): every product below 2^51, the sum below 2^53.
inline int64_t slab_form(const pcr_slab &s, int32_t x, int32_t y, int32_t z)
{
    return (int64_t)s.n[0] * x + (int64_t)s.n[1] * y + (int64_t)s.n[2] * z;
}

inline bool slab_in(const pcr_slab &s, int32_t x, int32_t y, int32_t z)
{
    const int64_t v = slab_form(s, x, y, z);
    return s.lo <= v && v <= s.hi;
}

// The class of a checked slab against the exact box bb = min x, y, z, max x, y, z.
inline int slab_class(const pcr_slab &s, const int32_t bb[6])
{
    if (s.lo > s.hi) return SLAB_MISS;
    int64_t smin = 0, smax = 0;
    for (int a = 0; a < 3; ++a) {
        const int64_t u = (int64_t)s.n[a] * bb[a], v = (int64_t)s.n[a] * bb[3 + a];
        smin += u < v ? u : v;
        smax += u < v ? v : u;
    }
    if (smax < s.lo || smin > s.hi) return SLAB_MISS;
    return s.lo <= smin && smax <= s.hi ? SLAB_ALL : SLAB_CUT;
}

inline bool plane_box_empty(const pcr_box &q) { return q.min[0] > q.max[0] || q.min[1] > q.max[1] || q.min[2] > q.max[2]; }

// clip (nullptr: everything) against the box: *within = the box lies inside it; returns false if they are disjoint.
inline bool plane_clip_meets(const pcr_box *clip, const int32_t bb[6], bool *within)
{
    *within = true;
    if (!clip) return true;
    if (plane_box_empty(*clip)) return false;
    for (int k = 0; k < 3; ++k) {
        if (bb[3 + k] < clip->min[k] || bb[k] > clip->max[k]) return false;
        *within = *within && bb[k] >= clip->min[k] && bb[3 + k] <= clip->max[k];
    }
    return true;
}

// pcr_plane_support's plan of one batch. PLANE_SKIPPED: no candidate, nothing appended. Otherwise `all` receives the indices of
// the hypotheses of class ALL, which count every candidate of the batch: 65 536 if *open, else what the kernel reports.
// PLANE_DECODED: the batch's exclusion slice (the CUT exclusions) is appended to `excl`, its hypothesis slice (the CUT hypotheses,
// each with its index in `reserved`) to `cut`. PLANE_WHOLE: neither list grows.
inline int plane_plan_batch(const pcr_slab *hyp, int num_hyp, const pcr_box *clip, const pcr_slab *exclude, int num_exclude, const int32_t bb[6],
                            std::vector<pcr_slab> &excl, std::vector<pcr_slab> &cut, std::vector<int32_t> &all, bool *open)
{
    bool within = true;
    *open = false;
    if (!plane_clip_meets(clip, bb, &within)) return PLANE_SKIPPED;
    const size_t e0 = excl.size(), c0 = cut.size();
    for (int k = 0; k < num_exclude; ++k) {
        const int cls = slab_class(exclude[k], bb);
        if (cls == SLAB_ALL) { excl.resize(e0); return PLANE_SKIPPED; }
        if (cls == SLAB_CUT) excl.push_back(exclude[k]);
    }
    *open = within && excl.size() == e0;
    for (int j = 0; j < num_hyp; ++j) {
        const int cls = slab_class(hyp[j], bb);
        if (cls == SLAB_ALL) all.push_back(j);
        else if (cls == SLAB_CUT) { cut.push_back(hyp[j]); cut.back().reserved = j; }
    }
    if (cut.size() > c0 || (!*open && !all.empty())) return PLANE_DECODED;
    excl.resize(e0);
    return PLANE_WHOLE;
}

// pcr_select_slabs' plan of one batch. SLABS_STRADDLING: the slabs a point of the batch has to be tested against (the CUT ones)
// are appended to `list`, and *invert tells whether "in all of them" selects (0) or rejects (1) a point inside the clip. An
// inverted call with a slab that misses the box selects every point of the box inside the clip: an empty list with *invert = 0.
inline int slabs_plan_batch(const pcr_slab *slabs, int num_slabs, const pcr_box *clip, uint32_t invert_call, const int32_t bb[6],
                            std::vector<pcr_slab> &list, uint32_t *invert)
{
    bool within = true;
    *invert = invert_call ? 1u : 0u;
    if (!plane_clip_meets(clip, bb, &within)) return SLABS_OUTSIDE;
    const size_t l0 = list.size();
    bool miss = false;
    for (int k = 0; k < num_slabs; ++k) {
        const int cls = slab_class(slabs[k], bb);
        if (cls == SLAB_MISS) { miss = true; break; }
        if (cls == SLAB_CUT) list.push_back(slabs[k]);
    }
    if (miss) {
        list.resize(l0);
        if (!invert_call) return SLABS_OUTSIDE;
        *invert = 0;
        return within ? SLABS_INSIDE : SLABS_STRADDLING;
    }
    if (list.size() == l0) {                                // every slab holds the whole box
        if (invert_call) return SLABS_OUTSIDE;
        if (within) return SLABS_INSIDE;
    }
    return SLABS_STRADDLING;
}
