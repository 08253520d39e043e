// The host plan of a polygon selection (pcr_select_polygon, include/pcr_hip.h has the rule): the checks on a pcr_polygon, its
// edges, in_poly for one point, and per batch -- from the batch's exact box -- the class, the base parity and the edge list.
// Plain C++ without a HIP dependency, so a host-only build can call it.
#pragma once
#include <cstdint>
#include <vector>

#include "pcr_types.h"

// An edge from its lower endpoint l: u = l + (dx, dy), dy >= 0. 16 bytes, the entry of the array the kernels read (there dy > 0).
// dy == 0: a horizontal edge, l its left end (dx >= 0); it takes part in the class rule only.
struct PolyEdge { int32_t lx, ly, dx, dy; };

// A checked polygon: the edges of all rings in ring order, the bounding rectangle of all vertices, the z range, the flag.
struct PolyShape {
    std::vector<PolyEdge> edges;
    int32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    int32_t z_min = 0, z_max = 0;
    uint32_t invert = 0;
};

enum { POLY_OUTSIDE = 0, POLY_INSIDE = 1, POLY_STRADDLING = 2 };

// nullptr and *s filled, or what is wrong with *p. The extent limit makes every difference of two coordinates inside the
// rectangle, dx and dy among them, fit 32 signed bits.
inline const char *poly_shape(const pcr_polygon *p, PolyShape *s)
{
    if (!p) return "the polygon is NULL";
    if (!p->xy) return "pcr_polygon::xy is NULL";
    if (!p->ring_sizes) return "pcr_polygon::ring_sizes is NULL";
    if (p->num_rings < 1) return "pcr_polygon::num_rings is below 1";
    if (p->flags & ~PCR_POLY_INVERT) return "pcr_polygon::flags has unknown bits";
    if (p->reserved != 0) return "pcr_polygon::reserved is not 0";
    int64_t total = 0;
    for (int32_t r = 0; r < p->num_rings; ++r) {
        if (p->ring_sizes[r] < 3) return "a ring has fewer than 3 vertices";
        total += p->ring_sizes[r];
        if (total > PCR_POLY_MAX_VERTICES) return "more vertices than PCR_POLY_MAX_VERTICES";
    }
    int32_t lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {INT32_MIN, INT32_MIN};
    for (int64_t i = 0; i < total; ++i)
        for (int k = 0; k < 2; ++k) {
            const int32_t v = p->xy[2 * i + k];
            if (v < lo[k]) lo[k] = v;
            if (v > hi[k]) hi[k] = v;
        }
    for (int k = 0; k < 2; ++k)
        if ((int64_t)hi[k] - (int64_t)lo[k] > (int64_t)INT32_MAX) return "the vertices span more than 2^31 - 1 on x or y";
    s->x0 = lo[0]; s->y0 = lo[1]; s->x1 = hi[0]; s->y1 = hi[1];
    s->z_min = p->z_min; s->z_max = p->z_max;
    s->invert = p->flags & PCR_POLY_INVERT;
    s->edges.clear();
    s->edges.reserve((size_t)total);
    const int32_t *ring = p->xy;
    for (int32_t r = 0; r < p->num_rings; ++r) {
        const int32_t m = p->ring_sizes[r];
        for (int32_t i = 0; i < m; ++i) {
            const int32_t *a = ring + 2 * i, *b = ring + 2 * ((i + 1) % m);
            const bool a_low = a[1] < b[1] || (a[1] == b[1] && a[0] <= b[0]);
            const int32_t *l = a_low ? a : b, *u = a_low ? b : a;
            s->edges.push_back(PolyEdge{l[0], l[1], (int32_t)((int64_t)u[0] - l[0]), (int32_t)((int64_t)u[1] - l[1])});
        }
        ring += 2 * (size_t)m;
    }
    return nullptr;
}

// in_poly(x, y). The rectangle first: a point outside it is not in the polygon, and inside it the products stay below 2^62.
inline bool poly_in(const PolyShape &s, int32_t x, int32_t y)
{
    if (x < s.x0 || x > s.x1 || y < s.y0 || y > s.y1) return false;
    bool odd = false;
    for (const PolyEdge &e : s.edges) {
        const int64_t t = (int64_t)y - e.ly;
        if (t < 0 || t >= e.dy) continue;                   // (never true for a horizontal edge)
        if (((int64_t)x - e.lx) * e.dy < t * e.dx) odd = !odd;
    }
    return odd;
}

// The class of a batch with the exact box bb = min x, y, z, max x, y, z. POLY_STRADDLING: the batch's edge list is appended to
// `list` (possibly nothing) and *base_parity is the parity of the edges every point of the box's rectangle counts.
inline int poly_plan_batch(const PolyShape &s, const int32_t bb[6], std::vector<PolyEdge> &list, uint32_t *base_parity)
{
    *base_parity = 0;
    if (s.z_min > s.z_max || bb[5] < s.z_min || bb[2] > s.z_max) return POLY_OUTSIDE;
    const bool z_all_in = s.z_min <= bb[2] && bb[5] <= s.z_max;
    const int64_t rx0 = bb[0], ry0 = bb[1], rx1 = bb[3], ry1 = bb[4];
    bool near = false;
    for (const PolyEdge &e : s.edges) {
        const int64_t ux = (int64_t)e.lx + e.dx, ex0 = ux < e.lx ? ux : e.lx, ex1 = ux < e.lx ? e.lx : ux, ey1 = (int64_t)e.ly + e.dy;
        if (ex0 <= rx1 && ex1 >= rx0 && e.ly <= ry1 && ey1 >= ry0) { near = true; break; }
    }
    if (!near) {
        if (poly_in(s, bb[0], bb[1]) == (s.invert != 0)) return POLY_OUTSIDE;
        if (z_all_in) return POLY_INSIDE;
    }
    for (const PolyEdge &e : s.edges) {
        if (e.dy == 0) continue;
        const int64_t ux = (int64_t)e.lx + e.dx, ex0 = ux < e.lx ? ux : e.lx, ex1 = ux < e.lx ? e.lx : ux, ey1 = (int64_t)e.ly + e.dy;
        if (e.ly > ry1 || ey1 <= ry0) continue;             // [l.y, u.y) misses the rectangle's rows
        if (ex1 <= rx0) continue;                           // no point of the rectangle is left of it
        if (ex0 > rx1 && e.ly <= ry0 && ey1 > ry1) { *base_parity ^= 1u; continue; }    // every point of the rectangle counts it
        list.push_back(e);
    }
    return POLY_STRADDLING;
}
