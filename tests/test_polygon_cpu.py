"""Polygon selection, the parts that need no GPU: the two entry points and two structs in the headers, the binding tables and the
cross-compiled library; the host plan of csrc/pcr_polygon.h, compiled with sanitizers into a stand-alone program and held against
the numpy restatement of tests/polygon_cases.py; that restatement's in_poly against a plain loop over Python integers;
polygon_from_world; the CLI's refusal of a malformed --polygon before any device is touched; and the preconditions of
tests/test_gpu_polygon.py, from the oracle's decoder.

The preconditions, as the oracle's decode gave them when the cases were chosen (class, base parity, listed edges per batch):
  synth CONCAVE:       batches 0 1 5 6 outside, 9 inside, 2 3 4 7 8 straddling (1 to 4 edges each, base parity 1); inverted: 0 1 5 6
                       inside, 9 outside
  clustered HOLE:      batch 1 (the centre cluster) outside, 4 inside, 0 2 3 straddling
  clustered zigzag:    batch 1 inside, the others straddling with 985, 648, 1550 and 498 of 4096 edges, batch 4 with base parity 1
  wide30 BOUNDARY:     4393 decoded points on an edge or a vertex, 2238 of them selected, 2155 not
  wide30 PART_A / _B:  34 decoded points on the shared diagonal
  garbage_tail TAIL:   29616 points selected, 50 of them beyond the header's box"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import oracle
from tests import polygon_cases as G
from tests import select_cases as S
from tests.test_abi import declared

SYMBOLS = ("pcr_select_polygon", "pcr_read_polygon")
PPB = G.PPB


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Polygon), C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(N.PolygonStats)]
    assert bound.pcr_select_polygon.argtypes == args and bound.pcr_read_polygon.argtypes == args


def test_structs_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirrors."""
    poly = [f for f, _ in N.Polygon._fields_]
    stats = [f for f, _ in N.PolygonStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\n'
                   'printf("%zu %zu ", sizeof(pcr_polygon), sizeof(pcr_polygon_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_polygon, {f}));\n' for f in poly)
                   + "".join(f'printf("%zu ", offsetof(pcr_polygon_stats, {f}));\n' for f in stats)
                   + 'printf("%d %u\\n", PCR_POLY_MAX_VERTICES, PCR_POLY_INVERT);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:2] == [40, 48] == [C.sizeof(N.Polygon), C.sizeof(N.PolygonStats)]
    assert poly == ["xy", "ring_sizes", "num_rings", "z_min", "z_max", "flags", "reserved"]
    assert stats == ["batches_outside", "batches_inside", "batches_straddling", "points_selected", "edges_listed", "edges_max"]
    assert [getattr(N.Polygon, f).offset for f in poly] == got[2:9] == [0, 8, 16, 20, 24, 28, 32]
    assert [getattr(N.PolygonStats, f).offset for f in stats] == got[9:15] == [0, 8, 16, 24, 32, 40]
    assert [N.POLY_MAX_VERTICES, N.POLY_INVERT] == got[15:] == [G.MAX_VERTICES, G.INVERT] == [P.POLY_MAX_VERTICES, P.POLY_INVERT]


# ---- the streams, decoded by the oracle ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(G.golden(name) if name in G.GOLDEN else G.stream(name))
    return np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)]).astype(np.int64), S.oracle_bounds(of)


NAMED = [("synth", G.CONCAVE), ("synth", G.CONCAVE.inverted()), ("synth", G.CONCAVE.with_z(20_000, 40_000)), ("clustered", G.HOLE),
         ("clustered", G.HOLE.inverted()), ("clustered", G.zigzag()), ("clustered", G.zigzag().inverted()), ("clustered", G.zigzag().with_z(0, 28_000)),
         ("wide30", G.BOUNDARY), ("wide30", G.PART_A), ("wide30", G.PART_B), ("wide30", G.PART_MERGED), ("garbage_tail", G.TAIL),
         ("garbage_tail", G.TAIL.inverted()), ("escape_heavy", G.EVERYTHING.with_z(-100, 20_000)), ("synth", G.COLLINEAR), ("wide30xy", G.WIDE),
         ("wide30xy", G.WIDE.inverted()), ("synth", G.CONCAVE.with_z(5, 4)), ("escape_heavy", G.ESCAPE_QUAD), ("escape_heavy", G.ESCAPE_QUAD.inverted()),
         ("synth", G.RECT), ("synth", G.SLAB), ("synth", G.EVERYTHING), ("wide30", G.COMB), ("wide30", G.COMB.inverted())]
NAMED += [(name, G.quantile_triangle(oracle_rows(name)[0])) for name in G.GOLDEN]        # (the GPU test builds them from read_points: the same rows)
NAMED += [(name, poly.inverted()) for name, poly in NAMED[-len(G.GOLDEN):]]


# ---- the host plan (csrc/pcr_polygon.h) in a program of its own ------------------------------------------------------------------------
PLAN_MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pcr_polygon.h"
// in: per case "nrings zmin zmax flags reserved", the ring sizes, the vertices, "nboxes", the boxes (min x y z, max x y z).
// out: per case "refused" or "ok", then per box "class base n" and n edges "lx ly dx dy".
int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long nr, zmin, zmax, flags, reserved;
    while (std::fscanf(f, "%lld %lld %lld %lld %lld", &nr, &zmin, &zmax, &flags, &reserved) == 5) {
        std::vector<int32_t> sizes((size_t)(nr > 0 ? nr : 0)), xy;
        long long total = 0, v;
        for (auto &s : sizes) { if (std::fscanf(f, "%lld", &v) != 1) return 3; s = (int32_t)v; total += v; }
        xy.resize((size_t)total * 2);
        for (auto &c : xy) { if (std::fscanf(f, "%lld", &v) != 1) return 3; c = (int32_t)v; }
        long long nb;
        if (std::fscanf(f, "%lld", &nb) != 1) return 3;
        std::vector<int32_t> boxes((size_t)nb * 6);
        for (auto &c : boxes) { if (std::fscanf(f, "%lld", &v) != 1) return 3; c = (int32_t)v; }
        const pcr_polygon p{xy.data(), sizes.data(), (int32_t)nr, (int32_t)zmin, (int32_t)zmax, (uint32_t)flags, (uint32_t)reserved};
        PolyShape s;
        if (poly_shape(&p, &s)) { std::puts("refused"); continue; }
        std::puts("ok");
        for (long long b = 0; b < nb; ++b) {
            std::vector<PolyEdge> list;
            uint32_t base = 7;
            const int cls = poly_plan_batch(s, boxes.data() + b * 6, list, &base);
            std::printf("%d %u %zu", cls, base, list.size());
            for (const PolyEdge &e : list) std::printf(" %d %d %d %d", e.lx, e.ly, e.dx, e.dy);
            std::puts("");
        }
    }
    std::fclose(f);
    return 0;
}
'''


def random_cases():
    """Random polygons of one to three rings over random boxes, among them boxes that touch an edge's bounding rectangle only at
    a corner and boxes that share only a border row or column with it."""
    rng = np.random.default_rng(4242)
    out = []
    for k in range(60):
        span = int(rng.choice([12, 40, 1000, 1 << 20]))
        rings = [[(int(a), int(b)) for a, b in rng.integers(-span, span + 1, (int(rng.integers(3, 9)), 2))] for _ in range(int(rng.integers(1, 4)))]
        if k % 5 == 0:
            rings[0].append(rings[0][0])                                    # a repeated closing vertex
        z = sorted(int(v) for v in rng.integers(-50, 51, 2))
        poly = G.Poly(rings, z[0], z[1] if k % 7 else z[0] - 1, invert=bool(k % 2))
        boxes = []
        for _ in range(12):
            lo = rng.integers(-span - 3, span + 3, 3)
            hi = lo + rng.integers(0, max(2, span // 2), 3)
            boxes.append([*lo[:2], int(rng.integers(-60, 60)), *hi[:2], 0])
            boxes[-1][5] = boxes[-1][2] + int(rng.integers(0, 40))
        for lx, ly, dx, dy in poly.edges()[:6]:
            ex0, ex1, ey1 = min(lx, lx + dx), max(lx, lx + dx), ly + dy
            w, h = int(rng.integers(0, 5)), int(rng.integers(0, 5))
            boxes.append([ex1, ey1, z[0], ex1 + w, ey1 + h, z[1]])          # touches the edge's rectangle at its north-east corner
            boxes.append([ex0 - w, ly - h, z[0], ex0, ly, z[0]])            # ... at its south-west corner
            boxes.append([ex1 + 1, ey1, z[0] - 5, ex1 + 1 + w, ey1 + h, z[1] + 5])      # one column off
            boxes.append([ex0 - w - 3, ly, z[0], ex0 - 1, ey1 - 1, z[1]])   # wholly left of it, its rows exactly
            boxes.append([ex0 - w - 3, ly + 1, z[0], ex0 - 1, ey1, z[1]])   # ... one row up: the top row is not the edge's
        out.append((poly, np.array(boxes, np.int64)))
    return out


REFUSED = [([[(0, 0), (1, 1)]], 0, 0), ([], 0, 0), ([G.ring_box(0, 0, 5, 5), [(1, 1), (2, 2)]], 0, 0), ([G.ring_box(0, 0, 5, 5)], 2, 0),
           ([G.ring_box(0, 0, 5, 5)], 1, 1), (G.WIDE_TOO_FAR, 0, 0), ([[(0, G.INT32_MIN), (5, 0), (0, 0)]], 0, 0),
           ([[(k, k * k % 97) for k in range(4097)]], 0, 0), ([[(k, k * k % 97) for k in range(2049)], [(k, 200 + k % 2) for k in range(2048)]], 0, 0)]


def test_host_plan_against_the_numpy_restatement(tmp_path):
    """poly_shape / poly_plan_batch, built with the address and undefined-behaviour sanitizers and run on their own: the named
    polygons over the oracle's exact batch boxes, random polygons over random boxes, and the polygons the call refuses."""
    cases = [(poly, oracle_rows(name)[1]) for name, poly in NAMED] + random_cases()
    cases.append((G.Poly([[(k, k * k % 97) for k in range(4096)]]), np.array([[0, 0, 0, 100, 100, 0], [50, 98, 0, 60, 99, 0]])))
    lines = []
    for poly, boxes in cases:
        lines.append(f"{len(poly.rings)} {poly.z_min} {poly.z_max} {int(poly.invert)} 0")
        lines.append(" ".join(str(len(r)) for r in poly.rings))
        lines.append(" ".join(f"{x} {y}" for r in poly.rings for x, y in r))
        lines.append(str(len(boxes)))
        lines += [" ".join(str(int(v)) for v in bb) for bb in boxes]
    for rings, flags, reserved in REFUSED:
        assert G.refusal(rings, flags, reserved) is not None
        lines.append(f"{len(rings)} 0 0 {flags} {reserved}")
        lines.append(" ".join(str(len(r)) for r in rings))
        lines.append(" ".join(f"{x} {y}" for r in rings for x, y in r))
        lines.append("0")
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "plan.cpp").write_text(PLAN_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", build.CSRC, "-I", build.INCLUDE, str(tmp_path / "plan.cpp"), "-o", str(tmp_path / "plan")], check=True)
    res = subprocess.run([str(tmp_path / "plan"), str(tmp_path / "cases.txt")], check=True, stdout=subprocess.PIPE, text=True)
    got = iter(res.stdout.splitlines())
    seen, parity, listed = set(), set(), 0
    for poly, boxes in cases:
        assert G.refusal(poly.rings) is None and next(got) == "ok"
        for bb in boxes:
            cls, base, edges = G.plan_batch(poly, bb)
            want = [cls, base, len(edges)] + [v for e in edges for v in e]
            assert [int(v) for v in next(got).split()] == want, (poly.rings[:1], bb.tolist())
            seen.add(cls); parity.add(base); listed += len(edges)
    for _ in REFUSED:
        assert next(got) == "refused"
    assert next(got, None) is None
    assert seen == {G.OUTSIDE, G.INSIDE, G.STRADDLING} and parity == {0, 1} and listed > 1000


def test_corner_touching_boxes_are_near_and_decide_by_the_rule():
    """A box that shares one corner with an edge's bounding rectangle is near (mixed), though no point of it may lie on the edge."""
    poly = G.Poly([[(0, 0), (10, 0), (10, 10)]])
    assert G.plan_batch(poly, [10, 10, 0, 15, 15, 0])[0] == G.STRADDLING and G.plan_batch(poly, [11, 10, 0, 15, 15, 0])[0] == G.OUTSIDE
    assert G.plan_batch(poly, [-5, -5, 0, 0, 0, 0])[0] == G.STRADDLING and G.plan_batch(poly.inverted(), [11, 11, 0, 12, 12, 0])[0] == G.INSIDE
    # the vertical edge lies wholly right of the box and covers its rows: folded into the base parity; one row more at the top: listed
    assert G.plan_batch(poly, [5, 1, 0, 8, 3, 0]) == (G.STRADDLING, 1, [(0, 0, 10, 10)])
    assert G.plan_batch(poly, [5, 1, 0, 8, 10, 0]) == (G.STRADDLING, 0, [(10, 0, 0, 10), (0, 0, 10, 10)])
    # no near edge, the polygon everywhere around the box, the z range across it: straddling with nothing to test but z
    assert G.plan_batch(G.EVERYTHING.with_z(0, 5), [0, 0, 3, 9, 9, 7]) == (G.STRADDLING, 1, [])


# ---- the reference against a plain loop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(NAMED)), ids=lambda k: f"{NAMED[k][0]}-{k}")
def test_reference_against_a_plain_loop(case):
    name, poly = NAMED[case]
    xyz, _ = oracle_rows(name)
    mask = G.selected(poly, xyz)
    step = 32 if sum(len(r) for r in poly.rings) > 1000 else 1             # (on_boundary and the loop are rows x edges)
    on = np.nonzero(G.on_boundary(poly, xyz[::step, 0], xyz[::step, 1]))[0] * step
    rows = np.unique(np.concatenate([np.arange(0, len(xyz), 257 * step), on[:400], np.nonzero(mask)[0][:300:step], np.nonzero(~mask)[0][:300:step]]))
    assert np.array_equal(mask[rows], G.selected_loop(poly, xyz[rows])) and len(rows) >= 50


def test_reference_on_small_polygons_point_by_point():
    for poly, _ in random_cases()[:20]:
        g = np.arange(-15, 16)
        xyz = np.stack([np.repeat(g, len(g)), np.tile(g, len(g)), np.zeros(len(g) ** 2, np.int64) + poly.z_min], axis=1)
        if max(abs(v) for r in poly.rings for p in r for v in p) <= 40:
            assert np.array_equal(G.selected(poly, xyz), G.selected_loop(poly, xyz))
    x0, y0, x1, y1 = 3, -2, 9, 4                                            # the rectangle polygon: x0 <= x < x1, y0 <= y < y1
    g = np.arange(-5, 12)
    x, y = np.repeat(g, len(g)), np.tile(g, len(g))
    assert np.array_equal(G.in_poly(G.Poly([G.ring_box(x0, y0, x1, y1)]), x, y), (x >= x0) & (x < x1) & (y >= y0) & (y < y1))


# ---- preconditions of the GPU cases ------------------------------------------------------------------------------------------------------
def classes(poly, bounds):
    return [p[0] for p in G.plan(poly, bounds)]


def test_concave_polygon_and_its_inverse_reach_all_three_classes():
    xyz, bounds = oracle_rows("synth")
    for poly in (G.CONCAVE, G.CONCAVE.inverted()):
        assert set(classes(poly, bounds)) == {G.OUTSIDE, G.INSIDE, G.STRADDLING}
        assert 0 < G.selected(poly, xyz).sum() < len(xyz)
    assert classes(G.CONCAVE, bounds)[9] == G.INSIDE and classes(G.CONCAVE.inverted(), bounds)[9] == G.OUTSIDE


def test_hole_puts_the_centre_cluster_outside():
    xyz, bounds = oracle_rows("clustered")
    cls = classes(G.HOLE, bounds)
    hole = G.HOLE.rings[1]
    assert cls[1] == G.OUTSIDE and set(cls) == {G.OUTSIDE, G.INSIDE, G.STRADDLING}
    assert hole[0][0] < bounds[1, 0] and hole[0][1] < bounds[1, 1] and hole[2][0] > bounds[1, 3] and hole[2][1] > bounds[1, 4]
    assert not G.selected(G.HOLE, xyz[PPB:2 * PPB]).any() and G.selected(G.HOLE.inverted(), xyz[PPB:2 * PPB]).all()


def test_boundary_case_has_points_on_its_edges_both_ways():
    xyz, _ = oracle_rows("wide30")
    decoded = set(map(tuple, xyz[:, :2].tolist()))
    assert all(v in decoded for v in G.BOUNDARY.rings[0]), "every vertex is a decoded point"
    kinds = {(dx == 0, dy == 0) for _, _, dx, dy in G.BOUNDARY.edges()}
    assert kinds == {(True, False), (False, True), (False, False)}, "vertical, horizontal and diagonal edges"
    on = G.on_boundary(G.BOUNDARY, xyz[:, 0], xyz[:, 1])
    sel = G.selected(G.BOUNDARY, xyz)
    print(f"{on.sum()} points on the boundary, {(on & sel).sum()} selected, {(on & ~sel).sum()} not")
    assert on.sum() >= 16 and (on & sel).sum() >= 4 and (on & ~sel).sum() >= 4
    shared = G.on_boundary(G.PART_A, xyz[:, 0], xyz[:, 1]) & G.on_boundary(G.PART_B, xyz[:, 0], xyz[:, 1])
    assert shared.sum() >= 4, "decoded points on the edge the two parts share"


def test_many_vertex_case():
    xyz, bounds = oracle_rows("clustered")
    poly = G.zigzag()
    assert len(poly.rings) == 1 and len(poly.rings[0]) == G.MAX_VERTICES == len(set(poly.rings[0]))
    plans = G.plan(poly, bounds)
    st = G.plan_stats(plans)
    non_horizontal = sum(1 for e in poly.edges() if e[3])
    print(st, non_horizontal)
    assert st["batches_straddling"] >= 2 and st["edges_max"] < non_horizontal / 2
    assert any(p[0] == G.STRADDLING and p[1] == 1 for p in plans), "a straddling batch with base parity 1"
    assert 0 < G.selected(poly, xyz).sum() < len(xyz)


def test_comb_lists_all_its_teeth_for_both_batches_and_the_other_gpu_cases_select_something():
    xyz, bounds = oracle_rows("wide30")
    plans = G.plan(G.COMB, bounds)
    assert [(p[0], len(p[2])) for p in plans] == [(G.STRADDLING, G.COMB_LISTED)] * 2 and len(G.COMB.rings[0]) == G.MAX_VERTICES
    assert G.COMB_LISTED >= G.MAX_VERTICES - 8, "16 KiB of table and nearly 64 KiB of edges in one launch"
    for name, poly in (("wide30", G.COMB), ("escape_heavy", G.ESCAPE_QUAD), ("synth", G.RECT), ("synth", G.SLAB)):
        rows = oracle_rows(name)[0]
        assert 0 < G.selected(poly, rows).sum() < len(rows)
    for name in G.GOLDEN:
        rows = oracle_rows(name)[0]
        tri = G.quantile_triangle(rows)
        assert 0 < G.selected(tri, rows).sum() < len(rows) and 0 < G.selected(tri.inverted(), rows).sum()
    sub = oracle_rows("synth")[1][3:8]                                      # the sub-range case: other batches inside with the inverse
    a, b = G.plan_stats(G.plan(G.CONCAVE, sub)), G.plan_stats(G.plan(G.CONCAVE.inverted(), sub))
    assert a["batches_straddling"] >= 2 and a["batches_inside"] != b["batches_inside"]


def test_tail_polygon_reaches_the_artefact_and_wide_polygon_splits_both_clusters():
    xyz, _ = oracle_rows("garbage_tail")
    sel = G.selected(G.TAIL, xyz)
    assert (xyz[sel][:, 1] > G.TAIL_BEYOND_Y).sum() >= 1 and sel.sum() > 1000
    xyz, bounds = oracle_rows("wide30xy")
    sel = G.selected(G.WIDE, xyz)
    x0, y0, x1, y1 = G.WIDE.rect()
    assert x1 - x0 == y1 - y0 == G.MAX_EXTENT and G.refusal(G.WIDE.rings) is None and G.refusal(G.WIDE_TOO_FAR) == "extent"
    for far in (False, True):
        m = (xyz[:, 0] >= 1 << 30) == far
        assert 0.2 < sel[m & (np.abs(xyz[:, 2]) < 100)].mean() < 0.8
    big = max(abs((int(x) - lx) * dy) for x, y, _ in xyz[sel][:2000] for lx, ly, dx, dy in G.WIDE.edges() if ly <= y < ly + dy)
    assert 1 << 60 <= big < 1 << 62
    assert classes(G.WIDE, bounds) == [G.STRADDLING, G.STRADDLING]


# ---- polygon_from_world ----------------------------------------------------------------------------------------------------------------
def las(scale=(0.001, 0.001, 0.001), offset=(0.0, 0.0, 0.0)):
    info = P.LasInfo()
    for k in range(3):
        info.scale[k], info.offset[k], info.min[k], info.max[k] = scale[k], offset[k], 0.0, 1000.0
    return info


def test_polygon_from_world():
    world = [(0.0004, 0.0), (1.0014, 0.0), (0.5, 2.0026), (-0.0006, 1.0)]
    p = P.polygon_from_world(las(), world)
    assert [r.tolist() for r in p.rings] == [[[0, 0], [1001, 0], [500, 2003], [-1, 1000]]]          # the nearest step
    assert (np.abs(np.array(world) - p.rings[0] * 0.001) <= 0.0005 + 1e-12).all()                  # ... at most half a step away
    half = P.polygon_from_world(las((0.5, 0.5, 0.5)), [(0.25, 0.75), (1.2, -0.3), (10.0, 3.9)])
    assert half.rings[0].tolist() == [[0, 2], [2, -1], [20, 8]]                                     # exact ties go to the even step
    assert (p.z_min, p.z_max, p.invert) == (G.INT32_MIN, G.INT32_MAX, False) and p.c.num_rings == 1 and p.c.flags == 0
    p = P.polygon_from_world(las((0.01, 0.02, 0.5), (100.0, -50.0, 3.0)), [[(100.0, -50.0), (101.0, -50.0), (101.0, -49.0)], [(100.2, -49.9), (100.4, -49.9), (100.4, -49.8)]],
                             z_lo=3.2, z_hi=10.0, invert=True)
    assert [r.tolist() for r in p.rings] == [[[0, 0], [100, 0], [100, 50]], [[20, 5], [40, 5], [40, 10]]]
    box = P.box_from_world(las((0.01, 0.02, 0.5), (100.0, -50.0, 3.0)), (-np.inf, -np.inf, 3.2), (np.inf, np.inf, 10.0))
    assert (p.z_min, p.z_max) == (box.min[2], box.max[2]) == (1, 14) and p.invert and p.c.flags == P.POLY_INVERT and p.c.num_rings == 2
    assert [p.c.xy[k] for k in range(12)] == [0, 0, 100, 0, 100, 50, 20, 5, 40, 5, 40, 10] and [p.c.ring_sizes[k] for k in range(2)] == [3, 3]
    empty = P.polygon_from_world(las(), G.ring_box(0.0, 0.0, 1.0, 1.0), z_lo=5.0, z_hi=4.0)
    assert empty.z_min > empty.z_max


@pytest.mark.parametrize("rings", [[(0.0, 0.0), (1.0, 1.0)], [[(0.0, 0.0), (1.0, 0.0), (3.0e6, 1.0)]], [[(0.0, 0.0), (1.0, 0.0), (float("nan"), 1.0)]],
                                   [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)], [(0.0, 0.0)]], [[(0.0, 0.0), (1.0, 0.0), (-2147483.649, 1.0)]]])
def test_polygon_from_world_refuses(rings):
    with pytest.raises(ValueError):
        P.polygon_from_world(las(), rings)


def test_polygon_accepts_the_edge_of_int32_and_refuses_beyond():
    assert P.polygon_from_world(las(), [(0.0, 0.0), (1.0, 0.0), (2147483.647, -2147483.648)]).rings[0][2].tolist() == [G.INT32_MAX, G.INT32_MIN]
    with pytest.raises(ValueError):
        P.Polygon([[(0, 0), (1, 0), (1 << 31, 5)]])
    with pytest.raises(ValueError):
        P.Polygon([[(0, 0), (1, 0), (1, 1)]], z_min=-(1 << 31) - 1)
    for bad in ([(0.9, 0.9), (1, 0), (1, 1)], [[(0, 0), (1, 0), (1 << 70, 1)]], [[(0, 0), (1, 0), (float("nan"), 1)]]):
        with pytest.raises(ValueError):                                     # nothing is rounded or wrapped silently
            P.Polygon(bad)
    with pytest.raises(ValueError):
        P.Polygon([(0, 0), (4, 0), (4, 4)], z_min=1.5)
    assert P.Polygon([[(0.0, 0), (4, 0), (4, 4.0)]]).rings[0].tolist() == [[0, 0], [4, 0], [4, 4]]      # whole numbers as floats are taken
    p = P.Polygon([(0, 0), (4, 0), (4, 4)], 1, 2, True)                     # a single ring given alone
    assert len(p.rings) == 1 and p.inverted().invert is False and p.inverted().c.flags == 0


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
GOOD = "0 0\n10 0\n10 10\n\n2 2\n3 2\n3 3\n"


@pytest.mark.parametrize("text,args", [(None, []), ("", []), ("\n\n", []), ("0 0\n1 1\n", []), ("0 0\n1 0\n1 1\n\n5 5\n6 6\n", []), ("0 0\n1 0 7\n1 1\n", []),
                                       ("0 0\n1 x\n1 1\n", []), ("0 0\n1\n1 1\n", []), ("0 0\n1 nan\n1 1\n", []), (GOOD, ["--z", "1"]), (GOOD, ["--z", "a", "2"]),
                                       (GOOD, ["--outside", "--outside"]), (GOOD, ["--box", "0", "0", "0", "1", "1", "1"]), (GOOD, ["--z", "0", "1", "--z", "0", "1"]),
                                       ("".join(f"{k} {k * k % 97}\n" for k in range(4097)), [])])
def test_cli_refuses_a_malformed_polygon_before_it_creates_a_context(tmp_path, text, args):
    build.build_tools()
    out, poly = tmp_path / "out.las", tmp_path / "poly.txt"
    if text is not None:
        poly.write_text(text)
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), "--polygon", str(poly), *args], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and "usage: pcr_decode" in res.stderr and "--polygon FILE" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()


def test_cli_accepts_a_well_formed_polygon_and_then_looks_for_the_stream(tmp_path):
    build.build_tools()
    (tmp_path / "poly.txt").write_text(GOOD)
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(tmp_path / "out.las"), "--polygon", str(tmp_path / "poly.txt"), "--z", "0", "5",
                          "--outside"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 1 and "usage" not in res.stderr
