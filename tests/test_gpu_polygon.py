"""pcr_select_polygon / pcr_read_polygon: the points of a loaded stream inside a polygon prism, selected on the GPU.

The contract is pcr_select_box's with another predicate -- the output equals pcr_decode_points of the same range with the
unselected records removed, byte for byte -- so the reference of every selection here is Context.read_points masked in numpy
(tests/polygon_cases.py: in_poly in int64; for the polygon of extent 2^31 - 1 the plain loop over Python integers), colours
included, and the reference of the batch classes and edge lists is the numpy restatement of the host plan over
Context.batch_point_bounds (which tests/test_gpu_select.py holds against the oracle). Every case runs for a context loaded with
PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there through both variants, which have to agree), as
tests/test_gpu_select.py does. tests/test_polygon_cpu.py checks on the CPU that the polygons reach every class, lie on decoded
points and fold edges into the base parity."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import scenes
from tests import polygon_cases as G
from tests import select_cases as S
from tests.polygon_cases import GOLDEN, golden
from tests.test_gpu_select import LAYOUTS, load, through_variants, xyz_of

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
STAT_NAMES = list(N.PolygonStats().as_dict())
CLASS_NAMES = ("batches_outside", "batches_inside", "batches_straddling")


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


def image_of(name):
    return golden(name) if name in GOLDEN else G.stream(name)


_points = {}        # stream -> (read_points of the whole stream, its xyz as int64, the exact batch boxes): computed once, never changed
_masks = {}         # (stream, id of the polygon) -> (the polygon, the reference's mask over the whole stream)


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, xyz_of(pts).astype(np.int64), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def mask_of(name, poly, loop=False):
    key = (name, id(poly))
    if key not in _masks:
        xyz = _points[name][1]
        _masks[key] = (poly, G.selected_loop(poly, xyz) if loop else G.selected(poly, xyz))
    return _masks[key][1]


def select(c, poly, first=0, count=None):
    """read_polygon of the range (both variants) and the statistics it reported."""
    native = poly.native()

    def go():
        return c.read_polygon(native, first, count), np.array([c.polygon_stats[k] for k in STAT_NAMES])
    pts, st = through_variants(c, go)
    return pts, dict(zip(STAT_NAMES, (int(v) for v in st)))


def check(c, name, poly, first=0, count=None, loop=False, loaded=None):
    """read_polygon == read_points of the same range masked by the reference, byte for byte; the classes are the restatement's,
    edges_listed is at most the rule's, points_selected the length. loaded = (a, n): the context holds batches [a, a + n) of the
    stream only, and `first` counts from a."""
    pts_all, _, bounds = _points[name]
    if loaded:
        pts_all, bounds = pts_all[loaded[0] * PPB:sum(loaded) * PPB], bounds[loaded[0]:sum(loaded)]
    last = len(pts_all) // PPB if count is None else first + count
    mask = mask_of(name, poly, loop)[loaded[0] * PPB:sum(loaded) * PPB] if loaded else mask_of(name, poly, loop)
    want = pts_all[first * PPB:last * PPB][mask[first * PPB:last * PPB]]
    got, st = select(c, poly, first, count)
    assert got.dtype == want.dtype and len(got) == len(want), f"{len(got)} records selected, {len(want)} expected ({name})"
    assert got.tobytes() == want.tobytes(), f"records differ, first at {np.nonzero(got != want)[0][:4]} ({name})"
    rule = G.plan_stats(G.plan(poly, bounds[first:last]))
    assert {k: st[k] for k in CLASS_NAMES} == {k: rule[k] for k in CLASS_NAMES}, (name, st, rule)
    assert st["edges_listed"] <= rule["edges_listed"] and st["edges_max"] <= rule["edges_max"], (name, st, rule)
    assert st["points_selected"] == len(want)
    return got, st


def check_both(c, name, poly, **kw):
    """... and the same with PCR_POLY_INVERT (the inverse is kept alive with the polygon, so id() stays a key)."""
    if not hasattr(poly, "inverse"):
        poly.inverse = poly.inverted()
    a, b = check(c, name, poly, **kw), check(c, name, poly.inverse, **kw)
    if poly.z_min == G.INT32_MIN and poly.z_max == G.INT32_MAX and not kw:
        assert len(a[0]) + len(b[0]) == len(_points[name][0]), "a polygon and its inverse share the stream out between them"
    return a, b


# ---- 1. selections against read_points masked ------------------------------------------------------------------------------------
_triangles = {}


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_golden_streams_with_a_triangle_through_quantile_points(ctx, name, frame):
    load(ctx, image_of(name), frame=frame)
    _, xyz, _ = points_of(ctx, name)
    tri = _triangles.setdefault(name, G.quantile_triangle(xyz))
    (got, st), _ = check_both(ctx, name, tri)
    print(f"{name}: {len(got)} of {len(xyz)} records, {st}")
    assert 0 < len(got) < len(xyz)


CASES = [("synth", G.CONCAVE), ("clustered", G.HOLE), ("wide30", G.BOUNDARY), ("clustered", G.zigzag()), ("garbage_tail", G.TAIL),
         ("escape_heavy", G.ESCAPE_QUAD), ("synth", G.CONCAVE.with_z(20_000, 40_000)), ("clustered", G.zigzag().with_z(0, 28_000)), ("wide30", G.COMB)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["concave", "hole", "boundary", "zigzag", "garbage_tail", "escape_heavy", "concave_z", "zigzag_z", "comb"])
def test_named_polygons_and_their_inverses(ctx, case):
    name, poly = CASES[case]
    load(ctx, image_of(name))
    _, xyz, _ = points_of(ctx, name)
    (got, st), (inv, ist) = check_both(ctx, name, poly)
    print(f"{name}: {len(got)} / {len(inv)} of {len(xyz)} records, {st}, inverted {ist}")
    assert 0 < len(got) < len(xyz) and 0 < len(inv) < len(xyz)
    if poly is G.CONCAVE:
        assert min(st[k] for k in CLASS_NAMES) >= 1 and min(ist[k] for k in CLASS_NAMES) >= 1
    if poly is G.HOLE:
        assert st["batches_outside"] >= 1 and not mask_of(name, poly)[PPB:2 * PPB].any()
    if poly is G.BOUNDARY:
        on = G.on_boundary(poly, xyz[:, 0], xyz[:, 1])
        assert (on & mask_of(name, poly)).sum() >= 4 and (on & ~mask_of(name, poly)).sum() >= 4
    if poly is G.zigzag():
        assert st["batches_straddling"] >= 2 and 0 < st["edges_max"] < G.MAX_VERTICES // 2
    if poly is G.TAIL:
        assert (got["y"] > G.TAIL_BEYOND_Y).any(), "the polygon reaches the tail artefact"
    if poly is G.COMB:                                                      # the table and all but two of 4096 edges in one workgroup's LDS
        assert st["edges_max"] == ist["edges_max"] == G.COMB_LISTED and st["batches_straddling"] == 2


def test_sub_range_of_a_stream_loaded_with_upload_tail(ctx):
    image = image_of("synth")
    load(ctx, image)
    points_of(ctx, "synth")
    load(ctx, image, first=3, count=5)                                      # batches 3..7 of the file, the follower's head words behind them
    ref = through_variants(ctx, ctx.read_points)
    assert ref.tobytes() == _points["synth"][0][3 * PPB:8 * PPB].tobytes()
    assert np.array_equal(ctx.batch_point_bounds(), _points["synth"][2][3:8])
    (whole, st), (whole_inv, ist) = check_both(ctx, "synth", G.CONCAVE, loaded=(3, 5))
    assert len(whole) > 0 and len(whole_inv) > 0 and st["batches_straddling"] >= 2 and ist["batches_straddling"] >= 2
    assert ist["batches_inside"] != st["batches_inside"], "the inverse writes other batches whole, so other offsets"
    parts, parts_inv = [], []
    for first, count in ((0, 2), (2, 0), (2, 1), (3, None)):                # ranges of the loaded part: batch `first` of the context is batch 3 + first
        (pts, _), (inv, _) = check_both(ctx, "synth", G.CONCAVE, first=first, count=count, loaded=(3, 5))
        parts.append(pts); parts_inv.append(inv)
    assert np.concatenate(parts).tobytes() == whole.tobytes() and np.concatenate(parts_inv).tobytes() == whole_inv.tobytes()
    for poly in (G.CONCAVE, G.CONCAVE.inverse):
        pts, st = select(ctx, poly, 5, None)
        assert len(pts) == 0 and sum(st[k] for k in CLASS_NAMES) == 0


# ---- 2. against the box selection ---------------------------------------------------------------------------------------------------
def test_rectangle_and_slab_equal_read_box(ctx):
    load(ctx, image_of("synth"))
    _, xyz, _ = points_of(ctx, "synth")
    (x0, y0, z0), (x1, y1, z1) = G.RECT_BOX
    got, st = check(ctx, "synth", G.RECT)
    box = through_variants(ctx, lambda: ctx.read_box(((x0, y0, z0), (x1 - 1, y1 - 1, z1))))
    assert got.tobytes() == box.tobytes() and len(got) > 0 and st["batches_straddling"] >= 1
    got, st = check(ctx, "synth", G.SLAB)
    box = through_variants(ctx, lambda: ctx.read_box(((G.INT32_MIN,) * 2 + (20_000,), (G.INT32_MAX,) * 2 + (40_000,))))
    assert got.tobytes() == box.tobytes() and 0 < len(got) < len(xyz) and st["edges_listed"] == 0 and st["batches_straddling"] >= 1
    got, st = check(ctx, "synth", G.EVERYTHING)
    assert got.tobytes() == _points["synth"][0].tobytes() and st["batches_inside"] == len(xyz) // PPB


# ---- 3. partition ---------------------------------------------------------------------------------------------------------------------
def test_two_polygons_that_share_an_edge_share_its_points_out(ctx):
    load(ctx, image_of("wide30"))
    pts, xyz, _ = points_of(ctx, "wide30")
    shared = G.on_boundary(G.PART_A, xyz[:, 0], xyz[:, 1]) & G.on_boundary(G.PART_B, xyz[:, 0], xyz[:, 1])
    assert shared.sum() >= 4, "decoded points on the shared edge"
    a, _ = check(ctx, "wide30", G.PART_A)
    b, _ = check(ctx, "wide30", G.PART_B)
    merged, _ = check(ctx, "wide30", G.PART_MERGED)

    def rows_of(sel, mask):                                                 # the rows of read_points the selection is
        rows = np.nonzero(mask)[0]
        assert pts[rows].tobytes() == sel.tobytes()
        return rows
    ra, rb, rm = rows_of(a, mask_of("wide30", G.PART_A)), rows_of(b, mask_of("wide30", G.PART_B)), rows_of(merged, mask_of("wide30", G.PART_MERGED))
    assert len(np.intersect1d(ra, rb)) == 0 and np.array_equal(np.union1d(ra, rb), rm)
    on = np.nonzero(shared)[0]
    assert np.isin(on, rm).all() and (np.isin(on, ra) != np.isin(on, rb)).all()


# ---- 4. arithmetic --------------------------------------------------------------------------------------------------------------------
def test_extent_of_2_31_minus_1_against_python_integers(ctx):
    load(ctx, image_of("wide30xy"))
    _, xyz, _ = points_of(ctx, "wide30xy")
    (got, st), (inv, _) = check_both(ctx, "wide30xy", G.WIDE, loop=True)
    far = got["x"] >= 1 << 30
    assert far.sum() > 1000 and (~far).sum() > 1000 and len(inv) > 1000 and st["batches_straddling"] == 2
    with pytest.raises(P.PcrError, match="2\\^31 - 1"):
        ctx.read_polygon(P.Polygon(G.WIDE_TOO_FAR))


# ---- 5. the interface -------------------------------------------------------------------------------------------------------------------
def native_polygon(rings, z_min=G.INT32_MIN, z_max=G.INT32_MAX, flags=0, reserved=0):
    xy = np.array([v for r in rings for p in r for v in p], np.int32)
    sizes = np.array([len(r) for r in rings], np.int32)
    p = N.Polygon(xy.ctypes.data_as(C.POINTER(C.c_int32)), sizes.ctypes.data_as(C.POINTER(C.c_int32)), len(rings), z_min, z_max, flags, reserved)
    p.keep = (xy, sizes)
    return p


def test_count_capacity_and_the_torch_entry(ctx):
    import torch
    load(ctx, image_of("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    want = pts_all[mask_of("synth", G.CONCAVE)]
    poly = G.CONCAVE.native()
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.PolygonStats()
    assert lib.pcr_select_polygon(h, 0, -1, C.byref(poly.c), None, 0, C.byref(cnt), C.byref(st)) == 0          # count only
    assert cnt.value == len(want) == st.points_selected and st.batches_straddling >= 1
    cnt.value = -5
    assert lib.pcr_read_polygon(h, 0, -1, C.byref(poly.c), None, 0, C.byref(cnt), None) == 0 and cnt.value == len(want)    # stats may be NULL
    SENT = 0x5A5A5A5A
    dev = torch.full((len(want) + 16, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    torch.cuda.synchronize()
    assert lib.pcr_select_polygon(h, 0, -1, C.byref(poly.c), C.c_void_p(dev.data_ptr()), len(want), C.byref(cnt), C.byref(st)) == 0
    got = dev.cpu().numpy()
    assert cnt.value == len(want) and got[:len(want)].tobytes() == want.tobytes() and (got[len(want):] == SENT).all()
    dev.fill_(SENT); torch.cuda.synchronize()
    cnt.value = -5
    assert lib.pcr_select_polygon(h, 0, -1, C.byref(poly.c), C.c_void_p(dev.data_ptr()), len(want) - 1, C.byref(cnt), C.byref(st)) == PCR_E_ARG
    assert cnt.value == len(want) and (lib.pcr_last_error(h) or b"") != b""
    ctx.synchronize(); torch.cuda.synchronize()
    assert (dev.cpu().numpy() == SENT).all(), "a refused selection wrote into the buffer"
    host = np.full((len(want) + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    before = host.tobytes()
    cnt.value = -5
    assert lib.pcr_read_polygon(h, 0, -1, C.byref(poly.c), host.ctypes.data, len(want) - 1, C.byref(cnt), None) == PCR_E_ARG
    assert cnt.value == len(want) and host.tobytes() == before
    assert lib.pcr_read_polygon(h, 0, -1, C.byref(poly.c), host.ctypes.data, len(want), C.byref(cnt), None) == 0
    assert host[:len(want)].tobytes() == want.tobytes() and host[len(want):].tobytes() == before[len(want) * 16:]
    # Context.select_polygon: the torch tensor, with and without `out`
    t = through_variants(ctx, lambda: ctx.select_polygon(poly).cpu().numpy())
    assert t.dtype == np.int32 and t.shape == (len(want), 4) and t.tobytes() == want.tobytes()
    assert ctx.polygon_stats["points_selected"] == len(want)
    out = torch.empty((len(want) + 3, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    res = ctx.select_polygon(poly, out=out)
    assert res.is_cuda and res.dtype == torch.int32 and res.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(P.PcrError):
        ctx.select_polygon(poly, out=torch.empty((len(want) - 1, 4), dtype=torch.int32, device=out.device))
    assert ctx.polygon_stats["points_selected"] == len(want)
    # an empty z range and a polygon of collinear vertices: 0 records, PCR_OK
    assert tuple(ctx.select_polygon(G.CONCAVE.with_z(5, 4).native()).shape) == (0, 4) and ctx.polygon_stats["batches_outside"] == len(xyz) // PPB
    got, st = check(ctx, "synth", G.COLLINEAR)
    assert len(got) == 0
    got, st = check(ctx, "synth", G.CONCAVE.with_z(5, 4).inverted())
    assert len(got) == 0 and st["batches_outside"] == len(xyz) // PPB


def test_errors_are_pcr_e_arg_with_a_message(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    SENT = 0x5A5A5A5A
    buf = torch.full((2 * PPB + 1, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    host = np.full((2 * PPB + 1) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    good = native_polygon([G.ring_box(-5_000_000, -5_000_000, 5_000_000, 5_000_000)])
    cnt = C.c_int64()

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    entries = ((lib.pcr_select_polygon, buf.data_ptr()), (lib.pcr_read_polygon, host.ctypes.data))
    for entry, dst in entries:                                              # no stream loaded
        refused(entry(h, 0, 1, C.byref(good), C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
    load(ctx, image_of("synth"))
    nb = ctx.batches_loaded
    no_xy, no_sizes = native_polygon([G.ring_box(0, 0, 5, 5)]), native_polygon([G.ring_box(0, 0, 5, 5)])
    no_xy.xy, no_sizes.ring_sizes = None, None
    no_rings = native_polygon([G.ring_box(0, 0, 5, 5)]); no_rings.num_rings = 0
    bad = [no_xy, no_sizes, no_rings,
           native_polygon([G.ring_box(0, 0, 5, 5), [(1, 1), (2, 2)]]),                                  # a ring of 2 vertices
           native_polygon([[(k, k * k % 97) for k in range(4097)]]),                                   # 4097 vertices
           native_polygon([[(k, k * k % 97) for k in range(2049)], [(k, 200 + k % 2) for k in range(2048)]]),
           native_polygon([G.ring_box(0, 0, 5, 5)], flags=2), native_polygon([G.ring_box(0, 0, 5, 5)], flags=3),
           native_polygon([G.ring_box(0, 0, 5, 5)], reserved=1),
           native_polygon(G.WIDE_TOO_FAR), native_polygon([[(0, G.INT32_MIN), (5, 0), (0, 0)]])]      # an extent of 2^31 on x, on y
    for entry, dst in entries:
        for p in bad:
            refused(entry(h, 0, 1, C.byref(p), C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
        refused(entry(h, 0, 1, None, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))                   # a NULL polygon
        refused(entry(h, 0, 1, C.byref(good), C.c_void_p(dst), 2 * PPB, None, None))                  # a NULL out_count
        refused(entry(h, nb - 1, 2, C.byref(good), C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))     # a range outside the resident batches
        refused(entry(h, -1, 1, C.byref(good), C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
        refused(entry(h, nb + 1, -1, C.byref(good), C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
        refused(entry(h, 0, 2, C.byref(good), C.c_void_p(dst), 2 * PPB - 1, C.byref(cnt), None))      # capacity below the result
        assert cnt.value == 2 * PPB
        assert entry(h, 0, 0, C.byref(good), None, 0, C.byref(cnt), None) == 0 and cnt.value == 0     # 0 batches: succeeds
    refused(lib.pcr_select_polygon(h, 0, 1, C.byref(good), C.c_void_p(buf.data_ptr() + 4), 2 * PPB, C.byref(cnt), None))   # not 16-byte aligned
    refused(lib.pcr_read_polygon(h, 0, 1, C.byref(good), C.c_void_p(host.ctypes.data + 2), PPB, C.byref(cnt), None))     # not aligned for a pcr_point
    ctx.synchronize(); torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENT).all() and (host.view(np.uint32) == SENT).all(), "a refused call wrote into its destination"
    # 4096 vertices are accepted, and a refused call leaves the context usable
    assert lib.pcr_read_polygon(h, 0, 1, C.byref(native_polygon([[(k, k * k % 97) for k in range(4096)]])), None, 0, C.byref(cnt), None) == 0
    points_of(ctx, "synth")
    check(ctx, "synth", G.CONCAVE, 0, 2)


def test_selection_leaves_frames_statistics_and_a_pending_frame_alone(ctx):
    image = image_of("synth")
    load(ctx, image)
    points_of(ctx, "synth")
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    poly = G.CONCAVE.native()
    pts = ctx.select_polygon(poly)
    assert pts.shape[0] > 0 and ctx.polygon_stats["batches_straddling"] >= 1 and ctx.polygon_stats["batches_inside"] >= 1
    assert len(ctx.read_polygon(poly.inverted())) > 0
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    # between pcr_frame_begin and the render call, where the frame's prepass is pending
    ctx.frame_begin(p); ctx.render_basic(p)
    want, want_stats = ctx.read_framebuffer(full=True), ctx.stats()
    ctx.frame_begin(p)
    ctx.read_polygon(poly); ctx.select_polygon(poly.inverted())
    ctx.render_basic(p)
    assert np.array_equal(ctx.read_framebuffer(full=True), want) and ctx.stats() == want_stats


# ---- 6. the resource and the CLI ---------------------------------------------------------------------------------------------------------
WORLD_RINGS = [[(524.0, -10.0), (1010.0, -10.0), (1010.0, 1010.0), (524.0, 1010.0), (524.0, 600.0), (800.0, 500.0), (524.0, 400.0)],
               [(850.0, 100.0), (950.0, 100.0), (900.0, 250.0)]]                # G.CONCAVE in metres, with a triangular hole
WORLD_Z = (20.0, 45.0)


def world_reference(info, xyz):
    """The integer polygon polygon_from_world makes of WORLD_RINGS and WORLD_Z (tests/test_polygon_cpu.py checks its rounding) and
    the reference's mask over the integer rows xyz."""
    poly = P.polygon_from_world(info, WORLD_RINGS, *WORLD_Z)
    ints = G.Poly([r.tolist() for r in poly.rings], poly.z_min, poly.z_max)
    assert ints.rings[0][0] == (524_000, -10_000) and ints.rings[1][2] == (900_000, 250_000) and abs(ints.z_min - 20_000) <= 1 and abs(ints.z_max - 45_000) <= 1
    return ints, G.selected(ints, xyz)


def test_resource_points_in_polygon():
    import torch
    r = P.Renderer(160, 90)
    try:
        las = P.HuffmanLasData.create(scenes.synth_stream(600_000)[0])
        las.load_all(r)
        xyz_all, pts_all = las.points(r, world=True)
        rows = pts_all.cpu().numpy().astype(np.int64)[:, :3]
        ints, m = world_reference(las.las_info(), rows)
        m = torch.from_numpy(m).to(pts_all.device)
        xyz, pts = las.points_in_polygon(r, WORLD_RINGS, *WORLD_Z)
        assert 0 < pts.shape[0] < pts_all.shape[0]
        assert torch.equal(pts, pts_all[m]) and torch.equal(xyz, xyz_all[m]) and xyz.dtype == torch.float64
        assert torch.equal(las.points_in_polygon(r, ints.rings, ints.z_min, ints.z_max, world=False), pts_all[m])
        zm = torch.from_numpy(G.selected(ints.inverted(), rows)).to(pts_all.device)
        assert torch.equal(las.points_in_polygon(r, WORLD_RINGS, *WORLD_Z, invert=True)[1], pts_all[zm])
    finally:
        r.ctx.close()


def test_cli_polygon_round_trip(tmp_path):
    build.build_tools()
    image = scenes.synth_stream(600_000)[0]
    (tmp_path / "a.huffman").write_bytes(bytes(image.view()))
    (tmp_path / "poly.txt").write_text("\n\n".join("\n".join(f"{x!r} {y!r}" for x, y in r) for r in WORLD_RINGS) + "\n")

    def run(*cmd):
        res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        return res
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "all.las")
    res = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "in.las", "--polygon", tmp_path / "poly.txt", "--z", *(repr(v) for v in WORLD_Z))
    inv = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "out.las", "--polygon", tmp_path / "poly.txt", "--outside")
    ax, ay, az, ac, las = P.read_las(str(tmp_path / "all.las"))
    rows = np.stack([ax, ay, az], axis=1).astype(np.int64)
    ints, m = world_reference(las, rows)
    for path, mask in (("in.las", m), ("out.las", G.selected(ints.with_z(G.INT32_MIN, G.INT32_MAX).inverted(), rows))):
        bx, by, bz, bc, blas = P.read_las(str(tmp_path / path))
        assert 0 < mask.sum() < len(ax) and len(bx) == mask.sum(), res.stdout
        assert np.array_equal(bx, ax[mask]) and np.array_equal(by, ay[mask]) and np.array_equal(bz, az[mask]) and np.array_equal(bc, ac[mask])
        assert tuple(blas.scale) == tuple(las.scale) and tuple(blas.offset) == tuple(las.offset)
    assert "straddling" in res.stdout and "straddling" in inv.stdout
    # the Python path gives the same records
    r = P.Renderer(160, 90)
    try:
        hl = P.HuffmanLasData.create(image)
        hl.load_all(r)
        pts = hl.points_in_polygon(r, WORLD_RINGS, *WORLD_Z)[1].cpu().numpy()
        bx, by, bz, bc, _ = P.read_las(str(tmp_path / "in.las"))
        assert np.array_equal(pts[:, 0], bx) and np.array_equal(pts[:, 1], by) and np.array_equal(pts[:, 2], bz) and np.array_equal(pts[:, 3].view(np.uint32), bc)
    finally:
        r.ctx.close()
    # a polygon that holds no point is an error, not an empty file
    (tmp_path / "far.txt").write_text("5000 5000\n6000 5000\n6000 6000\n")
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.las"), "--polygon", str(tmp_path / "far.txt")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 1 and "no points" in res.stderr and not (tmp_path / "none.las").exists()
