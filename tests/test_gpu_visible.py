"""pcr_select_visible / pcr_read_visible: the points that make up the picture, selected on the GPU.

The reference of every comparison is tests/visible_cases.py's numpy restatement of the definitions over Context.read_screen(p,
None) -- the screen selection of the whole image, which tests/test_gpu_screen.py pins to the oracle's trace. Every comparison is
byte equality. Every case runs for a context loaded with PCR_LAYOUT_WORDS and one loaded with PCR_LAYOUT_POINT_WINDOWS, before
and after a first frame. tests/test_visible_cpu.py proves on the CPU that the cases make every rule decide: several hits that
share front depth and colour (tie_all: 415 pixels), the f64 rule against the f32 product (edge_64: 1037 hits, edge_double: 966),
dilation that changes the selection and leaves covered pixels without a hit (tie_64), dilation that changes nothing (edge_64),
hits in the framebuffer's extra row, past the planes of the image (extra_row).
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import contention as K
from tests import screen_cases as SC
from tests import visible_cases as V
from tests.test_gpu_screen import EMPTY_RECTS, LAYOUTS

pytestmark = pytest.mark.gpu

PCR_E_ARG = -1
U32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    yield c
    c.close()


def load(c, sname, p, frame=True):
    """tests/test_gpu_screen.py's load for the streams of tests/visible_cases.py: the stream resident, the image sized for the
    camera; frame: one HQS depth frame drawn first."""
    f = P.HuffmanFile(V.stream(sname))
    if c.batches_loaded:
        c.stream_unload()
    c.stream_begin(f.header(0, f.numBatches), 0)
    for i in range(f.numBatches):
        c.upload_batch(i, f.blob(i))
    c.set_image_size(p.width, p.height)
    if frame:
        c.clear(); c.render_hqs_depth(p); c.synchronize()
    return f


_REFERENCES = {}


def reference(c, name, p):
    """The case's Reference over read_screen(p, None) and the batch counts of that call; worked out once and shared (the screen
    selection is the same bytes whatever the layout and whenever it is made)."""
    pts, hits = c.read_screen(p, None)
    batches = {k: c.screen_stats[k] for k in ("batches_skipped", "batches_decoded")}
    if name not in _REFERENCES:
        _REFERENCES[name] = (pts.tobytes(), hits.tobytes(), V.Reference(pts, hits, p), batches)
    want = _REFERENCES[name]
    assert pts.tobytes() == want[0] and hits.tobytes() == want[1] and batches == want[3]
    return want[2], batches


def check_call(c, R, batches, p, rect, mode, radius):
    pts, hits, plane = c.read_visible(p, rect, mode, radius, depth=True)
    st = dict(c.visible_stats)
    sel, want = R.select(rect, mode, radius)
    what = (mode, radius, rect)
    assert pts.dtype == P.POINT_DTYPE and hits.dtype == P.HIT_DTYPE and plane.dtype == np.uint32 and plane.shape == (p.height, p.width)
    assert len(pts) == len(hits) == want["selected"], what
    assert hits.tobytes() == R.hits[sel].tobytes(), f"{what}: other hits selected than the reference names"
    assert pts.tobytes() == R.pts[sel].tobytes(), f"{what}: the records differ"
    assert plane.tobytes() == R.plane(radius).tobytes(), f"{what}: the depth plane differs"
    assert st == dict(batches, **want), what
    return pts, hits, plane


# ---- 1: every case x mode x radius x rect ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.CASES))
def test_selection_equals_the_definitions_over_read_screen(ctx, name):
    import torch
    sname, of, p = V.case(name)
    load(ctx, sname, p, frame=False)
    R, batches = reference(ctx, name, p)
    rects = V.rects(p)
    for mode in V.MODES:                                    # before any frame
        for radius in (0, 2):
            check_call(ctx, R, batches, p, None, mode, radius)
        check_call(ctx, R, batches, p, rects["border"], mode, 8)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.synchronize()
    for mode in V.MODES:
        for radius in V.RADII:
            for rect in rects.values():
                check_call(ctx, R, batches, p, rect, mode, radius)
    # the torch route returns the same bytes; the mode by its number; the radius-0 plane is the front depth
    pts, hits, plane = check_call(ctx, R, batches, p, rects["inner"], "front", 1)
    tp, th, td = ctx.select_visible(p, rects["inner"], P.VISIBLE_FRONT, 1, depth=True)
    assert tp.dtype == torch.int32 and th.dtype == torch.int64 and td.dtype == torch.int32
    assert tuple(tp.shape) == (len(pts), 4) and tuple(th.shape) == (len(pts), 2) and tuple(td.shape) == (p.height, p.width)
    assert tp.cpu().numpy().tobytes() == pts.tobytes() and th.cpu().numpy().tobytes() == hits.tobytes() and td.cpu().numpy().tobytes() == plane.tobytes()
    assert len(ctx.select_visible(p, rects["inner"], "surface", 1)) == 2
    assert ctx.read_visible(p, None, "front", 0, depth=True)[2].tobytes() == R.front_depth.tobytes()


def test_dilation_does_nothing_where_the_cpu_test_says_so(ctx):
    sname, of, p = V.case("edge_64")
    load(ctx, sname, p)
    got = [ctx.read_visible(p, None, "surface", radius) for radius in V.RADII]
    assert len(got[0][0]) == 196039
    for pts, hits in got[1:]:
        assert pts.tobytes() == got[0][0].tobytes() and hits.tobytes() == got[0][1].tobytes()


# ---- 2: FRONT at radius 0 is the basic method's frame ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tie_all", "tie_64", "edge_64", "synth_cull", "garbage_tail", "extra_row"])
def test_front_is_the_frame_render_basic_leaves(ctx, name):
    sname, of, p = V.case(name)
    load(ctx, sname, p)
    ctx.clear(); ctx.render_basic(p)
    fb = ctx.read_framebuffer()
    assert len(fb) == p.width * p.height
    pts, hits = ctx.read_visible(p, None, "front", 0)
    assert ctx.visible_stats["selected"] == len(pts) == int((fb != K.EMPTY).sum()) > 0
    assert len(np.unique(hits["pixel"])) == len(hits)
    assert np.array_equal(SC.key_of(hits["depth_bits"], pts["color"]), fb[hits["pixel"]])


# ---- 3: a one-pixel rect is pcr_pick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [SC.PICK_CASE, "tie_all_bc7", "tie_64"])
def test_front_of_a_one_pixel_rect_is_pick(ctx, name):
    sname, of, p = V.case(name)
    load(ctx, sname, p)
    R, _ = reference(ctx, name, p)
    covered = np.nonzero(R.front_depth.reshape(-1) != V.NONE)[0]
    empty = np.nonzero(R.front_depth.reshape(-1) == V.NONE)[0]
    assert len(covered) and len(empty)
    rng = np.random.default_rng(12)
    pixels = [int(v) for v in rng.choice(covered, 24, replace=False)] + [int(v) for v in rng.choice(empty, 4, replace=False)]
    if name == SC.PICK_CASE:
        pixels.append(SC.PICK_TIE[0] + SC.PICK_TIE[1] * p.width)
    found = 0
    for pix in pixels:
        px, py = pix % p.width, pix // p.width
        want = ctx.pick(p, px, py, 0)
        pts, hits = ctx.read_visible(p, (px, py, px, py), "front", 0)
        if want is None:
            assert len(pts) == 0, (px, py)
            continue
        assert len(pts) == 1 and bytes(want[0]) == pts[0].tobytes() and bytes(want[1]) == hits[0].tobytes(), (px, py)
        found += 1
    assert found >= 24


# ---- 4: SURFACE at radius 0 is what the HQS colour pass averages -------------------------------------------------------------------
@pytest.mark.parametrize("name", V.ACCUM_CASES)
def test_surface_is_what_the_hqs_colour_pass_sums(ctx, name):
    sname, of, p = V.case(name)
    load(ctx, sname, p)
    ctx.clear(); ctx.render_hqs_depth(p)
    fb = ctx.read_framebuffer()
    ctx.render_hqs_color(p)
    rg, ba = ctx.read_accum()
    pts, hits, plane = ctx.read_visible(p, None, "surface", 0, depth=True)
    n = p.width * p.height
    assert plane.tobytes() == (fb[:n] >> np.uint64(32)).astype(np.uint32).tobytes(), "the depth plane is not the HQS depth frame's high halves"
    pix = hits["pixel"].astype(np.int64)
    colour = pts["color"].astype(np.uint64)
    sums = [np.zeros(n, np.uint64) for _ in range(4)]
    for s, v in zip(sums, (colour & np.uint64(255), (colour >> np.uint64(8)) & np.uint64(255), (colour >> np.uint64(16)) & np.uint64(255), np.ones(len(pix), np.uint64))):
        np.add.at(s, pix, v)
    assert np.array_equal(sums[3], ba[:n] & U32), "per-pixel counts differ from the accumulator's"
    assert np.array_equal(sums[0], rg[:n] >> np.uint64(32)) and np.array_equal(sums[1], rg[:n] & U32) and np.array_equal(sums[2], ba[:n] >> np.uint64(32))
    assert len(pts) > 0


# ---- 5: the contract ---------------------------------------------------------------------------------------------------------------
def raw(c, fn, p, rect, mode, radius, points, hits, depth, capacity, stats=True):
    cnt, st = C.c_int64(-5), N.VisibleStats()
    r = P.as_rect(rect)
    rc = getattr(c.lib, fn)(c.h, C.byref(p), C.byref(r) if r is not None else None, mode, radius, points, hits, depth, capacity, C.byref(cnt),
                            C.byref(st) if stats else None)
    return rc, cnt.value, st.as_dict()


def test_counts_capacity_and_null_pointers(ctx):
    import torch
    name, mode, radius = "synth_cull", "surface", 1
    sname, of, p = V.case(name)
    load(ctx, sname, p)
    R, batches = reference(ctx, name, p)
    rect = V.rects(p)["inner"]
    pts, hits, plane = check_call(ctx, R, batches, p, rect, mode, radius)
    n, m, npix = len(pts), V.MODES[mode], p.width * p.height
    assert n > 1000
    # count-only equals the written count, with and without stats
    rc, cnt, st = raw(ctx, "pcr_select_visible", p, rect, m, radius, None, None, None, 0)
    assert (rc, cnt) == (0, n) and st == ctx.visible_stats
    assert raw(ctx, "pcr_read_visible", p, rect, m, radius, None, None, None, 0, stats=False)[:2] == (0, n)
    # a capacity one below: PCR_E_ARG, the count, nothing written -- host
    hp, hh, hd = np.full(n * 16, 0x5A, np.uint8), np.full(n * 16, 0xA5, np.uint8), np.full(npix, 0x5A5A5A5A, np.uint32)
    rc, cnt, _ = raw(ctx, "pcr_read_visible", p, rect, m, radius, hp.ctypes.data, hh.ctypes.data, hd.ctypes.data, n - 1)
    assert rc == PCR_E_ARG and cnt == n and (hp == 0x5A).all() and (hh == 0xA5).all() and (hd == 0x5A5A5A5A).all()
    assert b"capacity" in ctx.lib.pcr_last_error(ctx.h)
    # ... and device
    dp = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dh = torch.full((n, 2), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    dd = torch.full((npix,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc, cnt, _ = raw(ctx, "pcr_select_visible", p, rect, m, radius, ptr(dp), ptr(dh), ptr(dd), n - 1)
    assert rc == PCR_E_ARG and cnt == n
    assert bool((dp == 0x5A5A5A5A).all()) and bool((dh == 0x5A5A5A5A).all()) and bool((dd == 0x5A5A5A5A).all())
    # each pointer alone; the exact capacity is enough
    rc, cnt, _ = raw(ctx, "pcr_select_visible", p, rect, m, radius, ptr(dp), None, None, n)
    assert (rc, cnt) == (0, n) and dp.cpu().numpy().tobytes() == pts.tobytes() and bool((dh == 0x5A5A5A5A).all()) and bool((dd == 0x5A5A5A5A).all())
    rc, cnt, _ = raw(ctx, "pcr_select_visible", p, rect, m, radius, None, ptr(dh), None, n)
    assert (rc, cnt) == (0, n) and dh.cpu().numpy().tobytes() == hits.tobytes() and bool((dd == 0x5A5A5A5A).all())
    dp.fill_(0x5A5A5A5A); torch.cuda.synchronize()
    rc, cnt, _ = raw(ctx, "pcr_select_visible", p, rect, m, radius, None, None, ptr(dd), 0)            # (the capacity does not matter without records)
    assert (rc, cnt) == (0, n) and dd.cpu().numpy().tobytes() == plane.tobytes() and bool((dp == 0x5A5A5A5A).all())
    hp[:] = 0x5A
    rc, cnt, _ = raw(ctx, "pcr_read_visible", p, rect, m, radius, None, hh.ctypes.data, None, n)
    assert (rc, cnt) == (0, n) and hh.tobytes() == hits.tobytes() and (hp == 0x5A).all()
    rc, cnt, _ = raw(ctx, "pcr_read_visible", p, rect, m, radius, hp.ctypes.data, None, hd.ctypes.data, n + 7)
    assert (rc, cnt) == (0, n) and hp.tobytes() == pts.tobytes() and hd.tobytes() == plane.tobytes()


def test_refusals(ctx):
    import torch
    sname, of, p = V.case("synth_cull")
    load(ctx, sname, p)
    dd = torch.zeros(p.width * p.height + 4, dtype=torch.int32, device="cuda")
    dp = torch.zeros((1 << 19, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ok = lambda **kw: dict(dict(p=p, rect=None, mode=P.VISIBLE_SURFACE, radius=0, points=None, hits=None, depth=None, capacity=0), **kw)
    other = p.copy(); other.width += 1
    ppt = p.copy(); ppt.points_per_thread = 32
    bad = [ok(mode=2), ok(mode=-1), ok(radius=-1), ok(radius=P.VISIBLE_MAX_RADIUS + 1), ok(depth=C.c_void_p(dd.data_ptr() + 2)),
           ok(points=C.c_void_p(dp.data_ptr() + 4), capacity=1 << 19), ok(hits=C.c_void_p(dp.data_ptr() + 8), capacity=1 << 19), ok(p=other), ok(p=ppt)]
    for kw in bad:
        rc, cnt, _ = raw(ctx, "pcr_select_visible", **kw)
        assert rc == PCR_E_ARG and cnt == 0 and ctx.lib.pcr_last_error(ctx.h), kw
    for kw in bad[:4] + bad[7:]:
        assert raw(ctx, "pcr_read_visible", **kw)[0] == PCR_E_ARG, kw
    hd = np.zeros(p.width * p.height + 1, np.uint32)
    assert raw(ctx, "pcr_read_visible", **ok(depth=hd.ctypes.data + 1))[0] == PCR_E_ARG
    r = P.as_rect((0, 0, 5, 5))
    assert ctx.lib.pcr_select_visible(ctx.h, C.byref(p), C.byref(r), 0, 0, None, None, None, 0, None, None) == PCR_E_ARG          # out_count NULL
    for mode, radius in (("nearest", 0), ("front", 9), ("surface", -1), (5, 0)):
        with pytest.raises((P.PcrError, ValueError)):
            ctx.read_visible(p, None, mode, radius)
    assert raw(ctx, "pcr_select_visible", **ok(radius=P.VISIBLE_MAX_RADIUS))[0] == 0


def test_empty_rects_and_empty_contexts_select_nothing(ctx):
    name = "synth_far_lod"
    sname, of, p = V.case(name)
    load(ctx, sname, p)
    R, batches = reference(ctx, name, p)
    for rect in EMPTY_RECTS:
        for mode in V.MODES:
            pts, hits, plane = check_call(ctx, R, batches, p, rect, mode, 2)      # (the image's counts and the plane all the same)
            assert len(pts) == 0 and ctx.visible_stats["candidates"] == 0 and ctx.visible_stats["hits"] == len(R.pix)
    ctx.stream_unload()
    f = P.HuffmanFile(SC.stream(sname))
    ctx.stream_begin(f.header(0, f.numBatches), 0)                         # a stream with no batch resident yet
    pts, hits, plane = ctx.read_visible(p, None, "front", 1, depth=True)
    assert len(pts) == 0 and len(hits) == 0 and (plane == V.NONE).all() and set(ctx.visible_stats.values()) == {0}


@pytest.mark.parametrize("name", ["synth_cull", "tie_all_bc7"])
def test_frames_and_statistics_are_left_alone(ctx, name):
    """The framebuffer and the render statistics are unchanged by a call; with the call between pcr_frame_begin and the render
    call, for this camera and for another, the frame is still the oracle's."""
    sname, of, p = V.case(name)
    load(ctx, sname, p, frame=False)
    bc7 = ctx.stream_color_format() == 7
    other = V.case("synth_far_lod")[2].copy()
    other.width, other.height = p.width, p.height
    want = (of.render_hqs_depth(p) if bc7 else of.render_basic(p))[0]

    def draw():
        (ctx.render_hqs_depth if bc7 else ctx.render_basic)(p)
        stats = ctx.stats()
        return ctx.read_framebuffer(full=True), stats
    ctx.frame_begin(p, hqs=bc7)
    plain, plain_stats = draw()
    assert np.array_equal(plain, want)
    for mode in V.MODES:
        ctx.read_visible(p, V.rects(p)["inner"], mode, 2, depth=True)
        ctx.select_visible(other, None, mode, 1)
        assert np.array_equal(ctx.read_framebuffer(full=True), plain), "a call changed the framebuffer"
        assert ctx.stats() == plain_stats, "a call changed the render statistics"
    for q, mode in ((p, "front"), (other, "surface")):
        ctx.frame_begin(p, hqs=bc7)
        ctx.read_visible(q, None, mode, 1, depth=True)
        fb, stats = draw()
        assert np.array_equal(fb, want), "a call between frame_begin and the render call changed the frame"
        assert stats == plain_stats


# ---- 6: repeatability ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(V.MODES))
def test_two_identical_calls_give_identical_bytes(ctx, mode):
    sname, of, p = V.case("tie_64")
    load(ctx, sname, p)
    rect = V.rects(p)["border"]
    a = ctx.read_visible(p, rect, mode, 2, depth=True)
    sa = dict(ctx.visible_stats)
    ctx.read_visible(p, None, "surface" if mode == "front" else "front", 8, depth=True)      # (another call in between: the planes are reused)
    b = ctx.read_visible(p, rect, mode, 2, depth=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and sa == ctx.visible_stats and len(a[0]) > 0


# ---- upper layers ------------------------------------------------------------------------------------------------------------------
def test_visible_points_of_the_resource():
    import torch
    sname, of, p = V.case("synth_cull")
    rect = V.rects(p)["inner"]
    r = P.Renderer(p.width, p.height)
    d = P.HuffmanLasData.create(SC.stream(sname))
    d.load_all(r)
    want_pts, want_hits = r.ctx.read_visible(p, rect, "surface", 1)
    xyz, pts, hits = d.visible_points(r, p, rect, "surface", 1)
    assert len(want_pts) > 1000
    assert pts.cpu().numpy().tobytes() == want_pts.tobytes() and hits.cpu().numpy().tobytes() == want_hits.tobytes()
    info = d.las_info()
    want_xyz = np.stack([want_pts[k].astype(np.float64) * info.scale[i] + info.offset[i] for i, k in enumerate("xyz")], axis=1)
    assert xyz.dtype == torch.float64 and np.array_equal(xyz.cpu().numpy(), want_xyz)
    pts2, hits2 = d.visible_points(r, p, rect, world=False)
    want_pts, want_hits = r.ctx.read_visible(p, rect, "front", 0)
    assert pts2.cpu().numpy().tobytes() == want_pts.tobytes() and hits2.cpu().numpy().tobytes() == want_hits.tobytes()
    r.ctx.close()


def test_cli_decode_view_visible_writes_the_selection(tmp_path):
    from tests.test_gpu_screen import VIEW, cli_case
    build.build_tools()
    sname, p = cli_case()
    rect = (40, 30, 250, 170)
    src, out = tmp_path / "in.huffman", tmp_path / "out.las"
    src.write_bytes(bytes(SC.stream(sname)))
    res = subprocess.run([build.DECODE_BIN, str(src), str(out), "--view", *VIEW, "--rect", *(str(v) for v in rect), "--visible", "front", "--occluder", "1"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    c = P.Context(0)
    try:
        load(c, sname, p, frame=False)
        pts, hits = c.read_visible(p, rect, "front", 1)
        everything = len(c.read_screen(p, rect)[0])
    finally:
        c.close()
    assert 100 < len(pts) < everything
    x, y, z, colour, las = P.read_las(str(out))
    assert len(x) == len(pts)
    assert np.array_equal(x, pts["x"]) and np.array_equal(y, pts["y"]) and np.array_equal(z, pts["z"]) and np.array_equal(colour, pts["color"])
