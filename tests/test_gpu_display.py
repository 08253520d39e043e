"""pcr_resolve_basic_display / _hqs_display / _las_display: n x n point size and eye-dome lighting in the resolve.

Every case first holds the GPU's framebuffer (and accumulators) against the CPU oracle's, then compares the display image with
the numpy reference of tests/display_ref.py computed from the ORACLE's buffers: byte for byte without EDL; with EDL within 1
per channel of the float64 image, equal where the response is 0, and different at all in at most 1 % of the drawn pixels
(tests/test_display_cpu.py shows the formula itself inside that cap, and that the cameras used here make every window offset
decide some pixel, fill and replace pixels, and give the HQS 1 % test neighbours to accept and to reject)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import build
from tests import display_ref as R
from tests import oracle, scenes
from tests.test_gpu_las import _load as las_load
from tests.test_gpu_las import _points as las_points
from tests.test_ref_packed import load as golden_load
from tests.test_ref_packed import params_of as golden_params

pytestmark = pytest.mark.gpu

PCR_E_ARG = -1
LAYOUTS = {"words": P.Context.LAYOUT_WORDS, "point_windows": P.Context.LAYOUT_POINT_WINDOWS}


def load(c, image):
    f = P.HuffmanFile(image)
    if c.batches_loaded:
        c.stream_unload()
    c.stream_begin(f.header(0, f.numBatches), 0)
    for i in range(f.numBatches):
        c.upload_batch(i, f.blob(i))


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    load(c, R.stream().view())
    yield c
    c.close()


def size(c, p):
    if (getattr(c, "width", 0), getattr(c, "height", 0)) != (p.width, p.height):
        c.set_image_size(p.width, p.height)


def draw_basic(c, p, ofb):
    """The basic frame of camera p in the context, held against the oracle's."""
    size(c, p)
    c.clear(); c.render_basic(p)
    assert np.array_equal(c.read_framebuffer(full=True), ofb)


def draw_hqs(c, p, ofb, org, oba):
    size(c, p)
    c.clear(); c.render_hqs_depth(p); c.render_hqs_color(p)
    assert np.array_equal(c.read_framebuffer(full=True), ofb)
    rg, ba = c.read_accum(full=True)
    assert np.array_equal(rg, org) and np.array_equal(ba, oba)


def same(got, want, what=""):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, f"{what}: {diff.size} pixels differ, first {diff[:5]}: gpu {got[diff[:3]]} reference {want[diff[:3]]}"


# ---- identity ------------------------------------------------------------------------------------------------------------------
def test_zero_opts_give_the_plain_resolve(ctx):
    p, ofb = R.basic_frame("closeup", 320, 200)
    draw_basic(ctx, p, ofb)
    ctx.resolve_basic(p)
    plain = ctx.read_rgba()
    same(plain, oracle.resolve_basic(p, ofb), "plain basic")
    ctx.resolve_basic_display(p, R.opts(4))              # (so that the image is not the plain one already)
    assert not np.array_equal(ctx.read_rgba(), plain)
    ctx.resolve_basic_display(p, R.opts())
    same(ctx.read_rgba(), plain, "basic")
    p, ofb, org, oba = R.hqs_frame("closeup", 320, 200)
    draw_hqs(ctx, p, ofb, org, oba)
    ctx.resolve_hqs(p)
    plain = ctx.read_rgba()
    same(plain, oracle.resolve_hqs(p, ofb, org, oba), "plain hqs")
    ctx.resolve_hqs_display(p, R.opts(4))
    assert not np.array_equal(ctx.read_rgba(), plain)
    ctx.resolve_hqs_display(p, R.opts(0, 0, float("nan")))      # (the strength is ignored without EDL)
    same(ctx.read_rgba(), plain, "hqs")


# ---- basic, window only --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["closeup", "overview"])
@pytest.mark.parametrize("w", R.WINDOWS)
def test_basic_window(ctx, cam, w):
    p, ofb = R.basic_frame(cam, 320, 200)
    draw_basic(ctx, p, ofb)
    ctx.resolve_basic_display(p, R.opts(w))
    same(ctx.read_rgba(), R.basic_image(p, ofb, w)[0], f"{cam} window {w}")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_basic_window_on_either_resident_layout(layout):
    c = P.Context(0)
    try:
        c.set_stream_layout(LAYOUTS[layout])
        load(c, R.stream().view())
        p, ofb = R.basic_frame("closeup", 320, 200)
        draw_basic(c, p, ofb)
        assert c.stream_layout == LAYOUTS[layout]
        c.resolve_basic_display(p, R.opts(2))
        same(c.read_rgba(), R.basic_image(p, ofb, 2)[0], layout)
    finally:
        c.close()


@pytest.mark.parametrize("cam", ["closeup", "overview"])
@pytest.mark.parametrize("wh", [(333, 77), (67, 19), (5, 3), (1, 1)])
def test_shapes(ctx, cam, wh):
    """A multiple of no tile, smaller than a tile, smaller than the window (both sides clip at once), one pixel."""
    p, ofb = R.basic_frame(cam, *wh)
    draw_basic(ctx, p, ofb)
    ctx.resolve_basic_display(p, R.opts(4))
    same(ctx.read_rgba(), R.basic_image(p, ofb, 4)[0], f"{cam} {wh}")
    p, ofb, org, oba = R.hqs_frame(cam, *wh)
    draw_hqs(ctx, p, ofb, org, oba)
    ctx.resolve_hqs_display(p, R.opts(4))
    same(ctx.read_rgba(), R.hqs_image(p, ofb, org, oba, 4)[0], f"hqs {cam} {wh}")


# ---- hqs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["closeup", "overview"])
@pytest.mark.parametrize("w", [1, 4])
def test_hqs_window(ctx, cam, w):
    p, ofb, org, oba = R.hqs_frame(cam, 320, 200)
    draw_hqs(ctx, p, ofb, org, oba)
    ctx.resolve_hqs_display(p, R.opts(w))
    same(ctx.read_rgba(), R.hqs_image(p, ofb, org, oba, w)[0], f"{cam} window {w}")


def test_hqs_window_on_the_reference_packed_bc7_stream():
    data, exp = golden_load("ref_packed_bc7")
    of = oracle.OracleFile(data)
    c = P.Context(0)
    try:
        load(c, data)
        assert c.stream_color_format() == 7
        for case in exp["cases"][:2]:
            p = golden_params(case, exp)
            ofb, org, oba = R.hqs_frame_of(of, p)
            draw_hqs(c, p, ofb, org, oba)
            for w in (1, 4):
                c.resolve_hqs_display(p, R.opts(w))
                same(c.read_rgba(), R.hqs_image(p, ofb, org, oba, w)[0], f"bc7 window {w}")
    finally:
        c.close()


# ---- las -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def las():
    """The 10-10-10 inputs of tests/test_gpu_las.py (tile order: every level occurs) in a renderer of its own, the closeup frame
    drawn and held against the oracle's."""
    pts = las_points(2_000_000, "tiles")
    q = P.las_quantize(*pts)
    r = P.Renderer(320, 200, device=0)
    _, method = las_load(r, pts)
    p = R.camera("closeup", 320, 200)
    ofb, _ = oracle.render_las(q[0], q[1], q[2], q[3], p)
    ofb.setflags(write=False)
    r.ctx.clear(); r.ctx.render_las(p)
    assert np.array_equal(r.ctx.read_framebuffer(full=True), ofb)
    yield r, p, ofb, q[4], method
    r.ctx.close()
    P.Runtime.reset()


@pytest.mark.parametrize("w", [0, 1, 4])
def test_las_window(las, w):
    r, p, ofb, rgba_points, _ = las
    r.ctx.resolve_las_display(p, R.opts(w))
    want = R.las_image(p, ofb, rgba_points, w)[0]
    same(r.ctx.read_rgba(), want, f"las window {w}")
    if w == 0:
        same(want, oracle.resolve_las(p, ofb, rgba_points), "the reference at window 0")


# ---- eye-dome lighting ---------------------------------------------------------------------------------------------------------------
def edl_cases(c, resolve, p, image_of):
    worst = 0
    for w in (0, 2):
        img, D = image_of(w)
        for e in R.EDL_WINDOWS:
            for s in R.EDL_STRENGTHS:
                resolve(p, R.opts(w, e, s))
                ref, response = R.edl(img, D, e, s)
                n = R.edl_check(c.read_rgba(), ref, response, D)
                print(f"edl window {w} edl_window {e} strength {s}: {n} of {int((D != R.EMPTY).sum())} drawn pixels differ by 1")
                worst = max(worst, n)
    return worst


@pytest.mark.parametrize("cam,wh", [("closeup", (320, 200)), ("overview", (320, 200)), ("closeup", (333, 77)), ("overview", (5, 3))])
def test_edl_basic(ctx, cam, wh):
    p, ofb = R.basic_frame(cam, *wh)
    draw_basic(ctx, p, ofb)
    edl_cases(ctx, ctx.resolve_basic_display, p, lambda w: R.basic_image(p, ofb, w))


@pytest.mark.parametrize("cam,wh", [("closeup", (320, 200)), ("overview", (333, 77))])
def test_edl_hqs(ctx, cam, wh):
    p, ofb, org, oba = R.hqs_frame(cam, *wh)
    draw_hqs(ctx, p, ofb, org, oba)
    edl_cases(ctx, ctx.resolve_hqs_display, p, lambda w: R.hqs_image(p, ofb, org, oba, w))


def test_edl_las(las):
    r, p, ofb, rgba_points, _ = las
    edl_cases(r.ctx, r.ctx.resolve_las_display, p, lambda w: R.las_image(p, ofb, rgba_points, w))


# ---- the INT64_MAX empty word --------------------------------------------------------------------------------------------------------
def test_int64_mergeable_empty_word():
    c = P.Context(0)
    try:
        c.set_int64_mergeable(True)
        load(c, R.stream().view())
        p, ofb = R.basic_frame("closeup", 333, 77)
        draw_basic(c, p, ofb)                              # (read_framebuffer shows the reference's empty word)
        img, D = R.basic_image(p, ofb, 4)
        c.resolve_basic_display(p, R.opts(4))
        same(c.read_rgba(), img, "window 4")
        c.resolve_basic_display(p, R.opts(4, 2, 0.02))
        ref, response = R.edl(img, D, 2, 0.02)
        R.edl_check(c.read_rgba(), ref, response, D)
        p, ofb, org, oba = R.hqs_frame("closeup", 333, 77)
        draw_hqs(c, p, ofb, org, oba)
        c.resolve_hqs_display(p, R.opts(4))
        same(c.read_rgba(), R.hqs_image(p, ofb, org, oba, 4)[0], "hqs window 4")
    finally:
        c.close()


# ---- debug payloads ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["show_num_points", "colorize_chunks"])
def test_debug_payloads(ctx, flag):
    p, ofb = R.basic_frame("closeup", 320, 200, **{flag: 1})
    draw_basic(ctx, p, ofb)
    ctx.resolve_basic_display(p, R.opts(1))
    want = R.basic_image(p, ofb, 1)[0]
    same(ctx.read_rgba(), want, flag)
    assert not np.array_equal(want, R.basic_image(R.camera("closeup", 320, 200), ofb, 1)[0]), "the flag changes nothing"
    p, ofb, org, oba = R.hqs_frame("closeup", 320, 200, **{flag: 1})
    draw_hqs(ctx, p, ofb, org, oba)
    ctx.resolve_hqs_display(p, R.opts(1))
    same(ctx.read_rgba(), R.hqs_image(p, ofb, org, oba, 1)[0], "hqs " + flag)


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def test_the_call_writes_the_image_only(ctx):
    p, ofb, org, oba = R.hqs_frame("closeup", 320, 200)
    size(ctx, p)
    ctx.frame_begin(p, hqs=True); ctx.render_hqs_depth(p); ctx.render_hqs_color(p)
    stats = ctx.stats()
    ctx.resolve_hqs_display(p, R.opts(4, 2, 0.02))
    ctx.resolve_basic_display(p, R.opts(2, 1, 0.0005))
    assert np.array_equal(ctx.read_framebuffer(full=True), ofb)
    rg, ba = ctx.read_accum(full=True)
    assert np.array_equal(rg, org) and np.array_equal(ba, oba) and ctx.stats() == stats
    # the next frame, begun through the tile-tracked clear, and its plain resolve
    ctx.frame_begin(p); ctx.render_basic(p); ctx.resolve_basic(p)
    pfb = R.basic_frame("closeup", 320, 200)[1]
    assert np.array_equal(ctx.read_framebuffer(full=True), pfb)
    same(ctx.read_rgba(), oracle.resolve_basic(p, pfb), "the plain frame after")


def test_methods_display_attribute():
    """HuffmanMemIter / HuffmanHQS with `display` set draw the reference image of the direct call; without it the plain one."""
    lod, cull = P.Debug.LOD, P.Debug.frustumCullingEnabled
    P.Runtime.reset()
    r = P.Renderer(320, 200)
    try:
        P.Debug.LOD, P.Debug.frustumCullingEnabled = 1.0, True
        las = P.HuffmanLasData.create(R.stream())
        basic, hqs = P.HuffmanMemIter(r, las), P.HuffmanHQS(r, las)
        assert basic.display is None and hqs.display is None
        p, ofb = R.basic_frame("closeup", 320, 200)
        r.params_override = p
        basic.update(r)
        basic.render(r)
        assert las.numBatchesLoaded == R.oracle_file().num_batches
        same(r.ctx.read_rgba(), oracle.resolve_basic(p, ofb), "plain")
        basic.display = R.opts(2, 1, 0.0)                 # (strength 0: shade 1, so the image is exact; byte 3 is cleared)
        basic.render(r)
        assert np.array_equal(r.ctx.read_framebuffer(full=True), ofb)
        img, D = R.basic_image(p, ofb, 2)
        same(r.ctx.read_rgba(), np.where(D != R.EMPTY, img & np.uint32(0xFFFFFF), img), "basic display")
        assert hqs.display is None
        p, ofb, org, oba = R.hqs_frame("closeup", 320, 200)
        hqs.display = R.opts(4)
        hqs.update(r)
        hqs.render(r)
        same(r.ctx.read_rgba(), R.hqs_image(p, ofb, org, oba, 4)[0], "hqs display")
        las.unload(r)
    finally:
        P.Debug.LOD, P.Debug.frustumCullingEnabled = lod, cull
        r.ctx.close()
        P.Runtime.reset()


def test_las_methods_display_attribute(las):
    r, p, ofb, rgba_points, _ = las
    lod, cull = P.Debug.LOD, P.Debug.frustumCullingEnabled
    try:
        P.Debug.LOD, P.Debug.frustumCullingEnabled = 1.0, True
        r.params_override = p
        m = las[4]
        assert isinstance(m, P.ComputeLoopLasCUDA) and m.display is None
        m.display = R.opts(4)
        m.render(r)
        same(r.ctx.read_rgba(), R.las_image(p, ofb, rgba_points, 4)[0], "loop_las_cuda display")
        m.display = None
        h = P.ComputeLoopLasHQS(r, m.las)
        h.display = R.opts(1, 2, 0.02)
        h.render(r)
        got = r.ctx.read_rgba()
        r.ctx.resolve_hqs_display(p, h.display)
        same(got, r.ctx.read_rgba(), "loop_las_hqs display against the direct call")
        r.ctx.resolve_hqs(p)
        assert not np.array_equal(got, r.ctx.read_rgba())
    finally:
        P.Debug.LOD, P.Debug.frustumCullingEnabled = lod, cull
        r.params_override = None
        r.ctx.clear(); r.ctx.render_las(p)                 # (the fixture's frame, for whoever comes next)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_image(ctx, las):
    p, ofb = R.basic_frame("closeup", 320, 200)
    draw_basic(ctx, p, ofb)
    ctx.resolve_basic_display(p, R.opts(1))
    before = ctx.read_rgba()
    lib, h = ctx.lib, ctx.h
    bad_size = p.copy(); bad_size.width = 13
    calls = [(p, None, "NULL")]
    calls += [(p, R.opts(w), "window") for w in (-1, 5)]
    calls += [(p, R.opts(0, e, 0.001), "edl_window") for e in (-1, 3)]
    calls += [(p, R.opts(1, 1, s), "edl_strength") for s in (float("nan"), float("inf"), -float("inf"), -0.001)]
    calls += [(p, R.opts(1, 0, 0.0, reserved=1), "reserved"), (None, R.opts(1), "params"), (bad_size, R.opts(1), "image size")]
    for fn in (lib.pcr_resolve_basic_display, lib.pcr_resolve_hqs_display):
        for q, o, word in calls:
            rc = fn(h, C.byref(q) if q is not None else None, C.byref(o) if o is not None else None)
            msg = (lib.pcr_last_error(h) or b"").decode()
            assert rc == PCR_E_ARG and word in msg, (word, rc, msg)
            same(ctx.read_rgba(), before, word)
    # the 10-10-10 call refuses what pcr_resolve_las refuses: no 10-10-10 data in this context
    rc = lib.pcr_resolve_las_display(h, C.byref(p), C.byref(R.opts(1)))
    assert rc == PCR_E_ARG and "10-10-10" in (lib.pcr_last_error(h) or b"").decode()
    same(ctx.read_rgba(), before, "las")
    r = las[0]
    for o, word in ((None, "NULL"), (R.opts(5), "window"), (R.opts(0, 1, float("nan")), "edl_strength")):
        rc = r.ctx.lib.pcr_resolve_las_display(r.ctx.h, C.byref(las[1]), C.byref(o) if o is not None else None)
        assert rc == PCR_E_ARG and word in (r.ctx.lib.pcr_last_error(r.ctx.h) or b"").decode()
    with pytest.raises(P.PcrError, match="window"):
        ctx.resolve_basic_display(p, R.opts(9))


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
def test_render_cli_dumps_the_display_image(ctx, tmp_path):
    build.build_tools()
    W, H = 320, 200
    path = tmp_path / "scene.huffman"
    path.write_bytes(bytes(R.stream().view()))
    cam = (-1.68, -0.39, 70.0, 300.0, 20.0, 45.0)          # scenes.cameras: closeup
    res = subprocess.run([build.RENDER_BIN, str(path), "--size", f"{W}x{H}", "--camera", *(repr(v) for v in cam), "--lod", "1.0", "--cull", "1",
                          "--window", "2", "--edl", "0.0005", "--dump-rgba", str(tmp_path / "o.ppm")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    p, ofb = R.basic_frame("closeup", W, H)
    assert bytes(p) == bytes(scenes.with_flags(P.camera_orbit(cam[0], cam[1], cam[2], cam[3:], W, H), lod_percent=100, cull=1))
    draw_basic(ctx, p, ofb)
    ctx.resolve_basic_display(p, R.opts(2, 1, 0.0005))
    want = R.channels(ctx.read_rgba().reshape(H, W))[::-1, :, :3].astype(np.uint8)     # the PPM's row 0 is the image's last
    raw = (tmp_path / "o.ppm").read_bytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + W * H * 3
    assert np.array_equal(np.frombuffer(raw, np.uint8, offset=len(head)).reshape(H, W, 3), want)
    plain = R.channels(oracle.resolve_basic(p, ofb).reshape(H, W))[::-1, :, :3].astype(np.uint8)
    assert not np.array_equal(want, plain)
