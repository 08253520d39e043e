"""GPU parity of the 10-10-10 HQS method ("loop_las_hqs"): depth pass, colour sums and resolve through the C ABI against the CPU
reference (tests/las_hqs_ref.c) and the oracle, bit-exact."""
import json
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import build
from tests import las_hqs_ref, oracle, scenes
from tests.test_cli import write_las

pytestmark = pytest.mark.gpu

W, H = 640, 360
PPB = 65536


@pytest.fixture(scope="module")
def renderer():
    r = P.Renderer(W, H, device=0)
    yield r
    r.ctx.close()


def _points(total, order):
    x, y, z, c = P.synth_points(total, scenes.SEED, 0, total)
    las = P.synth_las_info(total, scenes.SEED)
    if order == "tiles":
        key = (y // 40000).astype(np.int64) * 1000 + x // 40000
        idx = np.argsort(key, kind="stable")
        x, y, z, c = x[idx], y[idx], z[idx], c[idx]
    return x, y, z, c, las


@pytest.fixture(scope="module", params=["strips", "tiles"])
def cloud(request):
    pts = _points(2_000_000, request.param)
    return pts, P.las_quantize(*pts)


def _load(renderer, pts):
    P.Runtime.reset()
    las = P.ComputeLasData.from_points(*pts)
    P.Runtime.addMethod(P.ComputeLoopLasCUDA(renderer, las))
    m = P.ComputeLoopLasHQS(renderer, las)
    P.Runtime.addMethod(m)
    P.Runtime.setSelectedMethod("loop_las_hqs")
    m.update(renderer)
    while las.state == P.Resource.LOADING:
        las.process(renderer)
    return las, m


def _reference(q, p, num_batches=None):
    batches, x12, x8, x4, rgba = q
    fb, st = las_hqs_ref.render_depth(batches, x12, x8, x4, p, num_batches=num_batches)
    rg, ba, _ = las_hqs_ref.render_color(batches, x12, x8, x4, rgba, p, fb, num_batches=num_batches)
    return fb, rg, ba, st


def _check(ctx, q, p):
    """clear -> depth -> colour -> resolve, every stage against the reference."""
    fb, rg, ba, st = _reference(q, p)
    ost = oracle.render_las(*q[:4], p)[1]
    assert st == ost
    ctx.clear()
    ctx.render_las_hqs_depth(p)
    assert ctx.stats() == ost
    gfb = ctx.read_framebuffer(full=True)
    diff = np.nonzero(gfb != fb)[0]
    assert diff.size == 0, f"{diff.size} depth words differ, first at {diff[:5]}: gpu {gfb[diff[:3]]} ref {fb[diff[:3]]}"
    ctx.render_las_hqs_color(p)
    assert ctx.stats() == ost
    grg, gba = ctx.read_accum(full=True)
    diff = np.nonzero((grg != rg) | (gba != ba))[0]
    assert diff.size == 0, f"{diff.size} sums differ, first at {diff[:5]}: gpu {grg[diff[:3]]} {gba[diff[:3]]} ref {rg[diff[:3]]} {ba[diff[:3]]}"
    assert np.array_equal(ctx.read_framebuffer(full=True), fb)          # the colour pass leaves the depth alone
    ctx.resolve_hqs(p)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_hqs(p, fb, rg, ba))
    return fb, rg, ba


@pytest.mark.parametrize("cam", ["overview", "closeup", "inside", "far"])
@pytest.mark.parametrize("cull", [0, 1])
def test_las_hqs_matches_reference(renderer, cloud, cam, cull):
    pts, q = cloud
    _load(renderer, pts)
    p = scenes.with_flags(scenes.cameras(W, H)[cam], cull=cull)
    fb, _, _ = _check(renderer.ctx, q, p)
    drawn = fb[:W * H] != np.uint64(0xFFFFFFFFFFFFFFFF)
    assert ((fb[:W * H][drawn] & np.uint64(0xFFFFFFFF)) == 0).all()
    # the depth half is the basic frame's
    ofb = oracle.render_las(*q[:4], p)[0]
    assert np.array_equal(fb >> np.uint64(32), ofb >> np.uint64(32))
    levels = [oracle.las_level(q[0][b], p) for b in range(len(q[0]) - 1)]
    expect = sum(64 + PPB * 4 * ((1 if l >= 2 else 2 if l == 1 else 3) + 1) for l in levels if l >= 0)
    assert renderer.ctx.las_algorithmic_bytes == expect           # + 4 B of colour per point after the colour pass


def test_las_hqs_windows_and_global_paths(cloud):
    """A 4096 x 4096 close-up (batches larger than the colour window: partial windows, points outside them) and a camera inside
    the cloud (batches without a window: every point on the global path)."""
    pts, q = cloud
    r = P.Renderer(4096, 4096, device=0)
    try:
        _load(r, pts)
        for cam in ("closeup", "inside"):
            _check(r.ctx, q, scenes.with_flags(scenes.cameras(4096, 4096)[cam], cull=1))
    finally:
        r.ctx.close()


def test_las_hqs_method_frame_and_progressive_loading(renderer):
    """Runtime/Method surface: Runtime.setSelectedMethod("loop_las_hqs") frames equal the direct calls; frames while the resource
    is still loading draw only complete batches but the last."""
    total = 150 * PPB + 777
    x, y, z, c = P.synth_points(total, scenes.SEED, 0, total)
    pts = (x, y, z, c, P.synth_las_info(total, scenes.SEED))
    P.Runtime.reset()
    las = P.ComputeLasData.from_points(*pts)
    P.Runtime.addMethod(P.ComputeLoopLasCUDA(renderer, las))
    P.Runtime.addMethod(P.ComputeLoopLasHQS(renderer, las))
    P.Runtime.setSelectedMethod("loop_las_hqs")
    m = P.Runtime.getSelectedMethod()
    assert (m.name, m.group) == ("loop_las_hqs", "10-10-10 bit encoded")
    renderer.set_camera(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0))
    P.Debug.frustumCullingEnabled = True
    m.update(renderer)
    q = P.las_quantize(*pts)
    loaded = []
    for _ in range(3):
        m.render(renderer)                      # process() + CLEAR + DEPTH + COLORS + RESOLVE
        loaded.append(las.numBatchesLoaded)
        fb, rg, ba, st = _reference(q, m.last_params, num_batches=las.numBatchesLoaded)
        assert renderer.ctx.stats() == st
        assert np.array_equal(renderer.ctx.read_framebuffer(full=True), fb)
        grg, gba = renderer.ctx.read_accum(full=True)
        assert np.array_equal(grg, rg) and np.array_equal(gba, ba)
        img = renderer.ctx.read_rgba()
        assert np.array_equal(img, oracle.resolve_hqs(m.last_params, fb, rg, ba))
    assert loaded == [100, 151, 151] and las.state == P.Resource.LOADED
    ctx = renderer.ctx                          # the direct calls give the same frame
    p = m.last_params
    ctx.clear(); ctx.render_las_hqs_depth(p); ctx.render_las_hqs_color(p); ctx.resolve_hqs(p)
    assert np.array_equal(ctx.read_rgba(), img)
    las.unload(renderer)


def test_las_hqs_buffer_state_across_frames_and_methods(renderer, cloud):
    """Two HQS frames with different cameras (the second must not see the first's sums), then a loop_las_cuda frame (must not
    see the HQS frame's words), then HQS again."""
    pts, q = cloud
    _load(renderer, pts)
    cams = scenes.cameras(W, H)
    _check(renderer.ctx, q, cams["closeup"])
    _check(renderer.ctx, q, cams["overview"])
    ctx = renderer.ctx
    p = cams["far"]
    ctx.clear(); ctx.render_las(p); ctx.resolve_las(p)
    ofb, ost = oracle.render_las(*q[:4], p)
    assert ctx.stats() == ost
    assert np.array_equal(ctx.read_framebuffer(full=True), ofb)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_las(p, ofb, q[4]))
    _check(renderer.ctx, q, cams["inside"])


def test_las_hqs_argument_errors(renderer):
    ctx = renderer.ctx
    ctx.las_unload()
    p = scenes.cameras(W, H)["overview"]
    for call in (ctx.render_las_hqs_depth, ctx.render_las_hqs_color):
        with pytest.raises(P.PcrError, match="no 10-10-10 data"):
            call(p)
    pts = _points(PPB, "strips")
    q = P.las_quantize(*pts)
    ctx.las_begin(PPB)
    ctx.las_upload(0, *q)
    bad_p = p.copy()
    bad_p.width = 10
    for call in (ctx.render_las_hqs_depth, ctx.render_las_hqs_color):
        with pytest.raises(P.PcrError, match="image size"):
            call(bad_p)
    ctx.clear()
    ctx.render_las_hqs_depth(p)                 # a single batch: it is the last one, nothing is drawn
    ctx.render_las_hqs_color(p)
    assert ctx.stats()["points_iterated"] == 0
    assert (ctx.read_framebuffer() == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    rg, ba = ctx.read_accum()
    assert not rg.any() and not ba.any()
    ctx.las_unload()


def test_render_cli_loop_las_hqs_matches_python(tmp_path, renderer):
    """pcr_render <file.las> --method loop_las_hqs --dump-rgba: the C++ ComputeLoopLasHQS gives the Python path's image."""
    build.build_tools()
    n = 5 * PPB + 99
    x, y, z, c = P.synth_points(n, scenes.SEED, 0, n)
    r, g, b = (c & 255).astype(np.uint16), ((c >> 8) & 255).astype(np.uint16), ((c >> 16) & 255).astype(np.uint16)
    write_las(tmp_path / "scene.las", x, y, z, r, g, b, offset=(0.0, 0.0, 0.0))
    cam = ["-0.15", "-0.57", "1500", "500", "500", "40"]
    res = subprocess.run([build.RENDER_BIN, str(tmp_path / "scene.las"), "--method", "loop_las_hqs", "--size", f"{W}x{H}",
                          "--camera", *cam, "--dump-fb", str(tmp_path / "fb.u64"), "--dump-rgba", str(tmp_path / "out.ppm")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["method"] == "loop_las_hqs" and info["batches"] == 6 and info["points_iterated"] == 5 * PPB
    # the same frame in Python
    P.Runtime.reset()
    las = P.ComputeLasData.create(str(tmp_path / "scene.las"))
    m = P.ComputeLoopLasHQS(renderer, las)
    P.Runtime.addMethod(m)
    renderer.set_camera(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0))
    P.Debug.frustumCullingEnabled = True
    m.update(renderer)
    while las.state == P.Resource.LOADING:
        m.render(renderer)
    m.render(renderer)
    img = renderer.ctx.read_rgba()
    assert np.array_equal(np.fromfile(tmp_path / "fb.u64", np.uint64), renderer.ctx.read_framebuffer())
    ppm = (tmp_path / "out.ppm").read_bytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert ppm.startswith(head)
    pix = np.frombuffer(ppm[len(head):], np.uint8).reshape(H, W, 3)[::-1].reshape(-1, 3).astype(np.uint32)
    assert np.array_equal(pix[:, 0] | (pix[:, 1] << 8) | (pix[:, 2] << 16), img & np.uint32(0xFFFFFF))
    p = m.last_params
    px, py, pz, pc, li = P.read_las(str(tmp_path / "scene.las"))
    fb, rg, ba, _ = _reference(P.las_quantize(px, py, pz, pc, li), p)
    assert np.array_equal(img, oracle.resolve_hqs(p, fb, rg, ba))
    las.unload(renderer)
