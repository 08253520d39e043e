"""The host forms of the selection calls over more than one piece of the staging buffers: pcr_read_polygon, pcr_read_slabs,
pcr_read_height, pcr_read_screen and pcr_read_visible walk their batches through the stages in pieces (kept_write in pcr_api.hip;
pcr_read_box over several pieces is tests/test_gpu_select.py::test_twenty_million_points).

One stream of 9 000 000 synthetic points, 138 batches, loaded once per layout. For every call the host form equals the device form
of the same call brought to the host, byte for byte; the device forms are held against the oracles by the modules of each call.
Every predicate selects a proper, non-empty subset, and the call's own statistics show more than 128 batches walked -- the whole
range for polygon and slabs, which have to hold all three classes of batch, the listed or decoded batches for height, screen and
visible -- which is three pieces or more with a short last one, whether a piece is 32 batches or 64."""
import pytest

import pcrhpg24_amd as P
from tests import scenes

pytestmark = pytest.mark.gpu

PPB = 65536
BATCHES = 138
W, H = 160, 90
LAYOUTS = {"words": P.Context.LAYOUT_WORDS, "point_windows": P.Context.LAYOUT_POINT_WINDOWS}


@pytest.fixture(scope="module")
def image():
    return scenes.synth_stream(9_000_000)[0]


@pytest.fixture(scope="module", params=list(LAYOUTS))
def ctx(request, image):
    f = P.HuffmanFile(image.view())
    assert f.numBatches == BATCHES
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(W, H)
    c.stream_begin(f.header())
    c.upload_batches(0, [f.blob(b) for b in range(f.numBatches)])
    c.clear(); c.render_hqs_depth(camera()); c.synchronize()
    yield c
    c.close()


def camera():
    """The whole tile in view, every point walked: level of detail 100 %, no culling."""
    return scenes.with_flags(P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), W, H), lod_percent=100, cull=0)


def same(host, dev):
    """A host result (numpy) and the device result (torch) of the same call: the same bytes."""
    d = dev.cpu().numpy()
    assert host.nbytes == d.nbytes, f"{len(host)} rows on the host, {len(d)} on the device"
    assert host.tobytes() == d.tobytes()


def check_classes(st):
    print(st)
    assert st["batches_outside"] > 0 and st["batches_inside"] > 0 and st["batches_straddling"] > 0
    assert st["batches_outside"] + st["batches_inside"] + st["batches_straddling"] == BATCHES > 128
    assert 0 < st["points_selected"] < BATCHES * PPB


def test_read_polygon(ctx):
    poly = P.Polygon([(100_000, 100_000), (900_000, 150_000), (800_000, 900_000), (150_000, 700_000)])
    host = ctx.read_polygon(poly)
    check_classes(ctx.polygon_stats)
    assert len(host) == ctx.polygon_stats["points_selected"]
    same(host, ctx.select_polygon(poly))


def test_read_slabs(ctx):
    slabs = [P.Slab((1, 1, 0), 500_000, 1_300_000), P.Slab((1, -1, 0), -600_000, 500_000)]      # two diagonal bands across the tile
    host = ctx.read_slabs(slabs)
    check_classes(ctx.slab_stats)
    assert len(host) == ctx.slab_stats["points_selected"]
    same(host, ctx.select_slabs(slabs))


def test_read_height(ctx):
    import torch
    grid = (0, 0, 2000, 500, 500)                                               # 2 m cells over the whole kilometre
    cx = torch.arange(500, dtype=torch.int32, device=torch.device("cuda", ctx.device))
    ground = (cx * 40).repeat(500, 1).contiguous()                              # a plane that rises 20 m from west to east
    pts, hts = ctx.read_height(grid, ground, 2_000, 30_000, heights=True)
    st = dict(ctx.height_stats)
    print(st)
    assert st["batches_decoded"] > 128 and 0 < st["points_selected"] < BATCHES * PPB and len(pts) == len(hts) == st["points_selected"]
    dp, dh = ctx.select_height(grid, ground, 2_000, 30_000, heights=True)
    same(pts, dp)
    same(hts, dh)


def test_read_screen(ctx):
    p, rect = camera(), (0, 0, W // 2 - 1, H - 1)                          # the left half of the image: about half the tile
    pts, hits = ctx.read_screen(p, rect)
    st = dict(ctx.screen_stats)
    print(st)
    assert st["batches_decoded"] > 128 and 0 < st["points_selected"] < BATCHES * PPB and len(pts) == len(hits) == st["points_selected"]
    dp, dh = ctx.select_screen(p, rect)
    same(pts, dp)
    same(hits, dh)


@pytest.mark.parametrize("mode", ["front", "surface"])
def test_read_visible(ctx, mode):
    p, rect = camera(), (0, 0, W // 2 - 1, H - 1)                          # the left half of the image: about half the tile
    pts, hits = ctx.read_visible(p, rect, mode, 1)
    st = dict(ctx.visible_stats)
    print(st)
    assert st["batches_decoded"] > 128 and 0 < st["selected"] < st["hits"] and len(pts) == len(hits) == st["selected"]
    dp, dh = ctx.select_visible(p, rect, mode, 1)
    same(pts, dp)
    same(hits, dh)
