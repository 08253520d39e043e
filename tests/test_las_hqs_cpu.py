"""CPU reference of the 10-10-10 HQS method ("loop_las_hqs", tests/las_hqs_ref.c): pinned to the oracle's 10-10-10 renderer,
and its colour sums checked for consistency. No GPU."""
import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import las_hqs_ref, oracle, scenes

W, H = 640, 360
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _points(total, order):
    x, y, z, c = P.synth_points(total, scenes.SEED, 0, total)
    las = P.synth_las_info(total, scenes.SEED)
    if order == "tiles":          # the clouds of test_gpu_las.py
        key = (y // 40000).astype(np.int64) * 1000 + x // 40000
        idx = np.argsort(key, kind="stable")
        x, y, z, c = x[idx], y[idx], z[idx], c[idx]
    return x, y, z, c, las


@pytest.fixture(scope="module", params=["strips", "tiles"])
def cloud(request):
    return P.las_quantize(*_points(2_000_000, request.param))


@pytest.mark.parametrize("cam", ["overview", "closeup", "inside", "far"])
@pytest.mark.parametrize("cull", [0, 1])
def test_depth_pass_is_the_oracle_frame_without_index(cloud, cam, cull):
    batches, x12, x8, x4, _ = cloud
    p = scenes.with_flags(scenes.cameras(W, H)[cam], cull=cull)
    fb, st = las_hqs_ref.render_depth(batches, x12, x8, x4, p)
    ofb, ost = oracle.render_las(batches, x12, x8, x4, p)
    assert st == ost
    drawn = ofb != EMPTY
    assert drawn.any()
    expect = np.where(drawn, ofb & np.uint64(0xFFFFFFFF00000000), ofb)
    assert np.array_equal(fb, expect)


@pytest.mark.parametrize("cam", ["overview", "closeup", "inside", "far"])
def test_colour_sums_are_consistent(cloud, cam):
    batches, x12, x8, x4, rgba = cloud
    p = scenes.with_flags(scenes.cameras(W, H)[cam], cull=1)
    fb, _ = las_hqs_ref.render_depth(batches, x12, x8, x4, p)
    rg, ba, st = las_hqs_ref.render_color(batches, x12, x8, x4, rgba, p, fb)
    assert st == oracle.render_las(batches, x12, x8, x4, p)[1]
    drawn = fb != EMPTY
    count = ba & np.uint64(0xFFFFFFFF)
    assert (count[drawn] >= 1).all()                           # the nearest point of a pixel always passes its own test
    assert (rg[~drawn] == 0).all() and (ba[~drawn] == 0).all()
    # the 1 % test counted independently: every drawn point against its pixel's depth, an f32 product
    pix, w = las_hqs_ref.drawn_points(batches, x12, x8, x4, p)
    d = (fb[pix] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    passing = w <= d * np.float32(1.01)
    assert int(count.sum()) == int(passing.sum())
    assert np.array_equal(np.bincount(pix[passing], minlength=len(fb)).astype(np.uint64), count)

