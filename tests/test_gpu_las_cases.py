"""GPU parity of both 10-10-10 methods on the constructed cases of tests/las_cases.py (level cuts, fields and masks, the frustum
border, depth ties, the f32 1 % edge, window shapes, the draw list): every pass and both resolves against the oracle and
tests/las_hqs_ref.c, bit-exact. tests/test_las_cases_cpu.py proves that each case is the case its name says."""
import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import las_cases as LC
from tests import las_hqs_ref, oracle

pytestmark = pytest.mark.gpu


def _same(what, got, ref):
    diff = np.nonzero(got != ref)[0]
    assert diff.size == 0, f"{what}: {diff.size} words differ, first at {diff[:5]}: gpu {got[diff[:3]]} reference {ref[diff[:3]]}"


def _check_frame(ctx, q, p, levels, refs):
    batches, x12, x8, x4, rgba = q
    key = bytes(p)
    if key not in refs:                        # a frame drawn twice (many ... many again) is referenced once
        ofb, ost = oracle.render_las(batches, x12, x8, x4, p)
        fb, st = las_hqs_ref.render_depth(batches, x12, x8, x4, p)
        rg, ba, _ = las_hqs_ref.render_color(batches, x12, x8, x4, rgba, p, fb)
        assert st == ost
        refs[key] = (ofb, ost, fb, rg, ba)
    ofb, ost, fb, rg, ba = refs[key]
    # loop_las_cuda
    ctx.clear()
    ctx.render_las(p)
    ctx.resolve_las(p)
    assert ctx.stats() == ost
    _same("framebuffer", ctx.read_framebuffer(full=True), ofb)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_las(p, ofb, rgba))
    assert ctx.las_algorithmic_bytes == LC.algorithmic_bytes(levels, False)
    # loop_las_hqs
    ctx.clear()
    ctx.render_las_hqs_depth(p)
    assert ctx.stats() == ost
    _same("depth", ctx.read_framebuffer(full=True), fb)
    ctx.render_las_hqs_color(p)
    assert ctx.stats() == ost
    grg, gba = ctx.read_accum(full=True)
    _same("RG sums", grg, rg)
    _same("BA sums", gba, ba)
    assert np.array_equal(ctx.read_framebuffer(full=True), fb)          # the colour pass leaves the depth alone
    ctx.resolve_hqs(p)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_hqs(p, fb, rg, ba))
    assert ctx.las_algorithmic_bytes == LC.algorithmic_bytes(levels, True)


@pytest.mark.parametrize("name", list(LC.CASES))
def test_las_case(name):
    batches, x12, x8, x4, rgba, params, W, H, facts = LC.build(name)
    q = (batches, x12, x8, x4, rgba)
    ctx = P.Context(0)
    try:
        ctx.set_image_size(W, H)
        ctx.las_begin(len(batches) * LC.PPB)
        ctx.las_upload(0, *q)
        refs = {}
        for fname, p in facts["frames"]:           # in this order on the one context: a frame must not see the one before it
            levels = [oracle.las_level(batches[b], p) for b in range(len(batches))]
            _check_frame(ctx, q, p, levels, refs)
    finally:
        ctx.close()
