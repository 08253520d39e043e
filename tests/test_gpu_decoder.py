"""k_render, k_decode_points and the decode_chain() calls on the streams of tests/decoder_cases.py: every bit phase against every
point size, the escape queue in all its states, the escape pools at their limits, table values at the limit of the packed entry,
waves of 8-word chains beside waves of 72-word chains.

Nothing here is new on the reference side. Every comparison is word for word against the oracle through the helpers of the suites
that introduced the calls (tests/test_gpu_decode.py, test_gpu_edge_cases.py, test_gpu_select.py, test_gpu_screen.py); what is new is
the input, and tests/test_decoder_cpu.py proves from the oracle's decode which decoder states each stream reaches. The contexts are
those of tests/test_gpu_edge_cases.py: the half and the whole escape pool are each exercised only by the matching workgroup shape."""
import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import decoder_cases as D
from tests import screen_cases as SC
from tests import select_cases as S
from tests import test_gpu_decode as GD
from tests import test_gpu_screen as GSC
from tests import test_gpu_select as GS
from tests.test_gpu_contention import check_hqs
from tests.test_gpu_edge_cases import check_all

pytestmark = pytest.mark.gpu

IDS = [D.variant_id(v) for v in D.VARIANTS]
for _v in D.VARIANTS:                                   # the far camera of every stream as a case of tests/screen_cases.py
    SC.CASES.setdefault("decoder/" + D.variant_id(_v), ("decoder/" + D.variant_id(_v), (lambda name=_v[0]: D.cameras(name)[1]), None))


@pytest.fixture(params=["point_windows", "words", "point_windows_whole"])
def ctx(request):
    c = P.Context(0)
    if request.param == "point_windows_whole":          # one 1024-thread workgroup per batch: the whole batch's pool
        c.set_workgroup_parts(1)
    if request.param == "words":
        c.set_stream_layout(P.Context.LAYOUT_BOTH)      # both layouts resident, the packed-words kernel forced
    c.set_render_variant(P.Context.VARIANT_WORDS if request.param == "words" else P.Context.VARIANT_POINT_WINDOWS)
    c.layout_name = "both" if request.param == "words" else "point_windows"
    c.forced_variant = P.Context.VARIANT_WORDS if request.param == "words" else P.Context.VARIANT_POINT_WINDOWS
    c.set_image_size(D.WIDTH, D.HEIGHT)
    yield c
    c.close()


def loaded(c, v):
    GD.load(c, D.stream(*v), frame=False)
    return D.oracle_file(*v)


def one_frame(c, v):
    c.clear(); c.render_hqs_depth(D.cameras(v[0])[0]); c.synchronize()


def force(c):
    c.set_render_variant(c.forced_variant)              # (the helpers that go through both variants leave VARIANT_AUTO behind)


@pytest.mark.parametrize("v", D.VARIANTS, ids=IDS)
def test_read_points_before_and_after_a_frame(ctx, v):
    """pcr_read_points (k_decode_points; from both layouts where both are resident) against the oracle's decode_batch and its BC1 /
    BC7 colours, before any frame; after a first frame the same bytes."""
    of = loaded(ctx, v)
    before = GD.decode(ctx)
    GD.check_against_oracle(before, of)
    force(ctx)
    before_bytes = ctx.resident_bytes
    one_frame(ctx, v)
    assert ctx.resident_bytes < before_bytes, "the first frame releases the load-time buffers"
    after = GD.decode(ctx)
    assert after.tobytes() == before.tobytes(), f"records differ after the first frame, first at {np.nonzero(after != before)[0][:4]}"


@pytest.mark.parametrize("v", D.VARIANTS, ids=IDS)
def test_frames_near_and_far(ctx, v):
    """Basic, HQS depth, HQS colour sums, both resolves and the statistics (check_all; a BC7 stream: check_hqs): a frame that walks all 64 points of every chain, and one
    from so far away that every batch is drawn with npr < 64. (Every point inside the 1 % shell adds to its pixel's sums: a point
    decoded wrongly changes them even where it is hidden.)"""
    of = loaded(ctx, v)
    force(ctx)
    near, far = D.cameras(v[0])
    for p, whole in ((near, True), (far, False)):
        if v[2]:                                        # (the basic method has no BC7 result: the HQS half is all there is)
            check_hqs(ctx, of, p)
            st = ctx.stats()
        else:
            st = check_all(ctx, of, p)
        assert (st["points_iterated"] == of.num_batches * D.PPB) if whole else (0 < st["points_iterated"] < of.num_batches * D.PPB)


@pytest.mark.parametrize("v", D.VARIANTS, ids=IDS)
def test_decode_chain_calls(ctx, v):
    """The instantiations of decode_chain(): pcr_batch_point_bounds (no colours) against the oracle's boxes, pcr_read_box (the
    counting pass without colours, the writing pass with BC1 or BC7) with a box every batch straddles against the masked records,
    and pcr_read_screen with the far camera (npr < 64) against the oracle's trace."""
    of = loaded(ctx, v)
    want = S.oracle_bounds(of)
    got = GS.through_variants(ctx, ctx.batch_point_bounds)
    assert np.array_equal(got, want), f"batches {np.nonzero((got != want).any(axis=1))[0][:8]} differ"
    force(ctx)
    one_frame(ctx, v)
    assert np.array_equal(ctx.batch_point_bounds(), want)                   # from the cache, and the first frame changes nothing
    ref = GS.decode(ctx)
    if v[0] == "lengths":                               # (its first batch is one point 65 536 times: the box holds or misses all of it)
        ref, want, first = ref[D.PPB:], want[1:], 1
    else:
        first = 0
    box = GS.quantile_box(ref, 0.25, 0.75)
    assert (S.classify(want, box) == S.STRADDLING).all(), "the box was to cut through every batch"
    sel, st = GS.check_selection(ctx, box, ref, want, first=first)
    assert 0 < len(sel) < len(ref) and st["batches_straddling"] == len(want)
    force(ctx)
    GSC.check_case(ctx, "decoder/" + D.variant_id(v))
    assert ctx.screen_stats["points_tested"] < of.num_batches * D.PPB
