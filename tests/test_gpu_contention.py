"""GPU parity where a rule of the rasterizer decides, on frames constructed so that it decides often (tests/scenes.py,
tests/contention.py; their preconditions without a GPU: tests/test_contention_cpu.py):
  depth ties      thousands of pixels whose nearest depth is shared by points of different colour (10-10-10: index), between
                  chains, the workgroups of a batch, batches, the LDS window and the global atomics, two contexts merged;
  the 1 % edge    hundreds of drawn points for which float64(w) <= float64(d) * 1.01 (k_render) and the f32 product
                  w <= d * 1.01f (k_las_render_color) decide differently;
  overdraw        whole batches of pure white points in one pixel: the 16-bit run sums, the 32-bit per-batch LDS sums and the
                  64-bit planes of the colour pass at their stated bounds, against analytic values.
Every Huffman case runs over the context variants of tests/test_gpu_edge_cases.py with that file's check_all, and once more
through frame_begin / frame_turn. Each test asserts its precondition from the oracle's trace before it looks at the GPU.

What the module was seen to catch (each change built once into a library that was never committed and run once on an MI355X; cases failed):
  scatter_min `depth > old_hi` -> `>=`                                     31 (ties on planes, clusters, payloads, merge, edge)
  window merge of k_render skips the atomic unless its depth is smaller    34 (the same groups)
  both f64 comparisons of k_render's colour pass -> `pw <= old_depth * 1.01f`   18 (every case of test_one_percent_edge)
  k_las_render_color's f32 product -> the f64 form                          1 (test_one_percent_edge_in_loop_las_hqs)
  k_las_render scatter_pending `<=` -> `<`                                  3 (the 10-10-10 tie and edge cases)
  flush_run `run_rg16 & 0xFFFFu` -> `& 0x1FFFu`                            24 (one pixel, the Morton-sorted corner, edge)"""
import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import contention as K
from tests import oracle, scenes
from tests.test_gpu_edge_cases import check_all, ctx, load  # noqa: F401  (ctx: the fixture of the three context variants)
from tests.test_gpu_las import _check as check_las
from tests.test_gpu_las_hqs import _check as check_las_hqs

pytestmark = pytest.mark.gpu

EMPTY = K.EMPTY


def _differ(what, a, b):
    bad = np.nonzero(a != b)[0]
    return f"{what}: {bad.size} words differ, first at {bad[:4]}: gpu {[hex(int(v)) for v in a[bad[:4]]]} oracle {[hex(int(v)) for v in b[bad[:4]]]}"


def check_hqs(ctx, of, p):
    """The HQS half of check_all with the mismatching pixels named (and all there is for a BC7 stream: the basic method has
    no BC7 result). Returns the oracle's (depth, RG, BA)."""
    ctx.clear(); ctx.render_hqs_depth(p)
    hfb, hst = of.render_hqs_depth(p)
    assert ctx.stats() == hst
    fb = ctx.read_framebuffer(full=True)
    assert np.array_equal(fb, hfb), _differ("HQS depth", fb, hfb)
    ctx.render_hqs_color(p); ctx.resolve_hqs(p)
    org, oba, _ = of.render_hqs_color(p, hfb)
    rg, ba = ctx.read_accum(full=True)
    assert np.array_equal(rg, org), _differ("RG sums", rg, org)
    assert np.array_equal(ba, oba), _differ("BA sums", ba, oba)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_hqs(p, hfb, org, oba))
    return hfb, org, oba


def check_turns(ctx, of, p, basic=True):
    """The same frames through frame_begin / frame_turn: the tile-tracking resolve and clear see them too."""
    if basic:
        ofb, _ = of.render_basic(p)
        ctx.frame_begin(p)
        for _ in range(2):                  # (the second frame is drawn into what the first turn cleared)
            ctx.render_basic(p)
            fb = ctx.read_framebuffer(full=True)
            assert np.array_equal(fb, ofb), _differ("basic after frame_begin / frame_turn", fb, ofb)
            ctx.frame_turn(p, p)
            assert np.array_equal(ctx.read_rgba(), oracle.resolve_basic(p, ofb))
            assert np.all(ctx.read_framebuffer(full=True) == EMPTY)
    hfb, _ = of.render_hqs_depth(p)
    org, oba, _ = of.render_hqs_color(p, hfb)
    ctx.frame_begin(p, hqs=True)
    for _ in range(2):
        ctx.render_hqs_depth(p); ctx.render_hqs_color(p)
        fb = ctx.read_framebuffer(full=True)
        assert np.array_equal(fb, hfb), _differ("HQS depth after frame_begin / frame_turn", fb, hfb)
        rg, ba = ctx.read_accum(full=True)
        assert np.array_equal(rg, org), _differ("RG sums after frame_begin / frame_turn", rg, org)
        assert np.array_equal(ba, oba), _differ("BA sums after frame_begin / frame_turn", ba, oba)
        ctx.frame_turn(p, p, hqs=True)
        assert np.array_equal(ctx.read_rgba(), oracle.resolve_hqs(p, hfb, org, oba))
        rg, ba = ctx.read_accum(full=True)
        assert np.all(ctx.read_framebuffer(full=True) == EMPTY) and not rg.any() and not ba.any()
    ctx.clear()


def check_everything(ctx, stream, p):
    image, of = K.stream(stream)
    ctx.set_image_size(p.width, p.height)
    load(ctx, image)
    bc7 = stream.endswith("_bc7")
    if bc7:
        with pytest.raises(P.PcrError, match="BC7"):
            ctx.render_basic(p)
    else:
        # the basic frame first with the mismatching pixels named, then the full chain of check_all
        ctx.clear(); ctx.render_basic(p)
        ofb, _ = of.render_basic(p)
        fb = ctx.read_framebuffer(full=True)
        assert np.array_equal(fb, ofb), _differ("basic", fb, ofb)
        check_all(ctx, of, p)
    got = check_hqs(ctx, of, p)
    check_turns(ctx, of, p, basic=not bc7)
    return of, got


@pytest.fixture
def las_ctx():
    c = P.Context(0)
    yield c
    c.close()


def load_las(c, q, w, h):
    c.set_image_size(w, h)
    c.las_begin(len(q[0]) * 65536)
    c.las_upload(0, *q)


# ---- depth ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["tie_320", "tie_64"])
@pytest.mark.parametrize("stream", ["tie_planes", "tie_planes_unsorted"])
def test_depth_ties_on_planes(ctx, stream, frame):
    """Four planes seen straight down: equal z is equal depth bits, and the smaller colour word has to win wherever the tied
    points meet -- in a chain's registers, the LDS window, the merge of two workgroups' windows or of two batches."""
    st = K.huffman_tie_stats(stream, frame)
    assert st["other_tag"] >= 1000, st
    if stream == "tie_planes_unsorted":
        assert st["other_batch"] >= 1000, st
    check_everything(ctx, stream, K.frame(frame))


@pytest.mark.parametrize("frame", ["clusters_1080", "clusters_4096"])
def test_depth_ties_between_windows_and_global_atomics(ctx, frame):
    """Batches that fall apart into clusters (a window per run of chains, straddling chains and what lies off the windows on the
    global path), z snapped to planes: the tied points of a pixel come by both routes and from different batches."""
    st = K.huffman_tie_stats("tie_clusters", frame)
    assert st["other_tag"] >= 1000 and st["other_batch"] >= 100, st
    check_everything(ctx, "tie_clusters", K.frame(frame))


@pytest.mark.parametrize("flag", ["show_num_points", "colorize_chunks"])
def test_depth_ties_with_payloads(ctx, flag):
    """The HQS depth pass writes a payload under the depth (points per chain / batch index): ties between batches are ties
    between payloads."""
    st = K.huffman_tie_stats("tie_planes_unsorted", "tie_320", oracle.HQS)
    assert st["other_batch"] >= 1000, st
    image, of = K.stream("tie_planes_unsorted")
    p = scenes.with_flags(K.frame("tie_320"), **{flag: 1})
    ctx.set_image_size(p.width, p.height)
    load(ctx, image)
    check_all(ctx, of, p)
    hfb, _, _ = check_hqs(ctx, of, p)
    if flag == "colorize_chunks":
        assert np.unique(hfb[hfb != EMPTY] & K.U32).size == of.num_batches          # every batch wins somewhere
    check_turns(ctx, of, p)


@pytest.mark.parametrize("frame", ["tie_320", "tie_64"])
def test_depth_ties_in_the_10_10_10_methods(las_ctx, frame):
    """The same planes through pcr_render_las + pcr_resolve_las (winner: the smallest point index) and loop_las_hqs."""
    st = K.las_tie_stats("tie_planes", frame)
    assert st["other_tag"] >= 1000 and st["other_batch"] >= 100, st
    q, p = K.las_cloud("tie_planes"), K.frame(frame)
    load_las(las_ctx, q, p.width, p.height)
    check_las(las_ctx, q, p)
    check_las_hqs(las_ctx, q, p)


def test_depth_ties_across_merge_min(ctx):
    """Two contexts hold half the batches of the unsorted planes each: every pixel's tie is decided by pcr_merge_min."""
    image, of = K.stream("tie_planes_unsorted")
    p = K.frame("tie_320")
    pix, depth, colour, batch = K.trace(of, p, oracle.MEM_ITER)
    st = K.tie_stats(pix, depth, colour, batch // 2, len(of.new_fb(p)))           # "batch" = which context
    assert st["other_tag"] >= 1000 and st["other_batch"] >= 1000, st
    f = P.HuffmanFile(image)
    shard = P.Context(0)
    try:
        ctxs = [ctx, shard]
        half = f.numBatches // 2
        for c, (first, count) in zip(ctxs, [(0, half), (half, f.numBatches - half)]):
            c.set_image_size(p.width, p.height)
            c.stream_begin(f.header(first, count), first)
            for i in range(count):
                c.upload_batch(i, f.blob(first + i))
            if first + count < f.numBatches:
                c.upload_tail(*f.head_words(first + count))
        for c in ctxs:
            c.clear(); c.render_basic(p)
        shard.synchronize()
        ctx.merge_min(shard.device_framebuffer())
        ofb, _ = of.render_basic(p)
        fb = ctx.read_framebuffer(full=True)
        assert np.array_equal(fb, ofb), _differ("merged basic", fb, ofb)
        q = scenes.with_flags(p, colorize_chunks=1)                                # payload ties across the merge
        for c in ctxs:
            c.clear(); c.render_hqs_depth(q)
        shard.synchronize(); ctx.synchronize()
        ctx.merge_min(shard.device_framebuffer()); ctx.synchronize()
        shard.merge_min(ctx.device_framebuffer())
        hfb, _ = of.render_hqs_depth(q)
        for c in ctxs:
            fb = c.read_framebuffer(full=True)
            assert np.array_equal(fb, hfb), _differ("merged HQS depth", fb, hfb)
        for c in ctxs:
            c.render_hqs_color(q)
        shard.synchronize()
        ctx.merge_sum(int(ctx.lib.pcr_device_rg(shard.h)), int(ctx.lib.pcr_device_ba(shard.h)))
        org, oba, _ = of.render_hqs_color(q, hfb)
        rg, ba = ctx.read_accum(full=True)
        assert np.array_equal(rg, org) and np.array_equal(ba, oba)
    finally:
        shard.close()


# ---- the 1 % edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,double", [("edge_320", 0), ("edge_64", 0), ("edge_double", 4)])
@pytest.mark.parametrize("stream", ["edge", "edge_bc7"])
def test_one_percent_edge(ctx, stream, frame, double):
    """Two thin layers 1 % apart in depth: about half of the lower one passes the colour pass's test, and for hundreds of points
    the f64 form of the Huffman kernels and the f32 product decide differently. Float and double dequantisation, BC1 and BC7."""
    st = K.huffman_edge_stats(stream, frame)
    assert st["differ"] >= 100 and 0.25 <= st["lower_passing"] <= 0.75, st
    of, _ = check_everything(ctx, stream, K.frame(frame))
    assert of.render_hqs_depth(K.frame(frame))[1]["batches_double"] == double


def test_one_percent_edge_in_loop_las_hqs(las_ctx):
    """The 10-10-10 HQS method compares in f32, after its reference: the same layers at 20-bit precision."""
    st = K.las_edge_stats("edge", "edge_las")
    assert st["differ"] >= 100 and 0.25 <= st["lower_passing"] <= 0.75, st
    q, p = K.las_cloud("edge"), K.frame("edge_las")
    assert [oracle.las_level(q[0][b], p) for b in range(len(q[0]))] == [1, 1, 1, 1]
    load_las(las_ctx, q, p.width, p.height)
    check_las_hqs(las_ctx, q, p)
    check_las(las_ctx, q, p)


# ---- one-pixel overdraw ----------------------------------------------------------------------------------------------
def _assert_white(ctx, p, got, counts):
    """The oracle's sums and the GPU's (equal by now) are the analytic ones: 255 * count three times and the count; white pixels."""
    hfb, org, oba = got
    erg, eba = K.white_sums(counts)
    assert np.array_equal(org, erg) and np.array_equal(oba, eba)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)
    rg, ba = ctx.read_accum(full=True)
    assert np.array_equal(rg, erg), _differ("RG sums against 255 * n", rg, erg)
    assert np.array_equal(ba, eba), _differ("BA sums against 255 * n | n", ba, eba)
    img = ctx.read_rgba()
    drawn = counts[:p.width * p.height] > 0
    assert (img[drawn] & 0xFFFFFF == 0xFFFFFF).all() and (img[~drawn] == img[0]).all()


@pytest.mark.parametrize("stream,batches", [("one", 3), ("one_bc7", 3), ("twenty", 20), ("twenty_bc7", 20)])
def test_whole_batches_in_one_pixel(ctx, stream, batches):
    """Every point white, in pixel 1202, passing the 1 % test: each chain's run sums reach 64 * 255 per 16-bit half, each batch's
    LDS sums 65 536 * 255 per 32-bit half, and twenty of those are added into one pair of global words."""
    p = K.frame("one")
    n = batches * 65536
    counts = np.zeros(len(K.stream(stream)[1].new_fb(p)), np.uint64)
    counts[1202] = n
    of, got = check_everything(ctx, stream, p)
    _assert_white(ctx, p, got, counts)
    if batches == 3:
        assert int(got[1][1202]) == 0x02FD0000_02FD0000 and int(got[2][1202]) == 0x02FD0000_00030000
    if not stream.endswith("_bc7"):
        ctx.clear(); ctx.render_basic(p)
        fb = ctx.read_framebuffer(full=True)
        assert np.array_equal(np.nonzero(fb != EMPTY)[0], [1202]) and fb[1202] == (got[0][1202] | np.uint64(0xFFFFFF))


@pytest.mark.parametrize("stream", ["one", "one_unsorted", "one_unsorted_bc7"])
def test_a_cloud_across_the_corner_of_four_pixels(ctx, stream):
    """The same cloud over the corner of four pixels: in input order a chain changes pixel on three points of four, so the
    run sums are flushed on nearly every point; Morton-sorted, only the chains on the seams alternate."""
    of, p = K.stream(stream)[1], K.frame("corner")
    pix = K.trace(of, p, oracle.HQS)[0]
    counts = np.bincount(pix, minlength=len(of.new_fb(p))).astype(np.uint64)
    assert np.array_equal(np.nonzero(counts)[0], [1136, 1137, 1201, 1202]) and counts.sum() == 3 * 65536 and counts[counts > 0].min() > 40_000
    _, got = check_everything(ctx, stream, p)
    _assert_white(ctx, p, got, counts)


def test_whole_batches_in_one_pixel_in_loop_las_hqs(las_ctx):
    q, p = K.las_cloud("one"), K.frame("one")
    load_las(las_ctx, q, p.width, p.height)
    fb, rg, ba = check_las_hqs(las_ctx, q, p)
    erg, eba = K.white_sums(3 * 65536)
    assert rg[1202] == erg and ba[1202] == eba and np.count_nonzero(rg) == 1 and np.count_nonzero(ba) == 1
    grg, gba = las_ctx.read_accum(full=True)
    assert grg[1202] == erg and gba[1202] == eba
    assert las_ctx.read_rgba()[1202] & 0xFFFFFF == 0xFFFFFF
    check_las(las_ctx, q, p)
