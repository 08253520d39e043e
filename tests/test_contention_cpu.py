"""The constructed scenes of tests/test_gpu_contention.py on the CPU: the oracle's point trace rebuilds the oracle's three frames in
numpy (independently of its frame code), every scene meets the precondition its GPU test rests on (depth ties by the thousand,
the f32 / f64 forms of the 1 % test disagreeing for hundreds of drawn points, one pixel holding whole batches), and the
one-pixel sums are the analytic ones. No GPU."""
import ctypes as C

import numpy as np
import pytest

from pcrhpg24_amd._native import fb_elems
from tests import contention as K
from tests import las_hqs_ref, oracle, scenes

HUFFMAN_FRAMES = [("tie_planes", "tie_320"), ("tie_planes", "tie_64"), ("tie_planes_unsorted", "tie_320"), ("tie_planes_unsorted", "tie_64"),
                  ("tie_clusters", "clusters_1080"), ("tie_clusters", "clusters_4096"),
                  ("edge", "edge_320"), ("edge", "edge_64"), ("edge", "edge_double"),
                  ("edge_bc7", "edge_320"), ("edge_bc7", "edge_64"), ("edge_bc7", "edge_double"),
                  ("one", "one"), ("one_bc7", "one"), ("one", "corner"), ("one_unsorted", "corner"), ("one_unsorted_bc7", "corner"),
                  ("twenty", "one"), ("twenty_bc7", "one")]


def _differ(a, b):
    bad = np.nonzero(a != b)[0]
    return f"{bad.size} words differ, first at {bad[:4]}: {a[bad[:4]]} / {b[bad[:4]]}"


@pytest.mark.parametrize("stream,frame", HUFFMAN_FRAMES)
def test_trace_rebuilds_the_oracle_frames(stream, frame):
    """basic = per-pixel min of depth << 32 | colour, HQS depth = per-pixel min depth, sums = np.add.at over the points with
    float64(w) <= float64(d) * 1.01: each equals the oracle's frame exactly."""
    of, p = K.stream(stream)[1], K.frame(frame)
    if not stream.endswith("_bc7"):                     # (the basic method has no BC7 result)
        ofb, ost = of.render_basic(p)
        fb = K.rebuild_basic(of, p)
        assert np.array_equal(fb, ofb), _differ(fb, ofb)
        assert ost["points_iterated"] == of.num_batches * 65536             # LOD 100, no culling: every point is walked
    hfb, _ = of.render_hqs_depth(p)
    org, oba, _ = of.render_hqs_color(p, hfb)
    fb, rg, ba = K.rebuild_hqs(of, p)
    assert np.array_equal(fb, hfb), _differ(fb, hfb)
    assert np.array_equal(rg, org), _differ(rg, org)
    assert np.array_equal(ba, oba), _differ(ba, oba)


@pytest.mark.parametrize("flag", ["show_num_points", "colorize_chunks"])
def test_trace_rebuilds_the_payload_frames(flag):
    of = K.stream("tie_planes_unsorted")[1]
    p = scenes.with_flags(K.frame("tie_320"), **{flag: 1})
    payload = [64] * of.num_batches if flag == "show_num_points" else list(range(of.num_batches))
    hfb, _ = of.render_hqs_depth(p)
    fb = K.rebuild_hqs(of, p, payload)[0]
    assert np.array_equal(fb, hfb), _differ(fb, hfb)


def test_trace_calling_convention():
    """One entry per inside point in walk order; a batch range gives that range's points; the return value counts past `cap`."""
    of, p = K.stream("tie_planes")[1], K.frame("tie_64")
    pix, depth, colour = of.trace_points(p)
    assert len(pix) > 100_000 and pix.min() >= 0 and pix.max() < p.width * p.height
    halves = [of.trace_points(p, first=f, count=2) for f in (0, 2)]
    for k, whole in enumerate((pix, depth, colour)):
        assert np.array_equal(np.concatenate([h[k] for h in halves]), whole)
    cap = 1000
    a, b, c = np.zeros(cap + 1, np.int64), np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.uint32)
    n = oracle.lib().pcr_oracle_trace_points(of.stream, C.byref(p), 0, of.num_batches, oracle.MEM_ITER, a.ctypes.data, b.ctypes.data,
                                             c.ctypes.data, cap)
    assert n == len(pix) and np.array_equal(a[:cap], pix[:cap]) and a[cap] == 0 and b[cap] == 0 and c[cap] == 0
    # the colours are the decoder's: every winner of the basic frame is a traced (depth, colour) pair of its pixel
    ofb, _ = of.render_basic(p)
    keys = (depth.astype(np.uint64) << np.uint64(32)) | colour.astype(np.uint64)
    assert np.isin(ofb[:p.width * p.height][ofb[:p.width * p.height] != K.EMPTY], keys).all()


# ---- depth ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream,frame", HUFFMAN_FRAMES[:6])
def test_tie_frames_hold_thousands_of_decided_ties(stream, frame):
    st = K.huffman_tie_stats(stream, frame)
    assert st["other_tag"] >= 1000, st
    of, p = K.stream(stream)[1], K.frame(frame)
    fb, _ = of.render_basic(p)
    assert of.count_depth_ties(p, fb)[1] == st["other_tag"]                # the oracle's own count agrees with the trace's
    if stream != "tie_planes":                          # (Morton-sorted planes: a batch is a quadrant, ties cross batches only at the seams)
        assert st["other_batch"] >= 100, st
    hst = K.huffman_tie_stats(stream, frame, oracle.HQS)
    assert hst == st                                    # LOD 100: both LOD expressions walk every point


def test_tie_planes_paths():
    of = K.stream("tie_planes")[1]
    assert of.render_basic(K.frame("tie_320"))[1]["batches_double"] == of.num_batches == 4
    assert of.render_basic(K.frame("tie_64"))[1]["batches_double"] == 0
    assert K.huffman_tie_stats("tie_planes", "tie_64")["max_per_pixel"] >= 64
    # payload ties of the HQS depth pass (colorize_chunks writes the batch index): tied points of different batches
    assert K.huffman_tie_stats("tie_planes_unsorted", "tie_320", oracle.HQS)["other_batch"] >= 1000


@pytest.mark.parametrize("frame", ["tie_320", "tie_64"])
def test_tie_planes_in_the_10_10_10_form(frame):
    """Winner = smallest point index. The frames from the point list: min of depth << 32 | index; the HQS pair from it as well."""
    q, p = K.las_cloud("tie_planes"), K.frame(frame)
    st = K.las_tie_stats("tie_planes", frame)
    assert st["other_tag"] >= 1000 and st["other_batch"] >= 100, st
    pix, w, index = las_hqs_ref.drawn_points(*q[:4], p, with_index=True)
    n = fb_elems(p.width, p.height)
    fb = np.full(n, K.EMPTY, np.uint64)
    np.minimum.at(fb, pix, (w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64))
    ofb, _ = oracle.render_las(*q[:4], p)
    assert np.array_equal(fb, ofb), _differ(fb, ofb)
    hfb, _ = las_hqs_ref.render_depth(*q[:4], p)
    assert np.array_equal(hfb, np.where(fb == K.EMPTY, fb, fb & ~K.U32))


# ---- the 1 % edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["edge", "edge_bc7"])
@pytest.mark.parametrize("frame,double", [("edge_320", 0), ("edge_64", 0), ("edge_double", 4)])
def test_edge_frames_hold_points_the_two_forms_decide_differently(stream, frame, double):
    st = K.huffman_edge_stats(stream, frame)
    assert st["differ"] >= 100, st
    assert 0.25 <= st["lower_passing"] <= 0.75 and st["lower"] > 100_000, st
    of, p = K.stream(stream)[1], K.frame(frame)
    assert of.render_hqs_depth(p)[1]["batches_double"] == double
    # what the disagreement is worth in the frame: the count plane of the f32 form differs in that many points
    pix, depth, _, _ = K.trace(of, p, oracle.HQS)
    hfb, _ = of.render_hqs_depth(p)
    _, oba, _ = of.render_hqs_color(p, hfb)
    w, d = depth.view(np.float32), (hfb >> np.uint64(32)).astype(np.uint32).view(np.float32)
    f32 = w <= (d[pix] * np.float32(1.01)).astype(np.float32)
    cnt32 = np.bincount(pix[f32], minlength=len(hfb))
    assert int(np.abs(cnt32 - (oba & K.U32).astype(np.int64)).sum()) >= 100


def test_edge_frame_in_the_10_10_10_form():
    """20-bit coordinates (level 1) for every batch, or the layers collapse onto a handful of 10-bit steps; the reference of that
    method uses the f32 product, and the f64 form would count differently."""
    q, p = K.las_cloud("edge"), K.frame("edge_las")
    assert [oracle.las_level(q[0][b], p) for b in range(len(q[0]))] == [1, 1, 1, 1]
    st = K.las_edge_stats("edge", "edge_las")
    assert st["differ"] >= 100 and 0.25 <= st["lower_passing"] <= 0.75, st
    pix, w, index = las_hqs_ref.drawn_points(*q[:4], p, with_index=True)
    fb, _ = las_hqs_ref.render_depth(*q[:4], p)
    rg, ba, _ = las_hqs_ref.render_color(*q, p, fb)
    d = (fb >> np.uint64(32)).astype(np.uint32).view(np.float32)
    passing = w <= (d[pix] * np.float32(1.01)).astype(np.float32)
    rgba = q[4][index].astype(np.uint64)
    r, g, b = ((rgba >> np.uint64(s)) & np.uint64(255) for s in (0, 8, 16))
    erg, eba = np.zeros(len(fb), np.uint64), np.zeros(len(fb), np.uint64)
    np.add.at(erg, pix[passing], ((r << np.uint64(32)) | g)[passing])
    np.add.at(eba, pix[passing], ((b << np.uint64(32)) | np.uint64(1))[passing])
    assert np.array_equal(rg, erg) and np.array_equal(ba, eba)


# ---- one-pixel overdraw ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream,batches", [("one", 3), ("one_bc7", 3), ("twenty", 20), ("twenty_bc7", 20)])
def test_one_pixel_holds_every_point_and_the_sums_are_analytic(stream, batches):
    of, p = K.stream(stream)[1], K.frame("one")
    hfb, hst = of.render_hqs_depth(p)
    rg, ba, _ = of.render_hqs_color(p, hfb)
    n = batches * 65536
    assert hst["points_iterated"] == n and np.array_equal(np.nonzero(ba)[0], [1202]) and np.array_equal(np.nonzero(rg)[0], [1202])
    erg, eba = K.white_sums(n)
    assert rg[1202] == erg and ba[1202] == eba
    if batches == 3:
        assert int(rg[1202]) == 0x02FD0000_02FD0000 and int(ba[1202]) == 0x02FD0000_00030000
    assert oracle.resolve_hqs(p, hfb, rg, ba)[1202] & 0xFFFFFF == 0xFFFFFF
    if not stream.endswith("_bc7"):
        fb, _ = of.render_basic(p)
        assert np.array_equal(np.nonzero(fb != K.EMPTY)[0], [1202])
        assert fb[1202] == (hfb[1202] | np.uint64(0xFFFFFF))                # the nearest depth, pure white


@pytest.mark.parametrize("stream", ["one", "one_unsorted", "one_unsorted_bc7"])
def test_corner_frame_spreads_the_cloud_over_four_pixels(stream):
    of, p = K.stream(stream)[1], K.frame("corner")
    pix, _, colour, _ = K.trace(of, p, oracle.HQS)
    cnt = np.bincount(pix, minlength=fb_elems(p.width, p.height))
    assert np.array_equal(np.nonzero(cnt)[0], [1136, 1137, 1201, 1202]) and cnt.sum() == 3 * 65536 and cnt[cnt > 0].min() > 40_000
    assert (colour & 0xFFFFFF == 0xFFFFFF).all()
    hfb, _ = of.render_hqs_depth(p)
    rg, ba, _ = of.render_hqs_color(p, hfb)
    erg, eba = K.white_sums(cnt)
    assert np.array_equal(rg, erg) and np.array_equal(ba, eba)
    if "unsorted" in stream:            # input order: consecutive points of a chain change pixel three times out of four
        assert (np.diff(pix) != 0).mean() > 0.7


def test_one_pixel_in_the_10_10_10_form():
    q, p = K.las_cloud("one"), K.frame("one")
    pix, w = las_hqs_ref.drawn_points(*q[:4], p)
    assert len(pix) == 3 * 65536 and (pix == 1202).all()
    fb, _ = las_hqs_ref.render_depth(*q[:4], p)
    rg, ba, _ = las_hqs_ref.render_color(*q, p, fb)
    erg, eba = K.white_sums(3 * 65536)
    assert rg[1202] == erg and ba[1202] == eba and np.count_nonzero(rg) == 1 and np.count_nonzero(ba) == 1
