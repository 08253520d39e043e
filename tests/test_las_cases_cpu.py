"""The constructed 10-10-10 cases of tests/las_cases.py are the cases their names say: every fact a case relies on, proved on the
CPU from the reference side only (the oracle and tests/las_hqs_ref.c). No GPU."""
import numpy as np
import pytest

from tests import las_cases as LC
from tests import las_hqs_ref, oracle

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
F32 = np.float32


def _frames(name):
    batches, x12, x8, x4, rgba, params, W, H, facts = LC.build(name)
    seen = {}
    for fname, p in facts["frames"]:
        key = bytes(p)
        if key not in seen:
            seen[key] = (fname, p)
    return (batches, x12, x8, x4, rgba), W, H, facts, list(seen.values())


def _set_words(fb):
    return np.nonzero(fb != EMPTY)[0].tolist()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_levels_pixels_and_counts(name):
    """Per frame: the oracle's level of every batch but the last, the set words of its frame, and -- where a case puts a known
    number of points on a pixel -- the count the HQS reference reports there."""
    q, W, H, facts, frames = _frames(name)
    batches = q[0]
    for fname, p in frames:
        levels = [oracle.las_level(batches[b], p) for b in range(len(batches) - 1)]
        expect = facts["levels"][:-1] if "classes" not in facts else [-1 if c == "C" else 4 for c in facts["classes"][fname][:-1]]
        assert levels == expect, fname
        ofb, ost = oracle.render_las(*q[:4], p)
        assert ofb.size == LC.full_frame_elems(W, H)
        if "pixels" in facts:
            assert _set_words(ofb) == facts["pixels"][fname], fname
        fb, st = las_hqs_ref.render_depth(*q[:4], p)
        assert st == ost and np.array_equal(fb >> np.uint64(32), ofb >> np.uint64(32))
        pix, w = las_hqs_ref.drawn_points(*q[:4], p)
        assert sorted(set(pix.tolist())) == _set_words(ofb)
        if "drawn" in facts:                       # G: 65 536 points on each drawn batch's pixel, none elsewhere
            counts = np.bincount(pix, minlength=ofb.size)
            assert np.nonzero(counts)[0].tolist() == facts["pixels"][fname]
            assert (counts[facts["pixels"][fname]] == LC.PPB).all()
            _, ba, _ = las_hqs_ref.render_color(*q, p, fb)
            assert ((ba & np.uint64(0xFFFFFFFF)) == counts.astype(np.uint64)).all()
            assert ost["batches_culled"] == facts["classes"][fname].count("C")
            assert ost["points_iterated"] == LC.PPB * len(facts["drawn"][fname])


def test_level_cuts_are_adjacent_floats():
    q, W, H, facts, frames = _frames("A_level_cuts")
    p = frames[0][1]
    assert facts["levels"][:-1] == [2, 1, 1, 0, 0, 2, 3, 4]
    for below, above, cut, pair_b, pair_a in facts["cuts"]:
        for b, pair, k in ((below, pair_b, 0), (above, pair_a, 1)):
            bits = np.asarray(pair, F32).view(np.uint32)
            assert int(bits[1]) - int(bits[0]) == 1
            assert float(q[0][b].max_y) == pair[k]
            g = LC.make_batch((q[0][b].min_x, q[0][b].min_y, q[0][b].min_z), (q[0][b].max_x, pair[1 - k], q[0][b].max_z))
            assert oracle.las_level(g, p) == oracle.las_level(q[0][b], p) + (-1 if k == 0 else 1)    # one float further: the other level
        assert oracle.las_level(q[0][below], p) == oracle.las_level(q[0][above], p) + 1 == {500: 2, 10000: 1}[cut]
        # the batch above sits on the cut itself, where `px < cut` and `px <= cut` part; the one below is the float before it
        assert LC.level_px(q[0][above], p) == float(cut) and LC.level_px(q[0][below], p) < cut
    assert oracle.las_level(q[0][4], p) == 0                  # pc.w == 0: px is NaN, every comparison fails


def test_fields_case_ignores_the_bits_it_sets():
    """B: the oracle's frame is unchanged when bits 30-31 and the arrays a level does not read are zeroed; and the case does hold
    all-zero and all-ones fields, X == 0x3FFFFFFF at level 0 included."""
    (batches, x12, x8, x4, rgba), W, H, facts, frames = _frames("B_fields")
    p = frames[0][1]
    assert facts["levels"][:-1] == [0, 1, 2, 3, 4]
    ofb, _ = oracle.render_las(batches, x12, x8, x4, p)
    m = np.uint32(0x3FFFFFFF)
    c12, c8, c4 = x12 & m, x8 & m, x4 & m
    for b, level in enumerate(facts["levels"]):
        sl = slice(b * LC.PPB, (b + 1) * LC.PPB)
        assert ((x4[sl] >> np.uint32(30)) == (np.arange(LC.PPB) & 3)).all()
        for arr, reads in ((x8, level <= 1), (x12, level == 0)):
            f = arr[sl] & m
            if not reads:
                assert (f == m).all()
            elif b < len(batches) - 1:
                for shift in (0, 10, 20):
                    v = (f >> np.uint32(shift)) & np.uint32(1023)
                    assert (v == 0).any() and (v == 1023).any()
        if level >= 2:
            c8[sl] = 0
        if level >= 1:
            c12[sl] = 0
    x30 = (x4[:LC.PPB] & 1023).astype(np.int64) << 20 | (x8[:LC.PPB] & 1023).astype(np.int64) << 10 | (x12[:LC.PPB] & 1023)
    assert (x30 == 0x3FFFFFFF).any() and float(F32(0x3FFFFFFF)) == 2.0 ** 30
    assert (x12 >> np.uint32(30)).any() and (x8 >> np.uint32(30)).any()
    cfb, _ = oracle.render_las(batches, c12, c8, c4, p)
    assert np.array_equal(cfb, ofb)
    assert len(_set_words(ofb)) > 1000


def test_border_words():
    q, W, H, facts, frames = _frames("C_border")
    ofb, _ = oracle.render_las(*q[:4], frames[0][1])
    words = _set_words(ofb)
    assert set(facts["border_words"]) <= set(words)
    assert any(v % W == 0 and v < W * H for v in words) and any(W * H <= v < W * (H + 1) for v in words)
    p = frames[0][1]
    rects = [LC.window_rect(p, (b.min_x, b.min_y, b.min_z), (b.max_x, b.max_y, b.max_z), LC.WIN_PIXELS) for b in q[0]]
    assert all(r[2] > 0 and not r[4] for r in rects[:5])          # whole windows
    assert rects[5][2:] == (90, 45, True) and rects[6][2:] == (0, 0, True)      # cut from the whole image; none
    # the border points are outside every window: column W and row H are no pixels of the image
    assert all(r[0] + r[2] <= W and r[1] + r[3] <= H for r in rects)


@pytest.mark.parametrize("order", LC.TIE_ORDERS)
def test_ties(order):
    q, W, H, facts, frames = _frames("D_ties_" + order)
    p = frames[0][1]
    pixel, winner, tied = facts["tie"]
    pix, w, index = las_hqs_ref.drawn_points(*q[:4], p, with_index=True)
    assert (pix == pixel).all() and len(pix) == LC.PPB * len(order)
    nearest = w.min()
    assert int((w == nearest).sum()) == tied and int(index[w == nearest].min()) == winner
    assert float(nearest) == (255.0 if "n" in order else 256.0)
    ofb, _ = oracle.render_las(*q[:4], p)
    assert int(ofb[pixel]) & 0xFFFFFFFF == winner and int(ofb[pixel]) >> 32 == int(F32(nearest).view(np.uint32))
    for b, kind in enumerate(order):
        g = q[0][b]
        r = LC.window_rect(p, (g.min_x, g.min_y, g.min_z), (g.max_x, g.max_y, g.max_z), LC.WIN_PIXELS)
        if kind == "s":
            x0, y0, ww, wh, partial = r
            assert not partial and x0 <= 300 < x0 + ww and y0 <= 140 < y0 + wh
        else:
            assert r[2] == 0 and W * H > 16 * LC.WIN_PIXELS


def test_hqs_edge_triples():
    """E: w_in passes and w_out fails `w <= d * 1.01f` in float32; on every 'edge' triple w_in is the rounded product itself and the
    product widened to double rejects it. The reference counts exactly the points at d and w_in."""
    q, W, H, facts, frames = _frames("E_hqs_edge")
    p = frames[0][1]
    one01 = F32(1.01)
    g = q[0][0]
    for cap in (LC.WIN_PIXELS, LC.WIN_PIXELS_HQS):
        assert LC.window_rect(p, (g.min_x, g.min_y, g.min_z), (g.max_x, g.max_y, g.max_z), cap)[:4] == facts["window"]
    x0, y0, ww, wh = facts["window"]
    pix, w = las_hqs_ref.drawn_points(*q[:4], p)
    fb, _ = las_hqs_ref.render_depth(*q[:4], p)
    _, ba, _ = las_hqs_ref.render_color(*q, p, fb)
    inside = widened_rejects = f64_rejects = 0
    fine = {"n": 0, "widened": 0, "f64": 0}
    assert len(facts["triples"]) == 2900 and len({t[0] for t in facts["triples"]}) == 2900
    for pixel, d, w_in, w_out, kind in facts["triples"]:
        limit = F32(d) * one01
        assert F32(w_in) <= limit and not F32(w_out) <= limit
        if kind == "edge":
            assert float(limit) == w_in and not float(w_in) <= float(d) * float(one01)
            widened_rejects += 1
            f64_rejects += not float(w_in) <= d * 1.01
        if kind == "fine":
            assert float(limit) == w_in
            fine["n"] += 1
            fine["widened"] += not float(w_in) <= float(d) * float(one01)
            fine["f64"] += not float(w_in) <= d * 1.01
        inside += x0 <= pixel % W < x0 + ww and y0 <= pixel // W < y0 + wh
        here = w[pix == pixel]
        assert set(here.tolist()) == {float(d), float(w_in), float(w_out)}
        assert int(fb[pixel] >> np.uint64(32)) == int(F32(d).view(np.uint32))
        assert int(ba[pixel]) & 0xFFFFFFFF == int((here <= F32(w_in)).sum()) < len(here)
    assert inside == 1450 and widened_rejects == 1000
    # the fine triples: the widened product rejects some and admits others, and so does d * 1.01 in double
    assert fine["n"] == 900 and 100 < fine["widened"] < 800 and 100 < fine["f64"] < 800
    assert f64_rejects == 0          # d * 1.01 in double is 101 m or a hair above: it admits w_in, as the Huffman HQS pass would


@pytest.mark.parametrize("name", list(LC.WINDOW_CASES))
def test_window_rectangles(name):
    q, W, H, facts, frames = _frames(name)
    p = frames[0][1]
    g = q[0][0]
    lo, hi = (g.min_x, g.min_y, g.min_z), (g.max_x, g.max_y, g.max_z)
    assert g.min_z == g.max_z
    rx0, ry0, rx1, ry1 = facts["rect"]
    area = (rx1 - rx0 + 1) * (ry1 - ry0 + 1)
    for cap, window in facts["windows"].items():
        x0, y0, ww, wh, partial = LC.window_rect(p, lo, hi, cap)
        assert (x0, y0, ww, wh) == window, cap
        assert partial == (area > cap)
        if area <= cap:
            assert (x0, y0, x0 + ww - 1, y0 + wh - 1) == facts["rect"]
        elif area > 16 * cap:
            assert ww == 0
        else:
            assert 0 < ww * wh <= cap
    # one point on every pixel the case names, each with a depth of its own where two batches meet
    pix, w, index = las_hqs_ref.drawn_points(*q[:4], p, with_index=True)
    assert sorted(set(pix.tolist())) == facts["pixels"]["frame"]
    assert int((index < LC.PPB).sum()) == LC.PPB and (w[index < LC.PPB] == w[0]).all()
    if len(q[0]) == 3:
        second = pix[index >= LC.PPB]
        depth = w[index >= LC.PPB]
        first = np.unique(second, return_index=True)[1]
        assert len(set(depth[first].tolist())) == len(first) == len(facts["pixels"]["frame"])


@pytest.mark.parametrize("name", [n for n in LC.CASES if n.startswith("G_")])
def test_list_classes(name):
    """G: the class of every batch in every frame -- culled by the oracle, heavy iff the rectangle rule says the box does not fit
    the window -- and which side of `heavy * 4 < all` the frame is on."""
    q, W, H, facts, frames = _frames(name)
    for fname, p in frames:
        classes = []
        for b, g in enumerate(q[0]):
            if oracle.las_level(g, p) < 0:
                classes.append("C")
            else:
                classes.append("H" if LC.window_rect(p, (g.min_x, g.min_y, g.min_z), (g.max_x, g.max_y, g.max_z), LC.WIN_PIXELS)[4] else "L")
        assert classes == facts["classes"][fname], fname
        if "heavy_drawn" in facts:
            heavy = sum(classes[b] == "H" for b in facts["drawn"][fname])
            assert heavy == facts["heavy_drawn"][fname]
    if name == "G_list_258_under_quarter":
        assert len(facts["drawn"]["frame"]) == 257 and 64 * 4 < 257
        assert all(facts["classes"]["frame"][b] == "H" for b in (63, 64, 127, 128, 191, 192, 255, 256))
    if name == "G_list_260_quarter":
        assert len(facts["drawn"]["frame"]) == 256 == 4 * 64 and {255, 256, 257, 258} <= set(facts["drawn"]["frame"])
        assert all(facts["classes"]["frame"][b] == "H" for b in (63, 64, 127, 128, 191, 192, 255, 256))
    if name == "G_list_258_frames":
        assert [len(facts["drawn"][f]) for f, _ in facts["frames"]] == [256, 1, 0, 256]
        assert facts["heavy_drawn"]["many"] * 4 == 256 and facts["drawn"]["few"] == [256]


def test_small_lists_cover_the_orders_around_the_last_batch():
    kinds = {"".join("C" if c.islower() else c for c in k[-2:]) for k in LC.SMALL_LISTS if k.startswith("LHl")}
    assert kinds == {a + b for a in "CHL" for b in "CHL"}
    assert LC.build("G_list_llll")[8]["drawn"]["frame"] == [] and LC.build("G_list_lllL")[8]["drawn"]["frame"] == []
