"""pcr_select_screen / pcr_read_screen / pcr_pick: the points a frame draws, selected by screen position on the GPU.

The reference of every comparison is the oracle's point trace of one batch (tests/screen_cases.py): where every walked point of a
batch is inside the frustum the trace position names the record, and index, pixel, depth bits and colour are compared one by
one; for every drawn batch the multiset of (pixel, depth bits, colour) and the count are compared; and whatever the batch,
points == read_points()[index] byte for byte. Every case runs for a context loaded with PCR_LAYOUT_WORDS and one loaded with
PCR_LAYOUT_POINT_WINDOWS. tests/test_screen_cpu.py checks on the CPU that the cases exercise what they are meant to.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import oracle
from tests import screen_cases as SC

pytestmark = pytest.mark.gpu

PPB = SC.PPB
PCR_E_ARG = -1
LAYOUTS = {"words": P.Context.LAYOUT_WORDS, "point_windows": P.Context.LAYOUT_POINT_WINDOWS}
EMPTY_RECTS = [(5, 5, 4, 9), (0, 7, 10, 6), (-20, -20, -1, -1), (100000, 0, 100010, 10)]


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    yield c
    c.close()


def load(c, sname, p, frame=True):
    """The stream resident in the context, the image sized for the camera; frame: one HQS depth frame drawn first (it releases
    what only the load-time transcode reads)."""
    f = P.HuffmanFile(SC.stream(sname))
    if c.batches_loaded:
        c.stream_unload()
    c.stream_begin(f.header(0, f.numBatches), 0)
    for i in range(f.numBatches):
        c.upload_batch(i, f.blob(i))
    c.set_image_size(p.width, p.height)
    if frame:
        c.clear(); c.render_hqs_depth(p); c.synchronize()
    return f


def count_only(c, p, rect):
    cnt, st = C.c_int64(-5), N.ScreenStats()
    r = P.as_rect(rect)
    rc = c.lib.pcr_select_screen(c.h, C.byref(p), C.byref(r) if r is not None else None, None, None, 0, C.byref(cnt), C.byref(st))
    assert rc == 0, c.lib.pcr_last_error(c.h)
    return cnt.value, st.as_dict()


def check_case(c, name, frame=True):
    """Checks 1 to 3 of one case; returns (points, hits, reference)."""
    sname, of, p, rect = SC.case(name)
    load(c, sname, p, frame)
    pts, hits = c.read_screen(p, rect)
    st = dict(c.screen_stats)
    ref = SC.reference(sname, p, rect)
    everything = c.read_points()
    assert pts.dtype == P.POINT_DTYPE and hits.dtype == P.HIT_DTYPE and len(pts) == len(hits)
    index = hits["index"]
    # 3. always
    assert (np.diff(index) > 0).all(), "index is not strictly increasing"
    assert len(index) == 0 or (index[0] >= 0 and index[-1] < len(everything))
    assert pts.tobytes() == everything[index].tobytes(), "points differ from read_points()[index]"
    want_total = sum(len(r["pix"]) for r in ref)
    assert len(hits) == want_total, f"{len(hits)} records selected, the trace has {want_total}"
    n, st2 = count_only(c, p, rect)
    assert n == len(hits) and st2 == st and st["points_selected"] == n
    drawn = [r["drawn"] for r in ref]
    assert st["batches_decoded"] == sum(drawn) and st["batches_skipped"] == len(ref) - sum(drawn)
    assert st["points_tested"] == sum(r["npr"] * 1024 for r in ref if r["drawn"])
    # 2. every drawn batch: the multiset of (pixel, depth bits, colour); 1. the batches wholly inside: record by record
    batch = index // PPB
    exact = 0
    for b, r in enumerate(ref):
        m = batch == b
        got = SC.sorted_triples(hits["pixel"][m], hits["depth_bits"][m], pts["color"][m])
        want = SC.sorted_triples(r["pix"], r["depth"], r["colour"])
        assert got.shape == want.shape, f"batch {b}: {len(got)} hits, the trace has {len(want)}"
        assert np.array_equal(got, want), f"batch {b}: the (pixel, depth bits, colour) multisets differ"
        if r["full"]:
            order = np.argsort(r["index"], kind="stable")
            assert np.array_equal(index[m], r["index"][order]), f"batch {b}: other records selected than the trace names"
            assert np.array_equal(hits["pixel"][m].astype(np.int64), r["pix"][order]), f"batch {b}: pixels differ"
            assert np.array_equal(hits["depth_bits"][m], r["depth"][order]), f"batch {b}: depth bits differ"
            assert np.array_equal(pts["color"][m], r["colour"][order]), f"batch {b}: colours differ"
            exact += int(m.sum())
    if name in SC.PRECONDITIONED and want_total:
        assert 2 * exact >= want_total                     # the hold-out condition, restated where it matters
    return p, rect, pts, hits, ref


# ---- 1 - 3: the preconditioned cameras -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.PRECONDITIONED + ["synth_inside", "tie_all", "tie_all_bc7", "tie_320"])
def test_selection_equals_the_oracles_trace(ctx, name):
    check_case(ctx, name)


@pytest.mark.parametrize("name", ["synth_cull_rect", "clustered_cull_lod", "tie_all_bc7"])
def test_selection_before_any_frame(ctx, name):
    check_case(ctx, name, frame=False)


# ---- 4: streams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.STREAM_CASES)
def test_special_streams(ctx, name):
    check_case(ctx, name)


# ---- 3: rects, capacity, state -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synth_cull", "clustered_down"])
def test_null_rect_is_the_full_image_rect_and_flags_do_not_matter(ctx, name):
    sname, of, p, _ = SC.case(name)
    load(ctx, sname, p)
    a = ctx.read_screen(p, None)
    b = ctx.read_screen(p, (0, 0, p.width - 1, p.height - 1))
    c = ctx.read_screen(p, (-7, -7, p.width + 5, p.height + 5))          # clipped to the image
    q = p.copy(); q.show_num_points = 1; q.colorize_chunks = 1
    d = ctx.read_screen(q, None)
    for o in (b, c, d):
        assert o[0].tobytes() == a[0].tobytes() and o[1].tobytes() == a[1].tobytes()
    assert len(a[0]) > 0


def test_empty_rects_and_empty_contexts_select_nothing(ctx):
    sname, of, p, _ = SC.case("synth_overview")
    load(ctx, sname, p)
    for rect in EMPTY_RECTS:
        pts, hits = ctx.read_screen(p, rect)
        assert len(pts) == 0 and len(hits) == 0 and ctx.screen_stats["points_selected"] == 0
        assert count_only(ctx, p, rect)[0] == 0
    assert ctx.pick(p, -50, -50, 3) is None
    ctx.stream_unload()
    f = P.HuffmanFile(SC.stream(sname))
    ctx.stream_begin(f.header(0, f.numBatches), 0)                         # a stream with no batch resident yet
    assert len(ctx.read_screen(p, None)[0]) == 0 and ctx.pick(p, 10, 10, 2) is None


def test_short_capacity_is_refused_with_the_count_and_nothing_written(ctx):
    import torch
    sname, of, p, rect = SC.case("synth_cull_rect")
    load(ctx, sname, p)
    pts, hits = ctx.read_screen(p, rect)
    n = len(pts)
    assert n > 1000
    r = P.as_rect(rect)
    # host
    hp, hh = np.full(n, 0x5A, np.uint8).repeat(16), np.full(n, 0xA5, np.uint8).repeat(16)
    cnt = C.c_int64()
    rc = ctx.lib.pcr_read_screen(ctx.h, C.byref(p), C.byref(r), hp.ctypes.data, hh.ctypes.data, n - 1, C.byref(cnt), None)
    assert rc == PCR_E_ARG and cnt.value == n and (hp == 0x5A).all() and (hh == 0xA5).all()
    assert b"capacity" in ctx.lib.pcr_last_error(ctx.h)
    # device
    dp = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dh = torch.full((n, 2), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.pcr_select_screen(ctx.h, C.byref(p), C.byref(r), C.c_void_p(dp.data_ptr()), C.c_void_p(dh.data_ptr()), n - 1, C.byref(cnt), None)
    assert rc == PCR_E_ARG and cnt.value == n
    assert bool((dp == 0x5A5A5A5A).all()) and bool((dh == 0x5A5A5A5A).all())
    # the exact capacity is enough, either array alone works, and the device path returns what the host path returns
    rc = ctx.lib.pcr_select_screen(ctx.h, C.byref(p), C.byref(r), C.c_void_p(dp.data_ptr()), None, n, C.byref(cnt), None)
    assert rc == 0 and cnt.value == n and dp.cpu().numpy().tobytes() == pts.tobytes() and bool((dh == 0x5A5A5A5A).all())
    rc = ctx.lib.pcr_select_screen(ctx.h, C.byref(p), C.byref(r), None, C.c_void_p(dh.data_ptr()), n, C.byref(cnt), None)
    assert rc == 0 and dh.cpu().numpy().tobytes() == hits.tobytes()
    tp, th = ctx.select_screen(p, rect)
    assert tp.dtype == torch.int32 and th.dtype == torch.int64 and tuple(tp.shape) == (n, 4) and tuple(th.shape) == (n, 2)
    assert tp.cpu().numpy().tobytes() == pts.tobytes() and th.cpu().numpy().tobytes() == hits.tobytes()
    assert np.array_equal((th[:, 0] & 0xFFFFFFFF).cpu().numpy(), hits["pixel"].astype(np.int64))
    assert np.array_equal((th[:, 0] >> 32).cpu().numpy(), hits["depth_bits"].astype(np.int64)) and np.array_equal(th[:, 1].cpu().numpy(), hits["index"])
    # a misaligned device pointer, a NULL out_count
    rc = ctx.lib.pcr_select_screen(ctx.h, C.byref(p), C.byref(r), C.c_void_p(dp.data_ptr() + 4), None, n, C.byref(cnt), None)
    assert rc == PCR_E_ARG
    assert ctx.lib.pcr_select_screen(ctx.h, C.byref(p), C.byref(r), None, None, 0, None, None) == PCR_E_ARG


@pytest.mark.parametrize("name", ["synth_cull_rect", "clustered_cull_lod", "tie_all_bc7"])
def test_a_frame_drawn_after_a_select_is_the_oracles(ctx, name):
    """... with the select between pcr_frame_begin and the render call, where the prepass of the frame is pending, and with a
    select for ANOTHER camera there."""
    sname, of, p, rect = SC.case(name)
    load(ctx, sname, p, frame=False)
    bc7 = ctx.stream_color_format() == 7
    other = SC.case("synth_far_lod")[2].copy()
    other.width, other.height = p.width, p.height
    want = (of.render_hqs_depth(p) if bc7 else of.render_basic(p))[0]

    def draw():
        (ctx.render_hqs_depth if bc7 else ctx.render_basic)(p)
        stats = ctx.stats()
        return ctx.read_framebuffer(full=True), stats
    ctx.frame_begin(p, hqs=bc7)
    plain, plain_stats = draw()
    assert np.array_equal(plain, want)
    for q, r in ((p, rect), (other, None)):
        ctx.frame_begin(p, hqs=bc7)
        ctx.read_screen(q, r)
        ctx.pick(q, p.width // 2, p.height // 2, 2)
        fb, stats = draw()
        assert np.array_equal(fb, want), "a select between frame_begin and the render call changed the frame"
        assert stats == plain_stats, "a select changed the render statistics"
    ctx.clear(); ctx.read_screen(p, rect)
    fb, _ = draw()
    assert np.array_equal(fb, want)


# ---- 5: pick ---------------------------------------------------------------------------------------------------------------------
def hit_key(pt, hit):
    return (int(hit.depth_bits) << 32) | int(pt.color)


@pytest.mark.parametrize("name", [SC.PICK_CASE, "clustered_down"])
def test_pick_at_radius_0_is_the_word_render_basic_leaves(ctx, name):
    sname, of, p, _ = SC.case(name)
    load(ctx, sname, p)
    fb = of.render_basic(p)[0]
    pts, hits = ctx.read_screen(p, None)
    rng = np.random.default_rng(9)
    occupied = np.nonzero(fb[:p.width * p.height] != oracle_empty())[0]
    empty = np.nonzero(fb[:p.width * p.height] == oracle_empty())[0]
    sample = np.concatenate([rng.choice(occupied, min(250, len(occupied)), replace=False), rng.choice(empty, min(100, len(empty)), replace=False)])
    assert len(occupied) and len(empty)
    for pix in sample:
        got = ctx.pick(p, int(pix % p.width), int(pix // p.width), 0)
        if fb[pix] == oracle_empty():
            assert got is None, f"pixel {pix} is empty in the oracle's frame"
            continue
        assert got is not None, f"pixel {pix} is occupied in the oracle's frame"
        pt, hit = got
        assert hit.pixel == pix and hit_key(pt, hit) == int(fb[pix]), f"pixel {pix}"
        k = np.searchsorted(hits["index"], hit.index)
        assert hits["index"][k] == hit.index and hits["pixel"][k] == pix and hits["depth_bits"][k] == hit.depth_bits
        assert bytes(pt) == pts[k].tobytes()


def oracle_empty():
    return np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.mark.parametrize("name", [SC.PICK_CASE, "tie_all_bc7", "clustered_cull_lod"])
def test_pick_in_a_window_is_the_minimum_over_the_windows_hits(ctx, name):
    sname, of, p, _ = SC.case(name)
    load(ctx, sname, p)
    pts, hits = ctx.read_screen(p, None)
    pix, depth, colour, index = hits["pixel"].astype(np.int64), hits["depth_bits"], pts["color"], hits["index"]
    rng = np.random.default_rng(4)
    # twenty centres anywhere (off the image's edge too), twenty on pixels that hold a hit: every window of those holds one
    centres = [(int(x), int(y)) for x, y in zip(rng.integers(-4, p.width + 4, 20), rng.integers(-4, p.height + 4, 20))]
    centres += [(int(v % p.width), int(v // p.width)) for v in rng.choice(pix, 20)]
    found = 0
    for (px, py) in centres:
        for radius in SC.PICK_RADII:
            want = SC.pick_reference(pix, depth, colour, index, p, px, py, radius)
            got = ctx.pick(p, px, py, radius)
            assert (got is None) == (want is None), (px, py, radius)
            if got is not None:
                w = want[0]
                assert (got[1].index, got[1].pixel, got[1].depth_bits) == (index[w], pix[w], depth[w]), (px, py, radius)
                assert bytes(got[0]) == pts[w].tobytes()
                found += 1
    assert found >= 20 * len(SC.PICK_RADII)


def test_pick_breaks_a_tie_of_depth_and_colour_by_the_lowest_index(ctx):
    sname, of, p, _ = SC.case(SC.PICK_CASE)
    load(ctx, sname, p)
    pts, hits = ctx.read_screen(p, None)
    px, py = SC.PICK_TIE
    w, tied = SC.pick_reference(hits["pixel"].astype(np.int64), hits["depth_bits"], pts["color"], hits["index"], p, px, py, 0)
    assert tied > 1
    m = (hits["pixel"] == px + py * p.width) & (hits["depth_bits"] == hits["depth_bits"][w]) & (pts["color"] == pts["color"][w])
    assert m.sum() == tied and hits["index"][m].min() == hits["index"][w] and hits["index"][m].max() > hits["index"][w]
    pt, hit = ctx.pick(p, px, py, 0)
    assert hit.index == hits["index"][w] and bytes(pt) == pts[w].tobytes()
    with pytest.raises(P.PcrError):
        ctx.pick(p, px, py, -1)


# ---- upper layers ----------------------------------------------------------------------------------------------------------------
def test_points_on_screen_of_the_resource():
    import torch
    sname, of, p, rect = SC.case("clustered_rect")
    r = P.Renderer(p.width, p.height)
    d = P.HuffmanLasData.create(SC.stream(sname))
    d.load_all(r)
    want_pts, want_hits = r.ctx.read_screen(p, rect)
    xyz, pts, hits = d.points_on_screen(r, p, rect)
    assert pts.cpu().numpy().tobytes() == want_pts.tobytes() and hits.cpu().numpy().tobytes() == want_hits.tobytes()
    info = d.las_info()
    want_xyz = np.stack([want_pts[k].astype(np.float64) * info.scale[i] + info.offset[i] for i, k in enumerate("xyz")], axis=1)
    assert xyz.dtype == torch.float64 and np.array_equal(xyz.cpu().numpy(), want_xyz)
    r.params_override = p
    P.Debug.LOD = p.lod_percent / 100.0
    try:
        pts2, hits2 = d.points_on_screen(r, None, rect, world=False)
    finally:
        P.Debug.LOD = 0.1
    assert pts2.cpu().numpy().tobytes() == want_pts.tobytes() and hits2.cpu().numpy().tobytes() == want_hits.tobytes()
    r.ctx.close()


# ---- 6: the CLI ------------------------------------------------------------------------------------------------------------------
VIEW = ["--size", "320x200", "--camera", "0.0", "-1.5", "700", "500", "900", "20", "--lod", "0.1"]


def cli_case():
    sname = "clustered"
    p = SC._orbit(0.0, -1.5, 700.0, (500.0, 900.0, 20.0), 320, 200, lod=10)
    return sname, p


def test_cli_decode_view_rect_writes_the_selection(tmp_path):
    build.build_tools()
    sname, p = cli_case()
    rect = (40, 30, 250, 170)
    src, out = tmp_path / "in.huffman", tmp_path / "out.las"
    src.write_bytes(bytes(SC.stream(sname)))
    res = subprocess.run([build.DECODE_BIN, str(src), str(out), "--view", *VIEW, "--rect", *(str(v) for v in rect)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    c = P.Context(0)
    try:
        load(c, sname, p, frame=False)
        pts, hits = c.read_screen(p, rect)
    finally:
        c.close()
    assert len(pts) > 1000
    x, y, z, colour, las = P.read_las(str(out))
    assert len(x) == len(pts)
    assert np.array_equal(x, pts["x"]) and np.array_equal(y, pts["y"]) and np.array_equal(z, pts["z"]) and np.array_equal(colour, pts["color"])


def test_cli_render_pick_prints_the_picked_point(tmp_path):
    build.build_tools()
    sname, p = cli_case()
    src = tmp_path / "in.huffman"
    src.write_bytes(bytes(SC.stream(sname)))
    c = P.Context(0)
    try:
        load(c, sname, p, frame=False)
        pts, hits = c.read_screen(p, None)
        pix = int(hits["pixel"][len(hits) // 2])
        px, py = pix % p.width, pix // p.width
        want = c.pick(p, px, py, 2)
    finally:
        c.close()
    assert want is not None
    res = subprocess.run([build.RENDER_BIN, str(src), *VIEW, "--pick", str(px), str(py), "2"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("pick ")]
    assert len(line) == 1, res.stdout
    pt, hit = want
    assert line[0] == (f"pick x={pt.x} y={pt.y} z={pt.z} color=0x{pt.color:06x} index={hit.index} pixel={hit.pixel} "
                       f"px={hit.pixel % p.width} py={hit.pixel // p.width} depth_bits=0x{hit.depth_bits:08x}"), line[0]
    res = subprocess.run([build.RENDER_BIN, str(src), *VIEW, "--pick", "-30", "-30"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0 and "pick none" in res.stdout.splitlines()
