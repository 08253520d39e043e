"""pcr_plane_support and pcr_select_slabs / pcr_read_slabs: plane hypotheses counted, and oriented selections made, on the GPU.

The reference of every count and selection is Context.read_points in numpy (tests/plane_cases.py: n . p in int64, for the large
hypothesis lists one float64 matmul, exact because every value is below 2^53), and the reference of the batch classes and of
every statistic is the numpy restatement of the two host plans over Context.batch_point_bounds. Every case runs for a context
loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there through both variants, which have to agree).
tests/test_plane_cpu.py checks on the CPU that the calls made here reach every branch of both plans."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import plane_cases as G
from tests import scenes
from tests.test_gpu_select import LAYOUTS, load, through_variants, xyz_of
from tests.test_plane_cpu import EDGES_SELECT

pytestmark = pytest.mark.gpu

PPB = G.PPB
PCR_E_ARG = -1
PLANE_NAMES = list(N.PlaneStats().as_dict())
SLAB_NAMES = list(N.SlabStats().as_dict())


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


_points = {}        # stream -> (read_points of the whole stream, its xyz as int64, the exact batch boxes): computed once, never changed
_support = {}       # (stream, call) -> the reference's counts and statistics
_native = {}        # id of a list of Sl -> (the list, its P.Slab objects)


def points_of(c, name):
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, xyz_of(pts).astype(np.int64), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def native(slabs):
    key = tuple(slabs)
    if key not in _native:
        _native[key] = P.as_slabs(G.native(slabs))
    return _native[key]


def support(c, hyp, clip, exclude, first=0, count=None):
    def go():
        got = c.plane_support(native(hyp), clip, native(exclude), first, count)
        return got, np.array([c.plane_stats[k] for k in PLANE_NAMES])
    got, st = through_variants(c, go)
    return got, dict(zip(PLANE_NAMES, (int(v) for v in st)))


def check_support(c, name, key, hyp, clip, exclude):
    _, xyz, bounds = _points[name]
    if (name, key) not in _support:
        plan = G.support_plan(bounds, hyp, clip, exclude)
        want = G.support(xyz, hyp, clip, exclude)
        by_plan, st = G.support_by_plan(xyz, plan, hyp, clip, exclude, count=len(hyp) <= 65)     # (the long lists are counted once, by the matmul)
        assert len(hyp) > 65 or np.array_equal(by_plan, want)
        _support[(name, key)] = (want, st)
    want, st = _support[(name, key)]
    got, gst = support(c, hyp, clip, exclude)
    assert got.dtype == np.int64 and np.array_equal(got, want), (name, key, np.nonzero(got != want)[0][:8], got[:8], want[:8])
    assert gst == st, (name, key)
    return got, gst


def select(c, slabs, clip, invert, first=0, count=None):
    def go():
        return c.read_slabs(native(slabs), clip, invert, first, count), np.array([c.slab_stats[k] for k in SLAB_NAMES])
    pts, st = through_variants(c, go)
    return pts, dict(zip(SLAB_NAMES, (int(v) for v in st)))


def check_select(c, name, slabs, clip, invert, first=0, count=None):
    pts_all, xyz, bounds = _points[name]
    last = len(pts_all) // PPB if count is None else first + count
    mask = G.selected(xyz[first * PPB:last * PPB], slabs, clip, invert)
    want = pts_all[first * PPB:last * PPB][mask]
    got, st = select(c, slabs, clip, invert, first, count)
    assert got.dtype == want.dtype and len(got) == len(want), f"{len(got)} records selected, {len(want)} expected ({name})"
    assert got.tobytes() == want.tobytes(), f"records differ, first at {np.nonzero(got != want)[0][:4]} ({name})"
    rule = G.slabs_stats(G.slabs_plan(bounds[first:last], slabs, clip, invert))
    assert st == dict(rule, points_selected=len(want)), (name, st, rule)
    return got, st, mask


# ---- 1. the constructed batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_plane_edges_support_for_every_list_size(ctx, frame):
    load(ctx, G.stream("plane_edges"), frame=frame)
    _, xyz, bounds = points_of(ctx, "plane_edges")
    assert np.array_equal(np.sort(xyz, axis=0), np.sort(G.edges_points(), axis=0))
    for nh, ne, clipped in G.EDGES_CASES:
        got, st = check_support(ctx, "plane_edges", (nh, ne, clipped), *G.edges_case(nh, ne, clipped))
        assert st["batches_decoded"] == 1 and st["exclusions_listed"] == ne and len(got) == nh
        if nh == G.MAX_HYP:
            assert st["hypotheses_max"] > 900 and (got > 0).sum() > 900
    got, _ = check_support(ctx, "plane_edges", "named", G.edges_pool()[:8], None, ())
    on = lambda group: len(G.rows_of(xyz, group))
    assert got[0] == G.in_slab(G.E_SLAB, xyz).sum() and got[0] >= on("on_lo") + on("on_hi") and got[1] == 2 and got[3] == 1
    assert got[4] == got[6] == PPB and got[5] == got[7] == 0


def test_plane_edges_branches_of_the_plan(ctx):
    load(ctx, G.stream("plane_edges"))
    points_of(ctx, "plane_edges")
    want = {"clip_holds_no_point": (0, 0, 1), "skipped_by_all_exclusion": (1, 0, 0), "open_with_all": (0, 1, 0), "not_open_with_all": (0, 0, 1), "empty_clip": (1, 0, 0)}
    for key, (hyp, clip, exclude) in G.EDGES_BRANCHES.items():
        got, st = check_support(ctx, "plane_edges", key, hyp, clip, exclude)
        assert (st["batches_skipped"], st["batches_whole"], st["batches_decoded"]) == want[key], key
    assert ctx.plane_support(native([G.E_SLAB]), None, (), 0, 0).tolist() == [0] and ctx.plane_stats["batches_skipped"] == 0      # an empty range


def test_plane_edges_selections(ctx):
    load(ctx, G.stream("plane_edges"))
    _, xyz, _ = points_of(ctx, "plane_edges")
    for slabs, clip, invert in EDGES_SELECT:
        check_select(ctx, "plane_edges", slabs, clip, invert)
    got, _, _ = check_select(ctx, "plane_edges", [G.BIG1_SLAB], None, False)
    rows = set(map(tuple, xyz_of(got).tolist()))
    assert G.P_PAIR_IN in rows and G.P_PAIR_OUT not in rows, "two points one apart in n . p, near 3 * 2^51, on either side of lo"
    got, _, _ = check_select(ctx, "plane_edges", [G.BOTTOM_SLAB], None, False)
    assert xyz_of(got).tolist() == [list(G.P_BOTTOM)]


# ---- 2. multi-batch streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.STREAMS)
def test_streams_support_and_selection(ctx, name):
    load(ctx, G.stream(name), frame=name != "clustered")
    pts, xyz, _ = points_of(ctx, name)
    calls = G.support_cases(name, xyz)
    for k, (hyp, clip, exclude) in enumerate(calls):
        got, st = check_support(ctx, name, k, hyp, clip, exclude)
    hyp, _, _ = calls[0]
    plain, _ = check_support(ctx, name, 0, *calls[0])
    for slabs, clip, invert in G.select_cases(name, xyz):
        got, st, mask = check_select(ctx, name, slabs, clip, invert)
        if not invert:                                                      # a slab and its inverse share the clip's records out between them
            inv, _ = select(ctx, slabs, clip, True)
            assert len(got) + len(inv) == G.in_clip(xyz, clip).sum()
            both = np.zeros(len(pts), bool)
            both[mask] = True
            assert pts[both].tobytes() == got.tobytes() and pts[G.in_clip(xyz, clip) & ~both].tobytes() == inv.tobytes()
        if len(slabs) == 1 and clip is None and not invert:                 # a plane's slab writes exactly its support when nothing is excluded
            j = [h.n for h in hyp].index(slabs[0].n)
            assert len(got) == plain[j]


def test_sub_ranges_add_up(ctx):
    load(ctx, G.stream("synth"))
    pts, xyz, _ = points_of(ctx, "synth")
    hyp, clip, exclude = G.support_cases("synth", xyz)[3]
    whole, _ = support(ctx, hyp, clip, exclude)
    parts = [support(ctx, hyp, clip, exclude, first, count)[0] for first, count in ((0, 3), (3, 0), (3, 4), (7, None))]
    assert np.array_equal(sum(parts), whole) and whole.sum() > 0
    for first, count in ((0, 3), (3, 4), (7, None), (10, None)):
        check_select(ctx, "synth", hyp[:2], clip, False, first, count)
        check_select(ctx, "synth", hyp[:2], clip, True, first, count)


# ---- 3. the interface ---------------------------------------------------------------------------------------------------------------------
def test_count_capacity_and_the_torch_entry(ctx):
    import torch
    load(ctx, G.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    thick, thin, half, excl = G.quantile_slabs(xyz)
    slabs, arr = [thick, half], native([thick, half])
    want = pts_all[G.selected(xyz, slabs)]
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.SlabStats()
    assert lib.pcr_select_slabs(h, 0, -1, arr, 2, None, 0, None, 0, C.byref(cnt), C.byref(st)) == 0                 # count only
    assert cnt.value == len(want) == st.points_selected > 0 and st.batches_straddling >= 1
    cnt.value = -5
    assert lib.pcr_read_slabs(h, 0, -1, arr, 2, None, 0, None, 0, C.byref(cnt), None) == 0 and cnt.value == len(want)     # stats may be NULL
    SENT = 0x5A5A5A5A
    dev = torch.full((len(want) + 16, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    torch.cuda.synchronize()
    assert lib.pcr_select_slabs(h, 0, -1, arr, 2, None, 0, C.c_void_p(dev.data_ptr()), len(want), C.byref(cnt), C.byref(st)) == 0
    got = dev.cpu().numpy()
    assert cnt.value == len(want) and got[:len(want)].tobytes() == want.tobytes() and (got[len(want):] == SENT).all()
    dev.fill_(SENT); torch.cuda.synchronize()
    cnt.value = -5
    assert lib.pcr_select_slabs(h, 0, -1, arr, 2, None, 0, C.c_void_p(dev.data_ptr()), len(want) - 1, C.byref(cnt), C.byref(st)) == PCR_E_ARG
    assert cnt.value == len(want) and (lib.pcr_last_error(h) or b"") != b""
    ctx.synchronize(); torch.cuda.synchronize()
    assert (dev.cpu().numpy() == SENT).all(), "a refused selection wrote into the buffer"
    host = np.full((len(want) + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    before = host.tobytes()
    cnt.value = -5
    assert lib.pcr_read_slabs(h, 0, -1, arr, 2, None, 0, host.ctypes.data, len(want) - 1, C.byref(cnt), None) == PCR_E_ARG
    assert cnt.value == len(want) and host.tobytes() == before
    assert lib.pcr_read_slabs(h, 0, -1, arr, 2, None, 0, host.ctypes.data, len(want), C.byref(cnt), None) == 0
    assert host[:len(want)].tobytes() == want.tobytes() and host[len(want):].tobytes() == before[len(want) * 16:]
    # Context.select_slabs: the torch tensor, with and without `out`
    t = through_variants(ctx, lambda: ctx.select_slabs(arr).cpu().numpy())
    assert t.dtype == np.int32 and t.shape == (len(want), 4) and t.tobytes() == want.tobytes() and ctx.slab_stats["points_selected"] == len(want)
    out = torch.empty((len(want) + 3, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    res = ctx.select_slabs(arr, out=out)
    assert res.is_cuda and res.dtype == torch.int32 and res.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(P.PcrError):
        ctx.select_slabs(arr, out=torch.empty((len(want) - 1, 4), dtype=torch.int32, device=out.device))
    assert ctx.slab_stats["points_selected"] == len(want)
    inv = ctx.select_slabs(arr, invert=True).cpu().numpy()
    assert inv.tobytes() == pts_all[G.selected(xyz, slabs, None, True)].tobytes() and len(inv) + len(want) == len(pts_all)
    assert tuple(ctx.select_slabs(native([G.NOTHING])).shape) == (0, 4) and ctx.slab_stats["batches_outside"] == len(xyz) // PPB
    assert len(ctx.read_slabs(arr, clip=G.S.EMPTY)) == 0 and len(ctx.read_slabs(arr, clip=G.S.EMPTY, invert=True)) == 0


def native_slab(sl, reserved=0):
    return N.Slab((C.c_int32 * 3)(*[((a + (1 << 31)) % (1 << 32)) - (1 << 31) for a in sl.n]), reserved, sl.lo, sl.hi)


def test_errors_are_pcr_e_arg_with_a_message(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    SENT = 0x5A5A5A5A
    buf = torch.full((2 * PPB + 1, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    host = np.full((2 * PPB + 1) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    good = (N.Slab * 1)(native_slab(G.EVERYTHING))
    cnt, counts = C.c_int64(), (C.c_int64 * 1025)(*([77] * 1025))

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    entries = ((lib.pcr_select_slabs, buf.data_ptr()), (lib.pcr_read_slabs, host.ctypes.data))
    for entry, dst in entries:                                              # no stream loaded
        refused(entry(h, 0, 1, good, 1, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
    refused(lib.pcr_plane_support(h, 0, 1, good, 1, None, None, 0, counts, None))
    load(ctx, G.stream("synth"))
    nb = ctx.batches_loaded
    bad = [(N.Slab * 1)(native_slab(sl, r)) for sl, r in ((G.Sl(((1 << 20) + 1, 0, 0), 0, 1), 0), (G.Sl((0, 0, -(1 << 20) - 1), 0, 1), 0),
                                                         (G.Sl((1, 2, 3), -(1 << 61) - 1, 0), 0), (G.Sl((1, 2, 3), 0, (1 << 61) + 1), 0), (G.Sl((1, 2, 3), 0, 5), 1),
                                                         (G.Sl((1, 2, 3), 0, 5), -1))]
    many = (N.Slab * 1025)(*[native_slab(G.E_SLAB)] * 1025)
    for entry, dst in entries:
        for p in bad:
            refused(entry(h, 0, 1, p, 1, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
        refused(entry(h, 0, 1, None, 1, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))                      # a NULL list
        refused(entry(h, 0, 1, good, 0, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))                      # no slab
        refused(entry(h, 0, 1, many, 17, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))                     # 17 slabs
        refused(entry(h, 0, 1, good, 1, None, 2, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))                      # an unknown flag
        refused(entry(h, 0, 1, good, 1, None, 0, C.c_void_p(dst), 2 * PPB, None, None))                              # a NULL out_count
        refused(entry(h, nb - 1, 2, good, 1, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))                 # a range outside the resident batches
        refused(entry(h, -1, 1, good, 1, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
        refused(entry(h, nb + 1, -1, good, 1, None, 0, C.c_void_p(dst), 2 * PPB, C.byref(cnt), None))
        refused(entry(h, 0, 2, good, 1, None, 0, C.c_void_p(dst), 2 * PPB - 1, C.byref(cnt), None))                  # capacity below the result
        assert cnt.value == 2 * PPB
        assert entry(h, 0, 0, good, 1, None, 0, None, 0, C.byref(cnt), None) == 0 and cnt.value == 0                 # 0 batches: succeeds
        assert entry(h, 0, 1, many, 16, None, 0, None, 0, C.byref(cnt), None) == 0                                   # 16 slabs are taken
    refused(lib.pcr_select_slabs(h, 0, 1, good, 1, None, 0, C.c_void_p(buf.data_ptr() + 4), 2 * PPB, C.byref(cnt), None))    # not 16-byte aligned
    refused(lib.pcr_read_slabs(h, 0, 1, good, 1, None, 0, C.c_void_p(host.ctypes.data + 2), PPB, C.byref(cnt), None))        # not aligned for a pcr_point
    ctx.synchronize(); torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENT).all() and (host.view(np.uint32) == SENT).all(), "a refused call wrote into its destination"
    # pcr_plane_support
    for p in bad:
        refused(lib.pcr_plane_support(h, 0, 1, p, 1, None, None, 0, counts, None))
        refused(lib.pcr_plane_support(h, 0, 1, good, 1, None, p, 1, counts, None))
    refused(lib.pcr_plane_support(h, 0, 1, None, 1, None, None, 0, counts, None))                                    # NULL hyp
    refused(lib.pcr_plane_support(h, 0, 1, good, 1, None, None, 0, None, None))                                      # NULL host_counts
    refused(lib.pcr_plane_support(h, 0, 1, good, 0, None, None, 0, counts, None))
    refused(lib.pcr_plane_support(h, 0, 1, many, 1025, None, None, 0, counts, None))
    refused(lib.pcr_plane_support(h, 0, 1, good, 1, None, None, 1, counts, None))                                    # exclusions announced, none given
    refused(lib.pcr_plane_support(h, 0, 1, good, 1, None, many, 17, counts, None))
    refused(lib.pcr_plane_support(h, 0, 1, good, 1, None, many, -1, counts, None))
    refused(lib.pcr_plane_support(h, nb - 1, 2, good, 1, None, None, 0, counts, None))
    refused(lib.pcr_plane_support(h, -1, 1, good, 1, None, None, 0, counts, None))
    assert list(counts) == [77] * 1025, "a refused call wrote counts"
    st = N.PlaneStats()
    assert lib.pcr_plane_support(h, 0, 2, many, 1024, None, many, 16, counts, C.byref(st)) == 0                      # the limits themselves are taken
    assert counts[1024] == 77 and st.batches_skipped + st.batches_whole + st.batches_decoded == 2
    # a refused call leaves the context usable
    points_of(ctx, "synth")
    check_select(ctx, "synth", list(G.quantile_slabs(_points["synth"][1])[:2]), None, False, 0, 2)


def test_calls_leave_frames_statistics_and_a_pending_frame_alone(ctx):
    load(ctx, G.stream("synth"))
    _, xyz, _ = points_of(ctx, "synth")
    thick, thin, half, excl = (native([s]) for s in G.quantile_slabs(xyz))
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    assert ctx.select_slabs(thick).shape[0] > 0 and len(ctx.read_slabs(thin, invert=True)) > 0 and ctx.plane_support(half, None, excl)[0] > 0
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    ctx.frame_begin(p); ctx.render_basic(p)
    want, want_stats = ctx.read_framebuffer(full=True), ctx.stats()
    ctx.frame_begin(p)
    ctx.read_slabs(thick); ctx.plane_support(thin, None, excl)
    ctx.render_basic(p)
    assert np.array_equal(ctx.read_framebuffer(full=True), want) and ctx.stats() == want_stats


# ---- 4. the resource, the RANSAC rounds and the CLI -----------------------------------------------------------------------------------------
def test_fit_planes_finds_the_planted_planes():
    r = P.Renderer(160, 90)
    try:
        las = P.HuffmanLasData.create(G.stream("planted"))
        las.load_all(r)
        pts = r.ctx.read_points()
        xyz = xyz_of(pts).astype(np.int64)
        slabs, supports, candidates = las.fit_planes(r, G.PLANTED_DISTANCE, num_planes=3, hypotheses=256, seed=G.PLANTED_SEED)
        assert [s.normal for s in slabs] == [p[0] for p in G.PLANTED] and all(s.lo <= d <= s.hi for s, (_, d, _) in zip(slabs, G.PLANTED))
        in_slab, planted = G.planted_supports(xyz, slabs)
        print(supports, planted, candidates)
        assert supports == in_slab and all(s >= c for s, c in zip(supports, planted)) and planted[0] > 0.39 * len(xyz)
        assert candidates == [len(xyz), len(xyz) - supports[0], len(xyz) - supports[0] - supports[1]]
        ref = P.fit_planes_rounds(lambda b: xyz[b * PPB:(b + 1) * PPB],
                                  lambda hyp, ex: G.support(xyz, [G.Sl(s.normal, s.lo, s.hi) for s in hyp], None, [G.Sl(s.normal, s.lo, s.hi) for s in ex]),
                                  len(xyz) // PPB, 1, 3, 256, G.PLANTED_SEED)
        assert [(s.normal, s.lo, s.hi) for s in ref[0]] == [(s.normal, s.lo, s.hi) for s in slabs] and ref[1:] == (supports, candidates)
        # the inliers of the first plane, through the resource: exactly its support
        sel = las.points_in_slabs(r, [slabs[0]], world=False)
        assert sel.shape[0] == supports[0] and sel.cpu().numpy().tobytes() == pts[G.in_slab(G.Sl(slabs[0].normal, slabs[0].lo, slabs[0].hi), xyz)].tobytes()
        a_fourth = las.fit_planes(r, G.PLANTED_DISTANCE, num_planes=1, hypotheses=8, seed=1, min_support=len(xyz))
        assert a_fourth[0] == [] and a_fourth[1] == [] and a_fourth[2] == [len(xyz)]
    finally:
        r.ctx.close()


SLAB_WORLD = ((500.0, 500.0, 40.0), (0.3, -0.2, 1.0), 6.0)


def test_resource_and_cli_slab_round_trip(tmp_path):
    import torch
    build.build_tools()
    image = scenes.synth_stream(600_000)[0]
    (tmp_path / "a.huffman").write_bytes(bytes(image.view()))

    def run(*cmd):
        res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        return res
    nums = [repr(v) for v in (*SLAB_WORLD[0], *SLAB_WORLD[1], SLAB_WORLD[2])]
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "all.las")
    res = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "in.las", "--slab", *nums)
    inv = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "out.las", "--slab", *nums, "--outside")
    ax, ay, az, ac, info = P.read_las(str(tmp_path / "all.las"))
    rows = np.stack([ax, ay, az], axis=1).astype(np.int64)
    sl = P.slab_from_world(info, *SLAB_WORLD)
    ref = G.Sl(sl.normal, sl.lo, sl.hi)
    box = P.box_from_world(info, tuple(info.min), tuple(info.max))
    clip = (tuple(box.min), tuple(box.max))
    assert f"normal {sl.normal[0]} {sl.normal[1]} {sl.normal[2]}, {sl.lo} .. {sl.hi}" in res.stdout, "the C++ slabFromWorld and the Python one agree"
    r = P.Renderer(160, 90)
    try:
        hl = P.HuffmanLasData.create(image)
        hl.load_all(r)
        for path, invert, text in (("in.las", False, res.stdout), ("out.las", True, inv.stdout)):
            mask = G.selected(rows, [ref], clip, invert)
            bx, by, bz, bc, blas = P.read_las(str(tmp_path / path))
            assert 0 < mask.sum() < len(ax) and len(bx) == mask.sum(), text
            assert np.array_equal(bx, ax[mask]) and np.array_equal(by, ay[mask]) and np.array_equal(bz, az[mask]) and np.array_equal(bc, ac[mask])
            assert f"written {mask.sum()}" in text and "straddling" in text and "inside" in text and "outside" in text
            xyz, pts = hl.points_in_slabs(r, [sl], invert=invert)
            pts = pts.cpu().numpy()
            assert np.array_equal(pts[:, 0], bx) and np.array_equal(pts[:, 1], by) and np.array_equal(pts[:, 2], bz) and np.array_equal(pts[:, 3].view(np.uint32), bc)
            assert xyz.dtype == torch.float64 and tuple(xyz.shape) == (len(bx), 3)
    finally:
        r.ctx.close()
    # a slab that holds no point is an error, not an empty file
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.las"), "--slab", "0", "0", "90000", "0", "0", "1", "1"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 1 and "no points" in res.stderr and not (tmp_path / "none.las").exists()
