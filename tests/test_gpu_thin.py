"""pcr_thin / pcr_read_thin: one record per voxel of a cubic lattice, thinned on the GPU straight from the compressed stream.

The contract: of the rows pcr_decode_points writes for the range that lie inside the clip, exactly one per non-empty voxel is
kept -- the lowest row (FIRST) or the least by (d2, row) (CENTER) -- and the kept records and their rows come out byte for byte, in
increasing row order. So the reference of every call here is Context.read_points of the same range, reduced in numpy
(tests/thin_cases.py: int64 floor_divide, np.unique / np.lexsort), colours included. Every case runs for a context loaded with
PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there through both variants, which have to agree), as
tests/test_gpu_select.py does. tests/test_thin_cpu.py checks on the CPU that the streams and lattices used here have voxels that
span batches and chains, runs, chains that come back to a voxel, CENTER winners that are not the FIRST ones and ties in d2."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import oracle, scenes
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_gpu_select import LAYOUTS, load, one_frame, through_variants, variants

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
BIG = ("synth", "clustered", "garbage_tail")        # 5 and 10 batches: these run every second combination (all cells, origins, modes)
STAT_NAMES = list(N.ThinStats().as_dict())


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


_points = {}        # stream -> (read_points of the whole stream, its xyz as int64, the exact batch boxes): computed once, never changed
_wanted = {}        # (stream, first, count, vox, clip, mode) -> (kept rows, runs, candidates)


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, T.xyz_of(pts), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def wanted(name, vox, clip, mode, first=0, count=None):
    key = (name, first, count, vox, clip, mode)
    if key not in _wanted:
        xyz = _points[name][1]
        xyz = xyz[first * PPB:len(xyz) if count is None else (first + count) * PPB]
        _wanted[key] = (T.reference(xyz, vox, clip, mode), T.count_runs(xyz, vox, clip), int(T.candidates(xyz, clip).sum()))
    return _wanted[key]


def thin(c, vox, clip, mode, first=0, count=None):
    """read_thin of the range with the rows (both variants) and the statistics it reported."""
    def go():
        pts, rows = c.read_thin(vox, clip, mode, first, count, rows=True)
        return pts, rows, np.array([c.thin_stats[k] for k in STAT_NAMES])
    pts, rows, st = through_variants(c, go)
    return pts, rows, dict(zip(STAT_NAMES, (int(v) for v in st)))


def check_thin(c, name, vox, clip, mode, first=0, count=None):
    """read_thin == the reference over read_points of the same range, byte for byte, rows and statistics included; or, where
    the lattice limits say so, a refusal that names the way out."""
    pts_all, _, bounds = _points[name]
    last = len(pts_all) // PPB if count is None else first + count
    refusal = T.lattice_refusal(bounds[first:last], vox, clip)
    if refusal:
        with pytest.raises(P.PcrError, match="clip or a larger cell"):
            c.read_thin(vox, clip, mode, first, count)
        return None
    rows, runs, cand = wanted(name, vox, clip, mode, first, count)
    got, got_rows, st = thin(c, vox, clip, mode, first, count)
    want = pts_all[first * PPB:last * PPB][rows]
    assert got.dtype == want.dtype and got_rows.dtype == np.int64
    assert len(got) == len(want) == len(got_rows), f"{len(got)} records kept, {len(want)} expected ({name} {vox} {clip} mode {mode})"
    assert np.array_equal(got_rows, rows), f"rows differ, first at {np.nonzero(got_rows != rows)[0][:4]} ({name} {vox} {clip} mode {mode})"
    assert got.tobytes() == want.tobytes(), f"records differ ({name} {vox} {clip} mode {mode})"
    dec = T.decoded_batches(bounds[first:last], clip)
    assert st == dict(batches_outside=last - first - dec, batches_decoded=dec, points_considered=cand, runs=runs, points_kept=len(rows),
                      table_slots=T.table_slots(runs)), (name, vox, clip, mode)
    return got, got_rows, st


def combos_of(name):
    for cell, o, mode, clipped in (T.COMBOS[::2] if name in BIG else T.COMBOS):
        yield (*T.ORIGINS[o], cell), mode, clipped or name == "garbage_tail"     # (garbage_tail: always with a clip, see test 6)


# ---- 1. against the numpy reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.STREAMS)
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_thinning_equals_the_reference(ctx, name, frame):
    load(ctx, T.stream(name), frame=frame)
    _, xyz, _ = points_of(ctx, name)
    clip = T.clip_for(name, xyz)
    done = 0
    for vox, mode, clipped in combos_of(name):
        out = check_thin(ctx, name, vox, clip if clipped else None, mode)
        if out:
            done += 1
            print(f"{name} vox {vox} mode {mode} clip {clip if clipped else None}: {out[2]}")
    assert done >= (4 if name == "wide30" else 8)                            # (wide30 without a clip is refused at every cell)
    if not frame:                                                           # ... and the first frame changes nothing
        vox, mode, clipped = next(iter(combos_of(name)))
        before = ctx.read_thin(vox, clip if clipped or name == "wide30" else None, mode, rows=True)
        one_frame(ctx)
        after = ctx.read_thin(vox, clip if clipped or name == "wide30" else None, mode, rows=True)
        assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("name,cell,origin,clip,needs", T.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_preconditioned_cases(ctx, name, cell, origin, clip, needs):
    """The cases tests/test_thin_cpu.py proves hard: voxels over batches and chains, re-entered voxels, CENTER != FIRST, d2 ties."""
    load(ctx, T.stream(name))
    _, xyz, _ = points_of(ctx, name)
    clip = T.case_clip(name, clip, xyz)
    for mode in (T.FIRST, T.CENTER) if cell <= T.MAX_CENTER_CELL else (T.FIRST,):
        got, rows, st = check_thin(ctx, name, (*origin, cell), clip, mode)
        assert 0 < len(rows) < st["points_considered"]
        print(f"{name} cell {cell} mode {mode}: {st}")


# ---- 2. edge cases ------------------------------------------------------------------------------------------------------------------
def test_edge_cases(ctx):
    load(ctx, T.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    nb = len(pts_all) // PPB
    # the largest cell: a handful of records
    for o in T.ORIGINS:
        got, rows, st = check_thin(ctx, "synth", (*o, T.MAX_CELL), None, T.FIRST)
        assert 1 <= len(rows) <= 8 and rows[0] == 0
    # a clip on a single known point (a padding duplicate may put more than one candidate there: still one record)
    for k in (0, len(pts_all) // 2 + 777, len(pts_all) - 1):
        pt = tuple(int(v) for v in xyz[k])
        for mode in (T.FIRST, T.CENTER):
            got, rows, st = check_thin(ctx, "synth", (0, 0, 0, 64), (pt, pt), mode)
            assert len(rows) == 1 and rows[0] <= k and (T.xyz_of(got) == np.array(pt)).all() and st["points_considered"] >= 1
    # the empty clip, and a clip that misses everything: no batch decoded, no kernel runs, the context stays usable
    for clip in (S.EMPTY, S.NOTHING):
        got, rows, st = check_thin(ctx, "synth", (0, 0, 0, 1000), clip, T.CENTER)
        assert len(got) == 0 and len(rows) == 0
        assert st == dict(batches_outside=nb, batches_decoded=0, points_considered=0, runs=0, points_kept=0, table_slots=0)
    # count == 0, at either end of the stream
    for first in (0, 3, nb):
        got, rows, st = thin(ctx, (0, 0, 0, 1000), None, T.FIRST, first, 0)
        assert len(got) == 0 and st["batches_outside"] == 0 and st["batches_decoded"] == 0
    check_thin(ctx, "synth", (0, 0, 0, 1000), None, T.CENTER)


# ---- 3. counting, capacity --------------------------------------------------------------------------------------------------------
def test_count_then_exact_capacity_then_one_short(ctx):
    import torch
    load(ctx, T.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    vt, clip_t, mode = (-12345, 777, -1, 2047), S.BOXES["synth"], T.CENTER
    rows, _, _ = wanted("synth", vt, clip_t, mode)
    want, n = pts_all[rows], len(rows)
    assert n > 1000
    vox, box = P.as_voxels(vt), P.as_box(clip_t)
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.ThinStats()

    def dev_call(points, rws, cap, stats=st):
        return lib.pcr_thin(h, 0, -1, C.byref(vox), C.byref(box), mode, C.c_void_p(points), C.c_void_p(rws), cap, C.byref(cnt), stats)

    def host_call(points, rws, cap, stats=None):
        return lib.pcr_read_thin(h, 0, -1, C.byref(vox), C.byref(box), mode, C.c_void_p(points), C.c_void_p(rws), cap, C.byref(cnt), stats)

    # count only: both destinations NULL, on the device and on the host
    assert dev_call(None, None, 0) == 0 and cnt.value == n == st.points_kept
    cnt.value = -5
    assert host_call(None, None, 0) == 0 and cnt.value == n                 # stats may be NULL
    SENT = 0x5A5A5A5A
    dev = torch.full((n + 16, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    drows = torch.full((n + 16,), SENT, dtype=torch.int64, device=dev.device)

    def reset():
        dev.fill_(SENT); drows.fill_(SENT); torch.cuda.synchronize(); cnt.value = -5

    # exact capacity: points only, rows only, both
    for with_points, with_rows in ((True, False), (False, True), (True, True)):
        reset()
        assert dev_call(dev.data_ptr() if with_points else None, drows.data_ptr() if with_rows else None, n) == 0 and cnt.value == n
        gp, gr = dev.cpu().numpy(), drows.cpu().numpy()
        assert (gp[:n].tobytes() == want.tobytes()) if with_points else (gp == SENT).all()
        assert np.array_equal(gr[:n], rows) if with_rows else (gr == SENT).all()
        assert (gp[n:] == SENT).all() and (gr[n:] == SENT).all()
    # one short: PCR_E_ARG, *out_count = the count needed, nothing written
    for with_points, with_rows in ((True, False), (False, True), (True, True)):
        reset()
        assert dev_call(dev.data_ptr() if with_points else None, drows.data_ptr() if with_rows else None, n - 1) == PCR_E_ARG
        assert cnt.value == n and (lib.pcr_last_error(h) or b"") != b""
        ctx.synchronize(); torch.cuda.synchronize()
        assert (dev.cpu().numpy() == SENT).all() and (drows.cpu().numpy() == SENT).all(), "a refused thinning wrote into a buffer"
    # the same on the host
    host = np.full((n + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    hrows = np.full(n + 4, SENT, np.int64)
    before, rbefore = host.tobytes(), hrows.tobytes()
    cnt.value = -5
    assert host_call(host.ctypes.data, hrows.ctypes.data, n - 1) == PCR_E_ARG
    assert cnt.value == n and host.tobytes() == before and hrows.tobytes() == rbefore
    assert host_call(host.ctypes.data, None, n) == 0
    assert host[:n].tobytes() == want.tobytes() and host[n:].tobytes() == before[n * 16:] and hrows.tobytes() == rbefore
    host[:] = np.frombuffer(before, P.POINT_DTYPE)
    assert host_call(None, hrows.ctypes.data, n) == 0
    assert np.array_equal(hrows[:n], rows) and (hrows[n:] == SENT).all() and host.tobytes() == before
    assert host_call(host.ctypes.data, hrows.ctypes.data, n) == 0
    assert host[:n].tobytes() == want.tobytes() and np.array_equal(hrows[:n], rows) and host[n:].tobytes() == before[n * 16:]
    # Context.thin: the torch tensors, with and without `out` and rows
    t = ctx.thin(vt, clip_t, "center")
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (n, 4) and t.cpu().numpy().tobytes() == want.tobytes()
    assert ctx.thin_stats["points_kept"] == n
    t2, r2 = ctx.thin(vt, clip_t, "center", rows=True)
    assert torch.equal(t2, t) and r2.dtype == torch.int64 and np.array_equal(r2.cpu().numpy(), rows)
    out = torch.empty((n + 3, 4), dtype=torch.int32, device=t.device)
    assert torch.equal(ctx.thin(vt, clip_t, "center", out=out), t)
    with pytest.raises(P.PcrError):
        ctx.thin(vt, clip_t, "center", out=torch.empty((n - 1, 4), dtype=torch.int32, device=t.device))
    assert ctx.thin_stats["points_kept"] == n
    assert tuple(ctx.thin(vt, S.EMPTY).shape) == (0, 4)
    with pytest.raises(ValueError):
        ctx.thin(vt, clip_t, "centre")


# ---- 4. sub-ranges --------------------------------------------------------------------------------------------------------------------
def test_sub_ranges_thin_their_own_rows(ctx):
    """Thinning [first, first + count) is the reference over that range's rows: a voxel that spans the cut is kept once per range."""
    load(ctx, T.stream("synth"))
    pts_all, _, _ = points_of(ctx, "synth")
    nb = len(pts_all) // PPB
    vox = (0, 0, 0, 7001)
    whole = check_thin(ctx, "synth", vox, None, T.FIRST)[1]
    total = 0
    for first, count in ((0, 3), (3, 1), (4, 0), (4, 5), (9, None)):
        for mode, v in ((T.FIRST, vox), (T.CENTER, (-12345, 777, -1, 2048))):
            rows = check_thin(ctx, "synth", v, S.BOXES["synth"] if first == 4 else None, mode, first, count)[1]
            assert len(rows) == 0 or (0 <= rows[0] and rows[-1] < (nb - first if count is None else count) * PPB)   # rows count from the range's start
        total += len(check_thin(ctx, "synth", vox, None, T.FIRST, first, count)[1])
    assert total > len(whole), "no voxel of the lattice spans a cut between the ranges: the case shows nothing"
    got, rows, st = thin(ctx, vox, None, T.FIRST, nb, None)
    assert len(got) == 0 and st["batches_outside"] == 0


# ---- 5. the scratch is cleared and regrown; run-to-run equality ----------------------------------------------------------------------
def test_calls_in_a_row_do_not_see_each_other(ctx):
    load(ctx, T.stream("synth"))
    points_of(ctx, "synth")
    a = ((0, 0, 0, 7001), None, T.FIRST)                    # a small table ...
    b = ((-12345, 777, -1, 64), None, T.CENTER)             # ... a large one, most slots taken by other keys, other rows flagged ...
    c = ((0, 0, 0, 1 << 20), S.BOXES["synth"], T.FIRST)     # ... and a tiny one
    first = check_thin(ctx, "synth", *a)
    assert check_thin(ctx, "synth", *b)[2]["table_slots"] > first[2]["table_slots"]
    assert check_thin(ctx, "synth", *c)[2]["table_slots"] < first[2]["table_slots"]
    again = check_thin(ctx, "synth", *a)
    assert again[0].tobytes() == first[0].tobytes() and np.array_equal(again[1], first[1]) and again[2] == first[2]
    for call in (b, b, a, a):
        x, y = ctx.read_thin(*call, rows=True), ctx.read_thin(*call, rows=True)
        assert x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_are_pcr_e_arg_with_a_message(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    buf = torch.empty((2 * PPB + 1, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    rbuf = torch.empty(2 * PPB + 1, dtype=torch.int64, device=buf.device)
    host, hrows = np.empty(2 * PPB + 1, P.POINT_DTYPE), np.empty(2 * PPB + 1, np.int64)
    vox = P.as_voxels((0, 0, 0, 1000))
    cnt = C.c_int64()
    entries = ((lib.pcr_thin, buf.data_ptr(), rbuf.data_ptr()), (lib.pcr_read_thin, host.ctypes.data, hrows.ctypes.data))

    def call(entry, first, count, v, mode, points, rows, out=cnt, cap=2 * PPB, clip=None):
        return entry(h, first, count, None if v is None else C.byref(v), None if clip is None else C.byref(clip), mode, C.c_void_p(points), C.c_void_p(rows),
                     cap, None if out is None else C.byref(out), None)

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    def still_fine():
        check_thin(ctx, "synth", (0, 0, 0, 7001), None, T.FIRST, 0, 2)

    for entry, dp, dr in entries:                                           # no stream loaded
        refused(call(entry, 0, 1, vox, T.FIRST, dp, dr))
    load(ctx, T.stream("synth"))
    points_of(ctx, "synth")
    nb = ctx.batches_loaded
    for entry, dp, dr in entries:
        for first, count in ((nb - 1, 2), (-1, 1), (nb + 1, -1)):           # a range outside the resident batches
            refused(call(entry, first, count, vox, T.FIRST, dp, dr))
        refused(call(entry, 0, 1, None, T.FIRST, dp, dr))                   # a NULL lattice
        refused(call(entry, 0, 1, vox, T.FIRST, dp, dr, out=None))          # a NULL out_count
        still_fine()
        for cell in (0, -1, T.MAX_CELL + 1):
            refused(call(entry, 0, 1, P.as_voxels((0, 0, 0, cell)), T.FIRST, dp, dr))
        refused(call(entry, 0, 1, P.as_voxels((0, 0, 0, T.MAX_CENTER_CELL + 1)), T.CENTER, dp, dr))
        assert call(entry, 0, 1, P.as_voxels((0, 0, 0, T.MAX_CENTER_CELL + 1)), T.FIRST, dp, dr) == 0
        assert call(entry, 0, 1, P.as_voxels((0, 0, 0, T.MAX_CENTER_CELL)), T.CENTER, dp, dr) == 0
        for mode in (7, -1, 2):
            refused(call(entry, 0, 1, vox, mode, dp, dr))
        still_fine()
        refused(call(entry, 0, 2, P.as_voxels((0, 0, 0, 1)), T.FIRST, dp, dr, cap=1000))            # capacity below the result
        assert cnt.value > 1000
        assert call(entry, 0, 0, vox, T.FIRST, None, None, cap=0) == 0 and cnt.value == 0           # 0 batches: succeeds
    refused(call(lib.pcr_thin, 0, 1, vox, T.FIRST, buf.data_ptr() + 8, rbuf.data_ptr()))            # not 16-byte aligned
    refused(call(lib.pcr_thin, 0, 1, vox, T.FIRST, buf.data_ptr(), rbuf.data_ptr() + 4))            # not 8-byte aligned
    refused(call(lib.pcr_thin, 0, 1, vox, T.FIRST, None, rbuf.data_ptr() + 4))
    refused(call(lib.pcr_read_thin, 0, 1, vox, T.FIRST, host.ctypes.data + 2, hrows.ctypes.data))
    refused(call(lib.pcr_read_thin, 0, 1, vox, T.FIRST, host.ctypes.data, hrows.ctypes.data + 4))
    still_fine()


def test_lattice_limits(ctx):
    """wide30 spans 2^30 on x: cell 1 without a clip needs more than 2^21 voxels there and is refused, the message names the way
    out; with a clip of a smaller extent the same call succeeds. garbage_tail's artefact spans far less than 2^31
    (tests/test_thin_cpu.py::test_lattice_limits_of_the_streams): thinned without a clip it is simply correct."""
    load(ctx, T.stream("wide30"))
    _, _, bounds = points_of(ctx, "wide30")
    assert T.lattice_refusal(bounds, (0, 0, 0, 1)) == "voxels" and T.lattice_refusal(bounds, (0, 0, 0, 1 << 20)) == "extent"
    vox, cnt = P.as_voxels((0, 0, 0, 1)), C.c_int64(-5)
    for entry in (ctx.lib.pcr_thin, ctx.lib.pcr_read_thin):
        for v in (vox, P.as_voxels((0, 0, 0, 1 << 20))):
            assert entry(ctx.h, 0, -1, C.byref(v), None, T.FIRST, None, None, 0, C.byref(cnt), None) == PCR_E_ARG and cnt.value == 0
            msg = ctx.lib.pcr_last_error(ctx.h) or b""
            assert b"clip" in msg and b"larger cell" in msg
    assert check_thin(ctx, "wide30", (0, 0, 0, 1), None, T.FIRST) is None
    got, rows, st = check_thin(ctx, "wide30", (0, 0, 0, 1), T.WIDE30_LOW, T.FIRST)
    assert 0 < len(rows) < st["points_considered"]                          # exact duplicates collapse
    wide = ((0, 0, 0), ((1 << 21) - 3, 1999, 49))                            # extent 2^21 - 3: the most cell 1 takes
    assert check_thin(ctx, "wide30", (0, 0, 0, 1), wide, T.CENTER) is not None
    assert check_thin(ctx, "wide30", (0, 0, 0, 1), ((0, 0, 0), ((1 << 21) - 2, 1999, 49)), T.CENTER) is not None
    assert check_thin(ctx, "wide30", (0, 0, 0, 1), ((0, 0, 0), ((1 << 21) - 1, 1999, 49)), T.CENTER) is None          # one more: refused
    load(ctx, T.stream("garbage_tail"))
    _, xyz, bounds = points_of(ctx, "garbage_tail")
    assert T.lattice_refusal(bounds, (0, 0, 0, 1)) == T.GARBAGE_TAIL_UNCLIPPED
    unclipped = check_thin(ctx, "garbage_tail", (0, 0, 0, 7001), None, T.FIRST)
    clipped = check_thin(ctx, "garbage_tail", (0, 0, 0, 7001), T.header_clip("garbage_tail"), T.FIRST)
    assert unclipped is not None and len(unclipped[1]) > len(clipped[1]), "the tail artefact adds voxels of its own"


# ---- 7. no side effects ------------------------------------------------------------------------------------------------------------
def test_thinning_leaves_frames_and_statistics_alone(ctx):
    image = T.stream("synth")
    of = oracle.OracleFile(image)
    load(ctx, image)
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    pts = ctx.thin((0, 0, 0, 2048), None, "center")
    assert pts.shape[0] > 0 and ctx.thin_stats["batches_decoded"] == of.num_batches
    pts, rows = ctx.thin((0, 0, 0, 7001), S.BOXES["synth"], "first", rows=True)
    assert pts.shape[0] > 0 and ctx.thin_stats["batches_outside"] >= 1
    assert len(ctx.read_thin((5, 5, 5, 1), None, "first")) > 0
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    ctx.clear(); ctx.render_basic(p); ctx.resolve_basic(p)
    ofb, ost = of.render_basic(p)
    assert ctx.stats() == ost and np.array_equal(ctx.read_framebuffer(full=True), ofb)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_basic(p, ofb))


# ---- 8. size ---------------------------------------------------------------------------------------------------------------------------
def test_twenty_million_points(ctx):
    import torch
    image, _ = scenes.synth_stream(20_000_000)
    f = P.HuffmanFile(image.view())
    assert f.numBatches == 306
    ctx.stream_begin(f.header())
    for b0 in range(0, f.numBatches, 100):
        ctx.upload_batches(b0, [f.blob(b) for b in range(b0, min(b0 + 100, f.numBatches))])
    one_frame(ctx)
    ref = ctx.decode_points()                                                # (tests/test_gpu_decode.py holds it against the oracle)
    n = ref.shape[0]
    row = torch.arange(n, dtype=torch.int64, device=ref.device)
    xyz = ref[:, :3].to(torch.int64)
    for origin, cell in (((0, 0, 0), 1024), ((-12345, 777, -1), 1000)):     # (d2 << 40 stays below 2^63 for these cells: int64 will do)
        d = xyz - torch.tensor(origin, dtype=torch.int64, device=ref.device)
        v = torch.div(d, cell, rounding_mode="floor")
        e = 2 * (d - v * cell) - (cell - 1)
        d2 = (e * e).sum(dim=1)
        v = v - v.amin(dim=0)
        key = v[:, 0] | (v[:, 1] << 21) | (v[:, 2] << 42)
        start = (row % 64 == 0)
        start[1:] |= key[1:] != key[:-1]
        runs = int(start.sum())
        uniq, inv = torch.unique(key, return_inverse=True)
        for mode, val in ((T.FIRST, row), (T.CENTER, (d2 << 40) | row)):
            best = torch.full((uniq.shape[0],), (1 << 63) - 1, dtype=torch.int64, device=ref.device).scatter_reduce(0, inv, val, "amin")
            want_rows = torch.sort(best & ((1 << 40) - 1)).values
            for variant in variants(ctx):
                ctx.set_render_variant(variant)
                got, got_rows = ctx.thin((*origin, cell), None, mode, rows=True)
                stats = dict(ctx.thin_stats)
                ctx.set_render_variant(P.Context.VARIANT_AUTO)
                assert torch.equal(got_rows, want_rows), f"{got_rows.shape[0]} rows kept, {want_rows.shape[0]} expected"
                assert torch.equal(got, ref[want_rows])
                assert stats == dict(batches_outside=0, batches_decoded=306, points_considered=n, runs=runs, points_kept=uniq.shape[0],
                                     table_slots=T.table_slots(runs))
            print(f"cell {cell} mode {mode}: {uniq.shape[0]} of {n} records, {runs} runs, {T.table_slots(runs)} slots")
        assert 0 < uniq.shape[0] < runs < n
    # the host read goes through the 64-batch staging buffers in five pieces
    got, got_rows = ctx.read_thin((*origin, cell), None, T.CENTER, rows=True)
    assert np.array_equal(got_rows, want_rows.cpu().numpy()) and got.tobytes() == ref[want_rows].cpu().numpy().tobytes()
    # The other host reads of the family go through the same loop, with their own columns (k words a row for read_knn): each
    # against its device form, which writes in one emit and not through the loop. The clip is a slab 4 m thick through the whole
    # cloud: on the host-decoded stream 76 000 candidates in 31 batches, in each of the five pieces -- which the stats and
    # the returned rows have to confirm.
    slab = ((500_000, -(1 << 31), -(1 << 31)), (503_999, (1 << 31) - 1, (1 << 31) - 1))
    reads = (("components", "components_stats", 3, dict(vox=(0, 0, 0, 500), min_points=10, connectivity=6, rows=True, labels=True)),
             ("voxel_mean", "voxel_mean_stats", 3, dict(vox=(-12345, 777, -1, 1000), rows=True, counts=True)),
             ("neighbors", "neighbors_stats", 4, dict(radius=1000, min_count=1, rows=True, counts=True, nn2=True)),
             ("local_moments", "moments_stats", 4, dict(radius=1000, min_count=3, rows=True, moments=True, eigen=True)),
             ("knn", "knn_stats", 4, dict(k=3, radius=1000, rows=True, neighbors=True)))
    for name, stats, outputs, kw in reads:
        host = getattr(ctx, "read_" + name)(clip=slab, **kw)
        host_stats = dict(getattr(ctx, stats))
        dev = getattr(ctx, name)(clip=slab, **kw)
        assert dict(getattr(ctx, stats)) == host_stats
        assert 0 < host_stats["points_considered"] <= 300_000, name
        assert len(host) == len(dev) == outputs, name
        for k, (h, d) in enumerate(zip(host, dev)):
            assert h.tobytes() == d.cpu().numpy().tobytes(), f"{name}: output {k}"
        assert len(np.unique(host[1] // (64 * PPB))) >= 3, name
        print(f"{name}: {len(host[1])} rows of {host_stats['points_considered']} candidates")


# ---- 9. the resource and the CLI ----------------------------------------------------------------------------------------------------
def test_resource_thinned_world_coordinates():
    import torch
    r = P.Renderer(160, 90)
    try:
        las = P.HuffmanLasData.create(scenes.synth_stream(600_000)[0])
        las.load_all(r)
        info = las.las_info()
        xyz_all, pts_all = las.points(r, world=True)
        ints = pts_all[:, :3].cpu().numpy().astype(np.int64)
        header = P.box_from_world(info, tuple(info.min), tuple(info.max))
        header = (tuple(header.min), tuple(header.max))
        for cell_size, lo, hi, mode in ((2.0, None, None, "first"), (1.5, None, None, "center"), (7.001, (500.0, 640.0, 0.0), (1000.0, 1000.0, 70.0), "first")):
            vox = P.voxels_from_world(info, cell_size)
            assert vox.cell == round(cell_size * 1000)
            clip = header if lo is None else S.BOXES["synth"]
            rows = torch.from_numpy(T.reference(ints, (*vox.origin, vox.cell), clip, T.FIRST if mode == "first" else T.CENTER)).to(pts_all.device)
            xyz, pts = las.thinned(r, cell_size, lo, hi, mode)
            assert 0 < pts.shape[0] < pts_all.shape[0]
            assert torch.equal(pts, pts_all[rows]) and torch.equal(xyz, xyz_all[rows]) and xyz.dtype == torch.float64
        rows = torch.from_numpy(T.reference(ints, (0, 0, 0, 4096), None, T.FIRST)).to(pts_all.device)
        assert torch.equal(las.thinned(r, 4096, world=False), pts_all[rows])
        with pytest.raises(ValueError):
            las.thinned(r, 0.0015)
    finally:
        r.ctx.close()


def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def test_cli_thin_round_trip(tmp_path):
    build.build_tools()
    image = scenes.synth_stream(600_000)[0]
    (tmp_path / "a.huffman").write_bytes(bytes(image.view()))
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "all.las")
    ax, ay, az, ac, las = P.read_las(str(tmp_path / "all.las"))
    ints = np.stack([ax, ay, az], axis=1).astype(np.int64)
    info = P.HuffmanFile(image.view()).batch_las_info(0)
    header = P.box_from_world(info, tuple(info.min), tuple(info.max))
    header = (tuple(header.min), tuple(header.max))
    lo, hi = (500.0, 640.0, 0.0), (1000.0, 1000.0, 70.0)                    # S.BOXES["synth"] in metres
    for k, (cell, center, boxed) in enumerate(((2.0, False, False), (1.5, True, False), (7.001, False, True), (2.048, True, True))):
        args = ["--thin", repr(cell)] + (["--center"] if center else []) + (["--box", *(repr(v) for v in lo + hi)] if boxed else [])
        res = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / f"t{k}.las", *args)
        vox = P.voxels_from_world(info, cell)
        rows = T.reference(ints, (*vox.origin, vox.cell), S.BOXES["synth"] if boxed else header, T.CENTER if center else T.FIRST)
        bx, by, bz, bc, blas = P.read_las(str(tmp_path / f"t{k}.las"))
        assert 0 < len(rows) < len(ax) and len(bx) == len(rows), res.stdout
        assert np.array_equal(bx, ax[rows]) and np.array_equal(by, ay[rows]) and np.array_equal(bz, az[rows]) and np.array_equal(bc, ac[rows])
        assert tuple(blas.scale) == tuple(las.scale) and tuple(blas.offset) == tuple(las.offset)
        assert f"kept {len(rows)}," in res.stdout and "runs" in res.stdout and "table slots" in res.stdout
    # without --thin the tool does what it did
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "again.las")
    assert open(tmp_path / "again.las", "rb").read() == open(tmp_path / "all.las", "rb").read()
    # no point to thin is an error, not an empty file
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.las"), "--thin", "1", "--box", "5000", "5000", "5000", "6000",
                          "6000", "6000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 1 and "no points" in res.stderr and not (tmp_path / "none.las").exists()
