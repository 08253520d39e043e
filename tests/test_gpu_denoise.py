"""pcr_denoise / pcr_read_denoise: the rows of a range without the isolated ones, or those alone, on the GPU straight from the
compressed stream.

The contract: of the rows pcr_decode_points writes for the range that lie inside the clip (the candidates), a row is isolated iff
the 27 voxels around its own hold at most max_count candidates, itself included; KEEP writes the others, ISOLATED those, byte for
byte and in increasing row order, with their rows. So the reference of every call here is Context.read_points of the same range,
reduced in numpy (tests/denoise_cases.py: int64 floor_divide, np.unique with counts, 27 searchsorted lookups), colours and every
statistic included. Every case runs for a context loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there
through both variants, which have to agree), as tests/test_gpu_thin.py does. tests/test_denoise_cpu.py checks on the CPU that the
preconditioned cases have rows only their neighbours' counts keep and rows only another batch's candidates keep."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import denoise_cases as D
from tests import oracle, scenes
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_gpu_select import LAYOUTS, load, one_frame, through_variants

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
STAT_NAMES = list(N.DenoiseStats().as_dict())
ZERO = dict.fromkeys(STAT_NAMES, 0)


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


_points = {}        # stream -> (read_points of the whole stream, its xyz as int64, the exact batch boxes): computed once, never changed
_analysed = {}      # (stream, first, count, vox, clip) -> (analyse()'s dict, runs)


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, T.xyz_of(pts), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def analysed(name, vox, clip, first=0, count=None):
    """The reference's counts over batches [first, first + count) of the whole stream `name`, and only over those."""
    xyz = _points[name][1]
    count = len(xyz) // PPB - first if count is None else count
    key = (name, first, count, vox, clip)
    if key not in _analysed:
        xyz = xyz[first * PPB:(first + count) * PPB]
        _analysed[key] = (D.analyse(xyz, vox, clip), D.count_runs(xyz, vox, clip))
    return _analysed[key]


def denoise(c, vox, max_count, clip, mode, first=0, count=None):
    """read_denoise of the range with the rows (both variants) and the statistics it reported."""
    def go():
        pts, rows = c.read_denoise(vox, max_count, clip, mode, first, count, rows=True)
        return pts, rows, np.array([c.denoise_stats[k] for k in STAT_NAMES])
    pts, rows, st = through_variants(c, go)
    return pts, rows, dict(zip(STAT_NAMES, (int(v) for v in st)))


def check_denoise(c, name, vox, max_count, clip, mode, first=0, count=None, base=0):
    """read_denoise == the reference over read_points of the same range, byte for byte, rows and statistics included; or, where the
    lattice limits say so, a refusal that names the way out. `base`: the batch of the stream that is batch 0 of the context."""
    pts_all, _, bounds = _points[name]
    f0 = base + first
    last = len(pts_all) // PPB if count is None else f0 + count
    refusal = D.lattice_refusal(bounds[f0:last], vox, clip)
    if refusal:
        with pytest.raises(P.PcrError, match="clip or a larger cell"):
            c.read_denoise(vox, max_count, clip, mode, first, count)
        return None
    an, runs = analysed(name, vox, clip, f0, last - f0)
    rows = D.select(an, max_count, mode)
    got, got_rows, st = denoise(c, vox, max_count, clip, mode, first, count)
    want = pts_all[f0 * PPB:last * PPB][rows]
    what = f"({name} {vox} max_count {max_count} {clip} mode {mode})"
    assert got.dtype == want.dtype and got_rows.dtype == np.int64
    assert len(got) == len(want) == len(got_rows), f"{len(got)} records written, {len(want)} expected {what}"
    assert np.array_equal(got_rows, rows), f"rows differ, first at {np.nonzero(got_rows != rows)[0][:4]} {what}"
    assert got.tobytes() == want.tobytes(), f"records differ {what}"
    dec = D.decoded_batches(bounds[f0:last], clip)
    voxels, voxels_isolated, points_isolated = D.voxel_stats(an, max_count)
    assert st == dict(batches_outside=last - f0 - dec, batches_decoded=dec, points_considered=len(an["rows"]), runs=runs, voxels=voxels,
                      voxels_isolated=voxels_isolated, points_isolated=points_isolated, points_written=len(rows), table_slots=D.table_slots(runs)), what
    return got, got_rows, st


def check_both_modes(c, name, vox, max_count, clip, first=0, count=None, base=0):
    """Both modes against the reference; their row sets are disjoint and their union is the candidates. None: refused."""
    keep = check_denoise(c, name, vox, max_count, clip, D.KEEP, first, count, base)
    iso = check_denoise(c, name, vox, max_count, clip, D.ISOLATED, first, count, base)
    if keep is None or iso is None:
        assert keep is None and iso is None
        return None
    assert len(np.intersect1d(keep[1], iso[1])) == 0
    pts_all = _points[name][0]
    last = len(pts_all) // PPB if count is None else base + first + count
    an, _ = analysed(name, vox, clip, base + first, last - base - first)
    assert np.array_equal(np.union1d(keep[1], iso[1]), an["rows"])
    assert keep[2]["points_isolated"] == iso[2]["points_isolated"] == len(iso[1]) and keep[2]["voxels_isolated"] == iso[2]["voxels_isolated"]
    return keep, iso


def combos_of(name):
    for cell, o in D.COMBOS:
        for clipped in (False, True):
            yield (*D.ORIGINS[o], cell), clipped


# ---- 1. against the numpy reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.STREAMS)
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_denoising_equals_the_reference(ctx, name, frame):
    load(ctx, D.stream(name), frame=frame)
    _, xyz, bounds = points_of(ctx, name)
    clip = D.clip_for(name, xyz)
    done = 0
    for vox, clipped in combos_of(name):
        q = clip if clipped else None
        if D.lattice_refusal(bounds, vox, q):
            assert check_both_modes(ctx, name, vox, 3, q) is None
            continue
        median = D.median_n27(analysed(name, vox, q)[0])
        for max_count in (median, 0, D.HUGE):
            keep, iso = check_both_modes(ctx, name, vox, max_count, q)
            if max_count == 0:
                assert len(iso[1]) == 0 and keep[2]["voxels_isolated"] == 0
            if max_count == D.HUGE:
                assert len(keep[1]) == 0 and iso[2]["voxels_isolated"] == iso[2]["voxels"]
        done += 1
        print(f"{name} vox {vox} clip {q}: median N27 {median}, {keep[2]}")
    assert done >= (5 if name == "wide30" else 10)                          # (wide30 without a clip is refused at every cell)
    if not frame:                                                           # ... and the first frame changes nothing
        before = ctx.read_denoise(vox, median, q, "keep", rows=True)
        one_frame(ctx)
        after = ctx.read_denoise(vox, median, q, "keep", rows=True)
        assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("name,cell,max_count,clip,needs", D.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_preconditioned_cases(ctx, name, cell, max_count, clip, needs):
    """The cases tests/test_denoise_cpu.py proves hard: rows only the neighbours keep, rows only another batch's candidates keep."""
    load(ctx, D.stream(name))
    _, xyz, _ = points_of(ctx, name)
    clip = D.case_clip(name, clip, xyz)
    keep, iso = check_both_modes(ctx, name, (0, 0, 0, cell), max_count, clip)
    assert len(keep[1]) > 0 and len(iso[1]) > 0
    print(f"{name} cell {cell} max_count {max_count}: {keep[2]}")


# ---- 2. sub-ranges --------------------------------------------------------------------------------------------------------------------
def test_sub_range_counts_its_own_batches_only(ctx):
    """first = 1, count = 2: the reference is taken over those two batches' rows, so neighbours in batches 0 and 3 do not count."""
    load(ctx, D.stream("synth"))
    _, xyz, _ = points_of(ctx, "synth")
    vox, max_count = (0, 0, 0, 7001), 262
    keep, iso = check_both_modes(ctx, "synth", vox, max_count, None, 1, 2)
    whole = D.select(analysed("synth", vox, None)[0], max_count, D.ISOLATED)
    inside = whole[(whole >= PPB) & (whole < 3 * PPB)] - PPB
    extra = np.setdiff1d(iso[1], inside)
    assert len(np.setdiff1d(inside, iso[1])) == 0 and len(extra) >= 1, "no row of batches 1..2 has its deciding neighbours in batches 0 or 3"
    assert 0 <= iso[1][0] and iso[1][-1] < 2 * PPB                          # rows count from the range's start
    nb = len(xyz) // PPB
    got, rows, st = denoise(ctx, vox, max_count, None, D.KEEP, nb, None)
    assert len(got) == 0 and st == ZERO


def test_sub_range_of_a_stream_loaded_with_upload_tail(ctx):
    image = D.stream("synth")
    load(ctx, image)
    points_of(ctx, "synth")
    load(ctx, image, first=3, count=5)                                      # batches 3..7 of the file, the follower's head words behind them
    ref = through_variants(ctx, ctx.read_points)
    assert ref.tobytes() == _points["synth"][0][3 * PPB:8 * PPB].tobytes()
    vox, max_count = (-12345, 777, -1, 2048), 23
    keep, iso = check_both_modes(ctx, "synth", vox, max_count, None, 0, 5, base=3)
    assert len(keep[1]) > 0 and len(iso[1]) > 0
    for first, count in ((0, 2), (2, 0), (2, 1), (4, 1)):                   # batch `first` of the context is batch 3 + first of the stream
        check_both_modes(ctx, "synth", vox, max_count, S.BOXES["synth"] if first == 2 else None, first, count, base=3)


# ---- 3. edge cases ------------------------------------------------------------------------------------------------------------------
def test_edge_cases(ctx):
    load(ctx, D.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    nb = len(pts_all) // PPB
    # the empty clip, and a clip that misses everything: no batch decoded, no kernel runs, the context stays usable
    for clip in (S.EMPTY, S.NOTHING):
        for mode in (D.KEEP, D.ISOLATED):
            got, rows, st = check_denoise(ctx, "synth", (0, 0, 0, 1000), 6, clip, mode)
            assert len(got) == 0 and len(rows) == 0 and st == dict(ZERO, batches_outside=nb)
    # count == 0, at either end of the stream
    for first in (0, 3, nb):
        got, rows, st = denoise(ctx, (0, 0, 0, 1000), 6, None, D.KEEP, first, 0)
        assert len(got) == 0 and st == ZERO
    # a clip on a single known point: its duplicates are all there is, so N27 is their number
    for k in (0, len(pts_all) // 2 + 777, len(pts_all) - 1):
        pt = tuple(int(v) for v in xyz[k])
        same = int((xyz == np.array(pt)).all(axis=1).sum())
        for max_count, mode, n in ((same, D.ISOLATED, same), (same, D.KEEP, 0), (same - 1, D.KEEP, same), (same - 1, D.ISOLATED, 0)):
            got, rows, st = check_denoise(ctx, "synth", (0, 0, 0, 64), max_count, (pt, pt), mode)
            assert len(rows) == n and (T.xyz_of(got) == np.array(pt)).all() and st["points_considered"] == same and st["voxels"] == 1
    check_both_modes(ctx, "synth", (0, 0, 0, 1000), 6, None)


def test_lattice_limits(ctx):
    """wide30 spans 2^30 on x: without a clip the call is refused and the message names the way out; with a clip of a smaller extent
    the same call succeeds. The denoising lattice takes two voxels more per axis than pcr_thin's."""
    load(ctx, D.stream("wide30"))
    _, _, bounds = points_of(ctx, "wide30")
    assert D.lattice_refusal(bounds, (0, 0, 0, 1)) == "voxels" and D.lattice_refusal(bounds, (0, 0, 0, 1 << 20)) == "extent"
    cnt = C.c_int64(-5)
    for entry in (ctx.lib.pcr_denoise, ctx.lib.pcr_read_denoise):
        for v in (P.as_voxels((0, 0, 0, 1)), P.as_voxels((0, 0, 0, 1 << 20))):
            assert entry(ctx.h, 0, -1, C.byref(v), None, 5, D.KEEP, None, None, 0, C.byref(cnt), None) == PCR_E_ARG and cnt.value == 0
            msg = ctx.lib.pcr_last_error(ctx.h) or b""
            assert b"clip" in msg and b"larger cell" in msg
    assert check_both_modes(ctx, "wide30", (0, 0, 0, 1), 5, None) is None
    keep, iso = check_both_modes(ctx, "wide30", (0, 0, 0, 1), 5, D.WIDE30_LOW)
    assert len(keep[1]) > 0 and len(iso[1]) > 0
    assert check_both_modes(ctx, "wide30", (0, 0, 0, 1), 5, ((0, 0, 0), ((1 << 21) - 4, 1999, 49))) is not None      # extent / cell + 4 = 2^21
    assert check_both_modes(ctx, "wide30", (0, 0, 0, 1), 5, ((0, 0, 0), ((1 << 21) - 3, 1999, 49))) is None          # one more: refused
    assert T.lattice_refusal(bounds, (0, 0, 0, 1), ((0, 0, 0), ((1 << 21) - 3, 1999, 49))) is None                   # (pcr_thin takes it)


# ---- 4. counting, capacity ----------------------------------------------------------------------------------------------------------
def test_count_then_exact_capacity_then_one_short(ctx):
    import torch
    load(ctx, D.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    vt, clip_t, max_count, mode = (-12345, 777, -1, 2047), S.BOXES["synth"], 23, D.KEEP
    rows = D.select(analysed("synth", vt, clip_t)[0], max_count, mode)
    want, n = pts_all[rows], len(rows)
    assert 1000 < n < int(D.candidates(xyz, clip_t).sum())
    vox, box = P.as_voxels(vt), P.as_box(clip_t)
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.DenoiseStats()

    def dev_call(points, rws, cap, stats=st):
        return lib.pcr_denoise(h, 0, -1, C.byref(vox), C.byref(box), max_count, mode, C.c_void_p(points), C.c_void_p(rws), cap, C.byref(cnt), stats)

    def host_call(points, rws, cap, stats=None):
        return lib.pcr_read_denoise(h, 0, -1, C.byref(vox), C.byref(box), max_count, mode, C.c_void_p(points), C.c_void_p(rws), cap, C.byref(cnt), stats)

    # count only: both destinations NULL, on the device and on the host
    assert dev_call(None, None, 0) == 0 and cnt.value == n == st.points_written
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
        assert (dev.cpu().numpy() == SENT).all() and (drows.cpu().numpy() == SENT).all(), "a refused call wrote into a buffer"
    # the same on the host
    host = np.full((n + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    hrows = np.full(n + 4, SENT, np.int64)
    before, rbefore = host.tobytes(), hrows.tobytes()
    cnt.value = -5
    assert host_call(host.ctypes.data, hrows.ctypes.data, n - 1) == PCR_E_ARG
    assert cnt.value == n and host.tobytes() == before and hrows.tobytes() == rbefore
    assert host_call(None, hrows.ctypes.data, n) == 0
    assert np.array_equal(hrows[:n], rows) and (hrows[n:] == SENT).all() and host.tobytes() == before
    assert host_call(host.ctypes.data, hrows.ctypes.data, n) == 0
    assert host[:n].tobytes() == want.tobytes() and np.array_equal(hrows[:n], rows) and host[n:].tobytes() == before[n * 16:]
    # Context.denoise (device, torch) equals read_denoise: with and without `out` and rows, both modes
    t = ctx.denoise(vt, max_count, clip_t)
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (n, 4) and t.cpu().numpy().tobytes() == want.tobytes()
    assert ctx.denoise_stats["points_written"] == n
    t2, r2 = ctx.denoise(vt, max_count, clip_t, "keep", rows=True)
    assert torch.equal(t2, t) and r2.dtype == torch.int64 and np.array_equal(r2.cpu().numpy(), rows)
    ti, ri = ctx.denoise(vt, max_count, clip_t, "isolated", rows=True)
    hi, hri = ctx.read_denoise(vt, max_count, clip_t, "isolated", rows=True)
    assert ti.cpu().numpy().tobytes() == hi.tobytes() and np.array_equal(ri.cpu().numpy(), hri) and len(hri) + n == ctx.denoise_stats["points_considered"]
    out = torch.empty((n + 3, 4), dtype=torch.int32, device=t.device)
    assert torch.equal(ctx.denoise(vt, max_count, clip_t, out=out), t)
    with pytest.raises(P.PcrError):
        ctx.denoise(vt, max_count, clip_t, out=torch.empty((n - 1, 4), dtype=torch.int32, device=t.device))
    assert ctx.denoise_stats["points_written"] == n
    assert tuple(ctx.denoise(vt, max_count, S.EMPTY).shape) == (0, 4)
    with pytest.raises(ValueError):
        ctx.denoise(vt, max_count, clip_t, "isolate")


# ---- 5. the scratch is shared with pcr_thin; run-to-run equality ------------------------------------------------------------------------
def thin_matches(c, vox, clip, mode):
    xyz = _points["synth"][1]
    pts, rows = through_variants(c, lambda: c.read_thin(vox, clip, mode, rows=True))
    want = T.reference(xyz, vox, clip, mode)
    assert np.array_equal(rows, want) and pts.tobytes() == _points["synth"][0][want].tobytes()
    assert c.thin_stats["runs"] == T.count_runs(xyz, vox, clip) and c.thin_stats["points_kept"] == len(want)


def test_calls_in_a_row_do_not_see_each_other(ctx):
    load(ctx, D.stream("synth"))
    points_of(ctx, "synth")
    a = ((0, 0, 0, 7001), 262, None)                        # a small table ...
    b = ((-12345, 777, -1, 64), 2, None)                    # ... a large one, most slots taken by other keys ...
    c = ((0, 0, 0, 1 << 20), 100000, S.BOXES["synth"])      # ... and a tiny one
    first = check_both_modes(ctx, "synth", *a)
    assert check_both_modes(ctx, "synth", *b)[0][2]["table_slots"] > first[0][2]["table_slots"]
    assert check_both_modes(ctx, "synth", *c)[0][2]["table_slots"] < first[0][2]["table_slots"]
    again = check_both_modes(ctx, "synth", *a)
    for x, y in zip(first, again):
        assert x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1]) and x[2] == y[2]
    for call in (b, b, a, a):
        x, y = ctx.read_denoise(*call, "isolated", rows=True), ctx.read_denoise(*call, "isolated", rows=True)
        assert x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1])
    # pcr_thin after a pcr_denoise and the reverse: the table, the bitmap and the lists are shared
    thin_matches(ctx, (0, 0, 0, 7001), None, T.FIRST)
    check_both_modes(ctx, "synth", *b)
    thin_matches(ctx, (-12345, 777, -1, 64), S.BOXES["synth"], T.CENTER)
    check_both_modes(ctx, "synth", *a)
    thin_matches(ctx, (0, 0, 0, 1 << 20), None, T.FIRST)
    check_both_modes(ctx, "synth", *c)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_are_pcr_e_arg_with_a_message(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    buf = torch.empty((2 * PPB + 1, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    rbuf = torch.empty(2 * PPB + 1, dtype=torch.int64, device=buf.device)
    host, hrows = np.empty(2 * PPB + 1, P.POINT_DTYPE), np.empty(2 * PPB + 1, np.int64)
    vox = P.as_voxels((0, 0, 0, 1000))
    cnt = C.c_int64()
    entries = ((lib.pcr_denoise, buf.data_ptr(), rbuf.data_ptr()), (lib.pcr_read_denoise, host.ctypes.data, hrows.ctypes.data))

    def call(entry, first, count, v, max_count, mode, points, rows, out=cnt, cap=2 * PPB, clip=None):
        return entry(h, first, count, None if v is None else C.byref(v), None if clip is None else C.byref(clip), max_count, mode, C.c_void_p(points),
                     C.c_void_p(rows), cap, None if out is None else C.byref(out), None)

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    def still_fine():
        check_denoise(ctx, "synth", (0, 0, 0, 7001), 262, None, D.KEEP, 0, 2)

    for entry, dp, dr in entries:                                           # no stream loaded
        refused(call(entry, 0, 1, vox, 6, D.KEEP, dp, dr))
    load(ctx, D.stream("synth"))
    points_of(ctx, "synth")
    nb = ctx.batches_loaded
    for entry, dp, dr in entries:
        for first, count in ((nb - 1, 2), (-1, 1), (nb + 1, -1)):           # a range outside the resident batches
            refused(call(entry, first, count, vox, 6, D.KEEP, dp, dr))
        refused(call(entry, 0, 1, None, 6, D.KEEP, dp, dr))                 # a NULL lattice
        refused(call(entry, 0, 1, vox, 6, D.KEEP, dp, dr, out=None))        # a NULL out_count
        still_fine()
        for cell in (0, -1, T.MAX_CELL + 1):
            refused(call(entry, 0, 1, P.as_voxels((0, 0, 0, cell)), 6, D.KEEP, dp, dr))
        for max_count in (-1, -(1 << 62)):
            refused(call(entry, 0, 1, vox, max_count, D.KEEP, dp, dr))
        for mode in (7, -1, 2):
            refused(call(entry, 0, 1, vox, 6, mode, dp, dr))
        assert call(entry, 0, 1, vox, 0, D.ISOLATED, dp, dr) == 0 and cnt.value == 0
        assert call(entry, 0, 1, vox, (1 << 63) - 1, D.KEEP, dp, dr) == 0 and cnt.value == 0
        still_fine()
        refused(call(entry, 0, 2, vox, 0, D.KEEP, dp, dr, cap=1000))        # capacity below the result
        assert cnt.value == 2 * PPB
        assert call(entry, 0, 0, vox, 6, D.KEEP, None, None, cap=0) == 0 and cnt.value == 0         # 0 batches: succeeds
    refused(call(lib.pcr_denoise, 0, 1, vox, 6, D.KEEP, buf.data_ptr() + 8, rbuf.data_ptr()))       # not 16-byte aligned
    refused(call(lib.pcr_denoise, 0, 1, vox, 6, D.KEEP, buf.data_ptr(), rbuf.data_ptr() + 4))       # not 8-byte aligned
    refused(call(lib.pcr_read_denoise, 0, 1, vox, 6, D.KEEP, host.ctypes.data + 2, hrows.ctypes.data))
    refused(call(lib.pcr_read_denoise, 0, 1, vox, 6, D.KEEP, host.ctypes.data, hrows.ctypes.data + 4))
    still_fine()


# ---- 7. no side effects ------------------------------------------------------------------------------------------------------------
def test_denoising_leaves_frames_and_statistics_alone(ctx):
    image = D.stream("synth")
    of = oracle.OracleFile(image)
    load(ctx, image)
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    assert ctx.denoise((0, 0, 0, 2048), 23).shape[0] > 0 and ctx.denoise_stats["batches_decoded"] == of.num_batches
    pts, rows = ctx.denoise((0, 0, 0, 7001), 262, S.BOXES["synth"], "isolated", rows=True)
    assert pts.shape[0] > 0 and ctx.denoise_stats["batches_outside"] >= 1
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    ctx.clear(); ctx.render_basic(p); ctx.resolve_basic(p)
    ofb, ost = of.render_basic(p)
    assert ctx.stats() == ost and np.array_equal(ctx.read_framebuffer(full=True), ofb)


# ---- 8. the resource and the CLI ----------------------------------------------------------------------------------------------------
def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def test_resource_and_cli_round_trip(tmp_path):
    """HuffmanLasData.denoised and pcr_decode --denoise give the reference over the decoded LAS, in world units."""
    import torch
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
    r = P.Renderer(160, 90)
    try:
        res = P.HuffmanLasData.create(image)
        res.load_all(r)
        xyz_all, pts_all = res.points(r, world=True)
        for k, (cell, max_count, isolated, boxed) in enumerate(((2.048, 23, False, False), (7.001, 262, True, False), (1.0, 6, False, True),
                                                                (2.0, 20, True, True))):
            vox = P.voxels_from_world(info, cell)
            rows = D.reference(ints, (*vox.origin, vox.cell), max_count, S.BOXES["synth"] if boxed else header, D.ISOLATED if isolated else D.KEEP)
            assert 0 < len(rows) < len(ax)
            args = ["--denoise", repr(cell), str(max_count)] + (["--isolated"] if isolated else []) + (["--box", *(repr(v) for v in lo + hi)] if boxed else [])
            out = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / f"d{k}.las", *args)
            bx, by, bz, bc, blas = P.read_las(str(tmp_path / f"d{k}.las"))
            assert len(bx) == len(rows), out.stdout
            assert np.array_equal(bx, ax[rows]) and np.array_equal(by, ay[rows]) and np.array_equal(bz, az[rows]) and np.array_equal(bc, ac[rows])
            assert tuple(blas.scale) == tuple(las.scale) and tuple(blas.offset) == tuple(las.offset)
            assert f"written {len(rows)}," in out.stdout and "isolated voxels" in out.stdout and "table slots" in out.stdout
            t = torch.from_numpy(rows).to(pts_all.device)
            xyz, pts = res.denoised(r, cell, max_count, lo if boxed else None, hi if boxed else None, isolated=isolated)
            assert torch.equal(pts, pts_all[t]) and torch.equal(xyz, xyz_all[t]) and xyz.dtype == torch.float64
        t = torch.from_numpy(D.reference(ints, (0, 0, 0, 4096), 100, None, D.KEEP)).to(pts_all.device)
        assert torch.equal(res.denoised(r, 4096, 100, world=False), pts_all[t]) and 0 < len(t) < len(ax)
    finally:
        r.ctx.close()
    # nothing to write is an error, not an empty file
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.las"), "--denoise", "1", "0", "--isolated"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 1 and "no points" in res.stderr and not (tmp_path / "none.las").exists()
