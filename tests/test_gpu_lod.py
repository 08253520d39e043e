"""pcr_lod_order / pcr_read_lod_order on the GPU against the numpy reference of tests/lod_cases.py over Context.read_points(): records,
rows, levels and every statistic, byte for byte, in both orders, with and without the rest, for both resident layouts, before and
after the first frame; against pcr_thin (the parent's code) level by level; the edges, the capacity protocol, the refusals, the
scratch reuse, a host read of more than one piece, the absence of side effects, the resource in world coordinates and the CLI.
tests/test_lod_cpu.py proves on the CPU that the cases are the hard ones."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import lod_cases as D
from tests import oracle, scenes
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_gpu_select import LAYOUTS, load, one_frame, through_variants

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
SCALARS = ["batches_outside", "batches_decoded", "points_considered", "runs", "table_slots", "points_written"]
ALL_FLAGS = (0, D.DROP_REST, D.ROW_ORDER, D.DROP_REST | D.ROW_ORDER)


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


_points = {}        # stream -> (read_points of the whole stream, its xyz as int64, the exact batch boxes): computed once, never changed
_levels = {}        # (stream, first, count, lod, clip) -> (levels() of the range's rows, runs at the finest cell)


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, T.xyz_of(pts), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def span(name, first, count):
    last = len(_points[name][0]) // PPB if count is None else first + count
    return first, last


def wanted(name, lod, clip, first=0, count=None):
    key = (name, first, count, lod, clip)
    if key not in _levels:
        first, last = span(name, first, count)
        xyz = _points[name][1][first * PPB:last * PPB]
        lv = D.levels(xyz, lod, clip)
        lv.setflags(write=False)
        _levels[key] = (lv, D.stats(xyz, _points[name][2][first:last], lod, clip, 0, lv))
    return _levels[key]


def flags_kw(flags):
    return dict(drop_rest=bool(flags & D.DROP_REST), row_order=bool(flags & D.ROW_ORDER))


def stats_list(st):
    return [st[k] for k in SCALARS] + list(st["level_count"])


def lod_read(c, lod, clip, flags, first=0, count=None):
    """read_lod_order of the range with rows and levels (both variants) and the statistics it reported."""
    def go():
        pts, rows, lv = c.read_lod_order(lod, clip, first, count, rows=True, levels=True, **flags_kw(flags))
        return pts, rows, lv, np.array(stats_list(c.lod_stats))
    pts, rows, lv, st = through_variants(c, go)
    return pts, rows, lv, [int(v) for v in st]


def check_lod(c, name, lod, clip, first=0, count=None, flags=ALL_FLAGS):
    """read_lod_order == the reference over read_points of the same range, byte for byte, rows, levels and statistics included, for
    every combination of the flags; or, where the lattice limits say so, a refusal that names the way out."""
    pts_all, _, bounds = _points[name]
    a, b = span(name, first, count)
    if D.lattice_refusal(bounds[a:b], lod, clip):
        with pytest.raises(P.PcrError, match="clip or a larger cell"):
            c.read_lod_order(lod, clip, first, count)
        return None
    lv_all, st = wanted(name, lod, clip, first, count)
    out = None
    for f in flags:
        rows, lv = D.order(lv_all, lod, f)
        got, got_rows, got_lv, got_st = lod_read(c, lod, clip, f, first, count)
        what = f"{name} {lod} {clip} flags {f} range {first}, {count}"
        assert got.dtype == P.POINT_DTYPE and got_rows.dtype == np.int64 and got_lv.dtype == np.uint8
        assert len(got) == len(got_rows) == len(got_lv) == len(rows), f"{len(got)} records written, {len(rows)} expected ({what})"
        assert np.array_equal(got_rows, rows), f"rows differ, first at {np.nonzero(got_rows != rows)[0][:4]} ({what})"
        assert np.array_equal(got_lv, lv), f"levels differ, first at {np.nonzero(got_lv != lv)[0][:4]} ({what})"
        assert got.tobytes() == pts_all[a * PPB:b * PPB][rows].tobytes(), f"records differ ({what})"
        want_st = dict(st, points_written=len(rows))
        assert got_st == stats_list(want_st), what
        out = out or (got, got_rows, got_lv, want_st)
    return out


# ---- 1. against the numpy reference ---------------------------------------------------------------------------------------------
CASES = D.CASES + [(name, (0, 0, 0), D.GOLDEN_LOD[3], D.GOLDEN_LOD[4], "middle", ()) for name in T.GOLDEN]


@pytest.mark.parametrize("name,origin,cell,levels,clip,needs", CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_ordering_equals_the_reference(ctx, name, origin, cell, levels, clip, needs, frame):
    load(ctx, T.stream(name), frame=frame)
    _, xyz, _ = points_of(ctx, name)
    clip = T.middle_clip(xyz) if clip == "middle" else T.case_clip(name, clip, xyz)
    lod = (*origin, cell, levels)
    got, rows, lv, st = check_lod(ctx, name, lod, clip)
    print(f"{name} lod {lod} clip {clip}: {st}")
    assert len(rows) > 0 and st["points_considered"] == len(rows) == sum(st["level_count"])
    if not frame:                                                           # ... and the first frame changes nothing
        one_frame(ctx)
        after = lod_read(ctx, lod, clip, 0)
        assert after[0].tobytes() == got.tobytes() and np.array_equal(after[1], rows) and np.array_equal(after[2], lv)


# ---- 2. against pcr_thin ------------------------------------------------------------------------------------------------------------
def test_levels_are_what_thinning_keeps(ctx):
    load(ctx, T.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    name, origin, cell, L, _, _ = D.CASES[0]
    lod = (*origin, cell, L)
    pts, rows, lv = ctx.read_lod_order(lod, rows=True, levels=True)
    for l in range(L):
        tp, tr = ctx.read_thin(D.vox_of(lod, l), None, "first", rows=True)
        m = lv <= l
        assert np.array_equal(np.sort(rows[m]), tr) and pts[m][np.argsort(rows[m], kind="stable")].tobytes() == tp.tobytes(), f"level {l}"
        assert int(m.sum()) == sum(ctx.lod_stats["level_count"][:l + 1]) == ctx.thin_stats["points_kept"]
    # levels == 1 is pcr_thin FIRST plus a rest
    for clip in (None, S.BOXES["synth"]):
        one = (*origin, 7001, 1)
        tp, tr = ctx.read_thin(D.vox_of(one, 0), clip, "first", rows=True)
        thin_stats = dict(ctx.thin_stats)
        p1, r1, l1 = ctx.read_lod_order(one, clip, drop_rest=True, row_order=True, rows=True, levels=True)
        assert p1.tobytes() == tp.tobytes() and np.array_equal(r1, tr) and (l1 == 0).all() and len(tr) > 0
        st = ctx.lod_stats
        assert (st["runs"], st["table_slots"], st["points_considered"]) == (thin_stats["runs"], thin_stats["table_slots"], thin_stats["points_considered"])
        assert (st["batches_outside"], st["batches_decoded"]) == (thin_stats["batches_outside"], thin_stats["batches_decoded"])
        # without DROP_REST, in row order, the records are those of the clip's box
        p2, r2 = ctx.read_lod_order(one, clip, row_order=True, rows=True)
        box = ctx.read_box(S.FULL if clip is None else clip)
        assert p2.tobytes() == box.tobytes() and np.array_equal(r2, np.nonzero(T.candidates(xyz, clip))[0])
    # runs and table slots of the hierarchy are those of thinning at the finest cell
    ctx.read_thin(D.vox_of(lod, L - 1), None, "first")
    ctx.read_lod_order(lod)
    assert (ctx.lod_stats["runs"], ctx.lod_stats["table_slots"]) == (ctx.thin_stats["runs"], ctx.thin_stats["table_slots"])


# ---- 3. edge cases ------------------------------------------------------------------------------------------------------------------
def per_batch(lv, L):
    return np.stack([np.bincount(lv[b * PPB:(b + 1) * PPB], minlength=256)[:L + 1] for b in range(len(lv) // PPB)])


def test_edge_cases_on_synth(ctx):
    load(ctx, T.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    nb = len(pts_all) // PPB
    # 16 levels, the coarsest cell the largest there is: level 0 holds a handful of records
    deep = (0, 0, 0, T.MAX_CELL >> 15, 16)
    got, rows, lv, st = check_lod(ctx, "synth", deep, None)
    assert 1 <= st["level_count"][0] <= 8 and rows[0] == 0 and lv[0] == 0
    # one level, the largest cell: a handful of records, and batches that contribute only rest
    flat = (0, 0, 0, T.MAX_CELL, 1)
    got, rows, lv, st = check_lod(ctx, "synth", flat, None)
    assert 1 <= st["level_count"][0] <= 8 and st["level_count"][1] == nb * PPB - st["level_count"][0]
    # ... also in a sub-range, whose later batches find every voxel won earlier in the range
    check_lod(ctx, "synth", flat, None, 4, 5)
    per = per_batch(wanted("synth", flat, None, 4, 5)[0], 1)
    assert (per[1:, 0] == 0).any() and (per[1:, 1] == PPB).any(), "no batch of the range contributes only rest: the case shows nothing"
    # a batch in which some level is empty (tests/test_lod_cpu.py: batch_without_a_level)
    case = (*D.CASES[0][1], D.CASES[0][2], D.CASES[0][3])
    check_lod(ctx, "synth", case, None, flags=(0,))
    assert (per_batch(wanted("synth", case, None)[0], case[4]) == 0).any()
    # a clip on a single known point (a padding duplicate may put more than one candidate there: one record of level 0, the others rest)
    for k in (0, len(pts_all) // 2 + 777, len(pts_all) - 1):
        pt = tuple(int(v) for v in xyz[k])
        got, rows, lv, st = check_lod(ctx, "synth", (0, 0, 0, 64, 5), (pt, pt))
        assert st["level_count"][0] == 1 and lv[0] == 0 and rows[0] <= k and (T.xyz_of(got) == np.array(pt)).all()
        assert st["level_count"][5] == st["points_considered"] - 1
    # the empty clip, a clip that misses everything and count == 0: nothing decoded, no kernel runs, the context stays usable
    zero = [0] * 17
    for clip in (S.EMPTY, S.NOTHING):
        got, rows, lv, st = check_lod(ctx, "synth", case, clip)
        assert len(got) == 0 and stats_list(st) == [nb, 0, 0, 0, 0, 0] + zero
    for first in (0, 3, nb):
        for f in ALL_FLAGS:
            got, rows, lv, st = lod_read(ctx, case, None, f, first, 0)
            assert len(got) == len(rows) == len(lv) == 0 and st == [0] * 6 + zero
    check_lod(ctx, "synth", case, S.BOXES["synth"])


def test_one_and_sixteen_levels_at_cell_one(ctx):
    load(ctx, T.stream("wide30"))
    points_of(ctx, "wide30")
    for levels in (1, 16):
        got, rows, lv, st = check_lod(ctx, "wide30", (0, 0, 0, 1, levels), T.WIDE30_LOW)
        assert 0 < st["level_count"][0] and st["level_count"][levels] > 0 and len(rows) == st["points_considered"] >= PPB


def test_sub_ranges_order_their_own_rows(ctx):
    """Ordering [first, first + count) is the reference over that range's rows: a voxel that spans the cut has a first row per range."""
    load(ctx, T.stream("synth"))
    pts_all, _, _ = points_of(ctx, "synth")
    nb = len(pts_all) // PPB
    lod = (0, 0, 0, 7001, 3)
    whole = check_lod(ctx, "synth", lod, None, flags=(D.DROP_REST,))[1]
    total = 0
    for first, count in ((0, 3), (3, 1), (4, 0), (4, 5), (9, None)):
        out = check_lod(ctx, "synth", lod, S.BOXES["synth"] if first == 4 else None, first, count, flags=(0, D.DROP_REST | D.ROW_ORDER))
        rows = out[1]
        assert len(rows) == 0 or (0 <= rows.min() and rows.max() < (nb - first if count is None else count) * PPB)      # rows count from the range's start
        total += len(check_lod(ctx, "synth", lod, None, first, count, flags=(D.DROP_REST,))[1])
    assert total > len(whole), "no voxel of the lattice spans a cut between the ranges: the case shows nothing"
    got, rows, lv, st = lod_read(ctx, lod, None, 0, nb, None)
    assert len(got) == 0 and st[0] == 0


# ---- 4. counting, capacity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, D.DROP_REST | D.ROW_ORDER])
def test_count_then_exact_capacity_then_one_short(ctx, flags):
    import torch
    load(ctx, T.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    lt, clip_t = (-12345, 777, -1, 2047, 3), S.BOXES["synth"]
    rows, lv = D.order(wanted("synth", lt, clip_t)[0], lt, flags)
    want, n = pts_all[rows], len(rows)
    assert n > 1000
    lod, box = P.as_lod(lt), P.as_box(clip_t)
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.LodStats()

    def dev_call(points, rws, lvs, cap, stats=st):
        return lib.pcr_lod_order(h, 0, -1, C.byref(lod), C.byref(box), flags, C.c_void_p(points), C.c_void_p(rws), C.c_void_p(lvs), cap, C.byref(cnt), stats)

    def host_call(points, rws, lvs, cap, stats=None):
        return lib.pcr_read_lod_order(h, 0, -1, C.byref(lod), C.byref(box), flags, C.c_void_p(points), C.c_void_p(rws), C.c_void_p(lvs), cap, C.byref(cnt), stats)

    # count only: all three destinations NULL, on the device and on the host
    assert dev_call(None, None, None, 0) == 0 and cnt.value == n == st.points_written
    cnt.value = -5
    assert host_call(None, None, None, 0) == 0 and cnt.value == n           # stats may be NULL
    SENT = 0x5A5A5A5A
    dev = torch.full((n + 16, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    drows = torch.full((n + 16,), SENT, dtype=torch.int64, device=dev.device)
    dlv = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device=dev.device)

    def reset():
        dev.fill_(SENT); drows.fill_(SENT); dlv.fill_(0x5A); torch.cuda.synchronize(); cnt.value = -5

    subsets = [s for s in itertools.product((True, False), repeat=3) if any(s)]
    for wp, wr, wl in subsets:                                              # exact capacity
        reset()
        assert dev_call(dev.data_ptr() if wp else None, drows.data_ptr() if wr else None, dlv.data_ptr() if wl else None, n) == 0 and cnt.value == n
        gp, gr, gl = dev.cpu().numpy(), drows.cpu().numpy(), dlv.cpu().numpy()
        assert (gp[:n].tobytes() == want.tobytes()) if wp else (gp == SENT).all()
        assert np.array_equal(gr[:n], rows) if wr else (gr == SENT).all()
        assert np.array_equal(gl[:n], lv) if wl else (gl == 0x5A).all()
        assert (gp[n:] == SENT).all() and (gr[n:] == SENT).all() and (gl[n:] == 0x5A).all()
    for wp, wr, wl in subsets:                                              # one short: PCR_E_ARG, the count needed, nothing written
        reset()
        assert dev_call(dev.data_ptr() if wp else None, drows.data_ptr() if wr else None, dlv.data_ptr() if wl else None, n - 1) == PCR_E_ARG
        assert cnt.value == n and (lib.pcr_last_error(h) or b"") != b""
        ctx.synchronize(); torch.cuda.synchronize()
        assert (dev.cpu().numpy() == SENT).all() and (drows.cpu().numpy() == SENT).all() and (dlv.cpu().numpy() == 0x5A).all(), "a refused call wrote into a buffer"
    # the same on the host
    host = np.full((n + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    hrows = np.full(n + 4, SENT, np.int64)
    hlv = np.full(n + 5, 0x5A, np.uint8)[1:]                               # (an odd address: bytes need no alignment)
    before = host.tobytes(), hrows.tobytes(), hlv.tobytes()
    for wp, wr, wl in subsets:
        cnt.value = -5
        args = (host.ctypes.data if wp else None, hrows.ctypes.data if wr else None, hlv.ctypes.data if wl else None)
        assert host_call(*args, n - 1) == PCR_E_ARG and cnt.value == n
        assert (host.tobytes(), hrows.tobytes(), hlv.tobytes()) == before
        assert host_call(*args, n) == 0 and cnt.value == n
        assert host[:n].tobytes() == want.tobytes() if wp else host.tobytes() == before[0]
        assert np.array_equal(hrows[:n], rows) if wr else hrows.tobytes() == before[1]
        assert np.array_equal(hlv[:n], lv) if wl else hlv.tobytes() == before[2]
        assert host[n:].tobytes() == before[0][n * 16:] and (hrows[n:] == SENT).all() and (hlv[n:] == 0x5A).all()
        host[:] = np.frombuffer(before[0], P.POINT_DTYPE); hrows[:] = SENT; hlv[:] = 0x5A
    # Context.lod_order: the torch tensors, with and without `out`, rows and levels
    kw = flags_kw(flags)
    t = ctx.lod_order(lt, clip_t, **kw)
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (n, 4) and t.cpu().numpy().tobytes() == want.tobytes()
    assert ctx.lod_stats["points_written"] == n
    t2, r2, l2 = ctx.lod_order(lt, clip_t, rows=True, levels=True, **kw)
    assert torch.equal(t2, t) and r2.dtype == torch.int64 and l2.dtype == torch.uint8
    assert np.array_equal(r2.cpu().numpy(), rows) and np.array_equal(l2.cpu().numpy(), lv)
    t3, l3 = ctx.lod_order(lt, clip_t, levels=True, **kw)
    assert torch.equal(t3, t) and torch.equal(l3, l2)
    out = torch.empty((n + 3, 4), dtype=torch.int32, device=t.device)
    assert torch.equal(ctx.lod_order(lt, clip_t, out=out, **kw), t)
    with pytest.raises(P.PcrError):
        ctx.lod_order(lt, clip_t, out=torch.empty((n - 1, 4), dtype=torch.int32, device=t.device), **kw)
    assert ctx.lod_stats["points_written"] == n
    assert tuple(ctx.lod_order(lt, S.EMPTY, **kw).shape) == (0, 4)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_are_pcr_e_arg_with_a_message(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    cap = 2 * PPB
    buf = torch.empty((cap + 1, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    rbuf = torch.empty(cap + 1, dtype=torch.int64, device=buf.device)
    lbuf = torch.empty(cap + 16, dtype=torch.uint8, device=buf.device)
    host, hrows, hlv = np.empty(cap + 1, P.POINT_DTYPE), np.empty(cap + 1, np.int64), np.empty(cap + 1, np.uint8)
    lod = P.as_lod((0, 0, 0, 1000, 4))
    cnt = C.c_int64()
    entries = ((lib.pcr_lod_order, buf.data_ptr(), rbuf.data_ptr(), lbuf.data_ptr()), (lib.pcr_read_lod_order, host.ctypes.data, hrows.ctypes.data, hlv.ctypes.data))

    def call(entry, first, count, v, flags, points, rows, lvs, out=cnt, cap=cap, clip=None):
        return entry(h, first, count, None if v is None else C.byref(v), None if clip is None else C.byref(clip), flags, C.c_void_p(points), C.c_void_p(rows),
                     C.c_void_p(lvs), cap, None if out is None else C.byref(out), None)

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    def still_fine():
        check_lod(ctx, "synth", (0, 0, 0, 500, 6), None, 0, 2, flags=(0, D.ROW_ORDER))

    def with_fields(cell=1000, levels=4, reserved=0):
        v = P.as_lod((0, 0, 0, cell, levels))
        v.reserved = reserved
        return v

    for entry, dp, dr, dl in entries:                                       # no stream loaded
        refused(call(entry, 0, 1, lod, 0, dp, dr, dl))
    load(ctx, T.stream("synth"))
    points_of(ctx, "synth")
    nb = ctx.batches_loaded
    for entry, dp, dr, dl in entries:
        for first, count in ((nb - 1, 2), (-1, 1), (nb + 1, -1)):           # a range outside the resident batches
            refused(call(entry, first, count, lod, 0, dp, dr, dl))
        refused(call(entry, 0, 1, None, 0, dp, dr, dl))                     # a NULL lod
        refused(call(entry, 0, 1, lod, 0, dp, dr, dl, out=None))            # a NULL out_count
        still_fine()
        for cell in (0, -1):
            refused(call(entry, 0, 1, with_fields(cell=cell), 0, dp, dr, dl))
        for cell, levels in ((T.MAX_CELL + 1, 1), (T.MAX_CELL, 2), ((T.MAX_CELL >> 15) + 1, 16), (1 << 16, 16)):        # the coarsest cell over the limit
            refused(call(entry, 0, 1, with_fields(cell=cell, levels=levels), 0, dp, dr, dl))
        assert call(entry, 0, 1, with_fields(cell=T.MAX_CELL >> 15, levels=16), 0, dp, dr, dl) == 0
        assert call(entry, 0, 1, with_fields(cell=T.MAX_CELL, levels=1), 0, dp, dr, dl) == 0
        for levels in (0, 17, -1):
            refused(call(entry, 0, 1, with_fields(levels=levels), 0, dp, dr, dl))
        refused(call(entry, 0, 1, with_fields(reserved=1), 0, dp, dr, dl))
        still_fine()
        for flags in (4, 8, 1 << 31, 7):
            refused(call(entry, 0, 1, lod, flags, dp, dr, dl))
        refused(call(entry, 0, 2, with_fields(cell=1, levels=2), 0, dp, dr, dl, cap=1000))         # capacity below the result
        assert cnt.value == 2 * PPB
        assert call(entry, 0, 0, lod, 0, None, None, None, cap=0) == 0 and cnt.value == 0           # 0 batches: succeeds
        still_fine()
    d = lib.pcr_lod_order
    refused(call(d, 0, 1, lod, 0, buf.data_ptr() + 8, rbuf.data_ptr(), lbuf.data_ptr()))            # not 16-byte aligned
    refused(call(d, 0, 1, lod, 0, buf.data_ptr(), rbuf.data_ptr() + 4, lbuf.data_ptr()))            # not 8-byte aligned
    refused(call(d, 0, 1, lod, 0, buf.data_ptr(), rbuf.data_ptr(), lbuf.data_ptr() + 4))
    refused(call(d, 0, 1, lod, 0, None, None, lbuf.data_ptr() + 1))
    r = lib.pcr_read_lod_order
    refused(call(r, 0, 1, lod, 0, host.ctypes.data + 2, hrows.ctypes.data, hlv.ctypes.data))
    refused(call(r, 0, 1, lod, 0, host.ctypes.data, hrows.ctypes.data + 4, hlv.ctypes.data))
    assert call(r, 0, 1, lod, 0, host.ctypes.data, hrows.ctypes.data, hlv.ctypes.data + 1, cap=cap - 1) == 0       # bytes: any address
    still_fine()


def test_lattice_limits(ctx):
    """wide30 spans 2^30 on x. With a clip from x = 0 the call takes an extent of 2^21 - 2^(levels - 1) - 1 at cell 1 and refuses
    one more, for 1, 2 and 16 levels, as lod_cases.lattice_refusal says; the message names the way out."""
    load(ctx, T.stream("wide30"))
    _, _, bounds = points_of(ctx, "wide30")
    cnt = C.c_int64(-5)
    for lod in ((0, 0, 0, 1, 3), (0, 0, 0, 1 << 20, 3)):                     # without a clip: too many voxels, too wide
        assert D.lattice_refusal(bounds, lod) == ("voxels" if lod[3] == 1 else "extent")
        v = P.as_lod(lod)
        for entry in (ctx.lib.pcr_lod_order, ctx.lib.pcr_read_lod_order):
            assert entry(ctx.h, 0, -1, C.byref(v), None, 0, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG and cnt.value == 0
            msg = ctx.lib.pcr_last_error(ctx.h) or b""
            assert b"clip" in msg and b"larger cell" in msg
        assert check_lod(ctx, "wide30", lod, None) is None
    for levels in (1, 2, 16):
        limit = (1 << 21) - (1 << (levels - 1)) - 1
        lod = (0, 0, 0, 1, levels)
        verdicts = [D.lattice_refusal(bounds, lod, ((0, 0, 0), (limit + over, 1999, 49))) for over in (-1, 0, 1)]
        assert verdicts == [None, None, "voxels"]
        for over in (-1, 0, 1):
            out = check_lod(ctx, "wide30", lod, ((0, 0, 0), (limit + over, 1999, 49)), flags=(D.DROP_REST,))
            assert (out is None) == (over == 1)
            assert out is None or 0 < len(out[1]) < out[3]["points_considered"]          # exact duplicates are rest


# ---- 6. the scratch is cleared and regrown; run-to-run equality ----------------------------------------------------------------------
def test_calls_in_a_row_do_not_see_each_other(ctx):
    load(ctx, T.stream("synth"))
    points_of(ctx, "synth")
    large = ((-12345, 777, -1, 64, 12), None)                              # a large hierarchy: twelve tables ...
    small = ((0, 0, 0, 1 << 20, 2), S.BOXES["synth"])                      # ... then two tiny ones over a few batches ...
    first = check_lod(ctx, "synth", *large)
    assert check_lod(ctx, "synth", *small)[3]["table_slots"] < first[3]["table_slots"]
    again = check_lod(ctx, "synth", *large)                                 # ... and the large one again
    assert again[0].tobytes() == first[0].tobytes() and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2]) and again[3] == first[3]
    ctx.read_thin((0, 0, 0, 2047), None, "center")                          # a thinning call in between shares the table and the keep words
    for call in (large, small, large):
        for f in (0, D.ROW_ORDER):
            x = ctx.read_lod_order(*call, rows=True, levels=True, **flags_kw(f))
            y = ctx.read_lod_order(*call, rows=True, levels=True, **flags_kw(f))
            assert x[0].tobytes() == y[0].tobytes() and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
    tp, tr = ctx.read_thin((0, 0, 0, 7001), None, "first", rows=True)        # ... and thinning is what it was
    assert np.array_equal(tr, T.reference(_points["synth"][1], (0, 0, 0, 7001), None, T.FIRST))


# ---- 7. a host read of more than one piece ---------------------------------------------------------------------------------------------
def test_host_read_in_two_pieces_equals_the_device_form(ctx):
    """4 600 000 points are 71 batches: the smallest stream whose host read takes two pieces of the 64-batch staging buffers, so
    every level of the result is put together from two copies."""
    image, _ = scenes.synth_stream(4_600_000)
    f = P.HuffmanFile(image.view())
    assert 64 < f.numBatches <= 72
    ctx.stream_begin(f.header())
    ctx.upload_batches(0, [f.blob(b) for b in range(f.numBatches)])
    lod = (0, 0, 0, 512, 5)
    for flags in (0, D.DROP_REST, D.ROW_ORDER):
        kw = flags_kw(flags)
        dev = ctx.lod_order(lod, rows=True, levels=True, **kw)
        dev_stats = dict(ctx.lod_stats)
        host = ctx.read_lod_order(lod, rows=True, levels=True, **kw)
        assert dict(ctx.lod_stats) == dev_stats and len(host[0]) == dev_stats["points_written"] > 32 * PPB
        for k, (hh, dd) in enumerate(zip(host, dev)):
            assert hh.tobytes() == dd.cpu().numpy().tobytes(), f"flags {flags}: output {k}"
        rows, lv = host[1], host[2]
        counts = dev_stats["level_count"]
        assert np.array_equal(np.bincount(lv, minlength=17)[:5], counts[:5]) and all(c > 0 for c in counts[:6])
        if not flags & D.ROW_ORDER:                                         # increasing (level, row), every level from both pieces
            assert (np.diff(lv.astype(np.int64) * (1 << 40) + rows) > 0).all()
            both = [l for l in range(5 if flags else 6) if len(np.unique(rows[lv == l] // (64 * PPB))) == 2]
            print(f"flags {flags}: level counts {counts[:6]}, levels with rows of both pieces {both}")
            assert 4 in both and len(both) >= 2
        else:
            assert (np.diff(rows) > 0).all()
    # the levels are what thinning keeps, level by level, also at this size
    pts, rows, lv = ctx.read_lod_order(lod, drop_rest=True, rows=True, levels=True)
    for l in (0, 4):
        tr = ctx.read_thin(D.vox_of(lod, l), None, "first", rows=True)[1]
        assert np.array_equal(np.sort(rows[lv <= l]), tr)


# ---- 8. no side effects ------------------------------------------------------------------------------------------------------------
def test_ordering_leaves_frames_and_statistics_alone(ctx):
    image = T.stream("synth")
    of = oracle.OracleFile(image)
    load(ctx, image)
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    pts = ctx.lod_order((0, 0, 0, 500, 6))
    assert pts.shape[0] > 0 and ctx.lod_stats["batches_decoded"] == of.num_batches
    pts, rows, lv = ctx.lod_order((0, 0, 0, 875, 4), S.BOXES["synth"], row_order=True, rows=True, levels=True)
    assert pts.shape[0] > 0 and ctx.lod_stats["batches_outside"] >= 1
    assert len(ctx.read_lod_order((5, 5, 5, 1, 16), None, drop_rest=True)) > 0
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    ctx.clear(); ctx.render_basic(p); ctx.resolve_basic(p)
    ofb, ost = of.render_basic(p)
    assert ctx.stats() == ost and np.array_equal(ctx.read_framebuffer(full=True), ofb)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_basic(p, ofb))


# ---- 9. the resource and the CLI ----------------------------------------------------------------------------------------------------
def test_resource_lod_ordered_world_coordinates():
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
        for cell_size, levels, lo, hi, drop in ((0.5, 6, None, None, False), (0.875, 4, (500.0, 640.0, 0.0), (1000.0, 1000.0, 70.0), True)):
            lod = P.lod_from_world(info, cell_size, levels)
            assert lod.cell == round(cell_size * 1000) and lod.levels == levels
            lod_t = (*lod.origin, lod.cell, lod.levels)
            lv = D.levels(ints, lod_t, header if lo is None else S.BOXES["synth"])
            rows = torch.from_numpy(D.order(lv, lod_t, D.DROP_REST if drop else 0)[0]).to(pts_all.device)
            xyz, pts, counts = las.lod_ordered(r, cell_size, levels, lo, hi, drop_rest=drop)
            assert 0 < pts.shape[0] <= pts_all.shape[0] and counts == D.level_counts(lv, lod_t)[:levels + 1]
            assert torch.equal(pts, pts_all[rows]) and torch.equal(xyz, xyz_all[rows]) and xyz.dtype == torch.float64
            # a prefix that ends at a level boundary is the thinned cloud of that level's cell
            for l in (0, levels - 1):
                thin = las.thinned(r, cell_size * (1 << (levels - 1 - l)), lo, hi, "first")[1]
                head = pts[:sum(counts[:l + 1])]
                key = lambda t: t[torch.argsort(t[:, 0].to(torch.int64) * (1 << 42) + t[:, 1].to(torch.int64) * (1 << 21) + t[:, 2].to(torch.int64), stable=True)]
                assert head.shape == thin.shape and torch.equal(key(head), key(thin))
        lv = D.levels(ints, (0, 0, 0, 4096, 3), None)
        pts, counts = las.lod_ordered(r, 4096, 3, world=False)
        assert torch.equal(pts, pts_all[torch.from_numpy(D.order(lv, (0, 0, 0, 4096, 3))[0]).to(pts_all.device)]) and counts == D.level_counts(lv, (0, 0, 0, 4096, 3))[:4]
        with pytest.raises(ValueError):
            las.lod_ordered(r, 0.0015, 3)
        with pytest.raises(ValueError):
            las.lod_ordered(r, 0.5, 17)
    finally:
        r.ctx.close()


def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def test_cli_lod_round_trip(tmp_path):
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
    for k, (cell, levels, drop, boxed) in enumerate(((0.5, 6, False, False), (0.875, 4, True, True), (2.0, 1, True, False))):
        args = ["--lod", repr(cell), str(levels)] + (["--drop-rest"] if drop else []) + (["--box", *(repr(v) for v in lo + hi)] if boxed else [])
        res = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / f"l{k}.las", *args)
        lod = P.lod_from_world(info, cell, levels)
        lod_t = (*lod.origin, lod.cell, lod.levels)
        clip = S.BOXES["synth"] if boxed else header
        lv = D.levels(ints, lod_t, clip)
        rows, _ = D.order(lv, lod_t, D.DROP_REST if drop else 0)
        counts = D.level_counts(lv, lod_t)
        bx, by, bz, bc, blas = P.read_las(str(tmp_path / f"l{k}.las"))
        assert 0 < len(rows) <= len(ax) and len(bx) == len(rows), res.stdout
        assert np.array_equal(bx, ax[rows]) and np.array_equal(by, ay[rows]) and np.array_equal(bz, az[rows]) and np.array_equal(bc, ac[rows])
        assert tuple(blas.scale) == tuple(las.scale) and tuple(blas.offset) == tuple(las.offset)
        lines = res.stdout.splitlines()
        for l in range(levels):
            assert f"level {l}: {counts[l]}" in lines, res.stdout
        assert any(line.startswith(f"rest: {counts[levels]}") for line in lines)
        assert f"written {len(rows)} / considered {sum(counts)} / runs " in res.stdout and "table slots" in res.stdout
        # the point records cut off at a level boundary are the thinned cloud of that level
        for l in range(levels):
            vox = D.vox_of(lod_t, l)
            thin = T.reference(ints, vox, clip, T.FIRST)
            m = sum(counts[:l + 1])
            assert np.array_equal(np.sort(rows[:m]), thin)
    # without --lod the tool does what it did
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "again.las")
    assert open(tmp_path / "again.las", "rb").read() == open(tmp_path / "all.las", "rb").read()
    # no point to order is an error, not an empty file
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.las"), "--lod", "1", "3", "--box", "5000", "5000", "5000",
                          "6000", "6000", "6000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 1 and "no points" in res.stderr and not (tmp_path / "none.las").exists()
