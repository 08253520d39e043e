"""pcr_voxel_mean / pcr_read_voxel_mean: centroid and mean colour per voxel, on the GPU straight from the compressed stream.

The contract: one record per non-empty voxel among the rows pcr_decode_points writes for the range that lie inside the clip, in the
order of pcr_thin FIRST -- the mean position rounded half up inside the voxel, the mean of each colour byte, the voxel's least row
and its count, exact and byte for byte. So the reference of every call here is Context.read_points of the same range, reduced in
numpy (tests/voxel_mean_cases.py: int64 sums by np.add.reduceat, integer rounding). Every case runs for a context loaded with
PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there through both variants, which have to agree), and every
comparison is tobytes() equality. tests/test_voxel_mean_cpu.py checks on the CPU that the streams and lattices used here have voxels
over batches and chains, re-entered voxels, half-way ties in position and colour and means that are no member's value. The limit of
2^32 rows a call cannot be reached by a loaded stream: its check is a comparison read in review, its arithmetic is held in
tests/test_voxel_mean_cpu.py."""
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
from tests import voxel_mean_cases as V
from tests.test_gpu_select import LAYOUTS, load, one_frame, through_variants

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
STAT_NAMES = list(N.ThinStats().as_dict())
O = T.ORIGINS


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


_points = {}        # stream -> (read_points of the whole stream, its xyz as int64, the exact batch boxes): computed once, never changed
_wanted = {}        # (stream, first, count, vox, clip) -> (records, rows, counts, runs, candidates)


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, T.xyz_of(pts), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def wanted(name, vox, clip, first=0, count=None):
    key = (name, first, count, vox, clip)
    if key not in _wanted:
        pts, xyz, _ = _points[name]
        last = len(pts) if count is None else (first + count) * PPB
        pts, xyz = pts[first * PPB:last], xyz[first * PPB:last]
        recs, rows, counts = V.reference(pts, vox, clip)
        for a in (recs, rows, counts):
            a.setflags(write=False)
        _wanted[key] = (recs, rows, counts, T.count_runs(xyz, vox, clip), int(T.candidates(xyz, clip).sum()))
    return _wanted[key]


def mean(c, vox, clip, first=0, count=None):
    """read_voxel_mean of the range with rows and counts (both variants) and the statistics it reported."""
    def go():
        pts, rows, counts = c.read_voxel_mean(vox, clip, first, count, rows=True, counts=True)
        return pts, rows, counts, np.array([c.voxel_mean_stats[k] for k in STAT_NAMES])
    pts, rows, counts, st = through_variants(c, go)
    return pts, rows, counts, dict(zip(STAT_NAMES, (int(v) for v in st)))


def check_mean(c, name, vox, clip, first=0, count=None):
    """read_voxel_mean == the reference over read_points of the same range, byte for byte: records, rows, counts and statistics."""
    pts_all, _, bounds = _points[name]
    last = len(pts_all) // PPB if count is None else first + count
    assert T.lattice_refusal(bounds[first:last], vox, clip) is None
    want, rows, counts, runs, cand = wanted(name, vox, clip, first, count)
    got, got_rows, got_counts, st = mean(c, vox, clip, first, count)
    where = f"({name} {vox} {clip} [{first}, {last}))"
    assert got.dtype == want.dtype and got_rows.dtype == np.int64 and got_counts.dtype == np.int64
    assert len(got) == len(want) == len(got_rows) == len(got_counts), f"{len(got)} records, {len(want)} expected {where}"
    assert got_rows.tobytes() == rows.tobytes(), f"rows differ, first at {np.nonzero(got_rows != rows)[0][:4]} {where}"
    assert got_counts.tobytes() == counts.tobytes(), f"counts differ, first at {np.nonzero(got_counts != counts)[0][:4]} {where}"
    assert got.tobytes() == want.tobytes(), f"records differ, first at {np.nonzero(got != want)[0][:4]} {where}"
    dec = T.decoded_batches(bounds[first:last], clip)
    assert st == dict(batches_outside=last - first - dec, batches_decoded=dec, points_considered=cand, runs=runs, points_kept=len(rows),
                      table_slots=T.table_slots(runs)), where
    return got, got_rows, got_counts, st


# ---- 1. against the numpy reference ---------------------------------------------------------------------------------------------
def lattices_of(name, xyz):
    """(lattice, clip) of every call of test 1 on a stream; the three origins of T.ORIGINS each run at least once a stream where the
    stream has three calls"""
    if name == "mean_edges":
        return [(v, None) for v in V.EDGE_LATTICES]
    if name == "wide30":
        return [((*O[0], 1), T.WIDE30_LOW), ((*O[1], 2), T.WIDE30_LOW), ((*O[2], 7), T.WIDE30_LOW), ((*O[0], 2), T.WIDE30_LOW)]
    if name == "plateau":
        return [((*O[0], 64), None), ((*O[2], 1000), None), ((*O[1], 64), None)]
    if name == "clustered":
        mid = T.middle_clip(xyz)
        return [((*O[0], 1000), None), ((*O[1], 7001), None), ((*O[2], 1000), mid), ((*O[0], 7001), mid)]
    if name == "escape_heavy":
        return [((*O[0], 1000), None), ((*O[2], 1000), None)]
    if name == "garbage_tail":
        return [((*O[2], 2048), T.header_clip(name)), ((*O[0], 7001), T.header_clip(name))]
    if name == "synth":
        return [((*O[0], 7001), None), ((*O[1], 1), None), ((*O[2], T.MAX_CELL), None)]
    return [((*O[0], 1000), None), ((*O[1], 1000), None)]                   # the golden files


@pytest.mark.parametrize("name", ["mean_edges", "wide30", "plateau", "clustered", "escape_heavy", "garbage_tail", "synth", "config1", "ref_packed_bc7"])
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_voxel_means_equal_the_reference(ctx, name, frame):
    load(ctx, V.stream(name), frame=frame)
    _, xyz, _ = points_of(ctx, name)
    assert (ctx.stream_color_format() == 7) == (name == "ref_packed_bc7")
    calls = lattices_of(name, xyz)
    for vox, clip in calls:
        got, rows, counts, st = check_mean(ctx, name, vox, clip)
        assert len(got) > 0
        print(f"{name} vox {vox} clip {clip}: {st}, largest n {int(counts.max())}")
        if name == "synth" and vox[3] == 1:                                 # only exact duplicates share a voxel: the padding's, mostly
            assert int(counts.sum()) - len(counts) >= 55361
        if name == "synth" and vox[3] == T.MAX_CELL:
            assert 1 <= len(got) <= 8 and int(counts.max()) > 1 << 16       # tens of thousands of runs into one accumulator
    if not frame:                                                           # ... and the first frame changes nothing
        before = mean(ctx, *calls[0])
        one_frame(ctx)
        after = mean(ctx, *calls[0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:3], after[:3])) and before[3] == after[3]


def test_mean_edges_sites(ctx):
    """The named sites of the constructed batch, as the call returns them (tests/test_voxel_mean_cpu.py has the same from the
    oracle's decode)."""
    load(ctx, V.stream("mean_edges"))
    pts_all, xyz, _ = points_of(ctx, "mean_edges")
    got, rows, counts, _ = check_mean(ctx, "mean_edges", V.EDGE_LATTICES[0], None)
    at = {tuple(int(v) for v in p): i for i, p in enumerate(np.floor_divide(T.xyz_of(got), V.EDGE_CELL))}
    rec = lambda v: tuple(int(got[at[v]][k]) for k in ("x", "y", "z"))
    assert rec(V.HALF) == (2 * V.EDGE_CELL + 1, 7, 9) and counts[at[V.HALF]] == 2
    assert rec(V.TOP) == (5 * V.EDGE_CELL - 1, V.EDGE_CELL - 1, V.EDGE_CELL - 1) and counts[at[V.TOP]] == 5
    assert rec(V.BELOW) == (-7, -7, -7) and counts[at[V.ABOVE]] == 3 and rec(V.MIXED)[0] < 0
    assert counts[at[V.ENDS]] == 4 and rows[at[V.ENDS]] == 320 and counts[at[V.RETURNS]] == 20 and counts[at[V.LEFT]] == 10
    assert counts[at[V.BIG]] == V.BIG_POINTS and rec(V.BIG) == tuple(int(v) for v in V.site(V.BIG, (8, 5, 5)))
    a, b = V.colour_bytes(np.unique(pts_all["color"][V.BIG_FIRST:V.BIG_FIRST + V.BIG_POINTS]))
    assert int(got[at[V.BIG]]["color"]) == sum(int((a[j] + b[j] + 1) // 2) << (8 * j) for j in range(4))


# ---- 2. agreement with pcr_thin FIRST ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vox,clip", [("synth", (0, 0, 0, 7001), None), ("synth", (-12345, 777, -1, 1), S.BOXES["synth"]),
                                           ("wide30", (S.INT32_MAX, S.INT32_MIN, 0, 2), T.WIDE30_LOW)], ids=["synth7001", "synth1", "wide30"])
def test_agreement_with_thinning_first(ctx, name, vox, clip):
    load(ctx, V.stream(name))
    pts_all, xyz, _ = points_of(ctx, name)
    got, rows, counts, st = mean(ctx, vox, clip)
    thin_pts, thin_rows = ctx.read_thin(vox, clip, "first", rows=True)
    assert rows.tobytes() == thin_rows.tobytes() and st == {k: int(v) for k, v in ctx.thin_stats.items()}
    assert int(counts.sum()) == st["points_considered"] and (counts >= 1).all() and len(got) == st["points_kept"]
    key, _ = T.voxel_keys(np.concatenate([T.xyz_of(got), xyz[rows]]), vox)
    assert np.array_equal(key[:len(got)], key[len(got):]), "a mean lies outside its row's voxel"
    if vox[3] == 1:
        assert T.xyz_of(got).tobytes() == T.xyz_of(thin_pts).tobytes()
    else:
        assert T.xyz_of(got).tobytes() != T.xyz_of(thin_pts).tobytes()


# ---- 3. counting, capacity --------------------------------------------------------------------------------------------------------
def test_count_then_exact_capacity_then_one_short(ctx):
    import torch
    load(ctx, V.stream("synth"))
    points_of(ctx, "synth")
    vt, clip_t = (-12345, 777, -1, 2047), S.BOXES["synth"]
    want, rows, counts, _, _ = wanted("synth", vt, clip_t)
    n = len(rows)
    assert n > 1000
    vox, box = P.as_voxels(vt), P.as_box(clip_t)
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.ThinStats()

    def dev_call(points, rws, cts, cap, stats=st):
        return lib.pcr_voxel_mean(h, 0, -1, C.byref(vox), C.byref(box), C.c_void_p(points), C.c_void_p(rws), C.c_void_p(cts), cap, C.byref(cnt), stats)

    def host_call(points, rws, cts, cap, stats=None):
        return lib.pcr_read_voxel_mean(h, 0, -1, C.byref(vox), C.byref(box), C.c_void_p(points), C.c_void_p(rws), C.c_void_p(cts), cap, C.byref(cnt), stats)

    # count only: all three destinations NULL, on the device and on the host
    assert dev_call(None, None, None, 0) == 0 and cnt.value == n == st.points_kept
    cnt.value = -5
    assert host_call(None, None, None, 0) == 0 and cnt.value == n            # stats may be NULL
    SENT = 0x5A5A5A5A
    dev = torch.full((n + 16, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    drows = torch.full((n + 16,), SENT, dtype=torch.int64, device=dev.device)
    dcounts = torch.full((n + 16,), SENT, dtype=torch.int64, device=dev.device)
    subsets = [(p, r, k) for p in (True, False) for r in (True, False) for k in (True, False) if p or r or k]

    def reset():
        dev.fill_(SENT); drows.fill_(SENT); dcounts.fill_(SENT); torch.cuda.synchronize(); cnt.value = -5

    for wp, wr, wc in subsets:                                               # exact capacity, every subset of the destinations
        reset()
        assert dev_call(dev.data_ptr() if wp else None, drows.data_ptr() if wr else None, dcounts.data_ptr() if wc else None, n) == 0 and cnt.value == n
        gp, gr, gc = dev.cpu().numpy(), drows.cpu().numpy(), dcounts.cpu().numpy()
        assert (gp[:n].tobytes() == want.tobytes()) if wp else (gp == SENT).all()
        assert (gr[:n].tobytes() == rows.tobytes()) if wr else (gr == SENT).all()
        assert (gc[:n].tobytes() == counts.tobytes()) if wc else (gc == SENT).all()
        assert (gp[n:] == SENT).all() and (gr[n:] == SENT).all() and (gc[n:] == SENT).all()
    for wp, wr, wc in subsets:                                               # one short: PCR_E_ARG, the count needed, nothing written
        reset()
        assert dev_call(dev.data_ptr() if wp else None, drows.data_ptr() if wr else None, dcounts.data_ptr() if wc else None, n - 1) == PCR_E_ARG
        assert cnt.value == n and (lib.pcr_last_error(h) or b"") != b""
        ctx.synchronize(); torch.cuda.synchronize()
        assert (dev.cpu().numpy() == SENT).all() and (drows.cpu().numpy() == SENT).all() and (dcounts.cpu().numpy() == SENT).all(), "a refused call wrote"
    # the same on the host
    host = np.full((n + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    hrows, hcounts = np.full(n + 4, SENT, np.int64), np.full(n + 4, SENT, np.int64)
    clean = (host.tobytes(), hrows.tobytes(), hcounts.tobytes())
    for wp, wr, wc in subsets:
        cnt.value = -5
        assert host_call(host.ctypes.data if wp else None, hrows.ctypes.data if wr else None, hcounts.ctypes.data if wc else None, n - 1) == PCR_E_ARG
        assert cnt.value == n and (host.tobytes(), hrows.tobytes(), hcounts.tobytes()) == clean
        assert host_call(host.ctypes.data if wp else None, hrows.ctypes.data if wr else None, hcounts.ctypes.data if wc else None, n) == 0 and cnt.value == n
        assert host[:n].tobytes() == want.tobytes() if wp else host.tobytes() == clean[0]
        assert hrows[:n].tobytes() == rows.tobytes() if wr else hrows.tobytes() == clean[1]
        assert hcounts[:n].tobytes() == counts.tobytes() if wc else hcounts.tobytes() == clean[2]
        assert host[n:].tobytes() == clean[0][n * 16:] and (hrows[n:] == SENT).all() and (hcounts[n:] == SENT).all()
        host[:] = np.frombuffer(clean[0], P.POINT_DTYPE); hrows[:] = SENT; hcounts[:] = SENT
    # Context.voxel_mean: the torch tensors, with and without `out`, rows and counts
    t = ctx.voxel_mean(vt, clip_t)
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (n, 4) and t.cpu().numpy().tobytes() == want.tobytes()
    assert ctx.voxel_mean_stats["points_kept"] == n
    t2, r2 = ctx.voxel_mean(vt, clip_t, rows=True)
    assert torch.equal(t2, t) and r2.dtype == torch.int64 and r2.cpu().numpy().tobytes() == rows.tobytes()
    t3, c3 = ctx.voxel_mean(vt, clip_t, counts=True)
    assert torch.equal(t3, t) and c3.dtype == torch.int64 and c3.cpu().numpy().tobytes() == counts.tobytes()
    out = torch.empty((n + 3, 4), dtype=torch.int32, device=t.device)
    t4, r4, c4 = ctx.voxel_mean(vt, clip_t, out=out, rows=True, counts=True)
    assert torch.equal(t4, t) and torch.equal(r4, r2) and torch.equal(c4, c3) and t4.data_ptr() == out.data_ptr()
    with pytest.raises(P.PcrError):
        ctx.voxel_mean(vt, clip_t, out=torch.empty((n - 1, 4), dtype=torch.int32, device=t.device))
    assert ctx.voxel_mean_stats["points_kept"] == n
    assert tuple(ctx.voxel_mean(vt, S.EMPTY).shape) == (0, 4)
    for clip in (S.EMPTY, S.NOTHING):                                       # no batch decoded, no kernel runs
        got, r, k, s = mean(ctx, vt, clip)
        assert len(got) == len(r) == len(k) == 0 and s == dict(batches_outside=10, batches_decoded=0, points_considered=0, runs=0, points_kept=0, table_slots=0)
    got, r, k, s = mean(ctx, vt, None, 3, 0)
    assert len(got) == 0 and s["batches_decoded"] == 0


# ---- 4. sub-ranges --------------------------------------------------------------------------------------------------------------------
def test_sub_ranges_average_their_own_rows(ctx):
    """A voxel that spans the cut appears once per range, with counts that add up to the whole call's count for that voxel."""
    load(ctx, V.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    vox = (0, 0, 0, 7001)
    whole, whole_rows, whole_counts, _ = check_mean(ctx, "synth", vox, None)
    key_of = lambda p: [tuple(v) for v in np.floor_divide(T.xyz_of(p), vox[3])]
    total = dict.fromkeys(key_of(whole), 0)
    records = 0
    for first, count in ((0, 3), (3, 1), (4, 0), (4, 5), (9, None)):
        got, rows, counts, _ = check_mean(ctx, "synth", vox, None, first, count)
        assert len(rows) == 0 or (0 <= rows[0] and rows[-1] < (10 - first if count is None else count) * PPB)      # rows count from the range's start
        for k, n in zip(key_of(got), counts):
            total[k] += int(n)
        records += len(got)
    assert records > len(whole), "no voxel of the lattice spans a cut between the ranges: the case shows nothing"
    assert [total[k] for k in key_of(whole)] == whole_counts.tolist()


# ---- 5. the scratch is cleared and regrown; run-to-run equality; other calls in between ---------------------------------------------------
def test_calls_in_a_row_do_not_see_each_other(ctx):
    load(ctx, V.stream("synth"))
    points_of(ctx, "synth")
    a = ((0, 0, 0, 7001), None)                             # a small table and few accumulators ...
    b = ((-12345, 777, -1, 64), None)                       # ... large ones, most slots taken by other keys ...
    c = ((0, 0, 0, 1 << 20), S.BOXES["synth"])              # ... and tiny ones
    others = {"thin": lambda: ctx.read_thin((5, 5, 5, 1000), None, "center", rows=True),
              "denoise": lambda: ctx.read_denoise((0, 0, 0, 2048), 3, None, "isolated", rows=True),
              "neighbors": lambda: ctx.read_neighbors(300, 2, S.BOXES["synth"], "keep", rows=True, counts=True, nn2=True)}
    alone = {k: f() for k, f in others.items()}
    first = check_mean(ctx, "synth", *a)
    assert check_mean(ctx, "synth", *b)[3]["table_slots"] > first[3]["table_slots"]
    assert check_mean(ctx, "synth", *c)[3]["table_slots"] < first[3]["table_slots"]
    again = check_mean(ctx, "synth", *a)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again[:3], first[:3])) and again[3] == first[3]
    for call, other in ((b, "thin"), (a, "denoise"), (b, "neighbors"), (c, "thin"), (a, "neighbors")):
        x = mean(ctx, *call)
        between = others[other]()
        y = mean(ctx, *call)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x[:3], y[:3])) and x[3] == y[3]
        assert all(p.tobytes() == q.tobytes() for p, q in zip(between, alone[other])), f"{other} after a voxel mean is not what it was"
        check_mean(ctx, "synth", *call)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_are_pcr_e_arg_with_a_message(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    buf = torch.empty((2 * PPB + 1, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    rbuf = torch.empty(2 * PPB + 1, dtype=torch.int64, device=buf.device)
    cbuf = torch.empty(2 * PPB + 1, dtype=torch.int64, device=buf.device)
    host, hrows, hcounts = np.empty(2 * PPB + 1, P.POINT_DTYPE), np.empty(2 * PPB + 1, np.int64), np.empty(2 * PPB + 1, np.int64)
    vox = P.as_voxels((0, 0, 0, 1000))
    cnt = C.c_int64()
    entries = ((lib.pcr_voxel_mean, buf.data_ptr(), rbuf.data_ptr(), cbuf.data_ptr()),
               (lib.pcr_read_voxel_mean, host.ctypes.data, hrows.ctypes.data, hcounts.ctypes.data))

    def call(entry, first, count, v, points, rows, counts, out=cnt, cap=2 * PPB, clip=None):
        return entry(h, first, count, None if v is None else C.byref(v), None if clip is None else C.byref(clip), C.c_void_p(points), C.c_void_p(rows),
                     C.c_void_p(counts), cap, None if out is None else C.byref(out), None)

    def refused(rc, text=None):
        assert rc == PCR_E_ARG
        msg = lib.pcr_last_error(h) or b""
        assert msg != b"" and (text is None or text in msg), msg

    def still_fine():
        check_mean(ctx, "synth", (0, 0, 0, 7001), None, 0, 2)

    for entry, dp, dr, dc in entries:                                       # no stream loaded
        refused(call(entry, 0, 1, vox, dp, dr, dc))
    load(ctx, V.stream("synth"))
    points_of(ctx, "synth")
    nb = ctx.batches_loaded
    for entry, dp, dr, dc in entries:
        for first, count in ((nb - 1, 2), (-1, 1), (nb + 1, -1)):           # a range outside the resident batches
            refused(call(entry, first, count, vox, dp, dr, dc))
        refused(call(entry, 0, 1, None, dp, dr, dc), b"lattice")            # a NULL lattice
        refused(call(entry, 0, 1, vox, dp, dr, dc, out=None), b"out_count") # a NULL out_count
        still_fine()
        for cell in (0, -1, T.MAX_CELL + 1):
            refused(call(entry, 0, 1, P.as_voxels((0, 0, 0, cell)), dp, dr, dc), b"cell")
        assert call(entry, 0, 1, P.as_voxels((0, 0, 0, T.MAX_CELL)), dp, dr, dc) == 0
        assert call(entry, 0, 1, P.as_voxels((0, 0, 0, T.MAX_CENTER_CELL + 1)), dp, dr, dc) == 0        # (no CENTER limit here)
        refused(call(entry, 0, 2, P.as_voxels((0, 0, 0, 1)), dp, dr, dc, cap=1000), b"capacity")         # capacity below the result
        assert cnt.value > 1000
        assert call(entry, 0, 0, vox, None, None, None, cap=0) == 0 and cnt.value == 0                  # 0 batches: succeeds
        still_fine()
    # misaligned pointers, each destination on its own and beside good ones
    refused(call(lib.pcr_voxel_mean, 0, 1, vox, buf.data_ptr() + 8, rbuf.data_ptr(), cbuf.data_ptr()), b"misaligned")     # not 16-byte aligned
    refused(call(lib.pcr_voxel_mean, 0, 1, vox, buf.data_ptr() + 8, None, None), b"points")
    refused(call(lib.pcr_voxel_mean, 0, 1, vox, buf.data_ptr(), rbuf.data_ptr() + 4, cbuf.data_ptr()), b"rows")           # not 8-byte aligned
    refused(call(lib.pcr_voxel_mean, 0, 1, vox, None, rbuf.data_ptr() + 4, None), b"rows")
    refused(call(lib.pcr_voxel_mean, 0, 1, vox, buf.data_ptr(), rbuf.data_ptr(), cbuf.data_ptr() + 4), b"counts")
    refused(call(lib.pcr_voxel_mean, 0, 1, vox, None, None, cbuf.data_ptr() + 4), b"counts")
    refused(call(lib.pcr_read_voxel_mean, 0, 1, vox, host.ctypes.data + 2, hrows.ctypes.data, hcounts.ctypes.data), b"points")
    refused(call(lib.pcr_read_voxel_mean, 0, 1, vox, host.ctypes.data, hrows.ctypes.data + 4, hcounts.ctypes.data), b"rows")
    refused(call(lib.pcr_read_voxel_mean, 0, 1, vox, host.ctypes.data, hrows.ctypes.data, hcounts.ctypes.data + 4), b"counts")
    still_fine()


def test_lattice_limits(ctx):
    """wide30 spans 2^30 on x: without a clip every cell is refused, and the message names the way out."""
    load(ctx, V.stream("wide30"))
    _, _, bounds = points_of(ctx, "wide30")
    assert T.lattice_refusal(bounds, (0, 0, 0, 1)) == "voxels" and T.lattice_refusal(bounds, (0, 0, 0, 1 << 20)) == "extent"
    cnt = C.c_int64(-5)
    for entry in (ctx.lib.pcr_voxel_mean, ctx.lib.pcr_read_voxel_mean):
        for v in (P.as_voxels((0, 0, 0, 1)), P.as_voxels((0, 0, 0, 1 << 20))):
            assert entry(ctx.h, 0, -1, C.byref(v), None, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG and cnt.value == 0
            msg = ctx.lib.pcr_last_error(ctx.h) or b""
            assert b"clip" in msg and b"larger cell" in msg
    with pytest.raises(P.PcrError, match="clip or a larger cell"):
        ctx.read_voxel_mean((0, 0, 0, 1))
    check_mean(ctx, "wide30", (0, 0, 0, 1), ((0, 0, 0), ((1 << 21) - 2, 1999, 49)))                     # the most cell 1 takes
    assert T.lattice_refusal(bounds, (0, 0, 0, 1), ((0, 0, 0), ((1 << 21) - 1, 1999, 49))) == "voxels"
    with pytest.raises(P.PcrError, match="clip or a larger cell"):
        ctx.read_voxel_mean((0, 0, 0, 1), ((0, 0, 0), ((1 << 21) - 1, 1999, 49)))                       # one more: refused
    check_mean(ctx, "wide30", (0, 0, 0, 2), T.WIDE30_LOW)


# ---- 7. no side effects ------------------------------------------------------------------------------------------------------------
def test_voxel_means_leave_frames_and_statistics_alone(ctx):
    image = V.stream("synth")
    of = oracle.OracleFile(image)
    load(ctx, image)
    p = scenes.with_flags(scenes.cameras(160, 90)["overview"], lod_percent=100, cull=1)
    ctx.clear(); ctx.render_hqs_depth(p); ctx.render_hqs_color(p); ctx.resolve_hqs(p)

    def state():
        return ctx.read_framebuffer(full=True), *ctx.read_accum(full=True), ctx.read_rgba(), ctx.stats()

    before = state()
    pts = ctx.voxel_mean((0, 0, 0, 2048), None)
    assert pts.shape[0] > 0 and ctx.voxel_mean_stats["batches_decoded"] == of.num_batches
    pts, rows, counts = ctx.voxel_mean((0, 0, 0, 7001), S.BOXES["synth"], rows=True, counts=True)
    assert pts.shape[0] > 0 and ctx.voxel_mean_stats["batches_outside"] >= 1
    assert len(ctx.read_voxel_mean((5, 5, 5, 1), None)) > 0
    after = state()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    assert before[4] == after[4]
    ctx.clear(); ctx.render_basic(p); ctx.resolve_basic(p)
    ofb, ost = of.render_basic(p)
    assert ctx.stats() == ost and np.array_equal(ctx.read_framebuffer(full=True), ofb)
    assert np.array_equal(ctx.read_rgba(), oracle.resolve_basic(p, ofb))


# ---- 8. the resource and the CLI ----------------------------------------------------------------------------------------------------
def header_box(info):
    b = P.box_from_world(info, tuple(info.min), tuple(info.max))
    return tuple(b.min), tuple(b.max)


def test_resource_voxel_centroids_world_coordinates():
    import torch
    r = P.Renderer(160, 90)
    try:
        las = P.HuffmanLasData.create(scenes.synth_stream(600_000)[0])
        las.load_all(r)
        info = las.las_info()
        pts_all = r.ctx.read_points()
        for cell_size, lo, hi in ((2.0, None, None), (7.001, (500.0, 640.0, 0.0), (1000.0, 1000.0, 70.0))):
            vox = P.voxels_from_world(info, cell_size)
            assert vox.cell == round(cell_size * 1000)
            want, _, counts = V.reference(pts_all, (*vox.origin, vox.cell), header_box(info) if lo is None else S.BOXES["synth"])
            xyz, pts, n = las.voxel_centroids(r, cell_size, lo, hi)
            assert 0 < pts.shape[0] < len(pts_all) and pts.dtype == torch.int32 and n.dtype == torch.int64 and xyz.dtype == torch.float64
            assert pts.cpu().numpy().tobytes() == want.tobytes() and n.cpu().numpy().tobytes() == counts.tobytes()
            world = T.xyz_of(want).astype(np.float64) * np.array(tuple(info.scale)) + np.array(tuple(info.offset))
            assert xyz.cpu().numpy().tobytes() == world.tobytes()
        want, _, counts = V.reference(pts_all, (0, 0, 0, 4096), None)
        pts, n = las.voxel_centroids(r, 4096, world=False)
        assert pts.cpu().numpy().tobytes() == want.tobytes() and n.cpu().numpy().tobytes() == counts.tobytes()
        with pytest.raises(ValueError):
            las.voxel_centroids(r, 0.0015)
    finally:
        r.ctx.close()


def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def test_cli_mean_round_trip(tmp_path):
    build.build_tools()
    image = scenes.synth_stream(600_000)[0]
    (tmp_path / "a.huffman").write_bytes(bytes(image.view()))
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "all.las")
    ax, ay, az, ac, las = P.read_las(str(tmp_path / "all.las"))
    pts_all = np.empty(len(ax), P.POINT_DTYPE)
    pts_all["x"], pts_all["y"], pts_all["z"], pts_all["color"] = ax, ay, az, ac
    info = P.HuffmanFile(image.view()).batch_las_info(0)
    lo, hi = (500.0, 640.0, 0.0), (1000.0, 1000.0, 70.0)                    # S.BOXES["synth"] in metres
    for k, (cell, boxed) in enumerate(((2.0, False), (7.001, True))):
        box = ["--box", *(repr(v) for v in lo + hi)] if boxed else []
        res = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / f"m{k}.las", "--thin", repr(cell), "--mean", *box)
        vox = P.voxels_from_world(info, cell)
        want, rows, _ = V.reference(pts_all, (*vox.origin, vox.cell), S.BOXES["synth"] if boxed else header_box(info))
        bx, by, bz, bc, blas = P.read_las(str(tmp_path / f"m{k}.las"))
        assert 0 < len(want) < len(ax) and len(bx) == len(want), res.stdout
        assert np.array_equal(bx, want["x"]) and np.array_equal(by, want["y"]) and np.array_equal(bz, want["z"]) and np.array_equal(bc, want["color"])
        assert tuple(blas.scale) == tuple(las.scale) and tuple(blas.offset) == tuple(las.offset)
        assert res.stdout.startswith("thin: cell of") and f"kept {len(want)}," in res.stdout and "runs" in res.stdout and "table slots" in res.stdout
        # without --mean the tool writes what pcr_thin FIRST keeps, and prints the same line
        plain = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / f"t{k}.las", "--thin", repr(cell), *box)
        tx, ty, tz, tc, _ = P.read_las(str(tmp_path / f"t{k}.las"))
        assert np.array_equal(tx, ax[rows]) and np.array_equal(ty, ay[rows]) and np.array_equal(tz, az[rows]) and np.array_equal(tc, ac[rows])
        assert plain.stdout.splitlines()[0] == res.stdout.splitlines()[0]
    run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / "again.las")
    assert open(tmp_path / "again.las", "rb").read() == open(tmp_path / "all.las", "rb").read()
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.las"), "--thin", "1", "--mean", "--box", "5000", "5000", "5000",
                          "6000", "6000", "6000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 1 and "no points" in res.stderr and not (tmp_path / "none.las").exists()
