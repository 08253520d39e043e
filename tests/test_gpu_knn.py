"""pcr_knn / pcr_read_knn: per row of a range inside a clip its k nearest other rows within a radius, in the order (squared distance,
row), on the GPU straight from the compressed stream.

The contract: of the rows pcr_decode_points writes for the range that lie inside the clip (the candidates), the neighbours of p are
the candidates q of another row with d2(p, q) <= r * r in exact integers; knn(p) is the first min(k, N(p) - 1) of them by (d2, row),
one word d2 << 32 | row each, all ones behind them; a candidate is written iff it has at least min_found. So the reference of every
call here is Context.read_points of the same range, reduced in numpy (tests/knn_cases.py), colours and every statistic included, and
every comparison is byte for byte. Every case runs for a context loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and
PCR_LAYOUT_BOTH (there through both variants, which have to agree), as tests/test_gpu_neighbors.py does. tests/test_knn_cpu.py checks
the reference against every pair and the preconditions of the constructed stream on the CPU."""
import ctypes as C

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from tests import knn_cases as KC
from tests import neighbors_cases as NC
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_gpu_select import LAYOUTS, load, one_frame, through_variants

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
STAT_NAMES = list(N.NeighborsStats().as_dict())
ZERO = dict.fromkeys(STAT_NAMES, 0)
STREAMS = ("clustered", "synth", "wide30")


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


_points = {}        # stream -> (read_points of the whole stream, its xyz as int64, the exact batch boxes): computed once, never changed
_analysed = {}      # (stream, k, r, clip, first, count) -> (analyse()'s dict, runs)


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, T.xyz_of(pts), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def analysed(name, k, r, clip, first=0, count=None):
    """The reference over batches [first, first + count) of the whole stream `name`, and only over those."""
    xyz = _points[name][1]
    count = len(xyz) // PPB - first if count is None else count
    key = (name, k, r, clip, first, count)
    if key not in _analysed:
        xyz = xyz[first * PPB:(first + count) * PPB]
        an = KC.analyse(xyz, k, r, clip)
        assert an["pairs"] < 3e7 and an["expanded"] < 3e7, "the reference of this case is slow: choose a smaller radius"
        # (synth without a clip: its 55 409 padding duplicates are one voxel, 3.07e9 tests, as in tests/test_gpu_neighbors.py)
        assert an["pairs_bound"] < 1e9 or (name == "synth" and clip is None and first == 0), "the case is expensive on the GPU"
        for v in an.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _analysed[key] = (an, NC.count_runs(xyz, r, clip))
    return _analysed[key]


def knn(c, k, r, min_found, clip, first=0, count=None):
    """read_knn of the range with rows and neighbours (both variants) and the statistics it reported."""
    def go():
        pts, rows, krows, kd2 = c.read_knn(k, r, min_found, clip, first, count, rows=True)
        return pts, rows, krows, kd2, np.array([c.knn_stats[s] for s in STAT_NAMES])
    pts, rows, krows, kd2, st = through_variants(c, go)
    return pts, rows, krows, kd2, dict(zip(STAT_NAMES, (int(v) for v in st)))


def check(c, name, k, r, min_found, clip, first=0, count=None):
    """read_knn == the reference over read_points of the same range: records, rows and neighbours byte for byte and every statistic;
    or, where the lattice limits say so, a refusal that names the way out. Returns (records, rows, knn_rows, knn_d2, statistics), or
    None for a refusal."""
    pts_all, _, bounds = _points[name]
    last = len(pts_all) // PPB if count is None else first + count
    if NC.lattice_refusal(bounds[first:last], r, clip):
        with pytest.raises(P.PcrError, match="clip or a larger radius"):
            c.read_knn(k, r, min_found, clip, first, count)
        return None
    an, runs = analysed(name, k, r, clip, first, last - first)
    at = KC.select(an, min_found)
    rows = an["rows"][at]
    want_rows, want_d2 = KC.split(an["knn"][at])
    got, got_rows, got_krows, got_kd2, st = knn(c, k, r, min_found, clip, first, count)
    want = pts_all[first * PPB:last * PPB][rows]
    what = f"({name} k {k} r {r} min_found {min_found} {clip} batches {first}..{last})"
    assert got.dtype == want.dtype and got_rows.dtype == got_krows.dtype == got_kd2.dtype == np.int64
    assert len(got) == len(want) == len(got_rows) and got_krows.shape == got_kd2.shape == (len(want), k), f"{len(got)} records written, {len(want)} expected {what}"
    assert got_rows.tobytes() == rows.tobytes(), f"rows differ, first at {np.nonzero(got_rows != rows)[0][:4]} {what}"
    assert got.tobytes() == want.tobytes(), f"records differ {what}"
    bad = np.nonzero((got_kd2 != want_d2).any(axis=1))[0]
    assert got_kd2.tobytes() == want_d2.tobytes(), f"distances differ at {bad[:4]}: {got_kd2[bad[:2]]} for {want_d2[bad[:2]]} {what}"
    bad = np.nonzero((got_krows != want_rows).any(axis=1))[0]
    assert got_krows.tobytes() == want_rows.tobytes(), f"neighbour rows differ at {bad[:4]}: {got_krows[bad[:2]]} for {want_rows[bad[:2]]} {what}"
    dec = NC.decoded_batches(bounds[first:last], clip)
    assert st == KC.stats(an, runs, last - first, dec, min_found), what
    return got, got_rows, got_krows, got_kd2, st


# ---- 1. the constructed stream ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [KC.R_BIG, KC.R_SMALL])
@pytest.mark.parametrize("k", KC.KS)
def test_knn_edges_equal_the_reference(ctx, r, k):
    """The 32-bit wrap, the radius edge (r = 32767); ties at place k, duplicates, tile and bucket edges, the corner (r = 64)."""
    load(ctx, KC.stream())
    _, xyz, _ = points_of(ctx, "knn_edges")
    assert np.array_equal(xyz, KC.points())
    for min_found in (0, 1, k):
        res = check(ctx, "knn_edges", k, r, min_found, None)
        assert (min_found == 0) == (len(res[1]) == PPB) and 0 < len(res[1])
    if r == KC.R_BIG:                               # (a) and (b) by name: who is whose neighbour
        an = analysed("knn_edges", k, r, None)[0]
        a, b = (int(np.nonzero((xyz == p).all(axis=1))[0][0]) for p in KC.edges_plan()["wrap"])
        assert an["found"][a] == an["found"][b] == 0 and res is not None
        got = check(ctx, "knn_edges", k, r, 0, None)
        assert (got[2][a] == -1).all() and (got[2][b] == -1).all(), "the pair 2^32 + 1177 apart became neighbours: d2 wrapped"
        centre, inside, outside = (int(np.nonzero((xyz == p).all(axis=1))[0][0]) for p in KC.edges_plan()["radius_edge"])
        assert got[2][centre][0] == inside and got[3][centre][0] == r * r, "the point at exactly the radius is no neighbour"
        assert outside not in got[2][centre] and (got[2][centre][1:] == -1).all()


# ---- 2. streams: no clip and the stream's clip, sub-ranges --------------------------------------------------------------------------
@pytest.mark.parametrize("name", STREAMS)
@pytest.mark.parametrize("k", [1, 8])
def test_streams_equal_the_reference(ctx, name, k):
    load(ctx, NC.stream(name))
    pts_all, xyz, bounds = points_of(ctx, name)
    r = min(min(NC.RADII[name]), KC.MAX_RADIUS)
    clip = NC.clip_for(name, xyz)
    done = 0
    for q in (None, clip):
        res = check(ctx, name, k, r, 0, q)
        if res is None:
            assert name == "wide30" and q is None   # refused with the advice: the expected result
            continue
        done += 1
        assert len(check(ctx, name, k, r, k, q)[1]) <= len(res[1])
    assert done == (1 if name == "wide30" else 2)
    nb = len(pts_all) // PPB
    assert nb >= 2
    # first > 0: rows count from the range's start, the points of the batches outside the range do not exist
    q, m = (NC.WIDE30_LOW if name == "wide30" else None), min(2, nb - 1)
    sub = check(ctx, name, k, r, 0, q, 1, m)
    assert sub is not None and (len(sub[1]) == 0 or (0 <= sub[1][0] and sub[1][-1] < m * PPB and sub[2].max() < m * PPB))
    if name != "wide30":
        assert len(sub[1]) == m * PPB
    got = knn(ctx, k, r, 0, q, nb, None)
    assert len(got[0]) == 0 and got[4] == ZERO


# ---- 3. invariants against pcr_neighbors and read_points --------------------------------------------------------------------------------
def test_invariants_against_existing_calls(ctx):
    load(ctx, NC.stream("clustered"))
    pts_all, xyz, _ = points_of(ctx, "clustered")
    r = min(NC.RADII["clustered"])
    pts, rows, n, nn2 = ctx.read_neighbors(r, 0, None, "all", rows=True, counts=True, nn2=True)
    one = ctx.read_knn(1, r, 0, None, rows=True)
    assert one[0].tobytes() == pts.tobytes() and one[1].tobytes() == rows.tobytes()
    assert np.array_equal(one[3][:, 0] == -1, nn2 == NC.NONE) and np.array_equal(one[3][:, 0].view(np.uint64), nn2)   # NONE maps to NONE
    for k in (1, 5, 16):
        p, rr, krows, kd2 = ctx.read_knn(k, r, 0, None, rows=True)
        found = (krows >= 0).sum(axis=1)
        assert np.array_equal(found, np.minimum(k, n - 1)), "found != min(k, N - 1)"
        assert ((krows >= 0) == (np.arange(k)[None, :] < found[:, None])).all(), "a gap inside a list"
        have = krows >= 0
        centre = np.broadcast_to(xyz[rr][:, None, :], (len(rr), k, 3))[have]
        d = centre - xyz[krows[have]]
        assert np.array_equal((d * d).sum(axis=1), kd2[have]), "a stored d2 is not the distance to the stored row"
        assert (krows != rr[:, None]).all() and (kd2[have] <= r * r).all()
        words = KC.word(np.where(have, kd2, 0), np.where(have, krows, 0))
        assert (~have[:, 1:] | (words[:, 1:] > words[:, :-1])).all(), "a list is not strictly ascending in (d2, row)"


# ---- 4. call shapes ---------------------------------------------------------------------------------------------------------------
def test_count_single_outputs_capacity_and_torch(ctx):
    import torch
    load(ctx, KC.stream(), frame=False)
    pts_all, xyz, _ = points_of(ctx, "knn_edges")
    k, r, min_found = 8, KC.R_SMALL, 3
    an, runs = analysed("knn_edges", k, r, None)
    at = KC.select(an, min_found)
    rows, words, want = an["rows"][at], an["knn"][at], pts_all[an["rows"][at]]
    n = len(rows)
    assert 1000 < n < PPB
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.NeighborsStats()
    full = KC.stats(an, runs, 1, 1, min_found)

    def dev_call(ptrs, cap, stats=st):
        return lib.pcr_knn(h, 0, -1, k, r, None, min_found, *(C.c_void_p(p) for p in ptrs), cap, C.byref(cnt), stats)

    def host_call(ptrs, cap, stats=None):
        return lib.pcr_read_knn(h, 0, -1, k, r, None, min_found, *(C.c_void_p(p) for p in ptrs), cap, C.byref(cnt), stats)

    assert dev_call((None,) * 3, 0) == 0 and cnt.value == n and st.as_dict() == full          # count only, before any frame
    cnt.value = -5
    assert host_call((None,) * 3, 0) == 0 and cnt.value == n                                # stats may be NULL
    SENT = 0x5A5A5A5A
    dev = torch.full((n + 16, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    drows = torch.full((n + 16,), SENT, dtype=torch.int64, device=dev.device)
    dknn = torch.full((n + 16, k), SENT, dtype=torch.int64, device=dev.device)
    bufs, wants = (dev, drows, dknn), (want, rows, words)

    def reset():
        for t in bufs:
            t.fill_(SENT)
        torch.cuda.synchronize(); cnt.value = -5

    for with_ in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        ptrs = [t.data_ptr() if w else None for t, w in zip(bufs, with_)]
        reset()
        assert dev_call(ptrs, n) == 0 and cnt.value == n and st.as_dict() == full, "a call with other outputs reports other statistics"
        for t, w, ref in zip(bufs, with_, wants):
            g = t.cpu().numpy()
            assert (g[:n].tobytes() == ref.tobytes()) if w else (g == SENT).all()
            assert (g[n:] == SENT).all(), "a sentinel behind the result was overwritten"
        reset()                                                                             # one short: PCR_E_ARG, the count needed, nothing written
        assert dev_call(ptrs, n - 1) == PCR_E_ARG and cnt.value == n and (lib.pcr_last_error(h) or b"") != b""
        ctx.synchronize(); torch.cuda.synchronize()
        assert all((t.cpu().numpy() == SENT).all() for t in bufs), "a refused call wrote into a buffer"
    host = np.full((n + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    hrows, hknn = np.full(n + 4, SENT, np.int64), np.full((n + 4, k), SENT, np.uint64)
    before = host.tobytes(), hrows.tobytes(), hknn.tobytes()
    hptrs = [host.ctypes.data, hrows.ctypes.data, hknn.ctypes.data]
    cnt.value = -5
    assert host_call(hptrs, n - 1) == PCR_E_ARG and cnt.value == n and (host.tobytes(), hrows.tobytes(), hknn.tobytes()) == before
    assert host_call([None, None, hknn.ctypes.data], n) == 0 and hknn[:n].tobytes() == words.tobytes() and (hknn[n:] == SENT).all()
    assert host_call(hptrs, n) == 0
    assert host[:n].tobytes() == want.tobytes() and hrows[:n].tobytes() == rows.tobytes() and hknn[:n].tobytes() == words.tobytes()
    assert host[n:].tobytes() == before[0][n * 16:] and (hrows[n:] == SENT).all() and (hknn[n:] == SENT).all()
    # Context.knn (device, torch) equals read_knn, before and after the first frame
    want_rows, want_d2 = KC.split(words)
    for frame in (False, True):
        if frame:
            one_frame(ctx)
        t, tr, tk, td = ctx.knn(k, r, min_found, None, rows=True)
        assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (n, 4) and tr.dtype == tk.dtype == td.dtype == torch.int64
        assert tuple(tk.shape) == tuple(td.shape) == (n, k) and ctx.knn_stats == full
        hv = ctx.read_knn(k, r, min_found, None, rows=True)
        assert all(a.cpu().numpy().tobytes() == b.tobytes() for a, b in zip((t, tr, tk, td), hv))
        assert hv[0].tobytes() == want.tobytes() and hv[1].tobytes() == rows.tobytes() and hv[2].tobytes() == want_rows.tobytes() and hv[3].tobytes() == want_d2.tobytes()
    only = ctx.knn(k, r, min_found, None, neighbors=False)
    assert torch.equal(only, t) and ctx.knn_stats == full
    out = torch.empty((n + 3, 4), dtype=torch.int32, device=t.device)
    assert torch.equal(ctx.knn(k, r, min_found, None, out=out)[0], t)
    with pytest.raises(P.PcrError):
        ctx.knn(k, r, min_found, None, out=torch.empty((n - 1, 4), dtype=torch.int32, device=t.device))
    assert ctx.knn_stats["points_written"] == n
    assert tuple(ctx.knn(k, r, 0, S.EMPTY, neighbors=False).shape) == (0, 4) and ctx.knn_stats == dict(ZERO, batches_outside=1)


def test_bc7_stream(ctx):
    load(ctx, NC.stream("ref_packed_bc7"))
    _, xyz, _ = points_of(ctx, "ref_packed_bc7")
    r = min(NC.RADII["ref_packed_bc7"])
    for k, min_found in ((4, 0), (16, 2)):
        res = check(ctx, "ref_packed_bc7", k, r, min_found, NC.clip_for("ref_packed_bc7", xyz))
        assert res is not None and len(res[1]) > 0


def test_calls_in_a_row_do_not_see_each_other(ctx):
    """pcr_neighbors and pcr_local_moments share the index and pcr_thin's scratch with pcr_knn: each returns before and after a pcr_knn
    call what it returned alone, and pcr_knn the same from run to run."""
    load(ctx, KC.stream())
    points_of(ctx, "knn_edges")

    def neighbors():
        res = through_variants(ctx, lambda: ctx.read_neighbors(KC.R_SMALL, 3, None, "keep", rows=True, counts=True, nn2=True))
        return [a.tobytes() for a in res], dict(ctx.neighbors_stats)

    def moments():
        res = through_variants(ctx, lambda: ctx.read_local_moments(KC.R_SMALL, 3, None, rows=True, moments=True, eigen=True))
        return [a.tobytes() for a in res], dict(ctx.moments_stats)

    alone = neighbors(), moments()
    assert len(alone[0][0][0]) > 0 and len(alone[1][0][0]) > 0
    first = check(ctx, "knn_edges", 8, KC.R_SMALL, 1, None)
    assert (neighbors(), moments()) == alone
    assert check(ctx, "knn_edges", 16, KC.R_BIG, 0, None) is not None
    assert (moments(), neighbors()) == alone[::-1]
    again = check(ctx, "knn_edges", 8, KC.R_SMALL, 1, None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:4], again[:4])) and first[4] == again[4]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_are_pcr_e_arg_with_a_message(ctx):
    """k, radius and min_found outside their ranges, misaligned destinations, ranges outside the stream, a NULL out_count. (A range of
    more than 2^32 rows needs more than 65 536 resident batches: the check is pcr_neighbors' own line and is not constructed here.)"""
    import torch
    lib, h = ctx.lib, ctx.h
    buf = torch.empty((PPB + 1, 4), dtype=torch.int32, device=f"cuda:{ctx.device}")
    ebuf = [torch.empty(PPB + 1, dtype=torch.int64, device=buf.device), torch.empty((PPB + 1) * 16, dtype=torch.int64, device=buf.device)]
    host, hextra = np.empty(PPB + 1, P.POINT_DTYPE), [np.empty(PPB + 1, np.int64), np.empty((PPB + 1) * 16, np.uint64)]
    cnt = C.c_int64()
    entries = ((lib.pcr_knn, [buf.data_ptr()] + [t.data_ptr() for t in ebuf]), (lib.pcr_read_knn, [host.ctypes.data] + [a.ctypes.data for a in hextra]))

    def call(entry, first, count, k, r, min_found, ptrs, out=cnt, cap=PPB):
        return entry(h, first, count, k, r, None, min_found, *(C.c_void_p(p) for p in ptrs), cap, None if out is None else C.byref(out), None)

    def refused(rc, word=b""):
        assert rc == PCR_E_ARG
        msg = lib.pcr_last_error(h) or b""
        assert msg != b"" and word in msg, msg

    for entry, ptrs in entries:                                             # no stream loaded
        refused(call(entry, 0, 1, 4, 64, 0, ptrs))
    load(ctx, KC.stream())
    points_of(ctx, "knn_edges")
    for entry, ptrs in entries:
        for first, count in ((0, 2), (-1, 1), (2, -1)):                     # a range outside the resident batch
            refused(call(entry, first, count, 4, 64, 0, ptrs))
        refused(call(entry, 0, 1, 4, 64, 0, ptrs, out=None))
        for k in (0, 17, -1):
            refused(call(entry, 0, 1, k, 64, 0, ptrs), b"PCR_KNN_MAX_K")
        for r in (0, 32768, -1, S.INT32_MAX):
            refused(call(entry, 0, 1, 4, r, 0, ptrs), b"PCR_KNN_MAX_RADIUS")
        for k, min_found in ((4, -1), (4, 5), (16, 17), (1, 2)):
            refused(call(entry, 0, 1, k, 64, min_found, ptrs), b"min_found")
        refused(call(entry, 0, 1, 4, 64, 0, ptrs, cap=1000))                # capacity below the result
        assert cnt.value == PPB
        assert call(entry, 0, 0, 4, 64, 0, (None,) * 3, cap=0) == 0 and cnt.value == 0      # 0 batches: succeeds
        assert call(entry, 0, 1, 16, 32767, 16, (None,) * 3, cap=0) == 0                    # the limits themselves are accepted
    for i, off in ((0, 8), (1, 4), (2, 4)):                                 # records not 16-byte aligned, the others not 8-byte aligned
        ptrs = list(entries[0][1])
        ptrs[i] += off
        refused(call(lib.pcr_knn, 0, 1, 4, 64, 0, ptrs), b"misaligned")
    for i, off in ((0, 2), (1, 4), (2, 4)):
        ptrs = list(entries[1][1])
        ptrs[i] += off
        refused(call(lib.pcr_read_knn, 0, 1, 4, 64, 0, ptrs), b"misaligned")
    with pytest.raises(P.PcrError):
        ctx.read_knn(17, 64)
    check(ctx, "knn_edges", 3, KC.R_SMALL, 1, None)                         # the context stays usable
