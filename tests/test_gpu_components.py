"""pcr_components / pcr_read_components: the rows of a range without those of the small connected components of its occupied
voxels, or those alone, with the label of every row's component, on the GPU straight from the compressed stream.

The contract: of the rows pcr_decode_points writes for the range that lie inside the clip (the candidates), two occupied voxels are
adjacent if they differ by at most 1 on every axis (26) or by exactly 1 on one axis (6); a component's size is the number of its
candidates, its label the least of their rows; KEEP writes the candidates of the components of at least min_points, SMALL the
others, byte for byte and in increasing row order, with rows and labels. So the reference of every call here is Context.read_points
of the same range, reduced in numpy (tests/components_cases.py), colours and every statistic included. Every case runs for a context
loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there through both variants, which have to agree), as
tests/test_gpu_denoise.py does. tests/test_components_cpu.py checks on the CPU that the preconditioned cases have components that span
batches, components too deep for a fixed number of neighbour rounds, and thousands of components."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import components_cases as K
from tests import denoise_cases as D
from tests import scenes
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_gpu_select import LAYOUTS, load, one_frame, through_variants

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
STAT_NAMES = list(N.ComponentsStats().as_dict())
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
_analysed = {}      # (stream, first, count, vox, clip, connectivity) -> (analyse()'s dict, runs)


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, T.xyz_of(pts), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def analysed(name, vox, clip, conn, first=0, count=None):
    """The reference's components over batches [first, first + count) of the whole stream `name`, and only over those."""
    xyz = _points[name][1]
    count = len(xyz) // PPB - first if count is None else count
    key = (name, first, count, vox, clip, conn)
    if key not in _analysed:
        xyz = xyz[first * PPB:(first + count) * PPB]
        runs = next((v[1] for k, v in _analysed.items() if k[:5] == key[:5]), None)
        an = K.analyse(xyz, vox, clip, conn)
        for a in an.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _analysed[key] = (an, K.count_runs(xyz, vox, clip) if runs is None else runs)
    return _analysed[key]


def components(c, vox, min_points, conn, clip, mode, first=0, count=None):
    """read_components of the range with rows and labels (both variants) and the statistics it reported."""
    def go():
        pts, rows, labels = c.read_components(vox, min_points, conn, clip, mode, first, count, rows=True, labels=True)
        return pts, rows, labels, np.array([c.components_stats[k] for k in STAT_NAMES])
    pts, rows, labels, st = through_variants(c, go)
    return pts, rows, labels, dict(zip(STAT_NAMES, (int(v) for v in st)))


def check(c, name, vox, min_points, conn, clip, mode, first=0, count=None, base=0):
    """read_components == the reference over read_points of the same range, byte for byte, rows, labels and statistics included;
    or, where the lattice limits say so, a refusal that names the way out. `base`: the batch of the stream that is batch 0 of the
    context."""
    pts_all, _, bounds = _points[name]
    f0 = base + first
    last = len(pts_all) // PPB if count is None else f0 + count
    if K.lattice_refusal(bounds[f0:last], vox, clip):
        with pytest.raises(P.PcrError, match="clip or a larger cell"):
            c.read_components(vox, min_points, conn, clip, mode, first, count)
        return None
    an, runs = analysed(name, vox, clip, conn, f0, last - f0)
    rows, labels = K.select(an, min_points, mode)
    got, got_rows, got_labels, st = components(c, vox, min_points, conn, clip, mode, first, count)
    want = pts_all[f0 * PPB:last * PPB][rows]
    what = f"({name} {vox} min_points {min_points} conn {conn} {clip} mode {mode})"
    assert got.dtype == want.dtype and got_rows.dtype == np.int64 and got_labels.dtype == np.int64
    assert len(got) == len(want) == len(got_rows) == len(got_labels), f"{len(got)} records written, {len(want)} expected {what}"
    assert np.array_equal(got_rows, rows), f"rows differ, first at {np.nonzero(got_rows != rows)[0][:4]} {what}"
    assert np.array_equal(got_labels, labels), f"labels differ, first at {np.nonzero(got_labels != labels)[0][:4]} {what}"
    assert got.tobytes() == want.tobytes(), f"records differ {what}"
    dec = K.decoded_batches(bounds[f0:last], clip)
    assert st == dict(batches_outside=last - f0 - dec, batches_decoded=dec, points_considered=len(an["rows"]), runs=runs, **K.stats(an, min_points),
                      points_written=len(rows), table_slots=K.table_slots(runs)), what
    return got, got_rows, got_labels, st


def check_both_modes(c, name, vox, min_points, conn, clip, first=0, count=None, base=0):
    """Both modes against the reference; their row sets are disjoint and their union is the candidates. None: refused."""
    keep = check(c, name, vox, min_points, conn, clip, K.KEEP, first, count, base)
    small = check(c, name, vox, min_points, conn, clip, K.SMALL, first, count, base)
    if keep is None or small is None:
        assert keep is None and small is None
        return None
    assert len(np.intersect1d(keep[1], small[1])) == 0
    last = len(_points[name][0]) // PPB if count is None else base + first + count
    an, _ = analysed(name, vox, clip, conn, base + first, last - base - first)
    assert np.array_equal(np.union1d(keep[1], small[1]), an["rows"])
    assert keep[3]["points_small"] == small[3]["points_small"] == len(small[1]) and keep[3]["components_small"] == small[3]["components_small"]
    return keep, small


def labels_are_first_rows(rows, labels):
    """Every label is the first row of its component in the output, and a component's rows carry one label."""
    uniq, first = np.unique(labels, return_index=True)
    assert np.array_equal(rows[first], uniq) and (labels <= rows).all()


# ---- 1. against the numpy reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.STREAMS)
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_components_equal_the_reference(ctx, name, frame):
    load(ctx, K.stream(name), frame=frame)
    _, xyz, bounds = points_of(ctx, name)
    clip = K.clip_for(name, xyz)
    done = 0
    for cell, o in K.COMBOS:
        vox = (*K.ORIGINS[o], cell)
        for q in (None, clip):
            for conn in (6, 26):
                if K.lattice_refusal(bounds, vox, q):
                    assert check_both_modes(ctx, name, vox, 3, conn, q) is None
                    continue
                median = K.median_size(analysed(name, vox, q, conn)[0])
                for min_points in (median, 1, K.HUGE) if not frame else (median,):      # (the first frame changes nothing: the median will do)
                    keep, small = check_both_modes(ctx, name, vox, min_points, conn, q)
                    if min_points == 1:
                        assert len(small[1]) == 0 and keep[3]["components_small"] == 0
                        labels_are_first_rows(keep[1], keep[2])
                    if min_points == K.HUGE:
                        assert len(keep[1]) == 0 and small[3]["components_small"] == small[3]["components"]
                        labels_are_first_rows(small[1], small[2])
                done += 1
        print(f"{name} vox {vox} clip {q}: median size {median}, {keep[3]}")
    assert done >= (10 if name == "wide30" else 20)                         # (wide30 without a clip is refused at every cell)
    if not frame:                                                           # ... and the first frame changes nothing
        before = ctx.read_components(vox, median, conn, q, "keep", rows=True, labels=True)
        one_frame(ctx)
        after = ctx.read_components(vox, median, conn, q, "keep", rows=True, labels=True)
        assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


# ---- 2. the preconditioned cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(K.CASES)), ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in K.CASES])
def test_preconditioned_cases(ctx, case):
    """The cases tests/test_components_cpu.py proves hard: components over several batches, deep ones, thousands of them."""
    name, cell, conn, clip, min_points, figures, _ = K.CASES[case]
    load(ctx, K.stream(name))
    _, xyz, _ = points_of(ctx, name)
    clip = K.case_clip(name, clip, xyz)
    keep, small = check_both_modes(ctx, name, (0, 0, 0, cell), min_points, conn, clip)
    assert len(keep[1]) > 0 and len(small[1]) > 0
    assert (keep[3]["voxels"], keep[3]["components"], keep[3]["largest_points"]) == (figures[0], figures[1], figures[2][0])
    labels_are_first_rows(keep[1], keep[2])
    print(f"{name} cell {cell} conn {conn} min_points {min_points}: {keep[3]}")


# ---- 3. run to run ----------------------------------------------------------------------------------------------------------------------
_first_run = {}     # what the first context that ran the case wrote: the other layouts have to write the same bytes


def test_the_same_call_twice_and_on_another_layout_gives_the_same_bytes(ctx):
    load(ctx, K.stream("synth"))
    points_of(ctx, "synth")
    for k, (vox, min_points, conn, clip) in enumerate((((0, 0, 0, 1000), 13, 26, None), ((-12345, 777, -1, 64), 2, 6, None))):
        a = ctx.read_components(vox, min_points, conn, clip, "keep", rows=True, labels=True)
        b = ctx.read_components(vox, min_points, conn, clip, "keep", rows=True, labels=True)
        mine = tuple(x.tobytes() for x in a)
        assert len(a[1]) > 0 and mine == tuple(x.tobytes() for x in b)
        assert _first_run.setdefault(k, mine) == mine


# ---- 4. sub-ranges --------------------------------------------------------------------------------------------------------------------
def test_sub_range_labels_its_own_batches_only(ctx):
    """first = 1, count = 2: the reference is taken over those two batches' rows, so voxels of batches 0 and 3 connect nothing."""
    load(ctx, K.stream("synth"))
    _, xyz, _ = points_of(ctx, "synth")
    vox, min_points, conn = (0, 0, 0, 1000), 13, 26
    keep, small = check_both_modes(ctx, "synth", vox, min_points, conn, None, 1, 2)
    whole = analysed("synth", vox, None, conn)[0]
    inside = (whole["rows"] >= PPB) & (whole["rows"] < 3 * PPB)
    sub = analysed("synth", vox, None, conn, 1, 2)[0]
    assert np.array_equal(whole["rows"][inside] - PPB, sub["rows"])
    differs = (whole["label"][inside] - PPB != sub["label"]) | ((whole["size"][inside] < min_points) != (sub["size"] < min_points))
    assert differs.sum() >= 1, "no row of batches 1..2 is labelled or classed through batches 0 or 3"
    both = np.concatenate([keep[2], small[2]])
    assert 0 <= both.min() and both.max() < 2 * PPB and 0 <= keep[1][0] and keep[1][-1] < 2 * PPB       # rows and labels count from the range's start
    nb = len(xyz) // PPB
    got, rows, labels, st = components(ctx, vox, min_points, conn, None, K.KEEP, nb, None)
    assert len(got) == 0 and len(labels) == 0 and st == ZERO


def test_sub_range_of_a_stream_loaded_with_upload_tail(ctx):
    image = K.stream("synth")
    load(ctx, image)
    points_of(ctx, "synth")
    load(ctx, image, first=3, count=5)                                      # batches 3..7 of the file, the follower's head words behind them
    ref = through_variants(ctx, ctx.read_points)
    assert ref.tobytes() == _points["synth"][0][3 * PPB:8 * PPB].tobytes()
    vox, min_points = (-12345, 777, -1, 2048), 200
    keep, small = check_both_modes(ctx, "synth", vox, min_points, 26, None, 0, 5, base=3)
    assert len(keep[1]) > 0 and len(small[1]) > 0
    for first, count in ((0, 2), (2, 0), (2, 1), (4, 1)):                   # batch `first` of the context is batch 3 + first of the stream
        check_both_modes(ctx, "synth", vox, min_points, 6, S.BOXES["synth"] if first == 2 else None, first, count, base=3)


# ---- 5. edge cases ------------------------------------------------------------------------------------------------------------------
def test_edge_cases(ctx):
    load(ctx, K.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    nb = len(pts_all) // PPB
    # the empty clip, and a clip that misses everything: no batch decoded, no kernel runs, the context stays usable
    for clip in (S.EMPTY, S.NOTHING):
        for mode in (K.KEEP, K.SMALL):
            got, rows, labels, st = check(ctx, "synth", (0, 0, 0, 1000), 6, 26, clip, mode)
            assert len(got) == 0 and len(rows) == 0 and len(labels) == 0 and st == dict(ZERO, batches_outside=nb)
    for first in (0, 3, nb):                                                # count == 0, at either end of the stream
        got, rows, labels, st = components(ctx, (0, 0, 0, 1000), 6, 26, None, K.KEEP, first, 0)
        assert len(got) == 0 and st == ZERO
    # a clip on a single known point: its duplicates are all there is, one component of their number
    for k in (0, len(pts_all) // 2 + 777, len(pts_all) - 1):
        pt = tuple(int(v) for v in xyz[k])
        same = np.nonzero((xyz == np.array(pt)).all(axis=1))[0]
        for min_points, mode, n in ((len(same), K.KEEP, len(same)), (len(same), K.SMALL, 0), (len(same) + 1, K.SMALL, len(same)), (len(same) + 1, K.KEEP, 0)):
            got, rows, labels, st = check(ctx, "synth", (0, 0, 0, 64), min_points, 6, (pt, pt), mode)
            assert len(rows) == n and (T.xyz_of(got) == np.array(pt)).all() and (labels == same[0]).all()
            assert (st["points_considered"], st["voxels"], st["components"], st["largest_points"]) == (len(same), 1, 1, len(same))
    # a single candidate: one component of size 1 (a point no other row shares)
    _, idx, cnt = np.unique(xyz, axis=0, return_index=True, return_counts=True)
    k = int(idx[cnt == 1][0])
    pt = tuple(int(v) for v in xyz[k])
    got, rows, labels, st = check(ctx, "synth", (0, 0, 0, 7), 1, 26, (pt, pt), K.KEEP)
    assert rows.tolist() == [k] and labels.tolist() == [k] and (st["components"], st["largest_points"], st["points_written"]) == (1, 1, 1)
    # the largest cell: a handful of voxels, all adjacent
    keep, small = check_both_modes(ctx, "synth", (S.INT32_MAX, S.INT32_MIN, 0, 1 << 30), 1, 26, None)
    assert keep[3]["components"] == 1 and (keep[2] == 0).all() and len(keep[1]) == len(xyz)
    check_both_modes(ctx, "synth", (0, 0, 0, 1000), 13, 6, None)


def test_lattice_limits(ctx):
    """wide30 spans 2^30 on x: without a clip the call is refused and the message names the way out, as pcr_denoise's does."""
    load(ctx, K.stream("wide30"))
    _, _, bounds = points_of(ctx, "wide30")
    assert K.lattice_refusal(bounds, (0, 0, 0, 1)) == "voxels" and K.lattice_refusal(bounds, (0, 0, 0, 1 << 20)) == "extent"
    cnt = C.c_int64(-5)
    for entry in (ctx.lib.pcr_components, ctx.lib.pcr_read_components):
        for v in (P.as_voxels((0, 0, 0, 1)), P.as_voxels((0, 0, 0, 1 << 20))):
            assert entry(ctx.h, 0, -1, C.byref(v), None, 26, 5, K.KEEP, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG and cnt.value == 0
            msg = ctx.lib.pcr_last_error(ctx.h) or b""
            assert b"clip" in msg and b"larger cell" in msg
    assert check_both_modes(ctx, "wide30", (0, 0, 0, 1), 5, 26, None) is None
    assert check_both_modes(ctx, "wide30", (0, 0, 0, 1), 5, 6, ((0, 0, 0), ((1 << 21) - 4, 1999, 49))) is not None     # extent / cell + 4 = 2^21
    assert check_both_modes(ctx, "wide30", (0, 0, 0, 1), 5, 6, ((0, 0, 0), ((1 << 21) - 3, 1999, 49))) is None         # one more: refused


def test_count_then_exact_capacity_then_one_short(ctx):
    import torch
    load(ctx, K.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    vt, clip_t, min_points, conn, mode = (-12345, 777, -1, 2047), S.BOXES["synth"], 100, 26, K.KEEP
    rows, labels = K.select(analysed("synth", vt, clip_t, conn)[0], min_points, mode)
    want, n = pts_all[rows], len(rows)
    assert 1000 < n < int(K.candidates(xyz, clip_t).sum())
    vox, box = P.as_voxels(vt), P.as_box(clip_t)
    lib, h = ctx.lib, ctx.h
    cnt, st = C.c_int64(-5), N.ComponentsStats()

    def dev_call(points, rws, labs, cap, stats=st):
        return lib.pcr_components(h, 0, -1, C.byref(vox), C.byref(box), conn, min_points, mode, C.c_void_p(points), C.c_void_p(rws), C.c_void_p(labs), cap,
                                  C.byref(cnt), stats)

    def host_call(points, rws, labs, cap, stats=None):
        return lib.pcr_read_components(h, 0, -1, C.byref(vox), C.byref(box), conn, min_points, mode, C.c_void_p(points), C.c_void_p(rws), C.c_void_p(labs),
                                       cap, C.byref(cnt), stats)

    # count only: all three destinations NULL, on the device and on the host
    assert dev_call(None, None, None, 0) == 0 and cnt.value == n == st.points_written
    cnt.value = -5
    assert host_call(None, None, None, 0) == 0 and cnt.value == n           # stats may be NULL
    SENT = 0x5A5A5A5A
    dev = torch.full((n + 16, 4), SENT, dtype=torch.int32, device=f"cuda:{ctx.device}")
    drows = torch.full((n + 16,), SENT, dtype=torch.int64, device=dev.device)
    dlabels = torch.full((n + 16,), SENT, dtype=torch.int64, device=dev.device)

    def reset():
        dev.fill_(SENT); drows.fill_(SENT); dlabels.fill_(SENT); torch.cuda.synchronize(); cnt.value = -5

    def ptrs(wp, wr, wl):
        return dev.data_ptr() if wp else None, drows.data_ptr() if wr else None, dlabels.data_ptr() if wl else None

    which = ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, False, True), (True, True, False), (True, True, True))
    for wp, wr, wl in which:                                                # exact capacity: each pointer alone, each one NULL, all three
        reset()
        assert dev_call(*ptrs(wp, wr, wl), n) == 0 and cnt.value == n
        gp, gr, gl = dev.cpu().numpy(), drows.cpu().numpy(), dlabels.cpu().numpy()
        assert (gp[:n].tobytes() == want.tobytes()) if wp else (gp == SENT).all()
        assert np.array_equal(gr[:n], rows) if wr else (gr == SENT).all()
        assert np.array_equal(gl[:n], labels) if wl else (gl == SENT).all()
        assert (gp[n:] == SENT).all() and (gr[n:] == SENT).all() and (gl[n:] == SENT).all()
    for wp, wr, wl in which:                                                # one short: PCR_E_ARG, *out_count = the count needed, nothing written
        reset()
        assert dev_call(*ptrs(wp, wr, wl), n - 1) == PCR_E_ARG
        assert cnt.value == n and (lib.pcr_last_error(h) or b"") != b""
        ctx.synchronize(); torch.cuda.synchronize()
        assert (dev.cpu().numpy() == SENT).all() and (drows.cpu().numpy() == SENT).all() and (dlabels.cpu().numpy() == SENT).all(), "a refused call wrote into a buffer"
    # the same on the host
    host = np.full((n + 4) * 4, SENT, np.uint32).view(P.POINT_DTYPE)
    hrows, hlabels = np.full(n + 4, SENT, np.int64), np.full(n + 4, SENT, np.int64)
    before, rbefore = host.tobytes(), hrows.tobytes()
    cnt.value = -5
    assert host_call(host.ctypes.data, hrows.ctypes.data, hlabels.ctypes.data, n - 1) == PCR_E_ARG
    assert cnt.value == n and host.tobytes() == before and hrows.tobytes() == rbefore and hlabels.tobytes() == rbefore
    assert host_call(None, None, hlabels.ctypes.data, n) == 0
    assert np.array_equal(hlabels[:n], labels) and (hlabels[n:] == SENT).all() and host.tobytes() == before and hrows.tobytes() == rbefore
    assert host_call(host.ctypes.data, hrows.ctypes.data, hlabels.ctypes.data, n) == 0
    assert host[:n].tobytes() == want.tobytes() and np.array_equal(hrows[:n], rows) and np.array_equal(hlabels[:n], labels)
    assert host[n:].tobytes() == before[n * 16:]
    # Context.components (device, torch) equals read_components: with and without `out`, rows and labels, both modes
    t = ctx.components(vt, min_points, conn, clip_t)
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (n, 4) and t.cpu().numpy().tobytes() == want.tobytes()
    assert ctx.components_stats["points_written"] == n
    t2, r2, l2 = ctx.components(vt, min_points, conn, clip_t, "keep", rows=True, labels=True)
    assert torch.equal(t2, t) and r2.dtype == l2.dtype == torch.int64 and np.array_equal(r2.cpu().numpy(), rows) and np.array_equal(l2.cpu().numpy(), labels)
    ts, ls = ctx.components(vt, min_points, conn, clip_t, "small", labels=True)
    hs, hrs, hls = ctx.read_components(vt, min_points, conn, clip_t, "small", rows=True, labels=True)
    assert ts.cpu().numpy().tobytes() == hs.tobytes() and np.array_equal(ls.cpu().numpy(), hls) and len(hrs) + n == ctx.components_stats["points_considered"]
    out = torch.empty((n + 3, 4), dtype=torch.int32, device=t.device)
    assert torch.equal(ctx.components(vt, min_points, conn, clip_t, out=out), t)
    with pytest.raises(P.PcrError):
        ctx.components(vt, min_points, conn, clip_t, out=torch.empty((n - 1, 4), dtype=torch.int32, device=t.device))
    assert ctx.components_stats["points_written"] == n
    assert tuple(ctx.components(vt, min_points, conn, S.EMPTY).shape) == (0, 4)
    with pytest.raises(ValueError):
        ctx.components(vt, min_points, conn, clip_t, "smal")


def test_refusals_are_pcr_e_arg_with_a_message(ctx):
    lib, h = ctx.lib, ctx.h
    host, hrows, hlabels = np.empty(2 * PPB + 1, P.POINT_DTYPE), np.empty(2 * PPB + 1, np.int64), np.empty(2 * PPB + 1, np.int64)
    vox = P.as_voxels((0, 0, 0, 1000))
    cnt = C.c_int64()

    def call(first, count, v, conn, min_points, mode, out=cnt, cap=2 * PPB, points=host.ctypes.data, rows=hrows.ctypes.data, labels=hlabels.ctypes.data):
        return lib.pcr_read_components(h, first, count, None if v is None else C.byref(v), None, conn, min_points, mode, C.c_void_p(points), C.c_void_p(rows),
                                       C.c_void_p(labels), cap, None if out is None else C.byref(out), None)

    def refused(rc):
        assert rc == PCR_E_ARG
        assert (lib.pcr_last_error(h) or b"") != b""

    refused(call(0, 1, vox, 26, 6, K.KEEP))                                 # no stream loaded
    load(ctx, K.stream("synth"))
    points_of(ctx, "synth")
    nb = ctx.batches_loaded
    for first, count in ((nb - 1, 2), (-1, 1), (nb + 1, -1)):               # a range outside the resident batches
        refused(call(first, count, vox, 26, 6, K.KEEP))
    refused(call(0, 1, None, 26, 6, K.KEEP))                                # a NULL lattice
    refused(call(0, 1, vox, 26, 6, K.KEEP, out=None))                       # a NULL out_count
    for cell in (0, -1, T.MAX_CELL + 1):
        refused(call(0, 1, P.as_voxels((0, 0, 0, cell)), 26, 6, K.KEEP))
    for conn in (18, 0, -6, 27):
        refused(call(0, 1, vox, conn, 6, K.KEEP))
    for min_points in (-1, -(1 << 62)):
        refused(call(0, 1, vox, 26, min_points, K.KEEP))
    for mode in (7, -1, 2):
        refused(call(0, 1, vox, 26, 6, mode))
    assert call(0, 1, vox, 26, 0, K.SMALL) == 0 and cnt.value == 0
    assert call(0, 1, vox, 6, (1 << 63) - 1, K.KEEP) == 0 and cnt.value == 0
    refused(call(0, 2, vox, 26, 0, K.KEEP, cap=1000))                       # capacity below the result
    assert cnt.value == 2 * PPB
    assert call(0, 0, vox, 26, 6, K.KEEP, cap=0, points=None, rows=None, labels=None) == 0 and cnt.value == 0      # 0 batches: succeeds
    refused(call(0, 1, vox, 26, 6, K.KEEP, points=host.ctypes.data + 2))
    refused(call(0, 1, vox, 26, 6, K.KEEP, rows=hrows.ctypes.data + 4))
    refused(call(0, 1, vox, 26, 6, K.KEEP, labels=hlabels.ctypes.data + 4))
    check(ctx, "synth", (0, 0, 0, 7001), 26, 26, None, K.KEEP, 0, 2)        # the context stays usable


# ---- 6. neighbours: the table scratch is shared with pcr_thin and pcr_denoise ---------------------------------------------------------
def test_thin_and_denoise_keep_their_results_after_a_components_call(ctx):
    load(ctx, K.stream("synth"))
    _, xyz, _ = points_of(ctx, "synth")

    def neighbours():
        d = ctx.read_denoise((0, 0, 0, 2048), 23, None, "keep", rows=True)
        ds = dict(ctx.denoise_stats)
        t = ctx.read_thin((-12345, 777, -1, 64), S.BOXES["synth"], T.CENTER, rows=True)
        return d[0].tobytes(), d[1].tobytes(), ds, t[0].tobytes(), t[1].tobytes(), dict(ctx.thin_stats)

    before = neighbours()
    assert np.array_equal(np.frombuffer(before[1], np.int64), D.reference(xyz, (0, 0, 0, 2048), 23, None, D.KEEP))
    assert np.array_equal(np.frombuffer(before[4], np.int64), T.reference(xyz, (-12345, 777, -1, 64), S.BOXES["synth"], T.CENTER))
    check_both_modes(ctx, "synth", (0, 0, 0, 64), 2, 26, None)              # a larger table than either neighbour's
    assert neighbours() == before
    check_both_modes(ctx, "synth", (0, 0, 0, 1 << 20), 100000, 6, S.BOXES["synth"])        # ... and a tiny one
    assert neighbours() == before
    check_both_modes(ctx, "synth", (0, 0, 0, 64), 2, 26, None)


# ---- 7. the resource and the CLI ----------------------------------------------------------------------------------------------------
def run(*cmd):
    res = subprocess.run([str(c) for c in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


def test_resource_and_cli_round_trip(tmp_path):
    """HuffmanLasData.components and pcr_decode --components give the reference over the decoded LAS, in world units."""
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
        for k, (cell, min_points, conn, small, boxed) in enumerate(((1.0, 13, 26, False, False), (1.0, 13, 6, True, False), (2.048, 200, 26, True, True))):
            vox = P.voxels_from_world(info, cell)
            rows, labels = K.reference(ints, (*vox.origin, vox.cell), min_points, S.BOXES["synth"] if boxed else header, conn, K.SMALL if small else K.KEEP)
            assert 0 < len(rows) < len(ax)
            args = ["--components", repr(cell), str(min_points)] + (["--conn", str(conn)] if conn == 6 or boxed else []) + (["--small"] if small else []) \
                + (["--box", *(repr(v) for v in lo + hi)] if boxed else [])
            out = run(build.DECODE_BIN, tmp_path / "a.huffman", tmp_path / f"d{k}.las", *args)
            bx, by, bz, bc, blas = P.read_las(str(tmp_path / f"d{k}.las"))
            assert len(bx) == len(rows), out.stdout
            assert np.array_equal(bx, ax[rows]) and np.array_equal(by, ay[rows]) and np.array_equal(bz, az[rows]) and np.array_equal(bc, ac[rows])
            assert tuple(blas.scale) == tuple(las.scale) and tuple(blas.offset) == tuple(las.offset)
            assert f"written {len(rows)}," in out.stdout and f"connectivity {conn}," in out.stdout and "small components" in out.stdout
            t = torch.from_numpy(rows).to(pts_all.device)
            xyz, pts, lab = res.components(r, cell, min_points, conn, lo if boxed else None, hi if boxed else None, small=small)
            assert torch.equal(pts, pts_all[t]) and torch.equal(xyz, xyz_all[t]) and xyz.dtype == torch.float64
            assert lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), labels)
        rows, labels = K.reference(ints, (0, 0, 0, 4096), 100, None, 26, K.KEEP)
        pts, lab = res.components(r, 4096, 100, world=False)
        assert torch.equal(pts, pts_all[torch.from_numpy(rows).to(pts.device)]) and np.array_equal(lab.cpu().numpy(), labels) and 0 < len(rows) < len(ax)
    finally:
        r.ctx.close()
    # nothing to write is an error, not an empty file
    res = subprocess.run([str(build.DECODE_BIN), str(tmp_path / "a.huffman"), str(tmp_path / "none.las"), "--components", "1", "0", "--small"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 1 and "no points" in res.stderr and not (tmp_path / "none.las").exists()
