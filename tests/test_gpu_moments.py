"""pcr_local_moments / pcr_read_local_moments / pcr_moments_eigen: per row of a range inside a clip the exact moments of the offsets
to the rows within a radius, and the eigenvalues and the normal of their covariance, on the GPU straight from the compressed stream.

The contract: of the rows pcr_decode_points writes for the range that lie inside the clip (the candidates), B(p) holds the
candidates q with d2(p, q) <= r * r, p itself included; n = |B(p)|, s = the sum of q - p, q = the sums of the products of its
components; a candidate is written iff n >= min_count, byte for byte and in increasing row order, with its row, its 80-byte moments
and its 48-byte eigen record. The moments are exact integers: the reference of every call is Context.read_points of the same
range, reduced in numpy (tests/moments_cases.py), compared as bytes, every statistic included. The eigen record is a function of
the moments record alone (cyclic Jacobi in f64): it is held byte for byte against pcr_moments_eigen of the reference's moments, and
that against properties -- ascending finite eigenvalues close to numpy.linalg.eigvalsh's, a unit normal that is an eigenvector of
value[0], the sign rule -- with a tolerance measured in the test: 16 times what numpy.linalg.eigh leaves on the same matrices, at
least 64 * 2^-52 (a plain cyclic Jacobi in numpy left 10.4 * 2^-52 where eigh left 7.0 * 2^-52 over 3000 such matrices; two
backward-stable solvers differ by a small multiple of the unit roundoff per sweep, and at most 6 sweeps were seen). Every case
runs for a context loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH (there through both variants, which
have to agree). tests/test_moments_cpu.py checks the reference and the preconditions of the cases on the CPU.

Measured on an MI355X over all of these cases (printed by every test): numpy.linalg.eigh leaves at most 11.0 * 2^-52, the GPU's
Jacobi at most 3.2 * 2^-52."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from tests import denoise_cases as D
from tests import moments_cases as MC
from tests import neighbors_cases as NC
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_gpu_select import LAYOUTS, load, one_frame, through_variants

pytestmark = pytest.mark.gpu

PPB = S.PPB
PCR_E_ARG = -1
STAT_NAMES = list(N.NeighborsStats().as_dict())
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
_analysed = {}      # (stream, first, count, r, clip) -> (analyse()'s dict, runs, its records, their eigen records -- checked once)
_worst = {"numpy": 0.0, "gpu": 0.0}


def points_of(c, name):
    """read_points of the loaded stream `name` (both variants), held against the first read of it by any context."""
    pts = through_variants(c, c.read_points)
    if name not in _points:
        _points[name] = (pts, T.xyz_of(pts), c.batch_point_bounds())
        _points[name][0].setflags(write=False)
    assert pts.tobytes() == _points[name][0].tobytes()
    return _points[name]


def eigen_checked(c, rec, what):
    """pcr_moments_eigen of the records `rec`, with the eigen properties asserted on every one of them."""
    eig = c.moments_eigen(rec)
    assert eig.dtype == P.EIGEN_DTYPE and len(eig) == len(rec)
    tol, numpy_worst, gpu_worst = MC.check_eigen(rec, eig, what)
    _worst["numpy"], _worst["gpu"] = max(_worst["numpy"], numpy_worst), max(_worst["gpu"], gpu_worst)
    print(f"eigen {what}: {len(rec)} records, numpy.linalg.eigh leaves {numpy_worst:.1f} * 2^-52, the GPU {gpu_worst:.1f} * 2^-52, tol {tol / MC.EPS:.1f} * 2^-52; "
          f"so far numpy {_worst['numpy']:.1f}, GPU {_worst['gpu']:.1f}")
    eig.setflags(write=False)
    return eig


def analysed(c, name, r, clip, first=0, count=None):
    """The reference over batches [first, first + count) of the whole stream `name`, and only over those: analyse()'s dict, the
    runs, the moments records of all candidates and their eigen records (pcr_moments_eigen's, the properties checked)."""
    xyz = _points[name][1]
    count = len(xyz) // PPB - first if count is None else count
    key = (name, first, count, r, clip)
    if key not in _analysed:
        xyz = xyz[first * PPB:(first + count) * PPB]
        an = MC.analyse(xyz, r, clip)
        assert an["pairs"] < 3e7, "the reference of this case is slow: choose a smaller radius"
        assert np.array_equal(an["q"][:, 0] + an["q"][:, 3] + an["q"][:, 5] >= 0, np.ones(len(an["n"]), bool))
        rec = MC.records(an)
        for v in list(an.values()) + [rec]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _analysed[key] = (an, MC.count_runs(xyz, r, clip), rec, eigen_checked(c, rec, f"({name} r {r} {clip} batches {first}..{first + count})"))
    return _analysed[key]


def moments(c, r, min_count, clip, first=0, count=None):
    """read_local_moments of the range with rows, moments and eigen (both variants) and the statistics it reported."""
    def go():
        pts, rows, mom, eig = c.read_local_moments(r, min_count, clip, first, count, rows=True, moments=True, eigen=True)
        return pts, rows, mom, eig, np.array([c.moments_stats[k] for k in STAT_NAMES])
    pts, rows, mom, eig, st = through_variants(c, go)
    return pts, rows, mom, eig, dict(zip(STAT_NAMES, (int(v) for v in st)))


def check(c, name, r, min_count, clip, first=0, count=None, base=0, extras=False):
    """read_local_moments == the reference over read_points of the same range: records, rows and moments byte for byte, every
    statistic, and the eigen records byte for byte pcr_moments_eigen's of the reference's moments; or, where the lattice limits
    say so, a refusal that names the way out. extras: also the count-only call, the call without moments and eigen, and
    read_neighbors' N on the same arguments. `base`: the batch of the stream that is batch 0 of the context. Returns (records,
    rows, moments, eigen, statistics), or None for a refusal."""
    pts_all, _, bounds = _points[name]
    f0 = base + first
    last = len(pts_all) // PPB if count is None else f0 + count
    if MC.lattice_refusal(bounds[f0:last], r, clip):
        with pytest.raises(P.PcrError, match="clip or a larger radius"):
            c.read_local_moments(r, min_count, clip, first, count)
        return None
    an, runs, rec, eig = analysed(c, name, r, clip, f0, last - f0)
    at = MC.written(an, min_count)
    rows = an["rows"][at]
    got, got_rows, got_m, got_e, st = moments(c, r, min_count, clip, first, count)
    want = pts_all[f0 * PPB:last * PPB][rows]
    what = f"({name} r {r} min_count {min_count} {clip} batches {f0}..{last})"
    assert got.dtype == want.dtype and got_rows.dtype == np.int64 and got_m.dtype == P.MOMENTS_DTYPE and got_e.dtype == P.EIGEN_DTYPE
    assert len(got) == len(want) == len(got_rows) == len(got_m) == len(got_e), f"{len(got)} records written, {len(want)} expected {what}"
    assert got_rows.tobytes() == rows.tobytes(), f"rows differ, first at {np.nonzero(got_rows != rows)[0][:4]} {what}"
    assert got.tobytes() == want.tobytes(), f"records differ {what}"
    bad = np.nonzero(got_m != rec[at])[0]
    assert got_m.tobytes() == rec[at].tobytes(), f"moments differ at {bad[:4]}: {got_m[bad[:4]]} for {rec[at][bad[:4]]} {what}"
    bad = np.nonzero(got_e != eig[at])[0]
    assert got_e.tobytes() == eig[at].tobytes(), f"eigen records differ from pcr_moments_eigen's at {bad[:4]}: {got_e[bad[:4]]} for {eig[at][bad[:4]]} {what}"
    dec = MC.decoded_batches(bounds[f0:last], clip)
    assert st == MC.stats(an, runs, last - f0, dec, min_count), what
    if extras:
        pts, only_rows = through_variants(c, lambda: c.read_local_moments(r, min_count, clip, first, count, rows=True))
        assert pts.tobytes() == got.tobytes() and only_rows.tobytes() == rows.tobytes()
        assert {k: c.moments_stats[k] for k in STAT_NAMES} == st, "the statistics of the call without moments and eigen differ"
        cnt, cst = C.c_int64(-5), N.NeighborsStats()
        box = None if clip is None else P.as_box(clip)
        assert c.lib.pcr_local_moments(c.h, first, -1 if count is None else count, r, None if box is None else C.byref(box), min_count, None, None, None,
                                       None, 0, C.byref(cnt), C.byref(cst)) == 0
        assert cnt.value == len(rows) and cst.as_dict() == st, "the counting-only call differs"
        _, n_rows, n = c.read_neighbors(r, min_count, clip, "keep", first, count, rows=True, counts=True)
        assert n_rows.tobytes() == rows.tobytes() and n.tobytes() == np.ascontiguousarray(got_m["n"]).tobytes(), "n is not pcr_neighbors' N"
    return got, got_rows, got_m, got_e, st


def threshold(c, name, r, clip, first=0, count=None):
    """min_count of a case: the median of N, but at least 2 (at 1 everything is written)."""
    return max(MC.median_n(analysed(c, name, r, clip, first, count)[0]), 2)


# ---- 1. against the numpy reference (and 3., 4.: the eigen records are pcr_moments_eigen's, whose properties hold) ----------------
@pytest.mark.parametrize("name", MC.STREAMS)
@pytest.mark.parametrize("frame", [True, False], ids=["after_frame", "before_any_frame"])
def test_moments_equal_the_reference(ctx, name, frame):
    load(ctx, MC.stream(name), frame=frame)
    _, xyz, bounds = points_of(ctx, name)
    clip = MC.clip_for(name, xyz)
    done = 0
    for r, q in itertools.product(MC.RADII[name], (None, clip)):
        assert r <= MC.MAX_RADIUS
        if MC.lattice_refusal(bounds, r, q):
            assert check(ctx, name, r, 3, q) is None
            continue
        k = threshold(ctx, name, r, q)
        kept = check(ctx, name, r, k, q, extras=True)
        everything = check(ctx, name, r, 0, q)
        assert check(ctx, name, r, 1, q)[1].tobytes() == everything[1].tobytes() and everything[4]["points_sparse"] == 0
        nothing = check(ctx, name, r, MC.HUGE, q)
        assert len(nothing[1]) == 0 and nothing[4]["points_sparse"] == len(everything[1]) == nothing[4]["points_considered"]
        assert len(kept[1]) <= len(everything[1])                           # (escape_heavy at r = 64: no row has a neighbour)
        done += 1
        print(f"{name} r {r} clip {q}: min_count {k}, {kept[4]}")
    assert done >= (2 if name == "wide30" else 4)                           # (wide30 without a clip is refused at every radius)
    if not frame:                                                           # ... and the first frame changes nothing
        before = ctx.read_local_moments(r, k, q, rows=True, moments=True, eigen=True)
        one_frame(ctx)
        after = ctx.read_local_moments(r, k, q, rows=True, moments=True, eigen=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


# ---- 2. ranges ------------------------------------------------------------------------------------------------------------------------
def test_sub_range_counts_its_own_batches_only(ctx):
    """first = 1, count = 2: the reference is taken over those two batches' rows, so neighbours in batches 0 and 3 do not exist."""
    load(ctx, MC.stream("synth"))
    _, xyz, _ = points_of(ctx, "synth")
    r = 2500
    everything = check(ctx, "synth", r, 0, None, 1, 2, extras=True)
    an = analysed(ctx, "synth", r, None)[0]
    inside = (an["rows"] >= PPB) & (an["rows"] < 3 * PPB)
    assert np.array_equal(an["rows"][inside] - PPB, everything[1])
    assert (everything[2]["n"] <= an["n"][inside]).all() and (everything[2]["n"] < an["n"][inside]).sum() >= 1, "no row of batches 1..2 has a neighbour in batches 0 or 3"
    assert 0 <= everything[1][0] and everything[1][-1] < 2 * PPB            # rows count from the range's start
    check(ctx, "synth", r, threshold(ctx, "synth", r, None, 1, 2), S.BOXES["synth"], 1, 2)
    nb = len(xyz) // PPB
    got = moments(ctx, r, 3, None, nb, None)
    assert len(got[0]) == 0 and got[4] == ZERO


def test_sub_range_of_a_stream_loaded_from_a_later_batch(ctx):
    image = MC.stream("synth")
    load(ctx, image)
    points_of(ctx, "synth")
    load(ctx, image, first=3, count=5)                                      # batches 3..7 of the file, the follower's head words behind them
    ref = through_variants(ctx, ctx.read_points)
    assert ref.tobytes() == _points["synth"][0][3 * PPB:8 * PPB].tobytes()
    r = 2500
    k = threshold(ctx, "synth", r, None, 3, 5)
    kept = check(ctx, "synth", r, k, None, 0, 5, base=3, extras=True)
    assert 0 < len(kept[1]) < 5 * PPB
    for first, count in ((0, 2), (2, 0), (2, 1), (4, 1)):                   # batch `first` of the context is batch 3 + first of the stream
        check(ctx, "synth", r, k, S.BOXES["synth"] if first == 2 else None, first, count, base=3)


# ---- 3. the eigen record as a function of the moments -----------------------------------------------------------------------------
def test_eigen_is_a_function_of_the_moments(ctx):
    """The eigen array of a call == moments_eigen of its moments on the device == the standalone call on the host-read moments
    uploaded again, byte for byte."""
    import torch
    load(ctx, MC.stream("clustered"))
    points_of(ctx, "clustered")
    r = 400
    pts, rows, mom, eig = ctx.local_moments(r, 5, None, rows=True, moments=True, eigen=True)
    assert mom.dtype == torch.int64 and tuple(mom.shape) == (len(pts), 10) and eig.dtype == torch.float64 and tuple(eig.shape) == (len(pts), 6)
    again = ctx.moments_eigen(mom)
    assert again.dtype == torch.float64 and again.is_cuda and again.cpu().numpy().tobytes() == eig.cpu().numpy().tobytes()
    hp, hr, hm, he = ctx.read_local_moments(r, 5, None, rows=True, moments=True, eigen=True)
    assert hm.tobytes() == mom.cpu().numpy().tobytes() and he.tobytes() == eig.cpu().numpy().tobytes() and len(hm) > 1000
    up = ctx.moments_eigen(hm)
    assert up.dtype == P.EIGEN_DTYPE and up.tobytes() == he.tobytes()
    assert ctx.moments_eigen(hm.view("<i8").reshape(-1, 10)).tobytes() == he.tobytes()
    eig_only = ctx.local_moments(r, 5, None, eigen=True)[1]                 # the dense moments are not allocated for this one
    mom_only = ctx.local_moments(r, 5, None, moments=True)[1]
    assert eig_only.cpu().numpy().tobytes() == he.tobytes() and mom_only.cpu().numpy().tobytes() == hm.tobytes()


# ---- 5. facets, exact ----------------------------------------------------------------------------------------------------------------
def test_facets_are_exact(ctx):
    load(ctx, MC.stream("facets"))
    _, xyz, _ = points_of(ctx, "facets")
    got, rows, mom, eig, st = check(ctx, "facets", MC.FACETS_R, 0, None, extras=True)
    assert np.array_equal(rows, np.arange(PPB))
    cls = MC.facets_classes(xyz)
    cov = P.covariance_from_moments(mom)
    scale = np.abs(cov).reshape(-1, 9).max(axis=1)
    live = scale > 0
    tol, numpy_worst = MC.measured_tolerance(cov[live])
    up, east = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    h, w = eig[cls["horizontal"]], eig[cls["wall"]]
    assert len(h) >= 1000 and len(w) >= 1000
    assert np.ascontiguousarray(h["value"][:, 0]).tobytes() == np.zeros(len(h)).tobytes(), "a horizontal row's least eigenvalue is not 0.0"
    assert np.ascontiguousarray(h["normal"]).tobytes() == np.tile(up, len(h)).tobytes(), "a horizontal row's normal is not (0, 0, 1) to the bit"
    assert np.ascontiguousarray(w["value"][:, 0]).tobytes() == np.zeros(len(w)).tobytes()
    assert np.ascontiguousarray(w["normal"]).tobytes() == np.tile(east, len(w)).tobytes(), "a wall row's normal is not (1, 0, 0) to the bit"
    one = eig[cls["single"]]
    assert len(one) == 1 and mom[cls["single"]]["n"][0] == 1
    assert np.ascontiguousarray(one["value"]).tobytes() == np.zeros(3).tobytes() and np.ascontiguousarray(one["normal"]).tobytes() == east.tobytes()
    pad = eig[cls["padding"]]                                               # the zero matrix with n > 1
    assert (pad["value"] == 0).all() and (pad["normal"] == east).all() and (mom[cls["padding"]]["n"] == len(pad)).all()
    o = cls["oblique"]
    assert o.sum() >= 1000
    assert np.abs(eig["normal"][o] - np.ones(3) / np.sqrt(3.0)).max() <= tol and (eig["value"][o][:, 0] <= tol * scale[o]).all()
    line = cls["line"]
    assert line.sum() >= 100 and (eig["value"][line][:, :2] <= tol * scale[line][:, None]).all() and (eig["value"][line][:, 2] > 0).all()
    assert (mom["n"] == 2).sum() == 2 and np.array_equal(mom["n"] == 2, cls["pair"])
    # min_count = 3 drops the single point and the pair, and nothing else
    kept = check(ctx, "facets", MC.FACETS_R, 3, None)
    assert np.array_equal(kept[1], np.nonzero(~(cls["single"] | cls["pair"]))[0]) and kept[4]["points_sparse"] == 3


# ---- 6. ball: every point sees all of them ---------------------------------------------------------------------------------------
def test_ball_equals_the_closed_form(ctx):
    load(ctx, MC.stream("ball"))
    _, xyz, _ = points_of(ctx, "ball")
    want = MC.closed_form(xyz)
    assert np.abs(want["q"]).max() >= 1 << 40
    got, rows, mom, eig, st = moments(ctx, MC.BALL_R, PPB, None)
    assert np.array_equal(rows, np.arange(PPB)) and got.tobytes() == _points["ball"][0].tobytes()
    bad = np.nonzero(mom != want)[0]
    assert mom.tobytes() == want.tobytes(), f"moments differ at {bad[:4]}: {mom[bad[:4]]} for {want[bad[:4]]}"
    assert st["pairs_bound"] == PPB * PPB and st["voxels"] == 1 and st["max_voxel_points"] == PPB and st["points_sparse"] == 0
    assert eig.tobytes() == eigen_checked(ctx, want, "(ball)").tobytes()
    assert moments(ctx, MC.BALL_R, PPB + 1, None)[4]["points_sparse"] == PPB


# ---- 7. hand-made moments through pcr_moments_eigen -----------------------------------------------------------------------------
def test_handmade_moments(ctx):
    import torch
    m, names = MC.handmade()
    e = eigen_checked(ctx, m, "(hand-made)")
    by = dict(zip(names, e))
    assert by["n = 0"].tobytes() == by["n = -1"].tobytes() == bytes(48)
    assert tuple(by["diagonal, tie of x and z below y"]["value"]) == (4.0, 4.0, 9.0) and tuple(by["diagonal, tie of x and z below y"]["normal"]) == (1.0, 0.0, 0.0)
    assert tuple(by["diagonal, tie of y and z below x"]["value"]) == (4.0, 4.0, 9.0) and tuple(by["diagonal, tie of y and z below x"]["normal"]) == (0.0, 1.0, 0.0)
    assert tuple(by["diagonal, descending"]["value"]) == (1.0, 4.0, 9.0) and tuple(by["diagonal, descending"]["normal"]) == (0.0, 0.0, 1.0)
    assert tuple(by["k * identity"]["value"]) == (7.0, 7.0, 7.0) and tuple(by["k * identity"]["normal"]) == (1.0, 0.0, 0.0)
    assert by["the zero matrix"].tobytes() == np.array([0, 0, 0, 1.0, 0, 0]).tobytes()
    # n = 0 records: nothing happens, whatever the pointers
    lib, h = ctx.lib, ctx.h
    assert lib.pcr_moments_eigen(h, None, 0, None) == 0 and len(ctx.moments_eigen(m[:0])) == 0
    dev = f"cuda:{ctx.device}"
    src = torch.zeros(4 * 10 + 2, dtype=torch.int64, device=dev)
    dst = torch.full((4 * 6 + 2,), 7.0, dtype=torch.float64, device=dev)
    for args in ((None, dst.data_ptr()), (src.data_ptr(), None), (src.data_ptr() + 4, dst.data_ptr()), (src.data_ptr(), dst.data_ptr() + 4)):
        assert lib.pcr_moments_eigen(h, C.c_void_p(args[0]), 4, C.c_void_p(args[1])) == PCR_E_ARG and (lib.pcr_last_error(h) or b"") != b""
    assert lib.pcr_moments_eigen(h, C.c_void_p(src.data_ptr()), -1, C.c_void_p(dst.data_ptr())) == PCR_E_ARG
    assert (dst.cpu().numpy() == 7.0).all()
    assert lib.pcr_moments_eigen(h, C.c_void_p(src.data_ptr() + 8), 4, C.c_void_p(dst.data_ptr() + 8)) == 0      # 8-byte alignment is enough
    out = dst.cpu().numpy()
    assert out[0] == 7.0 and out[-1] == 7.0 and (out[1:-1] == 0).all()


# ---- 8. the contract ---------------------------------------------------------------------------------------------------------------
def test_refusals_capacity_and_canaries(ctx):
    import torch
    lib, h = ctx.lib, ctx.h
    cnt = C.c_int64(-5)
    assert lib.pcr_local_moments(h, 0, 1, 700, None, 3, None, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG     # no stream loaded
    load(ctx, MC.stream("synth"))
    pts_all, xyz, _ = points_of(ctx, "synth")
    r, clip_t = 2500, S.BOXES["synth"]
    box = P.as_box(clip_t)
    for entry in (lib.pcr_local_moments, lib.pcr_read_local_moments):
        for bad_r in (0, -1, 32768, 1 << 20, S.INT32_MIN, S.INT32_MAX):
            assert entry(h, 0, 1, bad_r, None, 3, None, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG and cnt.value == 0
            assert b"PCR_MOMENTS_MAX_RADIUS" in (lib.pcr_last_error(h) or b"")
        for bad_min in (-1, -(1 << 62)):
            assert entry(h, 0, 1, r, None, bad_min, None, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG
        assert entry(h, 0, 1, r, None, 3, None, None, None, None, 0, None, None) == PCR_E_ARG                            # a NULL out_count
        for first, count in ((ctx.batches_loaded - 1, 2), (-1, 1), (ctx.batches_loaded + 1, -1)):
            assert entry(h, first, count, r, None, 3, None, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG
        assert entry(h, 0, 1, 32767, None, 3, None, None, None, None, 0, C.byref(cnt), None) == 0                        # the largest radius
    an, runs, rec, eig = analysed(ctx, "synth", r, clip_t)
    k = threshold(ctx, "synth", r, clip_t)
    at = MC.written(an, k)
    rows, n = an["rows"][at], len(at)
    assert 1000 < n < len(an["rows"])
    wants = (pts_all[rows].tobytes(), rows.tobytes(), rec[at].tobytes(), eig[at].tobytes())
    sizes = (16, 8, 80, 48)
    PAD, SENT = 64, 0x5A
    # the device path: canaries before and behind all four outputs
    bufs = [torch.full(((n + 2 * PAD) * size,), SENT, dtype=torch.uint8, device=f"cuda:{ctx.device}") for size in sizes]
    ptrs = [b.data_ptr() + PAD * size for b, size in zip(bufs, sizes)]
    assert all(p % 16 == 0 for p in ptrs)
    st = N.NeighborsStats()

    def dev_call(with_, cap):
        torch.cuda.synchronize()
        return lib.pcr_local_moments(h, 0, -1, r, C.byref(box), k, *(C.c_void_p(p if w else None) for p, w in zip(ptrs, with_)), cap, C.byref(cnt), C.byref(st))

    for with_ in ((True,) * 4, (True, False, False, True), (False, True, True, False), (False, False, True, False), (False, False, False, True)):
        for b in bufs:
            b.fill_(SENT)
        cnt.value = -5
        assert dev_call(with_, n - 1) == PCR_E_ARG and cnt.value == n and (lib.pcr_last_error(h) or b"") != b""
        ctx.synchronize(); torch.cuda.synchronize()
        assert all((b.cpu().numpy() == SENT).all() for b in bufs), "a refused call wrote into a buffer"
        assert dev_call(with_, n) == 0 and cnt.value == n == st.points_written
        for b, size, w, want in zip(bufs, sizes, with_, wants):
            g = b.cpu().numpy()
            assert (g[:PAD * size] == SENT).all() and (g[(PAD + n) * size:] == SENT).all(), "a canary around the result was overwritten"
            assert (g[PAD * size:(PAD + n) * size].tobytes() == want) if w else (g == SENT).all()
    for k_ptr, off in ((0, 8), (1, 4), (2, 4), (3, 4)):                     # records not 16-byte aligned, the others not 8-byte aligned
        bad = list(ptrs)
        bad[k_ptr] += off
        assert lib.pcr_local_moments(h, 0, -1, r, C.byref(box), k, *(C.c_void_p(p) for p in bad), n, C.byref(cnt), None) == PCR_E_ARG
    # the host path
    hbufs = [np.full((n + 2 * PAD) * size, SENT, np.uint8) for size in sizes]
    hptrs = [b.ctypes.data + PAD * size for b, size in zip(hbufs, sizes)]
    cnt.value = -5
    assert lib.pcr_read_local_moments(h, 0, -1, r, C.byref(box), k, *(C.c_void_p(p) for p in hptrs), n - 1, C.byref(cnt), None) == PCR_E_ARG
    assert cnt.value == n and all((b == SENT).all() for b in hbufs)
    assert lib.pcr_read_local_moments(h, 0, -1, r, C.byref(box), k, *(C.c_void_p(p) for p in hptrs), n + 5, C.byref(cnt), None) == 0 and cnt.value == n
    for b, size, want in zip(hbufs, sizes, wants):
        assert (b[:PAD * size] == SENT).all() and (b[(PAD + n) * size:] == SENT).all() and b[PAD * size:(PAD + n) * size].tobytes() == want
    # an empty clip, a clip that misses everything, an empty range: 0 records, zero statistics
    nb = len(pts_all) // PPB
    for clip in (S.EMPTY, S.NOTHING):
        got = check(ctx, "synth", 700, 3, clip, extras=True)
        assert len(got[0]) == 0 and got[4] == dict(ZERO, batches_outside=nb)
    for first in (0, 3, nb):
        got = moments(ctx, 700, 3, None, first, 0)
        assert len(got[0]) == 0 and got[4] == ZERO
    # Context.local_moments (torch) equals read_local_moments (numpy), with and without `out`
    t, tr, tm, te = ctx.local_moments(r, k, clip_t, rows=True, moments=True, eigen=True)
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (n, 4) and ctx.moments_stats["points_written"] == n
    assert tuple(g.cpu().numpy().tobytes() for g in (t, tr, tm, te)) == wants
    only = ctx.local_moments(r, k, clip_t)
    assert torch.equal(only, t)
    out = torch.empty((n + 3, 4), dtype=torch.int32, device=t.device)
    o, oe = ctx.local_moments(r, k, clip_t, out=out, eigen=True)
    assert torch.equal(o, t) and torch.equal(oe, te)
    with pytest.raises(P.PcrError):
        ctx.local_moments(r, k, clip_t, out=torch.empty((n - 1, 4), dtype=torch.int32, device=t.device))
    assert ctx.moments_stats["points_written"] == n
    assert tuple(ctx.local_moments(r, k, S.EMPTY).shape) == (0, 4)


def test_lattice_limits(ctx):
    """wide30 spans 2^30 on x: without a clip the call is refused with pcr_neighbors' advice; with a clip it succeeds."""
    load(ctx, MC.stream("wide30"))
    _, _, bounds = points_of(ctx, "wide30")
    assert MC.lattice_refusal(bounds, 1) == "voxels" and MC.lattice_refusal(bounds, 2) == "voxels"
    cnt = C.c_int64(-5)
    for entry in (ctx.lib.pcr_local_moments, ctx.lib.pcr_read_local_moments):
        for r in (1, 2):
            assert entry(ctx.h, 0, -1, r, None, 5, None, None, None, None, 0, C.byref(cnt), None) == PCR_E_ARG and cnt.value == 0
            msg = ctx.lib.pcr_last_error(ctx.h) or b""
            assert b"clip" in msg and b"larger radius" in msg
    assert check(ctx, "wide30", 1, 2, ((0, 0, 0), ((1 << 21) - 4, 1999, 49))) is not None        # extent / r + 4 = 2^21
    assert check(ctx, "wide30", 1, 2, ((0, 0, 0), ((1 << 21) - 3, 1999, 49))) is None            # one more: refused


# ---- 9. the other calls of the shared scratch are unchanged -------------------------------------------------------------------------
def test_other_calls_are_unchanged_after_local_moments(ctx):
    load(ctx, MC.stream("synth"))
    _, xyz, _ = points_of(ctx, "synth")

    def thin():
        vox = (-12345, 777, -1, 64)
        pts, rows = through_variants(ctx, lambda: ctx.read_thin(vox, S.BOXES["synth"], T.CENTER, rows=True))
        return pts.tobytes(), rows.tobytes(), dict(ctx.thin_stats)

    def denoise():
        pts, rows = through_variants(ctx, lambda: ctx.read_denoise((0, 0, 0, 7001), 262, None, "isolated", rows=True))
        return pts.tobytes(), rows.tobytes(), dict(ctx.denoise_stats)

    def neighbors():
        res = through_variants(ctx, lambda: ctx.read_neighbors(2500, 9, None, "all", rows=True, counts=True, nn2=True))
        return tuple(a.tobytes() for a in res) + (dict(ctx.neighbors_stats),)

    others = (thin, denoise, neighbors)
    alone = [f() for f in others]
    assert alone[0][1] == T.reference(xyz, (-12345, 777, -1, 64), S.BOXES["synth"], T.CENTER).tobytes()
    assert alone[1][1] == D.reference(xyz, (0, 0, 0, 7001), 262, None, D.ISOLATED).tobytes()
    an = NC.analyse(xyz, 2500)
    assert alone[2][2] == an["n"].tobytes() and alone[2][3] == an["nn2"].tobytes()
    a, b = (2500, 9, None), (700, 2, S.BOXES["synth"])
    first = check(ctx, "synth", *a)
    for f, ref in zip(others, alone):                                       # each of the others right after a pcr_local_moments ...
        check(ctx, "synth", *b)
        assert f() == ref
        again = check(ctx, "synth", *a)                                     # ... and pcr_local_moments right after each of them
        assert all(p.tobytes() == q.tobytes() for p, q in zip(first[:4], again[:4])) and first[4] == again[4]
