"""pcr_thin, pcr_denoise, pcr_components, pcr_neighbors and pcr_local_moments on the streams of tests/adversarial_cases.py: one long
cluster of colliding keys that wraps the table's end, voxel populations at the 64-entry edges of the pair kernels, the arithmetic at
its documented limits, and components whose structure is the hard part.

Nothing here is new on the reference side: every call is held against the numpy reference of its own suite with that suite's
helper (records, rows, labels, N, nn2, moments byte for byte, every statistic; the eigen records as tests/test_gpu_moments.py holds
them). What is new is the input, and tests/test_adversarial_cpu.py proves from the oracle's decode that each stream is what it
claims. The one piece of evidence that the GPU ran the table that was proven is `table_slots` in the statistics: it has to be the
CPU's value. Every case runs for a context loaded with PCR_LAYOUT_WORDS, PCR_LAYOUT_POINT_WINDOWS and PCR_LAYOUT_BOTH."""
import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import adversarial_cases as A
from tests import components_cases as K
from tests import denoise_cases as D
from tests import moments_cases as MC
from tests import neighbors_cases as NC
from tests import test_gpu_components as GK
from tests import test_gpu_denoise as GD
from tests import test_gpu_moments as GM
from tests import test_gpu_neighbors as GN
from tests import test_gpu_thin as GT
from tests import thin_cases as T
from tests.test_gpu_select import LAYOUTS, load

pytestmark = pytest.mark.gpu

PPB = A.PPB
SUITES = (GT, GD, GK, GN, GM)


@pytest.fixture(params=list(LAYOUTS))
def ctx(request):
    c = P.Context(0)
    c.set_stream_layout(LAYOUTS[request.param])
    c.set_image_size(160, 90)
    c.layout_name = request.param
    yield c
    c.close()


def loaded(c, name, suites=SUITES):
    """The stream loaded, its decode held against the rows it was built from, and registered with the suites whose helpers check it.
    Returns the rows as int64 [65536, 3]."""
    load(c, A.stream(name))
    for suite in suites:
        _, xyz, _ = suite.points_of(c, name)
    assert np.array_equal(xyz, A.points(name)), "the GPU does not decode the rows the case was built from"
    return xyz


# ---- 1. collide ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, A.COLLIDE_CLIP], ids=["whole", "clipped"])
def test_collide_thin(ctx, clip):
    xyz = loaded(ctx, "collide", (GT,))
    vox = (0, 0, 0, A.COLLIDE_CELL)
    slots = T.table_slots(T.count_runs(xyz, vox, clip))
    assert slots == (A.COLLIDE_SLOTS if clip is None else A.COLLIDE_CLIP_SLOTS)
    for mode in (T.FIRST, T.CENTER):
        got, rows, st = GT.check_thin(ctx, "collide", vox, clip, mode)
        assert st["table_slots"] == slots and 0 < len(rows) < st["points_considered"]
        print(f"collide thin mode {mode} clip {clip}: {st}")


@pytest.mark.parametrize("clip", [None, A.COLLIDE_CLIP], ids=["whole", "clipped"])
def test_collide_denoise(ctx, clip):
    xyz = loaded(ctx, "collide", (GD,))
    vox = (0, 0, 0, A.COLLIDE_CELL)
    slots = D.table_slots(D.count_runs(xyz, vox, clip))
    assert slots == (A.COLLIDE_SLOTS if clip is None else A.COLLIDE_CLIP_SLOTS)
    median = D.median_n27(GD.analysed("collide", vox, clip)[0])
    keep, iso = GD.check_both_modes(ctx, "collide", vox, median, clip)
    assert len(keep[1]) > 0 and len(iso[1]) > 0 and keep[2]["table_slots"] == slots
    keep, iso = GD.check_both_modes(ctx, "collide", vox, D.HUGE, clip)      # no voxel reaches it: all 26 lookups of every voxel
    assert len(keep[1]) == 0 and iso[2]["voxels_isolated"] == iso[2]["voxels"] and iso[2]["table_slots"] == slots
    print(f"collide denoise clip {clip}: median N27 {median}, {iso[2]}")


@pytest.mark.parametrize("clip", [None, A.COLLIDE_CLIP], ids=["whole", "clipped"])
def test_collide_components(ctx, clip):
    xyz = loaded(ctx, "collide", (GK,))
    vox = (0, 0, 0, A.COLLIDE_CELL)
    slots = K.table_slots(K.count_runs(xyz, vox, clip))
    assert slots == (A.COLLIDE_SLOTS if clip is None else A.COLLIDE_CLIP_SLOTS)
    for conn in (6, 26):
        median = K.median_size(GK.analysed("collide", vox, clip, conn)[0])
        keep, small = GK.check_both_modes(ctx, "collide", vox, median, conn, clip)
        assert len(keep[1]) > 0 and len(small[1]) > 0 and keep[3]["table_slots"] == slots
        GK.labels_are_first_rows(keep[1], keep[2])
        print(f"collide components conn {conn} clip {clip}: min_points {median}, {keep[3]}")


@pytest.mark.parametrize("clip", [None, A.COLLIDE_CLIP], ids=["whole", "clipped"])
def test_collide_neighbors(ctx, clip):
    xyz = loaded(ctx, "collide", (GN,))
    r = A.COLLIDE_CELL
    slots = NC.table_slots(NC.count_runs(xyz, r, clip))
    assert slots == (A.COLLIDE_SLOTS if clip is None else A.COLLIDE_CLIP_SLOTS)
    k = GN.threshold("collide", r, clip)
    everything, keep, sparse = GN.check_modes(ctx, "collide", r, k, clip)   # ALL with N and nn2, KEEP and SPARSE with and without them
    assert len(keep[1]) > 0 and len(sparse[1]) > 0 and everything[4]["table_slots"] == slots
    assert (everything[3] == 0).any() and ((everything[3] != 0) & (everything[3] != NC.NONE)).any()
    print(f"collide neighbors clip {clip}: min_count {k}, {keep[4]}")


@pytest.mark.parametrize("clip", [None, A.COLLIDE_CLIP], ids=["whole", "clipped"])
def test_collide_moments(ctx, clip):
    xyz = loaded(ctx, "collide", (GM,))
    r = A.COLLIDE_CELL
    slots = NC.table_slots(MC.count_runs(xyz, r, clip))
    assert slots == (A.COLLIDE_SLOTS if clip is None else A.COLLIDE_CLIP_SLOTS)
    got = GM.check(ctx, "collide", r, 0, clip)
    assert got[4]["table_slots"] == slots and len(got[1]) == got[4]["points_considered"] > 0
    kept = GM.check(ctx, "collide", r, GM.threshold(ctx, "collide", r, clip), clip)
    assert 0 < len(kept[1]) < len(got[1])
    print(f"collide moments clip {clip}: {kept[4]}")


# ---- 2. edges64 ------------------------------------------------------------------------------------------------------------------
def test_edges64_neighbors(ctx):
    loaded(ctx, "edges64", (GN,))
    r = A.EDGE_CELL
    for k in A.THRESHOLDS:
        # ALL with N and nn2; KEEP and SPARSE with them and, where a wave may leave the pair loop early, without
        everything, keep, sparse = GN.check_modes(ctx, "edges64", r, k, None)
        assert len(keep[1]) > 0 and len(sparse[1]) > 0
        print(f"edges64 neighbors min_count {k}: {keep[4]}")
    n, nn2 = everything[2], everything[3]
    assert (nn2 == 0).any() and (nn2 == NC.NONE).any() and ((nn2 != 0) & (nn2 != NC.NONE)).any()
    assert all((n == c).any() for c in (1, 63, 64, 65, 127, 128, 129, 4096, 4097))


def test_edges64_moments(ctx):
    loaded(ctx, "edges64", (GM,))
    got = GM.check(ctx, "edges64", A.EDGE_CELL, 0, None, extras=True)
    assert np.array_equal(got[1], np.arange(PPB))
    assert all((got[2]["n"] == c).any() for c in (1, 63, 64, 65, 127, 128, 129, 4096, 4097))
    print(f"edges64 moments: {got[4]}")


def test_edges64_denoise_and_components(ctx):
    loaded(ctx, "edges64", (GD, GK))
    vox = (0, 0, 0, A.EDGE_CELL)
    median = D.median_n27(GD.analysed("edges64", vox, None)[0])
    keep, iso = GD.check_both_modes(ctx, "edges64", vox, median, None)
    assert len(keep[1]) > 0 and len(iso[1]) > 0
    for conn in (6, 26):
        k = max(K.median_size(GK.analysed("edges64", vox, None, conn)[0]), 2)
        keep, small = GK.check_both_modes(ctx, "edges64", vox, k, conn, None)
        assert len(keep[1]) > 0 and len(small[1]) > 0
        GK.labels_are_first_rows(keep[1], keep[2])


# ---- 3. extremes -----------------------------------------------------------------------------------------------------------------
def test_moments_at_the_largest_radius(ctx):
    """Four squares of 32767^2 between two flushes, sums of -64 * 32767, a point one step outside the sphere."""
    xyz = loaded(ctx, "moments_limit", (GM,))
    r = A.MOMENTS_R
    got, rows, mom, eig, st = GM.check(ctx, "moments_limit", r, 0, None, extras=True)
    assert np.array_equal(rows, np.arange(PPB))
    origin = (xyz == 0).all(axis=1)
    assert origin.sum() == A.MOMENTS_COPIES and (mom["q"][origin][:, (0, 3, 5)] >= 64 * r * r).all() and (mom["n"][origin] == 6 * A.MOMENTS_COPIES).all()
    assert (mom["s"][:, 0] <= -64 * r).any() and (mom["s"][:, 1] <= -64 * r).any() and (mom["s"][:, 2] <= -64 * r).any()
    print(f"moments_limit: {st}")


def test_neighbors_at_the_largest_radius(ctx):
    """Pairs at exactly 2^20 (nn2 = 2^40, counted), one step outside (not counted), and 2^40 - 447 (odd low word, high word needed)."""
    loaded(ctx, "neighbors_limit", (GN,))
    r = A.NEIGHBORS_R
    everything, keep, sparse = GN.check_modes(ctx, "neighbors_limit", r, 2, None)
    got, rows, n, nn2, st = everything
    assert np.array_equal(rows, np.arange(PPB)) and len(sparse[1]) == 3
    assert (nn2 == np.uint64(1 << 40)).sum() == 6 and (nn2 == np.uint64((1 << 40) - 447)).sum() == 2 and (nn2 == NC.NONE).sum() == 3 and (nn2 == 0).sum() > 2
    assert (n[nn2 == NC.NONE] == 1).all()
    print(f"neighbors_limit: {st}")


# ---- 4. shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
def test_shapes_components(ctx, conn):
    loaded(ctx, "shapes", (GK,))
    vox = (0, 0, 0, A.SHAPES_CELL)
    path = PPB - 2 * A.STAIRS
    for min_points in (2, A.STAIRS + 1, path + 1):
        keep, small = GK.check_both_modes(ctx, "shapes", vox, min_points, conn, None)
        st = keep[3]
        assert st["table_slots"] == 2 * PPB and st["components"] == (3 if conn == 26 else 1 + 2 * A.STAIRS) and st["largest_points"] == path
        if len(keep[1]):
            GK.labels_are_first_rows(keep[1], keep[2])
        if len(small[1]):
            GK.labels_are_first_rows(small[1], small[2])
        print(f"shapes conn {conn} min_points {min_points}: {st}")
    assert len(keep[1]) == 0 and len(small[1]) == PPB                       # one above the path's size: everything is small
