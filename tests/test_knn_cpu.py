"""k nearest neighbours, the parts that need no GPU: the two entry points and the constants in the headers, the binding tables and
the cross-compiled library; the numpy reference of tests/knn_cases.py against the definition evaluated over every pair; the
preconditions of tests/test_gpu_knn.py counted from the oracle's decode of `knn_edges`; the size of every reference the GPU tests
compute; knn_mean_distance and the outlier rule on hand-made arrays, and on the scene of tests/test_gpu_knn_cli.py; the CLI's refusal
of a malformed --sor before any device is touched.

The preconditions as the oracle's decode gave them when the stream was built (r: k: wrap_32_bits, exactly_r, one_outside, tie_at_k
over the grid's 729 points, duplicates_differ, found_below_k (some, none), tiles_and_buckets, corner_elsewhere):
  32767:  1: 2, 2, 2, 729, 5, (0, 13064), 0, 0      3: 2, 2, 2, 721, 5, (7, 13064), 0, 0
          8: 2, 2, 2, 729, 5, (7, 13064), 0, 0     16: 2, 2, 2, 721, 5, (32023, 13064), 0, 0
  64:     1: 0, 2430, 2, 729, 5, (0, 13065), 33, 1  3: 0, 2430, 2, 721, 5, (6, 13065), 33, 1
          8: 0, 2430, 2, 729, 5, (6, 13065), 33, 1 16: 0, 2430, 2, 721, 5, (32035, 13065), 33, 1
(the two ordered pairs of (a); (b)'s pair at exactly r and the one outside; at r = 64 the grid's pairs 64 apart)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import knn_cases as KC
from tests import neighbors_cases as NC
from tests import oracle
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_abi import declared

SYMBOLS = ("pcr_knn", "pcr_read_knn")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int32, C.POINTER(N.Box), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_int64), C.POINTER(N.NeighborsStats)]
    assert bound.pcr_knn.argtypes == args and bound.pcr_read_knn.argtypes == args
    for name in ("KNN_MAX_K", "KNN_MAX_RADIUS", "KNN_NONE", "knn_mean_distance", "knn_split", "statistical_outlier_mask"):
        assert hasattr(P, name)
    for name in ("knn", "read_knn"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.nearest_neighbors) and callable(P.HuffmanLasData.statistical_outliers)
    methods = open(os.path.join(build.CSRC, "pcr_methods.hpp")).read()
    assert "pcr_neighbors_stats nearestNeighbors(" in methods and "pcr_neighbors_stats statisticalOutliers(" in methods


def test_constants_match_the_header(tmp_path):
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "pcr_types.h"\nint main(void) {\n'
                   'printf("%d %d %llu\\n", PCR_KNN_MAX_K, PCR_KNN_MAX_RADIUS, (unsigned long long)PCR_KNN_NONE);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "consts")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "consts")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [16, 32767, (1 << 64) - 1] == [N.KNN_MAX_K, N.KNN_MAX_RADIUS, N.KNN_NONE] == [P.KNN_MAX_K, P.KNN_MAX_RADIUS, P.KNN_NONE]
    assert got == [KC.MAX_K, KC.MAX_RADIUS, int(KC.NONE)]
    # the word: the largest d2 and the largest row leave the top two bits clear, so no word is NONE and the unsigned order is (d2, row)
    assert KC.MAX_RADIUS ** 2 < 1 << 30 and int(KC.word(KC.MAX_RADIUS ** 2, (1 << 32) - 1)) < int(KC.NONE)
    assert int(KC.word(5, 0)) > int(KC.word(4, (1 << 32) - 1)) and int(KC.word(5, 7)) < int(KC.word(5, 8))


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
def cloud():
    """2590 rows: lattice sites 1 apart (ties at every place, and exact duplicates), a random blob, far points, and 400 copies of
    earlier rows."""
    rng = np.random.default_rng(11)
    sites = np.stack([rng.integers(0, 3, 1000), rng.integers(0, 40, 1000), rng.integers(0, 4, 1000)], axis=1)
    blob = rng.integers(-40, 41, (1100, 3)) + np.array([500, 0, 0])
    far = np.stack([np.arange(90) * 1000 + 5000, np.arange(90) * -777, np.full(90, 9)], axis=1)
    xyz = np.concatenate([sites, blob, far]).astype(np.int64)
    xyz = xyz[rng.permutation(len(xyz))]
    xyz = np.concatenate([xyz, xyz[5:405]])
    return xyz[rng.permutation(len(xyz))]


@pytest.mark.parametrize("clipped", [False, True], ids=["no_clip", "clip"])
@pytest.mark.parametrize("r", [1, 2, 7, 40, 32767])
def test_reference_against_every_pair(r, clipped):
    xyz = cloud()
    clip = ((0, -30, -40), (540, 39, 40)) if clipped else None
    plain = NC.analyse(xyz, r, clip)
    for k in (1, 2, 3, 8, 16):
        rows, want = KC.by_every_pair(xyz, k, r, clip)
        an = KC.analyse(xyz, k, r, clip)
        assert np.array_equal(an["rows"], rows) and an["knn"].dtype == np.uint64 and an["knn"].shape == (len(rows), k)
        bad = np.nonzero((an["knn"] != want).any(axis=1))[0]
        assert an["knn"].tobytes() == want.tobytes(), f"k {k} r {r}: lists differ at {bad[:4]}"
        assert np.array_equal(an["n"], plain["n"]) and np.array_equal(an["found"], np.minimum(k, plain["n"] - 1))
        if k == 1:                                              # the nearest one is pcr_neighbors' nn2
            nn2 = np.where(an["knn"][:, 0] == KC.NONE, NC.NONE, an["knn"][:, 0] >> np.uint64(32))
            assert np.array_equal(nn2, plain["nn2"])
        for key in ("voxels", "max_voxel_points", "pairs_bound"):
            assert an[key] == plain[key]
        krows, kd2 = KC.split(an["knn"])
        assert ((krows >= 0) == (kd2 >= 0)).all() and (kd2 <= r * r).all() and (krows != rows[:, None]).all()
        for min_found in (0, 1, k):
            at = KC.select(an, min_found)
            st = KC.stats(an, 77, 5, 3, min_found)
            assert list(st) == list(N.NeighborsStats().as_dict())
            assert st["points_written"] == len(at) == int((an["found"] >= min_found).sum()) and st["points_sparse"] == len(rows) - len(at)
            assert min_found > 0 or len(at) == len(rows)


def test_reference_of_an_empty_selection():
    an = KC.analyse(cloud(), 4, 5, S.EMPTY)
    assert len(an["rows"]) == 0 and an["knn"].shape == (0, 4) and an["pairs_bound"] == 0
    assert KC.stats(an, 0, 4, 0, 2) == dict(dict.fromkeys(N.NeighborsStats().as_dict(), 0), batches_outside=4)


# ---- knn_edges -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges_rows():
    of = oracle.OracleFile(KC.stream())
    assert of.num_batches == 1
    xyz = S.oracle_points(of, 0).astype(np.int64)
    xyz.setflags(write=False)
    return xyz


def test_the_stream_decodes_to_the_rows_given():
    xyz = edges_rows()
    assert xyz.shape == (KC.PPB, 3) and np.array_equal(xyz, KC.points()) and xyz.min() == 0
    plan = KC.edges_plan()
    far = (xyz == np.array(KC.FAR)).all(axis=1)
    assert far.sum() == KC.FAR_COPIES <= 20000 and KC.FAR_COPIES ** 2 < 4e8
    # every group is further than 3 r from every point outside it (except inside (a), which says otherwise)
    groups = {g: KC.rows_of(xyz, g) for g in plan}
    assert sum(len(v) for v in groups.values()) == sum(len(v) for v in plan.values())
    for g, rows in groups.items():
        others = np.ones(len(xyz), bool)
        others[rows] = False
        lo, hi = xyz[rows].min(axis=0), xyz[rows].max(axis=0)
        gap = np.maximum(np.maximum(lo - xyz[others], xyz[others] - hi), 0)
        assert (gap.max(axis=1) > 3 * KC.R_BIG).all(), g
    a, b = plan["wrap"]
    assert int(((a - b) ** 2).sum()) == 4294968473 == (1 << 32) + 1177 > KC.R_BIG ** 2 >= 1177 and ((a // KC.R_BIG) != (b // KC.R_BIG)).sum() == 1
    c, inside, outside = plan["radius_edge"]
    assert int(((c - inside) ** 2).sum()) == KC.R_BIG ** 2 and int(((c - outside) ** 2).sum()) == KC.R_BIG ** 2 + 1


@pytest.mark.parametrize("r,ks,needs", KC.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_cases_show_the_properties_claimed(r, ks, needs):
    xyz = edges_rows()
    assert NC.lattice_refusal([[*xyz.min(axis=0), *xyz.max(axis=0)]], r) is None
    for k in ks:
        got = KC.properties(xyz, k, r)
        print(f"knn_edges r {r} k {k}: {got}")
        for name in needs:
            if name == "found_below_k":
                assert got[name][1] >= 1 and (k == 1 or got[name][0] >= 1), f"{name}: no such candidate for k {k}"
            elif name == "tie_at_k":
                assert k == 1 or got[name] >= 1, f"no tie at place {k}"
            elif name == "corner_elsewhere":
                assert got[name] == 1
            else:
                assert got[name] >= 1, f"{name}: no such candidate in this case (k {k})"


def test_every_property_is_covered():
    assert set(KC.PROPERTIES) == {p for c in KC.CASES for p in c[2]}
    assert {c[0] for c in KC.CASES} == {KC.R_BIG, KC.R_SMALL} and all(c[1] == (1, 3, 8, 16) for c in KC.CASES)


def test_group_sizes():
    """(e): populations around the 64-entry tile (a voxel's points may be further than r apart); lone voxels of 1 and 2 points have
    found < k for every k >= 2."""
    xyz = edges_rows()
    an = KC.analyse(xyz, 16, KC.R_SMALL)
    for count in KC.LONE:
        rows = KC.rows_of(xyz, f"lone {count}")
        assert len(rows) == count and len(np.unique(xyz[rows] // KC.R_SMALL, axis=0)) == 1
        at = np.searchsorted(an["rows"], rows)
        assert (an["found"][at] == np.minimum(16, an["n"][at] - 1)).all() and (an["n"][at] <= count).all() and (count > 2 or (an["found"][at] < 2).all())
    v, cnt = np.unique(xyz[KC.rows_of(xyz, "crowd")] // KC.R_SMALL, axis=0, return_counts=True)
    assert sorted(cnt.tolist()) == [KC.CROWD_AROUND] * 7 + [KC.CROWD] and (v.max(axis=0) - v.min(axis=0) == 1).all()
    for copies in KC.DUPLICATES:
        rows = KC.rows_of(xyz, f"duplicates {copies}")
        at = np.searchsorted(an["rows"], rows)
        assert len(rows) == copies and (an["found"][at] == min(16, copies - 1)).all()
        krows, kd2 = KC.split(an["knn"][at])
        assert (kd2[krows >= 0] == 0).all() and np.isin(krows[krows >= 0], rows).all()


# ---- the references the GPU tests compute stay small ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(T.stream(name))
    return np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)]).astype(np.int64)


GPU_STREAMS = ("clustered", "synth", "wide30")


def gpu_radius(name):
    return min(min(NC.RADII[name]), KC.MAX_RADIUS)


def test_expansion_of_the_constructed_cases():
    xyz = edges_rows()
    for r in (KC.R_BIG, KC.R_SMALL):
        an = KC.analyse(xyz, 16, r)
        assert an["pairs"] < 3e7 and an["expanded"] < 3e7 and an["pairs_bound"] < 1e9, (r, an["pairs"], an["expanded"], an["pairs_bound"])


@pytest.mark.parametrize("name", GPU_STREAMS)
def test_expansion_of_the_stream_cases(name):
    """k = 8 without a clip is the largest reference tests/test_gpu_knn.py computes for the stream (a clip or a smaller k expands less)."""
    xyz = oracle_rows(name)
    clip = NC.WIDE30_LOW if name == "wide30" else None
    an = KC.analyse(xyz, 8, gpu_radius(name), clip)
    print(f"{name} r {gpu_radius(name)}: pairs {an['pairs']}, expanded {an['expanded']}, pairs_bound {an['pairs_bound']}")
    assert an["pairs"] < 3e7 and an["expanded"] < 3e7
    assert (an["found"] == np.minimum(8, an["n"] - 1)).all()


# ---- the mean distance and the outlier rule ---------------------------------------------------------------------------------------
def test_mean_distance_and_outlier_rule_by_hand():
    d2 = np.array([[9, 16, -1], [0, 0, 100], [-1, -1, -1], [25, -1, -1], [4, 4, 4]], np.int64)
    mean = P.knn_mean_distance(d2, 0.5)
    assert mean.dtype == np.float64 and mean.tolist() == [1.75, (0.0 + 0.0 + 5.0) / 3, float("inf"), 2.5, 1.0]
    assert P.knn_mean_distance(d2).tolist() == [3.5, 10.0 / 3, float("inf"), 5.0, 2.0]
    assert P.knn_mean_distance(np.zeros((0, 4), np.int64)).shape == (0,)
    # in entry order: ((sqrt(2) + sqrt(3)) + sqrt(5)) / 3, every operation rounded once
    one = P.knn_mean_distance(np.array([[2, 3, 5]]), 0.001)
    assert one[0] == ((np.sqrt(2.0) * 0.001 + np.sqrt(3.0) * 0.001) + np.sqrt(5.0) * 0.001) / 3
    means = np.array([1.0, 1.0, 1.0, 1.0, 5.0, np.inf])
    mu, sigma = 9.0 / 5, np.sqrt(((np.array([1.0, 1.0, 1.0, 1.0, 5.0]) - 9.0 / 5) ** 2).mean())      # the population sigma of the finite means: 1.6
    assert abs(sigma - 1.6) < 1e-12
    assert P.statistical_outlier_mask(means, 1.0).tolist() == [False, False, False, False, True, True]      # 5 > 1.8 + 1.6
    assert P.statistical_outlier_mask(means, 2.001).tolist() == [False, False, False, False, False, True]   # 5 <= 1.8 + 3.2016
    assert P.statistical_outlier_mask(means, 1.999).tolist() == [False, False, False, False, True, True]    # 5 > 1.8 + 3.1984
    assert P.statistical_outlier_mask(np.array([np.inf, np.inf]), 1.0).tolist() == [True, True]
    assert P.statistical_outlier_mask(np.array([2.0, 2.0, 2.0]), 0.0).tolist() == [False, False, False]     # the limit itself is no outlier
    rows, sq = P.knn_split(np.array([[KC.word(25, 7), KC.NONE]], np.uint64))
    assert rows.tolist() == [[7, -1]] and sq.tolist() == [[25, -1]] and rows.dtype == sq.dtype == np.int64


def test_the_filter_scene_has_exactly_the_five_strays_as_outliers():
    """tests/test_gpu_knn_cli.py's scene from the numpy reference: k = 8, multiplier 2, a radius that reaches the strays' nearest grid
    points; over the oracle's decode of the stream with the clip of the calls."""
    of = oracle.OracleFile(KC.sor_stream())
    xyz = S.oracle_points(of, 0).astype(np.int64)
    assert np.array_equal(xyz, KC.sor_rows())
    an = KC.analyse(xyz, KC.SOR_K, KC.SOR_R, KC.SOR_BOX)
    assert len(an["rows"]) == KC.SOR_SIDE ** 2 + 5 and an["pairs"] < 3e7 and an["expanded"] < 3e7 and an["pairs_bound"] < 1e9
    assert (an["found"] == KC.SOR_K).all()
    mean = P.knn_mean_distance(KC.split(an["knn"])[1], 0.001)
    out = P.statistical_outlier_mask(mean, KC.SOR_MULT)
    strays = xyz[an["rows"]][:, 2] != 1000
    assert strays.sum() == 5 and np.array_equal(out, strays)
    assert mean[strays].min() > 0.3 and mean[~strays].max() < 0.02
    # a radius that does not reach the grid from a stray: no neighbour, an infinite mean, an outlier all the same (mu and sigma are then
    # the grid's alone, so its rim turns up as well)
    short = KC.analyse(xyz, KC.SOR_K, KC.SOR_OFF - 1, KC.SOR_BOX)
    mean = P.knn_mean_distance(KC.split(short["knn"])[1], 0.001)
    assert np.isinf(mean[strays]).all() and P.statistical_outlier_mask(mean, KC.SOR_MULT)[strays].all()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--sor"], ["--sor", "8"], ["--sor", "8", "2"], ["--sor", "0", "2", "1"], ["--sor", "17", "2", "1"], ["--sor", "x", "2", "1"],
                                  ["--sor", "8", "-1", "1"], ["--sor", "8", "nan", "1"], ["--sor", "8", "2", "0"], ["--sor", "8", "2", "-3"],
                                  ["--sor", "8", "2", "1", "--outlier"], ["--sor", "8", "2", "1", "--outliers", "--outliers"], ["--sor", "8", "2", "1", "4"],
                                  ["--sor", "8", "2", "1", "--box", "0", "0", "0", "1", "1"], ["--sor", "8", "2", "1", "--sparse"], ["--sor", "2.5", "2", "1"]])
def test_cli_refuses_a_malformed_sor_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--sor K MULT R" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
