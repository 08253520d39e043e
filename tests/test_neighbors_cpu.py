"""Radius neighbourhoods, the parts that need no GPU: the two entry points and the struct in the headers, the binding tables and the
cross-compiled library; radius_from_world; the numpy reference of tests/neighbors_cases.py against the definition evaluated over
every pair; the CLI's refusal of a malformed --radius before any device is touched; and the preconditions of
tests/test_gpu_neighbors.py, from the oracle's decoder.

The preconditions, as the oracle's decode gave them when the cases were chosen, at min_count = the median of N
(stream radius clip: sparse / candidates, median, sphere_decides, other_batch_decides, exactly_r, nn2_zero, no_neighbour; pairs
of distinct points the reference expands):
  clustered 400 none:             156646 / 327680, 13, 125041, 656, 2, 27685, 17811;       23836344
  wide30 2 x in 0..2:             24291 / 65536, 6, 24289, 31261, 53430, 12742, 365;       1267132
  wide30 1 x in 0..2:             16806 / 65536, 2, 15760, 16340, 61000, 12742, 16806;     287372
  synth 2500 none:                5324 / 655360, 9, 5265, 11518, 0, 55409, 85;             20353323
  plateau 100 none:               48325 / 131072, 2, 40791, 69, 18, 0, 48325;              506350
  garbage_tail 1000 header box:   0 / 327630, 1, 0, 0, 0, 27704, 299876;                   542052
sphere_decides counts N < median <= N27; exactly_r counts ordered pairs of distinct points. garbage_tail's median is 1, at which
nothing is sparse: the GPU test takes max(median, 2) as min_count, which makes its 299876 points without a neighbour sparse. With
that, both classes are non-empty in every case, so no mode can pass by writing everything or nothing."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import neighbors_cases as NC
from tests import oracle
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_abi import declared

SYMBOLS = ("pcr_neighbors", "pcr_read_neighbors")
STATS = ["batches_outside", "batches_decoded", "points_considered", "runs", "voxels", "table_slots", "max_voxel_points", "pairs_bound", "points_sparse",
         "points_written"]


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(N.Box), C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_int64), C.POINTER(N.NeighborsStats)]
    assert bound.pcr_neighbors.argtypes == args and bound.pcr_read_neighbors.argtypes == args
    for name in ("NeighborsStats", "NEIGHBORS_ALL", "NEIGHBORS_KEEP", "NEIGHBORS_SPARSE", "NEIGHBORS_MAX_RADIUS", "NN2_NONE", "radius_from_world"):
        assert hasattr(P, name)
    for name in ("neighbors", "read_neighbors"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.radius_filtered) and callable(P.HuffmanLasData.point_spacing)
    methods = open(os.path.join(build.CSRC, "pcr_methods.hpp")).read()
    assert "pcr_neighbors_stats radiusFiltered(" in methods and "radiusFromWorld(" in methods


def test_struct_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirror."""
    stats = [f for f, _ in N.NeighborsStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\nprintf("%zu ", sizeof(pcr_neighbors_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_neighbors_stats, {f}));\n' for f in stats)
                   + 'printf("%d %d %d %d %llu\\n", PCR_NEIGHBORS_ALL, PCR_NEIGHBORS_KEEP, PCR_NEIGHBORS_SPARSE, PCR_NEIGHBORS_MAX_RADIUS, '
                     '(unsigned long long)PCR_NN2_NONE);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert stats == STATS
    assert got[0] == 80 == C.sizeof(N.NeighborsStats) and got[1:11] == [8 * k for k in range(10)] == [getattr(N.NeighborsStats, f).offset for f in stats]
    assert got[11:] == [N.NEIGHBORS_ALL, N.NEIGHBORS_KEEP, N.NEIGHBORS_SPARSE, N.NEIGHBORS_MAX_RADIUS, N.NN2_NONE]
    assert got[11:] == [NC.ALL, NC.KEEP, NC.SPARSE, NC.MAX_RADIUS, int(NC.NONE)] == [0, 1, 2, 1 << 20, (1 << 64) - 1]
    assert [P.NEIGHBORS_ALL, P.NEIGHBORS_KEEP, P.NEIGHBORS_SPARSE, P.NEIGHBORS_MAX_RADIUS, P.NN2_NONE] == got[11:]


def las(scale, offset=(0.0, 0.0, 0.0)):
    info = N.LasInfo()
    for k in range(3):
        info.scale[k], info.offset[k], info.min[k], info.max[k] = scale[k], offset[k], 0.0, 1.0
    return info


def test_radius_from_world():
    """The largest r with r * scale <= radius as float64 evaluates the product; differing scales and results outside 1 .. 2^20 are
    refused."""
    for scale in (0.001, 0.01, 0.1, 0.25, 1.0, 0.003):
        info = las((scale,) * 3, (5.0, -7.0, 100.0))
        for radius in (scale, 2.5 * scale, 0.3, 1.0, 2.5, 7 * scale, 1000 * scale, 0.1 + 0.2, scale * (1 << 20)):
            if radius / scale > (1 << 20) + 0.5 or radius < scale:
                continue
            r = P.radius_from_world(info, radius)
            assert isinstance(r, int) and 1 <= r <= 1 << 20
            assert r * scale <= radius and ((r + 1) * scale > radius or r == 1 << 20), (scale, radius, r)
    info = las((0.01,) * 3)
    assert P.radius_from_world(info, 0.01) == 1 and P.radius_from_world(info, 0.0199) == 1 and P.radius_from_world(info, 1.0) == 100
    assert P.radius_from_world(info, 0.01 * (1 << 20)) == 1 << 20
    for bad in (0.0099, 0.0, -1.0, float("nan"), float("inf"), 0.01 * ((1 << 20) + 1)):
        with pytest.raises(ValueError):
            P.radius_from_world(info, bad)
    for scales in ((0.01, 0.01, 0.001), (0.01, 0.02, 0.01), (0.5, 0.25, 0.25)):
        with pytest.raises(ValueError, match="differ"):
            P.radius_from_world(las(scales), 1.0)


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
def cloud():
    """2990 rows: a lattice like wide30's low cluster (sites 1 apart: many pairs at exactly distance 1 and 2, and exact duplicates),
    a random blob, copies of earlier rows, and points far from everything."""
    rng = np.random.default_rng(7)
    sites = np.stack([rng.integers(0, 3, 1200), rng.integers(0, 40, 1200), rng.integers(0, 4, 1200)], axis=1)
    blob = rng.integers(-40, 41, (1300, 3)) + np.array([500, 0, 0])
    far = np.stack([np.arange(90) * 1000 + 5000, np.arange(90) * -777, np.full(90, 9)], axis=1)
    xyz = np.concatenate([sites, blob, far]).astype(np.int64)
    xyz = xyz[rng.permutation(len(xyz))]
    xyz = np.concatenate([xyz, xyz[5:405]])                     # 400 exact duplicates, far ones among them
    return xyz[rng.permutation(len(xyz))]


@pytest.mark.parametrize("clipped", [False, True], ids=["no_clip", "clip"])
@pytest.mark.parametrize("r", [1, 2, 3, 7, 40, 1 << 20])
def test_reference_against_every_pair(r, clipped):
    xyz = cloud()
    assert len(xyz) <= 3000
    clip = ((0, -30, -40), (540, 39, 40)) if clipped else None
    m = NC.candidates(xyz, clip)
    rows = np.nonzero(m)[0]
    p = xyz[m]
    d = p[:, None, :] - p[None, :, :]
    d2 = (d * d).sum(axis=2)                                    # int64, exact
    inside = d2 <= r * r
    n = inside.sum(axis=1)
    other = inside & ~np.eye(len(p), dtype=bool)                # another row, the same point or not
    nn2 = np.where(other, d2, np.iinfo(np.int64).max).min(axis=1)
    want_nn2 = np.where(other.any(axis=1), nn2, -1).astype(np.int64).view(np.uint64)
    exact = []
    an = NC.analyse(xyz, r, clip, exact)
    assert np.array_equal(an["rows"], rows) and an["rows"].dtype == np.int64
    assert np.array_equal(an["n"], n) and an["n"].dtype == np.int64 and (an["n"] >= 1).all()
    assert np.array_equal(an["nn2"], want_nn2) and an["nn2"].dtype == np.uint64
    # the statistics: voxels of cell r, the fullest, and the candidates in the 27 voxels around each candidate's own
    v = np.floor_divide(p, r)
    same = (np.abs(v[:, None, :] - v[None, :, :]) <= 1).all(axis=2)
    assert np.array_equal(an["n27"], same.sum(axis=1)) and an["pairs_bound"] == int(same.sum())
    uv, cnt = np.unique(v, axis=0, return_counts=True)
    assert an["voxels"] == len(uv) and an["max_voxel_points"] == int(cnt.max())
    if r <= 3:
        assert exact[0] > 0 and (d2 == r * r).sum() > 0, "no pair at exactly the radius"
        assert (an["nn2"] == 0).sum() > 0 and (an["nn2"] == NC.NONE).sum() > 0 and (n > 3).sum() > 0
    # select(): the three modes at several thresholds
    for min_count in (0, 1, 2, NC.median_n(an), NC.HUGE):
        keep, sparse, everything = (NC.select(an, mode, min_count) for mode in (NC.KEEP, NC.SPARSE, NC.ALL))
        assert np.array_equal(keep, np.nonzero(n >= min_count)[0]) and np.array_equal(sparse, np.nonzero(n < min_count)[0])
        assert np.array_equal(everything, np.arange(len(n)))
        assert (min_count > 1 or len(sparse) == 0) and (min_count != NC.HUGE or len(keep) == 0)
        st = NC.stats(an, 77, 5, 3, NC.KEEP, min_count)
        assert list(st) == STATS and st["points_sparse"] == len(sparse) and st["points_written"] == len(keep) and st["table_slots"] == 1024


def test_reference_of_an_empty_selection():
    an = NC.analyse(cloud(), 5, S.EMPTY)
    assert len(an["rows"]) == 0 and len(an["n"]) == 0 and an["pairs_bound"] == 0
    assert NC.stats(an, 0, 4, 0, NC.ALL, 3) == dict(dict.fromkeys(STATS, 0), batches_outside=4)


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(T.stream(name))
    return np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)]).astype(np.int64), S.oracle_bounds(of)


@pytest.mark.parametrize("name,r,clip,needs", NC.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_cases_show_the_properties_claimed(name, r, clip, needs):
    xyz, bounds = oracle_rows(name)
    clip = NC.case_clip(name, clip, xyz)
    assert NC.lattice_refusal(bounds, r, clip) is None
    got = NC.properties(xyz, r, clip)
    print(f"{name} r {r} clip {clip}: {got}")
    assert got["pairs"] < 3e7, "the reference would be slow"
    if name == "garbage_tail":
        assert (~S.in_box(xyz, clip)).sum() >= 1, "no row of the tail artefact lies outside the header's box"
        assert got["median"] == 1 and 0 < got["no_neighbour"] < got["candidates"]          # min_count 2 splits it
    else:
        assert 0 < got["sparse"] < got["candidates"] and got["median"] >= 2, "a mode could pass by writing everything or nothing"
    for k in needs:
        assert got[k] >= 1, f"{k}: no such candidate in this case"


def test_every_property_is_covered():
    assert set(NC.PROPERTIES) == {k for c in NC.CASES for k in c[3]}
    assert {c[0] for c in NC.CASES} == {"synth", "plateau", "wide30", "clustered", "garbage_tail"}
    assert set(NC.RADII) == set(NC.STREAMS) and all(len(set(v)) == 2 for v in NC.RADII.values())


def test_lattice_limits_of_the_streams():
    """wide30 without a clip is refused; with the clip on its low cluster radius 1 is accepted. The limit is pcr_denoise's."""
    _, wide = oracle_rows("wide30")
    assert NC.lattice_refusal(wide, 1) == "voxels" and NC.lattice_refusal(wide, 1 << 20) == "extent"
    assert NC.lattice_refusal(wide, 1, NC.WIDE30_LOW) is None
    assert NC.lattice_refusal([[0, 0, 0, (1 << 21) - 4, 0, 0]], 1) is None and NC.lattice_refusal([[0, 0, 0, (1 << 21) - 3, 0, 0]], 1) == "voxels"
    assert NC.lattice_refusal([[0, 0, 0, 2 * ((1 << 21) - 3), 0, 0]], 2) == "voxels" and NC.lattice_refusal([[0, 0, 0, 2 * ((1 << 21) - 3) - 1, 0, 0]], 2) is None


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--radius"], ["--radius", "1"], ["--radius", "x", "3"], ["--radius", "0", "3"], ["--radius", "-1", "3"],
                                  ["--radius", "nan", "3"], ["--radius", "1", "x"], ["--radius", "1", "-1"], ["--radius", "1", "2.5"],
                                  ["--radius", "1", "99999999999999999999"], ["--radius", "1", "3", "--spars"],
                                  ["--radius", "1", "3", "--sparse", "--sparse"], ["--radius", "1", "3", "4"],
                                  ["--radius", "1", "3", "--box", "0", "0", "0", "1", "1"], ["--radius", "1", "3", "--isolated"],
                                  ["--radius", "1", "3", "--box", "0", "0", "0", "1", "1", "1", "--box", "0", "0", "0", "1", "1", "1"]])
def test_cli_refuses_a_malformed_radius_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--radius R MINCOUNT" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
