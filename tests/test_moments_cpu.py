"""Local moments, the parts that need no GPU: the entry points and the two records in the headers, the binding tables and the
cross-compiled library; covariance_from_moments and geometric_features; the numpy reference of tests/moments_cases.py against the
definition evaluated over every pair; the closed form of `ball`; the Jacobi restatement on the exact cases; the CLI's refusal of
a malformed --normals before any device is touched; and the preconditions of tests/test_gpu_moments.py, from the oracle's decoder.

The preconditions, as the oracle's decode gave them when the cases were chosen:
  facets, r = 50 (65 536 rows, 30 504 distinct points; the 35 033 rows at the anchor (19000, 19000, 19000) are the last point given
  and the encoder's padding copies of it: n = 35 033 each, s = q = 0, the zero matrix with n > 1):
    horizontal  10000 rows, 8100 interior (n = 81, C diagonal) and 1900 at the edge; C_xz = C_yz = C_zz = 0 and both other
                eigenvalues > 0 on all of them
    wall        10000 rows, 8100 interior and 1900 at the edge; C_xx = C_xy = C_xz = 0 and both other eigenvalues > 0 on all
    oblique     10000 rows, line 500 rows, single 1 row with n = 1, pair 2 rows with n = 2
    Exactly one row has n = 1. The two rows of the isolated pair are the only ones with n = 2: a symmetric relation gives the
    pair's two rows the same count, so "one row with n = 2" stands for this one pair.
    numpy.linalg.eigh leaves 4.5 * 2^-52 on these matrices, the numpy restatement of the Jacobi rules 2.0 * 2^-52.
  ball, r = 32767: 65 536 distinct rows in one voxel, every n = 65 536, the largest |q| component 7.13e12 >= 2^40 (and so >= 2^32),
    pairs_bound = 65536^2.
  plateau, r = 100, no clip: 123 rows have a neighbour in the other batch (their sphere crosses the batch border), 18 ordered
    pairs of distinct points lie at exactly d2 == r * r."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import moments_cases as MC
from tests import neighbors_cases as NC
from tests import oracle
from tests import select_cases as S
from tests.test_abi import declared

SYMBOLS = ("pcr_local_moments", "pcr_read_local_moments", "pcr_moments_eigen")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(N.Box), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_int64), C.POINTER(N.NeighborsStats)]
    assert bound.pcr_local_moments.argtypes == args and bound.pcr_read_local_moments.argtypes == args
    assert bound.pcr_moments_eigen.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    for name in ("Moments", "Eigen", "MOMENTS_MAX_RADIUS", "MOMENTS_DTYPE", "EIGEN_DTYPE", "covariance_from_moments", "geometric_features"):
        assert hasattr(P, name)
    for name in ("local_moments", "read_local_moments", "moments_eigen"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.normals)
    assert "pcr_neighbors_stats normals(" in open(os.path.join(build.CSRC, "pcr_methods.hpp")).read()
    kernels = open(os.path.join(build.CSRC, "pcr_kernels.hip.h")).read()
    for name in ("k_moments_pairs", "k_moments_eigen", "k_moments_write"):
        assert name + "(" in kernels


def test_records_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the radius limit as a C compiler sees include/pcr_types.h, against the ctypes and numpy mirrors."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu ", sizeof(pcr_moments), offsetof(pcr_moments, n), offsetof(pcr_moments, s), offsetof(pcr_moments, q));\n'
                   'printf("%zu %zu %zu %d\\n", sizeof(pcr_eigen), offsetof(pcr_eigen, value), offsetof(pcr_eigen, normal), PCR_MOMENTS_MAX_RADIUS);\n'
                   'return 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [80, 0, 8, 32, 48, 0, 24, 32767]
    assert [C.sizeof(N.Moments), N.Moments.n.offset, N.Moments.s.offset, N.Moments.q.offset] == got[:4]
    assert [C.sizeof(N.Eigen), N.Eigen.value.offset, N.Eigen.normal.offset] == got[4:7]
    assert [P.MOMENTS_DTYPE.itemsize] + [P.MOMENTS_DTYPE.fields[k][1] for k in ("n", "s", "q")] == got[:4]
    assert [P.EIGEN_DTYPE.itemsize] + [P.EIGEN_DTYPE.fields[k][1] for k in ("value", "normal")] == got[4:7]
    assert P.MOMENTS_MAX_RADIUS == MC.MAX_RADIUS == got[7]
    # the reason for the limit: 2^32 rows of products below 2^30 stay below 2^62
    assert MC.MAX_RADIUS ** 2 < 1 << 30 and (1 << 32) * MC.MAX_RADIUS ** 2 < 1 << 62 and (MC.MAX_RADIUS + 1) ** 2 == 1 << 30


def test_covariance_and_features():
    m = np.zeros(3, P.MOMENTS_DTYPE)
    m["n"] = [4, 0, -2]
    m["s"][0], m["q"][0] = (2, 0, -4), (4, 1, 0, 8, 0, 12)
    m["s"][1], m["q"][1] = (1, 1, 1), (1, 1, 1, 1, 1, 1)
    cov = P.covariance_from_moments(m)
    assert cov.shape == (3, 3, 3) and cov.dtype == np.float64 and (cov[1:] == 0).all()
    assert np.array_equal(cov[0], [[4 / 4 - 0.25, 0.25, 0.5], [0.25, 2.0, 0.0], [0.5, 0.0, 3.0 - 1.0]])
    assert np.array_equal(P.covariance_from_moments(m.view("<i8").reshape(-1, 10)), cov)
    f = P.geometric_features(np.array([[1.0, 2.0, 5.0], [0.0, 0.0, 0.0], [0.0, 3.0, 3.0]]))
    assert np.array_equal(f["curvature"], [1 / 8, 0, 0]) and np.array_equal(f["linearity"], [3 / 5, 0, 0])
    assert np.array_equal(f["planarity"], [1 / 5, 0, 1]) and np.array_equal(f["scattering"], [1 / 5, 0, 0])


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(MC.stream(name))
    return np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)]).astype(np.int64), S.oracle_bounds(of)


def every_pair(xyz, r):
    """n, s, q and the sum of d2 of every row over every pair of `xyz` (at most 3000 rows): the definition, in int64."""
    assert len(xyz) <= 3000
    d = xyz[None, :, :] - xyz[:, None, :]                       # [centre, neighbour]: neighbour minus centre
    d2 = (d * d).sum(axis=2)
    inside = d2 <= r * r
    q = np.stack([(d[:, :, a] * d[:, :, b] * inside).sum(axis=1) for a, b in MC.PRODUCTS], axis=1)
    return inside.sum(axis=1), (d * inside[:, :, None]).sum(axis=1), q, (d2 * inside).sum(axis=1)


@pytest.mark.parametrize("name,r,start", [("synth", 2500, 70000), ("clustered", 400, 0), ("plateau", 100, 65000)])
def test_reference_against_every_pair(name, r, start):
    """2000 consecutive rows of three streams (Morton order keeps them close; plateau's straddle its batch border)."""
    xyz = oracle_rows(name)[0][start:start + 2000]
    n, s, q, sum_d2 = every_pair(xyz, r)
    an = MC.analyse(xyz, r)
    assert np.array_equal(an["rows"], np.arange(2000))
    assert np.array_equal(an["n"], n) and np.array_equal(an["s"], s) and np.array_equal(an["q"], q)
    assert an["s"].dtype == an["q"].dtype == np.int64 and (n > 1).sum() > 100 and (s != 0).any() and (q[:, 1] != 0).any()
    assert np.array_equal(q[:, 0] + q[:, 3] + q[:, 5], sum_d2)
    plain = NC.analyse(xyz, r)
    for k in ("rows", "n", "nn2", "n27"):
        assert np.array_equal(an[k], plain[k])
    assert all(an[k] == plain[k] for k in ("voxels", "max_voxel_points", "pairs_bound", "pairs"))
    clip = (tuple(int(v) for v in np.percentile(xyz, 20, axis=0)), tuple(int(v) for v in np.percentile(xyz, 80, axis=0)))
    inside = S.in_box(xyz, clip)
    n, s, q, _ = every_pair(xyz[inside], r)
    an = MC.analyse(xyz, r, clip)
    assert np.array_equal(an["rows"], np.nonzero(inside)[0]) and 0 < len(an["rows"]) < 2000
    assert np.array_equal(an["n"], n) and np.array_equal(an["s"], s) and np.array_equal(an["q"], q)
    rec = MC.records(an, MC.written(an, 2))
    assert rec.dtype == P.MOMENTS_DTYPE and np.array_equal(rec["n"], n[n >= 2]) and np.array_equal(rec["q"], q[n >= 2])


def test_reference_of_an_empty_selection():
    an = MC.analyse(oracle_rows("plateau")[0][:500], 5, S.EMPTY)
    assert len(an["rows"]) == 0 and an["s"].shape == (0, 3) and an["q"].shape == (0, 6) and len(MC.records(an)) == 0


def test_closed_form_of_ball():
    xyz, _ = oracle_rows("ball")
    assert len(np.unique(xyz, axis=0)) == MC.PPB == len(xyz) and xyz.min() >= 0 and xyz.max() < 18000
    assert 3 * 17999 ** 2 <= MC.BALL_R ** 2 and (xyz // MC.BALL_R == 0).all()         # the diagonal is below r; one voxel
    assert sorted(map(tuple, xyz)) == sorted(map(tuple, MC.ball_points()))
    sub = xyz[:3000]
    an = MC.analyse(sub, MC.BALL_R)
    assert (an["n"] == 3000).all() and an["voxels"] == 1 and an["pairs_bound"] == 3000 ** 2
    assert MC.records(an).tobytes() == MC.closed_form(sub).tobytes()
    n, s, q, _ = every_pair(sub, MC.BALL_R)
    assert np.array_equal(an["s"], s) and np.array_equal(an["q"], q)
    full = MC.closed_form(xyz)
    print(f"ball: the largest |q| component {np.abs(full['q']).max():.3g}")
    assert np.abs(full["q"]).max() >= 1 << 40 and (full["n"] == MC.PPB).all() and np.abs(full["q"]).max() < 1 << 62


def test_a_sphere_crosses_a_batch_border_and_a_pair_lies_at_exactly_r():
    xyz, bounds = oracle_rows("plateau")
    r = 100
    assert r in MC.RADII["plateau"] and MC.lattice_refusal(bounds, r) is None
    exact = []
    an = MC.analyse(xyz, r, None, exact)
    assert an["pairs"] < 3e7
    crossing = 0
    for b in range(len(xyz) // MC.PPB):
        alone = NC.analyse(xyz[b * MC.PPB:(b + 1) * MC.PPB], r)
        crossing += int((alone["n"] < an["n"][b * MC.PPB:(b + 1) * MC.PPB]).sum())
    print(f"plateau r {r}: {crossing} rows with a neighbour in the other batch, {exact[0]} ordered pairs at exactly r")
    assert crossing >= 1 and exact[0] >= 1
    assert np.array_equal(an["n"], NC.analyse(xyz, r)["n"])
    assert np.array_equal(an["q"][:, 0] + an["q"][:, 3] + an["q"][:, 5] <= an["n"] * r * r, np.ones(len(an["n"]), bool))


# ---- facets ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def facets():
    xyz, bounds = oracle_rows("facets")
    assert MC.lattice_refusal(bounds, MC.FACETS_R) is None
    an = MC.analyse(xyz, MC.FACETS_R)
    assert np.array_equal(an["rows"], np.arange(MC.PPB))
    return xyz, an, MC.facets_classes(xyz)


def test_facets_preconditions():
    xyz, an, cls = facets()
    rec = MC.records(an)
    cov = P.covariance_from_moments(rec)
    distinct, copies = np.unique(xyz, axis=0, return_counts=True)
    assert sorted(map(tuple, distinct)) == sorted(map(tuple, MC.facets_points()))
    padded = distinct[copies.argmax()]
    assert (copies > 1).sum() == 1, "only the last point is duplicated"
    print(f"facets: {len(distinct)} distinct points, {copies.max()} rows at {padded}; " + ", ".join(f"{k} {int(v.sum())}" for k, v in cls.items()))
    n = an["n"]
    for name, zero, other in (("horizontal", (2, 5, 8, 6, 7), (0, 1)), ("wall", (0, 1, 2, 3, 6), (1, 2))):
        m = cls[name]
        flat = cov[m].reshape(-1, 9)
        interior = n[m] == n[m].max()
        print(f"  {name}: {int(m.sum())} rows, {int(interior.sum())} interior with n = {int(n[m].max())}, {int((~interior).sum())} at the edge")
        assert m.sum() >= 1000 and interior.sum() >= 100 and (~interior).sum() >= 100
        assert (flat[:, zero] == 0).all(), "the flat axis does not decouple exactly"
        block = cov[m][:, other][:, :, other]
        assert (np.linalg.eigvalsh(block)[:, 0] > 0).all(), "an in-plane eigenvalue is not positive"
        diagonal = (flat[interior][:, (1, 2, 5)] == 0).all(axis=1)
        assert diagonal.all(), "an interior row's covariance is not diagonal"
    assert cls["oblique"].sum() >= 1000 and cls["line"].sum() >= 100
    assert (n == 1).sum() == 1 and cls["single"].sum() == 1 and n[cls["single"]][0] == 1
    assert cls["pair"].sum() == 2 and (n[cls["pair"]] == 2).all() and np.array_equal(n == 2, cls["pair"])
    pad = cls["padding"]
    assert np.array_equal(padded, MC.ANCHOR) and pad.sum() == copies.max() > 30000 and (n[pad] == pad.sum()).all()
    assert (rec["s"][pad] == 0).all() and (rec["q"][pad] == 0).all()       # the zero matrix with n > 1


def test_jacobi_restatement_gives_the_exact_facets_results():
    xyz, an, cls = facets()
    rec = MC.records(an)
    eig = MC.eigen_reference(rec)
    tol, numpy_worst, worst = MC.check_eigen(rec, eig, "(facets, numpy Jacobi)")
    print(f"facets: numpy.linalg.eigh leaves {numpy_worst:.1f} * 2^-52, the numpy Jacobi {worst:.1f} * 2^-52; tol {tol / MC.EPS:.1f} * 2^-52")
    cov = P.covariance_from_moments(rec)
    _, _, sweeps = MC.jacobi(cov)
    assert 1 <= sweeps <= 12
    up, east = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    h, w = eig[cls["horizontal"]], eig[cls["wall"]]
    assert h["value"][:, 0].tobytes() == np.zeros(len(h)).tobytes() and h["normal"].tobytes() == np.tile(up, len(h)).tobytes()
    assert w["value"][:, 0].tobytes() == np.zeros(len(w)).tobytes() and w["normal"].tobytes() == np.tile(east, len(w)).tobytes()
    assert (h["value"][:, 1] > 0).all() and (w["value"][:, 1] > 0).all()
    one = eig[cls["single"]]
    assert one["value"].tobytes() == np.zeros(3).tobytes() and one["normal"].tobytes() == east.tobytes()
    scale = np.abs(cov).reshape(-1, 9).max(axis=1)
    o = cls["oblique"]
    assert np.abs(eig["normal"][o] - np.ones(3) / np.sqrt(3.0)).max() <= tol and (eig["value"][o][:, 0] <= tol * scale[o]).all()
    line = cls["line"]
    assert (np.abs(eig["value"][line][:, :2]) <= tol * scale[line][:, None]).all() and (eig["value"][line][:, 2] > 0).all()
    pair = eig[cls["pair"]]
    assert (pair["value"][:, :2] == 0).all() and (pair["value"][:, 2] == 15.0 ** 2).all()
    f = P.geometric_features(eig["value"])
    assert (f["curvature"][cls["horizontal"]] == 0).all() and (f["planarity"][cls["horizontal"]] > 0).all()
    assert (f["linearity"][line] > 0.99).all() and (f["curvature"][cls["single"]] == 0).all()


def test_handmade_moments_through_the_restatement():
    m, names = MC.handmade()
    e = MC.eigen_reference(m)
    tol, numpy_worst, worst = MC.check_eigen(m, e, "(hand-made)")
    by = dict(zip(names, e))
    assert by["n = 0"].tobytes() == by["n = -1"].tobytes() == bytes(48)
    assert tuple(by["diagonal, tie of x and z below y"]["value"]) == (4.0, 4.0, 9.0) and tuple(by["diagonal, tie of x and z below y"]["normal"]) == (1.0, 0.0, 0.0)
    assert tuple(by["diagonal, tie of y and z below x"]["normal"]) == (0.0, 1.0, 0.0)
    assert tuple(by["diagonal, descending"]["value"]) == (1.0, 4.0, 9.0) and tuple(by["diagonal, descending"]["normal"]) == (0.0, 0.0, 1.0)
    assert tuple(by["k * identity"]["value"]) == (7.0, 7.0, 7.0) and tuple(by["k * identity"]["normal"]) == (1.0, 0.0, 0.0)
    assert tuple(by["the zero matrix"]["normal"]) == (1.0, 0.0, 0.0)


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--normals"], ["--normals", "x"], ["--normals", "0"], ["--normals", "-1"], ["--normals", "nan"],
                                  ["--normals", "1", "x"], ["--normals", "1", "-1"], ["--normals", "1", "2.5"], ["--normals", "1", "3", "4"],
                                  ["--normals", "1", "99999999999999999999"], ["--normals", "1", "3", "--sparse"],
                                  ["--normals", "1", "3", "--box", "0", "0", "0", "1", "1"],
                                  ["--normals", "1", "--box", "0", "0", "0", "1", "1", "1", "--box", "0", "0", "0", "1", "1", "1"]])
def test_cli_refuses_malformed_normals_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.ply"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--normals R [MINCOUNT]" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
