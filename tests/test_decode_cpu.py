"""The decode feature's parts that need no GPU: the LAS writer of libpcr_host (pcr_write_las) against the LAS reader, the 16-byte
point record, and the two decode entry points in the headers, the binding tables and the cross-compiled library."""
import ctypes as C
import os

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import scenes
from tests.test_abi import declared


def test_write_las_read_las_round_trip(tmp_path):
    n = 100_000
    x, y, z, c, las = scenes.random_points(n, seed=11)
    path = tmp_path / "out.las"
    P.write_las(path, x, y, z, c, las)
    assert os.path.getsize(path) == 227 + 26 * n                    # LAS 1.2 header, point format 2
    X, Y, Z, Cc, L = P.read_las(str(path))
    assert X.dtype == np.int32 and len(X) == n
    assert np.array_equal(X, x) and np.array_equal(Y, y) and np.array_equal(Z, z) and np.array_equal(Cc, c)
    for k in range(3):
        assert L.scale[k] == las.scale[k] and L.offset[k] == las.offset[k] and L.min[k] == las.min[k] and L.max[k] == las.max[k]
    # the strided twin writes the same bytes
    pts = np.empty(n, P.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"], pts["color"] = x, y, z, c
    P.write_las(tmp_path / "twin.las", points=pts, las=las)
    assert open(path, "rb").read() == open(tmp_path / "twin.las", "rb").read()


def test_write_las_single_point(tmp_path):
    x, y, z, c, las = scenes.random_points(1, seed=5)
    P.write_las(tmp_path / "one.las", x, y, z, c, las)
    X, Y, Z, Cc, _ = P.read_las(str(tmp_path / "one.las"))
    assert (X[0], Y[0], Z[0], Cc[0]) == (x[0], y[0], z[0], c[0]) and len(X) == 1


def test_write_las_refusals(tmp_path):
    x, y, z, c, las = scenes.random_points(4, seed=5)
    with pytest.raises(P.PcrError, match="no points"):
        P.write_las(tmp_path / "empty.las", x[:0], y[:0], z[:0], c[:0], las)
    assert not os.path.exists(tmp_path / "empty.las")
    with pytest.raises(P.PcrError, match="cannot open"):
        P.write_las(tmp_path / "no_such_dir" / "out.las", x, y, z, c, las)


def test_point_record_is_16_bytes():
    assert C.sizeof(N.Point) == 16 and P.POINT_DTYPE.itemsize == 16
    assert [(f, N.Point.__dict__[f].offset) for f, _ in N.Point._fields_] == [("x", 0), ("y", 4), ("z", 8), ("color", 12)]
    assert [P.POINT_DTYPE.fields[f][1] for f in ("x", "y", "z", "color")] == [0, 4, 8, 12]


def test_decode_entry_points_are_declared_bound_and_exported():
    for name in ("pcr_decode_points", "pcr_read_points"):
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    for name in ("pcr_write_las", "pcr_write_las_points"):
        assert name in declared("pcr_encode.h") and name in N.HOST_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    assert hasattr(lib, "pcr_decode_points") and hasattr(lib, "pcr_read_points")
    bound = N.hip_lib()
    assert bound.pcr_decode_points.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]
    assert bound.pcr_read_points.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]
