"""Box selection, the parts that need no GPU: the three entry points and two structs in the headers, the binding tables and the
cross-compiled library; box_from_world against the float64 predicate it promises; the CLI's refusal of a malformed --box before
any device is touched; and the preconditions of tests/test_gpu_select.py, from the oracle's decoder: the boxes of
tests/select_cases.py make every class of batch occur, a straddling batch holds a chain with none and a chain with all 64
of its points selected, and the garbage-tail stream has a batch whose exact box outgrows its record's float box."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import oracle
from tests import select_cases as S
from tests.test_abi import declared

SYMBOLS = ("pcr_batch_point_bounds", "pcr_select_box", "pcr_read_box")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    assert bound.pcr_batch_point_bounds.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    sel = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Box), C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(N.SelectStats)]
    assert bound.pcr_select_box.argtypes == sel and bound.pcr_read_box.argtypes == sel


def test_structs_match_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/pcr_types.h, against the ctypes mirrors."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pcr_box), offsetof(pcr_box, min), offsetof(pcr_box, max),\n'
                   'sizeof(pcr_select_stats), offsetof(pcr_select_stats, batches_outside), offsetof(pcr_select_stats, batches_inside),\n'
                   'offsetof(pcr_select_stats, batches_straddling), offsetof(pcr_select_stats, points_selected)); return 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [24, 0, 12, 32, 0, 8, 16, 24]
    assert [C.sizeof(N.Box), N.Box.min.offset, N.Box.max.offset] == got[:3]
    assert [C.sizeof(N.SelectStats)] + [getattr(N.SelectStats, f).offset for f, _ in N.SelectStats._fields_] == got[3:]
    assert [f for f, _ in N.SelectStats._fields_] == ["batches_outside", "batches_inside", "batches_straddling", "points_selected"]


# ---- box_from_world ----------------------------------------------------------------------------------------------------------
def world(i, scale, offset):
    """HuffmanLasData.points(world=True): float64(i) * scale + offset, two roundings."""
    return np.asarray(i, np.int64).astype(np.float64) * np.float64(scale) + np.float64(offset)


def test_box_from_world_is_the_float64_predicate():
    rng = np.random.default_rng(5)
    near = np.arange(-2, 3)
    for trial in range(400):
        las = P.LasInfo()
        lo, hi = [], []
        for k in range(3):
            las.scale[k] = float(rng.choice([0.001, 0.01, 0.0001, 0.00025, 1.0, 0.1, 10 ** rng.uniform(-5, 1)]))
            las.offset[k] = float(rng.choice([0.0, 100.0, -2.5e6, 4.5e5 + 0.123, rng.uniform(-1e7, 1e7)]))
            i0, i1 = sorted(int(v) for v in rng.integers(-(1 << 30), 1 << 30, 2))
            # bounds that sit exactly on lattice values, a hair beside them, and anywhere
            jitter = rng.choice([0.0, 1e-9, -1e-9, rng.uniform(-1, 1) * las.scale[k]])
            lo.append(float(world(i0, las.scale[k], las.offset[k])) + jitter)
            hi.append(float(world(i1, las.scale[k], las.offset[k])) - jitter)
        box = P.box_from_world(las, lo, hi)
        for k in range(3):
            a, z = int(box.min[k]), int(box.max[k])
            if a > z:                                   # empty on this axis: nothing near the guesses satisfies the predicate
                g = int(round((lo[k] - las.offset[k]) / las.scale[k]))
                w = world(g + np.arange(-3, 4), las.scale[k], las.offset[k])
                assert not ((w >= lo[k]) & (w <= hi[k])).any()
                continue
            for bound in (a, z):
                i = bound + near
                i = i[(i >= S.INT32_MIN) & (i <= S.INT32_MAX)]
                w = world(i, las.scale[k], las.offset[k])
                want = (w >= lo[k]) & (w <= hi[k])
                got = (i >= a) & (i <= z)
                assert np.array_equal(got, want), (trial, k, las.scale[k], las.offset[k], lo[k], hi[k], a, z)


def test_box_from_world_edges():
    las = P.LasInfo()
    for k in range(3):
        las.scale[k] = 0.001; las.offset[k] = 0.0
    inf = float("inf")
    b = P.box_from_world(las, (-inf,) * 3, (inf,) * 3)
    assert list(b.min) == [S.INT32_MIN] * 3 and list(b.max) == [S.INT32_MAX] * 3
    b = P.box_from_world(las, (0.0, 0.0, 5.0), (1.0, 1.0, 4.0))
    assert b.min[2] > b.max[2] and (b.min[0], b.max[0]) == (0, 1000)
    b = P.box_from_world(las, (0.0, 0.0, 1e9), (1.0, 1.0, 2e9))            # beyond every int32 coordinate
    assert b.min[2] > b.max[2]
    las.scale[1] = 0.0
    with pytest.raises(ValueError):
        P.box_from_world(las, (0, 0, 0), (1, 1, 1))
    assert list(P.as_box(((1, 2, 3), (4, 5, 6))).max) == [4, 5, 6] and list(P.as_box([1, 2, 3, 4, 5, 6]).min) == [1, 2, 3]
    with pytest.raises(ValueError):
        P.as_box(((0, 0, 0), (1 << 31, 0, 0)))


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--box"], ["--box", "0", "0", "0", "1", "1"], ["--box", "0", "0", "0", "1", "1", "x"],
                                  ["--box", "0", "0", "0", "1", "1", "1", "2"], ["--bax", "0", "0", "0", "1", "1", "1"],
                                  ["--box", "0", "0", "0", "1", "1", "nan"], ["--box", "0", "0", "0", "1", "1", "1e999"]])
def test_cli_refuses_a_malformed_box_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    # (the input does not exist and HIP sees no device: either would be the message if the tool got that far)
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--box x0 y0 z0 x1 y1 z1" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()


# ---- preconditions of the GPU cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batches", [("synth", 10), ("clustered", 5)])
def test_preconditioned_boxes_make_every_class_occur(name, batches):
    of = oracle.OracleFile(S.stream(name))
    assert of.num_batches == batches
    box = S.BOXES[name]
    cls = S.classify(S.oracle_bounds(of), box)
    for k in (S.OUTSIDE, S.INSIDE, S.STRADDLING):
        assert (cls == k).any(), (name, cls)
    none = full = some = False
    for b in np.nonzero(cls == S.STRADDLING)[0]:
        per_chain = S.in_box(S.oracle_points(of, int(b)), box).reshape(1024, 64).sum(axis=1)
        none, full = none or (per_chain == 0).any(), full or (per_chain == 64).any()
        some = some or ((per_chain > 0) & (per_chain < 64)).any()
    assert none and full and some, "a straddling batch needs a chain with 0, a chain with 64 and a chain with some of its points selected"
    # inside means inside, outside means outside, point by point
    for b in range(batches):
        m = S.in_box(S.oracle_points(of, b), box)
        assert m.all() if cls[b] == S.INSIDE else not m.any() if cls[b] == S.OUTSIDE else True


def test_special_boxes_classify_as_the_gpu_cases_expect():
    of = oracle.OracleFile(S.stream("synth"))
    bounds = S.oracle_bounds(of)
    assert (S.classify(bounds, S.FULL) == S.INSIDE).all()
    assert (S.classify(bounds, S.NOTHING) == S.OUTSIDE).all() and (S.classify(bounds, S.EMPTY) == S.OUTSIDE).all()


def test_garbage_tail_stream_outgrows_its_float_boxes():
    of = oracle.OracleFile(S.stream("garbage_tail"))
    bounds = S.oracle_bounds(of)
    larger = 0
    for b in range(of.num_batches):
        lo, hi = S.float_box_as_integers(of.batch(b))
        larger += bool((bounds[b, :3] < lo).any() or (bounds[b, 3:] > hi).any())
    assert larger >= 1, "no batch's exact box is larger than its record's float box: the tail artefact was not exercised"
