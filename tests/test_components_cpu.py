"""Connected components, the parts that need no GPU: the two entry points and the struct in the headers, the binding tables and
the cross-compiled library; the numpy reference of tests/components_cases.py against a plain breadth-first search (and against
scipy.ndimage.label where scipy is installed); the CLI's refusal of a malformed --components before any device is touched; and
the preconditions of tests/test_gpu_components.py, recomputed from the oracle's decoder.

The preconditions are in tests/components_cases.py's CASES, origin (0, 0, 0): voxels, components, the largest sizes and the
components with candidates in two or more batches are asserted exactly; `deep` is asserted as "32 plain neighbour-minimum sweeps
have not reached the fixed point" (the full counts, up to 1052 sweeps, are recorded in SWEEPS and not recomputed: the longest
takes ten seconds)."""
import collections
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import components_cases as K
from tests import oracle
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_abi import declared

SYMBOLS = ("pcr_components", "pcr_read_components")
STATS = ["batches_outside", "batches_decoded", "points_considered", "runs", "voxels", "components", "components_small", "points_small",
         "largest_points", "points_written", "table_slots"]


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Voxels), C.POINTER(N.Box), C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_size_t, C.POINTER(C.c_int64), C.POINTER(N.ComponentsStats)]
    assert bound.pcr_components.argtypes == args and bound.pcr_read_components.argtypes == args
    for name in ("ComponentsStats", "COMPONENTS_KEEP", "COMPONENTS_SMALL"):
        assert hasattr(P, name)
    for name in ("components", "read_components"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.components)


def test_struct_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirror."""
    stats = [f for f, _ in N.ComponentsStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\nprintf("%zu ", sizeof(pcr_components_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_components_stats, {f}));\n' for f in stats)
                   + 'printf("%d %d\\n", PCR_COMPONENTS_KEEP, PCR_COMPONENTS_SMALL);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert stats == STATS
    assert got[0] == 88 == C.sizeof(N.ComponentsStats) and got[1:12] == [8 * k for k in range(11)] == [getattr(N.ComponentsStats, f).offset for f in stats]
    assert got[12:] == [N.COMPONENTS_KEEP, N.COMPONENTS_SMALL] == [K.KEEP, K.SMALL] == [P.COMPONENTS_KEEP, P.COMPONENTS_SMALL] == [0, 1]


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
def by_search(xyz, vox, clip, connectivity):
    """row -> (label, size) by a breadth-first search over a dict of voxels."""
    voxel, members = {}, collections.defaultdict(list)
    for row, p in enumerate(xyz):
        p = [int(v) for v in p]
        if all(clip[0][k] <= p[k] <= clip[1][k] for k in range(3)):
            voxel[row] = tuple((p[k] - vox[k]) // vox[3] for k in range(3))
            members[voxel[row]].append(row)
    steps = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    seen, out = set(), {}
    for start in members:
        if start in seen:
            continue
        seen.add(start)
        queue, comp = collections.deque([start]), []
        while queue:
            v = queue.popleft()
            comp.append(v)
            for d in steps:
                w = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
                if w in members and w not in seen:
                    seen.add(w)
                    queue.append(w)
        rows = [r for v in comp for r in members[v]]
        for r in rows:
            out[r] = (min(rows), len(rows))
    return out


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("vox", [(0, 0, 0, 1), (-3, 5, 1, 4), (S.INT32_MAX, S.INT32_MIN, 0, 7), (2, 2, 2, 3)])
def test_reference_against_a_breadth_first_search(vox, connectivity):
    rng = np.random.default_rng((sum(vox) & 0xFFFF) + connectivity)
    xyz = rng.integers(-20, 21, (3000, 3))
    xyz[::7] = xyz[1::7][:len(xyz[::7])]                                    # exact duplicates
    clip = ((-15, -20, -18), (20, 12, 20))
    want = by_search(xyz, vox, clip, connectivity)
    an = K.analyse(xyz, vox, clip, connectivity)
    rows = sorted(want)
    assert an["rows"].tolist() == rows and len(rows) > 1000
    assert an["label"].tolist() == [want[r][0] for r in rows] and an["size"].tolist() == [want[r][1] for r in rows]
    comps = sorted(set(want.values()))
    assert an["clabel"].tolist() == [c[0] for c in comps] and an["csize"].tolist() == [c[1] for c in comps]
    assert set(an["clabel"].tolist()) <= set(rows), "a label is a row of its component"
    for min_points in (0, 1, 2, K.median_size(an), K.HUGE):
        small = [r for r in rows if want[r][1] < min_points]
        kept = [r for r in rows if want[r][1] >= min_points]
        got_small, got_kept = K.select(an, min_points, K.SMALL), K.select(an, min_points, K.KEEP)
        assert got_small[0].tolist() == small and got_kept[0].tolist() == kept and got_kept[0].dtype == got_kept[1].dtype == np.int64
        assert got_small[1].tolist() == [want[r][0] for r in small] and got_kept[1].tolist() == [want[r][0] for r in kept]
        assert K.stats(an, min_points) == dict(voxels=len({tuple((int(xyz[r][k]) - vox[k]) // vox[3] for k in range(3)) for r in rows}),
                                               components=len(comps), components_small=sum(c[1] < min_points for c in comps),
                                               points_small=len(small), largest_points=max(c[1] for c in comps))
        assert (min_points > 1 or not small) and (min_points != K.HUGE or not kept)
    if vox[3] == 1:
        assert len(comps) > 1 and 0 < len(K.select(an, K.median_size(an) + 1, K.SMALL)[0]) < len(rows)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_six_never_has_fewer_components_than_twenty_six(seed):
    xyz = np.random.default_rng(seed).integers(-30, 31, (4000, 3))
    a6, a26 = K.analyse(xyz, (0, 0, 0, 2), None, 6), K.analyse(xyz, (0, 0, 0, 2), None, 26)
    assert len(a6["clabel"]) >= len(a26["clabel"]) > 1 and a6["voxels"] == a26["voxels"]
    assert (a6["label"] >= a26["label"]).all() and (a6["size"] <= a26["size"]).all()        # 6's partition refines 26's
    assert len(a6["clabel"]) > len(a26["clabel"])


@pytest.mark.parametrize("connectivity", [6, 26])
def test_reference_against_scipy_label_on_dense_grids(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(connectivity)
    grid = rng.random((24, 20, 16)) < 0.22
    xyz = np.argwhere(grid)[:, ::-1].copy()                                  # (x, y, z) of the set cells, any order of rows will do
    rng.shuffle(xyz)
    lab, n = ndimage.label(grid, structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    an = K.analyse(xyz, (0, 0, 0, 1), None, connectivity)
    theirs = lab[xyz[:, 2], xyz[:, 1], xyz[:, 0]]
    assert len(an["clabel"]) == n
    assert len(set(zip(theirs.tolist(), an["label"].tolist()))) == n, "the two labellings are not the same partition"
    assert sorted(np.bincount(theirs)[1:].tolist()) == sorted(an["csize"].tolist())


def test_label_graph_on_a_long_path():
    """A path of 20 001 nodes numbered against its direction, and a second component: pointer jumping reaches the ends."""
    n = 20001
    u, v = np.arange(n - 1), np.arange(1, n)
    root = K.label_graph(n + 3, np.concatenate([u, [n, n + 1]]), np.concatenate([v, [n + 1, n + 2]]))
    assert (root[:n] == 0).all() and root[n:].tolist() == [n, n, n]
    assert K.label_graph(4, [], []).tolist() == [0, 1, 2, 3]


# ---- the preconditions of the GPU cases ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(T.stream(name))
    return np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)]).astype(np.int64), S.oracle_bounds(of)


@pytest.mark.parametrize("case", range(len(K.CASES)), ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in K.CASES])
def test_cases_show_the_properties_claimed(case):
    name, cell, conn, clip, min_points, figures, needs = K.CASES[case]
    xyz, bounds = oracle_rows(name)
    vox, clip = (0, 0, 0, cell), K.case_clip(name, clip, xyz)
    assert K.lattice_refusal(bounds, vox, clip) is None
    got = K.properties(xyz, vox, min_points, clip, conn)
    print(f"{name} cell {cell} conn {conn} min_points {min_points} clip {clip}: {got}")
    voxels, components, largest, multi_batch = figures
    assert (got["voxels"], got["components"], got["multi_batch"]) == (voxels, components, multi_batch)
    assert got["largest"][:len(largest)] == largest
    claimed = dict(both_classes=got["kept"] > 0 and got["small"] > 0, multi_batch=got["multi_batch"] >= 1, deep=got["sweeps"] >= 32,
                   conn_differs=got["conn_differs"], many=got["components"] >= 1000)
    for k in needs:
        assert claimed[k], f"{k}: not shown by this case"
    assert claimed["deep"] == (K.SWEEPS[case] >= 32) == ("deep" in needs)
    if K.SWEEPS[case] < 32:
        assert got["sweeps"] == K.SWEEPS[case]
    if name == "garbage_tail":
        assert (~S.in_box(xyz, clip)).sum() >= 1, "no row of the tail artefact lies outside the header's box"


def test_every_property_is_covered():
    assert set(K.PROPERTIES) == {k for c in K.CASES for k in c[6]}
    assert {c[0] for c in K.CASES} == {"synth", "plateau", "wide30", "clustered", "garbage_tail", "escape_heavy"}
    assert {c[2] for c in K.CASES} == {6, 26} and len(K.SWEEPS) == len(K.CASES)
    assert len(K.forward_offsets(6)) == 3 and len(K.forward_offsets(26)) == 13
    both = K.forward_offsets(26) + [-o for o in K.forward_offsets(26)]
    assert len(set(both)) == 26 and 0 not in both


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--components"], ["--components", "1"], ["--components", "x", "3"], ["--components", "0", "3"],
                                  ["--components", "-1", "3"], ["--components", "nan", "3"], ["--components", "1", "x"], ["--components", "1", "-1"],
                                  ["--components", "1", "2.5"], ["--components", "1", "99999999999999999999"], ["--components", "1", "3", "--smal"],
                                  ["--components", "1", "3", "--small", "--small"], ["--components", "1", "3", "4"],
                                  ["--components", "1", "3", "--conn"], ["--components", "1", "3", "--conn", "18"],
                                  ["--components", "1", "3", "--conn", "0"], ["--components", "1", "3", "--conn", "6", "--conn", "26"],
                                  ["--components", "1", "3", "--box", "0", "0", "0", "1", "1"], ["--components", "1", "3", "--isolated"],
                                  ["--components", "1", "3", "--box", "0", "0", "0", "1", "1", "1", "--box", "0", "0", "0", "1", "1", "1"]])
def test_cli_refuses_a_malformed_components_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--components CELL MINPOINTS" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
