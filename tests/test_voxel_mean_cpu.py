"""Voxel means, the parts that need no GPU: the two entry points and the constant in the headers, the binding tables and the
cross-compiled library; voxel_mean_round of csrc/pcr_lattice.h compiled into a stand-alone program under the sanitizers and held
against Python integers at the limits of its 64-bit fields (no small stream reaches them); the numpy reference of
tests/voxel_mean_cases.py against a plain loop; the CLI's refusal of --mean with --center before any device is touched; and the
preconditions of tests/test_gpu_voxel_mean.py, counted on the oracle's decode (positions and colours).

Counts over the generators' integer points, as stated when the cases were chosen (stream and clip, cell: non-empty voxels,
multi-point voxels, largest n, position-tie voxels, voxels whose mean is no member):
  wide30 inside WIDE30_LOW, 1:   58 942,  6148,  5,      0,    0     (only colours are averaged)
  wide30 inside WIDE30_LOW, 2:   35 206, 18 539, 10, 10 408, 3139
  wide30 inside WIDE30_LOW, 7:     2281,  2268, 52,    125, 1754
  plateau, 64:                  122 746,  7983,  4,   6710, 7979
  plateau, 1000:                   4096,  4096, 56,    237, 4096
test_preconditions_on_the_oracles_decode prints what the oracle's decode gives and holds wide30's against these (plateau's
decode carries the tail artefact's rows as well: see PRECONDITIONS)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import oracle
from tests import select_cases as S
from tests import thin_cases as T
from tests import voxel_mean_cases as V
from tests.test_abi import declared

SYMBOLS = ("pcr_voxel_mean", "pcr_read_voxel_mean")
PPB = S.PPB


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Voxels), C.POINTER(N.Box), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64),
            C.POINTER(N.ThinStats)]
    assert bound.pcr_voxel_mean.argtypes == args and bound.pcr_read_voxel_mean.argtypes == args
    for name in ("voxel_mean", "read_voxel_mean"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.voxel_centroids)


def test_constant_and_statistics_match_the_header(tmp_path):
    """PCR_VOXEL_MEAN_MAX_ROWS and the statistics struct as a C compiler sees include/pcr_types.h, against the Python mirrors."""
    stats = [f for f, _ in N.ThinStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\n'
                   'printf("%lld %zu %zu ", (long long)PCR_VOXEL_MEAN_MAX_ROWS, sizeof(PCR_VOXEL_MEAN_MAX_ROWS), sizeof(pcr_thin_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_thin_stats, {f}));\n' for f in stats) + 'printf("%d\\n", PCR_THIN_MAX_CELL);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:3] == [1 << 32, 8, 48] and got[3:9] == [getattr(N.ThinStats, f).offset for f in stats]
    assert N.VOXEL_MEAN_MAX_ROWS == P.VOXEL_MEAN_MAX_ROWS == V.MAX_ROWS == got[0]
    # the argument of the limit: offsets below the largest cell, at most MAX_ROWS of them, bytes below 256
    assert (got[9] - 1) * got[0] < 1 << 62 and 255 * got[0] < 1 << 40 and 2 * (got[9] - 1) * got[0] + got[0] < 1 << 64
    assert got[0] // PPB == 65536


# ---- voxel_mean_round (csrc/pcr_lattice.h) in a program of its own -----------------------------------------------------------------
def round_cases():
    top = (1 << 62) - 1
    cases = [(0, 1), (0, 1 << 32), (1, 1), (1, 2), (2, 4), (1, 3), (2, 3), (5, 2), (255, 1), (255 * (1 << 32), 1 << 32), (top, 1 << 32), (top - (1 << 31), 1 << 32),
             (top, 1), (top, (1 << 32) - 1), ((1 << 61), 1 << 32), ((1 << 32) * ((1 << 30) - 1), 1 << 32), ((1 << 31) * ((1 << 30) - 1) * 2 + (1 << 31), 1 << 32),
             (6000 // 2 * 15, 6000), (3, 6), (9, 6), (64 * ((1 << 30) - 1), 64)]
    for n in (1, 2, 3, 7, 64, 65536, (1 << 32) - 1, 1 << 32):                # exact halves, and one below and above them
        for q in (0, 1, 12345, (1 << 30) - 2):
            if n % 2 == 0:
                cases += [(q * n + n // 2, n), (q * n + n // 2 - 1, n), (q * n + n // 2 + 1, n)]
            cases += [(q * n, n), (q * n + n - 1, n)]
    rng = np.random.default_rng(62)
    for _ in range(200):
        n = int(rng.integers(1, (1 << 32) + 1))
        cases.append((int(rng.integers(0, 1 << 62)) % (n * (1 << 30)), n))
    return cases


def test_voxel_mean_round_against_python_integers(tmp_path):
    """(2 s + n) / (2 n) in unsigned 64-bit integers for s up to just below 2^62 and n up to 2^32, under the sanitizers."""
    cases = round_cases()
    assert all(0 <= s < 1 << 62 and 1 <= n <= 1 << 32 for s, n in cases)
    assert any(s == (1 << 62) - 1 and n == 1 << 32 for s, n in cases) and any(n == 1 for _, n in cases) and any(s == 0 for s, _ in cases)
    halves = [(s, n) for s, n in cases if (2 * s) % (2 * n) == n]
    assert len(halves) >= 20 and any(n == 1 << 32 for _, n in halves)
    rows = ",\n".join("{%dull, %dull}" % c for c in cases)
    src = tmp_path / "round.cpp"
    src.write_text('#include <cstdio>\n#include "pcr_lattice.h"\nstruct Case { unsigned long long s, n; };\nstatic const Case cases[] = {\n' + rows +
                   '\n};\nstatic_assert(voxel_mean_round(1, 2) == 1 && voxel_mean_round(0, 1) == 0, "usable in constant expressions");\n'
                   'int main() {\n  for (const Case &c : cases) std::printf("%llu\\n", voxel_mean_round(c.s, c.n));\n  return 0;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", build.CSRC,
                    str(src), "-o", str(tmp_path / "round")], check=True)
    res = subprocess.run([str(tmp_path / "round")], check=True, stdout=subprocess.PIPE, text=True)
    got = [int(v) for v in res.stdout.split()]
    want = [(2 * s + n) // (2 * n) for s, n in cases]
    assert got == want
    for (s, n), w in zip(cases, want):                                      # half up, and never outside [floor, ceil] of the mean
        assert s // n <= w <= -(-s // n) and (w == s // n + 1 if (2 * s) % (2 * n) >= n and s % n else True)


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vox", [(0, 0, 0, 1), (-3, 5, 1, 4), (S.INT32_MAX, S.INT32_MIN, 0, 7), (2, 2, 2, 6), (0, 0, 0, 64)])
@pytest.mark.parametrize("clipped", [False, True])
def test_reference_against_a_plain_loop(vox, clipped):
    rng = np.random.default_rng(sum(vox) & 0xFFFF)
    pts = np.empty(3000, P.POINT_DTYPE)
    xyz = rng.integers(-20, 21, (3000, 3))
    xyz[::7] = xyz[1::7][:len(xyz[::7])]                                    # exact duplicates
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["color"] = rng.integers(0, 1 << 32, 3000, dtype=np.int64).astype(np.uint32)
    pts["color"][::5] &= 0x00FFFF00                                         # bytes that are zero in many candidates
    clip = ((-15, -20, -18), (20, 12, 20)) if clipped else None
    want = V.by_loop(pts, vox, clip)
    got, rows, counts = V.reference(pts, vox, clip)
    assert got.dtype == P.POINT_DTYPE and rows.dtype == np.int64 and counts.dtype == np.int64
    assert [(int(p["x"]), int(p["y"]), int(p["z"]), int(p["color"]), int(r), int(n)) for p, r, n in zip(got, rows, counts)] == want
    assert len(want) > (50 if vox[3] < 64 else 0) and np.array_equal(rows, T.reference(xyz, vox, clip, T.FIRST))
    assert int(counts.sum()) == int(T.candidates(xyz, clip).sum())


# ---- the preconditions, on the oracle's decode ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_records(name):
    """The oracle's decode of a stream as POINT_DTYPE records (colours by its own BC1 / BC7 rule, 0x00BBGGRR), and its batch boxes."""
    of = oracle.OracleFile(V.stream(name))
    bc7 = int(of.s.color_format) == 7
    col = np.ctypeslib.as_array(C.cast(of.s.colors, C.POINTER(C.c_uint8)), (of.num_batches * (PPB if bc7 else PPB // 2),))
    fn = oracle.lib().pcr_oracle_decode_bc7 if bc7 else oracle.lib().pcr_oracle_decode_bc1
    ptr = col.ctypes.data
    pts = np.empty(of.num_batches * PPB, P.POINT_DTYPE)
    xyz = np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)])
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["color"] = np.fromiter((fn(i, ptr) & 0xFFFFFF for i in range(len(pts))), np.uint32, len(pts))
    pts.setflags(write=False)
    return pts, S.oracle_bounds(of)


def test_mean_edges_decodes_to_its_sites():
    """The constructed batch: every named site holds what the GPU test needs, by the oracle's decode -- the colours included."""
    pts, _ = oracle_records("mean_edges")
    xyz, _ = V.edges_rows()
    assert np.array_equal(T.xyz_of(pts), xyz)
    vox = (0, 0, 0, V.EDGE_CELL)
    got, rows, counts = V.reference(pts, vox)
    at = {tuple(int(v) for v in np.floor_divide(T.xyz_of(got[i:i + 1])[0], V.EDGE_CELL)): i for i in range(len(got))}
    rec = lambda v: (int(got[at[v]]["x"]), int(got[at[v]]["y"]), int(got[at[v]]["z"]))
    # the mean 0.5 rounds up
    assert counts[at[V.HALF]] == 2 and rec(V.HALF) == (2 * V.EDGE_CELL + 1, 7, 9) and np.array_equal(V.voxel_of(pts, V.HALF), [1000, 1001])
    # all at offset cell - 1: no carry
    assert counts[at[V.TOP]] == 5 and rec(V.TOP) == (5 * V.EDGE_CELL - 1, V.EDGE_CELL - 1, V.EDGE_CELL - 1) and (5, 1, 1) not in at
    # on both sides of coordinate 0
    assert counts[at[V.BELOW]] == 4 and counts[at[V.ABOVE]] == 3 and counts[at[V.MIXED]] == 3
    assert rec(V.BELOW) == (-16 + (36 * 2 + 4) // 8, -16 + (34 * 2 + 4) // 8, -16 + (36 * 2 + 4) // 8) == (-7, -7, -7)
    assert rec(V.ABOVE) == ((2 * 16 + 3) // 6, (2 * 17 + 3) // 6, (2 * 17 + 3) // 6) and rec(V.MIXED)[0] < 0 <= rec(V.MIXED)[1] and rec(V.MIXED)[2] < 0
    # different chains, both ends of a chain
    ends = V.voxel_of(pts, V.ENDS)
    assert sorted(ends // 64) == [5, 5, 700, 900] and sorted(ends % 64) == [0, 0, 63, 63] and rows[at[V.ENDS]] == 320
    # a chain that leaves a voxel and comes back
    back = V.voxel_of(pts, V.RETURNS)
    assert np.array_equal(back, np.r_[640:650, 660:670]) and np.array_equal(V.voxel_of(pts, V.LEFT), np.arange(650, 660))
    assert T.properties(T.xyz_of(pts), vox)["reentered"] >= 1
    # several thousand points, two positions, two colours: the decoded colours differ and tie half way
    big = V.voxel_of(pts, V.BIG)
    assert np.array_equal(big, np.arange(V.BIG_FIRST, V.BIG_FIRST + V.BIG_POINTS)) and counts[at[V.BIG]] == V.BIG_POINTS > 64 * 64
    colours = np.unique(pts["color"][big])
    assert len(colours) == 2 and set(colours) == {V.COLOUR_A, V.COLOUR_B}, "BC1 flattened the two colours: pick others"
    a, b = V.colour_bytes(colours)
    assert ((a + b) % 2 == 1)[:3].all(), "no half-way tie in the decoded colours"
    assert int(got[at[V.BIG]]["color"]) == sum(int((a[j] + b[j] + 1) // 2) << (8 * j) for j in range(4))
    assert rec(V.BIG) == tuple(int(v) for v in V.site(V.BIG, (8, 5, 5)))     # (3 + 12) / 2 and (1 + 8) / 2 round up
    # the filler: voxels of three rows, some over two chains
    props = V.properties(pts, vox)
    print(f"mean_edges cell {V.EDGE_CELL}: {props}, {T.properties(T.xyz_of(pts), vox)}")
    assert props["voxels"] > 15000 and props["position_ties"] >= 2 and props["mean_no_member"] > 1000 and props["colour_no_member"] > 1000
    assert T.properties(T.xyz_of(pts), vox)["multi_chain"] > 100
    for lattice in V.EDGE_LATTICES:
        assert T.lattice_refusal(oracle_records("mean_edges")[1], lattice) is None


# (stream, cell, clip, the counts stated above or None, the properties that have to show). plateau is written without padding: the
# oracle's decode has the tail artefact's rows on top of the generator's points (122 754 and 4164 voxels at cells 64 and 1000,
# 6707 and 237 position ties), so its counts are printed and only held to be positive.
PRECONDITIONS = [
    ("wide30", 1, T.WIDE30_LOW, (58942, 6148, 5, 0, 0), ("multi_point", "colours_differ", "colour_no_member")),
    ("wide30", 2, T.WIDE30_LOW, (35206, 18539, 10, 10408, 3139), ("position_ties", "mean_no_member", "colour_no_member")),
    ("wide30", 7, T.WIDE30_LOW, (2281, 2268, 52, 125, 1754), ("position_ties", "mean_no_member", "colour_no_member")),
    ("plateau", 64, None, None, ("position_ties", "mean_no_member", "colour_no_member")),
    ("plateau", 1000, None, None, ("position_ties", "mean_no_member", "colour_no_member", "colour_ties")),
    ("synth", 7001, None, None, ("position_ties", "mean_no_member", "colour_no_member", "colour_ties")),
]


@pytest.mark.parametrize("name,cell,clip,counts,needs", PRECONDITIONS, ids=lambda v: str(v).replace(" ", "")[:24])
def test_preconditions_on_the_oracles_decode(name, cell, clip, counts, needs):
    pts, bounds = oracle_records(name)
    vox = (0, 0, 0, cell)
    assert T.lattice_refusal(bounds, vox, clip) is None
    got = V.properties(pts, vox, clip)
    spans = T.properties(T.xyz_of(pts), vox, clip)
    print(f"{name} cell {cell} clip {clip}: {got}; {spans}")
    for k in needs:
        assert got[k] >= 1, f"{k}: no such voxel in this case"
    if counts is not None:
        assert (got["voxels"], got["multi_point"], got["largest_n"], got["position_ties"], got["mean_no_member"]) == counts
    if name == "synth":
        for k in ("multi_batch", "multi_chain", "reentered"):
            assert spans[k] >= 1, f"{k}: no such voxel in this case"
    recs, rows, n = V.reference(pts, vox, clip)
    assert np.array_equal(rows, T.reference(T.xyz_of(pts), vox, clip, T.FIRST)) and int(n.sum()) == int(T.candidates(T.xyz_of(pts), clip).sum())
    key_in, _ = T.voxel_keys(np.concatenate([T.xyz_of(recs), T.xyz_of(pts)[rows]]), vox)
    assert np.array_equal(key_in[:len(recs)], key_in[len(recs):]), "a mean left its voxel"


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--thin", "1", "--mean", "--center"], ["--thin", "1", "--center", "--mean"], ["--thin", "1", "--mean", "--mean"],
                                  ["--thin", "--mean"], ["--thin", "0", "--mean"], ["--thin", "1", "--means"], ["--thin", "1", "--mean", "2"],
                                  ["--thin", "1", "--mean", "--box", "0", "0", "0", "1", "1"], ["--mean", "--thin", "1"],
                                  ["--thin", "1", "--box", "0", "0", "0", "1", "1", "1", "--mean", "--center"]])
def test_cli_refuses_mean_with_center_and_a_malformed_mean_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--mean" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
