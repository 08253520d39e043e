"""Level-of-detail ordering, the parts that need no GPU: the two entry points and two structs in the headers, the binding tables
and the cross-compiled library; lod_lattice, lod_parent_key and the level-byte arithmetic of csrc/pcr_lattice.h, compiled into a
stand-alone program (address and undefined-behaviour sanitizers on) and held against Python integers; lod_from_world; the numpy
reference of tests/lod_cases.py against a plain loop; the CLI's refusal of a malformed --lod before any device is touched; and the
preconditions of tests/test_gpu_lod.py, from the oracle's decoder.

The level counts, as the oracle's decode gave them when the cases were chosen (stream, origin, cell x levels, clip: counts, rest):
  synth (0,0,0) 500 x 6 none:             [5409, 16067, 60257, 208304, 309850, 29], rest 55444
  synth (-12345,777,-1) 64 x 12 none:     [72, 228, 991, 3921, 15483, 57778, 200061, 321354, 29, 16, 10, 9], rest 55408
  clustered (0,0,0) 125 x 8 none:         [81, 182, 786, 3757, 17157, 65057, 131297, 67699], rest 41664
  garbage_tail (0,0,0) 875 x 4 header:    [26951, 72139, 200075, 747], rest 27718
  plateau (0,0,0) 1 x 7 none:             [122754, 6162, 1613, 421, 95, 24, 3], rest 0
  wide30 (0,0,0) 1 x 3 x in 0..2:         [6495, 28711, 23736], rest 6594
The tests assert the properties named in lod_cases.CASES, not these numbers, and print what they find."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import lod_cases as D
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_abi import declared
from tests.test_thin_cpu import las, oracle_rows

SYMBOLS = ("pcr_lod_order", "pcr_read_lod_order")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Lod), C.POINTER(N.Box), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_int64), C.POINTER(N.LodStats)]
    assert bound.pcr_lod_order.argtypes == args and bound.pcr_read_lod_order.argtypes == args
    for name in ("Lod", "LodStats", "LOD_MAX_LEVELS", "LOD_DROP_REST", "LOD_ROW_ORDER", "as_lod", "lod_from_world"):
        assert hasattr(P, name)
    for name in ("lod_order", "read_lod_order"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.lod_ordered)


def test_structs_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirrors."""
    lod = [f for f, _ in N.Lod._fields_]
    stats = [f for f, _ in N.LodStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\n'
                   'printf("%zu %zu ", sizeof(pcr_lod), sizeof(pcr_lod_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_lod, {f}));\n' for f in lod)
                   + "".join(f'printf("%zu ", offsetof(pcr_lod_stats, {f}));\n' for f in stats)
                   + 'printf("%d %u %u %d\\n", PCR_LOD_MAX_LEVELS, PCR_LOD_DROP_REST, PCR_LOD_ROW_ORDER, PCR_THIN_MAX_CELL);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:2] == [24, 48 + 8 * 17] == [C.sizeof(N.Lod), C.sizeof(N.LodStats)]
    assert got[2:6] == [0, 12, 16, 20] == [getattr(N.Lod, f).offset for f in lod]
    assert got[6:13] == [0, 8, 16, 24, 32, 40, 48] == [getattr(N.LodStats, f).offset for f in stats]
    assert lod == ["origin", "cell", "levels", "reserved"]
    assert stats == ["batches_outside", "batches_decoded", "points_considered", "runs", "table_slots", "points_written", "level_count"]
    assert got[13:] == [N.LOD_MAX_LEVELS, N.LOD_DROP_REST, N.LOD_ROW_ORDER, N.THIN_MAX_CELL] == [D.MAX_LEVELS, D.DROP_REST, D.ROW_ORDER, T.MAX_CELL]
    assert N.LodStats().as_dict()["level_count"] == [0] * 17


# ---- the lattice (csrc/pcr_lattice.h) in a program of its own ------------------------------------------------------------------
I32 = (S.INT32_MIN, S.INT32_MAX)


def lattice_cases():
    """origin, finest cell, levels, q.min, q.max: thin_cases.ORIGINS (the third one needs the 64-bit shift); the extents 2^31 - 1 and
    2^31; one voxel below, at and above the limit for levels 1, 2 and 16; the coarsest cell at its maximum."""
    out = []
    for o in T.ORIGINS:
        for levels in (1, 2, 16):
            cell = 3
            for over in (-1, 0, 1):
                # extent // cell + 2^(levels - 1) + 1 == 2^21 + over
                extent = ((1 << 21) + over - (1 << (levels - 1)) - 1) * cell + (cell - 1 if over <= 0 else 0)
                out.append((o, cell, levels, (-7, 11, I32[0]), (-7 + extent, 11, I32[0] + 5)))
                out.append((o, cell, levels, (5, 5, 100 - extent), (5, 5, 100)))
            top = (1 << 30) >> (levels - 1)                                 # the coarsest cell is PCR_THIN_MAX_CELL
            out.append((o, top, levels, (I32[0], 0, 0), (-2, 5, 5)))                          # extent 2^31 - 2
            out.append((o, top, levels, (0, I32[0] + 1, 0), (0, 0, 0)))                       # extent 2^31 - 1: accepted
            out.append((o, top, levels, (0, 0, I32[0]), (0, 0, 0)))                           # extent 2^31: refused
            out.append((o, top, levels, (I32[0], I32[0], I32[0]), (I32[1] - 1, -1, 0)))
            out.append((o, 64, levels, (593, 593, 241), (999406, 999406, 74106)))
            out.append((o, 7001, min(levels, 2), (-1048562, -1048564, -67759), (1048571, 1048556, 68709)))
    return out


def lattice_by_hand(origin, cell, levels, qmin, qmax):
    coarsest = cell << (levels - 1)
    out = []
    for k in range(3):
        extent = qmax[k] - qmin[k]
        if extent >= 1 << 31:
            return [1, k]
        if extent // cell + (1 << (levels - 1)) + 1 > 1 << 21:
            return [2, k]
        shifted = origin[k] + (qmin[k] - origin[k]) // coarsest * coarsest          # Python's // is the floor
        assert shifted <= qmin[k] < shifted + coarsest and (shifted - origin[k]) % coarsest == 0
        assert qmax[k] - shifted < 1 << 32 and (qmax[k] - shifted) // cell < 1 << 21  # d fits 32 bits, the finest index its field
        # nested: the index of every level is the finest one shifted, for the corners of q
        for p in (qmin[k], qmax[k]):
            for l in range(levels):
                assert (p - origin[k]) // (cell << (levels - 1 - l)) - (shifted - origin[k]) // (cell << (levels - 1 - l)) == ((p - shifted) // cell) >> (levels - 1 - l)
        out.append(shifted % (1 << 32))
    pow2 = cell & (cell - 1) == 0
    return [0, 2] + out + [cell, cell.bit_length() - 1 if pow2 else 32, 0 if pow2 else -(-(1 << 64) // cell)]


BYTE_PROGRAM = r'''
static uint64_t rnd(uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static int check_bytes()
{
    uint64_t s = 0x9E3779B97F4A7C15ull;
    const uint8_t pool[] = {0, 1, 2, 5, 15, 16, 0x7F, 0x80, 0xFE, 0xFF};
    for (int it = 0; it < 200000; ++it) {
        uint8_t b[8];
        uint64_t w = 0;
        for (int j = 0; j < 8; ++j) { b[j] = (it & 1) ? pool[rnd(s) % sizeof pool] : (uint8_t)rnd(s); w |= (uint64_t)b[j] << (8 * j); }
        const uint32_t v = (it & 2) ? pool[rnd(s) % sizeof pool] : (uint32_t)(rnd(s) & 0xFF), cand = (uint32_t)(rnd(s) & 0xFF);
        const uint32_t levels = 1 + (uint32_t)(rnd(s) % 16), classes = levels + (uint32_t)(rnd(s) & 1);
        uint64_t nz = 0, eq = 0, spread = 0, fin = 0, wr = 0;
        for (int j = 0; j < 8; ++j) {
            if (b[j]) nz |= 0x80ull << (8 * j);
            if (b[j] == v) eq |= 0x80ull << (8 * j);
            if ((cand >> j) & 1) spread |= 0x80ull << (8 * j);
            const uint8_t f = (b[j] == 0xFF && ((cand >> j) & 1)) ? (uint8_t)levels : b[j];
            fin |= (uint64_t)f << (8 * j);
        }
        if (lod_bytes_nonzero(w) != nz || lod_bytes_equal(w, v) != eq || lod_flags_of_bits(cand) != spread || lod_bytes_final(w, cand, levels) != fin) return 1;
        if (lod_bits_of_flags(spread) != cand) return 2;
        // the bytes a call sees are levels 0 .. levels or LOD_NO_LEVEL
        uint64_t lw = 0;
        for (int j = 0; j < 8; ++j) {
            const uint32_t r = (uint32_t)(rnd(s) % (levels + 2));
            const uint8_t l = r > levels ? 0xFF : (uint8_t)r;
            lw |= (uint64_t)l << (8 * j);
            if (l < classes) wr |= 0x80ull << (8 * j);
        }
        if (lod_bytes_written(lw, levels, classes) != wr) return 3;
        // the parent key: every 21-bit field halved
        const uint64_t x = rnd(s) & 0x1FFFFF, y = rnd(s) & 0x1FFFFF, z = rnd(s) & 0x1FFFFF;
        if (lod_parent_key(x | y << 21 | z << 42) != ((x >> 1) | (y >> 1) << 21 | (z >> 1) << 42)) return 4;
    }
    return 0;
}
'''


def test_lattice_shift_limits_and_bytes_against_python_integers(tmp_path):
    """lod_lattice() for origins and boxes at the edges of int32: the refusals, the shifted origin modulo 2^32 and the divisor;
    the level-byte arithmetic and lod_parent_key against loops over the bytes. A program of its own, sanitizers on."""
    cases = lattice_cases()
    rows = ",\n".join("{{%d, %d, %d}, %d, %d, {%d, %d, %d}, {%d, %d, %d}}" % (*o, c, n, *lo, *hi) for o, c, n, lo, hi in cases)
    rows = rows.replace("-2147483648", "(-2147483647 - 1)")
    src = tmp_path / "lod_lattice.cpp"
    src.write_text('#include <cstdio>\n#include "pcr_lattice.h"\nstruct Case { int32_t origin[3]; int32_t cell, levels; int32_t lo[3], hi[3]; };\n'
                   'static const Case cases[] = {\n' + rows + '\n};\n' + BYTE_PROGRAM + 'int main() {\n  for (const Case &c : cases) {\n'
                   '    ThinLattice l{}; int axis = -1;\n'
                   '    const int rc = lod_lattice(c.origin, c.cell, c.levels, c.lo, c.hi, &l, &axis);\n'
                   '    if (rc) std::printf("%d %d\\n", rc, axis);\n'
                   '    else std::printf("0 %d %u %u %u %u %u %llu\\n", axis, l.origin[0], l.origin[1], l.origin[2], l.cell, l.div.shift, l.div.magic);\n'
                   '    if (c.levels == 1) { ThinLattice t{}; int a2 = -1;\n'
                   '      if (thin_lattice(c.origin, c.cell, c.lo, c.hi, &t, &a2) != rc || a2 != axis || (!rc && (t.origin[0] != l.origin[0] || t.origin[1] != l.origin[1] || t.origin[2] != l.origin[2]))) return 3; }\n'
                   '  }\n  const int bad = check_bytes();\n  if (bad) { std::printf("bytes %d\\n", bad); return 4; }\n  return 0;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", build.CSRC,
                    str(src), "-o", str(tmp_path / "lod_lattice")], check=True)
    res = subprocess.run([str(tmp_path / "lod_lattice")], check=True, stdout=subprocess.PIPE, text=True)
    got = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
    want = [lattice_by_hand(*case) for case in cases]
    assert got == want
    assert sorted({w[0] for w in want}) == [0, 1, 2], "the cases reach both refusals and the accepted path"
    # one voxel below and at the limit are accepted, one above is refused, for every origin and number of levels
    verdicts = [w[0] for w, c in zip(want, cases) if c[1] == 3]
    assert verdicts == [0, 0, 0, 0, 2, 2] * (len(verdicts) // 6) and len(verdicts) == 6 * 9


# ---- lod_from_world ----------------------------------------------------------------------------------------------------------------
def lod_fields(v):
    return tuple(v.origin) + (v.cell, v.levels, v.reserved)


def test_lod_from_world():
    assert lod_fields(P.lod_from_world(las(), 0.5, 4)) == (0, 0, 0, 500, 4, 0)
    assert lod_fields(P.lod_from_world(las(lo=(1.0005, -2.0, 3.0)), 0.001, 16)) == (1001, -2000, 3000, 1, 16, 0)
    assert lod_fields(P.lod_from_world(las(), 1073741.824, 1)) == (0, 0, 0, 1 << 30, 1, 0)
    assert lod_fields(P.lod_from_world(las(), 32.768, 16)) == (0, 0, 0, 1 << 15, 16, 0)
    assert lod_fields(P.as_lod((1, -2, 3, 4, 5))) == (1, -2, 3, 4, 5, 0) and lod_fields(P.as_lod(P.as_lod((1, -2, 3, 4, 5)))) == (1, -2, 3, 4, 5, 0)
    with pytest.raises(ValueError):
        P.as_lod((0, 0, 1 << 31, 1, 1))
    for cell_size, levels in ((0.5, 0), (0.5, 17), (32.769, 16), (65.536, 16), (1073741.824, 2), (0.0015, 3), (0.0, 3), (-1.0, 2)):
        with pytest.raises(ValueError):
            P.lod_from_world(las(), cell_size, levels)
    with pytest.raises(ValueError):
        P.lod_from_world(las((0.001, 0.001, 0.002)), 0.004, 2)              # what voxels_from_world refuses
    with pytest.raises(ValueError):
        P.lod_from_world(las(), 1.0, 2, origin=(0.0, 1e10, 0.0))


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lod", [(0, 0, 0, 1, 1), (-3, 5, 1, 2, 4), (S.INT32_MAX, S.INT32_MIN, 0, 3, 3), (2, 2, 2, 1, 7)])
def test_reference_against_a_plain_loop(lod):
    rng = np.random.default_rng(sum(lod) & 0xFFFF)
    xyz = rng.integers(-20, 21, (3000, 3))
    xyz[::7] = xyz[1::7][:len(xyz[::7])]                                    # exact duplicates
    clip = ((-15, -20, -18), (20, 12, 20))
    L = lod[4]
    first = [{} for _ in range(L)]                                          # per level: voxel -> lowest row
    cand = []
    for row, p in enumerate(xyz):
        p = [int(v) for v in p]
        if not all(clip[0][k] <= p[k] <= clip[1][k] for k in range(3)):
            continue
        cand.append(row)
        for l in range(L):
            first[l].setdefault(tuple((p[k] - lod[k]) // D.cell_of(lod, l) for k in range(3)), row)
    want = np.full(len(xyz), D.NO_LEVEL, np.uint8)
    for row in cand:
        p = [int(v) for v in xyz[row]]
        want[row] = min([l for l in range(L) if first[l][tuple((p[k] - lod[k]) // D.cell_of(lod, l) for k in range(3))] == row], default=L)
    got = D.levels(xyz, lod, clip)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and {0, L - 1, L, D.NO_LEVEL} <= set(want.tolist())
    for flags in (0, D.DROP_REST, D.ROW_ORDER, D.DROP_REST | D.ROW_ORDER):
        rows, lv = D.order(got, lod, flags)
        keep = [r for r in cand if want[r] < (L if flags & D.DROP_REST else L + 1)]
        assert rows.tolist() == (keep if flags & D.ROW_ORDER else sorted(keep, key=lambda r: (want[r], r))) and np.array_equal(lv, want[rows])
    assert D.level_counts(got, lod) == np.bincount(want[cand], minlength=17).tolist()


@pytest.mark.parametrize("name,origin,cell,levels,clip,needs", D.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_cases_show_the_properties_claimed(name, origin, cell, levels, clip, needs):
    xyz, bounds = oracle_rows(name)
    lod, clip = (*origin, cell, levels), T.case_clip(name, clip, xyz)
    assert D.lattice_refusal(bounds, lod, clip) is None
    lv = D.levels(xyz, lod, clip)
    got = D.properties(lv, lod)
    counts = D.level_counts(lv, lod)
    print(f"{name} origin {origin} cell {cell} x {levels} clip {clip}: level counts {counts[:levels]}, rest {counts[levels]}, {got}")
    for k in needs:
        assert got[k] >= 1, f"{k}: this case does not show it"
    cand = T.candidates(xyz, clip)
    assert sum(counts) == int(cand.sum()) and counts[levels + 1:] == [0] * (D.MAX_LEVELS - levels) and (lv[~cand] == D.NO_LEVEL).all()
    previous = None
    for l in range(levels):
        # per level the equality with the thinning reference: the rows of level <= l are what pcr_thin FIRST keeps with that cell
        thin = T.reference(xyz, D.vox_of(lod, l), clip, T.FIRST)
        assert np.array_equal(np.nonzero(lv <= l)[0], thin), f"level {l}"
        # the nesting itself: a coarse voxel's first row is the first row of a finer voxel
        if previous is not None:
            assert np.isin(previous, thin).all()
        previous = thin


def test_every_property_is_covered_and_the_cases_are_the_ones_listed():
    assert set(D.PROPERTIES) == {k for c in D.CASES for k in c[5]}
    assert [(c[0], c[2], c[3]) for c in D.CASES] == [("synth", 500, 6), ("synth", 64, 12), ("clustered", 125, 8), ("garbage_tail", 875, 4), ("plateau", 1, 7),
                                                      ("wide30", 1, 3)]
    assert all((c[2] << (c[3] - 1)) <= T.MAX_CELL for c in D.CASES)


def test_lattice_refusal_of_the_reference_restates_the_rule():
    b = [[0, 0, 0, (1 << 21) - 2, 5, 5]]
    assert D.lattice_refusal(b, (0, 0, 0, 1, 1)) is None and D.lattice_refusal(b, (0, 0, 0, 1, 2)) == "voxels"
    assert D.lattice_refusal(b, (0, 0, 0, 1, 2), ((0, 0, 0), ((1 << 21) - 3, 5, 5))) is None
    assert D.lattice_refusal(b, (0, 0, 0, 1 << 10, 16)) is None and D.lattice_refusal(b, (0, 0, 0, 1, 16)) == "voxels"
    assert D.lattice_refusal([[S.INT32_MIN, 0, 0, 0, 0, 0]], (0, 0, 0, 1 << 20, 3)) == "extent"
    assert D.lattice_refusal(b, (0, 0, 0, 1, 16), S.EMPTY) is None and D.lattice_refusal([], (0, 0, 0, 1, 16)) is None
    for L in (1, 2, 16):                                                    # levels == 1 is pcr_thin's rule
        assert (D.lattice_refusal(b, (0, 0, 0, 1, L)) is None) == (L == 1)
    assert D.lattice_refusal(b, (0, 0, 0, 7, 1)) == T.lattice_refusal(b, (0, 0, 0, 7))
    assert D.table_slots(513) == 2048 and D.table_slots(0) == 0


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--lod"], ["--lod", "1"], ["--lod", "x", "3"], ["--lod", "0", "3"], ["--lod", "-1", "3"], ["--lod", "nan", "3"],
                                  ["--lod", "1", "0"], ["--lod", "1", "17"], ["--lod", "1", "3.5"], ["--lod", "1", "x"], ["--lod", "1", "3", "--drop"],
                                  ["--lod", "1", "3", "--drop-rest", "--drop-rest"], ["--lod", "1", "3", "--box", "0", "0", "0", "1", "1"],
                                  ["--lod", "1", "3", "--thin", "1"], ["--thin", "1", "--lod", "1", "3"], ["--lod", "1", "3", "--denoise", "1", "2"],
                                  ["--denoise", "1", "2", "--lod", "1", "3"], ["--lod", "1", "3", "--center"], ["--lod", "1", "3", "--view"],
                                  ["--lod", "1", "3", "--box", "0", "0", "0", "1", "1", "1", "--box", "0", "0", "0", "1", "1", "1"]])
def test_cli_refuses_a_malformed_lod_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--lod CELL LEVELS" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
