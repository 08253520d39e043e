"""The numpy side of the voxel-mean tests: the reference over read_points rows, the properties tests/test_voxel_mean_cpu.py counts on
the oracle's decode, and `mean_edges`, one constructed batch whose lattice sites are named below. Inputs and reference arithmetic
only."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import select_cases as S
from tests import thin_cases as T

PPB = S.PPB
MAX_ROWS = 1 << 32                                  # PCR_VOXEL_MEAN_MAX_ROWS


def mean_round(s, n):
    """(2 s + n) // (2 n): the mean of n non-negative integers with sum s, rounded half up (int64 arrays or Python integers)."""
    return (2 * s + n) // (2 * n)


def colour_bytes(colour):
    c = np.asarray(colour).astype(np.int64)
    return np.stack([(c >> (8 * j)) & 255 for j in range(4)], axis=1)


def groups(pts, vox, clip=None):
    """The candidates of `pts` (POINT_DTYPE, in row order) grouped by voxel, the groups in the order of their least row:
    a dict of rows (the candidates' rows, grouped, ascending inside a group), starts (the first entry of every group), n, xyz and
    r (position and offset inside the voxel per entry) and colour bytes per entry (all int64)."""
    xyz = T.xyz_of(pts)
    m = T.candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    if len(rows) == 0:
        return None
    key, r = T.voxel_keys(xyz[m], vox)
    order = np.argsort(key, kind="stable")          # rows ascend inside a key
    ks = key[order]
    starts = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    n = np.diff(np.r_[starts, len(ks)]).astype(np.int64)
    by_row = np.argsort(rows[order][starts], kind="stable")     # regroup so that the groups come in the order of their least row
    order = order[_regroup(starts, n, by_row)]
    n = n[by_row]
    starts = np.r_[0, np.cumsum(n)[:-1]]
    return dict(rows=rows[order], starts=starts, n=n, xyz=xyz[m][order], r=r[order], bytes=colour_bytes(pts["color"][m][order]))


def _regroup(starts, n, by_row):
    """The entries of the groups `by_row`, group after group (a vectorised concatenation of ranges)."""
    n2 = n[by_row]
    first = np.repeat(starts[by_row], n2)
    within = np.arange(int(n2.sum())) - np.repeat(np.r_[0, np.cumsum(n2)[:-1]], n2)
    return first + within


def reference(pts, vox, clip=None):
    """(records POINT_DTYPE, rows int64, counts int64) of pcr_voxel_mean over the rows `pts`: integer sums by np.add.reduceat on
    int64, integer rounding, the voxels ordered by their least row."""
    g = groups(pts, vox, clip)
    if g is None:
        return np.empty(0, P.POINT_DTYPE), np.empty(0, np.int64), np.empty(0, np.int64)
    n = g["n"]
    s = np.add.reduceat(g["r"], g["starts"], axis=0)
    c = np.add.reduceat(g["bytes"], g["starts"], axis=0)
    corner = (g["xyz"] - g["r"])[g["starts"]]                   # the voxel's min corner
    pos = corner + mean_round(s, n[:, None])
    col = mean_round(c, n[:, None])
    assert pos.min() >= S.INT32_MIN and pos.max() <= S.INT32_MAX and col.min() >= 0 and col.max() <= 255
    out = np.empty(len(n), P.POINT_DTYPE)
    out["x"], out["y"], out["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    out["color"] = (col[:, 0] | col[:, 1] << 8 | col[:, 2] << 16 | col[:, 3] << 24).astype(np.uint32)
    return out, g["rows"][g["starts"]], n


def by_loop(pts, vox, clip=None):
    """The same by a plain loop over the rows with Python integers (for a few thousand rows)."""
    acc, order = {}, []
    for row, p in enumerate(pts):
        xyz = [int(p["x"]), int(p["y"]), int(p["z"])]
        if clip is not None and not all(clip[0][k] <= xyz[k] <= clip[1][k] for k in range(3)):
            continue
        v = tuple((xyz[k] - vox[k]) // vox[3] for k in range(3))
        if v not in acc:
            acc[v] = [row, 0, [0, 0, 0], [0, 0, 0, 0]]
            order.append(v)
        a = acc[v]
        a[1] += 1
        for k in range(3):
            a[2][k] += xyz[k] - vox[k] - v[k] * vox[3]
        for j in range(4):
            a[3][j] += (int(p["color"]) >> (8 * j)) & 255
    out = []
    for v in order:                                 # (first seen = least row)
        row, n, s, c = acc[v]
        pos = [vox[k] + v[k] * vox[3] + (2 * s[k] + n) // (2 * n) for k in range(3)]
        col = sum(((2 * c[j] + n) // (2 * n)) << (8 * j) for j in range(4))
        out.append((pos[0], pos[1], pos[2], col, row, n))
    return out


PROPERTIES = ("voxels", "multi_point", "largest_n", "position_ties", "mean_no_member", "colour_ties", "colour_no_member", "colours_differ")


def properties(pts, vox, clip=None):
    """Counts over the voxels of a call:
      voxels, multi_point, largest_n
      position_ties     voxels whose mean offset is exactly half way between two integers on some axis (the rounding decides)
      mean_no_member    voxels whose mean position is no candidate's position
      colour_ties       voxels with a half-way tie in some colour byte
      colour_no_member  voxels whose mean colour is no candidate's colour
      colours_differ    voxels whose candidates do not all have one colour"""
    g = groups(pts, vox, clip)
    out = dict.fromkeys(PROPERTIES, 0)
    if g is None:
        return out
    n, starts = g["n"], g["starts"]
    s = np.add.reduceat(g["r"], starts, axis=0)
    c = np.add.reduceat(g["bytes"], starts, axis=0)
    mean_r, mean_c = mean_round(s, n[:, None]), mean_round(c, n[:, None])
    gid = np.repeat(np.arange(len(n)), n)
    member = np.zeros(len(n), bool)
    np.logical_or.at(member, gid, (g["r"] == mean_r[gid]).all(axis=1))
    cmember = np.zeros(len(n), bool)
    np.logical_or.at(cmember, gid, (g["bytes"] == mean_c[gid]).all(axis=1))
    differ = np.zeros(len(n), bool)
    np.logical_or.at(differ, gid, (g["bytes"] != g["bytes"][starts][gid]).any(axis=1))
    out.update(voxels=len(n), multi_point=int((n > 1).sum()), largest_n=int(n.max()),
               position_ties=int(((2 * s) % (2 * n[:, None]) == n[:, None]).any(axis=1).sum()), mean_no_member=int((~member).sum()),
               colour_ties=int(((2 * c) % (2 * n[:, None]) == n[:, None]).any(axis=1).sum()), colour_no_member=int((~cmember).sum()),
               colours_differ=int(differ.sum()))
    return out


# ---- mean_edges: one batch of 65 536 given rows ------------------------------------------------------------------------------------
# Lattice sites at cell EDGE_CELL and origin (0, 0, 0); a voxel is named by its three indices.
EDGE_CELL = 16
HALF = (2, 0, 0)                                    # two points at offsets 0 and 1 on x: the mean 0.5 rounds up to 1
TOP = (4, 0, 0)                                     # five points at offset cell - 1 on every axis: no carry into the next voxel
BELOW, ABOVE, MIXED = (-1, -1, -1), (0, 0, 0), (-3, 0, -1)     # on both sides of coordinate 0
ENDS = (8, 8, 0)                                    # points in the first and last row of chains 5, 700 and 900
LEFT, RETURNS = (12, 2, 0), (13, 2, 0)              # chain 10 visits RETURNS, LEFT and RETURNS again
BIG = (20, 20, 1)                                   # BIG_POINTS points, alternating between two positions and two colours
BIG_POINTS, BIG_FIRST = 6000, 8192                  # rows 8192 .. 14191: 94 chains
BIG_A, BIG_B = (3, 5, 1), (12, 5, 8)                # their offsets: x 3 + 12 and z 1 + 8 are odd, so both means are half way
FILLER_Y = 64                                       # the other rows: three consecutive rows a voxel, in rows y >= 64 of the lattice
EDGE_LATTICES = [(0, 0, 0, EDGE_CELL), (-12345, 777, -1, EDGE_CELL), (S.INT32_MAX, S.INT32_MIN, 0, EDGE_CELL), (0, 0, 0, 1), (5, 5, 5, 7), (0, 0, 0, 64),
                 (0, 0, 0, T.MAX_CELL)]


def expand565(r5, g6, b5):
    """0x00BBGGRR of a 5-6-5 colour by bit replication: what BC1 stores exactly"""
    return ((r5 << 3) | (r5 >> 2)) | (((g6 << 2) | (g6 >> 4)) << 8) | (((b5 << 3) | (b5 >> 2)) << 16)


COLOUR_A, COLOUR_B = expand565(0, 10, 31), expand565(4, 50, 3)      # red 0 and 33, green 40 and 203, blue 255 and 24: every sum is odd


def site(v, offset=(0, 0, 0)):
    return np.array(v, np.int64) * EDGE_CELL + np.array(offset, np.int64)


@functools.lru_cache(maxsize=None)
def edges_rows():
    """(xyz int64 [65536, 3], colours uint32 [65536]) as given to the encoder, read-only."""
    rng = np.random.default_rng(2323)
    r = np.arange(PPB, dtype=np.int64)
    g = r // 3
    xyz = np.stack([(g % 256) * EDGE_CELL + r * 7 % EDGE_CELL, (FILLER_Y + g // 256) * EDGE_CELL + r * 3 % EDGE_CELL, 3 * EDGE_CELL + r * 5 % EDGE_CELL], axis=1)
    col = np.repeat(rng.integers(0, 1 << 24, PPB // 16), 16).astype(np.uint32)      # one colour a block: BC1 keeps it (to 5-6-5)
    col[1::2] ^= 0x00080408                                                          # ... and a second one that differs a little
    xyz[[1000, 1001]] = [site(HALF, (0, 7, 9)), site(HALF, (1, 7, 9))]
    xyz[2000:2005] = site(TOP, (EDGE_CELL - 1,) * 3)
    xyz[3000:3004] = [site(BELOW, (15, 15, 15)), site(BELOW, (0, 13, 14)), site(BELOW, (15, 0, 0)), site(BELOW, (6, 6, 7))]      # (-1, -1, -1) ..
    xyz[3004:3007] = [site(ABOVE), site(ABOVE, (1, 2, 3)), site(ABOVE, (15, 15, 14))]
    xyz[3007:3010] = [site(MIXED, (0, 0, 15)), site(MIXED, (15, 15, 0)), site(MIXED, (2, 9, 4))]
    for k, row in enumerate((5 * 64, 5 * 64 + 63, 700 * 64, 900 * 64 + 63)):
        xyz[row] = site(ENDS, (1 + 4 * k, 15 - 2 * k, k))
    xyz[640:650] = site(RETURNS) + rng.integers(0, EDGE_CELL, (10, 3))
    xyz[650:660] = site(LEFT) + rng.integers(0, EDGE_CELL, (10, 3))
    xyz[660:670] = site(RETURNS) + rng.integers(0, EDGE_CELL, (10, 3))
    big = np.arange(BIG_FIRST, BIG_FIRST + BIG_POINTS)
    xyz[big[0::2]], xyz[big[1::2]] = site(BIG, BIG_A), site(BIG, BIG_B)
    col[big[0::2]], col[big[1::2]] = COLOUR_A, COLOUR_B
    xyz.setflags(write=False); col.setflags(write=False)
    return xyz, col


EDGE_LO, EDGE_HI = (-4 * EDGE_CELL,) * 3, (256 * EDGE_CELL, (FILLER_Y + 86) * EDGE_CELL, 4 * EDGE_CELL)


@functools.lru_cache(maxsize=None)
def stream(name: str):
    """The .huffman image of a named stream: `mean_edges`, or one of tests/thin_cases.py."""
    if name != "mean_edges":
        return T.stream(name)
    xyz, col = edges_rows()
    assert (xyz >= np.array(EDGE_LO)).all() and (xyz <= np.array(EDGE_HI)).all()
    x, y, z = (np.ascontiguousarray(xyz[:, k].astype(np.int32)) for k in range(3))
    return S._keep(P.encode_points(x, y, z, col, S.las_for(EDGE_LO, EDGE_HI), morton_sort=False, nthreads=2, pad_tails=True)[0])


def voxel_of(pts, v, vox=(0, 0, 0, EDGE_CELL)):
    """The rows of `pts` in voxel v of the lattice `vox`"""
    xyz = T.xyz_of(pts)
    return np.nonzero((np.floor_divide(xyz - np.array(vox[:3], np.int64), vox[3]) == np.array(v, np.int64)).all(axis=1))[0]
