"""Streams, lattices and the numpy side of the voxel-thinning tests (tests/test_thin_cpu.py checks on the CPU, against the oracle's
decoder, that the cases do what tests/test_gpu_thin.py needs them to do). Inputs and reference arithmetic only."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import grid_cases as G
from tests import select_cases as S

PPB = S.PPB
INT32_MIN, INT32_MAX = S.INT32_MIN, S.INT32_MAX
FIRST, CENTER = 0, 1                                # PCR_THIN_FIRST / PCR_THIN_CENTER
MAX_CELL, MAX_CENTER_CELL = 1 << 30, 2048           # PCR_THIN_MAX_CELL / PCR_THIN_MAX_CENTER_CELL
KEY_BITS = 21                                       # voxels per axis the key holds: 2^21
GOLDEN = ["config1", "ref_packed_batch", "ref_packed_lowentropy", "ref_packed_bc7"]
SYNTHETIC = ["synth", "clustered", "escape_heavy", "wide30", "garbage_tail", "plateau"]
STREAMS = SYNTHETIC + GOLDEN

ORIGINS = [(0, 0, 0), (-12345, 777, -1), (INT32_MAX, INT32_MIN, 0)]       # the last one: the lattice shift needs 64 bits
# cells: 1 collapses exact duplicates only (padding included); 64 and 2^20 take the shift, 1000, 7001 and 2047 the multiply-high
# division; 2048 is the CENTER limit; MAX_CELL the largest. Every stream runs all of these (tests/test_gpu_thin.py), each entry
# without a clip and with the stream's clip in turn: (cell, origin index, mode, clipped).
COMBOS = [
    (1, 0, FIRST, False), (1, 1, CENTER, True),
    (64, 2, CENTER, False), (64, 0, FIRST, True),
    (1 << 20, 1, FIRST, False),
    (1000, 0, CENTER, False), (1000, 2, FIRST, True),
    (7001, 1, FIRST, False), (7001, 0, FIRST, True),
    (2047, 2, CENTER, True), (2047, 1, CENTER, False),
    (2048, 0, CENTER, False), (2048, 2, CENTER, True),
    (MAX_CELL, 2, FIRST, False), (MAX_CELL, 0, FIRST, True),
]

# The preconditioned cases of tests/test_thin_cpu.py: (stream, cell, origin, clip -- None, "stream" for clip_for()'s, or a box), and
# the properties each has to show at least once (see properties()). Chosen from the oracle's decode; the counts it printed are
# in that file's docstring.
WIDE30_LOW = ((0, 0, -100), (2, 1999, 100))         # wide30's cluster at x = 0..2: 65 536 points on 3 x 2000 x 50 lattice sites
CASES = [
    ("synth", 7001, ORIGINS[0], None, ("multi_batch", "multi_chain", "long_runs", "reentered")),
    ("synth", 2048, ORIGINS[1], None, ("multi_batch", "multi_chain", "long_runs", "center_differs")),
    ("clustered", 1000, ORIGINS[0], None, ("multi_batch", "multi_chain", "long_runs", "reentered", "center_differs")),
    ("garbage_tail", 7001, ORIGINS[0], "stream", ("reentered", "multi_batch", "multi_chain")),
    ("garbage_tail", 2048, ORIGINS[2], "stream", ("reentered", "center_differs", "multi_chain")),
    ("plateau", 64, ORIGINS[0], None, ("d2_ties", "multi_chain", "center_differs")),
    ("wide30", 2, ORIGINS[0], WIDE30_LOW, ("d2_ties", "multi_chain", "reentered")),
    ("wide30", 1, ORIGINS[1], WIDE30_LOW, ("d2_ties",)),
]
GARBAGE_TAIL_UNCLIPPED = None                       # lattice_refusal of garbage_tail without a clip: its artefact spans far less than 2^31
PROPERTIES = ("multi_batch", "multi_chain", "long_runs", "reentered", "center_differs", "d2_ties")


def stream(name: str):
    """The .huffman image of a named stream: those of tests/select_cases.py and tests/grid_cases.py, and the four golden files."""
    return G.golden(name) if name in GOLDEN else G.stream(name)


@functools.lru_cache(maxsize=None)
def header_clip(name: str):
    """The box of the stream's header in its integer coordinates (box_from_world of the first batch record's min / max), as
    ((min xyz), (max xyz)): the clip that keeps the tail artefact of an unpadded stream out."""
    info = P.HuffmanFile(stream(name)).batch_las_info(0)
    b = P.box_from_world(info, tuple(info.min), tuple(info.max))
    return tuple(int(v) for v in b.min), tuple(int(v) for v in b.max)


def middle_clip(xyz, lo=0.2, hi=0.8):
    """A box over the middle of the points on every axis (order statistics: exact integers)."""
    s = np.sort(np.asarray(xyz), axis=0)
    n = len(s)
    return tuple(int(v) for v in s[int(n * lo)]), tuple(int(v) for v in s[min(int(n * hi), n - 1)])


def clip_for(name: str, xyz):
    """The clip the clipped cases of a stream use: the header's box for garbage_tail (its tail artefact lies outside), the
    cluster at x = 0..2 for wide30 (a clip over both clusters spans 2^30: too many voxels for a small cell), else the middle
    of the cloud."""
    return header_clip(name) if name == "garbage_tail" else WIDE30_LOW if name == "wide30" else middle_clip(xyz)


def case_clip(name: str, clip, xyz):
    return clip_for(name, xyz) if clip == "stream" else clip


def xyz_of(pts):
    return np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.int64)


def candidates(xyz, clip):
    return np.ones(len(xyz), bool) if clip is None else S.in_box(xyz, clip)


def voxel_keys(xyz, vox):
    """Per row: a key that is equal for two rows iff they share a voxel, and d = p - origin - v * cell per axis (int64 [n, 3]).
    v = floor_divide(p - origin, cell) in int64; the three voxel indices are ranked per axis so that the key fits 63 bits
    whatever their range."""
    org, cell = np.array(vox[:3], np.int64), int(vox[3])
    d = np.asarray(xyz, np.int64) - org
    v = np.floor_divide(d, cell)
    key = np.zeros(len(v), np.int64)
    for k in range(3):
        u, inv = np.unique(v[:, k], return_inverse=True)
        key = key * len(u) + inv.reshape(-1)
    return key, d - v * cell


def d2_of(r, cell):
    """Four times the squared distance to the voxel's centre: sum over the axes of (2 r - (cell - 1))^2."""
    e = 2 * r - (int(cell) - 1)
    return (e * e).sum(axis=1)


def reference(xyz, vox, clip=None, mode=FIRST):
    """The rows pcr_thin keeps of the rows `xyz` (int [n, 3], in row order): int64, increasing. FIRST: np.unique's first
    occurrence of every key among the candidates; CENTER: lexsort by (key, d2, row), the first of every key."""
    m = candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    if len(rows) == 0:
        return rows
    key, r = voxel_keys(np.asarray(xyz)[m], vox)
    if mode == FIRST:
        _, idx = np.unique(key, return_index=True)
        return np.sort(rows[idx])
    d2 = d2_of(r, vox[3])
    order = np.lexsort((rows, d2, key))
    first = np.ones(len(order), bool)
    first[1:] = key[order][1:] != key[order][:-1]
    return np.sort(rows[order[first]])


def lattice_refusal(bounds, vox, clip=None):
    """What pcr_thin says about the lattice: None (accepted; also when the clip is empty or misses every batch), "extent" (q
    spans 2^31 or more on an axis) or "voxels" (more than 2^21 voxels). q = the union of the exact boxes of the batches the
    clip does not miss, intersected with the clip."""
    lo = np.array(S.FULL[0] if clip is None else clip[0], np.int64)
    hi = np.array(S.FULL[1] if clip is None else clip[1], np.int64)
    b = np.asarray(bounds, np.int64).reshape(-1, 6)
    if (lo > hi).any() or len(b) == 0:
        return None
    hit = ~((b[:, 3:] < lo) | (b[:, :3] > hi)).any(axis=1)
    if not hit.any():
        return None
    qlo, qhi = np.maximum(b[hit, :3].min(axis=0), lo), np.minimum(b[hit, 3:].max(axis=0), hi)
    for k in range(3):
        extent = int(qhi[k] - qlo[k])
        if extent >= 1 << 31:
            return "extent"
        if extent // int(vox[3]) + 2 > 1 << KEY_BITS:
            return "voxels"
    return None


def decoded_batches(bounds, clip=None):
    """How many batch boxes the clip does not miss (pcr_thin_stats::batches_decoded)."""
    lo = np.array(S.FULL[0] if clip is None else clip[0], np.int64)
    hi = np.array(S.FULL[1] if clip is None else clip[1], np.int64)
    b = np.asarray(bounds, np.int64).reshape(-1, 6)
    if (lo > hi).any():
        return 0
    return int((~((b[:, 3:] < lo) | (b[:, :3] > hi)).any(axis=1)).sum())


def runs_of(xyz, vox, clip=None):
    """(run id per candidate, candidate rows, keys): a run is a maximal stretch of consecutive candidates of one chain (64
    consecutive rows) with one key; a row that is no candidate ends a run."""
    m = candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    key, _ = voxel_keys(np.asarray(xyz)[m], vox)
    full = np.full(len(xyz), -1, np.int64)
    full[rows] = key
    start = np.ones(len(rows), bool)
    prev = rows - 1
    inside = (rows % 64) != 0
    start[inside] = full[prev[inside]] != key[inside]
    return np.cumsum(start) - 1, rows, key


def count_runs(xyz, vox, clip=None):
    run, rows, _ = runs_of(xyz, vox, clip)
    return int(run[-1]) + 1 if len(rows) else 0


def properties(xyz, vox, clip=None):
    """The counts tests/test_thin_cpu.py asserts, over the rows `xyz` of a whole stream:
      multi_batch     voxels whose candidates lie in two or more batches
      multi_chain     voxels whose candidates lie in two or more chains of one batch
      long_runs       runs longer than one point
      reentered       (chain, voxel) pairs with two or more runs: the chain comes back to the voxel
      center_differs  voxels where the CENTER winner is not the FIRST winner (cell <= MAX_CENTER_CELL, else 0)
      d2_ties         voxels where two or more candidates share CENTER's least d2, so the row decides"""
    run, rows, key = runs_of(xyz, vox, clip)
    out = dict.fromkeys(PROPERTIES, 0)
    if len(rows) == 0:
        return out
    _, kid = np.unique(key, return_inverse=True)
    kid = kid.reshape(-1)
    nk = int(kid.max()) + 1
    batch, chain = rows >> 16, rows >> 6

    def spread(group, value):
        """per group: does `value` take two or more values"""
        lo = np.full(int(group.max()) + 1, np.iinfo(np.int64).max)
        hi = np.full(int(group.max()) + 1, -1)
        np.minimum.at(lo, group, value)
        np.maximum.at(hi, group, value)
        return hi > lo

    out["multi_batch"] = int(spread(kid, batch).sum())
    _, kb = np.unique(kid * (int(batch.max()) + 1) + batch, return_inverse=True)
    kb = kb.reshape(-1)
    multi = spread(kb, chain)
    out["multi_chain"] = len(np.unique(kid[multi[kb]]))
    out["long_runs"] = int((np.bincount(run) > 1).sum())
    _, ck = np.unique(chain * nk + kid, return_inverse=True)
    out["reentered"] = int(spread(ck.reshape(-1), run).sum())
    if int(vox[3]) <= MAX_CENTER_CELL:
        first, center = reference(xyz, vox, clip, FIRST), reference(xyz, vox, clip, CENTER)
        out["center_differs"] = len(np.setdiff1d(center, first))
        _, r = voxel_keys(np.asarray(xyz)[rows], vox)
        d2 = d2_of(r, vox[3])
        least = np.full(nk, np.iinfo(np.int64).max)
        np.minimum.at(least, kid, d2)
        out["d2_ties"] = int((np.bincount(kid[d2 == least[kid]], minlength=nk) >= 2).sum())
    return out


def table_slots(runs: int) -> int:
    """max(1024, the power of two >= 2 * runs); 0 when nothing is inserted."""
    if runs == 0:
        return 0
    s = 1024
    while s < 2 * runs:
        s *= 2
    return s
