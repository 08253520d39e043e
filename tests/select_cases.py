"""Streams, boxes and the numpy side of the box-selection tests (tests/test_select_cpu.py checks on the CPU, against the oracle's
decoder, that the boxes do what tests/test_gpu_select.py needs them to do). Inputs and reference arithmetic only."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import oracle, scenes

PPB = 65536
OUTSIDE, INSIDE, STRADDLING = 0, 1, 2
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
FULL = ((INT32_MIN,) * 3, (INT32_MAX,) * 3)
EMPTY = ((1, 0, 0), (0, 10, 10))                    # min > max on one axis
NOTHING = ((2_000_000_000, 2_000_000_000, 2_000_000_000), (2_000_000_100, 2_000_000_100, 2_000_000_100))   # a valid box far from every stream here

# The preconditioned boxes (int32 coordinates of the stream), chosen from the oracle's exact batch boxes:
#   synth      the 600 000-point synthetic tile, 10 batches: the box covers its north-east, batch 9 whole
#   clustered  five Gaussian clusters, Morton-sorted, 5 batches: the box holds the centre cluster (batch 1) whole
BOXES = {
    "synth": ((500_000, 640_000, 0), (1_000_000, 1_000_000, 70_000)),
    "clustered": ((470_000, 480_000, 20_000), (520_000, 530_000, 40_000)),
}


def las_for(lo, hi, scale=0.001):
    las = P.LasInfo()
    for k in range(3):
        las.scale[k] = scale; las.offset[k] = 0.0; las.min[k] = lo[k] * scale; las.max[k] = hi[k] * scale
    return las


@functools.lru_cache(maxsize=None)
def stream(name: str):
    """The .huffman image (something with the buffer protocol) of a named stream."""
    if name == "synth":
        return scenes.synth_stream(600_000)[0].view()
    if name == "clustered":                             # as tests/test_gpu_decode.py::test_batches_that_fall_apart_into_clusters
        rng = np.random.default_rng(77)
        n = 300_000
        centres = np.array([[50_000, 60_000, 2_000], [900_000, 80_000, 9_000], [120_000, 950_000, 4_000], [880_000, 900_000, 1_000], [500_000, 500_000, 30_000]])
        which = rng.integers(0, len(centres), n)
        xyz = centres[which] + rng.normal(0, [6_000, 6_000, 800], (n, 3))
        x, y, z = (np.clip(xyz[:, k], 0, 1_000_000).astype(np.int32) for k in range(3))
        c = rng.integers(0, 1 << 24, n, dtype=np.int64).astype(np.uint32)
        return _keep(P.encode_points(x, y, z, c, las_for((0, 0, 0), (1_000_000, 1_000_000, 40_000)), morton_sort=True, nthreads=2)[0])
    if name == "garbage_tail":                          # as test_reference_default_stream_equals_the_oracle_garbage_included
        x, y, z, c = P.synth_points(300_000, scenes.SEED, 0, 300_000)
        return _keep(P.encode_points(x, y, z, c, P.synth_las_info(300_000), morton_sort=False, pad_tails=False, nthreads=2)[0])
    if name == "escape_heavy":                          # as test_escape_heavy_stream
        x, y, z, c, las = scenes.random_points(131072, seed=3)
        return _keep(P.encode_points(x, y, z, c, las, morton_sort=True, nthreads=2)[0])
    if name in ("wide30", "wide20"):                    # as test_wide_table_values
        hop_bits = int(name[4:])
        rng = np.random.default_rng(21)
        n = 65536 * 2
        hop = np.where(np.arange(n) % 2 == 0, 0, 1 << hop_bits).astype(np.int64)
        x = (hop + rng.integers(0, 3, n)).astype(np.int32)
        y = rng.integers(0, 2000, n).astype(np.int32)
        z = rng.integers(0, 50, n).astype(np.int32)
        c = rng.integers(0, 1 << 24, n).astype(np.uint32)
        return _keep(P.encode_points(x, y, z, c, las_for((0, 0, 0), (1 << 30, 2000, 50)), morton_sort=False, nthreads=2)[0])
    raise KeyError(name)


_alive = []


def _keep(native):
    _alive.append(native)                               # the view borrows the encoder's buffer
    return native.view()


def oracle_points(of, b):
    return of.decode_batch(b).reshape(PPB, 3)


def oracle_bounds(of, first=0, count=None):
    """int32 [n, 6]: min xyz, max xyz over the oracle's 65 536 points of every batch."""
    count = of.num_batches - first if count is None else count
    out = np.empty((count, 6), np.int32)
    for i in range(count):
        p = oracle_points(of, first + i)
        out[i, :3], out[i, 3:] = p.min(axis=0), p.max(axis=0)
    return out


def classify(bounds, box):
    """Class of every batch box against the query: OUTSIDE (disjoint), INSIDE (contained), else STRADDLING; all OUTSIDE for an
    empty query."""
    lo, hi = np.asarray(box[0], np.int64), np.asarray(box[1], np.int64)
    b = np.asarray(bounds, np.int64)
    if (lo > hi).any():
        return np.full(len(b), OUTSIDE)
    disjoint = ((b[:, 3:] < lo) | (b[:, :3] > hi)).any(axis=1)
    within = ((b[:, :3] >= lo) & (b[:, 3:] <= hi)).all(axis=1)
    return np.where(disjoint, OUTSIDE, np.where(within, INSIDE, STRADDLING))


def class_counts(cls):
    return {"batches_outside": int((cls == OUTSIDE).sum()), "batches_inside": int((cls == INSIDE).sum()),
            "batches_straddling": int((cls == STRADDLING).sum())}


def in_box(xyz, box):
    """Boolean mask of the rows of an integer [n, 3] array inside the box (bounds inclusive)."""
    lo, hi = np.asarray(box[0], np.int64), np.asarray(box[1], np.int64)
    xyz = np.asarray(xyz, np.int64)
    return ((xyz >= lo) & (xyz <= hi)).all(axis=1)


def float_box_as_integers(g):
    """A batch record's single-precision box in the stream's integer coordinates, rounded outwards (the most it could cover)."""
    sc, off = (g.scale_x, g.scale_y, g.scale_z), (g.offset_x, g.offset_y, g.offset_z)
    lo = [int(np.floor((float(v) - o) / s)) for v, s, o in zip((g.min_x, g.min_y, g.min_z), sc, off)]
    hi = [int(np.ceil((float(v) - o) / s)) for v, s, o in zip((g.max_x, g.max_y, g.max_z), sc, off)]
    return lo, hi
