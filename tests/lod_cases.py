"""Lattices, cases and the numpy side of the level-of-detail tests (tests/test_lod_cpu.py checks on the CPU, against the oracle's
decoder, that the cases do what tests/test_gpu_lod.py needs them to do). Inputs and reference arithmetic only.

A lod is (origin x, y, z, finest cell, levels); level l (0 = coarsest) is the thinning lattice (origin, cell << (levels - 1 - l))."""
from __future__ import annotations

import numpy as np

from tests import select_cases as S
from tests import thin_cases as T

PPB = S.PPB
MAX_LEVELS = 16                                     # PCR_LOD_MAX_LEVELS
DROP_REST, ROW_ORDER = 1, 2                         # PCR_LOD_DROP_REST / PCR_LOD_ROW_ORDER
NO_LEVEL = 0xFF                                     # levels(): a row that is no candidate
KEY_BITS = T.KEY_BITS

# (stream, origin, finest cell, levels, clip -- None, "stream" for thin_cases.clip_for()'s, or a box) and what the case has to
# show (see properties()). Chosen from the oracle's decode; the counts it printed are in tests/test_lod_cpu.py's docstring.
CASES = [
    ("synth", T.ORIGINS[0], 500, 6, None, ("all_levels", "rest", "several_batches", "level0_everywhere")),
    ("synth", T.ORIGINS[1], 64, 12, None, ("climbs5", "several_batches")),
    ("clustered", T.ORIGINS[0], 125, 8, None, ("several_batches", "level0_everywhere")),
    ("garbage_tail", T.ORIGINS[0], 875, 4, "stream", ("uniform_chain", "several_batches")),
    ("plateau", T.ORIGINS[0], 1, 7, None, ("uniform_chain", "no_rest", "batch_without_a_level", "several_batches")),
    ("wide30", T.ORIGINS[0], 1, 3, T.WIDE30_LOW, ("several_batches", "level0_everywhere")),
]
PROPERTIES = ("all_levels", "rest", "no_rest", "several_batches", "level0_everywhere", "uniform_chain", "batch_without_a_level", "climbs5")
GOLDEN_LOD = (0, 0, 0, 64, 5)                       # the four golden streams run this one, with thin_cases.middle_clip


def cell_of(lod, l: int) -> int:
    return int(lod[3]) << (int(lod[4]) - 1 - l)


def vox_of(lod, l: int):
    """The thinning lattice of level l"""
    return (int(lod[0]), int(lod[1]), int(lod[2]), cell_of(lod, l))


def levels(xyz, lod, clip=None):
    """Per row of `xyz` (int [n, 3], in row order) its level as uint8: by floor_divide and the first occurrence of every voxel per
    level, from the finest level up, so that the least level at which a row is its voxel's first stays; `levels` for a candidate
    that is first at none, NO_LEVEL for a row outside the clip."""
    L = int(lod[4])
    m = T.candidates(xyz, clip)
    rows = np.nonzero(m)[0]
    out = np.full(len(xyz), NO_LEVEL, np.uint8)
    out[rows] = L
    inside = np.asarray(xyz)[m]
    for l in range(L - 1, -1, -1):
        if len(rows) == 0:
            break
        key, _ = T.voxel_keys(inside, vox_of(lod, l))
        _, idx = np.unique(key, return_index=True)
        out[rows[idx]] = l
    return out


def order(lv, lod, flags=0):
    """The rows a call writes and their levels, in its order, from levels()'s result: the candidates (without the rest under
    DROP_REST) in increasing (level, row) -- a stable sort by level -- or in increasing row order under ROW_ORDER."""
    L = int(lod[4])
    rows = np.nonzero(lv < (L if flags & DROP_REST else L + 1))[0].astype(np.int64)
    if not flags & ROW_ORDER:
        rows = rows[np.argsort(lv[rows], kind="stable")]
    return rows, lv[rows]


def level_counts(lv, lod):
    """pcr_lod_stats::level_count: MAX_LEVELS + 1 numbers, the rest at index `levels`, zeros above"""
    return np.bincount(lv[lv != NO_LEVEL], minlength=MAX_LEVELS + 1)[:MAX_LEVELS + 1].tolist()


def lattice_refusal(bounds, lod, clip=None):
    """What pcr_lod_order says about the lattice: None (accepted; also when the clip is empty or misses every batch), "extent" (q
    spans 2^31 or more on an axis) or "voxels" ((q.max - q.min) / cell + 2^(levels - 1) + 1 > 2^21 there). q = the union of the
    exact boxes of the batches the clip does not miss, intersected with the clip."""
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
        if extent // int(lod[3]) + (1 << (int(lod[4]) - 1)) + 1 > 1 << KEY_BITS:
            return "voxels"
    return None


def table_slots(runs: int) -> int:
    """The slots of the finest level's table: pcr_thin's for the finest cell"""
    return T.table_slots(runs)


def stats(xyz, bounds, lod, clip, flags, lv=None):
    """pcr_lod_stats as a dict, for the rows `xyz` of a range and the exact boxes of its batches"""
    lv = levels(xyz, lod, clip) if lv is None else lv
    counts = level_counts(lv, lod)
    runs = T.count_runs(xyz, vox_of(lod, int(lod[4]) - 1), clip)
    dec = T.decoded_batches(bounds, clip)
    cand = int((lv != NO_LEVEL).sum())
    return dict(batches_outside=len(np.asarray(bounds).reshape(-1, 6)) - dec, batches_decoded=dec, points_considered=cand, runs=runs,
                table_slots=table_slots(runs), points_written=cand - (counts[int(lod[4])] if flags & DROP_REST else 0), level_count=counts)


def properties(lv, lod):
    """The counts tests/test_lod_cpu.py asserts, from levels() over the rows of a whole stream:
      all_levels             1 if every level 0 .. levels - 1 has a row, else 0
      rest / no_rest         the rows of the rest / 1 if there is none
      several_batches        levels whose rows lie in two or more batches
      level0_everywhere      1 if every batch holds a row of level 0
      uniform_chain          chains (64 consecutive rows) whose rows are all candidates of one level
      batch_without_a_level  (batch, level) pairs, the rest included, without a row, in batches that hold a candidate
      climbs5                rows whose level is at least five below the finest: first in their voxel at six levels or more"""
    L = int(lod[4])
    nb = len(lv) // PPB
    per = np.stack([np.bincount(lv[b * PPB:(b + 1) * PPB], minlength=256)[:L + 1] for b in range(nb)])     # [batch, level]
    chains = lv.reshape(-1, 64)
    return dict(all_levels=int((per[:, :L].sum(axis=0) > 0).all()), rest=int(per[:, L].sum()), no_rest=int(per[:, L].sum() == 0),
                several_batches=int(((per > 0).sum(axis=0) >= 2).sum()), level0_everywhere=int((per[:, 0] > 0).all()),
                uniform_chain=int(((chains == chains[:, :1]).all(axis=1) & (chains[:, 0] != NO_LEVEL)).sum()),
                batch_without_a_level=int(((per == 0) & (per.sum(axis=1, keepdims=True) > 0)).sum()),
                climbs5=int((lv <= L - 6).sum()) if L >= 6 else 0)
