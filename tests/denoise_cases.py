"""Cases and the numpy side of the voxel-denoising tests (tests/test_denoise_cpu.py checks on the CPU, against the oracle's decoder,
that the cases do what tests/test_gpu_denoise.py needs them to do). The streams, clips and lattices are those of tests/thin_cases.py.
Inputs and reference arithmetic only."""
from __future__ import annotations

import numpy as np

from tests import select_cases as S
from tests import thin_cases as T

PPB = T.PPB
KEEP, ISOLATED = 0, 1                               # PCR_DENOISE_KEEP / PCR_DENOISE_ISOLATED
KEY_BITS = T.KEY_BITS
HUGE = 1 << 40                                      # a max_count no call reaches: everything is isolated
STREAMS, ORIGINS, WIDE30_LOW = T.STREAMS, T.ORIGINS, T.WIDE30_LOW
stream, header_clip, middle_clip, clip_for, case_clip, xyz_of, candidates = (T.stream, T.header_clip, T.middle_clip, T.clip_for, T.case_clip,
                                                                             T.xyz_of, T.candidates)
count_runs, decoded_batches, table_slots = T.count_runs, T.decoded_batches, T.table_slots

# Every stream runs all of these (tests/test_gpu_denoise.py), each without a clip and with the stream's clip: (cell, origin index).
# 1 counts exact duplicates and the lattice neighbours only; 64 and 2048 take the shift, 1000 the multiply-high division; with 2^30
# all points share a handful of voxels.
COMBOS = [(1, 0), (64, 2), (1000, 1), (2048, 0), (1 << 30, 2)]

# The preconditioned cases: (stream, cell, max_count, clip -- None, "stream" for clip_for()'s, or a box), origin (0, 0, 0), and the
# properties each has to show at least once (see properties()). Chosen from the oracle's decode; the counts it gave are in the
# docstring of tests/test_denoise_cpu.py.
CASES = [
    ("synth", 2048, 23, None, ("neighbour_decides", "other_batch_decides")),
    ("synth", 7001, 262, None, ("neighbour_decides", "other_batch_decides")),
    ("synth", 1000, 6, "stream", ("neighbour_decides", "other_batch_decides")),
    ("plateau", 64, 2, None, ("neighbour_decides", "other_batch_decides")),
    ("wide30", 1, 5, WIDE30_LOW, ("neighbour_decides", "other_batch_decides")),
    ("clustered", 1000, 6, None, ("other_batch_decides",)),
    ("garbage_tail", 2048, 23, "stream", ()),       # here for the tail artefact the clip keeps out, not for its neighbours
]
PROPERTIES = ("neighbour_decides", "other_batch_decides")


def analyse(xyz, vox, clip=None):
    """What a denoising call over the rows `xyz` (int [n, 3], in row order) counts, whatever max_count: a dict of
      rows   the candidates' rows, int64, increasing
      own    per candidate: the candidates in its own voxel
      n27    per candidate: the candidates in the 27 voxels around its own (N27)
      vown / vn27  the same per non-empty voxel
    Voxels by int64 floor_divide, np.unique with counts, then 27 searchsorted lookups of the shifted keys. The voxel indices are
    taken relative to the least one less 1 on every axis, so that a neighbour's index is >= 0; they have to fit 21 bits each
    (the calls the library accepts do: lattice_refusal)."""
    m = candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    empty = np.zeros(0, np.int64)
    if len(rows) == 0:
        return dict(rows=rows, own=empty, n27=empty, vown=empty, vn27=empty)
    org, cell = np.array(vox[:3], np.int64), int(vox[3])
    v = np.floor_divide(np.asarray(xyz, np.int64)[m] - org, cell)
    v = v - v.min(axis=0) + 1
    assert int(v.max()) + 1 < 1 << KEY_BITS, "the voxels of the candidates do not fit the key"
    key = v[:, 0] | (v[:, 1] << KEY_BITS) | (v[:, 2] << (2 * KEY_BITS))
    uniq, inv, vown = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    vown = vown.astype(np.int64)
    vn27 = np.zeros(len(uniq), np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                other = uniq + dx + dy * (1 << KEY_BITS) + dz * (1 << (2 * KEY_BITS))
                at = np.minimum(np.searchsorted(uniq, other), len(uniq) - 1)
                vn27 += np.where(uniq[at] == other, vown[at], 0)
    return dict(rows=rows, own=vown[inv], n27=vn27[inv], vown=vown, vn27=vn27)


def select(an, max_count: int, mode: int = KEEP):
    """The rows pcr_denoise writes, from analyse()'s dict: isolated iff N27 <= max_count."""
    isolated = an["n27"] <= max_count
    return an["rows"][isolated if mode == ISOLATED else ~isolated]


def reference(xyz, vox, max_count, clip=None, mode=KEEP):
    return select(analyse(xyz, vox, clip), max_count, mode)


def median_n27(an) -> int:
    """The median of N27 over the candidates (the upper one of an even number): an exact integer; 0 without candidates."""
    n = an["n27"]
    return int(np.sort(n)[len(n) // 2]) if len(n) else 0


def voxel_stats(an, max_count: int):
    """(voxels, voxels_isolated, points_isolated) of pcr_denoise_stats."""
    iso = an["vn27"] <= max_count
    return len(an["vown"]), int(iso.sum()), int(an["vown"][iso].sum())


def lattice_refusal(bounds, vox, clip=None):
    """What pcr_denoise says about the lattice: T.lattice_refusal with the two voxels more the neighbours need on every axis
    (refused when extent / cell + 4 > 2^21)."""
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
        if extent // int(vox[3]) + 4 > 1 << KEY_BITS:
            return "voxels"
    return None


def properties(xyz, vox, max_count, clip=None):
    """The counts tests/test_denoise_cpu.py asserts, over the rows `xyz` of a whole stream:
      isolated / candidates
      neighbour_decides    rows whose own voxel holds <= max_count candidates but whose N27 exceeds it: only the neighbours'
                           counts keep them
      other_batch_decides  rows that would be isolated counting only the candidates of their own batch but are not over the range:
                           the table has to sum over workgroups"""
    an = analyse(xyz, vox, clip)
    iso = an["n27"] <= max_count
    out = dict(isolated=int(iso.sum()), candidates=len(iso), neighbour_decides=int(((an["own"] <= max_count) & ~iso).sum()), other_batch_decides=0)
    for b in range(len(xyz) // PPB):
        alone = analyse(xyz[b * PPB:(b + 1) * PPB], vox, clip)
        mine = (an["rows"] >> 16) == b
        assert np.array_equal(alone["rows"] + b * PPB, an["rows"][mine])
        out["other_batch_decides"] += int(((alone["n27"] <= max_count) & ~iso[mine]).sum())
    return out
