"""Cases and the numpy side of the radius-neighbourhood tests (tests/test_neighbors_cpu.py checks on the CPU, against the oracle's
decoder and a plain loop, that the reference is right and that the cases do what tests/test_gpu_neighbors.py needs them to do).
The streams, clips and run counting are those of tests/thin_cases.py. Inputs and reference arithmetic only."""
from __future__ import annotations

import numpy as np

from tests import denoise_cases as D
from tests import thin_cases as T

PPB = T.PPB
ALL, KEEP, SPARSE = 0, 1, 2                         # PCR_NEIGHBORS_ALL / _KEEP / _SPARSE
MAX_RADIUS = 1 << 20                                # PCR_NEIGHBORS_MAX_RADIUS
NONE = np.uint64((1 << 64) - 1)                     # PCR_NN2_NONE
KEY_BITS = T.KEY_BITS
HUGE = 1 << 40                                      # a min_count no call reaches: everything is sparse
PAIR_CHUNK = 20_000_000                             # pairs expanded at a time
STREAMS, WIDE30_LOW = T.STREAMS, T.WIDE30_LOW
stream, header_clip, clip_for, case_clip, xyz_of, candidates = T.stream, T.header_clip, T.clip_for, T.case_clip, T.xyz_of, T.candidates
decoded_batches, table_slots = T.decoded_batches, T.table_slots

# Two radii per stream (tests/test_gpu_neighbors.py runs each without a clip and with the stream's clip): chosen from the oracle's
# decode so that the reference expands fewer than 3e7 pairs of distinct points (tests/test_neighbors_cpu.py asserts it) and so
# that, where the stream allows it, the median N is above 1. wide30 without a clip is refused at every radius.
RADII = {
    "synth": (700, 2500), "clustered": (150, 400), "escape_heavy": (64, 2000), "wide30": (1, 2), "garbage_tail": (300, 1000),
    "plateau": (30, 100), "config1": (100, 400), "ref_packed_batch": (100, 400), "ref_packed_lowentropy": (100, 400),
    "ref_packed_bc7": (100, 400),
}

# The preconditioned cases: (stream, radius, clip -- None, "stream" for clip_for()'s, or a box, needs). min_count is the median of
# N (the upper one). The counts the oracle's decode gave are in the docstring of tests/test_neighbors_cpu.py.
CASES = [
    ("clustered", 400, None, ("sphere_decides", "other_batch_decides", "exactly_r")),
    ("wide30", 2, WIDE30_LOW, ("sphere_decides", "other_batch_decides", "exactly_r", "nn2_zero", "no_neighbour")),
    ("wide30", 1, WIDE30_LOW, ("exactly_r",)),
    ("synth", 2500, None, ("sphere_decides", "no_neighbour")),
    ("plateau", 100, None, ("sphere_decides",)),
    ("garbage_tail", 1000, "stream", ()),           # here for the tail artefact the clip keeps out
]
PROPERTIES = ("sphere_decides", "other_batch_decides", "exactly_r", "nn2_zero", "no_neighbour")


def count_runs(xyz, r, clip=None):
    return T.count_runs(xyz, (0, 0, 0, int(r)), clip)


def lattice_refusal(bounds, r, clip=None):
    """What pcr_neighbors says about the lattice: denoise_cases' with cell = r, origin (0, 0, 0)."""
    return D.lattice_refusal(bounds, (0, 0, 0, int(r)), clip)


def analyse(xyz, r, clip=None, exactly_r=None):
    """What a call over the rows `xyz` (int [n, 3], in row order) with radius r finds, whatever min_count: a dict of
      rows   the candidates' rows, int64, increasing
      n      per candidate N: the candidates q with d2(p, q) <= r * r, itself included (int64)
      nn2    per candidate: the least d2 <= r * r to a candidate of another row, NONE without one (uint64)
      n27    per candidate: the candidates in the 27 voxels (cell = r) around its own
      voxels, max_voxel_points, pairs_bound (= n27 summed over the candidates), pairs (the pairs of distinct points expanded)
    Exact duplicates are collapsed first and carried as weights; the distinct points are bucketed by voxel key, and for each of the
    27 offsets the buckets are joined by searchsorted and expanded to pairs, PAIR_CHUNK at a time. exactly_r: a list that gets
    the number of ordered pairs of distinct points with d2 == r * r appended."""
    r = int(r)
    m = candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    empty = np.zeros(0, np.int64)
    if len(rows) == 0:
        return dict(rows=rows, n=empty, nn2=np.zeros(0, np.uint64), n27=empty, voxels=0, max_voxel_points=0, pairs_bound=0, pairs=0)
    uniq, inv, w = np.unique(np.asarray(xyz, np.int64)[m], axis=0, return_inverse=True, return_counts=True)
    inv, w = inv.reshape(-1), w.astype(np.int64)
    v = np.floor_divide(uniq, r)
    v = v - v.min(axis=0) + 1
    assert int(v.max()) + 1 < 1 << KEY_BITS, "the voxels of the candidates do not fit the key"
    key = v[:, 0] | (v[:, 1] << KEY_BITS) | (v[:, 2] << (2 * KEY_BITS))
    order = np.argsort(key, kind="stable")
    pts, wts, key = uniq[order], w[order], key[order]
    at_sorted = np.empty(len(order), np.int64)
    at_sorted[order] = np.arange(len(order))
    vkeys, vstart, vlen = np.unique(key, return_index=True, return_counts=True)
    vweight = np.add.reduceat(wts, vstart)
    vid = np.repeat(np.arange(len(vkeys)), vlen)
    n = np.zeros(len(pts), np.int64)
    best = np.full(len(pts), np.iinfo(np.int64).max)
    vn27 = np.zeros(len(vkeys), np.int64)
    r2, pairs, exact = r * r, 0, 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                other = vkeys + dx + dy * (1 << KEY_BITS) + dz * (1 << (2 * KEY_BITS))
                at = np.minimum(np.searchsorted(vkeys, other), len(vkeys) - 1)
                hit = vkeys[at] == other
                vn27 += np.where(hit, vweight[at], 0)
                centre = np.nonzero(hit[vid])[0]
                first, cnt = vstart[at][vid[centre]], vlen[at][vid[centre]]
                cum = np.cumsum(cnt)
                a = 0
                while a < len(centre):
                    b = max(a + 1, int(np.searchsorted(cum, (cum[a - 1] if a else 0) + PAIR_CHUNK, side="right")))
                    c = cnt[a:b]
                    total = int(c.sum())
                    seg = np.cumsum(c) - c                                  # every centre's pairs are one stretch (c >= 1)
                    ii = np.repeat(centre[a:b], c)
                    jj = np.repeat(first[a:b] - seg, c) + np.arange(total)
                    d = pts[ii] - pts[jj]
                    d2 = (d * d).sum(axis=1)
                    inside = d2 <= r2
                    n[centre[a:b]] += np.add.reduceat(np.where(inside, wts[jj], 0), seg)
                    least = np.minimum.reduceat(np.where(inside & (d2 > 0), d2, np.iinfo(np.int64).max), seg)
                    best[centre[a:b]] = np.minimum(best[centre[a:b]], least)
                    pairs += total
                    exact += int((d2 == r2).sum())
                    a = b
    if exactly_r is not None:
        exactly_r.append(exact)
    nn2 = np.where(wts >= 2, 0, best).astype(np.uint64)
    nn2[(wts < 2) & (best == np.iinfo(np.int64).max)] = NONE
    back = at_sorted[inv]
    return dict(rows=rows, n=n[back], nn2=nn2[back], n27=vn27[vid][back], voxels=len(vkeys), max_voxel_points=int(vweight.max()),
                pairs_bound=int((vweight * vn27).sum()), pairs=pairs)


def select(an, mode: int, min_count: int):
    """The indices into analyse()'s per-candidate arrays of the candidates pcr_neighbors writes: sparse iff N < min_count."""
    sparse = an["n"] < min_count
    return np.nonzero(np.ones(len(sparse), bool) if mode == ALL else sparse if mode == SPARSE else ~sparse)[0]


def median_n(an) -> int:
    """The median of N over the candidates (the upper one of an even number): an exact integer; 0 without candidates."""
    n = an["n"]
    return int(np.sort(n)[len(n) // 2]) if len(n) else 0


def stats(an, runs: int, batches: int, decoded: int, mode: int, min_count: int):
    """pcr_neighbors_stats of the call."""
    if len(an["rows"]) == 0:
        return dict(batches_outside=batches - decoded, batches_decoded=decoded, points_considered=0, runs=0, voxels=0, table_slots=0, max_voxel_points=0,
                    pairs_bound=0, points_sparse=0, points_written=0)
    return dict(batches_outside=batches - decoded, batches_decoded=decoded, points_considered=len(an["rows"]), runs=runs, voxels=an["voxels"],
                table_slots=table_slots(runs), max_voxel_points=an["max_voxel_points"], pairs_bound=an["pairs_bound"],
                points_sparse=int((an["n"] < min_count).sum()), points_written=len(select(an, mode, min_count)))


def properties(xyz, r, clip=None):
    """The counts tests/test_neighbors_cpu.py asserts, over the rows `xyz` of a whole stream, at min_count = the median of N:
      sparse / candidates / median
      sphere_decides       candidates sparse by the sphere but not by the 27-voxel count (N < median <= N27)
      other_batch_decides  candidates that are not sparse but would be with the candidates of their own batch alone
      exactly_r            ordered pairs of distinct points with d2 == r * r: they test the <=
      nn2_zero             candidates with an exact duplicate
      no_neighbour         candidates with nn2 = NONE"""
    exact = []
    an = analyse(xyz, r, clip, exact)
    k = median_n(an)
    sparse = an["n"] < k
    out = dict(sparse=int(sparse.sum()), candidates=len(sparse), median=k, pairs=an["pairs"], sphere_decides=int((sparse & (an["n27"] >= k)).sum()),
               other_batch_decides=0, exactly_r=exact[0], nn2_zero=int((an["nn2"] == 0).sum()), no_neighbour=int((an["nn2"] == NONE).sum()))
    for b in range(len(xyz) // PPB):
        alone = analyse(xyz[b * PPB:(b + 1) * PPB], r, clip)
        mine = (an["rows"] >> 16) == b
        assert np.array_equal(alone["rows"] + b * PPB, an["rows"][mine])
        out["other_batch_decides"] += int(((alone["n"] < k) & ~sparse[mine]).sum())
    return out
