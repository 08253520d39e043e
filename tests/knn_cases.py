"""Cases and the numpy side of the k-nearest-neighbour tests (tests/test_knn_cpu.py checks on the CPU, against a plain loop over
every pair and the oracle's decoder, that the reference is right and that the cases do what tests/test_gpu_knn.py needs them to
do). The streams, clips and run counting are those of tests/neighbors_cases.py, with one constructed one-batch stream of its own,
`knn_edges`. Inputs and reference arithmetic only.

The contract the reference restates: of the rows pcr_decode_points writes for the range that lie inside the clip (the candidates),
the neighbours of p are the candidates q of another row with d2(p, q) <= r * r; ordered by (d2, row) the first k of them are
knn(p), each a word d2 << 32 | row, NONE behind the last one found."""
from __future__ import annotations

import functools

import numpy as np

from tests import adversarial_cases as A
from tests import neighbors_cases as NC

PPB = NC.PPB
MAX_K, MAX_RADIUS = 16, 32767                       # PCR_KNN_MAX_K / PCR_KNN_MAX_RADIUS
NONE = np.uint64((1 << 64) - 1)                     # PCR_KNN_NONE
KEY_BITS = NC.KEY_BITS
PAIR_CHUNK = 2_000_000                              # pairs of distinct points expanded at a time
KS = (1, 3, 8, 16)                                  # the k values of the constructed stream's calls


def word(d2, row):
    return (np.asarray(d2).astype(np.uint64) << np.uint64(32)) | np.asarray(row).astype(np.uint64)


def analyse(xyz, k, r, clip=None):
    """What a call over the rows `xyz` (int [n, 3], in row order) with k and radius r finds, whatever min_found: a dict of
      rows   the candidates' rows, int64, increasing
      knn    per candidate its k words, uint64 [n, k]: d2 << 32 | row ascending, NONE behind the last one found
      found  per candidate the number of words that are not NONE: min(k, N - 1)
      n      per candidate pcr_neighbors' N (itself included)
      voxels, max_voxel_points, pairs_bound   as neighbors_cases.analyse has them
      pairs, expanded   the pairs of distinct points tested, and the (distinct centre, neighbour row) entries expanded from them
    neighbors_cases.analyse's join (distinct points bucketed by voxel key, 27 searchsorted joins, int64 distances); the rows of a
    distinct point are cut to its k + 1 lowest before a pair is expanded: no other row of it can be among the first k + 1 entries
    of anybody's list, and with the centre's own row taken out of those k + 1 at least k are left. So per distinct point the first
    k + 1 entries of (d2, row) order over ALL candidates, own rows included, are kept (one lexsort per chunk of pairs), and a
    candidate's list is its distinct point's without its own row."""
    k, r = int(k), int(r)
    m = NC.candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    if len(rows) == 0:
        return dict(rows=rows, knn=np.zeros((0, k), np.uint64), found=np.zeros(0, np.int64), n=np.zeros(0, np.int64), voxels=0, max_voxel_points=0,
                    pairs_bound=0, pairs=0, expanded=0)
    uniq, inv, w = np.unique(np.asarray(xyz, np.int64)[m], axis=0, return_inverse=True, return_counts=True)
    inv, w = inv.reshape(-1), w.astype(np.int64)
    # the rows of every distinct point, ascending: by_point[start[u] : start[u] + w[u]]
    by_point = rows[np.argsort(inv, kind="stable")]
    start = np.cumsum(w) - w
    v = np.floor_divide(uniq, r)
    v = v - v.min(axis=0) + 1
    assert int(v.max()) + 1 < 1 << KEY_BITS, "the voxels of the candidates do not fit the key"
    key = v[:, 0] | (v[:, 1] << KEY_BITS) | (v[:, 2] << (2 * KEY_BITS))
    order = np.argsort(key, kind="stable")
    pts, wts, key, start = uniq[order], w[order], key[order], start[order]
    cut = np.minimum(wts, k + 1)
    at_sorted = np.empty(len(order), np.int64)
    at_sorted[order] = np.arange(len(order))
    vkeys, vstart, vlen = np.unique(key, return_index=True, return_counts=True)
    vweight = np.add.reduceat(wts, vstart)
    vid = np.repeat(np.arange(len(vkeys)), vlen)
    n = np.zeros(len(pts), np.int64)
    lists = np.full((len(pts), k + 1), NONE, np.uint64)         # per distinct point: the first k + 1 words over all candidates
    vn27 = np.zeros(len(vkeys), np.int64)
    r2, pairs, expanded = r * r, 0, 0
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
                    pairs += total
                    # the inside pairs, each expanded to the neighbour's k + 1 lowest rows
                    ii, jj, d2 = ii[inside], jj[inside], d2[inside]
                    if len(ii):
                        e = cut[jj]
                        tot = int(e.sum())
                        off = np.arange(tot) - np.repeat(np.cumsum(e) - e, e)
                        ci = np.repeat(ii, e)
                        words = word(np.repeat(d2, e), by_point[np.repeat(start[jj], e) + off])
                        expanded += tot
                        o = np.lexsort((words, ci))
                        ci, words = ci[o], words[o]
                        new = np.ones(len(ci), bool)
                        new[1:] = ci[1:] != ci[:-1]
                        head = np.nonzero(new)[0]
                        rank = np.arange(len(ci)) - np.repeat(head, np.diff(np.append(head, len(ci))))
                        keep = rank <= k
                        who = ci[head]                                      # the distinct centres of this chunk, each once
                        slot = np.cumsum(new) - 1
                        fresh = np.full((len(who), k + 1), NONE, np.uint64)
                        fresh[slot[keep], rank[keep]] = words[keep]
                        lists[who] = np.sort(np.concatenate([lists[who], fresh], axis=1), axis=1)[:, :k + 1]
                    a = b
    back = at_sorted[inv]
    mine = lists[back]                                                      # [candidates, k + 1]
    mine[mine == rows.astype(np.uint64)[:, None]] = NONE                    # the own row: d2 == 0, so the word is the row
    knn = np.ascontiguousarray(np.sort(mine, axis=1)[:, :k])
    found = (knn != NONE).sum(axis=1).astype(np.int64)
    return dict(rows=rows, knn=knn, found=found, n=n[back], voxels=len(vkeys), max_voxel_points=int(vweight.max()),
                pairs_bound=int((vweight * vn27).sum()), pairs=pairs, expanded=expanded)


def select(an, min_found: int):
    """The indices into analyse()'s per-candidate arrays of the candidates pcr_knn writes: found >= min_found."""
    return np.nonzero(an["found"] >= min_found)[0]


def stats(an, runs: int, batches: int, decoded: int, min_found: int):
    """pcr_neighbors_stats of the call: neighbors_cases.stats with points_sparse = the candidates with found < min_found."""
    st = NC.stats(an, runs, batches, decoded, NC.ALL, 0)
    if len(an["rows"]):
        st["points_sparse"] = int((an["found"] < min_found).sum())
        st["points_written"] = len(select(an, min_found))
    return st


def split(words):
    """(rows, d2) of an array of words as Context.knn returns them: int64, -1 for NONE."""
    words = np.asarray(words, np.uint64)
    none = words == NONE
    return (np.where(none, -1, (words & np.uint64(0xFFFFFFFF)).astype(np.int64)), np.where(none, -1, (words >> np.uint64(32)).astype(np.int64)))


def by_every_pair(xyz, k, r, clip=None):
    """(rows, knn) straight from the definition, over every pair of the candidates: for small inputs."""
    m = NC.candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    p = np.asarray(xyz, np.int64)[m]
    d = p[:, None, :] - p[None, :, :]
    d2 = (d * d).sum(axis=2)
    ok = (d2 <= int(r) * int(r)) & ~np.eye(len(p), dtype=bool)
    words = np.where(ok, word(d2, np.broadcast_to(rows[None, :], d2.shape)), NONE)
    words = np.sort(words, axis=1)[:, :k]
    if words.shape[1] < k:
        words = np.concatenate([words, np.full((len(p), k - words.shape[1]), NONE, np.uint64)], axis=1)
    return rows, np.ascontiguousarray(words)


# ---- knn_edges: one batch of 65 536 given rows --------------------------------------------------------------------------------------
R_BIG, R_SMALL = 32767, 64                          # the radii of the two families of calls
SLOT = 8 * R_BIG                                    # groups sit on the x axis, this far apart (a multiple of 32767: (a)'s voxels are adjacent)
WRAP = ((0, 0, 0), (65533, 628, 0))                 # (a): adjacent voxels at r = 32767; d2 = 4 294 968 473 = 2^32 + 1177
EDGE_IN, EDGE_OUT = A.MOMENTS_OUTSIDE[0:1] + (0, 0), A.MOMENTS_OUTSIDE     # (b): (32767, 0, 0) at exactly r, (32767, 1, 0) outside
GRID_SIDE, GRID_STEP = 9, 16                        # (c)
DUPLICATES = (1, 2, MAX_K, MAX_K + 1, MAX_K + 2, 40)   # (d): copies per group
LONE = (1, 2, 17, 63, 64, 65, 129)                  # (e): distinct points of voxels without a neighbour
CROWD, CROWD_AROUND = 65, 30                        # (e): a voxel of 65 with seven neighbour voxels of 30 each
FAR_COPIES = 19000                                  # 3.61e8 pairs among them
FAR = (0, 40 * SLOT, 0)
CLUSTERS, CLUSTER_POINTS, CLUSTER_BOX = 2000, 16, 48
FIELD_STEP = 4 * R_BIG                              # the sites of the filler: further apart than 3 r


@functools.lru_cache(maxsize=None)
def edges_plan():
    """The groups of `knn_edges`: a dict name -> int64 [n, 3] in the order the groups were laid out (before the shuffle)."""
    rng = np.random.default_rng(1616)
    out, slot = {}, [0]

    def base():
        b = np.array([slot[0] * SLOT, 0, 0], np.int64)
        slot[0] += 1
        return b

    out["wrap"] = base() + np.array(WRAP, np.int64)
    out["radius_edge"] = base() + np.array([(0, 0, 0), EDGE_IN, EDGE_OUT], np.int64)
    g = np.arange(GRID_SIDE) * GRID_STEP
    x, y, z = (a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij"))
    out["ties"] = base() + np.stack([x, y, z], axis=1)
    for copies in DUPLICATES:
        out[f"duplicates {copies}"] = np.tile(base() + np.array([7, 9, 11], np.int64), (copies, 1))
    for count in LONE:                              # distinct sites of one voxel of 64, whose min corner is a multiple of 64
        b = base()
        b = b - b % R_SMALL + R_SMALL               # the voxel's min corner
        sites = rng.permutation(R_SMALL ** 3)[:count]
        out[f"lone {count}"] = b + np.stack([sites % R_SMALL, sites // R_SMALL % R_SMALL, sites // (R_SMALL * R_SMALL)], axis=1)
    b = base()
    b = b - b % R_SMALL + R_SMALL
    crowd = [b + rng.integers(0, R_SMALL, (CROWD, 3))]
    for n in range(1, 8):
        d = np.array([n & 1, n >> 1 & 1, n >> 2 & 1], np.int64) * R_SMALL
        crowd.append(b + d + rng.integers(0, R_SMALL, (CROWD_AROUND, 3)))
    out["crowd"] = np.concatenate(crowd)
    b = base()
    b = b - b % R_SMALL + R_SMALL                   # the corner is b + (64, 64, 64); the point lies one unit inside voxel (1, 1, 1)
    corner = b + R_SMALL
    near = []
    for n in range(7):                              # the seven other voxels at the corner: three points each, within 3 of it
        side = np.array([n & 1, n >> 1 & 1, n >> 2 & 1], np.int64)          # 1: the same side as the point
        for t in range(3):
            near.append(corner + np.where(side == 1, t, -1 - t))
    own = [corner + np.array([20 + 3 * t, 20, 20 + t], np.int64) for t in range(10)]
    out["corner"] = np.array([corner + 1] + near + own, np.int64)
    return out


def edges_points():
    plan = edges_plan()
    rng = np.random.default_rng(6464)
    rows = list(plan.values())
    rows.append(np.tile(np.array(FAR, np.int64), (FAR_COPIES, 1)))
    used = sum(len(v) for v in rows)
    left = PPB - used
    assert left > CLUSTERS * CLUSTER_POINTS
    singles = left - CLUSTERS * CLUSTER_POINTS
    sites = np.arange(CLUSTERS + singles)
    at = np.stack([sites % 30, 4 + sites // 30 % 30, sites // 900], axis=1) * FIELD_STEP   # y >= 4 steps: clear of the groups on the x axis
    assert at[:, 1].max() + FIELD_STEP < FAR[1] - 3 * R_BIG
    rows.append(np.repeat(at[:CLUSTERS], CLUSTER_POINTS, axis=0) + rng.integers(0, CLUSTER_BOX, (CLUSTERS * CLUSTER_POINTS, 3)))
    rows.append(at[CLUSTERS:])
    xyz = np.concatenate(rows)
    assert xyz.shape == (PPB, 3) and xyz.min() == 0
    return xyz[rng.permutation(PPB)]                # (a group's rows lie all over the batch: rows, not positions, break the ties)


@functools.lru_cache(maxsize=None)
def points(name: str = "knn_edges"):
    assert name == "knn_edges"
    xyz = np.ascontiguousarray(edges_points(), np.int64)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def stream(name: str = "knn_edges"):
    xyz = points(name)
    return A.encode(xyz, tuple(int(v) + 1 for v in xyz.max(axis=0)))


def rows_of(xyz, group):
    """The rows of `xyz` that hold a point of the plan's group `group` (the groups share no point)."""
    want = np.unique(edges_plan()[group], axis=0)
    xyz = np.asarray(xyz, np.int64)
    hit = np.zeros(len(xyz), bool)
    for p in want:
        hit |= (xyz == p).all(axis=1)
    return np.nonzero(hit)[0]


# The calls of tests/test_gpu_knn.py on knn_edges and what each has to show (tests/test_knn_cpu.py counts every one from the oracle's
# decode): (radius, k values, properties).
CASES = [
    (R_BIG, KS, ("wrap_32_bits", "exactly_r", "one_outside")),
    (R_SMALL, KS, ("tie_at_k", "duplicates_differ", "found_below_k", "tiles_and_buckets", "corner_elsewhere")),
]
PROPERTIES = ("wrap_32_bits", "exactly_r", "one_outside", "tie_at_k", "duplicates_differ", "found_below_k", "tiles_and_buckets", "corner_elsewhere")


def properties(xyz, k, r):
    """The counts tests/test_knn_cpu.py asserts over the decoded rows of knn_edges for a call (k, r):
      wrap_32_bits       ordered pairs of rows in adjacent voxels (cell r) with d2 > r * r whose d2 modulo 2^32 is <= r * r: a 32-bit
                         sum would make them neighbours
      exactly_r          ordered pairs of distinct points with d2 == r * r
      one_outside        ordered pairs of distinct points with d2 == r * r + 1
      tie_at_k           points of the grid (c) with more than k neighbours whose k-th and (k + 1)-th have the same d2: the row decides
      duplicates_differ  groups of exact copies whose lowest and highest row have different lists
      found_below_k      candidates with 0 < found < k, and with found == 0
      tiles_and_buckets  voxels whose 27 buckets hold more than 128 candidates with a bucket boundary that is no multiple of 64
      corner_elsewhere   1 if the corner point's k nearest all lie outside its own voxel, though its voxel holds other points"""
    xyz = np.asarray(xyz, np.int64)
    r2 = r * r
    out = dict.fromkeys(PROPERTIES, 0)
    an = analyse(xyz, k, r)
    more = analyse(xyz, k + 1, r)
    krows, kd2 = split(more["knn"])
    grid = np.isin(more["rows"], rows_of(xyz, "ties"))                      # (counted over the grid of (c) alone: duplicates tie as well)
    out["tie_at_k"] = int((grid & (kd2[:, k] >= 0) & (kd2[:, k] == kd2[:, k - 1])).sum())
    out["found_below_k"] = (int(((an["found"] > 0) & (an["found"] < k)).sum()), int((an["found"] == 0).sum()))
    # the pairs of the small groups, every one against every other (the filler and the far point are further than 3 r from them)
    small = np.concatenate([rows_of(xyz, g) for g in edges_plan()])
    p = xyz[small]
    d = p[:, None, :] - p[None, :, :]
    d2 = (d * d).sum(axis=2)
    v = p // r
    adjacent = (np.abs(v[:, None, :] - v[None, :, :]) <= 1).all(axis=2)
    out["wrap_32_bits"] = int((adjacent & (d2 > r2) & ((d2 & 0xFFFFFFFF) <= r2)).sum())
    out["exactly_r"] = int(((d2 == r2) & (d2 > 0)).sum())
    out["one_outside"] = int((d2 == r2 + 1).sum())
    for copies in DUPLICATES[1:]:
        rr = rows_of(xyz, f"duplicates {copies}")
        lo, hi = np.searchsorted(an["rows"], [rr.min(), rr.max()])
        out["duplicates_differ"] += int(an["knn"][lo].tobytes() != an["knn"][hi].tobytes())
    _, lengths, _ = A.bucket_layout(xyz, r)
    ends = np.cumsum(lengths, axis=1)
    out["tiles_and_buckets"] = int(((ends[:, -1] > 128) & ((ends[:, :-1] % 64 != 0) & (lengths[:, :-1] > 0) & (ends[:, :-1] < ends[:, -1:])).any(axis=1)).sum())
    c = edges_plan()["corner"][0]
    i = int(np.nonzero((xyz == c).all(axis=1))[0][0])
    at = int(np.searchsorted(an["rows"], i))
    nb = split(an["knn"][at])[0]
    nb = nb[nb >= 0]
    own_voxel = ((xyz // r) == (c // r)).all(axis=1)
    out["corner_elsewhere"] = int(len(nb) == k and not own_voxel[nb].any() and own_voxel.sum() > 1)
    return out


# ---- the statistical filter's scene (tests/test_gpu_knn_cli.py): a planar grid and five strays -------------------------------------------
SOR_SIDE, SOR_STEP, SOR_OFF = 60, 10, 300
SOR_K, SOR_MULT, SOR_R = 8, 2.0, 320                # the radius, in lattice steps, reaches a stray's nearest grid points (300.08 away)
SOR_FAR = (100000, 100000, 100000)                  # the rest of the batch: copies of one point outside SOR_BOX
SOR_BOX = ((0, 0, 0), (2000, 2000, 2000))           # the clip of the calls: the scene and nothing else


def sor_points():
    """60 x 60 grid points of spacing 10 on z = 1000 and five strays 300 units above or below it, as distinct points int64 [3605, 3]."""
    g = np.arange(SOR_SIDE) * SOR_STEP + 1000
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    grid = np.stack([x, y, np.full(len(x), 1000)], axis=1)
    strays = np.array([(1105, 1105, 1000 + SOR_OFF), (1105, 1485, 1000 + SOR_OFF), (1485, 1105, 1000 + SOR_OFF), (1485, 1485, 1000 + SOR_OFF),
                       (1295, 1295, 1000 - SOR_OFF)], np.int64)    # (further than the radius from each other)
    return np.concatenate([grid, strays]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def sor_rows():
    """65 536 rows: the scene in a shuffled order among copies of SOR_FAR, which lies outside SOR_BOX: with that clip the scene's
    3605 points are the call's candidates (padding inside the clip would be tens of thousands of points at mean distance 0)."""
    pts = sor_points()
    xyz = np.concatenate([pts, np.tile(np.array(SOR_FAR, np.int64), (PPB - len(pts), 1))])
    xyz = xyz[np.random.default_rng(60).permutation(PPB)]
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def sor_stream():
    xyz = sor_rows()
    return A.encode(xyz, tuple(int(v) + 1 for v in xyz.max(axis=0)))
