"""Cases and the numpy side of the local-moments tests (tests/test_moments_cpu.py checks on the CPU, against the oracle's decoder and
a plain loop, that the reference is right and that the cases do what tests/test_gpu_moments.py needs them to do). The streams,
radii and clips are those of tests/neighbors_cases.py, with two one-batch streams of their own: `facets` (planes, a line, a single
point and a pair, whose covariances decouple exactly) and `ball` (65 536 points that all see each other, closed form). Inputs and
reference arithmetic only."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import neighbors_cases as NC
from tests import select_cases as S

PPB = NC.PPB
MAX_RADIUS = 32767                                  # PCR_MOMENTS_MAX_RADIUS
KEY_BITS = NC.KEY_BITS
HUGE = NC.HUGE
PAIR_CHUNK = 8_000_000                              # pairs expanded at a time
STREAMS, RADII, WIDE30_LOW = NC.STREAMS, NC.RADII, NC.WIDE30_LOW
clip_for, case_clip, xyz_of, candidates = NC.clip_for, NC.case_clip, NC.xyz_of, NC.candidates
decoded_batches, count_runs, lattice_refusal, median_n = NC.decoded_batches, NC.count_runs, NC.lattice_refusal, NC.median_n
OWN = ("facets", "ball")                            # the streams built here
FACETS_R, BALL_R = 50, 32767
PRODUCTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # q: xx, xy, xz, yy, yz, zz
EPS = 2.0 ** -52
TOL_FLOOR = 64 * EPS


def analyse(xyz, r, clip=None, exactly_r=None):
    """neighbors_cases.analyse's join, which additionally reduces per centre w * d and w * d_a * d_b in int64, d = neighbour -
    centre: its dict (rows, n, nn2, n27, voxels, max_voxel_points, pairs_bound, pairs) and
      s    per candidate the sum of d over the candidates within r, int64 [n, 3]
      q    per candidate the sums of d_a * d_b for xx, xy, xz, yy, yz, zz, int64 [n, 6]"""
    r = int(r)
    m = candidates(xyz, clip)
    rows = np.nonzero(m)[0].astype(np.int64)
    empty = np.zeros(0, np.int64)
    if len(rows) == 0:
        return dict(rows=rows, n=empty, nn2=np.zeros(0, np.uint64), n27=empty, voxels=0, max_voxel_points=0, pairs_bound=0, pairs=0,
                    s=np.zeros((0, 3), np.int64), q=np.zeros((0, 6), np.int64))
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
    s = np.zeros((len(pts), 3), np.int64)
    q = np.zeros((len(pts), 6), np.int64)
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
                    d = pts[jj] - pts[ii]                                   # neighbour minus centre
                    d2 = (d * d).sum(axis=1)
                    inside = d2 <= r2
                    wd = np.where(inside, wts[jj], 0)
                    n[centre[a:b]] += np.add.reduceat(wd, seg)
                    for k in range(3):
                        s[centre[a:b], k] += np.add.reduceat(wd * d[:, k], seg)
                    for k, (p0, p1) in enumerate(PRODUCTS):
                        q[centre[a:b], k] += np.add.reduceat(wd * d[:, p0] * d[:, p1], seg)
                    least = np.minimum.reduceat(np.where(inside & (d2 > 0), d2, np.iinfo(np.int64).max), seg)
                    best[centre[a:b]] = np.minimum(best[centre[a:b]], least)
                    pairs += total
                    exact += int((d2 == r2).sum())
                    a = b
    if exactly_r is not None:
        exactly_r.append(exact)
    nn2 = np.where(wts >= 2, 0, best).astype(np.uint64)
    nn2[(wts < 2) & (best == np.iinfo(np.int64).max)] = NC.NONE
    back = at_sorted[inv]
    return dict(rows=rows, n=n[back], nn2=nn2[back], n27=vn27[vid][back], voxels=len(vkeys), max_voxel_points=int(vweight.max()),
                pairs_bound=int((vweight * vn27).sum()), pairs=pairs, s=s[back], q=q[back])


def records(an, at=None):
    """analyse()'s n, s and q as pcr_moments records (MOMENTS_DTYPE), all of them or those at the indices `at`."""
    at = np.arange(len(an["n"])) if at is None else at
    out = np.zeros(len(at), P.MOMENTS_DTYPE)
    out["n"], out["s"], out["q"] = an["n"][at], an["s"][at], an["q"][at]
    return out


def written(an, min_count: int):
    """The indices into analyse()'s per-candidate arrays of the candidates pcr_local_moments writes: n >= min_count."""
    return np.nonzero(an["n"] >= min_count)[0]


def stats(an, runs: int, batches: int, decoded: int, min_count: int):
    """pcr_neighbors_stats of a pcr_local_moments call: points_sparse = the candidates with n < min_count."""
    return NC.stats(an, runs, batches, decoded, NC.KEEP, min_count)


# ---- the streams ---------------------------------------------------------------------------------------------------------------
SIDE = 100                                          # points per side of a facets patch
HORIZONTAL_Z, WALL_X, OBLIQUE_C = 1000, 5000, 14000
LINE_START, LINE_STEP, LINE_POINTS = (12000, 2000, 2000), (1, 2, 3), 500
SINGLE, PAIR = (100, 100, 100), ((100, 3000, 100), (130, 3000, 100))
ANCHOR = (19000, 19000, 19000)                     # the last point given: the encoder pads the batch with copies of it


def facets_points():
    """The distinct points of `facets`, int64 [n, 3]: patches further apart than FACETS_R, all on lattice sites."""
    i, j = (v.reshape(-1) for v in np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij"))
    horizontal = np.stack([2000 + 10 * i, 2000 + 10 * j, np.full(len(i), HORIZONTAL_Z)], axis=1)
    wall = np.stack([np.full(len(i), WALL_X), 2000 + 10 * i, 2000 + 10 * j], axis=1)
    x, y = 8000 + 10 * i, 2000 + 10 * j
    oblique = np.stack([x, y, OBLIQUE_C - x - y], axis=1)
    k = np.arange(LINE_POINTS)[:, None]
    line = np.array(LINE_START)[None, :] + k * np.array(LINE_STEP)[None, :]
    # (a patch with tens of thousands of copies of one point beside it would lose its small eigenvalues to the cancellation in
    # q / n - m * m: the copies get a place of their own, where the covariance is the zero matrix)
    return np.concatenate([horizontal, wall, oblique, line, np.array([SINGLE]), np.array(PAIR), np.array([ANCHOR])]).astype(np.int64)


def facets_classes(xyz):
    """Boolean masks over rows of `facets` by where they lie: horizontal, wall, oblique, line, single, pair, padding (the anchor
    and its copies). Every row of the stream is in exactly one."""
    xyz = np.asarray(xyz, np.int64)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    start, step = np.array(LINE_START), np.array(LINE_STEP)
    k = x - start[0]
    out = dict(horizontal=(z == HORIZONTAL_Z) & (x >= 2000) & (x < 2000 + 10 * SIDE),
               wall=x == WALL_X,
               oblique=(x >= 8000) & (x < 8000 + 10 * SIDE) & (x + y + z == OBLIQUE_C),
               line=(k >= 0) & (k < LINE_POINTS) & (y == start[1] + k * step[1]) & (z == start[2] + k * step[2]),
               single=(xyz == np.array(SINGLE)).all(axis=1),
               pair=(xyz == np.array(PAIR[0])).all(axis=1) | (xyz == np.array(PAIR[1])).all(axis=1),
               padding=(xyz == np.array(ANCHOR)).all(axis=1))
    assert (sum(v.astype(int) for v in out.values()) == 1).all(), "a row of facets is in no class or in two"
    return out


def ball_points():
    """65 536 distinct points in a cube of side 18 000 at the origin's corner: its diagonal is below BALL_R and it lies in one
    voxel of cell BALL_R, so every point sees all of them."""
    rng = np.random.default_rng(11)
    flat = rng.choice(18000 ** 3, PPB, replace=False)
    return np.stack([flat % 18000, flat // 18000 % 18000, flat // 18000 ** 2], axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def stream(name: str):
    """The .huffman image of a named stream: neighbors_cases' and the two built here (one batch each, Morton-sorted, with padded
    tails: they decode to exactly the points given and copies of the last one)."""
    if name not in OWN:
        return NC.stream(name)
    xyz = facets_points() if name == "facets" else ball_points()
    rng = np.random.default_rng(3)
    c = rng.integers(0, 1 << 24, len(xyz)).astype(np.uint32)
    x, y, z = (np.ascontiguousarray(xyz[:, k].astype(np.int32)) for k in range(3))
    return S._keep(P.encode_points(x, y, z, c, S.las_for((0, 0, 0), (20000, 20000, 20000)), morton_sort=True, nthreads=2, pad_tails=True)[0])


def closed_form(xyz):
    """The moments of every row of `xyz` when every row sees all of them, from the global sums in Python integers:
    S_p = sum(q) - N p, Q_p = sum(q q^T) - p sum(q)^T - sum(q) p^T + N p p^T. MOMENTS_DTYPE."""
    p = np.asarray(xyz, np.int64).astype(object)
    count = len(p)
    total = [sum(p[:, a].tolist()) for a in range(3)]
    total2 = {(a, b): sum((p[:, a] * p[:, b]).tolist()) for a, b in PRODUCTS}
    out = np.zeros(count, P.MOMENTS_DTYPE)
    out["n"] = count
    for a in range(3):
        v = total[a] - count * p[:, a]
        assert max(abs(int(t)) for t in v) < 1 << 62
        out["s"][:, a] = v.astype(np.int64)
    for k, (a, b) in enumerate(PRODUCTS):
        v = total2[(a, b)] - p[:, a] * total[b] - total[a] * p[:, b] + count * p[:, a] * p[:, b]
        assert max(abs(int(t)) for t in v) < 1 << 62
        out["q"][:, k] = v.astype(np.int64)
    return out


# ---- the eigen record ----------------------------------------------------------------------------------------------------------
def jacobi(cov):
    """pcr_moments_eigen's solver restated in numpy over matrices [n, 3, 3] (float64, every operation rounded once): cyclic
    Jacobi, pivots (0,1), (0,2), (1,2), a zero off-diagonal skipped, at most 12 sweeps; the eigenvalues ascending, ties keep the
    lower axis first; the eigenvector of value[0] with the sign rule. Returns (values [n, 3], normal [n, 3], sweeps that still
    rotated something)."""
    cov = np.asarray(cov, np.float64)
    count = len(cov)
    a = {(i, j): cov[:, i, j].copy() for i in range(3) for j in range(i, 3)}
    v = [[np.full(count, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(12):
            if not ((a[0, 1] != 0) | (a[0, 2] != 0) | (a[1, 2] != 0)).any():
                break
            sweeps += 1
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
                on = a[p, q] != 0
                apq = np.where(on, a[p, q], 1.0)
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                tau = s / (1.0 + c)
                h = t * apq
                a[p, p] = np.where(on, a[p, p] - h, a[p, p])
                a[q, q] = np.where(on, a[q, q] + h, a[q, q])
                a[p, q] = np.where(on, 0.0, a[p, q])
                g, k = a[rp], a[rq]
                a[rp] = np.where(on, g - s * (k + g * tau), g)
                a[rq] = np.where(on, k + s * (g - k * tau), k)
                for i in range(3):
                    vp, vq = v[i][p], v[i][q]
                    v[i][p] = np.where(on, vp - s * (vq + vp * tau), vp)
                    v[i][q] = np.where(on, vq + s * (vp - vq * tau), vq)
    diag = np.stack([a[0, 0], a[1, 1], a[2, 2]], axis=1)
    least = np.argmin(diag, axis=1)                                         # (the first of equal ones)
    normal = np.stack([np.choose(least, v[i]) for i in range(3)], axis=1)
    nx, ny, nz = normal[:, 0], normal[:, 1], normal[:, 2]
    flip = (nz < 0) | ((nz == 0) & ((ny < 0) | ((ny == 0) & (nx < 0))))
    normal = np.where(flip[:, None], -normal, normal) + 0.0
    return np.sort(diag, axis=1) + 0.0, normal, sweeps


def eigen_reference(moments):
    """The EIGEN_DTYPE records of MOMENTS_DTYPE records by the definition: covariance_from_moments and jacobi(); zeros for n <= 0."""
    m = np.asarray(moments)
    values, normal, _ = jacobi(P.covariance_from_moments(m))
    out = np.zeros(len(m), P.EIGEN_DTYPE)
    ok = m["n"] > 0
    out["value"][ok], out["normal"][ok] = values[ok], normal[ok]
    return out


def residuals(cov, values, normal):
    """Per matrix: scale = max |C_ab|, | |normal|^2 - 1 | and max |C normal - value[0] normal| / scale (0 where scale is 0)."""
    cov = np.asarray(cov, np.float64)
    scale = np.abs(cov).reshape(len(cov), 9).max(axis=1)
    unit = np.abs((normal * normal).sum(axis=1) - 1.0)
    res = np.abs(np.einsum("nij,nj->ni", cov, normal) - values[:, :1] * normal).max(axis=1)
    return scale, unit, np.where(scale > 0, res / np.where(scale > 0, scale, 1.0), 0.0)


def sign_rule(normal):
    nx, ny, nz = normal[:, 0], normal[:, 1], normal[:, 2]
    return (nz > 0) | ((nz == 0) & ((ny > 0) | ((ny == 0) & (nx > 0))))


def measured_tolerance(cov):
    """The tolerance of the eigen properties for the matrices `cov` (those with scale > 0): 16 times the worst of | |normal|^2 -
    1 | and max |C normal - value[0] normal| / scale that numpy.linalg.eigh leaves on the same matrices, at least 64 * 2^-52.
    Returns (tol, numpy's worst)."""
    cov = np.asarray(cov, np.float64)
    if len(cov) == 0:
        return TOL_FLOOR, 0.0
    w, vec = np.linalg.eigh(cov)
    _, unit, res = residuals(cov, w, vec[:, :, 0])
    worst = float(max(unit.max(), res.max()))
    return max(16.0 * worst, TOL_FLOOR), worst


def check_eigen(moments, eigen, what=""):
    """The eigen properties of tests/test_gpu_moments.py's case 4 on every record; returns (tol, numpy's worst, the worst of
    `eigen`), the worsts in units of 2^-52."""
    m, e = np.asarray(moments), np.asarray(eigen)
    assert len(m) == len(e)
    values, normal = e["value"], e["normal"]
    assert np.isfinite(values).all() and np.isfinite(normal).all(), f"a NaN or Inf {what}"
    dead = m["n"] <= 0
    assert (values[dead] == 0).all() and (normal[dead] == 0).all(), f"n <= 0 does not give zeros {what}"
    cov = P.covariance_from_moments(m)
    scale, unit, res = residuals(cov, values, normal)
    flat = ~dead & (scale == 0)
    assert (values[flat] == 0).all() and (normal[flat] == np.array([1.0, 0.0, 0.0])).all(), f"the zero matrix does not give 0 and (1, 0, 0) {what}"
    live = ~dead & (scale > 0)
    if not live.any():
        return TOL_FLOOR, 0.0, 0.0
    tol, worst_numpy = measured_tolerance(cov[live])
    v, sc = values[live], scale[live]
    assert (v[:, 0] <= v[:, 1]).all() and (v[:, 1] <= v[:, 2]).all(), f"the eigenvalues are not ascending {what}"
    want = np.linalg.eigvalsh(cov[live])
    off = np.abs(v - want).max(axis=1) / sc
    assert off.max() <= tol, f"an eigenvalue is off by {off.max() / EPS:.1f} * 2^-52 of the scale, tol {tol / EPS:.1f} {what}"
    assert unit[live].max() <= tol, f"|normal|^2 - 1 is {unit[live].max() / EPS:.1f} * 2^-52, tol {tol / EPS:.1f} {what}"
    assert res[live].max() <= tol, f"C normal - value[0] normal is {res[live].max() / EPS:.1f} * 2^-52 of the scale, tol {tol / EPS:.1f} {what}"
    assert sign_rule(normal[live]).all(), f"the sign rule is broken {what}"
    return tol, worst_numpy / EPS, float(max(unit[live].max(), res[live].max())) / EPS


def handmade():
    """Hand-made pcr_moments records for pcr_moments_eigen (MOMENTS_DTYPE) with what each is there for."""
    big = 1 << 61
    rows = [
        ("n = 0", 0, (5, 6, 7), (100, 1, 2, 100, 3, 100)),
        ("n = -1", -1, (5, 6, 7), (100, 1, 2, 100, 3, 100)),
        ("diagonal, tie of x and z below y", 1, (0, 0, 0), (4, 0, 0, 9, 0, 4)),
        ("diagonal, tie of y and z below x", 1, (0, 0, 0), (9, 0, 0, 4, 0, 4)),
        ("diagonal, descending", 1, (0, 0, 0), (9, 0, 0, 4, 0, 1)),
        ("k * identity", 2, (0, 0, 0), (14, 0, 0, 14, 0, 14)),
        ("the zero matrix", 1, (0, 0, 0), (0, 0, 0, 0, 0, 0)),
        ("q near 2^62 with n = 2^32", 1 << 32, (1 << 40, -(1 << 41), 1 << 39), ((1 << 62) - 12345, 1 << 60, -(1 << 59), (1 << 62) - 999, 1 << 58, (1 << 61) + 7)),
        ("one off-diagonal of 1 against diagonals near 2^61", 1, (0, 0, 0), (big, 1, 0, 3, 0, big - 5)),
        ("an off-diagonal of 1 against one huge diagonal", 1, (0, 0, 0), (big, 0, 1, 2, 1, 1)),
        ("a general matrix", 7, (3, -2, 5), (70, 11, -13, 50, 17, 90)),
    ]
    out = np.zeros(len(rows), P.MOMENTS_DTYPE)
    for k, (_, count, s, q) in enumerate(rows):
        out["n"][k], out["s"][k], out["q"][k] = count, s, q
    return out, [r[0] for r in rows]
