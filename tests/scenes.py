"""Seeded synthetic streams and cameras shared by the tests (inputs only — no expectations here)."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P

SEED = 0x5EED


@functools.lru_cache(maxsize=8)
def synth_stream(total_points: int, seed: int = SEED, chunk_points: int = 0):
    """(.huffman image as NativeBytes, encoder stats) of the whole synthetic scene of `total_points`."""
    return P.synth_encode(total_points, seed, chunk_points=chunk_points, nthreads=4)


def cameras(width: int, height: int) -> dict:
    """Cameras over the 1 km synthetic tile (world units = metres, las_min = 0)."""
    c = {
        # whole tile in view, every batch far away -> float path, LOD floor
        "overview": P.camera_orbit(-0.15, -0.57, 1500.0, (500.0, 500.0, 40.0), width, height),
        # near the surface: big projected batches -> double path, npr up to 64, heavy overdraw, partial cull
        "closeup": P.camera_orbit(-1.68, -0.39, 70.0, (300.0, 20.0, 45.0), width, height),
        # looking along the strip from inside: w <= 0 points, frustum-straddling batches
        "inside": P.camera_orbit(0.9, -0.05, 5.0, (400.0, 10.0, 48.0), width, height),
        # far away: every batch small on screen -> float path, LOD between the floor and 64
        "far": P.camera_orbit(0.4, -0.9, 6000.0, (500.0, 500.0, 40.0), width, height),
    }
    return c


def with_flags(p: P.RenderParams, lod_percent=None, cull=None, show_num_points=None, colorize_chunks=None):
    q = p.copy()
    if lod_percent is not None:
        q.lod_percent = lod_percent
    if cull is not None:
        q.enable_frustum_culling = int(cull)
    if show_num_points is not None:
        q.show_num_points = int(show_num_points)
    if colorize_chunks is not None:
        q.colorize_chunks = int(colorize_chunks)
    return q


def random_points(n: int, seed: int, spread: int = 1 << 20):
    """Unstructured points with wide deltas: many escapes, large symbols, negative coordinates."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-spread, spread, n, dtype=np.int64).astype(np.int32)
    y = rng.integers(-spread, spread, n, dtype=np.int64).astype(np.int32)
    z = (rng.normal(0, spread / 64, n)).astype(np.int32)
    c = rng.integers(0, 1 << 24, n, dtype=np.int64).astype(np.uint32)
    las = P.LasInfo()
    for k in range(3):
        las.scale[k] = 0.001
        las.offset[k] = 100.0
        las.min[k] = 100.0 - spread * 0.001
        las.max[k] = 100.0 + spread * 0.001
    return x, y, z, c, las


# ---- constructed scenes for tests/test_gpu_contention.py and tests/test_contention_cpu.py ------------------------------
def lattice_las(lo, hi, scale=0.001) -> P.LasInfo:
    """LasInfo of integer lattice points in [lo, hi] per axis: offset 0, so world = lattice * scale and the renderers see
    (lattice - lo) * scale."""
    las = P.LasInfo()
    for k in range(3):
        las.scale[k] = scale
        las.offset[k] = 0.0
        las.min[k] = lo[k] * scale
        las.max[k] = hi[k] * scale
    return las


def straight_down(radius: float, target, width: int, height: int, **kw) -> P.RenderParams:
    """A camera looking straight down at `target`: the w row of its transform is [0, 6e-17, -1, d], so w depends on z alone and
    points of equal z have equal depth bits. LOD 100, no culling: every point of the stream is walked."""
    return with_flags(P.camera_orbit(0.0, -np.pi / 2, radius, target, width, height, **kw), lod_percent=100, cull=0)


TIE_PLANES_Z = (50_000, 49_100, 48_900, 45_000)


def tie_planes(seed: int = 11, n: int = 4 * 65536):
    """Lattice points on four horizontal planes with random colours, 200 m x 200 m at 1 mm: under tie_planes_camera() thousands of
    pixels hold several points of exactly the same depth and different colours. The top plane has a checkerboard of holes, so
    ties are decided on every plane that shows through."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 200_000, n).astype(np.int32)
    y = rng.integers(0, 200_000, n).astype(np.int32)
    layer = rng.integers(0, 4, n)
    z = np.asarray(TIE_PLANES_Z, np.int32)[layer]
    hole = ((x // 20_000 + y // 20_000) % 2 == 0) & (layer == 0)
    z[hole] = TIE_PLANES_Z[1]
    c = rng.integers(0, 1 << 24, n).astype(np.uint32)
    return x, y, z, c, lattice_las((0, 0, 0), (200_000, 200_000, 50_000))


def tie_planes_camera(width: int, height: int) -> P.RenderParams:
    return straight_down(100.0, (100.0, 100.0, 50.0), width, height)


def tie_clusters(seed: int = 77, n: int = 5 * 65536):
    """The clustered cloud of test_batches_that_fall_apart_into_clusters_get_a_window_per_run (batches made of clusters far
    apart: a window per run of chains, chains that straddle a jump on the global path) with z snapped to planes 0.5 m apart, for
    tie_clusters_camera(). Encode with morton_sort=False: the points come ordered by cluster and 8 m tile, and runs of 2048 of
    them (32 chains) are dealt out to the batches in turn, so every batch has a part of every cluster and the tied points of
    one pixel come from different runs, workgroups and batches."""
    rng = np.random.default_rng(seed)
    centres = np.array([[50_000, 60_000, 2_000], [900_000, 80_000, 9_000], [120_000, 950_000, 4_000], [880_000, 900_000, 1_000], [500_000, 500_000, 30_000]])
    which = rng.integers(0, len(centres), n)
    xyz = centres[which] + rng.normal(0, [6_000, 6_000, 800], (n, 3))
    x, y = (np.clip(xyz[:, k], 0, 1_000_000).astype(np.int32) for k in range(2))
    z = (np.clip(xyz[:, 2], 0, 40_000) // 500 * 500).astype(np.int32)
    c = rng.integers(0, 1 << 24, n, dtype=np.int64).astype(np.uint32)
    tiles = np.argsort((which * 1024 + y // 8_000) * 1024 + x // 8_000, kind="stable")
    nb = n // 65536
    order = tiles.reshape(-1, nb, 2048).transpose(1, 0, 2).reshape(-1)         # run r of the sorted points -> batch r % nb
    return x[order], y[order], z[order], c[order], lattice_las((0, 0, 0), (1_000_000, 1_000_000, 40_000))


def tie_clusters_camera(width: int, height: int) -> P.RenderParams:
    return straight_down(1200.0, (500.0, 500.0, 20.0), width, height)


def hqs_edge(seed: int = 5, n: int = 4 * 65536, scale: float = 0.001, radius: float = 10000.0, extent: int = 2_000_000, outliers: bool = False):
    """Two thin layers whose depths under straight_down(radius, target, ...) straddle the 1 % test of the HQS colour pass within a few dozen ulps:
    the top layer at w ~ radius (z random within +-32 lattice steps), the lower one 1 % of the radius below it (+-64 steps,
    raised by 32: a pixel's depth is the nearest of its many top points, 32 steps above their plane, and about half of the
    lower points pass against it); one lattice step is about one f32 ulp of w (scale 1e-3 at w ~ 1e4, scale 1e-5 at w ~ 150).
    Encode with pad_tails=True: the garbage points of unpadded chain tails lie metres above the top layer and would
    set the depth of every pixel. outliers: the first two points of every 65 536 are moved to opposite corners of a square 16
    times as wide, far outside the view -- the 10-10-10 method takes batches in input order and picks its precision by the size of
    their boxes, and 20-bit coordinates (steps finer than an ulp of w) need a box of 500 pixels. Returns the points and the
    camera's target."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, extent, n).astype(np.int32)
    y = rng.integers(0, extent, n).astype(np.int32)
    top = rng.integers(0, 2, n) == 0
    ztop = 50_000
    zlow = ztop - int(round(0.01 * radius / scale)) + 32
    z = np.where(top, ztop + rng.integers(-32, 33, n), zlow + rng.integers(-64, 65, n)).astype(np.int32)
    c = rng.integers(0, 1 << 24, n).astype(np.uint32)
    lo, hi = 0, extent
    if outliers:
        lo, hi = -8 * extent + extent // 2, 8 * extent + extent // 2
        x[0::65536] = y[0::65536] = lo
        x[1::65536] = y[1::65536] = hi
    las = lattice_las((lo, lo, int(z.min())), (hi, hi, int(z.max())), scale)
    target = ((extent / 2 - lo) * scale, (extent / 2 - lo) * scale, (ztop - int(z.min())) * scale)
    return x, y, z, c, las, target


def one_pixel(batches: int = 3, seed: int = 3):
    """`batches` x 65 536 pure white points in a 20 m x 20 m x 2 m box: under one_pixel_camera() all of them fall into one pixel
    and pass the 1 % test, so every accumulator of the colour pass runs to its stated bound (64 x 255 per chain, 65 536 x 255 per
    batch and 32-bit half)."""
    rng = np.random.default_rng(seed)
    n = batches * 65536
    x = rng.integers(0, 20_000, n).astype(np.int32)
    y = rng.integers(0, 20_000, n).astype(np.int32)
    z = rng.integers(0, 2_000, n).astype(np.int32)
    c = np.full(n, 0xFFFFFF, np.uint32)
    return x, y, z, c, lattice_las((0, 0, 0), (20_000, 20_000, 2_000))


def one_pixel_camera(width: int = 65, height: int = 37, target=(10.0, 10.0, 1.0)) -> P.RenderParams:
    return with_flags(P.camera_orbit(0.3, -0.8, 20000.0, target, width, height), lod_percent=100, cull=0)
