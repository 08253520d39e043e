"""Host-side mirror of the reference's plugin surface for the Huffman path, over the C ABI.

The names, call order and error behaviour follow the reference so the parity tests read like a session
of the reference viewer without a window:

    Method   {name, description, group, update(renderer), render(renderer)}     include/Method.h:10-23
    Resource {state, load(renderer), unload(renderer), process(renderer)}        modules/compute/Resources.h:27-35
    HuffmanLasData.create(path)                                                  modules/compute/HuffmanLasLoader.h:87-92
    HuffmanMemIter  ("huffman_mem_iter_cuda")                                    modules/huffman_mem_iter_cuda/huffman_mem_iter_cuda.h
    HuffmanHQS      ("huffman_hqs")                                              modules/huffman_hqs/huffman_hqs.h
    ComputeLasData.create(path) / ComputeLoopLasCUDA ("loop_las_cuda")           modules/compute/ComputeLasLoader.{h,cpp},
                                                                                 modules/compute_loop_las_cuda/compute_loop_las_cuda.h
    ComputeLoopLasHQS ("loop_las_hqs")                                           modules/compute_loop_las_hqs/compute_loop_las_hqs.h
    Runtime.addMethod / setSelectedMethod / resource                             include/Runtime.h:15-55
    Debug.LOD / frustumCullingEnabled / colorizeChunks / showNumPoints           include/Debug.h:14-31

Python here is plumbing only (ctypes calls, byte slicing); all compute is in libpcr_hip.so /
libpcr_host.so. A C++ twin of these adapters lives in csrc/pcr_methods.hpp.
"""
from __future__ import annotations

import ctypes as C
import mmap
import os
import struct
from typing import Iterator, Optional

import numpy as np

from . import _native as N
from ._native import Box, DisplayOpts, EncodeStats, Grid, GridStats, QuantileStats, GroundStats, HeightStats, FileHeader, LasInfo, RenderParams, RenderStats, SelectStats, ComponentsStats, DenoiseStats, NeighborsStats, ThinStats, Lod, LodStats, Voxels, XyzBatch, c_i64, fb_elems

POINTS_PER_BATCH = 65536
ENCODED_PAD_WORDS = 1024
SEPARATE_PAD_WORDS = 256
BATCH_FIXED_HEADER = 124
_BATCH_FIXED = BATCH_FIXED_HEADER + 4 * (3072 + 1024 + 4096 + 4096 + 32)
PCR_COLOR_BYTES = 32768             # BC1: 8 bytes per 16 points


class PcrError(RuntimeError):
    pass


# --------------------------------------------------------------------------------------------------
# native buffers / encoder front-ends (libpcr_host.so)
# --------------------------------------------------------------------------------------------------
class NativeBytes:
    """A malloc'ed byte buffer owned by libpcr_host.so, exposed through the buffer protocol."""

    def __init__(self, ptr: int, length: int):
        self._ptr, self._len = ptr, length
        self._arr = (C.c_uint8 * length).from_address(ptr)

    def __len__(self) -> int:
        return self._len

    def view(self) -> memoryview:
        return memoryview(self._arr).cast("B")

    def free(self) -> None:
        if self._ptr:
            self._arr = None
            N.host_lib().pcr_host_free(C.c_void_p(self._ptr))
            self._ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def synth_encode(total_points: int, seed: int = 0x5EED, first: int = 0, count: Optional[int] = None,
                 chunk_points: int = 0, nthreads: int = 0) -> tuple[NativeBytes, dict]:
    """Generate + encode points [first, first+count) of the synthetic scene -> (.huffman image, stats)."""
    lib = N.host_lib()
    if count is None:
        count = total_points - first
    out, ln, st = C.c_void_p(), C.c_size_t(), EncodeStats()
    rc = lib.pcr_synth_encode(total_points, seed, first, count, chunk_points, nthreads, C.byref(out), C.byref(ln), C.byref(st))
    if rc:
        raise PcrError(f"pcr_synth_encode: {N.host_error()}")
    return NativeBytes(out.value, ln.value), st.as_dict()


def kernel_version() -> str:
    """Version tag of the render/transcode kernels in libpcr_hip.so (pcr_kernel_version): stored measurements name theirs."""
    return N.hip_lib().pcr_kernel_version().decode()


def synth_points(total_points: int, seed: int, first: int, count: int):
    x = np.empty(count, np.int32); y = np.empty(count, np.int32); z = np.empty(count, np.int32)
    c = np.empty(count, np.uint32)
    rc = N.host_lib().pcr_synth_points(total_points, seed, first, count, x.ctypes.data, y.ctypes.data, z.ctypes.data, c.ctypes.data)
    if rc:
        raise PcrError(f"pcr_synth_points: {N.host_error()}")
    return x, y, z, c


def synth_las_info(total_points: int, seed: int = 0x5EED) -> LasInfo:
    las = LasInfo()
    N.host_lib().pcr_synth_las_info(total_points, seed, C.byref(las))
    return las


def encode_points(x, y, z, color, las: LasInfo, morton_sort: bool = True, chunk_points: int = 0,
                  nthreads: int = 0, pad_tails: bool = False, bc7: bool = False) -> tuple[NativeBytes, dict]:
    """`preprocess in.las out.huffman <sort>` on in-memory points (src/preprocess.cpp:1167-1279). pad_tails: the
    PCR_ENCODE_PAD_TAILS variant (not in the reference) whose streams decode without the tail artefact. bc7: colours as BC7
    mode-6 blocks, the file of a reference built with COLOR_COMPRESSION == 7 (PCR_ENCODE_BC7)."""
    x = np.ascontiguousarray(x, np.int32); y = np.ascontiguousarray(y, np.int32); z = np.ascontiguousarray(z, np.int32)
    color = np.ascontiguousarray(color, np.uint32)
    out, ln, st = C.c_void_p(), C.c_size_t(), EncodeStats()
    rc = N.host_lib().pcr_encode_points(x.ctypes.data, y.ctypes.data, z.ctypes.data, color.ctypes.data, len(x), C.byref(las),
                                        int(bool(morton_sort)) | (2 if pad_tails else 0) | (4 if bc7 else 0), chunk_points, nthreads,
                                        C.byref(out), C.byref(ln), C.byref(st))
    if rc:
        raise PcrError(f"pcr_encode_points: {N.host_error()}")
    return NativeBytes(out.value, ln.value), st.as_dict()


def camera_orbit(yaw: float, pitch: float, radius: float, target, width: int, height: int,
                 fovy: float = 60.0, near: float = 0.1, far: float = 200000.0) -> RenderParams:
    """OrbitControls + Camera + the ChangingRenderData setup of HuffmanHQS::render (huffman_hqs.h:157-183)."""
    p = RenderParams()
    t = (C.c_double * 3)(*target)
    rc = N.host_lib().pcr_camera_orbit(yaw, pitch, radius, t, width, height, fovy, near, far, C.byref(p))
    if rc:
        raise PcrError(f"pcr_camera_orbit: {N.host_error()}")
    return p


# --------------------------------------------------------------------------------------------------
# .huffman container (HuffmanLasData::loadHeader, HuffmanLasLoader.h:57-85)
# --------------------------------------------------------------------------------------------------
def las_quantize(x, y, z, color, las: LasInfo, nthreads: int = 0):
    """10-10-10 three-level quantisation of points in input order (pcr_las_quantize): returns
    (batches[nB] XyzBatch array, xyz12, xyz8, xyz4, rgba) with nB*65536 slots each."""
    x, y, z = (np.ascontiguousarray(a, np.int32) for a in (x, y, z))
    color = np.ascontiguousarray(color, np.uint32)
    n = len(x)
    if not (len(y) == len(z) == len(color) == n) or n == 0:
        raise ValueError("x, y, z, color must be non-empty and of equal length")
    nb = (n + POINTS_PER_BATCH - 1) // POINTS_PER_BATCH
    batches = (XyzBatch * nb)()
    arrs = [np.empty(nb * POINTS_PER_BATCH, np.uint32) for _ in range(4)]
    rc = N.host_lib().pcr_las_quantize(x.ctypes.data, y.ctypes.data, z.ctypes.data, color.ctypes.data, n, C.byref(las),
                                       C.addressof(batches), *(a.ctypes.data for a in arrs), nthreads)
    if rc:
        raise PcrError(f"pcr_las_quantize failed: {N.host_error()}")
    return (batches, *arrs)


def read_las(path: str):
    """Minimal LAS 1.x reader for the loaders (header fields and point layout as ComputeLasData::loadHeader reads
    them, modules/compute/ComputeLasLoader.h:55-95, and getPoint, computeLasLoader.cs:147-190): returns
    (x, y, z int32, color 0x00BBGGRR uint32, LasInfo)."""
    with open(path, "rb") as f:
        hdr = f.read(375)
        if len(hdr) < 227 or hdr[:4] != b"LASF":
            raise PcrError(f"{path}: not a LAS file")
        major, minor = hdr[24], hdr[25]
        n = struct.unpack_from("<I", hdr, 107)[0] if (major == 1 and minor < 4) else struct.unpack_from("<Q", hdr, 247)[0]
        n = min(n, 1_000_000_000)                                     # ComputeLasLoader.h:69
        off, fmt, bpp = struct.unpack_from("<I", hdr, 96)[0], hdr[104], struct.unpack_from("<H", hdr, 105)[0]
        las = LasInfo()
        sc = struct.unpack_from("<6d", hdr, 131)
        las.scale[:], las.offset[:] = sc[:3], sc[3:]
        mx_x, mn_x, mx_y, mn_y, mx_z, mn_z = struct.unpack_from("<6d", hdr, 179)
        las.min[:], las.max[:] = (mn_x, mn_y, mn_z), (mx_x, mx_y, mx_z)
        f.seek(off)
        raw = np.frombuffer(f.read(n * bpp), np.uint8)
    if len(raw) != n * bpp:
        raise PcrError(f"{path}: truncated point data")
    raw = raw.reshape(n, bpp)
    xyz = np.ascontiguousarray(raw[:, :12]).view("<i4")
    off_rgb = {2: 20, 3: 28, 7: 30, 8: 30}.get(fmt % 128, 0)         # computeLasLoader.cs:151-160 (0: reads X's bytes)
    rgb = np.ascontiguousarray(raw[:, off_rgb:off_rgb + 6]).view("<u2").astype(np.uint32)
    rgb = np.where(rgb > 255, rgb // 256, rgb)                       # :170-172
    color = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
    return (np.ascontiguousarray(xyz[:, 0]), np.ascontiguousarray(xyz[:, 1]), np.ascontiguousarray(xyz[:, 2]),
            color.astype(np.uint32), las)


POINT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("color", "<u4")])     # pcr_point

HIT_DTYPE = np.dtype([("pixel", "<u4"), ("depth_bits", "<u4"), ("index", "<i8")])          # pcr_screen_hit
MOMENTS_DTYPE = np.dtype([("n", "<i8"), ("s", "<i8", (3,)), ("q", "<i8", (6,))])              # pcr_moments; q: xx, xy, xz, yy, yz, zz
EIGEN_DTYPE = np.dtype([("value", "<f8", (3,)), ("normal", "<f8", (3,))])                   # pcr_eigen
ROW_DTYPE = np.dtype("<i8")                                                                # a row of pcr_thin

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def as_rect(rect):
    """A pcr_rect from a Rect or four numbers x0, y0, x1, y1 (pixels, bounds inclusive); None stays None: the whole image."""
    if rect is None or isinstance(rect, N.Rect):
        return rect
    v = [int(a) for a in np.asarray(rect, dtype=np.int64).reshape(4)]
    if any(a < INT32_MIN or a > INT32_MAX for a in v):
        raise ValueError("rect coordinates are int32")
    return N.Rect(*v)


def as_box(box) -> Box:
    """A pcr_box from a Box, (min xyz, max xyz) or six numbers min x, y, z, max x, y, z (int32, bounds inclusive)."""
    if isinstance(box, Box):
        return box
    v = [int(a) for a in np.asarray(box, dtype=np.int64).reshape(6)]
    if any(a < INT32_MIN or a > INT32_MAX for a in v):
        raise ValueError("box coordinates are int32")
    b = Box()
    b.min[:], b.max[:] = v[:3], v[3:]
    return b


def box_from_world(las: LasInfo, lo, hi) -> Box:
    """The largest int32 box whose points i satisfy lo <= i * scale + offset <= hi on every axis, the expression evaluated in
    float64 exactly as HuffmanLasData.points(world=True) evaluates it (a product rounded, then a sum rounded: monotone in i
    for a positive scale). ceil / floor of the inverse give a guess; it is then moved by evaluating the expression itself
    until the bound and its outer neighbour disagree, so no rounding of the inverse can leak a point in or out. An axis no
    int32 coordinate satisfies makes the box empty (min > max)."""
    import math
    b = Box()
    for k in range(3):
        s, o, l, h = float(las.scale[k]), float(las.offset[k]), float(lo[k]), float(hi[k])
        if not s > 0.0 or math.isnan(o) or math.isnan(l) or math.isnan(h):
            raise ValueError("box_from_world needs a positive scale and numbers for offset and bounds")

        def f(i):
            return float(i) * s + o

        def guess(v, rnd):
            g = (v - o) / s
            return INT32_MIN if g <= INT32_MIN else INT32_MAX if g >= INT32_MAX else int(rnd(g))

        a = guess(l, math.ceil)                             # the smallest i with f(i) >= lo
        while a > INT32_MIN and f(a - 1) >= l:
            a -= 1
        while a <= INT32_MAX and f(a) < l:
            a += 1
        z = guess(h, math.floor)                            # the largest i with f(i) <= hi
        while z < INT32_MAX and f(z + 1) <= h:
            z += 1
        while z >= INT32_MIN and f(z) > h:
            z -= 1
        if a > z:
            a, z = 0, -1
        b.min[k], b.max[k] = a, z
    return b


class Polygon:
    """A polygon prism in the stream's int32 coordinates (pcr_polygon): `rings` is a sequence of rings, each a sequence of at
    least 3 (x, y) vertices (a single ring may be given alone, as an [m, 2] array); the first ring and every further one
    combine by the even-odd rule, so a ring inside another is a hole. A ring is closed implicitly. z_min..z_max is
    inclusive; invert=True keeps the points NOT inside the polygon (the z range still applies). The boundary is half-open
    (include/pcr_types.h): of two polygons that share an edge exactly one takes a point on it. ValueError for a ring of
    fewer than 3 vertices, a coordinate that is not a whole number (nothing is rounded here: polygon_from_world does that) or
    one beyond int32; the limits on the vertex count and the extent are the call's."""

    @staticmethod
    def _ring(r) -> np.ndarray:
        try:
            a = np.asarray(r)
            if a.dtype.kind not in "iu":                    # floats, Python integers beyond int64 (object)
                if a.dtype.kind not in "fO" or not all(float(v) == int(v) for v in a.ravel()):
                    raise ValueError
                a = np.array([int(v) for v in a.ravel()], dtype=object).reshape(a.shape)
            if a.size and (a.min() < INT32_MIN or a.max() > INT32_MAX):
                raise ValueError
            return a.astype(np.int64)
        except (ValueError, TypeError, OverflowError):
            raise ValueError("polygon vertices are whole numbers within int32, (x, y) per vertex") from None

    def __init__(self, rings, z_min: int = INT32_MIN, z_max: int = INT32_MAX, invert: bool = False):
        try:
            single = np.asarray(rings)
        except ValueError:                                  # rings of different lengths
            single = None
        if single is not None and single.ndim == 2 and single.dtype.kind != "O":
            rings = [single]
        self.rings = [self._ring(r) for r in rings]
        if not self.rings or any(r.ndim != 2 or r.shape[1] != 2 or len(r) < 3 for r in self.rings):
            raise ValueError("a polygon is one or more rings of at least 3 (x, y) vertices")
        zs = (int(z_min), int(z_max))
        if zs != (z_min, z_max) or any(v < INT32_MIN or v > INT32_MAX for v in zs):
            raise ValueError("z_min and z_max are whole numbers within int32")
        self.z_min, self.z_max, self.invert = zs[0], zs[1], bool(invert)
        self._xy = np.ascontiguousarray(np.concatenate(self.rings), dtype=np.int32)
        self._sizes = np.array([len(r) for r in self.rings], np.int32)
        self.c = N.Polygon(self._xy.ctypes.data_as(C.POINTER(N.c_i32)), self._sizes.ctypes.data_as(C.POINTER(N.c_i32)), len(self.rings),
                           self.z_min, self.z_max, N.POLY_INVERT if invert else 0, 0)

    def inverted(self) -> "Polygon":
        return Polygon(self.rings, self.z_min, self.z_max, not self.invert)


def polygon_from_world(las: LasInfo, rings, z_lo=None, z_hi=None, invert: bool = False) -> Polygon:
    """The Polygon of rings given in world coordinates. A vertex goes to the nearest lattice step, rint((v - offset) / scale) in
    float64, which moves it by at most half a step (and a few units in the last place of the division): unlike a box, a
    polygon has no largest integer counterpart, since its edges pass between lattice points whichever vertices are chosen.
    z_lo / z_hi (None: unbounded) follow box_from_world's rule: the largest integer range whose points satisfy
    z_lo <= z * scale + offset <= z_hi in float64. ValueError for a vertex that is not a number or lands beyond int32."""
    try:
        single = np.asarray(rings, dtype=np.float64)
    except ValueError:
        single = None
    if single is not None and single.ndim == 2:
        rings = [single]
    s, o = np.array(tuple(las.scale)[:2]), np.array(tuple(las.offset)[:2])
    if not (s > 0.0).all():
        raise ValueError("polygon_from_world needs a positive scale")
    out = []
    for r in rings:
        r = np.asarray(r, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != 2 or len(r) < 3:
            raise ValueError("a polygon is one or more rings of at least 3 (x, y) vertices")
        v = np.rint((r - o) / s)
        if not np.isfinite(v).all() or (v < INT32_MIN).any() or (v > INT32_MAX).any():
            raise ValueError("a polygon vertex lies beyond the int32 lattice of the stream")
        out.append(v.astype(np.int64))
    inf = float("inf")
    zb = box_from_world(las, (-inf, -inf, -inf if z_lo is None else z_lo), (inf, inf, inf if z_hi is None else z_hi))
    return Polygon(out, zb.min[2], zb.max[2], invert)


class Slab:
    """A slab in the stream's int32 coordinates (pcr_slab): the points p with lo <= normal . p <= hi, the form taken in exact
    integers. lo > hi is legal and empty; a bound at -/+SLAB_MAX_BOUND makes a half-space; the zero normal holds every point or
    none. ValueError for a value that is not a whole number, a normal component beyond SLAB_MAX_NORMAL or a bound beyond
    SLAB_MAX_BOUND (nothing is rounded or wrapped here)."""

    def __init__(self, normal, lo, hi):
        try:
            n = tuple(int(v) for v in normal)
            b = (int(lo), int(hi))
            if len(n) != 3 or any(float(a) != float(v) for a, v in zip(n + b, tuple(normal) + (lo, hi))):
                raise ValueError
        except (ValueError, TypeError, OverflowError):
            raise ValueError("a slab is three whole numbers (the normal) and two whole bounds") from None
        if any(abs(v) > N.SLAB_MAX_NORMAL for v in n):
            raise ValueError(f"a normal component beyond {N.SLAB_MAX_NORMAL}")
        if any(abs(v) > N.SLAB_MAX_BOUND for v in b):
            raise ValueError("a bound beyond 2^61")
        self.normal, self.lo, self.hi = n, b[0], b[1]
        self.c = N.Slab((N.c_i32 * 3)(*n), 0, b[0], b[1])

    def __repr__(self):
        return f"Slab({self.normal}, {self.lo}, {self.hi})"


def slab_from_plane(normal, d, tol) -> Slab:
    """The slab |normal . p - d| <= tol: lo = d - tol, hi = d + tol."""
    return Slab(normal, int(d) - int(tol), int(d) + int(tol))


def as_slabs(slabs):
    """A ctypes array of pcr_slab from a sequence of Slab (or one Slab); such an array is passed through."""
    if isinstance(slabs, C.Array) and slabs._type_ is N.Slab:
        return slabs
    if isinstance(slabs, (Slab, N.Slab)):
        slabs = [slabs]
    slabs = list(slabs)
    out = (N.Slab * len(slabs))()
    for k, sl in enumerate(slabs):
        if isinstance(sl, Slab):
            sl = sl.c
        elif not isinstance(sl, N.Slab):
            sl = Slab(*sl).c
        out[k] = sl
    return out


def plane_through(p0, p1, p2):
    """The plane through three integer points as (normal, d) with normal . p = d on it, in Python integers: the cross product of
    the differences divided by its gcd; if a component then exceeds M = SLAB_MAX_NORMAL, every component becomes
    floor((2 * n_a * M + m) / (2 * m)) with m = max |n_a| (the nearest multiple, floor division); the sign such that the first
    non-zero of n[2], n[1], n[0] is positive (pcr_eigen's convention); d = normal . p0 exactly. None for collinear points."""
    import math
    p0, p1, p2 = (tuple(int(v) for v in p) for p in (p0, p1, p2))
    u, v = [p1[k] - p0[k] for k in range(3)], [p2[k] - p0[k] for k in range(3)]
    n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    g = math.gcd(*n)
    if g == 0:
        return None
    n = [a // g for a in n]
    m, M = max(abs(a) for a in n), N.SLAB_MAX_NORMAL
    if m > M:
        n = [(2 * a * M + m) // (2 * m) for a in n]
    lead = next(a for a in (n[2], n[1], n[0]) if a != 0)
    if lead < 0:
        n = [-a for a in n]
    return tuple(n), sum(a * b for a, b in zip(n, p0))


def slab_tolerance(normal, dist) -> int:
    """isqrt(dist^2 * (normal . normal)): the largest whole t with t <= dist * |normal|, so that |normal . p - d| <= t iff the
    point lies within `dist` stream units of the plane (dist a whole number of lattice steps)."""
    import math
    dist = int(dist)
    if dist < 0:
        raise ValueError("a distance is not negative")
    return math.isqrt(dist * dist * sum(int(a) * int(a) for a in normal))


PLANE_REDRAWS = 8


def plane_hypotheses(xyz, count: int, rng):
    """`count` plane hypotheses through triples of the integer points xyz -- one [n, 3] array, or a sequence of them (one per
    batch): the three points of a hypothesis come from the same array, hence from one neighbourhood of the Morton order. Per
    hypothesis: an array (rng.integers), three rows of it (rng.integers), redrawn at most PLANE_REDRAWS times while the points are
    collinear; a hypothesis that stays collinear is left out, so fewer than `count` may come back. Returns (normals int64 [m, 3],
    d int64 [m]) as plane_through gives them. Pure numpy and Python integers; the same rng state gives the same list."""
    groups = [np.asarray(xyz)] if isinstance(xyz, np.ndarray) else [np.asarray(g) for g in xyz]
    groups = [g.reshape(-1, 3) for g in groups if g.size >= 9]
    normals, ds = [], []
    for _ in range(int(count) if groups else 0):
        g = groups[int(rng.integers(0, len(groups)))]
        for _ in range(1 + PLANE_REDRAWS):
            i, j, k = (int(v) for v in rng.integers(0, len(g), 3))
            plane = plane_through(g[i], g[j], g[k])
            if plane is not None:
                normals.append(plane[0]); ds.append(plane[1])
                break
    return np.array(normals, np.int64).reshape(-1, 3), np.array(ds, np.int64)


def slab_from_world(las: LasInfo, point, normal, distance: float) -> Slab:
    """The slab of the points within `distance` world units of the plane through `point` with the normal `normal` (world
    coordinates; any length). In lattice coordinates the form is (nw_a * scale_a) . p: n_a = rint(nw_a * scale_a * k) with
    k = SLAB_MAX_NORMAL / max |nw_a * scale_a|, p = rint((point - offset) / scale), d = n . p exactly, and the tolerance
    floor(distance * |nw| * k) in float64. ValueError for a zero or non-finite normal, a point beyond int32 or a negative distance."""
    import math
    sc, off = [float(v) for v in las.scale], [float(v) for v in las.offset]
    nw, pw = [float(v) for v in normal], [float(v) for v in point]
    w = [a * b for a, b in zip(nw, sc)]
    m = max(abs(a) for a in w)
    if len(nw) != 3 or len(pw) != 3 or not all(math.isfinite(a) for a in w + pw) or not m > 0.0 or not all(a > 0.0 for a in sc):
        raise ValueError("slab_from_world needs a positive scale, a finite point and a finite normal that is not zero")
    distance = float(distance)
    if not distance >= 0.0 or math.isinf(distance):
        raise ValueError("slab_from_world needs a finite distance that is not negative")
    k = float(N.SLAB_MAX_NORMAL) / m
    n = [int(np.rint(a * k)) for a in w]
    p = [float(np.rint((a - o) / s)) for a, o, s in zip(pw, off, sc)]
    if any(a < INT32_MIN or a > INT32_MAX for a in p):
        raise ValueError("the point lies beyond the int32 lattice of the stream")
    d = sum(a * int(b) for a, b in zip(n, p))
    tol = int(math.floor(distance * math.sqrt(sum(a * a for a in nw)) * k))
    return slab_from_plane(n, d, tol)


def fit_planes_rounds(read_batch, support, num_batches: int, tolerance_steps: int, num_planes: int = 1, hypotheses: int = 256, seed: int = 0,
                      min_support: int = 3, clip=None, sample_batches: int = 4):
    """The RANSAC rounds of HuffmanLasData.fit_planes over two callables: read_batch(b) -> integer [65536, 3] points of batch b,
    support(hyp, exclude) -> the number of candidates in every Slab of hyp, the candidates being the points inside the clip and
    in no Slab of exclude. Per round: `sample_batches` batches chosen by numpy.random.default_rng(seed) (rng.choice without
    replacement, sorted), their points that are still candidates (inside `clip`, in no plane found so far), `hypotheses` planes
    through them (plane_hypotheses) with the tolerance slab_tolerance(normal, tolerance_steps), one support call with a
    zero-normal slab appended (it counts every candidate), the hypothesis of greatest support (ties: the lowest index). Stops after
    num_planes planes, when the best support is below min_support or when no hypothesis can be drawn. Returns (slabs, supports,
    candidates): the planes found, their supports and the candidate count of every round made."""
    rng = np.random.default_rng(seed)
    found, supports, candidates = [], [], []
    for _ in range(int(num_planes)):
        pick = np.sort(rng.choice(num_batches, size=min(int(sample_batches), num_batches), replace=False))
        groups = []
        for b in pick:
            g = np.asarray(read_batch(int(b)), np.int64).reshape(-1, 3)
            keep = np.ones(len(g), bool)
            if clip is not None:
                keep &= ((g >= np.array(tuple(clip.min), np.int64)) & (g <= np.array(tuple(clip.max), np.int64))).all(axis=1)
            for sl in found:
                v = g @ np.array(sl.normal, np.int64)
                keep &= ~((v >= sl.lo) & (v <= sl.hi))
            groups.append(g[keep])
        normals, d = plane_hypotheses(groups, hypotheses, rng)
        if len(d) == 0:
            break
        hyp = [slab_from_plane(n, int(dk), slab_tolerance(n, tolerance_steps)) for n, dk in zip(normals.tolist(), d.tolist())]
        counts = np.asarray(support(hyp + [Slab((0, 0, 0), 0, 0)], list(found)), np.int64)
        candidates.append(int(counts[-1]))
        best = int(np.argmax(counts[:-1]))
        if int(counts[best]) < int(min_support):
            break
        found.append(hyp[best]); supports.append(int(counts[best]))
    return found, supports, candidates


def as_grid(grid) -> Grid:
    """A pcr_grid from a Grid or five numbers origin_x, origin_y, cell, width, height (the stream's int32 coordinates, cells)."""
    if isinstance(grid, Grid):
        return grid
    v = [int(a) for a in np.asarray(grid, dtype=np.int64).reshape(5)]
    if any(a < INT32_MIN or a > INT32_MAX for a in v):
        raise ValueError("grid fields are int32")
    return Grid(*v, 0)


def grid_from_world(las: LasInfo, lo_xy, hi_xy, cell_size: float) -> Grid:
    """The grid of square cells of `cell_size` world units that covers lo <= x, y <= hi (world coordinates): the origin is the
    first lattice point at or above lo on each axis (box_from_world's), the cell the whole number of lattice steps cell_size
    is on x and on y, width and height reach the last lattice point at or below hi. ValueError for a cell_size that is not a
    whole number (>= 1) of steps of both the x and the y lattice -- the cells are squares of integer coordinates, so scale_x
    and scale_y have to agree on that number -- or for a range that holds no lattice point."""
    inf = float("inf")
    cells = []
    for k in range(2):
        s = float(las.scale[k])
        if not s > 0.0 or not cell_size > 0.0:
            raise ValueError("grid_from_world needs positive scales and a positive cell size")
        n = round(cell_size / s)
        if n < 1 or n > INT32_MAX or abs(n * s - cell_size) > 1e-9 * cell_size:
            raise ValueError(f"a cell of {cell_size} is not a whole number of lattice steps of {s}")
        cells.append(int(n))
    if cells[0] != cells[1]:
        raise ValueError(f"a cell of {cell_size} is {cells[0]} steps on x and {cells[1]} on y: the cells are squares of lattice steps")
    box = box_from_world(las, (lo_xy[0], lo_xy[1], -inf), (hi_xy[0], hi_xy[1], inf))
    if box.min[0] > box.max[0] or box.min[1] > box.max[1]:
        raise ValueError("the range holds no lattice point")
    w, h = ((int(box.max[k]) - int(box.min[k])) // cells[0] + 1 for k in range(2))
    if w * h > N.GRID_MAX_CELLS:
        raise ValueError(f"{w} x {h} cells: more than the {N.GRID_MAX_CELLS} a grid may have")
    return Grid(int(box.min[0]), int(box.min[1]), cells[0], w, h, 0)


class GroundParams(N.GroundParams):
    """pcr_ground_params: step k of the ground filter opens the surface over the square window of radii[k] cells (1 .. 64) and
    flags the cells it lowers by more than thresholds[k] (the stream's z units, >= 0); at most 16 steps, none: the call only
    fills. fill_rounds (0 .. 4096): the most rounds of the hole fill. The native call checks the ranges."""

    def __init__(self, radii=(), thresholds=(), fill_rounds: int = 4096):
        super().__init__()
        radii, thresholds = [int(r) for r in radii], [int(t) for t in thresholds]
        if len(radii) != len(thresholds):
            raise ValueError("one threshold per radius")
        if any(v < INT32_MIN or v > INT32_MAX for v in radii + thresholds + [int(fill_rounds)]):
            raise ValueError("ground parameters are int32")
        self.num_steps, self.fill_rounds = len(radii), int(fill_rounds)
        for k in range(min(len(radii), N.GROUND_MAX_STEPS)):    # (more than 16 steps: num_steps says so and the call refuses)
            self.radius[k], self.threshold[k] = radii[k], thresholds[k]

    @property
    def radii(self):
        return tuple(self.radius[:min(self.num_steps, N.GROUND_MAX_STEPS)])

    @property
    def thresholds(self):
        return tuple(self.threshold[:min(self.num_steps, N.GROUND_MAX_STEPS)])


def ground_params_from_world(las: LasInfo, cell_size: float, slope: float = 1.0, initial_distance: float = 0.15, max_distance: float = 2.5,
                             max_window: float = 33.0, fill_rounds: int = 4096) -> GroundParams:
    """Zhang et al.'s schedule for a grid of `cell_size` world units: radii 1, 2, 4, ... cells while the window (2 r + 1) *
    cell_size is at most max_window (at least one step, at most 16, r <= 64); with w_k the window of step k in world units the
    elevation thresholds are dh_0 = initial_distance and dh_k = min(max_distance, slope * (w_k - w_(k-1)) + initial_distance),
    turned into the stream's z units by threshold_k = round(dh_k / scale_z)."""
    sz = float(las.scale[2])
    if not sz > 0.0 or not cell_size > 0.0:
        raise ValueError("ground_params_from_world needs a positive z scale and a positive cell size")
    radii = [1]
    while len(radii) < N.GROUND_MAX_STEPS and 2 * radii[-1] <= N.GROUND_MAX_RADIUS and (4 * radii[-1] + 1) * cell_size <= max_window:
        radii.append(2 * radii[-1])
    thresholds, prev = [], None
    for r in radii:
        w = (2 * r + 1) * cell_size
        dh = initial_distance if prev is None else min(max_distance, slope * (w - prev) + initial_distance)
        thresholds.append(min(INT32_MAX, max(0, int(round(dh / sz)))))
        prev = w
    return GroundParams(radii, thresholds, fill_rounds)


def quantile_rank(q, n):
    """The rank Context.grid_quantiles takes from a cell of n >= 1 candidates sorted ascending for q basis points (q <=
    QUANTILE_ONE): (q * (n - 1) + QUANTILE_ONE // 2) // QUANTILE_ONE in unsigned 64-bit integers -- the nearest rank, a half
    rounded up. q and n broadcast; numpy uint64."""
    q, n = np.asarray(q, np.uint64), np.asarray(n, np.uint64)
    one = np.uint64(N.QUANTILE_ONE)
    return (q * (n - np.uint64(1)) + one // np.uint64(2)) // one


def as_quantiles(q) -> np.ndarray:
    """q (basis points, 0 .. QUANTILE_ONE, at most QUANTILES_MAX of them) as the uint32 array the C ABI takes."""
    a = np.atleast_1d(np.asarray(q))
    if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) >= 1 << 32)):
        raise ValueError("q is a sequence of integers in basis points (0 .. 10000)")
    return np.ascontiguousarray(a, np.uint32)


def as_voxels(vox) -> Voxels:
    """A pcr_voxels from a Voxels or four numbers origin x, y, z, cell (the stream's int32 coordinates)."""
    if isinstance(vox, Voxels):
        return vox
    v = [int(a) for a in np.asarray(vox, dtype=np.int64).reshape(4)]
    if any(a < INT32_MIN or a > INT32_MAX for a in v):
        raise ValueError("voxel fields are int32")
    out = Voxels()
    out.origin[:], out.cell = v[:3], v[3]
    return out


def as_lod(lod) -> Lod:
    """A pcr_lod from a Lod or five numbers origin x, y, z, the finest cell, levels (the stream's int32 coordinates)."""
    if isinstance(lod, Lod):
        return lod
    v = [int(a) for a in np.asarray(lod, dtype=np.int64).reshape(5)]
    if any(a < INT32_MIN or a > INT32_MAX for a in v):
        raise ValueError("level-of-detail fields are int32")
    out = Lod()
    out.origin[:], out.cell, out.levels, out.reserved = v[:3], v[3], v[4], 0
    return out


def lod_flags(drop_rest: bool, row_order: bool) -> int:
    return (N.LOD_DROP_REST if drop_rest else 0) | (N.LOD_ROW_ORDER if row_order else 0)


def thin_mode(mode) -> int:
    """PCR_THIN_FIRST / PCR_THIN_CENTER from "first" / "center" (an integer passes through: the library checks it)."""
    if isinstance(mode, str):
        if mode not in ("first", "center"):
            raise ValueError('mode is "first" or "center"')
        return N.THIN_FIRST if mode == "first" else N.THIN_CENTER
    return int(mode)


def denoise_mode(mode) -> int:
    """PCR_DENOISE_KEEP / PCR_DENOISE_ISOLATED from "keep" / "isolated" (an integer passes through: the library checks it)."""
    if isinstance(mode, str):
        if mode not in ("keep", "isolated"):
            raise ValueError(f'mode is "keep" or "isolated", not {mode!r}')
        return N.DENOISE_KEEP if mode == "keep" else N.DENOISE_ISOLATED
    return int(mode)


def components_mode(mode) -> int:
    """PCR_COMPONENTS_KEEP / PCR_COMPONENTS_SMALL from "keep" / "small" (an integer passes through: the library checks it)."""
    if isinstance(mode, str):
        if mode not in ("keep", "small"):
            raise ValueError(f'mode is "keep" or "small", not {mode!r}')
        return N.COMPONENTS_KEEP if mode == "keep" else N.COMPONENTS_SMALL
    return int(mode)


def neighbors_mode(mode) -> int:
    """PCR_NEIGHBORS_ALL / _KEEP / _SPARSE from "all" / "keep" / "sparse" (an integer passes through: the library checks it)."""
    if isinstance(mode, str):
        if mode not in ("all", "keep", "sparse"):
            raise ValueError(f'mode is "all", "keep" or "sparse", not {mode!r}')
        return {"all": N.NEIGHBORS_ALL, "keep": N.NEIGHBORS_KEEP, "sparse": N.NEIGHBORS_SPARSE}[mode]
    return int(mode)


def radius_from_world(las: LasInfo, radius: float) -> int:
    """The largest whole number r of lattice steps with r * scale <= radius as float64 evaluates the product: the radius
    Context.neighbors takes for `radius` world units. ValueError for a header whose three scales differ (the sphere is one of
    integer coordinates), and for a result below 1 or above NEIGHBORS_MAX_RADIUS."""
    sx, sy, sz = (float(las.scale[k]) for k in range(3))
    if not (sx == sy == sz):
        raise ValueError(f"the scales {sx}, {sy} and {sz} differ: a radius in world units is no sphere of lattice steps")
    radius = float(radius)
    if not sx > 0.0 or not radius > 0.0 or radius == float("inf"):
        raise ValueError("radius_from_world needs a positive scale and a positive finite radius")
    r = min(int(radius / sx), N.NEIGHBORS_MAX_RADIUS + 1)
    while r * sx > radius:                       # (the quotient may be one step off either way: the product decides)
        r -= 1
    while r <= N.NEIGHBORS_MAX_RADIUS and (r + 1) * sx <= radius:
        r += 1
    if r < 1 or r > N.NEIGHBORS_MAX_RADIUS:
        raise ValueError(f"a radius of {radius} is {r} lattice steps of {sx}: 1 .. {N.NEIGHBORS_MAX_RADIUS}")
    return r


def covariance_from_moments(moments) -> np.ndarray:
    """The covariance matrices [n, 3, 3] (float64) of pcr_moments records -- a MOMENTS_DTYPE array or an int [n, 10] array of n, s,
    q (xx, xy, xz, yy, yz, zz) -- by pcr_moments_eigen's formula, every operation rounded once: nf = float(n), m_a = float(s_a) /
    nf, C_ab = float(q_ab) / nf - m_a * m_b. Zero for n <= 0."""
    m = np.asarray(moments)
    if m.dtype == MOMENTS_DTYPE:
        m = m.view("<i8").reshape(-1, 10)
    m = m.reshape(-1, 10).astype(np.int64)
    ok = m[:, 0] > 0
    nf = np.where(ok, m[:, 0], 1).astype(np.float64)
    mean = m[:, 1:4].astype(np.float64) / nf[:, None]
    out = np.zeros((len(m), 3, 3), np.float64)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        out[:, a, b] = out[:, b, a] = m[:, 4 + k].astype(np.float64) / nf - mean[:, a] * mean[:, b]
    out[~ok] = 0.0
    return out


def knn_split(words):
    """A uint64 array of pcr_knn's words (d2 << 32 | row, KNN_NONE for none) as two int64 arrays of the same shape: the rows and
    the squared distances, -1 where there is no neighbour."""
    w = np.asarray(words, np.uint64)
    none = w == np.uint64(N.KNN_NONE)
    rows = np.where(none, -1, (w & np.uint64(0xFFFFFFFF)).astype(np.int64))
    d2 = np.where(none, -1, (w >> np.uint64(32)).astype(np.int64))
    return rows, d2


def knn_mean_distance(knn_d2, scale: float = 1.0) -> np.ndarray:
    """Per row of knn_d2 (int [n, k]: squared distances, -1 for no neighbour, as Context.read_knn returns them) the mean distance to
    the neighbours found: float64 sqrt(d2) * scale summed over the found entries in entry order, divided by their number; inf
    where none was found."""
    d2 = np.asarray(knn_d2, np.int64)
    d2 = d2.reshape(len(d2), d2.size // max(len(d2), 1)) if d2.ndim != 2 else d2
    total = np.zeros(len(d2), np.float64)
    found = np.zeros(len(d2), np.int64)
    for j in range(d2.shape[1]):
        have = d2[:, j] >= 0
        total = total + np.where(have, np.sqrt(np.where(have, d2[:, j], 0).astype(np.float64)) * float(scale), 0.0)
        found += have
    return np.where(found > 0, total / np.where(found > 0, found, 1), np.inf)


def statistical_outlier_mask(mean, multiplier: float) -> np.ndarray:
    """The statistical outlier rule over per-point mean neighbour distances (knn_mean_distance): with mu and sigma the mean and the
    population standard deviation of the finite entries, a point is an outlier iff its entry is > mu + multiplier * sigma or
    infinite. A bool array."""
    mean = np.asarray(mean, np.float64)
    finite = np.isfinite(mean)
    if not finite.any():
        return ~finite
    mu, sigma = float(mean[finite].mean()), float(mean[finite].std())
    return ~finite | (mean > mu + float(multiplier) * sigma)


def geometric_features(values) -> dict:
    """From ascending eigenvalues l0 <= l1 <= l2 ([n, 3]; numpy, or a torch tensor that is brought to the host): float64 arrays of
    curvature l0 / (l0 + l1 + l2), linearity (l2 - l1) / l2, planarity (l1 - l0) / l2 and scattering l0 / l2, each 0 where its
    denominator is 0."""
    v = np.asarray(values.cpu() if hasattr(values, "cpu") else values, np.float64).reshape(-1, 3)
    l0, l1, l2 = v[:, 0], v[:, 1], v[:, 2]

    def ratio(num, den):
        return np.where(den != 0.0, num / np.where(den != 0.0, den, 1.0), 0.0)
    return dict(curvature=ratio(l0, l0 + l1 + l2), linearity=ratio(l2 - l1, l2), planarity=ratio(l1 - l0, l2), scattering=ratio(l0, l2))


def voxels_from_world(las: LasInfo, cell_size: float, origin=None) -> Voxels:
    """The lattice of cubic voxels of `cell_size` world units whose voxel (0, 0, 0) has its min corner at the first lattice point
    at or above `origin` (world x, y, z; None: las.min) on each axis (box_from_world's). ValueError for a cell_size that is not a
    whole number (1 .. THIN_MAX_CELL) of steps of the x, the y and the z lattice -- the voxels are cubes of integer coordinates,
    so the three scales have to agree on that number -- or for an origin beyond every int32 coordinate."""
    inf = float("inf")
    cells = []
    for k in range(3):
        s = float(las.scale[k])
        if not s > 0.0 or not cell_size > 0.0:
            raise ValueError("voxels_from_world needs positive scales and a positive cell size")
        n = round(cell_size / s)
        if n < 1 or n > N.THIN_MAX_CELL or abs(n * s - cell_size) > 1e-9 * cell_size:
            raise ValueError(f"a cell of {cell_size} is not a whole number (1 .. {N.THIN_MAX_CELL}) of lattice steps of {s}")
        cells.append(int(n))
    if not cells[0] == cells[1] == cells[2]:
        raise ValueError(f"a cell of {cell_size} is {cells[0]}, {cells[1]} and {cells[2]} steps on x, y and z: the voxels are cubes of lattice steps")
    origin = tuple(las.min) if origin is None else origin
    box = box_from_world(las, origin, (inf, inf, inf))
    if any(box.min[k] > box.max[k] for k in range(3)):
        raise ValueError("the origin lies beyond every int32 coordinate")
    return as_voxels((box.min[0], box.min[1], box.min[2], cells[0]))


def lod_from_world(las: LasInfo, cell_size: float, levels: int, origin=None) -> Lod:
    """The nested lattices of Context.lod_order whose finest level is voxels_from_world(las, cell_size, origin) and whose level l
    (0 = coarsest) has cells of cell_size * 2 ** (levels - 1 - l). ValueError for what voxels_from_world refuses, for levels
    outside 1 .. LOD_MAX_LEVELS and for a coarsest cell of more than THIN_MAX_CELL lattice steps."""
    levels = int(levels)
    if levels < 1 or levels > N.LOD_MAX_LEVELS:
        raise ValueError(f"levels is 1 .. {N.LOD_MAX_LEVELS}, not {levels}")
    vox = voxels_from_world(las, cell_size, origin)
    if vox.cell << (levels - 1) > N.THIN_MAX_CELL:
        raise ValueError(f"a finest cell of {vox.cell} lattice steps with {levels} levels: the coarsest cell is more than {N.THIN_MAX_CELL} steps")
    return as_lod((vox.origin[0], vox.origin[1], vox.origin[2], vox.cell, levels))


def write_las(path, x=None, y=None, z=None, color=None, las: Optional[LasInfo] = None, points=None) -> None:
    """LAS 1.2 / point format 2 file of the given points (pcr_write_las): either four arrays (int32 coordinates, 0x00BBGGRR
    colours) or `points`, a structured array of POINT_DTYPE as Context.read_points returns it. `las`: the header's scale,
    offset, min and max. read_las gives the same values back."""
    if las is None:
        raise ValueError("write_las needs the LasInfo of the header")
    lib = N.host_lib()
    if points is not None:
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        rc = lib.pcr_write_las_points(os.fsencode(path), pts.ctypes.data, len(pts), C.byref(las))
    else:
        x, y, z = (np.ascontiguousarray(a, np.int32) for a in (x, y, z))
        color = np.ascontiguousarray(color, np.uint32)
        if not (len(x) == len(y) == len(z) == len(color)):
            raise ValueError("x, y, z, color must be of equal length")
        rc = lib.pcr_write_las(os.fsencode(path), x.ctypes.data, y.ctypes.data, z.ctypes.data, color.ctypes.data, len(x), C.byref(las))
    if rc:
        raise PcrError(f"pcr_write_las: {N.host_error()}")


class HuffmanFile:
    """Header + batch-record slicing of a .huffman image held in memory or memory-mapped from disk."""

    def __init__(self, data):
        self._mm = None
        if isinstance(data, (str, os.PathLike)):
            f = open(data, "rb")
            self._mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            f.close()
            data = self._mm
        elif isinstance(data, NativeBytes):
            self._keep = data
            data = data.view()
        self.buf = memoryview(data).cast("B")
        if len(self.buf) < 40:
            raise PcrError("file shorter than its 40-byte header")
        (self.numPoints, self.numBatches, self.encodedBytes, self.separateBytes, self.clusterBytes) = \
            struct.unpack_from("<5q", self.buf, 0)
        if self.numBatches < 0 or len(self.buf) < 40 + 8 * self.numBatches:
            raise PcrError("file shorter than its batch size table")
        self.batch_data_sizes = np.frombuffer(self.buf, np.int64, self.numBatches, 40)
        if self.numBatches and int(self.batch_data_sizes.min()) < _BATCH_FIXED + PCR_COLOR_BYTES:
            raise PcrError("a batch record is shorter than its fixed part (size table entry %d)" % int(self.batch_data_sizes.min()))
        self.offsetToBatchData = 40 + 8 * self.numBatches
        self.batch_offsets = self.offsetToBatchData + np.concatenate([[0], np.cumsum(self.batch_data_sizes)])
        if int(self.batch_offsets[-1]) > len(self.buf):
            raise PcrError("batch records exceed the file")

    def header(self, first: int = 0, count: Optional[int] = None) -> FileHeader:
        """Header of the whole file, or of the sub-stream of batches [first, first+count)."""
        if count is None:
            count = self.numBatches - first
        if first == 0 and count == self.numBatches:
            return FileHeader(self.numPoints, self.numBatches, self.encodedBytes, self.separateBytes, self.clusterBytes)
        enc = sep = 0
        for b in range(first, first + count):
            ne, ns = self.stream_lengths(b)
            enc += 4 * ne; sep += 4 * ns
        return FileHeader(count * POINTS_PER_BATCH, count, enc, sep, 128 * count)

    def blob(self, b: int) -> memoryview:
        return self.buf[int(self.batch_offsets[b]):int(self.batch_offsets[b + 1])]

    def stream_lengths(self, b: int) -> tuple[int, int]:
        """(#encoded words, #escape words) of batch b, read from its inclusive prefixes."""
        o = int(self.batch_offsets[b])
        ns = struct.unpack_from("<i", self.buf, o + BATCH_FIXED_HEADER + 4 * 3072 + 4 * 1023)[0]
        ne = struct.unpack_from("<i", self.buf, o + BATCH_FIXED_HEADER + 4 * (3072 + 1024 + 4096 + 4096) + 4 * 31)[0]
        return ne, ns

    def head_words(self, b: int) -> tuple[np.ndarray, np.ndarray]:
        """First words of batch b's encoded / escape streams: the tail a shard ending before b must carry."""
        ne, ns = self.stream_lengths(b)
        o = int(self.batch_offsets[b]) + _BATCH_FIXED
        enc = np.frombuffer(self.buf, np.uint32, min(ne, ENCODED_PAD_WORDS), o)
        sep = np.frombuffer(self.buf, np.int32, min(ns, SEPARATE_PAD_WORDS), o + 4 * ne)
        return enc, sep

    def batch_las_info(self, b: int) -> LasInfo:
        """Scale, offset and the cloud's min / max as batch b's record carries them (include/BatchDumpData.h:60-107: doubles
        at 20 and 44, the LAS box as floats at 92 and 104)."""
        o = int(self.batch_offsets[b])
        las = LasInfo()
        las.scale[:] = struct.unpack_from("<3d", self.buf, o + 20); las.offset[:] = struct.unpack_from("<3d", self.buf, o + 44)
        las.min[:] = struct.unpack_from("<3f", self.buf, o + 92); las.max[:] = struct.unpack_from("<3f", self.buf, o + 104)
        return las

    def blobs(self, first: int = 0, count: Optional[int] = None) -> Iterator[memoryview]:
        if count is None:
            count = self.numBatches - first
        for b in range(first, first + count):
            yield self.blob(b)


# --------------------------------------------------------------------------------------------------
# C-ABI context wrapper
# --------------------------------------------------------------------------------------------------
class Context:
    """Owns one pcr_ctx (one GPU, one stream)."""

    def __init__(self, device: int = 0):
        self.lib = N.hip_lib()
        h = C.c_void_p()
        rc = self.lib.pcr_create(device, C.byref(h))
        if rc:
            raise PcrError(f"pcr_create({device}) -> {rc}: {(self.lib.pcr_last_error(None) or b'').decode()}")
        self.h = h
        self.device = device

    def _chk(self, rc: int, what: str) -> None:
        if rc:
            raise PcrError(f"{what} -> {rc}: {(self.lib.pcr_last_error(self.h) or b'').decode()}")

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.pcr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # resource side
    def stream_begin(self, hdr: FileHeader, batch_index_base: int = 0):
        self._chk(self.lib.pcr_stream_begin(self.h, C.byref(hdr), batch_index_base), "pcr_stream_begin")

    def upload_batch(self, index: int, blob) -> None:
        mv = memoryview(blob).cast("B")
        arr = np.frombuffer(mv, np.uint8)
        self._chk(self.lib.pcr_upload_batch(self.h, index, arr.ctypes.data, len(mv)), "pcr_upload_batch")

    def upload_batches(self, first: int, blobs) -> None:
        """One loader task: `blobs` are the records of batches first, first+1, ... (buffer-protocol objects)."""
        arrs = [np.frombuffer(memoryview(b).cast("B"), np.uint8) for b in blobs]
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        sizes = (C.c_size_t * n)(*[a.size for a in arrs])
        self._chk(self.lib.pcr_upload_batches(self.h, first, n, ptrs, sizes), "pcr_upload_batches")

    def upload_tail(self, enc: np.ndarray, sep: np.ndarray) -> None:
        enc = np.ascontiguousarray(enc, np.uint32); sep = np.ascontiguousarray(sep, np.int32)
        self._chk(self.lib.pcr_upload_tail(self.h, enc.ctypes.data, len(enc), sep.ctypes.data, len(sep)), "pcr_upload_tail")

    def stream_unload(self):
        self._chk(self.lib.pcr_stream_unload(self.h), "pcr_stream_unload")

    @property
    def batches_loaded(self) -> int:
        return int(self.lib.pcr_batches_loaded(self.h))

    @property
    def points_loaded(self) -> int:
        return int(self.lib.pcr_points_loaded(self.h))

    @property
    def algorithmic_bytes(self) -> int:
        return int(self.lib.pcr_stream_algorithmic_bytes(self.h))

    @property
    def last_frame_algorithmic_bytes(self) -> int:
        """Algorithmic bytes of the frame the last render call drew: culled batches left out, a drawn batch's words by the
        share of its chains' points its level of detail decodes (pcr_last_frame_algorithmic_bytes; synchronises)."""
        return int(self.lib.pcr_last_frame_algorithmic_bytes(self.h))

    # method side
    # -- GPU encoder (include/pcr_gpu_encode.h) ---------------------------------------------------------
    @property
    def resident_bytes(self) -> int:
        """Device bytes the loaded stream occupies right now (pcr_stream_resident_bytes)."""
        return int(self.lib.pcr_stream_resident_bytes(self.h))

    def stream_color_format(self) -> int:
        """1 (BC1) / 7 (BC7 mode 6) / 0 before the first record (pcr_stream_color_format)."""
        return int(self.lib.pcr_stream_color_format(self.h))

    def gpu_encode_points(self, x, y, z, color, las: LasInfo, morton_sort: bool = True, chunk_points: int = 0,
                          pad_tails: bool = False) -> tuple[NativeBytes, dict]:
        """The encoder of `encode_points`, run on the GPU; same file image byte for byte."""
        x = np.ascontiguousarray(x, np.int32); y = np.ascontiguousarray(y, np.int32); z = np.ascontiguousarray(z, np.int32)
        color = np.ascontiguousarray(color, np.uint32)
        out, ln, st = C.c_void_p(), C.c_size_t(), EncodeStats()
        self._chk(self.lib.pcr_gpu_encode_points(self.h, x.ctypes.data, y.ctypes.data, z.ctypes.data, color.ctypes.data, len(x),
                                                 C.byref(las), int(bool(morton_sort)) | (2 if pad_tails else 0), chunk_points,
                                                 C.byref(out), C.byref(ln), C.byref(st)), "pcr_gpu_encode_points")
        return NativeBytes(out.value, ln.value), st.as_dict()

    # -- 10-10-10 resource / method ----------------------------------------------------------------
    def las_begin(self, num_points: int):
        self._chk(self.lib.pcr_las_begin(self.h, num_points), "pcr_las_begin")

    def las_upload(self, first_batch: int, batches, xyz12, xyz8, xyz4, rgba) -> None:
        count = len(batches)
        for a in (xyz12, xyz8, xyz4, rgba):
            if a.dtype != np.uint32 or not a.flags.c_contiguous or len(a) != count * POINTS_PER_BATCH:
                raise ValueError("level arrays must be contiguous uint32 with 65536 slots per batch")
        self._chk(self.lib.pcr_las_upload(self.h, first_batch, count, C.addressof(batches), xyz12.ctypes.data,
                                           xyz8.ctypes.data, xyz4.ctypes.data, rgba.ctypes.data), "pcr_las_upload")

    def las_unload(self):
        self._chk(self.lib.pcr_las_unload(self.h), "pcr_las_unload")

    @property
    def las_batches_loaded(self) -> int:
        return int(self.lib.pcr_las_batches_loaded(self.h))

    @property
    def las_algorithmic_bytes(self) -> int:
        return int(self.lib.pcr_las_algorithmic_bytes(self.h))

    def render_las(self, p: RenderParams):
        self._chk(self.lib.pcr_render_las(self.h, C.byref(p)), "pcr_render_las")

    def resolve_las(self, p: RenderParams):
        self._chk(self.lib.pcr_resolve_las(self.h, C.byref(p)), "pcr_resolve_las")

    def render_las_hqs_depth(self, p: RenderParams):
        self._chk(self.lib.pcr_render_las_hqs_depth(self.h, C.byref(p)), "pcr_render_las_hqs_depth")

    def render_las_hqs_color(self, p: RenderParams):
        self._chk(self.lib.pcr_render_las_hqs_color(self.h, C.byref(p)), "pcr_render_las_hqs_color")

    def set_image_size(self, w: int, h: int):
        self._chk(self.lib.pcr_set_image_size(self.h, w, h), "pcr_set_image_size")
        self.width, self.height = w, h

    def clear(self):
        self._chk(self.lib.pcr_clear(self.h), "pcr_clear")

    def frame_begin(self, p: RenderParams, hqs: bool = False):
        """pcr_clear + the prepass of the render call that follows, in one launch (pcr_hip.h)."""
        self._chk(self.lib.pcr_frame_begin(self.h, C.byref(p), 1 if hqs else 0), "pcr_frame_begin")

    def frame_turn(self, done: RenderParams, nxt: RenderParams, hqs: bool = False):
        """Resolve the finished frame, clear, and run the next frame's prepass in one launch (pcr_frame_turn)."""
        self._chk(self.lib.pcr_frame_turn(self.h, C.byref(done), C.byref(nxt), 1 if hqs else 0), "pcr_frame_turn")

    def render_basic(self, p: RenderParams):
        self._chk(self.lib.pcr_render_basic(self.h, C.byref(p)), "pcr_render_basic")

    def render_hqs_depth(self, p: RenderParams):
        self._chk(self.lib.pcr_render_hqs_depth(self.h, C.byref(p)), "pcr_render_hqs_depth")

    def render_hqs_color(self, p: RenderParams):
        self._chk(self.lib.pcr_render_hqs_color(self.h, C.byref(p)), "pcr_render_hqs_color")

    def resolve_basic(self, p: RenderParams):
        self._chk(self.lib.pcr_resolve_basic(self.h, C.byref(p)), "pcr_resolve_basic")

    def resolve_hqs(self, p: RenderParams):
        self._chk(self.lib.pcr_resolve_hqs(self.h, C.byref(p)), "pcr_resolve_hqs")

    # -- display resolves (pcr_resolve_*_display): n x n point size and eye-dome lighting ------------------
    def resolve_basic_display(self, p: RenderParams, opts: DisplayOpts):
        """resolve_basic with every point (2 * opts.window + 1)^2 pixels large and, with opts.edl_window > 0, eye-dome lighting
        (pcr_hip.h states the arithmetic). Writes the image only; zero opts give resolve_basic's bytes."""
        self._chk(self.lib.pcr_resolve_basic_display(self.h, C.byref(p), C.byref(opts) if opts is not None else None), "pcr_resolve_basic_display")

    def resolve_hqs_display(self, p: RenderParams, opts: DisplayOpts):
        """The same for resolve_hqs: the sums of the window's pixels within 1 % of the dilated depth are averaged."""
        self._chk(self.lib.pcr_resolve_hqs_display(self.h, C.byref(p), C.byref(opts) if opts is not None else None), "pcr_resolve_hqs_display")

    def resolve_las_display(self, p: RenderParams, opts: DisplayOpts):
        """The same for resolve_las."""
        self._chk(self.lib.pcr_resolve_las_display(self.h, C.byref(p), C.byref(opts) if opts is not None else None), "pcr_resolve_las_display")

    def synchronize(self):
        self._chk(self.lib.pcr_synchronize(self.h), "pcr_synchronize")

    # -- decode (pcr_decode_points / pcr_read_points) -------------------------------------------------
    def _decode_count(self, first: int, count: Optional[int]) -> int:
        return self.batches_resident - first if count is None or count < 0 else int(count)

    def decode_points(self, first: int = 0, count: Optional[int] = None, out=None):
        """Batches [first, first + count) of the loaded stream as a torch.int32 tensor [n, 4] on the context's device:
        columns x, y, z and the colour 0x00BBGGRR (its bits, as int32: torch's uint32 has few operators). count None:
        every resident batch from `first` on. `out`: a contiguous int32 CUDA tensor of at least n * 4 elements to fill
        instead of a new one. The kernel runs on the context's own stream, which nothing orders against torch's: the
        call synchronises torch's current stream before it (the tensor's memory may be in use there) and the context's
        stream after it, so the tensor is ready on return."""
        import torch
        n = self._decode_count(first, count) * POINTS_PER_BATCH
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((max(n, 0), 4), dtype=torch.int32, device=dev)
        elif out.dtype != torch.int32 or not out.is_contiguous() or out.device != dev or out.numel() < 4 * n:
            raise ValueError(f"out must be a contiguous int32 tensor of at least {4 * n} elements on {dev}")
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self.lib.pcr_decode_points(self.h, first, -1 if count is None else count, C.c_void_p(out.data_ptr() if out.numel() else None),
                                             out.numel() // 4), "pcr_decode_points")
        self.synchronize()
        return out.view(-1, 4)[:max(n, 0)]

    def read_points(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE (pcr_read_points; synchronises)."""
        n = max(self._decode_count(first, count), 0) * POINTS_PER_BATCH
        out = np.empty(n, POINT_DTYPE)
        self._chk(self.lib.pcr_read_points(self.h, first, -1 if count is None else count, out.ctypes.data if n else None, n), "pcr_read_points")
        return out

    # -- box selection (pcr_batch_point_bounds / pcr_select_box / pcr_read_box) ----------------------------
    def batch_point_bounds(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The exact integer box of the 65 536 records decode_points writes for each batch of the range: int32 [n, 6], columns
        min x, y, z, max x, y, z (computed on the GPU once per batch, then cached by the context; synchronises)."""
        n = max(self._decode_count(first, count), 0)
        out = np.empty((n, 6), np.int32)
        self._chk(self.lib.pcr_batch_point_bounds(self.h, first, -1 if count is None else count, out.ctypes.data if n else None), "pcr_batch_point_bounds")
        return out

    def select_box(self, box, first: int = 0, count: Optional[int] = None, out=None):
        """The points of batches [first, first + count) inside `box` (as_box: a Box or (min xyz, max xyz), int32, inclusive) as
        a torch.int32 tensor [n, 4] on the context's device: decode_points of the range with the rows outside the box removed.
        `out`: a contiguous int32 CUDA tensor to fill; it has to hold the result (PcrError if not; select_stats then tells
        the count). Without it the call counts first and allocates exactly. Stream ordering as decode_points. The batch
        classes and the count of the last call are in self.select_stats."""
        args = (first, -1 if count is None else count, C.byref(as_box(box)))
        return self._kept_device(self.lib.pcr_select_box, args, N.SelectStats, "select_stats", "points_selected", out, [])

    def read_box(self, box, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE (pcr_read_box: a counting call, then
        the read; synchronises)."""
        args = (first, -1 if count is None else count, C.byref(as_box(box)))
        return self._kept_host(self.lib.pcr_read_box, args, N.SelectStats, "select_stats", [])

    # -- polygon selection (pcr_select_polygon / pcr_read_polygon) ------------------------------------------
    def select_polygon(self, poly: Polygon, first: int = 0, count: Optional[int] = None, out=None):
        """The points of batches [first, first + count) inside the prism `poly` (a Polygon) as a torch.int32 tensor [n, 4] on the
        context's device: select_box with the polygon's predicate, `out` and the stream ordering as there. The batch classes,
        the count and the edge-list sizes of the last call are in self.polygon_stats."""
        args = (first, -1 if count is None else count, C.byref(poly.c))
        return self._kept_device(self.lib.pcr_select_polygon, args, N.PolygonStats, "polygon_stats", "points_selected", out, [])

    def read_polygon(self, poly: Polygon, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE (pcr_read_polygon: a counting call, then
        the read; synchronises)."""
        args = (first, -1 if count is None else count, C.byref(poly.c))
        return self._kept_host(self.lib.pcr_read_polygon, args, N.PolygonStats, "polygon_stats", [])

    # -- slabs (pcr_plane_support / pcr_select_slabs / pcr_read_slabs) -----------------------------------------
    def plane_support(self, hyp, clip=None, exclude=(), first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The support of plane hypotheses: numpy int64 [num_hyp], entry j the number of candidates in hyp[j] -- the records of
        batches [first, first + count) inside `clip` (as_box; None: all) and in no slab of `exclude` (the planes found already).
        hyp and exclude are sequences of Slab (as_slabs). Counted on the GPU from the compressed stream; no record is written
        (pcr_plane_support; synchronises). What the host plan did is in self.plane_stats."""
        h, x = as_slabs(hyp), as_slabs(exclude)
        box = None if clip is None else as_box(clip)
        out = np.zeros(len(h), np.int64)
        st = N.PlaneStats()
        self._chk(self.lib.pcr_plane_support(self.h, first, -1 if count is None else count, h, len(h), None if box is None else C.byref(box),
                                             x if len(x) else None, len(x), out.ctypes.data_as(C.POINTER(c_i64)), C.byref(st)), "pcr_plane_support")
        self.plane_stats = st.as_dict()
        return out

    @staticmethod
    def _slab_args(slabs, clip, invert: bool, first: int, count: Optional[int]):
        """What pcr_select_slabs / pcr_read_slabs take between the context and the destination."""
        s = as_slabs(slabs)
        box = None if clip is None else as_box(clip)
        return (first, -1 if count is None else count, s, len(s), None if box is None else C.byref(box), N.SLAB_INVERT if invert else 0)

    def select_slabs(self, slabs, clip=None, invert: bool = False, first: int = 0, count: Optional[int] = None, out=None):
        """The points of batches [first, first + count) inside `clip` (as_box; None: all) that are in all of `slabs` (a sequence of
        1 to 16 Slab) -- with invert=True those inside the clip that are not -- as a torch.int32 tensor [n, 4] on the context's
        device: select_box with another predicate, `out` and the stream ordering as there. The batch classes, the count and the
        slab-list sizes of the last call are in self.slab_stats."""
        args = self._slab_args(slabs, clip, invert, first, count)
        return self._kept_device(self.lib.pcr_select_slabs, args, N.SlabStats, "slab_stats", "points_selected", out, [])

    def read_slabs(self, slabs, clip=None, invert: bool = False, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE (pcr_read_slabs: a counting call, then
        the read; synchronises)."""
        args = self._slab_args(slabs, clip, invert, first, count)
        return self._kept_host(self.lib.pcr_read_slabs, args, N.SlabStats, "slab_stats", [])

    # -- top-down grid (pcr_grid_clear / pcr_grid_accumulate / pcr_grid_unpack / pcr_read_grid) --------------
    def _grid_plane(self, t, bits: int, cells: int, what: str):
        """The device pointer of a plane given as a torch tensor (None: the plane is left out)."""
        import torch
        if t is None:
            return None
        dev = torch.device("cuda", self.device)
        ok = (torch.int64, torch.uint64) if bits == 64 else (torch.int32, torch.uint32)
        if t.dtype not in ok or not t.is_contiguous() or t.device != dev or t.numel() < cells:
            raise ValueError(f"{what} must be a contiguous {bits}-bit integer tensor of at least {cells} elements on {dev}")
        return C.c_void_p(t.data_ptr())

    def grid_clear(self, grid, top=None, bottom=None, counts=None) -> None:
        """The empty values into the planes of `grid` (as_grid) given: torch tensors on the context's device, top / bottom of
        64-bit integers (0 / all ones), counts of 32-bit integers (0), width * height elements each, row cy at cy * width.
        Stream ordering as decode_points."""
        import torch
        grid = as_grid(grid)
        cells = grid.width * grid.height
        ptrs = [self._grid_plane(t, b, cells, w) for t, b, w in ((top, 64, "top"), (bottom, 64, "bottom"), (counts, 32, "counts"))]
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()
        self._chk(self.lib.pcr_grid_clear(self.h, C.byref(grid), *ptrs), "pcr_grid_clear")
        self.synchronize()

    def grid_accumulate(self, grid, top=None, bottom=None, counts=None, clip=None, first: int = 0, count: Optional[int] = None,
                        flags: int = 0) -> dict:
        """The points of batches [first, first + count) inside `clip` (as_box; None: everywhere) into the planes of `grid`, on top
        of what they hold: per cell top = unsigned max and bottom = unsigned min of (z ^ 0x80000000) << 32 | colour (int64
        tensors hold the bits), counts += the number of points. Any plane may be None. Returns the classes of the batches
        (also in self.grid_stats). Stream ordering as decode_points."""
        import torch
        grid = as_grid(grid)
        cells = grid.width * grid.height
        ptrs = [self._grid_plane(t, b, cells, w) for t, b, w in ((top, 64, "top"), (bottom, 64, "bottom"), (counts, 32, "counts"))]
        clip = None if clip is None else as_box(clip)
        st = GridStats()
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()
        self._chk(self.lib.pcr_grid_accumulate(self.h, first, -1 if count is None else count, C.byref(grid), None if clip is None else C.byref(clip),
                                               *ptrs, flags, C.byref(st)), "pcr_grid_accumulate")
        self.synchronize()
        self.grid_stats = st.as_dict()
        return self.grid_stats

    def grid_unpack(self, grid, words, which: int = N.GRID_TOP):
        """(height, rgba) of a top or bottom plane (`which`: GRID_TOP / GRID_BOTTOM tells its empty value): torch.int32 tensors
        [height, width], height = z of the cell's word (INT32_MIN for an empty cell), rgba = the bits of colour | 0xFF000000
        (0 for an empty cell)."""
        import torch
        grid = as_grid(grid)
        cells = grid.width * grid.height
        ptr = self._grid_plane(words, 64, cells, "words")
        height = torch.empty((grid.height, grid.width), dtype=torch.int32, device=words.device)
        rgba = torch.empty_like(height)
        torch.cuda.current_stream(words.device).synchronize()
        self._chk(self.lib.pcr_grid_unpack(self.h, C.byref(grid), ptr, which, C.c_void_p(height.data_ptr()), C.c_void_p(rgba.data_ptr())), "pcr_grid_unpack")
        self.synchronize()
        return height, rgba

    def read_grid(self, grid, clip=None, first: int = 0, count: Optional[int] = None, flags: int = 0):
        """The three planes of `grid` over batches [first, first + count) on the host, without torch (pcr_read_grid: clear,
        accumulate, copy; synchronises): numpy top and bottom (uint64) and count (uint32), shaped [height, width]. The classes
        of the batches are in self.grid_stats."""
        grid = as_grid(grid)
        clip = None if clip is None else as_box(clip)
        shape = (max(grid.height, 0), max(grid.width, 0))
        top, bottom, cnt = np.empty(shape, np.uint64), np.empty(shape, np.uint64), np.empty(shape, np.uint32)
        st = GridStats()
        self._chk(self.lib.pcr_read_grid(self.h, first, -1 if count is None else count, C.byref(grid), None if clip is None else C.byref(clip),
                                         top.ctypes.data, bottom.ctypes.data, cnt.ctypes.data, flags, C.byref(st)), "pcr_read_grid")
        self.grid_stats = st.as_dict()
        return top, bottom, cnt

    # -- height percentiles per grid cell (pcr_grid_quantiles / pcr_read_grid_quantiles) ----------------------
    def grid_quantiles(self, grid, q, clip=None, floor=None, first: int = 0, count: Optional[int] = None, flags: int = 0, counts: bool = False):
        """Exact percentiles of z per cell of `grid` (as_grid) over batches [first, first + count) inside `clip` (as_box; None:
        everywhere): a torch.int32 tensor [len(q), height, width], plane j the z of rank quantile_rank(q[j], n) among the cell's
        n candidates sorted ascending, INT32_MIN for a cell without one. q: basis points (9500 = the 95th percentile), 1 ..
        QUANTILES_MAX of them, any order, repeats allowed. floor: a torch.int32 tensor of the grid's cells, only records with
        z >= floor[cell] are candidates (None: all). counts=True: (planes, counts) with the candidates per cell as a torch.int32
        tensor [height, width] (the bits of the uint32). The statistics are in self.quantile_stats. Synchronises."""
        import torch
        grid = as_grid(grid)
        qa = as_quantiles(q)
        cells = grid.width * grid.height
        dev = torch.device("cuda", self.device)
        shape = (max(grid.height, 0), max(grid.width, 0))
        planes = torch.empty((len(qa),) + shape, dtype=torch.int32, device=dev)
        cnt = torch.empty(shape, dtype=torch.int32, device=dev) if counts else None
        clip = None if clip is None else as_box(clip)
        st = QuantileStats()
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self.lib.pcr_grid_quantiles(self.h, first, -1 if count is None else count, C.byref(grid), None if clip is None else C.byref(clip),
                                              None if floor is None else self._int32_plane(floor, cells, "floor"),
                                              qa.ctypes.data_as(C.POINTER(N.c_u32)), len(qa), C.c_void_p(planes.data_ptr()),
                                              None if cnt is None else C.c_void_p(cnt.data_ptr()), flags, C.byref(st)), "pcr_grid_quantiles")
        self.quantile_stats = st.as_dict()
        return (planes, cnt) if counts else planes

    def read_grid_quantiles(self, grid, q, clip=None, floor=None, first: int = 0, count: Optional[int] = None, flags: int = 0, counts: bool = False):
        """The same on the host, without torch (pcr_read_grid_quantiles; synchronises): numpy int32 [len(q), height, width], with
        counts=True also the candidates per cell as uint32 [height, width]. floor: a numpy int32 array of the grid's cells or None."""
        grid = as_grid(grid)
        qa = as_quantiles(q)
        shape = (max(grid.height, 0), max(grid.width, 0))
        planes = np.empty((len(qa),) + shape, np.int32)
        cnt = np.empty(shape, np.uint32) if counts else None
        if floor is not None:
            floor = np.ascontiguousarray(floor, np.int32)
            if floor.size != shape[0] * shape[1]:
                raise ValueError(f"floor must have the {shape[0]} x {shape[1]} cells of the grid")
        clip = None if clip is None else as_box(clip)
        st = QuantileStats()
        self._chk(self.lib.pcr_read_grid_quantiles(self.h, first, -1 if count is None else count, C.byref(grid), None if clip is None else C.byref(clip),
                                                   None if floor is None else floor.ctypes.data, qa.ctypes.data_as(C.POINTER(N.c_u32)), len(qa),
                                                   planes.ctypes.data, None if cnt is None else cnt.ctypes.data, flags, C.byref(st)),
                  "pcr_read_grid_quantiles")
        self.quantile_stats = st.as_dict()
        return (planes, cnt) if counts else planes

    # -- ground model and heights (pcr_ground_filter / pcr_read_ground / pcr_select_height / pcr_read_height) ----------
    def _int32_plane(self, t, cells: int, what: str, dtype=None):
        import torch
        dev = torch.device("cuda", self.device)
        dtype = torch.int32 if dtype is None else dtype
        if t.dtype != dtype or not t.is_contiguous() or t.device != dev or t.numel() < cells:
            raise ValueError(f"{what} must be a contiguous {dtype} tensor of at least {cells} elements on {dev}")
        return C.c_void_p(t.data_ptr())

    def ground_filter(self, grid, params, lowest, ground=None, classes=None):
        """The ground plane of a lowest-point height plane (pcr_ground_filter): `lowest` is a torch.int32 tensor of the cells of
        `grid` (as_grid; only width and height matter), INT32_MIN = empty, as grid_unpack gives it for a bottom plane; `params`
        a GroundParams. Returns (ground, classes): torch.int32 heights [height, width] -- the input height on ground cells, the
        8-neighbour fill elsewhere, INT32_MIN where the fill did not reach -- and torch.uint8 classes (CELL_EMPTY / CELL_GROUND /
        CELL_NONGROUND of the input). `ground` / `classes`: tensors to fill instead of new ones; classes=False: no classes
        (None is returned for them). The counts of the call are in self.ground_stats. Stream ordering as decode_points."""
        import torch
        grid = as_grid(grid)
        cells = grid.width * grid.height
        dev = torch.device("cuda", self.device)
        shape = (max(grid.height, 0), max(grid.width, 0))
        if ground is None:
            ground = torch.empty(shape, dtype=torch.int32, device=dev)
        if classes is None:
            classes = torch.empty(shape, dtype=torch.uint8, device=dev)
        ptrs = [self._int32_plane(lowest, cells, "lowest"), self._int32_plane(ground, cells, "ground"),
                None if classes is False else self._int32_plane(classes, cells, "classes", torch.uint8)]
        st = GroundStats()
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self.lib.pcr_ground_filter(self.h, C.byref(grid), C.byref(params), *ptrs, C.byref(st)), "pcr_ground_filter")
        self.ground_stats = st.as_dict()
        return ground, (None if classes is False else classes)

    def read_ground(self, grid, params, clip=None, first: int = 0, count: Optional[int] = None):
        """The lowest-point plane of `grid` over batches [first, first + count) inside `clip`, its ground plane and the classes on
        the host, without torch (pcr_read_ground: clear, accumulate the bottom plane, unpack, filter, copy; synchronises): numpy
        lowest and ground (int32) and classes (uint8), shaped [height, width]. The counts are in self.ground_stats."""
        grid = as_grid(grid)
        clip = None if clip is None else as_box(clip)
        shape = (max(grid.height, 0), max(grid.width, 0))
        lowest, ground, classes = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.uint8)
        st = GroundStats()
        self._chk(self.lib.pcr_read_ground(self.h, first, -1 if count is None else count, C.byref(grid), None if clip is None else C.byref(clip),
                                           C.byref(params), lowest.ctypes.data, ground.ctypes.data, classes.ctypes.data, C.byref(st)), "pcr_read_ground")
        self.ground_stats = st.as_dict()
        return lowest, ground, classes

    def select_height(self, grid, ground, h_min: int, h_max: int, clip=None, replace_z: bool = False, heights: bool = False, first: int = 0,
                      count: Optional[int] = None, out=None, points: bool = True):
        """The points of batches [first, first + count) inside `clip` and the cells of `grid` whose height h = z - ground[cell]
        above the ground plane (a torch.int32 tensor of the grid's cells, INT32_MIN = no ground: never selected) lies in
        h_min .. h_max, as a torch.int32 tensor [n, 4] as select_box gives it; replace_z: column 2 holds h. heights=True: (points,
        h) with h a torch.int32 tensor [n]; points=False: h alone, or with neither the count. `out`: a tensor for the records,
        as select_box takes it. The counts of the call are in self.height_stats. Stream ordering as decode_points."""
        import torch
        grid = as_grid(grid)
        clip = None if clip is None else as_box(clip)
        dev = torch.device("cuda", self.device)
        gptr = self._int32_plane(ground, grid.width * grid.height, "ground")
        cnt, st, nb = c_i64(), HeightStats(), -1 if count is None else count
        flags = N.HEIGHT_REPLACE_Z if replace_z else 0
        args = (self.h, first, nb, C.byref(grid), gptr, None if clip is None else C.byref(clip), int(h_min), int(h_max), flags)
        torch.cuda.current_stream(dev).synchronize()
        if out is None or not points:
            self._chk(self.lib.pcr_select_height(*args, None, None, 0, C.byref(cnt), C.byref(st)), "pcr_select_height")
            self.height_stats = st.as_dict()
            if not points and not heights:
                return cnt.value
            out = torch.empty((cnt.value, 4), dtype=torch.int32, device=dev) if points else None
        elif out.dtype != torch.int32 or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous int32 tensor on {dev}")
        cap = out.numel() // 4 if points else cnt.value
        hts = torch.empty((cap,), dtype=torch.int32, device=dev) if heights else None
        rc = self.lib.pcr_select_height(*args, C.c_void_p(out.data_ptr() if out.numel() else None) if points else None,
                                        C.c_void_p(hts.data_ptr() if hts.numel() else None) if heights else None, cap, C.byref(cnt), C.byref(st))
        self.height_stats = st.as_dict()
        if rc:
            self.height_stats["points_selected"] = cnt.value
        self._chk(rc, "pcr_select_height")
        res = ((out.view(-1, 4)[:cnt.value],) if points else ()) + ((hts[:cnt.value],) if heights else ())
        return res[0] if len(res) == 1 else res

    def read_height(self, grid, ground, h_min: int, h_max: int, clip=None, replace_z: bool = False, heights: bool = False, first: int = 0,
                    count: Optional[int] = None):
        """The same on the host: a numpy structured array of POINT_DTYPE, with heights=True (points, h) with h an int32 array
        (pcr_read_height: a counting call, then the read; synchronises). `ground` is a device plane: a torch.int32 tensor, or
        the integer address of one."""
        grid = as_grid(grid)
        clip = None if clip is None else as_box(clip)
        gptr = C.c_void_p(int(ground)) if isinstance(ground, int) else self._int32_plane(ground, grid.width * grid.height, "ground")
        cnt, st, nb = c_i64(), HeightStats(), -1 if count is None else count
        args = (self.h, first, nb, C.byref(grid), gptr, None if clip is None else C.byref(clip), int(h_min), int(h_max), N.HEIGHT_REPLACE_Z if replace_z else 0)
        self._chk(self.lib.pcr_read_height(*args, None, None, 0, C.byref(cnt), C.byref(st)), "pcr_read_height")
        pts, hts = np.empty(cnt.value, POINT_DTYPE), np.empty(cnt.value if heights else 0, np.int32)
        if cnt.value:
            self._chk(self.lib.pcr_read_height(*args, pts.ctypes.data, hts.ctypes.data if heights else None, cnt.value, C.byref(cnt), C.byref(st)),
                      "pcr_read_height")
        self.height_stats = st.as_dict()
        return (pts, hts) if heights else pts

    # -- the calls that write kept rows: the records and a few columns per row (pcr_thin .. pcr_knn; without columns the
    # selections by box, polygon and slabs above) -------------------------------------------------------------
    def _kept_device(self, fn, args, stats, attr: str, key: str, out, extra):
        """The device form of such a call: `fn` with `args` between the context and the destinations, `stats` its statistics
        structure, left as a dict in self.<attr> (its `key` is the count). `out` as Context.thin takes it: without it a counting
        call, then the exact allocation. `extra`: (asked for, torch dtype name, shape of one row) per column the call can write.
        The records, followed by the columns asked for; the records alone if there is none."""
        import torch
        dev = torch.device("cuda", self.device)
        name, cnt, st, none = fn.__name__, c_i64(), stats(), (None,) * len(extra)
        if out is None:
            self._chk(fn(self.h, *args, None, *none, 0, C.byref(cnt), C.byref(st)), name)
            out = torch.empty((cnt.value, 4), dtype=torch.int32, device=dev)
        elif out.dtype != torch.int32 or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous int32 tensor on {dev}")
        cap = out.numel() // 4
        cols = [torch.empty((cap,) + tuple(row), dtype=getattr(torch, dt), device=dev) if want else None for want, dt, row in extra]
        torch.cuda.current_stream(dev).synchronize()
        ptrs = [C.c_void_p(t.data_ptr() if cap else None) if t is not None else None for t in cols]
        rc = fn(self.h, *args, C.c_void_p(out.data_ptr() if cap else None), *ptrs, cap, C.byref(cnt), C.byref(st))
        setattr(self, attr, st.as_dict())
        if rc:
            getattr(self, attr)[key] = cnt.value
        self._chk(rc, name)
        res = (out.view(-1, 4)[:cnt.value],) + tuple(t[:cnt.value] for t in cols if t is not None)
        return res if len(res) > 1 else res[0]

    def _kept_host(self, fn, args, stats, attr: str, extra):
        """The host form: a counting call, then the read into numpy arrays. `extra`: (asked for, numpy dtype, shape of one row) per
        column. The records (POINT_DTYPE), followed by the columns asked for; the records alone if there is none."""
        name, cnt, st, none = fn.__name__, c_i64(), stats(), (None,) * len(extra)
        self._chk(fn(self.h, *args, None, *none, 0, C.byref(cnt), C.byref(st)), name)
        pts = np.empty(cnt.value, POINT_DTYPE)
        cols = [np.empty((cnt.value,) + tuple(row), dt) if want else None for want, dt, row in extra]
        if cnt.value:
            self._chk(fn(self.h, *args, pts.ctypes.data, *[None if a is None else a.ctypes.data for a in cols], len(pts), C.byref(cnt), C.byref(st)), name)
        setattr(self, attr, st.as_dict())
        res = (pts,) + tuple(a for a in cols if a is not None)
        return res if len(res) > 1 else res[0]

    # -- voxel thinning (pcr_thin / pcr_read_thin) ----------------------------------------------------------
    def thin(self, vox, clip=None, mode="first", first: int = 0, count: Optional[int] = None, out=None, rows: bool = False):
        """One point per voxel of `vox` (as_voxels: a Voxels or origin x, y, z, cell) among the rows of batches [first, first + count)
        inside `clip` (as_box; None: everywhere), straight from the compressed stream: mode "first" keeps a voxel's lowest row,
        "center" the point nearest to its centre (ties to the lowest row). A torch.int32 tensor [n, 4] on the context's device,
        rows of decode_points of the range in increasing row order; with rows=True (points, rows), rows a torch.int64 tensor [n]
        of their row numbers there. `out`: a contiguous int32 CUDA tensor to fill; it has to hold the result (PcrError if not;
        thin_stats then tells the count). Without it the call counts first and allocates exactly. Stream ordering as
        decode_points. What the last call did is in self.thin_stats."""
        vox, clip, mode = as_voxels(vox), None if clip is None else as_box(clip), thin_mode(mode)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip), mode)
        return self._kept_device(self.lib.pcr_thin, args, ThinStats, "thin_stats", "points_kept", out, [(rows, "int64", ())])

    def read_thin(self, vox, clip=None, mode="first", first: int = 0, count: Optional[int] = None, rows: bool = False):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, with rows=True (points, rows), rows an
        int64 array (pcr_read_thin: a counting call, then the read; synchronises)."""
        vox, clip, mode = as_voxels(vox), None if clip is None else as_box(clip), thin_mode(mode)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip), mode)
        return self._kept_host(self.lib.pcr_read_thin, args, ThinStats, "thin_stats", [(rows, ROW_DTYPE, ())])

    # -- levels of detail (pcr_lod_order / pcr_read_lod_order) ---------------------------------------------
    def lod_order(self, lod, clip=None, first: int = 0, count: Optional[int] = None, drop_rest: bool = False, row_order: bool = False, out=None,
                  rows: bool = False, levels: bool = False):
        """The rows of batches [first, first + count) inside `clip` (as_box; None: everywhere) ordered by the nested lattices of `lod`
        (as_lod: a Lod or origin x, y, z, finest cell, levels), straight from the compressed stream: a row's level is the least l
        (0 = coarsest) at which it is the lowest row of its voxel, `levels` ("the rest") if at none, so the rows of level <= l
        are thin() "first" with the cell of level l. A torch.int32 tensor [n, 4] on the context's device, rows of decode_points of
        the range in increasing (level, row): the first lod_stats["level_count"][0] records are level 0, and so on. drop_rest=True
        leaves the rest out; row_order=True gives increasing row order instead. rows=True appends a torch.int64 tensor [n] of
        the row numbers, levels=True a torch.uint8 tensor [n] of the levels: points, then rows, then levels. `out` and the
        allocation behave as in thin. Stream ordering as decode_points. What the last call did is in self.lod_stats."""
        lod, clip = as_lod(lod), None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, C.byref(lod), None if clip is None else C.byref(clip), lod_flags(drop_rest, row_order))
        return self._kept_device(self.lib.pcr_lod_order, args, LodStats, "lod_stats", "points_written", out, [(rows, "int64", ()), (levels, "uint8", ())])

    def read_lod_order(self, lod, clip=None, first: int = 0, count: Optional[int] = None, drop_rest: bool = False, row_order: bool = False,
                       rows: bool = False, levels: bool = False):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, then with rows=True an int64 array of the
        rows and with levels=True a uint8 array of the levels (pcr_read_lod_order: a counting call, then the read; synchronises)."""
        lod, clip = as_lod(lod), None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, C.byref(lod), None if clip is None else C.byref(clip), lod_flags(drop_rest, row_order))
        return self._kept_host(self.lib.pcr_read_lod_order, args, LodStats, "lod_stats", [(rows, ROW_DTYPE, ()), (levels, np.dtype("u1"), ())])

    # -- voxel means (pcr_voxel_mean / pcr_read_voxel_mean) --------------------------------------------------
    def voxel_mean(self, vox, clip=None, first: int = 0, count: Optional[int] = None, out=None, rows: bool = False, counts: bool = False):
        """One computed point per non-empty voxel of `vox` (as_voxels) among the rows of batches [first, first + count) inside `clip`
        (as_box; None: everywhere), straight from the compressed stream: the mean position of the voxel's points, rounded half up
        inside the voxel, and the mean of each colour byte. A torch.int32 tensor [n, 4] on the context's device, in the order of
        thin(vox, clip, "first"); rows=True appends a torch.int64 tensor [n] of each voxel's lowest row (the rows thin returns),
        counts=True one of the points per voxel: points, then rows, then counts. `out` and the allocation behave as in thin.
        Stream ordering as decode_points. What the last call did is in self.voxel_mean_stats (a ThinStats)."""
        vox, clip = as_voxels(vox), None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip))
        return self._kept_device(self.lib.pcr_voxel_mean, args, ThinStats, "voxel_mean_stats", "points_kept", out,
                                 [(rows, "int64", ()), (counts, "int64", ())])

    def read_voxel_mean(self, vox, clip=None, first: int = 0, count: Optional[int] = None, rows: bool = False, counts: bool = False):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, then with rows=True an int64 array of the
        lowest rows, with counts=True one of the points per voxel (pcr_read_voxel_mean: a counting call, then the read;
        synchronises)."""
        vox, clip = as_voxels(vox), None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip))
        return self._kept_host(self.lib.pcr_read_voxel_mean, args, ThinStats, "voxel_mean_stats", [(rows, ROW_DTYPE, ()), (counts, ROW_DTYPE, ())])

    # -- voxel denoising (pcr_denoise / pcr_read_denoise) ----------------------------------------------------
    def denoise(self, vox, max_count: int, clip=None, mode="keep", first: int = 0, count: Optional[int] = None, out=None, rows: bool = False):
        """The rows of batches [first, first + count) inside `clip` (as_box; None: everywhere) without the isolated ones (mode
        "keep") or the isolated ones alone (mode "isolated"), straight from the compressed stream. A row is isolated iff the 27
        voxels of `vox` (as_voxels) around its own hold at most `max_count` rows of the range inside the clip, itself included.
        Results, `out`, rows=True and stream ordering as Context.thin. What the last call did is in self.denoise_stats."""
        vox, clip, mode = as_voxels(vox), None if clip is None else as_box(clip), denoise_mode(mode)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip), max_count, mode)
        return self._kept_device(self.lib.pcr_denoise, args, DenoiseStats, "denoise_stats", "points_written", out, [(rows, "int64", ())])

    def read_denoise(self, vox, max_count: int, clip=None, mode="keep", first: int = 0, count: Optional[int] = None, rows: bool = False):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, with rows=True (points, rows), rows an
        int64 array (pcr_read_denoise: a counting call, then the read; synchronises)."""
        vox, clip, mode = as_voxels(vox), None if clip is None else as_box(clip), denoise_mode(mode)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip), max_count, mode)
        return self._kept_host(self.lib.pcr_read_denoise, args, DenoiseStats, "denoise_stats", [(rows, ROW_DTYPE, ())])

    # -- connected components (pcr_components / pcr_read_components) -----------------------------------------
    def components(self, vox, min_points: int = 1, connectivity: int = 26, clip=None, mode="keep", first: int = 0, count: Optional[int] = None, out=None,
                   rows: bool = False, labels: bool = False):
        """The rows of batches [first, first + count) inside `clip` (as_box; None: everywhere) without those of the small connected
        components (mode "keep") or those alone (mode "small"), straight from the compressed stream. The occupied voxels of `vox`
        (as_voxels) are adjacent if they differ by at most 1 on every axis (connectivity 26) or by exactly 1 on one axis (6); a
        component is small iff its voxels hold fewer than `min_points` rows of the range inside the clip. The label of a component
        is the least of its rows. Results, `out`, rows=True and stream ordering as Context.denoise; labels=True appends an int64
        tensor of the labels: points, (points, rows), (points, labels) or (points, rows, labels). What the last call did is in
        self.components_stats."""
        vox, clip, mode = as_voxels(vox), None if clip is None else as_box(clip), components_mode(mode)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip), connectivity, min_points, mode)
        return self._kept_device(self.lib.pcr_components, args, ComponentsStats, "components_stats", "points_written", out,
                                 [(rows, "int64", ()), (labels, "int64", ())])

    def read_components(self, vox, min_points: int = 1, connectivity: int = 26, clip=None, mode="keep", first: int = 0, count: Optional[int] = None,
                        rows: bool = False, labels: bool = False):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, with rows=True / labels=True followed by
        int64 arrays of the rows / the labels (pcr_read_components: a counting call, then the read; synchronises)."""
        vox, clip, mode = as_voxels(vox), None if clip is None else as_box(clip), components_mode(mode)
        args = (first, -1 if count is None else count, C.byref(vox), None if clip is None else C.byref(clip), connectivity, min_points, mode)
        return self._kept_host(self.lib.pcr_read_components, args, ComponentsStats, "components_stats", [(rows, ROW_DTYPE, ()), (labels, ROW_DTYPE, ())])

    # -- radius neighbourhoods (pcr_neighbors / pcr_read_neighbors) ------------------------------------------
    def neighbors(self, radius: int, min_count: int = 1, clip=None, mode="all", first: int = 0, count: Optional[int] = None, out=None,
                  rows: bool = False, counts: bool = False, nn2: bool = False):
        """The rows of batches [first, first + count) inside `clip` (as_box; None: everywhere), straight from the compressed stream:
        all of them (mode "all"), those with at least `min_count` rows of the range and clip within `radius` lattice steps, the row
        itself included (mode "keep"), or the others (mode "sparse"). Results, `out`, rows=True and stream ordering as
        Context.denoise; counts=True appends an int64 tensor of N (the rows within the radius), nn2=True an int64 tensor holding
        the squared distance to the nearest other row within the radius (-1, the bits of NN2_NONE, for none): points, then rows,
        counts, nn2 as asked for. What the last call did is in self.neighbors_stats."""
        clip, mode = None if clip is None else as_box(clip), neighbors_mode(mode)
        args = (first, -1 if count is None else count, radius, None if clip is None else C.byref(clip), min_count, mode)
        return self._kept_device(self.lib.pcr_neighbors, args, NeighborsStats, "neighbors_stats", "points_written", out,
                                 [(rows, "int64", ()), (counts, "int64", ()), (nn2, "int64", ())])

    def read_neighbors(self, radius: int, min_count: int = 1, clip=None, mode="all", first: int = 0, count: Optional[int] = None, rows: bool = False,
                       counts: bool = False, nn2: bool = False):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, followed as asked for by int64 arrays of
        the rows and of N and a uint64 array of nn2 (NN2_NONE for none) (pcr_read_neighbors: a counting call, then the read;
        synchronises)."""
        clip, mode = None if clip is None else as_box(clip), neighbors_mode(mode)
        args = (first, -1 if count is None else count, radius, None if clip is None else C.byref(clip), min_count, mode)
        return self._kept_host(self.lib.pcr_read_neighbors, args, NeighborsStats, "neighbors_stats",
                               [(rows, ROW_DTYPE, ()), (counts, np.int64, ()), (nn2, np.uint64, ())])

    # -- local moments (pcr_local_moments / pcr_read_local_moments / pcr_moments_eigen) ------------------------
    def local_moments(self, radius: int, min_count: int = 1, clip=None, first: int = 0, count: Optional[int] = None, out=None,
                      rows: bool = False, moments: bool = False, eigen: bool = False):
        """The rows of batches [first, first + count) inside `clip` (as_box; None: everywhere) that have at least `min_count` rows of
        the range and clip within `radius` lattice steps (1 .. MOMENTS_MAX_RADIUS), the row itself included, straight from the
        compressed stream. Results, `out`, rows=True and stream ordering as Context.neighbors; moments=True appends an int64
        tensor [n, 10] of the exact moments of the offsets to the rows within the radius (n, s x y z, q xx xy xz yy yz zz),
        eigen=True a float64 tensor [n, 6] (the eigenvalues of the covariance, ascending, and the unit normal): points, then rows,
        moments, eigen as asked for. What the last call did is in self.moments_stats."""
        clip = None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, radius, None if clip is None else C.byref(clip), min_count)
        return self._kept_device(self.lib.pcr_local_moments, args, NeighborsStats, "moments_stats", "points_written", out,
                                 [(rows, "int64", ()), (moments, "int64", (10,)), (eigen, "float64", (6,))])

    def read_local_moments(self, radius: int, min_count: int = 1, clip=None, first: int = 0, count: Optional[int] = None, rows: bool = False,
                           moments: bool = False, eigen: bool = False):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, followed as asked for by an int64 array of
        the rows, a MOMENTS_DTYPE array and an EIGEN_DTYPE array (pcr_read_local_moments: a counting call, then the read;
        synchronises)."""
        clip = None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, radius, None if clip is None else C.byref(clip), min_count)
        return self._kept_host(self.lib.pcr_read_local_moments, args, NeighborsStats, "moments_stats",
                               [(rows, ROW_DTYPE, ()), (moments, MOMENTS_DTYPE, ()), (eigen, EIGEN_DTYPE, ())])

    # -- k nearest neighbours (pcr_knn / pcr_read_knn) --------------------------------------------------------
    def knn(self, k: int, radius: int, min_found: int = 0, clip=None, first: int = 0, count: Optional[int] = None, out=None, rows: bool = False,
            neighbors: bool = True):
        """The rows of batches [first, first + count) inside `clip` (as_box; None: everywhere) that have at least `min_found` (0 ..
        k) other rows of the range and clip within `radius` lattice steps (1 .. KNN_MAX_RADIUS), with their k (1 .. KNN_MAX_K)
        nearest ones in the order (squared distance, row), straight from the compressed stream. Results, `out`, rows=True and stream
        ordering as Context.neighbors; neighbors=True appends two int64 tensors [n, k], knn_rows (rows relative to `first`) and
        knn_d2, both -1 where a row has fewer than k neighbours: points, then rows, knn_rows, knn_d2 as asked for. What the last
        call did is in self.knn_stats."""
        import torch
        clip = None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, k, radius, None if clip is None else C.byref(clip), min_found)
        res = self._kept_device(self.lib.pcr_knn, args, NeighborsStats, "knn_stats", "points_written", out, [(rows, "int64", ()), (neighbors, "int64", (k,))])
        if neighbors:
            w = res[-1]
            none = w == -1                                  # (KNN_NONE's bits)
            res = res[:-1] + (torch.where(none, w, w & 0xFFFFFFFF), torch.where(none, w, w >> 32))
        return res

    def read_knn(self, k: int, radius: int, min_found: int = 0, clip=None, first: int = 0, count: Optional[int] = None, rows: bool = False,
                 neighbors: bool = True):
        """The same on the host, without torch: a numpy structured array of POINT_DTYPE, followed as asked for by an int64 array of
        the rows and the int64 arrays [n, k] knn_rows and knn_d2 (pcr_read_knn: a counting call, then the read; synchronises)."""
        clip = None if clip is None else as_box(clip)
        args = (first, -1 if count is None else count, k, radius, None if clip is None else C.byref(clip), min_found)
        res = self._kept_host(self.lib.pcr_read_knn, args, NeighborsStats, "knn_stats", [(rows, ROW_DTYPE, ()), (neighbors, np.uint64, (k,))])
        return res[:-1] + knn_split(res[-1]) if neighbors else res

    def moments_eigen(self, moments):
        """pcr_moments_eigen: the eigen records of moments records. An int64 torch tensor [n, 10] on this context's device gives a
        float64 tensor [n, 6] there; a numpy array (MOMENTS_DTYPE, or int64 [n, 10]) is uploaded and gives an EIGEN_DTYPE array.
        Needs no stream loaded; synchronises."""
        import torch
        dev = torch.device("cuda", self.device)
        on_host = not isinstance(moments, torch.Tensor)
        if on_host:
            m = np.ascontiguousarray(moments)
            m = m.view("<i8") if m.dtype == MOMENTS_DTYPE else m.astype(np.int64, copy=False)
            moments = torch.from_numpy(m.reshape(-1, 10).copy()).to(dev)
        if moments.dtype != torch.int64 or moments.device != dev or not moments.is_contiguous() or moments.dim() != 2 or moments.shape[1] != 10:
            raise ValueError(f"moments must be a contiguous int64 tensor [n, 10] on {dev}")
        n = moments.shape[0]
        out = torch.empty((n, 6), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self.lib.pcr_moments_eigen(self.h, C.c_void_p(moments.data_ptr() if n else None), n, C.c_void_p(out.data_ptr() if n else None)),
                  "pcr_moments_eigen")
        return out.cpu().numpy().reshape(-1).view(EIGEN_DTYPE) if on_host else out

    # -- screen selection and picking (pcr_select_screen / pcr_read_screen / pcr_pick) ---------------------
    def select_screen(self, p: RenderParams, rect=None):
        """The points a frame of camera `p` draws (render_basic's cull, level of detail, precision and inside test) whose pixel lies
        in `rect` (as_rect: a Rect or x0, y0, x1, y1, inclusive, clipped to the image; None: the whole image), on the context's
        device: (points, hits). points is a torch.int32 tensor [n, 4], the rows decode_points gives for them (x, y, z, colour
        0x00BBGGRR). hits is a torch.int64 tensor [n, 2], the bytes of n pcr_screen_hit records: column 0 = depth_bits << 32 |
        pixel (pixel = x + y * width, depth_bits = the float32 bits of w: hits[:, 0] & 0xFFFFFFFF and hits[:, 0] >> 32), column 1 =
        the point's row in decode_points(0, None). Rows are in increasing index order. The call counts first and allocates
        exactly; stream ordering as decode_points. The counts of the last call are in self.screen_stats."""
        import torch
        rect = as_rect(rect)
        dev = torch.device("cuda", self.device)
        cnt, st = c_i64(), N.ScreenStats()
        rp = C.byref(rect) if rect is not None else None
        self._chk(self.lib.pcr_select_screen(self.h, C.byref(p), rp, None, None, 0, C.byref(cnt), C.byref(st)), "pcr_select_screen")
        pts = torch.empty((cnt.value, 4), dtype=torch.int32, device=dev)
        hits = torch.empty((cnt.value, 2), dtype=torch.int64, device=dev)
        if cnt.value:
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.lib.pcr_select_screen(self.h, C.byref(p), rp, C.c_void_p(pts.data_ptr()), C.c_void_p(hits.data_ptr()), cnt.value,
                                                 C.byref(cnt), C.byref(st)), "pcr_select_screen")
        self.screen_stats = st.as_dict()
        return pts, hits

    def read_screen(self, p: RenderParams, rect=None):
        """The same on the host, without torch: (points, hits), numpy structured arrays of POINT_DTYPE and HIT_DTYPE
        (pcr_read_screen: a counting call, then the read; synchronises)."""
        rect = as_rect(rect)
        args = (C.byref(p), C.byref(rect) if rect is not None else None)
        return self._kept_host(self.lib.pcr_read_screen, args, N.ScreenStats, "screen_stats", [(True, HIT_DTYPE, ())])

    def pick(self, p: RenderParams, px: int, py: int, radius: int = 0):
        """The point under pixel (px, py) of a frame of camera `p`: among the select_screen hits within `radius` pixels (a square
        window, clipped to the image) the least by (depth_bits, colour, index). None if the window holds no point, else
        (point, hit): a Point (x, y, z, color) and a ScreenHit (pixel, depth_bits, index). Synchronises."""
        pt, hit, found = N.Point(), N.ScreenHit(), C.c_int()
        self._chk(self.lib.pcr_pick(self.h, C.byref(p), int(px), int(py), int(radius), C.byref(pt), C.byref(hit), C.byref(found)), "pcr_pick")
        return (pt, hit) if found.value else None

    # -- visible selection (pcr_select_visible / pcr_read_visible) -----------------------------------------
    VISIBLE_FRONT, VISIBLE_SURFACE = N.VISIBLE_FRONT, N.VISIBLE_SURFACE
    _VISIBLE_MODES = {"front": N.VISIBLE_FRONT, "surface": N.VISIBLE_SURFACE}

    def _visible_mode(self, mode) -> int:
        if isinstance(mode, str):
            if mode not in self._VISIBLE_MODES:
                raise ValueError(f"mode must be 'front' or 'surface', not {mode!r}")
            return self._VISIBLE_MODES[mode]
        return int(mode)

    def select_visible(self, p: RenderParams, rect=None, mode="front", radius: int = 0, depth: bool = False):
        """Of select_screen(p, rect)'s hits those that make up the picture, on the context's device: (points, hits), shaped as
        select_screen's and in increasing index order, or (points, hits, depth) with depth=True. mode "front" (VISIBLE_FRONT):
        per pixel of the rect the one hit that is least by (depth_bits, colour, index); "surface" (VISIBLE_SURFACE): every hit of
        the rect within 1 % of its pixel's front depth, float64(w) <= float64(dr) * 1.01. The front depth of a pixel is taken
        over all hits of the image, and with radius > 0 (up to VISIBLE_MAX_RADIUS) over the pixels within `radius` columns and
        rows as well: hidden-point removal for a cloud with gaps; a front hit that fails the test is dropped. depth is that
        plane of the whole image, a torch.int32 tensor [height, width] holding the uint32 float bits of w (0xFFFFFFFF = -1: no
        hit within the radius; depth.view(torch.float32) gives w, NaN where empty). The call counts first and allocates
        exactly; synchronises. The counts of the last call are in self.visible_stats."""
        import torch
        rect, mode, radius = as_rect(rect), self._visible_mode(mode), int(radius)
        dev = torch.device("cuda", self.device)
        cnt, st = c_i64(), N.VisibleStats()
        rp = C.byref(rect) if rect is not None else None
        plane = torch.empty((p.height, p.width), dtype=torch.int32, device=dev) if depth else None
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self.lib.pcr_select_visible(self.h, C.byref(p), rp, mode, radius, None, None, C.c_void_p(plane.data_ptr()) if depth else None, 0,
                                              C.byref(cnt), C.byref(st)), "pcr_select_visible")
        pts = torch.empty((cnt.value, 4), dtype=torch.int32, device=dev)
        hits = torch.empty((cnt.value, 2), dtype=torch.int64, device=dev)
        if cnt.value:
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.lib.pcr_select_visible(self.h, C.byref(p), rp, mode, radius, C.c_void_p(pts.data_ptr()), C.c_void_p(hits.data_ptr()), None,
                                                  cnt.value, C.byref(cnt), C.byref(st)), "pcr_select_visible")
        self.visible_stats = st.as_dict()
        return (pts, hits, plane) if depth else (pts, hits)

    def read_visible(self, p: RenderParams, rect=None, mode="front", radius: int = 0, depth: bool = False):
        """The same on the host, without torch: numpy structured arrays of POINT_DTYPE and HIT_DTYPE, and with depth=True the
        plane as a uint32 array [height, width] (pcr_read_visible: a counting call, then the read; synchronises)."""
        rect, mode, radius = as_rect(rect), self._visible_mode(mode), int(radius)
        cnt, st = c_i64(), N.VisibleStats()
        rp = C.byref(rect) if rect is not None else None
        plane = np.empty((p.height, p.width), np.uint32) if depth else None
        self._chk(self.lib.pcr_read_visible(self.h, C.byref(p), rp, mode, radius, None, None, plane.ctypes.data if depth else None, 0, C.byref(cnt),
                                            C.byref(st)), "pcr_read_visible")
        pts, hits = np.empty(cnt.value, POINT_DTYPE), np.empty(cnt.value, HIT_DTYPE)
        if cnt.value:
            self._chk(self.lib.pcr_read_visible(self.h, C.byref(p), rp, mode, radius, pts.ctypes.data, hits.ctypes.data, None, cnt.value, C.byref(cnt),
                                                C.byref(st)), "pcr_read_visible")
        self.visible_stats = st.as_dict()
        return (pts, hits, plane) if depth else (pts, hits)

    def stats(self) -> dict:
        st = RenderStats()
        self._chk(self.lib.pcr_get_stats(self.h, C.byref(st)), "pcr_get_stats")
        return st.as_dict()

    def read_framebuffer(self, full: bool = False) -> np.ndarray:
        n = fb_elems(self.width, self.height) if full else self.width * self.height
        out = np.empty(n, np.uint64)
        self._chk(self.lib.pcr_read_framebuffer(self.h, out.ctypes.data, n), "pcr_read_framebuffer")
        return out

    def read_accum(self, full: bool = False):
        n = fb_elems(self.width, self.height) if full else self.width * self.height
        rg, ba = np.empty(n, np.uint64), np.empty(n, np.uint64)
        self._chk(self.lib.pcr_read_accum(self.h, rg.ctypes.data, ba.ctypes.data, n), "pcr_read_accum")
        return rg, ba

    def read_rgba(self) -> np.ndarray:
        n = self.width * self.height
        out = np.empty(n, np.uint32)
        self._chk(self.lib.pcr_read_rgba(self.h, out.ctypes.data, n), "pcr_read_rgba")
        return out

    # multi-GPU plumbing / measurement
    def device_framebuffer(self) -> int:
        return int(self.lib.pcr_device_framebuffer(self.h) or 0)

    def framebuffer_private(self) -> None:
        """Pointers handed out by device_framebuffer() are no longer written through: dirty tiles are used again (pcr_hip.h)."""
        self._chk(self.lib.pcr_framebuffer_private(self.h), "pcr_framebuffer_private")

    def use_external_buffers(self, fb: int = 0, rg: int = 0, ba: int = 0):
        self._chk(self.lib.pcr_use_external_buffers(self.h, C.c_void_p(fb or None), C.c_void_p(rg or None), C.c_void_p(ba or None)),
                  "pcr_use_external_buffers")

    def set_stream(self, hip_stream: int):
        self._chk(self.lib.pcr_set_stream(self.h, C.c_void_p(hip_stream or None)), "pcr_set_stream")

    def merge_min(self, other_fb: int):
        self._chk(self.lib.pcr_merge_min(self.h, C.c_void_p(other_fb)), "pcr_merge_min")

    def merge_sum(self, other_rg: int, other_ba: int):
        self._chk(self.lib.pcr_merge_sum(self.h, C.c_void_p(other_rg or None), C.c_void_p(other_ba or None)), "pcr_merge_sum")

    def flip_sign(self):
        self._chk(self.lib.pcr_flip_sign(self.h), "pcr_flip_sign")

    LAYOUT_WORDS, LAYOUT_POINT_WINDOWS, LAYOUT_BOTH, LAYOUT_AUTO = 0, 1, 2, 3

    def set_stream_layout(self, layout: int) -> None:
        """HBM layout of the next stream this context loads (pcr_hip.h: PCR_LAYOUT_*)."""
        self._chk(self.lib.pcr_set_stream_layout(self.h, int(layout)), "pcr_set_stream_layout")

    def set_hbm_budget(self, nbytes: int) -> None:
        """LAYOUT_AUTO: a stream whose point windows would take more than this many bytes is loaded as packed words."""
        self._chk(self.lib.pcr_set_hbm_budget(self.h, int(nbytes)), "pcr_set_hbm_budget")

    @property
    def stream_layout(self) -> int:
        return int(self.lib.pcr_stream_layout(self.h))

    VARIANT_AUTO, VARIANT_WORDS, VARIANT_POINT_WINDOWS = 0, 1, 2

    def set_render_variant(self, variant: int) -> None:
        """Which decode variant draws a stream that has both layouts resident (pcr_hip.h: PCR_VARIANT_*)."""
        self._chk(self.lib.pcr_set_render_variant(self.h, int(variant)), "pcr_set_render_variant")

    def set_workgroup_parts(self, parts: int) -> None:
        """Workgroups per batch of the render kernels: 0 = library's choice, 1 = whole batches (1024 threads), 2 = half-batches."""
        self._chk(self.lib.pcr_set_workgroup_parts(self.h, int(parts)), "pcr_set_workgroup_parts")

    def merge_min_slices(self, slices_ptr: int, nslices: int, slice_elems: int) -> None:
        self._chk(self.lib.pcr_merge_min_slices(self.h, slices_ptr, nslices, slice_elems), "pcr_merge_min_slices")

    def resolve_basic_range(self, p: RenderParams, fb_ptr: int, count: int, rgba_ptr: int) -> None:
        self._chk(self.lib.pcr_resolve_basic_range(self.h, C.byref(p), fb_ptr, count, rgba_ptr), "pcr_resolve_basic_range")

    def fence_record(self, slot: int, hip_stream: int = 0) -> None:
        self._chk(self.lib.pcr_fence_record(self.h, slot, hip_stream), "pcr_fence_record")

    def fence_wait(self, slot: int, hip_stream: int = 0) -> None:
        self._chk(self.lib.pcr_fence_wait(self.h, slot, hip_stream), "pcr_fence_wait")

    def set_int64_mergeable(self, on: bool) -> None:
        """Empty pixels as INT64_MAX so that a signed 64-bit MIN collective orders the framebuffer (pcr_hip.h)."""
        self._chk(self.lib.pcr_set_int64_mergeable(self.h, int(on)), "pcr_set_int64_mergeable")

    def set_async_upload(self, on: bool) -> None:
        """Loader copies + transcode on the context's loader stream; frames draw what has arrived (pcr_hip.h)."""
        self._chk(self.lib.pcr_set_async_upload(self.h, int(on)), "pcr_set_async_upload")

    @property
    def batches_resident(self) -> int:
        return int(self.lib.pcr_batches_resident(self.h))

    @property
    def last_frame_batches(self) -> int:
        return int(self.lib.pcr_last_frame_batches(self.h))

    def measure_hbm(self, nbytes: int = 2 << 30, reps: int = 5) -> tuple[float, float]:
        """(streaming read GB/s, streaming copy GB/s) of this device: the practical HBM ceiling."""
        r, w = C.c_float(), C.c_float()
        self._chk(self.lib.pcr_measure_hbm(self.h, nbytes, reps, C.byref(r), C.byref(w)), "pcr_measure_hbm")
        return float(r.value), float(w.value)

    def kernel_timing(self, every: int) -> None:
        """Bracket every `every`-th decode+rasterize launch with HIP events (0/False = off)."""
        self._chk(self.lib.pcr_kernel_timing_enable(self.h, int(every)), "pcr_kernel_timing_enable")

    def kernel_timing_read(self) -> tuple[float, int]:
        """(average ms of the decode+rasterize kernel over the most recent launches, how many)."""
        ms, n = C.c_float(), C.c_int()
        self._chk(self.lib.pcr_kernel_timing_read(self.h, C.byref(ms), C.byref(n)), "pcr_kernel_timing_read")
        return float(ms.value), int(n.value)

    def timing_begin(self):
        self._chk(self.lib.pcr_timing_begin(self.h), "pcr_timing_begin")

    def timing_end(self) -> float:
        ms = C.c_float()
        self._chk(self.lib.pcr_timing_end(self.h, C.byref(ms)), "pcr_timing_end")
        return float(ms.value)


# --------------------------------------------------------------------------------------------------
# the reference's plugin surface, headless
# --------------------------------------------------------------------------------------------------
class Debug:                      # include/Debug.h:14-31 (the flags the Huffman methods read)
    LOD = 0.1
    frustumCullingEnabled = True
    colorizeChunks = False
    showNumPoints = False


class Renderer:
    """Headless stand-in for the reference Renderer: window size + orbit camera + one GPU context."""

    def __init__(self, width: int = 1920, height: int = 1080, device: int = 0):   # Renderer.cpp:142-143
        self.width, self.height = width, height
        self.ctx = Context(device)
        self.ctx.set_image_size(width, height)
        self.yaw, self.pitch, self.radius, self.target = 0.0, 0.0, 10.0, (0.0, 0.0, 0.0)
        self.params_override: Optional[RenderParams] = None

    def set_camera(self, yaw, pitch, radius, target):
        self.yaw, self.pitch, self.radius, self.target = yaw, pitch, radius, tuple(target)

    def render_params(self) -> RenderParams:
        p = self.params_override.copy() if self.params_override is not None else \
            camera_orbit(self.yaw, self.pitch, self.radius, self.target, self.width, self.height)
        p.lod_percent = int(Debug.LOD * 100)                       # huffman_hqs.h:177
        p.enable_frustum_culling = int(Debug.frustumCullingEnabled)
        p.colorize_chunks = int(Debug.colorizeChunks)
        p.show_num_points = int(Debug.showNumPoints)
        return p


class Resource:                   # modules/compute/Resources.h:20-35
    UNLOADED, LOADING, LOADED, UNLOADING = range(4)

    def __init__(self):
        self.state = Resource.UNLOADED

    def load(self, renderer): raise NotImplementedError
    def unload(self, renderer): raise NotImplementedError
    def process(self, renderer): raise NotImplementedError


class Method:                     # include/Method.h:10-23
    name = "no name"
    description = ""
    group = "no group"

    def update(self, renderer): raise NotImplementedError
    def render(self, renderer): raise NotImplementedError


class Runtime:                    # include/Runtime.h:15-55
    methods: list = []
    selectedMethod: Optional[Method] = None
    resource: Optional[Resource] = None

    @staticmethod
    def addMethod(m: Method):
        Runtime.methods.append(m)

    @staticmethod
    def setSelectedMethod(name: str):
        for m in Runtime.methods:
            if m.name == name:
                Runtime.selectedMethod = m

    @staticmethod
    def getSelectedMethod():
        return Runtime.selectedMethod

    @staticmethod
    def reset():
        Runtime.methods, Runtime.selectedMethod, Runtime.resource = [], None, None


class HuffmanLasData(Resource):
    """modules/compute/HuffmanLasLoader.{h,cpp}. `first_batch`/`num_batches` select a contiguous shard
    (multi-GPU); the reference always loads the whole file."""

    BATCHES_PER_TASK = 100        # HuffmanLasLoader.cpp:106

    def __init__(self):
        super().__init__()
        self.path = ""
        self.file: Optional[HuffmanFile] = None
        self.numBatches = self.numPoints = 0
        self.numBatchesLoaded = self.numPointsLoaded = 0
        self.first_batch = 0
        self._next = 0

    @staticmethod
    def create(path_or_bytes, first_batch: int = 0, num_batches: Optional[int] = None) -> "HuffmanLasData":
        d = HuffmanLasData()
        d.path = path_or_bytes if isinstance(path_or_bytes, (str, os.PathLike)) else "<memory>"
        d.file = HuffmanFile(path_or_bytes)                          # loadHeader()
        d.first_batch = first_batch
        d.numBatches = d.file.numBatches - first_batch if num_batches is None else num_batches
        d.numPoints = d.numBatches * POINTS_PER_BATCH
        return d

    def load(self, renderer: Renderer):
        if self.state != Resource.UNLOADED:                          # HuffmanLasLoader.cpp:25-31
            return
        self.state = Resource.LOADING
        hdr = self.file.header(self.first_batch, self.numBatches)
        renderer.ctx.stream_begin(hdr, self.first_batch)
        self._next = 0
        self.numBatchesLoaded = self.numPointsLoaded = 0

    def process(self, renderer: Renderer):
        """Upload the next task of <= 100 batches (HuffmanLasLoader.cpp:301-313; the reference's reader
        thread hands them over one task per frame — here the file is already mapped)."""
        if self.state not in (Resource.LOADING,):
            return
        end = min(self.numBatches, self._next + self.BATCHES_PER_TASK)
        renderer.ctx.upload_batches(self._next, [self.file.blob(self.first_batch + i) for i in range(self._next, end)])
        self._next = end
        self.numBatchesLoaded = renderer.ctx.batches_loaded
        self.numPointsLoaded = renderer.ctx.points_loaded
        if self._next == self.numBatches:
            nxt = self.first_batch + self.numBatches
            if nxt < self.file.numBatches:                            # shard boundary: carry the follower's head words
                renderer.ctx.upload_tail(*self.file.head_words(nxt))
            self.state = Resource.LOADED

    def load_all(self, renderer: Renderer):
        self.load(renderer)
        while self.state == Resource.LOADING:
            self.process(renderer)

    def unload(self, renderer: Renderer):
        self.numBatchesLoaded = 0
        renderer.ctx.stream_unload()
        self.state = Resource.UNLOADED

    def points(self, renderer: Renderer, world: bool = False):
        """Every point of the loaded resource, decoded on the GPU (Context.decode_points): a torch.int32 tensor [n, 4] of
        x, y, z, colour in the stream's order. world=True: (xyz, pts) with xyz a float64 tensor [n, 3] = x * scale + offset,
        computed by torch on the device from every batch record's own scale and offset, and pts the int32 tensor (its
        column 3 holds the colours)."""
        import torch
        pts = renderer.ctx.decode_points(0, None)
        if not world:
            return pts
        nb = pts.shape[0] // POINTS_PER_BATCH
        so = np.empty((nb, 2, 3), np.float64)
        for i in range(nb):
            g = self.file.batch_las_info(self.first_batch + i)
            so[i, 0], so[i, 1] = tuple(g.scale), tuple(g.offset)
        so = torch.from_numpy(so).to(pts.device)
        xyz = pts[:, :3].view(nb, POINTS_PER_BATCH, 3).to(torch.float64) * so[:, None, 0, :] + so[:, None, 1, :]
        return xyz.view(-1, 3), pts

    def points_in_box(self, renderer: Renderer, lo, hi, world: bool = True):
        """The points of the loaded resource inside a box, selected on the GPU (Context.select_box): what points() returns with the
        rows outside the box removed, without decoding the batches the box misses. world=True: lo / hi are world coordinates,
        turned into the largest integer box by box_from_world with las_info()'s scale and offset (the stream's: the reference's
        encoder writes the same into every batch record), and the result is (xyz, pts) as points(world=True) returns it.
        world=False: lo / hi are the stream's int32 coordinates, the result the int32 tensor alone."""
        import torch
        info = self.las_info()
        box = box_from_world(info, lo, hi) if world else as_box((lo, hi))
        pts = renderer.ctx.select_box(box)
        if not world:
            return pts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts

    def points_in_polygon(self, renderer: Renderer, rings, z_lo=None, z_hi=None, invert: bool = False, world: bool = True):
        """The points of the loaded resource inside a polygon prism, selected on the GPU (Context.select_polygon). world=True:
        rings, z_lo and z_hi are world coordinates, turned into a Polygon by polygon_from_world with las_info()'s scale and
        offset, and the result is (xyz, pts) as points(world=True) returns it. world=False: they are the stream's int32
        coordinates (z_lo / z_hi None: unbounded), the result the int32 tensor alone."""
        import torch
        info = self.las_info()
        if world:
            poly = polygon_from_world(info, rings, z_lo, z_hi, invert)
        else:
            poly = Polygon(rings, INT32_MIN if z_lo is None else z_lo, INT32_MAX if z_hi is None else z_hi, invert)
        pts = renderer.ctx.select_polygon(poly)
        if not world:
            return pts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts

    def points_in_slabs(self, renderer: Renderer, slabs, lo=None, hi=None, invert: bool = False, world: bool = True):
        """The points of the loaded resource in all of `slabs` (Slab objects in the stream's coordinates: slab_from_world makes them
        from a world plane), or with invert=True the others, selected on the GPU (Context.select_slabs). world=True: lo / hi are
        world coordinates of a clip box (None: the header's min / max) and the result is (xyz, pts) as points(world=True) returns
        it. world=False: lo / hi are the stream's int32 coordinates (None: no clip), the result the int32 tensor alone."""
        import torch
        info = self.las_info()
        if world:
            clip = box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        else:
            clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
        pts = renderer.ctx.select_slabs(slabs, clip, invert)
        if not world:
            return pts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts

    def fit_planes(self, renderer: Renderer, distance: float, num_planes: int = 1, hypotheses: int = 256, seed: int = 0, lo=None, hi=None,
                   min_support: int = 3):
        """The dominant planes of the loaded resource by sequential RANSAC (fit_planes_rounds has the rounds): per round a few
        batches are read back to draw `hypotheses` planes from, and one Context.plane_support call counts, for all of them at once
        and straight from the compressed stream, the points within `distance` world units (radius_from_world + slab_tolerance)
        that no plane found earlier holds. lo / hi: a clip box in world coordinates (None: the header's min / max). Returns
        (slabs, supports, candidates): the planes as Slab objects in the stream's coordinates, their supports, and the number of
        points each round had left. No refinement: a plane is the best hypothesis as drawn."""
        info = self.las_info()
        clip = box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        ctx = renderer.ctx

        def read_batch(b):
            pts = ctx.read_points(b, 1)
            return np.stack([pts["x"], pts["y"], pts["z"]], axis=1)

        return fit_planes_rounds(read_batch, lambda hyp, exclude: ctx.plane_support(hyp, clip, exclude), ctx.batches_resident,
                                 radius_from_world(info, distance), num_planes, hypotheses, seed, min_support, clip)

    def points_on_screen(self, renderer: Renderer, params: Optional[RenderParams] = None, rect=None, world: bool = True):
        """The points of the loaded resource a frame of `params` (None: renderer.render_params()) draws inside `rect` (pixels,
        None: the whole image), selected on the GPU (Context.select_screen). world=True: (xyz, pts, hits) with xyz a float64
        tensor [n, 3] = x * scale + offset from las_info()'s scale and offset, as points_in_box; world=False: (pts, hits)."""
        import torch
        pts, hits = renderer.ctx.select_screen(renderer.render_params() if params is None else params, rect)
        if not world:
            return pts, hits
        info = self.las_info()
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts, hits

    def visible_points(self, renderer: Renderer, params: Optional[RenderParams] = None, rect=None, mode="front", radius: int = 0, world: bool = True):
        """The points of the loaded resource that make up the picture of `params` (None: renderer.render_params()) inside `rect`:
        points_on_screen without what lies behind the surface (Context.select_visible: mode "front" / "surface", radius = the
        occluder window). world=True: (xyz, pts, hits) as points_on_screen; world=False: (pts, hits)."""
        import torch
        pts, hits = renderer.ctx.select_visible(renderer.render_params() if params is None else params, rect, mode, radius)
        if not world:
            return pts, hits
        info = self.las_info()
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts, hits

    def height_map(self, renderer: Renderer, cell_size: float, lo_xy=None, hi_xy=None, which: str = "top", clip_z=None):
        """A top-down map of the loaded resource, rasterized on the GPU in one pass over the compressed stream (Context.
        grid_accumulate): (height, rgba, count, grid) over the cells of grid_from_world(las_info(), lo_xy, hi_xy, cell_size) --
        lo_xy / hi_xy None: las_info()'s min / max. which="top": per cell the highest point (the surface model and its
        orthophoto), "bottom": the lowest. height is a float64 tensor [h, w] = z * scale + offset of that point, NaN for an
        empty cell; rgba a uint8 tensor [h, w, 4] with its colour and alpha 255, zeros for an empty cell; count an int32
        tensor [h, w] with the bits of the number of points per cell. Row 0 is the southern edge (the lowest y). clip_z:
        (lo, hi) in world units, only the points with lo <= z <= hi count."""
        import torch
        if which not in ("top", "bottom"):
            raise ValueError('which is "top" or "bottom"')
        info = self.las_info()
        lo_xy = (info.min[0], info.min[1]) if lo_xy is None else lo_xy
        hi_xy = (info.max[0], info.max[1]) if hi_xy is None else hi_xy
        grid = grid_from_world(info, lo_xy, hi_xy, cell_size)
        inf = float("inf")
        clip = None if clip_z is None else box_from_world(info, (-inf, -inf, clip_z[0]), (inf, inf, clip_z[1]))
        ctx = renderer.ctx
        dev = torch.device("cuda", ctx.device)
        words = torch.empty((grid.height, grid.width), dtype=torch.int64, device=dev)
        count = torch.empty((grid.height, grid.width), dtype=torch.int32, device=dev)
        planes = dict(top=words) if which == "top" else dict(bottom=words)
        ctx.grid_clear(grid, counts=count, **planes)
        ctx.grid_accumulate(grid, counts=count, clip=clip, **planes)
        z, rgba = ctx.grid_unpack(grid, words, N.GRID_TOP if which == "top" else N.GRID_BOTTOM)
        height = z.to(torch.float64) * float(info.scale[2]) + float(info.offset[2])
        height[rgba == 0] = float("nan")
        return height, rgba.view(torch.uint8).view(grid.height, grid.width, 4), count, grid

    def height_percentiles(self, renderer: Renderer, cell_size: float, percentiles, lo_xy=None, hi_xy=None, clip_z=None, ground=None,
                           cutoff: float = 0.0):
        """Exact height percentiles per cell of the loaded resource, in one call over the compressed stream (Context.
        grid_quantiles): (heights, counts, grid) over the cells of grid_from_world(las_info(), lo_xy, hi_xy, cell_size).
        percentiles: floats in 0 .. 100, each a whole number of basis points (95, 99.5, 2.25; not 33.333). heights is a float64
        tensor [len(percentiles), h, w] in world units, the z of the nearest-rank point (no interpolation), NaN for a cell without
        candidates; counts an int32 tensor [h, w] of candidates per cell. Row 0 is the southern edge. clip_z: (lo, hi) in world
        units. ground: the int32 plane of the same grid that ground_model's filter gives (_ground_planes / Context.
        ground_filter); then only points at least `cutoff` world units above their cell's ground are candidates (counts / all
        points = canopy cover), the heights are above ground, and cells without ground come back NaN with count 0."""
        import torch
        bp = []
        for p in np.atleast_1d(np.asarray(percentiles, np.float64)):
            v = round(float(p) * 100.0)
            if not 0.0 <= p <= 100.0 or abs(float(p) * 100.0 - v) > 1e-6:
                raise ValueError(f"percentile {p}: a value in 0 .. 100 that is a whole number of basis points (hundredths)")
            bp.append(int(v))
        info = self.las_info()
        lo_xy = (info.min[0], info.min[1]) if lo_xy is None else lo_xy
        hi_xy = (info.max[0], info.max[1]) if hi_xy is None else hi_xy
        grid = grid_from_world(info, lo_xy, hi_xy, cell_size)
        inf = float("inf")
        clip = None if clip_z is None else box_from_world(info, (-inf, -inf, clip_z[0]), (inf, inf, clip_z[1]))
        ctx = renderer.ctx
        floor = base = None
        if ground is not None:
            if tuple(ground.shape) != (grid.height, grid.width) or ground.dtype != torch.int32:
                raise ValueError(f"ground must be an int32 tensor of the grid's {grid.height} x {grid.width} cells")
            none = ground == INT32_MIN
            lift = int(np.ceil(cutoff / float(info.scale[2]) - 1e-9))
            floor = torch.clamp(ground.to(torch.int64) + lift, INT32_MIN + 1, INT32_MAX).to(torch.int32)
            base = ground.to(torch.float64)
        planes, counts = ctx.grid_quantiles(grid, bp, clip=clip, floor=None if floor is None else floor.contiguous(), counts=True)
        empty = planes == INT32_MIN
        if ground is None:
            heights = planes.to(torch.float64) * float(info.scale[2]) + float(info.offset[2])
        else:
            heights = (planes.to(torch.float64) - base) * float(info.scale[2])
            empty = empty | none
            counts = torch.where(none, torch.zeros_like(counts), counts)
        heights[empty] = float("nan")
        return heights, counts, grid

    def _ground_planes(self, renderer: Renderer, cell_size: float, lo_xy, hi_xy, pmf: dict):
        """(grid, ground, classes): the ground filter over the lowest-point grid of the resource, int32 / uint8 tensors."""
        import torch
        info = self.las_info()
        lo_xy = (info.min[0], info.min[1]) if lo_xy is None else lo_xy
        hi_xy = (info.max[0], info.max[1]) if hi_xy is None else hi_xy
        grid = grid_from_world(info, lo_xy, hi_xy, cell_size)
        params = pmf.pop("params", None) or ground_params_from_world(info, cell_size, **pmf)
        ctx = renderer.ctx
        words = torch.empty((grid.height, grid.width), dtype=torch.int64, device=torch.device("cuda", ctx.device))
        ctx.grid_clear(grid, bottom=words)
        ctx.grid_accumulate(grid, bottom=words)
        lowest, _ = ctx.grid_unpack(grid, words, N.GRID_BOTTOM)
        ground, classes = ctx.ground_filter(grid, params, lowest)
        return grid, ground, classes

    def ground_model(self, renderer: Renderer, cell_size: float, lo_xy=None, hi_xy=None, **pmf):
        """A terrain model of the loaded resource (Context.grid_accumulate's lowest-point grid through Context.ground_filter):
        (height, classes, grid) over the cells of grid_from_world(las_info(), lo_xy, hi_xy, cell_size), lo_xy / hi_xy None:
        las_info()'s min / max. height is a float64 tensor [h, w] = ground * scale + offset in world units, NaN where the fill
        did not reach; classes a uint8 tensor [h, w] of CELL_EMPTY / CELL_GROUND / CELL_NONGROUND. Row 0 is the southern edge.
        **pmf: ground_params_from_world's arguments (slope, initial_distance, max_distance, max_window, fill_rounds), or
        params=GroundParams(...) in the stream's units."""
        import torch
        info = self.las_info()
        grid, ground, classes = self._ground_planes(renderer, cell_size, lo_xy, hi_xy, dict(pmf))
        height = ground.to(torch.float64) * float(info.scale[2]) + float(info.offset[2])
        height[ground == INT32_MIN] = float("nan")
        return height, classes, grid

    def points_by_height(self, renderer: Renderer, cell_size: float, h_lo: float, h_hi: float, lo=None, hi=None, normalize: bool = False,
                         world: bool = True, **pmf):
        """The points of the loaded resource whose height above the ground model of `cell_size` cells lies in h_lo .. h_hi
        (Context.select_height over ground_model's plane). lo / hi: a box to stay inside (None: las_info()'s min / max); the
        ground model covers its x and y range. normalize: the z of the result is the height. world=True: h_lo / h_hi, lo / hi are
        world units (heights are multiples of scale_z; the offset cancels) and the result is (xyz, pts, h) with xyz and h float64
        tensors; world=False: h_lo / h_hi and lo / hi are the stream's integers, cell_size stays in world units, the result
        (pts, h) with int32 tensors."""
        import math
        import torch
        info = self.las_info()
        sz = float(info.scale[2])
        if world:
            lo_w, hi_w = (tuple(info.min) if lo is None else lo), (tuple(info.max) if hi is None else hi)
            clip = box_from_world(info, lo_w, hi_w)
            lo_xy, hi_xy = lo_w[:2], hi_w[:2]
            h_min = max(INT32_MIN, min(INT32_MAX, math.ceil(h_lo / sz - 1e-9)))
            h_max = max(INT32_MIN, min(INT32_MAX, math.floor(h_hi / sz + 1e-9)))
        else:
            clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
            lo_xy = None if lo is None else tuple(float(lo[k]) * float(info.scale[k]) + float(info.offset[k]) for k in range(2))
            hi_xy = None if hi is None else tuple(float(hi[k]) * float(info.scale[k]) + float(info.offset[k]) for k in range(2))
            h_min, h_max = int(h_lo), int(h_hi)
        grid, ground, _ = self._ground_planes(renderer, cell_size, lo_xy, hi_xy, dict(pmf))
        pts, h = renderer.ctx.select_height(grid, ground, h_min, h_max, clip=clip, replace_z=normalize, heights=True)
        if not world:
            return pts, h
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        xyz = pts[:, :3].to(torch.float64) * so[0] + so[1]
        hw = h.to(torch.float64) * sz
        if normalize:
            xyz[:, 2] = hw
        return xyz, pts, hw

    def thinned(self, renderer: Renderer, cell_size: float, lo=None, hi=None, mode: str = "first", world: bool = True):
        """The loaded resource thinned to one point per cubic voxel of `cell_size`, on the GPU and straight from the compressed
        stream (Context.thin): mode "first" keeps a voxel's first point in the stream's order, "center" the one nearest to the
        voxel's centre. world=True: cell_size, lo and hi are world units -- the lattice is voxels_from_world(las_info(), cell_size)
        (its origin at the header's min corner), the clip box_from_world(las_info(), lo, hi) with lo / hi None: the header's min /
        max, so the tail artefact of a stream written without padding neither lands in the output nor stretches the lattice --
        and the result is (xyz, pts) as points_in_box returns it. world=False: cell_size is a whole number of lattice steps, lo / hi
        are the stream's int32 coordinates (None: no clip), the lattice's origin is (0, 0, 0), the result the int32 tensor alone."""
        import torch
        info = self.las_info()
        if world:
            vox = voxels_from_world(info, cell_size)
            clip = box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        else:
            vox = as_voxels((0, 0, 0, cell_size))
            clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
        pts = renderer.ctx.thin(vox, clip, mode)
        if not world:
            return pts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts

    def lod_ordered(self, renderer: Renderer, cell_size: float, levels: int, lo=None, hi=None, drop_rest: bool = False, world: bool = True):
        """The loaded resource in level-of-detail order, on the GPU and straight from the compressed stream (Context.lod_order):
        `levels` nested voxel lattices, the finest with cells of `cell_size`, every coarser one with cells twice as large; the
        points that are first in a voxel of the coarsest lattice come first, then those of the next level, and so on, last the rest
        (left out with drop_rest=True). Every prefix that ends at a level boundary is thinned() "first" with that level's cell.
        cell_size, lo, hi and world are as for thinned(). world=True: (xyz, pts, level_counts) -- level_counts a list of levels + 1
        numbers, the last one the rest (counted also when it is dropped); world=False: (pts, level_counts)."""
        import torch
        info = self.las_info()
        if world:
            lod = lod_from_world(info, cell_size, levels)
            clip = box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        else:
            lod = as_lod((0, 0, 0, cell_size, levels))
            clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
        pts = renderer.ctx.lod_order(lod, clip, drop_rest=drop_rest)
        counts = renderer.ctx.lod_stats["level_count"][:int(levels) + 1]
        if not world:
            return pts, counts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts, counts

    def voxel_centroids(self, renderer: Renderer, cell_size: float, lo=None, hi=None, world: bool = True):
        """The loaded resource down-sampled to the centroid of every non-empty cubic voxel of `cell_size`, on the GPU and straight
        from the compressed stream (Context.voxel_mean): the mean position, rounded to the stream's lattice inside the voxel, and
        the mean colour of the voxel's points. cell_size, lo, hi and world are as for thinned(). world=True: (xyz, pts, counts) --
        float64 world positions (i * scale + offset), the int32 records and the int64 points per voxel; world=False: (pts, counts)."""
        import torch
        info = self.las_info()
        if world:
            vox = voxels_from_world(info, cell_size)
            clip = box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        else:
            vox = as_voxels((0, 0, 0, cell_size))
            clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
        pts, counts = renderer.ctx.voxel_mean(vox, clip, counts=True)
        if not world:
            return pts, counts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts, counts

    def denoised(self, renderer: Renderer, cell_size: float, max_count: int, lo=None, hi=None, isolated: bool = False, world: bool = True):
        """The loaded resource without its isolated points -- those whose 3 x 3 x 3 cubic voxels of `cell_size` hold at most
        `max_count` points, the point itself included -- or, with isolated=True, those points alone; on the GPU and straight from
        the compressed stream (Context.denoise). cell_size, lo, hi, world and the result are as for thinned(): with world=True the
        clip defaults to the header's box, so the tail artefact of a stream written without padding neither counts as a
        neighbour nor lands in the output."""
        import torch
        info = self.las_info()
        if world:
            vox = voxels_from_world(info, cell_size)
            clip = box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        else:
            vox = as_voxels((0, 0, 0, cell_size))
            clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
        pts = renderer.ctx.denoise(vox, max_count, clip, "isolated" if isolated else "keep")
        if not world:
            return pts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts

    def components(self, renderer: Renderer, cell_size: float, min_points: int = 1, connectivity: int = 26, lo=None, hi=None, small: bool = False,
                   world: bool = True):
        """The loaded resource split into the connected components of its occupied cubic voxels of `cell_size` (adjacent: at most 1
        apart on every axis with connectivity 26, exactly 1 on one axis with 6), without the components of fewer than `min_points`
        points or, with small=True, those alone; on the GPU and straight from the compressed stream (Context.components). Returns
        what denoised() returns with the labels appended -- (xyz, points, labels), with world=False (points, labels) -- labels an
        int64 tensor: per point the least row of its component, rows counted over the whole stream. cell_size, lo, hi and world
        are as for denoised(): with world=True the clip defaults to the header's box."""
        import torch
        info = self.las_info()
        if world:
            vox = voxels_from_world(info, cell_size)
            clip = box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        else:
            vox = as_voxels((0, 0, 0, cell_size))
            clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
        pts, lab = renderer.ctx.components(vox, min_points, connectivity, clip, "small" if small else "keep", labels=True)
        if not world:
            return pts, lab
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts, lab

    def _neighbors_clip(self, info, radius, lo, hi, world):
        if world:
            return radius_from_world(info, radius), box_from_world(info, tuple(info.min) if lo is None else lo, tuple(info.max) if hi is None else hi)
        clip = None if lo is None and hi is None else as_box(((INT32_MIN,) * 3 if lo is None else lo, (INT32_MAX,) * 3 if hi is None else hi))
        return int(radius), clip

    def radius_filtered(self, renderer: Renderer, radius: float, min_count: int, lo=None, hi=None, sparse: bool = False, world: bool = True):
        """The loaded resource without the points that have fewer than `min_count` points within `radius` (the point itself and
        exact duplicates included) or, with sparse=True, those points alone: the radius outlier filter, exact, on the GPU and
        straight from the compressed stream (Context.neighbors). radius is in world units (radius_from_world), with world=False in
        lattice steps; lo, hi, world and the result are as for denoised(): with world=True the clip defaults to the header's box."""
        import torch
        info = self.las_info()
        r, clip = self._neighbors_clip(info, radius, lo, hi, world)
        pts = renderer.ctx.neighbors(r, min_count, clip, "sparse" if sparse else "keep")
        if not world:
            return pts
        so = torch.tensor([tuple(info.scale), tuple(info.offset)], dtype=torch.float64, device=pts.device)
        return pts[:, :3].to(torch.float64) * so[0] + so[1], pts

    def point_spacing(self, renderer: Renderer, radius: float, lo=None, hi=None, world: bool = True):
        """Per point of the loaded resource inside the clip: (points, N, spacing) -- the int32 records, N = the points within
        `radius` (itself included, int64) and the distance to the nearest other point within the radius (float64: sqrt(nn2) *
        scale in world units, with world=False sqrt(nn2) in lattice steps; inf for none). radius, lo, hi and world as for
        radius_filtered()."""
        import torch
        info = self.las_info()
        r, clip = self._neighbors_clip(info, radius, lo, hi, world)
        pts, n, nn2 = renderer.ctx.neighbors(r, 1, clip, "all", counts=True, nn2=True)
        scale = float(info.scale[0]) if world else 1.0
        spacing = torch.where(nn2 < 0, torch.full_like(nn2, float("inf"), dtype=torch.float64), torch.sqrt(nn2.to(torch.float64)) * scale)
        return pts, n, spacing

    def normals(self, renderer: Renderer, radius: float, min_count: int = 3, lo=None, hi=None, world: bool = True):
        """Per point of the loaded resource inside the clip that has at least `min_count` points within `radius` (itself and exact
        duplicates included): (points, normals, curvature) -- the int32 records, the unit normal of the neighbourhood's covariance
        (float64 [n, 3]; its sign is pcr_eigen's, not a viewpoint's) and the curvature l0 / (l0 + l1 + l2) (float64, 0 where the
        sum is 0), on the GPU straight from the compressed stream (Context.local_moments). radius, lo, hi and world as for
        radius_filtered(); radius_from_world refuses differing axis scales, so the normal of the lattice is the world's."""
        import torch
        info = self.las_info()
        r, clip = self._neighbors_clip(info, radius, lo, hi, world)
        pts, eig = renderer.ctx.local_moments(r, min_count, clip, eigen=True)
        total = eig[:, 0] + eig[:, 1] + eig[:, 2]
        curvature = torch.where(total != 0.0, eig[:, 0] / torch.where(total != 0.0, total, torch.ones_like(total)), torch.zeros_like(total))
        return pts, eig[:, 3:6], curvature

    def nearest_neighbors(self, renderer: Renderer, k: int, radius: float, lo=None, hi=None, world: bool = True):
        """Per point of the loaded resource inside the clip: (points, rows, knn_rows, distances) -- the int32 records, their rows,
        the rows of their k nearest other points within `radius` in the order (distance, row) (int64 [n, k], -1 for none; rows as
        Context.knn counts them, over the whole resource) and the distances to them (float64 [n, k]: sqrt(d2) * scale in world
        units, with world=False sqrt(d2) in lattice steps; inf for none), on the GPU straight from the compressed stream
        (Context.knn). radius, lo, hi and world as for radius_filtered(); radius is at most KNN_MAX_RADIUS lattice steps."""
        import torch
        info = self.las_info()
        r, clip = self._neighbors_clip(info, radius, lo, hi, world)
        pts, rows, knn_rows, d2 = renderer.ctx.knn(k, r, 0, clip, rows=True)
        scale = float(info.scale[0]) if world else 1.0
        dist = torch.where(d2 < 0, torch.full_like(d2, float("inf"), dtype=torch.float64), torch.sqrt(d2.clamp(min=0).to(torch.float64)) * scale)
        return pts, rows, knn_rows, dist

    def statistical_outliers(self, renderer: Renderer, k: int, multiplier: float, radius: float, lo=None, hi=None, outliers: bool = False,
                             world: bool = True):
        """The statistical outlier filter with the search capped at `radius`: per point inside the clip the mean distance to its k
        nearest other points within the radius (knn_mean_distance; Context.read_knn with min_found = 0), mu and the population
        sigma of the finite means; a point is an outlier iff its mean is > mu + multiplier * sigma or it has no neighbour within
        the radius. Returns (points, rows) of the inliers, or with outliers=True of the outliers: numpy arrays (POINT_DTYPE,
        int64). radius, lo, hi and world as for radius_filtered(). (PDAL's filters.outlier with method=statistical has mean_k and
        multiplier and no radius; this reading of its definition has not been checked against the tool.)"""
        info = self.las_info()
        r, clip = self._neighbors_clip(info, radius, lo, hi, world)
        pts, rows, _, d2 = renderer.ctx.read_knn(k, r, 0, clip, rows=True)
        out = statistical_outlier_mask(knn_mean_distance(d2, float(info.scale[0]) if world else 1.0), multiplier)
        sel = out if outliers else ~out
        return pts[sel], rows[sel]

    def las_info(self) -> LasInfo:
        """Scale, offset, min and max of the LAS file the stream was made from, as its first batch record carries them (the
        box as floats)."""
        return self.file.batch_las_info(self.first_batch)


class _HuffmanMethod(Method):
    group = "none"
    display: Optional[DisplayOpts] = None     # set: the frame's resolve is the display resolve with these options

    def __init__(self, renderer: Renderer, las: HuffmanLasData):
        self.renderer, self.las = renderer, las

    def update(self, renderer: Renderer):                            # huffman_hqs.h:116-124
        if Runtime.resource is not self.las:
            if Runtime.resource is not None:
                Runtime.resource.unload(renderer)
            self.las.load(renderer)
            Runtime.resource = self.las


class HuffmanMemIter(_HuffmanMethod):
    """modules/huffman_mem_iter_cuda/huffman_mem_iter_cuda.h:122-254: decode + {depth,BC1 colour} atomicMin."""
    name = "huffman_mem_iter_cuda"
    description = "- Decodes Huffman Encoded values on the GPU"

    def render(self, renderer: Renderer):
        """One frame. The reference clears at the END of render() for the next frame (:250-252); headless
        callers want to read the result, so the clear happens at the START of the next frame instead."""
        self.las.process(renderer)
        if self.las.numPointsLoaded == 0:
            return
        p = renderer.render_params()
        ctx = renderer.ctx
        ctx.frame_begin(p)            # CLEAR (of the previous frame) + the cull/LOD prepass, one launch
        ctx.render_basic(p)           # RENDER
        if self.display is not None:  # RESOLVE
            ctx.resolve_basic_display(p, self.display)
        else:
            ctx.resolve_basic(p)
        self.last_params = p


class ComputeHuffman(HuffmanMemIter):
    """modules/huffman_cuda/huffman_cuda.h:60-75: the reference's first Huffman method, registered as "huffman_cuda" (commented
    out in its main.cpp:19, 265 in favour of huffman_mem_iter_cuda: same decode + atomicMin raster). The name north_star lists."""
    name = "huffman_cuda"


class HuffmanHQS(_HuffmanMethod):
    """modules/huffman_hqs/huffman_hqs.h:126-273: depth pass, 1 % colour accumulation pass, averaging resolve."""
    name = "huffman_hqs"
    description = "- Decodes Huffman Encoded values on the GPU"

    def render(self, renderer: Renderer):
        self.las.process(renderer)
        if self.las.numPointsLoaded == 0:
            return
        p = renderer.render_params()
        ctx = renderer.ctx
        ctx.frame_begin(p, hqs=True)
        ctx.render_hqs_depth(p)
        ctx.render_hqs_color(p)
        if self.display is not None:
            ctx.resolve_hqs_display(p, self.display)
        else:
            ctx.resolve_hqs(p)
        self.last_params = p


class ComputeLasData(Resource):
    """modules/compute/ComputeLasLoader.{h,cpp}: a LAS file quantised batch by batch into three 10-10-10 levels.
    The reference uploads raw LAS bytes and quantises in a compute shader (computeLasLoader.cs); here the host library
    quantises (pcr_las_quantize) and the four arrays are uploaded."""

    POINTS_PER_TASK = 100 * POINTS_PER_BATCH      # MAX_POINTS_PER_BATCH, Resources.h:10

    def __init__(self):
        super().__init__()
        self.path = ""
        self.numPoints = self.numPointsLoaded = self.numBatchesLoaded = 0
        self._pts = None
        self.las: Optional[LasInfo] = None

    @staticmethod
    def create(path: str) -> "ComputeLasData":                        # ComputeLasLoader.h:97-103
        return ComputeLasData.from_points(*read_las(path), path=path)

    @staticmethod
    def from_points(x, y, z, color, las: LasInfo, path: str = "<memory>") -> "ComputeLasData":
        d = ComputeLasData()
        d.path, d.las = path, las
        d._pts = tuple(np.ascontiguousarray(a, t) for a, t in ((x, np.int32), (y, np.int32), (z, np.int32), (color, np.uint32)))
        d.numPoints = len(d._pts[0])
        return d

    def load(self, renderer: Renderer):                               # ComputeLasLoader.cpp:14-38
        if self.state != Resource.UNLOADED:
            return
        self.state = Resource.LOADING
        renderer.ctx.las_begin(self.numPoints)
        self.numPointsLoaded = self.numBatchesLoaded = 0

    def process(self, renderer: Renderer):                            # ComputeLasLoader.cpp:140-262
        if self.state != Resource.LOADING:
            return
        a, b = self.numPointsLoaded, min(self.numPoints, self.numPointsLoaded + self.POINTS_PER_TASK)
        q = las_quantize(*(v[a:b] for v in self._pts), self.las)
        renderer.ctx.las_upload(self.numBatchesLoaded, *q)
        self.numPointsLoaded = b
        self.numBatchesLoaded = renderer.ctx.las_batches_loaded
        if b == self.numPoints:
            self.state = Resource.LOADED

    def load_all(self, renderer: Renderer):
        self.load(renderer)
        while self.state == Resource.LOADING:
            self.process(renderer)

    def unload(self, renderer: Renderer):                             # ComputeLasLoader.cpp:114-131
        self.numPointsLoaded = self.numBatchesLoaded = 0
        renderer.ctx.las_unload()
        self.state = Resource.UNLOADED


class ComputeLoopLasCUDA(Method):
    """modules/compute_loop_las_cuda/compute_loop_las_cuda.h:52-222: per-batch level of detail picks how many of the
    three 10-bit levels a workgroup reads; {depth, point index} atomicMin; resolve looks the colour up by index."""
    name = "loop_las_cuda"
    description = "- Each thread renders X points.\n- Loads points from LAS file\n- encodes point coordinates in 10+10+10 bits"
    group = "10-10-10 bit encoded"
    display: Optional[DisplayOpts] = None     # set: the frame's resolve is the display resolve with these options

    def __init__(self, renderer: Renderer, las: ComputeLasData):
        self.renderer, self.las = renderer, las

    def update(self, renderer: Renderer):                             # empty in the reference (:92-93); resource switch as huffman_hqs.h:116-124
        if Runtime.resource is not self.las:
            if Runtime.resource is not None:
                Runtime.resource.unload(renderer)
            self.las.load(renderer)
            Runtime.resource = self.las

    def render(self, renderer: Renderer):                             # compute_loop_las_cuda.h:99-222
        self.las.process(renderer)
        if self.las.numPointsLoaded == 0:
            return
        p = renderer.render_params()
        ctx = renderer.ctx
        ctx.clear()
        ctx.render_las(p)
        if self.display is not None:
            ctx.resolve_las_display(p, self.display)
        else:
            ctx.resolve_las(p)
        self.last_params = p


class ComputeLoopLasHQS(ComputeLoopLasCUDA):
    """modules/compute_loop_las_hqs/compute_loop_las_hqs.h:36-309: the batches and levels of loop_las_cuda, a depth pass, a
    colour pass that averages the points within 1 % of the nearest (w <= d * 1.01f), the averaging resolve of the HQS method."""
    name = "loop_las_hqs"
    description = "Like compute las, but also \naverages overlapping points"
    group = "10-10-10 bit encoded"

    def render(self, renderer: Renderer):                             # compute_loop_las_hqs.h:126-300
        self.las.process(renderer)
        if self.las.numPointsLoaded == 0:
            return
        p = renderer.render_params()
        ctx = renderer.ctx
        ctx.clear()
        ctx.render_las_hqs_depth(p)   # DEPTH   (:172-196)
        ctx.render_las_hqs_color(p)   # COLORS  (:199-223)
        if self.display is not None:  # RESOLVE (:226-245)
            ctx.resolve_hqs_display(p, self.display)
        else:
            ctx.resolve_hqs(p)
        self.last_params = p
