"""ctypes bindings of the two native libraries. No compute happens in Python.

libpcr_hip.so is the product path: loading it fails loudly (RuntimeError) when the library is
missing — there is no CPU fallback for rendering.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

c_i64, c_i32, c_u64, c_u32, c_f32, c_f64 = C.c_int64, C.c_int32, C.c_uint64, C.c_uint32, C.c_float, C.c_double


class GpuBatch(C.Structure):                      # include/pcr_types.h: pcr_gpu_batch
    _fields_ = [(n, c_f32) for n in ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z")] + \
               [(n, c_f64) for n in ("scale_x", "scale_y", "scale_z", "offset_x", "offset_y", "offset_z",
                                     "las_min_x", "las_min_y", "las_min_z", "las_max_x", "las_max_y", "las_max_z")] + \
               [(n, c_i64) for n in ("encoding_batch_offset", "separate_batch_offset", "decoder_table_offset",
                                     "cluster_sizes_offset", "max_cw_len")]


class XyzBatch(C.Structure):                      # pcr_xyz_batch (kernel_data.h:4-22)
    _fields_ = [("state", c_i32)] + [(n, c_f32) for n in ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z")] + \
               [("num_points", c_i32), ("padding", c_i32 * 8)]


class FileHeader(C.Structure):                    # pcr_file_header
    _fields_ = [(n, c_i64) for n in ("num_points", "num_batches", "encoded_bytes", "separate_bytes", "cluster_bytes")]


class RenderParams(C.Structure):                  # pcr_render_params
    _fields_ = [("transform", c_f32 * 16), ("world_view", c_f32 * 16), ("proj", c_f32 * 16),
                ("width", c_i32), ("height", c_i32), ("points_per_thread", c_i32), ("lod_percent", c_i32),
                ("enable_frustum_culling", c_i32), ("show_num_points", c_i32), ("colorize_chunks", c_i32),
                ("reserved", c_i32)]

    def copy(self) -> "RenderParams":
        out = RenderParams()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(RenderParams))
        return out


class RenderStats(C.Structure):                   # pcr_render_stats
    _fields_ = [(n, c_i64) for n in ("batches_total", "batches_culled", "points_iterated", "batches_double")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class LasInfo(C.Structure):                       # pcr_las_info
    _fields_ = [("scale", c_f64 * 3), ("offset", c_f64 * 3), ("min", c_f64 * 3), ("max", c_f64 * 3)]


class Point(C.Structure):                         # pcr_point: one decoded point, 16 bytes (colour 0x00BBGGRR)
    _fields_ = [("x", c_i32), ("y", c_i32), ("z", c_i32), ("color", c_u32)]


class Box(C.Structure):                           # pcr_box: int32 coordinates, bounds inclusive; min > max on an axis = empty
    _fields_ = [("min", c_i32 * 3), ("max", c_i32 * 3)]


class SelectStats(C.Structure):                   # pcr_select_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_inside", "batches_straddling", "points_selected")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Polygon(C.Structure):                       # pcr_polygon: rings of int32 vertices and a z range, 40 bytes (host.Polygon fills one)
    _fields_ = [("xy", C.POINTER(c_i32)), ("ring_sizes", C.POINTER(c_i32)), ("num_rings", c_i32), ("z_min", c_i32), ("z_max", c_i32),
                ("flags", c_u32), ("reserved", c_u32)]


class PolygonStats(C.Structure):                  # pcr_polygon_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_inside", "batches_straddling", "points_selected", "edges_listed", "edges_max")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


POLY_MAX_VERTICES, POLY_INVERT = 4096, 1                                                                # pcr_types.h


class Slab(C.Structure):                          # pcr_slab: lo <= n.p <= hi in exact integers, 32 bytes (host.Slab fills one)
    _fields_ = [("n", c_i32 * 3), ("reserved", c_i32), ("lo", c_i64), ("hi", c_i64)]


class PlaneStats(C.Structure):                    # pcr_plane_stats
    _fields_ = [(n, c_i64) for n in ("batches_skipped", "batches_whole", "batches_decoded", "hypotheses_listed", "hypotheses_max", "exclusions_listed",
                                     "candidates_decoded", "reserved")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:-1]}


class SlabStats(C.Structure):                     # pcr_slab_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_inside", "batches_straddling", "points_selected", "slabs_listed", "slabs_max")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


SLAB_MAX_NORMAL, SLAB_MAX_BOUND, PLANE_MAX_HYPOTHESES, SLAB_MAX_EXCLUDE, SLAB_MAX_SELECT, SLAB_INVERT = 1 << 20, 1 << 61, 1024, 16, 16, 1    # pcr_types.h


class Grid(C.Structure):                          # pcr_grid: a top-down grid over the stream's int32 x and y, 24 bytes
    _fields_ = [(n, c_i32) for n in ("origin_x", "origin_y", "cell", "width", "height", "reserved")]


class GridStats(C.Structure):                     # pcr_grid_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_windowed", "batches_direct")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


GRID_MAX_CELLS, GRID_WINDOW_CELLS, GRID_NO_WINDOW, GRID_TOP, GRID_BOTTOM = 1 << 26, 4096, 1, 0, 1      # pcr_types.h


class QuantileStats(C.Structure):                 # pcr_quantile_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_windowed", "batches_direct", "candidates", "cells_occupied", "max_cell_points")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


QUANTILE_ONE, QUANTILES_MAX, QUANTILE_MAX_BATCHES = 10000, 8, 65535                                     # pcr_types.h


class GroundParams(C.Structure):                  # pcr_ground_params: the steps of the ground filter and the rounds of its fill, 136 bytes
    _fields_ = [("num_steps", c_i32), ("fill_rounds", c_i32), ("radius", c_i32 * 16), ("threshold", c_i32 * 16)]


class GroundStats(C.Structure):                   # pcr_ground_stats
    _fields_ = [(n, c_i64) for n in ("cells_empty", "cells_ground", "cells_nonground", "cells_filled", "cells_unfilled", "fill_rounds")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class HeightStats(C.Structure):                   # pcr_height_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_decoded", "points_no_ground", "points_selected")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


GROUND_MAX_STEPS, GROUND_MAX_RADIUS, GROUND_MAX_FILL, GROUND_EMPTY = 16, 64, 4096, -(1 << 31)          # pcr_types.h
CELL_EMPTY, CELL_GROUND, CELL_NONGROUND, HEIGHT_REPLACE_Z = 0, 1, 2, 1


class Voxels(C.Structure):                        # pcr_voxels: a lattice of cubic voxels over the stream's int32 coordinates, 16 bytes
    _fields_ = [("origin", c_i32 * 3), ("cell", c_i32)]


class ThinStats(C.Structure):                     # pcr_thin_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_decoded", "points_considered", "runs", "points_kept", "table_slots")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


THIN_FIRST, THIN_CENTER, THIN_MAX_CELL, THIN_MAX_CENTER_CELL = 0, 1, 1 << 30, 2048                      # pcr_types.h
VOXEL_MEAN_MAX_ROWS = 1 << 32                                                                           # pcr_types.h
LOD_MAX_LEVELS, LOD_DROP_REST, LOD_ROW_ORDER = 16, 1, 2                                                 # pcr_types.h


class Lod(C.Structure):                           # pcr_lod: nested lattices, level l with the cell cell << (levels - 1 - l), 24 bytes
    _fields_ = [("origin", c_i32 * 3), ("cell", c_i32), ("levels", c_i32), ("reserved", c_i32)]


class LodStats(C.Structure):                      # pcr_lod_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_decoded", "points_considered", "runs", "table_slots", "points_written")] + [
        ("level_count", c_i64 * (LOD_MAX_LEVELS + 1))]

    def as_dict(self) -> dict:
        d = {n: int(getattr(self, n)) for n, _ in self._fields_[:-1]}
        d["level_count"] = [int(v) for v in self.level_count]
        return d


class DenoiseStats(C.Structure):                  # pcr_denoise_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_decoded", "points_considered", "runs", "voxels", "voxels_isolated",
                                     "points_isolated", "points_written", "table_slots")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


DENOISE_KEEP, DENOISE_ISOLATED = 0, 1                                                                   # pcr_types.h


class ComponentsStats(C.Structure):               # pcr_components_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_decoded", "points_considered", "runs", "voxels", "components", "components_small",
                                     "points_small", "largest_points", "points_written", "table_slots")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


COMPONENTS_KEEP, COMPONENTS_SMALL = 0, 1                                                                # pcr_types.h


class NeighborsStats(C.Structure):                # pcr_neighbors_stats
    _fields_ = [(n, c_i64) for n in ("batches_outside", "batches_decoded", "points_considered", "runs", "voxels", "table_slots", "max_voxel_points",
                                     "pairs_bound", "points_sparse", "points_written")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


NEIGHBORS_ALL, NEIGHBORS_KEEP, NEIGHBORS_SPARSE, NEIGHBORS_MAX_RADIUS, NN2_NONE = 0, 1, 2, 1 << 20, (1 << 64) - 1   # pcr_types.h


class Moments(C.Structure):                       # pcr_moments: n, the sums of the offsets, the sums of their products xx xy xz yy yz zz
    _fields_ = [("n", c_i64), ("s", c_i64 * 3), ("q", c_i64 * 6)]


class Eigen(C.Structure):                         # pcr_eigen: the eigenvalues of the covariance, ascending; the unit normal
    _fields_ = [("value", C.c_double * 3), ("normal", C.c_double * 3)]


MOMENTS_MAX_RADIUS = 32767                                                                              # pcr_types.h
KNN_MAX_K, KNN_MAX_RADIUS, KNN_NONE = 16, 32767, (1 << 64) - 1                                          # pcr_types.h


class Rect(C.Structure):                          # pcr_rect: pixel bounds, inclusive; x0 > x1 or y0 > y1 = empty
    _fields_ = [(n, c_i32) for n in ("x0", "y0", "x1", "y1")]


class ScreenHit(C.Structure):                     # pcr_screen_hit: where a selected point lands in the frame, 16 bytes
    _fields_ = [("pixel", c_u32), ("depth_bits", c_u32), ("index", c_i64)]


class ScreenStats(C.Structure):                   # pcr_screen_stats
    _fields_ = [(n, c_i64) for n in ("batches_skipped", "batches_decoded", "points_tested", "points_selected")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


VISIBLE_FRONT, VISIBLE_SURFACE, VISIBLE_MAX_RADIUS = 0, 1, 8                                            # pcr_types.h


class VisibleStats(C.Structure):                  # pcr_visible_stats
    _fields_ = [(n, c_i64) for n in ("batches_skipped", "batches_decoded", "hits", "pixels_covered", "candidates", "selected")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class DisplayOpts(C.Structure):                   # pcr_display_opts: point size and eye-dome lighting of a display resolve, 16 bytes
    _fields_ = [("window", c_i32), ("edl_window", c_i32), ("edl_strength", c_f32), ("reserved", c_i32)]


class EncodeStats(C.Structure):                   # pcr_encode_stats
    _fields_ = [(n, c_i64) for n in ("num_points_in", "num_points", "num_batches", "encoded_bytes", "separate_bytes",
                                     "cluster_bytes", "escaped_symbols", "total_symbols", "file_bytes")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


assert C.sizeof(Point) == 16 and C.sizeof(Box) == 24 and C.sizeof(SelectStats) == 32
assert C.sizeof(Polygon) == 40 and C.sizeof(PolygonStats) == 48
assert C.sizeof(Slab) == 32 and C.sizeof(PlaneStats) == 64 and C.sizeof(SlabStats) == 48
assert C.sizeof(Rect) == 16 and C.sizeof(ScreenHit) == 16 and C.sizeof(ScreenStats) == 32 and C.sizeof(VisibleStats) == 48
assert C.sizeof(DisplayOpts) == 16
assert C.sizeof(Grid) == 24 and C.sizeof(GridStats) == 24 and C.sizeof(QuantileStats) == 48
assert C.sizeof(GroundParams) == 136 and C.sizeof(GroundStats) == 48 and C.sizeof(HeightStats) == 32
assert C.sizeof(Voxels) == 16 and C.sizeof(ThinStats) == 48 and C.sizeof(DenoiseStats) == 72 and C.sizeof(ComponentsStats) == 88
assert C.sizeof(Lod) == 24 and C.sizeof(LodStats) == 48 + 8 * (LOD_MAX_LEVELS + 1)
assert C.sizeof(NeighborsStats) == 80 and C.sizeof(Moments) == 80 and C.sizeof(Eigen) == 48
assert C.sizeof(XyzBatch) == 64 and C.sizeof(GpuBatch) == 160 and C.sizeof(FileHeader) == 40 and C.sizeof(RenderParams) == 224


def fb_elems(w: int, h: int) -> int:
    return w * (h + 1) + 1


HIP_SYMBOLS = [
    "pcr_create", "pcr_destroy", "pcr_last_error", "pcr_set_stream", "pcr_synchronize",
    "pcr_stream_begin", "pcr_upload_batch", "pcr_upload_batches", "pcr_upload_tail", "pcr_stream_unload", "pcr_batches_loaded",
    "pcr_points_loaded", "pcr_set_image_size", "pcr_clear", "pcr_render_basic", "pcr_render_hqs_depth",
    "pcr_render_hqs_color", "pcr_resolve_basic", "pcr_resolve_hqs", "pcr_get_stats", "pcr_read_framebuffer",
    "pcr_read_accum", "pcr_read_rgba", "pcr_device_framebuffer", "pcr_device_rg", "pcr_device_ba", "pcr_framebuffer_private",
    "pcr_use_external_buffers", "pcr_merge_min", "pcr_merge_sum", "pcr_flip_sign", "pcr_timing_begin",
    "pcr_timing_end", "pcr_kernel_timing_enable", "pcr_kernel_timing_read", "pcr_measure_hbm",
    "pcr_frame_begin", "pcr_frame_turn", "pcr_set_stream_layout", "pcr_set_hbm_budget", "pcr_stream_layout", "pcr_set_render_variant", "pcr_set_workgroup_parts", "pcr_set_int64_mergeable", "pcr_fence_record", "pcr_fence_wait", "pcr_merge_min_slices", "pcr_resolve_basic_range", "pcr_set_async_upload", "pcr_batches_resident", "pcr_last_frame_batches", "pcr_stream_algorithmic_bytes", "pcr_last_frame_algorithmic_bytes", "pcr_stream_resident_bytes", "pcr_stream_color_format", "pcr_kernel_version", "pcr_get_stream", "pcr_get_device", "pcr_framebuffer_elems", "pcr_framebuffer_capacity", "pcr_device_rgba", "pcr_resolve_hqs_range",
    "pcr_las_begin", "pcr_las_upload", "pcr_las_unload", "pcr_las_batches_loaded", "pcr_render_las", "pcr_resolve_las",
    "pcr_render_las_hqs_depth", "pcr_render_las_hqs_color",
    "pcr_las_algorithmic_bytes", "pcr_gpu_encode_points", "pcr_gpu_encode_free",
    "pcr_decode_points", "pcr_read_points",
    "pcr_batch_point_bounds", "pcr_select_box", "pcr_read_box",
    "pcr_select_polygon", "pcr_read_polygon",
    "pcr_plane_support", "pcr_select_slabs", "pcr_read_slabs",
    "pcr_select_screen", "pcr_read_screen", "pcr_pick",
    "pcr_select_visible", "pcr_read_visible",
    "pcr_resolve_basic_display", "pcr_resolve_hqs_display", "pcr_resolve_las_display",
    "pcr_grid_clear", "pcr_grid_accumulate", "pcr_grid_unpack", "pcr_read_grid",
    "pcr_grid_quantiles", "pcr_read_grid_quantiles",
    "pcr_ground_filter", "pcr_read_ground", "pcr_select_height", "pcr_read_height",
    "pcr_thin", "pcr_read_thin",
    "pcr_denoise", "pcr_read_denoise",
    "pcr_components", "pcr_read_components",
    "pcr_neighbors", "pcr_read_neighbors",
    "pcr_local_moments", "pcr_read_local_moments", "pcr_moments_eigen",
    "pcr_knn", "pcr_read_knn",
    "pcr_voxel_mean", "pcr_read_voxel_mean",
    "pcr_lod_order", "pcr_read_lod_order",
]

HOST_SYMBOLS = [
    "pcr_host_last_error", "pcr_host_free", "pcr_encode_points", "pcr_synth_points", "pcr_synth_las_info",
    "pcr_synth_encode", "pcr_morton_key", "pcr_huffman_build", "pcr_pack_chain", "pcr_table_from_dict",
    "pcr_bc1_encode_block", "pcr_bc7_encode_block", "pcr_las_quantize", "pcr_camera_orbit",
    "pcr_write_las", "pcr_write_las_points",
]

_hip = None
_host = None


def hip_lib() -> C.CDLL:
    """The HIP library. Raises if it is not built — the product has no other rendering path."""
    global _hip
    if _hip is None:
        path = _build.HIP_LIB
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `python -m pcrhpg24_amd.build` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # One HIP runtime per process: torch ships its own libamdhip64/libhsa-runtime64 under torch/lib with the same
        # SONAMEs as /opt/rocm's. Whichever copy is mapped first serves both torch and this library; with ROCm's mapped
        # first, torch's own device initialisation later fails ("No HIP GPUs are available"). torch is the plumbing for
        # streams and RCCL on the multi-GPU path, so its copy goes first whenever torch is installed.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(path)
        lib.pcr_last_error.restype = C.c_char_p
        lib.pcr_last_error.argtypes = [C.c_void_p]
        lib.pcr_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.pcr_destroy.argtypes = [C.c_void_p]
        lib.pcr_destroy.restype = None
        for n in ("pcr_batches_loaded", "pcr_points_loaded", "pcr_stream_algorithmic_bytes", "pcr_last_frame_algorithmic_bytes", "pcr_stream_resident_bytes", "pcr_las_batches_loaded",
                  "pcr_las_algorithmic_bytes"):
            getattr(lib, n).restype = c_i64
            getattr(lib, n).argtypes = [C.c_void_p]
        for n in ("pcr_device_framebuffer", "pcr_device_rg", "pcr_device_ba"):
            getattr(lib, n).restype = C.c_void_p
            getattr(lib, n).argtypes = [C.c_void_p]
        lib.pcr_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.pcr_synchronize.argtypes = [C.c_void_p]
        lib.pcr_stream_begin.argtypes = [C.c_void_p, C.POINTER(FileHeader), c_i64]
        lib.pcr_upload_batch.argtypes = [C.c_void_p, c_i64, C.c_void_p, C.c_size_t]
        lib.pcr_upload_batches.argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        lib.pcr_upload_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.pcr_stream_unload.argtypes = [C.c_void_p]
        lib.pcr_set_image_size.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.pcr_clear.argtypes = [C.c_void_p]
        for n in ("pcr_render_basic", "pcr_render_hqs_depth", "pcr_render_hqs_color", "pcr_resolve_basic", "pcr_resolve_hqs"):
            getattr(lib, n).argtypes = [C.c_void_p, C.POINTER(RenderParams)]
        for n in ("pcr_render_las", "pcr_resolve_las", "pcr_render_las_hqs_depth", "pcr_render_las_hqs_color"):
            getattr(lib, n).argtypes = [C.c_void_p, C.POINTER(RenderParams)]
        lib.pcr_gpu_encode_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.POINTER(LasInfo),
                                              C.c_int, c_i64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(EncodeStats)]
        lib.pcr_gpu_encode_free.argtypes = [C.c_void_p]
        lib.pcr_gpu_encode_free.restype = None
        lib.pcr_las_begin.argtypes = [C.c_void_p, c_i64]
        lib.pcr_las_upload.argtypes = [C.c_void_p, c_i64, c_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pcr_las_unload.argtypes = [C.c_void_p]
        lib.pcr_get_stats.argtypes = [C.c_void_p, C.POINTER(RenderStats)]
        lib.pcr_read_framebuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.pcr_read_accum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.pcr_read_rgba.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.pcr_use_external_buffers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pcr_merge_min.argtypes = [C.c_void_p, C.c_void_p]
        lib.pcr_merge_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pcr_flip_sign.argtypes = [C.c_void_p]
        lib.pcr_timing_begin.argtypes = [C.c_void_p]
        lib.pcr_timing_end.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        lib.pcr_measure_hbm.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.pcr_frame_begin.argtypes = [C.c_void_p, C.POINTER(RenderParams), C.c_int]
        lib.pcr_frame_turn.argtypes = [C.c_void_p, C.POINTER(RenderParams), C.POINTER(RenderParams), C.c_int]
        lib.pcr_kernel_version.restype = C.c_char_p
        lib.pcr_kernel_version.argtypes = []
        lib.pcr_stream_resident_bytes.restype = C.c_int64
        lib.pcr_stream_resident_bytes.argtypes = [C.c_void_p]
        lib.pcr_stream_color_format.restype = C.c_int
        lib.pcr_stream_color_format.argtypes = [C.c_void_p]
        lib.pcr_set_stream_layout.argtypes = [C.c_void_p, C.c_int]
        lib.pcr_set_render_variant.argtypes = [C.c_void_p, C.c_int]
        lib.pcr_set_workgroup_parts.argtypes = [C.c_void_p, C.c_int]
        lib.pcr_framebuffer_private.argtypes = [C.c_void_p]
        lib.pcr_set_int64_mergeable.argtypes = [C.c_void_p, C.c_int]
        lib.pcr_merge_min_slices.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]
        lib.pcr_resolve_basic_range.argtypes = [C.c_void_p, C.POINTER(RenderParams), C.c_void_p, C.c_size_t, C.c_void_p]
        lib.pcr_resolve_hqs_range.argtypes = [C.c_void_p, C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.pcr_set_hbm_budget.argtypes = [C.c_void_p, C.c_int64]
        lib.pcr_stream_layout.argtypes = [C.c_void_p]
        lib.pcr_last_frame_algorithmic_bytes.argtypes = [C.c_void_p]
        lib.pcr_last_frame_algorithmic_bytes.restype = C.c_int64
        lib.pcr_framebuffer_capacity.argtypes = [C.c_void_p]
        lib.pcr_framebuffer_capacity.restype = C.c_size_t
        lib.pcr_device_rgba.argtypes = [C.c_void_p]
        lib.pcr_device_rgba.restype = C.c_void_p
        lib.pcr_fence_record.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.pcr_fence_wait.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.pcr_set_async_upload.argtypes = [C.c_void_p, C.c_int]
        lib.pcr_batches_resident.argtypes = [C.c_void_p]
        lib.pcr_batches_resident.restype = C.c_int64
        lib.pcr_last_frame_batches.argtypes = [C.c_void_p]
        lib.pcr_last_frame_batches.restype = C.c_int64
        lib.pcr_kernel_timing_enable.argtypes = [C.c_void_p, C.c_int]
        lib.pcr_kernel_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        lib.pcr_decode_points.argtypes = [C.c_void_p, c_i64, c_i64, C.c_void_p, C.c_size_t]
        lib.pcr_read_points.argtypes = [C.c_void_p, c_i64, c_i64, C.c_void_p, C.c_size_t]
        lib.pcr_batch_point_bounds.argtypes = [C.c_void_p, c_i64, c_i64, C.c_void_p]
        for n in ("pcr_select_box", "pcr_read_box"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Box), C.c_void_p, C.c_size_t, C.POINTER(c_i64), C.POINTER(SelectStats)]
        for n in ("pcr_select_polygon", "pcr_read_polygon"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Polygon), C.c_void_p, C.c_size_t, C.POINTER(c_i64), C.POINTER(PolygonStats)]
        lib.pcr_plane_support.argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Slab), C.c_int, C.POINTER(Box), C.POINTER(Slab), C.c_int, C.POINTER(c_i64),
                                          C.POINTER(PlaneStats)]
        for n in ("pcr_select_slabs", "pcr_read_slabs"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Slab), C.c_int, C.POINTER(Box), c_u32, C.c_void_p, C.c_size_t, C.POINTER(c_i64),
                                        C.POINTER(SlabStats)]
        for n in ("pcr_select_screen", "pcr_read_screen"):
            getattr(lib, n).argtypes = [C.c_void_p, C.POINTER(RenderParams), C.POINTER(Rect), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(c_i64),
                                        C.POINTER(ScreenStats)]
        lib.pcr_pick.argtypes = [C.c_void_p, C.POINTER(RenderParams), C.c_int, C.c_int, C.c_int, C.POINTER(Point), C.POINTER(ScreenHit), C.POINTER(C.c_int)]
        for n in ("pcr_select_visible", "pcr_read_visible"):
            getattr(lib, n).argtypes = [C.c_void_p, C.POINTER(RenderParams), C.POINTER(Rect), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.POINTER(c_i64), C.POINTER(VisibleStats)]
        for n in ("pcr_resolve_basic_display", "pcr_resolve_hqs_display", "pcr_resolve_las_display"):
            getattr(lib, n).argtypes = [C.c_void_p, C.POINTER(RenderParams), C.POINTER(DisplayOpts)]
        lib.pcr_grid_clear.argtypes = [C.c_void_p, C.POINTER(Grid), C.c_void_p, C.c_void_p, C.c_void_p]
        for n in ("pcr_grid_accumulate", "pcr_read_grid"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Grid), C.POINTER(Box), C.c_void_p, C.c_void_p, C.c_void_p, c_u32,
                                        C.POINTER(GridStats)]
        for n in ("pcr_grid_quantiles", "pcr_read_grid_quantiles"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Grid), C.POINTER(Box), C.c_void_p, C.POINTER(c_u32), c_i32, C.c_void_p,
                                        C.c_void_p, c_u32, C.POINTER(QuantileStats)]
        lib.pcr_grid_unpack.argtypes = [C.c_void_p, C.POINTER(Grid), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.pcr_ground_filter.argtypes = [C.c_void_p, C.POINTER(Grid), C.POINTER(GroundParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GroundStats)]
        lib.pcr_read_ground.argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Grid), C.POINTER(Box), C.POINTER(GroundParams), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(GroundStats)]
        for n in ("pcr_select_height", "pcr_read_height"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Grid), C.c_void_p, C.POINTER(Box), c_i32, c_i32, c_u32, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.POINTER(c_i64), C.POINTER(HeightStats)]
        for n in ("pcr_thin", "pcr_read_thin"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Voxels), C.POINTER(Box), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(c_i64), C.POINTER(ThinStats)]
        for n in ("pcr_denoise", "pcr_read_denoise"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Voxels), C.POINTER(Box), c_i64, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(c_i64), C.POINTER(DenoiseStats)]
        for n in ("pcr_components", "pcr_read_components"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Voxels), C.POINTER(Box), C.c_int, c_i64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.POINTER(c_i64), C.POINTER(ComponentsStats)]
        for n in ("pcr_neighbors", "pcr_read_neighbors"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, c_i32, C.POINTER(Box), c_i64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.POINTER(c_i64), C.POINTER(NeighborsStats)]
        for n in ("pcr_local_moments", "pcr_read_local_moments"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, c_i32, C.POINTER(Box), c_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.POINTER(c_i64), C.POINTER(NeighborsStats)]
        lib.pcr_moments_eigen.argtypes = [C.c_void_p, C.c_void_p, c_i64, C.c_void_p]
        for n in ("pcr_knn", "pcr_read_knn"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.c_int, c_i32, C.POINTER(Box), c_i64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.POINTER(c_i64), C.POINTER(NeighborsStats)]
        for n in ("pcr_voxel_mean", "pcr_read_voxel_mean"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Voxels), C.POINTER(Box), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(c_i64), C.POINTER(ThinStats)]
        for n in ("pcr_lod_order", "pcr_read_lod_order"):
            getattr(lib, n).argtypes = [C.c_void_p, c_i64, c_i64, C.POINTER(Lod), C.POINTER(Box), c_u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(c_i64), C.POINTER(LodStats)]
        _hip = lib
    return _hip


def host_lib() -> C.CDLL:
    global _host
    if _host is None:
        path = _build.HOST_LIB
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `python -m pcrhpg24_amd.build`")
        lib = C.CDLL(path)
        lib.pcr_host_last_error.restype = C.c_char_p
        lib.pcr_host_free.argtypes = [C.c_void_p]
        lib.pcr_host_free.restype = None
        lib.pcr_encode_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.POINTER(LasInfo),
                                          C.c_int, c_i64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                          C.POINTER(EncodeStats)]
        lib.pcr_synth_points.argtypes = [c_i64, c_u64, c_i64, c_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pcr_synth_las_info.argtypes = [c_i64, c_u64, C.POINTER(LasInfo)]
        lib.pcr_synth_encode.argtypes = [c_i64, c_u64, c_i64, c_i64, c_i64, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_size_t), C.POINTER(EncodeStats)]
        lib.pcr_morton_key.argtypes = [c_u32, c_u32, c_u32, C.POINTER(c_u32), C.POINTER(c_u64)]
        lib.pcr_morton_key.restype = None
        lib.pcr_huffman_build.argtypes = [C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.c_void_p, C.c_void_p]
        lib.pcr_pack_chain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, c_i64,
                                       C.POINTER(C.c_void_p), C.POINTER(c_i32), C.POINTER(C.c_void_p), C.POINTER(c_i32),
                                       C.POINTER(C.c_void_p)]
        lib.pcr_table_from_dict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.c_void_p, C.c_void_p]
        lib.pcr_bc1_encode_block.argtypes = [C.c_void_p, C.c_void_p]
        lib.pcr_bc1_encode_block.restype = None
        lib.pcr_bc7_encode_block.argtypes = [C.c_void_p, C.c_void_p]
        lib.pcr_bc7_encode_block.restype = None
        lib.pcr_las_quantize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.POINTER(LasInfo), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.pcr_camera_orbit.argtypes = [c_f64, c_f64, c_f64, C.POINTER(c_f64), C.c_int, C.c_int, c_f64, c_f64, c_f64,
                                         C.POINTER(RenderParams)]
        lib.pcr_write_las.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.POINTER(LasInfo)]
        lib.pcr_write_las_points.argtypes = [C.c_char_p, C.c_void_p, c_i64, C.POINTER(LasInfo)]
        _host = lib
    return _host


def host_error() -> str:
    return (host_lib().pcr_host_last_error() or b"").decode()
