"""pcrhpg24_amd — MI355X-native Huffman point-cloud decode + rasterize path (hot path of rahul-goel/pcrhpg24).

Layout:  csrc/ (HIP kernels, C ABI, CPU encoder)  ·  host.py (the reference's Method/Resource surface over the C ABI)
         ·  dist.py (batch sharding + framebuffer merge over torch.distributed)  ·  build.py (in-tree builds)
"""
from .host import (ComputeHuffman, ComputeLasData, ComputeLoopLasCUDA, ComputeLoopLasHQS, Context, Debug, HuffmanFile, HuffmanHQS, HuffmanLasData, HuffmanMemIter, Method, PcrError,  # noqa: F401
                   Renderer, Resource, Runtime, camera_orbit, encode_points, kernel_version, synth_encode, synth_las_info, synth_points, las_quantize, read_las, write_las, POINT_DTYPE, HIT_DTYPE, as_box, as_rect, box_from_world, as_grid, grid_from_world, GroundParams, ground_params_from_world, as_voxels, voxels_from_world, ROW_DTYPE, Polygon, polygon_from_world)
from ._native import Box, PolygonStats, POLY_MAX_VERTICES, POLY_INVERT, DisplayOpts, Grid, GridStats, GRID_MAX_CELLS, GRID_WINDOW_CELLS, GRID_NO_WINDOW, GRID_TOP, GRID_BOTTOM, GroundStats, HeightStats, GROUND_MAX_STEPS, GROUND_MAX_RADIUS, GROUND_MAX_FILL, GROUND_EMPTY, CELL_EMPTY, CELL_GROUND, CELL_NONGROUND, HEIGHT_REPLACE_Z, Rect, ScreenHit, ScreenStats, SelectStats, ThinStats, DenoiseStats, DENOISE_KEEP, DENOISE_ISOLATED, ComponentsStats, COMPONENTS_KEEP, COMPONENTS_SMALL, Voxels, THIN_FIRST, THIN_CENTER, THIN_MAX_CELL, THIN_MAX_CENTER_CELL, FileHeader, LasInfo, Point, RenderParams, RenderStats, XyzBatch, fb_elems  # noqa: F401
