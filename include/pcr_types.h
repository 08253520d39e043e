/*
 * pcr_types.h — plain-old-data types shared by the C ABI (pcr_hip.h), the HIP kernels,
 * the host-side method/resource adapters and the CPU oracle.
 *
 * Every struct is little-endian, naturally aligned, and free of pointers so it can be passed
 * through cgo / ctypes / JNI unchanged.
 *
 * Reference interfaces these mirror (paths relative to the reference checkout):
 *   pcr_gpu_batch      <- struct GPUBatch, modules/huffman_cuda/huffman_kernel_data.h:4-38 (160 B, same field order)
 *   pcr_render_params  <- struct ChangingRenderData + Mat, modules/compute_loop_las_cuda/kernel_data.h:24-26,54-74
 *                         (only the fields the Huffman kernels read; own packing, no CUDA int2 alignment quirk)
 *   pcr_file_header    <- 5 x int64 at the start of a .huffman file, src/preprocess.cpp:1205-1234,
 *                         modules/compute/HuffmanLasLoader.h:57-85
 *   geometry constants <- modules/compute/Resources.h:4-15
 */
#ifndef PCR_TYPES_H
#define PCR_TYPES_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* modules/compute/Resources.h:4-15 */
#define PCR_POINTS_PER_THREAD     64
#define PCR_WORKGROUP_SIZE        1024
#define PCR_CLUSTERS_PER_THREAD   1
#define PCR_POINTS_PER_BATCH      (PCR_POINTS_PER_THREAD * PCR_WORKGROUP_SIZE) /* 65536 */
#define PCR_HUFFMAN_TABLE_SIZE    4096
#define PCR_MAX_CW_LEN            12
#define PCR_CLUSTER_LANES         32     /* the stream is interleaved for 32-lane clusters (src/preprocess.cpp:540-587) */
#define PCR_CLUSTERS_PER_BATCH    (PCR_WORKGROUP_SIZE / PCR_CLUSTER_LANES)     /* 32 */
#define PCR_COLOR_BYTES_PER_BATCH (PCR_POINTS_PER_BATCH / 2)                   /* BC1: 8 B per 16 points */
#define PCR_COLOR_BYTES_PER_BATCH_BC7 PCR_POINTS_PER_BATCH                     /* BC7 mode 6: 16 B per 16 points (COLOR_COMPRESSION == 7) */
/* colour format of a stream (the reference's compile-time COLOR_COMPRESSION, BatchDumpData.h:130-136): told by the size of its records */
#define PCR_COLOR_BC1 1
#define PCR_COLOR_BC7 7
#define PCR_BATCH_FIXED_HEADER    124    /* bytes before start_values in a batch record (include/BatchDumpData.h:60-107) */

/* Zero padding (in 32-bit words) kept behind the encoded / escape streams so the reference's tail
 * over-reads stay inside the allocation. The reference pads EncodedData with
 * 4*1024 bytes (modules/compute/HuffmanLasLoader.cpp:39-41) and SeparateData with nothing. */
#define PCR_ENCODED_PAD_WORDS     1024
#define PCR_SEPARATE_PAD_WORDS    256
/* Zero words kept behind each pad that no upload ever writes: device loads clamp their index into them. */
#define PCR_GUARD_WORDS           8

/* u64 words allocated behind each of a context's own framebuffers (and u32 behind its RGBA8 image): room for the frame to
 * be cut into N equal slices (N <= 128) by the sliced multi-GPU exchange of include/pcr_dist.h. */
#define PCR_FRAME_PAD_ELEMS       256

#define PCR_BACKGROUND_COLOR      0x00443322u /* resolve.cu:166 */

/* struct GPUBatch (160 bytes) */
typedef struct pcr_gpu_batch {
    float   min_x, min_y, min_z;
    float   max_x, max_y, max_z;
    double  scale_x, scale_y, scale_z;
    double  offset_x, offset_y, offset_z;
    double  las_min_x, las_min_y, las_min_z;
    double  las_max_x, las_max_y, las_max_z;
    int64_t encoding_batch_offset;   /* word offset into EncodedData   */
    int64_t separate_batch_offset;   /* word offset into SeparateData  */
    int64_t decoder_table_offset;    /* entry offset into the tables   */
    int64_t cluster_sizes_offset;    /* entry offset into ClusterSizes */
    int64_t max_cw_len;              /* 12 */
} pcr_gpu_batch;

/* struct XYZBatch of the 10-10-10 path (modules/compute_loop_las_cuda/kernel_data.h:4-22, 64 bytes): bounding box of
 * the batch relative to the cloud's box minimum, and how many of its 65 536 slots hold real points. */
typedef struct pcr_xyz_batch {
    int32_t state;
    float   min_x, min_y, min_z;
    float   max_x, max_y, max_z;
    int32_t num_points;
    int32_t padding[8];
} pcr_xyz_batch;

/* First 40 bytes of a .huffman file. */
typedef struct pcr_file_header {
    int64_t num_points;      /* after padding; multiple of 65536 */
    int64_t num_batches;
    int64_t encoded_bytes;   /* sum over batches of 4*len(encoding)  */
    int64_t separate_bytes;  /* sum over batches of 4*len(separate)  */
    int64_t cluster_bytes;   /* 128 * num_batches */
} pcr_file_header;

/* Per-frame parameters (the fields of ChangingRenderData the Huffman kernels read).
 * Matrices are 4 rows of 4 floats: pos[r] = dot(row r, (x,y,z,1)). The reference host stores
 * glm::transpose(proj*view*world) there (modules/huffman_hqs/huffman_hqs.h:167-169), i.e. exactly rows. */
typedef struct pcr_render_params {
    float   transform[16];            /* uTransform  = proj * view * world */
    float   world_view[16];           /* uWorldView  = view * world        */
    float   proj[16];                 /* uProj                              */
    int32_t width, height;            /* uImageSize                         */
    int32_t points_per_thread;        /* uPointsPerThread, must be 64       */
    int32_t lod_percent;              /* uPointFormat = (int)(Debug::LOD*100), default 10 */
    int32_t enable_frustum_culling;   /* uEnableFrustumCulling, default 1   */
    int32_t show_num_points;          /* debug payload modes (render.cu:289-294) */
    int32_t colorize_chunks;
    int32_t reserved;
} pcr_render_params;

/* Counters a render call reports back (what the metric is computed from: SURVEY 8d). */
typedef struct pcr_render_stats {
    int64_t batches_total;
    int64_t batches_culled;
    int64_t points_iterated;   /* sum over non-culled batches of 1024 * NumPointsToRender */
    int64_t batches_double;    /* batches that took the double-precision dequantisation path */
} pcr_render_stats;

/* One decoded point (pcr_decode_points / pcr_read_points, pcr_write_las_points): the int32 LAS coordinates of the stream and
 * the colour as 0x00BBGGRR, 16 bytes. */
typedef struct pcr_point {
    int32_t  x, y, z;
    uint32_t color;
} pcr_point;

/* An axis-aligned box in the stream's int32 coordinates (pcr_select_box), bounds inclusive. min[k] > max[k] on any axis: the
 * empty box. */
typedef struct pcr_box {
    int32_t min[3], max[3];
} pcr_box;

/* What a selection did (pcr_select_box / pcr_read_box): the batches of the range by their exact box against the query -- wholly
 * outside (not decoded), wholly inside (decoded whole), straddling (decoded twice: counted, then written) -- and the records
 * selected, which is the call's *out_count. */
typedef struct pcr_select_stats {
    int64_t batches_outside;
    int64_t batches_inside;
    int64_t batches_straddling;
    int64_t points_selected;
} pcr_select_stats;

/* A polygon prism in the stream's int32 coordinates (pcr_select_polygon), 40 bytes: rings of vertices in x and y, a z range.
 * Ring vertices v0..v(m-1) give the edges (v_i, v_((i+1) mod m)): a ring is closed implicitly, a repeated closing vertex is
 * harmless. in_poly(x, y): take every edge of every ring, ordered so that l.y < u.y (horizontal edges never count); an edge
 * counts iff l.y <= y < u.y and (x - l.x) * (u.y - l.y) < (y - l.y) * (u.x - l.x), the products exact; in_poly is true iff the
 * number of counting edges is odd -- the even-odd rule with a half-open boundary: further rings are holes or islands, the
 * rectangle (x0,y0),(x1,y0),(x1,y1),(x0,y1) selects x0 <= x < x1, y0 <= y < y1, and of two polygons that share an edge exactly
 * one takes a point on it. A record is selected iff z_min <= z <= z_max and in_poly(x, y) != (flags & PCR_POLY_INVERT).
 * The bounding rectangle of all vertices spans at most 2^31 - 1 on x and on y. */
#define PCR_POLY_MAX_VERTICES 4096
#define PCR_POLY_INVERT 1u            /* flags: keep the points NOT inside the polygon (the z range still applies) */
typedef struct pcr_polygon {
    const int32_t *xy;           /* x0, y0, x1, y1, ...: the vertices of all rings, ring after ring, stream coordinates */
    const int32_t *ring_sizes;   /* vertices of each ring, each >= 3 */
    int32_t num_rings;           /* >= 1 */
    int32_t z_min, z_max;        /* inclusive; z_min > z_max: the empty query */
    uint32_t flags;
    uint32_t reserved;           /* 0 */
} pcr_polygon;

/* What a polygon selection did (pcr_select_polygon / pcr_read_polygon): the batches of the range by their exact box against the
 * prism (pcr_hip.h has the rule) -- outside (not decoded), inside (decoded whole), straddling (counted, then written, each point
 * tested against the batch's own edge list) -- the records selected, which is the call's *out_count, and the sum and the
 * largest of the straddling batches' edge lists. */
typedef struct pcr_polygon_stats {
    int64_t batches_outside;
    int64_t batches_inside;
    int64_t batches_straddling;
    int64_t points_selected;
    int64_t edges_listed;
    int64_t edges_max;
} pcr_polygon_stats;

/* A slab in the stream's int32 coordinates (pcr_plane_support, pcr_select_slabs), 32 bytes: one linear form with two bounds.
 * s(S, p) = n[0]*x + n[1]*y + n[2]*z in exact 64-bit integers: with |n[a]| <= PCR_SLAB_MAX_NORMAL every product is below 2^51
 * and the sum below 2^53 for any int32 point. p is in S iff lo <= s(S, p) <= hi. lo > hi: legal and empty. A bound at
 * -/+PCR_SLAB_MAX_BOUND: a half-space. n = (0, 0, 0): legal, in iff lo <= 0 <= hi.
 * The class of a slab against an exact batch box bb: smin = sum over a of min(n[a]*bb.min[a], n[a]*bb.max[a]), smax likewise
 * with max (a linear form takes its extremes at the corners, so both are attained); MISS iff lo > hi || smax < lo || smin > hi;
 * ALL iff not MISS and lo <= smin && smax <= hi; CUT otherwise. */
#define PCR_SLAB_MAX_NORMAL (1 << 20)            /* |n[a]| <= this */
#define PCR_SLAB_MAX_BOUND ((int64_t)1 << 61)    /* |lo|, |hi| <= this */
#define PCR_PLANE_MAX_HYPOTHESES 1024
#define PCR_SLAB_MAX_EXCLUDE 16
#define PCR_SLAB_MAX_SELECT 16
#define PCR_SLAB_INVERT 1u                       /* pcr_select_slabs flags: keep the points NOT in all of the slabs (the clip still applies) */
typedef struct pcr_slab {
    int32_t n[3];
    int32_t reserved;            /* 0 */
    int64_t lo, hi;              /* inclusive */
} pcr_slab;

/* What pcr_plane_support did: the batches of the range by the host plan (pcr_hip.h has the rule) -- skipped (no candidate),
 * whole (neither skipped nor decoded: every contribution known from the box), decoded (one workgroup of k_plane_support) --
 * the sum and the largest of the decoded batches' hypothesis slices, the sum of their exclusion slices, and the sum of the
 * kernel's per-batch candidate counts. */
typedef struct pcr_plane_stats {
    int64_t batches_skipped;
    int64_t batches_whole;
    int64_t batches_decoded;
    int64_t hypotheses_listed;
    int64_t hypotheses_max;
    int64_t exclusions_listed;
    int64_t candidates_decoded;
    int64_t reserved;
} pcr_plane_stats;

/* What pcr_select_slabs / pcr_read_slabs did: pcr_polygon_stats with the slab lists in place of the edge lists. */
typedef struct pcr_slab_stats {
    int64_t batches_outside;
    int64_t batches_inside;
    int64_t batches_straddling;
    int64_t points_selected;
    int64_t slabs_listed;
    int64_t slabs_max;
} pcr_slab_stats;

/* A top-down grid over the stream's int32 x and y (pcr_grid_accumulate), 24 bytes. A point (x, y, z, colour) belongs to cell
 * (cx, cy) iff x >= origin_x, y >= origin_y, cx = (uint32)(x - origin_x) / cell < width and cy = (uint32)(y - origin_y) / cell
 * < height (the differences fit 32 unsigned bits for every int32 input); the cell's index in a plane is cx + cy * width.
 * A cell of a plane holds, with the key K = (uint64)((uint32)z ^ 0x80000000u) << 32 | colour (unsigned order of K = signed
 * order of z, ties in z decided by the colour: the whole word, as at depth ties in a frame):
 *   top     uint64  unsigned max of K over the cell's points   empty: 0
 *   bottom  uint64  unsigned min of K                          empty: all ones
 *   count   uint32  number of points, modulo 2^32              empty: 0 */
#define PCR_GRID_MAX_CELLS     (1 << 26)  /* width * height */
#define PCR_GRID_WINDOW_CELLS  4096       /* largest per-batch footprint accumulated in LDS */
#define PCR_GRID_NO_WINDOW     1          /* flags bit: every batch straight to global atomics */
#define PCR_GRID_TOP           0
#define PCR_GRID_BOTTOM        1
typedef struct pcr_grid {
    int32_t origin_x, origin_y;  /* min corner of cell (0, 0) */
    int32_t cell;                /* edge length, >= 1 */
    int32_t width, height;       /* cells, >= 1; width * height <= PCR_GRID_MAX_CELLS */
    int32_t reserved;            /* 0 */
} pcr_grid;

/* What pcr_grid_accumulate did with the batches of its range, by their exact box against grid and clip: outside (not decoded),
 * windowed (accumulated in LDS, then merged), direct (global atomics per point). */
typedef struct pcr_grid_stats {
    int64_t batches_outside, batches_windowed, batches_direct;
} pcr_grid_stats;

/* Height percentiles per cell (pcr_grid_quantiles). q is in basis points: 9500 = the 95th percentile. */
#define PCR_QUANTILE_ONE       10000
#define PCR_QUANTILES_MAX      8
#define PCR_QUANTILE_MAX_BATCHES 65535   /* batches of a call: the counts and segment offsets are 32 bits */
/* What pcr_grid_quantiles did: pcr_grid_stats' classes of the batches, the candidates (records inside grid and clip at or above
 * their cell's floor), the cells with at least one, and the most candidates a single cell holds (the select kernels read a
 * cell of m candidates up to 1 + 3 * num_q times in one workgroup: a very large value here explains a slow call). */
typedef struct pcr_quantile_stats {
    int64_t batches_outside, batches_windowed, batches_direct;
    int64_t candidates, cells_occupied, max_cell_points;
} pcr_quantile_stats;

/* The ground filter over a lowest-point height plane of a grid (pcr_ground_filter): Zhang et al.'s progressive morphological
 * filter, step k an opening (minimum, then maximum) of the running surface over the square window of radius[k] cells around
 * each cell; a cell whose surface drops by more than threshold[k] in a step is not ground. pcr_hip.h has the exact definition.
 * A cell is empty iff its height is PCR_GROUND_EMPTY, the value pcr_grid_unpack writes for a cell without points: a real
 * z == INT32_MIN cannot be told from it. */
#define PCR_GROUND_MAX_STEPS   16
#define PCR_GROUND_MAX_RADIUS  64
#define PCR_GROUND_MAX_FILL    4096
#define PCR_GROUND_EMPTY       INT32_MIN
#define PCR_CELL_EMPTY         0          /* classes of the input plane's cells */
#define PCR_CELL_GROUND        1
#define PCR_CELL_NONGROUND     2
typedef struct pcr_ground_params {       /* 136 bytes */
    int32_t num_steps;           /* 0 .. PCR_GROUND_MAX_STEPS; 0: no cell is flagged, the call only fills */
    int32_t fill_rounds;         /* 0 .. PCR_GROUND_MAX_FILL: the most rounds of the hole fill */
    int32_t radius[16];          /* cells, 1 .. PCR_GROUND_MAX_RADIUS for k < num_steps; the rest 0 */
    int32_t threshold[16];       /* the stream's z units, >= 0 */
} pcr_ground_params;

/* What pcr_ground_filter found: the cells of the input plane by class, of the empty and non-ground ones those the fill gave a
 * height and those it left PCR_GROUND_EMPTY, and the rounds of the fill that filled at least one cell. */
typedef struct pcr_ground_stats {
    int64_t cells_empty, cells_ground, cells_nonground;
    int64_t cells_filled, cells_unfilled;
    int64_t fill_rounds;
} pcr_ground_stats;

/* pcr_select_height: flags bit -- the z field of a written record holds its height above the ground plane instead of z. */
#define PCR_HEIGHT_REPLACE_Z 1
/* What pcr_select_height did: the batches of the range whose exact box misses grid and clip (not decoded) and the others (decoded
 * twice: counted, then written), the records inside grid and clip whose cell has no ground (never selected), and the records
 * selected, which is the call's *out_count. */
typedef struct pcr_height_stats {
    int64_t batches_outside, batches_decoded;
    int64_t points_no_ground;
    int64_t points_selected;
} pcr_height_stats;

/* A lattice of cubic voxels over the stream's int32 coordinates (pcr_thin, pcr_denoise, pcr_components), 16 bytes: a point (x, y, z) belongs to voxel
 * v[k] = floor((p[k] - origin[k]) / cell) on every axis, the difference and the division taken exactly (as 64-bit integers;
 * v may be negative). Every int32 point has a voxel: the lattice has no far edge. */
#define PCR_THIN_FIRST            0          /* mode: of a voxel's points the one with the lowest row */
#define PCR_THIN_CENTER           1          /* mode: the one nearest to the voxel's centre, ties to the lowest row */
#define PCR_THIN_MAX_CELL         (1 << 30)
#define PCR_THIN_MAX_CENTER_CELL  2048       /* PCR_THIN_CENTER: 3 * (cell - 1)^2 < 2^24 */
#define PCR_VOXEL_MEAN_MAX_ROWS   (1ll << 32) /* pcr_voxel_mean: rows of a call, so that n <= 2^32 and every sum S < 2^62 (offsets < 2^30) */
typedef struct pcr_voxels {
    int32_t origin[3];           /* min corner of voxel (0, 0, 0) */
    int32_t cell;                /* edge length, 1 .. PCR_THIN_MAX_CELL */
} pcr_voxels;

/* What pcr_thin did: the batches of the range whose exact box misses the clip (not decoded) and the others (decoded three
 * times: runs counted, voxels marked, records written; the last only for a batch that keeps a record), the rows inside the
 * clip, the runs of equal voxel they form along their chains (= insertions into the voxel table), the records kept, which
 * is the call's *out_count and the number of non-empty voxels, and the slots of the table. */
typedef struct pcr_thin_stats {
    int64_t batches_outside;
    int64_t batches_decoded;
    int64_t points_considered;
    int64_t runs;
    int64_t points_kept;
    int64_t table_slots;
} pcr_thin_stats;

/* pcr_lod_order: `levels` nested lattices of pcr_thin over one origin. Level l (0 = coarsest, levels - 1 = finest) has the cell
 * cell << (levels - 1 - l); the coarsest cell is at most PCR_THIN_MAX_CELL. 24 bytes. */
#define PCR_LOD_MAX_LEVELS        16
#define PCR_LOD_DROP_REST         1u         /* flag: do not write the candidates that are first in no voxel of any level */
#define PCR_LOD_ROW_ORDER         2u         /* flag: the records in increasing row order, not in increasing (level, row) */
typedef struct pcr_lod {
    int32_t origin[3];           /* min corner of voxel (0, 0, 0) of every level */
    int32_t cell;                /* edge length of the finest level, >= 1 */
    int32_t levels;              /* L, 1 .. PCR_LOD_MAX_LEVELS */
    int32_t reserved;            /* 0 */
} pcr_lod;

/* What pcr_lod_order did: pcr_thin_stats' batches, candidates and runs, the slots of the finest level's table, the records
 * written, and the candidates of every level: level_count[l] for l < levels, level_count[levels] those of no level ("the rest",
 * counted also when PCR_LOD_DROP_REST keeps them out of the result); the entries above are 0. */
typedef struct pcr_lod_stats {
    int64_t batches_outside;
    int64_t batches_decoded;
    int64_t points_considered;
    int64_t runs;
    int64_t table_slots;
    int64_t points_written;
    int64_t level_count[PCR_LOD_MAX_LEVELS + 1];
} pcr_lod_stats;

/* pcr_denoise: a candidate is isolated iff the 27 voxels around its own hold at most max_count candidates, itself included. */
#define PCR_DENOISE_KEEP          0          /* mode: write the candidates that are not isolated */
#define PCR_DENOISE_ISOLATED      1          /* mode: write the isolated ones */

/* What pcr_denoise did: the batches of the range whose exact box misses the clip (not decoded) and the others (decoded four
 * times: runs counted, voxels counted, rows flagged, records written; the last only for a batch that writes a record), the
 * rows inside the clip, the runs of equal voxel they form along their chains (= insertions into the voxel table), the
 * non-empty voxels (occupied slots), of those the ones whose points are isolated, the isolated points (whichever mode), the
 * records written, which is the call's *out_count, and the slots of the table. */
typedef struct pcr_denoise_stats {
    int64_t batches_outside;
    int64_t batches_decoded;
    int64_t points_considered;
    int64_t runs;
    int64_t voxels;
    int64_t voxels_isolated;
    int64_t points_isolated;
    int64_t points_written;
    int64_t table_slots;
} pcr_denoise_stats;

/* pcr_components: the occupied voxels form a graph; a component is small iff its voxels hold fewer than min_points candidates. */
#define PCR_COMPONENTS_KEEP       0          /* mode: write the candidates of the components that are not small */
#define PCR_COMPONENTS_SMALL      1          /* mode: write the candidates of the small ones */

/* What pcr_components did: the first four as in pcr_denoise_stats (a listed batch is decoded three times for the plan, a fourth
 * time if it writes a record, a fifth for its labels), the non-empty voxels, the components they form, of those the small ones
 * and the candidates they hold (whichever mode), the candidates of the largest component, the records written, which is the
 * call's *out_count, and the slots of the table. */
typedef struct pcr_components_stats {
    int64_t batches_outside;
    int64_t batches_decoded;
    int64_t points_considered;
    int64_t runs;
    int64_t voxels;
    int64_t components;
    int64_t components_small;
    int64_t points_small;
    int64_t largest_points;
    int64_t points_written;
    int64_t table_slots;
} pcr_components_stats;

/* pcr_neighbors: N(p) = the candidates within `radius` of p, itself included; a candidate is sparse iff N(p) < min_count. */
#define PCR_NEIGHBORS_ALL         0          /* mode: write every candidate; min_count only feeds the statistics */
#define PCR_NEIGHBORS_KEEP        1          /* mode: write the candidates that are not sparse */
#define PCR_NEIGHBORS_SPARSE      2          /* mode: write the sparse ones */
#define PCR_NEIGHBORS_MAX_RADIUS  (1 << 20)  /* stream units: coordinates of adjacent voxels then differ by less than 2^21 */
#define PCR_NN2_NONE              UINT64_MAX /* nn2 of a candidate with no other candidate within the radius */

/* What pcr_neighbors did: the first four as in pcr_denoise_stats (a listed batch is decoded three times for the index, a fourth
 * time if it writes a record), the non-empty voxels of the lattice with cell = radius, the slots of the table, the candidates of
 * the fullest voxel, pairs_bound = the sum over the candidates of the candidates in the 27 voxels around their own -- what the
 * pair kernel tests at most; computed from the table, so an early exit does not change it --, the sparse candidates (whichever
 * mode) and the records written, which is the call's *out_count. */
typedef struct pcr_neighbors_stats {
    int64_t batches_outside;
    int64_t batches_decoded;
    int64_t points_considered;
    int64_t runs;
    int64_t voxels;
    int64_t table_slots;
    int64_t max_voxel_points;
    int64_t pairs_bound;
    int64_t points_sparse;
    int64_t points_written;
} pcr_neighbors_stats;

/* pcr_local_moments: the moments of a candidate's neighbourhood B(p) = the candidates q with d2(p, q) <= radius * radius, p itself
 * included, over the offsets d = q - p. With radius <= PCR_MOMENTS_MAX_RADIUS every |d_a| <= 32767 and every product is below
 * 2^30; a call has at most 2^32 rows, so every sum stays below 2^62 and the int64 fields are exact: that is the reason for the
 * limit. n = |B(p)| (pcr_neighbors' N), s[a] = the sum of d_a, q = the sums of d_a * d_b in the order xx, xy, xz, yy, yz, zz. */
#define PCR_MOMENTS_MAX_RADIUS 32767
typedef struct pcr_moments {
    int64_t n;
    int64_t s[3];
    int64_t q[6];
} pcr_moments;

/* What pcr_moments_eigen makes of a pcr_moments record: the eigenvalues of its covariance matrix, ascending, and a unit
 * eigenvector of value[0] (the surface normal), its sign fixed: the first non-zero of normal[2], normal[1], normal[0] is
 * positive. All zero for n <= 0. */
typedef struct pcr_eigen {
    double value[3];
    double normal[3];
} pcr_eigen;

/* pcr_knn: a neighbour is one 64-bit word d2 << 32 | row -- the squared distance (below 2^30 with radius <= PCR_KNN_MAX_RADIUS) over
 * the row relative to first_batch (a call has at most 2^32 rows); the unsigned order of the words is the order (d2, row).
 * PCR_KNN_NONE fills the entries behind the last neighbour found. */
#define PCR_KNN_MAX_K       16
#define PCR_KNN_MAX_RADIUS  32767
#define PCR_KNN_NONE        UINT64_MAX

/* A rectangle of pixels (pcr_select_screen), bounds inclusive, clipped to the image by the call. x0 > x1 or y0 > y1: the
 * empty rect. */
typedef struct pcr_rect {
    int32_t x0, y0, x1, y1;
} pcr_rect;

/* Where a selected point lands in a frame of the given camera (pcr_select_screen / pcr_pick), 16 bytes. */
typedef struct pcr_screen_hit {
    uint32_t pixel;        /* x + y * width: exactly the index the render kernels scatter to */
    uint32_t depth_bits;   /* f32 bits of w: the high half of the framebuffer key */
    int64_t  index;        /* record index in pcr_decode_points order, relative to batch 0 of the context */
} pcr_screen_hit;

/* What a screen selection did (pcr_select_screen / pcr_read_screen / pcr_pick): the resident batches the cull/LOD prepass
 * drops for this camera (culled, or no point to draw: not decoded), the batches decoded, the points projected and tested
 * (1024 x the level of detail's points per chain, summed over the decoded batches) and the records selected, which is the
 * call's *out_count. (pcr_select_stats' classes -- outside / inside / straddling a box -- do not describe this.) */
typedef struct pcr_screen_stats {
    int64_t batches_skipped;
    int64_t batches_decoded;
    int64_t points_tested;
    int64_t points_selected;
} pcr_screen_stats;

/* pcr_select_visible: which of a frame's hits are selected, and how far a pixel's front depth occludes its neighbours. */
#define PCR_VISIBLE_FRONT       0   /* of every pixel the one hit that is least by (depth_bits, colour, index) */
#define PCR_VISIBLE_SURFACE     1   /* every hit within 1 % of its pixel's (dilated) front depth */
#define PCR_VISIBLE_MAX_RADIUS  8   /* the occluder window is (2 * radius + 1)^2 pixels */

/* What a visible selection did (pcr_select_visible / pcr_read_visible): batches as pcr_screen_stats; the hits of the whole image
 * (pixel < width * height) and the pixels that hold at least one; the hits in the rect; the records selected (*out_count). */
typedef struct pcr_visible_stats {
    int64_t batches_skipped;
    int64_t batches_decoded;
    int64_t hits;
    int64_t pixels_covered;
    int64_t candidates;
    int64_t selected;
} pcr_visible_stats;

/* How a display resolve (pcr_resolve_*_display) turns the framebuffer into the image: the point size and eye-dome lighting of
 * the reference's GLSL 10-10-10 resolve (modules/compute_loop_las/resolve.cs:98-128 `window`, :41-62 and :143-185 `edlWindow`). */
#define PCR_DISPLAY_MAX_WINDOW      4   /* point size 2*4+1 = 9 pixels */
#define PCR_DISPLAY_MAX_EDL_WINDOW  2
typedef struct pcr_display_opts {       /* 16 bytes */
    int32_t window;        /* 0..PCR_DISPLAY_MAX_WINDOW: a point covers (2*window+1)^2 pixels; 0 = one pixel */
    int32_t edl_window;    /* 0 = no eye-dome lighting; 1..PCR_DISPLAY_MAX_EDL_WINDOW */
    float   edl_strength;  /* finite, >= 0; the reference's constant is 0.0005f (resolve.cs:169); ignored when edl_window == 0 */
    int32_t reserved;      /* must be 0 */
} pcr_display_opts;

/* Number of u64 elements a framebuffer of w x h must hold: ndc == 1.0 maps to column w / row h
 * (SURVEY Appendix C.2), so pixel ids reach w*(h+1). */
static inline size_t pcr_fb_elems(int w, int h) { return (size_t)w * (size_t)(h + 1) + 1; }

#ifdef __cplusplus
}
#endif
#endif /* PCR_TYPES_H */
