// pcr_kernels.hip.h — hand-written HIP kernels for gfx950 (MI355X, wave64). Included by pcr_api.hip only.
//
// Compile flags that are part of the numeric contract: -ffp-contract=off (every FMA
// below is spelled __fmaf_rn/__fma_rn), default correctly-rounded f32 division and sqrt, no fast-math.
//
// Kernels
//   k_lod_prepass   eight lanes per batch: frustum cull + LOD (render.cu:333-379) -> lod word per batch + stats, the dense lists
//                   of the batches to draw (ballot + prefix compaction), and the LDS framebuffer windows of each (plan_windows)
//   k_transcode     once per loaded batch: the reference's lockstep walk over the cluster-interleaved stream
//                   (render.cu:404-451), recording per chain the words it receives -> lane-major stream, 40-bit point windows,
//                   packed decoder table, colour blocks in segment-major order
//   k_bounds        once per loaded batch: where the batch's chains fall apart into spatial clusters (runs of chains + boxes)
//   k_render<MODE>  every frame, one chain per lane -- two 512-thread workgroups per batch (PARTS = 2, the default) or the reference's
//                   one of 1024 (PARTS = 1): decodes the chain of <= 64 points from its own bits with the batch's decoder table in
//                   LDS, then projects and scatters every point (render.cu:383-540, huffman_hqs/depth.cu, huffman_hqs/render.cu;
//                   MODE 3: the colour pass over BC7 mode-6 colours)
//   k_decode_points on request: the same decode, every point of a range of batches written out as {x, y, z, colour} records
//   k_screen_* / k_pick*  on request: the points a frame draws, selected by pixel (projection restated in screen_project)
//   k_visible_*     on request: of those points the ones that make up the picture, by per-pixel planes of front depth and index
//   k_grid*         on request: the stream rasterized top-down into max / min / count planes over its integer x and y
//   k_polygon_*     on request: the records inside a polygon prism, each straddling batch against its own edge list in LDS
//   k_slab_* / k_plane_support  on request: the records in a set of slabs lo <= n.p <= hi; the support of plane hypotheses
//   k_thin_*        on request: one record per voxel of a cubic lattice, straight from the compressed stream
//   k_denoise_*     on request: the records whose 3 x 3 x 3 voxels hold few points (or the others), on k_thin_*'s frame
//   k_components_*  on request: the connected components of the occupied voxels, the small ones dropped or extracted
//   k_neighbors_*   on request: per point the points within a radius and the nearest one, from a copy bucketed by voxel
//   k_moments_*     on request: per point the exact moments of the offsets to the points within a radius, eigenvalues and normal
//   k_knn_*         on request: per point its k nearest other points within a radius, ordered by (distance, row), on k_neighbors_*'s index
//   k_voxel_*       on request: the mean position and colour, the least row and the count of every voxel, on k_thin_*'s FIRST plan
//   k_las_*         the 10-10-10 method (modules/compute_loop_las_cuda)
//   k_resolve_*     framebuffer -> RGBA8 (resolve.cu:149-191, huffman_hqs/resolve.cu:2-47)
//   k_merge_* / k_flip_sign  multi-GPU partial-framebuffer merges
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "pcr_types.h"
#include "pcr_lattice.h"
#include "pcr_polygon.h"
#include "pcr_plane.h"

namespace pcr {

// lod word written by the prepass
constexpr uint32_t LOD_NPR_MASK = 0xFFu;
constexpr uint32_t LOD_DOUBLE   = 0x100u;
constexpr uint32_t LOD_CULLED   = 0x200u;

enum { MODE_BASIC = 0, MODE_HQS_DEPTH = 1, MODE_HQS_COLOR = 2, MODE_HQS_COLOR_BC7 = 3 };   // (3: the colour pass over BC7 mode-6 colours)

// k_render's LDS plan (whole-batch workgroups: 76 KiB per 1024 threads -> two per CU; half-batch workgroups: see DYN_LDS_BYTES_HALF)
constexpr int CHUNK_WORDS    = 64;               // stream staging granule per cluster: 32 lanes x 2 words (8-byte loads)
constexpr int RING_WORDS     = 2 * CHUNK_WORDS;  // per cluster                                   -> 16 KiB
// 60 KiB of k_render's LDS are shared between the batch's escape words and its framebuffer window, divided per batch: the
// pool takes what the batch's escapes need (up to ESC_POOL_WORDS, which leaves 1024 window pixels), the window gets the rest.
// The benchmark stream's batches have 3831..7037 escape words: windows of 4090..5760 pixels. A fixed 24 + 36 KiB split put 6 %
// of those batches on the checked escape path, 1.5x slower each, and they finished last on their CUs (+17 % per launch).
// DYN_LDS_BYTES_BIG: the same kernels launched with 140 KiB of it -- one workgroup per CU, windows of up to ~17 000 pixels --
// for frames whose batches' rectangles outgrow the small windows (4096x4096 over 1526 batches: most points would go through
// global pre-reads and global atomics; with the big windows k_render 0.564 -> 0.48 ms). At 1080p it is 40 % slower: half
// the waves per SIMD. The host chooses per frame (launch_render); the size travels in RenderArgs::dyn_lds_bytes.
constexpr int DYN_LDS_BYTES  = 60 * 1024;
constexpr int DYN_LDS_BYTES_BIG = 140 * 1024;
constexpr int ESC_POOL_WORDS = 13312;            // most escape words of a batch the pool ever holds -> 52 KiB
constexpr int ESC_SLACK      = 64;               // words behind the batch's own escapes kept in the pool as well
// HALF-BATCH WORKGROUPS (round 4; k_render<..., PARTS = 2>): a workgroup of 512 threads draws chains [512 part, 512 part + 512) of
// a batch, four such workgroups per CU: 16 KiB table + 24 KiB of dynamic LDS each (the part's own escape words + windows for the
// part's rectangle, about half the batch's). Same eight waves per SIMD; what changes is the granularity at which LDS and wave
// slots turn over: a workgroup's waves leave their point loop up to 12 us apart (oldest-first arbiter), its LDS is held from
// set-up to merge, and a launch of 1526 whole batches is three lock-step generations. Departs from render.cu:328 (one block per
// batch) and :383-395 (the table staged once per block: here twice, the second read from L2 -- the two halves of a batch are
// mapped to the same XCD, see k_render).
constexpr int DYN_LDS_BYTES_HALF     = 24 * 1024;    // four workgroups per CU (4 x (16 + 24) KiB = 160 KiB)
constexpr int DYN_LDS_BYTES_HALF_BIG = 62 * 1024;    // two per CU: large images (the 140 KiB configuration's counterpart)
constexpr int ESC_POOL_WORDS_HALF    = 5120;         // most escape words of a half-batch its pool ever holds -> 20 KiB
constexpr int MAX_PARTS = 2;
__host__ __device__ constexpr int esc_pool_max(int parts) { return parts == 1 ? ESC_POOL_WORDS : ESC_POOL_WORDS_HALF; }
constexpr int WIN_PIXELS     = 4096;             // nominal window (a batch with 7104 escape words); the 10-10-10 kernel's fixed one
constexpr int WIN_PIXEL_BYTES     = 8;           // basic / HQS depth: the u64 framebuffer word
constexpr int WIN_PIXEL_BYTES_HQS = 20;          // HQS colour: {RG u64, BA u64, depth u32}
constexpr int WIN_PIXELS_MAX = DYN_LDS_BYTES / WIN_PIXEL_BYTES;         // of the small configuration
// How many of a batch's escape words k_render keeps in LDS: all of them plus ESC_SLACK words that follow them in memory
// (the reference's tail over-reads), or as many as the pool holds. A batch with more than that is flagged
// (BF_GENERIC_SLOW_PATH) and its chains check every escape index: the first ESC_POOL_WORDS still come from LDS, only
// the rest from global memory. (Pooling none of an oversized batch's escapes made that batch twice as slow, and a few
// such batches made the whole launch 14 % longer: they finish last on their CUs.)
// (`esc_count`: the escape words of the workgroup's own chains -- the whole batch's, or one part's)
__device__ __forceinline__ uint32_t esc_pool_words(uint32_t esc_count, int parts = 1)
{
    return min(esc_count + (uint32_t)ESC_SLACK, (uint32_t)esc_pool_max(parts));
}
__device__ __forceinline__ uint32_t esc_pool_bytes(uint32_t pool_words) { return (pool_words * 4u + 15u) & ~15u; }
// pixels the batch's LDS window can hold next to its escape pool
__device__ __forceinline__ int window_capacity(uint32_t esc_count, int pixel_bytes, uint32_t dyn_lds_bytes, int parts = 1)
{
    // (one pixel less than fits: the slot behind the last window pixel is k_render's dummy slot, see there)
    return (int)((dyn_lds_bytes - esc_pool_bytes(esc_pool_words(esc_count, parts))) / (uint32_t)pixel_bytes) - 1;
}

// Lane-major copy of the word stream (k_transcode): row r holds the r-th word each of the batch's 1024 chains consumes.
// A chain consumes 2 words up front and one per 32 decoded bits (<= 192 x 12 / 32 = 72), and k_render reads four ahead.
constexpr int LW_ROWS        = 80;
constexpr uint32_t LW_ROW_BYTES = PCR_WORKGROUP_SIZE * 4;
// PCR_LAYOUT_WORDS keeps that copy compact (k_pack_words): per wave (64 chains) only the rows its longest chain consumed, 256
// bytes each, one block per batch. The benchmark stream's chains take 43.6 words on average, a wave's longest 46.7, against
// the 80 rows of the transcode's scratch form: 2.9 B per point resident instead of 5.
constexpr uint32_t LWC_ROW_BYTES = 64 * 4;
// Rows allocated behind the last wave's rows of a segment: a chain requests the two words behind its view for every point, up to four rows
// past the last row its wave's longest chain consumed (2 preloaded + every retired word + 1) -- words nobody looks at (a code's table
// entry does not depend on the bits behind the code), read from the next wave's rows or from this pad instead of being clamped
constexpr uint32_t LWC_PAD_ROWS = 8;
constexpr int LWC_WAVES = PCR_WORKGROUP_SIZE / 64;          // 16 blocks of rows per batch + one entry for the end
// Point windows (k_transcode, layout PCR_LAYOUT_POINT_WINDOWS): for point i of every chain the 40 bits of the chain's own
// bit stream that start at the point's first bit -- its three symbols (<= 36 bits) lie inside. Stored as two planes per
// batch: PW_ROWS rows of 1024 x u32 (bits 0..31 of the window) followed by PW_ROWS rows of 1024 x u8 (bits 32..39). Row i is
// read at point i by every lane of k_render (256 + 64 contiguous bytes per wave), with no word queue to maintain: 5 bytes per
// point of HBM instead of the ~3 the packed words take -- bytes traded for instructions. The key of a point's FIRST symbol is
// the top 12 bits of its own window, which do not depend on the point before it: k_render requests that table entry a whole
// point ahead, and only two of a point's three table reads are left on the dependent chain. (Round 1 stored 64 bits per
// point, round 2's first form 48: 36 + the look-ahead of the next point's first symbol, which the next window holds anyway.)
// PW_GUARD_BYTES: k_render requests two rows ahead, the last batch's low plane is followed by this much slack.
constexpr int PW_ROWS        = PCR_POINTS_PER_THREAD;
constexpr uint32_t PW_HI_ROW_BYTES = PCR_WORKGROUP_SIZE * 4, PW_LO_ROW_BYTES = PCR_WORKGROUP_SIZE * 1;
constexpr uint32_t PW_HI_BYTES = PW_ROWS * PW_HI_ROW_BYTES;                 // offset of the low plane inside a batch's block
constexpr uint32_t PW_BATCH_BYTES = PW_ROWS * (PW_HI_ROW_BYTES + PW_LO_ROW_BYTES);   // 320 KiB
constexpr uint32_t PW_GUARD_BYTES = 2 * PW_HI_ROW_BYTES;
enum { LAYOUT_WORDS = 0, LAYOUT_POINT_WINDOWS = 1 };
// batch_flags: set when some chain of the batch can meet an in-table value outside the packed entry's range or read an
// escape word outside k_render's LDS pool (k_transcode walks all 192 symbols of every chain, garbage tails included)
constexpr uint32_t BF_GENERIC_SLOW_PATH = 1u;      // ... of a whole-batch workgroup (PARTS == 1)
constexpr uint32_t BF_GENERIC_SLOW_PATH_HALF = 2u; // ... of a half-batch workgroup (PARTS == 2: its pool holds its own part's escapes only)
__host__ __device__ constexpr uint32_t bf_generic(int parts) { return parts == 1 ? BF_GENERIC_SLOW_PATH : BF_GENERIC_SLOW_PATH_HALF; }
// packed table entry: byte 0 = len, bits 31:10 = the value as a signed 22-bit number -- (int32)entry >> 10 is the delta, no
// bias to remove -- except that the most negative one, TE_SLOW_VALUE, is reserved: "the value is not in the entry" (an escape,
// bit 8, or an in-table value outside (-2^21, 2^21), bit 9). Cost model behind the layout (tools/exp/instr_rate2.hip, gfx950):
// v_ashrrev_i32 / v_add_u32 / v_sub_u32 / v_and_b32 on VGPRs and constants issue in ~2.3 cycles per wave64, anything VOP3,
// SDWA, 64-bit, packed, compare, convert or with an SGPR operand in ~4.2.
constexpr uint32_t TE_LEN = 0xFFu, TE_ESCAPE = 0x100u, TE_WIDE = 0x200u;
constexpr int TE_VALUE_SHIFT = 10;
constexpr int32_t TE_SLOW_VALUE = -(1 << 21);

// Device-side view of the loaded stream (own layout; the reference keeps nine flat CuBuffers,
// HuffmanLasLoader.h:39-47). Tables are stored as int32 values + int8 lengths (the reference narrows the
// length to `char` in-kernel, render.cu:393).
struct StreamView {
    const pcr_gpu_batch *batches;
    const int32_t  *start_values;     // [nB*1024*3]
    const uint32_t *encoded;          // [encoded_words]   (includes zero pad)
    const int32_t  *separate;         // [separate_words]  (includes zero pad)
    const int32_t  *separate_sizes;   // [nB*1024]
    const int32_t  *table_values;     // [nB*4096]
    const int8_t   *table_lens;       // [nB*4096]
    const int32_t  *cluster_sizes;    // [nB*32]
    const uint8_t  *colors;           // [nB*32768] BC1 (or [nB*65536] BC7 mode 6) as the file has them: block 4 t + s = points 16 s .. 16 s + 15 of chain t
    const uint8_t  *colors_t;         // the same blocks, k_transcode's order: [batch][segment s][chain t] -- the 1024 lanes of
                                      // k_render read the blocks of one segment side by side (as the file has them a wave's 64
                                      // blocks lie 32 B apart and every 128-byte line was fetched once per segment: 4x)
    uint32_t color_block_bytes;       // 8 (BC1) / 16 (BC7)
    const uint32_t *lane_words;       // k_transcode's scratch: [chunk][LW_ROWS][1024] lane-major stream
    const uint32_t *const *lw_block;  // [nB] PCR_LAYOUT_WORDS: the batch's compact copy (k_pack_words), or NULL (layout)
    const uint32_t *lw_wave_row;      // [nB * (LWC_WAVES + 1)] first row of each wave's rows inside the batch's block, and the end
    const uint32_t *batch_flags;      // [nB] BF_* bits written by k_transcode
    const uint32_t *packed_table;     // [nB*4096] k_render's table entries, packed by k_transcode
    const uint8_t  *point_windows;    // [nB * PW_BATCH_BYTES + PW_GUARD_BYTES] or NULL (layout), written by k_transcode
    const uint32_t *batch_runs;       // [nB * RUN_RECORDS * RUN_WORDS] k_bounds: where a batch's (a half-batch's) chains fall apart into spatial clusters
    int64_t encoded_words;
    int64_t separate_words;
    int64_t num_batches;
    int64_t batch_index_base;
};

// (esc_mid: the escape words of chains 0..511 -- where a half-batch workgroup's share of the batch's escapes begins / ends)
struct DrawRec { uint32_t b, lod, esc_total, esc_mid; int64_t sep_off; int64_t reserved2; };     // 32 bytes

struct FrameView {
    uint64_t *fb;
    uint64_t *rg;
    uint64_t *ba;
    uint32_t  fb_elems;
    // Dirty tiles: one byte per TILE_W x TILE_H pixels of the framebuffer, set for every tile a framebuffer word may be written
    // in: the prepass marks the tiles under the screen rectangle of every drawn batch's bounding box (every point of the batch
    // lands inside, in a window or not; a batch without such a rectangle -- its box reaches behind the camera -- sets the word
    // "everything" instead); a point that lands OUTSIDE that rectangle all the same -- the garbage tail of a chain, SURVEY B.4: a
    // thousandth of the points, anywhere on the screen -- has its tile marked by k_render, in its off-window branch.
    // The end of the frame (k_frame_turn_tiles) resolves and clears the marked tiles only -- at 4096x4096 the fused resolve + clear
    // is 57 us of a 420 us frame streaming 335 MB whether a pixel was touched or not. NULL: nobody keeps track (external buffers,
    // the 10-10-10 method), the whole frame is resolved and cleared. (Marking EVERY off-window point's tile in k_render's
    // point loop, with a load in front of the store, cost the loop 6 % for code it practically never runs; profiles/r03_experiments.md.)
    uint8_t  *tiles;                  // [ntiles]
    uint32_t *tiles_all;              // "everything": holds tiles_epoch if so (an epoch per frame: the word never has to be zeroed)
    uint32_t  tiles_x, tiles_epoch, tiles_total;
};
constexpr uint32_t TILE_W_SHIFT = 6, TILE_H_SHIFT = 4;     // 64 x 16 pixels: a tile row is 512 contiguous bytes of the framebuffer

// A batch's points are 65 536 consecutive points of the Morton order, chain t = points 64 t .. 64 t + 63. Where the curve
// jumps, the batch is two (or more) compact clusters far apart: at 1080p 25 of the benchmark's 1526 batches have bounding
// rectangles of up to 600 x 80 pixels for a few hundred touched ones, which no LDS window holds. Those batches took ~4x as
// long as the others -- their points went through global pre-reads and atomics -- and, being stragglers, cost the launch 9 %
// (4096x4096: a fifth of the batches, 38 %). So, once per loaded batch (k_bounds, camera independent): the three largest gaps
// between consecutive chains cut the batch into RUNS runs of chains, each with its own bounding box.
constexpr int RUNS = 4;
// One record per workgroup shape and part -- record 0: the whole batch, records 1 and 2: its halves (chains 0..511, 512..1023), each
// cut at ITS three largest jumps:
constexpr int RUN_WORDS = 4 + RUNS * 6 + 6; // {first chain of run 1, 2, 3, 0}, per run {min xyz, max xyz} as floats, then the box of ALL the part's chains
constexpr int RUN_RECORDS = 1 + MAX_PARTS;  // per batch
__host__ __device__ constexpr int run_record(int parts, int part) { return parts == 1 ? 0 : 1 + part; }
// Per frame (prepass, a placement hint: any plan gives the same frame): one LDS framebuffer window per run, or one for the
// whole batch when the runs' rectangles overlap anyway. first[r] = first chain of run r + 1 (1024: no such run); window r
// sits behind windows 0 .. r-1 in the array of window pixels.
struct WinPlan {
    uint32_t xy[RUNS], wh[RUNS];      // {x0 | y0<<16}, {w | h<<16}; w == 0: none
    uint32_t first[RUNS - 1];
    uint32_t mostly_outside;          // 1: the windows hold less than half of the runs' rectangles -- most points of the batch will land outside
                                      // them -- AND the same goes for most of the 32 batches around it (the prepass workgroup's vote): k_render
                                      // then pre-reads the framebuffer word of such a point, see project_request
    uint32_t whole_xy, whole_wh;      // the screen rectangle of the batch's own bounding box, in which the prepass marked the dirty tiles
                                      // (FrameView::tiles); w == 0: it has none, or no tiles are kept
};

struct RenderArgs {
    pcr_render_params p;
    StreamView s;
    FrameView f;
    uint32_t *lod;            // [nB]
    WinPlan *win;             // [nB * parts] LDS framebuffer windows per workgroup, for pixels of win_pixel_bytes
    WinPlan *win_hqs;         // prepass only: if not NULL, a second plan for the 20-byte pixels of the HQS colour pass is written here
                              // (the depth pass's prepass serves the colour pass of the same frame: one prepass per frame)
    pcr_render_stats *stats;  // device: one partial record per prepass workgroup
    // Dense lists of the batches k_render has to draw (frustum-culled batches and batches whose level of detail is zero
    // points are left out), compacted by the prepass in two levels that keep the file's (Morton) order: every prepass
    // workgroup compacts its PREPASS_BATCHES batches with a wave ballot + prefix count into order[kind][wg * PREPASS_BATCHES ..]
    // and writes how many there are to chunk_count[kind][wg]; k_render's workgroup x finds its batch with a wave-wide
    // prefix sum over the chunk counts. kind 0: ordinary batches, kind 1: those flagged BF_GENERIC_SLOW_PATH (drawn by the
    // checked variant of the kernel). No atomics, nothing to zero between frames. (A first version appended the chunks
    // with one atomic per workgroup: the chunks then land in arrival order, and the close-up frame, whose heavy batches
    // lead the file, ran 25 % longer with them shuffled.)
    struct DrawRec *order;    // [2][order_stride]
    uint32_t *chunk_count;    // [WORK_CLASSES + 1][PCR_MAX_PREPASS_WORKGROUPS]: the ordinary list's classes, then the checked list
    uint32_t order_stride;    // prepass workgroups * PREPASS_BATCHES
    // Longest first: with a level of detail the batches of a frame decode 1..64 points per chain, a workgroup lives 20..55 us, and in
    // the file's order the launch ends with a long tail of half-empty CUs (LOD 10 %: 153 us where the sum of the lifetimes over 512
    // slots is 106). The ordinary list is therefore drawn class by class -- WORK_CLASSES classes of points per chain, heaviest
    // first, the file's order inside a class: a chunk's records are stored class after class, chunk_count[class][chunk] counts them,
    // and k_render's scan walks the classes in turn. A frame at LOD 100 % has one class and scans as before. work_classes: 1 for
    // streams of more than 8192 batches (a scan round per 2048 batches AND class would cost their light workgroups more than it saves).
    uint32_t work_classes;
    // A list entry is a record, not just the batch's index: what k_render's workgroup needs to know before it can request the
    // batch's data (level-of-detail word, escape count, escape offset). Its set-up is then three dependent memory levels (chunk
    // counts -> record -> data) instead of four (... -> list entry -> lod / batch header / escape count -> data): 7 us of a
    // workgroup's 61 us life, spent with its sixteen wave slots idle (profiles/r03_experiments.md). (A fourth step -- the prepass
    // workgroup that finishes last moves the records into one dense array, so that workgroup x starts from ONE load -- was built
    // and measured: k_render -2 %, but 9 us more on the critical path of the launch that carries the prepass. Dropped.)
    int variant_hqs;          // LOD expression variant
    int parts;                // workgroups per batch of the following k_render launches (1: 1024 threads, 2: half-batches of 512): `win` /
                              // `win_hqs` then hold `parts` plans per batch ([b * parts + part]), the lists' "checked" class follows bf_generic(parts)
    int win_pixel_bytes;      // what a window pixel of the following k_render<MODE> takes in LDS (WIN_PIXEL_BYTES*)
    uint32_t dyn_lds_bytes;   // dynamic LDS of the following k_render launch: DYN_LDS_BYTES or DYN_LDS_BYTES_BIG
};

// ------------------------------------------------------------------------------------------------
// wave64 inclusive prefix sum in six DPP adds (row_shr 1 / 2 / 4 / 8 inside the rows of 16 lanes, then row_bcast 15 / 31 across
// them): no LDS, no wait. (__shfl_up compiles to ds_bpermute_b32: the scans at the top of k_render -- one per class of the list,
// every wave for itself -- were seven dependent LDS round trips each, ~1 us of a workgroup's set-up per class.)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);      // row_shr:1 (lanes without a source add 0)
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);      // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);      // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);      // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);     // row_bcast:15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);     // row_bcast:31 into rows 2 and 3
    return v;
}
// value of lane `lane` (uniform), as a scalar
__device__ __forceinline__ uint32_t wave_read_lane(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

// ------------------------------------------------------------------------------------------------
// strict-float helpers (helper_math.h semantics, Appendix C.1)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot4(const float *r, float x, float y, float z, float w)
{
    return __fmaf_rn(r[3], w, __fmaf_rn(r[2], z, __fmaf_rn(r[1], y, r[0] * x)));
}

__device__ __forceinline__ bool plane_accepts(float x, float y, float z, float w, const float *bmin, const float *bmax)
{
    float nl = sqrtf(__fmaf_rn(z, z, __fmaf_rn(y, y, x * x)));      // createPlane, render.cu:239-246
    float nx = x / nl, ny = y / nl, nz = z / nl, c = w / nl;
    float vx = nx > 0.0f ? bmax[0] : bmin[0];                       // :261-264
    float vy = ny > 0.0f ? bmax[1] : bmin[1];
    float vz = nz > 0.0f ? bmax[2] : bmin[2];
    float d = __fmaf_rn(nz, vz, __fmaf_rn(ny, vy, nx * vx)) + c;    // :235-237
    return !(d < 0.0f);
}

// Frame statistics: every prepass workgroup sums its batches in LDS and writes ONE partial record (no global atomics,
// nothing to zero beforehand); pcr_get_stats adds the partials of the last launch. PCR_STATS_PARTIALS bounds the grid.
constexpr uint32_t PCR_VOTE_NUM = 9u;   // the prepass workgroup's vote (WinPlan::mostly_outside): at least NUM / DEN of its drawn batches. (With 1 / 2 the
constexpr uint32_t PCR_VOTE_DEN = 10u;  // batches in front of a close-up camera, neighbours in the file, voted themselves in: +6 %, +20 % with culling.)
constexpr int PREPASS_THREADS = 256;
constexpr int PCR_MAX_PREPASS_WORKGROUPS = 2048;        // ceil(65535 batches / 32 batches per prepass workgroup)
constexpr int WORK_CLASSES = 4;                         // of the ordinary list, by points per chain: 49..64, 33..48, 17..32, 1..16 (RenderArgs::work_classes;
                                                        // 2, 3 and 4 classes measure alike, 8 cost the light workgroups' scans more than they gain)
__device__ __forceinline__ void commit_stats(const pcr_render_stats &mine, pcr_render_stats *partials, uint32_t index)
{
    __shared__ unsigned long long s_sum[4];
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
    __syncthreads();
    if (mine.batches_total)   atomicAdd(&s_sum[0], (unsigned long long)mine.batches_total);
    if (mine.batches_culled)  atomicAdd(&s_sum[1], (unsigned long long)mine.batches_culled);
    if (mine.points_iterated) atomicAdd(&s_sum[2], (unsigned long long)mine.points_iterated);
    if (mine.batches_double)  atomicAdd(&s_sum[3], (unsigned long long)mine.batches_double);
    __syncthreads();
    if (threadIdx.x == 0) {
        pcr_render_stats r;
        r.batches_total = (int64_t)s_sum[0]; r.batches_culled = (int64_t)s_sum[1];
        r.points_iterated = (int64_t)s_sum[2]; r.batches_double = (int64_t)s_sum[3];
        partials[index] = r;
    }
}

// ------------------------------------------------------------------------------------------------
// prepass: cull + LOD per batch
// ------------------------------------------------------------------------------------------------
// Eight lanes per batch: lane k tests frustum plane k (k < 6) and projects bounding-box corner k for the window
// rectangle; the LOD arithmetic is uniform. One lane doing all of it serially made this launch 9 us of every frame.
constexpr int PREPASS_LANES = 8;
constexpr int PREPASS_BATCHES = PREPASS_THREADS / PREPASS_LANES;     // batches per workgroup
struct PlanIn;
__device__ __forceinline__ uint32_t lod_prepass_batch(const RenderArgs &a, int64_t b, int lane, pcr_render_stats &st, bool publish);
__device__ __forceinline__ bool plan_windows(const RenderArgs &a, int64_t b, int part, int j, const PlanIn &in);

// What plan_windows reads from memory, requested at the top of the prepass block together with everything else the block
// reads: the block sits on the critical path of every frame (it shares a launch with the resolve + clear of the frame before:
// 7 us of work at 1080p) and was a chain of five dependent round trips (batch header -> the lod word read back -> list record ->
// runs of chains -> the window plan read back): 12-14 us. Now: one round of loads, values handed on through LDS and registers.
struct PlanIn {
    uint32_t esc_count;             // escape words of the (batch, part)'s chains
    uint32_t cut;                   // first chain of run r + 1 (runs[r]; unused for the last run)
    float box[6], all[6];           // the run's box, the box of all the part's chains (k_bounds)
    float gmin[3], gmax[3];         // the batch's own bounding box, relative to las_min (GPUBatch)
};
__device__ __forceinline__ PlanIn plan_preload(const RenderArgs &a, int64_t b, int part, int r)
{
    PlanIn in;
    const int32_t *ssz = a.s.separate_sizes + (size_t)b * 1024;
    const uint32_t mid = (uint32_t)ssz[511], total = (uint32_t)ssz[1023];
    in.esc_count = a.parts == 1 ? total : part == 0 ? mid : total - mid;
    const uint32_t *runs = a.s.batch_runs + ((size_t)b * RUN_RECORDS + run_record(a.parts, part)) * RUN_WORDS;
    in.cut = runs[min(r, RUNS - 2)];
    const float *box = reinterpret_cast<const float *>(runs + 4 + r * 6), *ab = reinterpret_cast<const float *>(runs + 4 + RUNS * 6);
#pragma unroll
    for (int k = 0; k < 6; ++k) { in.box[k] = box[k]; in.all[k] = ab[k]; }
    const pcr_gpu_batch *g = a.s.batches + b;
    const float lm[3] = { (float)g->las_min_x, (float)g->las_min_y, (float)g->las_min_z };
    in.gmin[0] = g->min_x - lm[0]; in.gmin[1] = g->min_y - lm[1]; in.gmin[2] = g->min_z - lm[2];
    in.gmax[0] = g->max_x - lm[0]; in.gmax[1] = g->max_y - lm[1]; in.gmax[2] = g->max_z - lm[2];
    return in;
}

// The prepass of a chunk of PREPASS_BATCHES batches is done by TWO workgroups of the launch, side by side (round 4): one writes what
// k_render's scan reads (lod words, statistics, the compacted lists), the other the window plans, the dirty tiles and the vote. Both
// work out the chunk's cull / LOD decisions for themselves (a microsecond of arithmetic on CUs that have nothing else to do): the
// block is a chain of cold starts -- kernel arguments, instruction cache, one round of loads -- and sits on every frame's critical
// path; as one workgroup it took 8.6-10.1 us from its start (phase stamps, profiles/r04_experiments.md), of which the plans 2.8-4.5.
template <bool LISTS>
__device__ __forceinline__ void lod_prepass_chunk(const RenderArgs &a, uint32_t block)
{
    const int64_t b = ((int64_t)block * PREPASS_THREADS + threadIdx.x) / PREPASS_LANES;
    const int lane = (int)(threadIdx.x % PREPASS_LANES);
    pcr_render_stats st = {0, 0, 0, 0};
    // the group's lod word (LOD_*), handed to the compaction / to the window plan through LDS (LOD_CULLED: no such batch)
    __shared__ uint32_t s_lod[PREPASS_BATCHES];
    // ---- every load of the block that does not depend on a result of the block, requested before anything is computed ----
    // the record lanes (first wave, one per batch of the block): what a list record holds besides the lod word
    const uint32_t bb = block * PREPASS_BATCHES + threadIdx.x;
    uint32_t rec_flags = 0, rec_esc_total = 0, rec_esc_mid = 0;
    int64_t rec_sep_off = 0;
    if (LISTS && threadIdx.x < PREPASS_BATCHES && (int64_t)bb < a.s.num_batches) {
        rec_flags = a.s.batch_flags[bb];
        rec_esc_total = (uint32_t)a.s.separate_sizes[(size_t)bb * 1024 + 1023];
        rec_esc_mid = (uint32_t)a.s.separate_sizes[(size_t)bb * 1024 + 511];
        rec_sep_off = a.s.batches[bb].separate_batch_offset;
    }
    // the plan lanes: RUNS lanes per batch and part, one per run of chains
    static_assert(PREPASS_BATCHES * RUNS * MAX_PARTS <= PREPASS_THREADS, "one round");
    const uint32_t parts = (uint32_t)a.parts, plan_lanes = RUNS * parts;
    const uint32_t slot = threadIdx.x / plan_lanes, part = (threadIdx.x / RUNS) % parts;
    const int64_t pb = (int64_t)block * PREPASS_BATCHES + slot;
    const bool plan_lane = !LISTS && threadIdx.x < PREPASS_BATCHES * plan_lanes && pb < a.s.num_batches;
    PlanIn pin = {};
    if (plan_lane) pin = plan_preload(a, pb, (int)part, (int)(threadIdx.x % RUNS));

    if (lane == 0) s_lod[threadIdx.x / PREPASS_LANES] = LOD_CULLED;
    if (b < a.s.num_batches) {
        const uint32_t lod = lod_prepass_batch(a, b, lane, st, LISTS);                          // uniform per 8-lane group
        if (lane == 0) s_lod[threadIdx.x / PREPASS_LANES] = lod;
    }
    if (LISTS) {
        commit_stats(st, a.stats, block);                   // (barriers inside: s_lod is complete afterwards)
        // first level of the compaction: one ballot and one prefix count per list, in the workgroup's first wave
        if (threadIdx.x < 64) {
            const uint32_t lod = threadIdx.x < PREPASS_BATCHES ? s_lod[threadIdx.x] : LOD_CULLED;
            // what k_render has to do for the batch: 0 nothing (culled, or no point to draw), 1 draw, 2 draw with the checked variant
            const uint32_t kind = !(lod & LOD_CULLED) && (lod & LOD_NPR_MASK) ? ((rec_flags & bf_generic(a.parts)) ? 2u : 1u) : 0u;
            const uint64_t below = (1ull << threadIdx.x) - 1ull;
            // (the list entry is the whole record k_render's workgroup starts from, see RenderArgs::order)
            DrawRec r = {0, 0, 0, 0, 0, 0};
            if (kind) { r.b = bb; r.lod = lod; r.esc_total = rec_esc_total; r.esc_mid = rec_esc_mid; r.sep_off = rec_sep_off; }
            // the ordinary list: class after class inside the chunk
            const uint32_t npr = r.lod & LOD_NPR_MASK;
            const uint32_t cls = a.work_classes > 1 && npr ? (uint32_t)(WORK_CLASSES - 1) - min((npr - 1u) / (64u / WORK_CLASSES), (uint32_t)(WORK_CLASSES - 1)) : 0u;
            uint32_t base = 0;
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)WORK_CLASSES; ++k) {
                const uint64_t m = __ballot(kind == 1u && cls == k);
                if (threadIdx.x == 0) a.chunk_count[k * PCR_MAX_PREPASS_WORKGROUPS + block] = (uint32_t)__popcll(m);
                if (kind == 1u && cls == k) a.order[block * PREPASS_BATCHES + base + (uint32_t)__popcll(m & below)] = r;
                base += (uint32_t)__popcll(m);
            }
            {   // the checked list
                const uint64_t m = __ballot(kind == 2u);
                if (threadIdx.x == 0) a.chunk_count[WORK_CLASSES * PCR_MAX_PREPASS_WORKGROUPS + block] = (uint32_t)__popcll(m);
                if (kind == 2u) a.order[(size_t)a.order_stride + block * PREPASS_BATCHES + (uint32_t)__popcll(m & below)] = r;
            }
        }
        return;
    }
    // LDS framebuffer windows of the workgroups that draw
    // ... and a vote: do (nearly) all of the chunk's batches (32 neighbours in the file) lie mostly outside their windows? Only then does
    // k_render pre-read the framebuffer words of such a batch's points (WinPlan::mostly_outside, project_request): a few batches of
    // that kind in a frame are cheaper unfiltered, a frame full of them (an unsorted stream) is not.
    __shared__ uint32_t s_vote[2];                          // plans drawn, of those mostly outside
    if (threadIdx.x < 2) s_vote[threadIdx.x] = 0;
    __syncthreads();                                        // (s_lod is complete)
    bool mine_drawn = false, mine_outside = false;
    if (plan_lane) {
        const uint32_t lod = s_lod[slot];
        if (!(lod & LOD_CULLED) && (lod & LOD_NPR_MASK)) {
            const bool outside = plan_windows(a, pb, (int)part, (int)(threadIdx.x % RUNS), pin);     // (uniform per RUNS lanes)
            if (threadIdx.x % RUNS == 0) {
                mine_drawn = true; mine_outside = outside;
                atomicAdd(&s_vote[0], 1u);
                if (outside) atomicAdd(&s_vote[1], 1u);
            }
        }
    }
    __syncthreads();
    // (the plan was written with the batch's own verdict; the neighbourhood's vote takes it back)
    if (mine_drawn && mine_outside && s_vote[1] * PCR_VOTE_DEN < s_vote[0] * PCR_VOTE_NUM) {
        a.win[pb * parts + part].mostly_outside = 0;
        if (a.win_hqs) a.win_hqs[pb * parts + part].mostly_outside = 0;
    }
}

// Workgroup w of a launch's prepass part: chunk w / 2, the lists (even) or the plans (odd)
constexpr uint32_t PREPASS_WGS_PER_CHUNK = 2;
__device__ __forceinline__ void lod_prepass_block(const RenderArgs &a, uint32_t w)
{
    if (w & 1u) lod_prepass_chunk<false>(a, w >> 1);
    else        lod_prepass_chunk<true>(a, w >> 1);
}

// One lane per run: the screen rectangle of the run's bounding box (k_bounds), then LDS pixels for the RUNS rectangles. Only a
// placement hint -- points that land outside their window take the global path -- so nothing here needs exactness, only
// rectangles inside the image and a pixel count within the LDS.
struct IRect { int x0, y0, x1, y1; };
__device__ __forceinline__ int rect_area(IRect r) { return r.x1 >= r.x0 && r.y1 >= r.y0 ? (r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) : 0; }
// the central part of a rectangle, scaled by sc < 1 per side (what is outside goes the global way)
__device__ __forceinline__ IRect rect_shrink(IRect r, float sc)
{
    const int w = r.x1 - r.x0 + 1, h = r.y1 - r.y0 + 1;
    if (w <= 0 || h <= 0) return r;
    const int nw = max(1, (int)floorf((float)w * sc)), nh = max(1, (int)floorf((float)h * sc));
    const int x0 = r.x0 + (w - nw) / 2, y0 = r.y0 + (h - nh) / 2;
    return { x0, y0, x0 + nw - 1, y0 + nh - 1 };
}
__device__ __forceinline__ void rect_pack(IRect r, uint32_t &xy, uint32_t &wh)
{
    if (r.x1 < r.x0 || r.y1 < r.y0 || r.x0 < 0 || r.y0 < 0 || r.x0 >= 65536 || r.y0 >= 65536) { xy = 0; wh = 0; return; }
    xy = (uint32_t)r.x0 | ((uint32_t)r.y0 << 16);
    wh = (uint32_t)(r.x1 - r.x0 + 1) | ((uint32_t)(r.y1 - r.y0 + 1) << 16);
}

// Windows for one pixel size, given the run's rectangle `mine` and the rectangle `single` that holds every chain of the workgroup
// (uniform work per RUNS lanes).
// Returns the plan's own verdict "most points will land outside" (the same in every lane of the group).
__device__ __forceinline__ bool assign_windows(int cap, IRect mine, IRect single, uint32_t cut, int r, WinPlan *out)
{
    auto group_sum = [](int v) { v += __shfl_xor(v, 1, RUNS); v += __shfl_xor(v, 2, RUNS); return v; };
    auto group_max = [](int v) { v = max(v, __shfl_xor(v, 1, RUNS)); v = max(v, __shfl_xor(v, 2, RUNS)); return v; };
    const IRect none = { 0x3FFFFFFF, 0x3FFFFFFF, -1, -1 };
    // The rectangle of all the workgroup's chains (the batch's own bounding box, GPUBatch, cut down to what k_bounds saw of the
    // part; the runs' boxes leave the straddling chains out): if the LDS holds it, it is the one window and no point lands outside.
    if (rect_area(single) > 0 && rect_area(single) <= cap) {
        uint32_t xy = 0, wh = 0;
        if (r == 0) rect_pack(single, xy, wh);
        out->xy[r] = xy; out->wh[r] = wh;                                           // (runs 1..3: no window of their own)
        if (r < RUNS - 1) out->first[r] = PCR_WORKGROUP_SIZE;                       // every chain belongs to run 0
        if (r == 0) out->mostly_outside = 0;
        return false;
    }
    // one window per run; while they do not fit together, the largest gives way (a run with a jump of its own inside)
    int sum = group_sum(rect_area(mine));
    const int wanted = sum;
#pragma unroll 1
    for (int round = 0; round < 6 && sum > cap; ++round) {
        const int area = rect_area(mine), largest = group_max(area);
        // (ties: every holder of the largest area shrinks -- the loop ends all the same)
        if (area == largest) {
            const int target = max(largest - (sum - cap), largest / 4);
            mine = target >= 1 ? rect_shrink(mine, sqrtf((float)target / (float)largest)) : none;
        }
        sum = group_sum(rect_area(mine));
    }
    if (sum > cap) mine = none;                                                     // hopeless: this run goes the global way
    rect_pack(mine, out->xy[r], out->wh[r]);
    if (r < RUNS - 1) out->first[r] = min(cut, (uint32_t)PCR_WORKGROUP_SIZE);
    const int kept = group_sum(rect_area(mine));                                    // (every lane of the group: a shuffle)
    const bool outside = kept * 2 < wanted;
    if (r == 0) out->mostly_outside = outside ? 1u : 0u;
    return outside;
}

// The screen rectangle of a box, worked out by a group of RUNS lanes (corners 2 r and 2 r + 1 per lane, then the union over the
// group); no rectangle for a box that reaches behind the camera, holds a NaN, or lies off screen.
__device__ __forceinline__ IRect group_box_rect(const pcr_render_params &p, const float *bmin, const float *bmax, int r)
{
    const IRect none = { 0x3FFFFFFF, 0x3FFFFFFF, -1, -1 };
    const float fw = (float)p.width, fh = (float)p.height;
    auto group_sum = [](int v) { v += __shfl_xor(v, 1, RUNS); v += __shfl_xor(v, 2, RUNS); return v; };
    bool front = true;
    float minx = 3.0e38f, maxx = -3.0e38f, miny = 3.0e38f, maxy = -3.0e38f;
#pragma unroll
    for (int c2 = 0; c2 < 8 / RUNS; ++c2) {
        const int c = r * (8 / RUNS) + c2;
        const float x = (c & 1) ? bmax[0] : bmin[0], y = (c & 2) ? bmax[1] : bmin[1], z = (c & 4) ? bmax[2] : bmin[2];
        const float w = dot4(p.transform + 12, x, y, z, 1.0f);
        front = front && w > 1.0e-6f;
        const float rw = __builtin_amdgcn_rcpf(w);              // (a placement hint: v_rcp_f32's 1 ulp is plenty, an IEEE division is ten instructions)
        const float sx = (dot4(p.transform + 0, x, y, z, 1.0f) * rw * 0.5f + 0.5f) * fw;
        const float sy = (dot4(p.transform + 4, x, y, z, 1.0f) * rw * 0.5f + 0.5f) * fh;
        minx = fminf(minx, sx); maxx = fmaxf(maxx, sx); miny = fminf(miny, sy); maxy = fmaxf(maxy, sy);
    }
#pragma unroll
    for (int m = 1; m < RUNS; m <<= 1) {
        minx = fminf(minx, __shfl_xor(minx, m, RUNS)); maxx = fmaxf(maxx, __shfl_xor(maxx, m, RUNS));
        miny = fminf(miny, __shfl_xor(miny, m, RUNS)); maxy = fmaxf(maxy, __shfl_xor(maxy, m, RUNS));
    }
    const bool all_front = (group_sum(front ? 1 : 0) == RUNS);
    IRect rc = none;
    if (all_front && maxx >= -1.0f && maxy >= -1.0f && minx <= fw + 1.0f && miny <= fh + 1.0f) {
        rc.x0 = max(0, (int)floorf(fmaxf(minx, -2.0f)) - 1); rc.x1 = min(p.width - 1, (int)floorf(fminf(maxx, fw + 2.0f)) + 1);
        rc.y0 = max(0, (int)floorf(fmaxf(miny, -2.0f)) - 1); rc.y1 = min(p.height - 1, (int)floorf(fminf(maxy, fh + 2.0f)) + 1);
        if (rc.x1 < rc.x0 || rc.y1 < rc.y0) rc = none;
    }
    return rc;
}
__device__ __forceinline__ IRect rect_intersect(IRect a, IRect b)
{
    const IRect none = { 0x3FFFFFFF, 0x3FFFFFFF, -1, -1 };
    const IRect c = { max(a.x0, b.x0), max(a.y0, b.y0), min(a.x1, b.x1), min(a.y1, b.y1) };
    return c.x1 >= c.x0 && c.y1 >= c.y0 ? c : none;
}

__device__ __forceinline__ bool plan_windows(const RenderArgs &a, int64_t b, int part, int r, const PlanIn &in)
{
    const pcr_render_params &p = a.p;
    const float fw = (float)p.width, fh = (float)p.height;
    const float bmin[3] = { in.box[0], in.box[1], in.box[2] }, bmax[3] = { in.box[3], in.box[4], in.box[5] };
    const IRect none = { 0x3FFFFFFF, 0x3FFFFFFF, -1, -1 };      // identity of the union
    // the batch's own bounding box (GPUBatch: it holds every point but the garbage tails of SURVEY B.4): the dirty tiles are marked under it
    const IRect whole = group_box_rect(p, in.gmin, in.gmax, r);
    // ... and what k_bounds saw of the workgroup's own chains, garbage tails included (a hint: float dequantisation): the one
    // window of the workgroup if the LDS holds it
    IRect single = group_box_rect(p, in.all, in.all + 3, r);
    if (rect_area(whole) > 0) single = rect_area(single) > 0 ? rect_intersect(single, whole) : whole;
    const int cap = window_capacity(in.esc_count, a.win_pixel_bytes, a.dyn_lds_bytes, a.parts);
    const int cap_hqs = a.win_hqs ? window_capacity(in.esc_count, WIN_PIXEL_BYTES_HQS, a.dyn_lds_bytes, a.parts) : cap;
    // The rectangle of MY run of chains -- eight corners per lane, two thirds of this function's arithmetic, and the prepass block sits
    // on every frame's critical path (it was 6 of the 12 us of the frame turn) -- is worked out only if some plan of the group needs
    // windows per run: 96 % of the half-batches of the benchmark frame get the one window.
    IRect mine = none;
    const bool single_fits = rect_area(single) > 0 && rect_area(single) <= min(cap, cap_hqs);
    if (!single_fits) {
        bool front = true;
        float minx = 3.0e38f, maxx = -3.0e38f, miny = 3.0e38f, maxy = -3.0e38f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float x = (c & 1) ? bmax[0] : bmin[0], y = (c & 2) ? bmax[1] : bmin[1], z = (c & 4) ? bmax[2] : bmin[2];
            const float w = dot4(p.transform + 12, x, y, z, 1.0f);
            front = front && w > 1.0e-6f;
            const float rw = __builtin_amdgcn_rcpf(w);
            const float sx = (dot4(p.transform + 0, x, y, z, 1.0f) * rw * 0.5f + 0.5f) * fw;
            const float sy = (dot4(p.transform + 4, x, y, z, 1.0f) * rw * 0.5f + 0.5f) * fh;
            minx = fminf(minx, sx); maxx = fmaxf(maxx, sx); miny = fminf(miny, sy); maxy = fmaxf(maxy, sy);
        }
        // (a box that reaches behind the camera, holds a NaN, or lies off screen gets no rectangle: its points take the global path)
        if (front && maxx >= -1.0f && maxy >= -1.0f && minx <= fw + 1.0f && miny <= fh + 1.0f) {
            mine.x0 = max(0, (int)floorf(fmaxf(minx, -2.0f)) - 1); mine.x1 = min(p.width - 1, (int)floorf(fminf(maxx, fw + 2.0f)) + 1);
            mine.y0 = max(0, (int)floorf(fmaxf(miny, -2.0f)) - 1); mine.y1 = min(p.height - 1, (int)floorf(fminf(maxy, fh + 2.0f)) + 1);
            if (mine.x1 < mine.x0 || mine.y1 < mine.y0) mine = none;
        }
        // No window reaches outside the rectangle the dirty tiles are marked under (FrameView::tiles): a point INSIDE its window is
        // never tested against that rectangle, so a window sticking out of it -- a run's box holds its chains' garbage tails -- would
        // let the merge write framebuffer words in a tile nobody marked. What lies outside goes the off-window way,
        // which marks. (`single` is cut to it above.)
        if (rect_area(whole) > 0) mine = rect_intersect(mine, whole);
    }
    const bool outside = assign_windows(cap, mine, single, in.cut, r, a.win + b * a.parts + part);
    if (a.win_hqs)                                              // (uniform) the colour pass of the same frame: 20-byte pixels
        assign_windows(cap_hqs, mine, single, in.cut, r, a.win_hqs + b * a.parts + part);
    // dirty tiles (FrameView::tiles): everything under the batch's rectangle; a batch without one can write anywhere
    uint32_t wxy = 0, wwh = 0;
    if (a.f.tiles) {
        if (rect_area(whole) > 0) {
            rect_pack(whole, wxy, wwh);
            const uint32_t tx0 = (uint32_t)whole.x0 >> TILE_W_SHIFT, ty0 = (uint32_t)whole.y0 >> TILE_H_SHIFT;
            const uint32_t ntx = ((uint32_t)whole.x1 >> TILE_W_SHIFT) - tx0 + 1u, nty = ((uint32_t)whole.y1 >> TILE_H_SHIFT) - ty0 + 1u;
            if (ntx * nty * 4u > a.f.tiles_total) {
                // a batch that close to the camera covers a quarter of the screen or more: "everything", and the turn walks the frame linearly
                if (r == 0 && part == 0) *a.f.tiles_all = a.f.tiles_epoch;
            } else if (part == 0) {                                                     // (the batch's first group of lanes marks)
                for (uint32_t ty = (uint32_t)r; ty < nty; ty += RUNS) {                  // a row of tiles per lane and turn
                    uint8_t *row = a.f.tiles + (ty0 + ty) * a.f.tiles_x + tx0, *end = row + ntx;
                    while (row < end && ((uintptr_t)row & 3u)) *row++ = 1;
                    for (; row + 4 <= end; row += 4) *(uint32_t *)row = 0x01010101u;
                    while (row < end) *row++ = 1;
                }
            }
        } else if (r == 0 && part == 0) {
            *a.f.tiles_all = a.f.tiles_epoch;
        }
    }
    if (r == 0) {
        WinPlan *w = a.win + b * a.parts + part;
        w->whole_xy = wxy; w->whole_wh = wwh;
        if (a.win_hqs) { w = a.win_hqs + b * a.parts + part; w->whole_xy = wxy; w->whole_wh = wwh; }
    }
    return outside;
}

__global__ void __launch_bounds__(PREPASS_THREADS) k_lod_prepass(RenderArgs a) { lod_prepass_block(a, blockIdx.x); }

// publish: write lod[b] and count the batch in the statistics (the lists' workgroup; the plans' workgroup only wants the decision)
__device__ __forceinline__ uint32_t lod_prepass_batch(const RenderArgs &a, int64_t b, int lane, pcr_render_stats &st, bool publish)
{
    const uint32_t group_shift = (threadIdx.x & 63u) & ~(uint32_t)(PREPASS_LANES - 1);   // my group's bits in a wave ballot
    const pcr_gpu_batch g = a.s.batches[b];
    const pcr_render_params &p = a.p;
    const float lm[3] = { (float)g.las_min_x, (float)g.las_min_y, (float)g.las_min_z };      // :336
    const float bmin[3] = { g.min_x - lm[0], g.min_y - lm[1], g.min_z - lm[2] };             // :340
    const float bmax[3] = { g.max_x - lm[0], g.max_y - lm[1], g.max_z - lm[2] };             // :341

    if (lane == 0 && publish) st.batches_total = 1;
    if (p.enable_frustum_culling) {                                                          // :342-344
        // planes (3-0), (3+0), (3+1), (3-1), (3-2), (3+2) of the transposed matrix (three.js convention, :246-259);
        // x + s*y with s = +-1 is the same rounding as x +- y
        const float *M = p.transform;
        const int r = (lane >> 1) & 3;
        const float sgn = (lane == 0 || lane == 3 || lane == 4) ? -1.0f : 1.0f;
        bool accept = true;
        if (lane < 6)
            accept = plane_accepts(M[12] + sgn * M[4 * r + 0], M[13] + sgn * M[4 * r + 1], M[14] + sgn * M[4 * r + 2],
                                   M[15] + sgn * M[4 * r + 3], bmin, bmax);
        const uint32_t votes = (uint32_t)(__ballot(accept) >> group_shift) & 0xFFu;
        if (votes != 0xFFu) {
            if (lane == 0 && publish) { a.lod[b] = LOD_CULLED; st.batches_culled = 1; }      // (plain stores to distinct fields: with `+=` hipcc
                                                                                      // merged them into one store at a computed offset -- scratch)
            return LOD_CULLED;
        }
    }
    // :349-375
    const float cx = 0.5f * (bmin[0] + bmax[0]), cy = 0.5f * (bmin[1] + bmax[1]), cz = 0.5f * (bmin[2] + bmax[2]);
    const float dx = bmin[0] - bmax[0], dy = bmin[1] - bmax[1], dz = bmin[2] - bmax[2];
    const float rad = sqrtf(__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx)));
    float vc[4], ve[4], pc[4], pe[4];
    for (int r = 0; r < 4; ++r) vc[r] = dot4(p.world_view + 4 * r, cx, cy, cz, 1.0f);
    ve[0] = vc[0] + rad; ve[1] = vc[1] + 0.0f; ve[2] = vc[2] + 0.0f; ve[3] = vc[3] + 0.0f;
    for (int r = 0; r < 4; ++r) {
        pc[r] = dot4(p.proj + 4 * r, vc[0], vc[1], vc[2], vc[3]);
        pe[r] = dot4(p.proj + 4 * r, ve[0], ve[1], ve[2], ve[3]);
    }
    const float fw = (float)p.width, fh = (float)p.height;
    const float scx = fw * (0.5f * (pc[0] / pc[3] + 1.0f)), scy = fh * (0.5f * (pc[1] / pc[3] + 1.0f));
    const float sex = fw * (0.5f * (pe[0] / pe[3] + 1.0f)), sey = fh * (0.5f * (pe[1] / pe[3] + 1.0f));
    const float ddx = sex - scx, ddy = sey - scy;
    float px = sqrtf(__fmaf_rn(ddy, ddy, ddx * ddx));
    const bool use_double = px >= 100.0f;                                    // :370
    if (a.variant_hqs) px = (float)((double)px / 100.0);                     // hqs depth.cu:223 / render.cu:388
    else               px = px / 100.0f;                                     // mem_iter render.cu:372
    float pct = (float)((double)(1.8f * px) - 0.3);                          // :373
    pct = fmaxf((float)p.lod_percent / 100.0f, fminf(pct, 1.0f));            // :374
    int npr = (int)(pct * (float)p.points_per_thread);                       // :375
    npr = min(npr, p.points_per_thread);
    npr = max(npr, 0);
    const uint32_t lod = (uint32_t)npr | (use_double ? LOD_DOUBLE : 0u);
    if (lane == 0 && publish) {
        a.lod[b] = lod;
        st.points_iterated = (int64_t)npr * PCR_WORKGROUP_SIZE;
        st.batches_double = use_double ? 1 : 0;
    }
    return lod;
}

// ------------------------------------------------------------------------------------------------
// decode + rasterize: one workgroup per batch, one chain per lane (lanes are independent after k_transcode)
//
// Memory plan per workgroup (PARTS = 1: LDS 76 KiB -> two workgroups per CU; PARTS = 2: 40 KiB -> four; 8 waves per SIMD either way):
//   s_table  16 KiB  decoder table packed to one dword per key (TE_* above): value << 10 | wide << 9 | escape << 8 | len
//                    (an in-table value outside +-2^21 is flagged `wide` and re-read from global memory)
//   s_dyn    60 KiB  (or 140 KiB) shared per batch (see DYN_LDS_BYTES above) between
//   s_esc            the escape ("separate") words of the batch, bulk-loaded coalesced up front (batches with
//                    more than ESC_POOL_WORDS escapes read the ones past the pool from global memory), and
//   s_win            the framebuffer words of the batch's screen rectangle -- or of one rectangle per run of chains
//                    (WinPlan, k_lod_prepass): they start empty, the depth pre-read and the atomicMin of every point that
//                    lands inside run on LDS (ds_read_b64 / ds_min_u64); at the end the windows are merged into the global
//                    framebuffer with one row-coalesced atomicMin per pixel a point reached and improved. min is
//                    associative, so the result is the same u64 per pixel; what changes is the number of global atomics:
//                    one per touched pixel and batch instead of one per new per-pixel minimum.
//   registers        the point's 40-bit window + the next one + the one in flight (LAYOUT_POINT_WINDOWS), or three words of
//                    the chain's own sequence + two requested a point ahead (LAYOUT_WORDS; see the word window below)
// Global loads left in the loop are consumed at least one iteration after they are issued.
// ------------------------------------------------------------------------------------------------
// BC1 block -> its four palette colours (render.cu:31-62, always 4-colour mode), one register per channel: byte k of
// r / g / b is that channel of palette entry k. A point's colour 0x00BBGGRR is then two v_perm_b32 with selectors built from
// its 2-bit index -- five instructions per point, no compare/select chain.
// ("Always 4-colour mode", c0 <= c1 included, and every (e0, e1, selector) of every channel at every local position are held against
// a numpy restatement of the rule by tests/test_gpu_colour.py, on the constructed blocks of tests/colour_cases.py.)
struct Bc1Palette { uint32_t r, g, b, selectors; };

__device__ __forceinline__ Bc1Palette bc1_palette(uint2 blk)
{
    const uint32_t l = blk.x & 0xFFFFu, h = blk.x >> 16;
    const uint32_t cr0 = (l >> 11) & 31, cg0 = (l >> 5) & 63, cb0 = l & 31;
    const uint32_t r0 = (cr0 << 3) | (cr0 >> 2), g0 = (cg0 << 2) | (cg0 >> 4), b0 = (cb0 << 3) | (cb0 >> 2);
    const uint32_t cr1 = (h >> 11) & 31, cg1 = (h >> 5) & 63, cb1 = h & 31;
    const uint32_t r1 = (cr1 << 3) | (cr1 >> 2), g1 = (cg1 << 2) | (cg1 >> 4), b1 = (cb1 << 3) | (cb1 >> 2);
    auto four = [](uint32_t c0, uint32_t c1) {              // entries 2 and 3: (2 c0 + c1) / 3 and (c0 + 2 c1) / 3, integer division
        return c0 | (c1 << 8) | (((c0 * 2 + c1) / 3) << 16) | (((c0 + c1 * 2) / 3) << 24);
    };
    Bc1Palette p;
    p.r = four(r0, r1); p.g = four(g0, g1); p.b = four(b0, b1);
    p.selectors = blk.y;                                    // byte 4 + local/4, bits 2*(local%4): render.cu:48
    return p;
}

__device__ __forceinline__ uint32_t bc1_color(const Bc1Palette &p, uint32_t local)
{
    const uint32_t sel = (p.selectors >> (2 * local)) & 3u;
    // v_perm_b32(s0, s1, m): result byte i = byte m.byte[i] of {s0 (4..7), s1 (0..3)}, 0x0c = zero
    const uint32_t rg = __builtin_amdgcn_perm(p.g, p.r, sel * 0x0101u + 0x0c0c0400u);          // g[sel] << 8 | r[sel]
    return __builtin_amdgcn_perm(p.b, rg, (sel << 16) + 0x0c040100u);                          // b[sel] << 16 | rg
}

// The same for the HQS colour pass, which wants r << 16 | g and b << 16 | 1 (the contribution of one point to the two packed sums): one
// selector, two v_perm_b32 -- the colour itself is never put together.
__device__ __forceinline__ void bc1_contribution(const Bc1Palette &p, uint32_t local, uint32_t &rg16, uint32_t &bc16)
{
    const uint32_t sel = (p.selectors >> (2 * local)) & 3u;
    const uint32_t m = sel * 0x00010001u + 0x0c040c00u;     // byte 2 <- s0[sel], byte 0 <- s1[sel], zero elsewhere
    rg16 = __builtin_amdgcn_perm(p.r, p.g, m);              // r[sel] << 16 | g[sel]
    bc16 = __builtin_amdgcn_perm(p.b, 0x01010101u, m);      // b[sel] << 16 | 1
}

// BC7 mode-6 block as the reference's kernels decode it (huffman_hqs/render.cu:240-273, struct bc7_mode_6 render.cu:66-110):
// endpoints = 7 bits << 1 | p-bit, the 4-bit field at 4 * local of the high quadword as the index of EVERY pixel (so pixel 0
// gets index << 1 | p1: reproduced), weight = round(idx * 64 / 15) = (idx * 64 + 7) / 15, channel = (e0 (64 - w) + e1 w + 32) >> 6.
// Kept per 16-point block as: r | b << 16 of endpoint 0, of endpoint 1, g0 | g1 << 16, and the two index words.
// (The mode bits are ignored. That, pixel 0's field and every (E0, E1, index) of every channel are held against a numpy restatement
// of the rule by tests/test_gpu_colour.py, on the constructed blocks of tests/colour_cases.py.)
struct Bc7Block { uint32_t rb0, rb1, g01, idx_lo, idx_hi; };
__device__ __forceinline__ Bc7Block bc7_block(uint4 blk)
{
    const uint64_t lo = ((uint64_t)blk.y << 32) | blk.x;
    const uint32_t p0 = blk.y >> 31, p1 = blk.z & 1u;
    auto end = [&](int shift, uint32_t pbit) { return ((((uint32_t)(lo >> shift)) & 127u) << 1) | pbit; };
    Bc7Block k;
    k.rb0 = end(7, p0) | (end(35, p0) << 16);
    k.rb1 = end(14, p1) | (end(42, p1) << 16);
    k.g01 = end(21, p0) | (end(28, p1) << 16);
    k.idx_lo = blk.z; k.idx_hi = blk.w;
    return k;
}
__device__ __forceinline__ uint32_t bc7_color(const Bc7Block &k, uint32_t local)        // 0x00BBGGRR (the pass has no use for alpha)
{
    const uint32_t idx = ((local < 8u ? k.idx_lo : k.idx_hi) >> (4u * (local & 7u))) & 15u;
    const uint32_t w = ((idx * 64u + 7u) * 4370u) >> 16, iw = 64u - w;                  // (n / 15 for the sixteen n = 64 idx + 7)
    const uint32_t rb = ((k.rb0 * iw + k.rb1 * w + 0x00200020u) >> 6) & 0x00FF00FFu;
    const uint32_t g = (((k.g01 & 0xFFFFu) * iw + (k.g01 >> 16) * w + 32u) >> 6) & 0xFFu;
    return rb | (g << 8);
}

// Row/column of linear index i in a window of width ww (i < 2^23): one float multiply and a correction of at most one
// row instead of a 32-bit integer division (which costs ~25 VALU on this hardware and sat in every set-up and merge).
__device__ __forceinline__ void window_row_col(uint32_t i, uint32_t ww, float inv_ww, uint32_t &y, uint32_t &x)
{
    y = (uint32_t)((float)i * inv_ww);
    int32_t r = (int32_t)(i - y * ww);
    if (r < 0) { --y; r += (int32_t)ww; }
    else if (r >= (int32_t)ww) { ++y; r -= (int32_t)ww; }
    x = (uint32_t)r;
}

// One packed dword per table key (layout above): value and length of render.cu:435-439 in a single LDS read.
__device__ __forceinline__ bool table_value_fits(int32_t value) { return value > TE_SLOW_VALUE && value < -TE_SLOW_VALUE; }
__device__ __forceinline__ uint32_t pack_table_entry(int32_t value, uint32_t lbyte)
{
    const int len = (int)(int8_t)lbyte;                             // render.cu:393 narrows to char
    const uint32_t slow = (uint32_t)TE_SLOW_VALUE << TE_VALUE_SHIFT;
    if (len <= 0) return slow | TE_ESCAPE | (uint32_t)abs(len);     // escapes never use the table value
    return table_value_fits(value) ? (((uint32_t)value << TE_VALUE_SHIFT) | (uint32_t)len) : (slow | TE_WIDE | (uint32_t)len);
}

// ------------------------------------------------------------------------------------------------
// k_transcode: the reference's lockstep decode (render.cu:404-451), run ONCE per loaded batch instead of every frame.
//
// The stream format interleaves the words of 32 chains in the order a 32-lane warp requests them, so finding "my next
// word" costs a ballot, a prefix count and a shared read per symbol — and the reference's tail quirk makes
// the word a lane receives depend on what the other 31 lanes did. This kernel performs exactly that walk (lengths only:
// no values, no escapes, no points) and writes down, per chain, the sequence of words it received: row r of
// lane_words holds the r-th word of each of the 1024 chains. k_render then decodes every chain from its own word
// sequence — same bits, same symbols, garbage tails included — without any cross-lane step. A decode truncated by the
// level of detail consumes a prefix of the same sequence (the walk is causal), so one transcode serves every frame.
// The walk also counts the escapes every chain reads, which tells whether k_render may take them from its LDS pool
// without checking (batch_flags).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_transcode(StreamView s, uint32_t *lane_words, uint32_t *batch_flags,
                                                                  uint32_t *packed_table, uint8_t *point_windows, uint8_t *colors_t,
                                                                  uint32_t *any_generic, int first_batch, int lane_words_first, uint32_t *wave_rows)
{
    const uint32_t b = (uint32_t)first_batch + blockIdx.x;
    const uint32_t tid = threadIdx.x;
    // my chain's four colour blocks -> segment-major order (StreamView::colors_t)
    if (s.color_block_bytes == 16) {
        const uint4 *src = reinterpret_cast<const uint4 *>(s.colors) + ((size_t)b * 4096 + tid * 4);
        uint4 *dst = reinterpret_cast<uint4 *>(colors_t) + (size_t)b * 4096 + tid;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k * PCR_WORKGROUP_SIZE] = src[k];
    } else {
        const uint2 *src = reinterpret_cast<const uint2 *>(s.colors) + ((size_t)b * 4096 + tid * 4);
        uint2 *dst = reinterpret_cast<uint2 *>(colors_t) + (size_t)b * 4096 + tid;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k * PCR_WORKGROUP_SIZE] = src[k];
    }
    __shared__ __align__(16) uint8_t s_len[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ __align__(16) uint32_t s_ring[PCR_CLUSTERS_PER_BATCH * RING_WORDS];
    bool generic = false;
    {
        const uint32_t l4 = reinterpret_cast<const uint32_t *>(s.table_lens + (size_t)b * PCR_HUFFMAN_TABLE_SIZE)[tid];
        const int4 v = reinterpret_cast<const int4 *>(s.table_values + (size_t)b * PCR_HUFFMAN_TABLE_SIZE)[tid];
        // byte: |len| (render.cu:393, :439), bit 7: escape (len <= 0, as k_render packs it)
        auto entry = [&](uint32_t lbyte, int32_t value) -> uint32_t {
            const int len = (int)(int8_t)lbyte;
            if (len > 0 && !table_value_fits(value)) generic = true;                       // "wide" entry of k_render's table
            return (uint32_t)abs(len) | (len <= 0 ? 0x80u : 0u);
        };
        reinterpret_cast<uint32_t *>(s_len)[tid] = entry(l4 & 0xFF, v.x) | (entry((l4 >> 8) & 0xFF, v.y) << 8) |
                                                   (entry((l4 >> 16) & 0xFF, v.z) << 16) | (entry(l4 >> 24, v.w) << 24);
        // k_render's table, packed once here instead of by every frame's prologue
        uint4 e;
        e.x = pack_table_entry(v.x, l4 & 0xFF); e.y = pack_table_entry(v.y, (l4 >> 8) & 0xFF);
        e.z = pack_table_entry(v.z, (l4 >> 16) & 0xFF); e.w = pack_table_entry(v.w, l4 >> 24);
        reinterpret_cast<uint4 *>(packed_table + (size_t)b * PCR_HUFFMAN_TABLE_SIZE)[tid] = e;
    }
    const pcr_gpu_batch *gb = s.batches + b;
    const int64_t enc_off = gb->encoding_batch_offset;      // :404
    const uint32_t *enc = s.encoded + enc_off;
    const uint32_t enc_last = (uint32_t)min((int64_t)0x7FFFFFF0, s.encoded_words + (PCR_GUARD_WORDS - 2) - enc_off);
    auto enc_load = [&](uint32_t i) -> uint32_t { return enc[min(i, enc_last)]; };
    auto enc_load2 = [&](uint32_t i) -> uint2 { uint2 v; __builtin_memcpy(&v, enc + min(i, enc_last), 8); return v; };
    const uint32_t cluster = tid >> 5, lane32 = tid & 31u, half_shift = tid & 32u, lanes_below = (1u << lane32) - 1u;
    const uint32_t cbase = cluster ? (uint32_t)s.cluster_sizes[(size_t)b * 32 + cluster - 1] : 0u;   // :407-410
    uint32_t *ring = s_ring + cluster * RING_WORDS;
    uint32_t *out = lane_words + (size_t)(b - (uint32_t)lane_words_first) * LW_ROWS * PCR_WORKGROUP_SIZE + tid;   // resident, or the launch's scratch
    uint32_t row = 2;
    uint64_t bits = ((uint64_t)enc_load(cbase + lane32) << 32) | enc_load(cbase + 32 + lane32);   // :416-417
    out[0] = (uint32_t)(bits >> 32);
    out[PCR_WORKGROUP_SIZE] = (uint32_t)bits;
    reinterpret_cast<uint2 *>(ring + CHUNK_WORDS)[lane32] = enc_load2(cbase + CHUNK_WORDS + lane32 * 2);
    reinterpret_cast<uint2 *>(ring)[lane32] = enc_load2(cbase + 2 * CHUNK_WORDS + lane32 * 2);
    uint2 stage = enc_load2(cbase + 3 * CHUNK_WORDS + lane32 * 2);
    uint32_t ep = 64, next_cross = 2 * CHUNK_WORDS;         // already_read (:418)
    uint32_t sft = 32 + 20;                                 // cur_bits (:419) + 20: (bits >> sft) & 0xFFF is the key of :431-433
    uint32_t nesc = 0;
    // my column of the batch's two window planes (high: u32 per point, low: u8 per point)
    uint32_t *pw = point_windows ? reinterpret_cast<uint32_t *>(point_windows + (size_t)b * PW_BATCH_BYTES) + tid : nullptr;
    uint8_t *pwl = point_windows ? point_windows + (size_t)b * PW_BATCH_BYTES + PW_HI_BYTES + tid : nullptr;
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < PCR_POINTS_PER_THREAD * 3; ++k) {   // :428-430
        // first bit of point k/3 in the chain's own word sequence: `bits` holds rows row-2 and row-1, of which 52 - sft
        // bits are consumed (parked in the window slot until the words behind it are known, see below)
        if (pw && k % 3 == 0) pw[(size_t)(k / 3) * PCR_WORKGROUP_SIZE] = 32u * (row - 2u) + (52u - sft);
        const uint32_t l = s_len[(uint32_t)(bits >> sft) & 0xFFFu];
        sft -= l & 0x7Fu;                                   // :435-439
        nesc += l >> 7;                                     // :438
        const bool need = sft <= 20u;                       // :442 (cur_bits <= 0)
        const uint64_t m = __ballot(need);                  // :443
        const uint32_t mh = (uint32_t)(m >> half_shift);
        if (need) {                                         // :444-449
            const uint32_t w = ring[(ep + __popc(mh & lanes_below)) & (RING_WORDS - 1)];
            out[(size_t)row * PCR_WORKGROUP_SIZE] = w;
            ++row;
            bits = (bits << 32) | w;
            sft += 32;
        }
        ep += __popc(mh);                                   // :450
        if (ep >= next_cross) {
            // My half of the wave has consumed the ring's older chunk (a step takes at most 32 words, so every refill
            // stays inside the two resident chunks): overwrite it with the staged chunk and fetch the chunk after that.
            // DS operations of a wave execute in order; the fences below only stop the compiler from reordering.
            reinterpret_cast<uint2 *>(ring + ((next_cross + CHUNK_WORDS) & (RING_WORDS - 1)))[lane32] = stage;
            stage = enc_load2(cbase + next_cross + 2 * CHUNK_WORDS + lane32 * 2);
            next_cross += CHUNK_WORDS;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // rows of the lane-major copy my wave's longest chain wrote (PCR_LAYOUT_WORDS keeps exactly those, k_pack_words)
    if (wave_rows) {
        uint32_t rows = row;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) rows = max(rows, (uint32_t)__shfl_xor((int)rows, m));
        if ((tid & 63u) == 0) wave_rows[(size_t)(b - (uint32_t)lane_words_first) * LWC_WAVES + (tid >> 6)] = rows;
    }
    // may k_render read this batch's escapes from its LDS pool unchecked? (same pool rules as there: the whole batch's escapes in
    // the pool of a 1024-thread workgroup, a half's in the pool of a half-batch workgroup)
    const int32_t *ssz = s.separate_sizes + (size_t)b * 1024;
    const uint32_t esc_total = (uint32_t)ssz[1023], esc_mid = (uint32_t)ssz[511];
    const uint32_t sp0 = tid ? (uint32_t)ssz[tid - 1] : 0u;
    const bool over1 = nesc && sp0 + nesc > esc_pool_words(esc_total, 1);
    const uint32_t e0 = tid < 512u ? 0u : esc_mid, e1 = tid < 512u ? esc_mid : esc_total;
    const bool over2 = nesc && (sp0 - e0) + nesc > esc_pool_words(e1 - e0, 2);
    const int any1 = __syncthreads_or(generic || over1 ? 1 : 0), any2 = __syncthreads_or(generic || over2 ? 1 : 0);
    if (tid == 0) {
        const uint32_t flags = (any1 ? BF_GENERIC_SLOW_PATH : 0u) | (any2 ? BF_GENERIC_SLOW_PATH_HALF : 0u);
        batch_flags[b] = flags;
        if (flags) atomicOr(any_generic, flags);            // sticky, per stream: the host launches the checked kernel only if set
    }

    // Point windows: 40 bits of my word sequence from each point's first bit. A point's window can reach two words past
    // the last word the walk had fetched when the point began, so they are cut once the whole sequence is written. The two
    // rows behind the chain's last word are zeroed first: no symbol can reach those bits, but the buffer may be the
    // transcode scratch of an earlier launch and the windows should not depend on what it held.
    if (pw) {
        out[(size_t)row * PCR_WORKGROUP_SIZE] = 0;
        out[(size_t)(row + 1) * PCR_WORKGROUP_SIZE] = 0;
        __threadfence();            // my own stores above (lane_words column, parked positions) before I read them back
#pragma unroll 4
        for (int i = 0; i < PW_ROWS; ++i) {
            const uint32_t pos = pw[(size_t)i * PCR_WORKGROUP_SIZE];
            const uint32_t r = pos >> 5, o = pos & 31u;
            const uint32_t a0 = out[(size_t)r * PCR_WORKGROUP_SIZE], a1 = out[(size_t)(r + 1) * PCR_WORKGROUP_SIZE],
                           a2 = out[(size_t)(r + 2) * PCR_WORKGROUP_SIZE];
            // alignbit(hi, lo, s) = low 32 bits of (hi:lo) >> (s & 31): s = 32 - o cuts 32 bits starting o bits into hi
            const uint32_t hi = o ? __builtin_amdgcn_alignbit(a0, a1, 32u - o) : a0;
            const uint32_t lo = o ? __builtin_amdgcn_alignbit(a1, a2, 32u - o) : a1;
            pw[(size_t)i * PCR_WORKGROUP_SIZE] = hi;                     // bits 0..31 of the window
            pwl[(size_t)i * PCR_WORKGROUP_SIZE] = (uint8_t)(lo >> 24);   // bits 32..39
        }
    }
}

// k_pack_words: the compact copy of the lane-major words (PCR_LAYOUT_WORDS), once per loaded batch behind k_transcode: wave w of
// batch b copies rows [0, rows_w) of its 64 columns from the scratch form into the batch's block, 256 bytes per row.
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_pack_words(const uint32_t *lane_words, uint32_t *const *lw_block,
                                                                   const uint32_t *lw_wave_row, int first_batch, int lane_words_first)
{
    const uint32_t b = (uint32_t)first_batch + blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t *src = lane_words + (size_t)(b - (uint32_t)lane_words_first) * LW_ROWS * PCR_WORKGROUP_SIZE + tid;
    const uint32_t r0 = lw_wave_row[(size_t)b * (LWC_WAVES + 1) + wave], r1 = lw_wave_row[(size_t)b * (LWC_WAVES + 1) + wave + 1];
    uint32_t *dst = lw_block[b] + (size_t)r0 * 64 + lane;
    for (uint32_t r = 0; r < r1 - r0; ++r) dst[(size_t)r * 64] = src[(size_t)r * PCR_WORKGROUP_SIZE];
}

// The provisional last batch of a stream that is still loading (enqueue_transcode): its block is a fixed scratch block, every wave's
// rows uncompacted (LW_ROWS each) -- nothing to read back, nothing to allocate.
__global__ void k_provisional_block(const uint32_t **lw_block, uint32_t *lw_wave_row, const uint32_t *scratch, int b)
{
    if (threadIdx.x == 0) lw_block[b] = scratch;
    if (threadIdx.x <= (uint32_t)LWC_WAVES) lw_wave_row[(size_t)b * (LWC_WAVES + 1) + threadIdx.x] = threadIdx.x * (uint32_t)LW_ROWS;
}

// ------------------------------------------------------------------------------------------------
// k_bounds: once per loaded batch, behind k_transcode (same launch geometry, same chunk of batches): where the batch's chains
// fall apart into spatial clusters (BatchRuns above). Every lane decodes its chain (the plain checked form of the decode, from
// the chain's own word sequence) and takes the bounding box of its 64 points; the three largest jumps between the box centres
// of consecutive chains cut the batch into four runs; each run gets the box of its chains. A hint and nothing more: it is
// computed with the float form of the dequantisation only (the double form of :459-461 differs by an ulp) and includes
// whatever the chains' garbage tails decode to -- and a frame is the same whatever the windows are.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t float_order(float f) { const uint32_t u = __float_as_uint(f); return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ float float_unorder(uint32_t u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_bounds(StreamView s, const uint32_t *lane_words, uint32_t *batch_runs,
                                                               int first_batch, int lane_words_first)
{
    const uint32_t b = (uint32_t)first_batch + blockIdx.x;
    const uint32_t tid = threadIdx.x;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ float s_centre[PCR_WORKGROUP_SIZE][3];
    __shared__ uint8_t s_outlier[PCR_WORKGROUP_SIZE];
    __shared__ float s_mean[PCR_WORKGROUP_SIZE / 64];
    __shared__ unsigned long long s_best[PCR_WORKGROUP_SIZE / 64];
    __shared__ uint32_t s_cut[MAX_PARTS][RUNS - 1];
    __shared__ uint32_t s_box[MAX_PARTS][RUNS][6];
    __shared__ uint32_t s_all[MAX_PARTS][6];
    reinterpret_cast<uint4 *>(s_table)[tid] = reinterpret_cast<const uint4 *>(s.packed_table + (size_t)b * PCR_HUFFMAN_TABLE_SIZE)[tid];
    const pcr_gpu_batch *gb = s.batches + b;
    const int32_t *sep = s.separate + gb->separate_batch_offset;
    const uint32_t sep_last = (uint32_t)min((int64_t)0x7FFFFFF0, s.separate_words + (PCR_GUARD_WORDS - 2) - gb->separate_batch_offset);
    const int32_t *tvalues = s.table_values + (size_t)b * PCR_HUFFMAN_TABLE_SIZE;
    uint32_t esc = tid ? (uint32_t)s.separate_sizes[(size_t)b * 1024 + tid - 1] : 0u;
    const uint32_t *col = lane_words + (size_t)(b - (uint32_t)lane_words_first) * LW_ROWS * PCR_WORKGROUP_SIZE + tid;
    const int32_t *sv = s.start_values + ((size_t)b * 1024 + tid) * 3;
    int32_t pos[3] = { sv[0], sv[1], sv[2] };
    const float fs[3] = { (float)gb->scale_x, (float)gb->scale_y, (float)gb->scale_z };
    const float fo[3] = { (float)(gb->offset_x - gb->las_min_x), (float)(gb->offset_y - gb->las_min_y), (float)(gb->offset_z - gb->las_min_z) };
    float mn[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, mx[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    __syncthreads();
    // the chain's bit stream = its words in order; `buf` holds the next `avail` (> 32) unconsumed bits at its top
    uint64_t buf = ((uint64_t)col[0] << 32) | col[PCR_WORKGROUP_SIZE];
    uint32_t row = 2;
    int avail = 64;
#pragma unroll 1
    for (int i = 0; i < PCR_POINTS_PER_THREAD; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t key = (uint32_t)(buf >> 52);
            const uint32_t e = s_table[key];
            int32_t val = (int32_t)e >> TE_VALUE_SHIFT;
            if (val == TE_SLOW_VALUE) {
                if (e & TE_ESCAPE) val = sep[min(esc++, sep_last)];
                else               val = tvalues[key];
            }
            pos[k] = (int32_t)((uint32_t)pos[k] + (uint32_t)val);
            const int len = (int)(e & 63u);                 // (a malformed table's longer "lengths" only make the hint useless)
            buf <<= len; avail -= len;
            if (avail <= 32) {
                const uint32_t w = row < (uint32_t)LW_ROWS ? col[(size_t)row * PCR_WORKGROUP_SIZE] : 0u;
                ++row;
                buf |= (uint64_t)w << ((32 - avail) & 63);
                avail += 32;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = __fmaf_rn((float)pos[k], fs[k], fo[k]);
            mn[k] = fminf(mn[k], f); mx[k] = fmaxf(mx[k], f);
        }
    }
    // A chain whose own 64 points straddle a jump of the curve (or whose garbage tail flew off) has a box far larger than its
    // neighbours': it would give a jump on either side and then blow up the box of the run it ends up in. Such chains -- extent
    // over four times the batch's mean -- are looked through when jumps are measured and left out of the runs' boxes (their few
    // points go the global way).
    float extent = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) extent = fmaxf(extent, mx[k] - mn[k]);
    if (!(extent >= 0.0f)) extent = 3.0e38f;                // (NaN)
    {
        float sum = fminf(extent, 1.0e30f);
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) sum += __shfl_xor(sum, m);
        if ((tid & 63u) == 0) s_mean[tid >> 6] = sum;
    }
    __syncthreads();
    float mean = 0.0f;
#pragma unroll
    for (int w = 0; w < PCR_WORKGROUP_SIZE / 64; ++w) mean += s_mean[w];
    mean *= 1.0f / (float)PCR_WORKGROUP_SIZE;
    const bool outlier = extent > 4.0f * mean;
    // jump between my chain's box centre and the one of the nearest ordinary chain before it (at most four back)
#pragma unroll
    for (int k = 0; k < 3; ++k) s_centre[tid][k] = 0.5f * mn[k] + 0.5f * mx[k];
    s_outlier[tid] = outlier ? 1 : 0;
    __syncthreads();
    float gap0 = -1.0f;
    uint32_t prev = 0;
    if (tid && !outlier) {
        prev = tid - 1;
#pragma unroll
        for (int back = 0; back < 3; ++back) if (prev && s_outlier[prev]) --prev;
        gap0 = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) gap0 = fmaxf(gap0, fabsf(s_centre[tid][k] - s_centre[prev][k]));
        if (!(gap0 >= 0.0f) || s_outlier[prev]) gap0 = 0.0f;
    }
    // One record per workgroup shape and part (RUN_RECORDS): the whole batch, then its two halves side by side (every chain
    // belongs to one of them), each cut at the RUNS - 1 largest jumps INSIDE it.
#pragma unroll 1
    for (int cfg = 0; cfg < 2; ++cfg) {
        const uint32_t part_shift = 10u - (uint32_t)cfg, part = tid >> part_shift, part_first = part << part_shift;
        const uint32_t part_waves = 16u >> cfg, wave0 = part * part_waves;
        if (tid < 2 * RUNS * 6) s_box[tid / (RUNS * 6)][(tid / 6) % RUNS][tid % 6] = (tid % 6) < 3 ? 0xFFFFFFFFu : 0u;
        if (tid < 2 * 6) s_all[tid / 6][tid % 6] = (tid % 6) < 3 ? 0xFFFFFFFFu : 0u;
        // (no jump into a part's first chain, none measured against a chain of the other part)
        float gap = (tid == part_first || prev < part_first) ? -1.0f : gap0;
        // the RUNS - 1 largest jumps, one after the other: wave maximum of (gap, chain) by shuffles, then over the part's waves
        for (int round = 0; round < RUNS - 1; ++round) {
            unsigned long long key = gap >= 0.0f ? ((unsigned long long)__float_as_uint(gap) << 32) | tid : 0ull;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(key >> 32), m) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)key, m);
                key = key > o ? key : o;
            }
            if ((tid & 63u) == 0) s_best[tid >> 6] = key;
            __syncthreads();
            unsigned long long best = s_best[wave0];
            for (uint32_t w = 1; w < part_waves; ++w) best = best > s_best[wave0 + w] ? best : s_best[wave0 + w];
            const uint32_t cut = (uint32_t)best;                // (0 if there is no chain left to cut at: a run of no chains)
            if (tid == cut) gap = -1.0f;
            if (tid == part_first) s_cut[part][round] = cut ? cut : (uint32_t)PCR_WORKGROUP_SIZE;
            __syncthreads();
        }
        uint32_t c0 = s_cut[part][0], c1 = s_cut[part][1], c2 = s_cut[part][2];
        static_assert(RUNS == 4, "three cuts, sorted by hand");
        if (c0 > c1) { const uint32_t t = c0; c0 = c1; c1 = t; }
        if (c1 > c2) { const uint32_t t = c1; c1 = c2; c2 = t; }
        if (c0 > c1) { const uint32_t t = c0; c0 = c1; c1 = t; }
        const uint32_t run = (tid >= c0) + (tid >= c1) + (tid >= c2);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!outlier) {
                atomicMin(&s_box[part][run][k], float_order(mn[k]));
                atomicMax(&s_box[part][run][3 + k], float_order(mx[k]));
            }
            // (every chain of the part, straddling ones and garbage tails included: the one window a workgroup would need)
            atomicMin(&s_all[part][k], float_order(mn[k]));
            atomicMax(&s_all[part][3 + k], float_order(mx[k]));
        }
        __syncthreads();
        // the records' words, one thread each: the parts of this shape lie back to back
        const uint32_t nparts = 1u << cfg;
        if (tid < nparts * RUN_WORDS) {
            const uint32_t pi = tid / RUN_WORDS, w = tid % RUN_WORDS;
            uint32_t *out = batch_runs + ((size_t)b * RUN_RECORDS + run_record((int)nparts, (int)pi)) * RUN_WORDS;
            uint32_t v;
            if (w < 4) {
                uint32_t d0 = s_cut[pi][0], d1 = s_cut[pi][1], d2 = s_cut[pi][2];
                if (d0 > d1) { const uint32_t t = d0; d0 = d1; d1 = t; }
                if (d1 > d2) { const uint32_t t = d1; d1 = d2; d2 = t; }
                if (d0 > d1) { const uint32_t t = d0; d0 = d1; d1 = t; }
                v = w == 0 ? d0 : w == 1 ? d1 : w == 2 ? d2 : 0u;
            } else if (w < 4 + RUNS * 6) {
                v = __float_as_uint(float_unorder(s_box[pi][(w - 4) / 6][(w - 4) % 6]));
            } else {
                v = __float_as_uint(float_unorder(s_all[pi][w - 4 - RUNS * 6]));
            }
            out[w] = v;
        }
        __syncthreads();
    }
}

constexpr uint32_t NO_PIXEL = 0xFFFFFFFFu;
typedef float v2f __attribute__((ext_vector_type(2)));

// GENERIC: the checked variant of the decode step, for the batches the prepass put on the second list (flagged
// BF_GENERIC_SLOW_PATH by k_transcode): escape indices are tested against the LDS pool, `wide` table values come from
// global memory. A kernel of its own, so that the ordinary batches' loop carries neither its tests nor its code; the host
// launches it only for streams that have such batches.
// PARTS: workgroups per batch. 1: 1024 threads, the batch's 1024 chains (the reference's shape, render.cu:328). 2: 512 threads,
// chains [512 part, 512 part + 512) -- four workgroups per CU (see DYN_LDS_BYTES_HALF). Workgroup x of the grid draws part
// (x >> 3) & 1 of list entry (x >> 4) * 8 + (x & 7): the hardware deals workgroups round-robin over the eight XCDs, so the two
// halves of a batch run on the same XCD and the second one's table comes out of that XCD's L2.
template <int MODE, int LAYOUT, bool GENERIC, int PARTS = 1>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE / PARTS, 8) k_render(RenderArgs a)   // 8 waves/SIMD = two (four) workgroups per CU -> <= 64 VGPRs
{
    constexpr bool COLOR_PASS = MODE == MODE_HQS_COLOR || MODE == MODE_HQS_COLOR_BC7, BC7 = MODE == MODE_HQS_COLOR_BC7;
    constexpr uint32_t THREADS = PCR_WORKGROUP_SIZE / PARTS;
    static_assert(PARTS == 1 || PARTS == 2, "whole batches or halves");
    const uint32_t part = PARTS == 1 ? 0u : (blockIdx.x >> 3) & 1u;
    // second level of the compaction: which batch is the blockIdx.x-th of my list? Every wave works it out for itself (a
    // 64-lane inclusive prefix sum over the chunk counts, 64 chunks = 2048 batches per round): no barrier, no LDS.
    DrawRec rec;
    {
        const uint32_t lane = threadIdx.x & 63u, chunks = a.order_stride / PREPASS_BATCHES;
        const uint32_t classes = GENERIC ? 1u : a.work_classes;
        uint32_t x = PARTS == 1 ? blockIdx.x : (blockIdx.x >> 4) * 8u + (blockIdx.x & 7u), found = 0xFFFFFFFFu;
        for (uint32_t cls = 0; cls < classes && found == 0xFFFFFFFFu; ++cls) {                  // (uniform; one class unless the frame has a level of detail)
            const uint32_t *cc = a.chunk_count + (GENERIC ? WORK_CLASSES : cls) * PCR_MAX_PREPASS_WORKGROUPS;
            uint32_t before = 0;
            for (uint32_t c0 = 0; c0 < chunks; c0 += 64) {                  // (uniform)
                const uint32_t cnt = c0 + lane < chunks ? cc[c0 + lane] : 0u;
                const uint32_t incl = wave_inclusive_sum(cnt);
                const uint32_t total = wave_read_lane(incl, 63);
                if (x < before + total) {
                    const uint64_t m = __ballot(before + incl > x);        // first chunk whose inclusive count passes x
                    const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1u;
                    const uint32_t excl = wave_read_lane(incl - cnt, first);
                    uint32_t lighter = 0;                                   // the chunk's records of the classes in front of this one
                    for (uint32_t k = 0; k < cls; ++k) lighter += a.chunk_count[k * PCR_MAX_PREPASS_WORKGROUPS + c0 + first];
                    found = (c0 + first) * PREPASS_BATCHES + lighter + (x - before - excl);
                    break;
                }
                before += total;
            }
            x -= before;                                                    // (not found: `before` is the class's total)
        }
        found = __builtin_amdgcn_readfirstlane(found);                      // (the same in every lane: keep it, and the record, scalar)
        if (found == 0xFFFFFFFFu) return;                                   // the grid is sized for "every batch visible"
        rec = a.order[(GENERIC ? (size_t)a.order_stride : 0) + found];
    }
    const uint32_t b = rec.b;
    const uint32_t lod = rec.lod;
    const int npr = (int)(lod & LOD_NPR_MASK);
    const bool use_double = (lod & LOD_DOUBLE) != 0;
    const uint32_t tid = threadIdx.x;
    const uint32_t chain = part * THREADS + tid;            // my chain of the batch's 1024
    // (the lambdas below capture these scalars, not the argument block: with `a` captured by reference and the loop body
    // instantiated five times, hipcc once kept the whole block in scratch memory)
    uint64_t *const g_fb = a.f.fb, *const g_rg = a.f.rg, *const g_ba = a.f.ba;
    uint8_t *const g_tiles = a.f.tiles;
    const uint32_t tiles_x = a.f.tiles_x;
    const int img_w = a.p.width;
    const uint32_t fb_elems = a.f.fb_elems;
    const float m00 = a.p.transform[0], m01 = a.p.transform[1], m02 = a.p.transform[2], m03 = a.p.transform[3];
    const float m10 = a.p.transform[4], m11 = a.p.transform[5], m12 = a.p.transform[6], m13 = a.p.transform[7];

    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // a.dyn_lds_bytes: escape pool, then the framebuffer window
    int32_t *const s_esc = reinterpret_cast<int32_t *>(s_dyn);

    // decoder table -> LDS (render.cu:383-395), four entries per thread, already packed by k_transcode
    const int32_t *tvalues = a.s.table_values + (size_t)b * PCR_HUFFMAN_TABLE_SIZE;   // only for `wide` entries
#pragma unroll
    for (int k = 0; k < PARTS; ++k)
        reinterpret_cast<uint4 *>(s_table)[tid + k * THREADS] = reinterpret_cast<const uint4 *>(a.s.packed_table + (size_t)b * PCR_HUFFMAN_TABLE_SIZE)[tid + k * THREADS];

    const pcr_gpu_batch *gb = a.s.batches + b;
    const int64_t sep_off = rec.sep_off;                    // :405
    const int32_t *sep = a.s.separate + sep_off;            // batch-relative base (uniform)
    // Reads past the logical end of the escape stream (zero pad included) are defined as 0. The allocation carries
    // PCR_GUARD_WORDS extra zero words that nothing ever writes, so clamping the index to the guard is enough:
    // branch-free loads keep every global load of the loop on one control-flow path (no conservative waits).
    const uint32_t sep_last = (uint32_t)min((int64_t)0x7FFFFFF0, a.s.separate_words + (PCR_GUARD_WORDS - 2) - sep_off);
    auto sep_load = [&](uint32_t i) -> int32_t { return sep[min(i, sep_last)]; };

    // ---- escape words of my chains -> LDS (all of them, or none) ---------------------------------------------
    const int32_t *ssz = a.s.separate_sizes + (size_t)b * 1024;
    // [esc_first, esc_first + esc_count): the escape words of the workgroup's chains inside the batch's
    const uint32_t esc_first = PARTS == 1 || part == 0 ? 0u : rec.esc_mid;
    const uint32_t esc_count = PARTS == 1 ? rec.esc_total : part == 0 ? rec.esc_mid : rec.esc_total - rec.esc_mid;
    // The pool also takes ESC_SLACK words that FOLLOW those in memory, so that the reference's tail over-reads
    // find in LDS what they would find in global memory; reads beyond even that, and workgroups whose escapes do not fit, go
    // to global memory (slow variant of the decode step).
    const uint32_t esc_lds = esc_pool_words(esc_count, PARTS);
    unsigned long long *const s_win = reinterpret_cast<unsigned long long *>(s_dyn + esc_pool_bytes(esc_lds));
    const uint32_t win_cap = (uint32_t)window_capacity(esc_count, COLOR_PASS ? WIN_PIXEL_BYTES_HQS : WIN_PIXEL_BYTES, a.dyn_lds_bytes, PARTS);
    {   // all loads of a thread in flight together (7-8 per thread: the pool of an ordinary batch)
        constexpr int EAGER = PARTS == 1 ? 7 : 8;
        int32_t v[EAGER];
#pragma unroll
        for (int k = 0; k < EAGER; ++k) v[k] = sep_load(esc_first + tid + k * THREADS);
#pragma unroll
        for (int k = 0; k < EAGER; ++k)
            if (tid + k * THREADS < esc_lds) s_esc[tid + k * THREADS] = v[k];
        constexpr int REST = (esc_pool_max(PARTS) - EAGER * (int)THREADS) / (int)THREADS;
        static_assert(REST * (int)THREADS + EAGER * (int)THREADS == esc_pool_max(PARTS), "the pool in whole rounds of the workgroup");
        if (esc_lds > (uint32_t)EAGER * THREADS) {          // (uniform) an escape-heavy batch: the rest of its pool
            int32_t u[REST];
#pragma unroll
            for (int k = 0; k < REST; ++k) u[k] = sep_load(esc_first + (EAGER + k) * THREADS + tid);
#pragma unroll
            for (int k = 0; k < REST; ++k) {
                const uint32_t i = (EAGER + k) * THREADS + tid;
                if (i < esc_lds) s_esc[i] = u[k];
            }
        }
    }
    // :411-413 (batch-relative): my chain's next escape word, as a pointer into the pool (the LDS address travels in one
    // register: nothing to add per read)
    const int32_t *esc_next = s_esc + ((chain ? (uint32_t)ssz[chain - 1] : 0u) - esc_first);

    // ---- framebuffer window of the batch's rectangle -> LDS --------------------------------------------------
    // Up to RUNS rectangles per batch (WinPlan): my chain scatters into the window of its run; all of them live in one array of
    // window pixels, in run order. The window is a per-lane matter (runs do not end at wave boundaries): its origin, size and
    // first pixel sit in vector registers.
    const WinPlan *const plan_p = a.win + ((size_t)b * PARTS + part);   // (read field by field: a local copy indexed in a loop lands in scratch)
    uint32_t wpix = 0;                                      // pixels of all windows together; 0: no window for this batch
    uint32_t wx0 = 0, wy0 = 0, ww = 0, wh = 0, wbase = 0;
    {
        const uint32_t run = (chain >= plan_p->first[0]) + (chain >= plan_p->first[1]) + (chain >= plan_p->first[2]);
        static_assert(RUNS == 4, "three run boundaries");
#pragma unroll
        for (int r = 0; r < RUNS; ++r) {
            const uint32_t xy = plan_p->xy[r], wh2 = plan_p->wh[r];
            if (run == (uint32_t)r) { wx0 = xy & 0xFFFFu; wy0 = xy >> 16; ww = wh2 & 0xFFFFu; wh = wh2 >> 16; wbase = wpix; }
            wpix += (wh2 & 0xFFFFu) * (wh2 >> 16);
        }
    }
    const uint32_t W = (uint32_t)a.p.width;
    // colour pass layout of the same bytes: sums in the framebuffer's own packed format + the depth to test against
    // (RG and BA of a pixel side by side: one address per flush of a run, the second add at offset 8; record `wpix`, behind the
    // last window pixel, is a dummy that the first flush of a chain -- which has no run yet -- adds zeros to)
    unsigned long long *const s_acc = s_win;
    uint32_t *const s_depth = reinterpret_cast<uint32_t *>(s_win + 2 * (win_cap + 1));
    // every pixel of every window in turn: fn(index in the window arrays, index in the framebuffer)
    // (row and column of a thread's first pixel by one multiply-and-correct, then stepped: THREADS pixels on are `qy` rows and `qx`
    // columns, one more row where the column wraps -- the division per pixel was 15 of the merge loop's 25 vector instructions per
    // pixel, 4 % of a 4096x4096 launch whose windows have 6000 pixels)
    auto for_window_pixels = [&](auto fn) __attribute__((always_inline)) {
        uint32_t base = 0;
#pragma unroll 1
        for (int r = 0; r < RUNS; ++r) {                                    // (uniform)
            const uint32_t xy = plan_p->xy[r], wh2 = plan_p->wh[r];
            const uint32_t x0 = xy & 0xFFFFu, y0 = xy >> 16, w2 = wh2 & 0xFFFFu, n = w2 * (wh2 >> 16);
            if (tid < n) {                                                   // (n == 0: no such window)
                const float inv_w2 = 1.0f / (float)max(w2, 1u);
                uint32_t y, x, qy, qx;
                window_row_col(tid, w2, inv_w2, y, x);
                window_row_col(THREADS, w2, inv_w2, qy, qx);                 // (uniform)
                uint32_t gp = (y0 + y) * W + x0 + x;
                const uint32_t step = qy * W + qx, wrap = W - w2;
                for (uint32_t i = tid; i < n; i += THREADS) {
                    fn(base + i, (size_t)gp);
                    x += qx; gp += step;
                    if (x >= w2) { x -= w2; gp += wrap; }
                }
            }
            base += n;
        }
    };
    if (!COLOR_PASS) {
        for (uint32_t i = tid; i < wpix; i += THREADS) s_win[i] = ~0ull;
        // The dummy slot, behind the last window pixel: the window word of every point that has none -- outside the frustum, or
        // inside it but outside its window. It starts as 0, so the depth pre-filter below turns such a lane away without a mask
        // for "the pending point is valid" having to be kept (an off-window point's word is replaced by the global one; what its
        // LDS atomic then leaves in the slot is a depth no smaller than any real one there: harmless, and never merged).
        if (tid == 0) s_win[wpix] = 0ull;
    } else {
        // colour pass: the depths of the rectangles as the depth pass left them, sums zeroed
        for_window_pixels([&](uint32_t i, size_t gp) {
            s_depth[i] = (uint32_t)(a.f.fb[gp] >> 32); s_acc[2 * i] = 0; s_acc[2 * i + 1] = 0;
        });
        if (tid == 0) { s_acc[2 * wpix] = 0; s_acc[2 * wpix + 1] = 0; }
    }

    // ---- my chain's own word sequence (k_transcode) ---------------------------------------------------------
    // The chain's bit stream is the concatenation of its words. w0..w2 are three consecutive words, `spare` = 32 minus
    // the number of bits of w0 already consumed (0..31); far0/far1 are the two words after w2, requested one point
    // before they can be needed. Per point a 64-bit view `bits` of the next unconsumed bits is cut out once, the three
    // symbols (<= 36 bits) and the look-ahead of the next point's first symbol (12 more) index into it, and the words
    // that ran dry are retired afterwards: no refill test, load or wait inside the symbol steps.
    // (Cur/Next of :416-419 are the first two words; the stand-in w0 = 0 is "fully consumed" from the start.)
    // LAYOUT_POINT_WINDOWS: the view of every point was cut by k_transcode; row i of point_windows is read at point i
    // (requested two points earlier) and there is no queue.
    // LAYOUT_WORDS: my wave's rows of the batch's compact block (k_pack_words); a request past the last row the wave's longest
    // chain consumed reads the next wave's rows or the segment's pad (LWC_PAD_ROWS: such a word is requested ahead but never looked at)
    // (a pointer loaded from memory is a generic one to hipcc: flat_load_dword behind a 64-bit vector add per request. Said to be
    // global, the block's base stays in a scalar register pair and a request is global_load_dword v, voffset, s[base:base+1])
    typedef const __attribute__((address_space(1))) char *global_bytes;
    global_bytes lwb = nullptr;
    if (LAYOUT == LAYOUT_WORDS) {
        const uint32_t wave = __builtin_amdgcn_readfirstlane(chain >> 6);
        const uint32_t *wr = a.s.lw_wave_row + (size_t)b * (LWC_WAVES + 1) + wave;
        lwb = (global_bytes)(reinterpret_cast<const char *>(a.s.lw_block[b]) + (size_t)wr[0] * LWC_ROW_BYTES);   // uniform per wave
    }
    auto lw_load = [&](uint32_t byte_off) -> uint32_t { return *(const __attribute__((address_space(1))) uint32_t *)(lwb + byte_off); };
    const char *pwb = reinterpret_cast<const char *>(a.s.point_windows) + (size_t)b * PW_BATCH_BYTES;               // uniform
    // the 40-bit window of a point as the top of a 64-bit view: high plane u32, low plane u8 (the 24 bits below are zero).
    // Window rows come through buffer loads: the lane's column offset stays put in a vector register, the row advances in a scalar
    // one (buffer_load_dword v, voffset, s[rsrc], soffset offen) -- no vector add per row and plane (with plain pointers hipcc either
    // advanced a per-lane offset or added the lane's offset to an advancing uniform pointer with a 64-bit vector add). (HQS -0.7 %,
    // LOD 10 % -1.2 %, LOD 100 % within the noise: the two adds were of the cheap class.) The descriptor's range check does not
    // cover the row reads: it looks at voffset alone (the column, always in range), not at the row in soffset. The rows read ahead
    // past the batch's block land in real memory only because the allocation carries PW_GUARD_BYTES behind the last block.
    const __amdgpu_buffer_rsrc_t pw_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)const_cast<char *>(pwb), 0, (int)(PW_BATCH_BYTES + PW_GUARD_BYTES), 0x00020000);
    uint32_t pw_row_hi = 0, pw_row_lo = PW_HI_BYTES;        // (uniform) byte offsets of the current row in the two planes
    const uint32_t pw_col_hi = chain * 4, pw_col_lo = chain;
    auto pw_load_hi = [&]() -> uint32_t { return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(pw_rsrc, (int)pw_col_hi, (int)pw_row_hi, 0); };
    auto pw_load_lo = [&]() -> uint32_t { return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(pw_rsrc, (int)pw_col_lo, (int)pw_row_lo, 0); };
#define PCR_PW_NEXT_ROW() do { pw_row_hi += PW_HI_ROW_BYTES; pw_row_lo += PW_LO_ROW_BYTES; } while (0)
    uint32_t lwo = (tid & 63u) * 4;                         // packed words: byte offset of my column in the row of far0
    uint32_t w0 = 0, w1 = 0, w2 = 0, far0 = 0, far1 = 0, spare = 0;
    uint64_t bits;
    uint32_t nwin_hi = 0, nwin_lo = 0;
    if (LAYOUT == LAYOUT_WORDS) {
        w1 = lw_load(lwo); w2 = lw_load(lwo + LWC_ROW_BYTES);
        far0 = lw_load(lwo + 2 * LWC_ROW_BYTES); far1 = lw_load(lwo + 3 * LWC_ROW_BYTES);
        lwo += 2 * LWC_ROW_BYTES;
        bits = ((uint64_t)__builtin_amdgcn_alignbit(w0, w1, spare) << 32) | __builtin_amdgcn_alignbit(w1, w2, spare);
    } else {
        bits = ((uint64_t)pw_load_hi() << 32) | (pw_load_lo() << 24);
        PCR_PW_NEXT_ROW();
        nwin_hi = pw_load_hi(); nwin_lo = pw_load_lo() << 24;
    }
    constexpr uint32_t SFT0 = 50;                           // (bits >> 50) & 0x3FFC = 4 x the top 12 bits of the view
    uint32_t sft = SFT0;

    const int32_t *sv = a.s.start_values + ((size_t)b * 1024 + chain) * 3; // :421-424
    int32_t px = sv[0], py = sv[1], pz = sv[2];

    const double sx = gb->scale_x, sy = gb->scale_y, sz = gb->scale_z;
    const double ox = gb->offset_x - gb->las_min_x, oy = gb->offset_y - gb->las_min_y, oz = gb->offset_z - gb->las_min_z;
    const float fsx = (float)sx, fsy = (float)sy, fsz = (float)sz;          // :469
    const float fox = (float)ox, foy = (float)oy, foz = (float)oz;          // :470

    uint32_t payload = 0;
    if (MODE == MODE_HQS_DEPTH) {
        if (a.p.show_num_points)      payload = (uint32_t)npr;                                   // depth.cu:139-140
        else if (a.p.colorize_chunks) payload = (uint32_t)(a.s.batch_index_base + b);            // :141-142
    }

    // BC1 blocks of my chain (4 blocks of 16 points, 8 bytes each): the block of the current 16-point segment in
    // registers, the next one prefetched a whole segment (16 iterations) before its first use
    const uint2 *cblocks = reinterpret_cast<const uint2 *>(a.s.colors_t) + ((size_t)b * 4096 + chain);        // [segment][chain]
    uint2 cnext = make_uint2(0, 0);
    Bc1Palette pal = {0, 0, 0, 0};
    if (MODE != MODE_HQS_DEPTH && !BC7) cnext = cblocks[0];
    // (BC7 colours, 16 bytes per block: the block of a segment is read at its start -- no register for a prefetched one)
    const uint4 *blocks7 = reinterpret_cast<const uint4 *>(a.s.colors_t) + ((size_t)b * 4096 + chain);
    Bc7Block pal7 = {0, 0, 0, 0, 0};

    // Second half of rasterize() (render.cu:297-301 / depth.cu:148-151 / hqs render.cu:292-313) for the point whose
    // framebuffer word `old` was fetched one iteration earlier, from the LDS window (widx) or from global memory.
    // A stale `old` only makes the filter less selective: framebuffer words never increase during a pass.
    // colour pass: run of contributions to one pixel held in registers
    // (two 16-bit sums per register: a chain adds at most 64 * 255 per channel)
    uint32_t run_pix = NO_PIXEL, run_widx = wpix;           // (no run yet: zeros for the dummy record)
    uint32_t run_rg16 = 0, run_bc16 = 0;                    // r << 16 | g,  b << 16 | count
    auto flush_run = [&]() __attribute__((always_inline)) {
        const unsigned long long run_rg = ((unsigned long long)(run_rg16 >> 16) << 32) | (run_rg16 & 0xFFFFu);
        const unsigned long long run_ba = ((unsigned long long)(run_bc16 >> 16) << 32) | (run_bc16 & 0xFFFFu);
        if (run_widx != NO_PIXEL) {
            // per-batch partial sums in LDS (a batch adds at most 65 536 * 255 < 2^32 per 32-bit half)
            __hip_atomic_fetch_add(&s_acc[2 * run_widx], run_rg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&s_acc[2 * run_widx + 1], run_ba, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            atomicAdd((unsigned long long *)&g_rg[run_pix], run_rg);        // :309-310
            atomicAdd((unsigned long long *)&g_ba[run_pix], run_ba);        // :311-312
        }
    };
    // colour pass: the contribution of a point that passed the 1 % test (hqs render.cu:297-313)
    auto accumulate = [&](bool off, uint32_t pix, uint32_t w, int point) __attribute__((always_inline)) {
        uint32_t vrg, vbc;                                                     // r << 16 | g,  b << 16 | 1
        if (BC7) {
            const uint32_t rgba = bc7_color(pal7, (uint32_t)point & 15u);
            vrg = __builtin_amdgcn_perm(0u, rgba, 0x0C000C01u);                 // (rgba = 0x00BBGGRR)
            vbc = (rgba & 0x00FF0000u) | 1u;
        } else {
            bc1_contribution(pal, (uint32_t)point & 15u, vrg, vbc);
        }
        // Consecutive points of a chain are Morton neighbours and mostly land in the same pixel: their
        // contributions are summed in registers and written once per run (sums commute, so the totals
        // are unchanged; a chain adds at most 64 * 255 per 32-bit half).
        if (pix == run_pix) {
            run_rg16 += vrg; run_bc16 += vbc;
        } else {
            flush_run();
            run_pix = pix; run_widx = off ? NO_PIXEL : w; run_rg16 = vrg; run_bc16 = vbc;
        }
    };
    // colour pass: the 1 % test of the pending point, then its contribution. `valid`: the point is inside the frustum; `off`:
    // ... but outside the batch's LDS window (then `pix` is its pixel and `old` came from global memory); `w`: its window index.
    // Both flags come from lane masks the compiler keeps in scalar registers, so choosing between the LDS and the global path
    // costs no vector instruction.
    auto scatter = [&](bool valid, bool off, uint32_t pix, uint32_t w, uint32_t depth, uint64_t old, int point) __attribute__((always_inline)) {
        const float pw = __uint_as_float(depth);
        const float old_depth = __uint_as_float((uint32_t)(old >> 32));
        if (valid && (double)pw <= (double)old_depth * 1.01) {              // hqs render.cu:296
            accumulate(off, pix, w, point);
        }
    };

    // Basic / depth pass: the same for a pending point described without per-lane flags. Its window word `wp` is the dummy slot
    // unless the point lies in its window; `old` is that word, or the global framebuffer word for the lanes of `off_mask`
    // (inside the frustum, outside the window). A lane with nothing pending holds a dummy word of depth 0 and fails the filter.
    // Scalar instructions are not free here (+16 of them per point: +6 % kernel time, profiles/r03_experiments.md): lane masks
    // carried as 64-bit values and tested as such cost a compare and a branch, bools carried across the loop cost three
    // mask merges each.
    auto scatter_min = [&](__attribute__((address_space(3))) unsigned long long *wp, uint32_t depth, uint32_t old_hi, uint64_t off_mask, uint32_t pix, int point) __attribute__((always_inline)) {
        // pre-read filter (:297-298) on the depth half only: the result is min(depth<<32|payload) over all inside points
        // whatever passes it (min is idempotent), so ties go to the atomic instead of a 64-bit compare here
        if (depth > old_hi) return;
        const unsigned long long key = ((unsigned long long)depth << 32) | (MODE == MODE_BASIC ? bc1_color(pal, (uint32_t)point & 15u) : payload);   // :299 / depth.cu:139-145
        __hip_atomic_fetch_min(wp, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__builtin_amdgcn_inverse_ballot_w64(off_mask)) atomicMin((unsigned long long *)&g_fb[pix], key);   // :300 (rare)
    };

    // Packed words, end of a point: SFT0 - sft bits were consumed. Retire the 0..2 words that ran dry, pull in far0/far1 (requested
    // a whole point ago), request the next two, cut the next view. u = spare - consumed + 64 lies in [28, 95].
#define PCR_ADVANCE_WORD_WINDOW()                                                          \
    do {                                                                                   \
        const uint32_t u_ = spare + (sft & 63u) + (64u - SFT0);                            \
        const uint32_t k_ = u_ >> 5;               /* 2: no word retired, 1: one, 0: two */ \
        spare = u_ & 31u;                                                                  \
        const uint32_t n0_ = k_ == 2u ? w0 : k_ == 1u ? w1 : w2;                           \
        const uint32_t n1_ = k_ == 2u ? w1 : k_ == 1u ? w2 : far0;                         \
        const uint32_t n2_ = k_ == 2u ? w2 : k_ == 1u ? far0 : far1;                       \
        w0 = n0_; w1 = n1_; w2 = n2_;                                                      \
        lwo += (2u - k_) * LWC_ROW_BYTES;                                                  \
        /* the two words behind w2, requested afresh for every point (round 3 fetched only the words that moved up, 0.7 loads per \
           point, under two branches: loads that may or may not have been issued make every later vmcnt wait a wait for all -- in the \
           depth pass hipcc ended up waiting for this iteration's requests in the middle of the iteration) */ \
        far0 = lw_load(lwo);                                                               \
        far1 = lw_load(lwo + LWC_ROW_BYTES);                                               \
        bits = ((uint64_t)__builtin_amdgcn_alignbit(w0, w1, spare) << 32) | __builtin_amdgcn_alignbit(w1, w2, spare); \
        sft = SFT0;                                                                        \
    } while (0)

    uint64_t pend_valid_mask = 0;                           // colour pass: lanes whose pending point is inside the frustum
    uint64_t pend_off_mask = 0;                             // lanes whose pending point is inside the frustum but outside its window
    const uint32_t whole_x0 = plan_p->whole_xy & 0xFFFFu, whole_y0 = plan_p->whole_xy >> 16;
    const uint32_t whole_w = plan_p->whole_wh & 0xFFFFu, whole_h = plan_p->whole_wh >> 16;
    const bool mostly_outside = plan_p->mostly_outside != 0;    // (uniform) the batch and most of its neighbours lie mostly outside their windows
    uint32_t pend_pix = NO_PIXEL, pend_w = 0, pend_depth = 0;
    typedef __attribute__((address_space(3))) unsigned long long lds_u64;
    lds_u64 *const s_win_mine = (lds_u64 *)(s_win + wbase); // my run's window
    lds_u64 *const s_dummy = (lds_u64 *)(s_win + wpix);     // (see the window's set-up)
    const uint32_t dummy_idx = wpix - wbase;                // ... as an index into my run's window
    lds_u64 *pend_p = s_dummy;                              // basic / depth pass: the pending point's word in the LDS window
    uint64_t pend_old = 0;                                  // (colour pass)
    uint32_t pend_old_hi = 0;                               // basic / depth pass: the depth half of the pending point's framebuffer word

    const float *M = a.p.transform;
    const float fw = (float)a.p.width, fh = (float)a.p.height;
    // Loop constants kept in vector registers on purpose: a v_fma_f32 / v_sub_u32 whose operands are all VGPRs or inline
    // constants issues in ~2.3 cycles per wave64, the same instruction with an SGPR operand in ~4.2
    // (tools/exp/instr_rate2.hip). The kernel has the registers to spare (<= 64 for eight waves per SIMD).
    // (only where there are registers to spare: not in the colour pass, which keeps its run of sums in registers, not with
    // the packed-words variant's five-word queue, not in the checked variant)
    constexpr bool VGPR_CONSTANTS = !COLOR_PASS && LAYOUT == LAYOUT_POINT_WINDOWS && !GENERIC;
    auto in_vgpr_f = [](float v) { if (!VGPR_CONSTANTS) return v; float r; asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(v)); return r; };
    const float m30 = in_vgpr_f(M[12]), m31 = in_vgpr_f(M[13]), m32 = in_vgpr_f(M[14]), m33 = in_vgpr_f(M[15]);   // the w row
    const uint32_t v_wx0 = wx0, v_wy0 = wy0;                // (per-lane values: in vector registers anyway)

    __syncthreads();        // table, escapes and window are visible

    // All three table entries of a point are requested during the iteration before it, spread over that iteration (see the
    // loop); these are the ones of point 0.
    // Packed words (round 4): the same order. A point's view is cut from the chain's word queue once the lengths of the point before
    // it are known -- at the top of the iteration, where all three of its entries have arrived -- so the queue advances THERE,
    // the words it needs were requested a whole iteration earlier, and the three entries of point i+1 are requested from the new
    // view during iteration i exactly as with the point windows. (Round 3 cut the view symbol by symbol: every table read of a
    // point hung on the one before it, two round trips per point exposed.)
    uint32_t toff_ahead = (uint32_t)(bits >> (sft & 63u)) & 0x3FFCu;
    uint32_t e_ahead = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s_table) + toff_ahead);
    const uint32_t sft_ahead = SFT0 - e_ahead;              // :439 (the whole entry: byte 0 is the length)
    uint32_t toff1_ahead = ((uint32_t)(bits >> 32) >> (sft_ahead & 31u)) & 0x3FFCu;
    uint32_t e1_ahead = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s_table) + toff1_ahead);
    uint32_t toff2_ahead = (uint32_t)(bits >> ((sft_ahead - e1_ahead) & 63u)) & 0x3FFCu;
    uint32_t e2_ahead = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s_table) + toff2_ahead);

    // ---- the point loop ---------------------------------------------------------------------------------------------------------
    // A wave issues in order and the decode is a chain of LDS round trips (table entry -> length -> next key -> next
    // entry). What can run inside those waits does: the table entries of a point are requested during the point before it, the
    // scatter of the previous point runs under the reads of this point's escape words, the framebuffer word of a point is requested
    // a whole point before it is used. A deeper software pipeline (decode k+2 | project k+1 | scatter k, the projection split over
    // the second and third table read) was built and measured: +4 %, hipcc spends the 64 registers on copies between the stages
    // (profiles/r02_experiments.md).

    // The delta a table entry stands for (:435-438): the entry's own value, or -- escape -- the chain's next escape word. `toff`
    // is the entry's byte offset in the table: 4 x the 12-bit window of :431-433 (== ((L|R) & mask) >> 20).
    auto entry_value = [&](uint32_t e, uint32_t toff) __attribute__((always_inline)) -> uint32_t {
        int32_t val = (int32_t)e >> TE_VALUE_SHIFT;                         // the delta itself (v_ashrrev_i32)
        if (val == TE_SLOW_VALUE) {                                         // escape or wide
            if (!GENERIC) {                                                 // every such entry is an escape whose word is in the pool
                val = *esc_next++;
            } else if (e & TE_ESCAPE) {                                     // :438
                if (esc_next < s_esc + esc_lds) {
                    val = *esc_next;
                } else {
                    // outside the pool: the load is consumed inside this branch so no pending VMEM result leaves it
                    val = sep_load(esc_first + (uint32_t)(esc_next - s_esc));
                    asm volatile("; escape word from global memory %0" : "+v"(val));
                }
                ++esc_next;
            } else {
                val = tvalues[toff >> 2];
                asm volatile("; wide table value from global memory %0" : "+v"(val));
            }
        }
        return (uint32_t)val;
    };
    auto table_entry = [&](uint32_t toff) __attribute__((always_inline)) -> uint32_t {
        return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s_table) + toff);
    };
    // Top of iteration i (the entries e0..e2 of point i have arrived): request the first entry of point i+1. Point
    // windows: its key is the top of the window that has been in registers for an iteration. Packed words: the queue advances by
    // what point i consumed (the three lengths: byte 0 of the entries, subtracted whole -- only the low six bits of `sft` count),
    // the view of point i+1 is cut, its top twelve bits are the key. (A macro, not a lambda: a closure that captures the word queue
    // by reference put the kernel's whole parameter block into scratch memory.)
#define PCR_NEXT_FIRST_ENTRY(e0_, e1_, e2_)                                                 \
    do {                                                                                    \
        if (LAYOUT == LAYOUT_POINT_WINDOWS) {                                               \
            toff_ahead = (nwin_hi >> (SFT0 & 31u)) & 0x3FFCu;                               \
        } else {                                                                            \
            sft = SFT0 - (e0_) - (e1_) - (e2_);                                             \
            PCR_ADVANCE_WORD_WINDOW();                                                      \
            toff_ahead = ((uint32_t)(bits >> 32) >> (SFT0 & 31u)) & 0x3FFCu;                \
        }                                                                                   \
        e_ahead = table_entry(toff_ahead);                                                  \
    } while (0)

    for (int seg = 0; seg < npr; seg += 16) {
      // Segment boundary: the point still pending belongs to the previous BC1 block, so it is scattered before the
      // block registers rotate (its framebuffer word has been in flight for the whole decode of the last point).
      if (COLOR_PASS) { scatter(__builtin_amdgcn_inverse_ballot_w64(pend_valid_mask), __builtin_amdgcn_inverse_ballot_w64(pend_off_mask), pend_pix, pend_w, pend_depth, pend_old, seg - 1); pend_valid_mask = 0; pend_off_mask = 0; }
      else { scatter_min(pend_p, pend_depth, pend_old_hi, pend_off_mask, pend_pix, seg - 1); pend_p = s_dummy; pend_off_mask = 0;
             // (the dummy slot's zero, READ rather than set: with an LDS read behind the last table request on this way into the loop
             // as well as on the way round it, hipcc's wait for that entry at the top of an iteration leaves one result in flight)
             pend_old_hi = reinterpret_cast<__attribute__((address_space(3))) const volatile uint32_t *>(s_dummy)[1]; }
      if (MODE != MODE_HQS_DEPTH) {
          if (BC7) pal7 = bc7_block(blocks7[(seg >> 4) * PCR_WORKGROUP_SIZE]);
          else {
              pal = bc1_palette(cnext);                 // once per 16 points instead of once per surviving point
                                                        // (palettes expanded at load time, 16 bytes per block: measured twice, rounds 2 and 4: nothing)
              cnext = cblocks[min((seg >> 4) + 1, 3) * PCR_WORKGROUP_SIZE];
          }
      }
      const int seg_end = min(seg + 16, npr);
#pragma unroll 1
      for (int i = seg; i < seg_end; ++i) {                                 // :428
        uint32_t fetched_hi = 0, fetched_lo = 0;
        if (LAYOUT == LAYOUT_POINT_WINDOWS) {
            // row i+2, requested at the top of point i and taken over at its very end: a whole point of latency cover
            // (past row 63 of a plane lies the batch's other plane, the next batch, or the guard)
            PCR_PW_NEXT_ROW();
            fetched_hi = pw_load_hi(); fetched_lo = pw_load_lo();
        }
        uint32_t d0, d1, d2;
        // All three table entries of point i were requested while point i-1 was projected: nothing of the decode's dependent
        // chain (entry -> length -> key -> entry) is waited for here. The escape words of the three symbols, if any, are
        // requested back to back; the scatter of point i-1 runs under them. The entries of point i+1 (its window has been in
        // registers since the top of the last iteration) are requested in three places of this iteration, each a table
        // round trip after the one before: here, in front of the dot products, behind the division.
        const uint32_t e0 = e_ahead, toff0 = toff_ahead, e1 = e1_ahead, toff1 = toff1_ahead, e2 = e2_ahead, toff2 = toff2_ahead;
        if (!GENERIC) {
            // Everything that hangs on a result of the last iteration -- the three entries, the framebuffer word of point i-1 --
            // is looked at BEFORE this iteration issues its first LDS instruction: results return in issue order and hipcc
            // counts a read under a branch (an escape word's) as maybe not issued, so a wait placed behind such reads waits for
            // them as well. What is tested becomes a lane mask in a scalar register pair.
            int32_t v0 = (int32_t)e0 >> TE_VALUE_SHIFT, v1 = (int32_t)e1 >> TE_VALUE_SHIFT, v2 = (int32_t)e2 >> TE_VALUE_SHIFT;
            const uint64_t esc0 = __builtin_amdgcn_ballot_w64(v0 == TE_SLOW_VALUE), esc1 = __builtin_amdgcn_ballot_w64(v1 == TE_SLOW_VALUE),
                           esc2 = __builtin_amdgcn_ballot_w64(v2 == TE_SLOW_VALUE);
            // the pre-read filter of scatter_min / the 1 % test of the colour pass (hqs render.cu:296)
            const uint64_t draw = COLOR_PASS
                ? pend_valid_mask & __builtin_amdgcn_ballot_w64((double)__uint_as_float(pend_depth) <= (double)__uint_as_float((uint32_t)(pend_old >> 32)) * 1.01)
                : __builtin_amdgcn_ballot_w64(pend_depth <= pend_old_hi);
            if (__builtin_expect(__builtin_amdgcn_inverse_ballot_w64(esc0), 1)) v0 = *esc_next++;               // :438 (every such entry is an escape whose word is in the pool)
            if (__builtin_expect(__builtin_amdgcn_inverse_ballot_w64(esc1), 1)) v1 = *esc_next++;
            if (__builtin_expect(__builtin_amdgcn_inverse_ballot_w64(esc2), 1)) v2 = *esc_next++;
            PCR_NEXT_FIRST_ENTRY(e0, e1, e2);
            if (COLOR_PASS) {
                if (__builtin_amdgcn_inverse_ballot_w64(draw)) accumulate(__builtin_amdgcn_inverse_ballot_w64(pend_off_mask), pend_pix, pend_w, i - 1);
            } else if (__builtin_amdgcn_inverse_ballot_w64(draw)) {                         // second half of rasterize() for point i-1
                const unsigned long long key = ((unsigned long long)pend_depth << 32) | (MODE == MODE_BASIC ? bc1_color(pal, (uint32_t)(i - 1) & 15u) : payload);
                __hip_atomic_fetch_min(pend_p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (__builtin_amdgcn_inverse_ballot_w64(pend_off_mask)) atomicMin((unsigned long long *)&g_fb[pend_pix], key);   // :300 (rare)
            }
            d0 = (uint32_t)v0; d1 = (uint32_t)v1; d2 = (uint32_t)v2;
        } else {
            d0 = entry_value(e0, toff0);                                    // :430
            d1 = entry_value(e1, toff1);
            d2 = entry_value(e2, toff2);
            PCR_NEXT_FIRST_ENTRY(e0, e1, e2);
            if (COLOR_PASS) scatter(__builtin_amdgcn_inverse_ballot_w64(pend_valid_mask), __builtin_amdgcn_inverse_ballot_w64(pend_off_mask), pend_pix, pend_w, pend_depth, pend_old, i - 1);
            else scatter_min(pend_p, pend_depth, pend_old_hi, pend_off_mask, pend_pix, i - 1);
        }
        px = (int32_t)((uint32_t)px + d0);                                  // :454-456, :463
        py = (int32_t)((uint32_t)py + d1);
        pz = (int32_t)((uint32_t)pz + d2);
        if (LAYOUT == LAYOUT_POINT_WINDOWS) {               // the view of point i+1 (packed words: cut at the top of the iteration)
            bits = ((uint64_t)nwin_hi << 32) | nwin_lo;
            sft = SFT0;
        }
        // (per-point temporaries and the three parts of the projection live inside the loop body: nothing of a point's
        // projection is carried into the next iteration -- with ix / iy declared outside, every iteration copied them)
        float fx, fy, fz;
        float qx, qy, qw;
        uint64_t cand_mask;                 // lanes whose point is inside the frustum, as a 64-bit lane mask (a scalar register pair)
        int ix, iy;
        // first half of rasterize() (:278-287), part 1: the three dot products and the inside test without dividing. For finite
        // w > 0 the correctly rounded quotient RN(x/w) lies in [-1,1] exactly when |x| <= w (if x > w then x/w >= 1 + ulp(w)/w >
        // 1 + 2^-24, which rounds above 1); the compare is false for a NaN and for w < 0.
        auto project_dots = [&]() __attribute__((always_inline)) {
            qx = __fmaf_rn(m03, 1.0f, __fmaf_rn(m02, fz, __fmaf_rn(m01, fy, m00 * fx)));       // dot4(M + 0, ...)
            qy = __fmaf_rn(m13, 1.0f, __fmaf_rn(m12, fz, __fmaf_rn(m11, fy, m10 * fx)));       // dot4(M + 4, ...)
            qw = __fmaf_rn(m33, 1.0f, __fmaf_rn(m32, fz, __fmaf_rn(m31, fy, m30 * fx)));       // dot4(M + 12, ...), operands in VGPRs
            // (lane masks as 64-bit scalars: a ballot of a compare IS the compare's result register, mask logic is one scalar
            // instruction each, and nothing is merged where control flow joins)
            cand_mask = __builtin_amdgcn_ballot_w64(fabsf(qx) <= qw) & __builtin_amdgcn_ballot_w64(fabsf(qy) <= qw);
        };
        // part 2: the division and the pixel (:279-285). The division is the IEEE sequence hipcc emits for `/` with its range
        // scaling removed, shared reciprocal, x and y packed; it is bit-identical to `/` for w in [2^-64, 2^64) (no intermediate
        // leaves the normal range unless |x/w| < 2^-36, where the pixel is the screen centre whatever the last bits are). A
        // wave in which some candidate's w lies outside that range (or is 0) takes `/` for all lanes.
        auto project_divide = [&]() __attribute__((always_inline)) {
            // (both forms run for every lane, candidate or not -- a lane that is not one produces a pixel nobody looks at: the
            // instructions issue for the wave anyway, and with ix / iy written on every path hipcc neither masks the block nor
            // carries last iteration's pixel along for the lanes that skipped it)
            {
                const float r0 = __builtin_amdgcn_rcpf(qw);
                const float r1 = __fmaf_rn(__fmaf_rn(-qw, r0, 1.0f), r0, r0);
                const v2f xy = {qx, qy}, rr = {r1, r1}, nw = {-qw, -qw};
                const v2f q0 = xy * rr;
                const v2f q1 = __builtin_elementwise_fma(__builtin_elementwise_fma(nw, q0, xy), rr, q0);
                const v2f q2 = __builtin_elementwise_fma(__builtin_elementwise_fma(nw, q1, xy), rr, q1);
                const v2f half = {0.5f, 0.5f}, size = {fw, fh};
                const v2f img = __builtin_elementwise_fma(q2, half, half) * size;       // :283
                ix = (int)img.x; iy = (int)img.y;                                       // :284 (a candidate's pixel index is always < fb_elems here)
            }
            // (the plain `/` as an override behind the fast form, not as its `else`: an if / else of a uniform condition costs the
            // common path two branches and three scalar instructions here, an `if` alone one of each)
            const uint64_t w_ok_mask = __builtin_amdgcn_ballot_w64((__float_as_uint(qw) - 0x1F800000u) < 0x40000000u);   // 2^-64 <= w < 2^64
            if (__builtin_expect((cand_mask & ~w_ok_mask) != 0, 0)) {
                const float nx = qx / qw, ny = qy / qw;
                ix = (int)(__fmaf_rn(nx, 0.5f, 0.5f) * fw);                 // :283-284
                iy = (int)(__fmaf_rn(ny, 0.5f, 0.5f) * fh);
                // (inside <=> candidate here as well: for w > 0 the correctly rounded quotient lies in [-1,1] exactly when |x| <= w,
                // a NaN or w < 0 fails both forms, and a pixel of a point inside is below fb_elems -- Appendix C.2. w == 0 with
                // x == y == 0 -- a point exactly in the eye, or a degenerate matrix -- passes |x| <= w and is no candidate: :296 `w <= 0`)
                cand_mask &= __builtin_amdgcn_ballot_w64(qw > 0.0f);
            }
        };
        // part 3: the point becomes the pending one; its framebuffer word is requested now and consumed an iteration later:
        // from the LDS window if the pixel lies in the batch's rectangle (nearly always), from global memory otherwise (:297)
        auto project_request = [&]() __attribute__((always_inline)) {
            if (!COLOR_PASS) {
                // No flags per lane, no block under `if (inside)`: every lane works out a window position (garbage for a lane that is
                // not inside), the masks decide. The window word is read by EVERY lane (the dummy slot's if it has none): with the
                // read issued on every path hipcc knows how many LDS results are outstanding at the top of the next iteration and
                // waits for the look-ahead table entry alone (lgkmcnt(1)) instead of for this read as well.
                const uint32_t rx = (uint32_t)ix - v_wx0, ry = (uint32_t)iy - v_wy0;
                // (bitwise: `&&` would put the two compares under a branch of their own)
                const uint64_t in_mask = cand_mask & __builtin_amdgcn_ballot_w64(rx < ww) & __builtin_amdgcn_ballot_w64(ry < wh);
                pend_off_mask = cand_mask & ~in_mask;
                pend_depth = __float_as_uint(qw);                                       // :287
                pend_p = s_win_mine + (__builtin_amdgcn_inverse_ballot_w64(in_mask) ? (uint32_t)__umul24(ry, ww) + rx : dummy_idx);
                // (the depth half alone: the filter looks at nothing else, and a 64-bit read whose low half nobody wants had hipcc reuse
                // that register while the read was in flight -- and wait for it)
                pend_old_hi = reinterpret_cast<__attribute__((address_space(3))) const uint32_t *>(pend_p)[1];
                if (__builtin_expect(pend_off_mask != 0, 0)) {              // (uniform, rare: the window plan keeps nearly every point inside)
                    // Is one of them outside the rectangle the prepass marked the dirty tiles under as well (FrameView::tiles)? The
                    // garbage tails of chains are: a thousandth of the points, anywhere on the screen. Whole-wave
                    // compares under the scalar branch: a mask updated inside the divergent branch below is no longer uniform -- and
                    // the packed-words variant then drew wrong frames (round 3; convergent operations in divergent control flow).
                    const uint64_t stray_now = g_tiles ? pend_off_mask & (__builtin_amdgcn_ballot_w64((uint32_t)ix - whole_x0 >= whole_w) |
                                                                          __builtin_amdgcn_ballot_w64((uint32_t)iy - whole_y0 >= whole_h)) : 0;
                    const bool sample = mostly_outside;                             // (uniform) see below
                    if (__builtin_amdgcn_inverse_ballot_w64(pend_off_mask)) {
                        pend_pix = (uint32_t)(ix + iy * img_w);                         // :285
                        if (__builtin_amdgcn_inverse_ballot_w64(stray_now)) {
                            // its own tile (ndc == 1.0 maps to column W, Appendix C.2: in the linear framebuffer that is column 0 of the next row)
                            const uint32_t mx = ix >= img_w ? 0u : (uint32_t)ix, my = ix >= img_w ? (uint32_t)iy + 1u : (uint32_t)iy;
                            g_tiles[(my >> TILE_H_SHIFT) * tiles_x + (mx >> TILE_W_SHIFT)] = 1;
                        }
                        // The pre-read of the global framebuffer word (:297) is a filter in front of the global atomic -- min is
                        // idempotent, the frame is the same without it -- that costs the wave a memory round trip per point. It stops
                        // 70-85 % of the points it sees, whatever the frame (profiles/r03_experiments.md); what differs is how many there
                        // are. In a Morton-sorted stream 0.2 % (1080p) to 5 % (close-up) of a frame's wave-iterations have such lanes,
                        // 9-31 of them, concentrated in a few waves that the round trips turn into the launch's stragglers: without
                        // the load 4096x4096 is 8 % faster, a close-up 7 %, the benchmark frame 2.6 %. In an unsorted stream (a batch
                        // is a strip across the scene, ten points per pixel) it is every iteration and 57 lanes, and unfiltered the
                        // frame takes 1.7 x the time in atomics. A few batches of that kind among the others are cheaper unfiltered (the
                        // atomic units have room), a frame full of them is not: the prepass votes per 32 neighbouring batches
                        // (WinPlan::mostly_outside).
                        pend_old_hi = 0xFFFFFFFFu;
                        if (sample) {
                            // (consumed inside the branch: no load is pending where the paths join, so hipcc's waits for the window
                            // rows, requested two points ahead, stay exact)
                            uint32_t seen = __hip_atomic_load(reinterpret_cast<const uint32_t *>(&g_fb[pend_pix]) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                            asm volatile("; framebuffer word of a point outside its window %0" : "+v"(seen));
                            pend_old_hi = seen;
                        }
                    }
                }
                return;
            }
            // colour pass, the same without flags per lane: every lane works out a pixel and a window position (garbage for a lane
            // that is not inside), the masks decide; a lane with no window word reads the window's first one (any valid address
            // will do: its result is not looked at, or replaced below)
            const uint32_t rx = (uint32_t)ix - v_wx0, ry = (uint32_t)iy - v_wy0;
            const uint64_t in_mask = cand_mask & __builtin_amdgcn_ballot_w64(rx < ww) & __builtin_amdgcn_ballot_w64(ry < wh);
            pend_valid_mask = cand_mask;
            pend_off_mask = cand_mask & ~in_mask;
            pend_depth = __float_as_uint(qw);                                           // :287
            pend_pix = (uint32_t)(ix + iy * img_w);                         // the colour pass names its runs by pixel
            pend_w = wbase + (__builtin_amdgcn_inverse_ballot_w64(in_mask) ? ry * ww + rx : 0u);
            pend_old = (uint64_t)s_depth[pend_w] << 32;
            if (__builtin_expect(pend_off_mask != 0, 0)) {
                if (__builtin_amdgcn_inverse_ballot_w64(pend_off_mask)) pend_old = __hip_atomic_load(&g_fb[pend_pix], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        };

        // (the float form always, the double form as an override for the batches that want it: see project_divide)
        fx = __fmaf_rn((float)px, fsx, fox);                                // :529-531
        fy = __fmaf_rn((float)py, fsy, foy);
        fz = __fmaf_rn((float)pz, fsz, foz);
        if (use_double) {                                                   // :459-461
            fx = (float)__fma_rn((double)px, sx, ox);
            fy = (float)__fma_rn((double)py, sy, oy);
            fz = (float)__fma_rn((double)pz, sz, oz);
        }
        // second entry of point i+1 (`bits` is its window by now; the first has arrived)
        const uint32_t sft1_next = SFT0 - e_ahead;
        toff1_ahead = ((uint32_t)(bits >> 32) >> (sft1_next & 31u)) & 0x3FFCu;
        e1_ahead = table_entry(toff1_ahead);
        project_dots();                                                     // first half of rasterize() (:278-287) for point i
        project_divide();
        // third entry of point i+1
        toff2_ahead = (uint32_t)(bits >> ((sft1_next - e1_ahead) & 63u)) & 0x3FFCu;
        e2_ahead = table_entry(toff2_ahead);
        project_request();
        if (LAYOUT == LAYOUT_POINT_WINDOWS) { nwin_hi = fetched_hi; nwin_lo = fetched_lo << 24; }
      }
    }
    if (COLOR_PASS) { scatter(__builtin_amdgcn_inverse_ballot_w64(pend_valid_mask), __builtin_amdgcn_inverse_ballot_w64(pend_off_mask), pend_pix, pend_w, pend_depth, pend_old, npr - 1); flush_run(); }
    else scatter_min(pend_p, pend_depth, pend_old_hi, pend_off_mask, pend_pix, npr - 1);

    // merge the window into the global framebuffer: rows of the rectangle are contiguous, so the 64 lanes of a wave
    // hit a handful of cache lines; only pixels this batch improved issue an atomic
    if (wpix) {
        __syncthreads();
        for_window_pixels([&](uint32_t i, size_t gp) {
            if (COLOR_PASS) {
                const unsigned long long vba = s_acc[2 * i + 1];
                if (vba) {
                    atomicAdd((unsigned long long *)&a.f.rg[gp], s_acc[2 * i]);
                    atomicAdd((unsigned long long *)&a.f.ba[gp], vba);
                }
            } else {
                const unsigned long long v = s_win[i];
                unsigned long long *g = (unsigned long long *)&a.f.fb[gp];
                // (no read of the global word in front of the atomic: the compare only saved atomics -- min is idempotent -- at the
                // price of a memory round trip per row of the window while the workgroup holds its LDS; 4096x4096 -4 %, 1080p -0.6 %)
                if (v != ~0ull) atomicMin(g, v);                            // (a pixel no point of the batch reached issues nothing)
            }
        });
    }
}

// ------------------------------------------------------------------------------------------------
// k_decode_points: the loaded stream back to points (pcr_decode_points). No counterpart in the reference, whose only decoder
// outside its render kernels is the per-chain CPU one of include/huffman.h:433-477. One workgroup per batch, one lane per
// chain, all 64 points of every chain -- no cull, no level of detail, the garbage tails as they are -- from what
// k_render reads and maybe_finalize() keeps: the packed table, start values, escape words, the colour blocks in segment-major
// order, and the chain's own bits in either resident layout (the same reads as k_render's at 64 points per chain: the
// packed words' rows up to four behind the wave's last one, window rows clamped to the batch's 64).
// Escapes and `wide` table values come from global memory as k_bounds reads them (index clamped into the guard): a flagged
// batch (BF_GENERIC_SLOW_PATH*) needs no second kernel and no pool in LDS. Escape words are requested a point ahead, at the
// top of every point and whether or not anybody reads them (three words per point: a point consumes at most three): the
// loads are on every path (no wait under a branch) -- nearly every wave has an escape in every point (3 % of the symbols
// x 192 per wave) -- and have a whole point to arrive in. (Measured against requesting them at the top of the same point:
// no difference on the benchmark stream; kept for the escape-heavy ones.)
// Output: record (b - first_batch) * 65536 + 64 chain + i = {x, y, z, 0x00BBGGRR}. A lane that stored its own records would
// write 16 bytes every 1024: 64 cache lines per store instruction. Instead every wave collects DEC_STAGE_POINTS points of its
// 64 chains in LDS (8 KiB; 16-byte slot j of chain c at c * 8 + (j ^ (c >> 1 & 7)): a 16-lane group of the ds_write_b128 --
// sixteen chains, one j -- and of the ds_read_b128 -- two chains, eight j -- covers the sixteen slots of a 256-byte bank row
// once) and writes them back eight lanes per chain: every global_store_dwordx4 writes eight whole 128-byte lines
// (non-temporal: nobody on the device reads the records back soon; 4 % on the 1e8-point stream, profiles/decode_points.json).
// The staging is per wave, so the point loop has no workgroup barrier. 16 KiB table + 128 KiB staging: one workgroup per CU,
// four waves per SIMD.
// ------------------------------------------------------------------------------------------------
constexpr int DEC_STAGE_POINTS = 8;
constexpr uint32_t DEC_STAGE_WAVE_SLOTS = 64 * DEC_STAGE_POINTS;                       // 16-byte records per wave
constexpr uint32_t DEC_LDS_BYTES = LWC_WAVES * DEC_STAGE_WAVE_SLOTS * 16;              // dynamic LDS of a launch: 128 KiB
static_assert(sizeof(pcr_point) == 16, "one dwordx4 store per record");

template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_decode_points(StreamView s, uint4 *out, uint32_t first_batch)
{
    static_assert(DEC_STAGE_POINTS == 8 && PCR_POINTS_PER_THREAD % 16 == 0, "eight lanes write a chain's 128 bytes; two flushes per colour block");
    const uint32_t b = first_batch + blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // DEC_LDS_BYTES
    uint4 *const stage = reinterpret_cast<uint4 *>(s_dyn) + wave * DEC_STAGE_WAVE_SLOTS;
    reinterpret_cast<uint4 *>(s_table)[tid] = reinterpret_cast<const uint4 *>(s.packed_table + (size_t)b * PCR_HUFFMAN_TABLE_SIZE)[tid];

    const pcr_gpu_batch *gb = s.batches + b;
    const int32_t *sep = s.separate + gb->separate_batch_offset;
    const uint32_t sep_last = (uint32_t)min((int64_t)0x7FFFFFF0, s.separate_words + (PCR_GUARD_WORDS - 2) - gb->separate_batch_offset);
    const int32_t *tvalues = s.table_values + (size_t)b * PCR_HUFFMAN_TABLE_SIZE;     // only for `wide` entries
    uint32_t esc = tid ? (uint32_t)s.separate_sizes[(size_t)b * 1024 + tid - 1] : 0u;
    const int32_t *sv = s.start_values + ((size_t)b * 1024 + tid) * 3;
    int32_t px = sv[0], py = sv[1], pz = sv[2];

    // my chain's bits. Packed words: three consecutive words w0..w2 of the chain's sequence, `spare` = 32 minus the bits of w0
    // already consumed, far0 / far1 the two words behind w2, requested a point before they can move up (k_render's queue).
    // Point windows: row i of the batch's two planes is the 40-bit view of point i, requested two points ahead.
    // (the block's base as a global pointer in scalar registers + a per-lane byte offset, as in k_render: a pointer loaded from
    // memory is a generic one to hipcc -- flat loads, which count on the LDS counter as well)
    typedef const __attribute__((address_space(1))) char *global_bytes;
    global_bytes lwb = nullptr;
    uint32_t lwo = lane * 4;                                // byte offset of my column in the row of far0
    auto lw_load = [&](uint32_t byte_off) -> uint32_t { return *(const __attribute__((address_space(1))) uint32_t *)(lwb + byte_off); };
    uint32_t w0 = 0, w1 = 0, w2 = 0, far0 = 0, far1 = 0, spare = 0;
    const uint32_t *pw_hi = nullptr;
    const uint8_t *pw_lo = nullptr;
    uint32_t win_hi[2] = {0, 0}, win_lo[2] = {0, 0};        // the views of points i and i + 1
    if (LAYOUT == LAYOUT_WORDS) {
        const uint32_t *wr = s.lw_wave_row + (size_t)b * (LWC_WAVES + 1) + wave;
        lwb = (global_bytes)(reinterpret_cast<const char *>(s.lw_block[b]) + (size_t)wr[0] * LWC_ROW_BYTES);    // uniform per wave
        w1 = lw_load(lwo); w2 = lw_load(lwo + LWC_ROW_BYTES);
        far0 = lw_load(lwo + 2 * LWC_ROW_BYTES); far1 = lw_load(lwo + 3 * LWC_ROW_BYTES);
        lwo += 2 * LWC_ROW_BYTES;
    } else {
        pw_hi = reinterpret_cast<const uint32_t *>(s.point_windows + (size_t)b * PW_BATCH_BYTES) + tid;
        pw_lo = s.point_windows + (size_t)b * PW_BATCH_BYTES + PW_HI_BYTES + tid;
        win_hi[0] = pw_hi[0]; win_lo[0] = pw_lo[0];
        win_hi[1] = pw_hi[PCR_WORKGROUP_SIZE]; win_lo[1] = pw_lo[PCR_WORKGROUP_SIZE];
    }

    // colour blocks of my chain: [segment][chain], the next segment's requested a segment ahead
    const uint2 *blocks1 = reinterpret_cast<const uint2 *>(s.colors_t) + ((size_t)b * 4096 + tid);
    const uint4 *blocks7 = reinterpret_cast<const uint4 *>(s.colors_t) + ((size_t)b * 4096 + tid);
    uint2 next1 = make_uint2(0, 0);
    uint4 next7 = make_uint4(0, 0, 0, 0);
    if (BC7) next7 = blocks7[0]; else next1 = blocks1[0];

    // write-back: lane l stores record (l & 7) of chains (l >> 3) + 8 k of the wave
    uint4 *const out_wave = out + ((size_t)blockIdx.x * PCR_POINTS_PER_BATCH + (size_t)wave * 64 * PCR_POINTS_PER_THREAD);
    const uint32_t my_slot = lane * DEC_STAGE_POINTS, my_swz = (lane >> 1) & 7u;
    const uint32_t rd_chain = lane >> 3, rd_j = lane & 7u;

    // Escape words: qa0..2 = the three at the chain's position before the last point, qb0..2 = the three behind those (requested
    // at the top of the last point), esc_prev = how many the last point consumed. A point's own three are cut out of those six
    // AFTER its table walk, so a request has a whole point to arrive in.
    int32_t qa0 = sep[min(esc, sep_last)], qa1 = sep[min(esc + 1u, sep_last)], qa2 = sep[min(esc + 2u, sep_last)];
    int32_t qb0 = sep[min(esc + 3u, sep_last)], qb1 = sep[min(esc + 4u, sep_last)], qb2 = sep[min(esc + 5u, sep_last)];
    uint32_t esc_prev = 0;

    __syncthreads();        // the table is visible

#pragma unroll 1
    for (int seg = 0; seg < PCR_POINTS_PER_THREAD / 16; ++seg) {
        Bc1Palette pal = {0, 0, 0, 0};
        Bc7Block pal7 = {0, 0, 0, 0, 0};
        const int seg_next = min(seg + 1, PCR_POINTS_PER_THREAD / 16 - 1);
        if (BC7) { pal7 = bc7_block(next7); next7 = blocks7[(size_t)seg_next * PCR_WORKGROUP_SIZE]; }
        else     { pal = bc1_palette(next1); next1 = blocks1[(size_t)seg_next * PCR_WORKGROUP_SIZE]; }
#pragma unroll 1
        for (int half = 0; half < 16 / DEC_STAGE_POINTS; ++half) {
            const int i0 = seg * 16 + half * DEC_STAGE_POINTS;
#pragma unroll
            for (int j = 0; j < DEC_STAGE_POINTS; ++j) {
                // the escape words three to five behind the chain's next one, whether any point reads them or not (see above)
                const int32_t c0 = sep[min(esc + 3u, sep_last)], c1 = sep[min(esc + 4u, sep_last)], c2 = sep[min(esc + 5u, sep_last)];
                uint64_t bits;
                if (LAYOUT == LAYOUT_WORDS) {
                    bits = ((uint64_t)__builtin_amdgcn_alignbit(w0, w1, spare) << 32) | __builtin_amdgcn_alignbit(w1, w2, spare);
                } else {
                    bits = ((uint64_t)win_hi[0] << 32) | (win_lo[0] << 24);
                    win_hi[0] = win_hi[1]; win_lo[0] = win_lo[1];
                    const uint32_t r = (uint32_t)min(i0 + j + 2, PW_ROWS - 1);          // (uniform)
                    win_hi[1] = pw_hi[(size_t)r * PCR_WORKGROUP_SIZE]; win_lo[1] = pw_lo[(size_t)r * PCR_WORKGROUP_SIZE];
                }
                // the three symbols (:430-439): key = the twelve bits at the head of the view, byte 0 of the entry = length
                const uint32_t hi = (uint32_t)(bits >> 32);
                const uint32_t k0 = hi >> 20, e0 = s_table[k0];
                const uint32_t l0 = e0 & 63u;
                const uint32_t k1 = ((hi << (l0 & 31u)) >> 20), e1 = s_table[k1];
                const uint32_t l01 = l0 + (e1 & 63u);
                const uint32_t k2 = (uint32_t)((bits << (l01 & 63u)) >> 52), e2 = s_table[k2];
                int32_t v0 = (int32_t)e0 >> TE_VALUE_SHIFT, v1 = (int32_t)e1 >> TE_VALUE_SHIFT, v2 = (int32_t)e2 >> TE_VALUE_SHIFT;
                // this point's escape words: three of the six requested one and two points ago, by what the last point consumed
                const int32_t q0 = esc_prev == 0u ? qa0 : esc_prev == 1u ? qa1 : esc_prev == 2u ? qa2 : qb0;
                const int32_t q1 = esc_prev == 0u ? qa1 : esc_prev == 1u ? qa2 : esc_prev == 2u ? qb0 : qb1;
                const int32_t q2 = esc_prev == 0u ? qa2 : esc_prev == 1u ? qb0 : esc_prev == 2u ? qb1 : qb2;
                qa0 = q0; qa1 = q1; qa2 = q2; qb0 = c0; qb1 = c1; qb2 = c2;
                uint32_t n = 0;
                if (v0 == TE_SLOW_VALUE) {
                    if (e0 & TE_ESCAPE) { v0 = q0; n = 1; }                                 // :438
                    else { v0 = tvalues[k0]; asm volatile("; wide table value from global memory %0" : "+v"(v0)); }
                }
                if (v1 == TE_SLOW_VALUE) {
                    if (e1 & TE_ESCAPE) { v1 = n ? q1 : q0; ++n; }
                    else { v1 = tvalues[k1]; asm volatile("; wide table value from global memory %0" : "+v"(v1)); }
                }
                if (v2 == TE_SLOW_VALUE) {
                    if (e2 & TE_ESCAPE) { v2 = n == 0 ? q0 : n == 1 ? q1 : q2; ++n; }
                    else { v2 = tvalues[k2]; asm volatile("; wide table value from global memory %0" : "+v"(v2)); }
                }
                esc += n; esc_prev = n;
                px = (int32_t)((uint32_t)px + (uint32_t)v0);                                // :454-456, :463
                py = (int32_t)((uint32_t)py + (uint32_t)v1);
                pz = (int32_t)((uint32_t)pz + (uint32_t)v2);
                if (LAYOUT == LAYOUT_WORDS) {
                    // retire the 0..2 words that ran dry, pull in far0 / far1, request the two behind the new w2 (k_render's
                    // PCR_ADVANCE_WORD_WINDOW: u = spare - consumed + 64)
                    const uint32_t u = spare + ((64u - l01 - (e2 & 63u)) & 127u);
                    const uint32_t k = min(u >> 5, 2u);     // 2: no word retired, 1: one, 0: two
                    spare = u & 31u;
                    const uint32_t n0 = k == 2u ? w0 : k == 1u ? w1 : w2;
                    const uint32_t n1 = k == 2u ? w1 : k == 1u ? w2 : far0;
                    const uint32_t n2 = k == 2u ? w2 : k == 1u ? far0 : far1;
                    w0 = n0; w1 = n1; w2 = n2;
                    lwo += (2u - k) * LWC_ROW_BYTES;
                    far0 = lw_load(lwo); far1 = lw_load(lwo + LWC_ROW_BYTES);
                }
                const uint32_t colour = BC7 ? bc7_color(pal7, (uint32_t)(half * DEC_STAGE_POINTS + j)) : bc1_color(pal, (uint32_t)(half * DEC_STAGE_POINTS + j));
                stage[my_slot + ((uint32_t)j ^ my_swz)] = make_uint4((uint32_t)px, (uint32_t)py, (uint32_t)pz, colour);
            }
            // my wave's 64 x 8 records are in LDS (DS operations of a wave execute in order; the fences only stop the compiler)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int k = 0; k < 64 / 8; ++k) {
                const uint32_t c = rd_chain + 8u * (uint32_t)k;
                const uint4 rec = stage[c * DEC_STAGE_POINTS + (rd_j ^ ((c >> 1) & 7u))];
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 v = {rec.x, rec.y, rec.z, rec.w};
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(&out_wave[(size_t)c * PCR_POINTS_PER_THREAD + (uint32_t)i0 + rd_j]));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Box selection (pcr_batch_point_bounds / pcr_select_box): the points of a range of batches that lie inside an axis-aligned
// box of the stream's int32 coordinates, as k_decode_points would write them with the records outside the box removed.
//   k_point_bounds  once per batch (cached by the context): the exact integer box of the 65 536 records k_decode_points writes
//                   for it, garbage tails and padding included -- pcr_gpu_batch::min/max and the k_bounds boxes are float hints
//   k_select_count  per batch that straddles the box: how many of each chain's 64 points are inside, and their sum
//   k_select_write  per straddling batch: a workgroup prefix over those 1024 counts, then every chain writes its selected
//                   records consecutively from its offset (batches wholly inside go through k_decode_points)
// The three share decode_chain(): k_decode_points' point loop restated with a sink per point instead of the staged write-back
// (k_decode_points itself is left as it is: its schedule was tuned around the staging). Without colours and staging a workgroup
// needs the 16 KiB table and a few hundred bytes of LDS, so several fit a CU. No workgroup waits for another one: the offsets
// between batches are a prefix sum on the host, which has to learn the count anyway.
// ------------------------------------------------------------------------------------------------
enum { SEL_NO_COLOUR = 0, SEL_BC1 = 1, SEL_BC7 = 2 };

// All 64 points of chain `tid` of batch b, in order: sink(i, x, y, z, colour) (colour 0 with SEL_NO_COLOUR). s_table holds the
// batch's packed table and is visible to the workgroup. The reads are k_decode_points' (see there). npr < 64 (uniform over the
// workgroup): the chain's first npr points only, as a level of detail draws them -- the walk stops at the end of the group of
// eight that holds point npr - 1 (the reads of a group are those of the full walk), the sink sees no point beyond it.
template <int LAYOUT, int COLOUR, class Sink>
__device__ __forceinline__ void decode_chain(const StreamView &s, uint32_t b, const uint32_t *s_table, Sink &&sink, int npr = PCR_POINTS_PER_THREAD)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const pcr_gpu_batch *gb = s.batches + b;
    const int32_t *sep = s.separate + gb->separate_batch_offset;
    const uint32_t sep_last = (uint32_t)min((int64_t)0x7FFFFFF0, s.separate_words + (PCR_GUARD_WORDS - 2) - gb->separate_batch_offset);
    const int32_t *tvalues = s.table_values + (size_t)b * PCR_HUFFMAN_TABLE_SIZE;     // only for `wide` entries
    uint32_t esc = tid ? (uint32_t)s.separate_sizes[(size_t)b * 1024 + tid - 1] : 0u;
    const int32_t *sv = s.start_values + ((size_t)b * 1024 + tid) * 3;
    int32_t px = sv[0], py = sv[1], pz = sv[2];

    typedef const __attribute__((address_space(1))) char *global_bytes;
    global_bytes lwb = nullptr;
    uint32_t lwo = lane * 4;
    auto lw_load = [&](uint32_t byte_off) -> uint32_t { return *(const __attribute__((address_space(1))) uint32_t *)(lwb + byte_off); };
    uint32_t w0 = 0, w1 = 0, w2 = 0, far0 = 0, far1 = 0, spare = 0;
    const uint32_t *pw_hi = nullptr;
    const uint8_t *pw_lo = nullptr;
    uint32_t win_hi[2] = {0, 0}, win_lo[2] = {0, 0};
    if (LAYOUT == LAYOUT_WORDS) {
        const uint32_t *wr = s.lw_wave_row + (size_t)b * (LWC_WAVES + 1) + wave;
        lwb = (global_bytes)(reinterpret_cast<const char *>(s.lw_block[b]) + (size_t)wr[0] * LWC_ROW_BYTES);
        w1 = lw_load(lwo); w2 = lw_load(lwo + LWC_ROW_BYTES);
        far0 = lw_load(lwo + 2 * LWC_ROW_BYTES); far1 = lw_load(lwo + 3 * LWC_ROW_BYTES);
        lwo += 2 * LWC_ROW_BYTES;
    } else {
        pw_hi = reinterpret_cast<const uint32_t *>(s.point_windows + (size_t)b * PW_BATCH_BYTES) + tid;
        pw_lo = s.point_windows + (size_t)b * PW_BATCH_BYTES + PW_HI_BYTES + tid;
        win_hi[0] = pw_hi[0]; win_lo[0] = pw_lo[0];
        win_hi[1] = pw_hi[PCR_WORKGROUP_SIZE]; win_lo[1] = pw_lo[PCR_WORKGROUP_SIZE];
    }

    const uint2 *blocks1 = reinterpret_cast<const uint2 *>(s.colors_t) + ((size_t)b * 4096 + tid);
    const uint4 *blocks7 = reinterpret_cast<const uint4 *>(s.colors_t) + ((size_t)b * 4096 + tid);
    uint2 next1 = make_uint2(0, 0);
    uint4 next7 = make_uint4(0, 0, 0, 0);
    if (COLOUR == SEL_BC7) next7 = blocks7[0]; else if (COLOUR == SEL_BC1) next1 = blocks1[0];

    int32_t qa0 = sep[min(esc, sep_last)], qa1 = sep[min(esc + 1u, sep_last)], qa2 = sep[min(esc + 2u, sep_last)];
    int32_t qb0 = sep[min(esc + 3u, sep_last)], qb1 = sep[min(esc + 4u, sep_last)], qb2 = sep[min(esc + 5u, sep_last)];
    uint32_t esc_prev = 0;

#pragma unroll 1
    for (int seg = 0; seg < PCR_POINTS_PER_THREAD / 16 && seg * 16 < npr; ++seg) {
        Bc1Palette pal = {0, 0, 0, 0};
        Bc7Block pal7 = {0, 0, 0, 0, 0};
        const int seg_next = min(seg + 1, PCR_POINTS_PER_THREAD / 16 - 1);
        if (COLOUR == SEL_BC7) { pal7 = bc7_block(next7); next7 = blocks7[(size_t)seg_next * PCR_WORKGROUP_SIZE]; }
        else if (COLOUR == SEL_BC1) { pal = bc1_palette(next1); next1 = blocks1[(size_t)seg_next * PCR_WORKGROUP_SIZE]; }
#pragma unroll 1
        for (int half = 0; half < 2 && seg * 16 + half * 8 < npr; ++half) {
            const int i0 = seg * 16 + half * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int32_t c0 = sep[min(esc + 3u, sep_last)], c1 = sep[min(esc + 4u, sep_last)], c2 = sep[min(esc + 5u, sep_last)];
                uint64_t bits;
                if (LAYOUT == LAYOUT_WORDS) {
                    bits = ((uint64_t)__builtin_amdgcn_alignbit(w0, w1, spare) << 32) | __builtin_amdgcn_alignbit(w1, w2, spare);
                } else {
                    bits = ((uint64_t)win_hi[0] << 32) | (win_lo[0] << 24);
                    win_hi[0] = win_hi[1]; win_lo[0] = win_lo[1];
                    const uint32_t r = (uint32_t)min(i0 + j + 2, PW_ROWS - 1);
                    win_hi[1] = pw_hi[(size_t)r * PCR_WORKGROUP_SIZE]; win_lo[1] = pw_lo[(size_t)r * PCR_WORKGROUP_SIZE];
                }
                const uint32_t hi = (uint32_t)(bits >> 32);
                const uint32_t k0 = hi >> 20, e0 = s_table[k0];
                const uint32_t l0 = e0 & 63u;
                const uint32_t k1 = ((hi << (l0 & 31u)) >> 20), e1 = s_table[k1];
                const uint32_t l01 = l0 + (e1 & 63u);
                const uint32_t k2 = (uint32_t)((bits << (l01 & 63u)) >> 52), e2 = s_table[k2];
                int32_t v0 = (int32_t)e0 >> TE_VALUE_SHIFT, v1 = (int32_t)e1 >> TE_VALUE_SHIFT, v2 = (int32_t)e2 >> TE_VALUE_SHIFT;
                const int32_t q0 = esc_prev == 0u ? qa0 : esc_prev == 1u ? qa1 : esc_prev == 2u ? qa2 : qb0;
                const int32_t q1 = esc_prev == 0u ? qa1 : esc_prev == 1u ? qa2 : esc_prev == 2u ? qb0 : qb1;
                const int32_t q2 = esc_prev == 0u ? qa2 : esc_prev == 1u ? qb0 : esc_prev == 2u ? qb1 : qb2;
                qa0 = q0; qa1 = q1; qa2 = q2; qb0 = c0; qb1 = c1; qb2 = c2;
                uint32_t n = 0;
                if (v0 == TE_SLOW_VALUE) {
                    if (e0 & TE_ESCAPE) { v0 = q0; n = 1; }
                    else { v0 = tvalues[k0]; asm volatile("; wide table value from global memory %0" : "+v"(v0)); }
                }
                if (v1 == TE_SLOW_VALUE) {
                    if (e1 & TE_ESCAPE) { v1 = n ? q1 : q0; ++n; }
                    else { v1 = tvalues[k1]; asm volatile("; wide table value from global memory %0" : "+v"(v1)); }
                }
                if (v2 == TE_SLOW_VALUE) {
                    if (e2 & TE_ESCAPE) { v2 = n == 0 ? q0 : n == 1 ? q1 : q2; ++n; }
                    else { v2 = tvalues[k2]; asm volatile("; wide table value from global memory %0" : "+v"(v2)); }
                }
                esc += n; esc_prev = n;
                px = (int32_t)((uint32_t)px + (uint32_t)v0);
                py = (int32_t)((uint32_t)py + (uint32_t)v1);
                pz = (int32_t)((uint32_t)pz + (uint32_t)v2);
                if (LAYOUT == LAYOUT_WORDS) {
                    const uint32_t u = spare + ((64u - l01 - (e2 & 63u)) & 127u);
                    const uint32_t k = min(u >> 5, 2u);
                    spare = u & 31u;
                    const uint32_t n0 = k == 2u ? w0 : k == 1u ? w1 : w2;
                    const uint32_t n1 = k == 2u ? w1 : k == 1u ? w2 : far0;
                    const uint32_t n2 = k == 2u ? w2 : k == 1u ? far0 : far1;
                    w0 = n0; w1 = n1; w2 = n2;
                    lwo += (2u - k) * LWC_ROW_BYTES;
                    far0 = lw_load(lwo); far1 = lw_load(lwo + LWC_ROW_BYTES);
                }
                const uint32_t colour = COLOUR == SEL_BC7 ? bc7_color(pal7, (uint32_t)(half * 8 + j))
                                      : COLOUR == SEL_BC1 ? bc1_color(pal, (uint32_t)(half * 8 + j)) : 0u;
                if (i0 + j < npr) sink(i0 + j, px, py, pz, colour);
            }
        }
    }
}

__device__ __forceinline__ void load_packed_table(const StreamView &s, uint32_t b, uint32_t *s_table)
{
    reinterpret_cast<uint4 *>(s_table)[threadIdx.x] = reinterpret_cast<const uint4 *>(s.packed_table + (size_t)b * PCR_HUFFMAN_TABLE_SIZE)[threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ bool in_box(const pcr_box &q, int32_t x, int32_t y, int32_t z)
{
    return x >= q.min[0] && x <= q.max[0] && y >= q.min[1] && y <= q.max[1] && z >= q.min[2] && z <= q.max[2];
}

// bounds[(first_batch + blockIdx.x) * 6 ..] = min x, y, z, max x, y, z of the batch's 65 536 decoded records
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_point_bounds(StreamView s, int32_t *bounds, uint32_t first_batch)
{
    const uint32_t b = first_batch + blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ int32_t s_part[LWC_WAVES][6];
    load_packed_table(s, b, s_table);
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        lo[0] = min(lo[0], x); lo[1] = min(lo[1], y); lo[2] = min(lo[2], z);
        hi[0] = max(hi[0], x); hi[1] = max(hi[1], y); hi[2] = max(hi[2], z);
    });
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo[k] = min(lo[k], __shfl_xor(lo[k], d, 64));
            hi[k] = max(hi[k], __shfl_xor(hi[k], d, 64));
        }
        if (lane == 0) { s_part[wave][k] = lo[k]; s_part[wave][3 + k] = hi[k]; }
    }
    __syncthreads();
    if (tid < 6) {
        int32_t v = s_part[0][tid];
        for (int w = 1; w < LWC_WAVES; ++w) v = tid < 3 ? min(v, s_part[w][tid]) : max(v, s_part[w][tid]);
        bounds[(size_t)b * 6 + tid] = v;
    }
}

// The write kernels' place of a chain among the chains of its workgroup, from each chain's count `mine`: the inclusive prefix inside
// the wave, whose last lane leaves the wave's sum in s_part; then, once a barrier has published s_part, the count of every chain
// before this one
__device__ __forceinline__ uint32_t chain_prefix_in_wave(uint32_t mine, uint32_t lane, uint32_t wave, uint32_t *s_part)
{
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) s_part[wave] = incl;
    return incl;
}
__device__ __forceinline__ uint32_t chain_prefix_before(uint32_t incl, uint32_t mine, uint32_t wave, const uint32_t *s_part)
{
    uint32_t before = incl - mine;
    for (uint32_t w = 0; w < wave; ++w) before += s_part[w];
    return before;
}

// Workgroup x takes the straddling batch list[x]: chain_counts[x * 1024 + chain] = its points inside q, totals[x] = their sum
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_select_count(StreamView s, const uint32_t *list, pcr_box q, uint32_t *chain_counts, uint32_t *totals)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    load_packed_table(s, b, s_table);
    uint32_t cnt = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) { cnt += in_box(q, x, y, z) ? 1u : 0u; });
    chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid] = cnt;
    uint32_t sum = cnt;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w];
        totals[blockIdx.x] = t;
    }
}

// Workgroup x takes the straddling batch list[x]: its selected records go to out[offsets[x] ..], chain after chain, each chain's
// in point order (k_decode_points' order with the gaps closed). chain_counts is k_select_count's, for the same list and box.
// The simplest store path: a lane stores its own 16-byte records where they belong.
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_select_write(StreamView s, const uint32_t *list, pcr_box q, const uint32_t *chain_counts,
                                                                     const int64_t *offsets, uint4 *out)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const uint32_t mine = chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid];
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_packed_table(s, b, s_table);                       // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    uint4 *dst = out + offsets[blockIdx.x] + before;
    uint4 *const end = dst + mine;                          // never past what k_select_count counted for this chain
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        if (in_box(q, x, y, z) && dst < end) *dst++ = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
    });
}

// ------------------------------------------------------------------------------------------------
// Polygon selection (pcr_select_polygon): k_select_count / k_select_write with a polygon prism as the test, for the batches
// whose exact box the prism's boundary crosses. The host (pcr_polygon.h) gives every such batch a slice of one edge array --
// only the edges a point of the batch's box can count -- and a base parity for the edges all its points count. The workgroup
// copies its slice into LDS beside the table (16 bytes an edge, launch-sized to the largest slice listed, at most 64 KiB).
// Per point: the z range and the bounding rectangle of the polygon's vertices first (outside it a point is not in the polygon;
// inside it every difference below fits 32 bits and every product stays below 2^62), then a loop over the slice in which all
// lanes read the same entry (one ds_read_b128 that broadcasts), an unsigned compare y - l.y < dy that covers both ends of the
// half-open row range, two 32 x 32 -> 64 multiplies and a signed compare, XORed into the parity.
// ------------------------------------------------------------------------------------------------
struct PolyBatch { uint32_t b, edge_first, edge_count, base_parity; };      // a straddling batch and its slice of the edge array
struct PolyArgs {
    int32_t x0, y0, x1, y1;         // the bounding rectangle of all vertices
    int32_t z_min, z_max;
    uint32_t invert;                // 0 or 1
    uint32_t lds_edges;             // edges the launch's dynamic LDS holds behind the table: the largest slice listed
    const PolyBatch *batches;
    const PolyEdge *edges;
};
constexpr uint32_t POLY_TABLE_BYTES = PCR_HUFFMAN_TABLE_SIZE * 4;

// The batch's table and edge slice into LDS; returns false (uniformly) for a slice the launch has no room for, which the host
// never lists. The barrier publishes both.
__device__ __forceinline__ bool load_polygon_batch(const StreamView &s, const PolyArgs &a, const PolyBatch &pb, uint32_t *s_table, int4 *s_edges)
{
    if (pb.edge_count > a.lds_edges) return false;
    const int4 *src = reinterpret_cast<const int4 *>(a.edges) + pb.edge_first;
    for (uint32_t i = threadIdx.x; i < pb.edge_count; i += PCR_WORKGROUP_SIZE) s_edges[i] = src[i];
    load_packed_table(s, pb.b, s_table);
    return true;
}

__device__ __forceinline__ bool in_polygon(const PolyArgs &a, const int4 *s_edges, uint32_t edge_count, uint32_t base_parity, int32_t x, int32_t y, int32_t z)
{
    if (z < a.z_min || z > a.z_max) return false;
    uint32_t parity = 0;
    if (x >= a.x0 && x <= a.x1 && y >= a.y0 && y <= a.y1) {
        parity = base_parity;
        for (uint32_t k = 0; k < edge_count; ++k) {
            const int4 e = s_edges[k];                                      // l.x, l.y, dx, dy
            const uint32_t t = (uint32_t)y - (uint32_t)e.y;                 // y - l.y: below dy iff l.y <= y < u.y
            const int64_t lhs = (int64_t)(int32_t)((uint32_t)x - (uint32_t)e.x) * (int64_t)e.w;
            const int64_t rhs = (int64_t)(int32_t)t * (int64_t)e.z;
            parity ^= (t < (uint32_t)e.w && lhs < rhs) ? 1u : 0u;
        }
    }
    return parity != a.invert;
}

// Workgroup x takes the straddling batch a.batches[x]: chain_counts[x * 1024 + chain] = its points selected, totals[x] = their sum
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_polygon_count(StreamView s, PolyArgs a, uint32_t *chain_counts, uint32_t *totals)
{
    const PolyBatch pb = a.batches[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // the table, then a.lds_edges edges
    __shared__ uint32_t s_part[LWC_WAVES];
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    int4 *s_edges = reinterpret_cast<int4 *>(s_dyn + POLY_TABLE_BYTES);
    if (!load_polygon_batch(s, a, pb, s_table, s_edges)) return;
    uint32_t cnt = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, pb.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        cnt += in_polygon(a, s_edges, pb.edge_count, pb.base_parity, x, y, z) ? 1u : 0u;
    });
    chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid] = cnt;
    uint32_t sum = cnt;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w];
        totals[blockIdx.x] = t;
    }
}

// Workgroup x takes the straddling batch a.batches[x]: its selected records go to out[offsets[x] ..] as k_select_write's do.
// chain_counts is k_polygon_count's, for the same batches, edges and arguments.
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_polygon_write(StreamView s, PolyArgs a, const uint32_t *chain_counts, const int64_t *offsets, uint4 *out)
{
    const PolyBatch pb = a.batches[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // the table, then a.lds_edges edges
    __shared__ uint32_t s_part[LWC_WAVES];
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    int4 *s_edges = reinterpret_cast<int4 *>(s_dyn + POLY_TABLE_BYTES);
    const uint32_t mine = chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid];
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    if (!load_polygon_batch(s, a, pb, s_table, s_edges)) return;            // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    uint4 *dst = out + offsets[blockIdx.x] + before;
    uint4 *const end = dst + mine;                          // never past what k_polygon_count counted for this chain
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, pb.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        if (in_polygon(a, s_edges, pb.edge_count, pb.base_parity, x, y, z) && dst < end) *dst++ = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
    });
}

// ------------------------------------------------------------------------------------------------
// Slabs (pcr_plane_support, pcr_select_slabs): lo <= n.p <= hi in exact 64-bit integers, for the batches whose exact box a slab
// cuts. The host (pcr_plane.h) gives every such batch its own slices of slab arrays; the workgroup copies them into LDS beside
// the table as 32-byte entries (n[3], a word, lo, hi), launch-sized to the largest slices listed. Per point and entry all lanes
// read the same entry (two ds_read_b128 that broadcast), three 32 x 32 -> 64 multiply-adds, two 64-bit compares.
//   k_slab_count / k_slab_write   k_select_count / k_select_write with "inside the clip and in all of the slice" as the test
//   k_plane_support               counts, per hypothesis of the batch's slice, the candidates in it: a wave-wide vote per
//                                 hypothesis, its population count added by one lane into the wave's own row of 32-bit LDS
//                                 counters (a zero vote adds nothing; a wave without a candidate skips the slice); after the
//                                 chain the rows are summed, one 64-bit global atomic add per non-zero hypothesis. Sums commute,
//                                 so the counts do not depend on the order of lanes, workgroups or launches.
// ------------------------------------------------------------------------------------------------
struct SlabBatch { uint32_t b, first, count, invert; };             // a straddling batch and its slice of the slab array
struct SlabArgs {
    pcr_box clip;
    uint32_t lds_slabs;             // slabs the launch's dynamic LDS holds behind the table: the largest slice listed
    const SlabBatch *batches;
    const pcr_slab *slabs;
};
struct PlaneBatch { uint32_t b, excl_first, excl_count, hyp_first, hyp_count; };    // a decoded batch and its two slices
struct PlaneArgs {
    pcr_box clip;
    uint32_t lds_excl, lds_hyp;     // entries the launch's dynamic LDS holds: table, lds_excl slabs, lds_hyp slabs, LWC_WAVES rows of lds_hyp counters
    const PlaneBatch *batches;
    const pcr_slab *excl, *hyp;     // the slices, back to back; a hypothesis carries its index in `reserved`
    unsigned long long *counts;     // [num_hyp], cleared by the host
    uint32_t *candidates;           // [decoded batches]
};
constexpr uint32_t SLAB_TABLE_BYTES = PCR_HUFFMAN_TABLE_SIZE * 4;

// entry k of a slice in LDS against one point
__device__ __forceinline__ bool in_slab(const int4 *s_slabs, uint32_t k, int32_t x, int32_t y, int32_t z)
{
    const int4 n = s_slabs[2 * k], w = s_slabs[2 * k + 1];                  // n0 n1 n2 word, lo, hi
    const int64_t v = (int64_t)n.x * x + (int64_t)n.y * y + (int64_t)n.z * z;
    const int64_t lo = (int64_t)(((uint64_t)(uint32_t)w.y << 32) | (uint32_t)w.x), hi = (int64_t)(((uint64_t)(uint32_t)w.w << 32) | (uint32_t)w.z);
    return v >= lo && v <= hi;
}

// `count` slabs from src[first ..] into LDS (no barrier)
__device__ __forceinline__ void load_slab_slice(const pcr_slab *src, uint32_t first, uint32_t count, int4 *s_slabs)
{
    const int4 *from = reinterpret_cast<const int4 *>(src + first);
    for (uint32_t i = threadIdx.x; i < 2u * count; i += PCR_WORKGROUP_SIZE) s_slabs[i] = from[i];
}

__device__ __forceinline__ bool in_slabs(const SlabArgs &a, const int4 *s_slabs, uint32_t count, uint32_t invert, int32_t x, int32_t y, int32_t z)
{
    if (!in_box(a.clip, x, y, z)) return false;
    bool all = true;
    for (uint32_t k = 0; k < count; ++k) all = all && in_slab(s_slabs, k, x, y, z);
    return all != (invert != 0u);
}

// Workgroup x takes the straddling batch a.batches[x]: chain_counts[x * 1024 + chain] = its points selected, totals[x] = their sum
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_slab_count(StreamView s, SlabArgs a, uint32_t *chain_counts, uint32_t *totals)
{
    const SlabBatch sb = a.batches[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // the table, then a.lds_slabs slabs
    __shared__ uint32_t s_part[LWC_WAVES];
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    int4 *s_slabs = reinterpret_cast<int4 *>(s_dyn + SLAB_TABLE_BYTES);
    if (sb.count > a.lds_slabs) return;                                     // (uniform; the host never lists such a slice)
    load_slab_slice(a.slabs, sb.first, sb.count, s_slabs);
    load_packed_table(s, sb.b, s_table);
    uint32_t cnt = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, sb.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        cnt += in_slabs(a, s_slabs, sb.count, sb.invert, x, y, z) ? 1u : 0u;
    });
    chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid] = cnt;
    uint32_t sum = cnt;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w];
        totals[blockIdx.x] = t;
    }
}

// Workgroup x takes the straddling batch a.batches[x]: its selected records go to out[offsets[x] ..] as k_select_write's do.
// chain_counts is k_slab_count's, for the same batches, slabs and arguments.
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_slab_write(StreamView s, SlabArgs a, const uint32_t *chain_counts, const int64_t *offsets, uint4 *out)
{
    const SlabBatch sb = a.batches[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // the table, then a.lds_slabs slabs
    __shared__ uint32_t s_part[LWC_WAVES];
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    int4 *s_slabs = reinterpret_cast<int4 *>(s_dyn + SLAB_TABLE_BYTES);
    if (sb.count > a.lds_slabs) return;
    const uint32_t mine = chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid];
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_slab_slice(a.slabs, sb.first, sb.count, s_slabs);
    load_packed_table(s, sb.b, s_table);                    // (its barrier publishes s_part and the slice as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    uint4 *dst = out + offsets[blockIdx.x] + before;
    uint4 *const end = dst + mine;                          // never past what k_slab_count counted for this chain
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, sb.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        if (in_slabs(a, s_slabs, sb.count, sb.invert, x, y, z) && dst < end) *dst++ = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
    });
}

// Workgroup x takes the decoded batch a.batches[x]: a.candidates[x] = its records inside the clip and in no slab of its exclusion
// slice; a.counts[j] += those of them in hypothesis j, for every j of its hypothesis slice. decode_chain calls the sink uniformly
// over the workgroup, so the votes see whole waves.
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_plane_support(StreamView s, PlaneArgs a)
{
    const PlaneBatch pb = a.batches[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ uint32_t s_part[LWC_WAVES];
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    int4 *s_excl = reinterpret_cast<int4 *>(s_dyn + SLAB_TABLE_BYTES);
    int4 *s_hyp = s_excl + 2u * a.lds_excl;
    uint32_t *s_rows = reinterpret_cast<uint32_t *>(s_hyp + 2u * a.lds_hyp);    // [LWC_WAVES][a.lds_hyp]
    if (pb.excl_count > a.lds_excl || pb.hyp_count > a.lds_hyp) return;         // (uniform; the host never lists such slices)
    load_slab_slice(a.excl, pb.excl_first, pb.excl_count, s_excl);
    load_slab_slice(a.hyp, pb.hyp_first, pb.hyp_count, s_hyp);
    for (uint32_t i = tid; i < (uint32_t)LWC_WAVES * a.lds_hyp; i += PCR_WORKGROUP_SIZE) s_rows[i] = 0u;
    load_packed_table(s, pb.b, s_table);                    // (its barrier publishes the slices and the cleared rows as well)
    uint32_t *const row = s_rows + wave * a.lds_hyp;
    uint32_t cand = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, pb.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        bool c = in_box(a.clip, x, y, z);
        for (uint32_t k = 0; k < pb.excl_count; ++k) c = c && !in_slab(s_excl, k, x, y, z);
        cand += c ? 1u : 0u;
        if (__ballot(c) == 0ull) return;
        for (uint32_t k = 0; k < pb.hyp_count; ++k) {
            const uint64_t vote = __ballot(c && in_slab(s_hyp, k, x, y, z));
            if (vote != 0ull && lane == 0u) row[k] += (uint32_t)__popcll(vote);     // the wave's own row: no other wave touches it
        }
    });
    uint32_t sum = cand;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    for (uint32_t k = tid; k < pb.hyp_count; k += PCR_WORKGROUP_SIZE) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_rows[(uint32_t)w * a.lds_hyp + k];
        if (t) atomicAdd(&a.counts[(uint32_t)s_hyp[2 * k].w], (unsigned long long)t);
    }
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w];
        a.candidates[blockIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// Top-down grid (pcr_grid_clear / pcr_grid_accumulate / pcr_grid_unpack): the stream rasterized into planes over its integer x
// and y -- per cell the unsigned max and min of (z ^ sign bit) << 32 | colour and the number of points (pcr_grid in
// pcr_types.h). k_render's window scheme with an integer orthographic projection: the host knows every batch's exact box, hence
// the rectangle of cells the batch can reach, and lists the batch with it.
//   k_grid<.., true>   windowed: the rectangle has at most PCR_GRID_WINDOW_CELLS cells. The workgroup keeps the planes asked for
//                      in LDS beside the table (8 + 8 + 4 bytes per cell of the launch's largest window, so a top-only call
//                      fits several workgroups per CU), accumulates with LDS atomics that return nothing, and after a barrier
//                      merges: one global atomic per non-empty cell and plane, rows of the rectangle contiguous.
//   k_grid<.., false>  direct: a global atomic per point and plane.
// Max, min and add commute, so the planes do not depend on the order of points, workgroups or launches. No workgroup waits for
// another one; every result goes out through vector atomics and stores.
// ------------------------------------------------------------------------------------------------
struct GridEntry { uint32_t b, wx0, wy0, ww, wh; };     // a listed batch and its window: first cell and size in cells
struct GridArgs {
    pcr_box q;                      // grid and clip intersected, in the stream's coordinates, not empty: a point inside has a cell
    int32_t ox, oy;                 // pcr_grid::origin_x / origin_y
    CellDiv div;                    // pcr_grid::cell as a divisor (pcr_lattice.h)
    uint32_t width;
    uint32_t win_cells;             // cells of each LDS plane of this launch (windowed): the largest window listed
    unsigned long long *top, *bottom;
    uint32_t *count;
};
constexpr uint32_t GRID_TABLE_BYTES = PCR_HUFFMAN_TABLE_SIZE * 4;

// d / cell, exact for every 32-bit d. With m = ceil(2^64 / c) and c no power of two, m * c = 2^64 + e with 0 < e < c, so
// d * m / 2^64 = d / c + d * e / (c * 2^64), and the excess is below 2^32 * c / (c * 2^64) = 2^-32 <= 1 / c: too little to
// carry the fraction of d / c (at most 1 - 1 / c) over the next integer.
__device__ __forceinline__ uint32_t grid_div(const CellDiv &c, uint32_t d)
{
    return c.shift < CELL_NO_SHIFT ? d >> c.shift : (uint32_t)__umul64hi((unsigned long long)d, c.magic);
}

template <int LAYOUT, int COLOUR, bool WINDOWED>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_grid(StreamView s, const GridEntry *list, GridArgs a)
{
    typedef unsigned long long u64;
    const GridEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // the table, then the planes asked for
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    u64 *s_top = reinterpret_cast<u64 *>(s_dyn + GRID_TABLE_BYTES);
    u64 *s_bottom = s_top + (a.top ? a.win_cells : 0u);
    uint32_t *s_count = reinterpret_cast<uint32_t *>(s_bottom + (a.bottom ? a.win_cells : 0u));
    const uint32_t ncell = e.ww * e.wh;
    if (WINDOWED) {
        if (ncell > a.win_cells) return;                                    // (uniform; the host lists no such window)
        for (uint32_t i = tid; i < ncell; i += PCR_WORKGROUP_SIZE) {
            if (a.top) s_top[i] = 0ull;
            if (a.bottom) s_bottom[i] = ~0ull;
            if (a.count) s_count[i] = 0u;
        }
    }
    load_packed_table(s, e.b, s_table);                                     // (its barrier publishes the window as well)
    decode_chain<LAYOUT, COLOUR>(s, e.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        if (!in_box(a.q, x, y, z)) return;
        const uint32_t cx = grid_div(a.div, (uint32_t)x - (uint32_t)a.ox), cy = grid_div(a.div, (uint32_t)y - (uint32_t)a.oy);
        const u64 key = ((u64)((uint32_t)z ^ 0x80000000u) << 32) | colour;
        if (WINDOWED) {
            const uint32_t lx = cx - e.wx0, ly = cy - e.wy0;
            if (lx >= e.ww || ly >= e.wh) return;                           // (no point of the batch: the window is its exact box's)
            const uint32_t i = ly * e.ww + lx;
            if (a.top) __hip_atomic_fetch_max(&s_top[i], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (a.bottom) __hip_atomic_fetch_min(&s_bottom[i], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (a.count) __hip_atomic_fetch_add(&s_count[i], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            const size_t g = (size_t)cy * a.width + cx;
            if (a.top) atomicMax(&a.top[g], key);
            if (a.bottom) atomicMin(&a.bottom[g], key);
            if (a.count) atomicAdd(&a.count[g], 1u);
        }
    });
    if (WINDOWED) {
        __syncthreads();
        // row by row: consecutive lanes take consecutive cells of a row of the rectangle, a handful of cache lines per wave; the
        // empty values are the identities of max and min, so a cell no point reached issues nothing
        for (uint32_t i = tid; i < ncell; i += PCR_WORKGROUP_SIZE) {
            const uint32_t ly = i / e.ww, lx = i - ly * e.ww;
            const size_t g = (size_t)(e.wy0 + ly) * a.width + e.wx0 + lx;
            if (a.top) { const u64 v = s_top[i]; if (v != 0ull) atomicMax(&a.top[g], v); }
            if (a.bottom) { const u64 v = s_bottom[i]; if (v != ~0ull) atomicMin(&a.bottom[g], v); }
            if (a.count) { const uint32_t v = s_count[i]; if (v) atomicAdd(&a.count[g], v); }
        }
    }
}

__global__ void __launch_bounds__(256) k_grid_clear(unsigned long long *top, unsigned long long *bottom, uint32_t *count, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (top) top[i] = 0ull;
        if (bottom) bottom[i] = ~0ull;
        if (count) count[i] = 0u;
    }
}

// height / rgba of every cell of a top or bottom plane (`empty`: the plane's empty value; either output may be NULL)
__global__ void __launch_bounds__(256) k_grid_unpack(const unsigned long long *words, unsigned long long empty, int32_t *height, uint32_t *rgba, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long w = words[i];
        if (height) height[i] = w == empty ? INT32_MIN : (int32_t)((uint32_t)(w >> 32) ^ 0x80000000u);
        if (rgba) rgba[i] = w == empty ? 0u : ((uint32_t)w | 0xFF000000u);
    }
}

// ------------------------------------------------------------------------------------------------
// Height percentiles per cell (pcr_grid_quantiles): the z of every candidate bucketed by cell, then an exact selection per cell.
// A candidate is a record inside grid and clip whose z is at least its cell's floor (no floor plane: every record). The host
// lists the batches as for k_grid (GridEntry, windowed ones first). One launch each, windowed and direct batches apart:
//   k_quant_count   colourless decode: count[cell] += 1 per candidate. Windowed: LDS adds in a window beside the table, then one
//                   global add per non-empty cell; direct: one global add per candidate.
//   k_quant_alloc   a thread per cell, k_neighbors_alloc's scheme with the cursors taken once per workgroup (a grid of 2^26 cells
//                   has 2^20 waves: an atomic each on one word measured 11 ms per 10^7 cells): an occupied cell takes its
//                   segment [start, start + n) of the value array from one cursor and its entry in the work list from another.
//                   Cells of at most 64 candidates are listed from the front, larger ones from the back, so each select
//                   launch is uniform. An empty cell gets INT32_MIN in every plane. The cursors are the call's statistics: candidates,
//                   occupied cells (both lists), and the largest n by an atomic max.
//   k_quant_fill    colourless decode again: (uint32)z ^ 0x80000000 of every candidate into its cell's segment. Windowed: the
//                   workgroup decodes its batch twice. The first decode counts per window cell in LDS; after a barrier one
//                   global atomic per non-empty window cell reserves the batch's share of the cell's segment and leaves its
//                   base and end in LDS; after a second barrier the second decode takes a slot with an LDS add that returns.
//                   One global atomic per cell and batch, not per candidate. Direct: one global atomic per candidate.
//   k_quant_select_small   n <= 64: a wave per cell, lane i holds value i; its rank is the number of lanes j with v_j < v_i or
//                   (v_j == v_i and j < i), taken with n wave-uniform lane reads -- no LDS, no barrier. The ranks are a
//                   permutation of 0 .. n - 1, so for every q exactly one lane stores. Cells of at most 4 candidates (a fine
//                   grid has little else) take a lane each instead: four values sorted in registers.
//   k_quant_select_large   n > 64: a 256-thread workgroup per cell, an MSB-first radix select with 8-bit digits over a 256-bin
//                   LDS histogram. The first pass's histogram serves every rank; the three later passes run per distinct
//                   rank. A cell of m candidates is read 1 + 3 * (distinct ranks) <= 1 + 3 * num_q times by one workgroup: a
//                   grid that puts the whole stream into one cell is slow, not wrong (max_cell_points tells).
// An order statistic of a multiset does not depend on the order of its elements, so which segment lies where and which slot a
// candidate takes is unobservable. No workgroup waits for another one; every loop is bounded by n, the cells or the list; every
// store into the value array or the list is tested against the end of its segment and of the array (a miss sets the error
// word, which the host reads).
// ------------------------------------------------------------------------------------------------
enum { QUANT_VALUES = 0, QUANT_SMALL, QUANT_LARGE, QUANT_MAX_CELL, QUANT_ERROR, QUANT_COUNTERS = 8 };
constexpr uint32_t QUANT_SMALL_MAX = 64, QUANT_TINY_MAX = 4;
struct QuantArgs {
    pcr_box q;                      // grid and clip intersected, not empty (GridArgs::q)
    int32_t ox, oy;
    CellDiv div;
    uint32_t width, cells;
    uint32_t win_cells;             // cells of each LDS array of a windowed launch: the largest window listed
    const int32_t *floor;           // [cells] or NULL: a candidate has z >= floor[cell]
    uint32_t *count;                // [cells] candidates per cell
    uint2 *seg;                     // [cells] x: the first entry of the cell's segment, y: entries reserved (k_quant_fill)
    uint32_t *values;               // [candidates] (uint32)z ^ 0x80000000, bucketed by cell
    uint32_t candidates;
    uint32_t *list;                 // [list_capacity] cells with 1 .. 64 candidates from the front, larger ones from the back
    uint32_t list_capacity;
    int32_t *planes;                // [num_q][cells] or NULL (count only: nothing but count and the counters is written)
    uint32_t num_q;
    uint32_t qv[PCR_QUANTILES_MAX]; // basis points
    uint32_t *counters;             // [QUANT_COUNTERS]
};

__device__ __forceinline__ bool quant_cell(const QuantArgs &a, int32_t x, int32_t y, int32_t z, uint32_t &cx, uint32_t &cy)
{
    if (!in_box(a.q, x, y, z)) return false;
    cx = grid_div(a.div, (uint32_t)x - (uint32_t)a.ox); cy = grid_div(a.div, (uint32_t)y - (uint32_t)a.oy);
    return !a.floor || z >= a.floor[(size_t)cy * a.width + cx];
}

template <int LAYOUT, bool WINDOWED>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_quant_count(StreamView s, const GridEntry *list, QuantArgs a)
{
    const GridEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // the table, then the window's counts
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    uint32_t *s_count = reinterpret_cast<uint32_t *>(s_dyn + GRID_TABLE_BYTES);
    const uint32_t ncell = e.ww * e.wh;
    if (WINDOWED) {
        if (ncell > a.win_cells) return;                                    // (uniform; the host lists no such window)
        for (uint32_t i = tid; i < ncell; i += PCR_WORKGROUP_SIZE) s_count[i] = 0u;
    }
    load_packed_table(s, e.b, s_table);                                     // (its barrier publishes the window as well)
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, e.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t cx, cy;
        if (!quant_cell(a, x, y, z, cx, cy)) return;
        if (WINDOWED) {
            const uint32_t lx = cx - e.wx0, ly = cy - e.wy0;
            if (lx >= e.ww || ly >= e.wh) return;                           // (no point of the batch: the window is its exact box's)
            __hip_atomic_fetch_add(&s_count[ly * e.ww + lx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            atomicAdd(&a.count[(size_t)cy * a.width + cx], 1u);
        }
    });
    if (WINDOWED) {
        __syncthreads();
        for (uint32_t i = tid; i < ncell; i += PCR_WORKGROUP_SIZE) {
            const uint32_t ly = i / e.ww, lx = i - ly * e.ww;
            const uint32_t v = s_count[i];
            if (v) atomicAdd(&a.count[(size_t)(e.wy0 + ly) * a.width + e.wx0 + lx], v);
        }
    }
}

// Workgroup x takes the cells [x * chunk, (x + 1) * chunk) (chunk: a multiple of 256; chunk * gridDim.x >= cells): first their
// totals, with one atomic per cursor and workgroup, then the cells in order with a running prefix -- a wave's prefix by
// shuffles, the waves' totals through LDS.
__global__ void __launch_bounds__(256) k_quant_alloc(QuantArgs a, uint32_t chunk)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ uint32_t s_wave[4][3], s_base[3];
    const uint32_t c0 = blockIdx.x * chunk, c1 = min(a.cells, c0 + chunk);
    if (c0 >= a.cells) return;                                              // (uniform)
    uint32_t total[3] = {0, 0, 0}, largest = 0;
    for (uint32_t i = c0 + tid; i < c1; i += 256u) {
        const uint32_t n = a.count[i];
        total[0] += n; total[1] += n >= 1u && n <= QUANT_SMALL_MAX ? 1u : 0u; total[2] += n > QUANT_SMALL_MAX ? 1u : 0u;
        largest = max(largest, n);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) total[k] += __shfl_xor(total[k], d, 64);
        largest = max(largest, (uint32_t)__shfl_xor(largest, d, 64));
    }
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) s_wave[wave][k] = total[k];
        if (largest) atomicMax(&a.counters[QUANT_MAX_CELL], largest);
    }
    __syncthreads();
    if (tid < 3u) {
        const uint32_t t = s_wave[0][tid] + s_wave[1][tid] + s_wave[2][tid] + s_wave[3][tid];
        s_base[tid] = t ? atomicAdd(&a.counters[QUANT_VALUES + tid], t) : 0u;   // (QUANT_VALUES, QUANT_SMALL, QUANT_LARGE are 0, 1, 2)
    }
    __syncthreads();
    if (!a.planes) return;                                                  // (uniform) count only: the cursors and the maximum are all there is
    uint32_t run[3] = {s_base[0], s_base[1], s_base[2]};
    for (uint32_t base = c0; base < c1; base += 256u) {                     // (every thread makes the same rounds)
        __syncthreads();                                                    // (the round before has read s_wave)
        const uint32_t i = base + tid;
        const uint32_t n = i < c1 ? a.count[i] : 0u;
        const uint32_t own[3] = {n, n >= 1u && n <= QUANT_SMALL_MAX ? 1u : 0u, n > QUANT_SMALL_MAX ? 1u : 0u};
        uint32_t incl[3] = {own[0], own[1], own[2]};                        // inclusive prefixes over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t u = __shfl_up(incl[k], d, 64);
                if (lane >= (uint32_t)d) incl[k] += u;
            }
        }
        if (lane == 63u) for (int k = 0; k < 3; ++k) s_wave[wave][k] = incl[k];
        __syncthreads();
        uint32_t at[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint32_t before = 0, all = 0;
#pragma unroll
            for (uint32_t w = 0; w < 4u; ++w) { const uint32_t t = s_wave[w][k]; all += t; before += w < wave ? t : 0u; }
            at[k] = run[k] + before + incl[k] - own[k];
            run[k] += all;
        }
        if (i < c1) {
            if (n == 0u) {
                for (uint32_t j = 0; j < a.num_q; ++j) a.planes[(size_t)j * a.cells + i] = INT32_MIN;
            } else {
                a.seg[i] = make_uint2(at[0], 0u);
                const uint32_t slot = own[1] ? at[1] : a.list_capacity - 1u - at[2];
                if (slot < a.list_capacity) a.list[slot] = i;
                else a.counters[QUANT_ERROR] = 1u;
            }
        }
    }
}

template <int LAYOUT, bool WINDOWED>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_quant_fill(StreamView s, const GridEntry *list, QuantArgs a)
{
    const GridEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    extern __shared__ __align__(16) unsigned char s_dyn[];                  // the table, then per window cell the next slot and the end
    uint32_t *s_table = reinterpret_cast<uint32_t *>(s_dyn);
    uint32_t *s_next = reinterpret_cast<uint32_t *>(s_dyn + GRID_TABLE_BYTES);
    uint32_t *s_end = s_next + a.win_cells;
    const uint32_t ncell = e.ww * e.wh;
    if (WINDOWED) {
        if (ncell > a.win_cells) return;                                    // (uniform; the host lists no such window)
        for (uint32_t i = tid; i < ncell; i += PCR_WORKGROUP_SIZE) s_next[i] = 0u;
    }
    load_packed_table(s, e.b, s_table);                                     // (its barrier publishes the window as well)
    if (WINDOWED) {
        decode_chain<LAYOUT, SEL_NO_COLOUR>(s, e.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
            uint32_t cx, cy;
            if (!quant_cell(a, x, y, z, cx, cy)) return;
            const uint32_t lx = cx - e.wx0, ly = cy - e.wy0;
            if (lx >= e.ww || ly >= e.wh) return;
            __hip_atomic_fetch_add(&s_next[ly * e.ww + lx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
        __syncthreads();
        // the batch's share of every cell it reaches: [first, first + n) of the cell's segment, never past what k_quant_count
        // counted for the cell nor past the array
        for (uint32_t i = tid; i < ncell; i += PCR_WORKGROUP_SIZE) {
            const uint32_t n = s_next[i];
            uint32_t first = 0, end = 0;
            if (n) {
                const uint32_t ly = i / e.ww, lx = i - ly * e.ww;
                const size_t g = (size_t)(e.wy0 + ly) * a.width + e.wx0 + lx;
                const unsigned long long taken = atomicAdd(&a.seg[g].y, n);
                const unsigned long long at = (unsigned long long)a.seg[g].x + taken;
                if (taken + n <= a.count[g] && at + n <= a.candidates) { first = (uint32_t)at; end = first + n; }
                else a.counters[QUANT_ERROR] = 1u;
            }
            s_next[i] = first; s_end[i] = end;
        }
        __syncthreads();
    }
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, e.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t cx, cy;
        if (!quant_cell(a, x, y, z, cx, cy)) return;
        const uint32_t value = (uint32_t)z ^ 0x80000000u;
        if (WINDOWED) {
            const uint32_t lx = cx - e.wx0, ly = cy - e.wy0;
            if (lx >= e.ww || ly >= e.wh) return;
            const uint32_t i = ly * e.ww + lx;
            const uint32_t at = __hip_atomic_fetch_add(&s_next[i], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (at < s_end[i]) a.values[at] = value;
            else a.counters[QUANT_ERROR] = 1u;
        } else {
            const size_t g = (size_t)cy * a.width + cx;
            const uint32_t taken = atomicAdd(&a.seg[g].y, 1u);
            const unsigned long long at = (unsigned long long)a.seg[g].x + taken;
            if (taken < a.count[g] && at < a.candidates) a.values[at] = value;
            else a.counters[QUANT_ERROR] = 1u;
        }
    });
}

// The segment of listed cell `cell` (uniform over the caller's wave or workgroup): false, with the error word set, unless it is
// full and inside the array
__device__ __forceinline__ bool quant_segment(const QuantArgs &a, uint32_t cell, uint32_t &start, uint32_t &n)
{
    const uint2 sg = a.seg[cell];
    start = sg.x; n = a.count[cell];
    if (cell < a.cells && n >= 1u && sg.y == n && (unsigned long long)start + n <= a.candidates) return true;
    a.counters[QUANT_ERROR] = 1u;
    return false;
}

__device__ __forceinline__ void quant_order(uint32_t &lo, uint32_t &hi)
{
    const uint32_t a = min(lo, hi), b = max(lo, hi);
    lo = a; hi = b;
}

// A wave takes 64 listed cells at a time. A cell of at most QUANT_TINY_MAX candidates is one lane's: its values sorted in
// registers by a network. The others go one after the other through the whole wave, lane i holding value i.
__global__ void __launch_bounds__(256) k_quant_select_small(QuantArgs a, uint32_t items)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6), waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w0 = wave * 64u; w0 < items; w0 += waves * 64u) {
        uint32_t cell = 0, start = 0, n = 0;
        if (w0 + lane < items) {
            cell = min(a.list[w0 + lane], a.cells - 1u);
            if (!quant_segment(a, cell, start, n)) n = 0u;
            n = min(n, QUANT_SMALL_MAX);
        }
        if (n >= 1u && n <= QUANT_TINY_MAX) {
            uint32_t v0 = a.values[start], v1 = n > 1u ? a.values[start + 1u] : 0xFFFFFFFFu;
            uint32_t v2 = n > 2u ? a.values[start + 2u] : 0xFFFFFFFFu, v3 = n > 3u ? a.values[start + 3u] : 0xFFFFFFFFu;
            quant_order(v0, v1); quant_order(v2, v3); quant_order(v0, v2); quant_order(v1, v3); quant_order(v1, v2);
            for (uint32_t k = 0; k < a.num_q; ++k) {
                const uint32_t r = (uint32_t)quantile_rank(a.qv[k], n);
                a.planes[(size_t)k * a.cells + cell] = (int32_t)((r == 0u ? v0 : r == 1u ? v1 : r == 2u ? v2 : v3) ^ 0x80000000u);
            }
        }
        unsigned long long todo = __ballot(n > QUANT_TINY_MAX);
        while (todo) {                                                      // (uniform: at most 64 rounds)
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cell, l), first = (uint32_t)__builtin_amdgcn_readlane((int)start, l);
            const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)n, l);
            const uint32_t v = lane < m ? a.values[first + lane] : 0xFFFFFFFFu;
            uint32_t rank = 0;
            for (uint32_t j = 0; j < m; ++j) {
                const uint32_t vj = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j);
                rank += vj < v || (vj == v && j < lane) ? 1u : 0u;
            }
            for (uint32_t k = 0; k < a.num_q; ++k)
                if (lane < m && rank == (uint32_t)quantile_rank(a.qv[k], m)) a.planes[(size_t)k * a.cells + c] = (int32_t)(v ^ 0x80000000u);
        }
    }
}

__global__ void __launch_bounds__(256) k_quant_select_large(QuantArgs a, uint32_t items)
{
    const uint32_t tid = threadIdx.x;
    __shared__ uint32_t s_first[256], s_hist[256], s_pick[2], s_result[PCR_QUANTILES_MAX];
    for (uint32_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint32_t cell = min(a.list[a.list_capacity - 1u - w], a.cells - 1u);
        uint32_t start, n;
        if (!quant_segment(a, cell, start, n)) continue;                    // (uniform: every thread read the same words)
        const uint32_t *v = a.values + start;
        s_first[tid] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += 256u) __hip_atomic_fetch_add(&s_first[v[i] >> 24], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        for (uint32_t j = 0; j < a.num_q; ++j) {
            uint32_t k = (uint32_t)quantile_rank(a.qv[j], n);
            int same = -1;                                                  // an earlier q with this rank: its result is this one's
            for (uint32_t jj = 0; jj < j; ++jj) if ((uint32_t)quantile_rank(a.qv[jj], n) == k) same = (int)jj;
            if (same >= 0) { if (tid == 0) s_result[j] = s_result[same]; continue; }
            uint32_t prefix = 0;                                            // the digits found so far, in place
            for (int pass = 0; pass < 4; ++pass) {
                const uint32_t shift = 24u - 8u * (uint32_t)pass;
                const uint32_t *hist = pass == 0 ? s_first : s_hist;
                if (pass) {
                    s_hist[tid] = 0u;
                    __syncthreads();
                    for (uint32_t i = tid; i < n; i += 256u) {
                        const uint32_t x = v[i];
                        if ((x >> (shift + 8u)) == (prefix >> (shift + 8u)))
                            __hip_atomic_fetch_add(&s_hist[(x >> shift) & 255u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    __syncthreads();
                }
                // the bin that holds rank k among the values that share the prefix: the first wave, four bins a lane
                if (tid < 64u) {
                    uint32_t c[4], sum = 0;
#pragma unroll
                    for (int d = 0; d < 4; ++d) { c[d] = hist[tid * 4u + (uint32_t)d]; sum += c[d]; }
                    uint32_t incl = sum;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t u = __shfl_up(incl, d, 64);
                        if (tid >= (uint32_t)d) incl += u;
                    }
                    const uint32_t excl = incl - sum;
                    if (excl <= k && k < incl) {
                        uint32_t r = k - excl, d = 0;
#pragma unroll
                        for (uint32_t t = 0; t < 3u; ++t) if (d == t && r >= c[t]) { r -= c[t]; d = t + 1u; }   // (r < sum: d ends on a bin that holds it)
                        s_pick[0] = tid * 4u + d; s_pick[1] = r;
                    }
                }
                __syncthreads();
                prefix |= s_pick[0] << shift; k = s_pick[1];
                __syncthreads();                                            // (before the next pass overwrites s_pick and s_hist)
            }
            if (tid == 0) s_result[j] = prefix;
        }
        __syncthreads();
        if (tid < a.num_q) a.planes[(size_t)tid * a.cells + cell] = (int32_t)(s_result[tid] ^ 0x80000000u);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// Ground filter (pcr_ground_filter): a progressive morphological filter over an int32 height plane, then a hole fill. The planes
// in global memory are int32 with INT32_MIN for "empty"; no legal height has that value, and a minimum or maximum over non-empty
// heights never produces it. Inside a kernel an empty cell is never compared as a height: k_ground_morph widens every cell to
// 64 bits and gives the empty ones the identity of the pass (beyond every int32), k_ground_fill tests the flag value first.
//   k_ground_morph  one separable pass of one step: minimum or maximum over 2 * r + 1 cells along a row or a column. A workgroup
//                   takes a tile of GM_LINES lines x GM_SPAN outputs, loads it with r cells of halo at both ends into LDS
//                   (8 bytes a cell), and widens the window by doubling: m_2c[i] = op(m_c[i], m_c[i + c]) while 2c <= w, then
//                   out[i] = op(m_c[i], m_c[i + w - c]) -- about log2(w) rounds whatever the radius, each a read of every cell
//                   into registers, a barrier, the write, a barrier. Rows: consecutive lanes along the row. Columns: consecutive
//                   lanes across GM_LINES neighbouring columns, the LDS index transposed to match (no bank conflicts either way).
//   k_ground_flag   per non-empty cell: the drop A - O of the step in 64 bits against the threshold, the flag, A = O.
//   k_ground_class  classes, H (the input height of ground cells, empty otherwise) and the three class counts.
//   k_ground_fill   one Jacobi round from one plane into another: an empty cell with m >= 1 non-empty neighbours of 8 takes
//                   floor(sum / m); counts the cells it filled and the cells still empty.
// Every loop is bounded by the tile; counters go out through one vector atomic per wave.
// ------------------------------------------------------------------------------------------------
constexpr int GM_THREADS = 256;
constexpr int GM_LINES = 16;                                // lines of a tile (rows of a row pass, columns of a column pass)
constexpr int GM_SPAN = 64;                                 // outputs per line of a tile
constexpr int GM_MAX_LL = GM_SPAN + 2 * PCR_GROUND_MAX_RADIUS;      // a line with its halo
constexpr int GM_EPT = GM_LINES * GM_MAX_LL / GM_THREADS;   // cells of the tile per thread
static_assert(GM_LINES * GM_MAX_LL % GM_THREADS == 0, "whole cells per thread");
constexpr long long GM_IDENTITY = 1ll << 40;                // beyond every int32: +GM_IDENTITY for a minimum, -GM_IDENTITY for a maximum

struct GroundMorphArgs {
    const int32_t *src;
    int32_t *dst;
    uint32_t width, height;
    uint32_t radius;                // 1 .. PCR_GROUND_MAX_RADIUS
    uint32_t column;                // 0: along rows, 1: along columns
    uint32_t is_max;                // 0: minimum, 1: maximum
    uint32_t tiles_along;           // tiles along the axis of the pass; blockIdx.x = tile across * tiles_along + tile along
};

__global__ void __launch_bounds__(GM_THREADS) k_ground_morph(GroundMorphArgs a)
{
    __shared__ long long s_m[GM_LINES * GM_MAX_LL];
    const uint32_t tid = threadIdx.x;
    const uint32_t na = a.column ? a.height : a.width, nc = a.column ? a.width : a.height;      // cells along a line, lines
    const size_t sa = a.column ? a.width : 1u, sc = a.column ? 1u : a.width;                    // strides in the plane
    const uint32_t t_along = blockIdx.x % a.tiles_along, t_across = blockIdx.x / a.tiles_along;
    const uint32_t r = min(a.radius, (uint32_t)PCR_GROUND_MAX_RADIUS), w = 2u * r + 1u;
    const uint32_t ll = GM_SPAN + 2u * r, cells = GM_LINES * ll;                                // cells of the tile, <= GM_LINES * GM_MAX_LL
    const uint32_t step = a.column ? GM_LINES : 1u;                                             // LDS distance of neighbours along the line
    const long long identity = a.is_max ? -GM_IDENTITY : GM_IDENTITY;
    const long long a0 = (long long)t_along * GM_SPAN - (long long)r;                           // position along the line of tile cell 0
    const uint32_t c0 = t_across * GM_LINES;

    uint32_t line[GM_EPT], pos[GM_EPT];
#pragma unroll
    for (int j = 0; j < GM_EPT; ++j) {
        const uint32_t e = tid + (uint32_t)j * GM_THREADS;
        line[j] = a.column ? e % GM_LINES : e / ll;
        pos[j] = a.column ? e / GM_LINES : e % ll;
        if (e < cells) {
            const long long p = a0 + pos[j];
            const uint32_t l = c0 + line[j];
            long long v = identity;
            if (p >= 0 && p < (long long)na && l < nc) {
                const int32_t z = a.src[(size_t)p * sa + (size_t)l * sc];
                if (z != INT32_MIN) v = z;
            }
            s_m[e] = v;
        }
    }
    __syncthreads();
    long long v[GM_EPT];
    uint32_t c = 1;
#pragma unroll 1
    for (int round = 0; round < 8 && 2u * c <= w; ++round, c *= 2u) {          // w <= 129: at most 7 doublings
#pragma unroll
        for (int j = 0; j < GM_EPT; ++j) {
            const uint32_t e = tid + (uint32_t)j * GM_THREADS;
            if (e < cells) {
                v[j] = s_m[e];
                if (pos[j] + c < ll) { const long long o = s_m[e + c * step]; v[j] = a.is_max ? max(v[j], o) : min(v[j], o); }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < GM_EPT; ++j) {
            const uint32_t e = tid + (uint32_t)j * GM_THREADS;
            if (e < cells) s_m[e] = v[j];
        }
        __syncthreads();
    }
    const uint32_t d = w - c;                                                  // 0 <= d < c: the two windows of c cells cover w
#pragma unroll
    for (int j = 0; j < GM_EPT; ++j) {
        const uint32_t e = tid + (uint32_t)j * GM_THREADS;
        if (e >= cells || pos[j] >= (uint32_t)GM_SPAN) continue;
        const long long p = (long long)t_along * GM_SPAN + pos[j];
        const uint32_t l = c0 + line[j];
        if (p >= (long long)na || l >= nc) continue;
        const long long x = s_m[e], y = s_m[e + d * step];                     // pos + d <= GM_SPAN - 1 + 2r - ... < ll
        const long long m = a.is_max ? max(x, y) : min(x, y);
        a.dst[(size_t)p * sa + (size_t)l * sc] = m == identity ? INT32_MIN : (int32_t)m;
    }
}

// One 64-bit add per wave of the sum of v over the workgroup's lanes that hold one
__device__ __forceinline__ void ground_count(unsigned long long *counter, uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(counter, (unsigned long long)v);
}

// a_in: the surface before the step (the input plane at step 0), o: its opening, a_out: the surface after it
__global__ void __launch_bounds__(256) k_ground_flag(const int32_t *z0, const int32_t *a_in, const int32_t *o, int32_t *a_out, uint8_t *flag,
                                                     int32_t threshold, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (z0[i] == INT32_MIN) { a_out[i] = INT32_MIN; return; }
    const int32_t av = a_in[i], ov = o[i];
    if ((long long)av - (long long)ov > (long long)threshold) flag[i] = 1;
    a_out[i] = ov;
}

// counters[0..2] += empty, ground, non-ground cells
__global__ void __launch_bounds__(256) k_ground_class(const int32_t *z0, const uint8_t *flag, int32_t *h, uint8_t *cls, unsigned long long *counters, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t k = 3;                                                            // past the grid: no class
    if (i < n) {
        const int32_t z = z0[i];
        k = z == INT32_MIN ? PCR_CELL_EMPTY : flag[i] ? PCR_CELL_NONGROUND : PCR_CELL_GROUND;
        h[i] = k == PCR_CELL_GROUND ? z : INT32_MIN;
        if (cls) cls[i] = (uint8_t)k;
    }
    ground_count(counters + 0, k == PCR_CELL_EMPTY ? 1u : 0u);
    ground_count(counters + 1, k == PCR_CELL_GROUND ? 1u : 0u);
    ground_count(counters + 2, k == PCR_CELL_NONGROUND ? 1u : 0u);
}

// counters[0] += cells filled by this round, counters[1] += cells still empty after it
__global__ void __launch_bounds__(256) k_ground_fill(const int32_t *src, int32_t *dst, uint32_t width, uint32_t height, unsigned long long *counters)
{
    const uint32_t n = width * height;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t filled = 0, left = 0;
    if (i < n) {
        int32_t v = src[i];
        if (v == INT32_MIN) {
            const uint32_t cy = i / width, cx = i - cy * width;
            long long sum = 0;
            int m = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const long long x = (long long)cx + dx, y = (long long)cy + dy;
                    if (x < 0 || y < 0 || x >= (long long)width || y >= (long long)height) continue;
                    const int32_t g = src[(size_t)y * width + (size_t)x];
                    if (g != INT32_MIN) { sum += g; ++m; }
                }
            }
            if (m) {
                long long q = sum / m;
                if (sum % m != 0 && sum < 0) --q;                              // floor: toward minus infinity
                v = (int32_t)q;                                                // a mean of int32 heights above INT32_MIN is one
                filled = 1;
            } else left = 1;
        }
        dst[i] = v;
    }
    ground_count(counters + 0, filled);
    ground_count(counters + 1, left);
}

// ------------------------------------------------------------------------------------------------
// Heights above a ground plane (pcr_select_height): k_select_count / k_select_write with a gather as the predicate. A record
// inside grid and clip intersected (a.q) has a cell -- k_grid's division -- whose ground height g is read from the plane; the
// record is selected iff g is not empty and h_min <= z - g <= h_max in 64 bits. The count pass decodes no colours; the write pass
// decodes them only when records are asked for.
// ------------------------------------------------------------------------------------------------
struct HeightArgs {
    pcr_box q;                      // grid and clip intersected, not empty: a point inside has a cell
    int32_t ox, oy;
    CellDiv div;
    uint32_t width;
    const int32_t *ground;
    int32_t h_min, h_max;
    uint32_t replace_z;
};

// 0: not selected, 1: selected (h set), 2: inside grid and clip on a cell without ground
__device__ __forceinline__ int height_test(const HeightArgs &a, int32_t x, int32_t y, int32_t z, int32_t &h)
{
    if (!in_box(a.q, x, y, z)) return 0;
    const uint32_t cx = grid_div(a.div, (uint32_t)x - (uint32_t)a.ox), cy = grid_div(a.div, (uint32_t)y - (uint32_t)a.oy);
    const int32_t g = a.ground[(size_t)cy * a.width + cx];
    if (g == INT32_MIN) return 2;
    const long long d = (long long)z - (long long)g;
    if (d < (long long)a.h_min || d > (long long)a.h_max) return 0;
    h = (int32_t)d;
    return 1;
}

// Workgroup x takes list[x]: chain_counts[x * 1024 + chain] = the chain's selected points, totals[2x] = their sum, totals[2x + 1] =
// the batch's points on cells without ground
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_height_count(StreamView s, const uint32_t *list, HeightArgs a, uint32_t *chain_counts, uint32_t *totals)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES][2];
    load_packed_table(s, b, s_table);
    uint32_t cnt = 0, bare = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        int32_t h;
        const int t = height_test(a, x, y, z, h);
        cnt += t == 1 ? 1u : 0u; bare += t == 2 ? 1u : 0u;
    });
    chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid] = cnt;
    uint32_t sum = cnt, sum2 = bare;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sum += __shfl_xor(sum, d, 64); sum2 += __shfl_xor(sum2, d, 64); }
    if (lane == 0) { s_part[wave][0] = sum; s_part[wave][1] = sum2; }
    __syncthreads();
    if (tid < 2) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w][tid];
        totals[(size_t)blockIdx.x * 2 + tid] = t;
    }
}

// Workgroup x takes list[x]: its selected records go to points[offsets[x] ..] and their heights to heights[offsets[x] ..] (either
// may be NULL; COLOUR is SEL_NO_COLOUR when points is), chain after chain, each chain's in point order. chain_counts is
// k_height_count's for the same list and arguments.
template <int LAYOUT, int COLOUR>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_height_write(StreamView s, const uint32_t *list, HeightArgs a, const uint32_t *chain_counts,
                                                                     const int64_t *offsets, uint4 *points, int32_t *heights)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const uint32_t mine = chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid];
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_packed_table(s, b, s_table);                       // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    const int64_t first = offsets[blockIdx.x] + before;
    uint32_t k = 0;                                         // never past what k_height_count counted for this chain
    decode_chain<LAYOUT, COLOUR>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        int32_t h;
        if (height_test(a, x, y, z, h) == 1 && k < mine) {
            if (COLOUR != SEL_NO_COLOUR && points) points[first + k] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)(a.replace_z ? h : z), colour);
            if (heights) heights[first + k] = h;
            ++k;
        }
    });
}

// ------------------------------------------------------------------------------------------------
// Voxel-grid thinning (pcr_thin / pcr_read_thin): of the rows of a range inside a clip box, one per voxel of a cubic lattice --
// the lowest row (PCR_THIN_FIRST) or the least by (distance to the voxel's centre, row) (PCR_THIN_CENTER). Four phases, each a
// launch of its own over the batches the clip does not miss (`list`), the sizes in between computed by the host:
//   k_thin_runs    colourless decode: per batch the candidates and the runs -- maximal stretches of consecutive candidates of a
//                  chain with one voxel key. The host sizes the table from their sum.
//   k_thin_mark    colourless decode again: at the end of every run one insertion of (key, the run's best value) into an
//                  open-addressing table in global memory: compare-and-swap on the key, unsigned minimum on the value.
//   k_thin_flag    a thread per slot: the winning row's bit into the keep bitmap (a 64-bit word per chain);
//   k_thin_totals  the kept records of every listed batch.
//   k_thin_write   decode with colour of the batches that keep a record: k_select_write with the chain's keep word as the test.
// The value is the row (FIRST) or d2 << 40 | row (CENTER; d2 < 2^24, row < 2^40), so the minimum decides both orders at once.
// Minimum commutes: the table's content does not depend on the order of lanes, workgroups or launches, and a voxel whose
// candidates are scattered over chains and batches (or come back later in one chain of an unsorted stream) still gets the one
// least value. No workgroup waits for another one; the probe loop makes at most `slots` steps.
// ------------------------------------------------------------------------------------------------
typedef unsigned long long thin_u64;
struct ThinSlot { thin_u64 key, val; };                     // empty: both all ones (a key has 63 bits)
constexpr thin_u64 THIN_EMPTY = ~0ull;
constexpr thin_u64 THIN_ROW_MASK = (1ull << 40) - 1;
constexpr thin_u64 THIN_HASH_MUL = 0x9E3779B97F4A7C15ull;   // odd: key -> key * MUL is a bijection of the 64-bit words

struct ThinArgs {
    pcr_box q;                      // the clip (every int32 point if the call has none)
    ThinLattice lat;                // pcr_lattice.h: for a point inside the call's q, (p - origin) mod 2^32 / cell < 2^21
    uint32_t first_batch;           // row = (b - first_batch) * 65536 + chain * 64 + i
    uint32_t log2_slots;            // >= 10
    ThinSlot *table;
    uint32_t *error;                // set to 1 by a lane that found no slot
};

__device__ __forceinline__ thin_u64 thin_key(const ThinArgs &a, int32_t x, int32_t y, int32_t z, uint32_t &d2)
{
    const uint32_t dx = (uint32_t)x - a.lat.origin[0], dy = (uint32_t)y - a.lat.origin[1], dz = (uint32_t)z - a.lat.origin[2];
    const uint32_t vx = grid_div(a.lat.div, dx), vy = grid_div(a.lat.div, dy), vz = grid_div(a.lat.div, dz);
    // 2 * (offset inside the voxel) - (cell - 1): twice the signed distance to the centre, |.| <= cell - 1
    const int32_t ex = (int32_t)(2u * (dx - vx * a.lat.cell)) - (int32_t)(a.lat.cell - 1u);
    const int32_t ey = (int32_t)(2u * (dy - vy * a.lat.cell)) - (int32_t)(a.lat.cell - 1u);
    const int32_t ez = (int32_t)(2u * (dz - vz * a.lat.cell)) - (int32_t)(a.lat.cell - 1u);
    d2 = (uint32_t)ex * (uint32_t)ex + (uint32_t)ey * (uint32_t)ey + (uint32_t)ez * (uint32_t)ez;   // (only read for cell <= PCR_THIN_MAX_CENTER_CELL)
    return (thin_u64)vx | ((thin_u64)vy << THIN_KEY_BITS) | ((thin_u64)vz << (2 * THIN_KEY_BITS));
}

// Workgroup x takes list[x]: totals[2 x] = its runs, totals[2 x + 1] = its candidates
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_thin_runs(StreamView s, const uint32_t *list, ThinArgs a, uint32_t *totals)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES][2];
    load_packed_table(s, b, s_table);
    uint32_t runs = 0, cand = 0;
    thin_u64 prev = THIN_EMPTY;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t d2;
        const thin_u64 key = in_box(a.q, x, y, z) ? thin_key(a, x, y, z, d2) : THIN_EMPTY;
        cand += key != THIN_EMPTY ? 1u : 0u;
        runs += key != THIN_EMPTY && key != prev ? 1u : 0u;
        prev = key;
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { runs += __shfl_xor(runs, d, 64); cand += __shfl_xor(cand, d, 64); }
    if (lane == 0) { s_part[wave][0] = runs; s_part[wave][1] = cand; }
    __syncthreads();
    if (tid < 2) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w][tid];
        totals[(size_t)blockIdx.x * 2 + tid] = t;
    }
}

// (key, val) into the table: the slot of the key, or the first free one from the key's home on, keeps the least val
__device__ __forceinline__ void thin_insert(const ThinArgs &a, thin_u64 key, thin_u64 val)
{
    const thin_u64 slots = 1ull << a.log2_slots, mask = slots - 1;
    thin_u64 h = (key * THIN_HASH_MUL) >> (64u - a.log2_slots);
    for (thin_u64 probe = 0; probe < slots; ++probe) {
        ThinSlot *slot = a.table + h;
        thin_u64 old = __hip_atomic_load(&slot->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (a taken slot never changes its key)
        if (old == THIN_EMPTY) old = atomicCAS(&slot->key, THIN_EMPTY, key);
        if (old == THIN_EMPTY || old == key) {
            __hip_atomic_fetch_min(&slot->val, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // (the result is not used)
            return;
        }
        h = (h + 1) & mask;
    }
    *a.error = 1u;                                          // every slot holds another key: the host sized the table wrongly
}

template <int LAYOUT, int MODE>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_thin_mark(StreamView s, const uint32_t *list, ThinArgs a)
{
    const uint32_t b = list[blockIdx.x];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    const thin_u64 row0 = (thin_u64)(b - a.first_batch) * PCR_POINTS_PER_BATCH + (thin_u64)threadIdx.x * PCR_POINTS_PER_THREAD;
    thin_u64 prev = THIN_EMPTY, best = THIN_EMPTY;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t d2 = 0;
        const thin_u64 key = in_box(a.q, x, y, z) ? thin_key(a, x, y, z, d2) : THIN_EMPTY;
        const thin_u64 val = MODE == PCR_THIN_CENTER ? ((thin_u64)d2 << 40) | (row0 + (uint32_t)i) : row0 + (uint32_t)i;
        if (key == prev) {
            if (MODE == PCR_THIN_CENTER) best = min(best, val);         // (FIRST: the run's first row is its least)
        } else {
            if (prev != THIN_EMPTY) thin_insert(a, prev, best);
            prev = key; best = val;
        }
    });
    if (prev != THIN_EMPTY) thin_insert(a, prev, best);
}

// keep[row >> 6] |= 1 << (row & 63) for the row of every taken slot (rows: those below `rows`, which is every row of the call)
__global__ void __launch_bounds__(256) k_thin_flag(const ThinSlot *table, thin_u64 slots, thin_u64 rows, thin_u64 *keep)
{
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        if (table[i].key == THIN_EMPTY) continue;
        const thin_u64 row = table[i].val & THIN_ROW_MASK;
        if (row < rows) atomicOr(&keep[row >> 6], 1ull << (row & 63u));
    }
}

// Workgroup x: totals[x] = the bits set in the 1024 keep words of batch list[x]
__global__ void __launch_bounds__(256) k_thin_totals(const uint32_t *list, uint32_t first_batch, const thin_u64 *keep, uint32_t *totals)
{
    const thin_u64 *words = keep + (size_t)(list[blockIdx.x] - first_batch) * PCR_WORKGROUP_SIZE;
    __shared__ uint32_t s_part[4];
    uint32_t sum = 0;
    for (uint32_t i = threadIdx.x; i < PCR_WORKGROUP_SIZE; i += 256) sum += (uint32_t)__popcll(words[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) totals[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// The body of the write kernels. Workgroup x takes list[x], a batch that keeps a record: the flagged records go to
// points[offsets[x] ..] and their rows to rows[offsets[x] ..] (either may be NULL), chain after chain, each chain's in point order;
// extra(dst, row) stores the call's other columns of that record. A lane's keep word is its chain's. k_thin_write and k_knn_write
// are this body; k_neighbors_write and k_moments_write spell it out once more: built on it they come out with other register
// counts and another block order, and these kernels are kept as measured.
template <int LAYOUT, bool BC7, class Extra>
__device__ __forceinline__ void write_kept_rows(const StreamView &s, const uint32_t *list, uint32_t first_batch, const thin_u64 *keep, const int64_t *offsets,
                                                uint4 *points, int64_t *rows, Extra extra)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const thin_u64 word = keep[(size_t)(b - first_batch) * PCR_WORKGROUP_SIZE + tid];
    const uint32_t mine = (uint32_t)__popcll(word);
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_packed_table(s, b, s_table);                       // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    int64_t dst = offsets[blockIdx.x] + before;
    const int64_t end = dst + mine;                         // never past the bits of this chain's word
    const int64_t row0 = (int64_t)(b - first_batch) * PCR_POINTS_PER_BATCH + (int64_t)tid * PCR_POINTS_PER_THREAD;
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        if (((word >> (uint32_t)i) & 1ull) && dst < end) {
            if (points) points[dst] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
            if (rows) rows[dst] = row0 + i;
            extra(dst, row0 + i);
            ++dst;
        }
    });
}

template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_thin_write(StreamView s, const uint32_t *list, uint32_t first_batch, const thin_u64 *keep,
                                                                   const int64_t *offsets, uint4 *points, int64_t *rows)
{
    write_kept_rows<LAYOUT, BC7>(s, list, first_batch, keep, offsets, points, rows, [](int64_t, int64_t) {});
}

// ------------------------------------------------------------------------------------------------
// Levels of detail (pcr_lod_order / pcr_read_lod_order): the candidates of pcr_thin ordered by `levels` nested lattices, level l
// (0 = coarsest) with the cell cell << (levels - 1 - l). level(p) = the least l at which p has the lowest row of its voxel,
// `levels` ("the rest") if at none. k_thin_runs and k_thin_mark<FIRST> (above) fill the finest table on the lattice of lod_lattice
// (pcr_lattice.h); then, the sizes in between computed by the host:
//   k_lod_coarsen  a thread per slot of level l + 1: (parent key, row) of an occupied slot into the table of level l with
//                  thin_insert. The minimum over the children's lowest rows is the lowest row of the parent voxel.
//   k_lod_mark     a thread per slot of a level's table: l into the level byte of the slot's row, and the occupied slots counted
//                  (the host sizes the next table from them; their differences are the level counts). Launched from the finest
//                  level to the coarsest, in stream order: the last store into a row's byte is its least level. The lattices are
//                  nested, so a row that is the lowest of a voxel of level l is the lowest of its voxel of every finer level: the
//                  levels between its least one and the finest stored before it, none is missing.
//   k_lod_count    a workgroup per listed batch: the bytes made final (a candidate whose byte was never stored gets `levels`; a
//                  row outside the clip keeps LOD_NO_LEVEL), the keep word of every chain and the batch's records per level. Only
//                  a batch the clip cuts is decoded (colourless); in any other every row is a candidate.
//   k_lod_write    a workgroup per listed batch, decode with colour: a stable partition of the batch's written records by level.
//                  Per level an exclusive prefix over the 1024 chains' counts (wave shuffles, then the 16 wave sums through LDS)
//                  gives every (chain, level) its first index; the running indices live in LDS as 16-bit words, a column per
//                  lane -- the greatest value a prefix takes is 1023 * 64, the greatest index stored to 65 535 -- and are picked by
//                  the record's level at run time; a register array indexed that way would go to scratch. The chain's 64 level
//                  bytes sit in eight 64-bit registers that move down one place every eight points, so no register is indexed
//                  at run time either.
//   k_lod_rows     PCR_LOD_ROW_ORDER: write_kept_rows with the level byte as the extra column.
// No workgroup waits for another one; the probe loops are thin_insert's.
// ------------------------------------------------------------------------------------------------
struct LodArgs {
    pcr_box q;                      // the clip (every int32 point if the call has none)
    uint32_t first_batch;           // row = (b - first_batch) * 65536 + chain * 64 + i
    uint32_t levels;                // L
    uint32_t classes;               // the levels a call writes: L + 1, or L with PCR_LOD_DROP_REST
    uint8_t *level;                 // [rows of the range]
};
constexpr uint32_t LOD_CUT = 1u << 31;                      // in a list entry: the clip cuts the batch's box
constexpr int LOD_CLASSES = PCR_LOD_MAX_LEVELS + 1;

__global__ void __launch_bounds__(256) k_lod_coarsen(const ThinSlot *src, thin_u64 src_slots, ThinArgs dst)
{
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < src_slots; i += (thin_u64)gridDim.x * blockDim.x) {
        const thin_u64 key = src[i].key;
        if (key != THIN_EMPTY) thin_insert(dst, lod_parent_key(key), src[i].val);
    }
}

__global__ void __launch_bounds__(256) k_lod_mark(const ThinSlot *table, thin_u64 slots, thin_u64 rows, uint32_t l, uint8_t *level, thin_u64 *occupied)
{
    uint32_t n = 0;
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        if (table[i].key == THIN_EMPTY) continue;
        ++n;
        const thin_u64 row = table[i].val & THIN_ROW_MASK;
        if (row < rows) level[row] = (uint8_t)l;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(occupied, (thin_u64)n);
}

// The 64 level bytes of chain `tid` of the batch at `row0`, eight to a word
__device__ __forceinline__ void lod_load_bytes(const uint8_t *level, thin_u64 row0, thin_u64 (&w)[8])
{
    const uint4 *src = reinterpret_cast<const uint4 *>(level + row0);           // (row0 is a multiple of 64, the array 256-byte aligned)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 v = src[k];
        w[2 * k] = (thin_u64)v.x | ((thin_u64)v.y << 32);
        w[2 * k + 1] = (thin_u64)v.z | ((thin_u64)v.w << 32);
    }
}

__device__ __forceinline__ uint32_t lod_count_level(const thin_u64 (&w)[8], uint32_t level)
{
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) n += (uint32_t)__popcll(lod_bytes_equal(w[k], level));
    return n;
}

// Workgroup x takes list[x]: counts[x * (levels + 1) + l] = its records of level l (the rest included, dropped or not)
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_lod_count(StreamView s, const uint32_t *list, LodArgs a, thin_u64 *keep, int64_t *counts)
{
    const uint32_t entry = list[blockIdx.x], b = entry & ~LOD_CUT;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LOD_CLASSES][LWC_WAVES];
    thin_u64 cand = ~0ull;
    if (entry & LOD_CUT) {                                  // (uniform over the workgroup)
        load_packed_table(s, b, s_table);
        cand = 0;
        decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
            cand |= (thin_u64)(in_box(a.q, x, y, z) ? 1u : 0u) << (uint32_t)i;
        });
    }
    const thin_u64 chain = (thin_u64)(b - a.first_batch) * PCR_WORKGROUP_SIZE + tid;
    thin_u64 w[8];
    lod_load_bytes(a.level, chain * PCR_POINTS_PER_THREAD, w);
    thin_u64 word = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w[k] = lod_bytes_final(w[k], (uint32_t)(cand >> (8 * k)) & 0xFFu, a.levels);
        word |= (thin_u64)lod_bits_of_flags(lod_bytes_written(w[k], a.levels, a.classes)) << (8 * k);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(a.level + chain * PCR_POINTS_PER_THREAD);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        dst[k] = make_uint4((uint32_t)w[2 * k], (uint32_t)(w[2 * k] >> 32), (uint32_t)w[2 * k + 1], (uint32_t)(w[2 * k + 1] >> 32));
    keep[chain] = word;
    for (uint32_t l = 0; l <= a.levels; ++l) {
        uint32_t n = lod_count_level(w, l);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
        if (lane == 0) s_part[l][wave] = n;
    }
    __syncthreads();
    if (tid <= a.levels) {
        uint32_t t = 0;
        for (int k = 0; k < LWC_WAVES; ++k) t += s_part[tid][k];
        counts[(size_t)blockIdx.x * (a.levels + 1) + tid] = t;
    }
}

// Workgroup x takes list[x]: its record of level l with the lowest row goes to index offsets[x * (levels + 1) + l] of points, rows
// and levels (each may be NULL), the others of that level behind it in row order. Nothing is stored at or beyond index `total`.
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_lod_write(StreamView s, const uint32_t *list, LodArgs a, const int64_t *offsets, thin_u64 total,
                                                                  uint4 *points, int64_t *rows, uint8_t *levels)
{
    const uint32_t b = list[blockIdx.x] & ~LOD_CUT;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint16_t s_index[LOD_CLASSES][PCR_WORKGROUP_SIZE];
    __shared__ uint32_t s_wave[LOD_CLASSES][LWC_WAVES];
    __shared__ int64_t s_first[LOD_CLASSES];
    const int64_t row0 = (int64_t)(b - a.first_batch) * PCR_POINTS_PER_BATCH + (int64_t)tid * PCR_POINTS_PER_THREAD;
    thin_u64 w[8];
    lod_load_bytes(a.level, (thin_u64)row0, w);
    for (uint32_t l = 0; l < a.classes; ++l) {
        const uint32_t mine = lod_count_level(w, l);
        uint32_t incl = mine;                               // chain_prefix_in_wave spelled out: on it every instantiation compiles to another stream
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63) s_wave[l][wave] = incl;
        s_index[l][tid] = (uint16_t)(incl - mine);
    }
    if (tid < a.classes) s_first[tid] = offsets[(size_t)blockIdx.x * (a.levels + 1) + tid];
    load_packed_table(s, b, s_table);                       // (its barrier publishes s_wave and s_first as well)
    for (uint32_t l = 0; l < a.classes; ++l) {
        uint32_t before = 0;
        for (uint32_t k = 0; k < wave; ++k) before += s_wave[l][k];
        s_index[l][tid] = (uint16_t)(s_index[l][tid] + before);                // (a lane reads and writes its own column only)
    }
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        const uint32_t l = (uint32_t)(w[0] >> (8u * ((uint32_t)i & 7u))) & 0xFFu;
        if (((uint32_t)i & 7u) == 7u) {
#pragma unroll
            for (int k = 0; k < 7; ++k) w[k] = w[k + 1];
        }
        if (l < a.classes) {
            const uint32_t at = s_index[l][tid];
            s_index[l][tid] = (uint16_t)(at + 1u);
            const int64_t dst = s_first[l] + at;
            if ((thin_u64)dst < total) {
                if (points) points[dst] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
                if (rows) rows[dst] = row0 + i;
                if (levels) levels[dst] = (uint8_t)l;
            }
        }
    });
}

template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_lod_rows(StreamView s, const uint32_t *list, uint32_t first_batch, const thin_u64 *keep,
                                                                 const int64_t *offsets, uint4 *points, int64_t *rows, const uint8_t *level, uint8_t *levels)
{
    write_kept_rows<LAYOUT, BC7>(s, list, first_batch, keep, offsets, points, rows, [&](int64_t dst, int64_t row) {
        if (levels) levels[dst] = level[row];
    });
}

// ------------------------------------------------------------------------------------------------
// Voxel denoising (pcr_denoise / pcr_read_denoise): a candidate is isolated iff the 27 voxels around its own hold at most
// max_count candidates of the call (itself included). pcr_thin's frame with a sum in the table instead of a minimum, on the
// lattice of noise_lattice (pcr_lattice.h: every voxel index in 1 .. 2^21 - 2, so a neighbour's key is the voxel's key plus or
// minus 1, 2^21, 2^42 and never leaves its fields). One launch each:
//   k_thin_runs        (above) runs and candidates per batch; the host sizes the table from the runs.
//   k_denoise_clear    key = all ones, value = 0 in every slot.
//   k_denoise_count    colourless decode: at the end of every run one insertion, compare-and-swap on the key as thin_insert,
//                      then a 64-bit atomic add of the run's length. Addition commutes: the table is exact and the same from run
//                      to run.
//   k_denoise_verdict  a thread per slot: the values of the 27 keys around an occupied slot's summed (each looked up from its
//                      home to the key or an empty slot), early out once the sum exceeds max_count; "isolated" goes into bit 63
//                      of the slot's own value with an atomic OR (counts are below 2^40: readers mask the bit out). The 27
//                      lookups are paid per voxel, not per point.
//   k_denoise_flag     colourless decode a third time: at every run start the run's own slot is looked up, the bits of the run's
//                      rows go into the lane's keep word by verdict and mode; the lane stores its chain's word once.
//   k_thin_totals / k_thin_write (above) size and write the output.
// No workgroup waits for another one; every probe loop makes at most `slots` steps.
// ------------------------------------------------------------------------------------------------
constexpr thin_u64 DENOISE_ISOLATED_BIT = 1ull << 63;

struct DenoiseArgs {
    ThinArgs t;                     // the clip, the shifted lattice, the first batch, the table and the error word
    thin_u64 max_count;             // isolated: N27 <= max_count
    thin_u64 *counters;             // [2] occupied slots, and of those the isolated ones (k_denoise_verdict adds)
};

__global__ void __launch_bounds__(256) k_denoise_clear(ThinSlot *table, thin_u64 slots)
{
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        table[i].key = THIN_EMPTY;
        table[i].val = 0ull;
    }
}

// thin_insert with a sum: the slot of the key, or the first free one from the key's home on, gets `count` added. Returns the
// slot's index, or THIN_EMPTY with the error word set.
__device__ __forceinline__ thin_u64 denoise_insert_slot(const ThinArgs &a, thin_u64 key, thin_u64 count)
{
    const thin_u64 slots = 1ull << a.log2_slots, mask = slots - 1;
    thin_u64 h = (key * THIN_HASH_MUL) >> (64u - a.log2_slots);
    for (thin_u64 probe = 0; probe < slots; ++probe) {
        ThinSlot *slot = a.table + h;
        thin_u64 old = __hip_atomic_load(&slot->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (a taken slot never changes its key)
        if (old == THIN_EMPTY) old = atomicCAS(&slot->key, THIN_EMPTY, key);
        if (old == THIN_EMPTY || old == key) {
            __hip_atomic_fetch_add(&slot->val, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (the result is not used)
            return h;
        }
        h = (h + 1) & mask;
    }
    *a.error = 1u;                                          // every slot holds another key: the host sized the table wrongly
    return THIN_EMPTY;
}

__device__ __forceinline__ void denoise_insert(const ThinArgs &a, thin_u64 key, thin_u64 count)
{
    (void)denoise_insert_slot(a, key, count);
}

// The value of `key` in a table nobody inserts into any more (bit 63 included): from the key's home on to the key or an empty
// slot. found: the key has a slot.
__device__ __forceinline__ thin_u64 denoise_lookup(const ThinSlot *table, uint32_t log2_slots, thin_u64 key, bool &found)
{
    const thin_u64 slots = 1ull << log2_slots, mask = slots - 1;
    thin_u64 h = (key * THIN_HASH_MUL) >> (64u - log2_slots);
    found = false;
    for (thin_u64 probe = 0; probe < slots; ++probe) {
        const thin_u64 k = table[h].key;
        if (k == key) { found = true; return __hip_atomic_load(&table[h].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        if (k == THIN_EMPTY) return 0ull;
        h = (h + 1) & mask;
    }
    return 0ull;
}

template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_denoise_count(StreamView s, const uint32_t *list, ThinArgs a)
{
    const uint32_t b = list[blockIdx.x];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    thin_u64 prev = THIN_EMPTY;
    uint32_t len = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t d2;
        const thin_u64 key = in_box(a.q, x, y, z) ? thin_key(a, x, y, z, d2) : THIN_EMPTY;
        if (key == prev) {
            ++len;
        } else {
            if (prev != THIN_EMPTY) denoise_insert(a, prev, len);
            prev = key; len = 1;
        }
    });
    if (prev != THIN_EMPTY) denoise_insert(a, prev, len);
}

__global__ void __launch_bounds__(256) k_denoise_verdict(DenoiseArgs a)
{
    ThinSlot *table = a.t.table;
    const thin_u64 slots = 1ull << a.t.log2_slots;
    uint32_t occupied = 0, isolated = 0;
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        const thin_u64 key = table[i].key;
        if (key == THIN_EMPTY) continue;
        // the voxel's own count first (no lookup), then the 26 around it; every index is in 1 .. 2^21 - 2 (noise_lattice)
        thin_u64 sum = __hip_atomic_load(&table[i].val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~DENOISE_ISOLATED_BIT;
        for (int n = 0; n < 27 && sum <= a.max_count; ++n) {
            if (n == 13) continue;
            const thin_u64 dx = (thin_u64)(n % 3), dy = (thin_u64)(n / 3 % 3), dz = (thin_u64)(n / 9);
            const thin_u64 other = key + dx + (dy << THIN_KEY_BITS) + (dz << (2 * THIN_KEY_BITS)) - (1ull + (1ull << THIN_KEY_BITS) + (1ull << (2 * THIN_KEY_BITS)));
            bool found;
            sum += denoise_lookup(table, a.t.log2_slots, other, found) & ~DENOISE_ISOLATED_BIT;
        }
        ++occupied;
        if (sum <= a.max_count) {
            ++isolated;
            atomicOr(&table[i].val, DENOISE_ISOLATED_BIT);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { occupied += __shfl_xor(occupied, d, 64); isolated += __shfl_xor(isolated, d, 64); }
    if ((threadIdx.x & 63u) == 0) {
        if (occupied) atomicAdd(&a.counters[0], (thin_u64)occupied);
        if (isolated) atomicAdd(&a.counters[1], (thin_u64)isolated);
    }
}

// Workgroup x takes list[x]: keep[(b - first_batch) * 1024 + chain] = the chain's rows to write, MODE's side of the verdict
template <int LAYOUT, int MODE>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_denoise_flag(StreamView s, const uint32_t *list, ThinArgs a, thin_u64 *keep)
{
    const uint32_t b = list[blockIdx.x];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    thin_u64 prev = THIN_EMPTY, word = 0;
    bool write = false;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t d2;
        const thin_u64 key = in_box(a.q, x, y, z) ? thin_key(a, x, y, z, d2) : THIN_EMPTY;
        if (key != prev) {
            prev = key; write = false;
            if (key != THIN_EMPTY) {
                bool found;
                const thin_u64 val = denoise_lookup(a.table, a.log2_slots, key, found);
                if (!found) *a.error = 1u;                                  // (k_denoise_count inserted every run's key)
                write = found && ((val & DENOISE_ISOLATED_BIT) != 0) == (MODE == PCR_DENOISE_ISOLATED);
            }
        }
        word |= write ? 1ull << (uint32_t)i : 0ull;
    });
    keep[(size_t)(b - a.first_batch) * PCR_WORKGROUP_SIZE + threadIdx.x] = word;
}

// ------------------------------------------------------------------------------------------------
// Connected components (pcr_components / pcr_read_components): the occupied voxels of pcr_denoise's table are the nodes of a
// graph, two of them adjacent if they differ by at most 1 on every axis (26) or by exactly 1 on one axis (6); a component whose
// voxels hold fewer than min_points candidates is small. pcr_denoise's frame and lattice with a union-find over the slots of the
// table between the counting and the flagging. One launch each:
//   k_thin_runs / k_denoise_clear (above), k_components_clear (min_row = all ones, total = 0, parent[i] = i).
//   k_components_count    k_denoise_count that also takes the minimum of the run's first row into min_row[slot].
//   k_components_link     a thread per slot: the forward half of the neighbourhood (13 of 26 keys, 3 of 6) looked up, every
//                         neighbour found united with the slot (components_unite). The total order of the forest is the slot
//                         index: a parent is always a lesser index than its child, so no cycle can form.
//   k_components_flatten  a thread per slot: parent[i] = the root, the slot's count added to total[root], its least row taken
//                         into min_row[root] by minimum: the root then holds the component's size and its label.
//   k_components_verdict  a thread per slot: DENOISE_ISOLATED_BIT into the slot's value iff total[root] < min_points, min_row[i]
//                         = min_row[root] (the label of every slot), and the counters of the statistics.
//   k_denoise_flag / k_thin_totals / k_thin_write (above) flag, size and write; k_components_labels writes the labels of the
//                         flagged rows in a colourless decode of its own (run -> slot -> label).
// While a kernel changes parent[], every read of it is a relaxed atomic load at agent scope and every write an atomic (another
// CU's L1 is never refreshed by a store: a plain re-read after a failed compare-and-swap could see "I am a root" forever).
// Kernel boundaries on the one stream are the only other synchronisation; no workgroup waits for another one. Every loop is
// bounded: a climb goes to a strictly lesser index with every step, at most `slots` of them; a union makes fewer than 4 * slots
// rounds. A lane that runs out sets the error word and leaves. The result is exact and canonical: which slot is a root depends on
// the table, but labels and sizes are minima and sums over the component, functions of the partition alone.
// ------------------------------------------------------------------------------------------------
struct ComponentsArgs {
    ThinArgs t;                     // the clip, the shifted lattice, the first batch, the table and the error word
    thin_u64 *min_row;              // [slots] the least row of the slot's voxel; at a root after k_components_flatten, everywhere after
                                    // k_components_verdict: of its component
    thin_u64 *total;                // [slots] at a root: the candidates of its component
    uint32_t *parent;               // [slots] the forest over slot indices
    thin_u64 min_points;            // small: total < min_points
    thin_u64 *counters;             // [5] occupied slots, components, small ones, their candidates, the largest total
    int32_t connectivity;           // 6 or 26
};

__global__ void __launch_bounds__(256) k_components_clear(ComponentsArgs a)
{
    const thin_u64 slots = 1ull << a.t.log2_slots;
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        a.min_row[i] = THIN_EMPTY;
        a.total[i] = 0ull;
        a.parent[i] = (uint32_t)i;
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_components_count(StreamView s, const uint32_t *list, ThinArgs a, thin_u64 *min_row)
{
    const uint32_t b = list[blockIdx.x];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    const thin_u64 row0 = (thin_u64)(b - a.first_batch) * PCR_POINTS_PER_BATCH + (thin_u64)threadIdx.x * PCR_POINTS_PER_THREAD;
    thin_u64 prev = THIN_EMPTY, start = 0;
    uint32_t len = 0;
    auto insert = [&]() {
        const thin_u64 slot = denoise_insert_slot(a, prev, len);
        if (slot != THIN_EMPTY) __hip_atomic_fetch_min(&min_row[slot], start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t d2;
        const thin_u64 key = in_box(a.q, x, y, z) ? thin_key(a, x, y, z, d2) : THIN_EMPTY;
        if (key == prev) {
            ++len;
        } else {
            if (prev != THIN_EMPTY) insert();
            prev = key; len = 1; start = row0 + (uint32_t)i;
        }
    });
    if (prev != THIN_EMPTY) insert();
}

// The slot of `key` in a table nobody inserts into any more: from the key's home on to the key or an empty slot
__device__ __forceinline__ bool components_lookup(const ThinSlot *table, uint32_t log2_slots, thin_u64 key, uint32_t &at)
{
    const thin_u64 slots = 1ull << log2_slots, mask = slots - 1;
    thin_u64 h = (key * THIN_HASH_MUL) >> (64u - log2_slots);
    for (thin_u64 probe = 0; probe < slots; ++probe) {
        const thin_u64 k = table[h].key;
        if (k == key) { at = (uint32_t)h; return true; }
        if (k == THIN_EMPTY) return false;
        h = (h + 1) & mask;
    }
    return false;
}

__device__ __forceinline__ uint32_t components_parent(const uint32_t *parent, uint32_t x)
{
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One tree out of the trees of x and y (Rem's algorithm with splicing, every step a compare-and-swap): of the two walkers the
// one whose parent is the greater moves. If it stands on a root, the root goes under the other walker's parent and the union is
// done; else its parent word is lowered to the other walker's parent -- a slot of the component this union forms, and a lesser
// index than the old parent -- and it steps to the old parent. Both walkers under one parent: done, without a look at the root.
// So lanes that unite inside a component that already hangs under one root read two parent words and leave the root's word
// alone: a cloud that is one large component does not turn that word into the one address every lane waits for.
// Every move takes a walker to a lesser index and a failed compare-and-swap on a root is followed by a move: fewer than
// 4 * slots rounds.
__device__ __forceinline__ void components_unite(const ComponentsArgs &a, uint32_t x, uint32_t y)
{
    const thin_u64 rounds = 4ull << a.t.log2_slots;
    for (thin_u64 round = 0; round < rounds; ++round) {
        uint32_t px = components_parent(a.parent, x), py = components_parent(a.parent, y);
        if (px == py) return;
        if (px < py) { uint32_t t = x; x = y; y = t; t = px; px = py; py = t; }     // x is the walker with the greater parent
        if (px == x) {
            if (atomicCAS(&a.parent[x], x, py) == x) return;
            // x has been hooked by another lane in between: it is no root any more, the next round moves on from it
        } else {
            (void)atomicCAS(&a.parent[x], px, py);          // (whoever changed it first lowered it as well)
            x = px;
        }
    }
    *a.t.error = 1u;
}

__global__ void __launch_bounds__(256) k_components_link(ComponentsArgs a)
{
    const ThinSlot *table = a.t.table;
    const thin_u64 slots = 1ull << a.t.log2_slots;
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        const thin_u64 key = table[i].key;
        if (key == THIN_EMPTY) continue;
        // n = (dx + 1) + 3 (dy + 1) + 9 (dz + 1) above the centre's 13: every undirected edge once; with 6 the three axes only.
        // Every index is in 1 .. 2^21 - 2 (noise_lattice), so no neighbour's key leaves its fields.
        for (int n = 14; n < 27; ++n) {
            if (a.connectivity == 6 && n != 14 && n != 16 && n != 22) continue;
            const thin_u64 dx = (thin_u64)(n % 3), dy = (thin_u64)(n / 3 % 3), dz = (thin_u64)(n / 9);
            const thin_u64 other = key + dx + (dy << THIN_KEY_BITS) + (dz << (2 * THIN_KEY_BITS)) - (1ull + (1ull << THIN_KEY_BITS) + (1ull << (2 * THIN_KEY_BITS)));
            uint32_t at;
            if (components_lookup(table, a.t.log2_slots, other, at)) components_unite(a, (uint32_t)i, at);
        }
    }
}

__global__ void __launch_bounds__(256) k_components_flatten(ComponentsArgs a)
{
    const ThinSlot *table = a.t.table;
    const thin_u64 slots = 1ull << a.t.log2_slots;
    const thin_u64 stride = (thin_u64)gridDim.x * blockDim.x;
    // (slots is a multiple of the stride or below it and the stride a multiple of 64: the lanes of a wave leave the loop together)
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {
        bool root = table[i].key != THIN_EMPTY;
        const bool occupied = root;
        // (the only store to parent[i] in this kernel is this lane's, so it is the root when the kernel ends; a lane that climbs
        // through i meanwhile sees the old parent or the root, an ancestor either way)
        uint32_t x = (uint32_t)i;
        if (occupied) {
            root = false;
            for (thin_u64 step = 0; step < slots && !root; ++step) {
                const uint32_t p = components_parent(a.parent, x);
                root = p == x;
                x = p;
            }
            if (!root) *a.t.error = 1u;
        }
        thin_u64 count = root ? table[i].val : 0ull, least = root ? a.min_row[i] : THIN_EMPTY;
        if (root) __hip_atomic_store(&a.parent[i], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the lanes of the wave that share the first such lane's root hand it their sums in one pair of atomics: in a cloud that
        // is one large component every lane would queue at the same two words otherwise
        const thin_u64 have = __ballot(root);
        if (have == 0ull) continue;
        const int lead = __ffsll((long long)have) - 1;
        const bool shared = root && x == (uint32_t)__shfl((int)x, lead, 64);
        thin_u64 sum = shared ? count : 0ull, low = shared ? least : THIN_EMPTY;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sum += (thin_u64)__shfl_xor((long long)sum, d, 64);
            low = min(low, (thin_u64)__shfl_xor((long long)low, d, 64));
        }
        if (shared ? (int)(threadIdx.x & 63u) == lead : root) {
            __hip_atomic_fetch_add(&a.total[x], shared ? sum : count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&a.min_row[x], shared ? low : least, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ void __launch_bounds__(256) k_components_verdict(ComponentsArgs a)
{
    ThinSlot *table = a.t.table;
    const thin_u64 slots = 1ull << a.t.log2_slots;
    uint32_t occupied = 0, roots = 0, small_roots = 0;
    thin_u64 small_points = 0, largest = 0;
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        if (table[i].key == THIN_EMPTY) continue;
        const uint32_t r = a.parent[i];
        const thin_u64 total = a.total[r];
        const bool small = total < a.min_points;
        ++occupied;
        if (small) atomicOr(&table[i].val, DENOISE_ISOLATED_BIT);
        if (r == (uint32_t)i) {
            ++roots;
            largest = max(largest, total);
            if (small) { ++small_roots; small_points += total; }
        } else {
            a.min_row[i] = a.min_row[r];                    // (a root's own min_row is written by nobody)
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        occupied += __shfl_xor(occupied, d, 64); roots += __shfl_xor(roots, d, 64); small_roots += __shfl_xor(small_roots, d, 64);
        small_points += __shfl_xor(small_points, d, 64);
        largest = max(largest, (thin_u64)__shfl_xor(largest, d, 64));
    }
    if ((threadIdx.x & 63u) == 0) {
        if (occupied) atomicAdd(&a.counters[0], (thin_u64)occupied);
        if (roots) atomicAdd(&a.counters[1], (thin_u64)roots);
        if (small_roots) atomicAdd(&a.counters[2], (thin_u64)small_roots);
        if (small_points) atomicAdd(&a.counters[3], small_points);
        if (largest) atomicMax(&a.counters[4], largest);
    }
}

// k_thin_write's placement without the records: workgroup x takes list[x], a batch that writes a record; the label of every
// flagged row goes to labels[offsets[x] ..], chain after chain. label[] is min_row after k_components_verdict.
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_components_labels(StreamView s, const uint32_t *list, ThinArgs a, const thin_u64 *keep,
                                                                          const int64_t *offsets, const thin_u64 *label, int64_t *labels)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const thin_u64 word = keep[(size_t)(b - a.first_batch) * PCR_WORKGROUP_SIZE + tid];
    const uint32_t mine = (uint32_t)__popcll(word);
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_packed_table(s, b, s_table);                       // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    int64_t dst = offsets[blockIdx.x] + before;
    const int64_t end = dst + mine;                         // never past the bits of this chain's word
    thin_u64 prev = THIN_EMPTY;
    int64_t mark = -1;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
        if (((word >> (uint32_t)i) & 1ull) && dst < end) {  // (a flagged row is a candidate: it has a key)
            uint32_t d2, at;
            const thin_u64 key = thin_key(a, x, y, z, d2);
            if (key != prev) {
                prev = key;
                if (components_lookup(a.table, a.log2_slots, key, at)) mark = (int64_t)label[at];
                else mark = -1;                             // (cannot happen: k_components_count inserted every run's key)
            }
            labels[dst] = mark;
            ++dst;
        }
    });
}

// ------------------------------------------------------------------------------------------------
// Radius neighbourhoods (pcr_neighbors / pcr_read_neighbors): per candidate N = the candidates within `radius` (itself included)
// and nn2 = the least squared distance to a candidate of another row within the radius. pcr_denoise's frame and lattice with
// cell = radius, so the 27 voxels around a point's own cover its sphere, and the counts of the table turned into an index: a copy
// of the candidates bucketed by voxel. One launch each:
//   k_thin_runs / k_denoise_clear (above).
//   k_neighbors_count   k_denoise_count that also stores, per chain, a word with a bit wherever the key differs from the previous
//                       point's: the starts of the runs (and of the stretches outside the clip).
//   k_neighbors_alloc   a thread per slot: an occupied slot takes its bucket [start, start + count) from one cursor and its
//                       ceil(count / 64) work items (slot, chunk) from another, both aggregated per wave (a prefix over the wave,
//                       one atomic by lane 63). Which bucket lies where depends on the order of the atomics; nothing observable
//                       does. The slot's value becomes (count - 1) | start << 32 (both fit 32 bits: at most 2^32 candidates), so
//                       that whoever finds a key has its bucket from the same 16 bytes. It also reduces the occupied slots and
//                       the largest count.
//   k_neighbors_fill    colourless decode: at every run start the run's length is read from the chain's word (the distance to
//                       the next set bit), the slot looked up and `length` entries reserved in its bucket with one atomic; the
//                       run's points then stream there as {x, y, z, row} with plain 16-byte stores.
//   k_neighbors_pairs   a wave per work item at a time, four waves to a workgroup, the work list walked with the grid's stride: lane j holds centre j of the chunk, lanes 0 .. 26 look up one
//                       neighbour voxel each (once per chunk, not per point), the 27 buckets laid end to end are read in tiles of
//                       64 entries (one 16-byte load per lane, whatever bucket the entry lies in: one load per 64 entries, not
//                       one per voxel) and broadcast entry by entry with a wave-uniform lane read -- no LDS, no barrier. Coordinates of adjacent voxels differ by less than 2 * radius <= 2^21, so the
//                       32-bit difference is exact and each square is one 32 x 32 -> 64 multiply-add. N and nn2 go by row into
//                       dense arrays (only those asked for), the row's bit into pcr_thin's keep bitmap by mode.
//   k_thin_totals (above) / k_neighbors_write   k_thin_write that also gathers N and nn2 of the written rows.
// Sums, minima and bit-ors commute: the result does not depend on the hash, the table size, the order of the buckets or of
// lanes, workgroups and launches. No workgroup waits for another one; every probe loop makes at most `slots` steps, and a store
// into the buckets or the work list is tested against the array's end (a miss sets the error word).
// ------------------------------------------------------------------------------------------------
struct NeighborsArgs {
    ThinArgs t;                     // the clip, the lattice (cell = radius), the first batch, the table and the error word
    uint2 *cursor;                  // [slots] x: the bucket's first entry, y: entries filled (k_neighbors_fill reserves from it)
    thin_u64 *starts;               // [batches of the range * 1024] the run-start word of every chain of a listed batch
    uint4 *bucket;                  // [candidates] x, y, z, row
    thin_u64 *work;                 // [work_capacity] slot << 32 | chunk
    thin_u64 *counters;             // [NEIGHBORS_COUNTERS]
    thin_u64 candidates, work_capacity, rows;   // the lengths of bucket and work, and the rows of the range (the dense arrays' length)
    thin_u64 r2, min_count;         // radius squared; sparse: N < min_count
    int mode, early;                // early: nobody reads N or nn2, a wave may stop once every centre has min_count
    thin_u64 *keep, *out_n, *out_nn2;   // the keep bitmap; dense by row, or NULL
};
// (pairs_bound and the sparse candidates are summed by every wave of k_neighbors_pairs over the work items it takes, in registers,
// and added to one of 64 partial sums each, picked by workgroup; the host adds them up. One atomic per work item into 64 adjacent
// words measured 16 ms for 1e7 work items.)
enum { NEIGHBORS_BUCKET_CURSOR = 0, NEIGHBORS_WORK_CURSOR, NEIGHBORS_VOXELS, NEIGHBORS_MAX_VOXEL, NEIGHBORS_PAIRS_BOUND, NEIGHBORS_SPARSE = NEIGHBORS_PAIRS_BOUND + 64,
       NEIGHBORS_COUNTERS = NEIGHBORS_SPARSE + 64 };

template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_neighbors_count(StreamView s, const uint32_t *list, ThinArgs a, thin_u64 *starts)
{
    const uint32_t b = list[blockIdx.x];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    thin_u64 prev = THIN_EMPTY, word = 0;
    uint32_t len = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t d2;
        const thin_u64 key = in_box(a.q, x, y, z) ? thin_key(a, x, y, z, d2) : THIN_EMPTY;
        if (key == prev) {
            ++len;
        } else {
            if (prev != THIN_EMPTY) denoise_insert(a, prev, len);
            prev = key; len = 1;
            word |= 1ull << (uint32_t)i;
        }
    });
    if (prev != THIN_EMPTY) denoise_insert(a, prev, len);
    starts[(size_t)(b - a.first_batch) * PCR_WORKGROUP_SIZE + threadIdx.x] = word;
}

__device__ __forceinline__ thin_u64 neighbors_key(thin_u64 key, int n)
{
    const thin_u64 dx = (thin_u64)(n % 3), dy = (thin_u64)(n / 3 % 3), dz = (thin_u64)(n / 9);
    return key + dx + (dy << THIN_KEY_BITS) + (dz << (2 * THIN_KEY_BITS)) - (1ull + (1ull << THIN_KEY_BITS) + (1ull << (2 * THIN_KEY_BITS)));
}

// (launched with a power of two of threads that divides the slots: every lane of a wave makes the same number of rounds)
__global__ void __launch_bounds__(256) k_neighbors_alloc(NeighborsArgs a)
{
    ThinSlot *table = a.t.table;
    const thin_u64 slots = 1ull << a.t.log2_slots;
    const uint32_t lane = threadIdx.x & 63u;
    thin_u64 voxels = 0, largest = 0;
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        const thin_u64 key = table[i].key;
        const thin_u64 cnt = key == THIN_EMPTY ? 0ull : table[i].val;
        const thin_u64 chunks = (cnt + 63u) >> 6;
        thin_u64 cnt_incl = cnt, chunks_incl = chunks;       // inclusive prefixes over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const thin_u64 u0 = __shfl_up(cnt_incl, d, 64), u1 = __shfl_up(chunks_incl, d, 64);
            if (lane >= (uint32_t)d) { cnt_incl += u0; chunks_incl += u1; }
        }
        thin_u64 base0 = 0, base1 = 0;
        if (lane == 63 && cnt_incl) {
            base0 = atomicAdd(&a.counters[NEIGHBORS_BUCKET_CURSOR], cnt_incl);
            base1 = atomicAdd(&a.counters[NEIGHBORS_WORK_CURSOR], chunks_incl);
        }
        base0 = __shfl(base0, 63, 64); base1 = __shfl(base1, 63, 64);
        if (cnt == 0) continue;                             // (the next round's shuffles run with the wave whole again: the loop has one latch)
        const thin_u64 start = base0 + cnt_incl - cnt;
        a.cursor[i] = make_uint2((uint32_t)start, 0u);
        thin_u64 w = base1 + chunks_incl - chunks;
        for (thin_u64 k = 0; k < chunks; ++k, ++w) {
            if (w < a.work_capacity) a.work[w] = (i << 32) | k;
            else *a.t.error = 1u;
        }
        table[i].val = (cnt - 1ull) | (start << 32);        // (only this thread reads or writes this slot's value in this kernel)
        ++voxels;
        largest = max(largest, cnt);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        voxels += __shfl_xor(voxels, d, 64);
        largest = max(largest, (thin_u64)__shfl_xor(largest, d, 64));
    }
    if (lane == 0 && voxels) {
        atomicAdd(&a.counters[NEIGHBORS_VOXELS], voxels);
        atomicMax(&a.counters[NEIGHBORS_MAX_VOXEL], largest);
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_neighbors_fill(StreamView s, const uint32_t *list, NeighborsArgs a)
{
    const uint32_t b = list[blockIdx.x];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    const thin_u64 word = a.starts[(size_t)(b - a.t.first_batch) * PCR_WORKGROUP_SIZE + threadIdx.x];
    const uint32_t row0 = (b - a.t.first_batch) * (uint32_t)PCR_POINTS_PER_BATCH + threadIdx.x * (uint32_t)PCR_POINTS_PER_THREAD;
    thin_u64 prev = THIN_EMPTY, pos = 0, end = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
        uint32_t d2;
        const thin_u64 key = in_box(a.t.q, x, y, z) ? thin_key(a.t, x, y, z, d2) : THIN_EMPTY;
        if (key != prev) {
            prev = key; pos = end = 0;
            if (key != THIN_EMPTY) {
                const thin_u64 rest = i < 63 ? word >> (uint32_t)(i + 1) : 0ull;
                const uint32_t len = rest ? (uint32_t)__builtin_ctzll(rest) + 1u : 64u - (uint32_t)i;
                uint32_t at;
                if (components_lookup(a.t.table, a.t.log2_slots, key, at)) {
                    pos = (thin_u64)a.cursor[at].x + atomicAdd(&a.cursor[at].y, len);
                    end = min(pos + len, a.candidates);
                    if (end != pos + len) *a.t.error = 1u;
                } else {
                    *a.t.error = 1u;                        // (cannot happen: k_neighbors_count inserted every run's key)
                }
            }
        }
        if (pos < end) a.bucket[pos++] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, row0 + (uint32_t)i);
    });
}

__device__ __forceinline__ thin_u64 neighbors_uniform(thin_u64 v)
{
    return ((thin_u64)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

__global__ void __launch_bounds__(256) k_neighbors_pairs(NeighborsArgs a, thin_u64 items)
{
    const uint32_t lane = threadIdx.x & 63u;
    thin_u64 bound = 0, sparse_total = 0;                   // this wave's share of pairs_bound and of the sparse candidates
    // (no barrier below: a wave is on its own; it takes every (waves of the grid)-th work item)
    for (thin_u64 wi = neighbors_uniform((thin_u64)blockIdx.x * 4u + (threadIdx.x >> 6)); wi < items; wi += (thin_u64)gridDim.x * 4u) {
    const thin_u64 item = neighbors_uniform(a.work[wi]);
    const uint32_t slot = (uint32_t)(item >> 32), chunk = (uint32_t)item;
    const ThinSlot *table = a.t.table;
    const thin_u64 key = neighbors_uniform(table[slot].key), own = neighbors_uniform(table[slot].val);     // (k_neighbors_alloc's value)
    const thin_u64 count = (own & 0xFFFFFFFFull) + 1ull, own_start = own >> 32;
    const thin_u64 idx = (thin_u64)chunk * 64u + lane;
    const bool valid = idx < count && own_start + idx < a.candidates;
    const uint4 centre = valid ? a.bucket[own_start + idx] : make_uint4(0, 0, 0, 0);

    // lane n < 27: the bucket of neighbour voxel n (13 is the chunk's own); lanes 27 .. 63 hold empty ones
    uint32_t nb_start = 0;
    thin_u64 nb_count = 0;
    if (lane < 27u) {
        uint32_t at = slot;
        if (lane == 13u || components_lookup(table, a.t.log2_slots, neighbors_key(key, (int)lane), at)) {
            const thin_u64 v = table[at].val;
            nb_start = (uint32_t)(v >> 32);
            nb_count = (v & 0xFFFFFFFFull) + 1ull;
        }
    }
    // The 27 buckets laid end to end: bucket n covers [excl(n), excl(n) + count(n)) of `total` entries, which the wave reads in
    // tiles of 64 whatever bucket they lie in -- one load per 64 entries, not one per neighbour voxel.
    thin_u64 nb_excl = nb_count;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const thin_u64 up = __shfl_up(nb_excl, d, 64);
        if (lane >= (uint32_t)d) nb_excl += up;
    }
    const thin_u64 total = neighbors_uniform(__shfl(nb_excl, 26, 64));
    nb_excl -= nb_count;
    const uint32_t excl_lo = (uint32_t)nb_excl, excl_hi = (uint32_t)(nb_excl >> 32), count_lo = (uint32_t)nb_count, count_hi = (uint32_t)(nb_count >> 32);

    // pairs_bound: what this chunk tests at most -- from the table, so the early exit below does not change it
    bound += (thin_u64)__popcll(__ballot(valid)) * total;

    thin_u64 n_in = 0, zeros = 0, least = ~0ull;            // least: the minimum of d2 - 1, so that d2 == 0 wraps out of the way
    for (thin_u64 t0 = 0; t0 < total; t0 += 64u) {
        const int m = (int)min((thin_u64)64u, total - t0);
        const thin_u64 g = t0 + lane;                       // this lane's entry of the tile
        thin_u64 at = ~0ull;
        for (int nb = 0; nb < 27; ++nb) {                   // (every value read here is wave-uniform)
            const thin_u64 e = ((thin_u64)(uint32_t)__builtin_amdgcn_readlane((int)excl_hi, nb) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)excl_lo, nb);
            const thin_u64 c = ((thin_u64)(uint32_t)__builtin_amdgcn_readlane((int)count_hi, nb) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)count_lo, nb);
            if (c == 0ull || e >= t0 + 64u || e + c <= t0) continue;
            const thin_u64 first = (uint32_t)__builtin_amdgcn_readlane((int)nb_start, nb);
            if (g >= e && g - e < c) at = first + (g - e);
        }
        const bool have = lane < (uint32_t)m && at < a.candidates;
        const uint4 tile = have ? a.bucket[at] : make_uint4(0, 0, 0, 0);
        uint32_t in32 = 0, zero32 = 0;
#pragma unroll 4
        for (int k = 0; k < m; ++k) {
            const int32_t dx = (int32_t)(centre.x - (uint32_t)__builtin_amdgcn_readlane((int)tile.x, k));
            const int32_t dy = (int32_t)(centre.y - (uint32_t)__builtin_amdgcn_readlane((int)tile.y, k));
            const int32_t dz = (int32_t)(centre.z - (uint32_t)__builtin_amdgcn_readlane((int)tile.z, k));
            const thin_u64 d2 = (thin_u64)((int64_t)dx * dx) + (thin_u64)((int64_t)dy * dy) + (thin_u64)((int64_t)dz * dz);
            in32 += d2 <= a.r2 ? 1u : 0u;
            zero32 += d2 == 0ull ? 1u : 0u;
            least = min(least, d2 - 1ull);
        }
        n_in += in32; zeros += zero32;
        if (a.early && __ballot(valid && n_in < a.min_count) == 0ull) break;
    }
    const bool sparse = valid && n_in < a.min_count;
    if (valid && centre.w < a.rows) {                       // (k_neighbors_fill wrote every entry: the row is one of the range)
        const thin_u64 row = centre.w;
        if (a.out_n) a.out_n[row] = n_in;
        if (a.out_nn2) a.out_nn2[row] = zeros >= 2ull ? 0ull : (least != ~0ull && least + 1ull <= a.r2 ? least + 1ull : ~0ull);
        if (a.mode == PCR_NEIGHBORS_ALL || (a.mode == PCR_NEIGHBORS_SPARSE) == sparse) atomicOr(&a.keep[row >> 6], 1ull << (row & 63u));
    }
    sparse_total += (thin_u64)__popcll(__ballot(sparse));
    }
    if (lane == 0) {
        if (bound) atomicAdd(&a.counters[NEIGHBORS_PAIRS_BOUND + (blockIdx.x & 63u)], bound);
        if (sparse_total) atomicAdd(&a.counters[NEIGHBORS_SPARSE + (blockIdx.x & 63u)], sparse_total);
    }
}

// k_thin_write that also gathers N and nn2 of the written rows from the dense arrays (any of the four outputs may be NULL);
// write_kept_rows' body written out, see there
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_neighbors_write(StreamView s, const uint32_t *list, uint32_t first_batch, const thin_u64 *keep,
                                                                        const int64_t *offsets, const thin_u64 *dense_n, const thin_u64 *dense_nn2,
                                                                        uint4 *points, int64_t *rows, int64_t *counts, thin_u64 *nn2)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const thin_u64 word = keep[(size_t)(b - first_batch) * PCR_WORKGROUP_SIZE + tid];
    const uint32_t mine = (uint32_t)__popcll(word);
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_packed_table(s, b, s_table);                       // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    int64_t dst = offsets[blockIdx.x] + before;
    const int64_t end = dst + mine;                         // never past the bits of this chain's word
    const int64_t row0 = (int64_t)(b - first_batch) * PCR_POINTS_PER_BATCH + (int64_t)tid * PCR_POINTS_PER_THREAD;
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        if (((word >> (uint32_t)i) & 1ull) && dst < end) {
            if (points) points[dst] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
            if (rows) rows[dst] = row0 + i;
            if (counts) counts[dst] = (int64_t)dense_n[row0 + i];
            if (nn2) nn2[dst] = dense_nn2[row0 + i];
            ++dst;
        }
    });
}

// ------------------------------------------------------------------------------------------------
// Local moments (pcr_local_moments / pcr_read_local_moments / pcr_moments_eigen): per candidate the count, the first and the
// second moments of the offsets d = q - p to the candidates q within `radius` of p (p included), exact int64 sums, and from them
// the eigenvalues of the covariance and the normal. The plan is pcr_neighbors' up to the filled buckets (k_neighbors_count /
// _alloc / _fill above); then
//   k_moments_pairs   k_neighbors_pairs' work distribution (a wave per work item, lane j holds centre j, lanes 0 .. 26 look up one
//                     neighbour voxel each, the 27 buckets laid end to end, read in tiles of 64 and broadcast by lane reads; no
//                     LDS, no barrier). Per lane and entry: three subtractions, d2 as there, the offsets masked to 0 where d2 >
//                     r2, then N, three first moments and six products. radius <= 32767 keeps a masked offset within 16 bits, so
//                     the products are exact 24-bit multiplies (v_mad_i32_i24, full rate, where the 32 x 32 -> 64 multiply-add
//                     is not) into 32-bit partial sums: a product is below 2^30, so the squares (unsigned) are flushed into
//                     the 64-bit sums every 4 entries and the mixed products (signed) every 2; N and the first moments fit 32
//                     bits over a tile of 64 and are flushed per tile. No early exit: every pair contributes. A valid lane
//                     sets its keep bit iff n >= min_count, stores its 80-byte record by row and runs moments_eigen in-lane.
//   k_moments_eigen   moments_eigen over an array of records, a thread each.
//   k_thin_totals (above) / k_moments_write   k_neighbors_write gathering the 80- and 48-byte records of the kept rows.
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(pcr_moments) == 80 && sizeof(pcr_eigen) == 48, "the records k_moments_* store");

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix: app, aqq, apq and, with r the third axis, arp, arq; v holds
// the eigenvectors as columns. Nothing happens for apq == 0. An overflowing theta * theta gives t = 0 and only clears apq.
__device__ __forceinline__ void moments_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double (&v)[3][3], int p, int q)
{
#pragma clang fp contract(off)
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    const double h = t * apq;
    app = app - h; aqq = aqq + h; apq = 0.0;
    const double g = arp, k = arq;
    arp = g - s * (k + g * tau);
    arq = k + s * (g - k * tau);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vp = v[i][p], vq = v[i][q];
        v[i][p] = vp - s * (vq + vp * tau);
        v[i][q] = vq + s * (vp - vq * tau);
    }
}

// pcr_eigen of a pcr_moments record (include/pcr_hip.h has the definition): out = value[0..2], normal[0..2]. f64, every operation
// rounded once, only + - * / and sqrt; no NaN or Inf for finite input.
__device__ __forceinline__ void moments_eigen(const pcr_moments &m, double (&out)[6])
{
#pragma clang fp contract(off)
    if (m.n <= 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = 0.0;
        return;
    }
    const double nf = (double)m.n;
    const double mx = (double)m.s[0] / nf, my = (double)m.s[1] / nf, mz = (double)m.s[2] / nf;
    double a00 = (double)m.q[0] / nf - mx * mx, a01 = (double)m.q[1] / nf - mx * my, a02 = (double)m.q[2] / nf - mx * mz;
    double a11 = (double)m.q[3] / nf - my * my, a12 = (double)m.q[4] / nf - my * mz, a22 = (double)m.q[5] / nf - mz * mz;
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 12 && (a01 != 0.0 || a02 != 0.0 || a12 != 0.0); ++sweep) {
        moments_rotate(a00, a11, a01, a02, a12, v, 0, 1);
        moments_rotate(a00, a22, a02, a01, a12, v, 0, 2);
        moments_rotate(a11, a22, a12, a01, a02, v, 1, 2);
    }
    // the least eigenvalue's axis, the lower one at a tie; the values ascending
    const int k = a22 < (a11 < a00 ? a11 : a00) ? 2 : (a11 < a00 ? 1 : 0);
    double nx = k == 0 ? v[0][0] : k == 1 ? v[0][1] : v[0][2];
    double ny = k == 0 ? v[1][0] : k == 1 ? v[1][1] : v[1][2];
    double nz = k == 0 ? v[2][0] : k == 1 ? v[2][1] : v[2][2];
    double e0 = a00, e1 = a11, e2 = a22, e;
    if (e1 < e0) { e = e0; e0 = e1; e1 = e; }
    if (e2 < e1) { e = e1; e1 = e2; e2 = e; }
    if (e1 < e0) { e = e0; e0 = e1; e1 = e; }
    // the sign: the first non-zero of nz, ny, nx is positive. (A chain of selects and an exact multiplication by +-1: as nested
    // branches, `if (nz < 0 || (nz == 0 && (ny < 0 || ...))) negate`, hipcc -O3 for gfx950 left the lanes with nz == 0 unflipped.)
    const double lead = nz != 0.0 ? nz : (ny != 0.0 ? ny : nx);
    const double sign = lead < 0.0 ? -1.0 : 1.0;
    nx = nx * sign; ny = ny * sign; nz = nz * sign;
    // (+ 0.0: a negative zero leaves as a positive one, so that equal results are equal bytes)
    out[0] = e0 + 0.0; out[1] = e1 + 0.0; out[2] = e2 + 0.0;
    out[3] = nx + 0.0; out[4] = ny + 0.0; out[5] = nz + 0.0;
}

__device__ __forceinline__ uint4 moments_pack(int64_t a, int64_t b)
{
    return make_uint4((uint32_t)(thin_u64)a, (uint32_t)((thin_u64)a >> 32), (uint32_t)(thin_u64)b, (uint32_t)((thin_u64)b >> 32));
}

// out_m: [a.rows * 5] the pcr_moments records by row, or NULL; out_e: [a.rows * 3] the pcr_eigen records by row, or NULL
__global__ void __launch_bounds__(256) k_moments_pairs(NeighborsArgs a, thin_u64 items, uint4 *out_m, uint4 *out_e)
{
    const uint32_t lane = threadIdx.x & 63u;
    thin_u64 bound = 0, sparse_total = 0;                   // this wave's share of pairs_bound and of the sparse candidates
    // (no barrier below: a wave is on its own; it takes every (waves of the grid)-th work item)
    for (thin_u64 wi = neighbors_uniform((thin_u64)blockIdx.x * 4u + (threadIdx.x >> 6)); wi < items; wi += (thin_u64)gridDim.x * 4u) {
    const thin_u64 item = neighbors_uniform(a.work[wi]);
    const uint32_t slot = (uint32_t)(item >> 32), chunk = (uint32_t)item;
    const ThinSlot *table = a.t.table;
    const thin_u64 key = neighbors_uniform(table[slot].key), own = neighbors_uniform(table[slot].val);     // (k_neighbors_alloc's value)
    const thin_u64 count = (own & 0xFFFFFFFFull) + 1ull, own_start = own >> 32;
    const thin_u64 idx = (thin_u64)chunk * 64u + lane;
    const bool valid = idx < count && own_start + idx < a.candidates;
    const uint4 centre = valid ? a.bucket[own_start + idx] : make_uint4(0, 0, 0, 0);

    // lane n < 27: the bucket of neighbour voxel n (13 is the chunk's own); lanes 27 .. 63 hold empty ones
    uint32_t nb_start = 0;
    thin_u64 nb_count = 0;
    if (lane < 27u) {
        uint32_t at = slot;
        if (lane == 13u || components_lookup(table, a.t.log2_slots, neighbors_key(key, (int)lane), at)) {
            const thin_u64 v = table[at].val;
            nb_start = (uint32_t)(v >> 32);
            nb_count = (v & 0xFFFFFFFFull) + 1ull;
        }
    }
    thin_u64 nb_excl = nb_count;                            // the 27 buckets laid end to end, as in k_neighbors_pairs
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const thin_u64 up = __shfl_up(nb_excl, d, 64);
        if (lane >= (uint32_t)d) nb_excl += up;
    }
    const thin_u64 total = neighbors_uniform(__shfl(nb_excl, 26, 64));
    nb_excl -= nb_count;
    const uint32_t excl_lo = (uint32_t)nb_excl, excl_hi = (uint32_t)(nb_excl >> 32), count_lo = (uint32_t)nb_count, count_hi = (uint32_t)(nb_count >> 32);

    bound += (thin_u64)__popcll(__ballot(valid)) * total;

    int64_t n_in = 0, sx = 0, sy = 0, sz = 0, qxy = 0, qxz = 0, qyz = 0;
    thin_u64 qxx = 0, qyy = 0, qzz = 0;
    for (thin_u64 t0 = 0; t0 < total; t0 += 64u) {
        const int m = (int)min((thin_u64)64u, total - t0);
        const thin_u64 g = t0 + lane;                       // this lane's entry of the tile
        thin_u64 at = ~0ull;
        for (int nb = 0; nb < 27; ++nb) {                   // (every value read here is wave-uniform)
            const thin_u64 e = ((thin_u64)(uint32_t)__builtin_amdgcn_readlane((int)excl_hi, nb) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)excl_lo, nb);
            const thin_u64 c = ((thin_u64)(uint32_t)__builtin_amdgcn_readlane((int)count_hi, nb) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)count_lo, nb);
            if (c == 0ull || e >= t0 + 64u || e + c <= t0) continue;
            const thin_u64 first = (uint32_t)__builtin_amdgcn_readlane((int)nb_start, nb);
            if (g >= e && g - e < c) at = first + (g - e);
        }
        const bool have = lane < (uint32_t)m && at < a.candidates;
        const uint4 tile = have ? a.bucket[at] : make_uint4(0, 0, 0, 0);
        int32_t n32 = 0, sx32 = 0, sy32 = 0, sz32 = 0;      // a tile's share: at most 64, at most 64 * 32767
        uint32_t xx32 = 0, yy32 = 0, zz32 = 0;              // at most 4 squares, each below 2^30
        int32_t xy32 = 0, xz32 = 0, yz32 = 0;               // at most 2 products, each below 2^30 in magnitude
        // entry k of the tile: offsets from the centre, masked to 0 outside the sphere (then every factor fits 16 bits)
#define PCR_MOMENTS_ENTRY(k)                                                                                                              \
        {                                                                                                                                 \
            const int32_t ex = (int32_t)((uint32_t)__builtin_amdgcn_readlane((int)tile.x, (k)) - centre.x);                              \
            const int32_t ey = (int32_t)((uint32_t)__builtin_amdgcn_readlane((int)tile.y, (k)) - centre.y);                              \
            const int32_t ez = (int32_t)((uint32_t)__builtin_amdgcn_readlane((int)tile.z, (k)) - centre.z);                              \
            const thin_u64 d2 = (thin_u64)((int64_t)ex * ex) + (thin_u64)((int64_t)ey * ey) + (thin_u64)((int64_t)ez * ez);             \
            const bool in = d2 <= a.r2;                                                                                                   \
            const int32_t dx = in ? ex : 0, dy = in ? ey : 0, dz = in ? ez : 0;                                                           \
            n32 += in ? 1 : 0; sx32 += dx; sy32 += dy; sz32 += dz;                                                                        \
            xx32 += (uint32_t)__mul24(dx, dx); yy32 += (uint32_t)__mul24(dy, dy); zz32 += (uint32_t)__mul24(dz, dz);                      \
            xy32 += __mul24(dx, dy); xz32 += __mul24(dx, dz); yz32 += __mul24(dy, dz);                                                    \
        }
#define PCR_MOMENTS_FLUSH_MIXED() { qxy += xy32; qxz += xz32; qyz += yz32; xy32 = xz32 = yz32 = 0; }
#define PCR_MOMENTS_FLUSH_SQUARES() { qxx += xx32; qyy += yy32; qzz += zz32; xx32 = yy32 = zz32 = 0u; }
        int k = 0;
        for (; k + 4 <= m; k += 4) {
            PCR_MOMENTS_ENTRY(k) PCR_MOMENTS_ENTRY(k + 1) PCR_MOMENTS_FLUSH_MIXED()
            PCR_MOMENTS_ENTRY(k + 2) PCR_MOMENTS_ENTRY(k + 3) PCR_MOMENTS_FLUSH_MIXED()
            PCR_MOMENTS_FLUSH_SQUARES()
        }
        for (; k < m; ++k) {                                // (at most 3 entries)
            PCR_MOMENTS_ENTRY(k) PCR_MOMENTS_FLUSH_MIXED()
        }
        PCR_MOMENTS_FLUSH_SQUARES()
#undef PCR_MOMENTS_ENTRY
#undef PCR_MOMENTS_FLUSH_MIXED
#undef PCR_MOMENTS_FLUSH_SQUARES
        n_in += n32; sx += sx32; sy += sy32; sz += sz32;
    }
    const bool sparse = valid && (thin_u64)n_in < a.min_count;
    if (valid && centre.w < a.rows) {                       // (k_neighbors_fill wrote every entry: the row is one of the range)
        const thin_u64 row = centre.w;
        pcr_moments rec;
        rec.n = n_in; rec.s[0] = sx; rec.s[1] = sy; rec.s[2] = sz;
        rec.q[0] = (int64_t)qxx; rec.q[1] = qxy; rec.q[2] = qxz; rec.q[3] = (int64_t)qyy; rec.q[4] = qyz; rec.q[5] = (int64_t)qzz;
        if (out_m) {
            uint4 *dst = out_m + row * 5u;
            dst[0] = moments_pack(rec.n, rec.s[0]); dst[1] = moments_pack(rec.s[1], rec.s[2]); dst[2] = moments_pack(rec.q[0], rec.q[1]);
            dst[3] = moments_pack(rec.q[2], rec.q[3]); dst[4] = moments_pack(rec.q[4], rec.q[5]);
        }
        if (out_e) {
            double e[6];
            moments_eigen(rec, e);
            uint4 *dst = out_e + row * 3u;
#pragma unroll
            for (int i = 0; i < 3; ++i) dst[i] = moments_pack(__double_as_longlong(e[2 * i]), __double_as_longlong(e[2 * i + 1]));
        }
        if (!sparse) atomicOr(&a.keep[row >> 6], 1ull << (row & 63u));
    }
    sparse_total += (thin_u64)__popcll(__ballot(sparse));
    }
    if (lane == 0) {
        if (bound) atomicAdd(&a.counters[NEIGHBORS_PAIRS_BOUND + (blockIdx.x & 63u)], bound);
        if (sparse_total) atomicAdd(&a.counters[NEIGHBORS_SPARSE + (blockIdx.x & 63u)], sparse_total);
    }
}

// moments: [n] pcr_moments, eigen: [n] pcr_eigen, both 8-byte aligned
__global__ void __launch_bounds__(256) k_moments_eigen(const int64_t *moments, thin_u64 n, double *eigen)
{
    const thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t *src = moments + i * 10u;
    pcr_moments rec;
    rec.n = src[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) rec.s[k] = src[1 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) rec.q[k] = src[4 + k];
    double e[6];
    moments_eigen(rec, e);
#pragma unroll
    for (int k = 0; k < 6; ++k) eigen[i * 6u + (thin_u64)k] = e[k];
}

// k_neighbors_write gathering the 80-byte and 48-byte records of the written rows from the dense arrays (any of the four outputs
// may be NULL; moments and eigen are 8-byte aligned, so they are stored word by word); write_kept_rows' body written out, see there
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_moments_write(StreamView s, const uint32_t *list, uint32_t first_batch, const thin_u64 *keep,
                                                                      const int64_t *offsets, const thin_u64 *dense_m, const thin_u64 *dense_e,
                                                                      uint4 *points, int64_t *rows, thin_u64 *moments, thin_u64 *eigen)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const thin_u64 word = keep[(size_t)(b - first_batch) * PCR_WORKGROUP_SIZE + tid];
    const uint32_t mine = (uint32_t)__popcll(word);
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_packed_table(s, b, s_table);                       // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    int64_t dst = offsets[blockIdx.x] + before;
    const int64_t end = dst + mine;                         // never past the bits of this chain's word
    const int64_t row0 = (int64_t)(b - first_batch) * PCR_POINTS_PER_BATCH + (int64_t)tid * PCR_POINTS_PER_THREAD;
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        if (((word >> (uint32_t)i) & 1ull) && dst < end) {
            if (points) points[dst] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
            if (rows) rows[dst] = row0 + i;
            if (moments) {
#pragma unroll
                for (int k = 0; k < 10; ++k) moments[dst * 10 + k] = dense_m[(row0 + i) * 10 + k];
            }
            if (eigen) {
#pragma unroll
                for (int k = 0; k < 6; ++k) eigen[dst * 6 + k] = dense_e[(row0 + i) * 6 + k];
            }
            ++dst;
        }
    });
}

// ------------------------------------------------------------------------------------------------
// k nearest neighbours (pcr_knn / pcr_read_knn): per candidate the first k, in the order (d2, row), of the candidates of another row
// within `radius`, as words d2 << 32 | row (radius <= 32767: d2 < 2^30; a call has at most 2^32 rows), all ones behind the last one
// found. The plan is pcr_neighbors' up to the filled buckets (k_neighbors_count / _alloc / _fill above); then
//   k_knn_pairs<K>   k_neighbors_pairs' work distribution (a wave per work item, lane j holds centre j, lanes 0 .. 26 look up one
//                    neighbour voxel each, the 27 buckets laid end to end, read in tiles of 64 and broadcast by lane reads; no LDS,
//                    no barrier), for the least K of 1, 2, 4, 8, 16 that holds k. Per lane best[K], sorted ascending, all ones at
//                    the start; per entry three subtractions, d2, the word, and, where one ballot finds a lane whose word is below
//                    its best[K - 1], an insertion pass over best[] (min / max, unrolled: best[] is indexed with constants only and
//                    stays in VGPRs). d2 is formed in 32 bits from exact 24-bit squares: coordinates of adjacent voxels differ by
//                    at most 2 r - 1 = 65533, so each square is below 2^32 and exact, but the sum of three is not; an entry
//                    counts iff the largest square and the sum are both <= r2 -- with every square <= r2 < 2^30 the sum cannot
//                    wrap. (k_neighbors_pairs' 64-bit multiply-adds would do as well; the 24-bit multiply is the full-rate one.)
//                    No early exit and no pruning of neighbour voxels. A valid lane stores its first k words by row into a dense
//                    array (when asked for) and sets its keep bit iff found >= min_found.
//   k_thin_totals (above) / k_knn_write   k_neighbors_write gathering the k words of the written rows.
// The words of a centre are distinct (rows are), so the first k of them are the same whatever order the entries arrive in.
// ------------------------------------------------------------------------------------------------
#define KNN_NONE (~0ull)

// a.min_count: min_found. out: [a.rows * k] by row, or NULL. 1 <= k <= K.
template <int K>
__global__ void __launch_bounds__(256) k_knn_pairs(NeighborsArgs a, thin_u64 items, int k, thin_u64 *out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r2 = (uint32_t)a.r2;
    thin_u64 bound = 0, sparse_total = 0;                   // this wave's share of pairs_bound and of the sparse candidates
    // (no barrier below: a wave is on its own; it takes every (waves of the grid)-th work item)
    for (thin_u64 wi = neighbors_uniform((thin_u64)blockIdx.x * 4u + (threadIdx.x >> 6)); wi < items; wi += (thin_u64)gridDim.x * 4u) {
    const thin_u64 item = neighbors_uniform(a.work[wi]);
    const uint32_t slot = (uint32_t)(item >> 32), chunk = (uint32_t)item;
    const ThinSlot *table = a.t.table;
    const thin_u64 key = neighbors_uniform(table[slot].key), own = neighbors_uniform(table[slot].val);     // (k_neighbors_alloc's value)
    const thin_u64 count = (own & 0xFFFFFFFFull) + 1ull, own_start = own >> 32;
    const thin_u64 idx = (thin_u64)chunk * 64u + lane;
    const bool valid = idx < count && own_start + idx < a.candidates;
    const uint4 centre = valid ? a.bucket[own_start + idx] : make_uint4(0, 0, 0, 0);

    // lane n < 27: the bucket of neighbour voxel n (13 is the chunk's own); lanes 27 .. 63 hold empty ones
    uint32_t nb_start = 0;
    thin_u64 nb_count = 0;
    if (lane < 27u) {
        uint32_t at = slot;
        if (lane == 13u || components_lookup(table, a.t.log2_slots, neighbors_key(key, (int)lane), at)) {
            const thin_u64 v = table[at].val;
            nb_start = (uint32_t)(v >> 32);
            nb_count = (v & 0xFFFFFFFFull) + 1ull;
        }
    }
    thin_u64 nb_excl = nb_count;                            // the 27 buckets laid end to end, as in k_neighbors_pairs
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const thin_u64 up = __shfl_up(nb_excl, d, 64);
        if (lane >= (uint32_t)d) nb_excl += up;
    }
    const thin_u64 total = neighbors_uniform(__shfl(nb_excl, 26, 64));
    nb_excl -= nb_count;
    const uint32_t excl_lo = (uint32_t)nb_excl, excl_hi = (uint32_t)(nb_excl >> 32), count_lo = (uint32_t)nb_count, count_hi = (uint32_t)(nb_count >> 32);

    bound += (thin_u64)__popcll(__ballot(valid)) * total;

    thin_u64 best[K];
#pragma unroll
    for (int i = 0; i < K; ++i) best[i] = KNN_NONE;
    for (thin_u64 t0 = 0; t0 < total; t0 += 64u) {
        const int m = (int)min((thin_u64)64u, total - t0);
        const thin_u64 g = t0 + lane;                       // this lane's entry of the tile
        thin_u64 at = ~0ull;
        for (int nb = 0; nb < 27; ++nb) {                   // (every value read here is wave-uniform)
            const thin_u64 e = ((thin_u64)(uint32_t)__builtin_amdgcn_readlane((int)excl_hi, nb) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)excl_lo, nb);
            const thin_u64 c = ((thin_u64)(uint32_t)__builtin_amdgcn_readlane((int)count_hi, nb) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)count_lo, nb);
            if (c == 0ull || e >= t0 + 64u || e + c <= t0) continue;
            const thin_u64 first = (uint32_t)__builtin_amdgcn_readlane((int)nb_start, nb);
            if (g >= e && g - e < c) at = first + (g - e);
        }
        const bool have = lane < (uint32_t)m && at < a.candidates;
        const uint4 tile = have ? a.bucket[at] : make_uint4(0, 0, 0, 0);
        for (int e = 0; e < m; ++e) {
            const uint32_t row = (uint32_t)__builtin_amdgcn_readlane((int)tile.w, e);
            const int32_t dx = (int32_t)(centre.x - (uint32_t)__builtin_amdgcn_readlane((int)tile.x, e));
            const int32_t dy = (int32_t)(centre.y - (uint32_t)__builtin_amdgcn_readlane((int)tile.y, e));
            const int32_t dz = (int32_t)(centre.z - (uint32_t)__builtin_amdgcn_readlane((int)tile.z, e));
            // |d| <= 65533 fits 24 bits and its square 32: exact; the sum is exact wherever it is used (every square <= r2 < 2^30)
            const uint32_t xx = (uint32_t)__mul24(dx, dx), yy = (uint32_t)__mul24(dy, dy), zz = (uint32_t)__mul24(dz, dz);
            const uint32_t d2 = xx + yy + zz;
            const bool in = valid && max(max(xx, yy), zz) <= r2 && d2 <= r2 && row != centre.w;
            thin_u64 word = in ? ((thin_u64)d2 << 32) | row : KNN_NONE;
            if (__ballot(word < best[K - 1]) != 0ull) {
#pragma unroll
                for (int i = 0; i < K; ++i) {               // lo = min(best[i], word); word = max(best[i], word): one compare for both
                    const bool below = word < best[i];
                    const thin_u64 lo = below ? word : best[i];
                    word = below ? best[i] : word;
                    best[i] = lo;
                }
            }
        }
    }
    uint32_t found = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) found += (i < k && best[i] != KNN_NONE) ? 1u : 0u;
    const bool sparse = valid && (thin_u64)found < a.min_count;
    if (valid && centre.w < a.rows) {                       // (k_neighbors_fill wrote every entry: the row is one of the range)
        const thin_u64 row = centre.w;
        if (out) {
            thin_u64 *dst = out + row * (thin_u64)k;        // (row < a.rows: inside the array of a.rows * k words)
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i < k) dst[i] = best[i];
        }
        if (!sparse) atomicOr(&a.keep[row >> 6], 1ull << (row & 63u));
    }
    sparse_total += (thin_u64)__popcll(__ballot(sparse));
    }
    if (lane == 0) {
        if (bound) atomicAdd(&a.counters[NEIGHBORS_PAIRS_BOUND + (blockIdx.x & 63u)], bound);
        if (sparse_total) atomicAdd(&a.counters[NEIGHBORS_SPARSE + (blockIdx.x & 63u)], sparse_total);
    }
}

// k_neighbors_write gathering the k words of the written rows from the dense array (any of the three outputs may be NULL)
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_knn_write(StreamView s, const uint32_t *list, uint32_t first_batch, const thin_u64 *keep,
                                                                  const int64_t *offsets, const thin_u64 *dense, int k, uint4 *points, int64_t *rows,
                                                                  thin_u64 *knn)
{
    write_kept_rows<LAYOUT, BC7>(s, list, first_batch, keep, offsets, points, rows, [&](int64_t dst, int64_t row) {
        if (knn) {
            for (int j = 0; j < k; ++j) knn[dst * k + j] = dense[row * k + j];
        }
    });
}

// ------------------------------------------------------------------------------------------------
// Voxel means (pcr_voxel_mean / pcr_read_voxel_mean): one computed record per non-empty voxel -- the mean position, rounded half
// up inside the voxel, and the mean of each colour byte -- with the voxel's least row and its count. pcr_thin's FIRST plan runs
// unchanged and leaves the table (key, least row), the keep bitmap and the records per batch; then
//   k_voxel_prefix   a workgroup per batch that keeps a row: the exclusive prefix of the popcounts of its 1024 keep words, on top
//                    of the batch's first record (from the host, as for k_thin_write): the record index of every chain's first bit.
//   k_voxel_index    a thread per slot: the record index of the voxel's least row -- prefix plus the bits below the row's in its
//                    word -- replaces the row in the slot's value; (key, row) go into the record's entry of `rec`.
//   k_voxel_sum      decode with colours: a lane sums a run's offsets inside the voxel, its length and its colour bytes in
//                    registers, looks the voxel's record up at the end of the run (denoise_lookup: the key is there) and adds the
//                    run into the record's accumulator -- eight 64-bit words, one 64-byte line: S_x, S_y, S_z, n, C_0 .. C_3 --
//                    with atomic adds whose results are not used (a zero byte sum is not added). Sums of integers commute: the
//                    accumulators are exact and the same from run to run.
//   k_voxel_finish   a thread per record of a range of records: the seven roundings (voxel_mean_round, pcr_lattice.h), the
//                    position rebuilt modulo 2^32 from the key's three indices and the shifted lattice, and the stores.
// Limits: an offset is below cell <= 2^30 and a call has at most 2^32 rows (PCR_VOXEL_MEAN_MAX_ROWS), so S < 2^62, C < 2^40 and
// 2 S + n < 2^64. Within a run of at most 64 points an offset sum is below 2^36 and a byte sum below 2^14: two bytes share a
// 32-bit register. No workgroup waits for another one; the probe loop makes at most `slots` steps.
// ------------------------------------------------------------------------------------------------
constexpr int VOXEL_ACC_WORDS = 8;                          // S_x, S_y, S_z, n, C_0, C_1, C_2, C_3
struct VoxelRec { thin_u64 key, row; };

// thin_key, and the point's offset inside its voxel on every axis (each in [0, cell))
__device__ __forceinline__ thin_u64 voxel_mean_key(const ThinArgs &a, int32_t x, int32_t y, int32_t z, uint32_t (&r)[3])
{
    const uint32_t dx = (uint32_t)x - a.lat.origin[0], dy = (uint32_t)y - a.lat.origin[1], dz = (uint32_t)z - a.lat.origin[2];
    const uint32_t vx = grid_div(a.lat.div, dx), vy = grid_div(a.lat.div, dy), vz = grid_div(a.lat.div, dz);
    r[0] = dx - vx * a.lat.cell; r[1] = dy - vy * a.lat.cell; r[2] = dz - vz * a.lat.cell;
    return (thin_u64)vx | ((thin_u64)vy << THIN_KEY_BITS) | ((thin_u64)vz << (2 * THIN_KEY_BITS));
}

// Workgroup x takes list[x], a batch that keeps a row: prefix[(b - first_batch) * 1024 + chain] = offsets[x] + the bits set in
// the keep words of the batch's chains before `chain`
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_voxel_prefix(const uint32_t *list, uint32_t first_batch, const thin_u64 *keep, const int64_t *offsets,
                                                                     thin_u64 *prefix)
{
    const uint32_t b = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ uint32_t s_part[LWC_WAVES];
    const size_t at = (size_t)(b - first_batch) * PCR_WORKGROUP_SIZE + tid;
    const uint32_t mine = (uint32_t)__popcll(keep[at]);
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    __syncthreads();
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    prefix[at] = (thin_u64)offsets[blockIdx.x] + before;
}

// The value of every taken slot: the row becomes the record index of the row's bit in the keep bitmap; rec[index] = (key, row).
// An index that is no record of the call (the bitmap and the table disagree) sets the error word and leaves the slot alone.
__global__ void __launch_bounds__(256) k_voxel_index(ThinSlot *table, thin_u64 slots, const thin_u64 *keep, const thin_u64 *prefix, thin_u64 records,
                                                     VoxelRec *rec, uint32_t *error)
{
    for (thin_u64 i = (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (thin_u64)gridDim.x * blockDim.x) {
        const thin_u64 key = table[i].key;
        if (key == THIN_EMPTY) continue;
        const thin_u64 row = table[i].val & THIN_ROW_MASK;
        const thin_u64 index = prefix[row >> 6] + (thin_u64)__popcll(keep[row >> 6] & ((1ull << (row & 63u)) - 1ull));
        if (index >= records) { *error = 1u; continue; }
        table[i].val = index;
        rec[index].key = key; rec[index].row = row;
    }
}

__device__ __forceinline__ void voxel_add(thin_u64 *p, thin_u64 v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                          // (the result is not used)
}

// Workgroup x takes list[x]: every run of its chains into the accumulator of the run's voxel (acc[index * 8 ..])
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_voxel_sum(StreamView s, const uint32_t *list, ThinArgs a, thin_u64 records, thin_u64 *acc)
{
    const uint32_t b = list[blockIdx.x];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    thin_u64 prev = THIN_EMPTY, sx = 0, sy = 0, sz = 0;
    uint32_t len = 0, c02 = 0, c13 = 0;                     // colour bytes 0 and 2, 1 and 3: two 16-bit sums a register
    auto flush = [&]() {
        bool found;
        const thin_u64 index = denoise_lookup(a.table, a.log2_slots, prev, found);
        if (!found || index >= records) { *a.error = 1u; return; }                     // (k_thin_mark inserted every run's key)
        thin_u64 *v = acc + index * VOXEL_ACC_WORDS;
        voxel_add(v + 0, sx); voxel_add(v + 1, sy); voxel_add(v + 2, sz); voxel_add(v + 3, len);
        if (c02 & 0xFFFFu) voxel_add(v + 4, c02 & 0xFFFFu);
        if (c13 & 0xFFFFu) voxel_add(v + 5, c13 & 0xFFFFu);
        if (c02 >> 16) voxel_add(v + 6, c02 >> 16);
        if (c13 >> 16) voxel_add(v + 7, c13 >> 16);
    };
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        uint32_t r[3];
        const thin_u64 key = in_box(a.q, x, y, z) ? voxel_mean_key(a, x, y, z, r) : THIN_EMPTY;
        if (key != prev) {
            if (prev != THIN_EMPTY) flush();
            prev = key; sx = sy = sz = 0; len = 0; c02 = c13 = 0;
        }
        if (key != THIN_EMPTY) {
            sx += r[0]; sy += r[1]; sz += r[2]; ++len;
            c02 += colour & 0x00FF00FFu; c13 += (colour >> 8) & 0x00FF00FFu;
        }
    });
    if (prev != THIN_EMPTY) flush();
}

// Records [i0, i1) of the call: points[i - i0], rows[i - i0], counts[i - i0] (each may be NULL) from acc and rec
__global__ void __launch_bounds__(256) k_voxel_finish(ThinLattice lat, const thin_u64 *acc, const VoxelRec *rec, thin_u64 i0, thin_u64 i1, uint4 *points,
                                                      int64_t *rows, int64_t *counts, uint32_t *error)
{
    for (thin_u64 i = i0 + (thin_u64)blockIdx.x * blockDim.x + threadIdx.x; i < i1; i += (thin_u64)gridDim.x * blockDim.x) {
        const thin_u64 *v = acc + i * VOXEL_ACC_WORDS;
        const thin_u64 n = v[3];
        if (n == 0) { *error = 1u; continue; }              // (every record's voxel has a run)
        if (points) {
            const thin_u64 key = rec[i].key;
            const uint32_t field = (1u << THIN_KEY_BITS) - 1u;
            const uint32_t vx = (uint32_t)key & field, vy = (uint32_t)(key >> THIN_KEY_BITS) & field, vz = (uint32_t)(key >> (2 * THIN_KEY_BITS)) & field;
            const uint32_t x = lat.origin[0] + vx * lat.cell + (uint32_t)voxel_mean_round(v[0], n);
            const uint32_t y = lat.origin[1] + vy * lat.cell + (uint32_t)voxel_mean_round(v[1], n);
            const uint32_t z = lat.origin[2] + vz * lat.cell + (uint32_t)voxel_mean_round(v[2], n);
            const uint32_t colour = (uint32_t)voxel_mean_round(v[4], n) | ((uint32_t)voxel_mean_round(v[5], n) << 8) |
                                    ((uint32_t)voxel_mean_round(v[6], n) << 16) | ((uint32_t)voxel_mean_round(v[7], n) << 24);
            points[i - i0] = make_uint4(x, y, z, colour);
        }
        if (rows) rows[i - i0] = (int64_t)rec[i].row;
        if (counts) counts[i - i0] = (int64_t)n;
    }
}

// ------------------------------------------------------------------------------------------------
// Screen selection and picking (pcr_select_screen / pcr_read_screen / pcr_pick): the points a frame of the given camera draws,
// with the pixel and the depth bits k_render computes for them -- the identity the framebuffer word (depth << 32 | colour) does
// not carry. All of it is on the decode path; k_render, k_transcode and the prepass are not touched.
//   k_screen_lod    the prepass's decision per batch (lod_prepass_batch with publish = false: culled, points per chain, f64
//                   dequantisation) into an array of the selection's own: a pending pcr_frame_begin keeps its lists, plans and
//                   statistics. The host reads the array and lists the kept batches.
//   k_screen_count  per kept batch: how many of each chain's first npr points pass the inside test and fall into the rect
//   k_screen_write  per kept batch: a workgroup prefix over those 1024 counts, then every chain writes its records and / or
//                   hits consecutively from its offset (k_select_write's scheme; offsets between batches from the host)
//   k_pick_key      per kept batch: 64-bit min of depth << 32 | colour over the window (lane, LDS, then one global atomic)
//   k_pick_index    per kept batch: min of the record index among the window's points that hold that key
//   k_pick_fetch    one workgroup: the winner's record and hit
// No workgroup waits for another; every result is written with vector stores and vector atomics.
// ------------------------------------------------------------------------------------------------
struct ScreenEntry { uint32_t b, lod; };    // a kept batch and its LOD_* word
struct ScreenArgs {
    float m[16];                            // pcr_render_params::transform
    int32_t width, height;
    uint32_t fb_elems;
    int32_t x0, y0, x1, y1;                 // the rect, clipped to the image, never empty
};

// What k_render works out per batch before its point loop (:1378-1381 there): the dequantisation in both precisions.
struct ScreenBatch {
    double sx, sy, sz, ox, oy, oz;
    float fsx, fsy, fsz, fox, foy, foz;
    bool use_double;
};
__device__ __forceinline__ ScreenBatch screen_batch(const StreamView &s, uint32_t b, uint32_t lod)
{
    const pcr_gpu_batch *gb = s.batches + b;
    ScreenBatch B;
    B.sx = gb->scale_x; B.sy = gb->scale_y; B.sz = gb->scale_z;
    B.ox = gb->offset_x - gb->las_min_x; B.oy = gb->offset_y - gb->las_min_y; B.oz = gb->offset_z - gb->las_min_z;
    B.fsx = (float)B.sx; B.fsy = (float)B.sy; B.fsz = (float)B.sz;
    B.fox = (float)B.ox; B.foy = (float)B.oy; B.foz = (float)B.oz;
    B.use_double = (lod & LOD_DOUBLE) != 0;
    return B;
}

// k_render's projection of one point, operation for operation in its plain form (oracle/pcr_oracle.c, sink_raster): the
// dequantisation in the batch's precision, the three dot products in dot4's order, the correctly rounded division k_render's
// reciprocal sequence is bit-identical to (see project_divide there), the inside test that rejects NaNs, the pixel by
// truncation. Every fused operation is spelled out and nothing else may be fused. false: the point is not drawn.
__device__ __forceinline__ bool screen_project(const ScreenArgs &q, const ScreenBatch &B, int32_t x, int32_t y, int32_t z,
                                               int &ix, int &iy, uint32_t &pixel, uint32_t &depth_bits)
{
#pragma clang fp contract(off)
    float fx, fy, fz;
    if (B.use_double) {
        fx = (float)__fma_rn((double)x, B.sx, B.ox);
        fy = (float)__fma_rn((double)y, B.sy, B.oy);
        fz = (float)__fma_rn((double)z, B.sz, B.oz);
    } else {
        fx = __fmaf_rn((float)x, B.fsx, B.fox);
        fy = __fmaf_rn((float)y, B.fsy, B.foy);
        fz = __fmaf_rn((float)z, B.fsz, B.foz);
    }
    const float qx = __fmaf_rn(q.m[3], 1.0f, __fmaf_rn(q.m[2], fz, __fmaf_rn(q.m[1], fy, q.m[0] * fx)));
    const float qy = __fmaf_rn(q.m[7], 1.0f, __fmaf_rn(q.m[6], fz, __fmaf_rn(q.m[5], fy, q.m[4] * fx)));
    const float qw = __fmaf_rn(q.m[15], 1.0f, __fmaf_rn(q.m[14], fz, __fmaf_rn(q.m[13], fy, q.m[12] * fx)));
    const float nx = qx / qw, ny = qy / qw;               // (correctly rounded: no fast-math, see the top of the file)
    if (!(qw > 0.0f && nx >= -1.0f && nx <= 1.0f && ny >= -1.0f && ny <= 1.0f)) return false;
    ix = (int)(__fmaf_rn(nx, 0.5f, 0.5f) * (float)q.width);
    iy = (int)(__fmaf_rn(ny, 0.5f, 0.5f) * (float)q.height);
    const int64_t pix = (int64_t)ix + (int64_t)iy * q.width;
    if (pix < 0 || pix >= (int64_t)q.fb_elems) return false;
    pixel = (uint32_t)pix;
    depth_bits = __float_as_uint(qw);
    return true;
}

// Does the pixel lie in the rect? Column and row are those of the linear index: ndc == 1.0 maps to column `width`, which in
// the framebuffer is column 0 of the next row.
__device__ __forceinline__ bool screen_in_rect(const ScreenArgs &q, int ix, int iy)
{
    const int cx = ix >= q.width ? ix - q.width : ix, cy = ix >= q.width ? iy + 1 : iy;
    return cx >= q.x0 && cx <= q.x1 && cy >= q.y0 && cy <= q.y1;
}

// lod[b] = the prepass's LOD_* word of batch b for the camera of `a` (a.variant_hqs picks the expression): nothing else is written
__global__ void __launch_bounds__(PREPASS_THREADS) k_screen_lod(RenderArgs a, uint32_t *lod)
{
    const int64_t b = ((int64_t)blockIdx.x * PREPASS_THREADS + threadIdx.x) / PREPASS_LANES;
    const int lane = (int)(threadIdx.x % PREPASS_LANES);
    pcr_render_stats st = {0, 0, 0, 0};
    if (b < a.s.num_batches) {                              // (uniform per group of PREPASS_LANES lanes)
        const uint32_t w = lod_prepass_batch(a, b, lane, st, false);
        if (lane == 0) lod[b] = w;
    }
}

// Workgroup x takes list[x]: chain_counts[x * 1024 + chain] = the chain's selected points, totals[x] = their sum
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_screen_count(StreamView s, const ScreenEntry *list, ScreenArgs q, uint32_t *chain_counts, uint32_t *totals)
{
    const ScreenEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    load_packed_table(s, e.b, s_table);
    const ScreenBatch B = screen_batch(s, e.b, e.lod);
    uint32_t cnt = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, e.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t) {
        int ix, iy; uint32_t pixel, depth;
        if (screen_project(q, B, x, y, z, ix, iy, pixel, depth) && screen_in_rect(q, ix, iy)) ++cnt;
    }, (int)(e.lod & LOD_NPR_MASK));
    chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid] = cnt;
    uint32_t sum = cnt;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w];
        totals[blockIdx.x] = t;
    }
}

// Workgroup x takes list[x]: its selected records go to points[offsets[x] ..] and their hits to hits[offsets[x] ..] (either may be
// NULL), chain after chain, each chain's in point order. chain_counts is k_screen_count's for the same list and arguments. A hit
// is {pixel, depth bits, index lo, index hi}: one 16-byte store.
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_screen_write(StreamView s, const ScreenEntry *list, ScreenArgs q, const uint32_t *chain_counts,
                                                                     const int64_t *offsets, uint4 *points, uint4 *hits)
{
    static_assert(sizeof(pcr_screen_hit) == 16, "one dwordx4 store per hit");
    const ScreenEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const uint32_t mine = chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid];
    const uint32_t incl = chain_prefix_in_wave(mine, lane, wave, s_part);
    load_packed_table(s, e.b, s_table);                     // (its barrier publishes s_part as well)
    const uint32_t before = chain_prefix_before(incl, mine, wave, s_part);
    const ScreenBatch B = screen_batch(s, e.b, e.lod);
    const int64_t first = offsets[blockIdx.x] + before;
    const uint64_t index0 = (uint64_t)e.b * PCR_POINTS_PER_BATCH + (uint64_t)tid * PCR_POINTS_PER_THREAD;
    uint32_t k = 0;                                         // never past what k_screen_count counted for this chain
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, e.b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        int ix, iy; uint32_t pixel, depth;
        if (screen_project(q, B, x, y, z, ix, iy, pixel, depth) && screen_in_rect(q, ix, iy) && k < mine) {
            const uint64_t index = index0 + (uint64_t)i;
            if (points) points[first + k] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
            if (hits) hits[first + k] = make_uint4(pixel, depth, (uint32_t)index, (uint32_t)(index >> 32));
            ++k;
        }
    }, (int)(e.lod & LOD_NPR_MASK));
}

// pick[0]: min of depth << 32 | colour over the points of the list's batches in the window; pick[1]: min record index among
// those that hold it (both start as all ones); pick[2..3], pick[4..5]: the winner's record and hit.
constexpr int PICK_WORDS = 6;
constexpr uint64_t PICK_NONE = ~0ull;

template <int LAYOUT, bool BC7, bool INDEX_PASS>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_pick(StreamView s, const ScreenEntry *list, ScreenArgs q, unsigned long long *pick)
{
    const ScreenEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ unsigned long long s_best;
    const uint64_t key_wanted = INDEX_PASS ? pick[0] : 0;
    if (INDEX_PASS && key_wanted == PICK_NONE) return;      // (uniform) the window is empty
    if (tid == 0) s_best = PICK_NONE;
    load_packed_table(s, e.b, s_table);                     // (its barrier publishes s_best as well)
    const ScreenBatch B = screen_batch(s, e.b, e.lod);
    const uint64_t index0 = (uint64_t)e.b * PCR_POINTS_PER_BATCH + (uint64_t)tid * PCR_POINTS_PER_THREAD;
    uint64_t best = PICK_NONE;
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, e.b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        int ix, iy; uint32_t pixel, depth;
        if (screen_project(q, B, x, y, z, ix, iy, pixel, depth) && screen_in_rect(q, ix, iy)) {
            const uint64_t key = ((uint64_t)depth << 32) | colour;
            if (!INDEX_PASS) best = min(best, key);
            else if (key == key_wanted) best = min(best, index0 + (uint64_t)i);
        }
    }, (int)(e.lod & LOD_NPR_MASK));
    if (best != PICK_NONE) atomicMin(&s_best, (unsigned long long)best);
    __syncthreads();
    if (tid == 0 && s_best != PICK_NONE) atomicMin(&pick[INDEX_PASS ? 1 : 0], s_best);
}

// One workgroup: the record and the hit of point pick[1] (nothing if there is none). lod: k_screen_lod's array.
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_pick_fetch(StreamView s, const uint32_t *lod, ScreenArgs q, unsigned long long *pick)
{
    const uint64_t winner = pick[1];
    if (winner == PICK_NONE) return;                        // (uniform)
    const uint32_t b = (uint32_t)(winner / PCR_POINTS_PER_BATCH), tid = threadIdx.x;
    if ((int64_t)b >= s.num_batches) return;
    const uint32_t w = lod[b];
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, b, s_table);
    const ScreenBatch B = screen_batch(s, b, w);
    const uint64_t index0 = (uint64_t)b * PCR_POINTS_PER_BATCH + (uint64_t)tid * PCR_POINTS_PER_THREAD;
    uint4 *const out = reinterpret_cast<uint4 *>(pick + 2);
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        int ix, iy; uint32_t pixel, depth;
        if (index0 + (uint64_t)i == winner && screen_project(q, B, x, y, z, ix, iy, pixel, depth)) {
            out[0] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
            out[1] = make_uint4(pixel, depth, (uint32_t)winner, (uint32_t)(winner >> 32));
        }
    }, (int)(w & LOD_NPR_MASK));
}

// ------------------------------------------------------------------------------------------------
// Visible selection (pcr_select_visible / pcr_read_visible): of pcr_select_screen's hits those that make up the picture. Per-pixel
// planes over the image (width * height words each, scratch of the context) take the place of a sort of the hits by pixel:
//   k_visible_key     per kept batch: 64-bit min of depth << 32 | colour of every hit into its pixel's word of the key plane
//                     (every hit of the image, whatever the rect). A chain's consecutive hits of one pixel are merged in
//                     registers, and the word is read before the atomic, which is skipped when it cannot lower the word.
//   k_visible_dilate  rows, then columns: min of the keys' high halves over +-radius pixels, clipped to the image (the min over
//                     a square window separates exactly) -- the depth plane Dr the surface test reads
//   k_visible_index   FRONT only, per kept batch: min of the record index among the rect's hits that hold their pixel's key
//   k_visible_count / k_visible_write   k_screen_count / k_screen_write with the extra predicate: the surface test
//                     (double)w <= (double)dr * 1.01 (the HQS colour pass's rule), and for FRONT index == the pixel's index word
// Hits of the framebuffer's extra row (pixel >= width * height, which screen_project admits) touch no plane and are in no rect.
// No workgroup waits for another; every result is written with vector stores and vector atomics.
// ------------------------------------------------------------------------------------------------
constexpr uint64_t VIS_NONE = ~0ull;
constexpr int VIS_DILATE_THREADS = 256;

// *word = min(*word, v). The word only ever falls during a pass, so one read as <= v already makes the atomic a no-op: skipped.
__device__ __forceinline__ void visible_min(unsigned long long *word, uint64_t v)
{
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(word, (unsigned long long)v);
}

// The HQS colour pass's 1 % rule (k_render_color): an f64 product, not 1.01f. dr = 0xFFFFFFFF (no hit near) is a NaN: false.
__device__ __forceinline__ bool visible_surface(uint32_t depth_bits, uint32_t dr_bits)
{
    return (double)__uint_as_float(depth_bits) <= (double)__uint_as_float(dr_bits) * 1.01;
}

// Workgroup x takes list[x]: the key of every hit into key_plane; hit_totals[x] = the batch's hits inside the image
template <int LAYOUT, int COLOUR>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_visible_key(StreamView s, const ScreenEntry *list, ScreenArgs q, unsigned long long *key_plane,
                                                                    uint32_t *hit_totals)
{
    const ScreenEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    load_packed_table(s, e.b, s_table);
    const ScreenBatch B = screen_batch(s, e.b, e.lod);
    const uint32_t npix = (uint32_t)q.width * (uint32_t)q.height, no_pixel = ~0u;
    uint32_t cnt = 0, run_pixel = no_pixel;                 // the run: the chain's latest hits, all of one pixel
    uint64_t run_key = VIS_NONE;
    decode_chain<LAYOUT, COLOUR>(s, e.b, s_table, [&](int, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        int ix, iy; uint32_t pixel, depth;
        if (!screen_project(q, B, x, y, z, ix, iy, pixel, depth) || pixel >= npix) return;
        ++cnt;
        const uint64_t key = ((uint64_t)depth << 32) | colour;
        if (pixel == run_pixel) { run_key = min(run_key, key); return; }
        if (run_pixel != no_pixel) visible_min(key_plane + run_pixel, run_key);
        run_pixel = pixel; run_key = key;
    }, (int)(e.lod & LOD_NPR_MASK));
    if (run_pixel != no_pixel) visible_min(key_plane + run_pixel, run_key);
    uint32_t sum = cnt;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[w];
        hit_totals[blockIdx.x] = t;
    }
}

// ROW: out[p] = min of the high halves of key_plane over the columns within `radius` of p's, in p's row; *covered += the pixels
// that hold a key. !ROW: out[p] = min of in[] over the rows within `radius` of p's, in p's column.
template <bool ROW>
__global__ void __launch_bounds__(VIS_DILATE_THREADS) k_visible_dilate(const unsigned long long *key_plane, const uint32_t *in, uint32_t *out, int32_t width,
                                                                       int32_t height, int32_t radius, unsigned long long *covered)
{
    const int64_t npix = (int64_t)width * height;
    uint32_t mine = 0;
    for (int64_t p = (int64_t)blockIdx.x * VIS_DILATE_THREADS + threadIdx.x; p < npix; p += (int64_t)gridDim.x * VIS_DILATE_THREADS) {
        const int32_t x = (int32_t)(p % width), y = (int32_t)(p / width);
        uint32_t m = 0xFFFFFFFFu;
        if (ROW) {
            const int32_t c0 = max(x - radius, 0), c1 = min(x + radius, width - 1);
            for (int32_t c = c0; c <= c1; ++c) m = min(m, (uint32_t)(key_plane[p - x + c] >> 32));
            if (key_plane[p] != VIS_NONE) ++mine;
        } else {
            const int32_t r0 = max(y - radius, 0), r1 = min(y + radius, height - 1);
            for (int32_t r = r0; r <= r1; ++r) m = min(m, in[(int64_t)r * width + x]);
        }
        out[p] = m;
    }
    if (ROW) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(covered, (unsigned long long)mine);
    }
}

// Workgroup x takes list[x]: index_plane[pixel] = min record index among the rect's hits whose key is the pixel's key word
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_visible_index(StreamView s, const ScreenEntry *list, ScreenArgs q, const unsigned long long *key_plane,
                                                                      unsigned long long *index_plane)
{
    const ScreenEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    load_packed_table(s, e.b, s_table);
    const ScreenBatch B = screen_batch(s, e.b, e.lod);
    const uint32_t npix = (uint32_t)q.width * (uint32_t)q.height;
    const uint64_t index0 = (uint64_t)e.b * PCR_POINTS_PER_BATCH + (uint64_t)tid * PCR_POINTS_PER_THREAD;
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, e.b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        int ix, iy; uint32_t pixel, depth;
        if (!screen_project(q, B, x, y, z, ix, iy, pixel, depth) || !screen_in_rect(q, ix, iy) || pixel >= npix) return;
        if (key_plane[pixel] == (((uint64_t)depth << 32) | colour)) visible_min(index_plane + pixel, index0 + (uint64_t)i);
    }, (int)(e.lod & LOD_NPR_MASK));
}

// Is hit (pixel, depth) of record `index`, which lies in the rect, selected? front: PCR_VISIBLE_FRONT, else PCR_VISIBLE_SURFACE.
__device__ __forceinline__ bool visible_selected(bool front, const uint32_t *depth_plane, const unsigned long long *index_plane, uint32_t pixel,
                                                 uint32_t depth, uint64_t index)
{
    if (!visible_surface(depth, depth_plane[pixel])) return false;
    return !front || index_plane[pixel] == index;
}

// Workgroup x takes list[x]: chain_counts[x * 1024 + chain] = the chain's selected hits, totals[2 x] = their sum, totals[2 x + 1]
// = the batch's hits in the rect (the candidates)
template <int LAYOUT>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_visible_count(StreamView s, const ScreenEntry *list, ScreenArgs q, bool front, const uint32_t *depth_plane,
                                                                      const unsigned long long *index_plane, uint32_t *chain_counts, uint32_t *totals)
{
    const ScreenEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[2][LWC_WAVES];
    load_packed_table(s, e.b, s_table);
    const ScreenBatch B = screen_batch(s, e.b, e.lod);
    const uint32_t npix = (uint32_t)q.width * (uint32_t)q.height;
    const uint64_t index0 = (uint64_t)e.b * PCR_POINTS_PER_BATCH + (uint64_t)tid * PCR_POINTS_PER_THREAD;
    uint32_t cnt = 0, cand = 0;
    decode_chain<LAYOUT, SEL_NO_COLOUR>(s, e.b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t) {
        int ix, iy; uint32_t pixel, depth;
        if (!screen_project(q, B, x, y, z, ix, iy, pixel, depth) || !screen_in_rect(q, ix, iy) || pixel >= npix) return;
        ++cand;
        if (visible_selected(front, depth_plane, index_plane, pixel, depth, index0 + (uint64_t)i)) ++cnt;
    }, (int)(e.lod & LOD_NPR_MASK));
    chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid] = cnt;
    uint32_t sum = cnt, sum_cand = cand;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sum += __shfl_xor(sum, d, 64); sum_cand += __shfl_xor(sum_cand, d, 64); }
    if (lane == 0) { s_part[0][wave] = sum; s_part[1][wave] = sum_cand; }
    __syncthreads();
    if (tid < 2) {
        uint32_t t = 0;
        for (int w = 0; w < LWC_WAVES; ++w) t += s_part[tid][w];
        totals[2 * (size_t)blockIdx.x + tid] = t;
    }
}

// Workgroup x takes list[x]: k_screen_write for the selected hits (chain_counts: k_visible_count's for the same arguments)
template <int LAYOUT, bool BC7>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE) k_visible_write(StreamView s, const ScreenEntry *list, ScreenArgs q, bool front, const uint32_t *depth_plane,
                                                                      const unsigned long long *index_plane, const uint32_t *chain_counts, const int64_t *offsets,
                                                                      uint4 *points, uint4 *hits)
{
    const ScreenEntry e = list[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ __align__(16) uint32_t s_table[PCR_HUFFMAN_TABLE_SIZE];
    __shared__ uint32_t s_part[LWC_WAVES];
    const uint32_t mine = chain_counts[(size_t)blockIdx.x * PCR_WORKGROUP_SIZE + tid];
    uint32_t incl = mine;                                   // chain_prefix_in_wave spelled out: on it <POINT_WINDOWS, false> compiles to another stream
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) s_part[wave] = incl;
    load_packed_table(s, e.b, s_table);                     // (its barrier publishes s_part as well)
    uint32_t before = incl - mine;
    for (uint32_t w = 0; w < wave; ++w) before += s_part[w];
    const ScreenBatch B = screen_batch(s, e.b, e.lod);
    const uint32_t npix = (uint32_t)q.width * (uint32_t)q.height;
    const int64_t first = offsets[blockIdx.x] + before;
    const uint64_t index0 = (uint64_t)e.b * PCR_POINTS_PER_BATCH + (uint64_t)tid * PCR_POINTS_PER_THREAD;
    uint32_t k = 0;                                         // never past what k_visible_count counted for this chain
    decode_chain<LAYOUT, BC7 ? SEL_BC7 : SEL_BC1>(s, e.b, s_table, [&](int i, int32_t x, int32_t y, int32_t z, uint32_t colour) {
        int ix, iy; uint32_t pixel, depth;
        if (!screen_project(q, B, x, y, z, ix, iy, pixel, depth) || !screen_in_rect(q, ix, iy) || pixel >= npix || k >= mine) return;
        const uint64_t index = index0 + (uint64_t)i;
        if (!visible_selected(front, depth_plane, index_plane, pixel, depth, index)) return;
        if (points) points[first + k] = make_uint4((uint32_t)x, (uint32_t)y, (uint32_t)z, colour);
        if (hits) hits[first + k] = make_uint4(pixel, depth, (uint32_t)index, (uint32_t)(index >> 32));
        ++k;
    }, (int)(e.lod & LOD_NPR_MASK));
}

// ------------------------------------------------------------------------------------------------
// 10-10-10 path ("loop_las_cuda", modules/compute_loop_las_cuda/render.cu:130-442)
//
// Streaming kernel: one workgroup per batch of 65 536 points, thread t takes the point quads t, t+1024, ... so every
// level buffer is read with 16-byte-per-lane loads (the reference's USE_PREFETCH uint4 idea, render.cu:204-327; the
// point -> thread mapping is free because the result is a min over all points). Level 2..4 batches read 4 B per
// point, level 1 reads 8 B, level 0 reads 12 B. Scatter uses the same LDS framebuffer window as the Huffman kernel.
// ------------------------------------------------------------------------------------------------
struct LasView {
    const pcr_xyz_batch *batches;
    const uint32_t *xyz12, *xyz8, *xyz4;
    int64_t num_batches;
};

struct LasArgs {
    pcr_render_params p;
    LasView s;
    FrameView f;
    int32_t *level;           // [nB] -1 culled, 0 / 1 / 2..4
    uint2 *win;               // [nB]
    pcr_render_stats *stats;
    int win_capacity;
    // dense list of the batches k_las_render draws (not culled, not the last one), compacted by the prepass per workgroup of
    // LAS_PREPASS_BATCHES batches in the file's order, as the Huffman methods' lists are (RenderArgs::order): order[wg * 256 ..],
    // chunk_count[wg]; workgroup x of k_las_render / k_las_render_color finds the x-th entry with a wave-wide prefix sum over the
    // chunk counts (las_list_batch)
    uint32_t *order;          // [chunks * LAS_PREPASS_BATCHES]
    uint32_t *chunk_count;    // [LAS_CLASSES][chunks]
    uint32_t chunks;
    // loop_las_hqs (k_las_render_color): the prepass plans a second rectangle per batch for the colour window's 20-byte pixels
    // (NULL: the basic method, nothing planned); the kernel reads the points' colours
    uint2 *win_hqs;           // [nB]
    int win_capacity_hqs;
    const uint32_t *rgba_points;
};
constexpr int LAS_PREPASS_BATCHES = PREPASS_THREADS;     // one lane per batch
// Heaviest first, as the Huffman lists' classes (RenderArgs::work_classes): class 0 = batches whose screen rectangle the LDS window does
// not hold (a batch of a tile-ordered cloud that straddles the end of one row of tiles and the start of the next: every point then
// goes through a global pre-read and a global atomic, 4-6 x the time of a batch with a window -- a few dozen of them in a frame, and
// drawn where the file has them they end the launch alone on their CUs: 0.23 ms where the wave lifetimes sum to 0.11), class 1 = the rest.
// A chunk's records are stored class after class, chunk_count[class][chunk] counts them.
constexpr int LAS_CLASSES = 2;

// (*partial: the rectangle had to be cut down to the capacity, or the batch gets no window at all although it is on screen -- its
// points, or many of them, take the global path)
__device__ __forceinline__ uint2 window_rect(const pcr_render_params &p, const float *bmin, const float *bmax, int capacity, bool *partial = nullptr)
{
    if (partial) *partial = true;
    float minx = 3.0e38f, maxx = -3.0e38f, miny = 3.0e38f, maxy = -3.0e38f;
    const float fw = (float)p.width, fh = (float)p.height;
    for (int c = 0; c < 8; ++c) {
        const float x = (c & 1) ? bmax[0] : bmin[0], y = (c & 2) ? bmax[1] : bmin[1], z = (c & 4) ? bmax[2] : bmin[2];
        const float w = dot4(p.transform + 12, x, y, z, 1.0f);
        if (!(w > 1.0e-6f)) return make_uint2(0, 0);
        const float sx = (dot4(p.transform + 0, x, y, z, 1.0f) / w * 0.5f + 0.5f) * fw;
        const float sy = (dot4(p.transform + 4, x, y, z, 1.0f) / w * 0.5f + 0.5f) * fh;
        minx = fminf(minx, sx); maxx = fmaxf(maxx, sx); miny = fminf(miny, sy); maxy = fmaxf(maxy, sy);
    }
    if (!(maxx >= -1.0f && maxy >= -1.0f && minx <= fw + 1.0f && miny <= fh + 1.0f)) return make_uint2(0, 0);
    int x0 = max(0, (int)floorf(fmaxf(minx, -2.0f)) - 1), x1 = min(p.width - 1, (int)floorf(fminf(maxx, fw + 2.0f)) + 1);
    int y0 = max(0, (int)floorf(fmaxf(miny, -2.0f)) - 1), y1 = min(p.height - 1, (int)floorf(fminf(maxy, fh + 2.0f)) + 1);
    int ww = x1 - x0 + 1, wh = y1 - y0 + 1;
    if (partial && ww > 0 && wh > 0 && (int64_t)ww * wh <= capacity) *partial = false;      // the whole rectangle fits
    if (ww > 0 && wh > 0 && (int64_t)ww * wh > capacity && (int64_t)ww * wh <= 16 * (int64_t)capacity) {
        const float sc = sqrtf((float)capacity / ((float)ww * (float)wh));
        const int nw = max(1, (int)floorf((float)ww * sc)), nh = max(1, (int)floorf((float)wh * sc));
        x0 += (ww - nw) / 2; y0 += (wh - nh) / 2; ww = nw; wh = nh;
    }
    if (ww > 0 && wh > 0 && ww * wh <= capacity && x0 < 65536 && y0 < 65536)
        return make_uint2((uint32_t)x0 | ((uint32_t)y0 << 16), (uint32_t)ww | ((uint32_t)wh << 16));
    return make_uint2(0, 0);
}

__device__ __forceinline__ void las_prepass_batch(const LasArgs &a, int64_t b, pcr_render_stats &st, bool *heavy);

__global__ void __launch_bounds__(PREPASS_THREADS) k_las_prepass(LasArgs a)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    pcr_render_stats st = {0, 0, 0, 0};
    uint32_t cls = LAS_CLASSES;                                             // not drawn
    if (b < a.s.num_batches) {
        bool heavy = false;
        las_prepass_batch(a, b, st, &heavy);
        if (a.level[b] >= 0 && b != a.s.num_batches - 1) cls = heavy ? 0u : 1u;      // render.cu:153-155, :201-202
    }
    commit_stats(st, a.stats, blockIdx.x);
    // compaction of the batches to draw, order preserving inside a class: a ballot per wave and class, the waves' counts through LDS
    __shared__ uint32_t s_wave_count[LAS_CLASSES][PREPASS_THREADS / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)LAS_CLASSES; ++k) {
        const uint64_t m = __ballot(cls == k);
        if (lane == 0) s_wave_count[k][wave] = (uint32_t)__popcll(m);
        if (cls == k) mine = m;
    }
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)LAS_CLASSES; ++k) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t w = 0; w < PREPASS_THREADS / 64; ++w) { if (k == cls && w < wave) base += s_wave_count[k][w]; total += s_wave_count[k][w]; }
        if (k < cls) base += total;                                         // my chunk's records of the classes in front of mine
        if (threadIdx.x == 0) a.chunk_count[k * a.chunks + blockIdx.x] = total;
    }
    if (cls < (uint32_t)LAS_CLASSES) a.order[(size_t)blockIdx.x * LAS_PREPASS_BATCHES + base + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull))] = (uint32_t)b;
}

__device__ __forceinline__ void las_prepass_batch(const LasArgs &a, int64_t b, pcr_render_stats &st, bool *heavy)
{
    const pcr_xyz_batch g = a.s.batches[b];
    const pcr_render_params &p = a.p;
    const float bmin[3] = { g.min_x, g.min_y, g.min_z }, bmax[3] = { g.max_x, g.max_y, g.max_z };
    st.batches_total += 1;
    if (p.enable_frustum_culling) {                                          // render.cu:153-155
        const float *M = p.transform;
#define T(i) M[((i) % 4) * 4 + ((i) / 4)]
        bool in = plane_accepts(T(3) - T(0), T(7) - T(4), T(11) - T(8),  T(15) - T(12), bmin, bmax)
               && plane_accepts(T(3) + T(0), T(7) + T(4), T(11) + T(8),  T(15) + T(12), bmin, bmax)
               && plane_accepts(T(3) + T(1), T(7) + T(5), T(11) + T(9),  T(15) + T(13), bmin, bmax)
               && plane_accepts(T(3) - T(1), T(7) - T(5), T(11) - T(9),  T(15) - T(13), bmin, bmax)
               && plane_accepts(T(3) - T(2), T(7) - T(6), T(11) - T(10), T(15) - T(14), bmin, bmax)
               && plane_accepts(T(3) + T(2), T(7) + T(6), T(11) + T(10), T(15) + T(14), bmin, bmax);
#undef T
        if (!in) {
            a.level[b] = -1;
            st.batches_culled += 1;
            return;
        }
    }
    // :157-197
    const float cx = 0.5f * (bmin[0] + bmax[0]), cy = 0.5f * (bmin[1] + bmax[1]), cz = 0.5f * (bmin[2] + bmax[2]);
    const float dx = bmin[0] - bmax[0], dy = bmin[1] - bmax[1], dz = bmin[2] - bmax[2];
    const float rad = sqrtf(__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx)));
    float vc[4], ve[4], pc[4], pe[4];
    for (int r = 0; r < 4; ++r) vc[r] = dot4(p.world_view + 4 * r, cx, cy, cz, 1.0f);
    ve[0] = vc[0] + rad; ve[1] = vc[1] + 0.0f; ve[2] = vc[2] + 0.0f; ve[3] = vc[3] + 0.0f;
    for (int r = 0; r < 4; ++r) {
        pc[r] = dot4(p.proj + 4 * r, vc[0], vc[1], vc[2], vc[3]);
        pe[r] = dot4(p.proj + 4 * r, ve[0], ve[1], ve[2], ve[3]);
    }
    const float fw = (float)p.width, fh = (float)p.height;
    const float scx = fw * (0.5f * (pc[0] / pc[3] + 1.0f)), scy = fh * (0.5f * (pc[1] / pc[3] + 1.0f));
    const float sex = fw * (0.5f * (pe[0] / pe[3] + 1.0f)), sey = fh * (0.5f * (pe[1] / pe[3] + 1.0f));
    const float ddx = sex - scx, ddy = sey - scy;
    const float px = sqrtf(__fmaf_rn(ddy, ddy, ddx * ddx));
    a.level[b] = px < 100.0f ? 4 : px < 200.0f ? 3 : px < 500.0f ? 2 : px < 10000.0f ? 1 : 0;
    if (b != a.s.num_batches - 1)                                            // the last workgroup returns early (:201-202)
        st.points_iterated += PCR_POINTS_PER_BATCH;
    a.win[b] = window_rect(p, bmin, bmax, a.win_capacity, heavy);
    if (a.win_hqs) a.win_hqs[b] = window_rect(p, bmin, bmax, a.win_capacity_hqs);
}

// Which batch is the blockIdx.x-th of the prepass's list (false: none)? Every wave for itself: a 64-lane inclusive prefix sum over
// the chunk counts. The list walk of k_las_render and k_las_render_color.
__device__ __forceinline__ bool las_list_batch(const LasArgs &a, uint32_t &b)
{
    const uint32_t lane = threadIdx.x & 63u;
    // Heaviest class first only while it is a minority (a few stragglers among batches with windows: started first, they run beside
    // everything else). A frame made of such batches (a close-up: every batch larger on screen than its window) is bound by its
    // global atomics, and drawn class by class it was 18 % slower than in the file's order -- then the chunks are walked in order.
    uint32_t heavy_total = 0, all_total = 0;
    for (uint32_t c0 = 0; c0 < a.chunks; c0 += 64) {                    // (uniform)
        uint32_t h = c0 + lane < a.chunks ? a.chunk_count[c0 + lane] : 0u, l = c0 + lane < a.chunks ? a.chunk_count[a.chunks + c0 + lane] : 0u;
        h = wave_read_lane(wave_inclusive_sum(h), 63); l = wave_read_lane(wave_inclusive_sum(l), 63);
        heavy_total += h; all_total += h + l;
    }
    const bool by_class = heavy_total * 4u < all_total;
    static_assert(LAS_CLASSES == 2, "heavy / light");
    uint32_t x = blockIdx.x, found = 0xFFFFFFFFu;
    for (uint32_t cls = 0; cls < (by_class ? 2u : 1u) && found == 0xFFFFFFFFu; ++cls) {       // (uniform)
        uint32_t before = 0;
        for (uint32_t c0 = 0; c0 < a.chunks; c0 += 64) {                // (uniform)
            const uint32_t c = c0 + lane;
            // by class: the chunk's records of this class; in the file's order: all of the chunk's records (heavy ones first inside it)
            const uint32_t cnt = c < a.chunks ? (by_class ? a.chunk_count[cls * a.chunks + c] : a.chunk_count[c] + a.chunk_count[a.chunks + c]) : 0u;
            const uint32_t incl = wave_inclusive_sum(cnt);
            const uint32_t total = wave_read_lane(incl, 63);
            if (x < before + total) {
                const uint64_t m = __ballot(before + incl > x);
                const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1u;
                const uint32_t excl = wave_read_lane(incl - cnt, first);
                const uint32_t lighter = by_class && cls == 1u ? a.chunk_count[c0 + first] : 0u;      // the chunk's heavy records lie in front
                found = (c0 + first) * LAS_PREPASS_BATCHES + lighter + (x - before - excl);
                break;
            }
            before += total;
        }
        x -= before;                                                    // (not found: `before` is the class's total)
    }
    found = __builtin_amdgcn_readfirstlane(found);
    if (found == 0xFFFFFFFFu) return false;                             // the grid is sized for "every batch drawn"
    b = a.order[found];
    return true;
}

// ------------------------------------------------------------------------------------------------
// What the two 10-10-10 kernels share (k_las_render, k_las_render_color): the batch set-up, the walk over its points and their
// projection, so that both passes of loop_las_hqs see identical positions.
// ------------------------------------------------------------------------------------------------
struct ProjRows { float m00, m01, m02, m03, m10, m11, m12, m13, m30, m31, m32, m33; };   // rows x, y and w of the matrix
struct Projection {
    uint64_t cand;      // lanes whose point is inside the frustum, as a 64-bit lane mask (a scalar register pair)
    float w;            // the point's depth
    int ix, iy;         // its pixel (computed by every lane: garbage for a lane that is not in `cand`)
};

// First half of rasterize() (render.cu:108-118), as in k_render: the three dot products and the inside test without dividing
// (for finite w > 0 the correctly rounded quotient lies in [-1,1] exactly when |x| <= w), then the division: the IEEE sequence
// hipcc emits for `/` with its range scaling removed, shared reciprocal, x and y packed -- bit-identical to `/` for w in
// [2^-64, 2^64). A wave in which some candidate's w lies outside that range (or is 0) takes `/` for all lanes.
__device__ __forceinline__ Projection project_point(const ProjRows &m, float fw, float fh, float x, float y, float z)
{
    Projection p;
    const float qx = __fmaf_rn(m.m03, 1.0f, __fmaf_rn(m.m02, z, __fmaf_rn(m.m01, y, m.m00 * x)));
    const float qy = __fmaf_rn(m.m13, 1.0f, __fmaf_rn(m.m12, z, __fmaf_rn(m.m11, y, m.m10 * x)));
    const float qw = __fmaf_rn(m.m33, 1.0f, __fmaf_rn(m.m32, z, __fmaf_rn(m.m31, y, m.m30 * x)));
    p.cand = __builtin_amdgcn_ballot_w64(fabsf(qx) <= qw) & __builtin_amdgcn_ballot_w64(fabsf(qy) <= qw);
    {
        const float r0 = __builtin_amdgcn_rcpf(qw);
        const float r1 = __fmaf_rn(__fmaf_rn(-qw, r0, 1.0f), r0, r0);
        const v2f xy = {qx, qy}, rr = {r1, r1}, nw = {-qw, -qw};
        const v2f q0 = xy * rr;
        const v2f q1 = __builtin_elementwise_fma(__builtin_elementwise_fma(nw, q0, xy), rr, q0);
        const v2f q2 = __builtin_elementwise_fma(__builtin_elementwise_fma(nw, q1, xy), rr, q1);
        const v2f half = {0.5f, 0.5f}, size = {fw, fh};
        const v2f img = __builtin_elementwise_fma(q2, half, half) * size;
        p.ix = (int)img.x; p.iy = (int)img.y;
    }
    const uint64_t w_ok_mask = __builtin_amdgcn_ballot_w64((__float_as_uint(qw) - 0x1F800000u) < 0x40000000u);   // 2^-64 <= w < 2^64
    if (__builtin_expect((p.cand & ~w_ok_mask) != 0, 0)) {              // (uniform, practically never) the plain `/` for all lanes
        const float nx = qx / qw, ny = qy / qw;
        p.ix = (int)(__fmaf_rn(nx, 0.5f, 0.5f) * fw);
        p.iy = (int)(__fmaf_rn(ny, 0.5f, 0.5f) * fh);
        p.cand &= __builtin_amdgcn_ballot_w64(qw > 0.0f);               // (w == 0 with x == y == 0 passes |x| <= w: rasterize rejects w <= 0, :113)
    }
    p.w = qw;
    return p;
}

struct LasBatch {
    int level;                          // 0 / 1 / 2..4: 12 / 8 / 4 bytes per point
    float sx, sy, sz, ox, oy, oz;       // dequantisation: x = X * sx + ox
    ProjRows m;
    float fw, fh;
    size_t base;                        // the batch's first point
    const uint4 *q4, *q8, *q12;         // its level arrays
};

// The set-up of batch b at level `level` (read by the kernel at its start)
__device__ __forceinline__ LasBatch las_batch(const LasArgs &a, uint32_t b, int level)
{
    LasBatch L;
    L.level = level;
    const pcr_xyz_batch g = a.s.batches[b];
    const float div = level >= 2 ? 1024.0f : 1073741824.0f;                  // STEPS_10BIT / STEPS_30BIT
    L.sx = (g.max_x - g.min_x) / div; L.sy = (g.max_y - g.min_y) / div; L.sz = (g.max_z - g.min_z) / div;   // :145, :345
    L.ox = g.min_x; L.oy = g.min_y; L.oz = g.min_z;
    // (the w row of the matrix in vector registers, as in k_render: a v_fma_f32 whose operands are all VGPRs issues in ~2.3 cycles,
    // with an SGPR operand in ~4.2; the x and y rows run as packed operations with scalar pairs)
    auto in_vgpr = [](float v) { float r; asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(v)); return r; };
    const float *M = a.p.transform;
    L.m = { M[0], M[1], M[2], M[3], M[4], M[5], M[6], M[7], in_vgpr(M[12]), in_vgpr(M[13]), in_vgpr(M[14]), in_vgpr(M[15]) };
    L.fw = (float)a.p.width; L.fh = (float)a.p.height;
    L.base = (size_t)b * PCR_POINTS_PER_BATCH;
    L.q4 = reinterpret_cast<const uint4 *>(a.s.xyz4 + L.base);
    L.q8 = reinterpret_cast<const uint4 *>(a.s.xyz8 + L.base);
    L.q12 = reinterpret_cast<const uint4 *>(a.s.xyz12 + L.base);
    return L;
}

// The batch's points: thread t takes the quads t, t + 1024, ..., read with 16-byte loads from the level's one to three arrays,
// the next quad in flight while this one is projected. Per quad, quad_fn(quad) runs first -- in front of the next quad's loads --
// and its result goes to point_fn(projection, result, j) for the quad's points j = 0..3 in turn.
template <typename QuadFn, typename PointFn>
__device__ __forceinline__ void las_points(const LasBatch &L, QuadFn quad_fn, PointFn point_fn)
{
    const uint32_t tid = threadIdx.x;
    // One copy of the loop per number of level arrays read (4 / 8 / 12 bytes per point): the copy that reads one array does not
    // carry the registers of the other two (with one loop for all three, the 64-register budget of eight waves per SIMD spilled).
    auto quads = [&](auto arrays_) __attribute__((always_inline)) {
        constexpr int ARRAYS = decltype(arrays_)::value;
        uint4 n4 = L.q4[tid], n8 = make_uint4(0, 0, 0, 0), n12 = make_uint4(0, 0, 0, 0);
        if (ARRAYS >= 2) n8 = L.q8[tid];
        if (ARRAYS >= 3) n12 = L.q12[tid];
#pragma unroll 1
        for (int i = 0; i < PCR_POINTS_PER_BATCH / 4 / PCR_WORKGROUP_SIZE; ++i) {
            const uint4 c4 = n4, c8 = n8, c12 = n12;
            const uint32_t quad = tid + (uint32_t)i * PCR_WORKGROUP_SIZE;
            const auto per_quad = quad_fn(quad);
            {   // next quad in flight while this one is projected (the last iteration re-reads its own: no branch around the loads)
                const uint32_t nq = min(quad + PCR_WORKGROUP_SIZE, (uint32_t)(PCR_POINTS_PER_BATCH / 4 - 1));
                n4 = L.q4[nq];
                if (ARRAYS >= 2) n8 = L.q8[nq];
                if (ARRAYS >= 3) n12 = L.q12[nq];
            }
            const uint32_t w4[4] = { c4.x, c4.y, c4.z, c4.w }, w8[4] = { c8.x, c8.y, c8.z, c8.w }, w12[4] = { c12.x, c12.y, c12.z, c12.w };
            auto point = [&](uint32_t X, uint32_t Y, uint32_t Z, int j) __attribute__((always_inline)) {
                const float x = __fmaf_rn((float)X, L.sx, L.ox), y = __fmaf_rn((float)Y, L.sy, L.oy), z = __fmaf_rn((float)Z, L.sz, L.oz);
                point_fn(project_point(L.m, L.fw, L.fh, x, y, z), per_quad, j);
            };
            if (ARRAYS == 1) {                                                   // :381-392 (levels 2..4)
#pragma unroll
                for (int j = 0; j < 4; ++j) point(w4[j] & 1023u, (w4[j] >> 10) & 1023u, (w4[j] >> 20) & 1023u, j);
            } else {                                                             // :333-378 (level 1: the 12-byte array's bits are zero)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    point(((w4[j] & 1023u) << 20) | ((w8[j] & 1023u) << 10) | (w12[j] & 1023u),
                          (((w4[j] >> 10) & 1023u) << 20) | (((w8[j] >> 10) & 1023u) << 10) | ((w12[j] >> 10) & 1023u),
                          (((w4[j] >> 20) & 1023u) << 20) | (((w8[j] >> 20) & 1023u) << 10) | ((w12[j] >> 20) & 1023u), j);
            }
        }
    };
    if (L.level >= 2)      quads(std::integral_constant<int, 1>{});
    else if (L.level == 1) quads(std::integral_constant<int, 2>{});
    else                   quads(std::integral_constant<int, 3>{});
}

// Round 4: brought to k_render's standard. The window starts EMPTY (round 1 copied the framebuffer's words into it: a global read
// of every window pixel in front of the barrier); a point's depth is tested against the depth half of its window word, read a
// whole point before it is used, and only then is the 64-bit key put together for the ds_min_u64 (round 1: a 64-bit LDS read and
// compare in front of the atomic, the round trip exposed four times per quad); "inside the frustum" / "inside the window" are
// lane masks in scalar registers, a lane without a window word reads a dummy slot whose depth 0 turns it away; the merge issues
// its atomic without reading the pixel first; batches are drawn through the prepass's compacted list. Points outside the window
// keep their pre-read of the global word (strip-ordered clouds put most points there: unfiltered 8 x the time in atomics), now
// requested a point ahead like the window word. Reference: modules/compute_loop_las_cuda/render.cu:204-327 (USE_PREFETCH loop),
// :108-128 (rasterize).
//
// DEPTH_ONLY: the depth pass of loop_las_hqs (modules/compute_loop_las_hqs/depth.cs:335-355): the same walk, tests and atomics
// with the key depth<<32 and payload 0, so that fb >> 32 is the basic frame's depth half at every pixel.
template <bool DEPTH_ONLY>
__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE, 8) k_las_render(LasArgs a)
{
    uint32_t b;
    if (!las_list_batch(a, b)) return;
    const int level = a.level[b];
    const uint32_t tid = threadIdx.x;
    __shared__ __align__(16) unsigned long long s_win[WIN_PIXELS + 1];

    const uint2 wr = a.win[b];
    const uint32_t wx0 = wr.x & 0xFFFFu, wy0 = wr.x >> 16, ww = wr.y & 0xFFFFu, wh = wr.y >> 16;
    const uint32_t wpix = ww * wh;
    const uint32_t W = (uint32_t)a.p.width;
    const float inv_ww = 1.0f / (float)max(ww, 1u);
    for (uint32_t i = tid; i < wpix; i += PCR_WORKGROUP_SIZE) s_win[i] = ~0ull;
    if (tid == 0) s_win[wpix] = 0ull;                                        // the dummy slot: depth 0, no point passes it
    const LasBatch L = las_batch(a, b, level);
    const int img_w = a.p.width;
    uint64_t *const g_fb = a.f.fb;
    typedef __attribute__((address_space(3))) unsigned long long lds_u64;
    lds_u64 *const s_w = (lds_u64 *)s_win;
    // the pending point: projected, its window word's depth half requested; scattered while the next point is projected
    lds_u64 *pend_p = s_w + wpix;
    uint32_t pend_depth = 0, pend_old_hi = 0, pend_index = 0, pend_pix = 0;
    uint64_t pend_off_mask = 0;                                              // lanes whose pending point is inside the frustum but outside the window
    __syncthreads();

    auto scatter_pending = [&]() __attribute__((always_inline)) {
        // rasterize, second half (:119-126): the pre-read filter on the depth half, then the min (ties go to the atomic: min is idempotent)
        if (pend_depth <= pend_old_hi) {
            const unsigned long long key = ((unsigned long long)pend_depth << 32) | (DEPTH_ONLY ? 0u : pend_index);  // :119-120, depth.cs:344-348
            // (either / or: in a strip-ordered cloud most lanes are outside the window, and 50 of them on the dummy slot's one
            // address would serialise the LDS atomic)
            if (__builtin_amdgcn_inverse_ballot_w64(pend_off_mask)) atomicMin((unsigned long long *)&g_fb[pend_pix], key);   // :123-126
            else __hip_atomic_fetch_min(pend_p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    // per quad: the index of its first point; per point: the pending one is scattered, this one becomes the pending one
    auto quad_index = [&](uint32_t quad) __attribute__((always_inline)) { return (uint32_t)L.base + quad * 4; };
    auto point = [&](const Projection &pr, uint32_t index0, int j) __attribute__((always_inline)) {
        const uint64_t cand_mask = pr.cand;
        const int ix = pr.ix, iy = pr.iy;
        scatter_pending();                                                   // the point before this one: its window word has arrived by now
        const uint32_t rx = (uint32_t)ix - wx0, ry = (uint32_t)iy - wy0;
        const uint64_t in_mask = cand_mask & __builtin_amdgcn_ballot_w64(rx < ww) & __builtin_amdgcn_ballot_w64(ry < wh);
        pend_off_mask = cand_mask & ~in_mask;
        pend_depth = __float_as_uint(pr.w);
        pend_index = index0 + j;
        pend_p = s_w + (__builtin_amdgcn_inverse_ballot_w64(in_mask) ? (uint32_t)__umul24(ry, ww) + rx : wpix);
        pend_old_hi = reinterpret_cast<__attribute__((address_space(3))) const uint32_t *>(pend_p)[1];
        if (__builtin_expect(pend_off_mask != 0, 0)) {                      // (uniform) some lane's point lies outside the window: the global word's depth (:123)
            if (__builtin_amdgcn_inverse_ballot_w64(pend_off_mask)) {
                pend_pix = (uint32_t)(ix + iy * img_w);
                // (consumed inside the branch: no load is pending where the paths join, so hipcc's waits for the next quad's words,
                // requested a whole quad ahead, stay counted instead of becoming vmcnt(0) in front of every scatter)
                uint32_t seen = __hip_atomic_load(reinterpret_cast<const uint32_t *>(&g_fb[pend_pix]) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                asm volatile("; framebuffer word of a point outside its window %0" : "+v"(seen));
                pend_old_hi = seen;
            }
        }
    };

    las_points(L, quad_index, point);
    scatter_pending();
    if (wpix) {
        __syncthreads();
        for (uint32_t i = tid; i < wpix; i += PCR_WORKGROUP_SIZE) {
            uint32_t y, x;
            window_row_col(i, ww, inv_ww, y, x);
            const unsigned long long v = s_win[i];
            if (v != ~0ull) atomicMin((unsigned long long *)&a.f.fb[(size_t)(wy0 + y) * W + wx0 + x], v);      // (a pixel no point reached issues nothing)
        }
    }
}

// ------------------------------------------------------------------------------------------------
// colour pass of "loop_las_hqs" (modules/compute_loop_las_hqs/color.cs:360-405): every point k_las_render<true> drew is averaged
// into its pixel iff w <= d * 1.01f, d = the pixel's depth after the depth pass -- an f32 product (color.cs:370: `1.01` is a GLSL
// float literal), where the Huffman HQS pass compares in f64 (huffman_hqs/render.cu:296). RG += R<<32 | G, BA += B<<32 | 1: the
// Huffman HQS packing, so that k_resolve<true> and the merges take both methods' sums (color.cs:399-400 packs R | G<<32; the
// resolved image is the same).
//
// It shares k_las_render's list walk, levels, 16-byte quad-ahead loads and projection (las_list_batch, las_batch, las_points),
// and reads the points' colours as well, 16 bytes per quad. The LDS window holds {RG u64, BA u64, depth u32} per pixel: 4096 slots of 20 B
// = 80 KiB, two workgroups per CU in the 160 KiB; the last slot is the dummy (depth all ones, a NaN: no point passes it). Its
// depth half is preloaded from fb at workgroup start, row by row; the sums go through ds_add_u64 and leave with one global
// 64-bit atomicAdd per word of every pixel that counted a point. A point outside the window, or in a batch without one, reads
// its depth from fb and adds to RG / BA in global memory.
// ------------------------------------------------------------------------------------------------
constexpr int LAS_WIN_SLOTS_HQS = 4096;
constexpr int LAS_WIN_PIXELS_HQS = LAS_WIN_SLOTS_HQS - 1;      // the prepass's capacity of the colour window

__global__ void __launch_bounds__(PCR_WORKGROUP_SIZE, 8) k_las_render_color(LasArgs a)
{
    uint32_t b;
    if (!las_list_batch(a, b)) return;
    const int level = a.level[b];
    const uint32_t tid = threadIdx.x;
    __shared__ __align__(16) unsigned long long s_rg[LAS_WIN_SLOTS_HQS], s_ba[LAS_WIN_SLOTS_HQS];
    __shared__ uint32_t s_depth[LAS_WIN_SLOTS_HQS];

    const uint2 wr = a.win_hqs[b];
    const uint32_t wx0 = wr.x & 0xFFFFu, wy0 = wr.x >> 16, ww = wr.y & 0xFFFFu, wh = wr.y >> 16;
    const uint32_t wpix = ww * wh;                                          // <= LAS_WIN_PIXELS_HQS (window_rect)
    const uint32_t W = (uint32_t)a.p.width;
    const float inv_ww = 1.0f / (float)max(ww, 1u);
    const uint64_t *const g_fb = a.f.fb;
    for (uint32_t i = tid; i < wpix; i += PCR_WORKGROUP_SIZE) {
        uint32_t y, x;
        window_row_col(i, ww, inv_ww, y, x);
        s_rg[i] = 0ull; s_ba[i] = 0ull;
        s_depth[i] = reinterpret_cast<const uint32_t *>(&g_fb[(size_t)(wy0 + y) * W + wx0 + x])[1];
    }
    if (tid == 0) { s_rg[wpix] = 0ull; s_ba[wpix] = 0ull; s_depth[wpix] = 0xFFFFFFFFu; }    // the dummy slot
    const LasBatch L = las_batch(a, b, level);
    const int img_w = a.p.width;
    unsigned long long *const g_rg = reinterpret_cast<unsigned long long *>(a.f.rg), *const g_ba = reinterpret_cast<unsigned long long *>(a.f.ba);
    const uint4 *qc = reinterpret_cast<const uint4 *>(a.rgba_points + L.base);
    typedef __attribute__((address_space(3))) unsigned long long lds_u64;
    // the pending point: projected, its depth requested; accumulated while the next point is projected. pend_at: its window slot
    // (the dummy slot wpix if it has none), or its pixel if it takes the global path (pend_off_mask)
    uint32_t pend_at = wpix, pend_depth = 0xFFFFFFFFu, pend_w = 0, pend_color = 0;
    uint64_t pend_off_mask = 0;                                              // lanes whose pending point is inside the frustum but outside the window
    __syncthreads();

    auto add_pending = [&]() __attribute__((always_inline)) {
        if (__uint_as_float(pend_w) <= __uint_as_float(pend_depth) * 1.01f) {    // color.cs:370 (NaN depth: untouched pixel or dummy slot)
            const uint64_t rg = ((uint64_t)(pend_color & 255u) << 32) | ((pend_color >> 8) & 255u);     // color.cs:387-400, repacked
            const uint64_t ba = ((uint64_t)((pend_color >> 16) & 255u) << 32) | 1u;
            if (__builtin_amdgcn_inverse_ballot_w64(pend_off_mask)) {
                uint32_t pix = pend_at;
                asm volatile("; pixel of a point outside its window %0" : "+v"(pix));     // (widened here, not carried as 64 bits)
                atomicAdd(&g_rg[pix], (unsigned long long)rg);
                atomicAdd(&g_ba[pix], (unsigned long long)ba);
            } else {
                __hip_atomic_fetch_add((lds_u64 *)s_rg + pend_at, (unsigned long long)rg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add((lds_u64 *)s_ba + pend_at, (unsigned long long)ba, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    };
    // the quad's colours: requested in front of the next quad's words, so that waiting for them does not wait for those (not a
    // quad ahead: four more registers would not fit the 64 of two workgroups per CU -- the three-array copy spilled)
    auto quad_colors = [&](uint32_t quad) __attribute__((always_inline)) {
        uint32_t cq = quad;
        asm volatile("; colour quad %0" : "+v"(cq));                        // (no 64-bit pointer induction variable: it spilled)
        return qc[cq];
    };
    auto point = [&](const Projection &pr, const uint4 &cc, int j) __attribute__((always_inline)) {
        const uint32_t wc[4] = { cc.x, cc.y, cc.z, cc.w };
        const uint64_t cand_mask = pr.cand;
        const int ix = pr.ix, iy = pr.iy;
        add_pending();                                                       // the point before this one: its depth has arrived by now
        const uint32_t rx = (uint32_t)ix - wx0, ry = (uint32_t)iy - wy0;
        const uint64_t in_mask = cand_mask & __builtin_amdgcn_ballot_w64(rx < ww) & __builtin_amdgcn_ballot_w64(ry < wh);
        pend_off_mask = cand_mask & ~in_mask;
        pend_w = __float_as_uint(pr.w);
        pend_color = wc[j];
        pend_at = __builtin_amdgcn_inverse_ballot_w64(in_mask) ? (uint32_t)__umul24(ry, ww) + rx : wpix;
        pend_depth = s_depth[pend_at];
        if (__builtin_expect(pend_off_mask != 0, 0)) {                      // (uniform) some lane's point lies outside the window: the global word's depth
            if (__builtin_amdgcn_inverse_ballot_w64(pend_off_mask)) {
                pend_at = (uint32_t)(ix + iy * img_w);
                uint32_t seen = reinterpret_cast<const uint32_t *>(&g_fb[pend_at])[1];
                asm volatile("; framebuffer depth of a point outside its window %0" : "+v"(seen));
                pend_depth = seen;
            }
        }
    };

    las_points(L, quad_colors, point);
    add_pending();
    if (wpix) {
        __syncthreads();
        for (uint32_t i = tid; i < wpix; i += PCR_WORKGROUP_SIZE) {
            const unsigned long long vba = s_ba[i];
            if ((uint32_t)vba == 0u) continue;                               // (a pixel no point was averaged into issues nothing)
            uint32_t y, x;
            window_row_col(i, ww, inv_ww, y, x);
            const size_t gp = (size_t)(wy0 + y) * W + wx0 + x;
            atomicAdd(&g_rg[gp], s_rg[i]);
            atomicAdd(&g_ba[gp], vba);
        }
    }
}

// modules/compute_loop_las_cuda/resolve.cu (every pixel; the reference's floor(w/16) x floor(h/16) launch skips the rest)
__global__ void __launch_bounds__(256) k_las_resolve(int width, int height, const uint64_t *fb, const uint32_t *rgba_points,
                                                     uint32_t *rgba)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= width || y >= height) return;
    const int pix = x + y * width;
    const uint32_t id = (uint32_t)fb[pix];
    rgba[pix] = id < 0x7FFFFFFFu ? rgba_points[id] : PCR_BACKGROUND_COLOR;
}

// ------------------------------------------------------------------------------------------------
// CLEAR block (huffman_hqs.h:266-270): fb <- all ones, and RG/BA <- 0 when a colour pass has written them; one launch,
// 16-byte stores
// ------------------------------------------------------------------------------------------------
// Tile flags at a CLEAR (FrameView::tiles): the half the coming frame marks starts empty; the other half -- tiles whose image pixels
// may hold something -- takes over what was marked so far (a separate resolve may have drawn it), or everything if nobody kept track.
struct TileFlags { uint8_t *cur, *prev; uint32_t *cur_all, *prev_all; uint32_t ntiles, e_cur, e_prev; int tracked; };
__device__ __forceinline__ void clear_tile_flags(const TileFlags &t)
{
    if (!t.cur) return;
    for (uint32_t i = threadIdx.x; i < t.ntiles; i += blockDim.x) {
        t.prev[i] = t.tracked ? (uint8_t)(t.prev[i] | t.cur[i]) : (uint8_t)1;
        t.cur[i] = 0;
    }
    // ("everything": the host gives the emptied half a fresh epoch, so its word needs no reset)
    if (threadIdx.x == 0 && (!t.tracked || *t.cur_all == t.e_cur)) *t.prev_all = t.e_prev;
}

__device__ __forceinline__ void clear_block(uint64_t *fb, uint64_t *rg, uint64_t *ba, size_t n, uint64_t empty,
                                            uint32_t block, uint32_t blocks)
{
    const size_t pairs = n / 2, stride = (size_t)blocks * blockDim.x;
    const ulonglong2 ones = make_ulonglong2(empty, empty), zero = make_ulonglong2(0ull, 0ull);
    for (size_t i = (size_t)block * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        reinterpret_cast<ulonglong2 *>(fb)[i] = ones;
        if (rg) reinterpret_cast<ulonglong2 *>(rg)[i] = zero;
        if (ba) reinterpret_cast<ulonglong2 *>(ba)[i] = zero;
    }
    if ((n & 1) && block == 0 && threadIdx.x == 0) {
        fb[n - 1] = empty;
        if (rg) rg[n - 1] = 0;
        if (ba) ba[n - 1] = 0;
    }
}

__global__ void __launch_bounds__(256) k_clear(uint64_t *fb, uint64_t *rg, uint64_t *ba, size_t n, uint64_t empty, TileFlags tiles)
{
    clear_block(fb, rg, ba, n, empty, blockIdx.x, gridDim.x);
    if (blockIdx.x == gridDim.x - 1) clear_tile_flags(tiles);
}

// CLEAR and the prepass of the frame's first pass in one launch (pcr_frame_begin): the first `prepass_blocks` workgroups
// do the cull/LOD work (it touches no framebuffer), the others fill. Saves the prepass's 5 us and a launch gap per frame.
static_assert(PREPASS_THREADS == 256, "k_frame_begin runs both bodies with 256 threads");
__global__ void __launch_bounds__(256) k_frame_begin(RenderArgs a, uint32_t prepass_blocks, uint64_t *fb, uint64_t *rg,
                                                     uint64_t *ba, size_t n, uint64_t empty, TileFlags tiles)
{
    if (blockIdx.x < prepass_blocks) { lod_prepass_block(a, blockIdx.x); return; }
    clear_block(fb, rg, ba, n, empty, blockIdx.x - prepass_blocks, gridDim.x - prepass_blocks);
    if (blockIdx.x == gridDim.x - 1) clear_tile_flags(tiles);
}

// ------------------------------------------------------------------------------------------------
// HBM ceiling probes (pcr_measure_hbm): a streaming read (16-byte loads, xor-folded so nothing is optimised away) and a
// streaming copy, over buffers larger than the 256 MiB Infinity Cache. The practical ceiling the roofline is set beside.
// ------------------------------------------------------------------------------------------------
typedef uint32_t hbm_vec4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_hbm_read(const hbm_vec4 *src, size_t n16, uint32_t *sink)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    hbm_vec4 acc = {0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride)
        acc ^= __builtin_nontemporal_load(src + i);
    const uint32_t f = acc.x ^ acc.y ^ acc.z ^ acc.w;
    if (f == 0x9E3779B9u) *sink = f;          // practically never: keeps the loads alive
}

__global__ void __launch_bounds__(256) k_hbm_copy(const hbm_vec4 *src, hbm_vec4 *dst, size_t n16)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride)
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

// ------------------------------------------------------------------------------------------------
// resolve (resolve.cu:149-191, huffman_hqs/resolve.cu:2-47)
// ------------------------------------------------------------------------------------------------
// The basic method's resolve depends on the framebuffer word only, not on the pixel's position: a contiguous range of
// pixels (a slice of the frame a rank owns after the all-to-all merge) resolves on its own. Same arithmetic as k_resolve<false>.
__global__ void __launch_bounds__(256) k_resolve_range(int show_num_points, int colorize_chunks, const uint64_t *fb,
                                                       size_t count, uint32_t *rgba)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t id = (uint32_t)fb[i];
        uint32_t color = PCR_BACKGROUND_COLOR;
        if (id < 0xFFFFFFFFu) {
            if (show_num_points) {
                const uint32_t shade = (uint32_t)(((double)(float)(int)id / 64.0) * 255.0);
                color = (shade << 24) | (shade << 16) | (shade << 8) | shade;
            } else if (colorize_chunks) {
                color = id * 1234567u;
            } else {
                color = id;
            }
        }
        rgba[i] = color;
    }
}

// The HQS resolve of a contiguous range of pixels (a slice of the frame a rank owns after the sums were reduce-scattered):
// same arithmetic as k_resolve<true>, which depends on the pixel's three words only.
__global__ void __launch_bounds__(256) k_resolve_range_hqs(int show_num_points, int colorize_chunks, const uint64_t *fb,
                                                           const uint64_t *rg, const uint64_t *ba, size_t count, uint32_t *rgba)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t id = (uint32_t)fb[i];
        uint32_t color = PCR_BACKGROUND_COLOR;
        if (id < 0xFFFFFFFFu) {
            if (show_num_points) {
                const uint32_t shade = (uint32_t)(((double)(float)(int)id / 512.0) * 255.0);
                color = (shade << 24) | (shade << 16) | (shade << 8) | shade;
            } else if (colorize_chunks) {
                color = id * 1234567u;
            } else {
                const uint64_t vrg = rg[i], vba = ba[i];
                const uint32_t cnt = (uint32_t)vba;
                if (cnt == 0) color = 0;
                else color = (((uint32_t)(vba >> 32) / cnt) << 16) | (((uint32_t)vrg / cnt) << 8) | ((uint32_t)(vrg >> 32) / cnt);
            }
        }
        rgba[i] = color;
    }
}

// slices[0 .. S) <- element-wise min over `ns` slices of S words laid out back to back (what a rank holds after the
// all-to-all: everyone's copy of the slice of the frame it owns)
__global__ void __launch_bounds__(256) k_merge_min_slices(uint64_t *slices, int ns, size_t S)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t m = slices[i];
        for (int r = 1; r < ns; ++r) m = min(m, slices[(size_t)r * S + i]);
        slices[i] = m;
    }
}

template <bool HQS>
__global__ void __launch_bounds__(256) k_resolve(int show_num_points, int colorize_chunks, int width, int height,
                                                 const uint64_t *fb, const uint64_t *rg, const uint64_t *ba,
                                                 uint32_t *rgba)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15);     // 16x16 tiles as the reference launches
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= width || y >= height) return;
    const int pix = x + y * width;
    const uint32_t id = (uint32_t)fb[pix];
    uint32_t color = PCR_BACKGROUND_COLOR;
    if (id < 0xFFFFFFFFu) {
        if (show_num_points) {
            const double div = HQS ? 512.0 : 64.0;
            const uint32_t shade = (uint32_t)(((double)(float)(int)id / div) * 255.0);
            color = (shade << 24) | (shade << 16) | (shade << 8) | shade;
        } else if (colorize_chunks) {
            color = id * 1234567u;
        } else if (HQS) {
            const uint64_t vrg = rg[pix], vba = ba[pix];
            const uint32_t cnt = (uint32_t)vba;
            if (cnt == 0) color = 0;
            else color = (((uint32_t)(vba >> 32) / cnt) << 16) | (((uint32_t)vrg / cnt) << 8) | ((uint32_t)(vrg >> 32) / cnt);
        } else {
            color = id;
        }
    }
    rgba[pix] = color;
}

// ------------------------------------------------------------------------------------------------
// display resolve (pcr_resolve_*_display): n x n point size and eye-dome lighting, after the resolve of the reference's GLSL
// 10-10-10 method (compute_loop_las/resolve.cs:98-128 the window loop, :41-62 and :143-185 EDL). Not in its CUDA methods.
// ------------------------------------------------------------------------------------------------
// Point size is a stencil over the FINISHED framebuffer: the u64 minimum of the words of a pixel's (2w+1)^2 window is the word
// the 64-bit atomicMin would have left there had every point been drawn as a square of that size, so the render kernels stay
// as they are and the cost is O(pixels). One workgroup per 64 x 16 tile:
//   1. the tile's words with a halo of R = window + edl_window pixels go to LDS, row by row, 16-byte loads where the pair is
//      aligned and inside the row; slots outside the image hold the empty word (windows are clipped to the image)
//   2. minimum over the row window into a second array, 3. over the column window (2 (2w+1) comparisons for (2w+1)^2)
//   4. EDL: the dilated words of the tile and a halo of edl_window go to a third array; a pixel reads its neighbours' depths there
// Lanes walk a row, so the 8-byte LDS reads of a wave are to consecutive addresses: conflict-free in both halves of the wave.
// (The pair load's two stores per lane are 16 bytes apart: the 8 % of bank-conflict cycles profiles/README.md reports.)
// The HQS colour of a pixel: the rg/ba sums of the window's pixels whose OWN front depth passes the 1 % test against the dilated
// depth, gathered from global memory (neighbouring lanes read neighbouring words; the tile's rows are in L2 from step 1's pass).
enum { DISPLAY_BASIC = 0, DISPLAY_HQS = 1, DISPLAY_LAS = 2 };
enum { DISPLAY_TW = 64, DISPLAY_TH = 16, DISPLAY_THREADS = 256,
       DISPLAY_MAX_HALO = PCR_DISPLAY_MAX_WINDOW + PCR_DISPLAY_MAX_EDL_WINDOW,
       DISPLAY_PITCH = DISPLAY_TW + 2 * DISPLAY_MAX_HALO, DISPLAY_ROWS = DISPLAY_TH + 2 * DISPLAY_MAX_HALO };
static_assert(DISPLAY_TW == 64 && DISPLAY_THREADS == 4 * 64 && DISPLAY_TH % 4 == 0, "a wave per row of the tile, four rows per wave");
static_assert(DISPLAY_PITCH / 2 + 1 <= 64 && DISPLAY_ROWS % 4 == 0, "a row's pairs are loaded by one wave, the rows dealt out to four");

struct DisplayArgs {
    int width, height;
    int window, edl_window;
    float edl_strength;
    int show_num_points, colorize_chunks;
    uint64_t empty;
    const uint64_t *fb, *rg, *ba;
    const uint32_t *rgba_points;
    uint32_t *rgba;
};

// Minimum of the 2 w + 1 words p[0], p[stride], ...: the loop unrolled per window, so that its LDS reads are all in flight at once
// (w is uniform: a scalar branch).
template <int WN>
__device__ __forceinline__ uint64_t display_min_run(const uint64_t *p, int stride)
{
    uint64_t m = p[0];
#pragma unroll
    for (int k = 1; k <= 2 * WN; ++k) m = min(m, p[k * stride]);
    return m;
}
__device__ __forceinline__ uint64_t display_min_run(const uint64_t *p, int stride, int w)
{
    static_assert(PCR_DISPLAY_MAX_WINDOW == 4, "one case per window");
    switch (w) {
    case 1: return display_min_run<1>(p, stride);
    case 2: return display_min_run<2>(p, stride);
    case 3: return display_min_run<3>(p, stride);
    case 4: return display_min_run<4>(p, stride);
    default: return p[0];
    }
}

template <int METHOD, bool EDL>
__global__ void __launch_bounds__(DISPLAY_THREADS) k_resolve_display(DisplayArgs a)
{
    __shared__ uint64_t s_fb[DISPLAY_ROWS * DISPLAY_PITCH];              // the undilated words
    __shared__ uint64_t s_h[DISPLAY_ROWS * DISPLAY_PITCH];               // minimum over the row window
    __shared__ uint64_t s_d[EDL ? DISPLAY_ROWS * DISPLAY_PITCH : 1];     // the dilated words (EDL reads its neighbours' here)
    const int W = a.width, H = a.height, w = a.window, e = EDL ? a.edl_window : 0, R = w + e;
    const int LW = DISPLAY_TW + 2 * R, LH = DISPLAY_TH + 2 * R;
    const int x0 = (int)blockIdx.x * DISPLAY_TW - R, y0 = (int)blockIdx.y * DISPLAY_TH - R;    // image position of LDS slot (0, 0)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t empty = a.empty;

    // 1. load: a wave per row, a lane per aligned pair of words; every load of the wave is issued before the first LDS store, so
    // a wave waits for memory once, not once per row
    uint64_t v0[DISPLAY_ROWS / 4], v1[DISPLAY_ROWS / 4];
#pragma unroll
    for (int i = 0; i < DISPLAY_ROWS / 4; ++i) {
        const int ly = wave + 4 * i, gy = y0 + ly;
        const long long g0 = (long long)gy * W + x0;                     // linear index of the row's slot 0 (may lie left of the row)
        const int lx = (int)(((g0 >> 1) + lane) * 2 - g0);               // -1 or 0 for lane 0: the pair's first slot
        const int gx = x0 + lx;
        const bool row = ly < LH && gy >= 0 && gy < H;
        const bool in0 = row && lx >= 0 && lx < LW && gx >= 0 && gx < W, in1 = row && lx + 1 < LW && gx + 1 >= 0 && gx + 1 < W;
        v0[i] = empty; v1[i] = empty;
        const uint64_t *src = a.fb + (g0 + lx);
        if (in0 && in1) { const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(src); v0[i] = v.x; v1[i] = v.y; }
        else if (in0) v0[i] = src[0];
        else if (in1) v1[i] = src[1];
    }
#pragma unroll
    for (int i = 0; i < DISPLAY_ROWS / 4; ++i) {
        const int ly = wave + 4 * i;
        const long long g0 = (long long)(y0 + ly) * W + x0;
        const int lx = (int)(((g0 >> 1) + lane) * 2 - g0);
        if (ly < LH && lx >= 0 && lx < LW) s_fb[ly * DISPLAY_PITCH + lx] = v0[i];
        if (ly < LH && lx + 1 < LW) s_fb[ly * DISPLAY_PITCH + lx + 1] = v1[i];
    }
    __syncthreads();

    // 2. minimum over the row window: every row, columns [w, LW - w)
    const uint64_t *rows = s_fb;
    if (w > 0) {
        const uint32_t cw = (uint32_t)(LW - 2 * w), n = cw * (uint32_t)LH;
        const float inv_cw = 1.0f / (float)cw;
        for (uint32_t i = threadIdx.x; i < n; i += DISPLAY_THREADS) {
            uint32_t y, x;
            window_row_col(i, cw, inv_cw, y, x);
            const uint64_t *p = s_fb + y * DISPLAY_PITCH + x;            // slot x of the window that is centred on column x + w
            s_h[y * DISPLAY_PITCH + x + w] = display_min_run(p, 1, w);
        }
        __syncthreads();
        rows = s_h;
    }
    // 3. minimum over the column window at slot (lx, ly), w <= lx < LW - w, w <= ly < LH - w: the dilated word
    auto dilated = [&](int lx, int ly) {
        return display_min_run(rows + (ly - w) * DISPLAY_PITCH + lx, DISPLAY_PITCH, w);
    };
    if (EDL) {
        const uint32_t cw = (uint32_t)(DISPLAY_TW + 2 * e), n = cw * (uint32_t)(DISPLAY_TH + 2 * e);
        const float inv_cw = 1.0f / (float)cw;
        for (uint32_t i = threadIdx.x; i < n; i += DISPLAY_THREADS) {
            uint32_t y, x;
            window_row_col(i, cw, inv_cw, y, x);
            const int lx = (int)x + w, ly = (int)y + w, gx = x0 + lx, gy = y0 + ly;
            // (a slot outside the image is no pixel: its window reaches into the image, its word stays empty)
            s_d[ly * DISPLAY_PITCH + lx] = gx >= 0 && gx < W && gy >= 0 && gy < H ? dilated(lx, ly) : empty;
        }
        __syncthreads();
    }

    // the pixels: a wave per row, four rows per wave
    const int px = (int)blockIdx.x * DISPLAY_TW + lane;
    if (px >= W) return;
    for (int k = 0; k < DISPLAY_TH / 4; ++k) {
        const int ty = wave * (DISPLAY_TH / 4) + k, py = (int)blockIdx.y * DISPLAY_TH + ty;
        if (py >= H) break;
        const int lx = lane + R, ly = ty + R;
        const uint64_t D = EDL ? s_d[ly * DISPLAY_PITCH + lx] : dilated(lx, ly);
        const uint32_t id = (uint32_t)D;
        uint32_t color = PCR_BACKGROUND_COLOR;
        if (METHOD == DISPLAY_LAS) {
            if (id < 0x7FFFFFFFu) color = a.rgba_points[id];
        } else if (id < 0xFFFFFFFFu) {
            if (a.show_num_points) {
                const double div = METHOD == DISPLAY_HQS ? 512.0 : 64.0;
                const uint32_t shade = (uint32_t)(((double)(float)(int)id / div) * 255.0);
                color = (shade << 24) | (shade << 16) | (shade << 8) | shade;
            } else if (a.colorize_chunks) {
                color = id * 1234567u;
            } else if (METHOD == DISPLAY_HQS) {
                // the sums of the window's pixels that are drawn and whose own depth is within 1 % of the dilated depth
                // (w <= d * 1.01f, one rounded f32 product: color.cs:370); slots outside the image are empty
                const float limit = __uint_as_float((uint32_t)(D >> 32)) * 1.01f;
                uint64_t vrg = 0, vba = 0;
                for (int oy = -w; oy <= w; ++oy) {
                    const uint64_t *p = s_fb + (ly + oy) * DISPLAY_PITCH + lx;
                    const size_t g = (size_t)(py + oy) * (size_t)W + (size_t)px;
                    for (int ox = -w; ox <= w; ++ox) {
                        const uint64_t own = p[ox];
                        if (own != empty && __uint_as_float((uint32_t)(own >> 32)) <= limit) {
                            vrg += a.rg[g + ox];
                            vba += a.ba[g + ox];
                        }
                    }
                }
                const uint32_t cnt = (uint32_t)vba;
                if (cnt == 0) color = 0;
                else color = (((uint32_t)(vba >> 32) / cnt) << 16) | (((uint32_t)vrg / cnt) << 8) | ((uint32_t)(vrg >> 32) / cnt);
            } else {
                color = id;
            }
        }
        if (EDL && D != empty) {
            // resolve.cs:143-185 on the dilated depths: every f32 operation a statement of its own, none contracts
            const float dc = __uint_as_float((uint32_t)(D >> 32));
            float sum = 0.0f;
            for (int ox = -e; ox <= e; ++ox)
                for (int oy = -e; oy <= e; ++oy) {
                    const uint64_t nb = s_d[(ly + oy) * DISPLAY_PITCH + lx + ox];      // outside the image: empty
                    float t = 0.0f;
                    if (nb != empty) {
                        const float diff = __fsub_rn(dc, __uint_as_float((uint32_t)(nb >> 32)));
                        t = fmaxf(0.0f, diff);
                    }
                    sum = __fadd_rn(sum, t);
                }
            const float cells = (float)((2 * e + 1) * (2 * e + 1));
            const float response = __fdiv_rn(sum, cells);
            const float scaled = __fmul_rn(-response, 300.0f);
            const float shade = expf(__fmul_rn(scaled, a.edl_strength));
            const uint32_t r = (uint32_t)__fmul_rn((float)(color & 255u), shade);
            const uint32_t g = (uint32_t)__fmul_rn((float)((color >> 8) & 255u), shade);
            const uint32_t b = (uint32_t)__fmul_rn((float)((color >> 16) & 255u), shade);
            color = r | (g << 8) | (b << 16);
        }
        a.rgba[(size_t)py * (size_t)W + (size_t)px] = color;
    }
}

// RESOLVE of the finished frame, CLEAR for the next one and the next frame's cull/LOD prepass in ONE launch (pcr_frame_turn):
// the reference's frame ends with resolve + clear (huffman_hqs.h:240-270); done separately they are two passes over the
// framebuffer and two launches (21 us of a 269 us frame at 1080p), fused one pass reads every word once, writes the pixel,
// and writes the empty word back. The first `prepass_blocks` workgroups do the prepass instead (it touches no framebuffer).
// Same arithmetic as k_resolve<HQS>; pixels are walked linearly (the resolve is per pixel, the tile shape does not matter).
template <bool HQS>
__global__ void __launch_bounds__(256) k_frame_turn(RenderArgs a, uint32_t prepass_blocks, int show_num_points, int colorize_chunks,
                                                    uint32_t pixels, uint64_t *fb, uint64_t *rg, uint64_t *ba, uint32_t *rgba,
                                                    uint32_t n, uint64_t empty, TileFlags tiles)
{
    if (blockIdx.x < prepass_blocks) { lod_prepass_block(a, blockIdx.x); return; }
    // (the whole frame is resolved and cleared: from here on the tile flags can be kept again -- nothing written yet, any image
    // pixel may hold something)
    if (blockIdx.x == gridDim.x - 1) { TileFlags t = tiles; t.tracked = 0; clear_tile_flags(t); }
    const uint32_t stride = (gridDim.x - prepass_blocks) * 256u;
    for (uint32_t i = (blockIdx.x - prepass_blocks) * 256u + threadIdx.x; i < n; i += stride) {
        if (i < pixels) {
            const uint32_t id = (uint32_t)fb[i];
            uint32_t color = PCR_BACKGROUND_COLOR;
            if (id < 0xFFFFFFFFu) {
                if (show_num_points) {
                    const double div = HQS ? 512.0 : 64.0;
                    const uint32_t shade = (uint32_t)(((double)(float)(int)id / div) * 255.0);
                    color = (shade << 24) | (shade << 16) | (shade << 8) | shade;
                } else if (colorize_chunks) {
                    color = id * 1234567u;
                } else if (HQS) {
                    const uint64_t vrg = rg[i], vba = ba[i];
                    const uint32_t cnt = (uint32_t)vba;
                    if (cnt == 0) color = 0;
                    else color = (((uint32_t)(vba >> 32) / cnt) << 16) | (((uint32_t)vrg / cnt) << 8) | ((uint32_t)(vrg >> 32) / cnt);
                } else {
                    color = id;
                }
            }
            rgba[i] = color;
        }
        fb[i] = empty;
        if (HQS) { rg[i] = 0; ba[i] = 0; }
    }
}

// The same over the dirty tiles only (FrameView::tiles). `cur`: tiles a framebuffer word was written in during the finished frame
// -> resolved and cleared; `prev`: tiles whose image pixels may still hold something of the frame before -> background colour
// again, unless they are dirty now. A workgroup takes whole tiles (256 threads x 4 pixels), reads its tile's two flags, and
// leaves `prev` zeroed. Three arrays rotate: this launch's own prepass blocks mark the tiles of the NEXT frame in a third one
// (all zero since the turn before), `cur` is what the next turn reads as its `prev`, the zeroed `prev` is marked by the frame after.
template <bool HQS>
__global__ void __launch_bounds__(256) k_frame_turn_tiles(RenderArgs a, uint32_t prepass_blocks, int show_num_points, int colorize_chunks,
                                                          uint32_t width, uint32_t pixels, uint64_t *fb, uint64_t *rg, uint64_t *ba, uint32_t *rgba,
                                                          uint32_t n, uint64_t empty, TileFlags tf, uint32_t tiles_x)
{
    if (blockIdx.x < prepass_blocks) { lod_prepass_block(a, blockIdx.x); return; }
    const uint8_t *cur = tf.cur;
    uint8_t *prev = tf.prev;
    const uint32_t ntiles = tf.ntiles;
    const uint32_t row = threadIdx.x >> 4, col = (threadIdx.x & 15u) * 4u;
    const bool all_dirty = *tf.cur_all == tf.e_cur, all_was = *tf.prev_all == tf.e_prev;
    if (all_dirty) {
        // everything: the frame as k_frame_turn walks it (linear, 8-byte loads side by side), and `prev` zeroed on the way
        const uint32_t stride = (gridDim.x - prepass_blocks) * 256u, first = (blockIdx.x - prepass_blocks) * 256u + threadIdx.x;
        for (uint32_t t = first; t < ntiles; t += stride) prev[t] = 0;
        for (uint32_t i = first; i < n; i += stride) {
            if (i < pixels) {
                const uint32_t id = (uint32_t)fb[i];
                uint32_t color = PCR_BACKGROUND_COLOR;
                if (id < 0xFFFFFFFFu) {
                    if (show_num_points) {
                        const double div = HQS ? 512.0 : 64.0;
                        const uint32_t shade = (uint32_t)(((double)(float)(int)id / div) * 255.0);
                        color = (shade << 24) | (shade << 16) | (shade << 8) | shade;
                    } else if (colorize_chunks) {
                        color = id * 1234567u;
                    } else if (HQS) {
                        const uint64_t vrg = rg[i], vba = ba[i];
                        const uint32_t cnt = (uint32_t)vba;
                        if (cnt == 0) color = 0;
                        else color = (((uint32_t)(vba >> 32) / cnt) << 16) | (((uint32_t)vrg / cnt) << 8) | ((uint32_t)(vrg >> 32) / cnt);
                    } else {
                        color = id;
                    }
                }
                rgba[i] = color;
            }
            fb[i] = empty;
            if (HQS) { rg[i] = 0; ba[i] = 0; }
        }
        return;
    }
    for (uint32_t t = blockIdx.x - prepass_blocks; t < ntiles; t += gridDim.x - prepass_blocks) {       // (uniform)
        const bool dirty = cur[t] != 0, was = all_was || prev[t] != 0;
        if (!dirty && !was) continue;
        const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
        const uint32_t x = (tx << TILE_W_SHIFT) + col, y = (ty << TILE_H_SHIFT) + row;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t i = y * width + x + k;
            if (x + k >= width || i >= n) continue;
            if (!dirty) { if (i < pixels) rgba[i] = PCR_BACKGROUND_COLOR; continue; }
            if (i < pixels) {
                const uint32_t id = (uint32_t)fb[i];
                uint32_t color = PCR_BACKGROUND_COLOR;
                if (id < 0xFFFFFFFFu) {
                    if (show_num_points) {
                        const double div = HQS ? 512.0 : 64.0;
                        const uint32_t shade = (uint32_t)(((double)(float)(int)id / div) * 255.0);
                        color = (shade << 24) | (shade << 16) | (shade << 8) | shade;
                    } else if (colorize_chunks) {
                        color = id * 1234567u;
                    } else if (HQS) {
                        const uint64_t vrg = rg[i], vba = ba[i];
                        const uint32_t cnt = (uint32_t)vba;
                        if (cnt == 0) color = 0;
                        else color = (((uint32_t)(vba >> 32) / cnt) << 16) | (((uint32_t)vrg / cnt) << 8) | ((uint32_t)(vrg >> 32) / cnt);
                    } else {
                        color = id;
                    }
                }
                rgba[i] = color;
            }
            fb[i] = empty;
            if (HQS) { rg[i] = 0; ba[i] = 0; }
        }
        if (threadIdx.x == 0 && was) prev[t] = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// multi-GPU merges
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_merge_min(uint64_t *dst, const uint64_t *src, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        dst[i] = min(dst[i], src[i]);
}
__global__ void __launch_bounds__(256) k_merge_sum(uint64_t *dst, const uint64_t *src, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        dst[i] += src[i];
}
__global__ void __launch_bounds__(256) k_flip_sign(uint64_t *dst, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        dst[i] ^= 0x8000000000000000ull;
}

} // namespace pcr
