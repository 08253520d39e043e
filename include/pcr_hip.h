/*
 * pcr_hip.h — C ABI of libpcr_hip.so: the MI355X (gfx950) Huffman decode + rasterize path.
 *
 * This is the drop-in boundary for the reference's Huffman rendering methods. Each entry point names
 * the reference interface it replaces (paths relative to the reference checkout). The reference binds
 * its kernels through the CUDA driver API from C++ `Method`/`Resource` plugins; a maintainer replaces
 * those cu* calls with the functions below (INTEGRATION.md shows the adapter).
 *
 * Conventions: every function returns 0 on success or a negative PCR_E_* code; a human-readable
 * message is available from pcr_last_error(ctx) (ctx == NULL: message of the last failed pcr_create
 * on this thread). A context is externally synchronised (one caller thread at a time) and owns one
 * HIP stream on which all of its work is enqueued in call order; calls that return data to the host
 * synchronise that stream. No torch / C++ types cross this boundary.
 */
#ifndef PCR_HIP_H
#define PCR_HIP_H

#include "pcr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_OK            0
#define PCR_E_ARG        -1   /* bad argument / call order */
#define PCR_E_FORMAT     -2   /* malformed batch record or unsupported geometry */
#define PCR_E_HIP        -3   /* a HIP runtime call failed */
#define PCR_E_NOMEM      -4
#define PCR_E_NODEVICE   -5   /* no gfx950-class device / kernels not loadable */

typedef struct pcr_ctx pcr_ctx;

/* ---- lifecycle -------------------------------------------------------------------------------
 * replaces: cuInit/cuDeviceGet/cuCtxCreate (src/main.cpp:58-62) and the per-method
 * CudaProgram JIT (include/CudaProgram.h:15-70; here the code object is compiled ahead of time). */
int         pcr_create(int device, pcr_ctx **out);
void        pcr_destroy(pcr_ctx *ctx);
const char *pcr_last_error(const pcr_ctx *ctx);
/* Borrow an existing HIP stream (hipStream_t) instead of the context's own; NULL restores it (so the legacy default
 * stream, whose handle is NULL, cannot be borrowed: a caller that works on it has to create a stream and move there). Does
 * not synchronise: calls made afterwards are enqueued on the new stream, ordering against work already enqueued on the
 * previous one is the caller's (HIP events). */
int         pcr_set_stream(pcr_ctx *ctx, void *hip_stream);
int         pcr_synchronize(pcr_ctx *ctx);

/* ---- resource side: HuffmanLasData (modules/compute/HuffmanLasLoader.{h,cpp}) -------------------
 * pcr_stream_begin  <- HuffmanLasData::load buffer creation (HuffmanLasLoader.cpp:32-77): allocates the
 *                      stream buffers for `hdr` (+ zero pads, PCR_ENCODED_PAD_WORDS / PCR_SEPARATE_PAD_WORDS)
 *                      and zero-fills them. batch_index_base = global index of this context's first batch
 *                      when the file is sharded across GPUs (0 otherwise).
 * pcr_upload_batch  <- HuffmanLasData::uploadBatch (HuffmanLasLoader.cpp:176-299): `blob` is one batch
 *                      record (include/BatchDumpData.h:151-202), borrowed for the call. Batches must
 *                      arrive in index order 0,1,2,... (the reference's running offsets assume it too).
 * pcr_upload_tail   <- no reference counterpart (multi-GPU only): the first words of the batch that
 *                      follows this shard in the global stream, so that the reference's tail over-reads
 *                       see the same bytes as on one GPU. At most the pad sizes.
 * pcr_stream_unload <- HuffmanLasData::unload (HuffmanLasLoader.cpp:152-174). */
int     pcr_stream_begin(pcr_ctx *ctx, const pcr_file_header *hdr, int64_t batch_index_base);
int     pcr_upload_batch(pcr_ctx *ctx, int64_t batch_index, const void *blob, size_t n);
/* A whole loader task at once (HuffmanLasData::process hands over <= 100 records, HuffmanLasLoader.cpp:301-313):
 * records first_index .. first_index+count-1, validated up front (nothing is uploaded if one is malformed), packed
 * into pinned staging memory and moved with nine large asynchronous copies. The records may be released on return;
 * the copies complete in stream order before any later render call. Behind the copies the context also writes its own
 * HBM layout of the new batches (lane-major word order, packed decoder tables: DESIGN.md 4) — loading work, once per
 * batch, nothing decoded. */
int     pcr_upload_batches(pcr_ctx *ctx, int64_t first_index, int64_t count, const void *const *blobs, const size_t *sizes);
int     pcr_upload_tail(pcr_ctx *ctx, const uint32_t *encoded_words, size_t n_encoded,
                        const int32_t *separate_words, size_t n_separate);
int     pcr_stream_unload(pcr_ctx *ctx);
int64_t pcr_batches_loaded(const pcr_ctx *ctx);   /* HuffmanLasData::numBatchesLoaded */
int64_t pcr_points_loaded(const pcr_ctx *ctx);    /* HuffmanLasData::numPointsLoaded  */

/* ---- method side: HuffmanMemIter / HuffmanHQS ---------------------------------------------------
 * pcr_set_image_size <- cuMemAlloc(&fb, 8*2048*2048) (+RG, BA) in the method constructors
 *                       (modules/huffman_hqs/huffman_hqs.h:52-54); sized by resolution here
 *                       (pcr_fb_elems(w,h) u64 each) and cleared.
 * pcr_clear          <- the CLEAR block (huffman_hqs.h:266-270): fb <- all ones, RG/BA <- 0.
 * pcr_render_basic   <- cuLaunchKernel(renderProg) of HuffmanMemIter::render
 *                       (modules/huffman_mem_iter_cuda/huffman_mem_iter_cuda.h:185-195; kernel render.cu:315-540).
 * pcr_render_hqs_depth / pcr_render_hqs_color
 *                    <- the two launches of HuffmanHQS::render (huffman_hqs.h:191-213;
 *                       kernels huffman_hqs/depth.cu:166-397, huffman_hqs/render.cu:328-562).
 * pcr_resolve_basic / pcr_resolve_hqs
 *                    <- the RESOLVE blocks (huffman_mem_iter_cuda.h:226-247, huffman_hqs.h:240-263;
 *                       kernels resolve.cu:149-191, huffman_hqs/resolve.cu:2-47). Output is a device
 *                       RGBA8 buffer (no GL surface), read back with pcr_read_rgba.
 * All render/resolve calls only enqueue work. */
int pcr_set_image_size(pcr_ctx *ctx, int width, int height);
int pcr_clear(pcr_ctx *ctx);
int pcr_render_basic(pcr_ctx *ctx, const pcr_render_params *p);
int pcr_render_hqs_depth(pcr_ctx *ctx, const pcr_render_params *p);
int pcr_render_hqs_color(pcr_ctx *ctx, const pcr_render_params *p);
int pcr_resolve_basic(pcr_ctx *ctx, const pcr_render_params *p);
int pcr_resolve_hqs(pcr_ctx *ctx, const pcr_render_params *p);

/* ---- the 10-10-10 method: ComputeLasData + ComputeLoopLasCUDA ("loop_las_cuda") ---------------------
 * pcr_las_begin   <- ComputeLasData::load buffer creation (modules/compute/ComputeLasLoader.cpp:14-38): the batch
 *                    table and the four 4-byte-per-point arrays (three 10-10-10 levels + colour) for
 *                    ceil(num_points/65536) batches, zero-filled.
 * pcr_las_upload  <- ComputeLasData::process: upload + quantisation dispatch (ComputeLasLoader.cpp:140-262, computeLasLoader.cs):
 *                    `count` batches starting at first_batch, already quantised (pcr_las_quantize, pcr_encode.h);
 *                    batches arrive in index order. Arrays are borrowed for the call.
 * pcr_las_unload  <- ComputeLasData::unload (ComputeLasLoader.cpp:114-131).
 * pcr_render_las  <- cuLaunchKernel(renderProg) of ComputeLoopLasCUDA::render (modules/compute_loop_las_cuda/
 *                    compute_loop_las_cuda.h:164-182; kernel render.cu:130-442): one workgroup per loaded batch, the
 *                    last one does not draw (render.cu:201-202). Keys are depth<<32 | point index.
 * pcr_resolve_las <- the resolve launch (compute_loop_las_cuda.h:185-207; kernel resolve.cu): pixel <- colour of the
 *                    winning point index, background 0x00443322; all pixels (the reference skips partial 16x16 tiles).
 * pcr_las_algorithmic_bytes: HBM bytes the last pcr_render_las had to read at least once (4/8/12 B per point by
 *                    level + 64 B per drawn batch, + 4 B per point of colour after pcr_render_las_hqs_color); synchronises.
 *
 * ---- the 10-10-10 HQS method: ComputeLoopLasHqs ("loop_las_hqs", modules/compute_loop_las_hqs) ---------------------
 * A frame is pcr_clear -> pcr_render_las_hqs_depth -> pcr_render_las_hqs_color -> pcr_resolve_hqs (compute_loop_las_hqs.h:170-300).
 * Both passes draw the batches pcr_render_las draws, at the same levels, with the same positions; errors, stats, kernel timing
 * and the no-op on 0 batches are those of pcr_render_las.
 * pcr_render_las_hqs_depth <- the DEPTH dispatch (compute_loop_las_hqs.h:170-196; shader depth.cs:335-355): key depth<<32 with
 *                    payload 0, so fb >> 32 is the basic frame's depth half at every pixel, the low word 0 where a point landed.
 * pcr_render_las_hqs_color <- the COLORS dispatch (compute_loop_las_hqs.h:198-223; shader color.cs:360-405): a point is averaged
 *                    into its pixel iff w <= d * 1.01f, d the pixel's depth -- an f32 product as color.cs:370 (the Huffman HQS
 *                    pass compares in f64); RG += R<<32 | G, BA += B<<32 | 1 (the Huffman HQS packing; color.cs:399-400 packs
 *                    R | G<<32), so pcr_resolve_hqs, pcr_read_accum and pcr_merge_sum take these sums unchanged. The next
 *                    pcr_clear zeroes RG / BA.
 * pcr_resolve_hqs  <- the RESOLVE dispatch (compute_loop_las_hqs.h:225-245; shader resolve.cs). Its debug modes (show_num_points,
 *                    colorize_chunks) read the depth word's payload, which is 0 here: out of scope for this method.
 * Deviations from the GLSL method, each keeping the two 10-10-10 methods consistent: the CUDA method's level function
 * (compute_loop_las_cuda/render.cu:157-197, not color.cs:180-205), 1024-thread workgroups (not 128), the last loaded batch
 * is not drawn (render.cu:201-202), the accumulator packing above. */
int     pcr_las_begin(pcr_ctx *ctx, int64_t num_points);
int     pcr_las_upload(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_xyz_batch *batches,
                       const uint32_t *xyz12, const uint32_t *xyz8, const uint32_t *xyz4, const uint32_t *rgba);
int     pcr_las_unload(pcr_ctx *ctx);
int64_t pcr_las_batches_loaded(const pcr_ctx *ctx);
int     pcr_render_las(pcr_ctx *ctx, const pcr_render_params *p);
int     pcr_render_las_hqs_depth(pcr_ctx *ctx, const pcr_render_params *p);
int     pcr_render_las_hqs_color(pcr_ctx *ctx, const pcr_render_params *p);
int     pcr_resolve_las(pcr_ctx *ctx, const pcr_render_params *p);
int64_t pcr_las_algorithmic_bytes(pcr_ctx *ctx);

/* ---- display resolves: n x n point size and eye-dome lighting -------------------------------------------
 * pcr_resolve_basic_display / pcr_resolve_hqs_display / pcr_resolve_las_display <- the resolve of the reference's GLSL 10-10-10
 * method (modules/compute_loop_las/resolve.cs: :98-128 the "n x n pixel" loop over `window`, :41-62 and :143-185 eye-dome
 * lighting over `edlWindow`), which the reference never brought to its CUDA / Huffman methods. Each is called where its plain
 * counterpart (pcr_resolve_basic / _hqs / _las) is, with the same preconditions, and only enqueues on the context's stream. It
 * writes the context's RGBA8 image (pcr_read_rgba / pcr_device_rgba) and nothing else: the framebuffer, RG / BA, the prepass
 * state, the tile flags and the statistics stay as they are. It reads whichever buffers the context uses (external ones, and
 * either empty word: pcr_set_int64_mergeable). With window == 0 and edl_window == 0 the image is the plain resolve's, byte for byte.
 *
 * Pixel (x, y), 0 <= x < width, 0 <= y < height, has index x + y * width; a window is the square of the given radius around a
 * pixel, CLIPPED to the image.
 *  1. D(x, y) = the 64-bit unsigned minimum of the framebuffer's words over the window of radius opts->window. This is the frame
 *     that drawing every point as a (2 * window + 1)^2 square with the 64-bit atomicMin would leave (for points whose own pixel is
 *     in the image), at the cost of a stencil over the pixels instead of window^2 atomics per point.
 *  2. colour: basic -- D through pcr_resolve_basic's arithmetic (background, show_num_points, colorize_chunks included); las -- D
 *     through pcr_resolve_las's (the colour of point index D & 0xFFFFFFFF, background for an empty D); hqs -- background for an
 *     empty D, the debug flags on D's low word as pcr_resolve_hqs, else the 64-bit sums of RG and BA over the window's pixels n
 *     that are drawn and whose OWN depth d_n <= d * 1.01f (d = the depth half of D; one rounded f32 product, color.cs:370),
 *     divided as pcr_resolve_hqs divides (count 0: colour 0).
 *  3. eye-dome lighting, when opts->edl_window = e > 0, of every pixel with a non-empty D (background is never shaded), on the
 *     DILATED depths d(.) = D >> 32 as f32: response = (sum over ox = -e..e (outer), oy = -e..e (inner) of max(0, d(c) - d(n)),
 *     0 for n outside the image or with an empty D, accumulated in f32) / (2e+1)^2; shade = expf((-response * 300.0f) *
 *     opts->edl_strength); bytes 0..2 <- (uint32_t)((float)byte * shade), byte 3 <- 0 (resolve.cs:169-182).
 * Deviations from resolve.cs: windows are clipped to the image (the shader reads through the linear pixel index and so wraps
 * into the neighbouring rows at the left and right edges); the dilated word is the minimum of the whole 64-bit word, this
 * project's rule for depth ties (the shader compares depths only and breaks ties by loop order) -- that is what makes step 1
 * equal to drawing squares; EDL of a frame with window > 0 runs on the dilated depths. The hqs colour APPROXIMATES square
 * splats under the 1 % rule: a neighbour's RG / BA sums were filtered by the colour pass against that neighbour's own front
 * depth, not against d.
 * PCR_E_ARG, with a message and the image untouched: opts NULL; window outside [0, PCR_DISPLAY_MAX_WINDOW]; edl_window outside
 * [0, PCR_DISPLAY_MAX_EDL_WINDOW]; edl_strength NaN, infinite or negative while edl_window > 0; reserved != 0; and whatever the
 * plain resolve refuses. The whole frame is walked (the tile flags are not consulted). */
int pcr_resolve_basic_display(pcr_ctx *ctx, const pcr_render_params *p, const pcr_display_opts *opts);
int pcr_resolve_hqs_display(pcr_ctx *ctx, const pcr_render_params *p, const pcr_display_opts *opts);
int pcr_resolve_las_display(pcr_ctx *ctx, const pcr_render_params *p, const pcr_display_opts *opts);

/* Counters of the most recent render call (synchronises). */
int pcr_get_stats(pcr_ctx *ctx, pcr_render_stats *out);

/* ---- readback (the reference's cuMemcpyDtoH depth dump, huffman_hqs.h:217-237, generalised) ----- */
int pcr_read_framebuffer(pcr_ctx *ctx, uint64_t *host, size_t n_elems);          /* n_elems <= pcr_fb_elems(w,h) */
int pcr_read_accum(pcr_ctx *ctx, uint64_t *host_rg, uint64_t *host_ba, size_t n_elems);
int pcr_read_rgba(pcr_ctx *ctx, uint32_t *host, size_t n_pixels);                /* n_pixels <= w*h */

/* ---- multi-GPU plumbing (no reference counterpart) ------------------------------------
 * Device pointers of the context's buffers so a collective library (RCCL through torch.distributed)
 * can reduce them in place, or externally owned buffers to render into. */
/* The loaded stream back to points. The reference has no counterpart: its only decoder outside the render kernels is the
 * per-chain CPU one of include/huffman.h:433-477. Decodes batches [first_batch, first_batch + count) of the loaded stream into
 * dev_points (device memory of the context's device, capacity_points records, 16-byte aligned): all 64 points of all 1024
 * chains of every batch, no cull, no level of detail, the tail artefact of the reference's interleave
 * included -- exactly the points the render kernels draw. Point i of chain c of batch b is record
 * (b - first_batch) * 65536 + c * 64 + i, the stream's own order; the colour is 0x00BBGGRR (BC1 or BC7 by the stream's format)
 * as pcr_encode_points takes it. count < 0: up to the last batch the next frame would draw (pcr_batches_resident); with
 * pcr_set_async_upload on, only those batches may be decoded. count == 0 succeeds and does nothing. Works before and after the
 * first frame (it reads what the render kernels read, from either layout; with PCR_LAYOUT_BOTH the one pcr_set_render_variant
 * names, AUTO: the point windows). Enqueues on the context's stream; touches no framebuffer, no prepass state, no statistics.
 * PCR_E_ARG: no stream loaded, a range outside the resident batches, capacity_points < count * 65536, a NULL or misaligned
 * pointer. */
int pcr_decode_points(pcr_ctx *ctx, int64_t first_batch, int64_t count, void *dev_points, size_t capacity_points);
/* The same into host memory: staged through a device buffer of the context, 64 batches (64 MiB) at a time; synchronises. */
int pcr_read_points(pcr_ctx *ctx, int64_t first_batch, int64_t count, pcr_point *host, size_t capacity_points);

/* ---- box selection: a spatial read on the decode path (no reference counterpart) -----------------------------------------
 * CONTRACT: the output of pcr_select_box equals pcr_decode_points of the same range with the records outside the box removed,
 * byte for byte -- the same 16-byte records in the same relative order, packed without gaps; padding duplicates and the tail
 * artefact are points like any other; BC1 and BC7, either resident layout, before and after the first frame.
 *
 * pcr_batch_point_bounds: host_bounds[i * 6 ..] = min x, y, z, max x, y, z over all 65 536 records pcr_decode_points writes for
 *   batch first_batch + i: exact integers, computed on the GPU (k_point_bounds, about one colourless decode pass) and cached in
 *   the context per batch; the cache is dropped by pcr_stream_begin / pcr_stream_unload and grows as batches become resident.
 *   (pcr_gpu_batch::min/max are single-precision hints and do not cover the tail artefact.) Synchronises.
 * pcr_select_box: the records of batches [first_batch, first_batch + count) inside *box (bounds inclusive) to dev_points, their
 *   number to *out_count. Range semantics, count < 0 and the restriction under pcr_set_async_upload are pcr_decode_points'.
 *   Batches whose exact box misses the query are not decoded, those wholly inside go through the full-batch decode, the ones
 *   that straddle it are counted (k_select_count) and then written (k_select_write). dev_points == NULL only counts. A
 *   capacity_points below the result: PCR_E_ARG, *out_count = the count needed, nothing written. An empty box, or a range of
 *   0 batches: 0 records, PCR_OK. Synchronises (the host has to learn the count). Touches no framebuffer, no prepass state, no
 *   render statistics. stats may be NULL.
 * pcr_read_box: the same into host memory, staged through the context's decode staging buffer 64 batches at a time.
 * PCR_E_ARG with a message: no stream loaded, a range outside the resident batches, a NULL box, a NULL out_count, a misaligned
 * pointer (16 bytes on the device, alignof(pcr_point) on the host). */
int pcr_batch_point_bounds(pcr_ctx *ctx, int64_t first_batch, int64_t count, int32_t *host_bounds);
int pcr_select_box(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_box *box, void *dev_points, size_t capacity_points,
                   int64_t *out_count, pcr_select_stats *stats);
int pcr_read_box(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_box *box, pcr_point *host, size_t capacity_points,
                 int64_t *out_count, pcr_select_stats *stats);

/* ---- polygon selection: the stream clipped to a polygon prism (no reference counterpart) --------------------------------------
 * CONTRACT: pcr_select_polygon / pcr_read_polygon are pcr_select_box / pcr_read_box in every respect except the predicate: the
 * output equals pcr_decode_points of the same range with the unselected records removed, byte for byte, in the same order,
 * packed without gaps; padding duplicates and the tail artefact are points like any other; BC1 and BC7, either resident layout
 * (PCR_LAYOUT_BOTH follows pcr_set_render_variant), before and after the first frame; dev_points == NULL only counts; a capacity
 * below the result is PCR_E_ARG with *out_count = the count needed and nothing written; range semantics, count < 0 and the
 * restriction under pcr_set_async_upload are pcr_decode_points'. Synchronises. Touches no framebuffer, no prepass state, no
 * render statistics. stats may be NULL. The predicate is pcr_polygon's (pcr_types.h): all integer, all exact.
 *
 * How a batch is treated, from its exact box (pcr_batch_point_bounds): R is the closed xy rectangle of the box, [zb0, zb1] its z
 * range. An edge, horizontal ones included, is near if its bounding rectangle overlaps R. With no near edge every point of R has
 * the same in_poly, evaluated at R's min corner. The xy verdict is all in (no near edge, the corner value differs from the
 * invert flag), all out (no near edge, it equals the flag) or mixed (a near edge); the z verdict is all in, all out or mixed
 * from [zb0, zb1] against [z_min, z_max]. A batch is outside (not decoded) if either verdict is all out, inside (decoded whole
 * by the full-batch decode) if both are all in, else straddling: counted (k_polygon_count), then written (k_polygon_write).
 * A straddling batch tests its points against its own slice of one edge array (uploaded per call; scratch of the context,
 * grown on demand, released with it): the non-horizontal edges whose [l.y, u.y) meets R's rows and whose max x is above R's min
 * x, except those that lie wholly right of R with [l.y, u.y) covering all of R's rows, which every point of R counts and which
 * are folded into one parity bit of the batch. The kernels test a point against the z range and the vertices' bounding
 * rectangle before any edge, so every difference fits 32 bits and every product stays below 2^62.
 * PCR_E_ARG with a message, nothing written: a NULL polygon, xy, ring_sizes or out_count; num_rings < 1 or a ring of fewer than
 * 3 vertices; more than PCR_POLY_MAX_VERTICES vertices; unknown flag bits or reserved != 0; vertices that span more than
 * 2^31 - 1 on x or y; a misaligned destination; whatever pcr_select_box refuses about the range. */
int pcr_select_polygon(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_polygon *poly, void *dev_points, size_t capacity_points,
                       int64_t *out_count, pcr_polygon_stats *stats);
int pcr_read_polygon(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_polygon *poly, pcr_point *host, size_t capacity_points,
                     int64_t *out_count, pcr_polygon_stats *stats);

/* ---- slabs: plane hypotheses and oriented selections (no reference counterpart) ------------------------------------------------
 * A pcr_slab (pcr_types.h) is one linear form with two bounds, lo <= n.p <= hi, taken in exact 64-bit integers: a plane with a
 * tolerance, with one bound at the limit a half-space, several together an oriented box, a frustum, a tilted cross-section.
 *
 * CONTRACT of pcr_plane_support: the candidates are the records pcr_decode_points writes for the range (padding duplicates and
 * the tail artefact included) that lie inside clip (NULL: all) and are in NO slab of exclude; host_counts[j] = the number of
 * candidates in hyp[j]. 1 <= num_hyp <= PCR_PLANE_MAX_HYPOTHESES, 0 <= num_exclude <= PCR_SLAB_MAX_EXCLUDE. Sums commute: the
 * result is exact, the same from run to run, for both layouts, for BC1 and BC7 (no colour is decoded), before and after the
 * first frame. Synchronises. Touches no framebuffer, no prepass state, no render statistics. stats may be NULL. An empty clip
 * or an empty range gives all zeros.
 * The host plan, per batch from its exact box (pcr_batch_point_bounds): a box disjoint from the clip, or an exclusion of class
 * ALL: skipped. The exclusions of class CUT form the batch's exclusion slice. The batch is open iff its box lies within the clip
 * and that slice is empty: every record of an open batch is a candidate. A hypothesis of class MISS adds nothing; one of class
 * ALL adds the batch's candidate count (65 536 for an open batch, else what the kernel reports for the batch); those of class
 * CUT form the batch's hypothesis slice. A batch is decoded (one workgroup of k_plane_support, its slices in LDS) iff that slice
 * is not empty, or it is not open and has an ALL hypothesis; a batch neither skipped nor decoded is whole.
 * PCR_E_ARG with a message: NULL hyp or host_counts; counts out of range; exclude == NULL with num_exclude > 0; reserved != 0;
 * a normal component or a bound beyond its limit; whatever pcr_select_box refuses about the range. */
int pcr_plane_support(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_slab *hyp, int num_hyp, const pcr_box *clip,
                      const pcr_slab *exclude, int num_exclude, int64_t *host_counts, pcr_plane_stats *stats);

/* CONTRACT: pcr_select_slabs / pcr_read_slabs are pcr_select_polygon / pcr_read_polygon with another predicate: a record is
 * selected iff it lies inside clip (NULL: all) and (it is in ALL of slabs[0 .. num_slabs)) != (flags & PCR_SLAB_INVERT), with
 * 1 <= num_slabs <= PCR_SLAB_MAX_SELECT. Output, order, counting call, capacity rule, layouts, colour formats and what is left
 * alone are pcr_select_box's. A batch is outside (not decoded) if the clip or any slab misses its box, inside (decoded whole) if
 * its box lies within the clip and every slab is ALL, else straddling (k_slab_count, then k_slab_write, against the batch's CUT
 * slabs in LDS). With PCR_SLAB_INVERT the slab classes swap: a slab that misses the box selects all of it, slabs that are all
 * ALL none of it.
 * PCR_E_ARG with a message, nothing written: what pcr_plane_support refuses about a slab list; unknown flag bits; a NULL
 * out_count; a misaligned destination; whatever pcr_select_box refuses about the range. */
int pcr_select_slabs(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_slab *slabs, int num_slabs, const pcr_box *clip,
                     uint32_t flags, void *dev_points, size_t capacity_points, int64_t *out_count, pcr_slab_stats *stats);
int pcr_read_slabs(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_slab *slabs, int num_slabs, const pcr_box *clip,
                   uint32_t flags, pcr_point *host, size_t capacity_points, int64_t *out_count, pcr_slab_stats *stats);

/* ---- screen selection and picking: which points does a frame show, and where (no reference counterpart) -----------------------
 * CONTRACT of pcr_select_screen: the selected points are exactly those pcr_render_basic(params) scatters -- the batches its
 * cull/LOD prepass keeps, of each chain the first points by the prepass's level of detail, each batch dequantised in the
 * precision (f32 / f64) the prepass chose, and of those the points that pass the kernel's inside test (w > 0, NaNs rejected,
 * pixel index below pcr_fb_elems) -- whose pixel lies in *rect. (The basic method's LOD expression is used for every stream, a
 * BC7 stream included, which pcr_render_basic itself refuses; the HQS passes round one division differently and agree except
 * on a batch exactly at a level's edge.) hit.pixel and hit.depth_bits are bit-identical to what the render kernel computes for
 * the point: for a BC1 stream, the minimum of depth_bits << 32 | colour over the hits of a pixel is the word pcr_render_basic
 * leaves there. params are checked as a render call checks them (pcr_set_image_size first); show_num_points and
 * colorize_chunks have no effect.
 * rect: pixel bounds, inclusive, clipped to the image [0, width) x [0, height); NULL = the whole image. Column and row of a
 * point are those of its pixel index (pixel % width, pixel / width), so the few points at ndc == 1.0, which the kernels
 * scatter to column `width` = column 0 of the next row, are found there, and those in the framebuffer's extra row `height` are
 * in no rect.
 * dev_points gets the 16-byte records pcr_decode_points writes for the selected points, dev_hits the parallel pcr_screen_hit
 * array; both in increasing hit.index order, packed without gaps; capacity counts records of each. Either may be NULL to skip
 * that array, both NULL only counts. A capacity below the result: PCR_E_ARG, *out_count = the count needed, nothing written.
 * An empty rect or no resident batches: 0 records, PCR_OK. BC1 and BC7, either resident layout (PCR_LAYOUT_BOTH follows
 * pcr_set_render_variant, AUTO: the point windows), before and after the first frame; with pcr_set_async_upload on, the
 * batches the next frame would draw. Synchronises. Touches no framebuffer and no render statistics, and leaves the prepass
 * state of a pending pcr_frame_begin as it is (the cull/LOD decision is recomputed into an array of the selection's own).
 * Batches are skipped by the prepass's cull alone: no exact screen box per batch is at hand (pcr_gpu_batch::min/max do not
 * cover the tail artefact), so every kept batch is decoded whatever the rect.
 * pcr_read_screen: the same into host memory (either pointer may be NULL), staged through the context's decode staging buffer.
 * PCR_E_ARG with a message: what a render call refuses, a NULL out_count, a misaligned pointer (16 bytes on the device).
 *
 * pcr_pick: the window is the square of `radius` pixels around (px, py), clipped to the image; among the hits of
 * pcr_select_screen in it the winner is the least by (depth_bits, colour, index). *out_found = 0: no point in the window (not
 * an error; (px, py) outside the image with a window that misses it entirely is that case too). out_point / out_hit may be
 * NULL. For a BC1 stream and radius 0, depth_bits << 32 | colour of the winner is the word pcr_render_basic leaves at the
 * pixel. Scratch memory is a few words whatever the number of candidates: k_pick<key> takes the 64-bit minimum of
 * depth << 32 | colour, k_pick<index> the minimum index among the points that hold it, k_pick_fetch returns the record.
 * radius < 0: PCR_E_ARG. Synchronises; state as pcr_select_screen. */
int pcr_select_screen(pcr_ctx *ctx, const pcr_render_params *params, const pcr_rect *rect, void *dev_points, void *dev_hits,
                      size_t capacity, int64_t *out_count, pcr_screen_stats *stats);
int pcr_read_screen(pcr_ctx *ctx, const pcr_render_params *params, const pcr_rect *rect, pcr_point *host_points,
                    pcr_screen_hit *host_hits, size_t capacity, int64_t *out_count, pcr_screen_stats *stats);
int pcr_pick(pcr_ctx *ctx, const pcr_render_params *params, int px, int py, int radius, pcr_point *out_point,
             pcr_screen_hit *out_hit, int *out_found);

/* ---- visible selection: the points that make up the picture, occlusion-aware (no reference counterpart) -------------------------
 * CONTRACT of pcr_select_visible, in terms of pcr_select_screen's hits (same kept batches, level of detail, precision, inside
 * test, pixel and depth_bits). A pixel is a linear index p < width * height, column p % width, row p / width; hits of the
 * framebuffer's extra row (pixel >= width * height) are never selected and never occlude.
 *   D[p]   the least depth_bits over ALL hits of pixel p in the whole image, whatever the rect; 0xFFFFFFFF without a hit
 *          (w > 0, so the order of the bits is the order of w)
 *   Dr[p]  the least D over the pixels whose column and row both lie within `radius` of p's, inside the image;
 *          radius 0 .. PCR_VISIBLE_MAX_RADIUS, and radius 0 gives Dr = D. A radius above 0 makes this hidden-point removal
 *          for a cloud with gaps: the background seen through a hole between foreground points is occluded by their depths.
 *   surface test  a hit passes iff (double)w <= (double)dr * 1.01, w and dr the floats of depth_bits and Dr[pixel]: the HQS
 *          colour pass's rule, an f64 product
 *   PCR_VISIBLE_SURFACE  every hit in the rect that passes the surface test. At radius 0 these are the points whose colours
 *          pcr_render_hqs_color averages (where both LOD expressions agree).
 *   PCR_VISIBLE_FRONT    of every pixel in the rect the one hit that is least by (depth_bits, colour, index) -- pcr_pick's
 *          order, colour the record's 0x00BBGGRR -- if it passes the surface test (at radius 0 it always does). For a BC1
 *          stream and radius 0 these are the points whose words pcr_render_basic leaves in the framebuffer.
 * dev_points / dev_hits get the pcr_point and pcr_screen_hit records of the selected hits, in increasing index order, packed;
 * dev_depth gets uint32[width * height], the plane Dr of the whole image whatever the rect. Any pointer may be NULL; all three
 * NULL only counts. A capacity below the result with dev_points or dev_hits given: PCR_E_ARG, *out_count = the count needed,
 * nothing written (the depth plane neither). stats may be NULL.
 * An empty rect or no resident batch: 0 records, PCR_OK (the depth plane and the image's counts are still worked out).
 * Synchronises. Touches no framebuffer, no render statistics and no pending pcr_frame_begin state. The per-pixel planes (24
 * bytes a pixel) are scratch of the context, grown on demand.
 * PCR_E_ARG with a message: what pcr_select_screen refuses, an unknown mode, a radius outside the range, a misaligned dev_depth
 * (4 bytes).
 * pcr_read_visible: the same into host memory. */
int pcr_select_visible(pcr_ctx *ctx, const pcr_render_params *params, const pcr_rect *rect, int mode, int radius,
                       void *dev_points, void *dev_hits, void *dev_depth, size_t capacity, int64_t *out_count,
                       pcr_visible_stats *stats);
int pcr_read_visible(pcr_ctx *ctx, const pcr_render_params *params, const pcr_rect *rect, int mode, int radius,
                     pcr_point *host_points, pcr_screen_hit *host_hits, uint32_t *host_depth, size_t capacity,
                     int64_t *out_count, pcr_visible_stats *stats);

/* ---- top-down grid: the stream rasterized into height / colour / density planes (no reference counterpart) ------------------
 * CONTRACT: after pcr_grid_clear and pcr_grid_accumulate over a range, every cell of a plane holds the max / min / count
 * (pcr_grid in pcr_types.h) over exactly the records pcr_decode_points writes for that range that fall into the cell and into
 * *clip -- padding duplicates and the tail artefact included; BC1 and BC7, either resident layout, before and after the first
 * frame. Max, min and add do not depend on the order, so the planes are exact and the same from run to run. One pass over the
 * compressed stream; no record is written anywhere.
 *
 * The planes are device arrays of width * height cells, row cy at cy * width: dev_top / dev_bottom uint64 (8-byte aligned),
 * dev_count uint32 (4-byte aligned). Any of them may be NULL: that plane is left out (with neither top nor bottom the colours
 * are not decoded).
 * pcr_grid_clear: the empty values into the planes given. Only enqueues.
 * pcr_grid_accumulate: the points of batches [first_batch, first_batch + count) into the planes, on top of what they hold, so
 *   several ranges, shards, contexts or streams can fill one grid (order the calls of different contexts yourself). Range
 *   semantics, count < 0 and the restriction under pcr_set_async_upload are pcr_decode_points'. Points outside *clip (NULL: no
 *   clip) are ignored. The host puts every batch into a class from its exact box (pcr_batch_point_bounds' cache, filled on first
 *   use: that call synchronises) against grid and clip: outside -- the box misses them on x, y or z, the batch is not decoded;
 *   windowed -- the rectangle of cells the box covers inside them has at most PCR_GRID_WINDOW_CELLS cells: the workgroup
 *   accumulates in LDS and merges with one global atomic per non-empty cell and plane; direct -- more cells than that: a global
 *   atomic per point and plane. PCR_GRID_NO_WINDOW in flags makes every batch that is not outside direct. *stats (may be NULL)
 *   tells the three counts. With the boxes cached the call only enqueues (a list of a few words per batch is uploaded). Touches
 *   no framebuffer, no prepass state, no render statistics. All three planes NULL: PCR_OK, no work, *stats zero. An empty clip,
 *   or a range of 0 batches: PCR_OK, every batch outside.
 * pcr_grid_unpack: per cell of dev_words (a top or a bottom plane, `which` = PCR_GRID_TOP / PCR_GRID_BOTTOM tells the empty
 *   value) dev_height[i] = z of the word, INT32_MIN for an empty cell; dev_rgba[i] = colour | 0xFF000000, 0 for an empty cell.
 *   Either output may be NULL. Only enqueues.
 * pcr_read_grid: clear + accumulate + copy to the host (any of the three may be NULL) through scratch memory of the context,
 *   grown on demand and released with it. Synchronises.
 * PCR_E_ARG with a message, nothing written: no stream loaded, a range outside the resident batches, a NULL grid, cell < 1,
 * width or height < 1, more than PCR_GRID_MAX_CELLS cells, reserved != 0, unknown flag bits or `which`, a misaligned pointer. */
int pcr_grid_clear(pcr_ctx *ctx, const pcr_grid *grid, void *dev_top, void *dev_bottom, void *dev_count);
int pcr_grid_accumulate(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip,
                        void *dev_top, void *dev_bottom, void *dev_count, uint32_t flags, pcr_grid_stats *stats);
int pcr_grid_unpack(pcr_ctx *ctx, const pcr_grid *grid, const void *dev_words, int which, void *dev_height, void *dev_rgba);
int pcr_read_grid(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip,
                  uint64_t *host_top, uint64_t *host_bottom, uint32_t *host_count, uint32_t flags, pcr_grid_stats *stats);

/* ---- height percentiles per grid cell: exact order statistics of z (no reference counterpart) --------------------------------
 * CONTRACT: a record is a candidate of cell c iff it is one of the records pcr_decode_points writes for the range (padding
 * duplicates and the tail artefact included), lies inside clip (NULL: all), falls into cell c of *grid by pcr_grid's cell rule
 * exactly, and z >= floor[c] (dev_floor: int32[height * width], or NULL for no test; a floor of INT32_MIN admits every point of
 * its cell). For a cell with n >= 1 candidates whose z sorted ascending are z_0 <= ... <= z_{n-1}, plane j holds z_k with
 *   k = (q[j] * (n - 1) + PCR_QUANTILE_ONE / 2) / PCR_QUANTILE_ONE      (unsigned 64-bit integer division)
 * -- the nearest rank, a half rounded up: q = 0 the lowest z, q = 10000 the highest, never an interpolated value. A cell with
 * n == 0 holds INT32_MIN (PCR_GROUND_EMPTY, what pcr_grid_unpack writes; a real z == INT32_MIN cannot be told from empty, as
 * there). An order statistic of a multiset does not depend on the order of its elements: the planes are exact, the same from
 * run to run and for every layout and flag.
 * dev_quantiles: int32[num_q][height * width], plane-major, every plane a raster with the layout of pcr_grid_unpack's height
 *   plane (a low percentile can go to pcr_ground_filter as dev_lowest unchanged), or NULL: then no z is bucketed.
 * dev_count: uint32[height * width], the candidates per cell (with a floor: the numerator of canopy cover), or NULL. With both
 *   NULL the call still fills *stats (may be NULL itself).
 * 1 <= num_q <= PCR_QUANTILES_MAX, every q[j] <= PCR_QUANTILE_ONE, in any order, repeats allowed. flags: 0 or
 *   PCR_GRID_NO_WINDOW, as for pcr_grid_accumulate (the batch classes in *stats are that call's).
 * Every cell of every plane asked for is written: no clear call is needed. The call synchronises (the host sizes the scratch
 * from the candidate count). It touches no framebuffer, no prepass state and no render statistics, supports BC1 and BC7 and
 * either resident layout, and works before and after the first frame. Scratch memory of the context, grown on demand and
 * released with it: 12 to 16 bytes per cell and 4 bytes per candidate.
 * Cost: count and fill are two colourless decode passes; the selection reads a cell of m candidates 1 + 3 * num_q times at most
 * in a single workgroup, so a grid that puts the whole stream into one cell is slow, not wrong; stats->max_cell_points tells.
 * pcr_read_grid_quantiles: the same with host memory for the floor and both outputs, through scratch memory of the context.
 * PCR_E_ARG with a message, nothing written: pcr_grid_accumulate's refusals about range, grid and flags; num_q outside 1 ..
 * PCR_QUANTILES_MAX; a q above PCR_QUANTILE_ONE; q == NULL; a destination or floor misaligned to 4 bytes; a range of more than
 * PCR_QUANTILE_MAX_BATCHES batches (the counts and offsets are 32 bits). PCR_E_NOMEM names the scratch size. */
int pcr_grid_quantiles(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip,
                       const void *dev_floor, const uint32_t *q, int32_t num_q, void *dev_quantiles, void *dev_count, uint32_t flags,
                       pcr_quantile_stats *stats);
int pcr_read_grid_quantiles(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip,
                            const int32_t *host_floor, const uint32_t *q, int32_t num_q, int32_t *host_quantiles, uint32_t *host_count,
                            uint32_t flags, pcr_quantile_stats *stats);

/* ---- ground model and heights above it: lasground + lasheight on the grid (no reference counterpart) ---------------------------
 * pcr_ground_filter turns a lowest-point height plane (pcr_grid's bottom plane through pcr_grid_unpack) into a ground plane;
 * pcr_select_height is pcr_select_box with a predicate that looks the record's cell up in such a plane. All integer, all exact.
 *
 * pcr_ground_filter: dev_lowest and dev_ground are int32[height * width] (4-byte aligned, index cx + cy * width as in
 *   pcr_grid), dev_class uint8[height * width] or NULL. dev_ground must not be dev_lowest. Of *grid only width and height play
 *   a part. With Z0 the input plane and EMPTY = PCR_GROUND_EMPTY:
 *   1. A cell is empty iff Z0[c] == EMPTY (a real z == INT32_MIN cannot be told from an empty cell, as after pcr_grid_unpack).
 *   2. A = Z0, F = 0. W_r(c) = the cells within r of c on both axes that lie inside the grid.
 *   3. For k = 0 .. num_steps - 1, r = radius[k], t = threshold[k]: E[c] = the minimum of A over the non-empty cells of W_r(c)
 *      (EMPTY if there is none), O[c] = the maximum of E over the non-EMPTY cells of W_r(c) (likewise); for every non-empty c
 *      (O[c] <= A[c] holds): F[c] = 1 if (int64)A[c] - O[c] > t; then A[c] = O[c]. Empty cells stay EMPTY in A.
 *   4. Classes: empty -> PCR_CELL_EMPTY, F[c] -> PCR_CELL_NONGROUND, else PCR_CELL_GROUND. H[c] = Z0[c] for ground cells, EMPTY
 *      for the others.
 *   5. Fill, in Jacobi rounds that read the previous round's plane: every EMPTY cell with m >= 1 non-EMPTY cells among its 8
 *      neighbours inside the grid takes floor(sum / m), the sum in 64 bits, the floor toward minus infinity. Rounds end when
 *      fill_rounds have run, no cell is EMPTY, or a round fills nothing. dev_ground = H; unfilled cells stay EMPTY.
 *   Heights from INT32_MIN + 1 to INT32_MAX are legal beside empties: the kernels carry "empty" as a flag in a wider word.
 *   How: k_ground_morph is one separable pass (row or column, minimum or maximum, any radius up to 64) over a tile and its halo
 *   in LDS, four launches a step; k_ground_flag compares and flags; k_ground_class writes classes, H and the class counts;
 *   k_ground_fill is one round between two planes and counts what it filled and what stayed EMPTY; the host reads the two
 *   counters back after every round, so the result does not depend on when it looks. Scratch: three int32 planes and a byte
 *   plane in the scratch memory pcr_read_grid uses, grown on demand and released with the context. Synchronises. Needs no
 *   stream loaded; touches no framebuffer, no prepass state, no render statistics. stats may be NULL.
 *   PCR_E_ARG with a message, nothing written: a NULL grid, params, dev_lowest or dev_ground; width or height < 1 or more than
 *   PCR_GRID_MAX_CELLS cells; num_steps outside 0 .. 16; fill_rounds outside 0 .. 4096; a radius outside 1 .. 64 or a negative
 *   threshold for k < num_steps; dev_ground == dev_lowest; a misaligned plane.
 * pcr_read_ground: pcr_grid_clear + pcr_grid_accumulate (bottom plane only) + pcr_grid_unpack + pcr_ground_filter + copies to
 *   the host, through the same scratch memory. host_lowest / host_ground int32[height * width], host_class uint8; any may be
 *   NULL. Range semantics and grid / clip checks are pcr_read_grid's.
 *
 * pcr_select_height: of the records pcr_decode_points would write for the range, a record is selected iff it lies inside *clip
 *   (NULL: all), in a cell of *grid (pcr_grid's cell rule exactly), g = dev_ground[cell] != PCR_GROUND_EMPTY and
 *   h_min <= h <= h_max with h = (int64)z - g compared in 64 bits, so a selected h fits int32. The records go to dev_points
 *   (16-byte aligned), byte for byte, with PCR_HEIGHT_REPLACE_Z in flags the z field holding h; h goes to dev_heights (int32,
 *   4-byte aligned); both in increasing row order, packed; either may be NULL, both NULL only counts. capacity counts records
 *   of each; a capacity below the result: PCR_E_ARG, *out_count = the count needed, nothing written. h_min > h_max, an empty
 *   clip or a range of 0 batches: 0 records, PCR_OK. BC1 and BC7, either layout, before and after the first frame.
 *   A batch whose exact box (pcr_batch_point_bounds' cache) misses grid and clip intersected is outside and not decoded; every
 *   other one is counted (k_height_count, colourless) and then written (k_height_write, with colours only when dev_points is
 *   given). There is no "inside" class: the height test needs every record's cell. Synchronises. stats may be NULL.
 *   PCR_E_ARG: pcr_select_box's refusals about range and destination, pcr_grid_accumulate's about the grid, a NULL dev_ground
 *   or a misaligned one, unknown flag bits.
 * pcr_read_height: the same into host memory (either pointer may be NULL); dev_ground is still a device plane. */
int pcr_ground_filter(pcr_ctx *ctx, const pcr_grid *grid, const pcr_ground_params *gp, const void *dev_lowest, void *dev_ground,
                      void *dev_class, pcr_ground_stats *stats);
int pcr_read_ground(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip,
                    const pcr_ground_params *gp, int32_t *host_lowest, int32_t *host_ground, uint8_t *host_class,
                    pcr_ground_stats *stats);
int pcr_select_height(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_grid *grid, const void *dev_ground,
                      const pcr_box *clip, int32_t h_min, int32_t h_max, uint32_t flags, void *dev_points, void *dev_heights,
                      size_t capacity, int64_t *out_count, pcr_height_stats *stats);
int pcr_read_height(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_grid *grid, const void *dev_ground,
                    const pcr_box *clip, int32_t h_min, int32_t h_max, uint32_t flags, pcr_point *host_points, int32_t *host_heights,
                    size_t capacity, int64_t *out_count, pcr_height_stats *stats);

/* ---- voxel-grid thinning: one record per voxel, straight from the compressed stream (no reference counterpart) ----------------
 * The *rows* of a range are the records pcr_decode_points writes for it: row r = (b - first_batch) * 65536 + chain * 64 + i,
 * padding duplicates and the tail artefact included. A row inside *clip (bounds inclusive; NULL: every row) is a *candidate*;
 * its voxel is v[k] = floor((p[k] - origin[k]) / cell) on every axis, in exact integer arithmetic (pcr_voxels in pcr_types.h).
 * CONTRACT: pcr_thin keeps exactly one candidate of every non-empty voxel -- PCR_THIN_FIRST the one with the lowest row,
 * PCR_THIN_CENTER the least by (d2, row) with d2 = sum over the axes of (2 * (p[k] - origin[k] - v[k] * cell) - (cell - 1))^2,
 * four times the squared distance to the voxel's centre as an integer. The kept records go to dev_points, byte for byte the
 * records pcr_decode_points writes (colour included), their rows to dev_rows (int64), both in increasing row order, packed
 * without gaps. The result is exact and the same from run to run; BC1 and BC7, either resident layout, before and after the
 * first frame. A voxel that spans two ranges is kept once per range: thin the whole range in one call.
 *
 * pcr_thin: either of dev_points (16-byte aligned) and dev_rows (8-byte aligned) may be NULL, with both NULL the call only
 *   counts; capacity_points counts records of each. A capacity below the result: PCR_E_ARG, *out_count = the count needed,
 *   nothing written. Range semantics, count < 0 and the restriction under pcr_set_async_upload are pcr_decode_points'. An empty
 *   clip, a range of 0 batches or a clip that misses every batch (by pcr_batch_point_bounds' cached exact boxes; no kernel runs):
 *   0 records, PCR_OK. Synchronises (the host sizes the voxel table and the output from counts). Touches no framebuffer, no
 *   prepass state, no render statistics. stats may be NULL.
 *   How: the batches the clip does not miss are decoded without colours twice -- k_thin_runs counts the runs of consecutive
 *   candidates of a chain in one voxel (the stream is Morton-sorted, so a chain mostly stays in a voxel for a while), the host
 *   sizes an open-addressing table of max(1024, the power of two >= 2 * runs) slots of 16 bytes, k_thin_mark inserts one
 *   (voxel, best row) per run with a 64-bit compare-and-swap on the key and an atomic minimum on the value -- then k_thin_flag
 *   turns the table into a bitmap of kept rows (a 64-bit word per chain) and k_thin_write decodes the batches that keep a
 *   record once more, with colours, and stores the flagged records. Minimum commutes: the table, hence the result, does not
 *   depend on the order of lanes or workgroups, and run compression is exact on an unsorted stream too. The table, the bitmap
 *   and the lists are scratch memory of the context, grown on demand and released with it.
 * pcr_read_thin: the same into host memory (alignof(pcr_point) / alignof(int64_t)), staged through the context's decode
 *   staging buffer and a second one for the rows, 64 batches at a time.
 * PCR_E_ARG with a message, nothing written: no stream loaded, a range outside the resident batches, a NULL vox, a NULL
 * out_count, a misaligned pointer, cell < 1 or > PCR_THIN_MAX_CELL, PCR_THIN_CENTER with cell > PCR_THIN_MAX_CENTER_CELL, an
 * unknown mode, a range of more than 2^40 rows, and a lattice too large for the 3 x 21-bit voxel key: with q = the union of
 * the exact boxes of the batches the clip does not miss, intersected with the clip, the call is refused if on any axis
 * q.max - q.min >= 2^31 or (q.max - q.min) / cell + 2 > 2^21 -- pass a clip or a larger cell (the tail artefact far outside
 * the cloud is the usual cause). PCR_E_NOMEM: no device memory for the table ("voxel table overflow" cannot happen: the table
 * has twice as many slots as insertions; the probe loop is bounded all the same). */
int pcr_thin(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int mode,
             void *dev_points, void *dev_rows, size_t capacity_points, int64_t *out_count, pcr_thin_stats *stats);
int pcr_read_thin(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int mode,
                  pcr_point *host_points, int64_t *host_rows, size_t capacity_points, int64_t *out_count, pcr_thin_stats *stats);

/* ---- voxel denoising: drop or extract isolated points by 3 x 3 x 3 voxel count (no reference counterpart) -------------------
 * Rows, candidates and voxels are pcr_thin's: the records pcr_decode_points writes for the range that lie inside *clip (NULL:
 * all of them), v[k] = floor((p[k] - origin[k]) / cell), exact. N27(p) is the number of candidates of the call in the 27 voxels
 * v(p) + {-1, 0, 1}^3; it counts p itself, exact duplicates and padding duplicates.
 * CONTRACT: a candidate is isolated iff N27(p) <= max_count. max_count == 0 isolates nothing, a huge one everything.
 * PCR_DENOISE_KEEP writes the candidates that are not isolated, PCR_DENOISE_ISOLATED the isolated ones: byte for byte the
 * records pcr_decode_points writes (colour included) to dev_points, their rows to dev_rows (int64), both in increasing row
 * order, packed without gaps. The result is exact and the same from run to run; BC1 and BC7, either resident layout, before
 * and after the first frame. Only candidates of this call's range and clip count: a neighbour in another range or outside the
 * clip does not exist for the call, so a point next to the cut may come out isolated -- denoise the whole range in one call,
 * with a clip a little larger than the region wanted. (lasnoise's -isolated k counts the OTHER points of the 27 cells, which
 * would make max_count = k + 1 its equivalent; that reading of its documentation has not been checked against the tool.)
 *
 * pcr_denoise: dev_points (16-byte aligned), dev_rows (8-byte aligned), capacity_points, *out_count, the count-only call, a
 *   capacity below the result (PCR_E_ARG, *out_count = the count needed, nothing written), range semantics, the empty clip /
 *   empty range / clip that misses every batch (0 records, PCR_OK, no kernel runs) and the synchronisation are pcr_thin's, word
 *   for word. Touches no framebuffer, no prepass state, no render statistics. stats may be NULL.
 *   How: pcr_thin's frame with a sum in the table. The lattice is shifted by whole cells so that every voxel index of a
 *   candidate lies in 1 .. 2^21 - 2 (a neighbour's key never leaves its 21-bit fields). k_thin_runs counts the runs, the host
 *   sizes the table as pcr_thin does, k_denoise_count inserts one (voxel, run length) per run -- compare-and-swap on the key,
 *   64-bit atomic add on the value -- k_denoise_verdict sums, per occupied slot, the 27 values around it (stopping once the sum
 *   exceeds max_count) and puts the verdict into bit 63 of the slot's value, k_denoise_flag decodes once more and builds the
 *   bitmap of rows to write from the verdict of each run's voxel, and k_thin_totals / k_thin_write size and write the output.
 *   Addition commutes: the table, hence the result, does not depend on the order of lanes or workgroups. The 27 lookups are
 *   paid per voxel, not per point. The scratch memory is pcr_thin's.
 * pcr_read_denoise: the same into host memory (alignof(pcr_point) / alignof(int64_t)), staged as pcr_read_thin stages.
 * PCR_E_ARG with a message, nothing written: pcr_thin's refusals (without the PCR_THIN_CENTER limit), max_count < 0, a mode
 * that is neither PCR_DENOISE_KEEP nor PCR_DENOISE_ISOLATED, and a lattice too large for the key: with q as for pcr_thin the
 * call is refused if on any axis q.max - q.min >= 2^31 or (q.max - q.min) / cell + 4 > 2^21 -- pass a clip or a larger cell. */
int pcr_denoise(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int64_t max_count,
                int mode, void *dev_points, void *dev_rows, size_t capacity_points, int64_t *out_count, pcr_denoise_stats *stats);
int pcr_read_denoise(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip,
                     int64_t max_count, int mode, pcr_point *host_points, int64_t *host_rows, size_t capacity_points,
                     int64_t *out_count, pcr_denoise_stats *stats);

/* ---- connected components of the occupied voxels: split the cloud, or drop every blob below a size (no reference counterpart) ---
 * Rows, candidates, voxels and the lattice are pcr_denoise's, word for word: the records pcr_decode_points writes for the range
 * that lie inside *clip (NULL: all of them), padding duplicates and tail garbage included; v[k] = floor((p[k] - origin[k]) /
 * cell), exact. Two occupied voxels are adjacent if they differ by at most 1 on every axis (connectivity == 26) or by exactly 1
 * on exactly one axis (connectivity == 6). A component is a class of the transitive closure of adjacency; its size is the number
 * of candidates in its voxels, duplicates counted. Only candidates of this call's range and clip exist for the call.
 * CONTRACT: the label of a component is the least row (pcr_decode_points order, counted from first_batch) of any candidate in it.
 * It is canonical: it does not depend on the hash function, the table size, the resident layout or the order of lanes,
 * workgroups or launches, and it is itself a row of the output when the component is written. A component is small iff its size
 * is < min_points: min_points <= 1 makes nothing small, a huge one everything. PCR_COMPONENTS_KEEP writes the candidates of the
 * components that are not small, PCR_COMPONENTS_SMALL those of the small ones: byte for byte the records pcr_decode_points
 * writes to dev_points, their rows to dev_rows (int64), the labels of their components to dev_labels (int64), all three in
 * increasing row order, packed without gaps. Exact and the same from run to run; BC1 and BC7, either resident layout, before and
 * after the first frame.
 *
 * pcr_components: dev_points (16-byte aligned), dev_rows and dev_labels (8-byte aligned); any of them may be NULL, all three NULL
 *   only counts. capacity_points, *out_count, a capacity below the result (PCR_E_ARG, *out_count = the count needed, nothing
 *   written), range semantics, the empty clip / empty range / clip that misses every batch (0 records, PCR_OK, no kernel runs) and
 *   the synchronisation are pcr_denoise's. Touches no framebuffer, no prepass state, no render statistics. stats may be NULL.
 *   How: pcr_denoise's frame. k_components_count is k_denoise_count that also keeps the least row of every voxel; k_components_link
 *   looks up, per occupied slot, the forward half of the neighbourhood (13 keys of 26, 3 of 6) and unites the slot with every
 *   neighbour found in a lock-free union-find over the slot indices (Rem's algorithm with splicing: every step a compare-and-swap
 *   that lowers a parent word, a parent always the lesser index); k_components_flatten points every slot at its root and takes
 *   the sum of the sizes and the minimum of the least rows there; k_components_verdict marks the slots of small components and
 *   hands every slot its label; k_denoise_flag, k_thin_totals and k_thin_write flag, size and write as for pcr_denoise, k_components_labels writes the
 *   labels in a colourless decode of its own. Every loop is bounded by the number of slots. The scratch memory is pcr_thin's
 *   plus 20 bytes per slot of the table.
 * pcr_read_components: the same into host memory (alignof(pcr_point) / alignof(int64_t)), staged as pcr_read_thin stages.
 * PCR_E_ARG with a message, nothing written: pcr_denoise's refusals (the lattice too large for the key included: pass a clip or a
 * larger cell), a connectivity that is neither 6 nor 26, min_points < 0, a mode that is neither PCR_COMPONENTS_KEEP nor
 * PCR_COMPONENTS_SMALL. PCR_E_NOMEM: a table of more than 2^32 slots (the forest's parent words are 32-bit). */
int pcr_components(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int connectivity,
                   int64_t min_points, int mode, void *dev_points, void *dev_rows, void *dev_labels, size_t capacity_points,
                   int64_t *out_count, pcr_components_stats *stats);
int pcr_read_components(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int connectivity,
                        int64_t min_points, int mode, pcr_point *host_points, int64_t *host_rows, int64_t *host_labels,
                        size_t capacity_points, int64_t *out_count, pcr_components_stats *stats);

/* ---- radius neighbourhoods: exact counts within a radius and nearest distances per point (no reference counterpart) -----------
 * Rows and candidates are pcr_thin's: the records pcr_decode_points writes for the range that lie inside *clip (bounds inclusive;
 * NULL: all of them), padding duplicates and the tail artefact included. For an integer radius r, 1 <= r <=
 * PCR_NEIGHBORS_MAX_RADIUS stream units, and d2(p, q) the squared Euclidean distance of the integer coordinates in exact 64-bit
 * arithmetic:
 *   N(p)   = the number of candidates q of the call with d2(p, q) <= r * r. It counts p itself (N >= 1), exact duplicates and a
 *            point at exactly distance r.
 *   nn2(p) = the least d2(p, q) over the candidates q of another row with d2 <= r * r: 0 if an exact duplicate exists,
 *            PCR_NN2_NONE (all ones) if there is no such q.
 * CONTRACT: a candidate is sparse iff N(p) < min_count. min_count <= 1 makes nothing sparse, a huge one everything.
 * PCR_NEIGHBORS_ALL writes every candidate, PCR_NEIGHBORS_KEEP those that are not sparse, PCR_NEIGHBORS_SPARSE the sparse ones:
 * byte for byte the records pcr_decode_points writes to dev_points (16-byte aligned), their rows to dev_rows (int64), N to
 * dev_counts (int64) and nn2 to dev_nn2 (uint64; each 8-byte aligned), all in increasing row order, packed without gaps. Any of
 * the four may be NULL; with all four NULL the call only counts. The result is exact and the same from run to run: it depends on
 * no lattice, hash, table size, bucket order or order of lanes, workgroups and launches. BC1 and BC7, either resident layout,
 * before and after the first frame. Only candidates of this call's range and clip exist for the call: as with pcr_denoise, filter
 * with a clip a little larger than the region wanted.
 * (PDAL's filters.outlier with method=radius counts the OTHER points within the radius and drops a point with fewer than min_k of
 * them, which would make min_count = min_k + 1 its equivalent; that reading of its documentation has not been checked against the
 * tool. CloudCompare's noise filter and a statistical outlier filter start from the same N and nn2.)
 *
 * pcr_neighbors: capacity_points, *out_count, the count-only call, a capacity below the result (PCR_E_ARG, *out_count = the count
 *   needed, nothing written), range semantics, the empty clip / empty range / clip that misses every batch (0 records, PCR_OK, no
 *   kernel runs) and the synchronisation are pcr_denoise's, word for word. Touches no framebuffer, no prepass state, no render
 *   statistics. stats may be NULL.
 *   How: pcr_denoise's frame on the lattice with origin (0, 0, 0) and cell = r, whose 27 voxels around a point's own cover its
 *   sphere, with the counts of the table turned into an index. k_thin_runs counts the runs, the host sizes the table,
 *   k_neighbors_count sums the candidates per voxel and notes where every chain's runs start, k_neighbors_alloc hands every
 *   occupied voxel a bucket and ceil(count / 64) work items, k_neighbors_fill copies the candidates into their buckets as {x, y,
 *   z, row} (one atomic per run), k_neighbors_pairs gives every work item a wave -- a lane per centre, the 27 neighbour buckets
 *   looked up once per chunk, laid end to end and broadcast through the wave in tiles of 64 -- and k_thin_totals / k_neighbors_write size and write
 *   the output. With PCR_NEIGHBORS_KEEP / _SPARSE and dev_counts == dev_nn2 == NULL a wave stops once all its centres have
 *   min_count neighbours; the outputs are the same either way.
 *   Scratch, grown on demand and released with the context: pcr_thin's, 8 bytes per slot, 8 per chain, 16 per candidate, the work
 *   list, and 8 bytes per row of the range for each of N and nn2 that is asked for.
 *   COST: a voxel of m candidates costs m * m tests, and a stream's padding duplicates are such a voxel (tens of thousands of
 *   copies of the last point: some 1e9 tests). stats.pairs_bound is the number of tests the call makes at most.
 * pcr_read_neighbors: the same into host memory (alignof(pcr_point) / alignof(int64_t)), staged as pcr_read_thin stages.
 * PCR_E_ARG with a message, nothing written: pcr_denoise's refusals, a radius outside 1 .. PCR_NEIGHBORS_MAX_RADIUS, min_count
 * < 0, an unknown mode, a range of more than 2^32 rows (the index stores a 32-bit row), and a lattice too large for the key: with
 * q as for pcr_thin the call is refused if on any axis q.max - q.min >= 2^31 or (q.max - q.min) / r + 4 > 2^21 -- pass a clip or
 * a larger radius. PCR_E_NOMEM: a table of more than 2^32 slots. */
int pcr_neighbors(pcr_ctx *ctx, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count, int mode,
                  void *dev_points, void *dev_rows, void *dev_counts, void *dev_nn2, size_t capacity_points, int64_t *out_count,
                  pcr_neighbors_stats *stats);
int pcr_read_neighbors(pcr_ctx *ctx, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count,
                       int mode, pcr_point *host_points, int64_t *host_rows, int64_t *host_counts, uint64_t *host_nn2,
                       size_t capacity_points, int64_t *out_count, pcr_neighbors_stats *stats);

/* ---- local moments: exact neighbourhood covariance and normals per point (no reference counterpart) -----------------------------
 * Candidates are pcr_neighbors' own. For a candidate p and an integer radius r, 1 <= r <= PCR_MOMENTS_MAX_RADIUS, B(p) is the set
 * of candidates q with d2(p, q) <= r * r in exact 64-bit integers: p itself, exact duplicates and points at exactly distance r
 * included. With d = q - p (offsets from the centre, not the origin: every term stays below r, and the later floating-point
 * covariance is free of cancellation against large coordinates) a pcr_moments record holds n = |B(p)| (pcr_neighbors' N), s[a] =
 * the sum of d_a over B(p) and q = the sums of d_a * d_b for xx, xy, xz, yy, yz, zz. EXACT: with r <= 32767 every |d_a| <= r and
 * every product is below 2^30; a call has at most 2^32 rows, so every sum stays below 2^62 -- the reason for the radius limit.
 * Sums commute: the result does not depend on the hash, the table size, the bucket order or the lane order and is the same from
 * run to run.
 * A candidate is written iff n >= min_count (min_count <= 1: all of them): its 16-byte record to dev_points (16-byte aligned),
 * its row to dev_rows (int64), its pcr_moments to dev_moments and its pcr_eigen to dev_eigen (each 8-byte aligned), all in
 * increasing row order, packed. Any pointer may be NULL; all four NULL only counts. A capacity below the result is PCR_E_ARG with
 * *out_count = the count needed and nothing written. stats are pcr_neighbors': points_sparse = the candidates with n < min_count,
 * pairs_bound as there. PCR_E_ARG with a message, nothing written: pcr_neighbors' refusals word for word (range, alignment,
 * min_count < 0, more than 2^32 rows, the lattice rule with cell = radius and its advice), and a radius outside 1 ..
 * PCR_MOMENTS_MAX_RADIUS. The call synchronises, touches no framebuffer, no prepass state, no render statistics; BC1 and BC7,
 * either resident layout, before and after the first frame.
 *   How: pcr_neighbors' plan up to the filled buckets; k_moments_pairs has k_neighbors_pairs' work distribution and accumulates the
 *   ten sums per lane (no early exit: every pair contributes), stores the 80-byte record by row and runs the eigen function
 *   in-lane; k_moments_write gathers the records of the kept rows. Scratch: pcr_neighbors' plus 80 and 48 bytes per row of the
 *   range for the moments and the eigen records, each only when asked for (PCR_E_NOMEM: pass a clip or a shorter range).
 * pcr_read_local_moments: the same into host memory (alignof(pcr_point) / alignof(int64_t) / alignof(double)), in pieces through
 * staging buffers as pcr_read_neighbors.
 * pcr_moments_eigen: the eigen record of each of n pcr_moments records at dev_moments (8-byte aligned) into dev_eigen, one
 * thread each; needs no stream loaded; synchronises; n == 0 does nothing; a NULL or misaligned pointer with n > 0 and n < 0 are
 * PCR_E_ARG. The eigen record is a function of the moments record alone, and pcr_local_moments calls the same function: for the
 * same moments the two are byte-identical. In f64, each operation rounded once:
 *     nf = (double)n,  m_a = (double)s[a] / nf,  C_ab = (double)q[ab] / nf - m_a * m_b
 * n <= 0: all six doubles are 0. Otherwise cyclic Jacobi on C: pivots (0,1), (0,2), (1,2); a zero off-diagonal is skipped; it
 * stops when all three are zero or after 12 sweeps; theta = (C_qq - C_pp) / (2 C_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 +
 * 1)) (an overflowing theta^2 ends in t = 0), c = 1 / sqrt(t^2 + 1), s = t c, tau = s / (1 + c); only + - * / and sqrt. The
 * eigenvalues are sorted ascending, ties keep the lower axis first; normal is the eigenvector of value[0] with the sign rule of
 * pcr_eigen. A decoupled axis a (C_ab == 0 for both b != a) keeps exactly (C_aa, e_a): a flat roof has value[0] == 0.0 and
 * normal == (0, 0, 1) to the bit, the zero matrix (n == 1) values 0 and normal (1, 0, 0). No output is NaN or Inf for any
 * finite input. */
int pcr_local_moments(pcr_ctx *ctx, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count,
                      void *dev_points, void *dev_rows, void *dev_moments, void *dev_eigen, size_t capacity_points, int64_t *out_count,
                      pcr_neighbors_stats *stats);
int pcr_read_local_moments(pcr_ctx *ctx, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count,
                           pcr_point *host_points, int64_t *host_rows, pcr_moments *host_moments, pcr_eigen *host_eigen,
                           size_t capacity_points, int64_t *out_count, pcr_neighbors_stats *stats);
int pcr_moments_eigen(pcr_ctx *ctx, const void *dev_moments, int64_t n, void *dev_eigen);

/* ---- k nearest neighbours: per point the k nearest other points within a radius, exact (no reference counterpart) ---------------
 * Candidates are pcr_neighbors' own, padding duplicates and the tail artefact included. d2(p, q) is the squared distance of the
 * integer coordinates in exact integer arithmetic. The neighbours of a candidate p are the candidates q of ANOTHER ROW with d2(p,
 * q) <= radius * radius: an exact duplicate is a neighbour at d2 == 0, a point at exactly the radius is one. They are ordered by
 * (d2, row) ascending, row being the row in pcr_decode_points order relative to first_batch; rows are distinct, so the order is
 * total. knn(p) is the first found(p) = min(k, N(p) - 1) of them, N as pcr_neighbors defines it. CANONICAL: the result depends on
 * no hash, table size, bucket order or order of lanes, workgroups and launches and is the same bytes from run to run.
 * Limits: 1 <= k <= PCR_KNN_MAX_K, 1 <= radius <= PCR_KNN_MAX_RADIUS. With these d2 < 2^30, and a call has at most 2^32 rows, so a
 * neighbour is one 64-bit word d2 << 32 | row whose unsigned order is the order above.
 * A candidate is written iff found(p) >= min_found, 0 <= min_found <= k (0: all of them): its 16-byte record to dev_points (16-byte
 * aligned), its row to dev_rows (int64) and its k words to dev_knn (uint64 [n * k], entry j of written record i at i * k + j,
 * entries found .. k - 1 are PCR_KNN_NONE; each 8-byte aligned), all in increasing row order, packed. Any pointer may be NULL; all
 * three NULL only counts. A capacity below the result is PCR_E_ARG with *out_count = the count needed and nothing written. stats
 * are pcr_neighbors': points_sparse = the candidates with found < min_found, pairs_bound as there. PCR_E_ARG with a message,
 * nothing written: pcr_neighbors' refusals word for word (range, alignment, more than 2^32 rows, the lattice rule with cell =
 * radius and its advice to pass a clip or a larger radius), and k, radius or min_found outside their ranges. The call
 * synchronises, touches no framebuffer, no prepass state, no render statistics; BC1 and BC7, either resident layout, before and
 * after the first frame.
 *   How: pcr_neighbors' plan up to the filled buckets; k_knn_pairs<K> (K = the least of 1, 2, 4, 8, 16 that holds k) has
 *   k_neighbors_pairs' work distribution and keeps per lane the K least words in registers, sorted, by an insertion pass that runs
 *   only where some lane of the wave has a word below its K-th; it stores the first k words by row; k_knn_write gathers the words
 *   of the kept rows. No early exit, no pruning of voxels: the cost is pcr_neighbors' ALL call (stats.pairs_bound tests) plus the
 *   insertions. With min_found == 0 and dev_knn == NULL the pair kernel decides nothing but runs all the same (pairs_bound comes
 *   from it). Scratch: pcr_neighbors' plus k * 8 bytes per row of the range when dev_knn is asked for (PCR_E_NOMEM: pass a clip or
 *   a shorter range).
 * pcr_read_knn: the same into host memory (alignof(pcr_point) / alignof(int64_t)), in pieces through staging buffers as
 * pcr_read_local_moments. */
int pcr_knn(pcr_ctx *ctx, int64_t first_batch, int64_t count, int k, int32_t radius, const pcr_box *clip, int64_t min_found,
            void *dev_points, void *dev_rows, void *dev_knn, size_t capacity_points, int64_t *out_count, pcr_neighbors_stats *stats);
int pcr_read_knn(pcr_ctx *ctx, int64_t first_batch, int64_t count, int k, int32_t radius, const pcr_box *clip, int64_t min_found,
                 pcr_point *host_points, int64_t *host_rows, uint64_t *host_knn, size_t capacity_points, int64_t *out_count,
                 pcr_neighbors_stats *stats);

/* ---- voxel means: centroid and mean colour per voxel, straight from the compressed stream (no reference counterpart) ------------
 * Candidates, voxels and the lattice are pcr_thin's, word for word: the records pcr_decode_points writes for the range that lie
 * inside *clip (bounds inclusive; NULL: all; padding duplicates and the tail artefact included), v = floor((p - origin) / cell) in
 * exact integers, cell in 1 .. PCR_THIN_MAX_CELL. For a non-empty voxel V: n(V) = the number of its candidates; r(p) = p - origin -
 * v * cell per axis, in [0, cell); S_a = the sum of r_a over the candidates; C_j = the sum of byte j (j = 0 .. 3) of the
 * candidates' colour words; row(V) = the least row among the candidates.
 * CONTRACT: one record per non-empty voxel, record i that of the voxel whose row(V) is the i-th smallest -- exactly the order and
 * the count of pcr_thin with PCR_THIN_FIRST and the same arguments. dev_points[i] is a pcr_point: its position on axis a is
 * origin_a + v_a * cell + (2 * S_a + n) / (2 * n), integer division of non-negative 64-bit values (the mean offset rounded half
 * up); byte j of its colour is (2 * C_j + n) / (2 * n), every byte averaged on its own (a byte that is zero in every candidate
 * stays zero). The mean offset lies in [min r_a, max r_a], inside [0, cell - 1]: the mean point lies in its own voxel and inside
 * the coordinate range of its candidates, hence in int32 (the kernels form it modulo 2^32 from the shifted lattice, as for the
 * key). dev_rows[i] = row(V) as int64, the rows pcr_thin FIRST returns; dev_counts[i] = n(V) as int64. A voxel whose candidates
 * are identical (cell == 1 positions, padding duplicates) yields that record. Sums of integers commute: the result is exact,
 * depends on no hash, table size or order of lanes, workgroups and launches and is the same bytes from run to run.
 *
 * pcr_voxel_mean: any of dev_points (16-byte aligned), dev_rows and dev_counts (8-byte aligned) may be NULL, with all three NULL
 *   the call only counts (pcr_thin's count-only call: no sum is formed); capacity_points counts records of each. A capacity below
 *   the result: PCR_E_ARG, *out_count = the count needed, nothing written. Range semantics, count < 0, the restriction under
 *   pcr_set_async_upload, the empty clip / empty range / clip that misses every batch (0 records, PCR_OK, no kernel runs) and the
 *   synchronisation are pcr_thin's. Touches no framebuffer, no prepass state, no render statistics; BC1 and BC7, either resident
 *   layout, before and after the first frame. A voxel that spans two ranges is averaged once per range (the counts make a later
 *   merge possible). stats (may be NULL) holds what pcr_thin FIRST reports for these arguments, table_slots included; points_kept
 *   is the call's *out_count.
 *   How: pcr_thin's FIRST plan runs unchanged (table of (voxel, least row), keep bitmap, records per batch). k_voxel_prefix scans
 *   the popcounts of the keep words of every batch that keeps a row; k_voxel_index turns the least row in every occupied slot
 *   into its record index and notes (key, row) per record; k_voxel_sum decodes the listed batches with colours, sums every run
 *   of a chain in registers and adds it into the accumulator of the run's voxel -- eight 64-bit words indexed by record: S_x,
 *   S_y, S_z, n, C_0 .. C_3 -- with atomic adds whose results are not used; k_voxel_finish does the roundings and the stores, a
 *   thread per record. Scratch, grown on demand and released with the context: pcr_thin's (16 bytes per slot, 8 per chain), 8
 *   bytes per chain of the range, and 80 bytes per voxel (64 the accumulator, 16 key and row).
 *   With offsets below 2^30 and at most 2^32 rows a call (PCR_VOXEL_MEAN_MAX_ROWS) every S_a < 2^62, C_j < 2^40 and 2 * S_a + n <
 *   2^64: the unsigned 64-bit sums and the rounding are exact.
 * pcr_read_voxel_mean: the same into host memory (alignof(pcr_point) / alignof(int64_t)), in pieces of 64 * 65 536 records
 *   through staging buffers as pcr_read_knn.
 * PCR_E_ARG with a message, nothing written: pcr_thin's refusals without the PCR_THIN_CENTER limit (the lattice too large for
 * the key included: pass a clip or a larger cell), a misaligned destination, and a range of more than PCR_VOXEL_MEAN_MAX_ROWS
 * rows (65 536 batches): pass a shorter range. PCR_E_NOMEM: no device memory for the table or the sums -- pass a clip or a larger
 * cell. */
int pcr_voxel_mean(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, void *dev_points,
                   void *dev_rows, void *dev_counts, size_t capacity_points, int64_t *out_count, pcr_thin_stats *stats);
int pcr_read_voxel_mean(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip,
                        pcr_point *host_points, int64_t *host_rows, int64_t *host_counts, size_t capacity_points, int64_t *out_count,
                        pcr_thin_stats *stats);

/* ---- levels of detail: the stream ordered by nested voxel lattices, straight from the compressed stream (no reference counterpart)
 * Candidates and rows are pcr_thin's, word for word: the records pcr_decode_points writes for the range that lie inside *clip
 * (bounds inclusive; NULL: all; padding duplicates and the tail artefact included), rows counted from first_batch. Level l of
 * *lod (0 = coarsest, L - 1 = finest, L = lod->levels) is pcr_thin's lattice {origin, cell << (L - 1 - l)}.
 * CONTRACT: level(p) of a candidate is the least l such that p has the lowest row of all candidates in its level-l voxel, and L
 * ("the rest") if it has the lowest row at no level. The lattices are nested (floor(floor(d / c) / 2) == floor(d / 2c)), so the
 * lowest row of a coarse voxel is also the lowest row of the finer voxel it lies in: the candidates with level <= l are exactly
 * the rows pcr_thin(PCR_THIN_FIRST) keeps with {origin, cell << (L - 1 - l)} and the same clip, the levels are disjoint, and
 * levels == 1 is pcr_thin FIRST plus a rest. The records written are all candidates, with PCR_LOD_DROP_REST those with level <
 * L, each byte for byte pcr_decode_points' record. They come in increasing (level, row): records [0, level_count[0]) are level 0,
 * the next level_count[1] level 1, and so on -- every prefix that ends at a level boundary is a uniformly thinned cloud. With
 * PCR_LOD_ROW_ORDER they come in increasing row order instead (the level as a per-point attribute). dev_rows[i] is the row of
 * record i as int64, dev_levels[i] its level as uint8 (0 .. L). Minima commute: the result is exact, depends on no hash, table
 * size or order of lanes, workgroups and launches, and is the same bytes from run to run.
 *
 * pcr_lod_order: any of dev_points (16-byte aligned), dev_rows and dev_levels (8-byte aligned) may be NULL, with all three NULL
 *   the call only counts; capacity_points counts records of each. A capacity below the result: PCR_E_ARG, *out_count = the count
 *   needed, nothing written. Range semantics, count < 0, the restriction under pcr_set_async_upload, the empty clip / empty range /
 *   clip that misses every batch (0 records, PCR_OK, no kernel runs), the limit of 2^40 rows and the synchronisation are
 *   pcr_thin's. Touches no framebuffer, no prepass state, no render statistics and no pending pcr_frame_begin; BC1 and BC7,
 *   either resident layout, before and after the first frame. stats may be NULL.
 *   How: pcr_thin's FIRST plan fills the finest table with (voxel, lowest row) on the lattice of lod_lattice (pcr_lattice.h:
 *   shifted by whole coarsest cells, so that the shifted lattices stay nested). k_lod_coarsen, a thread per slot, inserts
 *   (parent voxel, row) of every occupied slot of level l + 1 into the table of level l -- compare-and-swap on the key, unsigned
 *   minimum on the row; the parent key is every 21-bit field shifted right by one. k_lod_mark, a thread per slot of the new
 *   table, stores l into the level byte of the slot's row and counts the occupied slots, from which the host sizes the next
 *   table; going from fine to coarse the last store of a row is its least level. k_lod_count, a workgroup per listed batch,
 *   makes the bytes final (a candidate without a level gets L), counts the batch's records per level and sets the keep words;
 *   it decodes only a batch that the clip cuts. k_lod_write decodes with colours and stores every written record at the
 *   running index of its level: a stable partition by level, the offsets per (batch, level) a prefix sum on the host. In row
 *   order the keep words go through pcr_thin's write. No workgroup waits for another one; every probe loop is bounded by the
 *   slot count. Scratch, grown on demand and released with the context: pcr_thin's, two tables for the coarser levels (each at
 *   most the slots of twice the occupied finest voxels), 1 byte per row of the range and 8 (L + 1) bytes per listed batch.
 * pcr_read_lod_order: the same into host memory (alignof(pcr_point) / alignof(int64_t) / 1), in pieces of 64 * 65 536 rows
 *   through staging buffers; a piece is written in (level, row) order and copied to the L + 1 regions of the result.
 * PCR_E_ARG with a message, nothing written: no stream loaded, a range outside the resident batches, a NULL lod or out_count, a
 * misaligned destination, cell < 1, levels outside 1 .. PCR_LOD_MAX_LEVELS, cell << (levels - 1) > PCR_THIN_MAX_CELL, reserved !=
 * 0, an unknown flag bit, and a lattice too large for the key: with q = the union of the exact boxes of the batches the clip
 * does not miss, intersected with the clip, the call is refused if on any axis q.max - q.min >= 2^31 or (q.max - q.min) / cell +
 * 2^(L - 1) + 1 > 2^21 -- pass a clip or a larger cell. PCR_E_NOMEM: no device memory for the tables or the level bytes. */
int pcr_lod_order(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_lod *lod, const pcr_box *clip, uint32_t flags,
                  void *dev_points, void *dev_rows, void *dev_levels, size_t capacity_points, int64_t *out_count, pcr_lod_stats *stats);
int pcr_read_lod_order(pcr_ctx *ctx, int64_t first_batch, int64_t count, const pcr_lod *lod, const pcr_box *clip, uint32_t flags,
                       pcr_point *host_points, int64_t *host_rows, uint8_t *host_levels, size_t capacity_points, int64_t *out_count,
                       pcr_lod_stats *stats);

/* What a collective library needs to merge partial frames in place (include/pcr_dist.h does it with RCCL): the HIP stream
 * the context enqueues on, its device ordinal and the length of each framebuffer in 64-bit words. */
void *pcr_get_stream(pcr_ctx *ctx);
int pcr_get_device(const pcr_ctx *ctx);
size_t pcr_framebuffer_elems(const pcr_ctx *ctx);
/* Words each of the three buffers can hold: pcr_framebuffer_elems + PCR_FRAME_PAD_ELEMS for the context's own buffers (the
 * pad holds the identity of min / sum: a collective over whole slices may include it), pcr_framebuffer_elems while
 * external buffers are in use. pcr_device_rgba: the RGBA8 image the resolves write (same capacity, in pixels). */
size_t pcr_framebuffer_capacity(const pcr_ctx *ctx);
void *pcr_device_rgba(pcr_ctx *ctx);
/* Raw device pointers to the context's framebuffers. CONTRACT: the library resolves and clears only the 64 x 16-pixel tiles its own
 * kernels wrote in (dirty tiles, pcr_frame_turn). Whoever holds one of these pointers may write anywhere behind the library's back
 * (a collective, a merge of their own), so from the first call of a getter on, EVERY frame turn and clear walks the whole frame --
 * correct whatever is written through the pointer, 10-20 us slower per 4096x4096 frame -- until pcr_framebuffer_private(ctx) says
 * the pointers are no longer written through. (pcr_merge_*, pcr_use_external_buffers, pcr_set_int64_mergeable and the 10-10-10
 * method drop the tile tracking by themselves until the next full clear.) */
void *pcr_device_framebuffer(pcr_ctx *ctx);
void *pcr_device_rg(pcr_ctx *ctx);
void *pcr_device_ba(pcr_ctx *ctx);
int   pcr_framebuffer_private(pcr_ctx *ctx);
int   pcr_use_external_buffers(pcr_ctx *ctx, void *dev_fb, void *dev_rg, void *dev_ba); /* NULLs: back to own */
/* fb[i] = min(fb[i], other[i]) over pcr_fb_elems elements; rg/ba[i] += other[i] (NULL: skip). */
int   pcr_merge_min(pcr_ctx *ctx, const void *dev_other_fb);
int   pcr_merge_sum(pcr_ctx *ctx, const void *dev_other_rg, const void *dev_other_ba);
/* x ^= 1<<63 on every framebuffer element: maps unsigned order to signed order so that a signed
 * int64 MIN all-reduce (the dtype torch.distributed exposes) computes the u64 min. */
int   pcr_flip_sign(pcr_ctx *ctx);

/* All-to-all form of the multi-GPU merge (pcrhpg24_amd/dist.py, merge="a2a"): the frame is cut into N contiguous slices
 * of slice_elems words; after an all-to-all a rank holds everyone's copy of the slice it owns, back to back.
 * pcr_merge_min_slices leaves their element-wise min in the first slice; pcr_resolve_basic_range resolves `count` pixels of
 * a framebuffer range as pcr_resolve_basic does (the basic resolve depends on the word only, resolve.cu:149-191) into
 * `rgba`, which an all-gather then assembles into the image. Both work on device pointers the caller owns and enqueue
 * on the context's stream. */
int pcr_merge_min_slices(pcr_ctx *ctx, void *slices, int nslices, size_t slice_elems);
int pcr_resolve_basic_range(pcr_ctx *ctx, const pcr_render_params *params, const void *fb, size_t count, void *rgba);
/* The same for the HQS resolve (huffman_hqs/resolve.cu:2-47 depends on the pixel's three words only): `count` pixels of
 * corresponding ranges of fb / RG / BA. */
int pcr_resolve_hqs_range(pcr_ctx *ctx, const pcr_render_params *params, const void *fb, const void *rg, const void *ba,
                          size_t count, void *rgba);

/* Ordering between two streams of the context's device without the system-scope release a default HIP event carries
 * (which writes the L2 back: the 16.6 MB framebuffer the next kernel is about to read). slot in [0, 8). A frame rendered
 * on one stream and merged on another uses two of these per frame. stream NULL = the context's stream. */
int pcr_fence_record(pcr_ctx *ctx, int slot, void *hip_stream);
int pcr_fence_wait(pcr_ctx *ctx, int slot, void *hip_stream);

/* HBM layout the context gives the next stream it loads (pcr_stream_begin fixes it). All hold the same bits and decode to
 * the same points; the Huffman decode runs every frame in all of them. Only what the layout's kernel reads is kept: the
 * raw cluster-interleaved words of the file, the int32/int8 decoder tables and the cluster prefix are released by the first
 * frame after the last batch was uploaded (pcr_upload_tail has to come before that frame).
 *   PCR_LAYOUT_WORDS          per chain the sequence of 32-bit words it consumes, kept compact: per 64 chains only the rows their
 *                             longest chain consumed (~2.9 B per point resident and read on the benchmark stream: the memory-lean
 *                             layout, 4.2 B per point with all side data against 3.7 in the file); the decode keeps a five-word queue
 *                             per lane. Loading it waits for the device once per 128 batches (the compact size is read back).
 *   PCR_LAYOUT_POINT_WINDOWS  (default) per point the 40 bits of its chain's stream that start at the point's first bit
 *                             (5 B per point, a u32 and a u8 plane): no queue in the decode, a point's first table read
 *                             off the dependent chain, fewer instructions per point for ~1.4x the bytes per frame, on a
 *                             kernel bound by issue and latency, not by HBM.
 *   PCR_LAYOUT_BOTH           both resident: either decode variant can draw a frame (pcr_set_render_variant).
 *   PCR_LAYOUT_AUTO           POINT_WINDOWS unless the stream's windows would exceed the budget of pcr_set_hbm_budget (bytes; 0 = no
 *                             budget, the default): then WORDS. pcr_stream_layout tells which one the loaded stream got. */
#define PCR_LAYOUT_WORDS 0
#define PCR_LAYOUT_POINT_WINDOWS 1
#define PCR_LAYOUT_BOTH 2
#define PCR_LAYOUT_AUTO 3
int pcr_set_stream_layout(pcr_ctx *ctx, int layout);
int pcr_set_hbm_budget(pcr_ctx *ctx, int64_t bytes);
int pcr_stream_layout(const pcr_ctx *ctx);
/* Which decode variant draws. AUTO (default): the one the stream's layout holds; with PCR_LAYOUT_BOTH the point-window
 * variant while the image has at most 4096 pixels (one LDS framebuffer window) per loaded batch, the packed-words variant
 * beyond that, where the frame is bound by global framebuffer traffic and the smaller stream wins. WORDS / POINT_WINDOWS
 * force one; a render call fails with PCR_E_ARG if the stream's layout does not hold it. Results are identical. */
#define PCR_VARIANT_AUTO 0
#define PCR_VARIANT_WORDS 1
#define PCR_VARIANT_POINT_WINDOWS 2
int pcr_set_render_variant(pcr_ctx *ctx, int variant);

/* Workgroups per batch of the render kernels. The reference launches one 1024-thread block per batch
 * (modules/huffman_mem_iter_cuda/render.cu:328, huffman_mem_iter_cuda.h: cuLaunchKernel grid = numBatches); this build can also
 * draw a batch with two workgroups of 512 threads (chains 0..511 and 512..1023, four workgroups per CU) -- same frames, finer
 * turnover of LDS and wave slots. parts: 0 = chosen by the library (default), 1 = whole batches, 2 = half-batches. Takes effect
 * with the next prepass (pcr_frame_begin / pcr_frame_turn / a render call). */
int pcr_set_workgroup_parts(pcr_ctx *ctx, int parts);
/* Device bytes the loaded stream occupies right now (every per-stream allocation of the context, pads and guards included;
 * framebuffers excluded). Drops when the first frame after the last upload releases what only the load-time transcode reads. */
int64_t pcr_stream_resident_bytes(const pcr_ctx *ctx);
/* Colour format of the loaded stream: PCR_COLOR_BC1, PCR_COLOR_BC7 (a file written by a reference built with
 * COLOR_COMPRESSION == 7, include/BatchDumpData.h:130-136: 16 colour bytes per 16 points; told by the size of the first
 * record uploaded), 0 before the first record. A BC7 stream is drawn by the HQS method only (pcr_render_hqs_color decodes
 * mode-6 blocks as huffman_hqs/render.cu:240-273 does); pcr_render_basic refuses it: the reference's basic method decodes
 * the array as BC1 whatever the setting (huffman_mem_iter_cuda/render.cu:299) and its resolve then indexes it with a colour
 * (resolve.cu:183), which is not a result to be identical to. */
int pcr_stream_color_format(const pcr_ctx *ctx);
/* Version tag of the render/transcode kernels in this library ("rNN.vMM"): stored measurements name the tag they belong to. */
const char *pcr_kernel_version(void);

/* pcr_clear and the cull/LOD prepass of the frame's first render call in ONE launch: equivalent to pcr_clear followed by
 * what pcr_render_basic (method PCR_METHOD_BASIC) or pcr_render_hqs_depth (PCR_METHOD_HQS) would do first. The render call
 * that follows skips its prepass if it is given the same parameters and the loaded batches have not changed; otherwise it
 * runs its own, so calling this is never wrong, only sometimes useless. The frame loop of the adapters uses it where the
 * reference clears (huffman_hqs.h:266-270 / huffman_mem_iter_cuda.h:250-252). */
#define PCR_METHOD_BASIC 0
#define PCR_METHOD_HQS 1
int pcr_frame_begin(pcr_ctx *ctx, const pcr_render_params *params, int method);
/* The reference's RESOLVE + CLEAR at the end of a frame (huffman_hqs.h:240-270) and pcr_frame_begin's prepass for the next
 * frame, in ONE launch and one pass over the framebuffer: pcr_resolve_basic / pcr_resolve_hqs with the flags of `done`, then
 * pcr_frame_begin(next, method). The image is where pcr_resolve_* leaves it (pcr_read_rgba); the u64 framebuffer is empty
 * afterwards, so read it first if it is wanted. A steady frame loop is then two launches: pcr_render_*, pcr_frame_turn. */
int pcr_frame_turn(pcr_ctx *ctx, const pcr_render_params *done, const pcr_render_params *next, int method);

/* Multi-GPU merges through a library that only has a SIGNED 64-bit MIN (RCCL as torch.distributed exposes it): with
 * on = 1, pcr_clear writes INT64_MAX (0x7FFF...F) into empty pixels instead of the reference's all-ones word. Every key a
 * point can produce has a clear top bit (the depth half is the bit pattern of a positive float), so the kernels' unsigned
 * atomicMin, the resolves (they test the low half against 0xFFFFFFFF) and the HQS depth test (both words read as NaN)
 * behave exactly as before, signed and unsigned order agree on the whole framebuffer, and no sign-flip passes are
 * needed around the collective. pcr_read_framebuffer reports empty pixels as all-ones in either mode. Takes effect with
 * the next pcr_clear. */
int pcr_set_int64_mergeable(pcr_ctx *ctx, int on);

/* Asynchronous loader. Off (default): pcr_upload_batches enqueues its copies and the transcode on the
 * context's stream, in order with the frames, and a frame draws every batch handed over so far, as the reference's
 * process() does (HuffmanLasLoader.cpp:301-313). On: they run on a loader stream of the context's own, the call
 * returns once the records are packed into a pinned arena, and a frame draws the batches whose loader task is known to
 * have completed (never the last arrived batch of an incomplete stream: its chains' tail over-reads reach into the
 * next batch's words), so frames do not wait for PCIe. pcr_batches_resident: how many batches the next frame draws at
 * least (= pcr_batches_loaded when the mode is off). Switching synchronises. */
int pcr_set_async_upload(pcr_ctx *ctx, int on);
int64_t pcr_batches_resident(pcr_ctx *ctx);
int64_t pcr_last_frame_batches(const pcr_ctx *ctx);   /* batches drawn by the last pcr_render_* call */

/* ---- measurement ---------------------------------------------------------------------------------
 * HIP events on the context's stream: begin/end bracket any sequence of enqueued calls;
 * pcr_timing_end synchronises and returns the elapsed milliseconds between the two events. */
int pcr_timing_begin(pcr_ctx *ctx);
int pcr_timing_end(pcr_ctx *ctx, float *elapsed_ms);
/* Practical HBM ceiling of this device, set beside the 8 TB/s spec peak in the roofline: best of `reps`
 * passes of a streaming read and of a streaming copy (read + write bytes counted) over temporary buffers of `bytes`
 * each (use >= 1 GiB: the Infinity Cache holds 256 MiB). GB/s = 1e9 bytes per second. */
int pcr_measure_hbm(pcr_ctx *ctx, size_t bytes, int reps, float *read_gbps, float *copy_gbps);

/* Per-launch duration of the dominant kernel: with every = n > 0, every n-th pcr_render_* call brackets its
 * decode+rasterize kernel (not the prepass) with a HIP event pair (device-scope release) on the stream it is launched on
 * (an event pair still costs stream time, hence the stride); every = 0 switches it off. pcr_kernel_timing_read synchronises and returns
 * the average over the most recent bracketed launches (at most 64) since enabling, and how many those were. */
int pcr_kernel_timing_enable(pcr_ctx *ctx, int every);
int pcr_kernel_timing_read(pcr_ctx *ctx, float *avg_ms, int *launches);

/* Algorithmic HBM bytes of one render launch over the loaded stream, SURVEY 8d's B_dec x points: every byte of the
 * compressed representation once (encoded + separate + cluster prefix + per batch 160 + 12 288 + 4 096 + 32 768). */
int64_t pcr_stream_algorithmic_bytes(const pcr_ctx *ctx);
/* The same for the frame the last render call drew (synchronises): the batches the cull kept, and of each batch's encoded +
 * escape words the share npr / 64 of the points per chain its level of detail decodes (a chain's prefix; proportional, the
 * exact prefix lengths are not recorded) + its side data whole. Equals pcr_stream_algorithmic_bytes for LOD 100 %, no culling. */
int64_t pcr_last_frame_algorithmic_bytes(pcr_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* PCR_HIP_H */
