// pcr_api.hip — implementation of the C ABI in include/pcr_hip.h (libpcr_hip.so, gfx950 only).
//
// Host-side structure follows the reference's split into a Resource (HuffmanLasData: stream buffers,
// modules/compute/HuffmanLasLoader.cpp) and Methods (HuffmanMemIter / HuffmanHQS: framebuffers + launches,
// modules/huffman_mem_iter_cuda/huffman_mem_iter_cuda.h, modules/huffman_hqs/huffman_hqs.h), but one context
// owns both so a foreign-language caller needs a single handle. There is no CPU fallback: every entry point
// that needs the device fails with PCR_E_HIP / PCR_E_NODEVICE when HIP does.
#include "pcr_hip.h"
#include "pcr_kernels.hip.h"

#include <algorithm>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <type_traits>
#include <vector>

using namespace pcr;

constexpr int PCR_STATS_PARTIALS = PCR_MAX_PREPASS_WORKGROUPS;   // one partial record per prepass workgroup
#ifndef PCR_DEFAULT_PARTS
#define PCR_DEFAULT_PARTS 2                     /* workgroups per batch of k_render unless pcr_set_workgroup_parts says otherwise */
#endif
constexpr int64_t DECODE_STAGE_BATCHES = 64;     // batches per piece of pcr_read_points and of the shared read loop of the kept-rows calls
                                                 // (kept_write): 64 MiB of records on the device
constexpr int64_t TRANSCODE_CHUNK = 128;        // batches per k_transcode launch when the lane-major words are scratch (40 MB)

// Scratch of the batches a selection decodes twice (counted, then written), grown on demand (scratch_reserve)
template <class Entry> struct BatchScratch {
    int64_t capacity = 0;                       // batches the four arrays below hold
    Entry *list = nullptr;                      // [capacity] the batches, ascending
    uint32_t *counts = nullptr;                 // [capacity * 1024] selected points per chain (the count kernel)
    uint32_t *totals = nullptr;                 // [capacity] ... and per batch
    int64_t *offsets = nullptr;                 // [capacity] first output record of each (the write kernel)
};

struct pcr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;

    // resource (HuffmanLasData)
    bool stream_open = false;
    pcr_file_header hdr{};
    int64_t batch_index_base = 0;
    int64_t batches_loaded = 0, points_loaded = 0;
    int64_t enc_ptr = 0, sep_ptr = 0;           // running word offsets (HuffmanLasLoader.h:50-53)
    int64_t enc_words = 0, sep_words = 0;       // allocation sizes in words incl. pads
    std::vector<int32_t> h_stream_words;        // per uploaded batch: encoded + escape words (pcr_last_frame_algorithmic_bytes)
    pcr_gpu_batch *d_batches = nullptr;
    int32_t *d_start = nullptr;
    uint32_t *d_encoded = nullptr;
    int32_t *d_separate = nullptr;
    int32_t *d_sep_sizes = nullptr;
    int32_t *d_table_values = nullptr;
    int8_t *d_table_lens = nullptr;
    int32_t *d_cluster_sizes = nullptr;
    uint8_t *d_colors = nullptr;                // as uploaded (k_transcode's input; released with the other raw arrays)
    uint8_t *d_colors_t = nullptr;              // segment-major copy k_render reads (StreamView::colors_t)
    size_t color_bytes = 0;                     // per batch: PCR_COLOR_BYTES_PER_BATCH (BC1) or ..._BC7, told by the first record; 0 = not known yet
    uint32_t *d_lod = nullptr;
    WinPlan *d_win = nullptr;                   // LDS framebuffer windows of the frame's batches (prepass): two plans of hdr.num_batches
                                                // entries, slot 0 for 8-byte pixels (basic / HQS depth), slot 1 for the colour pass's 20-byte pixels
    uint32_t *d_batch_runs = nullptr;           // runs of chains and their bounding boxes, RUN_WORDS per batch (k_bounds)
    uint32_t *d_batch_flags = nullptr;          // BF_* per batch (k_transcode)
    // dense lists of the batches a frame draws, compacted by k_lod_prepass per workgroup (see RenderArgs): d_order[2][order_stride],
    // d_chunk_count[WORK_CLASSES + 1][PCR_MAX_PREPASS_WORKGROUPS]
    DrawRec *d_order = nullptr;
    uint32_t *d_chunk_count = nullptr;
    uint32_t order_stride = 0;
    // "some batch of this stream was ever flagged BF_GENERIC_SLOW_PATH": set on the device by k_transcode, copied to a
    // pinned word behind every transcode; while the copy is in flight the answer is "maybe" and the checked kernel is launched
    uint32_t *d_any_generic = nullptr;
    uint32_t *h_any_generic = nullptr;
    hipEvent_t any_generic_ev = nullptr;
    bool any_generic_pending = false;
    uint32_t *d_packed_table = nullptr;         // k_render's table entries, 4096 per batch (k_transcode)
    uint32_t *d_lane_words = nullptr;           // k_transcode's scratch: lane-major copy of the word stream, LW_ROWS x 1024 per batch of a chunk
    // PCR_LAYOUT_WORDS / _BOTH: the compact copy k_render's packed-words variant reads (k_pack_words). One device allocation per
    // transcode chunk, sized from the rows the chunk's waves consumed (read back: loading such a stream synchronises per chunk)
    bool keep_words = false;
    std::vector<uint32_t *> lw_segments;
    const uint32_t **d_lw_block = nullptr;      // [nB] the batch's block inside its chunk's segment
    uint32_t *d_lw_wave_row = nullptr;          // [nB * (LWC_WAVES + 1)] first row of every wave inside the block, and the end
    uint32_t *d_lw_prov = nullptr;              // [LWC_WAVES * LW_ROWS * 64] uncompacted rows of the provisional last batch of a stream that is still loading
    uint32_t *d_wave_rows = nullptr;            // [TRANSCODE_CHUNK * LWC_WAVES] rows per wave of the chunk being transcoded (k_transcode)
    uint32_t *h_wave_rows = nullptr;            // pinned: the same on the host, then the staging of the two arrays above
    int64_t provisional_for = -1;               // batches_loaded when the provisional walk of an incomplete stream's last batch was last done
    uint8_t *d_point_windows = nullptr;         // PCR_LAYOUT_POINT_WINDOWS: 40-bit view per point (k_transcode), PW_BATCH_BYTES per batch
    int layout = PCR_LAYOUT_POINT_WINDOWS;      // of the stream being loaded (pcr_set_stream_layout, fixed at pcr_stream_begin)
    int next_layout = PCR_LAYOUT_POINT_WINDOWS;
    int64_t hbm_budget = 0;                     // PCR_LAYOUT_AUTO: streams whose point windows would take more than this are loaded as packed words
    int variant = PCR_VARIANT_AUTO;             // which k_render variant draws a stream that has both layouts resident
    int64_t transcoded = 0;                     // batches [0, transcoded) of d_lane_words / d_point_windows are final
    // PCR_LAYOUT_POINT_WINDOWS keeps no lane-major words: d_lane_words is then k_transcode's scratch for TRANSCODE_CHUNK
    // batches at a time (launches of a stream run in order, so consecutive launches may reuse it)
    bool lane_words_scratch = false;
    // set by the first frame after the last batch: the buffers only k_transcode reads (raw word stream, int32/int8 tables,
    // cluster prefix, the scratch) have been released; pcr_upload_tail is refused from then on
    bool finalized = false;
    size_t stream_bytes = 0;                    // device bytes the loaded stream occupies right now (pcr_stream_resident_bytes)
    pcr_render_stats *d_stats = nullptr;        // PCR_STATS_PARTIALS partial records, one per prepass workgroup
    int stats_partials = 0;                     // how many the last render launch wrote
    // pinned staging arenas of the loader (double-buffered)
    uint8_t *arena[2] = {nullptr, nullptr};
    size_t arena_size[2] = {0, 0};
    hipEvent_t arena_done[2] = {nullptr, nullptr};
    bool arena_busy[2] = {false, false};
    int arena_next = 0;
    // asynchronous loader (pcr_set_async_upload): copies + transcode on a stream of their own; a render launch draws the
    // batches whose loader task is known to have completed, so frames never wait for the PCIe copy
    bool async_upload = false;
    hipStream_t copy_stream = nullptr;
    struct LoaderTask { hipEvent_t done; int64_t resident_after; };
    std::deque<LoaderTask> loader_tasks;
    std::vector<hipEvent_t> loader_events;      // recycled
    int64_t batches_resident = 0;
    int64_t last_frame_batches = 0;
    uint64_t empty_key = ~0ull;                 // what pcr_clear writes (pcr_set_int64_mergeable)
    // pcr_frame_begin ran the prepass of the next render call already, for exactly these inputs
    bool prepass_ready = false;
    pcr_render_params prepass_params{};
    int prepass_variant_hqs = 0;
    unsigned prepass_slots = 0;                 // which of the two window plans that prepass wrote (bit 0: 8-byte pixels, bit 1: 20-byte)
    uint32_t prepass_dyn_lds = 0;
    int prepass_parts = 0;
    int parts_mode = 0;                         // pcr_set_workgroup_parts: 0 = chosen per frame, 1 = whole batches, 2 = half-batches
    bool big_lds_ready = false;                 // hipFuncSetAttribute done for the 140 KiB launches
    bool decode_lds_ready = false;              // ... and for k_decode_points' 128 KiB of staging
    pcr_point *d_decode_stage = nullptr;        // pcr_read_points: device staging of at most DECODE_STAGE_BATCHES batches of points
    int64_t decode_stage_batches = 0;
    // box selection (pcr_batch_point_bounds / pcr_select_box): the exact integer box of every batch's decoded records, computed on
    // request by k_point_bounds and kept per batch until the stream goes (only for batches whose transcode is final: the last
    // batch of a stream that is still loading decodes differently once its follower's words arrive), and the scratch of a
    // selection's straddling batches
    std::vector<int32_t> h_point_bounds;        // [hdr.num_batches * 6]
    std::vector<uint8_t> h_point_bounds_ok;     // [hdr.num_batches]
    int32_t *d_point_bounds = nullptr;          // [hdr.num_batches * 6]
    BatchScratch<uint32_t> sel;                 // the straddling batches by their indices
    // polygon selection (pcr_select_polygon): the straddling batches of a call with their slices of the edge array, and the array
    // (the per-chain counts, totals and offsets are the box selection's four arrays above)
    int64_t poly_capacity = 0;                  // entries d_poly_batches holds
    PolyBatch *d_poly_batches = nullptr;        // [poly_capacity]
    int64_t poly_edge_capacity = 0;             // edges d_poly_edges holds
    PolyEdge *d_poly_edges = nullptr;           // [poly_edge_capacity] the batches' edge lists, back to back
    bool poly_lds_ready = false;                // hipFuncSetAttribute done for the k_polygon_* launches
    // slabs (pcr_select_slabs, pcr_plane_support): the listed batches of a call with their slices of the slab arrays, the arrays,
    // and pcr_plane_support's counters (pcr_select_slabs' per-chain counts, totals and offsets are the box selection's)
    int64_t slab_capacity = 0;                  // entries d_slab_batches holds
    SlabBatch *d_slab_batches = nullptr;        // [slab_capacity]
    int64_t slab_entry_capacity = 0;            // slabs d_slab_entries holds
    pcr_slab *d_slab_entries = nullptr;         // [slab_entry_capacity] the batches' slab lists, back to back
    int64_t plane_capacity = 0;                 // entries d_plane_batches holds
    PlaneBatch *d_plane_batches = nullptr;      // [plane_capacity]
    int64_t plane_cand_capacity = 0;            // entries d_plane_candidates holds
    uint32_t *d_plane_candidates = nullptr;     // [plane_cand_capacity] candidates per decoded batch
    int64_t plane_entry_capacity = 0;           // slabs d_plane_entries holds: the exclusion slices, then the hypothesis slices
    pcr_slab *d_plane_entries = nullptr;        // [plane_entry_capacity]
    unsigned long long *d_plane_counts = nullptr;   // [PCR_PLANE_MAX_HYPOTHESES]
    bool slab_lds_ready = false;                // hipFuncSetAttribute done for the k_slab_* and k_plane_support launches
    // screen selection and picking (pcr_select_screen / pcr_pick): the cull/LOD words of the call's camera in an array of their own
    // (k_screen_lod; the frame's d_lod, lists and plans are not touched), and the scratch of the kept batches
    uint32_t *d_screen_lod = nullptr;           // [hdr.num_batches]
    BatchScratch<ScreenEntry> scr;              // the kept batches: batch and LOD word
    unsigned long long *d_pick = nullptr;       // [PICK_WORDS] pcr_pick: key, index, record, hit
    // visible selection (pcr_select_visible): the per-pixel planes of the image and the per-batch totals; list, per-chain counts
    // and offsets are the screen selection's arrays above
    size_t vis_pixels = 0;                      // pixels the four planes below hold each
    unsigned long long *d_vis_key = nullptr;    // [vis_pixels + 1] min of depth << 32 | colour per pixel (k_visible_key); then the covered-pixel counter
    unsigned long long *d_vis_index = nullptr;  // [vis_pixels] FRONT: min record index among the hits that hold the key (k_visible_index)
    uint32_t *d_vis_row = nullptr;              // [vis_pixels] the row pass of k_visible_dilate
    uint32_t *d_vis_depth = nullptr;            // [vis_pixels] the dilated depth plane Dr
    int64_t vis_capacity = 0;                   // words d_vis_totals holds
    uint32_t *d_vis_totals = nullptr;           // [3 per kept batch] per batch: hits in the image, then (selected, candidates) pairs
    // top-down grid (pcr_grid_accumulate / pcr_read_grid): the list of a call's batches with their windows, and pcr_read_grid's planes
    int64_t grid_capacity = 0;                  // entries d_grid_list holds
    GridEntry *d_grid_list = nullptr;           // [grid_capacity] the windowed batches of a call, then the direct ones
    std::vector<GridEntry> h_grid_list;         // what it holds (a call with the same list uploads nothing)
    bool grid_lds_ready = false;                // hipFuncSetAttribute done for the windowed k_grid launches
    unsigned char *d_grid_scratch = nullptr;    // pcr_read_grid: top, bottom, count planes back to back
    size_t grid_scratch_bytes = 0;
    // height percentiles (pcr_grid_quantiles) share the list above; their own: the counters, per cell the segment, the work list and
    // (when the caller takes no counts) the count plane, and the candidates' values bucketed by cell
    unsigned char *d_quant_scratch = nullptr;
    size_t quant_scratch_bytes = 0;
    uint32_t *d_quant_values = nullptr;         // [quant_values_entries]
    size_t quant_values_entries = 0;
    // voxel thinning (pcr_thin / pcr_read_thin): the lists of a call's batches, the voxel table and the keep bitmap
    int64_t thin_capacity = 0;                  // batches the four arrays below hold
    uint32_t *d_thin_list = nullptr;            // [thin_capacity] the batches the clip does not miss
    uint32_t *d_thin_totals = nullptr;          // [thin_capacity * 2] runs and candidates (k_thin_runs), then kept records (k_thin_totals)
    uint32_t *d_thin_wlist = nullptr;           // [thin_capacity] of those the batches that keep a record
    int64_t *d_thin_offsets = nullptr;          // [thin_capacity] first output record of each (k_thin_write)
    ThinSlot *d_thin_table = nullptr;           // [thin_slots]
    int64_t thin_slots = 0;
    unsigned long long *d_thin_keep = nullptr;  // [thin_keep_words] a word per chain of the call's range
    int64_t thin_keep_words = 0;
    uint32_t *d_thin_error = nullptr;           // [1] k_thin_mark found no slot
    // the host forms of the kept-rows calls (pcr_read_thin .. pcr_read_voxel_mean): the stage of column i of a call's outputs (the
    // records go through d_decode_stage)
    void *d_col_stage[3] = {};                  // [col_stage_bytes[i]]
    int64_t col_stage_bytes[3] = {};
    // voxel denoising (pcr_denoise / pcr_read_denoise) shares all of the above; its own: the voxel counters of k_denoise_verdict
    unsigned long long *d_denoise_counters = nullptr;   // [2] occupied slots, isolated ones
    // connected components (pcr_components / pcr_read_components) share all of the above; their own: per slot of the table the
    // least row / label (8 bytes), the component's total (8) and the parent word of the union-find (4), in this order
    unsigned char *d_components_scratch = nullptr;      // [components_slots * 20]
    int64_t components_slots = 0;
    unsigned long long *d_components_counters = nullptr; // [5] occupied slots, components, small ones, their candidates, the largest
    // radius neighbourhoods (pcr_neighbors / pcr_read_neighbors) share pcr_thin's scratch; their own: the index and the dense results
    uint2 *d_neighbors_cursor = nullptr;                // [neighbors_slots] per slot of the table: bucket start, entries filled
    int64_t neighbors_slots = 0;
    unsigned long long *d_neighbors_starts = nullptr;   // [neighbors_chains] the run-start word of every chain
    int64_t neighbors_chains = 0;
    uint4 *d_neighbors_bucket = nullptr;                // [neighbors_candidates] x, y, z, row, bucketed by voxel
    int64_t neighbors_candidates = 0;
    unsigned long long *d_neighbors_work = nullptr;     // [neighbors_work] slot << 32 | chunk
    int64_t neighbors_work = 0;
    unsigned long long *d_neighbors_n = nullptr, *d_neighbors_nn2 = nullptr;    // [.._rows] N and nn2 by row, each only once asked for
    int64_t neighbors_n_rows = 0, neighbors_nn2_rows = 0;
    unsigned long long *d_neighbors_counters = nullptr; // [NEIGHBORS_COUNTERS]
    // local moments (pcr_local_moments / pcr_read_local_moments) share pcr_neighbors' index; their own: the dense records
    uint4 *d_moments_dense = nullptr, *d_moments_eigen = nullptr;   // [.._rows * 5] pcr_moments and [.._rows * 3] pcr_eigen by row, each only once asked for
    int64_t moments_dense_rows = 0, moments_eigen_rows = 0;
    // k nearest neighbours (pcr_knn / pcr_read_knn) share pcr_neighbors' index; their own: the dense words
    unsigned long long *d_knn_dense = nullptr;          // [knn_dense_words] k words by row, only once asked for
    int64_t knn_dense_words = 0;
    // voxel means (pcr_voxel_mean / pcr_read_voxel_mean) share pcr_thin's scratch; their own: the record index of every chain's
    // first kept row, the accumulator and (key, row) of every record
    unsigned long long *d_voxel_prefix = nullptr;       // [voxel_prefix_words] a word per chain of the call's range
    int64_t voxel_prefix_words = 0;
    unsigned long long *d_voxel_acc = nullptr;          // [voxel_acc_records * VOXEL_ACC_WORDS]
    int64_t voxel_acc_records = 0;
    VoxelRec *d_voxel_rec = nullptr;                    // [voxel_rec_records]
    int64_t voxel_rec_records = 0;
    // levels of detail (pcr_lod_order / pcr_read_lod_order) share pcr_thin's scratch; their own: the tables of the coarser levels
    // (two, used in turn), the level byte of every row, the batches with their "the clip cuts it" bit, the counts and then the
    // offsets per (batch, level), and the occupied slots of every level
    ThinSlot *d_lod_tables = nullptr;                   // [lod_slots]
    int64_t lod_slots = 0;
    uint8_t *d_lod_level = nullptr;                     // [lod_level_rows] a byte per row of the call's range
    int64_t lod_level_rows = 0;
    uint32_t *d_lod_list = nullptr;                     // [lod_list_batches]
    int64_t lod_list_batches = 0;
    int64_t *d_lod_batch = nullptr;                     // [lod_batch_words] (levels + 1) words per listed batch
    int64_t lod_batch_words = 0;
    unsigned long long *d_lod_occupied = nullptr;       // [PCR_LOD_MAX_LEVELS]
    int64_t prepass_batches = 0;
    static constexpr int FENCES = 8;
    hipEvent_t fence[FENCES] = {};              // pcr_fence_record / pcr_fence_wait: device-scope ordering between streams
    int64_t visible_batches() const { return async_upload ? batches_resident : batches_loaded; }

    // resource of the 10-10-10 path (ComputeLasData)
    bool las_open = false;
    int64_t las_capacity = 0, las_loaded = 0;   // batches
    pcr_xyz_batch *d_xyzb = nullptr;
    uint32_t *d_xyz12 = nullptr, *d_xyz8 = nullptr, *d_xyz4 = nullptr, *d_point_rgba = nullptr;
    int32_t *d_las_level = nullptr;
    uint2 *d_las_win = nullptr, *d_las_win_hqs = nullptr;      // LasArgs::win / win_hqs
    bool las_last_color = false;                // the last LAS render call was loop_las_hqs's colour pass (pcr_las_algorithmic_bytes)
    uint32_t *d_las_order = nullptr, *d_las_chunk_count = nullptr;      // LasArgs::order / chunk_count

    // method (framebuffers)
    int width = 0, height = 0;
    size_t fb_elems = 0;
    size_t fb_alloc = 0;                        // elements of each own buffer: fb_elems + PCR_FRAME_PAD_ELEMS (pad: fb all ones, RG/BA/rgba zero, written once)
    uint64_t *own_fb = nullptr, *own_rg = nullptr, *own_ba = nullptr;
    uint64_t *fb = nullptr, *rg = nullptr, *ba = nullptr;
    uint32_t *d_rgba = nullptr;
    bool accum_dirty = true;    // RG/BA hold something other than zeros (only the HQS colour pass writes them)
    // dirty tiles (FrameView::tiles): two arrays of one byte per 64 x 16 pixels; `tile_cur` is the one the frame being drawn marks,
    // the other says where the image may hold something. `tiles_tracked`: every framebuffer write since the last clear went
    // through a marking kernel (false after merges, external buffers, the 10-10-10 method: the next turn does the whole frame)
    uint8_t *d_tiles = nullptr;                 // three arrays of ntiles bytes, then three "everything" words
    uint32_t tiles_x = 0, ntiles = 0, tiles_stride = 0;
    int tile_cur = 0, tile_prev = 1, tile_spare = 2;    // roles of the three arrays: marked by the frame being drawn / image state / all zero
    uint32_t tile_e_cur = 1, tile_e_prev = 0, tile_epochs = 1;      // epoch that means "everything" in the cur / prev array's word
    bool tiles_tracked = false;
    // a raw pointer to one of the context's own buffers has been handed out (pcr_device_framebuffer / _rg / _ba): whoever holds it
    // may write anywhere at any time, so tiles are not used at all until pcr_framebuffer_private says the pointers are dead
    bool fb_exposed = false;
    bool tiles_usable() const { return d_tiles && !fb_exposed && fb == own_fb && rg == own_rg && ba == own_ba; }
    uint8_t *tiles_half(int which) const { return d_tiles + (size_t)which * tiles_stride; }
    uint32_t *tiles_all(int which) const { return reinterpret_cast<uint32_t *>(d_tiles + 3 * (size_t)tiles_stride) + which; }

    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    // per-launch timing of the dominant kernel (pcr_kernel_timing_*): event pairs around k_render / k_las_render only
    static constexpr int KT_PAIRS = 64;
    hipEvent_t kt_begin[KT_PAIRS] = {}, kt_end[KT_PAIRS] = {};
    int kt_every = 0;                           // 0 = off, n = bracket every n-th launch
    int64_t kt_launches = 0;                    // launches since enable
    int64_t kt_samples = 0;                     // bracketed launches since enable (only the last KT_PAIRS are kept)
    bool kt_sample_now() const { return kt_every > 0 && kt_launches % kt_every == 0; }
};

namespace {

thread_local std::string g_create_err;

int set_err(pcr_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

#define HIP_TRY(c, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return set_err((c), PCR_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

template <class T> void dfree(T *&p) { if (p) { (void)hipFree(p); p = nullptr; } }
template <class E> void dfree(BatchScratch<E> &b) { dfree(b.list); dfree(b.counts); dfree(b.totals); dfree(b.offsets); b.capacity = 0; }

// Async loader: retire the tasks whose event has fired (or, with wait, all of them).
void poll_loader(pcr_ctx *c, bool wait)
{
    while (!c->loader_tasks.empty()) {
        pcr_ctx::LoaderTask &t = c->loader_tasks.front();
        if (wait) (void)hipEventSynchronize(t.done);
        else if (hipEventQuery(t.done) != hipSuccess) break;
        c->batches_resident = t.resident_after;
        c->loader_events.push_back(t.done);
        c->loader_tasks.pop_front();
    }
}

void free_stream_buffers(pcr_ctx *c)
{
    poll_loader(c, true);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    c->batches_resident = 0;
    dfree(c->d_batches); dfree(c->d_start); dfree(c->d_encoded); dfree(c->d_separate); dfree(c->d_sep_sizes);
    dfree(c->d_table_values); dfree(c->d_table_lens); dfree(c->d_cluster_sizes); dfree(c->d_colors); dfree(c->d_colors_t); dfree(c->d_lod); dfree(c->d_win);
    for (uint32_t *seg : c->lw_segments) (void)hipFree(seg);
    c->lw_segments.clear(); dfree(c->d_lw_block); dfree(c->d_lw_wave_row); dfree(c->d_wave_rows); dfree(c->d_lw_prov); c->provisional_for = -1;
    dfree(c->d_lane_words); dfree(c->d_batch_flags); dfree(c->d_packed_table); dfree(c->d_point_windows); dfree(c->d_batch_runs); c->transcoded = 0;
    dfree(c->d_order); dfree(c->d_chunk_count); dfree(c->d_any_generic); c->order_stride = 0;
    dfree(c->d_point_bounds); c->h_point_bounds.clear(); c->h_point_bounds_ok.clear();
    dfree(c->sel);
    dfree(c->d_poly_batches); c->poly_capacity = 0; dfree(c->d_poly_edges); c->poly_edge_capacity = 0;
    dfree(c->d_slab_batches); c->slab_capacity = 0; dfree(c->d_slab_entries); c->slab_entry_capacity = 0;
    dfree(c->d_plane_batches); c->plane_capacity = 0; dfree(c->d_plane_candidates); c->plane_cand_capacity = 0; dfree(c->d_plane_entries); c->plane_entry_capacity = 0;
    dfree(c->d_plane_counts);
    dfree(c->d_screen_lod); dfree(c->scr);
    dfree(c->d_pick);
    dfree(c->d_vis_key); dfree(c->d_vis_index); dfree(c->d_vis_row); dfree(c->d_vis_depth); dfree(c->d_vis_totals); c->vis_pixels = 0; c->vis_capacity = 0;
    dfree(c->d_grid_list); c->grid_capacity = 0; c->h_grid_list.clear();
    dfree(c->d_thin_list); dfree(c->d_thin_totals); dfree(c->d_thin_wlist); dfree(c->d_thin_offsets); c->thin_capacity = 0;
    dfree(c->d_thin_table); c->thin_slots = 0; dfree(c->d_thin_keep); c->thin_keep_words = 0; dfree(c->d_thin_error);
    for (int i = 0; i < 3; ++i) { dfree(c->d_col_stage[i]); c->col_stage_bytes[i] = 0; }
    dfree(c->d_denoise_counters);
    dfree(c->d_components_scratch); c->components_slots = 0; dfree(c->d_components_counters);
    dfree(c->d_neighbors_cursor); c->neighbors_slots = 0; dfree(c->d_neighbors_starts); c->neighbors_chains = 0;
    dfree(c->d_neighbors_bucket); c->neighbors_candidates = 0; dfree(c->d_neighbors_work); c->neighbors_work = 0;
    dfree(c->d_neighbors_n); c->neighbors_n_rows = 0; dfree(c->d_neighbors_nn2); c->neighbors_nn2_rows = 0; dfree(c->d_neighbors_counters);
    dfree(c->d_moments_dense); c->moments_dense_rows = 0; dfree(c->d_moments_eigen); c->moments_eigen_rows = 0;
    dfree(c->d_knn_dense); c->knn_dense_words = 0;
    dfree(c->d_voxel_prefix); c->voxel_prefix_words = 0; dfree(c->d_voxel_acc); c->voxel_acc_records = 0;
    dfree(c->d_voxel_rec); c->voxel_rec_records = 0;
    dfree(c->d_lod_tables); c->lod_slots = 0; dfree(c->d_lod_level); c->lod_level_rows = 0; dfree(c->d_lod_list); c->lod_list_batches = 0;
    dfree(c->d_lod_batch); c->lod_batch_words = 0; dfree(c->d_lod_occupied);

    if (c->any_generic_pending && c->any_generic_ev) (void)hipEventSynchronize(c->any_generic_ev);
    c->any_generic_pending = false;
    if (c->h_any_generic) *c->h_any_generic = 0;
    c->stream_open = false; c->batches_loaded = c->points_loaded = 0; c->prepass_ready = false;
    c->finalized = false; c->lane_words_scratch = false; c->stream_bytes = 0; c->color_bytes = 0;
    c->enc_ptr = c->sep_ptr = 0; c->enc_words = c->sep_words = 0;
    c->h_stream_words.clear();
}

void free_las_buffers(pcr_ctx *c)
{
    dfree(c->d_xyzb); dfree(c->d_xyz12); dfree(c->d_xyz8); dfree(c->d_xyz4); dfree(c->d_point_rgba);
    dfree(c->d_las_level); dfree(c->d_las_win); dfree(c->d_las_win_hqs); dfree(c->d_las_order); dfree(c->d_las_chunk_count);
    c->las_open = false; c->las_capacity = c->las_loaded = 0;
}

void free_frame_buffers(pcr_ctx *c)
{
    dfree(c->own_fb); dfree(c->own_rg); dfree(c->own_ba); dfree(c->d_rgba); dfree(c->d_tiles);
    c->tiles_tracked = false; c->ntiles = c->tiles_x = 0;
    c->fb = c->rg = c->ba = nullptr; c->fb_elems = 0; c->fb_alloc = 0; c->width = c->height = 0;
}

template <class T> int dalloc_zero(pcr_ctx *c, T *&p, size_t count, size_t *account = nullptr)
{
    size_t bytes = (count ? count : 1) * sizeof(T);
    HIP_TRY(c, hipMalloc((void **)&p, bytes));
    HIP_TRY(c, hipMemsetAsync(p, 0, bytes, c->stream));
    if (account) *account += bytes;
    return PCR_OK;
}
template <class T> void dfree_counted(pcr_ctx *c, T *&p, size_t count)
{
    if (!p) return;
    c->stream_bytes -= (count ? count : 1) * sizeof(T);
    dfree(p);
}

int check_params(pcr_ctx *c, const pcr_render_params *p)
{
    if (!c) return PCR_E_ARG;
    if (!p) return set_err(c, PCR_E_ARG, "render params are NULL");
    if (!c->stream_open) return set_err(c, PCR_E_ARG, "no stream loaded (call pcr_stream_begin / pcr_upload_batch)");
    if (!c->fb) return set_err(c, PCR_E_ARG, "no framebuffer (call pcr_set_image_size)");
    if (p->width != c->width || p->height != c->height)
        return set_err(c, PCR_E_ARG, "params image size %dx%d != framebuffer %dx%d", p->width, p->height, c->width, c->height);
    if (p->points_per_thread != PCR_POINTS_PER_THREAD)
        return set_err(c, PCR_E_ARG, "points_per_thread must be %d", PCR_POINTS_PER_THREAD);
    if (p->lod_percent < 0) return set_err(c, PCR_E_ARG, "lod_percent must be >= 0");
    return PCR_OK;
}

// Workgroups per batch of a frame's k_render launches (RenderArgs::parts): half-batch workgroups unless told otherwise
// (pcr_set_workgroup_parts).
int frame_parts(const pcr_ctx *c)
{
    return c->parts_mode ? c->parts_mode : PCR_DEFAULT_PARTS;
}

StreamView make_stream_view(pcr_ctx *c)
{
    StreamView s;
    s.batches = c->d_batches; s.start_values = c->d_start; s.encoded = c->d_encoded;
    s.separate = c->d_separate; s.separate_sizes = c->d_sep_sizes; s.table_values = c->d_table_values;
    s.table_lens = c->d_table_lens; s.cluster_sizes = c->d_cluster_sizes; s.colors = c->d_colors; s.colors_t = c->d_colors_t; s.color_block_bytes = c->color_bytes == PCR_COLOR_BYTES_PER_BATCH_BC7 ? 16u : 8u;
    s.lane_words = c->d_lane_words; s.batch_flags = c->d_batch_flags; s.packed_table = c->d_packed_table;
    s.lw_block = c->d_lw_block; s.lw_wave_row = c->d_lw_wave_row;
    s.point_windows = c->d_point_windows; s.batch_runs = c->d_batch_runs;
    s.encoded_words = c->enc_words; s.separate_words = c->sep_words;
    s.num_batches = c->visible_batches(); s.batch_index_base = c->batch_index_base;
    return s;
}

RenderArgs make_args(pcr_ctx *c, const pcr_render_params *p, int variant_hqs)
{
    RenderArgs a;
    a.p = *p;
    a.s = make_stream_view(c);
    a.f.fb = c->fb; a.f.rg = c->rg; a.f.ba = c->ba; a.f.fb_elems = (uint32_t)c->fb_elems;
    a.f.tiles = c->tiles_usable() && c->tiles_tracked ? c->tiles_half(c->tile_cur) : nullptr;
    a.f.tiles_all = c->d_tiles ? c->tiles_all(c->tile_cur) : nullptr;
    a.f.tiles_x = c->tiles_x; a.f.tiles_epoch = c->tile_e_cur; a.f.tiles_total = c->ntiles;
    a.lod = c->d_lod; a.win = c->d_win; a.win_hqs = nullptr; a.stats = c->d_stats; a.variant_hqs = variant_hqs;
    a.parts = frame_parts(c);
    a.order = c->d_order;
    a.chunk_count = c->d_chunk_count;
    // chunks of the batches this frame draws (the prepass of the frame covered exactly these)
    a.order_stride = (uint32_t)((a.s.num_batches + PREPASS_BATCHES - 1) / PREPASS_BATCHES) * PREPASS_BATCHES;
    a.work_classes = a.s.num_batches > 8192 ? 1u : (uint32_t)WORK_CLASSES;
    return a;
}

// Does the stream hold a batch for the checked kernel (of workgroups of 1024 / parts threads)? false only when the device has said so.
bool maybe_generic_batches(pcr_ctx *c, int parts)
{
    if (c->any_generic_pending && hipEventQuery(c->any_generic_ev) == hipSuccess) c->any_generic_pending = false;
    return c->any_generic_pending || (*c->h_any_generic & bf_generic(parts)) != 0;
}

// Lane-major word sequences + packed tables (k_transcode) for every loaded batch that does not have them yet. A batch is
// final once the batch behind it is loaded (its chains' tail over-reads, SURVEY B.4, reach into those words) or the
// stream is complete; the last batch of an incomplete stream is walked provisionally (`include_provisional`, render
// time only) and walked again when more data arrives. Part of loading: pcr_upload_batches calls this for what it can.
int enqueue_transcode(pcr_ctx *c, bool include_provisional, hipStream_t st)
{
    const int64_t loaded = c->batches_loaded;
    const int64_t final_end = loaded == c->hdr.num_batches ? loaded : loaded - 1;
    const int64_t end = include_provisional ? loaded : final_end;
    // (the provisional walk of the last batch is the same until more data arrives: once per arrival, not once per frame)
    if (end > c->transcoded && c->transcoded == final_end && c->provisional_for == loaded) return PCR_OK;
    if (end > c->transcoded) {
        for (int64_t b0 = c->transcoded; b0 < end; ) {
            // (the provisional batch is a launch of its own: with the packed-words layout its rows go to a fixed scratch block)
            const int64_t n = b0 < final_end ? std::min(TRANSCODE_CHUNK, final_end - b0) : 1;
            const bool provisional = b0 >= final_end;
            hipLaunchKernelGGL(k_transcode, dim3((unsigned)n), dim3(PCR_WORKGROUP_SIZE), 0, st,
                               make_stream_view(c), c->d_lane_words, c->d_batch_flags, c->d_packed_table, c->d_point_windows, c->d_colors_t,
                               c->d_any_generic, (int)b0, (int)b0, c->keep_words ? c->d_wave_rows : nullptr);
            hipLaunchKernelGGL(k_bounds, dim3((unsigned)n), dim3(PCR_WORKGROUP_SIZE), 0, st,
                               make_stream_view(c), c->d_lane_words, c->d_batch_runs, (int)b0, (int)b0);
            if (c->keep_words && provisional) {
                // The last batch of a stream that is still loading, walked in front of a render call: no read-back, no allocation,
                // no host synchronisation (a segment per provisional walk leaked ~190 KB per upload until the stream
                // was unloaded, and the render call blocked). Its rows are copied uncompacted -- LW_ROWS per wave -- into one
                // scratch block that every provisional walk reuses; the batch is packed into its chunk's segment once it is final.
                hipLaunchKernelGGL(k_provisional_block, dim3(1), dim3(64), 0, st, (const uint32_t **)c->d_lw_block, c->d_lw_wave_row, c->d_lw_prov, (int)b0);
                hipLaunchKernelGGL(k_pack_words, dim3(1), dim3(PCR_WORKGROUP_SIZE), 0, st, c->d_lane_words, (uint32_t *const *)c->d_lw_block,
                                   c->d_lw_wave_row, (int)b0, (int)b0);
            } else if (c->keep_words) {
                // the compact copy: how many rows did every wave of the chunk consume? (the one place loading waits for the device)
                uint32_t *h = c->h_wave_rows;
                HIP_TRY(c, hipMemcpyAsync(h, c->d_wave_rows, (size_t)n * LWC_WAVES * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(c, hipStreamSynchronize(st));
                const uint32_t **h_block = reinterpret_cast<const uint32_t **>(h + TRANSCODE_CHUNK * LWC_WAVES);
                uint32_t *h_rows = h + TRANSCODE_CHUNK * LWC_WAVES + TRANSCODE_CHUNK * 2;
                std::vector<size_t> first_row((size_t)n);
                size_t total_rows = 0;
                for (int64_t i = 0; i < n; ++i) {
                    first_row[(size_t)i] = total_rows;
                    uint32_t r = 0;
                    for (int w = 0; w < LWC_WAVES; ++w) {
                        h_rows[i * (LWC_WAVES + 1) + w] = r;
                        r += std::min<uint32_t>(std::max<uint32_t>(h[i * LWC_WAVES + w], 2u), (uint32_t)LW_ROWS);
                    }
                    h_rows[i * (LWC_WAVES + 1) + LWC_WAVES] = r;
                    total_rows += r;
                }
                uint32_t *seg = nullptr;
                total_rows += LWC_PAD_ROWS;                 // (requests run up to four rows past a wave's last row: LWC_PAD_ROWS)
                if (hipMalloc((void **)&seg, total_rows * LWC_ROW_BYTES) != hipSuccess)
                    return set_err(c, PCR_E_NOMEM, "out of device memory for %zu bytes of packed words", total_rows * (size_t)LWC_ROW_BYTES);
                c->lw_segments.push_back(seg);
                c->stream_bytes += total_rows * LWC_ROW_BYTES;
                for (int64_t i = 0; i < n; ++i) h_block[i] = seg + first_row[(size_t)i] * 64;
                HIP_TRY(c, hipMemcpyAsync(c->d_lw_block + b0, h_block, (size_t)n * sizeof(uint32_t *), hipMemcpyHostToDevice, st));
                HIP_TRY(c, hipMemcpyAsync(c->d_lw_wave_row + b0 * (LWC_WAVES + 1), h_rows, (size_t)n * (LWC_WAVES + 1) * 4, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_pack_words, dim3((unsigned)n), dim3(PCR_WORKGROUP_SIZE), 0, st, c->d_lane_words, (uint32_t *const *)c->d_lw_block,
                                   c->d_lw_wave_row, (int)b0, (int)b0);
                HIP_TRY(c, hipStreamSynchronize(st));       // (the pinned staging is reused by the next chunk)
            }
            b0 += n;
        }
        c->transcoded = std::max(c->transcoded, final_end);
        c->provisional_for = end > final_end ? loaded : -1;
        // the sticky "some batch needs the checked kernel" word follows every transcode to the host
        (void)hipMemcpyAsync(c->h_any_generic, c->d_any_generic, 4, hipMemcpyDeviceToHost, st);
        (void)hipEventRecord(c->any_generic_ev, st);
        c->any_generic_pending = true;
    }
    return PCR_OK;
}

// Dynamic LDS of a frame's k_render launches: the small configuration (two workgroups per CU) unless the image has more
// pixels than the loaded batches' small windows hold together -- then most points would leave the windows and the frame is
// bound by global pre-reads and atomics; one workgroup per CU with windows of ~17 000 pixels keeps them in LDS.
uint32_t frame_dyn_lds(const pcr_ctx *c, int64_t nB)
{
    const bool halves = frame_parts(c) == 2;
    const uint32_t small = halves ? (uint32_t)DYN_LDS_BYTES_HALF : (uint32_t)DYN_LDS_BYTES, big = halves ? (uint32_t)DYN_LDS_BYTES_HALF_BIG : (uint32_t)DYN_LDS_BYTES_BIG;
    return (int64_t)c->width * c->height > nB * (int64_t)WIN_PIXELS ? big : small;
}

template <int MODE, int LAYOUT, bool GENERIC> hipError_t allow_big_lds()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_render<MODE, LAYOUT, GENERIC, 1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, DYN_LDS_BYTES_BIG);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_render<MODE, LAYOUT, GENERIC, 2>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, DYN_LDS_BYTES_HALF_BIG);
    return e;
}
int enable_big_lds(pcr_ctx *c)
{
    if (c->big_lds_ready) return PCR_OK;
    hipError_t e = hipSuccess;
#define PCR_ALLOW(M, L) if (e == hipSuccess) e = allow_big_lds<M, L, false>(); if (e == hipSuccess) e = allow_big_lds<M, L, true>()
    PCR_ALLOW(MODE_BASIC, LAYOUT_WORDS); PCR_ALLOW(MODE_BASIC, LAYOUT_POINT_WINDOWS);
    PCR_ALLOW(MODE_HQS_DEPTH, LAYOUT_WORDS); PCR_ALLOW(MODE_HQS_DEPTH, LAYOUT_POINT_WINDOWS);
    PCR_ALLOW(MODE_HQS_COLOR, LAYOUT_WORDS); PCR_ALLOW(MODE_HQS_COLOR, LAYOUT_POINT_WINDOWS);
    PCR_ALLOW(MODE_HQS_COLOR_BC7, LAYOUT_WORDS); PCR_ALLOW(MODE_HQS_COLOR_BC7, LAYOUT_POINT_WINDOWS);
#undef PCR_ALLOW
    if (e != hipSuccess) return set_err(c, PCR_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(e));
    c->big_lds_ready = true;
    return PCR_OK;
}

// Once the whole stream is loaded and every batch has its final transcode, what only k_transcode reads is dead weight:
// the raw cluster-interleaved words (the largest array of the file), the int32 / int8 decoder tables (k_render reads the
// packed entries; the int32 values stay if some batch has `wide` entries), the cluster prefix and the transcode scratch.
// Called from the first frame after completion; hipFree waits for the device, once.
void maybe_finalize(pcr_ctx *c)
{
    if (c->finalized || c->batches_loaded != c->hdr.num_batches || c->transcoded != c->batches_loaded) return;
    if (c->async_upload && (!c->loader_tasks.empty() || c->batches_resident != c->batches_loaded)) return;   // the loader stream is still at it
    if (c->any_generic_pending) { (void)hipEventSynchronize(c->any_generic_ev); c->any_generic_pending = false; }
    const size_t nB = (size_t)c->hdr.num_batches;
    dfree_counted(c, c->d_encoded, (size_t)c->enc_words + PCR_GUARD_WORDS);
    dfree_counted(c, c->d_table_lens, nB * 4096);
    dfree_counted(c, c->d_cluster_sizes, nB * 32);
    dfree_counted(c, c->d_colors, nB * (c->color_bytes ? c->color_bytes : (size_t)PCR_COLOR_BYTES_PER_BATCH));     // k_render reads colors_t
    if (*c->h_any_generic == 0) dfree_counted(c, c->d_table_values, nB * 4096);
    dfree_counted(c, c->d_lane_words, (size_t)std::min<int64_t>(TRANSCODE_CHUNK, (int64_t)nB) * LW_ROWS * PCR_WORKGROUP_SIZE);
    if (c->d_wave_rows) dfree_counted(c, c->d_wave_rows, (size_t)TRANSCODE_CHUNK * LWC_WAVES);
    if (c->d_lw_prov) dfree_counted(c, c->d_lw_prov, (size_t)(LWC_WAVES * LW_ROWS + LWC_PAD_ROWS) * 64);
    c->finalized = true;
}

template <int MODE> int launch_render(pcr_ctx *c, const pcr_render_params *p)
{
    int rc = check_params(c, p);
    if (rc) return rc;
    if (c->async_upload) poll_loader(c, false);
    const int64_t nB = c->visible_batches();         // "don't execute a workgroup until all points inside are loaded"
    c->last_frame_batches = nB;
    if (nB == 0) { c->stats_partials = 0; return PCR_OK; }   // huffman_hqs.h:137
    if (!c->async_upload && (rc = enqueue_transcode(c, true, c->stream))) return rc;   // normally only the provisional last batch of a stream that is still loading
    maybe_finalize(c);
    constexpr bool color_pass = MODE == MODE_HQS_COLOR || MODE == MODE_HQS_COLOR_BC7;
    const int win_pixel_bytes = color_pass ? WIN_PIXEL_BYTES_HQS : WIN_PIXEL_BYTES;
    const unsigned my_slot = color_pass ? 2u : 1u;
    const int variant_hqs = MODE != MODE_BASIC;
    const uint32_t dyn_lds = frame_dyn_lds(c, nB);
    const int parts = frame_parts(c);
    const bool have_prepass = c->prepass_ready && c->prepass_batches == nB && c->prepass_variant_hqs == variant_hqs &&
                              (c->prepass_slots & my_slot) && c->prepass_dyn_lds == dyn_lds && c->prepass_parts == parts &&
                              std::memcmp(&c->prepass_params, p, sizeof *p) == 0;
    c->prepass_ready = false;
    RenderArgs a = make_args(c, p, variant_hqs);
    WinPlan *const plan_slot[2] = { c->d_win, c->d_win + c->hdr.num_batches * MAX_PARTS };
    a.win = plan_slot[color_pass ? 1 : 0];
    a.win_pixel_bytes = win_pixel_bytes;
    a.dyn_lds_bytes = dyn_lds;
    if (dyn_lds > (uint32_t)(parts == 2 ? DYN_LDS_BYTES_HALF : DYN_LDS_BYTES) && (rc = enable_big_lds(c))) return rc;
    unsigned slots = c->prepass_slots;
    if (!have_prepass) {
        // the depth pass's prepass writes the colour pass's window plan as well: cull, LOD and the batch lists are the same
        // for both passes of a frame (huffman_hqs/depth.cu:197-227 == render.cu:362-392), only the LDS pixel size differs
        if (MODE == MODE_HQS_DEPTH) a.win_hqs = plan_slot[1];
        slots = MODE == MODE_HQS_DEPTH ? 3u : my_slot;
        c->stats_partials = (int)((nB + PREPASS_BATCHES - 1) / PREPASS_BATCHES);
        hipLaunchKernelGGL(k_lod_prepass, dim3((unsigned)c->stats_partials * PREPASS_WGS_PER_CHUNK), dim3(PREPASS_THREADS), 0, c->stream, a);
        a.win_hqs = nullptr;
    }
    if (MODE == MODE_HQS_DEPTH && (slots & 2u)) {
        // what the colour pass of this frame needs is in place: it runs no prepass of its own if it is given the same parameters
        c->prepass_ready = true; c->prepass_slots = 2u;
        c->prepass_params = *p; c->prepass_variant_hqs = variant_hqs; c->prepass_dyn_lds = dyn_lds; c->prepass_batches = nB;
        c->prepass_parts = parts;
    }
    const bool timed = c->kt_sample_now();
    const int slot = (int)(c->kt_samples % pcr_ctx::KT_PAIRS);
    if (timed) HIP_TRY(c, hipEventRecord(c->kt_begin[slot], c->stream));
    // A stream loaded with PCR_LAYOUT_BOTH can be drawn by either variant. The windows variant trades bytes for
    // instructions, which pays while the scatter runs in the LDS framebuffer windows; when the batches' rectangles outgrow
    // those (more pixels per batch than a window holds: 4096x4096 over 1526 batches), the frame is bound by global
    // framebuffer traffic and the 3 B per point of the packed words win.
    const bool have_windows = c->layout != PCR_LAYOUT_WORDS, have_words = c->layout != PCR_LAYOUT_POINT_WINDOWS;
    if ((c->variant == PCR_VARIANT_WORDS && !have_words) || (c->variant == PCR_VARIANT_POINT_WINDOWS && !have_windows))
        return set_err(c, PCR_E_ARG, "render variant %d needs a stream loaded with that layout (or PCR_LAYOUT_BOTH); this one has layout %d",
                       c->variant, c->layout);
    const bool windows = have_windows && (c->variant == PCR_VARIANT_POINT_WINDOWS || !have_words ||
                                          (c->variant == PCR_VARIANT_AUTO && (int64_t)c->width * c->height <= nB * (int64_t)WIN_PIXELS));
    // The grid is sized for "every batch visible"; workgroups beyond the prepass's dense list return at once. The checked
    // kernel (second list) is launched only if the stream may hold a flagged batch.
    const bool generic = maybe_generic_batches(c, parts);
    // (half-batches: workgroup x draws part (x >> 3) & 1 of list entry (x >> 4) * 8 + (x & 7) -- both halves on one XCD, see k_render)
    const dim3 grid(parts == 2 ? (unsigned)((nB + 7) / 8) * 16u : (unsigned)nB), block((unsigned)(PCR_WORKGROUP_SIZE / parts));
#define PCR_LAUNCH(L, G) do { if (parts == 2) hipLaunchKernelGGL((k_render<MODE, L, G, 2>), grid, block, dyn_lds, c->stream, a); \
                              else hipLaunchKernelGGL((k_render<MODE, L, G, 1>), grid, block, dyn_lds, c->stream, a); } while (0)
    if (windows) {
        PCR_LAUNCH(LAYOUT_POINT_WINDOWS, false);
        if (generic) PCR_LAUNCH(LAYOUT_POINT_WINDOWS, true);
    } else {
        PCR_LAUNCH(LAYOUT_WORDS, false);
        if (generic) PCR_LAUNCH(LAYOUT_WORDS, true);
    }
#undef PCR_LAUNCH
    if (timed) { HIP_TRY(c, hipEventRecord(c->kt_end[slot], c->stream)); ++c->kt_samples; }
    if (c->kt_every > 0) ++c->kt_launches;
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

} // namespace

extern "C" {

const char *pcr_last_error(const pcr_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// Bumped with every change to k_render / k_transcode that can move a measured number: what a stored profile (HBM traffic
// from PMC counters, profiles/pmc_traffic_latest.json) was measured on is compared with this before it is quoted.
const char *pcr_kernel_version(void) { return "r04.v111"; }

int pcr_create(int device, pcr_ctx **out)
{
    if (!out) return set_err(nullptr, PCR_E_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return set_err(nullptr, PCR_E_NODEVICE, "no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return set_err(nullptr, PCR_E_ARG, "device %d out of range [0,%d)", device, ndev);
    HIP_TRY(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(nullptr, PCR_E_NODEVICE, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
    pcr_ctx *c = new (std::nothrow) pcr_ctx();
    if (!c) return set_err(nullptr, PCR_E_NOMEM, "out of host memory");
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev_begin) != hipSuccess || hipEventCreate(&c->ev_end) != hipSuccess ||
        hipEventCreateWithFlags(&c->arena_done[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->arena_done[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->any_generic_ev, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc((void **)&c->h_any_generic, 64, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&c->d_stats, PCR_STATS_PARTIALS * sizeof(pcr_render_stats)) != hipSuccess) {
        pcr_destroy(c);
        return set_err(nullptr, PCR_E_HIP, "could not create stream/events");
    }
    *c->h_any_generic = 0;
    c->stream = c->own_stream;
    *out = c;
    return PCR_OK;
}

void pcr_destroy(pcr_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_stream_buffers(c);
    free_las_buffers(c);
    free_frame_buffers(c);
    dfree(c->d_stats);
    dfree(c->d_decode_stage);
    dfree(c->d_grid_scratch);
    dfree(c->d_quant_scratch);
    dfree(c->d_quant_values);
    for (int i = 0; i < 2; ++i) {
        if (c->arena[i]) (void)hipHostFree(c->arena[i]);
        if (c->arena_done[i]) (void)hipEventDestroy(c->arena_done[i]);
    }
    for (int i = 0; i < pcr_ctx::KT_PAIRS; ++i) {
        if (c->kt_begin[i]) (void)hipEventDestroy(c->kt_begin[i]);
        if (c->kt_end[i]) (void)hipEventDestroy(c->kt_end[i]);
    }
    if (c->any_generic_ev) (void)hipEventDestroy(c->any_generic_ev);
    if (c->h_any_generic) (void)hipHostFree(c->h_any_generic);
    if (c->h_wave_rows) (void)hipHostFree(c->h_wave_rows);
    if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
    if (c->ev_end) (void)hipEventDestroy(c->ev_end);
    for (hipEvent_t e : c->loader_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->fence) if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int pcr_set_stream(pcr_ctx *c, void *hip_stream)
{
    if (!c) return PCR_E_ARG;
    // No synchronisation here: work already enqueued stays on the stream it was enqueued on, and ordering between
    // the old and the new stream is the caller's (events), which is what lets a merge overlap the next render.
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return PCR_OK;
}

int pcr_synchronize(pcr_ctx *c)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

// ---- resource ----------------------------------------------------------------------------------
int pcr_stream_begin(pcr_ctx *c, const pcr_file_header *h, int64_t batch_index_base)
{
    if (!c) return PCR_E_ARG;
    if (!h) return set_err(c, PCR_E_ARG, "header is NULL");
    if (h->num_batches <= 0 || h->num_points != h->num_batches * PCR_POINTS_PER_BATCH)
        return set_err(c, PCR_E_FORMAT, "header: numPoints %lld != numBatches %lld * 65536", (long long)h->num_points, (long long)h->num_batches);
    if (h->encoded_bytes < 0 || h->separate_bytes < 0 || (h->encoded_bytes & 3) || (h->separate_bytes & 3))
        return set_err(c, PCR_E_FORMAT, "header: bad stream byte counts");
    if (h->num_batches > 0xFFFF)
        return set_err(c, PCR_E_FORMAT, "at most 65535 batches (4.29e9 points) per context; shard larger files");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_stream_buffers(c);
    c->hdr = *h; c->batch_index_base = batch_index_base;
    const size_t nB = (size_t)h->num_batches;
    c->enc_words = h->encoded_bytes / 4 + PCR_ENCODED_PAD_WORDS;      // HuffmanLasLoader.cpp:39-41
    c->sep_words = h->separate_bytes / 4 + PCR_SEPARATE_PAD_WORDS;
    int rc;
    size_t *acc = &c->stream_bytes;
    int layout = c->next_layout;
    if (layout == PCR_LAYOUT_AUTO) {
        // what the stream would take as point windows (5 B per point + side data), against the budget the caller set
        const int64_t as_windows = (int64_t)nB * (int64_t)(PW_BATCH_BYTES + 4 * 4096 + 12288 + 4096 + PCR_COLOR_BYTES_PER_BATCH) + h->separate_bytes;
        layout = c->hbm_budget > 0 && as_windows > c->hbm_budget ? PCR_LAYOUT_WORDS : PCR_LAYOUT_POINT_WINDOWS;
    }
    const bool windows = layout != PCR_LAYOUT_WORDS, words = layout != PCR_LAYOUT_POINT_WINDOWS;
    c->lane_words_scratch = true;
    c->keep_words = words;
    const size_t lw_batches = (size_t)std::min<int64_t>(TRANSCODE_CHUNK, (int64_t)nB);
    if (words && !c->h_wave_rows)       // rows per wave of a chunk, then the staging of its block pointers and row offsets
        HIP_TRY(c, hipHostMalloc((void **)&c->h_wave_rows, (size_t)TRANSCODE_CHUNK * (LWC_WAVES + 2 + LWC_WAVES + 1) * 4, hipHostMallocDefault));
    if ((rc = dalloc_zero(c, c->d_batches, nB, acc)) || (rc = dalloc_zero(c, c->d_start, nB * 3072, acc)) ||
        (rc = dalloc_zero(c, c->d_encoded, (size_t)c->enc_words + PCR_GUARD_WORDS, acc)) ||
        (rc = dalloc_zero(c, c->d_separate, (size_t)c->sep_words + PCR_GUARD_WORDS, acc)) ||
        (rc = dalloc_zero(c, c->d_sep_sizes, nB * 1024, acc)) || (rc = dalloc_zero(c, c->d_table_values, nB * 4096, acc)) ||
        (rc = dalloc_zero(c, c->d_table_lens, nB * 4096, acc)) || (rc = dalloc_zero(c, c->d_cluster_sizes, nB * 32, acc)) ||
        (rc = dalloc_zero(c, c->d_colors, nB * PCR_COLOR_BYTES_PER_BATCH, acc)) || (rc = dalloc_zero(c, c->d_colors_t, nB * PCR_COLOR_BYTES_PER_BATCH, acc)) ||
        (rc = dalloc_zero(c, c->d_lod, nB, acc)) ||
        (rc = dalloc_zero(c, c->d_win, 2 * MAX_PARTS * nB, acc)) ||
        (rc = dalloc_zero(c, c->d_lane_words, lw_batches * LW_ROWS * PCR_WORKGROUP_SIZE, acc)) || (rc = dalloc_zero(c, c->d_batch_flags, nB, acc)) ||
        (rc = dalloc_zero(c, c->d_packed_table, nB * PCR_HUFFMAN_TABLE_SIZE, acc)) ||
        (rc = dalloc_zero(c, c->d_batch_runs, nB * RUN_RECORDS * RUN_WORDS, acc)) ||
        (rc = dalloc_zero(c, c->d_order, 2 * ((nB + PREPASS_BATCHES - 1) / PREPASS_BATCHES) * PREPASS_BATCHES, acc)) ||
        (rc = dalloc_zero(c, c->d_chunk_count, (WORK_CLASSES + 1) * PCR_MAX_PREPASS_WORKGROUPS, acc)) || (rc = dalloc_zero(c, c->d_any_generic, 1, acc)) ||
        (windows && (rc = dalloc_zero(c, c->d_point_windows, nB * PW_BATCH_BYTES + PW_GUARD_BYTES, acc))) ||
        (words && ((rc = dalloc_zero(c, c->d_lw_block, nB, acc)) || (rc = dalloc_zero(c, c->d_lw_wave_row, nB * (LWC_WAVES + 1), acc)) ||
                   (rc = dalloc_zero(c, c->d_wave_rows, (size_t)TRANSCODE_CHUNK * LWC_WAVES, acc)) ||
                   (rc = dalloc_zero(c, c->d_lw_prov, (size_t)(LWC_WAVES * LW_ROWS + LWC_PAD_ROWS) * 64, acc))))) {
        free_stream_buffers(c);
        return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->layout = layout;
    c->stream_open = true;
    return PCR_OK;
}

int pcr_upload_batch(pcr_ctx *c, int64_t batch_index, const void *blob, size_t n)
{
    return pcr_upload_batches(c, batch_index, 1, &blob, &n);
}

// One loader task (the reference hands over <= 100 records at a time, HuffmanLasLoader.cpp:106): every record is
// validated, the nine per-batch arrays of the whole task are packed contiguously into one of two pinned staging
// arenas, and nine large asynchronous copies move them; the arenas alternate, so packing task k+1 on the host
// overlaps the copies of task k. The reference issues nine synchronous cuMemcpyHtoD per record instead
// (HuffmanLasLoader.cpp:229-289).
int pcr_upload_batches(pcr_ctx *c, int64_t first_index, int64_t count, const void *const *blobs, const size_t *sizes)
{
    if (!c) return PCR_E_ARG;
    if (!c->stream_open) return set_err(c, PCR_E_ARG, "pcr_stream_begin has not been called");
    if (count <= 0 || !blobs || !sizes) return set_err(c, PCR_E_ARG, "no batch records given");
    if (first_index != c->batches_loaded)
        return set_err(c, PCR_E_ARG, "batches must be uploaded in order: expected %lld, got %lld", (long long)c->batches_loaded, (long long)first_index);
    if (first_index + count > c->hdr.num_batches) return set_err(c, PCR_E_ARG, "batch index %lld beyond header", (long long)(first_index + count - 1));

    const size_t fixed = PCR_BATCH_FIXED_HEADER + 4u * (3072 + 1024 + 4096 + 4096 + 32);
    struct View { const uint8_t *start, *sepsz, *tv, *tl, *cl, *enc, *sep, *col; int32_t ne, ns; };
    std::vector<View> views((size_t)count);
    int64_t sum_ne = 0, sum_ns = 0;
    size_t color_bytes = c->color_bytes;
    // ---- pass 1: validate (nothing is modified if any record is bad) --------------------------------------------
    for (int64_t k = 0; k < count; ++k) {
        const int64_t bi = first_index + k;
        const uint8_t *r = (const uint8_t *)blobs[k];
        const size_t n = sizes[k];
        if (!r) return set_err(c, PCR_E_ARG, "blob is NULL");
        if (n < fixed) return set_err(c, PCR_E_FORMAT, "batch %lld: record of %zu bytes is too short", (long long)bi, n);
        int32_t hdr[5]; std::memcpy(hdr, r, 20);                      // include/BatchDumpData.h:60-107
        int32_t dt_size, num_clusters;
        std::memcpy(&dt_size, r + 116, 4); std::memcpy(&num_clusters, r + 120, 4);
        if (hdr[1] != PCR_POINTS_PER_BATCH || hdr[2] != PCR_WORKGROUP_SIZE || hdr[3] != PCR_POINTS_PER_THREAD ||
            hdr[4] != PCR_CLUSTERS_PER_THREAD || dt_size != PCR_HUFFMAN_TABLE_SIZE || num_clusters != PCR_CLUSTERS_PER_BATCH)
            return set_err(c, PCR_E_FORMAT, "batch %lld: unsupported geometry (points %d threads %d ppt %d cpt %d table %d clusters %d)",
                           (long long)bi, hdr[1], hdr[2], hdr[3], hdr[4], dt_size, num_clusters);
        View &v = views[(size_t)k];
        v.start = r + PCR_BATCH_FIXED_HEADER;
        v.sepsz = v.start + 3072 * 4;
        v.tv = v.sepsz + 1024 * 4;
        v.tl = v.tv + 4096 * 4;
        v.cl = v.tl + 4096 * 4;
        v.enc = v.cl + 32 * 4;
        std::memcpy(&v.ne, v.cl + 31 * 4, 4);
        std::memcpy(&v.ns, v.sepsz + 1023 * 4, 4);
        if (v.ne < 64 || v.ns < 0) return set_err(c, PCR_E_FORMAT, "batch %lld: stream lengths %d / %d", (long long)bi, v.ne, v.ns);
        // BatchDumpData.h:130-136: 8 (BC1) or 16 (BC7 mode 6) colour bytes per 16 points, fixed when the reference is built
        // (COLOR_COMPRESSION); here the first record of a stream tells which, and the others have to agree
        const size_t streams = fixed + 4u * ((size_t)v.ne + (size_t)v.ns);
        if (color_bytes == 0) {
            if (n == streams + PCR_COLOR_BYTES_PER_BATCH) color_bytes = PCR_COLOR_BYTES_PER_BATCH;
            else if (n == streams + PCR_COLOR_BYTES_PER_BATCH_BC7) color_bytes = PCR_COLOR_BYTES_PER_BATCH_BC7;
        }
        if (color_bytes == 0 || n != streams + color_bytes)                                                          // BatchDumpData.h:148
            return set_err(c, PCR_E_FORMAT, "batch %lld: record size %zu does not match its stream lengths", (long long)bi, n);
        v.sep = v.enc + (size_t)v.ne * 4;
        v.col = v.sep + (size_t)v.ns * 4;
        sum_ne += v.ne; sum_ns += v.ns;
        if (c->enc_ptr + sum_ne > c->enc_words - PCR_ENCODED_PAD_WORDS || c->sep_ptr + sum_ns > c->sep_words - PCR_SEPARATE_PAD_WORDS)
            return set_err(c, PCR_E_FORMAT, "batch %lld: streams exceed the header's byte counts", (long long)bi);
        for (int i = 0; i < 4096; ++i) {                              // code lengths (narrowed to int8 below)
            int32_t l; std::memcpy(&l, v.tl + 4 * i, 4);
            if (l == 0 || l > PCR_MAX_CW_LEN || l < -PCR_MAX_CW_LEN)
                return set_err(c, PCR_E_FORMAT, "batch %lld: decoder table entry %d has code length %d", (long long)bi, i, l);
        }
        int32_t prev = 0;                                             // monotone prefixes keep in-range reads inside the batch
        for (int i = 0; i < 32; ++i) { int32_t x; std::memcpy(&x, v.cl + 4 * i, 4); if (x < prev) return set_err(c, PCR_E_FORMAT, "batch %lld: cluster sizes not monotone", (long long)bi); prev = x; }
        prev = 0;
        for (int i = 0; i < 1024; ++i) { int32_t x; std::memcpy(&x, v.sepsz + 4 * i, 4); if (x < prev) return set_err(c, PCR_E_FORMAT, "batch %lld: separate sizes not monotone", (long long)bi); prev = x; }
    }

    // ---- pass 2: pack into the free pinned arena ------------------------------------------------------------------
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->color_bytes == 0) {
        // the first records of the stream: its colour format is known now (the colour array was allocated for BC1)
        if (color_bytes != PCR_COLOR_BYTES_PER_BATCH) {
            const size_t nB = (size_t)c->hdr.num_batches;
            dfree_counted(c, c->d_colors, nB * PCR_COLOR_BYTES_PER_BATCH);
            dfree_counted(c, c->d_colors_t, nB * PCR_COLOR_BYTES_PER_BATCH);
            int rc = dalloc_zero(c, c->d_colors, nB * color_bytes, &c->stream_bytes);
            if (!rc) rc = dalloc_zero(c, c->d_colors_t, nB * color_bytes, &c->stream_bytes);
            if (rc) return rc;
            // the zero fill was enqueued on the context's stream; the copies and k_transcode's colors_t writes below may run on
            // the loader stream (pcr_set_async_upload), which nothing orders behind it: drain it first, as pcr_stream_begin does
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        c->color_bytes = color_bytes;
    }
    const size_t nb = (size_t)count;
    const size_t o_batches = 0;
    const size_t o_start = o_batches + nb * sizeof(pcr_gpu_batch);
    const size_t o_sepsz = o_start + nb * 3072 * 4;
    const size_t o_tv = o_sepsz + nb * 1024 * 4;
    const size_t o_tl = o_tv + nb * 4096 * 4;
    const size_t o_cl = o_tl + nb * 4096;
    const size_t o_col = o_cl + nb * 32 * 4;
    const size_t o_enc = o_col + nb * color_bytes;
    const size_t o_sep = o_enc + (size_t)sum_ne * 4;
    const size_t total = o_sep + (size_t)sum_ns * 4;
    const int slot = c->arena_next;
    c->arena_next ^= 1;
    if (c->arena_busy[slot]) { HIP_TRY(c, hipEventSynchronize(c->arena_done[slot])); c->arena_busy[slot] = false; }
    if (c->arena_size[slot] < total) {
        if (c->arena[slot]) { (void)hipHostFree(c->arena[slot]); c->arena[slot] = nullptr; c->arena_size[slot] = 0; }
        const size_t want = total + total / 4 + 4096;
        HIP_TRY(c, hipHostMalloc((void **)&c->arena[slot], want, hipHostMallocDefault));
        c->arena_size[slot] = want;
    }
    uint8_t *A = c->arena[slot];
    int64_t enc_ptr = c->enc_ptr, sep_ptr = c->sep_ptr;
    size_t eo = 0, so = 0;
    for (int64_t k = 0; k < count; ++k) {
        const View &v = views[(size_t)k];
        const uint8_t *r = (const uint8_t *)blobs[k];
        double sc[3], of[3]; float bmin[3], bmax[3], lmin[3], lmax[3];
        std::memcpy(sc, r + 20, 24); std::memcpy(of, r + 44, 24);
        std::memcpy(bmin, r + 68, 12); std::memcpy(bmax, r + 80, 12);
        std::memcpy(lmin, r + 92, 12); std::memcpy(lmax, r + 104, 12);
        pcr_gpu_batch g;                                  // HuffmanLasLoader.cpp:188-211
        g.min_x = bmin[0]; g.min_y = bmin[1]; g.min_z = bmin[2];
        g.max_x = bmax[0]; g.max_y = bmax[1]; g.max_z = bmax[2];
        g.scale_x = sc[0]; g.scale_y = sc[1]; g.scale_z = sc[2];
        g.offset_x = of[0]; g.offset_y = of[1]; g.offset_z = of[2];
        g.las_min_x = lmin[0]; g.las_min_y = lmin[1]; g.las_min_z = lmin[2];
        g.las_max_x = lmax[0]; g.las_max_y = lmax[1]; g.las_max_z = lmax[2];
        g.encoding_batch_offset = enc_ptr;
        g.separate_batch_offset = sep_ptr;
        g.decoder_table_offset = (first_index + k) * 4096;
        g.cluster_sizes_offset = (first_index + k) * 32;
        g.max_cw_len = PCR_MAX_CW_LEN;
        const size_t kk = (size_t)k;
        std::memcpy(A + o_batches + kk * sizeof g, &g, sizeof g);
        std::memcpy(A + o_start + kk * 3072 * 4, v.start, 3072 * 4);
        std::memcpy(A + o_sepsz + kk * 1024 * 4, v.sepsz, 1024 * 4);
        std::memcpy(A + o_tv + kk * 4096 * 4, v.tv, 4096 * 4);
        int8_t *tl8 = (int8_t *)(A + o_tl + kk * 4096);
        for (int i = 0; i < 4096; ++i) { int32_t l; std::memcpy(&l, v.tl + 4 * i, 4); tl8[i] = (int8_t)l; }   // render.cu:393
        std::memcpy(A + o_cl + kk * 32 * 4, v.cl, 32 * 4);
        std::memcpy(A + o_col + kk * color_bytes, v.col, color_bytes);
        std::memcpy(A + o_enc + eo, v.enc, (size_t)v.ne * 4); eo += (size_t)v.ne * 4;
        std::memcpy(A + o_sep + so, v.sep, (size_t)v.ns * 4); so += (size_t)v.ns * 4;
        enc_ptr += v.ne; sep_ptr += v.ns;
    }

    // ---- nine copies for the whole task ---------------------------------------------------------------------------
    const size_t b0 = (size_t)first_index;
    hipStream_t st = c->async_upload ? c->copy_stream : c->stream;
    HIP_TRY(c, hipMemcpyAsync(c->d_batches + b0, A + o_batches, nb * sizeof(pcr_gpu_batch), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_start + b0 * 3072, A + o_start, nb * 3072 * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_sep_sizes + b0 * 1024, A + o_sepsz, nb * 1024 * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_table_values + b0 * 4096, A + o_tv, nb * 4096 * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_table_lens + b0 * 4096, A + o_tl, nb * 4096, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_cluster_sizes + b0 * 32, A + o_cl, nb * 32 * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_colors + b0 * color_bytes, A + o_col, nb * color_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_encoded + c->enc_ptr, A + o_enc, (size_t)sum_ne * 4, hipMemcpyHostToDevice, st));
    if (sum_ns) HIP_TRY(c, hipMemcpyAsync(c->d_separate + c->sep_ptr, A + o_sep, (size_t)sum_ns * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->arena_done[slot], st));
    c->arena_busy[slot] = true;
    // the caller's records were copied into the arena: they may be released on return; the device copies complete in
    // stream order before any later render call
    c->enc_ptr = enc_ptr; c->sep_ptr = sep_ptr;
    for (const View &v : views) c->h_stream_words.push_back(v.ne + v.ns);
    c->batches_loaded += count; c->points_loaded += count * PCR_POINTS_PER_BATCH;   // HuffmanLasLoader.cpp:294-295
    { int trc = enqueue_transcode(c, false, st); if (trc) return trc; }    // this context's HBM layout of the stream is part of loading it
    HIP_TRY(c, hipGetLastError());
    if (c->async_upload) {
        // a batch becomes drawable with the task that brings the words behind it (its chains' tail over-reads)
        hipEvent_t ev;
        if (c->loader_events.empty()) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else { ev = c->loader_events.back(); c->loader_events.pop_back(); }
        HIP_TRY(c, hipEventRecord(ev, st));
        c->loader_tasks.push_back({ev, c->transcoded});
    }
    return PCR_OK;
}

int pcr_upload_tail(pcr_ctx *c, const uint32_t *enc, size_t n_enc, const int32_t *sep, size_t n_sep)
{
    if (!c) return PCR_E_ARG;
    c->prepass_ready = false;        // what pcr_frame_begin prepared no longer matches the context's state
    if (!c->stream_open) return set_err(c, PCR_E_ARG, "no stream");
    if (c->finalized) {
        if (n_enc == 0 && n_sep == 0) return PCR_OK;
        return set_err(c, PCR_E_ARG, "the stream was finalised by a frame (raw words released): upload the shard tail before the first render call");
    }
    if (n_enc > PCR_ENCODED_PAD_WORDS || n_sep > PCR_SEPARATE_PAD_WORDS)
        return set_err(c, PCR_E_ARG, "tail larger than the pads (%d / %d words)", PCR_ENCODED_PAD_WORDS, PCR_SEPARATE_PAD_WORDS);
    if ((size_t)(c->enc_words - c->enc_ptr) < n_enc || (size_t)(c->sep_words - c->sep_ptr) < n_sep)
        return set_err(c, PCR_E_ARG, "tail does not fit behind the uploaded batches");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->async_upload) poll_loader(c, true);
    if (n_enc) HIP_TRY(c, hipMemcpyAsync(c->d_encoded + c->enc_ptr, enc, n_enc * 4, hipMemcpyHostToDevice, c->stream));
    if (n_sep) HIP_TRY(c, hipMemcpyAsync(c->d_separate + c->sep_ptr, sep, n_sep * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->batches_loaded > 0 && c->transcoded >= c->batches_loaded) c->transcoded = c->batches_loaded - 1;   // its over-reads see these words
    c->provisional_for = -1;
    if (c->batches_loaded > 0 && (size_t)c->batches_loaded <= c->h_point_bounds_ok.size()) c->h_point_bounds_ok[(size_t)c->batches_loaded - 1] = 0;   // (its cached box too)
    if (c->async_upload) {           // no render-time transcode in this mode: redo the last batch now
        { int trc = enqueue_transcode(c, true, c->stream); if (trc) return trc; }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->batches_resident = c->transcoded;
    }
    return PCR_OK;
}

int pcr_stream_unload(pcr_ctx *c)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_stream_buffers(c);
    return PCR_OK;
}

int pcr_set_stream_layout(pcr_ctx *c, int layout)
{
    if (!c) return PCR_E_ARG;
    if (layout != PCR_LAYOUT_WORDS && layout != PCR_LAYOUT_POINT_WINDOWS && layout != PCR_LAYOUT_BOTH && layout != PCR_LAYOUT_AUTO)
        return set_err(c, PCR_E_ARG, "unknown stream layout %d", layout);
    c->next_layout = layout;         // the stream that is loaded keeps the layout it was loaded with
    return PCR_OK;
}

int pcr_set_hbm_budget(pcr_ctx *c, int64_t bytes)
{
    if (!c || bytes < 0) return PCR_E_ARG;
    c->hbm_budget = bytes;
    return PCR_OK;
}

int pcr_stream_layout(const pcr_ctx *c) { return c && c->stream_open ? c->layout : -1; }

int pcr_set_workgroup_parts(pcr_ctx *c, int parts)
{
    if (!c) return PCR_E_ARG;
    if (parts < 0 || parts > MAX_PARTS) return set_err(c, PCR_E_ARG, "workgroups per batch: 0 (chosen per frame), 1 or 2, not %d", parts);
    c->parts_mode = parts;
    return PCR_OK;
}

int pcr_set_render_variant(pcr_ctx *c, int variant)
{
    if (!c) return PCR_E_ARG;
    if (variant != PCR_VARIANT_AUTO && variant != PCR_VARIANT_WORDS && variant != PCR_VARIANT_POINT_WINDOWS)
        return set_err(c, PCR_E_ARG, "unknown render variant %d", variant);
    c->variant = variant;
    return PCR_OK;
}

int64_t pcr_batches_loaded(const pcr_ctx *c) { return c ? c->batches_loaded : 0; }

int pcr_set_async_upload(pcr_ctx *c, int on)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((on != 0) == c->async_upload) return PCR_OK;
    if (on) {
        if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HIP_TRY(c, hipStreamSynchronize(c->stream));         // earlier loader work (zero fill, copies, transcode) is behind us
        c->batches_resident = c->transcoded;                 // a provisional last batch is drawn again once its successor arrives
        c->async_upload = true;
    } else {
        poll_loader(c, true);
        HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
        c->async_upload = false;
    }
    return PCR_OK;
}

int64_t pcr_last_frame_batches(const pcr_ctx *c) { return c ? c->last_frame_batches : 0; }

int64_t pcr_batches_resident(pcr_ctx *c)
{
    if (!c) return 0;
    if (c->async_upload) poll_loader(c, false);
    return c->visible_batches();
}
int64_t pcr_points_loaded(const pcr_ctx *c) { return c ? c->points_loaded : 0; }

int64_t pcr_stream_resident_bytes(const pcr_ctx *c) { return c && c->stream_open ? (int64_t)c->stream_bytes : 0; }
int pcr_stream_color_format(const pcr_ctx *c)
{
    if (!c || !c->stream_open || c->color_bytes == 0) return 0;
    return c->color_bytes == PCR_COLOR_BYTES_PER_BATCH_BC7 ? PCR_COLOR_BC7 : PCR_COLOR_BC1;
}

int64_t pcr_stream_algorithmic_bytes(const pcr_ctx *c)
{
    if (!c || !c->stream_open) return 0;
    // SURVEY 8d, B_dec: every byte of the compressed representation once = encoded + separate + cluster prefix (128 B per
    // batch) + per-batch side data as the file holds it (GPUBatch 160 + start values 12 288 + escape prefix 4 096 + the
    // two int32 decoder-table arrays 32 768). k_render itself reads the table as 16 KiB of packed entries.
    const int64_t per_batch = 128 + 160 + 12288 + 4096 + 32768;
    return c->enc_ptr * 4 + c->sep_ptr * 4 + c->batches_loaded * per_batch;
}

int64_t pcr_last_frame_algorithmic_bytes(pcr_ctx *c)
{
    if (!c || !c->stream_open || c->last_frame_batches <= 0) return 0;
    const size_t nB = (size_t)std::min<int64_t>(c->last_frame_batches, (int64_t)c->h_stream_words.size());
    std::vector<uint32_t> lod(nB);
    if (hipSetDevice(c->device) != hipSuccess || hipMemcpyAsync(lod.data(), c->d_lod, nB * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    const int64_t per_batch = 128 + 160 + 12288 + 4096 + 32768;
    int64_t bytes = 0;
    for (size_t b = 0; b < nB; ++b) {
        const uint32_t npr = lod[b] & LOD_NPR_MASK;
        if ((lod[b] & LOD_CULLED) || npr == 0) continue;
        bytes += per_batch + (4 * (int64_t)c->h_stream_words[b] * (int64_t)npr) / PCR_POINTS_PER_THREAD;
    }
    return bytes;
}

// ---- method ------------------------------------------------------------------------------------
int pcr_set_image_size(pcr_ctx *c, int w, int h)
{
    if (!c) return PCR_E_ARG;
    c->prepass_ready = false;        // what pcr_frame_begin prepared no longer matches the context's state
    if (w <= 0 || h <= 0 || (int64_t)w * (h + 1) + 1 > 0x7FFFFFFF) return set_err(c, PCR_E_ARG, "bad image size %dx%d", w, h);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const bool external = c->fb && c->fb != c->own_fb;
    if (external) return set_err(c, PCR_E_ARG, "release external buffers before resizing");
    free_frame_buffers(c);
    c->width = w; c->height = h; c->fb_elems = pcr_fb_elems(w, h);
    // PCR_FRAME_PAD_ELEMS behind every buffer: a frame cut into N equal slices for the sliced multi-GPU exchange
    // (include/pcr_dist.h) reaches up to 2 N words past fb_elems. The pads are written here once -- identity of min / sum --
    // and by nothing else but those collectives, which leave them as they were.
    c->fb_alloc = c->fb_elems + PCR_FRAME_PAD_ELEMS;
    HIP_TRY(c, hipMalloc((void **)&c->own_fb, c->fb_alloc * 8));
    HIP_TRY(c, hipMalloc((void **)&c->own_rg, c->fb_alloc * 8));
    HIP_TRY(c, hipMalloc((void **)&c->own_ba, c->fb_alloc * 8));
    HIP_TRY(c, hipMalloc((void **)&c->d_rgba, c->fb_alloc * 4));
    HIP_TRY(c, hipMemsetAsync(c->own_fb + c->fb_elems, 0xFF, PCR_FRAME_PAD_ELEMS * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->own_rg + c->fb_elems, 0, PCR_FRAME_PAD_ELEMS * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->own_ba + c->fb_elems, 0, PCR_FRAME_PAD_ELEMS * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_rgba, 0, c->fb_alloc * 4, c->stream));
    c->tiles_x = (((uint32_t)w - 1u) >> TILE_W_SHIFT) + 1u;
    c->ntiles = c->tiles_x * ((((uint32_t)h + 1u) >> TILE_H_SHIFT) + 1u);        // rows 0 .. h + 1: pixel ids reach w * (h + 1)
    c->tiles_stride = (c->ntiles + 15u) & ~15u;
    HIP_TRY(c, hipMalloc((void **)&c->d_tiles, 3 * (size_t)c->tiles_stride + 16));
    HIP_TRY(c, hipMemsetAsync(c->d_tiles, 0, 3 * (size_t)c->tiles_stride + 16, c->stream));
    c->tile_cur = 0; c->tile_prev = 1; c->tile_spare = 2; c->tile_e_cur = 1; c->tile_e_prev = 0; c->tile_epochs = 1; c->tiles_tracked = false;
    c->fb = c->own_fb; c->rg = c->own_rg; c->ba = c->own_ba;
    c->accum_dirty = true;
    return pcr_clear(c);
}

// Tile flags as a clearing kernel has to leave them (clear_tile_flags); afterwards the context keeps track again. The array that was
// being marked is folded into the image-state array and zeroed by that kernel -- and retired to "spare": the frame that follows marks
// the all-zero third array, so a prepass running in the SAME launch as the clear (pcr_frame_begin, pcr_frame_turn) does not race with
// the zeroing. Call before make_args.
static TileFlags tiles_at_clear(pcr_ctx *c)
{
    TileFlags t = { nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0 };
    if (c->tiles_usable()) {
        t.cur = c->tiles_half(c->tile_cur); t.prev = c->tiles_half(c->tile_prev); t.cur_all = c->tiles_all(c->tile_cur); t.prev_all = c->tiles_all(c->tile_prev);
        t.ntiles = c->ntiles; t.tracked = c->tiles_tracked ? 1 : 0;
        if (c->tile_e_prev == 0) c->tile_e_prev = ++c->tile_epochs;     // (never used yet: any value no word holds)
        t.e_cur = c->tile_e_cur; t.e_prev = c->tile_e_prev;
        std::swap(c->tile_cur, c->tile_spare);
        c->tile_e_cur = ++c->tile_epochs;       // (a fresh epoch: the new array's "everything" word cannot hold it yet)
        c->tiles_tracked = true;
    } else {
        c->tiles_tracked = false;
    }
    return t;
}

int pcr_clear(pcr_ctx *c)
{
    if (!c) return PCR_E_ARG;
    c->prepass_ready = false;        // what pcr_frame_begin prepared no longer matches the context's state
    if (!c->fb) return set_err(c, PCR_E_ARG, "no framebuffer");
    HIP_TRY(c, hipSetDevice(c->device));
    // huffman_hqs.h:267-269. HuffmanMemIter clears only fb (huffman_mem_iter_cuda.h:250-252); RG/BA are re-zeroed only
    // after a colour pass (or when the buffers changed hands), which saves two 16.6 MB fills per basic frame at 1080p
    uint64_t *rg = c->accum_dirty ? c->rg : nullptr, *ba = c->accum_dirty ? c->ba : nullptr;
    if (((uintptr_t)c->fb | (uintptr_t)rg | (uintptr_t)ba) & 15) return set_err(c, PCR_E_ARG, "framebuffers must be 16-byte aligned");
    hipLaunchKernelGGL(k_clear, dim3(2048), dim3(256), 0, c->stream, c->fb, rg, ba, c->fb_elems, c->empty_key, tiles_at_clear(c));
    HIP_TRY(c, hipGetLastError());
    c->accum_dirty = false;
    return PCR_OK;
}

int pcr_frame_begin(pcr_ctx *c, const pcr_render_params *p, int method)
{
    int rc = check_params(c, p);
    if (rc) return rc;
    if (method != PCR_METHOD_BASIC && method != PCR_METHOD_HQS) return set_err(c, PCR_E_ARG, "unknown method %d", method);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->async_upload) poll_loader(c, false);
    const int64_t nB = c->visible_batches();
    if (nB == 0) return pcr_clear(c);
    uint64_t *rg = c->accum_dirty ? c->rg : nullptr, *ba = c->accum_dirty ? c->ba : nullptr;
    if (((uintptr_t)c->fb | (uintptr_t)rg | (uintptr_t)ba) & 15) return set_err(c, PCR_E_ARG, "framebuffers must be 16-byte aligned");
    if (!c->async_upload && (rc = enqueue_transcode(c, true, c->stream))) return rc;   // the prepass sorts batches by what k_transcode found out about them
    maybe_finalize(c);
    const TileFlags tflags = tiles_at_clear(c);
    RenderArgs a = make_args(c, p, method != PCR_METHOD_BASIC);
    a.win_pixel_bytes = WIN_PIXEL_BYTES;         // first pass of either method (basic / HQS depth)
    if (method == PCR_METHOD_HQS) a.win_hqs = c->d_win + c->hdr.num_batches * MAX_PARTS;     // ... and the colour pass's plan with it
    a.dyn_lds_bytes = frame_dyn_lds(c, nB);
    c->stats_partials = (int)((nB + PREPASS_BATCHES - 1) / PREPASS_BATCHES);
    const uint32_t prepass_wgs = (uint32_t)c->stats_partials * PREPASS_WGS_PER_CHUNK;       // (two workgroups per chunk: lists / plans)
    hipLaunchKernelGGL(k_frame_begin, dim3(prepass_wgs + 2048u), dim3(256), 0, c->stream, a,
                       prepass_wgs, c->fb, rg, ba, c->fb_elems, c->empty_key, tflags);
    HIP_TRY(c, hipGetLastError());
    c->accum_dirty = false;
    c->prepass_ready = true;
    c->prepass_params = *p; c->prepass_variant_hqs = a.variant_hqs; c->prepass_slots = a.win_hqs ? 3u : 1u;
    c->prepass_dyn_lds = a.dyn_lds_bytes; c->prepass_parts = a.parts;
    c->prepass_batches = nB;
    return PCR_OK;
}

static int launch_resolve(pcr_ctx *c, const pcr_render_params *p, bool hqs);

// The end of one frame and the start of the next in one launch: resolve (flags of p_done) -> d_rgba, CLEAR, and the cull/LOD
// prepass for p_next. Equivalent to pcr_resolve_* followed by pcr_frame_begin(p_next); the framebuffer is empty afterwards
// (read it before, if it is wanted: the depth dump does), the image is in pcr_read_rgba as after pcr_resolve_*.
int pcr_frame_turn(pcr_ctx *c, const pcr_render_params *p_done, const pcr_render_params *p_next, int method)
{
    int rc = check_params(c, p_next);
    if (rc) return rc;
    if (!p_done) return set_err(c, PCR_E_ARG, "params of the finished frame are NULL");
    if (p_done->width != c->width || p_done->height != c->height) return set_err(c, PCR_E_ARG, "params image size != framebuffer");
    if (method != PCR_METHOD_BASIC && method != PCR_METHOD_HQS) return set_err(c, PCR_E_ARG, "unknown method %d", method);
    const bool hqs = method == PCR_METHOD_HQS;
    if (hqs && (!c->rg || !c->ba)) return set_err(c, PCR_E_ARG, "no RG/BA accumulation buffers");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->async_upload) poll_loader(c, false);
    const int64_t nB = c->visible_batches();
    if (nB == 0) {                                   // nothing to prepare: the two separate steps
        if ((rc = launch_resolve(c, p_done, hqs))) return rc;
        return pcr_clear(c);
    }
    if (!hqs && c->accum_dirty) {                    // a basic frame behind an HQS one: RG/BA are zeroed by the ordinary CLEAR
        if ((rc = launch_resolve(c, p_done, false))) return rc;
        return pcr_frame_begin(c, p_next, method);
    }
    if (!c->async_upload && (rc = enqueue_transcode(c, true, c->stream))) return rc;
    maybe_finalize(c);
    RenderArgs a = make_args(c, p_next, hqs);
    a.win_pixel_bytes = WIN_PIXEL_BYTES;
    if (hqs) a.win_hqs = c->d_win + c->hdr.num_batches * MAX_PARTS;
    a.dyn_lds_bytes = frame_dyn_lds(c, nB);
    c->stats_partials = (int)((nB + PREPASS_BATCHES - 1) / PREPASS_BATCHES);
    const uint32_t prepass_wgs = (uint32_t)c->stats_partials * PREPASS_WGS_PER_CHUNK;       // (two workgroups per chunk: lists / plans)
    const uint32_t pixels = (uint32_t)((size_t)c->width * c->height);
    if (c->tiles_usable() && c->tiles_tracked) {
        // only the tiles something was written in (and those the image still holds something in): FrameView::tiles
        // what the finished frame marked (cur) and what the image may still hold (prev) are read, prev is left zeroed; this launch's
        // own prepass marks the NEXT frame's tiles in the third array (all zero since the turn before)
        TileFlags tf = { c->tiles_half(c->tile_cur), c->tiles_half(c->tile_prev), c->tiles_all(c->tile_cur), c->tiles_all(c->tile_prev),
                         c->ntiles, c->tile_e_cur, c->tile_e_prev, 1 };
        const int cur = c->tile_cur, prev = c->tile_prev, spare = c->tile_spare;
        c->tile_cur = spare; c->tile_prev = cur; c->tile_spare = prev;
        c->tile_e_prev = c->tile_e_cur; c->tile_e_cur = ++c->tile_epochs;
        a.f.tiles = c->tiles_half(c->tile_cur); a.f.tiles_all = c->tiles_all(c->tile_cur); a.f.tiles_epoch = c->tile_e_cur;      // (the prepass of the next frame)
        const unsigned grid = prepass_wgs + std::min<unsigned>(c->ntiles, 4096u);
        if (hqs) hipLaunchKernelGGL(k_frame_turn_tiles<true>, dim3(grid), dim3(256), 0, c->stream, a, prepass_wgs, p_done->show_num_points,
                                    p_done->colorize_chunks, (uint32_t)c->width, pixels, c->fb, c->rg, c->ba, c->d_rgba, (uint32_t)c->fb_elems, c->empty_key,
                                    tf, c->tiles_x);
        else     hipLaunchKernelGGL(k_frame_turn_tiles<false>, dim3(grid), dim3(256), 0, c->stream, a, prepass_wgs, p_done->show_num_points,
                                    p_done->colorize_chunks, (uint32_t)c->width, pixels, c->fb, c->rg, c->ba, c->d_rgba, (uint32_t)c->fb_elems, c->empty_key,
                                    tf, c->tiles_x);
    } else {
        const unsigned grid = prepass_wgs + 2048u;
        const TileFlags tflags = tiles_at_clear(c);
        a.f.tiles = c->tiles_tracked ? c->tiles_half(c->tile_cur) : nullptr;     // (the prepass of the next frame marks the fresh array)
        a.f.tiles_all = c->d_tiles ? c->tiles_all(c->tile_cur) : nullptr; a.f.tiles_epoch = c->tile_e_cur;
        if (hqs) hipLaunchKernelGGL(k_frame_turn<true>, dim3(grid), dim3(256), 0, c->stream, a, prepass_wgs, p_done->show_num_points,
                                    p_done->colorize_chunks, pixels, c->fb, c->rg, c->ba, c->d_rgba, (uint32_t)c->fb_elems, c->empty_key, tflags);
        else     hipLaunchKernelGGL(k_frame_turn<false>, dim3(grid), dim3(256), 0, c->stream, a, prepass_wgs, p_done->show_num_points,
                                    p_done->colorize_chunks, pixels, c->fb, c->rg, c->ba, c->d_rgba, (uint32_t)c->fb_elems, c->empty_key, tflags);
    }
    HIP_TRY(c, hipGetLastError());
    c->accum_dirty = false;
    c->prepass_ready = true;
    c->prepass_params = *p_next; c->prepass_variant_hqs = a.variant_hqs; c->prepass_slots = a.win_hqs ? 3u : 1u;
    c->prepass_dyn_lds = a.dyn_lds_bytes; c->prepass_parts = a.parts;
    c->prepass_batches = nB;
    return PCR_OK;
}

int pcr_set_int64_mergeable(pcr_ctx *c, int on)
{
    if (!c) return PCR_E_ARG;
    c->empty_key = on ? 0x7FFFFFFFFFFFFFFFull : ~0ull;
    c->tiles_tracked = false;       // a tile turn rewrites the empty word in the dirty tiles only: the next clear has to be a full one
    return PCR_OK;
}

int pcr_render_basic(pcr_ctx *c, const pcr_render_params *p)
{
    // COLOR_COMPRESSION == 7 is not a defined configuration of the reference's basic method: its rasterize decodes the colour
    // array as BC1 whatever the setting (huffman_mem_iter_cuda/render.cu:299) and its resolve then indexes that array with
    // the resulting COLOUR as if it were a point id (resolve.cu:183) -- an out-of-bounds read. Only the HQS method draws BC7.
    if (c && c->stream_open && c->color_bytes == PCR_COLOR_BYTES_PER_BATCH_BC7)
        return set_err(c, PCR_E_ARG, "the basic method is not defined for a stream with BC7 colours (use the HQS method)");
    return launch_render<MODE_BASIC>(c, p);
}
int pcr_render_hqs_depth(pcr_ctx *c, const pcr_render_params *p) { return launch_render<MODE_HQS_DEPTH>(c, p); }
int pcr_render_hqs_color(pcr_ctx *c, const pcr_render_params *p)
{
    if (c && (!c->rg || !c->ba)) return set_err(c, PCR_E_ARG, "no RG/BA accumulation buffers");
    if (c) c->accum_dirty = true;
    if (c && c->stream_open && c->color_bytes == PCR_COLOR_BYTES_PER_BATCH_BC7) return launch_render<MODE_HQS_COLOR_BC7>(c, p);
    return launch_render<MODE_HQS_COLOR>(c, p);
}

// ---- 10-10-10 path ------------------------------------------------------------------------------
int pcr_las_begin(pcr_ctx *c, int64_t num_points)
{
    if (!c) return PCR_E_ARG;
    if (num_points <= 0) return set_err(c, PCR_E_ARG, "num_points must be > 0");
    const int64_t nB = (num_points + PCR_POINTS_PER_BATCH - 1) / PCR_POINTS_PER_BATCH;
    if (nB * PCR_POINTS_PER_BATCH >= 0x7FFFFFFFll)         // the framebuffer key holds a 31-bit point index (resolve.cu)
        return set_err(c, PCR_E_ARG, "%lld points exceed the 31-bit point index of the 10-10-10 framebuffer", (long long)num_points);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_las_buffers(c);
    const size_t slots = (size_t)nB * PCR_POINTS_PER_BATCH;
    int rc;
    if ((rc = dalloc_zero(c, c->d_xyzb, (size_t)nB)) || (rc = dalloc_zero(c, c->d_xyz12, slots)) ||
        (rc = dalloc_zero(c, c->d_xyz8, slots)) || (rc = dalloc_zero(c, c->d_xyz4, slots)) ||
        (rc = dalloc_zero(c, c->d_point_rgba, slots)) || (rc = dalloc_zero(c, c->d_las_level, (size_t)nB)) ||
        (rc = dalloc_zero(c, c->d_las_win, (size_t)nB)) || (rc = dalloc_zero(c, c->d_las_win_hqs, (size_t)nB)) ||
        (rc = dalloc_zero(c, c->d_las_order, (size_t)((nB + LAS_PREPASS_BATCHES - 1) / LAS_PREPASS_BATCHES) * LAS_PREPASS_BATCHES)) ||
        (rc = dalloc_zero(c, c->d_las_chunk_count, (size_t)LAS_CLASSES * (size_t)((nB + LAS_PREPASS_BATCHES - 1) / LAS_PREPASS_BATCHES)))) {
        free_las_buffers(c);
        return rc == PCR_E_HIP ? set_err(c, PCR_E_NOMEM, "out of device memory for %lld batches", (long long)nB) : rc;
    }
    c->las_capacity = nB; c->las_loaded = 0; c->las_open = true;
    return PCR_OK;
}

int pcr_las_upload(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_xyz_batch *batches, const uint32_t *xyz12,
                   const uint32_t *xyz8, const uint32_t *xyz4, const uint32_t *rgba)
{
    if (!c) return PCR_E_ARG;
    if (!c->las_open) return set_err(c, PCR_E_ARG, "pcr_las_begin has not been called");
    if (!batches || !xyz12 || !xyz8 || !xyz4 || !rgba) return set_err(c, PCR_E_ARG, "NULL input array");
    if (count <= 0 || first_batch != c->las_loaded || first_batch + count > c->las_capacity)
        return set_err(c, PCR_E_ARG, "batches [%lld,%lld) out of order or beyond the %lld allocated (next expected %lld)",
                       (long long)first_batch, (long long)(first_batch + count), (long long)c->las_capacity, (long long)c->las_loaded);
    for (int64_t i = 0; i < count; ++i) {
        const pcr_xyz_batch &g = batches[i];
        if (!(g.min_x <= g.max_x && g.min_y <= g.max_y && g.min_z <= g.max_z) || g.num_points < 0 || g.num_points > PCR_POINTS_PER_BATCH)
            return set_err(c, PCR_E_FORMAT, "batch %lld: bad bounding box or point count", (long long)(first_batch + i));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t off = (size_t)first_batch * PCR_POINTS_PER_BATCH, n = (size_t)count * PCR_POINTS_PER_BATCH * 4;
    HIP_TRY(c, hipMemcpyAsync(c->d_xyzb + first_batch, batches, (size_t)count * sizeof(pcr_xyz_batch), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_xyz12 + off, xyz12, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_xyz8 + off, xyz8, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_xyz4 + off, xyz4, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_point_rgba + off, rgba, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));             // the arrays are borrowed for the call only
    c->las_loaded += count;
    return PCR_OK;
}

int pcr_las_unload(pcr_ctx *c)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_las_buffers(c);
    return PCR_OK;
}

int64_t pcr_las_batches_loaded(const pcr_ctx *c) { return c ? c->las_loaded : 0; }

static int check_las(pcr_ctx *c, const pcr_render_params *p)
{
    if (!c) return PCR_E_ARG;
    if (!p) return set_err(c, PCR_E_ARG, "render params are NULL");
    if (!c->las_open) return set_err(c, PCR_E_ARG, "no 10-10-10 data loaded (call pcr_las_begin / pcr_las_upload)");
    if (!c->fb) return set_err(c, PCR_E_ARG, "no framebuffer (call pcr_set_image_size)");
    if (p->width != c->width || p->height != c->height)
        return set_err(c, PCR_E_ARG, "params image size %dx%d != framebuffer %dx%d", p->width, p->height, c->width, c->height);
    return PCR_OK;
}

// The three 10-10-10 passes: prepass (cull, level, windows, draw list) + one workgroup per drawn batch. Every call runs its own
// prepass (a few microseconds: one lane per batch), so each fills pcr_get_stats and none depends on the one before.
enum LasPass { LAS_BASIC, LAS_HQS_DEPTH, LAS_HQS_COLOR };

static int launch_las(pcr_ctx *c, const pcr_render_params *p, LasPass pass)
{
    int rc = check_las(c, p);
    if (rc) return rc;
    const int64_t nB = c->las_loaded;
    if (nB == 0) { c->stats_partials = 0; return PCR_OK; }     // compute_loop_las_cuda.h:107
    c->prepass_ready = false;        // d_stats is shared with the Huffman methods' prepass
    LasArgs a;
    a.p = *p;
    a.s.batches = c->d_xyzb; a.s.xyz12 = c->d_xyz12; a.s.xyz8 = c->d_xyz8; a.s.xyz4 = c->d_xyz4; a.s.num_batches = nB;
    a.f.fb = c->fb; a.f.rg = c->rg; a.f.ba = c->ba; a.f.fb_elems = (uint32_t)c->fb_elems;
    a.f.tiles = nullptr; a.f.tiles_all = nullptr; a.f.tiles_x = 0; a.f.tiles_epoch = 0; a.f.tiles_total = 0;
    c->tiles_tracked = false;        // (this method's kernels do not mark tiles)
    a.level = c->d_las_level; a.win = c->d_las_win; a.stats = c->d_stats; a.win_capacity = WIN_PIXELS;
    c->stats_partials = (int)((nB + PREPASS_THREADS - 1) / PREPASS_THREADS);
    a.order = c->d_las_order; a.chunk_count = c->d_las_chunk_count; a.chunks = (uint32_t)c->stats_partials;
    a.win_hqs = pass == LAS_HQS_COLOR ? c->d_las_win_hqs : nullptr; a.win_capacity_hqs = LAS_WIN_PIXELS_HQS;
    a.rgba_points = c->d_point_rgba;
    hipLaunchKernelGGL(k_las_prepass, dim3((unsigned)c->stats_partials), dim3(PREPASS_THREADS), 0, c->stream, a);
    const bool timed = c->kt_sample_now();
    const int slot = (int)(c->kt_samples % pcr_ctx::KT_PAIRS);
    if (timed) HIP_TRY(c, hipEventRecord(c->kt_begin[slot], c->stream));
    if (pass == LAS_BASIC)          hipLaunchKernelGGL(k_las_render<false>, dim3((unsigned)nB), dim3(PCR_WORKGROUP_SIZE), 0, c->stream, a);
    else if (pass == LAS_HQS_DEPTH) hipLaunchKernelGGL(k_las_render<true>, dim3((unsigned)nB), dim3(PCR_WORKGROUP_SIZE), 0, c->stream, a);
    else                            hipLaunchKernelGGL(k_las_render_color, dim3((unsigned)nB), dim3(PCR_WORKGROUP_SIZE), 0, c->stream, a);
    if (timed) { HIP_TRY(c, hipEventRecord(c->kt_end[slot], c->stream)); ++c->kt_samples; }
    if (c->kt_every > 0) ++c->kt_launches;
    if (pass == LAS_HQS_COLOR) c->accum_dirty = true;           // RG / BA written: the next pcr_clear zeroes them
    c->las_last_color = pass == LAS_HQS_COLOR;
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_render_las(pcr_ctx *c, const pcr_render_params *p) { return launch_las(c, p, LAS_BASIC); }
int pcr_render_las_hqs_depth(pcr_ctx *c, const pcr_render_params *p) { return launch_las(c, p, LAS_HQS_DEPTH); }
int pcr_render_las_hqs_color(pcr_ctx *c, const pcr_render_params *p)
{
    if (c && (!c->rg || !c->ba)) return set_err(c, PCR_E_ARG, "no RG/BA accumulation buffers");
    return launch_las(c, p, LAS_HQS_COLOR);
}

int pcr_resolve_las(pcr_ctx *c, const pcr_render_params *p)
{
    int rc = check_las(c, p);
    if (rc) return rc;
    dim3 grid((unsigned)((c->width + 15) / 16), (unsigned)((c->height + 15) / 16));
    hipLaunchKernelGGL(k_las_resolve, grid, dim3(256), 0, c->stream, c->width, c->height, c->fb, c->d_point_rgba, c->d_rgba);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int64_t pcr_las_algorithmic_bytes(pcr_ctx *c)
{
    if (!c || !c->las_open || c->las_loaded == 0) return 0;
    std::vector<int32_t> level((size_t)c->las_loaded);
    if (hipMemcpyAsync(level.data(), c->d_las_level, level.size() * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    int64_t bytes = 0;
    for (int64_t b = 0; b + 1 < c->las_loaded; ++b) {         // the last workgroup does not run
        const int l = level[(size_t)b];
        if (l < 0) continue;
        bytes += (int64_t)sizeof(pcr_xyz_batch) + (int64_t)PCR_POINTS_PER_BATCH * 4 * ((l >= 2 ? 1 : l == 1 ? 2 : 3) + (c->las_last_color ? 1 : 0));
    }
    return bytes;
}

static int launch_resolve(pcr_ctx *c, const pcr_render_params *p, bool hqs)
{
    if (!c) return PCR_E_ARG;
    if (!p) return set_err(c, PCR_E_ARG, "params are NULL");
    if (!c->fb) return set_err(c, PCR_E_ARG, "no framebuffer");
    if (p->width != c->width || p->height != c->height) return set_err(c, PCR_E_ARG, "params image size != framebuffer");
    dim3 grid((unsigned)((c->width + 15) / 16), (unsigned)((c->height + 15) / 16));   // huffman_hqs.h:249-250
    if (hqs) hipLaunchKernelGGL(k_resolve<true>, grid, dim3(256), 0, c->stream, p->show_num_points, p->colorize_chunks, c->width, c->height, c->fb, c->rg, c->ba, c->d_rgba);
    else     hipLaunchKernelGGL(k_resolve<false>, grid, dim3(256), 0, c->stream, p->show_num_points, p->colorize_chunks, c->width, c->height, c->fb, c->rg, c->ba, c->d_rgba);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}
int pcr_resolve_basic(pcr_ctx *c, const pcr_render_params *p) { return launch_resolve(c, p, false); }
int pcr_resolve_hqs(pcr_ctx *c, const pcr_render_params *p) { return launch_resolve(c, p, true); }

// ---- display resolves (n x n point size, eye-dome lighting) ------------------------------------------------
// The preconditions of the plain resolve of `method`, then the options; one launch of k_resolve_display over the whole frame.
static int launch_resolve_display(pcr_ctx *c, const pcr_render_params *p, const pcr_display_opts *o, int method)
{
    if (method == DISPLAY_LAS) {
        const int rc = check_las(c, p);
        if (rc) return rc;
    } else {
        if (!c) return PCR_E_ARG;
        if (!p) return set_err(c, PCR_E_ARG, "params are NULL");
        if (!c->fb) return set_err(c, PCR_E_ARG, "no framebuffer");
        if (p->width != c->width || p->height != c->height) return set_err(c, PCR_E_ARG, "params image size != framebuffer");
        if (method == DISPLAY_HQS && (!c->rg || !c->ba)) return set_err(c, PCR_E_ARG, "no RG/BA accumulation buffers");
    }
    if (!o) return set_err(c, PCR_E_ARG, "display options are NULL");
    if (o->window < 0 || o->window > PCR_DISPLAY_MAX_WINDOW)
        return set_err(c, PCR_E_ARG, "display window %d outside [0, %d]", o->window, PCR_DISPLAY_MAX_WINDOW);
    if (o->edl_window < 0 || o->edl_window > PCR_DISPLAY_MAX_EDL_WINDOW)
        return set_err(c, PCR_E_ARG, "display edl_window %d outside [0, %d]", o->edl_window, PCR_DISPLAY_MAX_EDL_WINDOW);
    if (o->edl_window > 0 && !(o->edl_strength >= 0.0f && o->edl_strength <= FLT_MAX))
        return set_err(c, PCR_E_ARG, "display edl_strength must be finite and >= 0");
    if (o->reserved != 0) return set_err(c, PCR_E_ARG, "display options: reserved must be 0");
    DisplayArgs a{};
    a.width = c->width; a.height = c->height;
    a.window = o->window; a.edl_window = o->edl_window; a.edl_strength = o->edl_strength;
    a.show_num_points = p->show_num_points; a.colorize_chunks = p->colorize_chunks;
    a.empty = c->empty_key;
    a.fb = c->fb; a.rg = c->rg; a.ba = c->ba;
    a.rgba_points = c->d_point_rgba;
    a.rgba = c->d_rgba;
    const dim3 grid((unsigned)((c->width + DISPLAY_TW - 1) / DISPLAY_TW), (unsigned)((c->height + DISPLAY_TH - 1) / DISPLAY_TH));
    const bool edl = o->edl_window > 0;
#define PCR_DISPLAY_LAUNCH(M) \
    do { if (edl) hipLaunchKernelGGL((k_resolve_display<M, true>), grid, dim3(DISPLAY_THREADS), 0, c->stream, a); \
         else     hipLaunchKernelGGL((k_resolve_display<M, false>), grid, dim3(DISPLAY_THREADS), 0, c->stream, a); } while (0)
    if (method == DISPLAY_BASIC)    PCR_DISPLAY_LAUNCH(DISPLAY_BASIC);
    else if (method == DISPLAY_HQS) PCR_DISPLAY_LAUNCH(DISPLAY_HQS);
    else                            PCR_DISPLAY_LAUNCH(DISPLAY_LAS);
#undef PCR_DISPLAY_LAUNCH
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}
int pcr_resolve_basic_display(pcr_ctx *c, const pcr_render_params *p, const pcr_display_opts *o) { return launch_resolve_display(c, p, o, DISPLAY_BASIC); }
int pcr_resolve_hqs_display(pcr_ctx *c, const pcr_render_params *p, const pcr_display_opts *o) { return launch_resolve_display(c, p, o, DISPLAY_HQS); }
int pcr_resolve_las_display(pcr_ctx *c, const pcr_render_params *p, const pcr_display_opts *o) { return launch_resolve_display(c, p, o, DISPLAY_LAS); }

int pcr_get_stats(pcr_ctx *c, pcr_render_stats *out)
{
    if (!c || !out) return PCR_E_ARG;
    std::vector<pcr_render_stats> part((size_t)PCR_STATS_PARTIALS);
    std::memset(out, 0, sizeof *out);
    if (c->stats_partials > 0) {
        HIP_TRY(c, hipMemcpyAsync(part.data(), c->d_stats, (size_t)c->stats_partials * sizeof(pcr_render_stats), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < c->stats_partials; ++i) {
            out->batches_total += part[i].batches_total; out->batches_culled += part[i].batches_culled;
            out->points_iterated += part[i].points_iterated; out->batches_double += part[i].batches_double;
        }
    }
    return PCR_OK;
}

int pcr_read_framebuffer(pcr_ctx *c, uint64_t *host, size_t n)
{
    if (!c || !host) return PCR_E_ARG;
    if (!c->fb || n > c->fb_elems) return set_err(c, PCR_E_ARG, "bad framebuffer read of %zu elements", n);
    HIP_TRY(c, hipMemcpyAsync(host, c->fb, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->empty_key != ~0ull)                   // the caller always sees the reference's empty word
        for (size_t i = 0; i < n; ++i) if (host[i] == c->empty_key) host[i] = ~0ull;
    return PCR_OK;
}

int pcr_read_accum(pcr_ctx *c, uint64_t *hrg, uint64_t *hba, size_t n)
{
    if (!c || !hrg || !hba) return PCR_E_ARG;
    if (!c->rg || !c->ba || n > c->fb_elems) return set_err(c, PCR_E_ARG, "bad accumulation read");
    HIP_TRY(c, hipMemcpyAsync(hrg, c->rg, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hba, c->ba, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

int pcr_read_rgba(pcr_ctx *c, uint32_t *host, size_t n)
{
    if (!c || !host) return PCR_E_ARG;
    if (!c->d_rgba || n > (size_t)c->width * c->height) return set_err(c, PCR_E_ARG, "bad rgba read");
    HIP_TRY(c, hipMemcpyAsync(host, c->d_rgba, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

// ---- shared by the decode, selection and kept-rows calls -----------------------------------------
extern "C++" {                          // (templates among them)
namespace {
// A stream that holds both layouts follows pcr_set_render_variant (AUTO: point windows); either decodes to the same points.
bool select_reads_windows(const pcr_ctx *c)
{
    const bool have_windows = c->layout != PCR_LAYOUT_WORDS, have_words = c->layout != PCR_LAYOUT_POINT_WINDOWS;
    return have_windows && (c->variant != PCR_VARIANT_WORDS || !have_words);
}

// launch(layout) with the layout the calls read as a std::integral_constant: the template argument of a kernel that decodes
// positions only
template <class Launch>
void for_layout(const pcr_ctx *c, Launch launch)
{
    if (select_reads_windows(c)) launch(std::integral_constant<int, LAYOUT_POINT_WINDOWS>{});
    else                         launch(std::integral_constant<int, LAYOUT_WORDS>{});
}

// launch(layout, bc7) with the stream's colour format as well: the template arguments of a kernel that decodes with colour
template <class Launch>
void for_layout_bc7(const pcr_ctx *c, Launch launch)
{
    const bool bc7 = c->color_bytes == PCR_COLOR_BYTES_PER_BATCH_BC7;
    for_layout(c, [&](auto layout) { if (bc7) launch(layout, std::true_type{}); else launch(layout, std::false_type{}); });
}

// launch(layout, colour) for the kernels that can leave the colour out: SEL_NO_COLOUR unless `coloured`, else the stream's format
template <class Launch>
void for_layout_colour(const pcr_ctx *c, bool coloured, Launch launch)
{
    const bool bc7 = c->color_bytes == PCR_COLOR_BYTES_PER_BATCH_BC7;
    for_layout(c, [&](auto layout) {
        if (!coloured) launch(layout, std::integral_constant<int, SEL_NO_COLOUR>{});
        else if (bc7)  launch(layout, std::integral_constant<int, SEL_BC7>{});
        else           launch(layout, std::integral_constant<int, SEL_BC1>{});
    });
}

// Let each of `kernels` launch with `bytes` of dynamic LDS (the callers do it once per context)
template <class... Kernels>
int lds_allow(pcr_ctx *c, size_t bytes, Kernels... kernels)
{
    for (const void *k : {reinterpret_cast<const void *>(kernels)...}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return set_err(c, PCR_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(e));
    }
    return PCR_OK;
}

// *p holds at least `want` elements on return (a larger array replaces it, its content is not kept), or false
bool thin_grow(void **p, int64_t &have, int64_t want, size_t elem_bytes)
{
    if (*p && have >= want) return true;
    if (*p) (void)hipFree(*p);
    *p = nullptr; have = 0;
    if (hipMalloc(p, (size_t)want * elem_bytes) != hipSuccess) { *p = nullptr; return false; }
    have = want;
    return true;
}

// thin_grow for the scratch of the selections, with the refusal
template <class T>
int reserve(pcr_ctx *c, T *&p, int64_t &capacity, int64_t need, const char *what)
{
    if (thin_grow((void **)&p, capacity, need, sizeof(T))) return PCR_OK;
    return set_err(c, PCR_E_NOMEM, "out of device memory for %lld %s", (long long)need, what);
}

// Room for the list, counts, totals and offsets of `need` batches
template <class Entry>
int scratch_reserve(pcr_ctx *c, BatchScratch<Entry> &b, int64_t need, const char *what)
{
    if (b.capacity >= need) return PCR_OK;
    int64_t list = 0, totals = 0, offsets = 0, counts = 0;          // (nothing is kept: every array is replaced)
    b.capacity = 0;
    int rc;
    if ((rc = reserve(c, b.list, list, need, what)) || (rc = reserve(c, b.totals, totals, need, what)) || (rc = reserve(c, b.offsets, offsets, need, what)) ||
        (rc = reserve(c, b.counts, counts, need * PCR_WORKGROUP_SIZE, what))) return rc;
    b.capacity = need;
    return PCR_OK;
}

// Range check of the calls over batches: [first, first + count) inside the batches the next frame would draw; count < 0 = up to
// the last of them. Returns the count through *n.
int select_range(pcr_ctx *c, int64_t first, int64_t count, int64_t *n)
{
    if (!c->stream_open) return set_err(c, PCR_E_ARG, "no stream loaded (call pcr_stream_begin / pcr_upload_batch)");
    if (c->async_upload) poll_loader(c, false);
    const int64_t nB = c->visible_batches();
    if (first < 0 || first > nB) return set_err(c, PCR_E_ARG, "first batch %lld outside the %lld resident batches", (long long)first, (long long)nB);
    if (count < 0) count = nB - first;
    if (count > nB - first)
        return set_err(c, PCR_E_ARG, "batches [%lld, %lld) reach past the %lld resident batches", (long long)first, (long long)(first + count), (long long)nB);
    *n = count;
    return PCR_OK;
}

// What a call writes per row: the record to `points` and up to three columns, `name` as the messages call them, aligned to
// dev_align bytes on the device and host_align on the host. Any destination may be NULL, each holds `capacity` rows. host: the
// destinations are host memory (the pcr_read_ form).
struct KeptColumn { const char *name; void *dst; size_t row_bytes; size_t dev_align = 8, host_align = alignof(int64_t); };
struct KeptOut {
    bool host;
    void *points;
    size_t capacity;
    KeptColumn col[3];
};
// (the columns of the selections)
KeptColumn heights_column(void *dst) { return KeptColumn{"heights", dst, 4, 4, alignof(int32_t)}; }
KeptColumn hits_column(void *dst) { return KeptColumn{"hits", dst, sizeof(pcr_screen_hit), 16, alignof(pcr_screen_hit)}; }

// The checks every call starts with: the range into *n, the lattice where the call has one (has_lattice), out_count and the
// alignment of the destinations: 16 bytes for the points on the device, the type's own on the host. *out_count is 0 from here on.
int kept_begin(pcr_ctx *c, int64_t first, int64_t count, const KeptOut &o, int64_t *out_count, int64_t *n, bool has_lattice = false,
               const pcr_voxels *vox = nullptr)
{
    if (out_count) *out_count = 0;
    int rc = select_range(c, first, count, n);
    if (rc) return rc;
    if (has_lattice && !vox) return set_err(c, PCR_E_ARG, "the voxel lattice is NULL");
    if (!out_count) return set_err(c, PCR_E_ARG, "out_count is NULL");
    const size_t points_align = o.host ? alignof(pcr_point) : 16;
    if (o.points && reinterpret_cast<uintptr_t>(o.points) % points_align != 0)
        return set_err(c, PCR_E_ARG, "the destination of the points is misaligned (%zu bytes)", points_align);
    for (const KeptColumn &k : o.col)
        if (k.dst && reinterpret_cast<uintptr_t>(k.dst) % (o.host ? k.host_align : k.dev_align) != 0)
            return set_err(c, PCR_E_ARG, "the destination of the %s is misaligned (%zu bytes)", k.name, o.host ? k.host_align : k.dev_align);
    if (vox && (vox->cell < 1 || vox->cell > PCR_THIN_MAX_CELL))
        return set_err(c, PCR_E_ARG, "voxel cell of %d: the edge length is 1 .. %d (PCR_THIN_MAX_CELL)", vox->cell, PCR_THIN_MAX_CELL);
    return PCR_OK;
}

// After the plan: the count and the statistics out; *done unless something is left to write, which is not so for a count-only
// call, without rows, or where `kept` rows (`noun` in the message) do not fit the capacity
template <class Stats>
int kept_finish(pcr_ctx *c, const KeptOut &o, int64_t kept, const char *noun, const Stats &st, int64_t *out_count, Stats *stats, bool *done)
{
    *done = true;
    *out_count = kept;
    if (stats) *stats = st;
    if ((!o.points && !o.col[0].dst && !o.col[1].dst && !o.col[2].dst) || kept == 0) return PCR_OK;
    if (o.capacity < (size_t)kept) return set_err(c, PCR_E_ARG, "capacity of %zu records is below the %lld %s", o.capacity, (long long)kept, noun);
    *done = false;
    return PCR_OK;
}

// The device twin of a host description for `batches` batches of 65 536 rows: the points through d_decode_stage, column i through
// d_col_stage[i], NULL where the host takes none. The name of the buffer there is no memory for, or NULL.
const char *stage_reserve(pcr_ctx *c, const KeptOut &o, int64_t batches, KeptOut &d)
{
    d = o;
    d.host = false;
    if (o.points) {
        if (!thin_grow((void **)&c->d_decode_stage, c->decode_stage_batches, batches, (size_t)PCR_POINTS_PER_BATCH * sizeof(pcr_point))) return "points";
        d.points = c->d_decode_stage;
    }
    for (int i = 0; i < 3; ++i) {
        if (!o.col[i].dst) continue;
        if (!thin_grow(&c->d_col_stage[i], c->col_stage_bytes[i], batches * PCR_POINTS_PER_BATCH * (int64_t)o.col[i].row_bytes, 1)) return o.col[i].name;
        d.col[i].dst = c->d_col_stage[i];
    }
    return nullptr;
}

// The first m rows of the stages d to rows [at, at + m) of the host destinations o. Synchronises.
int stage_copy(pcr_ctx *c, const KeptOut &o, const KeptOut &d, int64_t at, int64_t m)
{
    if (d.points) HIP_TRY(c, hipMemcpyAsync(static_cast<pcr_point *>(o.points) + at, d.points, (size_t)m * sizeof(pcr_point), hipMemcpyDeviceToHost, c->stream));
    for (int i = 0; i < 3; ++i) {
        const size_t row_bytes = o.col[i].row_bytes;
        if (d.col[i].dst)
            HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(o.col[i].dst) + (size_t)at * row_bytes, d.col[i].dst, (size_t)m * row_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

// A plan's rows to the destinations. The plan has n units (the batches of its range, or the batches it lists); rows(i0, i1) is the
// number of rows of units [i0, i1), asked for ascending pieces; emit(i0, i1, d) enqueues their writes to the device destinations
// d, each holding those rows. On the device one emit into o itself; to the host in pieces through the stages. stage_named: a
// stage that does not fit is reported by name. Synchronises.
template <class Rows, class Emit>
int kept_write(pcr_ctx *c, int64_t n, const KeptOut &o, Rows rows, Emit emit, bool stage_named = false)
{
    int rc;
    if (!o.host) {
        if ((rc = emit(0, n, o))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return PCR_OK;
    }
    // pieces of at most DECODE_STAGE_BATCHES batches: a batch writes at most 65 536 rows, so a piece fits the stages
    const int64_t piece = std::min<int64_t>(n, DECODE_STAGE_BATCHES);
    KeptOut d;
    if (const char *what = stage_reserve(c, o, piece, d))
        return stage_named ? set_err(c, PCR_E_NOMEM, "out of device memory for a staging buffer of %lld batches of %s", (long long)piece, what)
                           : set_err(c, PCR_E_NOMEM, "out of device memory for the staging buffers of %lld batches", (long long)piece);
    int64_t written = 0;
    for (int64_t i0 = 0; i0 < n; i0 += piece) {
        const int64_t i1 = std::min(n, i0 + piece), m = rows(i0, i1);
        if (m == 0) continue;
        if ((rc = emit(i0, i1, d)) || (rc = stage_copy(c, o, d, written, m))) return rc;
        written += m;
    }
    return PCR_OK;
}
} // namespace
} // extern "C++"

// ---- decode ------------------------------------------------------------------------------------
// Range check shared by pcr_decode_points / pcr_read_points: select_range, and a destination that holds every record of the range.
static int decode_range(pcr_ctx *c, int64_t first, int64_t count, const void *dst, size_t capacity, int64_t *n)
{
    const int rc = select_range(c, first, count, n);
    if (rc || *n == 0) return rc;
    if (!dst) return set_err(c, PCR_E_ARG, "the destination is NULL");
    if (reinterpret_cast<uintptr_t>(dst) % alignof(pcr_point) != 0) return set_err(c, PCR_E_ARG, "the destination is misaligned");
    if (capacity < (size_t)*n * PCR_POINTS_PER_BATCH)
        return set_err(c, PCR_E_ARG, "capacity of %zu points is below the %lld x %d of the range", capacity, (long long)*n, PCR_POINTS_PER_BATCH);
    return PCR_OK;
}

static int launch_decode(pcr_ctx *c, int64_t first, int64_t count, void *dev_points)
{
    int rc;
    // (as a frame: the provisional last batch of a stream that is still loading is walked here if no frame has done so)
    if (!c->async_upload && (rc = enqueue_transcode(c, true, c->stream))) return rc;
    if (!c->decode_lds_ready) {
        if ((rc = lds_allow(c, DEC_LDS_BYTES, &k_decode_points<LAYOUT_WORDS, false>, &k_decode_points<LAYOUT_WORDS, true>,
                            &k_decode_points<LAYOUT_POINT_WINDOWS, false>, &k_decode_points<LAYOUT_POINT_WINDOWS, true>))) return rc;
        c->decode_lds_ready = true;
    }
    const StreamView s = make_stream_view(c);
    for_layout_bc7(c, [&](auto layout, auto bc7) {
        hipLaunchKernelGGL((k_decode_points<layout.value, bc7.value>), dim3((unsigned)count), dim3(PCR_WORKGROUP_SIZE), DEC_LDS_BYTES, c->stream, s,
                           static_cast<uint4 *>(dev_points), (uint32_t)first);
    });
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_decode_points(pcr_ctx *c, int64_t first_batch, int64_t count, void *dev_points, size_t capacity_points)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = decode_range(c, first_batch, count, dev_points, capacity_points, &n);
    if (rc || n == 0) return rc;
    if (reinterpret_cast<uintptr_t>(dev_points) % 16 != 0) return set_err(c, PCR_E_ARG, "dev_points must be 16-byte aligned");
    return launch_decode(c, first_batch, n, dev_points);
}

int pcr_read_points(pcr_ctx *c, int64_t first_batch, int64_t count, pcr_point *host, size_t capacity_points)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = decode_range(c, first_batch, count, host, capacity_points, &n);
    if (rc || n == 0) return rc;
    // staged through a device buffer of bounded size, piece by piece (never 16 bytes x the whole stream on the device)
    const int64_t piece = std::min<int64_t>(n, DECODE_STAGE_BATCHES);
    if (!c->d_decode_stage || c->decode_stage_batches < piece) {
        dfree(c->d_decode_stage); c->decode_stage_batches = 0;
        if (hipMalloc((void **)&c->d_decode_stage, (size_t)piece * PCR_POINTS_PER_BATCH * sizeof(pcr_point)) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for a staging buffer of %lld batches of points", (long long)piece);
        c->decode_stage_batches = piece;
    }
    for (int64_t done = 0; done < n; done += piece) {
        const int64_t m = std::min(piece, n - done);
        if ((rc = launch_decode(c, first_batch + done, m, c->d_decode_stage))) return rc;
        HIP_TRY(c, hipMemcpyAsync(host + (size_t)done * PCR_POINTS_PER_BATCH, c->d_decode_stage, (size_t)m * PCR_POINTS_PER_BATCH * sizeof(pcr_point),
                                  hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return PCR_OK;
}

// ---- box selection -----------------------------------------------------------------------------
// c->h_point_bounds holds the exact boxes of batches [first, first + n) on return: one k_point_bounds launch over the span of the
// batches not cached yet, read back. Synchronises if it launches.
static int ensure_point_bounds(pcr_ctx *c, int64_t first, int64_t n)
{
    int rc;
    if (!c->async_upload && (rc = enqueue_transcode(c, true, c->stream))) return rc;
    const size_t nB = (size_t)c->hdr.num_batches;
    if (c->h_point_bounds_ok.size() != nB) { c->h_point_bounds.assign(nB * 6, 0); c->h_point_bounds_ok.assign(nB, 0); }
    for (size_t b = (size_t)std::max<int64_t>(c->transcoded, 0); b < nB; ++b) c->h_point_bounds_ok[b] = 0;     // not final (yet, or any more: pcr_upload_tail)
    int64_t lo = -1, hi = -1;
    for (int64_t b = first; b < first + n; ++b)
        if (!c->h_point_bounds_ok[(size_t)b]) { if (lo < 0) lo = b; hi = b + 1; }
    if (lo < 0) return PCR_OK;
    if (!c->d_point_bounds) HIP_TRY(c, hipMalloc((void **)&c->d_point_bounds, nB * 6 * sizeof(int32_t)));
    const StreamView s = make_stream_view(c);
    for_layout(c, [&](auto layout) {
        hipLaunchKernelGGL((k_point_bounds<layout.value>), dim3((unsigned)(hi - lo)), dim3(PCR_WORKGROUP_SIZE), 0, c->stream, s, c->d_point_bounds, (uint32_t)lo);
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_point_bounds.data() + lo * 6, c->d_point_bounds + lo * 6, (size_t)(hi - lo) * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t b = lo; b < hi && b < c->transcoded; ++b) c->h_point_bounds_ok[(size_t)b] = 1;
    return PCR_OK;
}

int pcr_batch_point_bounds(pcr_ctx *c, int64_t first_batch, int64_t count, int32_t *host_bounds)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = select_range(c, first_batch, count, &n);
    if (rc || n == 0) return rc;
    if (!host_bounds) return set_err(c, PCR_E_ARG, "the destination is NULL");
    if ((rc = ensure_point_bounds(c, first_batch, n))) return rc;
    std::memcpy(host_bounds, c->h_point_bounds.data() + first_batch * 6, (size_t)n * 6 * sizeof(int32_t));
    return PCR_OK;
}

// ---- the host path of the selection calls --------------------------------------------------------
// Six predicates (box, polygon, slabs, height, screen, visible), each in a device form pcr_select_X and a host form pcr_read_X that
// are one function X_call behind two descriptions of the outputs (KeptOut), on the kept-rows calls' begin, finish and write. Box,
// polygon and slabs class the batches of a range by their exact boxes (select_plan, select_write); height, screen and visible list
// the batches they decode (listed_write).
extern "C++" {                          // (templates among them)
namespace {
enum : int8_t { SEL_OUTSIDE = 0, SEL_INSIDE = 1, SEL_STRADDLING = 2 };
static_assert((int)POLY_OUTSIDE == SEL_OUTSIDE && (int)POLY_INSIDE == SEL_INSIDE && (int)POLY_STRADDLING == SEL_STRADDLING, "poly_plan_batch returns a SEL_ class");
static_assert((int)SLABS_OUTSIDE == SEL_OUTSIDE && (int)SLABS_INSIDE == SEL_INSIDE && (int)SLABS_STRADDLING == SEL_STRADDLING, "slabs_plan_batch returns a SEL_ class");

// What a selection over batches [first, first + n) has to write: the class of every batch, its record count, and for the
// straddling ones (slot = position among them; their per-chain counts sit in c->sel.counts) the batch index.
struct SelectPlan {
    std::vector<int8_t> cls;
    std::vector<int64_t> cnt;
    std::vector<uint32_t> strad;        // batch indices of the straddling batches, ascending
    std::vector<int64_t> offsets;       // staging of the write kernel's offsets (alive until the stream has been synchronised)
};

// rows(i0, i1) of kept_write for a plan that holds the rows of every unit
auto rows_of(const std::vector<int64_t> &cnt)
{
    return [&cnt](int64_t i0, int64_t i1) { int64_t m = 0; for (int64_t i = i0; i < i1; ++i) m += cnt[(size_t)i]; return m; };
}

// The plan of a box-classified selection: classify(b, bb) classes batch b from its exact box bb (host) and notes what the
// predicate keeps per straddling batch; count(nS) uploads that and enqueues the predicate's count kernel over the nS straddling
// batches into c->sel.counts / c->sel.totals. st: the call's statistics, whose first four fields are pcr_select_stats'.
// nothing: the predicate selects no point at all. Synchronises.
template <class Stats, class Classify, class Count>
int select_plan(pcr_ctx *c, int64_t first, int64_t n, bool nothing, SelectPlan &p, Stats &st, Classify classify, Count count)
{
    p.cls.assign((size_t)n, SEL_OUTSIDE); p.cnt.assign((size_t)n, 0); p.strad.clear();
    st = Stats{};
    st.batches_outside = n;
    if (n == 0 || nothing) return PCR_OK;
    int rc;
    if ((rc = ensure_point_bounds(c, first, n))) return rc;
    for (int64_t i = 0; i < n; ++i) {
        const int cls = classify((uint32_t)(first + i), c->h_point_bounds.data() + (first + i) * 6);
        if (cls == SEL_OUTSIDE) continue;
        --st.batches_outside;
        p.cls[(size_t)i] = (int8_t)cls;
        if (cls == SEL_INSIDE) { p.cnt[(size_t)i] = PCR_POINTS_PER_BATCH; ++st.batches_inside; }
        else { p.strad.push_back((uint32_t)(first + i)); ++st.batches_straddling; }
    }
    const int64_t nS = (int64_t)p.strad.size();
    if (nS) {
        if ((rc = scratch_reserve(c, c->sel, nS, "straddling batches (their counts)")) || (rc = count(nS))) return rc;
        HIP_TRY(c, hipGetLastError());
        std::vector<uint32_t> totals((size_t)nS);
        HIP_TRY(c, hipMemcpyAsync(totals.data(), c->sel.totals, (size_t)nS * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int64_t k = 0; k < nS; ++k) p.cnt[(size_t)(p.strad[(size_t)k] - first)] = totals[(size_t)k];
    }
    for (int64_t i = 0; i < n; ++i) st.points_selected += p.cnt[(size_t)i];
    return PCR_OK;
}

// Enqueue the writes of batches [i0, i1) of the plan's range to `out` (device, holds their records): runs of inside batches
// through k_decode_points, the straddling ones through one launch of write(s0, grid, out): the kernel that writes the straddling
// batches [s0, s0 + grid.x) of the plan from c->sel.offsets + s0. The caller synchronises.
template <class Write>
int select_emit(pcr_ctx *c, int64_t first, int64_t i0, int64_t i1, SelectPlan &p, uint4 *out, Write &&write)
{
    int rc;
    const size_t s0 = (size_t)(std::lower_bound(p.strad.begin(), p.strad.end(), (uint32_t)(first + i0)) - p.strad.begin());
    p.offsets.clear();
    int64_t off = 0;
    for (int64_t i = i0; i < i1; ) {
        if (p.cls[(size_t)i] == SEL_INSIDE) {
            int64_t e = i;
            while (e < i1 && p.cls[(size_t)e] == SEL_INSIDE) ++e;
            if ((rc = launch_decode(c, first + i, e - i, out + off))) return rc;
            off += (e - i) * PCR_POINTS_PER_BATCH;
            i = e;
            continue;
        }
        if (p.cls[(size_t)i] == SEL_STRADDLING) { p.offsets.push_back(off); off += p.cnt[(size_t)i]; }
        ++i;
    }
    const size_t nS = p.offsets.size();
    if (nS) {
        HIP_TRY(c, hipMemcpyAsync(c->sel.offsets + s0, p.offsets.data(), nS * 8, hipMemcpyHostToDevice, c->stream));
        write(s0, dim3((unsigned)nS), out);
        HIP_TRY(c, hipGetLastError());
    }
    return PCR_OK;
}

// kept_write for a box-classified plan: the selected records to o.points (the range in pieces of whole batches on the host form)
template <class Write>
int select_write(pcr_ctx *c, int64_t first, int64_t n, SelectPlan &p, const KeptOut &o, Write write)
{
    return kept_write(c, n, o, rows_of(p.cnt), [&](int64_t i0, int64_t i1, const KeptOut &d) {
        return select_emit(c, first, i0, i1, p, static_cast<uint4 *>(d.points), write);
    }, true);
}

// kept_write for a plan that lists the batches it decodes, cnt[k] records from the k-th: launch(k0, grid, d) starts the call's
// write kernel over the listed batches [k0, k0 + grid.x), which finds the first output record of each at d_offsets + k0
template <class Launch>
int listed_write(pcr_ctx *c, const std::vector<int64_t> &cnt, std::vector<int64_t> &offsets, int64_t *d_offsets, const KeptOut &o, Launch launch)
{
    return kept_write(c, (int64_t)cnt.size(), o, rows_of(cnt), [&](int64_t k0, int64_t k1, const KeptOut &d) {
        offsets.clear();                                                        // (alive until the stream has been synchronised)
        int64_t off = 0;
        for (int64_t k = k0; k < k1; ++k) { offsets.push_back(off); off += cnt[(size_t)k]; }
        if (off == 0) return (int)PCR_OK;
        HIP_TRY(c, hipMemcpyAsync(d_offsets + k0, offsets.data(), (size_t)(k1 - k0) * 8, hipMemcpyHostToDevice, c->stream));
        launch(k0, dim3((unsigned)(k1 - k0)), d);
        HIP_TRY(c, hipGetLastError());
        return (int)PCR_OK;
    }, true);
}

bool box_empty(const pcr_box &q) { return q.min[0] > q.max[0] || q.min[1] > q.max[1] || q.min[2] > q.max[2]; }

// pcr_select_box / pcr_read_box
int box_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_box *box, const KeptOut &o, int64_t *out_count, pcr_select_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SelectPlan p;
    pcr_select_stats st;
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n);
    if (rc) return rc;
    if (!box) return set_err(c, PCR_E_ARG, "the box is NULL");
    const pcr_box q = *box;
    const dim3 block(PCR_WORKGROUP_SIZE);
    rc = select_plan(c, first, n, box_empty(q), p, st, [&](uint32_t, const int32_t *bb) {
        bool disjoint = false, within = true;
        for (int k = 0; k < 3; ++k) {
            disjoint = disjoint || bb[3 + k] < q.min[k] || bb[k] > q.max[k];
            within = within && bb[k] >= q.min[k] && bb[3 + k] <= q.max[k];
        }
        return disjoint ? SEL_OUTSIDE : within ? SEL_INSIDE : SEL_STRADDLING;
    }, [&](int64_t nS) {
        HIP_TRY(c, hipMemcpyAsync(c->sel.list, p.strad.data(), (size_t)nS * 4, hipMemcpyHostToDevice, c->stream));
        for_layout(c, [&](auto layout) {
            hipLaunchKernelGGL((k_select_count<layout.value>), dim3((unsigned)nS), block, 0, c->stream, make_stream_view(c), c->sel.list, q, c->sel.counts, c->sel.totals);
        });
        return (int)PCR_OK;
    });
    if (rc || (rc = kept_finish(c, o, st.points_selected, "selected", st, out_count, stats, &done)) || done) return rc;
    return select_write(c, first, n, p, o, [&](size_t s0, dim3 grid, uint4 *out) {
        for_layout_bc7(c, [&](auto layout, auto bc7) {
            hipLaunchKernelGGL((k_select_write<layout.value, bc7.value>), grid, block, 0, c->stream, make_stream_view(c), c->sel.list + s0, q,
                               c->sel.counts + s0 * PCR_WORKGROUP_SIZE, c->sel.offsets + s0, out);
        });
    });
}
} // namespace
} // extern "C++"

int pcr_select_box(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_box *box, void *dev_points, size_t capacity_points,
                   int64_t *out_count, pcr_select_stats *stats)
{
    return box_call(c, first_batch, count, box, KeptOut{false, dev_points, capacity_points, {}}, out_count, stats);
}

int pcr_read_box(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_box *box, pcr_point *host, size_t capacity_points,
                 int64_t *out_count, pcr_select_stats *stats)
{
    return box_call(c, first_batch, count, box, KeptOut{true, host, capacity_points, {}}, out_count, stats);
}

// ---- polygon selection -------------------------------------------------------------------------
extern "C++" {
namespace {
constexpr size_t POLY_MAX_LDS_BYTES = POLY_TABLE_BYTES + (size_t)PCR_POLY_MAX_VERTICES * sizeof(PolyEdge);

// pcr_select_polygon / pcr_read_polygon: what the polygon adds to select_plan is the straddling batches with their slices of the
// edge array (both alive until the stream has been synchronised)
int polygon_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_polygon *poly, const KeptOut &o, int64_t *out_count, pcr_polygon_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SelectPlan p;
    PolyShape shape;
    std::vector<PolyBatch> batches;
    std::vector<PolyEdge> edges;
    PolyArgs args{};
    size_t lds = 0;                     // dynamic LDS of the k_polygon_* launches
    pcr_polygon_stats st;
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n);
    if (rc) return rc;
    if (const char *why = poly_shape(poly, &shape)) return set_err(c, PCR_E_ARG, "%s", why);
    const dim3 block(PCR_WORKGROUP_SIZE);
    rc = select_plan(c, first, n, shape.z_min > shape.z_max, p, st, [&](uint32_t b, const int32_t *bb) {
        const size_t e0 = edges.size();
        uint32_t base = 0;
        const int cls = poly_plan_batch(shape, bb, edges, &base);
        if (cls != POLY_STRADDLING) return cls;
        const size_t ne = edges.size() - e0;
        batches.push_back(PolyBatch{b, (uint32_t)e0, (uint32_t)ne, base});
        st.edges_listed += (int64_t)ne;
        st.edges_max = std::max(st.edges_max, (int64_t)ne);
        return cls;
    }, [&](int64_t nS) {
        const int64_t nE = (int64_t)edges.size();
        int rc;
        if ((rc = reserve(c, c->d_poly_batches, c->poly_capacity, nS, "straddling batches")) ||
            (rc = reserve(c, c->d_poly_edges, c->poly_edge_capacity, std::max<int64_t>(nE, 1), "polygon edges"))) return rc;
        if (!c->poly_lds_ready) {
            if ((rc = lds_allow(c, POLY_MAX_LDS_BYTES, &k_polygon_count<LAYOUT_WORDS>, &k_polygon_count<LAYOUT_POINT_WINDOWS>,
                                &k_polygon_write<LAYOUT_WORDS, false>, &k_polygon_write<LAYOUT_WORDS, true>,
                                &k_polygon_write<LAYOUT_POINT_WINDOWS, false>, &k_polygon_write<LAYOUT_POINT_WINDOWS, true>))) return rc;
            c->poly_lds_ready = true;
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_poly_batches, batches.data(), (size_t)nS * sizeof(PolyBatch), hipMemcpyHostToDevice, c->stream));
        if (nE) HIP_TRY(c, hipMemcpyAsync(c->d_poly_edges, edges.data(), (size_t)nE * sizeof(PolyEdge), hipMemcpyHostToDevice, c->stream));
        args = PolyArgs{shape.x0, shape.y0, shape.x1, shape.y1, shape.z_min, shape.z_max, shape.invert ? 1u : 0u, (uint32_t)st.edges_max, c->d_poly_batches,
                        c->d_poly_edges};
        lds = POLY_TABLE_BYTES + (size_t)st.edges_max * sizeof(PolyEdge);
        for_layout(c, [&](auto layout) {
            hipLaunchKernelGGL((k_polygon_count<layout.value>), dim3((unsigned)nS), block, lds, c->stream, make_stream_view(c), args, c->sel.counts, c->sel.totals);
        });
        return (int)PCR_OK;
    });
    if (rc || (rc = kept_finish(c, o, st.points_selected, "selected", st, out_count, stats, &done)) || done) return rc;
    return select_write(c, first, n, p, o, [&](size_t s0, dim3 grid, uint4 *out) {
        PolyArgs a = args;
        a.batches += s0;
        for_layout_bc7(c, [&](auto layout, auto bc7) {
            hipLaunchKernelGGL((k_polygon_write<layout.value, bc7.value>), grid, block, lds, c->stream, make_stream_view(c), a,
                               c->sel.counts + s0 * PCR_WORKGROUP_SIZE, c->sel.offsets + s0, out);
        });
    });
}
} // namespace
} // extern "C++"

int pcr_select_polygon(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_polygon *poly, void *dev_points, size_t capacity_points,
                       int64_t *out_count, pcr_polygon_stats *stats)
{
    return polygon_call(c, first_batch, count, poly, KeptOut{false, dev_points, capacity_points, {}}, out_count, stats);
}

int pcr_read_polygon(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_polygon *poly, pcr_point *host, size_t capacity_points,
                     int64_t *out_count, pcr_polygon_stats *stats)
{
    return polygon_call(c, first_batch, count, poly, KeptOut{true, host, capacity_points, {}}, out_count, stats);
}

// ---- slabs: pcr_select_slabs / pcr_read_slabs / pcr_plane_support ------------------------------------
extern "C++" {
namespace {
constexpr size_t SLAB_MAX_LDS_BYTES = SLAB_TABLE_BYTES + (size_t)PCR_SLAB_MAX_SELECT * sizeof(pcr_slab);
constexpr size_t PLANE_MAX_LDS_BYTES = SLAB_TABLE_BYTES + (size_t)PCR_SLAB_MAX_EXCLUDE * sizeof(pcr_slab) +
                                       (size_t)PCR_PLANE_MAX_HYPOTHESES * (sizeof(pcr_slab) + LWC_WAVES * sizeof(uint32_t));
static_assert(sizeof(pcr_slab) == 32 && sizeof(pcr_plane_stats) == 64 && sizeof(pcr_slab_stats) == 48, "the slab structs of pcr_types.h");

int slab_lds_allow(pcr_ctx *c)
{
    if (c->slab_lds_ready) return PCR_OK;
    int rc;
    if ((rc = lds_allow(c, SLAB_MAX_LDS_BYTES, &k_slab_count<LAYOUT_WORDS>, &k_slab_count<LAYOUT_POINT_WINDOWS>, &k_slab_write<LAYOUT_WORDS, false>,
                        &k_slab_write<LAYOUT_WORDS, true>, &k_slab_write<LAYOUT_POINT_WINDOWS, false>, &k_slab_write<LAYOUT_POINT_WINDOWS, true>)) ||
        (rc = lds_allow(c, PLANE_MAX_LDS_BYTES, &k_plane_support<LAYOUT_WORDS>, &k_plane_support<LAYOUT_POINT_WINDOWS>))) return rc;
    c->slab_lds_ready = true;
    return PCR_OK;
}

// The checks on a list of slabs shared by the three entry points.
int slab_list_check(pcr_ctx *c, const pcr_slab *slabs, int n, int n_min, int n_max, const char *what)
{
    if (n < n_min || n > n_max) return set_err(c, PCR_E_ARG, "%d %s: %d to %d are taken", n, what, n_min, n_max);
    if (n > 0 && !slabs) return set_err(c, PCR_E_ARG, "the list of %s is NULL", what);
    for (int k = 0; k < n; ++k)
        if (const char *why = slab_check(slabs[k])) return set_err(c, PCR_E_ARG, "%s (entry %d of the %s)", why, k, what);
    return PCR_OK;
}

const pcr_box FULL_BOX = {{INT32_MIN, INT32_MIN, INT32_MIN}, {INT32_MAX, INT32_MAX, INT32_MAX}};

// pcr_select_slabs / pcr_read_slabs: what the slabs add to select_plan is the straddling batches with their slices of the slab
// array (both alive until the stream has been synchronised)
int slabs_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_slab *slabs, int num_slabs, const pcr_box *clip, uint32_t flags, const KeptOut &o,
               int64_t *out_count, pcr_slab_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SelectPlan p;
    std::vector<SlabBatch> batches;
    std::vector<pcr_slab> listed;
    SlabArgs args{};
    size_t lds = 0;                     // dynamic LDS of the k_slab_* launches
    pcr_slab_stats st;
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n);
    if (rc || (rc = slab_list_check(c, slabs, num_slabs, 1, PCR_SLAB_MAX_SELECT, "slabs"))) return rc;
    if (flags & ~PCR_SLAB_INVERT) return set_err(c, PCR_E_ARG, "unknown flag bits 0x%x", flags);
    const dim3 block(PCR_WORKGROUP_SIZE);
    rc = select_plan(c, first, n, clip && plane_box_empty(*clip), p, st, [&](uint32_t b, const int32_t *bb) {
        const size_t e0 = listed.size();
        uint32_t inv = 0;
        const int cls = slabs_plan_batch(slabs, num_slabs, clip, flags & PCR_SLAB_INVERT, bb, listed, &inv);
        if (cls != SLABS_STRADDLING) return cls;
        const size_t ne = listed.size() - e0;
        batches.push_back(SlabBatch{b, (uint32_t)e0, (uint32_t)ne, inv});
        st.slabs_listed += (int64_t)ne;
        st.slabs_max = std::max(st.slabs_max, (int64_t)ne);
        return cls;
    }, [&](int64_t nS) {
        const int64_t nE = (int64_t)listed.size();
        int rc;
        if ((rc = reserve(c, c->d_slab_batches, c->slab_capacity, nS, "straddling batches")) ||
            (rc = reserve(c, c->d_slab_entries, c->slab_entry_capacity, std::max<int64_t>(nE, 1), "slabs")) || (rc = slab_lds_allow(c))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_slab_batches, batches.data(), (size_t)nS * sizeof(SlabBatch), hipMemcpyHostToDevice, c->stream));
        if (nE) HIP_TRY(c, hipMemcpyAsync(c->d_slab_entries, listed.data(), (size_t)nE * sizeof(pcr_slab), hipMemcpyHostToDevice, c->stream));
        args = SlabArgs{clip ? *clip : FULL_BOX, (uint32_t)st.slabs_max, c->d_slab_batches, c->d_slab_entries};
        lds = SLAB_TABLE_BYTES + (size_t)st.slabs_max * sizeof(pcr_slab);
        for_layout(c, [&](auto layout) {
            hipLaunchKernelGGL((k_slab_count<layout.value>), dim3((unsigned)nS), block, lds, c->stream, make_stream_view(c), args, c->sel.counts, c->sel.totals);
        });
        return (int)PCR_OK;
    });
    if (rc || (rc = kept_finish(c, o, st.points_selected, "selected", st, out_count, stats, &done)) || done) return rc;
    return select_write(c, first, n, p, o, [&](size_t s0, dim3 grid, uint4 *out) {
        SlabArgs a = args;
        a.batches += s0;
        for_layout_bc7(c, [&](auto layout, auto bc7) {
            hipLaunchKernelGGL((k_slab_write<layout.value, bc7.value>), grid, block, lds, c->stream, make_stream_view(c), a,
                               c->sel.counts + s0 * PCR_WORKGROUP_SIZE, c->sel.offsets + s0, out);
        });
    });
}
} // namespace
} // extern "C++"

int pcr_select_slabs(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_slab *slabs, int num_slabs, const pcr_box *clip, uint32_t flags,
                     void *dev_points, size_t capacity_points, int64_t *out_count, pcr_slab_stats *stats)
{
    return slabs_call(c, first_batch, count, slabs, num_slabs, clip, flags, KeptOut{false, dev_points, capacity_points, {}}, out_count, stats);
}

int pcr_read_slabs(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_slab *slabs, int num_slabs, const pcr_box *clip, uint32_t flags,
                   pcr_point *host, size_t capacity_points, int64_t *out_count, pcr_slab_stats *stats)
{
    return slabs_call(c, first_batch, count, slabs, num_slabs, clip, flags, KeptOut{true, host, capacity_points, {}}, out_count, stats);
}

int pcr_plane_support(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_slab *hyp, int num_hyp, const pcr_box *clip, const pcr_slab *exclude,
                      int num_exclude, int64_t *host_counts, pcr_plane_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = select_range(c, first_batch, count, &n);
    if (rc) return rc;
    if (!host_counts) return set_err(c, PCR_E_ARG, "host_counts is NULL");
    if ((rc = slab_list_check(c, hyp, num_hyp, 1, PCR_PLANE_MAX_HYPOTHESES, "hypotheses"))) return rc;
    if (!hyp) return set_err(c, PCR_E_ARG, "the list of hypotheses is NULL");
    if ((rc = slab_list_check(c, exclude, num_exclude, 0, PCR_SLAB_MAX_EXCLUDE, "exclusions"))) return rc;
    std::fill(host_counts, host_counts + num_hyp, (int64_t)0);
    pcr_plane_stats st{};
    st.batches_skipped = n;
    if (stats) *stats = st;
    if (n == 0 || (clip && plane_box_empty(*clip))) return PCR_OK;
    if ((rc = ensure_point_bounds(c, first_batch, n))) return rc;

    // the plan: per decoded batch its slices and, for a batch that is not open, the hypotheses that take its candidate count
    std::vector<PlaneBatch> batches;
    std::vector<pcr_slab> excl, cut;
    std::vector<int32_t> all, later;                        // `later`: per decoded batch that is not open: count, then the indices
    for (int64_t i = 0; i < n; ++i) {
        const size_t e0 = excl.size(), c0 = cut.size();
        bool open = false;
        all.clear();
        const int cls = plane_plan_batch(hyp, num_hyp, clip, exclude, num_exclude, c->h_point_bounds.data() + (first_batch + i) * 6, excl, cut, all, &open);
        if (cls == PLANE_SKIPPED) continue;
        --st.batches_skipped;
        if (open) for (int32_t j : all) host_counts[j] += PCR_POINTS_PER_BATCH;
        if (cls == PLANE_WHOLE) { ++st.batches_whole; continue; }
        ++st.batches_decoded;
        const size_t ne = excl.size() - e0, nc = cut.size() - c0;
        batches.push_back(PlaneBatch{(uint32_t)(first_batch + i), (uint32_t)e0, (uint32_t)ne, (uint32_t)c0, (uint32_t)nc});
        st.hypotheses_listed += (int64_t)nc;
        st.hypotheses_max = std::max(st.hypotheses_max, (int64_t)nc);
        st.exclusions_listed += (int64_t)ne;
        later.push_back(open ? 0 : (int32_t)all.size());
        if (!open) later.insert(later.end(), all.begin(), all.end());
    }
    const int64_t nD = (int64_t)batches.size();
    if (nD) {
        size_t excl_max = 0;
        for (const PlaneBatch &b : batches) excl_max = std::max(excl_max, (size_t)b.excl_count);
        const int64_t nX = (int64_t)excl.size(), nH = (int64_t)cut.size();
        if ((rc = reserve(c, c->d_plane_batches, c->plane_capacity, nD, "decoded batches"))) return rc;
        if ((rc = reserve(c, c->d_plane_candidates, c->plane_cand_capacity, nD, "candidate counts"))) return rc;
        if ((rc = reserve(c, c->d_plane_entries, c->plane_entry_capacity, std::max<int64_t>(nX + nH, 1), "slabs"))) return rc;
        if (!c->d_plane_counts && hipMalloc((void **)&c->d_plane_counts, PCR_PLANE_MAX_HYPOTHESES * sizeof(unsigned long long)) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for the hypothesis counters");
        if ((rc = slab_lds_allow(c))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->d_plane_counts, 0, (size_t)num_hyp * sizeof(unsigned long long), c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_plane_batches, batches.data(), (size_t)nD * sizeof(PlaneBatch), hipMemcpyHostToDevice, c->stream));
        if (nX) HIP_TRY(c, hipMemcpyAsync(c->d_plane_entries, excl.data(), (size_t)nX * sizeof(pcr_slab), hipMemcpyHostToDevice, c->stream));
        if (nH) HIP_TRY(c, hipMemcpyAsync(c->d_plane_entries + nX, cut.data(), (size_t)nH * sizeof(pcr_slab), hipMemcpyHostToDevice, c->stream));
        const PlaneArgs a{clip ? *clip : FULL_BOX, (uint32_t)excl_max, (uint32_t)st.hypotheses_max, c->d_plane_batches, c->d_plane_entries,
                          c->d_plane_entries + nX, c->d_plane_counts, c->d_plane_candidates};
        const size_t lds = SLAB_TABLE_BYTES + excl_max * sizeof(pcr_slab) + (size_t)st.hypotheses_max * (sizeof(pcr_slab) + LWC_WAVES * sizeof(uint32_t));
        const StreamView s = make_stream_view(c);
        const dim3 grid((unsigned)nD), block(PCR_WORKGROUP_SIZE);
        if (select_reads_windows(c)) hipLaunchKernelGGL((k_plane_support<LAYOUT_POINT_WINDOWS>), grid, block, lds, c->stream, s, a);
        else                         hipLaunchKernelGGL((k_plane_support<LAYOUT_WORDS>), grid, block, lds, c->stream, s, a);
        HIP_TRY(c, hipGetLastError());
        std::vector<unsigned long long> counts((size_t)num_hyp);
        std::vector<uint32_t> cand((size_t)nD);
        HIP_TRY(c, hipMemcpyAsync(counts.data(), c->d_plane_counts, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(cand.data(), c->d_plane_candidates, cand.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int j = 0; j < num_hyp; ++j) host_counts[j] += (int64_t)counts[(size_t)j];
        size_t at = 0;
        for (int64_t k = 0; k < nD; ++k) {
            st.candidates_decoded += cand[(size_t)k];
            const int32_t m = later[at++];
            for (int32_t q = 0; q < m; ++q) host_counts[later[at++]] += cand[(size_t)k];
        }
    }
    if (stats) *stats = st;
    return PCR_OK;
}

// ---- top-down grid -----------------------------------------------------------------------------
namespace {
constexpr size_t GRID_MAX_LDS_BYTES = GRID_TABLE_BYTES + (size_t)PCR_GRID_WINDOW_CELLS * (8 + 8 + 4);

// The checks on a grid and its planes shared by the four entry points (dev: the planes are device pointers with an alignment to keep).
int grid_check(pcr_ctx *c, const pcr_grid *g, const void *top, const void *bottom, const void *count)
{
    if (!g) return set_err(c, PCR_E_ARG, "the grid is NULL");
    if (g->cell < 1) return set_err(c, PCR_E_ARG, "grid cell of %d: the edge length is at least 1", g->cell);
    if (g->width < 1 || g->height < 1) return set_err(c, PCR_E_ARG, "grid of %d x %d cells: width and height are at least 1", g->width, g->height);
    if ((int64_t)g->width * g->height > PCR_GRID_MAX_CELLS)
        return set_err(c, PCR_E_ARG, "grid of %d x %d cells: more than the %d of PCR_GRID_MAX_CELLS", g->width, g->height, PCR_GRID_MAX_CELLS);
    if (g->reserved != 0) return set_err(c, PCR_E_ARG, "pcr_grid::reserved is %d, not 0", g->reserved);
    if (reinterpret_cast<uintptr_t>(top) % 8 != 0 || reinterpret_cast<uintptr_t>(bottom) % 8 != 0)
        return set_err(c, PCR_E_ARG, "the top / bottom plane is misaligned (8 bytes)");
    if (reinterpret_cast<uintptr_t>(count) % 4 != 0) return set_err(c, PCR_E_ARG, "the count plane is misaligned (4 bytes)");
    return PCR_OK;
}

void grid_launch(pcr_ctx *c, bool windowed, bool coloured, unsigned nblocks, size_t lds, const GridEntry *list, const GridArgs &a)
{
    const StreamView s = make_stream_view(c);
    const dim3 grid(nblocks), block(PCR_WORKGROUP_SIZE);
    for_layout_colour(c, coloured, [&](auto layout, auto colour) {
        if (windowed) hipLaunchKernelGGL((k_grid<layout.value, colour.value, true>), grid, block, lds, c->stream, s, list, a);
        else          hipLaunchKernelGGL((k_grid<layout.value, colour.value, false>), grid, block, lds, c->stream, s, list, a);
    });
}

// The batches [first, first + n) by their exact box against q (grid and clip intersected, not empty): those the box does not miss
// into `list` with the rectangle of cells they can reach, the windowed ones (at most PCR_GRID_WINDOW_CELLS cells, and no
// PCR_GRID_NO_WINDOW) first -- nW of them, the largest window win_cells -- then the direct ones. outside starts as n.
int grid_classify(pcr_ctx *c, int64_t first, int64_t n, const pcr_grid &g, const pcr_box &q, uint32_t flags, std::vector<GridEntry> &list, size_t &nW,
                  uint32_t &win_cells, int64_t &outside, int64_t &windowed, int64_t &direct)
{
    int rc;
    if ((rc = ensure_point_bounds(c, first, n))) return rc;
    const int64_t org[2] = {g.origin_x, g.origin_y};
    std::vector<GridEntry> dir;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *bb = c->h_point_bounds.data() + (first + i) * 6;
        bool disjoint = false;
        for (int k = 0; k < 3; ++k) disjoint = disjoint || bb[3 + k] < q.min[k] || bb[k] > q.max[k];
        if (disjoint) continue;
        --outside;
        uint32_t c0[2], c1[2];                              // the cells the batch's box reaches inside grid and clip
        for (int k = 0; k < 2; ++k) {
            c0[k] = (uint32_t)(((int64_t)std::max(bb[k], q.min[k]) - org[k]) / g.cell);
            c1[k] = (uint32_t)(((int64_t)std::min(bb[3 + k], q.max[k]) - org[k]) / g.cell);
        }
        const GridEntry e{(uint32_t)(first + i), c0[0], c0[1], c1[0] - c0[0] + 1, c1[1] - c0[1] + 1};
        const int64_t cells = (int64_t)e.ww * e.wh;
        if (cells <= PCR_GRID_WINDOW_CELLS && !(flags & PCR_GRID_NO_WINDOW)) { list.push_back(e); win_cells = std::max(win_cells, (uint32_t)cells); ++windowed; }
        else { dir.push_back(e); ++direct; }
    }
    nW = list.size();
    list.insert(list.end(), dir.begin(), dir.end());
    return PCR_OK;
}

// `list` (not empty) into d_grid_list (a call that repeats the last one's list finds it on the device)
int grid_list_upload(pcr_ctx *c, const std::vector<GridEntry> &list)
{
    if (c->grid_capacity < (int64_t)list.size()) {
        dfree(c->d_grid_list); c->grid_capacity = 0; c->h_grid_list.clear();
        const int64_t cap = std::max<int64_t>((int64_t)list.size(), c->hdr.num_batches);
        if (hipMalloc((void **)&c->d_grid_list, (size_t)cap * sizeof(GridEntry)) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for a list of %lld batches", (long long)cap);
        c->grid_capacity = cap;
    }
    if (list.size() != c->h_grid_list.size() || std::memcmp(list.data(), c->h_grid_list.data(), list.size() * sizeof(GridEntry)) != 0) {
        c->h_grid_list.clear();
        HIP_TRY(c, hipMemcpyAsync(c->d_grid_list, list.data(), list.size() * sizeof(GridEntry), hipMemcpyHostToDevice, c->stream));
        c->h_grid_list = list;
    }
    return PCR_OK;
}

// pcr_grid_accumulate behind its range check: n batches from `first`, the planes checked.
int grid_accumulate(pcr_ctx *c, int64_t first, int64_t n, const pcr_grid &g, const pcr_box *clip, void *top, void *bottom, void *count,
                    uint32_t flags, pcr_grid_stats *stats)
{
    pcr_grid_stats st{0, 0, 0};
    if (!top && !bottom && !count) { if (stats) *stats = st; return PCR_OK; }
    st.batches_outside = n;
    // grid and clip intersected: a point inside this box has a cell of the grid (the far edges in 64 bits: origin + cell * width
    // may lie beyond every int32 coordinate)
    GridArgs a{};
    const int64_t org[2] = {g.origin_x, g.origin_y}, ext[2] = {g.width, g.height};
    bool empty = false;
    for (int k = 0; k < 3; ++k) {
        int64_t lo = clip ? clip->min[k] : INT32_MIN, hi = clip ? clip->max[k] : INT32_MAX;
        if (k < 2) { lo = std::max(lo, org[k]); hi = std::min(hi, org[k] + (int64_t)g.cell * ext[k] - 1); }
        empty = empty || lo > hi;
        a.q.min[k] = (int32_t)lo; a.q.max[k] = (int32_t)hi;
    }
    if (n == 0 || empty) { if (stats) *stats = st; return PCR_OK; }
    int rc;
    std::vector<GridEntry> win;
    size_t nW = 0;
    uint32_t win_cells = 0;
    if ((rc = grid_classify(c, first, n, g, a.q, flags, win, nW, win_cells, st.batches_outside, st.batches_windowed, st.batches_direct))) return rc;
    if (stats) *stats = st;
    const size_t nD = win.size() - nW;
    if (nW + nD == 0) return PCR_OK;
    if ((rc = grid_list_upload(c, win))) return rc;
    if (!c->grid_lds_ready) {
        if ((rc = lds_allow(c, GRID_MAX_LDS_BYTES, &k_grid<LAYOUT_WORDS, SEL_NO_COLOUR, true>, &k_grid<LAYOUT_WORDS, SEL_BC1, true>,
                            &k_grid<LAYOUT_WORDS, SEL_BC7, true>, &k_grid<LAYOUT_POINT_WINDOWS, SEL_NO_COLOUR, true>,
                            &k_grid<LAYOUT_POINT_WINDOWS, SEL_BC1, true>, &k_grid<LAYOUT_POINT_WINDOWS, SEL_BC7, true>))) return rc;
        c->grid_lds_ready = true;
    }
    a.ox = g.origin_x; a.oy = g.origin_y; a.width = (uint32_t)g.width;
    a.div = make_cell_div((uint32_t)g.cell);
    a.top = static_cast<unsigned long long *>(top); a.bottom = static_cast<unsigned long long *>(bottom); a.count = static_cast<uint32_t *>(count);
    a.win_cells = win_cells;
    const bool colour = top || bottom;
    if (nW) {
        const size_t lds = GRID_TABLE_BYTES + (size_t)win_cells * ((top ? 8 : 0) + (bottom ? 8 : 0) + (count ? 4 : 0));
        grid_launch(c, true, colour, (unsigned)nW, lds, c->d_grid_list, a);
        HIP_TRY(c, hipGetLastError());
    }
    if (nD) {
        grid_launch(c, false, colour, (unsigned)nD, GRID_TABLE_BYTES, c->d_grid_list + nW, a);
        HIP_TRY(c, hipGetLastError());
    }
    return PCR_OK;
}

void grid_clear(pcr_ctx *c, const pcr_grid &g, void *top, void *bottom, void *count)
{
    const uint32_t n = (uint32_t)g.width * (uint32_t)g.height;
    hipLaunchKernelGGL(k_grid_clear, dim3(std::min<uint32_t>((n + 255) / 256, 2048)), dim3(256), 0, c->stream, static_cast<unsigned long long *>(top),
                       static_cast<unsigned long long *>(bottom), static_cast<uint32_t *>(count), n);
}
} // namespace

int pcr_grid_clear(pcr_ctx *c, const pcr_grid *grid, void *dev_top, void *dev_bottom, void *dev_count)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = grid_check(c, grid, dev_top, dev_bottom, dev_count))) return rc;
    if (!dev_top && !dev_bottom && !dev_count) return PCR_OK;
    grid_clear(c, *grid, dev_top, dev_bottom, dev_count);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_grid_accumulate(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip,
                        void *dev_top, void *dev_bottom, void *dev_count, uint32_t flags, pcr_grid_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = select_range(c, first_batch, count, &n);
    if (rc) return rc;
    if ((rc = grid_check(c, grid, dev_top, dev_bottom, dev_count))) return rc;
    if (flags & ~(uint32_t)PCR_GRID_NO_WINDOW) return set_err(c, PCR_E_ARG, "unknown flag bits 0x%x", flags & ~(uint32_t)PCR_GRID_NO_WINDOW);
    return grid_accumulate(c, first_batch, n, *grid, clip, dev_top, dev_bottom, dev_count, flags, stats);
}

int pcr_grid_unpack(pcr_ctx *c, const pcr_grid *grid, const void *dev_words, int which, void *dev_height, void *dev_rgba)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = grid_check(c, grid, dev_words, nullptr, nullptr))) return rc;
    if (which != PCR_GRID_TOP && which != PCR_GRID_BOTTOM) return set_err(c, PCR_E_ARG, "which is %d, not PCR_GRID_TOP or PCR_GRID_BOTTOM", which);
    if (!dev_words) return set_err(c, PCR_E_ARG, "the plane to unpack is NULL");
    if (reinterpret_cast<uintptr_t>(dev_height) % 4 != 0 || reinterpret_cast<uintptr_t>(dev_rgba) % 4 != 0)
        return set_err(c, PCR_E_ARG, "the height / rgba output is misaligned (4 bytes)");
    if (!dev_height && !dev_rgba) return PCR_OK;
    const uint32_t n = (uint32_t)grid->width * (uint32_t)grid->height;
    hipLaunchKernelGGL(k_grid_unpack, dim3(std::min<uint32_t>((n + 255) / 256, 2048)), dim3(256), 0, c->stream, static_cast<const unsigned long long *>(dev_words),
                       which == PCR_GRID_TOP ? 0ull : ~0ull, static_cast<int32_t *>(dev_height), static_cast<uint32_t *>(dev_rgba), n);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_read_grid(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip,
                  uint64_t *host_top, uint64_t *host_bottom, uint32_t *host_count, uint32_t flags, pcr_grid_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = select_range(c, first_batch, count, &n);
    if (rc) return rc;
    if ((rc = grid_check(c, grid, nullptr, nullptr, nullptr))) return rc;
    if (flags & ~(uint32_t)PCR_GRID_NO_WINDOW) return set_err(c, PCR_E_ARG, "unknown flag bits 0x%x", flags & ~(uint32_t)PCR_GRID_NO_WINDOW);
    const size_t cells = (size_t)grid->width * (size_t)grid->height;
    if (c->grid_scratch_bytes < cells * 20) {
        dfree(c->d_grid_scratch); c->grid_scratch_bytes = 0;
        if (hipMalloc((void **)&c->d_grid_scratch, cells * 20) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for the planes of a grid of %zu cells", cells);
        c->grid_scratch_bytes = cells * 20;
    }
    void *top = host_top ? c->d_grid_scratch : nullptr, *bottom = host_bottom ? c->d_grid_scratch + cells * 8 : nullptr;
    void *cnt = host_count ? c->d_grid_scratch + cells * 16 : nullptr;
    if (!top && !bottom && !cnt) return grid_accumulate(c, first_batch, n, *grid, clip, nullptr, nullptr, nullptr, flags, stats);
    grid_clear(c, *grid, top, bottom, cnt);
    HIP_TRY(c, hipGetLastError());
    if ((rc = grid_accumulate(c, first_batch, n, *grid, clip, top, bottom, cnt, flags, stats))) return rc;
    if (top) HIP_TRY(c, hipMemcpyAsync(host_top, top, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (bottom) HIP_TRY(c, hipMemcpyAsync(host_bottom, bottom, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (cnt) HIP_TRY(c, hipMemcpyAsync(host_count, cnt, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

// ---- ground filter and heights -----------------------------------------------------------------
namespace {
constexpr size_t GROUND_COUNTER_WORDS = 4 + 2 * (size_t)PCR_GROUND_MAX_FILL;    // class counts, then two words per fill round

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The filter's scratch for a grid of `cells` cells: three int32 planes, the counters, a byte plane.
size_t ground_scratch_bytes(size_t cells) { return round_up(cells * 12, 8) + GROUND_COUNTER_WORDS * 8 + round_up(cells, 16); }

// At least `bytes` of the scratch memory pcr_read_grid uses.
int grid_scratch_reserve(pcr_ctx *c, size_t bytes)
{
    if (c->grid_scratch_bytes >= bytes) return PCR_OK;
    dfree(c->d_grid_scratch); c->grid_scratch_bytes = 0;
    if (hipMalloc((void **)&c->d_grid_scratch, bytes) != hipSuccess)
        return set_err(c, PCR_E_NOMEM, "out of device memory for %zu bytes of grid planes", bytes);
    c->grid_scratch_bytes = bytes;
    return PCR_OK;
}

int ground_check(pcr_ctx *c, const pcr_grid *g, const pcr_ground_params *gp)
{
    if (!g) return set_err(c, PCR_E_ARG, "the grid is NULL");
    if (g->width < 1 || g->height < 1) return set_err(c, PCR_E_ARG, "grid of %d x %d cells: width and height are at least 1", g->width, g->height);
    if ((int64_t)g->width * g->height > PCR_GRID_MAX_CELLS)
        return set_err(c, PCR_E_ARG, "grid of %d x %d cells: more than the %d of PCR_GRID_MAX_CELLS", g->width, g->height, PCR_GRID_MAX_CELLS);
    if (!gp) return set_err(c, PCR_E_ARG, "the ground parameters are NULL");
    if (gp->num_steps < 0 || gp->num_steps > PCR_GROUND_MAX_STEPS) return set_err(c, PCR_E_ARG, "num_steps is %d, not 0 .. %d", gp->num_steps, PCR_GROUND_MAX_STEPS);
    if (gp->fill_rounds < 0 || gp->fill_rounds > PCR_GROUND_MAX_FILL) return set_err(c, PCR_E_ARG, "fill_rounds is %d, not 0 .. %d", gp->fill_rounds, PCR_GROUND_MAX_FILL);
    for (int k = 0; k < gp->num_steps; ++k) {
        if (gp->radius[k] < 1 || gp->radius[k] > PCR_GROUND_MAX_RADIUS)
            return set_err(c, PCR_E_ARG, "radius[%d] is %d, not 1 .. %d", k, gp->radius[k], PCR_GROUND_MAX_RADIUS);
        if (gp->threshold[k] < 0) return set_err(c, PCR_E_ARG, "threshold[%d] is %d: negative", k, gp->threshold[k]);
    }
    return PCR_OK;
}

// pcr_ground_filter behind its checks. `scratch` holds ground_scratch_bytes(cells). Synchronises.
int ground_filter(pcr_ctx *c, const pcr_grid &g, const pcr_ground_params &gp, const int32_t *lowest, int32_t *ground, uint8_t *cls,
                  unsigned char *scratch, pcr_ground_stats *stats)
{
    typedef unsigned long long u64;
    const uint32_t W = (uint32_t)g.width, H = (uint32_t)g.height, n = W * H;
    int32_t *A = reinterpret_cast<int32_t *>(scratch), *T1 = A + n, *T2 = T1 + n;
    u64 *counters = reinterpret_cast<u64 *>(scratch + round_up((size_t)n * 12, 8));
    uint8_t *flag = reinterpret_cast<uint8_t *>(counters + GROUND_COUNTER_WORDS);
    const dim3 flat((n + 255) / 256), block(256);
    HIP_TRY(c, hipMemsetAsync(counters, 0, GROUND_COUNTER_WORDS * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(flag, 0, n, c->stream));
    auto morph = [&](const int32_t *src, int32_t *dst, int r, bool column, bool is_max) {
        const uint32_t na = column ? H : W, nc = column ? W : H;
        const uint32_t ta = (na + GM_SPAN - 1) / GM_SPAN, tc = (nc + GM_LINES - 1) / GM_LINES;
        const GroundMorphArgs a{src, dst, W, H, (uint32_t)r, column ? 1u : 0u, is_max ? 1u : 0u, ta};
        hipLaunchKernelGGL(k_ground_morph, dim3(ta * tc), dim3(GM_THREADS), 0, c->stream, a);
    };
    for (int k = 0; k < gp.num_steps; ++k) {
        const int32_t *a_in = k == 0 ? lowest : A;
        const int r = gp.radius[k];
        morph(a_in, T1, r, false, false); morph(T1, T2, r, true, false);        // E: the minimum over the square
        morph(T2, T1, r, false, true); morph(T1, T2, r, true, true);            // O: the maximum of E over the square
        hipLaunchKernelGGL(k_ground_flag, flat, block, 0, c->stream, lowest, a_in, T2, A, flag, gp.threshold[k], n);
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_ground_class, flat, block, 0, c->stream, lowest, flag, ground, cls, counters, n);
    HIP_TRY(c, hipGetLastError());
    u64 classes[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(classes, counters, sizeof classes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    pcr_ground_stats st{(int64_t)classes[0], (int64_t)classes[1], (int64_t)classes[2], 0, (int64_t)(classes[0] + classes[2]), 0};
    // the fill: rounds between `ground` and T1; the host learns after every round what it did, so nothing depends on when it looks
    int32_t *cur = ground, *other = T1;
    for (int round = 0; round < gp.fill_rounds && st.cells_unfilled > 0; ++round) {
        u64 *rc = counters + 4 + 2 * (size_t)round, did[2] = {0, 0};
        hipLaunchKernelGGL(k_ground_fill, flat, block, 0, c->stream, cur, other, W, H, rc);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(did, rc, sizeof did, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (did[0] == 0) break;                                                 // (`other` equals `cur`: the round changed nothing)
        st.cells_filled += (int64_t)did[0]; st.cells_unfilled = (int64_t)did[1]; ++st.fill_rounds;
        std::swap(cur, other);
    }
    if (cur != ground) {
        HIP_TRY(c, hipMemcpyAsync(ground, cur, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (stats) *stats = st;
    return PCR_OK;
}

// grid and clip intersected into q (the far edges in 64 bits, as grid_accumulate); false: nothing is left
bool grid_clip_box(const pcr_grid &g, const pcr_box *clip, pcr_box &q)
{
    const int64_t org[2] = {g.origin_x, g.origin_y}, ext[2] = {g.width, g.height};
    bool empty = false;
    for (int k = 0; k < 3; ++k) {
        int64_t lo = clip ? clip->min[k] : INT32_MIN, hi = clip ? clip->max[k] : INT32_MAX;
        if (k < 2) { lo = std::max(lo, org[k]); hi = std::min(hi, org[k] + (int64_t)g.cell * ext[k] - 1); }
        empty = empty || lo > hi;
        q.min[k] = (int32_t)lo; q.max[k] = (int32_t)hi;
    }
    return !empty;
}

// What a height selection over batches [first, first + n) has to write: the batches that are not outside (ascending; their
// per-chain counts sit in c->sel.counts in the same order) and each one's record count.
struct HeightPlan {
    std::vector<uint32_t> listed;
    std::vector<int64_t> cnt;
    std::vector<int64_t> offsets;       // listed_write's
    HeightArgs a{};
    pcr_height_stats st{};
};

// Classify (host, from the cached exact boxes) and count (k_height_count). Synchronises.
int height_plan(pcr_ctx *c, int64_t first, int64_t n, const pcr_grid &g, const pcr_box *clip, HeightPlan &p)
{
    p.listed.clear(); p.cnt.clear();
    p.st = pcr_height_stats{n, 0, 0, 0};
    if (n == 0 || p.a.h_min > p.a.h_max || !grid_clip_box(g, clip, p.a.q)) return PCR_OK;
    int rc;
    if ((rc = ensure_point_bounds(c, first, n))) return rc;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *bb = c->h_point_bounds.data() + (first + i) * 6;
        bool disjoint = false;
        for (int k = 0; k < 3; ++k) disjoint = disjoint || bb[3 + k] < p.a.q.min[k] || bb[k] > p.a.q.max[k];
        if (!disjoint) p.listed.push_back((uint32_t)(first + i));
    }
    const int64_t nL = (int64_t)p.listed.size();
    p.st.batches_outside = n - nL; p.st.batches_decoded = nL;
    p.cnt.assign((size_t)nL, 0);
    if (nL == 0) return PCR_OK;
    if ((rc = scratch_reserve(c, c->sel, 2 * nL, "totals of the listed batches (two each)"))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->sel.list, p.listed.data(), (size_t)nL * 4, hipMemcpyHostToDevice, c->stream));
    p.a.ox = g.origin_x; p.a.oy = g.origin_y; p.a.width = (uint32_t)g.width;
    p.a.div = make_cell_div((uint32_t)g.cell);
    for_layout(c, [&](auto layout) {
        hipLaunchKernelGGL((k_height_count<layout.value>), dim3((unsigned)nL), dim3(PCR_WORKGROUP_SIZE), 0, c->stream, make_stream_view(c), c->sel.list, p.a,
                           c->sel.counts, c->sel.totals);
    });
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> totals((size_t)nL * 2);
    HIP_TRY(c, hipMemcpyAsync(totals.data(), c->sel.totals, (size_t)nL * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < nL; ++k) {
        p.cnt[(size_t)k] = totals[(size_t)k * 2];
        p.st.points_selected += totals[(size_t)k * 2]; p.st.points_no_ground += totals[(size_t)k * 2 + 1];
    }
    return PCR_OK;
}

// pcr_select_height / pcr_read_height: the records to o.points, their heights to column 0
int height_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_grid *grid, const void *dev_ground, const pcr_box *clip, int32_t h_min, int32_t h_max,
                uint32_t flags, const KeptOut &o, int64_t *out_count, pcr_height_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HeightPlan p;
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n);
    if (rc || (rc = grid_check(c, grid, nullptr, nullptr, nullptr))) return rc;
    if (!dev_ground) return set_err(c, PCR_E_ARG, "the ground plane is NULL");
    if (reinterpret_cast<uintptr_t>(dev_ground) % 4 != 0) return set_err(c, PCR_E_ARG, "the ground plane is misaligned (4 bytes)");
    if (flags & ~(uint32_t)PCR_HEIGHT_REPLACE_Z) return set_err(c, PCR_E_ARG, "unknown flag bits 0x%x", flags & ~(uint32_t)PCR_HEIGHT_REPLACE_Z);
    p.a.ground = static_cast<const int32_t *>(dev_ground); p.a.h_min = h_min; p.a.h_max = h_max; p.a.replace_z = flags & PCR_HEIGHT_REPLACE_Z;
    if ((rc = height_plan(c, first, n, *grid, clip, p)) || (rc = kept_finish(c, o, p.st.points_selected, "selected", p.st, out_count, stats, &done)) || done) return rc;
    return listed_write(c, p.cnt, p.offsets, c->sel.offsets, o, [&](int64_t k0, dim3 grid, const KeptOut &d) {
        for_layout_colour(c, d.points != nullptr, [&](auto layout, auto colour) {
            hipLaunchKernelGGL((k_height_write<layout.value, colour.value>), grid, dim3(PCR_WORKGROUP_SIZE), 0, c->stream, make_stream_view(c), c->sel.list + k0, p.a,
                               c->sel.counts + k0 * PCR_WORKGROUP_SIZE, c->sel.offsets + k0, static_cast<uint4 *>(d.points), static_cast<int32_t *>(d.col[0].dst));
        });
    });
}
} // namespace

int pcr_ground_filter(pcr_ctx *c, const pcr_grid *grid, const pcr_ground_params *gp, const void *dev_lowest, void *dev_ground, void *dev_class,
                      pcr_ground_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ground_check(c, grid, gp))) return rc;
    if (!dev_lowest || !dev_ground) return set_err(c, PCR_E_ARG, "the lowest / ground plane is NULL");
    if (dev_lowest == dev_ground) return set_err(c, PCR_E_ARG, "dev_ground must not be dev_lowest");
    if (reinterpret_cast<uintptr_t>(dev_lowest) % 4 != 0 || reinterpret_cast<uintptr_t>(dev_ground) % 4 != 0)
        return set_err(c, PCR_E_ARG, "the lowest / ground plane is misaligned (4 bytes)");
    const size_t cells = (size_t)grid->width * (size_t)grid->height;
    if ((rc = grid_scratch_reserve(c, ground_scratch_bytes(cells)))) return rc;
    return ground_filter(c, *grid, *gp, static_cast<const int32_t *>(dev_lowest), static_cast<int32_t *>(dev_ground), static_cast<uint8_t *>(dev_class),
                         c->d_grid_scratch, stats);
}

int pcr_read_ground(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip, const pcr_ground_params *gp,
                    int32_t *host_lowest, int32_t *host_ground, uint8_t *host_class, pcr_ground_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = select_range(c, first_batch, count, &n);
    if (rc) return rc;
    if ((rc = grid_check(c, grid, nullptr, nullptr, nullptr)) || (rc = ground_check(c, grid, gp))) return rc;
    // the filter's scratch, then the bottom plane, the lowest and ground planes and the classes
    const size_t cells = (size_t)grid->width * (size_t)grid->height, own = round_up(ground_scratch_bytes(cells), 16);
    if ((rc = grid_scratch_reserve(c, own + cells * 8 + cells * 4 + cells * 4 + cells))) return rc;
    unsigned char *const bottom = c->d_grid_scratch + own;
    int32_t *const lowest = reinterpret_cast<int32_t *>(bottom + cells * 8), *const ground = lowest + cells;
    uint8_t *const cls = reinterpret_cast<uint8_t *>(ground + cells);
    grid_clear(c, *grid, nullptr, bottom, nullptr);
    HIP_TRY(c, hipGetLastError());
    if ((rc = grid_accumulate(c, first_batch, n, *grid, clip, nullptr, bottom, nullptr, 0, nullptr))) return rc;
    hipLaunchKernelGGL(k_grid_unpack, dim3(std::min<uint32_t>(((uint32_t)cells + 255) / 256, 2048)), dim3(256), 0, c->stream,
                       reinterpret_cast<const unsigned long long *>(bottom), ~0ull, lowest, static_cast<uint32_t *>(nullptr), (uint32_t)cells);
    HIP_TRY(c, hipGetLastError());
    if ((rc = ground_filter(c, *grid, *gp, lowest, ground, cls, c->d_grid_scratch, stats))) return rc;
    if (host_lowest) HIP_TRY(c, hipMemcpyAsync(host_lowest, lowest, cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (host_ground) HIP_TRY(c, hipMemcpyAsync(host_ground, ground, cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (host_class) HIP_TRY(c, hipMemcpyAsync(host_class, cls, cells, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

int pcr_select_height(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_grid *grid, const void *dev_ground, const pcr_box *clip,
                      int32_t h_min, int32_t h_max, uint32_t flags, void *dev_points, void *dev_heights, size_t capacity, int64_t *out_count,
                      pcr_height_stats *stats)
{
    return height_call(c, first_batch, count, grid, dev_ground, clip, h_min, h_max, flags, KeptOut{false, dev_points, capacity, {heights_column(dev_heights)}},
                       out_count, stats);
}

int pcr_read_height(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_grid *grid, const void *dev_ground, const pcr_box *clip,
                    int32_t h_min, int32_t h_max, uint32_t flags, pcr_point *host_points, int32_t *host_heights, size_t capacity,
                    int64_t *out_count, pcr_height_stats *stats)
{
    return height_call(c, first_batch, count, grid, dev_ground, clip, h_min, h_max, flags, KeptOut{true, host_points, capacity, {heights_column(host_heights)}},
                       out_count, stats);
}

// ---- height percentiles per grid cell ----------------------------------------------------------
namespace {
// The checks both entry points share behind the range check (dev: the floor and the outputs are device pointers, 4-byte aligned).
int quantiles_check(pcr_ctx *c, int64_t n, const pcr_grid *grid, const void *floor, const uint32_t *q, int32_t num_q, const void *quantiles,
                    const void *count, uint32_t flags)
{
    int rc;
    if ((rc = grid_check(c, grid, nullptr, nullptr, count))) return rc;
    if (flags & ~(uint32_t)PCR_GRID_NO_WINDOW) return set_err(c, PCR_E_ARG, "unknown flag bits 0x%x", flags & ~(uint32_t)PCR_GRID_NO_WINDOW);
    if (!q) return set_err(c, PCR_E_ARG, "q is NULL");
    if (num_q < 1 || num_q > PCR_QUANTILES_MAX) return set_err(c, PCR_E_ARG, "num_q of %d outside 1 .. %d", num_q, PCR_QUANTILES_MAX);
    for (int32_t j = 0; j < num_q; ++j)
        if (q[j] > PCR_QUANTILE_ONE) return set_err(c, PCR_E_ARG, "q[%d] of %u basis points: more than the %d of PCR_QUANTILE_ONE", j, q[j], PCR_QUANTILE_ONE);
    if (reinterpret_cast<uintptr_t>(quantiles) % 4 != 0) return set_err(c, PCR_E_ARG, "the quantile planes are misaligned (4 bytes)");
    if (reinterpret_cast<uintptr_t>(floor) % 4 != 0) return set_err(c, PCR_E_ARG, "the floor plane is misaligned (4 bytes)");
    // the counts, the segment offsets and the candidate total are 32 bits: 65 535 batches hold less than 2^32 records
    if (n > PCR_QUANTILE_MAX_BATCHES)
        return set_err(c, PCR_E_ARG, "a range of %lld batches: more than the %d of PCR_QUANTILE_MAX_BATCHES", (long long)n, PCR_QUANTILE_MAX_BATCHES);
    return PCR_OK;
}

void quantiles_launch(pcr_ctx *c, bool fill, bool windowed, unsigned nblocks, size_t lds, const GridEntry *list, const QuantArgs &a)
{
    const StreamView s = make_stream_view(c);
    const dim3 grid(nblocks), block(PCR_WORKGROUP_SIZE);
    auto both = [&](auto layout, auto win) {
        if (fill) hipLaunchKernelGGL((k_quant_fill<layout.value, win.value>), grid, block, lds, c->stream, s, list, a);
        else      hipLaunchKernelGGL((k_quant_count<layout.value, win.value>), grid, block, lds, c->stream, s, list, a);
    };
    for_layout(c, [&](auto layout) { if (windowed) both(layout, std::true_type{}); else both(layout, std::false_type{}); });
}

// pcr_grid_quantiles behind its checks: n batches from `first`; floor, planes and count are device pointers or NULL. Synchronises.
int grid_quantiles(pcr_ctx *c, int64_t first, int64_t n, const pcr_grid &g, const pcr_box *clip, const int32_t *floor, const uint32_t *q, int32_t num_q,
                   int32_t *planes, uint32_t *count, uint32_t flags, pcr_quantile_stats *stats)
{
    pcr_quantile_stats st{};
    st.batches_outside = n;
    QuantArgs a{};
    std::vector<GridEntry> list;
    size_t nW = 0;
    int rc = PCR_OK;
    if (n > 0 && grid_clip_box(g, clip, a.q) &&
        (rc = grid_classify(c, first, n, g, a.q, flags, list, nW, a.win_cells, st.batches_outside, st.batches_windowed, st.batches_direct))) return rc;
    const size_t nD = list.size() - nW;
    if (!list.empty() && (rc = grid_list_upload(c, list))) return rc;
    // the scratch: the counters, then per cell the segment (8 bytes), the work list (4 bytes per cell that can be occupied: no more
    // than the records decoded) and, if the caller takes no counts, the count plane
    const size_t cells = (size_t)g.width * (size_t)g.height;
    const size_t list_capacity = planes ? std::min(cells, list.size() * (size_t)PCR_POINTS_PER_BATCH) : 0;
    const size_t seg_at = QUANT_COUNTERS * 4, list_at = seg_at + (planes ? cells * 8 : 0), count_at = list_at + list_capacity * 4;
    const size_t need = count_at + (count ? 0 : cells * 4);
    if (c->quant_scratch_bytes < need) {
        dfree(c->d_quant_scratch); c->quant_scratch_bytes = 0;
        if (hipMalloc((void **)&c->d_quant_scratch, need) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for %zu bytes of scratch for a grid of %zu cells: pass a coarser grid", need, cells);
        c->quant_scratch_bytes = need;
    }
    a.ox = g.origin_x; a.oy = g.origin_y; a.width = (uint32_t)g.width; a.cells = (uint32_t)cells;
    a.div = make_cell_div((uint32_t)g.cell);
    a.floor = floor;
    a.counters = reinterpret_cast<uint32_t *>(c->d_quant_scratch);
    a.seg = reinterpret_cast<uint2 *>(c->d_quant_scratch + seg_at);
    a.list = reinterpret_cast<uint32_t *>(c->d_quant_scratch + list_at);
    a.list_capacity = (uint32_t)list_capacity;
    a.count = count ? count : reinterpret_cast<uint32_t *>(c->d_quant_scratch + count_at);
    a.planes = planes;
    a.num_q = (uint32_t)num_q;
    for (int32_t j = 0; j < num_q; ++j) a.qv[j] = q[j];
    const unsigned cell_blocks = (unsigned)std::min<size_t>((cells + 255) / 256, 2048);
    HIP_TRY(c, hipMemsetAsync(a.counters, 0, QUANT_COUNTERS * 4, c->stream));
    hipLaunchKernelGGL(k_grid_clear, dim3(cell_blocks), dim3(256), 0, c->stream, (unsigned long long *)nullptr, (unsigned long long *)nullptr, a.count, a.cells);
    HIP_TRY(c, hipGetLastError());
    // 1. count
    if (nW) { quantiles_launch(c, false, true, (unsigned)nW, GRID_TABLE_BYTES + (size_t)a.win_cells * 4, c->d_grid_list, a); HIP_TRY(c, hipGetLastError()); }
    if (nD) { quantiles_launch(c, false, false, (unsigned)nD, GRID_TABLE_BYTES, c->d_grid_list + nW, a); HIP_TRY(c, hipGetLastError()); }
    // 2. allocate: segments, work lists, INT32_MIN into the empty cells, the statistics
    const uint32_t chunk = (uint32_t)(((cells + cell_blocks - 1) / cell_blocks + 255) / 256 * 256);    // per workgroup: chunk * cell_blocks >= cells
    hipLaunchKernelGGL(k_quant_alloc, dim3(cell_blocks), dim3(256), 0, c->stream, a, chunk);
    HIP_TRY(c, hipGetLastError());
    uint32_t h[QUANT_COUNTERS] = {};
    HIP_TRY(c, hipMemcpyAsync(h, a.counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    st.candidates = h[QUANT_VALUES]; st.cells_occupied = (int64_t)h[QUANT_SMALL] + h[QUANT_LARGE]; st.max_cell_points = h[QUANT_MAX_CELL];
    if (stats) *stats = st;
    if (h[QUANT_ERROR]) return set_err(c, PCR_E_NOMEM, "the work list of the quantile call is too short");    // (cannot happen)
    if (!planes || st.candidates == 0) return PCR_OK;
    if (c->quant_values_entries < (size_t)st.candidates) {
        dfree(c->d_quant_values); c->quant_values_entries = 0;
        if (hipMalloc((void **)&c->d_quant_values, (size_t)st.candidates * 4) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for %zu bytes of scratch (the z of %lld candidates): pass a clip or a shorter range",
                           (size_t)st.candidates * 4, (long long)st.candidates);
        c->quant_values_entries = (size_t)st.candidates;
    }
    a.values = c->d_quant_values; a.candidates = (uint32_t)st.candidates;
    // 3. fill (the window holds the next slot and the end of every cell: 8 bytes a cell, 48 KiB with the table at most)
    if (nW) { quantiles_launch(c, true, true, (unsigned)nW, GRID_TABLE_BYTES + (size_t)a.win_cells * 8, c->d_grid_list, a); HIP_TRY(c, hipGetLastError()); }
    if (nD) { quantiles_launch(c, true, false, (unsigned)nD, GRID_TABLE_BYTES, c->d_grid_list + nW, a); HIP_TRY(c, hipGetLastError()); }
    // 4. select: a wave per 64 small cells, a workgroup per large one, each list walked with the grid's stride
    if (h[QUANT_SMALL]) {
        hipLaunchKernelGGL(k_quant_select_small, dim3(std::min<uint32_t>((h[QUANT_SMALL] + 255) / 256, 8192)), dim3(256), 0, c->stream, a, h[QUANT_SMALL]);
        HIP_TRY(c, hipGetLastError());
    }
    if (h[QUANT_LARGE]) {
        hipLaunchKernelGGL(k_quant_select_large, dim3(std::min<uint32_t>(h[QUANT_LARGE], 8192)), dim3(256), 0, c->stream, a, h[QUANT_LARGE]);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(h, a.counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h[QUANT_ERROR]) return set_err(c, PCR_E_NOMEM, "the counts and the segments of the quantile call disagree");   // (cannot happen)
    return PCR_OK;
}
} // namespace

int pcr_grid_quantiles(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip, const void *dev_floor,
                       const uint32_t *q, int32_t num_q, void *dev_quantiles, void *dev_count, uint32_t flags, pcr_quantile_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = select_range(c, first_batch, count, &n);
    if (rc) return rc;
    if ((rc = quantiles_check(c, n, grid, dev_floor, q, num_q, dev_quantiles, dev_count, flags))) return rc;
    return grid_quantiles(c, first_batch, n, *grid, clip, static_cast<const int32_t *>(dev_floor), q, num_q, static_cast<int32_t *>(dev_quantiles),
                          static_cast<uint32_t *>(dev_count), flags, stats);
}

int pcr_read_grid_quantiles(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_grid *grid, const pcr_box *clip, const int32_t *host_floor,
                            const uint32_t *q, int32_t num_q, int32_t *host_quantiles, uint32_t *host_count, uint32_t flags, pcr_quantile_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    int rc = select_range(c, first_batch, count, &n);
    if (rc) return rc;
    if ((rc = quantiles_check(c, n, grid, host_floor, q, num_q, host_quantiles, host_count, flags))) return rc;
    // the floor, the planes and the counts in the scratch memory pcr_read_grid uses
    const size_t cells = (size_t)grid->width * (size_t)grid->height;
    const size_t planes_at = host_floor ? cells * 4 : 0, count_at = planes_at + (host_quantiles ? cells * 4 * (size_t)num_q : 0);
    if ((rc = grid_scratch_reserve(c, std::max<size_t>(count_at + (host_count ? cells * 4 : 0), 16)))) return rc;
    int32_t *const d_floor = host_floor ? reinterpret_cast<int32_t *>(c->d_grid_scratch) : nullptr;
    int32_t *const d_planes = host_quantiles ? reinterpret_cast<int32_t *>(c->d_grid_scratch + planes_at) : nullptr;
    uint32_t *const d_count = host_count ? reinterpret_cast<uint32_t *>(c->d_grid_scratch + count_at) : nullptr;
    if (d_floor) HIP_TRY(c, hipMemcpyAsync(d_floor, host_floor, cells * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = grid_quantiles(c, first_batch, n, *grid, clip, d_floor, q, num_q, d_planes, d_count, flags, stats))) return rc;
    if (d_planes) HIP_TRY(c, hipMemcpyAsync(host_quantiles, d_planes, cells * 4 * (size_t)num_q, hipMemcpyDeviceToHost, c->stream));
    if (d_count) HIP_TRY(c, hipMemcpyAsync(host_count, d_count, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

// ---- kept rows: the host path of pcr_thin, _denoise, _components, _neighbors, _local_moments, _knn and _voxel_mean ----------
// Each of these calls classifies batches against a clip, builds a voxel table, sets bits in the keep bitmap c->d_thin_keep, counts
// them per batch and writes the kept records with a few columns per row; the device form (pcr_X) and the host form (pcr_read_X)
// differ in where the destinations live. What they share is here; the sections below hold each call's checks, plan and kernels.
extern "C++" {                          // (templates among them)
namespace {
// What a call over batches [first, first + n) has to write: the batches the clip does not miss, of those the ones that keep a
// record (their keep words sit in c->d_thin_keep) and each one's record count.
struct ThinPlan {
    std::vector<uint32_t> listed;       // ascending
    std::vector<uint32_t> writers;      // ascending
    std::vector<int64_t> cnt;           // [writers.size()]
    std::vector<int64_t> offsets;       // staging of the write kernels' offsets (alive until the stream has been synchronised)
    pcr_thin_stats st{};                // thin_plan only
    ThinArgs args{};                    // the clip, the lattice and the table of the plan (pcr_components: for k_components_labels;
                                        // thin_plan: for pcr_voxel_mean's kernels)
    const thin_u64 *label = nullptr;    // pcr_components only: the label of every slot
};

// The batches of [first, first + n) whose exact box the clip a.q does not miss into `listed` (ascending), and into q the union of
// their boxes intersected with the clip. a.q is not empty.
int thin_list_batches(pcr_ctx *c, int64_t first, int64_t n, const ThinArgs &a, std::vector<uint32_t> &listed, pcr_box &q)
{
    int rc;
    if ((rc = ensure_point_bounds(c, first, n))) return rc;
    q = pcr_box{{INT32_MAX, INT32_MAX, INT32_MAX}, {INT32_MIN, INT32_MIN, INT32_MIN}};
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *bb = c->h_point_bounds.data() + (first + i) * 6;
        bool disjoint = false;
        for (int k = 0; k < 3; ++k) disjoint = disjoint || bb[3 + k] < a.q.min[k] || bb[k] > a.q.max[k];
        if (disjoint) continue;
        listed.push_back((uint32_t)(first + i));
        for (int k = 0; k < 3; ++k) { q.min[k] = std::min(q.min[k], bb[k]); q.max[k] = std::max(q.max[k], bb[3 + k]); }
    }
    for (int k = 0; k < 3; ++k) { q.min[k] = std::max(q.min[k], a.q.min[k]); q.max[k] = std::min(q.max[k], a.q.max[k]); }
    return PCR_OK;
}

// The lists of nL batches, the error word and the keep bitmap of n batches
int thin_reserve(pcr_ctx *c, int64_t nL, int64_t n)
{
    if (c->thin_capacity < nL) {
        dfree(c->d_thin_list); dfree(c->d_thin_totals); dfree(c->d_thin_wlist); dfree(c->d_thin_offsets); c->thin_capacity = 0;
        if (hipMalloc((void **)&c->d_thin_list, (size_t)nL * 4) != hipSuccess || hipMalloc((void **)&c->d_thin_totals, (size_t)nL * 8) != hipSuccess ||
            hipMalloc((void **)&c->d_thin_wlist, (size_t)nL * 4) != hipSuccess || hipMalloc((void **)&c->d_thin_offsets, (size_t)nL * 8) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for the lists of %lld batches", (long long)nL);
        c->thin_capacity = nL;
    }
    if (!c->d_thin_error && hipMalloc((void **)&c->d_thin_error, 4) != hipSuccess) return set_err(c, PCR_E_NOMEM, "out of device memory for a word");
    if (!thin_grow((void **)&c->d_thin_keep, c->thin_keep_words, n * PCR_WORKGROUP_SIZE, 8))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the keep bitmap of %lld batches", (long long)n);
    return PCR_OK;
}

// What the plans share: the statistics common to all, and what the first half hands to the call's own kernels and to the tail.
struct VoxelPlan {
    int64_t batches_outside = 0, batches_decoded = 0, points_considered = 0, runs = 0, table_slots = 0, points_written = 0;
    int64_t nL = 0;                     // the listed batches
    bool windows = false;               // the layout the kernels read
    ThinArgs a{};                       // the clip, the lattice, the first batch, the table and the error word
    std::vector<uint32_t> totals;       // staging of d_thin_totals and the error word
};

// The two kinds of voxel table: the lattice (pcr_lattice.h), its voxel limit as the messages put it, and how the table starts.
// ones: every byte of the table 0xFF and the keep bitmap zeroed, for k_thin_mark's minima and k_thin_flag's bits; otherwise
// k_denoise_clear: key = all ones and value = 0 in every slot (every lane of a listed batch stores its keep word later).
// levels > 0: the lattice is lod_lattice with that many levels (`lattice` is not called).
struct VoxelTable {
    int (*lattice)(const int32_t origin[3], int32_t cell, const int32_t qmin[3], const int32_t qmax[3], ThinLattice *out, int *axis);
    const char *max_voxels;
    bool ones;
    int32_t levels = 0;
};
constexpr VoxelTable THIN_TABLE{thin_lattice, "2^21", true}, NOISE_TABLE{noise_lattice, "2^21 - 2", false};

// The first half of every plan: classify (host, from the cached exact boxes), the lattice, the scratch, the runs (k_thin_runs), the
// table sized from them and started as `table` says, the error word cleared. v.runs == 0 on return: nothing to do, no kernel has
// touched the table. `verb` names the call in the messages; a table of more than 2^max_log2_slots slots is refused. Synchronises.
int voxel_plan_begin(pcr_ctx *c, int64_t first, int64_t n, const pcr_voxels &vox, const pcr_box *clip, const char *verb, const VoxelTable &table,
                     uint32_t max_log2_slots, ThinPlan &p, VoxelPlan &v, const char *cell = "cell")
{
    p.listed.clear(); p.writers.clear(); p.cnt.clear();
    v = VoxelPlan{};
    v.batches_outside = n;
    ThinArgs &a = v.a;
    for (int k = 0; k < 3; ++k) { a.q.min[k] = clip ? clip->min[k] : INT32_MIN; a.q.max[k] = clip ? clip->max[k] : INT32_MAX; }
    if (n == 0 || box_empty(a.q)) return PCR_OK;
    int rc;
    pcr_box q{};                                    // the union of the listed batches' boxes, inside the clip
    if ((rc = thin_list_batches(c, first, n, a, p.listed, q))) return rc;
    const int64_t nL = (int64_t)p.listed.size();
    if (nL == 0) return PCR_OK;
    int axis = 0;
    switch (table.levels > 0 ? lod_lattice(vox.origin, vox.cell, table.levels, q.min, q.max, &a.lat, &axis)
                             : table.lattice(vox.origin, vox.cell, q.min, q.max, &a.lat, &axis)) {
    case THIN_LATTICE_EXTENT:
        return set_err(c, PCR_E_ARG, "the points to %s span %lld on axis %d, 2^31 or more: pass a clip or a larger %s (a tail artefact far outside the cloud?)",
                       verb, (long long)q.max[axis] - (long long)q.min[axis], axis, cell);
    case THIN_LATTICE_VOXELS:
        return set_err(c, PCR_E_ARG, "the points to %s span %lld on axis %d, more than %s voxels of %d: pass a clip or a larger %s (a tail artefact far outside the cloud?)",
                       verb, (long long)q.max[axis] - (long long)q.min[axis], axis, table.max_voxels, vox.cell, cell);
    default: break;
    }
    v.batches_outside = n - nL; v.batches_decoded = nL; v.nL = nL;
    if ((rc = thin_reserve(c, nL, n))) return rc;

    a.first_batch = (uint32_t)first;
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)nL), block(PCR_WORKGROUP_SIZE);
    v.windows = select_reads_windows(c);
    HIP_TRY(c, hipMemcpyAsync(c->d_thin_list, p.listed.data(), (size_t)nL * 4, hipMemcpyHostToDevice, c->stream));
    if (v.windows) hipLaunchKernelGGL((k_thin_runs<LAYOUT_POINT_WINDOWS>), grid, block, 0, c->stream, s, c->d_thin_list, a, c->d_thin_totals);
    else           hipLaunchKernelGGL((k_thin_runs<LAYOUT_WORDS>), grid, block, 0, c->stream, s, c->d_thin_list, a, c->d_thin_totals);
    HIP_TRY(c, hipGetLastError());
    v.totals.assign((size_t)nL * 2 + 1, 0u);
    HIP_TRY(c, hipMemcpyAsync(v.totals.data(), c->d_thin_totals, (size_t)nL * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < nL; ++k) { v.runs += v.totals[(size_t)k * 2]; v.points_considered += v.totals[(size_t)k * 2 + 1]; }
    if (v.runs == 0) return PCR_OK;

    uint32_t log2_slots = 10;
    while (((int64_t)1 << log2_slots) < 2 * v.runs) ++log2_slots;
    const int64_t slots = (int64_t)1 << log2_slots;
    if (log2_slots > max_log2_slots)
        return set_err(c, PCR_E_NOMEM, "a voxel table of %lld slots (%lld runs) is more than the 2^%u this call can index: pass a clip or a larger %s",
                       (long long)slots, (long long)v.runs, max_log2_slots, cell);
    if (!thin_grow((void **)&c->d_thin_table, c->thin_slots, slots, sizeof(ThinSlot)))
        return set_err(c, PCR_E_NOMEM, "out of device memory for a voxel table of %lld slots (%lld runs): pass a clip or a larger %s", (long long)slots,
                       (long long)v.runs, cell);
    v.table_slots = slots;
    a.log2_slots = log2_slots; a.table = c->d_thin_table; a.error = c->d_thin_error;
    if (table.ones) {
        HIP_TRY(c, hipMemsetAsync(c->d_thin_table, 0xFF, (size_t)slots * sizeof(ThinSlot), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_thin_keep, 0, (size_t)n * PCR_WORKGROUP_SIZE * 8, c->stream));
    } else {
        hipLaunchKernelGGL(k_denoise_clear, dim3((unsigned)std::min<int64_t>((slots + 255) / 256, 4096)), dim3(256), 0, c->stream, c->d_thin_table,
                           (unsigned long long)slots);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemsetAsync(c->d_thin_error, 0, 4, c->stream));
    return PCR_OK;
}

// The tail of every plan, once the keep bitmap is set: count the kept rows per batch (k_thin_totals), read the totals and the error
// word back, refuse an overflow of the table, and collect the plan an emit takes (p.writers, p.cnt) and v.points_written. `bytes` of
// the call's device counters `src` go to `dst` on the way. Synchronises.
int voxel_plan_collect(pcr_ctx *c, int64_t first, ThinPlan &p, VoxelPlan &v, void *dst = nullptr, const void *src = nullptr, size_t bytes = 0)
{
    const int64_t nL = v.nL;
    hipLaunchKernelGGL(k_thin_totals, dim3((unsigned)nL), dim3(256), 0, c->stream, c->d_thin_list, (uint32_t)first, c->d_thin_keep, c->d_thin_totals);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(v.totals.data(), c->d_thin_totals, (size_t)nL * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(v.totals.data() + nL * 2, c->d_thin_error, 4, hipMemcpyDeviceToHost, c->stream));
    if (bytes) HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (v.totals[(size_t)nL * 2]) return set_err(c, PCR_E_NOMEM, "voxel table overflow: %lld slots for %lld runs", (long long)v.table_slots, (long long)v.runs);
    for (int64_t k = 0; k < nL; ++k) {
        if (!v.totals[(size_t)k]) continue;
        p.writers.push_back(p.listed[(size_t)k]); p.cnt.push_back(v.totals[(size_t)k]);
        v.points_written += v.totals[(size_t)k];
    }
    return PCR_OK;
}

// The last of a call's checks: a range of n batches holds at most max_rows rows (`limit` words it: 2^40 where rows are 64-bit, 2^32
// where an index or a sum holds a 32-bit row)
constexpr const char *ROWS_2_40 = "2^40 rows", *ROWS_2_32_INDEX = "2^32 rows (the index stores a 32-bit row)";
int kept_row_limit(pcr_ctx *c, int64_t n, int64_t max_rows, const char *limit)
{
    if (n > max_rows / PCR_POINTS_PER_BATCH) return set_err(c, PCR_E_ARG, "a range of %lld batches has more than %s", (long long)n, limit);
    return PCR_OK;
}

// Where the write of some batches of a plan launches: a workgroup per writer among them, list[x] its batch and offsets[x] its
// first output record
struct EmitAt {
    StreamView s;
    dim3 grid, block;
    const uint32_t *list;
    const int64_t *offsets;
};

// The writers among batches [i0, i1) of the plan's range and the first output record of each, counted from the first of them, on
// their way to the device. e.grid.x == 0: there is none.
int emit_offsets(pcr_ctx *c, int64_t first, int64_t i0, int64_t i1, ThinPlan &p, EmitAt &e)
{
    const size_t w0 = (size_t)(std::lower_bound(p.writers.begin(), p.writers.end(), (uint32_t)(first + i0)) - p.writers.begin());
    const size_t w1 = (size_t)(std::lower_bound(p.writers.begin(), p.writers.end(), (uint32_t)(first + i1)) - p.writers.begin());
    e = EmitAt{make_stream_view(c), dim3((unsigned)(w1 - w0)), dim3(PCR_WORKGROUP_SIZE), c->d_thin_wlist + w0, c->d_thin_offsets + w0};
    if (w0 == w1) return PCR_OK;
    p.offsets.clear();
    int64_t off = 0;
    for (size_t w = w0; w < w1; ++w) { p.offsets.push_back(off); off += p.cnt[w]; }
    HIP_TRY(c, hipMemcpyAsync(c->d_thin_wlist + w0, p.writers.data() + w0, (w1 - w0) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_thin_offsets + w0, p.offsets.data(), (w1 - w0) * 8, hipMemcpyHostToDevice, c->stream));
    return PCR_OK;
}

// Enqueue the writes of batches [i0, i1) of the plan's range: launch(layout, bc7, e) starts the call's write kernel at e. The
// caller synchronises.
template <class Launch>
int kept_emit(pcr_ctx *c, int64_t first, int64_t i0, int64_t i1, ThinPlan &p, Launch launch)
{
    EmitAt e;
    const int rc = emit_offsets(c, first, i0, i1, p, e);
    if (rc || e.grid.x == 0) return rc;
    for_layout_bc7(c, [&](auto layout, auto bc7) { launch(layout, bc7, e); });
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

// kept_write for a plan of the kept-rows calls: its units are the n batches of the range, their rows are the writers' counts
template <class Emit>
int kept_write(pcr_ctx *c, int64_t first, int64_t n, const ThinPlan &p, const KeptOut &o, Emit emit, bool stage_named = false)
{
    size_t w = 0;
    return kept_write(c, n, o, [&](int64_t, int64_t i1) {
        int64_t m = 0;
        for (; w < p.writers.size() && p.writers[w] < (uint32_t)(first + i1); ++w) m += p.cnt[w];
        return m;
    }, emit, stage_named);
}
} // namespace
} // extern "C++"

// ---- voxel thinning ----------------------------------------------------------------------------
namespace {
// Phases one to three: the plan's first half, then fill the voxel table (k_thin_mark), flag the kept rows and count them per batch.
// Synchronises.
int thin_plan(pcr_ctx *c, int64_t first, int64_t n, const pcr_voxels &vox, const pcr_box *clip, int mode, ThinPlan &p)
{
    VoxelPlan v;
    int rc = voxel_plan_begin(c, first, n, vox, clip, "thin", THIN_TABLE, 62, p, v);    // (2^40 rows: never more than 2^41 slots)
    p.st = pcr_thin_stats{v.batches_outside, v.batches_decoded, v.points_considered, v.runs, 0, v.table_slots};
    if (rc || v.runs == 0) return rc;
    p.args = v.a;
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)v.nL), block(PCR_WORKGROUP_SIZE);
#define PCR_LAUNCH(L, M) hipLaunchKernelGGL((k_thin_mark<L, M>), grid, block, 0, c->stream, s, c->d_thin_list, v.a)
    if (v.windows) { if (mode == PCR_THIN_CENTER) PCR_LAUNCH(LAYOUT_POINT_WINDOWS, PCR_THIN_CENTER); else PCR_LAUNCH(LAYOUT_POINT_WINDOWS, PCR_THIN_FIRST); }
    else           { if (mode == PCR_THIN_CENTER) PCR_LAUNCH(LAYOUT_WORDS, PCR_THIN_CENTER); else PCR_LAUNCH(LAYOUT_WORDS, PCR_THIN_FIRST); }
#undef PCR_LAUNCH
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_thin_flag, dim3((unsigned)std::min<int64_t>((v.table_slots + 255) / 256, 4096)), dim3(256), 0, c->stream, c->d_thin_table,
                       (unsigned long long)v.table_slots, (unsigned long long)n * PCR_POINTS_PER_BATCH, c->d_thin_keep);
    HIP_TRY(c, hipGetLastError());
    rc = voxel_plan_collect(c, first, p, v);
    p.st.points_kept = v.points_written;
    return rc;
}

// Enqueue the writes of batches [i0, i1) of the plan's range: their kept records to d.points, the rows to column 0 (device, either
// may be NULL, each holds the records of those batches); for a plan of pcr_components the labels of the rows to column 1 as well
// (NULL: not). The caller synchronises.
int thin_emit(pcr_ctx *c, int64_t first, int64_t i0, int64_t i1, ThinPlan &p, const KeptOut &d)
{
    uint4 *const points = static_cast<uint4 *>(d.points);
    int64_t *const rows = static_cast<int64_t *>(d.col[0].dst), *const labels = static_cast<int64_t *>(d.col[1].dst);
    EmitAt e;
    const int rc = emit_offsets(c, first, i0, i1, p, e);
    if (rc || e.grid.x == 0) return rc;
    if (points || rows) {
        for_layout_bc7(c, [&](auto layout, auto bc7) {
            hipLaunchKernelGGL((k_thin_write<layout.value, bc7.value>), e.grid, e.block, 0, c->stream, e.s, e.list, (uint32_t)first, c->d_thin_keep, e.offsets,
                               points, rows);
        });
        HIP_TRY(c, hipGetLastError());
    }
    if (labels) {
        if (select_reads_windows(c))
            hipLaunchKernelGGL((k_components_labels<LAYOUT_POINT_WINDOWS>), e.grid, e.block, 0, c->stream, e.s, e.list, p.args, c->d_thin_keep, e.offsets,
                               p.label, labels);
        else
            hipLaunchKernelGGL((k_components_labels<LAYOUT_WORDS>), e.grid, e.block, 0, c->stream, e.s, e.list, p.args, c->d_thin_keep, e.offsets, p.label,
                               labels);
        HIP_TRY(c, hipGetLastError());
    }
    return PCR_OK;
}

// kept_write for the three calls that write with thin_emit
int thin_write(pcr_ctx *c, int64_t first, int64_t n, ThinPlan &p, const KeptOut &o)
{
    return kept_write(c, first, n, p, o, [&](int64_t i0, int64_t i1, const KeptOut &d) { return thin_emit(c, first, i0, i1, p, d); }, true);
}

// pcr_thin / pcr_read_thin
int thin_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int mode, const KeptOut &o, int64_t *out_count,
              pcr_thin_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ThinPlan p;
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n, true, vox);
    if (rc) return rc;
    if (mode != PCR_THIN_FIRST && mode != PCR_THIN_CENTER) return set_err(c, PCR_E_ARG, "mode is %d, not PCR_THIN_FIRST or PCR_THIN_CENTER", mode);
    if (mode == PCR_THIN_CENTER && vox->cell > PCR_THIN_MAX_CENTER_CELL)
        return set_err(c, PCR_E_ARG, "voxel cell of %d with PCR_THIN_CENTER: at most %d (PCR_THIN_MAX_CENTER_CELL)", vox->cell, PCR_THIN_MAX_CENTER_CELL);
    if ((rc = kept_row_limit(c, n, (int64_t)1 << 40, ROWS_2_40)) || (rc = thin_plan(c, first, n, *vox, clip, mode, p))) return rc;
    if ((rc = kept_finish(c, o, p.st.points_kept, "kept", p.st, out_count, stats, &done)) || done) return rc;
    return thin_write(c, first, n, p, o);
}
} // namespace

int pcr_thin(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int mode, void *dev_points, void *dev_rows,
             size_t capacity_points, int64_t *out_count, pcr_thin_stats *stats)
{
    return thin_call(c, first_batch, count, vox, clip, mode, KeptOut{false, dev_points, capacity_points, {{"rows", dev_rows, 8}}}, out_count, stats);
}

int pcr_read_thin(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int mode, pcr_point *host_points,
                  int64_t *host_rows, size_t capacity_points, int64_t *out_count, pcr_thin_stats *stats)
{
    return thin_call(c, first_batch, count, vox, clip, mode, KeptOut{true, host_points, capacity_points, {{"rows", host_rows, 8}}}, out_count, stats);
}

// ---- levels of detail --------------------------------------------------------------------------
namespace {
// What lod_plan leaves for the writes: the counts per (listed batch, level) and the kernels' arguments
struct LodPlan {
    ThinPlan p;
    pcr_lod_stats st{};
    LodArgs a{};
    int64_t nL = 0;
    int classes = 0;                    // the levels written: L + 1, or L where the rest is dropped
    std::vector<int64_t> counts;        // [nL * (L + 1)]
    std::vector<int64_t> offsets;       // staging of the write kernel's offsets (alive until the stream has been synchronised)
};

// pcr_thin's FIRST plan on the lattice of lod_lattice, then the tables of the coarser levels, one after the other from the
// finest, each sized from the occupied slots of the one below, and the level byte of every winning row. Fills st up to
// level_count; st.runs == 0: nothing to do, no kernel has touched a table. Synchronises.
int lod_plan(pcr_ctx *c, int64_t first, int64_t n, const pcr_lod &lod, const pcr_box *clip, LodPlan &lp)
{
    const int L = lod.levels;
    VoxelPlan v;
    char limit[32];
    snprintf(limit, sizeof limit, "2^21 - %d", 1 << (L - 1));
    const VoxelTable table{nullptr, L == 1 ? "2^21" : limit, true, L};
    const pcr_voxels vox{{lod.origin[0], lod.origin[1], lod.origin[2]}, lod.cell};
    int rc = voxel_plan_begin(c, first, n, vox, clip, "order", table, 62, lp.p, v);      // (2^40 rows: never more than 2^41 slots)
    lp.st = pcr_lod_stats{v.batches_outside, v.batches_decoded, v.points_considered, v.runs, v.table_slots, 0, {}};
    lp.nL = v.nL;
    if (rc || v.runs == 0) return rc;
    const int64_t rows = n * PCR_POINTS_PER_BATCH;
    if (!thin_grow((void **)&c->d_lod_level, c->lod_level_rows, rows, 1))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the level bytes of %lld batches", (long long)n);
    if (!c->d_lod_occupied && hipMalloc((void **)&c->d_lod_occupied, PCR_LOD_MAX_LEVELS * 8) != hipSuccess)
        return set_err(c, PCR_E_NOMEM, "out of device memory for the counters of the levels");
    HIP_TRY(c, hipMemsetAsync(c->d_lod_level, 0xFF, (size_t)rows, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_lod_occupied, 0, PCR_LOD_MAX_LEVELS * 8, c->stream));

    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)v.nL), block(PCR_WORKGROUP_SIZE);
    if (v.windows) hipLaunchKernelGGL((k_thin_mark<LAYOUT_POINT_WINDOWS, PCR_THIN_FIRST>), grid, block, 0, c->stream, s, c->d_thin_list, v.a);
    else           hipLaunchKernelGGL((k_thin_mark<LAYOUT_WORDS, PCR_THIN_FIRST>), grid, block, 0, c->stream, s, c->d_thin_list, v.a);
    HIP_TRY(c, hipGetLastError());

    // occupied[l]: the voxels of level l. The error word travels with every counter: an overflow ends the call at its level.
    unsigned long long occupied[PCR_LOD_MAX_LEVELS] = {};
    uint32_t error = 0;
    auto mark = [&](const ThinSlot *t, int64_t slots, int l) -> int {
        hipLaunchKernelGGL(k_lod_mark, dim3((unsigned)std::min<int64_t>((slots + 255) / 256, 4096)), dim3(256), 0, c->stream, t, (unsigned long long)slots,
                           (unsigned long long)rows, (uint32_t)l, c->d_lod_level, c->d_lod_occupied + l);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&occupied[l], c->d_lod_occupied + l, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&error, c->d_thin_error, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (error) return set_err(c, PCR_E_NOMEM, "voxel table overflow at level %d: %lld slots", l, (long long)slots);
        return PCR_OK;
    };
    if ((rc = mark(c->d_thin_table, v.table_slots, L - 1))) return rc;
    // The tables of levels L - 2 .. 0 take turns in two halves of one allocation: a level has at most the voxels of the level
    // below it, so no table is larger than the first of them.
    const ThinSlot *src = c->d_thin_table;
    int64_t src_slots = v.table_slots, half = 0;
    for (int l = L - 2; l >= 0; --l) {
        uint32_t log2_slots = 10;
        while (((int64_t)1 << log2_slots) < 2 * (int64_t)occupied[l + 1]) ++log2_slots;
        const int64_t slots = (int64_t)1 << log2_slots;
        if (l == L - 2) {
            half = slots;
            if (!thin_grow((void **)&c->d_lod_tables, c->lod_slots, L > 2 ? 2 * half : half, sizeof(ThinSlot)))
                return set_err(c, PCR_E_NOMEM, "out of device memory for the voxel tables of the coarser levels (%lld slots): pass a clip or a larger cell",
                               (long long)(L > 2 ? 2 * half : half));
        }
        ThinSlot *dst = c->d_lod_tables + (((L - 2 - l) & 1) ? half : 0);
        HIP_TRY(c, hipMemsetAsync(dst, 0xFF, (size_t)slots * sizeof(ThinSlot), c->stream));
        ThinArgs a = v.a;
        a.log2_slots = log2_slots; a.table = dst;
        hipLaunchKernelGGL(k_lod_coarsen, dim3((unsigned)std::min<int64_t>((src_slots + 255) / 256, 4096)), dim3(256), 0, c->stream, src,
                           (unsigned long long)src_slots, a);
        HIP_TRY(c, hipGetLastError());
        if ((rc = mark(dst, slots, l))) return rc;
        src = dst; src_slots = slots;
    }
    lp.st.level_count[0] = (int64_t)occupied[0];
    for (int l = 1; l < L; ++l) lp.st.level_count[l] = (int64_t)occupied[l] - (int64_t)occupied[l - 1];
    lp.st.level_count[L] = v.points_considered - (int64_t)occupied[L - 1];
    lp.a.q = v.a.q; lp.a.first_batch = (uint32_t)first; lp.a.levels = (uint32_t)L; lp.a.level = c->d_lod_level;
    return PCR_OK;
}

// After lod_plan, for a call that writes: the final level bytes, the keep words and the counts per (listed batch, level); for
// PCR_LOD_ROW_ORDER the plan kept_write takes as well. A batch whose box lies inside the clip is not decoded. Synchronises.
int lod_count(pcr_ctx *c, int64_t first, const pcr_box *clip, bool row_order, LodPlan &lp)
{
    const int64_t nL = lp.nL, per = (int64_t)lp.a.levels + 1;
    std::vector<uint32_t> list(lp.p.listed);
    for (int64_t k = 0; clip && k < nL; ++k) {
        const int32_t *bb = c->h_point_bounds.data() + (int64_t)list[(size_t)k] * 6;
        bool within = true;
        for (int d = 0; d < 3; ++d) within = within && bb[d] >= clip->min[d] && bb[3 + d] <= clip->max[d];
        if (!within) list[(size_t)k] |= LOD_CUT;
    }
    if (!thin_grow((void **)&c->d_lod_list, c->lod_list_batches, nL, 4) || !thin_grow((void **)&c->d_lod_batch, c->lod_batch_words, nL * per, 8))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the lists of %lld batches", (long long)nL);
    HIP_TRY(c, hipMemcpyAsync(c->d_lod_list, list.data(), (size_t)nL * 4, hipMemcpyHostToDevice, c->stream));
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)nL), block(PCR_WORKGROUP_SIZE);
    if (select_reads_windows(c)) hipLaunchKernelGGL((k_lod_count<LAYOUT_POINT_WINDOWS>), grid, block, 0, c->stream, s, c->d_lod_list, lp.a, c->d_thin_keep, c->d_lod_batch);
    else                         hipLaunchKernelGGL((k_lod_count<LAYOUT_WORDS>), grid, block, 0, c->stream, s, c->d_lod_list, lp.a, c->d_thin_keep, c->d_lod_batch);
    HIP_TRY(c, hipGetLastError());
    lp.counts.assign((size_t)(nL * per), 0);
    HIP_TRY(c, hipMemcpyAsync(lp.counts.data(), c->d_lod_batch, (size_t)(nL * per) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // the two ways of counting a level agree, or nothing is written: the offsets below rest on these counts
    for (int64_t l = 0; l < per; ++l) {
        int64_t sum = 0;
        for (int64_t k = 0; k < nL; ++k) sum += lp.counts[(size_t)(k * per + l)];
        if (sum != lp.st.level_count[l])
            return set_err(c, PCR_E_HIP, "level %lld holds %lld records by batch and %lld by table", (long long)l, (long long)sum, (long long)lp.st.level_count[l]);
    }
    if (row_order)
        for (int64_t k = 0; k < nL; ++k) {
            int64_t m = 0;
            for (int l = 0; l < lp.classes; ++l) m += lp.counts[(size_t)(k * per + l)];
            if (m) { lp.p.writers.push_back(lp.p.listed[(size_t)k]); lp.p.cnt.push_back(m); }
        }
    (void)first;
    return PCR_OK;
}

// Enqueue the level-ordered write of listed batches [k0, k1): level l of them starts at record base[l] of the destinations d and
// takes room[l] records there; d holds `total` records. The caller synchronises.
int lod_emit(pcr_ctx *c, int64_t k0, int64_t k1, LodPlan &lp, const int64_t *base, int64_t total, const KeptOut &d)
{
    const int64_t per = (int64_t)lp.a.levels + 1;
    if (k0 == k1) return PCR_OK;
    lp.offsets.assign((size_t)((k1 - k0) * per), 0);
    int64_t at[LOD_CLASSES];
    for (int l = 0; l < LOD_CLASSES; ++l) at[l] = base[l];
    for (int64_t k = k0; k < k1; ++k)
        for (int l = 0; l < lp.classes; ++l) { lp.offsets[(size_t)((k - k0) * per + l)] = at[l]; at[l] += lp.counts[(size_t)(k * per + l)]; }
    HIP_TRY(c, hipMemcpyAsync(c->d_lod_batch + k0 * per, lp.offsets.data(), (size_t)((k1 - k0) * per) * 8, hipMemcpyHostToDevice, c->stream));
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)(k1 - k0)), block(PCR_WORKGROUP_SIZE);
    for_layout_bc7(c, [&](auto layout, auto bc7) {
        hipLaunchKernelGGL((k_lod_write<layout.value, bc7.value>), grid, block, 0, c->stream, s, c->d_lod_list + k0, lp.a, c->d_lod_batch + k0 * per,
                           (unsigned long long)total, static_cast<uint4 *>(d.points), static_cast<int64_t *>(d.col[0].dst), static_cast<uint8_t *>(d.col[1].dst));
    });
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

// The records in (level, row) order. On the device one launch over every listed batch; to the host in pieces of at most
// DECODE_STAGE_BATCHES batches of the range: a piece goes into the stages in its own (level, row) order, then each of its levels
// to the place behind the earlier pieces' records of that level. Synchronises.
int lod_write_levels(pcr_ctx *c, int64_t first, int64_t n, LodPlan &lp, const KeptOut &o)
{
    const int64_t per = (int64_t)lp.a.levels + 1, nL = lp.nL;
    int rc;
    int64_t base[LOD_CLASSES] = {};                 // where every level starts in the result
    for (int l = 1; l < lp.classes; ++l) base[l] = base[l - 1] + lp.st.level_count[l - 1];
    if (!o.host) {
        if ((rc = lod_emit(c, 0, nL, lp, base, lp.st.points_written, o))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return PCR_OK;
    }
    const int64_t piece = std::min<int64_t>(n, DECODE_STAGE_BATCHES);
    KeptOut d;
    if (const char *what = stage_reserve(c, o, piece, d))
        return set_err(c, PCR_E_NOMEM, "out of device memory for a staging buffer of %lld batches of %s", (long long)piece, what);
    int64_t k0 = 0;
    for (int64_t i0 = 0; i0 < n; i0 += piece) {
        const int64_t i1 = std::min(n, i0 + piece);
        int64_t k1 = k0;
        int64_t room[LOD_CLASSES] = {}, start[LOD_CLASSES] = {}, m = 0;
        for (; k1 < nL && lp.p.listed[(size_t)k1] < (uint32_t)(first + i1); ++k1)
            for (int l = 0; l < lp.classes; ++l) room[l] += lp.counts[(size_t)(k1 * per + l)];
        for (int l = 0; l < lp.classes; ++l) { start[l] = m; m += room[l]; }
        if (m) {
            if ((rc = lod_emit(c, k0, k1, lp, start, m, d))) return rc;
            for (int l = 0; l < lp.classes; ++l) {
                if (!room[l]) continue;
                if (d.points)
                    HIP_TRY(c, hipMemcpyAsync(static_cast<pcr_point *>(o.points) + base[l], static_cast<pcr_point *>(d.points) + start[l],
                                              (size_t)room[l] * sizeof(pcr_point), hipMemcpyDeviceToHost, c->stream));
                for (int i = 0; i < 2; ++i) {
                    const size_t row_bytes = o.col[i].row_bytes;
                    if (d.col[i].dst)
                        HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(o.col[i].dst) + (size_t)base[l] * row_bytes,
                                                  static_cast<char *>(d.col[i].dst) + (size_t)start[l] * row_bytes, (size_t)room[l] * row_bytes,
                                                  hipMemcpyDeviceToHost, c->stream));
                }
                base[l] += room[l];
            }
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        k0 = k1;
    }
    return PCR_OK;
}

// pcr_lod_order / pcr_read_lod_order
int lod_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_lod *lod, const pcr_box *clip, uint32_t flags, const KeptOut &o, int64_t *out_count,
             pcr_lod_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n = 0;
    bool done = true;
    KeptOut checked = o;
    checked.col[1].dst = nullptr;                   // (the levels are bytes: on the host any address will do)
    int rc = kept_begin(c, first, count, checked, out_count, &n);
    if (rc) return rc;
    if (!lod) return set_err(c, PCR_E_ARG, "the level-of-detail lattice is NULL");
    if (!o.host && o.col[1].dst && reinterpret_cast<uintptr_t>(o.col[1].dst) % 8 != 0)
        return set_err(c, PCR_E_ARG, "the destination of the levels is misaligned (8 bytes)");
    if (flags & ~(PCR_LOD_DROP_REST | PCR_LOD_ROW_ORDER)) return set_err(c, PCR_E_ARG, "flags 0x%x: only PCR_LOD_DROP_REST and PCR_LOD_ROW_ORDER are known", flags);
    if (lod->reserved != 0) return set_err(c, PCR_E_ARG, "pcr_lod::reserved is %d, not 0", lod->reserved);
    if (lod->levels < 1 || lod->levels > PCR_LOD_MAX_LEVELS)
        return set_err(c, PCR_E_ARG, "%d levels: the number of levels is 1 .. %d (PCR_LOD_MAX_LEVELS)", lod->levels, PCR_LOD_MAX_LEVELS);
    if (lod->cell < 1 || ((int64_t)lod->cell << (lod->levels - 1)) > PCR_THIN_MAX_CELL)
        return set_err(c, PCR_E_ARG, "finest cell of %d with %d levels: the coarsest edge length, cell << (levels - 1), is 1 .. %d (PCR_THIN_MAX_CELL)",
                       lod->cell, lod->levels, PCR_THIN_MAX_CELL);
    if ((rc = kept_row_limit(c, n, (int64_t)1 << 40, ROWS_2_40))) return rc;
    LodPlan lp;
    const bool drop = (flags & PCR_LOD_DROP_REST) != 0, row_order = (flags & PCR_LOD_ROW_ORDER) != 0;
    lp.classes = lod->levels + (drop ? 0 : 1);
    if ((rc = lod_plan(c, first, n, *lod, clip, lp))) return rc;
    lp.a.classes = (uint32_t)lp.classes;
    lp.st.points_written = lp.st.points_considered - (drop ? lp.st.level_count[lod->levels] : 0);
    if ((rc = kept_finish(c, o, lp.st.points_written, "to write", lp.st, out_count, stats, &done)) || done) return rc;
    if ((rc = lod_count(c, first, clip, row_order, lp))) return rc;
    if (!row_order) return lod_write_levels(c, first, n, lp, o);
    return kept_write(c, first, n, lp.p, o, [&](int64_t i0, int64_t i1, const KeptOut &d) {
        return kept_emit(c, first, i0, i1, lp.p, [&](auto layout, auto bc7, const EmitAt &e) {
            hipLaunchKernelGGL((k_lod_rows<layout.value, bc7.value>), e.grid, e.block, 0, c->stream, e.s, e.list, (uint32_t)first, c->d_thin_keep, e.offsets,
                               static_cast<uint4 *>(d.points), static_cast<int64_t *>(d.col[0].dst), c->d_lod_level, static_cast<uint8_t *>(d.col[1].dst));
        });
    }, true);
}
} // namespace

int pcr_lod_order(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_lod *lod, const pcr_box *clip, uint32_t flags, void *dev_points, void *dev_rows,
                  void *dev_levels, size_t capacity_points, int64_t *out_count, pcr_lod_stats *stats)
{
    return lod_call(c, first_batch, count, lod, clip, flags, KeptOut{false, dev_points, capacity_points, {{"rows", dev_rows, 8}, {"levels", dev_levels, 1}}},
                    out_count, stats);
}

int pcr_read_lod_order(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_lod *lod, const pcr_box *clip, uint32_t flags, pcr_point *host_points,
                       int64_t *host_rows, uint8_t *host_levels, size_t capacity_points, int64_t *out_count, pcr_lod_stats *stats)
{
    return lod_call(c, first_batch, count, lod, clip, flags, KeptOut{true, host_points, capacity_points, {{"rows", host_rows, 8}, {"levels", host_levels, 1}}},
                    out_count, stats);
}

// ---- voxel denoising ---------------------------------------------------------------------------
namespace {
// The second half of a plan on the lattice of noise_lattice, after the call's own kernels have left their verdict in bit 63 of every
// occupied slot's value: flag the rows on `mode`'s side of it (PCR_DENOISE_KEEP: bit clear), then the tail (voxel_plan_collect,
// which copies the call's counters). Synchronises.
int voxel_plan_finish(pcr_ctx *c, int64_t first, int mode, ThinPlan &p, VoxelPlan &v, void *dst, const void *src, size_t bytes)
{
    const ThinArgs &a = v.a;
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)v.nL), block(PCR_WORKGROUP_SIZE);
    // (every lane of a listed batch stores its keep word, and only listed batches are read: the bitmap needs no clearing)
#define PCR_LAUNCH(L, M) hipLaunchKernelGGL((k_denoise_flag<L, M>), grid, block, 0, c->stream, s, c->d_thin_list, a, c->d_thin_keep)
    if (v.windows) { if (mode == PCR_DENOISE_ISOLATED) PCR_LAUNCH(LAYOUT_POINT_WINDOWS, PCR_DENOISE_ISOLATED); else PCR_LAUNCH(LAYOUT_POINT_WINDOWS, PCR_DENOISE_KEEP); }
    else           { if (mode == PCR_DENOISE_ISOLATED) PCR_LAUNCH(LAYOUT_WORDS, PCR_DENOISE_ISOLATED); else PCR_LAUNCH(LAYOUT_WORDS, PCR_DENOISE_KEEP); }
#undef PCR_LAUNCH
    HIP_TRY(c, hipGetLastError());
    return voxel_plan_collect(c, first, p, v, dst, src, bytes);
}

// pcr_thin's phases with a sum in the table: classify, count the runs, count the candidates per voxel, decide per voxel, flag the
// rows to write and count them per batch. Fills the plan thin_emit takes (p.st is not used) and st. Synchronises.
int denoise_plan(pcr_ctx *c, int64_t first, int64_t n, const pcr_voxels &vox, const pcr_box *clip, int64_t max_count, int mode, ThinPlan &p,
                 pcr_denoise_stats &st)
{
    st = pcr_denoise_stats{};
    VoxelPlan v;
    int rc = voxel_plan_begin(c, first, n, vox, clip, "denoise", NOISE_TABLE, 62, p, v);
    st.batches_outside = v.batches_outside; st.batches_decoded = v.batches_decoded; st.points_considered = v.points_considered; st.runs = v.runs;
    if (rc || v.runs == 0) return rc;
    if (!c->d_denoise_counters && hipMalloc((void **)&c->d_denoise_counters, 16) != hipSuccess)
        return set_err(c, PCR_E_NOMEM, "out of device memory for two words");
    st.table_slots = v.table_slots;
    DenoiseArgs d{};
    d.t = v.a; d.max_count = (unsigned long long)max_count; d.counters = c->d_denoise_counters;
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)v.nL), block(PCR_WORKGROUP_SIZE);
    const dim3 per_slot((unsigned)std::min<int64_t>((v.table_slots + 255) / 256, 4096));
    unsigned long long counters[2] = {0, 0};
    HIP_TRY(c, hipMemsetAsync(c->d_denoise_counters, 0, 16, c->stream));
    if (v.windows) hipLaunchKernelGGL((k_denoise_count<LAYOUT_POINT_WINDOWS>), grid, block, 0, c->stream, s, c->d_thin_list, v.a);
    else           hipLaunchKernelGGL((k_denoise_count<LAYOUT_WORDS>), grid, block, 0, c->stream, s, c->d_thin_list, v.a);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_denoise_verdict, per_slot, dim3(256), 0, c->stream, d);
    HIP_TRY(c, hipGetLastError());
    if ((rc = voxel_plan_finish(c, first, mode, p, v, counters, c->d_denoise_counters, 16))) return rc;
    st.points_written = v.points_written;
    st.voxels = (int64_t)counters[0]; st.voxels_isolated = (int64_t)counters[1];
    st.points_isolated = mode == PCR_DENOISE_ISOLATED ? st.points_written : st.points_considered - st.points_written;
    return PCR_OK;
}

// pcr_denoise / pcr_read_denoise
int denoise_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int64_t max_count, int mode, const KeptOut &o,
                 int64_t *out_count, pcr_denoise_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ThinPlan p;
    pcr_denoise_stats st{};
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n, true, vox);
    if (rc) return rc;
    if (max_count < 0) return set_err(c, PCR_E_ARG, "max_count is %lld: 0 or more", (long long)max_count);
    if (mode != PCR_DENOISE_KEEP && mode != PCR_DENOISE_ISOLATED) return set_err(c, PCR_E_ARG, "mode is %d, not PCR_DENOISE_KEEP or PCR_DENOISE_ISOLATED", mode);
    if ((rc = kept_row_limit(c, n, (int64_t)1 << 40, ROWS_2_40)) || (rc = denoise_plan(c, first, n, *vox, clip, max_count, mode, p, st))) return rc;
    if ((rc = kept_finish(c, o, st.points_written, "to write", st, out_count, stats, &done)) || done) return rc;
    return thin_write(c, first, n, p, o);
}
} // namespace

int pcr_denoise(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int64_t max_count, int mode, void *dev_points,
                void *dev_rows, size_t capacity_points, int64_t *out_count, pcr_denoise_stats *stats)
{
    return denoise_call(c, first_batch, count, vox, clip, max_count, mode, KeptOut{false, dev_points, capacity_points, {{"rows", dev_rows, 8}}}, out_count, stats);
}

int pcr_read_denoise(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int64_t max_count, int mode,
                     pcr_point *host_points, int64_t *host_rows, size_t capacity_points, int64_t *out_count, pcr_denoise_stats *stats)
{
    return denoise_call(c, first_batch, count, vox, clip, max_count, mode, KeptOut{true, host_points, capacity_points, {{"rows", host_rows, 8}}}, out_count, stats);
}

// ---- connected components -----------------------------------------------------------------------
namespace {
// pcr_denoise's plan with a union-find between the counting and the flagging: count the candidates and the least row per voxel,
// unite adjacent voxels, point every slot at its root and sum the sizes there, mark the slots of small components. Fills the plan
// thin_emit takes, labels included, and st. Synchronises.
int components_plan(pcr_ctx *c, int64_t first, int64_t n, const pcr_voxels &vox, const pcr_box *clip, int connectivity, int64_t min_points, int mode,
                    ThinPlan &p, pcr_components_stats &st)
{
    st = pcr_components_stats{};
    VoxelPlan v;
    int rc = voxel_plan_begin(c, first, n, vox, clip, "label", NOISE_TABLE, 32, p, v);       // (the parent words are 32-bit)
    st.batches_outside = v.batches_outside; st.batches_decoded = v.batches_decoded; st.points_considered = v.points_considered; st.runs = v.runs;
    if (rc || v.runs == 0) return rc;
    const int64_t slots = v.table_slots;
    if (!thin_grow((void **)&c->d_components_scratch, c->components_slots, slots, 20))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the union-find over %lld slots (%lld runs): pass a clip or a larger cell", (long long)slots,
                       (long long)v.runs);
    if (!c->d_components_counters && hipMalloc((void **)&c->d_components_counters, 40) != hipSuccess)
        return set_err(c, PCR_E_NOMEM, "out of device memory for five words");
    st.table_slots = slots;
    ComponentsArgs g{};
    g.t = v.a;
    g.min_row = reinterpret_cast<thin_u64 *>(c->d_components_scratch);
    g.total = g.min_row + slots;
    g.parent = reinterpret_cast<uint32_t *>(g.total + slots);
    g.min_points = (unsigned long long)min_points; g.counters = c->d_components_counters; g.connectivity = connectivity;
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)v.nL), block(PCR_WORKGROUP_SIZE);
    const dim3 per_slot((unsigned)std::min<int64_t>((slots + 255) / 256, 4096));
    unsigned long long counters[5] = {0, 0, 0, 0, 0};
    HIP_TRY(c, hipMemsetAsync(c->d_components_counters, 0, 40, c->stream));
    hipLaunchKernelGGL(k_components_clear, per_slot, dim3(256), 0, c->stream, g);
    HIP_TRY(c, hipGetLastError());
    if (v.windows) hipLaunchKernelGGL((k_components_count<LAYOUT_POINT_WINDOWS>), grid, block, 0, c->stream, s, c->d_thin_list, v.a, g.min_row);
    else           hipLaunchKernelGGL((k_components_count<LAYOUT_WORDS>), grid, block, 0, c->stream, s, c->d_thin_list, v.a, g.min_row);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_components_link, per_slot, dim3(256), 0, c->stream, g);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_components_flatten, per_slot, dim3(256), 0, c->stream, g);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_components_verdict, per_slot, dim3(256), 0, c->stream, g);
    HIP_TRY(c, hipGetLastError());
    if ((rc = voxel_plan_finish(c, first, mode == PCR_COMPONENTS_SMALL ? PCR_DENOISE_ISOLATED : PCR_DENOISE_KEEP, p, v, counters, c->d_components_counters, 40)))
        return rc;
    st.points_written = v.points_written;
    st.voxels = (int64_t)counters[0]; st.components = (int64_t)counters[1]; st.components_small = (int64_t)counters[2];
    st.points_small = (int64_t)counters[3]; st.largest_points = (int64_t)counters[4];
    p.args = v.a; p.label = g.min_row;
    return PCR_OK;
}

// pcr_components / pcr_read_components
int components_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int connectivity, int64_t min_points, int mode,
                    const KeptOut &o, int64_t *out_count, pcr_components_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ThinPlan p;
    pcr_components_stats st{};
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n, true, vox);
    if (rc) return rc;
    if (connectivity != 6 && connectivity != 26) return set_err(c, PCR_E_ARG, "connectivity is %d, not 6 or 26", connectivity);
    if (min_points < 0) return set_err(c, PCR_E_ARG, "min_points is %lld: 0 or more", (long long)min_points);
    if (mode != PCR_COMPONENTS_KEEP && mode != PCR_COMPONENTS_SMALL) return set_err(c, PCR_E_ARG, "mode is %d, not PCR_COMPONENTS_KEEP or PCR_COMPONENTS_SMALL", mode);
    if ((rc = kept_row_limit(c, n, (int64_t)1 << 40, ROWS_2_40)) || (rc = components_plan(c, first, n, *vox, clip, connectivity, min_points, mode, p, st)))
        return rc;
    if ((rc = kept_finish(c, o, st.points_written, "to write", st, out_count, stats, &done)) || done) return rc;
    return thin_write(c, first, n, p, o);
}
} // namespace

int pcr_components(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int connectivity, int64_t min_points, int mode,
                   void *dev_points, void *dev_rows, void *dev_labels, size_t capacity_points, int64_t *out_count, pcr_components_stats *stats)
{
    return components_call(c, first_batch, count, vox, clip, connectivity, min_points, mode,
                           KeptOut{false, dev_points, capacity_points, {{"rows", dev_rows, 8}, {"labels", dev_labels, 8}}}, out_count, stats);
}

int pcr_read_components(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, int connectivity, int64_t min_points,
                        int mode, pcr_point *host_points, int64_t *host_rows, int64_t *host_labels, size_t capacity_points, int64_t *out_count,
                        pcr_components_stats *stats)
{
    return components_call(c, first_batch, count, vox, clip, connectivity, min_points, mode,
                           KeptOut{true, host_points, capacity_points, {{"rows", host_rows, 8}, {"labels", host_labels, 8}}}, out_count, stats);
}

// ---- radius neighbourhoods ----------------------------------------------------------------------
namespace {
// pcr_denoise's plan with the counts of the table turned into buckets: count the candidates per voxel and note the run starts,
// hand out buckets and work items, fill the buckets, test the pairs, count the rows to write per batch. want_n / want_nn2: the
// dense arrays a later neighbors_emit gathers from. Fills the plan neighbors_emit takes (p.st is not used) and st. Synchronises.
// mom (pcr_local_moments): the same sequence with k_moments_pairs in k_neighbors_pairs' place, which keeps the rows with N >=
// min_count and fills the dense pcr_moments / pcr_eigen records asked for; mode, want_n and want_nn2 are not used then.
// knn (pcr_knn): the same sequence with k_knn_pairs<K> there, K the least of 1, 2, 4, 8, 16 that holds k, which keeps the rows with
// found >= min_count (the call's min_found) and fills the dense words if asked for; mode, want_n and want_nn2 are not used then.
struct MomentsWant { bool moments, eigen; };
struct KnnWant { int k; bool words; };
int neighbors_plan(pcr_ctx *c, int64_t first, int64_t n, int32_t radius, const pcr_box *clip, int64_t min_count, int mode, bool want_n, bool want_nn2,
                   ThinPlan &p, pcr_neighbors_stats &st, const MomentsWant *mom = nullptr, const KnnWant *knn = nullptr)
{
    st = pcr_neighbors_stats{};
    VoxelPlan v;
    const pcr_voxels vox{{0, 0, 0}, radius};
    int rc = voxel_plan_begin(c, first, n, vox, clip, "search", NOISE_TABLE, 32, p, v, "radius");      // (a work item holds a 32-bit slot)
    st.batches_outside = v.batches_outside; st.batches_decoded = v.batches_decoded; st.points_considered = v.points_considered; st.runs = v.runs;
    if (rc || v.runs == 0) return rc;
    const int64_t slots = v.table_slots, nL = v.nL;
    const int64_t work_capacity = v.runs + v.points_considered / 64 + 1;      // the sum of ceil(count / 64) over at most `runs` voxels
    if (!thin_grow((void **)&c->d_neighbors_cursor, c->neighbors_slots, slots, sizeof(uint2)) ||
        !thin_grow((void **)&c->d_neighbors_starts, c->neighbors_chains, n * PCR_WORKGROUP_SIZE, 8) ||
        !thin_grow((void **)&c->d_neighbors_bucket, c->neighbors_candidates, v.points_considered, sizeof(uint4)) ||
        !thin_grow((void **)&c->d_neighbors_work, c->neighbors_work, work_capacity, 8) ||
        (want_n && !thin_grow((void **)&c->d_neighbors_n, c->neighbors_n_rows, n * PCR_POINTS_PER_BATCH, 8)) ||
        (want_nn2 && !thin_grow((void **)&c->d_neighbors_nn2, c->neighbors_nn2_rows, n * PCR_POINTS_PER_BATCH, 8)))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the index of %lld candidates in %lld slots: pass a clip or a larger radius",
                       (long long)v.points_considered, (long long)slots);
    if (mom && ((mom->moments && !thin_grow((void **)&c->d_moments_dense, c->moments_dense_rows, n * PCR_POINTS_PER_BATCH, sizeof(pcr_moments))) ||
                (mom->eigen && !thin_grow((void **)&c->d_moments_eigen, c->moments_eigen_rows, n * PCR_POINTS_PER_BATCH, sizeof(pcr_eigen)))))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the moments of %lld rows (%d bytes each): pass a clip or a shorter range",
                       (long long)(n * PCR_POINTS_PER_BATCH), (int)((mom->moments ? sizeof(pcr_moments) : 0) + (mom->eigen ? sizeof(pcr_eigen) : 0)));
    if (knn && knn->words && !thin_grow((void **)&c->d_knn_dense, c->knn_dense_words, n * PCR_POINTS_PER_BATCH * knn->k, 8))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the neighbours of %lld rows (%d bytes each): pass a clip or a shorter range",
                       (long long)(n * PCR_POINTS_PER_BATCH), knn->k * 8);
    if (!c->d_neighbors_counters && hipMalloc((void **)&c->d_neighbors_counters, NEIGHBORS_COUNTERS * 8) != hipSuccess)
        return set_err(c, PCR_E_NOMEM, "out of device memory for the counters");
    st.table_slots = slots;
    NeighborsArgs g{};
    g.t = v.a;
    g.cursor = c->d_neighbors_cursor; g.starts = c->d_neighbors_starts; g.bucket = c->d_neighbors_bucket; g.work = c->d_neighbors_work;
    g.counters = c->d_neighbors_counters;
    g.candidates = (unsigned long long)v.points_considered; g.work_capacity = (unsigned long long)work_capacity;
    g.rows = (unsigned long long)n * PCR_POINTS_PER_BATCH;
    g.r2 = (unsigned long long)radius * (unsigned long long)radius; g.min_count = (unsigned long long)min_count;
    g.mode = mode; g.early = mode != PCR_NEIGHBORS_ALL && !want_n && !want_nn2;
    g.keep = c->d_thin_keep; g.out_n = want_n ? c->d_neighbors_n : nullptr; g.out_nn2 = want_nn2 ? c->d_neighbors_nn2 : nullptr;
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)nL), block(PCR_WORKGROUP_SIZE);
    const dim3 per_slot((unsigned)std::min<int64_t>((slots + 255) / 256, 4096));      // (slots and 4096 * 256 are powers of two)
    unsigned long long counters[NEIGHBORS_COUNTERS] = {};
    HIP_TRY(c, hipMemsetAsync(c->d_neighbors_counters, 0, sizeof counters, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_thin_keep, 0, (size_t)n * PCR_WORKGROUP_SIZE * 8, c->stream));
    if (v.windows) hipLaunchKernelGGL((k_neighbors_count<LAYOUT_POINT_WINDOWS>), grid, block, 0, c->stream, s, c->d_thin_list, v.a, g.starts);
    else           hipLaunchKernelGGL((k_neighbors_count<LAYOUT_WORDS>), grid, block, 0, c->stream, s, c->d_thin_list, v.a, g.starts);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_neighbors_alloc, per_slot, dim3(256), 0, c->stream, g);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(counters, c->d_neighbors_counters, sizeof counters, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(v.totals.data() + nL * 2, c->d_thin_error, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t items = (int64_t)counters[NEIGHBORS_WORK_CURSOR];
    if (v.totals[(size_t)nL * 2] || (int64_t)counters[NEIGHBORS_BUCKET_CURSOR] != v.points_considered || items > work_capacity)
        return set_err(c, PCR_E_NOMEM, "voxel table overflow: %lld slots for %lld runs", (long long)slots, (long long)v.runs);
    if (v.windows) hipLaunchKernelGGL((k_neighbors_fill<LAYOUT_POINT_WINDOWS>), grid, block, 0, c->stream, s, c->d_thin_list, g);
    else           hipLaunchKernelGGL((k_neighbors_fill<LAYOUT_WORDS>), grid, block, 0, c->stream, s, c->d_thin_list, g);
    HIP_TRY(c, hipGetLastError());
    // (at most 16 384 workgroups: a wave walks the work list with the grid's stride and adds its statistics up in registers)
    const dim3 per_item((unsigned)std::min<int64_t>((items + 3) / 4, 16384));
    if (knn) {
        unsigned long long *const words = knn->words ? c->d_knn_dense : nullptr;
#define PCR_LAUNCH(K) hipLaunchKernelGGL((k_knn_pairs<K>), per_item, dim3(256), 0, c->stream, g, (unsigned long long)items, knn->k, words)
        if (knn->k <= 1) PCR_LAUNCH(1); else if (knn->k <= 2) PCR_LAUNCH(2); else if (knn->k <= 4) PCR_LAUNCH(4); else if (knn->k <= 8) PCR_LAUNCH(8); else PCR_LAUNCH(16);
#undef PCR_LAUNCH
    }
    else if (mom) hipLaunchKernelGGL(k_moments_pairs, per_item, dim3(256), 0, c->stream, g, (unsigned long long)items, mom->moments ? c->d_moments_dense : nullptr,
                                mom->eigen ? c->d_moments_eigen : nullptr);
    else     hipLaunchKernelGGL(k_neighbors_pairs, per_item, dim3(256), 0, c->stream, g, (unsigned long long)items);
    HIP_TRY(c, hipGetLastError());
    if ((rc = voxel_plan_collect(c, first, p, v, counters, c->d_neighbors_counters, sizeof counters))) return rc;
    st.points_written = v.points_written;
    st.voxels = (int64_t)counters[NEIGHBORS_VOXELS]; st.max_voxel_points = (int64_t)counters[NEIGHBORS_MAX_VOXEL];
    for (int k = 0; k < 64; ++k) { st.pairs_bound += (int64_t)counters[NEIGHBORS_PAIRS_BOUND + k]; st.points_sparse += (int64_t)counters[NEIGHBORS_SPARSE + k]; }
    return PCR_OK;
}

// The write of pcr_neighbors: the records, the rows (column 0) and, gathered from the dense arrays, N (1) and nn2 (2)
int neighbors_emit(pcr_ctx *c, int64_t first, int64_t i0, int64_t i1, ThinPlan &p, const KeptOut &d)
{
    return kept_emit(c, first, i0, i1, p, [&](auto layout, auto bc7, const EmitAt &e) {
        hipLaunchKernelGGL((k_neighbors_write<layout.value, bc7.value>), e.grid, e.block, 0, c->stream, e.s, e.list, (uint32_t)first, c->d_thin_keep, e.offsets,
                           c->d_neighbors_n, c->d_neighbors_nn2, static_cast<uint4 *>(d.points), static_cast<int64_t *>(d.col[0].dst),
                           static_cast<int64_t *>(d.col[1].dst), static_cast<unsigned long long *>(d.col[2].dst));
    });
}

// pcr_neighbors / pcr_read_neighbors
int neighbors_call(pcr_ctx *c, int64_t first, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count, int mode, const KeptOut &o,
                   int64_t *out_count, pcr_neighbors_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ThinPlan p;
    pcr_neighbors_stats st{};
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n);
    if (rc) return rc;
    if (radius < 1 || radius > PCR_NEIGHBORS_MAX_RADIUS)
        return set_err(c, PCR_E_ARG, "radius of %d: 1 .. %d stream units (PCR_NEIGHBORS_MAX_RADIUS)", radius, PCR_NEIGHBORS_MAX_RADIUS);
    if (min_count < 0) return set_err(c, PCR_E_ARG, "min_count is %lld: 0 or more", (long long)min_count);
    if (mode != PCR_NEIGHBORS_ALL && mode != PCR_NEIGHBORS_KEEP && mode != PCR_NEIGHBORS_SPARSE)
        return set_err(c, PCR_E_ARG, "mode is %d, not PCR_NEIGHBORS_ALL, PCR_NEIGHBORS_KEEP or PCR_NEIGHBORS_SPARSE", mode);
    if ((rc = kept_row_limit(c, n, (int64_t)1 << 32, ROWS_2_32_INDEX)) ||
        (rc = neighbors_plan(c, first, n, radius, clip, min_count, mode, o.col[1].dst != nullptr, o.col[2].dst != nullptr, p, st)))
        return rc;
    if ((rc = kept_finish(c, o, st.points_written, "to write", st, out_count, stats, &done)) || done) return rc;
    return kept_write(c, first, n, p, o, [&](int64_t i0, int64_t i1, const KeptOut &d) { return neighbors_emit(c, first, i0, i1, p, d); });
}
} // namespace

int pcr_neighbors(pcr_ctx *c, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count, int mode, void *dev_points,
                  void *dev_rows, void *dev_counts, void *dev_nn2, size_t capacity_points, int64_t *out_count, pcr_neighbors_stats *stats)
{
    return neighbors_call(c, first_batch, count, radius, clip, min_count, mode,
                          KeptOut{false, dev_points, capacity_points, {{"rows", dev_rows, 8}, {"counts", dev_counts, 8}, {"nearest distances", dev_nn2, 8}}},
                          out_count, stats);
}

int pcr_read_neighbors(pcr_ctx *c, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count, int mode,
                       pcr_point *host_points, int64_t *host_rows, int64_t *host_counts, uint64_t *host_nn2, size_t capacity_points, int64_t *out_count,
                       pcr_neighbors_stats *stats)
{
    return neighbors_call(c, first_batch, count, radius, clip, min_count, mode,
                          KeptOut{true, host_points, capacity_points, {{"rows", host_rows, 8}, {"counts", host_counts, 8}, {"nearest distances", host_nn2, 8}}},
                          out_count, stats);
}

// ---- local moments ------------------------------------------------------------------------------
namespace {
// The write of pcr_local_moments: the records, the rows (column 0) and, gathered from the dense arrays, the 80-byte pcr_moments (1)
// and the 48-byte pcr_eigen (2)
int moments_emit(pcr_ctx *c, int64_t first, int64_t i0, int64_t i1, ThinPlan &p, const KeptOut &d)
{
    return kept_emit(c, first, i0, i1, p, [&](auto layout, auto bc7, const EmitAt &e) {
        hipLaunchKernelGGL((k_moments_write<layout.value, bc7.value>), e.grid, e.block, 0, c->stream, e.s, e.list, (uint32_t)first, c->d_thin_keep, e.offsets,
                           reinterpret_cast<const unsigned long long *>(c->d_moments_dense), reinterpret_cast<const unsigned long long *>(c->d_moments_eigen),
                           static_cast<uint4 *>(d.points), static_cast<int64_t *>(d.col[0].dst), static_cast<unsigned long long *>(d.col[1].dst),
                           static_cast<unsigned long long *>(d.col[2].dst));
    });
}

// pcr_local_moments / pcr_read_local_moments: pcr_neighbors' checks with the radius limit of the exact sums, its plan with
// k_moments_pairs
int moments_call(pcr_ctx *c, int64_t first, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count, const KeptOut &o, int64_t *out_count,
                 pcr_neighbors_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ThinPlan p;
    pcr_neighbors_stats st{};
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n);
    if (rc) return rc;
    if (radius < 1 || radius > PCR_MOMENTS_MAX_RADIUS)
        return set_err(c, PCR_E_ARG, "radius of %d: 1 .. %d stream units (PCR_MOMENTS_MAX_RADIUS: the sums stay exact in 64 bits)", radius, PCR_MOMENTS_MAX_RADIUS);
    if (min_count < 0) return set_err(c, PCR_E_ARG, "min_count is %lld: 0 or more", (long long)min_count);
    const MomentsWant want{o.col[1].dst != nullptr, o.col[2].dst != nullptr};
    if ((rc = kept_row_limit(c, n, (int64_t)1 << 32, ROWS_2_32_INDEX)) ||
        (rc = neighbors_plan(c, first, n, radius, clip, min_count, PCR_NEIGHBORS_ALL, false, false, p, st, &want)))
        return rc;
    if ((rc = kept_finish(c, o, st.points_written, "to write", st, out_count, stats, &done)) || done) return rc;
    return kept_write(c, first, n, p, o, [&](int64_t i0, int64_t i1, const KeptOut &d) { return moments_emit(c, first, i0, i1, p, d); });
}
} // namespace

int pcr_local_moments(pcr_ctx *c, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count, void *dev_points,
                      void *dev_rows, void *dev_moments, void *dev_eigen, size_t capacity_points, int64_t *out_count, pcr_neighbors_stats *stats)
{
    return moments_call(c, first_batch, count, radius, clip, min_count,
                        KeptOut{false, dev_points, capacity_points,
                                {{"rows", dev_rows, 8}, {"moments", dev_moments, sizeof(pcr_moments)}, {"eigen records", dev_eigen, sizeof(pcr_eigen)}}},
                        out_count, stats);
}

int pcr_read_local_moments(pcr_ctx *c, int64_t first_batch, int64_t count, int32_t radius, const pcr_box *clip, int64_t min_count, pcr_point *host_points,
                           int64_t *host_rows, pcr_moments *host_moments, pcr_eigen *host_eigen, size_t capacity_points, int64_t *out_count,
                           pcr_neighbors_stats *stats)
{
    return moments_call(c, first_batch, count, radius, clip, min_count,
                        KeptOut{true, host_points, capacity_points,
                                {{"rows", host_rows, 8}, {"moments", host_moments, sizeof(pcr_moments)}, {"eigen records", host_eigen, sizeof(pcr_eigen)}}},
                        out_count, stats);
}

int pcr_moments_eigen(pcr_ctx *c, const void *dev_moments, int64_t n, void *dev_eigen)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (n < 0) return set_err(c, PCR_E_ARG, "n is %lld: 0 or more records", (long long)n);
    if (n == 0) return PCR_OK;
    if (!dev_moments || !dev_eigen) return set_err(c, PCR_E_ARG, "the moments / eigen records are NULL");
    if (reinterpret_cast<uintptr_t>(dev_moments) % 8 != 0 || reinterpret_cast<uintptr_t>(dev_eigen) % 8 != 0)
        return set_err(c, PCR_E_ARG, "the moments / eigen records are misaligned (8 bytes)");
    const int64_t per_launch = (int64_t)1 << 30;        // (a grid of at most 2^22 workgroups)
    for (int64_t i0 = 0; i0 < n; i0 += per_launch) {
        const int64_t m = std::min(per_launch, n - i0);
        hipLaunchKernelGGL(k_moments_eigen, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, static_cast<const int64_t *>(dev_moments) + i0 * 10,
                           (unsigned long long)m, static_cast<double *>(dev_eigen) + i0 * 6);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PCR_OK;
}

// ---- k nearest neighbours -----------------------------------------------------------------------
namespace {
// The write of pcr_knn: the records, the rows (column 0) and, gathered from the dense array, the k words of every row (1)
int knn_emit(pcr_ctx *c, int64_t first, int64_t i0, int64_t i1, ThinPlan &p, int k, const KeptOut &d)
{
    return kept_emit(c, first, i0, i1, p, [&](auto layout, auto bc7, const EmitAt &e) {
        hipLaunchKernelGGL((k_knn_write<layout.value, bc7.value>), e.grid, e.block, 0, c->stream, e.s, e.list, (uint32_t)first, c->d_thin_keep, e.offsets,
                           c->d_knn_dense, k, static_cast<uint4 *>(d.points), static_cast<int64_t *>(d.col[0].dst),
                           static_cast<unsigned long long *>(d.col[1].dst));
    });
}

// pcr_knn / pcr_read_knn: pcr_neighbors' checks with the limits of the 64-bit word, its plan with k_knn_pairs<K>. With min_found
// == 0 and no words asked for every candidate is kept whatever the pair kernel finds; it runs all the same, and pairs_bound comes
// from it as in every other call.
int knn_call(pcr_ctx *c, int64_t first, int64_t count, int k, int32_t radius, const pcr_box *clip, int64_t min_found, const KeptOut &o, int64_t *out_count,
             pcr_neighbors_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ThinPlan p;
    pcr_neighbors_stats st{};
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n);
    if (rc) return rc;
    if (k < 1 || k > PCR_KNN_MAX_K) return set_err(c, PCR_E_ARG, "k of %d: 1 .. %d (PCR_KNN_MAX_K)", k, PCR_KNN_MAX_K);
    if (radius < 1 || radius > PCR_KNN_MAX_RADIUS)
        return set_err(c, PCR_E_ARG, "radius of %d: 1 .. %d stream units (PCR_KNN_MAX_RADIUS: a squared distance and a row share 64 bits)", radius, PCR_KNN_MAX_RADIUS);
    if (min_found < 0 || min_found > k) return set_err(c, PCR_E_ARG, "min_found is %lld: 0 .. k = %d", (long long)min_found, k);
    const KnnWant want{k, o.col[1].dst != nullptr};
    if ((rc = kept_row_limit(c, n, (int64_t)1 << 32, ROWS_2_32_INDEX)) ||
        (rc = neighbors_plan(c, first, n, radius, clip, min_found, PCR_NEIGHBORS_ALL, false, false, p, st, nullptr, &want)))
        return rc;
    if ((rc = kept_finish(c, o, st.points_written, "to write", st, out_count, stats, &done)) || done) return rc;
    return kept_write(c, first, n, p, o, [&](int64_t i0, int64_t i1, const KeptOut &d) { return knn_emit(c, first, i0, i1, p, k, d); });
}
} // namespace

// (a row of the words column is k words: only a k that knn_call accepts reaches the stages)
int pcr_knn(pcr_ctx *c, int64_t first_batch, int64_t count, int k, int32_t radius, const pcr_box *clip, int64_t min_found, void *dev_points, void *dev_rows,
            void *dev_knn, size_t capacity_points, int64_t *out_count, pcr_neighbors_stats *stats)
{
    return knn_call(c, first_batch, count, k, radius, clip, min_found,
                    KeptOut{false, dev_points, capacity_points, {{"rows", dev_rows, 8}, {"neighbours", dev_knn, (size_t)k * 8}}}, out_count, stats);
}

int pcr_read_knn(pcr_ctx *c, int64_t first_batch, int64_t count, int k, int32_t radius, const pcr_box *clip, int64_t min_found, pcr_point *host_points,
                 int64_t *host_rows, uint64_t *host_knn, size_t capacity_points, int64_t *out_count, pcr_neighbors_stats *stats)
{
    return knn_call(c, first_batch, count, k, radius, clip, min_found,
                    KeptOut{true, host_points, capacity_points, {{"rows", host_rows, 8}, {"neighbours", host_knn, (size_t)k * 8}}}, out_count, stats);
}

// ---- voxel means -------------------------------------------------------------------------------
namespace {
// After thin_plan: the record index of every voxel into its slot, (key, row) of every record, and the sums of every voxel into
// its accumulator. Enqueues only; the error word (zero after thin_plan) is read by voxel_mean_check.
int voxel_mean_sums(pcr_ctx *c, int64_t first, int64_t n, ThinPlan &p)
{
    const int64_t records = p.st.points_kept, slots = p.st.table_slots;
    if (!thin_grow((void **)&c->d_voxel_prefix, c->voxel_prefix_words, n * PCR_WORKGROUP_SIZE, 8))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the record index of %lld batches: pass a shorter range", (long long)n);
    if (!thin_grow((void **)&c->d_voxel_acc, c->voxel_acc_records, records, VOXEL_ACC_WORDS * 8) ||
        !thin_grow((void **)&c->d_voxel_rec, c->voxel_rec_records, records, sizeof(VoxelRec)))
        return set_err(c, PCR_E_NOMEM, "out of device memory for the sums of %lld voxels (80 bytes each): pass a clip or a larger cell", (long long)records);
    EmitAt e;                                       // every writer of the range: there is one, records > 0
    const int rc = emit_offsets(c, first, 0, n, p, e);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_voxel_acc, 0, (size_t)records * VOXEL_ACC_WORDS * 8, c->stream));
    hipLaunchKernelGGL(k_voxel_prefix, e.grid, e.block, 0, c->stream, e.list, (uint32_t)first, c->d_thin_keep, e.offsets, c->d_voxel_prefix);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_voxel_index, dim3((unsigned)std::min<int64_t>((slots + 255) / 256, 4096)), dim3(256), 0, c->stream, c->d_thin_table,
                       (unsigned long long)slots, c->d_thin_keep, c->d_voxel_prefix, (unsigned long long)records, c->d_voxel_rec, c->d_thin_error);
    HIP_TRY(c, hipGetLastError());
    const dim3 grid((unsigned)p.listed.size());
    for_layout_bc7(c, [&](auto layout, auto bc7) {
        hipLaunchKernelGGL((k_voxel_sum<layout.value, bc7.value>), grid, e.block, 0, c->stream, e.s, c->d_thin_list, p.args, (unsigned long long)records,
                           c->d_voxel_acc);
    });
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

// Enqueue the roundings and stores of records [i0, i1): the points, the rows (column 0) and the counts (1) to device destinations
// of i1 - i0 records, any may be NULL
int voxel_mean_emit(pcr_ctx *c, const ThinPlan &p, int64_t i0, int64_t i1, const KeptOut &d)
{
    hipLaunchKernelGGL(k_voxel_finish, dim3((unsigned)std::min<int64_t>((i1 - i0 + 255) / 256, 4096)), dim3(256), 0, c->stream, p.args.lat, c->d_voxel_acc,
                       c->d_voxel_rec, (unsigned long long)i0, (unsigned long long)i1, static_cast<uint4 *>(d.points), static_cast<int64_t *>(d.col[0].dst),
                       static_cast<int64_t *>(d.col[1].dst), c->d_thin_error);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

// Synchronises; the error word of the call's kernels: the table, the bitmap and the accumulators disagree (cannot happen)
int voxel_mean_check(pcr_ctx *c)
{
    uint32_t error = 0;
    HIP_TRY(c, hipMemcpyAsync(&error, c->d_thin_error, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (error) return set_err(c, PCR_E_NOMEM, "voxel table and record index disagree");
    return PCR_OK;
}

// pcr_voxel_mean / pcr_read_voxel_mean: pcr_thin's FIRST plan, unchanged, then the sums and one computed record per voxel. The
// records are not rows of batches, so the host form walks them in pieces of its own, through the same stages.
int voxel_mean_call(pcr_ctx *c, int64_t first, int64_t count, const pcr_voxels *vox, const pcr_box *clip, const KeptOut &o, int64_t *out_count,
                    pcr_thin_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ThinPlan p;
    int64_t n = 0;
    bool done = true;
    int rc = kept_begin(c, first, count, o, out_count, &n, true, vox);
    if (rc) return rc;
    if ((rc = kept_row_limit(c, n, PCR_VOXEL_MEAN_MAX_ROWS, "2^32 rows (the 64-bit sums of a voxel are exact up to there): pass a shorter range")) ||
        (rc = thin_plan(c, first, n, *vox, clip, PCR_THIN_FIRST, p)))
        return rc;
    if ((rc = kept_finish(c, o, p.st.points_kept, "voxels", p.st, out_count, stats, &done)) || done) return rc;
    const int64_t records = p.st.points_kept;
    KeptOut d = o;
    int64_t piece = records;                        // on the device: all at once
    if (o.host) {
        // pieces of at most DECODE_STAGE_BATCHES * 65 536 records through the stages
        const int64_t piece_batches = std::min<int64_t>((records + PCR_POINTS_PER_BATCH - 1) / PCR_POINTS_PER_BATCH, DECODE_STAGE_BATCHES);
        piece = piece_batches * PCR_POINTS_PER_BATCH;
        if (stage_reserve(c, o, piece_batches, d)) return set_err(c, PCR_E_NOMEM, "out of device memory for the staging buffers of %lld records", (long long)piece);
    }
    if ((rc = voxel_mean_sums(c, first, n, p))) return rc;
    for (int64_t i0 = 0; i0 < records; i0 += piece) {
        const int64_t i1 = std::min(records, i0 + piece);
        if ((rc = voxel_mean_emit(c, p, i0, i1, d)) || (o.host && (rc = stage_copy(c, o, d, i0, i1 - i0)))) return rc;
    }
    return voxel_mean_check(c);
}
} // namespace

int pcr_voxel_mean(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, void *dev_points, void *dev_rows,
                   void *dev_counts, size_t capacity_points, int64_t *out_count, pcr_thin_stats *stats)
{
    return voxel_mean_call(c, first_batch, count, vox, clip, KeptOut{false, dev_points, capacity_points, {{"rows", dev_rows, 8}, {"counts", dev_counts, 8}}},
                           out_count, stats);
}

int pcr_read_voxel_mean(pcr_ctx *c, int64_t first_batch, int64_t count, const pcr_voxels *vox, const pcr_box *clip, pcr_point *host_points,
                        int64_t *host_rows, int64_t *host_counts, size_t capacity_points, int64_t *out_count, pcr_thin_stats *stats)
{
    return voxel_mean_call(c, first_batch, count, vox, clip, KeptOut{true, host_points, capacity_points, {{"rows", host_rows, 8}, {"counts", host_counts, 8}}},
                           out_count, stats);
}

// ---- screen selection and picking --------------------------------------------------------------
namespace {
// What a screen selection has to write: the batches the prepass keeps for the camera (ascending, with their LOD words; their
// per-chain counts sit in c->scr.counts in the same order) and each one's record count.
struct ScreenPlan {
    std::vector<ScreenEntry> kept;
    std::vector<int64_t> cnt;
    std::vector<int64_t> offsets;       // listed_write's
    ScreenArgs q{};
    pcr_screen_stats st{};
};

// The rect clipped to the image into q; false: nothing is left of it.
bool screen_clip(const pcr_render_params *p, int64_t x0, int64_t y0, int64_t x1, int64_t y1, ScreenArgs &q)
{
    x0 = std::max<int64_t>(x0, 0); y0 = std::max<int64_t>(y0, 0);
    x1 = std::min<int64_t>(x1, p->width - 1); y1 = std::min<int64_t>(y1, p->height - 1);
    if (x0 > x1 || y0 > y1) return false;
    q.x0 = (int32_t)x0; q.y0 = (int32_t)y0; q.x1 = (int32_t)x1; q.y1 = (int32_t)y1;
    return true;
}

// The kept batches of the camera (k_screen_lod, read back: synchronises) and the scratch for them. nB resident batches, > 0.
int screen_list(pcr_ctx *c, const pcr_render_params *p, int64_t nB, ScreenPlan &pl)
{
    int rc;
    // (as a frame: the provisional last batch of a stream that is still loading is walked here if no frame has done so)
    if (!c->async_upload && (rc = enqueue_transcode(c, true, c->stream))) return rc;
    std::memcpy(pl.q.m, p->transform, sizeof pl.q.m);
    pl.q.width = p->width; pl.q.height = p->height; pl.q.fb_elems = (uint32_t)c->fb_elems;
    if (!c->d_screen_lod) HIP_TRY(c, hipMalloc((void **)&c->d_screen_lod, (size_t)c->hdr.num_batches * sizeof(uint32_t)));
    const RenderArgs a = make_args(c, p, 0);                // the basic method's LOD expression; only a.p and a.s.batches are read
    hipLaunchKernelGGL(k_screen_lod, dim3((unsigned)((nB + PREPASS_BATCHES - 1) / PREPASS_BATCHES)), dim3(PREPASS_THREADS), 0, c->stream, a, c->d_screen_lod);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> lod((size_t)nB);
    HIP_TRY(c, hipMemcpyAsync(lod.data(), c->d_screen_lod, (size_t)nB * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    pl.kept.clear();
    for (int64_t b = 0; b < nB; ++b) {
        const uint32_t w = lod[(size_t)b];
        if ((w & LOD_CULLED) || !(w & LOD_NPR_MASK)) continue;
        pl.kept.push_back(ScreenEntry{(uint32_t)b, w});
        pl.st.points_tested += (int64_t)(w & LOD_NPR_MASK) * PCR_WORKGROUP_SIZE;
    }
    const int64_t nK = (int64_t)pl.kept.size();
    pl.st.batches_decoded = nK; pl.st.batches_skipped = nB - nK;
    if (nK == 0) return PCR_OK;
    if ((rc = scratch_reserve(c, c->scr, nK, "kept batches (their counts)"))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->scr.list, pl.kept.data(), (size_t)nK * sizeof(ScreenEntry), hipMemcpyHostToDevice, c->stream));
    return PCR_OK;
}

// Count the kept batches' selected points (k_screen_count). Synchronises.
int screen_count(pcr_ctx *c, ScreenPlan &pl)
{
    const int64_t nK = (int64_t)pl.kept.size();
    pl.cnt.assign((size_t)nK, 0);
    if (nK == 0) return PCR_OK;
    for_layout(c, [&](auto layout) {
        hipLaunchKernelGGL((k_screen_count<layout.value>), dim3((unsigned)nK), dim3(PCR_WORKGROUP_SIZE), 0, c->stream, make_stream_view(c), c->scr.list, pl.q,
                           c->scr.counts, c->scr.totals);
    });
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> totals((size_t)nK);
    HIP_TRY(c, hipMemcpyAsync(totals.data(), c->scr.totals, (size_t)nK * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < nK; ++k) { pl.cnt[(size_t)k] = totals[(size_t)k]; pl.st.points_selected += totals[(size_t)k]; }
    return PCR_OK;
}

// The rect of a call (NULL: the image) clipped to the image into q; false: nothing is left of it.
bool screen_rect(const pcr_render_params *p, const pcr_rect *rect, ScreenArgs &q)
{
    return rect ? screen_clip(p, rect->x0, rect->y0, rect->x1, rect->y1, q) : screen_clip(p, 0, 0, p->width - 1, p->height - 1, q);
}

// pcr_select_screen / pcr_read_screen: the records to o.points, their hits to column 0
int screen_call(pcr_ctx *c, const pcr_render_params *p, const pcr_rect *rect, const KeptOut &o, int64_t *out_count, pcr_screen_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ScreenPlan pl;
    int64_t nB = 0;
    bool done = true;
    int rc = kept_begin(c, 0, -1, o, out_count, &nB);                           // (the range: every resident batch)
    if (rc || (rc = check_params(c, p))) return rc;
    pl.st = pcr_screen_stats{nB, 0, 0, 0};
    if (screen_rect(p, rect, pl.q) && nB > 0 && ((rc = screen_list(c, p, nB, pl)) || (rc = screen_count(c, pl)))) return rc;
    if ((rc = kept_finish(c, o, pl.st.points_selected, "selected", pl.st, out_count, stats, &done)) || done) return rc;
    return listed_write(c, pl.cnt, pl.offsets, c->scr.offsets, o, [&](int64_t k0, dim3 grid, const KeptOut &d) {
        for_layout_bc7(c, [&](auto layout, auto bc7) {
            hipLaunchKernelGGL((k_screen_write<layout.value, bc7.value>), grid, dim3(PCR_WORKGROUP_SIZE), 0, c->stream, make_stream_view(c), c->scr.list + k0, pl.q,
                               c->scr.counts + k0 * PCR_WORKGROUP_SIZE, c->scr.offsets + k0, static_cast<uint4 *>(d.points), static_cast<uint4 *>(d.col[0].dst));
        });
    });
}
} // namespace

int pcr_select_screen(pcr_ctx *c, const pcr_render_params *p, const pcr_rect *rect, void *dev_points, void *dev_hits, size_t capacity,
                      int64_t *out_count, pcr_screen_stats *stats)
{
    return screen_call(c, p, rect, KeptOut{false, dev_points, capacity, {hits_column(dev_hits)}}, out_count, stats);
}

int pcr_read_screen(pcr_ctx *c, const pcr_render_params *p, const pcr_rect *rect, pcr_point *host_points, pcr_screen_hit *host_hits,
                    size_t capacity, int64_t *out_count, pcr_screen_stats *stats)
{
    return screen_call(c, p, rect, KeptOut{true, host_points, capacity, {hits_column(host_hits)}}, out_count, stats);
}

int pcr_pick(pcr_ctx *c, const pcr_render_params *p, int px, int py, int radius, pcr_point *out_point, pcr_screen_hit *out_hit, int *out_found)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (out_found) *out_found = 0;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!out_found) return set_err(c, PCR_E_ARG, "out_found is NULL");
    if (radius < 0) return set_err(c, PCR_E_ARG, "radius must be >= 0");
    if (c->async_upload) poll_loader(c, false);
    const int64_t nB = c->visible_batches();
    ScreenPlan pl;
    if (nB == 0 || !screen_clip(p, (int64_t)px - radius, (int64_t)py - radius, (int64_t)px + radius, (int64_t)py + radius, pl.q)) return PCR_OK;
    if ((rc = screen_list(c, p, nB, pl))) return rc;
    const int64_t nK = (int64_t)pl.kept.size();
    if (nK == 0) return PCR_OK;
    if (!c->d_pick) HIP_TRY(c, hipMalloc((void **)&c->d_pick, PICK_WORDS * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemsetAsync(c->d_pick, 0xFF, PICK_WORDS * sizeof(unsigned long long), c->stream));
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)nK), block(PCR_WORKGROUP_SIZE);
    for_layout_bc7(c, [&](auto layout, auto bc7) {
        hipLaunchKernelGGL((k_pick<layout.value, bc7.value, false>), grid, block, 0, c->stream, s, c->scr.list, pl.q, c->d_pick);
        hipLaunchKernelGGL((k_pick<layout.value, bc7.value, true>), grid, block, 0, c->stream, s, c->scr.list, pl.q, c->d_pick);
        hipLaunchKernelGGL((k_pick_fetch<layout.value, bc7.value>), dim3(1), block, 0, c->stream, s, c->d_screen_lod, pl.q, c->d_pick);
    });
    HIP_TRY(c, hipGetLastError());
    unsigned long long h[PICK_WORDS];
    HIP_TRY(c, hipMemcpyAsync(h, c->d_pick, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h[1] == PICK_NONE) return PCR_OK;
    *out_found = 1;
    if (out_point) std::memcpy(out_point, &h[2], sizeof *out_point);
    if (out_hit) std::memcpy(out_hit, &h[4], sizeof *out_hit);
    return PCR_OK;
}

// ---- visible selection ---------------------------------------------------------------------------
namespace {
// What pcr_select_visible / pcr_read_visible share: the screen selection's plan (kept batches, ScreenArgs; pl.cnt = the selected
// hits per kept batch) and the call's mode. The depth plane of the call is in c->d_vis_depth.
struct VisiblePlan {
    ScreenPlan pl;
    bool front = true;
    pcr_visible_stats st{};
};

// The planes for an image of npix pixels, and the totals of nK kept batches
int visible_scratch(pcr_ctx *c, size_t npix, int64_t nK)
{
    if (c->vis_pixels < npix) {
        dfree(c->d_vis_key); dfree(c->d_vis_index); dfree(c->d_vis_row); dfree(c->d_vis_depth); c->vis_pixels = 0;
        if (hipMalloc((void **)&c->d_vis_key, (npix + 1) * 8) != hipSuccess || hipMalloc((void **)&c->d_vis_index, npix * 8) != hipSuccess ||
            hipMalloc((void **)&c->d_vis_row, npix * 4) != hipSuccess || hipMalloc((void **)&c->d_vis_depth, npix * 4) != hipSuccess)
            return set_err(c, PCR_E_NOMEM, "out of device memory for the planes of %zu pixels", npix);
        c->vis_pixels = npix;
    }
    return nK ? reserve(c, c->d_vis_totals, c->vis_capacity, nK * 3, "totals of the kept batches (three each)") : (int)PCR_OK;
}

// pcr_select_visible / pcr_read_visible: the planes, the counts, then the records to o.points and their hits to column 0. The
// depth plane goes to `depth` (memory of the form's side) unless the call is refused.
int visible_call(pcr_ctx *c, const pcr_render_params *p, const pcr_rect *rect, int mode, int radius, const KeptOut &o, void *depth, int64_t *out_count,
                 pcr_visible_stats *stats)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    VisiblePlan vp;
    ScreenPlan &pl = vp.pl;
    int64_t nB = 0;
    bool done = true;
    int rc = kept_begin(c, 0, -1, o, out_count, &nB);                           // (the range: every resident batch)
    if (rc || (rc = check_params(c, p))) return rc;
    if (mode != PCR_VISIBLE_FRONT && mode != PCR_VISIBLE_SURFACE) return set_err(c, PCR_E_ARG, "unknown mode %d (PCR_VISIBLE_FRONT or PCR_VISIBLE_SURFACE)", mode);
    if (radius < 0 || radius > PCR_VISIBLE_MAX_RADIUS) return set_err(c, PCR_E_ARG, "radius must be 0 .. %d", PCR_VISIBLE_MAX_RADIUS);
    if (depth && reinterpret_cast<uintptr_t>(depth) % alignof(uint32_t) != 0) return set_err(c, PCR_E_ARG, "the destination of the depth plane is misaligned (4 bytes)");
    const size_t npix = (size_t)p->width * (size_t)p->height;
    vp.front = mode == PCR_VISIBLE_FRONT;
    vp.st = pcr_visible_stats{nB, 0, 0, 0, 0, 0};
    const bool some = screen_rect(p, rect, pl.q);
    if (nB > 0 && (rc = screen_list(c, p, nB, pl))) return rc;
    const int64_t nK = (int64_t)pl.kept.size();
    vp.st.batches_decoded = nK; vp.st.batches_skipped = nB - nK;
    pl.cnt.assign((size_t)nK, 0);
    if ((rc = visible_scratch(c, npix, nK))) return rc;
    // the planes: empty, then the keys of every hit of the image, then the dilated depth
    unsigned long long *const d_covered = c->d_vis_key + npix;
    HIP_TRY(c, hipMemsetAsync(c->d_vis_key, 0xFF, npix * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_covered, 0, 8, c->stream));
    const StreamView s = make_stream_view(c);
    const dim3 grid((unsigned)nK), block(PCR_WORKGROUP_SIZE);
    uint32_t *const d_hit_totals = c->d_vis_totals, *const d_totals = c->d_vis_totals + nK;
    if (nK > 0) {
        // (SURFACE reads the keys' depth halves only: the colourless decode)
        for_layout_colour(c, vp.front, [&](auto layout, auto colour) {
            hipLaunchKernelGGL((k_visible_key<layout.value, colour.value>), grid, block, 0, c->stream, s, c->scr.list, pl.q, c->d_vis_key, d_hit_totals);
        });
        HIP_TRY(c, hipGetLastError());
    }
    const dim3 dgrid((unsigned)std::min<size_t>((npix + VIS_DILATE_THREADS - 1) / VIS_DILATE_THREADS, 4096)), dblock(VIS_DILATE_THREADS);
    hipLaunchKernelGGL((k_visible_dilate<true>), dgrid, dblock, 0, c->stream, c->d_vis_key, (const uint32_t *)nullptr, c->d_vis_row, p->width, p->height, radius, d_covered);
    hipLaunchKernelGGL((k_visible_dilate<false>), dgrid, dblock, 0, c->stream, c->d_vis_key, c->d_vis_row, c->d_vis_depth, p->width, p->height, radius, d_covered);
    HIP_TRY(c, hipGetLastError());
    const bool count = some && nK > 0;
    if (count) {
        if (vp.front) {
            HIP_TRY(c, hipMemsetAsync(c->d_vis_index, 0xFF, npix * 8, c->stream));
            for_layout_bc7(c, [&](auto layout, auto bc7) {
                hipLaunchKernelGGL((k_visible_index<layout.value, bc7.value>), grid, block, 0, c->stream, s, c->scr.list, pl.q, c->d_vis_key, c->d_vis_index);
            });
        }
        for_layout(c, [&](auto layout) {
            hipLaunchKernelGGL((k_visible_count<layout.value>), grid, block, 0, c->stream, s, c->scr.list, pl.q, vp.front, c->d_vis_depth, c->d_vis_index,
                               c->scr.counts, d_totals);
        });
        HIP_TRY(c, hipGetLastError());
    }
    std::vector<uint32_t> totals((size_t)nK * 3);
    unsigned long long covered = 0;
    if (nK > 0) HIP_TRY(c, hipMemcpyAsync(totals.data(), c->d_vis_totals, (size_t)nK * (count ? 3 : 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&covered, d_covered, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    vp.st.pixels_covered = (int64_t)covered;
    for (int64_t k = 0; k < nK; ++k) {
        vp.st.hits += totals[(size_t)k];
        if (!count) continue;
        pl.cnt[(size_t)k] = totals[(size_t)(nK + 2 * k)];
        vp.st.selected += totals[(size_t)(nK + 2 * k)];
        vp.st.candidates += totals[(size_t)(nK + 2 * k + 1)];
    }
    if ((rc = kept_finish(c, o, vp.st.selected, "selected", vp.st, out_count, stats, &done))) return rc;
    if (depth) {
        HIP_TRY(c, hipMemcpyAsync(depth, c->d_vis_depth, npix * 4, hipMemcpyDefault, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (done) return PCR_OK;
    return listed_write(c, pl.cnt, pl.offsets, c->scr.offsets, o, [&](int64_t k0, dim3 wgrid, const KeptOut &d) {
        for_layout_bc7(c, [&](auto layout, auto bc7) {
            hipLaunchKernelGGL((k_visible_write<layout.value, bc7.value>), wgrid, block, 0, c->stream, s, c->scr.list + k0, pl.q, vp.front, c->d_vis_depth,
                               c->d_vis_index, c->scr.counts + k0 * PCR_WORKGROUP_SIZE, c->scr.offsets + k0, static_cast<uint4 *>(d.points),
                               static_cast<uint4 *>(d.col[0].dst));
        });
    });
}
} // namespace

int pcr_select_visible(pcr_ctx *c, const pcr_render_params *p, const pcr_rect *rect, int mode, int radius, void *dev_points, void *dev_hits, void *dev_depth,
                       size_t capacity, int64_t *out_count, pcr_visible_stats *stats)
{
    return visible_call(c, p, rect, mode, radius, KeptOut{false, dev_points, capacity, {hits_column(dev_hits)}}, dev_depth, out_count, stats);
}

int pcr_read_visible(pcr_ctx *c, const pcr_render_params *p, const pcr_rect *rect, int mode, int radius, pcr_point *host_points, pcr_screen_hit *host_hits,
                     uint32_t *host_depth, size_t capacity, int64_t *out_count, pcr_visible_stats *stats)
{
    return visible_call(c, p, rect, mode, radius, KeptOut{true, host_points, capacity, {hits_column(host_hits)}}, host_depth, out_count, stats);
}

// ---- multi-GPU plumbing ------------------------------------------------------------------------
void *pcr_get_stream(pcr_ctx *c) { return c ? (void *)c->stream : nullptr; }
int pcr_get_device(const pcr_ctx *c) { return c ? c->device : -1; }
size_t pcr_framebuffer_elems(const pcr_ctx *c) { return c ? c->fb_elems : 0; }
size_t pcr_framebuffer_capacity(const pcr_ctx *c)
{
    if (!c || !c->fb) return 0;
    return (c->fb == c->own_fb && c->rg == c->own_rg && c->ba == c->own_ba) ? c->fb_alloc : c->fb_elems;
}
void *pcr_device_rgba(pcr_ctx *c) { return c ? c->d_rgba : nullptr; }
// (whoever asks for these may write through them -- a collective merging partial frames in place: no tile flags until the next clear)
static void expose(pcr_ctx *c) { if (c) { c->tiles_tracked = false; c->fb_exposed = true; } }
void *pcr_device_framebuffer(pcr_ctx *c) { expose(c); return c ? c->fb : nullptr; }
void *pcr_device_rg(pcr_ctx *c) { expose(c); return c ? c->rg : nullptr; }
void *pcr_device_ba(pcr_ctx *c) { expose(c); return c ? c->ba : nullptr; }
int pcr_framebuffer_private(pcr_ctx *c)
{
    if (!c) return PCR_E_ARG;
    c->fb_exposed = false; c->tiles_tracked = false;        // (tracking resumes with the next full clear)
    return PCR_OK;
}

int pcr_use_external_buffers(pcr_ctx *c, void *fb, void *rg, void *ba)
{
    if (!c) return PCR_E_ARG;
    c->prepass_ready = false;        // what pcr_frame_begin prepared no longer matches the context's state
    if (!c->own_fb) return set_err(c, PCR_E_ARG, "call pcr_set_image_size first");
    // pointers are captured by value at enqueue time: switching them does not disturb work already enqueued
    uint64_t *nrg = rg ? (uint64_t *)rg : c->own_rg, *nba = ba ? (uint64_t *)ba : c->own_ba;
    if (nrg != c->rg || nba != c->ba) c->accum_dirty = true;     // unknown contents: the next pcr_clear zeroes them
    c->fb = fb ? (uint64_t *)fb : c->own_fb;
    c->rg = nrg;
    c->ba = nba;
    c->tiles_tracked = false;
    return PCR_OK;
}

int pcr_merge_min_slices(pcr_ctx *c, void *slices, int nslices, size_t slice_elems)
{
    if (!c || !slices || nslices < 1 || slice_elems == 0) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (nslices > 1) {
        // few workgroups: this runs next to a render, whose 1024-thread workgroups wait for whole CUs' worth of wave slots
        hipLaunchKernelGGL(k_merge_min_slices, dim3(128), dim3(256), 0, c->stream, (uint64_t *)slices, nslices, slice_elems);
        HIP_TRY(c, hipGetLastError());
    }
    return PCR_OK;
}

int pcr_resolve_basic_range(pcr_ctx *c, const pcr_render_params *p, const void *fb, size_t count, void *rgba)
{
    if (!c || !p || !fb || !rgba) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (count == 0) return PCR_OK;
    hipLaunchKernelGGL(k_resolve_range, dim3(128), dim3(256), 0, c->stream, p->show_num_points, p->colorize_chunks,
                       (const uint64_t *)fb, count, (uint32_t *)rgba);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_resolve_hqs_range(pcr_ctx *c, const pcr_render_params *p, const void *fb, const void *rg, const void *ba, size_t count, void *rgba)
{
    if (!c || !p || !fb || !rg || !ba || !rgba) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (count == 0) return PCR_OK;
    hipLaunchKernelGGL(k_resolve_range_hqs, dim3(128), dim3(256), 0, c->stream, p->show_num_points, p->colorize_chunks,
                       (const uint64_t *)fb, (const uint64_t *)rg, (const uint64_t *)ba, count, (uint32_t *)rgba);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_fence_record(pcr_ctx *c, int slot, void *hip_stream)
{
    if (!c || slot < 0 || slot >= pcr_ctx::FENCES) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->fence[slot]) HIP_TRY(c, hipEventCreateWithFlags(&c->fence[slot], hipEventDisableTiming | hipEventReleaseToDevice));
    HIP_TRY(c, hipEventRecord(c->fence[slot], hip_stream ? (hipStream_t)hip_stream : c->stream));
    return PCR_OK;
}

int pcr_fence_wait(pcr_ctx *c, int slot, void *hip_stream)
{
    if (!c || slot < 0 || slot >= pcr_ctx::FENCES) return PCR_E_ARG;
    if (!c->fence[slot]) return PCR_OK;          // never recorded: nothing to wait for
    HIP_TRY(c, hipStreamWaitEvent(hip_stream ? (hipStream_t)hip_stream : c->stream, c->fence[slot], 0));
    return PCR_OK;
}

int pcr_merge_min(pcr_ctx *c, const void *other)
{
    if (!c || !other) return PCR_E_ARG;
    c->tiles_tracked = false;
    if (!c->fb) return set_err(c, PCR_E_ARG, "no framebuffer");
    hipLaunchKernelGGL(k_merge_min, dim3(2048), dim3(256), 0, c->stream, c->fb, (const uint64_t *)other, (uint32_t)c->fb_elems);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_merge_sum(pcr_ctx *c, const void *org, const void *oba)
{
    if (!c) return PCR_E_ARG;
    c->tiles_tracked = false;
    if (!c->rg || !c->ba) return set_err(c, PCR_E_ARG, "no accumulation buffers");
    c->accum_dirty = true;
    if (org) hipLaunchKernelGGL(k_merge_sum, dim3(2048), dim3(256), 0, c->stream, c->rg, (const uint64_t *)org, (uint32_t)c->fb_elems);
    if (oba) hipLaunchKernelGGL(k_merge_sum, dim3(2048), dim3(256), 0, c->stream, c->ba, (const uint64_t *)oba, (uint32_t)c->fb_elems);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

int pcr_flip_sign(pcr_ctx *c)
{
    if (!c) return PCR_E_ARG;
    c->tiles_tracked = false;
    if (!c->fb) return set_err(c, PCR_E_ARG, "no framebuffer");
    hipLaunchKernelGGL(k_flip_sign, dim3(2048), dim3(256), 0, c->stream, c->fb, (uint32_t)c->fb_elems);
    HIP_TRY(c, hipGetLastError());
    return PCR_OK;
}

// ---- measurement -------------------------------------------------------------------------------
int pcr_timing_begin(pcr_ctx *c)
{
    if (!c) return PCR_E_ARG;
    HIP_TRY(c, hipEventRecord(c->ev_begin, c->stream));
    return PCR_OK;
}

int pcr_timing_end(pcr_ctx *c, float *ms)
{
    if (!c || !ms) return PCR_E_ARG;
    HIP_TRY(c, hipEventRecord(c->ev_end, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev_end));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev_begin, c->ev_end));
    return PCR_OK;
}

int pcr_measure_hbm(pcr_ctx *c, size_t bytes, int reps, float *read_gbps, float *copy_gbps)
{
    if (!c || !read_gbps || !copy_gbps || reps <= 0 || bytes < (1u << 20)) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n16 = bytes / 16;
    hbm_vec4 *a = nullptr, *b = nullptr;
    uint32_t *sink = nullptr;
    auto cleanup = [&] { if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (sink) (void)hipFree(sink); };
    if (hipMalloc((void **)&a, n16 * 16) != hipSuccess || hipMalloc((void **)&b, n16 * 16) != hipSuccess ||
        hipMalloc((void **)&sink, 4) != hipSuccess) {
        cleanup();
        return set_err(c, PCR_E_NOMEM, "pcr_measure_hbm: cannot allocate 2 x %zu bytes", n16 * 16);
    }
    int rc = PCR_OK;
    auto run = [&](bool copy, float *out) {
        const unsigned grid = 256 * 16;          // 16 workgroups of 256 threads per CU
        float best = 0.0f;
        for (int r = 0; r < reps + 1; ++r) {     // first pass untimed
            if (hipEventRecord(c->ev_begin, c->stream) != hipSuccess) { rc = PCR_E_HIP; return; }
            if (copy) hipLaunchKernelGGL(k_hbm_copy, dim3(grid), dim3(256), 0, c->stream, a, b, n16);
            else hipLaunchKernelGGL(k_hbm_read, dim3(grid), dim3(256), 0, c->stream, a, n16, sink);
            float ms = 0.0f;
            if (hipEventRecord(c->ev_end, c->stream) != hipSuccess || hipEventSynchronize(c->ev_end) != hipSuccess ||
                hipEventElapsedTime(&ms, c->ev_begin, c->ev_end) != hipSuccess) { rc = PCR_E_HIP; return; }
            const float gbps = (float)((copy ? 2.0 : 1.0) * (double)(n16 * 16) / (ms * 1e-3) / 1e9);
            if (r > 0 && gbps > best) best = gbps;
        }
        *out = best;
    };
    if (hipMemsetAsync(a, 0x5A, n16 * 16, c->stream) != hipSuccess || hipMemsetAsync(b, 0, n16 * 16, c->stream) != hipSuccess)
        rc = PCR_E_HIP;
    if (rc == PCR_OK) run(false, read_gbps);
    if (rc == PCR_OK) run(true, copy_gbps);
    (void)hipStreamSynchronize(c->stream);
    cleanup();
    if (rc != PCR_OK) return set_err(c, rc, "pcr_measure_hbm: %s", hipGetErrorString(hipGetLastError()));
    return PCR_OK;
}

int pcr_kernel_timing_enable(pcr_ctx *c, int every)
{
    if (!c || every < 0) return PCR_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (every > 0)
        for (int i = 0; i < pcr_ctx::KT_PAIRS; ++i) {
            // device-scope release: the default system-scope one writes the L2 back around the kernel being timed
            if (!c->kt_begin[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->kt_begin[i], hipEventReleaseToDevice));
            if (!c->kt_end[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->kt_end[i], hipEventReleaseToDevice));
        }
    c->kt_every = every;
    c->kt_launches = 0;
    c->kt_samples = 0;
    return PCR_OK;
}

int pcr_kernel_timing_read(pcr_ctx *c, float *avg_ms, int *launches)
{
    if (!c || !avg_ms || !launches) return PCR_E_ARG;
    *avg_ms = 0.0f; *launches = 0;
    const int n = (int)std::min<int64_t>(c->kt_samples, pcr_ctx::KT_PAIRS);
    if (n == 0) return PCR_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        float ms = 0.0f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->kt_begin[i], c->kt_end[i]));
        sum += ms;
    }
    *avg_ms = (float)(sum / n); *launches = n;
    return PCR_OK;
}

} // extern "C"

#include "pcr_gpu_encoder.hip.h"   // pcr_gpu_encode_points (include/pcr_gpu_encode.h)
