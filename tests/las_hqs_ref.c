/*
 * las_hqs_ref.c — CPU reference of the 10-10-10 HQS method ("loop_las_hqs"). TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The oracle's 10-10-10 renderer returns the finished framebuffer only; the HQS method needs the per-pixel depth of the
 * depth pass and the colour sums of the colour pass. This file includes the oracle so that it reuses mat_mul, f32_bits,
 * bits_f32 and pcr_oracle_las_level bit for bit, and restates the per-point loop of pcr_oracle_render_las on top of them
 * (modules/compute_loop_las_cuda/render.cu:130-442: same batches, levels, decode and projection):
 *   las_hqs_ref_depth: key f32_bits(w) << 32, payload 0 (modules/compute_loop_las_hqs/depth.cs:335-355);
 *   las_hqs_ref_color: a point is averaged into its pixel iff w <= d * 1.01f, d = bits_f32(fb[pix] >> 32), an f32 product
 *                      (color.cs:370); RG += R<<32 | G, BA += B<<32 | 1 (the Huffman HQS packing).
 * Built with the oracle Makefile's flags (-ffp-contract=off -mfma): tests/las_hqs_ref.py.
 */
#include "../oracle/pcr_oracle.c"

typedef void (*las_point_fn)(void *ctx, size_t pix, float w, uint32_t index);

static void las_walk(const pcr_xyz_batch *batches, int64_t num_batches, const uint32_t *xyz12, const uint32_t *xyz8,
                     const uint32_t *xyz4, const pcr_render_params *p, pcr_render_stats *stats, las_point_fn fn, void *ctx)
{
    const size_t fb_elems = pcr_fb_elems(p->width, p->height);
    for (int64_t b = 0; b < num_batches; ++b) {
        const pcr_xyz_batch *g = &batches[b];
        if (stats) stats->batches_total++;
        int level = pcr_oracle_las_level(g, p);
        if (level < 0) { if (stats) stats->batches_culled++; continue; }
        if (b == num_batches - 1) continue;                       /* render.cu:201-202 */
        if (stats) stats->points_iterated += PCR_POINTS_PER_BATCH;
        const float bs[3] = { g->max_x - g->min_x, g->max_y - g->min_y, g->max_z - g->min_z };
        const float lo[3] = { g->min_x, g->min_y, g->min_z };
        const float div = level >= 2 ? 1024.0f : 1073741824.0f;
        const float sc[3] = { bs[0] / div, bs[1] / div, bs[2] / div };
        for (int64_t k = 0; k < PCR_POINTS_PER_BATCH; ++k) {
            const uint32_t index = (uint32_t)(b * PCR_POINTS_PER_BATCH + k);
            uint32_t X, Y, Z;
            const uint32_t b4 = xyz4[index];
            if (level >= 2) {
                X = b4 & 1023u; Y = (b4 >> 10) & 1023u; Z = (b4 >> 20) & 1023u;
            } else {
                const uint32_t b8 = xyz8[index];
                X = ((b4 & 1023u) << 20) | ((b8 & 1023u) << 10);
                Y = (((b4 >> 10) & 1023u) << 20) | (((b8 >> 10) & 1023u) << 10);
                Z = (((b4 >> 20) & 1023u) << 20) | (((b8 >> 20) & 1023u) << 10);
                if (level == 0) {
                    const uint32_t b12 = xyz12[index];
                    X |= b12 & 1023u; Y |= (b12 >> 10) & 1023u; Z |= (b12 >> 20) & 1023u;
                }
            }
            f4 pt = { fmaf((float)X, sc[0], lo[0]), fmaf((float)Y, sc[1], lo[1]), fmaf((float)Z, sc[2], lo[2]), 1.0f };
            f4 pos = mat_mul(p->transform, pt);
            float nx = pos.x / pos.w, ny = pos.y / pos.w;
            if (!(pos.w > 0.0f && nx >= -1.0f && nx <= 1.0f && ny >= -1.0f && ny <= 1.0f)) continue;
            float ix = fmaf(nx, 0.5f, 0.5f) * (float)p->width, iy = fmaf(ny, 0.5f, 0.5f) * (float)p->height;
            int64_t pix = (int64_t)(int)ix + (int64_t)(int)iy * p->width;
            if (pix < 0 || (size_t)pix >= fb_elems) continue;
            fn(ctx, (size_t)pix, pos.w, index);
        }
    }
}

typedef struct { uint64_t *fb; const uint32_t *rgba; uint64_t *rg, *ba; } las_hqs_ctx;

static void depth_point(void *vctx, size_t pix, float w, uint32_t index)
{
    las_hqs_ctx *c = (las_hqs_ctx *)vctx;
    (void)index;
    const uint64_t key = (uint64_t)f32_bits(w) << 32;            /* depth.cs:344-348, payload 0 */
    if (key < c->fb[pix]) c->fb[pix] = key;
}

static void color_point(void *vctx, size_t pix, float w, uint32_t index)
{
    las_hqs_ctx *c = (las_hqs_ctx *)vctx;
    const float d = bits_f32((uint32_t)(c->fb[pix] >> 32));
    const float limit = d * 1.01f;                                /* color.cs:370, f32 (no contraction: -ffp-contract=off) */
    if (!(w <= limit)) return;
    const uint32_t rgba = c->rgba[index];
    const uint64_t r = rgba & 255u, g = (rgba >> 8) & 255u, b = (rgba >> 16) & 255u;
    c->rg[pix] += (r << 32) | g;
    c->ba[pix] += (b << 32) | 1u;
}

void las_hqs_ref_depth(const pcr_xyz_batch *batches, int64_t num_batches, const uint32_t *xyz12, const uint32_t *xyz8,
                       const uint32_t *xyz4, const pcr_render_params *p, uint64_t *fb, pcr_render_stats *stats)
{
    las_hqs_ctx c = { fb, NULL, NULL, NULL };
    las_walk(batches, num_batches, xyz12, xyz8, xyz4, p, stats, depth_point, &c);
}

void las_hqs_ref_color(const pcr_xyz_batch *batches, int64_t num_batches, const uint32_t *xyz12, const uint32_t *xyz8,
                       const uint32_t *xyz4, const uint32_t *rgba, const pcr_render_params *p, const uint64_t *fb,
                       uint64_t *rg, uint64_t *ba, pcr_render_stats *stats)
{
    las_hqs_ctx c = { (uint64_t *)fb, rgba, rg, ba };
    las_walk(batches, num_batches, xyz12, xyz8, xyz4, p, stats, color_point, &c);
}

/* Every point the two passes draw, as (pixel, w) and, if `index` is not NULL, its point index: for counting the 1 % test and
 * depth ties independently of the frame code. Returns how many there are; at most `cap` are written. */
typedef struct { int64_t n, cap; int64_t *pix; float *w; uint32_t *index; } las_points_ctx;

static void list_point(void *vctx, size_t pix, float w, uint32_t index)
{
    las_points_ctx *c = (las_points_ctx *)vctx;
    if (c->n < c->cap) { c->pix[c->n] = (int64_t)pix; c->w[c->n] = w; if (c->index) c->index[c->n] = index; }
    c->n++;
}

int64_t las_hqs_ref_points(const pcr_xyz_batch *batches, int64_t num_batches, const uint32_t *xyz12, const uint32_t *xyz8,
                           const uint32_t *xyz4, const pcr_render_params *p, int64_t *pix, float *w, uint32_t *index, int64_t cap)
{
    las_points_ctx c = { 0, cap, pix, w, index };
    las_walk(batches, num_batches, xyz12, xyz8, xyz4, p, NULL, list_point, &c);
    return c.n;
}
