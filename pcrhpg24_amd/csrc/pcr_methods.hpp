// pcr_methods.hpp — C++ host-side adapters with the reference's plugin surface, over the C ABI (pcr_hip.h).
//
// A maintainer of the reference swaps the CUDA-driver bodies of these classes for the pcr_* calls below; the
// names, members and call order are the reference's:
//   Method / Runtime / Debug              include/Method.h:10-23, include/Runtime.h:15-55, include/Debug.h:14-31
//   Resource, HuffmanLasData              modules/compute/Resources.h:20-35, modules/compute/HuffmanLasLoader.{h,cpp}
//   HuffmanMemIter ("huffman_mem_iter_cuda")   modules/huffman_mem_iter_cuda/huffman_mem_iter_cuda.h
//   HuffmanHQS     ("huffman_hqs")              modules/huffman_hqs/huffman_hqs.h
//   ComputeLasData, ComputeLoopLasCUDA ("loop_las_cuda")   modules/compute/ComputeLasLoader.{h,cpp},
//                                                          modules/compute_loop_las_cuda/compute_loop_las_cuda.h
//   ComputeLoopLasHQS ("loop_las_hqs")                     modules/compute_loop_las_hqs/compute_loop_las_hqs.h
// Headless: `Renderer` carries the window size and the orbit camera only (no GLFW/GL/ImGui); the resolve target is
// a device RGBA8 buffer instead of a GL texture.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "pcr_encode.h"
#include "pcr_hip.h"
#include "pcr_las_reader.hpp"

namespace pcr_host {

struct Debug {                                  // include/Debug.h:21-30 (flags the Huffman methods read)
    inline static float LOD = 0.1f;
    inline static bool frustumCullingEnabled = true;
    inline static bool colorizeChunks = false;
    inline static bool showNumPoints = false;
    inline static bool saveDepthMap = false;            // include/Debug.h: one-shot, cleared after the dump
    inline static std::string depthMapPath = "depth.exr";   // the reference writes "out/depth.exr" (huffman_hqs.h:235)
};

// huffman_hqs.h:71-113 saves the depth map through tinyexr: one FLOAT channel "Z". Same file kind, written directly:
// OpenEXR 2 scanline file, no compression, increasing-Y line order.
inline bool saveSingleChannelEXR(const char *filename, const float *depthData, int width, int height)
{
    std::vector<uint8_t> f;
    auto raw = [&](const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; f.insert(f.end(), b, b + n); };
    auto i32 = [&](int32_t v) { raw(&v, 4); };
    auto str = [&](const char *z) { raw(z, std::strlen(z) + 1); };
    auto attr = [&](const char *name, const char *type, int32_t size) { str(name); str(type); i32(size); };
    const uint8_t magic[8] = {0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0};
    raw(magic, 8);
    attr("channels", "chlist", 2 + 16 + 1);
    str("Z"); i32(2 /* FLOAT */); { const uint8_t plin[4] = {0, 0, 0, 0}; raw(plin, 4); } i32(1); i32(1);
    { const uint8_t end = 0; raw(&end, 1); }
    attr("compression", "compression", 1); { const uint8_t none = 0; raw(&none, 1); }
    const int32_t box[4] = {0, 0, width - 1, height - 1};
    attr("dataWindow", "box2i", 16); raw(box, 16);
    attr("displayWindow", "box2i", 16); raw(box, 16);
    attr("lineOrder", "lineOrder", 1); { const uint8_t incy = 0; raw(&incy, 1); }
    const float one = 1.0f, zero2[2] = {0.0f, 0.0f};
    attr("pixelAspectRatio", "float", 4); raw(&one, 4);
    attr("screenWindowCenter", "v2f", 8); raw(zero2, 8);
    attr("screenWindowWidth", "float", 4); raw(&one, 4);
    { const uint8_t end = 0; raw(&end, 1); }
    const uint64_t table = f.size(), line = 8 + (uint64_t)width * 4;
    for (int y = 0; y < height; ++y) { const uint64_t off = table + 8ull * height + line * y; raw(&off, 8); }
    for (int y = 0; y < height; ++y) { i32(y); i32(width * 4); raw(depthData + (size_t)y * width, (size_t)width * 4); }
    std::ofstream o(filename, std::ios::binary);
    o.write((const char *)f.data(), (std::streamsize)f.size());
    return (bool)o;
}


struct Renderer {
    int width = 1920, height = 1080;            // src/Renderer.cpp:142-143
    pcr_ctx *ctx = nullptr;
    double yaw = 0, pitch = 0, radius = 10, target[3] = {0, 0, 0};   // include/OrbitControls.h

    explicit Renderer(int w = 1920, int h = 1080, int device = 0) : width(w), height(h)
    {
        if (pcr_create(device, &ctx) != PCR_OK) throw std::runtime_error(std::string("pcr_create: ") + pcr_last_error(nullptr));
        check(pcr_set_image_size(ctx, w, h), "pcr_set_image_size");
    }
    ~Renderer() { pcr_destroy(ctx); }
    Renderer(const Renderer &) = delete;

    void check(int rc, const char *what) const
    {
        if (rc != PCR_OK) throw std::runtime_error(std::string(what) + ": " + pcr_last_error(ctx));
    }

    // ChangingRenderData as HuffmanHQS::render fills it (huffman_hqs.h:157-183)
    pcr_render_params params() const
    {
        pcr_render_params p;
        if (pcr_camera_orbit(yaw, pitch, radius, target, width, height, 60.0, 0.1, 200000.0, &p))
            throw std::runtime_error(std::string("pcr_camera_orbit: ") + pcr_host_last_error());
        p.lod_percent = (int)(Debug::LOD * 100);
        p.enable_frustum_culling = Debug::frustumCullingEnabled;
        p.colorize_chunks = Debug::colorizeChunks;
        p.show_num_points = Debug::showNumPoints;
        return p;
    }
};

// huffman_hqs.h:217-237: depth of every covered pixel as float, image flipped vertically, empty pixels 0
inline bool dumpDepthMap(Renderer *r, pcr_ctx *ctx, int width, int height, const std::string &path)
{
    std::vector<uint64_t> fb_host((size_t)width * height);
    r->check(pcr_read_framebuffer(ctx, fb_host.data(), fb_host.size()), "pcr_read_framebuffer");
    std::vector<float> depthmap((size_t)width * height, 0.0f);
    for (int i = 0; i < height; ++i)
        for (int j = 0; j < width; ++j) {
            const uint32_t value = (uint32_t)(fb_host[(size_t)i * width + j] >> 32);
            if (value == 0xFFFFFFFFu) continue;
            std::memcpy(&depthmap[(size_t)(height - i - 1) * width + j], &value, 4);
        }
    return saveSingleChannelEXR(path.c_str(), depthmap.data(), width, height);
}

enum ResourceState { UNLOADED, LOADING, LOADED, UNLOADING };   // Resources.h:20-25

struct Resource {
    ResourceState state = UNLOADED;
    virtual ~Resource() = default;
    virtual void load(Renderer *renderer) = 0;
    virtual void unload(Renderer *renderer) = 0;
    virtual void process(Renderer *renderer) = 0;
};

struct Method {
    std::string name = "no name", description = "", group = "no group";
    // Set: the frame's resolve is the display resolve (pcr_resolve_*_display) with these options; nothing else in the frame changes.
    // Not in the reference's Method; read by the Huffman and the 10-10-10 methods below.
    std::optional<pcr_display_opts> display;
    virtual ~Method() = default;
    virtual void update(Renderer *renderer) = 0;
    virtual void render(Renderer *renderer) = 0;
};

struct Runtime {
    inline static std::vector<Method *> methods;
    inline static Method *selectedMethod = nullptr;
    inline static Resource *resource = nullptr;
    static void addMethod(Method *m) { methods.push_back(m); }
    static void setSelectedMethod(const std::string &name)
    {
        for (Method *m : methods) if (m->name == name) selectedMethod = m;
    }
    static Method *getSelectedMethod() { return selectedMethod; }
};

// modules/compute/HuffmanLasLoader.{h,cpp}: header parse, progressive loading through a reader thread that hands
// over tasks of <= 100 batch records (cpp:81-149), uploadBatch on the render thread (cpp:176-313).
struct HuffmanLasData : Resource {
    struct LoaderTask {
        std::vector<std::vector<char>> buffers;
        std::vector<int64_t> batchIndices;
    };

    std::string path;
    int64_t numBatches = 0, numPoints = 0, encodedBytes = 0, separateBytes = 0, clusterBytes = 0;
    std::vector<int64_t> batch_data_sizes, batch_data_sizes_prefix;
    int64_t numBatchesLoaded = 0, numPointsLoaded = 0, offsetToBatchData = 0;
    int64_t numBatchesResident = 0;     // what the next frame draws; lags numBatchesLoaded only with asyncUpload
    bool asyncUpload = false;           // copies + transcode on the context's loader stream (pcr_set_async_upload)
    Renderer *loadedOn = nullptr;       // the renderer whose context holds the stream (load() .. unload())

    std::shared_ptr<LoaderTask> task;
    std::mutex mtx_state, mtx_tasks;
    std::thread reader;
    std::string readerError;            // set by the reader thread (under mtx_tasks) when it had to give up; process() throws it

    ~HuffmanLasData() override { stopReader(); }

    void loadHeader()                                       // HuffmanLasLoader.h:57-85
    {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("cannot open " + path);
        int64_t h[5];
        f.read((char *)h, sizeof h);
        if (!f) throw std::runtime_error(path + ": shorter than its header");
        numPoints = h[0]; numBatches = h[1]; encodedBytes = h[2]; separateBytes = h[3]; clusterBytes = h[4];
        if (numBatches <= 0 || numPoints != numBatches * PCR_POINTS_PER_BATCH) throw std::runtime_error(path + ": bad header");
        batch_data_sizes.resize((size_t)numBatches);
        f.read((char *)batch_data_sizes.data(), 8 * numBatches);
        if (!f) throw std::runtime_error(path + ": shorter than its batch size table");
        offsetToBatchData = 40 + 8 * numBatches;
        // every record at least its fixed part, and all of them inside the file (the reference trusts these, HuffmanLasLoader.h:
        // 72-84; a negative or huge entry would otherwise end in an allocation failure inside the reader thread)
        f.seekg(0, std::ios::end);
        const int64_t fileBytes = (int64_t)f.tellg();
        const int64_t minRecord = PCR_BATCH_FIXED_HEADER + 4 * (3072 + 1024 + 4096 + 4096 + 32) + PCR_COLOR_BYTES_PER_BATCH;
        batch_data_sizes_prefix = batch_data_sizes;
        int64_t running = 0;
        for (int64_t i = 0; i < numBatches; ++i) {
            const int64_t sz = batch_data_sizes[(size_t)i];
            if (sz < minRecord || sz > fileBytes) throw std::runtime_error(path + ": batch " + std::to_string(i) + " has record size " + std::to_string(sz));
            running += sz;
            if (offsetToBatchData + running > fileBytes) throw std::runtime_error(path + ": batch records exceed the file");
            batch_data_sizes_prefix[(size_t)i] = running;
        }
    }

    static std::shared_ptr<HuffmanLasData> create(const std::string &path)   // HuffmanLasLoader.h:87-92
    {
        auto d = std::make_shared<HuffmanLasData>();
        d->path = path;
        d->loadHeader();
        return d;
    }

    void load(Renderer *renderer) override                  // HuffmanLasLoader.cpp:22-150
    {
        {
            std::lock_guard<std::mutex> lock(mtx_state);
            if (state != UNLOADED) return;
            state = LOADING;
        }
        pcr_file_header hdr{numPoints, numBatches, encodedBytes, separateBytes, clusterBytes};
        loadedOn = renderer;
        renderer->check(pcr_stream_begin(renderer->ctx, &hdr, 0), "pcr_stream_begin");
        renderer->check(pcr_set_async_upload(renderer->ctx, asyncUpload ? 1 : 0), "pcr_set_async_upload");
        numBatchesLoaded = numPointsLoaded = numBatchesResident = 0;
        readerError.clear();
        reader = std::thread([this] {
          try {
            std::ifstream f(path, std::ios::binary);
            if (!f) throw std::runtime_error("cannot open " + path);
            int64_t remaining = numBatches, read = 0;
            while (remaining > 0) {
                {
                    std::lock_guard<std::mutex> lock(mtx_state);
                    if (state == UNLOADING) { state = UNLOADED; return; }
                }
                {
                    std::lock_guard<std::mutex> lock(mtx_tasks);
                    if (task) { std::this_thread::sleep_for(std::chrono::microseconds(100)); continue; }
                }
                auto t = std::make_shared<LoaderTask>();
                int64_t n = remaining < 100 ? remaining : 100;
                for (int64_t i = 0; i < n; ++i) {
                    int64_t b = read + i;
                    int64_t start = offsetToBatchData + (b ? batch_data_sizes_prefix[(size_t)b - 1] : 0);
                    std::vector<char> buf((size_t)batch_data_sizes[(size_t)b]);
                    f.seekg(start);
                    f.read(buf.data(), (std::streamsize)buf.size());
                    if (!f) throw std::runtime_error(path + ": short read on batch " + std::to_string(b));
                    t->buffers.push_back(std::move(buf));
                    t->batchIndices.push_back(b);
                }
                read += n; remaining -= n;
                std::lock_guard<std::mutex> lock(mtx_tasks);
                task = t;
            }
            std::lock_guard<std::mutex> lock(mtx_state);
            if (state == UNLOADING) state = UNLOADED;
            else if (state == LOADING) state = LOADED;
          } catch (const std::exception &e) {              // never let an exception leave the thread (std::terminate)
            { std::lock_guard<std::mutex> lock(mtx_tasks); readerError = e.what(); }
            std::lock_guard<std::mutex> lock(mtx_state);
            state = UNLOADED;
          }
        });
    }

    void process(Renderer *renderer) override               // HuffmanLasLoader.cpp:301-313
    {
        std::lock_guard<std::mutex> lock(mtx_tasks);
        if (!readerError.empty()) { const std::string e = readerError; readerError.clear(); throw std::runtime_error("loader: " + e); }
        if (!task) return;
        // the task is dropped whatever happens to it: a record the library rejects must not be offered again every frame
        struct Drop { std::shared_ptr<LoaderTask> &t; ~Drop() { t = nullptr; } } drop{task};
        std::vector<const void *> blobs;
        std::vector<size_t> sizes;
        for (size_t i = 0; i < task->batchIndices.size(); ++i) { blobs.push_back(task->buffers[i].data()); sizes.push_back(task->buffers[i].size()); }
        renderer->check(pcr_upload_batches(renderer->ctx, task->batchIndices.front(), (int64_t)blobs.size(), blobs.data(), sizes.data()),
                        "pcr_upload_batches");
        numBatchesLoaded = pcr_batches_loaded(renderer->ctx);
        numPointsLoaded = pcr_points_loaded(renderer->ctx);
    }

    void unload(Renderer *renderer) override                // HuffmanLasLoader.cpp:152-174
    {
        stopReader();
        numBatchesLoaded = 0;
        loadedOn = nullptr;
        pcr_stream_unload(renderer->ctx);
        std::lock_guard<std::mutex> lock(mtx_state);
        state = UNLOADED;
    }

    bool fullyLoaded() const { return numBatchesLoaded == numBatches; }
    bool fullyResident(Renderer *renderer)
    {
        numBatchesResident = pcr_batches_resident(renderer->ctx);
        return numBatchesResident == numBatches;
    }

    // Every point the context it was loaded on holds right now, decoded on the GPU (pcr_read_points: the stream's order, 65 536
    // records per batch, padding and tail artefacts as the render kernels draw them). Not in the reference.
    void decodePoints(std::vector<pcr_point> &out)
    {
        if (!loadedOn) throw std::runtime_error("decodePoints: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        out.resize((size_t)nB * PCR_POINTS_PER_BATCH);
        loadedOn->check(pcr_read_points(loadedOn->ctx, 0, nB, out.data(), out.size()), "pcr_read_points");
    }

    // The points inside `box` (the stream's int32 coordinates, bounds inclusive) of every batch the context holds right now:
    // decodePoints() with the records outside the box removed, selected on the GPU (pcr_read_box: batches the box misses are
    // not decoded). Not in the reference.
    pcr_select_stats selectBox(const pcr_box &box, std::vector<pcr_point> &out)
    {
        if (!loadedOn) throw std::runtime_error("selectBox: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_select_stats st{};
        loadedOn->check(pcr_read_box(loadedOn->ctx, 0, nB, &box, nullptr, 0, &n, &st), "pcr_read_box");
        out.resize((size_t)n);
        if (n) loadedOn->check(pcr_read_box(loadedOn->ctx, 0, nB, &box, out.data(), out.size(), &n, &st), "pcr_read_box");
        return st;
    }

    // The points inside the polygon prism `poly` (the stream's int32 coordinates; pcr_types.h has the rule) of every batch the context
    // holds right now: decodePoints() with the unselected records removed, selected on the GPU (pcr_read_polygon: batches the prism
    // misses are not decoded, the ones its boundary crosses test their points against their own few edges). Not in the reference.
    pcr_polygon_stats pointsInPolygon(const pcr_polygon &poly, std::vector<pcr_point> &out)
    {
        if (!loadedOn) throw std::runtime_error("pointsInPolygon: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_polygon_stats st{};
        loadedOn->check(pcr_read_polygon(loadedOn->ctx, 0, nB, &poly, nullptr, 0, &n, &st), "pcr_read_polygon");
        out.resize((size_t)n);
        if (n) loadedOn->check(pcr_read_polygon(loadedOn->ctx, 0, nB, &poly, out.data(), out.size(), &n, &st), "pcr_read_polygon");
        return st;
    }

    // The support of plane hypotheses (pcr_plane_support): counts[j] = the points inside `clip` (NULL: everywhere) and in no slab of
    // `exclude` that are in hyp[j], of every batch the context holds right now, counted on the GPU straight from the compressed
    // stream. Not in the reference.
    pcr_plane_stats planeSupport(const std::vector<pcr_slab> &hyp, const pcr_box *clip, const std::vector<pcr_slab> &exclude, std::vector<int64_t> &counts)
    {
        if (!loadedOn) throw std::runtime_error("planeSupport: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        counts.assign(hyp.size(), 0);
        pcr_plane_stats st{};
        loadedOn->check(pcr_plane_support(loadedOn->ctx, 0, nB, hyp.data(), (int)hyp.size(), clip, exclude.empty() ? nullptr : exclude.data(),
                                          (int)exclude.size(), counts.data(), &st), "pcr_plane_support");
        return st;
    }

    // The points inside `clip` (NULL: everywhere) that are in all of `slabs`, with PCR_SLAB_INVERT in `flags` those that are not, of
    // every batch the context holds right now, selected on the GPU (pcr_read_slabs: batches a slab misses are not decoded). Not in
    // the reference.
    pcr_slab_stats selectSlabs(const std::vector<pcr_slab> &slabs, const pcr_box *clip, uint32_t flags, std::vector<pcr_point> &out)
    {
        if (!loadedOn) throw std::runtime_error("selectSlabs: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_slab_stats st{};
        loadedOn->check(pcr_read_slabs(loadedOn->ctx, 0, nB, slabs.data(), (int)slabs.size(), clip, flags, nullptr, 0, &n, &st), "pcr_read_slabs");
        out.resize((size_t)n);
        if (n) loadedOn->check(pcr_read_slabs(loadedOn->ctx, 0, nB, slabs.data(), (int)slabs.size(), clip, flags, out.data(), out.size(), &n, &st), "pcr_read_slabs");
        return st;
    }

    // One point per voxel of `vox` among the points inside `clip` (NULL: everywhere), thinned on the GPU straight from the compressed
    // stream (pcr_read_thin: a counting call, then the read). Not in the reference.
    pcr_thin_stats thin(const pcr_voxels &vox, const pcr_box *clip, int mode, std::vector<pcr_point> &out)
    {
        if (!loadedOn) throw std::runtime_error("thin: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_thin_stats st{};
        loadedOn->check(pcr_read_thin(loadedOn->ctx, 0, nB, &vox, clip, mode, nullptr, nullptr, 0, &n, &st), "pcr_read_thin");
        out.resize((size_t)n);
        if (n) loadedOn->check(pcr_read_thin(loadedOn->ctx, 0, nB, &vox, clip, mode, out.data(), nullptr, out.size(), &n, &st), "pcr_read_thin");
        return st;
    }

    // The points inside `clip` (NULL: everywhere) in level-of-detail order: by the least level of `lod`'s nested lattices at which a
    // point is the first of its voxel in the stream's order (0 = coarsest), inside a level in the stream's order, last the points
    // that are first at no level (left out with PCR_LOD_DROP_REST; PCR_LOD_ROW_ORDER: the stream's order throughout), on the GPU
    // straight from the compressed stream (pcr_read_lod_order: a counting call, then the read). `levels` (may be NULL) gets the level
    // of every point; the returned level_count tells where every level ends. Not in the reference.
    pcr_lod_stats lodOrdered(const pcr_lod &lod, const pcr_box *clip, uint32_t flags, std::vector<pcr_point> &out, std::vector<uint8_t> *levels = nullptr)
    {
        if (!loadedOn) throw std::runtime_error("lodOrdered: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_lod_stats st{};
        loadedOn->check(pcr_read_lod_order(loadedOn->ctx, 0, nB, &lod, clip, flags, nullptr, nullptr, nullptr, 0, &n, &st), "pcr_read_lod_order");
        out.resize((size_t)n);
        if (levels) levels->resize((size_t)n);
        if (n) loadedOn->check(pcr_read_lod_order(loadedOn->ctx, 0, nB, &lod, clip, flags, out.data(), nullptr, levels ? levels->data() : nullptr, out.size(), &n, &st),
                               "pcr_read_lod_order");
        return st;
    }

    // One computed point per non-empty voxel of `vox` among the points inside `clip` (NULL: everywhere): the mean position, rounded
    // half up inside the voxel, and the mean of each colour byte, in thin()'s PCR_THIN_FIRST order, with the points per voxel in
    // `counts`, on the GPU straight from the compressed stream (pcr_read_voxel_mean: a counting call, then the read). Not in the
    // reference.
    pcr_thin_stats voxelMean(const pcr_voxels &vox, const pcr_box *clip, std::vector<pcr_point> &points, std::vector<int64_t> &counts)
    {
        if (!loadedOn) throw std::runtime_error("voxelMean: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_thin_stats st{};
        loadedOn->check(pcr_read_voxel_mean(loadedOn->ctx, 0, nB, &vox, clip, nullptr, nullptr, nullptr, 0, &n, &st), "pcr_read_voxel_mean");
        points.resize((size_t)n); counts.resize((size_t)n);
        if (n) loadedOn->check(pcr_read_voxel_mean(loadedOn->ctx, 0, nB, &vox, clip, points.data(), nullptr, counts.data(), points.size(), &n, &st),
                               "pcr_read_voxel_mean");
        return st;
    }

    // The points inside `clip` (NULL: everywhere) without the isolated ones -- those whose 3 x 3 x 3 voxels of `vox` hold at most
    // max_count of them, the point itself included -- or with PCR_DENOISE_ISOLATED those alone, on the GPU straight from the
    // compressed stream (pcr_read_denoise: a counting call, then the read). Not in the reference.
    pcr_denoise_stats denoised(const pcr_voxels &vox, const pcr_box *clip, int64_t max_count, int mode, std::vector<pcr_point> &out)
    {
        if (!loadedOn) throw std::runtime_error("denoised: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_denoise_stats st{};
        loadedOn->check(pcr_read_denoise(loadedOn->ctx, 0, nB, &vox, clip, max_count, mode, nullptr, nullptr, 0, &n, &st), "pcr_read_denoise");
        out.resize((size_t)n);
        if (n) loadedOn->check(pcr_read_denoise(loadedOn->ctx, 0, nB, &vox, clip, max_count, mode, out.data(), nullptr, out.size(), &n, &st), "pcr_read_denoise");
        return st;
    }

    // The points inside `clip` (NULL: everywhere) of the connected components of the occupied voxels of `vox` (adjacent: at most 1
    // apart on every axis with connectivity 26, exactly 1 on one axis with 6) that hold at least min_points of them, or with
    // PCR_COMPONENTS_SMALL those of the others, on the GPU straight from the compressed stream (pcr_read_components: a counting
    // call, then the read). labels (may be NULL): per point the least row of its component. Not in the reference.
    pcr_components_stats components(const pcr_voxels &vox, const pcr_box *clip, int connectivity, int64_t min_points, int mode, std::vector<pcr_point> &out,
                                    std::vector<int64_t> *labels = nullptr)
    {
        if (!loadedOn) throw std::runtime_error("components: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_components_stats st{};
        loadedOn->check(pcr_read_components(loadedOn->ctx, 0, nB, &vox, clip, connectivity, min_points, mode, nullptr, nullptr, nullptr, 0, &n, &st),
                        "pcr_read_components");
        out.resize((size_t)n);
        if (labels) labels->resize((size_t)n);
        if (n) loadedOn->check(pcr_read_components(loadedOn->ctx, 0, nB, &vox, clip, connectivity, min_points, mode, out.data(), nullptr,
                                                   labels ? labels->data() : nullptr, out.size(), &n, &st), "pcr_read_components");
        return st;
    }

    // The points inside `clip` (NULL: everywhere) that have at least min_count of them within `radius` lattice steps, the point
    // itself and exact duplicates included, or with PCR_NEIGHBORS_SPARSE the others (PCR_NEIGHBORS_ALL: all of them), on the GPU
    // straight from the compressed stream (pcr_read_neighbors: a counting call, then the read). counts / nn2 (may be NULL): per
    // point the points within the radius and the squared distance to the nearest other one (PCR_NN2_NONE: none). Not in the reference.
    pcr_neighbors_stats radiusFiltered(int32_t radius, const pcr_box *clip, int64_t min_count, int mode, std::vector<pcr_point> &out,
                                       std::vector<int64_t> *counts = nullptr, std::vector<uint64_t> *nn2 = nullptr)
    {
        if (!loadedOn) throw std::runtime_error("radiusFiltered: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_neighbors_stats st{};
        loadedOn->check(pcr_read_neighbors(loadedOn->ctx, 0, nB, radius, clip, min_count, mode, nullptr, nullptr, nullptr, nullptr, 0, &n, &st),
                        "pcr_read_neighbors");
        out.resize((size_t)n);
        if (counts) counts->resize((size_t)n);
        if (nn2) nn2->resize((size_t)n);
        if (n) loadedOn->check(pcr_read_neighbors(loadedOn->ctx, 0, nB, radius, clip, min_count, mode, out.data(), nullptr, counts ? counts->data() : nullptr,
                                                  nn2 ? nn2->data() : nullptr, out.size(), &n, &st), "pcr_read_neighbors");
        return st;
    }

    // The points inside `clip` (NULL: everywhere) that have at least min_count of them within `radius` lattice steps (1 ..
    // PCR_MOMENTS_MAX_RADIUS), the point itself and exact duplicates included, with the eigenvalues of their neighbourhood's
    // covariance and its unit normal, on the GPU straight from the compressed stream (pcr_read_local_moments: a counting call,
    // then the read). moments (may be NULL): the exact moments the eigen records were made from. Not in the reference.
    pcr_neighbors_stats normals(int32_t radius, const pcr_box *clip, int64_t min_count, std::vector<pcr_point> &out, std::vector<pcr_eigen> &eigen,
                                std::vector<pcr_moments> *moments = nullptr)
    {
        if (!loadedOn) throw std::runtime_error("normals: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_neighbors_stats st{};
        loadedOn->check(pcr_read_local_moments(loadedOn->ctx, 0, nB, radius, clip, min_count, nullptr, nullptr, nullptr, nullptr, 0, &n, &st),
                        "pcr_read_local_moments");
        out.resize((size_t)n);
        eigen.resize((size_t)n);
        if (moments) moments->resize((size_t)n);
        if (n) loadedOn->check(pcr_read_local_moments(loadedOn->ctx, 0, nB, radius, clip, min_count, out.data(), nullptr, moments ? moments->data() : nullptr,
                                                      eigen.data(), out.size(), &n, &st), "pcr_read_local_moments");
        return st;
    }

    // Per point inside `clip` (NULL: everywhere) its k (1 .. PCR_KNN_MAX_K) nearest other points within `radius` lattice steps (1 ..
    // PCR_KNN_MAX_RADIUS) in the order (squared distance, row), on the GPU straight from the compressed stream (pcr_read_knn: a
    // counting call, then the read): knn holds k words d2 << 32 | row per point, PCR_KNN_NONE behind the last one found. Only the
    // points with at least min_found (0 .. k) such neighbours come back. rows (may be NULL): the points' rows. Not in the reference.
    pcr_neighbors_stats nearestNeighbors(int k, int32_t radius, const pcr_box *clip, int64_t min_found, std::vector<pcr_point> &out, std::vector<uint64_t> &knn,
                                         std::vector<int64_t> *rows = nullptr)
    {
        if (!loadedOn) throw std::runtime_error("nearestNeighbors: the resource is not loaded");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_neighbors_stats st{};
        loadedOn->check(pcr_read_knn(loadedOn->ctx, 0, nB, k, radius, clip, min_found, nullptr, nullptr, nullptr, 0, &n, &st), "pcr_read_knn");
        out.resize((size_t)n);
        knn.resize((size_t)n * (size_t)k);
        if (rows) rows->resize((size_t)n);
        if (n) loadedOn->check(pcr_read_knn(loadedOn->ctx, 0, nB, k, radius, clip, min_found, out.data(), rows ? rows->data() : nullptr, knn.data(), out.size(),
                                            &n, &st), "pcr_read_knn");
        return st;
    }

    // The statistical outlier filter with the search capped at `radius`: per point inside `clip` the mean of sqrt(d2) * scale over
    // its k nearest other points within the radius (in entry order; infinite without one), mu and the population sigma of the finite
    // means (summed in row order); a point is an outlier iff its mean is > mu + multiplier * sigma or infinite. out: the inliers, or
    // with `outliers` the outliers; *num_outliers (may be NULL): how many there are. (PDAL's filters.outlier with method=statistical
    // has no radius; this reading of its definition has not been checked against the tool.) Not in the reference.
    pcr_neighbors_stats statisticalOutliers(int k, double multiplier, int32_t radius, const pcr_box *clip, double scale, bool outliers, std::vector<pcr_point> &out,
                                            int64_t *num_outliers = nullptr)
    {
        std::vector<pcr_point> all;
        std::vector<uint64_t> knn;
        const pcr_neighbors_stats st = nearestNeighbors(k, radius, clip, 0, all, knn);
        const double inf = std::numeric_limits<double>::infinity();
        std::vector<double> mean(all.size(), inf);
        double sum = 0.0;
        size_t finite = 0;
        for (size_t i = 0; i < all.size(); ++i) {
            double total = 0.0;
            int found = 0;
            for (int j = 0; j < k; ++j) {
                const uint64_t w = knn[i * (size_t)k + (size_t)j];
                if (w == PCR_KNN_NONE) continue;
                total += std::sqrt((double)(w >> 32)) * scale;
                ++found;
            }
            if (found) { mean[i] = total / (double)found; sum += mean[i]; ++finite; }
        }
        const double mu = finite ? sum / (double)finite : 0.0;
        double var = 0.0;
        for (double m : mean) if (m != inf) var += (m - mu) * (m - mu);
        const double limit = mu + multiplier * (finite ? std::sqrt(var / (double)finite) : 0.0);
        out.clear();
        int64_t bad = 0;
        for (size_t i = 0; i < all.size(); ++i) {
            const bool is_outlier = mean[i] == inf || mean[i] > limit;
            bad += is_outlier;
            if (is_outlier == outliers) out.push_back(all[i]);
        }
        if (num_outliers) *num_outliers = bad;
        return st;
    }

    // The points a frame of camera `p` draws whose pixel lies in `rect` (NULL: the whole image), with where they land, selected on
    // the GPU (pcr_read_screen: a counting call, then the read). Either vector may be NULL. Not in the reference.
    pcr_screen_stats selectScreen(const pcr_render_params &p, const pcr_rect *rect, std::vector<pcr_point> *points, std::vector<pcr_screen_hit> *hits)
    {
        if (!loadedOn) throw std::runtime_error("selectScreen: the resource is not loaded");
        int64_t n = 0;
        pcr_screen_stats st{};
        loadedOn->check(pcr_read_screen(loadedOn->ctx, &p, rect, nullptr, nullptr, 0, &n, &st), "pcr_read_screen");
        if (points) points->resize((size_t)n);
        if (hits) hits->resize((size_t)n);
        if (n && (points || hits))
            loadedOn->check(pcr_read_screen(loadedOn->ctx, &p, rect, points ? points->data() : nullptr, hits ? hits->data() : nullptr, (size_t)n, &n, &st),
                            "pcr_read_screen");
        return st;
    }

    // Of selectScreen's hits those that make up the picture (pcr_read_visible: a counting call, then the read): mode
    // PCR_VISIBLE_FRONT / PCR_VISIBLE_SURFACE, radius = the occluder window. depth: the plane Dr of the whole image, width * height
    // words. Any vector may be NULL. Not in the reference.
    pcr_visible_stats selectVisible(const pcr_render_params &p, const pcr_rect *rect, int mode, int radius, std::vector<pcr_point> *points,
                                    std::vector<pcr_screen_hit> *hits, std::vector<uint32_t> *depth = nullptr)
    {
        if (!loadedOn) throw std::runtime_error("selectVisible: the resource is not loaded");
        int64_t n = 0;
        pcr_visible_stats st{};
        if (depth) depth->resize((size_t)p.width * (size_t)p.height);
        loadedOn->check(pcr_read_visible(loadedOn->ctx, &p, rect, mode, radius, nullptr, nullptr, depth ? depth->data() : nullptr, 0, &n, &st), "pcr_read_visible");
        if (points) points->resize((size_t)n);
        if (hits) hits->resize((size_t)n);
        if (n && (points || hits))
            loadedOn->check(pcr_read_visible(loadedOn->ctx, &p, rect, mode, radius, points ? points->data() : nullptr, hits ? hits->data() : nullptr, nullptr,
                                             (size_t)n, &n, &st), "pcr_read_visible");
        return st;
    }

    // The point under pixel (px, py) of a frame of camera `p`, within `radius` pixels (pcr_pick); false: none. Not in the reference.
    bool pick(const pcr_render_params &p, int px, int py, int radius, pcr_point &point, pcr_screen_hit &hit)
    {
        if (!loadedOn) throw std::runtime_error("pick: the resource is not loaded");
        int found = 0;
        loadedOn->check(pcr_pick(loadedOn->ctx, &p, px, py, radius, &point, &hit, &found), "pcr_pick");
        return found != 0;
    }

    // The three planes of `grid` (pcr_grid in pcr_types.h) over every batch the context holds right now, rasterized on the GPU in
    // one pass over the compressed stream (pcr_read_grid); clip may be NULL, a vector NULL leaves its plane out. Not in the reference.
    pcr_grid_stats readGrid(const pcr_grid &grid, const pcr_box *clip, std::vector<uint64_t> *top, std::vector<uint64_t> *bottom, std::vector<uint32_t> *count)
    {
        if (!loadedOn) throw std::runtime_error("readGrid: the resource is not loaded");
        const size_t cells = (size_t)std::max(grid.width, 0) * (size_t)std::max(grid.height, 0);
        if (top) top->resize(cells);
        if (bottom) bottom->resize(cells);
        if (count) count->resize(cells);
        pcr_grid_stats st{};
        loadedOn->check(pcr_read_grid(loadedOn->ctx, 0, pcr_batches_resident(loadedOn->ctx), &grid, clip, top ? top->data() : nullptr,
                                      bottom ? bottom->data() : nullptr, count ? count->data() : nullptr, 0, &st), "pcr_read_grid");
        return st;
    }

    // Exact percentiles of z per cell of `grid` over every batch the context holds right now (pcr_read_grid_quantiles): q in basis
    // points (1 .. PCR_QUANTILES_MAX of them), planes[j * cells + cell] the z of the nearest rank, INT32_MIN for a cell without
    // candidates; floor (the grid's cells, or NULL) admits only z >= floor[cell]; clip and count may be NULL. Not in the reference.
    pcr_quantile_stats heightQuantiles(const pcr_grid &grid, const pcr_box *clip, const std::vector<int32_t> *floor, const std::vector<uint32_t> &q,
                                       std::vector<int32_t> &planes, std::vector<uint32_t> *count)
    {
        if (!loadedOn) throw std::runtime_error("heightQuantiles: the resource is not loaded");
        const size_t cells = (size_t)std::max(grid.width, 0) * (size_t)std::max(grid.height, 0);
        if (floor && floor->size() != cells) throw std::runtime_error("heightQuantiles: the floor plane has not the grid's cells");
        planes.resize(cells * q.size());
        if (count) count->resize(cells);
        pcr_quantile_stats st{};
        loadedOn->check(pcr_read_grid_quantiles(loadedOn->ctx, 0, pcr_batches_resident(loadedOn->ctx), &grid, clip, floor ? floor->data() : nullptr, q.data(),
                                                (int32_t)q.size(), planes.data(), count ? count->data() : nullptr, 0, &st), "pcr_read_grid_quantiles");
        return st;
    }

    // The lowest-point plane of `grid` over every batch the context holds right now, its ground plane (the progressive morphological
    // filter and hole fill of pcr_ground_filter) and the classes of its cells, on the GPU in one call (pcr_read_ground); clip may be
    // NULL, a vector NULL leaves its plane out. Not in the reference.
    pcr_ground_stats groundModel(const pcr_grid &grid, const pcr_box *clip, const pcr_ground_params &gp, std::vector<int32_t> *lowest,
                                 std::vector<int32_t> *ground, std::vector<uint8_t> *classes)
    {
        if (!loadedOn) throw std::runtime_error("groundModel: the resource is not loaded");
        const size_t cells = (size_t)std::max(grid.width, 0) * (size_t)std::max(grid.height, 0);
        if (lowest) lowest->resize(cells);
        if (ground) ground->resize(cells);
        if (classes) classes->resize(cells);
        pcr_ground_stats st{};
        loadedOn->check(pcr_read_ground(loadedOn->ctx, 0, pcr_batches_resident(loadedOn->ctx), &grid, clip, &gp, lowest ? lowest->data() : nullptr,
                                        ground ? ground->data() : nullptr, classes ? classes->data() : nullptr, &st), "pcr_read_ground");
        return st;
    }

    // The points inside `clip` (NULL: everywhere) and the cells of `grid` whose height above `ground` (a plane of the grid's cells as
    // groundModel returns it, PCR_GROUND_EMPTY: no ground) lies in h_min .. h_max, with PCR_HEIGHT_REPLACE_Z in flags their z
    // replaced by the height, selected on the GPU (pcr_read_height: a counting call, then the read; the plane goes to the device for
    // the call). heights may be NULL. Not in the reference.
    pcr_height_stats pointsByHeight(const pcr_grid &grid, const std::vector<int32_t> &ground, const pcr_box *clip, int32_t h_min, int32_t h_max,
                                    uint32_t flags, std::vector<pcr_point> &out, std::vector<int32_t> *heights = nullptr)
    {
        if (!loadedOn) throw std::runtime_error("pointsByHeight: the resource is not loaded");
        const size_t cells = (size_t)std::max(grid.width, 0) * (size_t)std::max(grid.height, 0);
        if (ground.size() < cells || cells == 0) throw std::runtime_error("pointsByHeight: the ground plane is smaller than the grid");
        struct DevicePlane {
            void *p = nullptr;
            ~DevicePlane() { if (p) (void)hipFree(p); }
        } d;
        if (hipMalloc(&d.p, cells * sizeof(int32_t)) != hipSuccess || hipMemcpy(d.p, ground.data(), cells * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("pointsByHeight: no device memory for the ground plane");
        const int64_t nB = pcr_batches_resident(loadedOn->ctx);
        int64_t n = 0;
        pcr_height_stats st{};
        loadedOn->check(pcr_read_height(loadedOn->ctx, 0, nB, &grid, d.p, clip, h_min, h_max, flags, nullptr, nullptr, 0, &n, &st), "pcr_read_height");
        out.resize((size_t)n);
        if (heights) heights->resize((size_t)n);
        if (n) loadedOn->check(pcr_read_height(loadedOn->ctx, 0, nB, &grid, d.p, clip, h_min, h_max, flags, out.data(), heights ? heights->data() : nullptr,
                                               out.size(), &n, &st), "pcr_read_height");
        return st;
    }

    // Scale, offset and box of the LAS file the stream was made from, as the first batch record carries them
    // (include/BatchDumpData.h:60-107: doubles at 20 and 44, the LAS box as floats at 92 and 104).
    pcr_las_info lasInfo() const
    {
        std::ifstream f(path, std::ios::binary);
        char r[PCR_BATCH_FIXED_HEADER];
        f.seekg(offsetToBatchData);
        f.read(r, sizeof r);
        if (!f) throw std::runtime_error(path + ": short read on the first batch record");
        pcr_las_info las;
        float lmin[3], lmax[3];
        std::memcpy(las.scale, r + 20, 24); std::memcpy(las.offset, r + 44, 24);
        std::memcpy(lmin, r + 92, 12); std::memcpy(lmax, r + 104, 12);
        for (int k = 0; k < 3; ++k) { las.min[k] = lmin[k]; las.max[k] = lmax[k]; }
        return las;
    }

private:
    void stopReader()
    {
        {
            std::lock_guard<std::mutex> lock(mtx_state);
            if (state == LOADING) state = UNLOADING;
        }
        {
            std::lock_guard<std::mutex> lock(mtx_tasks);
            task = nullptr;
        }
        if (reader.joinable()) reader.join();
    }
};

struct HuffmanMethodBase : Method {
    std::shared_ptr<HuffmanLasData> las;
    Renderer *renderer;
    pcr_render_params lastParams{};
    HuffmanMethodBase(Renderer *r, std::shared_ptr<HuffmanLasData> l) : las(std::move(l)), renderer(r) { group = "none"; }

    void update(Renderer *r) override                      // huffman_hqs.h:116-124
    {
        if (Runtime::resource != (Resource *)las.get()) {
            if (Runtime::resource != nullptr) Runtime::resource->unload(r);
            las->load(r);
            Runtime::resource = (Resource *)las.get();
        }
    }
};

// One frame = CLEAR (of the previous frame) + RENDER + RESOLVE. The reference clears at the end of render()
// (huffman_mem_iter_cuda.h:250-252); headless callers read the result, so the clear opens the next frame instead.
struct HuffmanMemIter : HuffmanMethodBase {
    HuffmanMemIter(Renderer *r, std::shared_ptr<HuffmanLasData> l) : HuffmanMethodBase(r, std::move(l))
    {
        name = "huffman_mem_iter_cuda";
        description = "- Decodes Huffman Encoded values on the GPU";
    }
    void render(Renderer *r) override                      // huffman_mem_iter_cuda.h:122-254
    {
        las->process(r);
        if (las->numPointsLoaded == 0) return;
        lastParams = r->params();
        r->check(pcr_frame_begin(r->ctx, &lastParams, PCR_METHOD_BASIC), "pcr_frame_begin");   // CLEAR + cull/LOD prepass
        r->check(pcr_render_basic(r->ctx, &lastParams), "pcr_render_basic");
        if (display) r->check(pcr_resolve_basic_display(r->ctx, &lastParams, &*display), "pcr_resolve_basic_display");
        else r->check(pcr_resolve_basic(r->ctx, &lastParams), "pcr_resolve_basic");
    }
};

// The largest int32 box whose points i satisfy lo <= i * scale + offset <= hi on every axis, the expression evaluated in double
// as written (a product rounded, then a sum rounded: two statements, so no compiler contracts them). floor / ceil of the inverse
// give a guess, which is then moved by evaluating the expression until the bound and its outer neighbour disagree. An axis no
// int32 coordinate satisfies makes the box empty (min > max). The Python twin is host.box_from_world.
inline pcr_box boxFromWorld(const pcr_las_info &las, const double lo[3], const double hi[3])
{
    pcr_box b{};
    for (int k = 0; k < 3; ++k) {
        const double s = las.scale[k], o = las.offset[k];
        if (!(s > 0.0) || o != o || lo[k] != lo[k] || hi[k] != hi[k]) throw std::runtime_error("boxFromWorld: needs a positive scale and numbers for offset and bounds");
        auto f = [&](int64_t i) { const double p = (double)i * s; return p + o; };
        auto guess = [&](double v, bool up) -> int64_t {
            const double g = (v - o) / s;
            return g <= (double)INT32_MIN ? (int64_t)INT32_MIN : g >= (double)INT32_MAX ? (int64_t)INT32_MAX : (int64_t)(up ? std::ceil(g) : std::floor(g));
        };
        int64_t a = guess(lo[k], true);
        while (a > INT32_MIN && f(a - 1) >= lo[k]) --a;
        while (a <= INT32_MAX && f(a) < lo[k]) ++a;
        int64_t z = guess(hi[k], false);
        while (z < INT32_MAX && f(z + 1) <= hi[k]) ++z;
        while (z >= INT32_MIN && f(z) > hi[k]) --z;
        if (a > z) { a = 0; z = -1; }
        b.min[k] = (int32_t)a; b.max[k] = (int32_t)z;
    }
    return b;
}

// A pcr_polygon with the arrays it points to.
struct PolygonOwner {
    std::vector<int32_t> xy, ring_sizes;
    pcr_polygon poly{};
    PolygonOwner() = default;
    PolygonOwner(const PolygonOwner &) = delete;
    PolygonOwner &operator=(const PolygonOwner &) = delete;
};

// The polygon prism of rings given in world coordinates (xy: x0, y0, x1, y1, ... ring after ring): a vertex goes to the nearest
// lattice step, nearbyint((v - offset) / scale) in double (round to nearest even, the default mode), which moves it by at most half
// a step; z_lo / z_hi (NULL: unbounded) follow boxFromWorld's rule. A vertex beyond int32 is refused. The Python twin is
// host.polygon_from_world.
inline void polygonFromWorld(const pcr_las_info &las, const std::vector<double> &xy, const std::vector<int32_t> &ring_sizes, const double *z_lo,
                             const double *z_hi, bool invert, PolygonOwner &out)
{
    out.xy.resize(xy.size());
    for (size_t i = 0; i < xy.size(); ++i) {
        const double s = las.scale[i & 1], o = las.offset[i & 1];
        if (!(s > 0.0)) throw std::runtime_error("polygonFromWorld: needs a positive scale");
        const double v = std::nearbyint((xy[i] - o) / s);
        if (!(v >= (double)INT32_MIN && v <= (double)INT32_MAX)) throw std::runtime_error("polygonFromWorld: a vertex lies beyond the int32 lattice of the stream");
        out.xy[i] = (int32_t)v;
    }
    out.ring_sizes = ring_sizes;
    const double inf = std::numeric_limits<double>::infinity();
    const double l3[3] = {-inf, -inf, z_lo ? *z_lo : -inf}, h3[3] = {inf, inf, z_hi ? *z_hi : inf};
    const pcr_box b = boxFromWorld(las, l3, h3);
    out.poly = pcr_polygon{out.xy.data(), out.ring_sizes.data(), (int32_t)out.ring_sizes.size(), b.min[2], b.max[2], invert ? PCR_POLY_INVERT : 0u, 0u};
}

// The grid of square cells of `cell_size` world units over lo <= x, y <= hi: the origin is the first lattice point at or above lo on
// each axis (boxFromWorld's), the cell the whole number of lattice steps cell_size is on x and on y (it has to be one, the same
// on both, at least 1), width and height reach the last lattice point at or below hi. The Python twin is host.grid_from_world.
inline pcr_grid gridFromWorld(const pcr_las_info &las, const double lo[2], const double hi[2], double cell_size)
{
    int64_t cells[2];
    for (int k = 0; k < 2; ++k) {
        const double s = las.scale[k];
        if (!(s > 0.0) || !(cell_size > 0.0)) throw std::runtime_error("gridFromWorld: needs positive scales and a positive cell size");
        const double n = std::nearbyint(cell_size / s);
        if (!(n >= 1.0) || n > (double)INT32_MAX || std::fabs(n * s - cell_size) > 1e-9 * cell_size)
            throw std::runtime_error("gridFromWorld: the cell size is not a whole number of lattice steps");
        cells[k] = (int64_t)n;
    }
    if (cells[0] != cells[1]) throw std::runtime_error("gridFromWorld: the cell size is a different number of lattice steps on x and on y");
    const double inf = std::numeric_limits<double>::infinity();
    const double l3[3] = {lo[0], lo[1], -inf}, h3[3] = {hi[0], hi[1], inf};
    const pcr_box b = boxFromWorld(las, l3, h3);
    if (b.min[0] > b.max[0] || b.min[1] > b.max[1]) throw std::runtime_error("gridFromWorld: the range holds no lattice point");
    const int64_t w = ((int64_t)b.max[0] - b.min[0]) / cells[0] + 1, h = ((int64_t)b.max[1] - b.min[1]) / cells[0] + 1;
    if (w * h > PCR_GRID_MAX_CELLS) throw std::runtime_error("gridFromWorld: more cells than PCR_GRID_MAX_CELLS");
    return pcr_grid{b.min[0], b.min[1], (int32_t)cells[0], (int32_t)w, (int32_t)h, 0};
}

// Zhang et al.'s schedule for a ground filter over cells of `cell_size` world units: radii 1, 2, 4, ... cells while the window
// (2 r + 1) * cell_size is at most max_window (at least one step, at most PCR_GROUND_MAX_STEPS, r <= PCR_GROUND_MAX_RADIUS); with w_k
// the window of step k the thresholds are dh_0 = initial_distance, dh_k = min(max_distance, slope * (w_k - w_(k-1)) + initial_distance),
// in the stream's z units nearbyint(dh_k / scale_z). The Python twin is host.ground_params_from_world.
inline pcr_ground_params groundParamsFromWorld(const pcr_las_info &las, double cell_size, double slope = 1.0, double initial_distance = 0.15,
                                               double max_distance = 2.5, double max_window = 33.0, int fill_rounds = PCR_GROUND_MAX_FILL)
{
    if (!(las.scale[2] > 0.0) || !(cell_size > 0.0)) throw std::runtime_error("groundParamsFromWorld: needs a positive z scale and a positive cell size");
    pcr_ground_params gp{};
    gp.fill_rounds = fill_rounds;
    double prev = 0.0;
    for (int r = 1; gp.num_steps < PCR_GROUND_MAX_STEPS && r <= PCR_GROUND_MAX_RADIUS; r *= 2) {
        const double w = (2.0 * r + 1.0) * cell_size;
        if (gp.num_steps > 0 && w > max_window) break;
        const double dh = gp.num_steps == 0 ? initial_distance : std::min(max_distance, slope * (w - prev) + initial_distance);
        gp.radius[gp.num_steps] = r;
        gp.threshold[gp.num_steps] = (int32_t)std::min((double)INT32_MAX, std::max(0.0, std::nearbyint(dh / las.scale[2])));
        ++gp.num_steps;
        prev = w;
    }
    return gp;
}

// The lattice of cubic voxels of `cell_size` world units with the min corner of voxel (0, 0, 0) at the first lattice point at or above
// `origin` on each axis (boxFromWorld's): cell_size has to be the same whole number (1 .. PCR_THIN_MAX_CELL) of steps of the x, the y
// and the z lattice. The Python twin is host.voxels_from_world.
inline pcr_voxels voxelsFromWorld(const pcr_las_info &las, double cell_size, const double origin[3])
{
    int64_t cells[3];
    for (int k = 0; k < 3; ++k) {
        const double s = las.scale[k];
        if (!(s > 0.0) || !(cell_size > 0.0)) throw std::runtime_error("voxelsFromWorld: needs positive scales and a positive cell size");
        const double n = std::nearbyint(cell_size / s);
        if (!(n >= 1.0) || n > (double)PCR_THIN_MAX_CELL || std::fabs(n * s - cell_size) > 1e-9 * cell_size)
            throw std::runtime_error("voxelsFromWorld: the cell size is not a whole number (1 .. 2^30) of lattice steps");
        cells[k] = (int64_t)n;
    }
    if (cells[0] != cells[1] || cells[0] != cells[2]) throw std::runtime_error("voxelsFromWorld: the cell size is a different number of lattice steps on x, y and z");
    const double inf = std::numeric_limits<double>::infinity();
    const double h3[3] = {inf, inf, inf};
    const pcr_box b = boxFromWorld(las, origin, h3);
    for (int k = 0; k < 3; ++k) if (b.min[k] > b.max[k]) throw std::runtime_error("voxelsFromWorld: the origin lies beyond every int32 coordinate");
    return pcr_voxels{{b.min[0], b.min[1], b.min[2]}, (int32_t)cells[0]};
}

// The nested lattices pcr_lod_order takes for a finest cell of `cell_size` world units and `levels` levels, each coarser level with
// cells twice as large: voxelsFromWorld's lattice as the finest. levels in 1 .. PCR_LOD_MAX_LEVELS, the coarsest cell at most
// PCR_THIN_MAX_CELL lattice steps. The Python twin is host.lod_from_world.
inline pcr_lod lodFromWorld(const pcr_las_info &las, double cell_size, int levels, const double origin[3])
{
    if (levels < 1 || levels > PCR_LOD_MAX_LEVELS) throw std::runtime_error("lodFromWorld: the number of levels is 1 .. 16");
    const pcr_voxels vox = voxelsFromWorld(las, cell_size, origin);
    if (((int64_t)vox.cell << (levels - 1)) > PCR_THIN_MAX_CELL) throw std::runtime_error("lodFromWorld: the coarsest cell is more than 2^30 lattice steps");
    return pcr_lod{{vox.origin[0], vox.origin[1], vox.origin[2]}, vox.cell, levels, 0};
}

// The slab of the points within `distance` world units of the plane through `point` with the normal `normal` (world coordinates, any
// length). In lattice coordinates the form is (nw_a * scale_a) . p: n_a = rint(nw_a * scale_a * k) with k = 2^20 / max |nw_a * scale_a|,
// p = rint((point - offset) / scale), d = n . p exactly, the tolerance floor(distance * |nw| * k) in double. The Python twin is
// host.slab_from_world.
inline pcr_slab slabFromWorld(const pcr_las_info &las, const double point[3], const double normal[3], double distance)
{
    double w[3], m = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!(las.scale[k] > 0.0) || !std::isfinite(point[k]) || !std::isfinite(las.offset[k])) throw std::runtime_error("slabFromWorld: needs a positive scale and a finite point");
        w[k] = normal[k] * las.scale[k];
        if (!std::isfinite(w[k])) throw std::runtime_error("slabFromWorld: the normal is not finite");
        m = std::max(m, std::fabs(w[k]));
    }
    if (!(m > 0.0)) throw std::runtime_error("slabFromWorld: the normal is zero");
    if (!(distance >= 0.0) || !std::isfinite(distance)) throw std::runtime_error("slabFromWorld: needs a finite distance that is not negative");
    const double k = (double)PCR_SLAB_MAX_NORMAL / m;
    pcr_slab s{};
    int64_t d = 0;
    for (int a = 0; a < 3; ++a) {
        s.n[a] = (int32_t)std::nearbyint(w[a] * k);
        const double p = std::nearbyint((point[a] - las.offset[a]) / las.scale[a]);
        if (!(p >= (double)INT32_MIN && p <= (double)INT32_MAX)) throw std::runtime_error("slabFromWorld: the point lies beyond the int32 lattice of the stream");
        d += (int64_t)s.n[a] * (int64_t)p;
    }
    const double len = std::sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
    const double t = std::floor(distance * len * k);
    if (!(t <= (double)PCR_SLAB_MAX_BOUND / 2)) throw std::runtime_error("slabFromWorld: the distance is beyond the bounds of a slab");
    s.lo = d - (int64_t)t;
    s.hi = d + (int64_t)t;
    return s;
}

// The largest whole number r of lattice steps with r * scale <= radius (as doubles): the radius pcr_neighbors takes for `radius`
// world units. The three scales have to be equal and r in 1 .. PCR_NEIGHBORS_MAX_RADIUS. The Python twin is host.radius_from_world.
inline int32_t radiusFromWorld(const pcr_las_info &las, double radius)
{
    const double s = las.scale[0];
    if (las.scale[1] != s || las.scale[2] != s) throw std::runtime_error("radiusFromWorld: the scales of x, y and z differ");
    if (!(s > 0.0) || !(radius > 0.0) || radius == std::numeric_limits<double>::infinity()) throw std::runtime_error("radiusFromWorld: needs a positive scale and a positive finite radius");
    int64_t r = (int64_t)std::min(radius / s, (double)PCR_NEIGHBORS_MAX_RADIUS + 1.0);
    while ((double)r * s > radius) --r;
    while (r <= PCR_NEIGHBORS_MAX_RADIUS && (double)(r + 1) * s <= radius) ++r;
    if (r < 1 || r > PCR_NEIGHBORS_MAX_RADIUS) throw std::runtime_error("radiusFromWorld: the radius is not 1 .. 2^20 lattice steps");
    return (int32_t)r;
}

// modules/huffman_cuda/huffman_cuda.h:60-75: the reference's first Huffman method (class ComputeHuffman, registered as
// "huffman_cuda"; commented out in its main.cpp:19, 265 in favour of huffman_mem_iter_cuda, whose kernels are the same
// decode + {depth, BC1 colour} atomicMin with the loader's memory iteration added). The name north_star lists: the same frame
// as HuffmanMemIter under the reference's original method name.
struct ComputeHuffman : HuffmanMemIter {
    ComputeHuffman(Renderer *r, std::shared_ptr<HuffmanLasData> l) : HuffmanMemIter(r, std::move(l)) { name = "huffman_cuda"; }
};

struct HuffmanHQS : HuffmanMethodBase {
    HuffmanHQS(Renderer *r, std::shared_ptr<HuffmanLasData> l) : HuffmanMethodBase(r, std::move(l))
    {
        name = "huffman_hqs";
        description = "- Decodes Huffman Encoded values on the GPU";
    }
    void render(Renderer *r) override                      // huffman_hqs.h:126-273
    {
        las->process(r);
        if (las->numPointsLoaded == 0) return;
        lastParams = r->params();
        r->check(pcr_frame_begin(r->ctx, &lastParams, PCR_METHOD_HQS), "pcr_frame_begin");
        r->check(pcr_render_hqs_depth(r->ctx, &lastParams), "pcr_render_hqs_depth");
        r->check(pcr_render_hqs_color(r->ctx, &lastParams), "pcr_render_hqs_color");
        if (Debug::saveDepthMap) {                          // huffman_hqs.h:217-237
            dumpDepthMap(r, r->ctx, r->width, r->height, Debug::depthMapPath);
            Debug::saveDepthMap = false;
        }
        if (display) r->check(pcr_resolve_hqs_display(r->ctx, &lastParams, &*display), "pcr_resolve_hqs_display");
        else r->check(pcr_resolve_hqs(r->ctx, &lastParams), "pcr_resolve_hqs");
    }
};

// modules/compute/ComputeLasLoader.{h,cpp}: the LAS file is quantised task by task (<= 100 batches per frame, the
// reference's MAX_POINTS_PER_BATCH load buffer) into the three 10-10-10 levels. The reference quantises in a compute
// shader on upload (computeLasLoader.cs); here libpcr_host.so does it (pcr_las_quantize).
struct ComputeLasData : Resource {
    std::string path;
    LasPoints pts;
    int64_t numPoints = 0, numPointsLoaded = 0, numBatchesLoaded = 0;

    static std::shared_ptr<ComputeLasData> create(const std::string &path)      // ComputeLasLoader.h:97-103
    {
        auto d = std::make_shared<ComputeLasData>();
        d->path = path;
        std::string err;
        if (!read_las(path, d->pts, err)) throw std::runtime_error(err);
        d->numPoints = d->pts.numPoints;
        return d;
    }

    void load(Renderer *renderer) override                                       // ComputeLasLoader.cpp:14-38
    {
        if (state != UNLOADED) return;
        state = LOADING;
        renderer->check(pcr_las_begin(renderer->ctx, numPoints), "pcr_las_begin");
        numPointsLoaded = numBatchesLoaded = 0;
    }

    void process(Renderer *renderer) override                                    // ComputeLasLoader.cpp:140-262
    {
        if (state != LOADING) return;
        const int64_t first = numPointsLoaded, n = std::min<int64_t>(numPoints - first, PCR_DEFAULT_CHUNK_POINTS);
        const int64_t nb = (n + PCR_POINTS_PER_BATCH - 1) / PCR_POINTS_PER_BATCH;
        const size_t slots = (size_t)nb * PCR_POINTS_PER_BATCH;
        std::vector<pcr_xyz_batch> batches((size_t)nb);
        std::vector<uint32_t> xyz12(slots), xyz8(slots), xyz4(slots), rgba(slots);
        if (pcr_las_quantize(pts.x.data() + first, pts.y.data() + first, pts.z.data() + first, pts.color.data() + first, n,
                             &pts.las, batches.data(), xyz12.data(), xyz8.data(), xyz4.data(), rgba.data(), 0))
            throw std::runtime_error(std::string("pcr_las_quantize: ") + pcr_host_last_error());
        renderer->check(pcr_las_upload(renderer->ctx, numBatchesLoaded, nb, batches.data(), xyz12.data(), xyz8.data(),
                                       xyz4.data(), rgba.data()), "pcr_las_upload");
        numPointsLoaded += n;
        numBatchesLoaded = pcr_las_batches_loaded(renderer->ctx);
        if (numPointsLoaded == numPoints) state = LOADED;
    }

    void unload(Renderer *renderer) override                                     // ComputeLasLoader.cpp:114-131
    {
        numPointsLoaded = numBatchesLoaded = 0;
        pcr_las_unload(renderer->ctx);
        state = UNLOADED;
    }

    bool fullyLoaded() const { return numPointsLoaded == numPoints; }
};

struct ComputeLoopLasCUDA : Method {                                             // compute_loop_las_cuda.h:52-222
    std::shared_ptr<ComputeLasData> las;
    Renderer *renderer;
    pcr_render_params lastParams{};
    ComputeLoopLasCUDA(Renderer *r, std::shared_ptr<ComputeLasData> l) : las(std::move(l)), renderer(r)
    {
        name = "loop_las_cuda";
        description = "- Each thread renders X points.\n- Loads points from LAS file\n- Workgroup picks 4, 8, or 12 byte precision\n  depending on screen size of bounding box";
        group = "10-10-10 bit encoded";
    }
    void update(Renderer *r) override        // empty in the reference (:92-93); resource switch as huffman_hqs.h:116-124
    {
        if (Runtime::resource != (Resource *)las.get()) {
            if (Runtime::resource != nullptr) Runtime::resource->unload(r);
            las->load(r);
            Runtime::resource = (Resource *)las.get();
        }
    }
    void render(Renderer *r) override                                            // compute_loop_las_cuda.h:99-222
    {
        las->process(r);
        if (las->numPointsLoaded == 0) return;
        lastParams = r->params();
        r->check(pcr_clear(r->ctx), "pcr_clear");
        r->check(pcr_render_las(r->ctx, &lastParams), "pcr_render_las");
        if (display) r->check(pcr_resolve_las_display(r->ctx, &lastParams, &*display), "pcr_resolve_las_display");
        else r->check(pcr_resolve_las(r->ctx, &lastParams), "pcr_resolve_las");
    }
};

struct ComputeLoopLasHQS : ComputeLoopLasCUDA {                                  // compute_loop_las_hqs.h:36-309
    ComputeLoopLasHQS(Renderer *r, std::shared_ptr<ComputeLasData> l) : ComputeLoopLasCUDA(r, std::move(l))
    {
        name = "loop_las_hqs";
        description = "Like compute las, but also \naverages overlapping points";
        group = "10-10-10 bit encoded";
    }
    void render(Renderer *r) override                                            // compute_loop_las_hqs.h:126-300
    {
        las->process(r);
        if (las->numPointsLoaded == 0) return;
        lastParams = r->params();
        r->check(pcr_clear(r->ctx), "pcr_clear");
        r->check(pcr_render_las_hqs_depth(r->ctx, &lastParams), "pcr_render_las_hqs_depth");   // DEPTH   (:172-196)
        r->check(pcr_render_las_hqs_color(r->ctx, &lastParams), "pcr_render_las_hqs_color");   // COLORS  (:199-223)
        if (display) r->check(pcr_resolve_hqs_display(r->ctx, &lastParams, &*display), "pcr_resolve_hqs_display");
        else r->check(pcr_resolve_hqs(r->ctx, &lastParams), "pcr_resolve_hqs");                     // RESOLVE (:226-245)
    }
};

} // namespace pcr_host
