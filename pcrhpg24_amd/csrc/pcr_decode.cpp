// pcr_decode — a .huffman file back to a LAS file, decoded on the GPU (pcr_read_points). The reference has no such tool: its only
// decoder outside the render kernels is the per-chain CPU one of include/huffman.h:433-477.
//     pcr_decode <in.huffman> <out.las> [--box x0 y0 z0 x1 y1 z1]
// Loads the file with the loader of the render tools (HuffmanLasData, csrc/pcr_methods.hpp), reads the points back in pieces of
// 64 batches and writes LAS 1.2 / point format 2 (pcr_write_las_points). With --box only the points inside a box of world
// coordinates are read back (pcr_read_box: batches the box misses are not decoded).
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pcr_methods.hpp"

using namespace pcr_host;

static const char *USAGE =
    "usage: pcr_decode <in.huffman> <out.las> [--box x0 y0 z0 x1 y1 z1]\n"
    "  Decodes every point of the stream on the GPU and writes a LAS 1.2 file (point format 2, 26-byte records).\n"
    "  A .huffman header stores the point count after padding only (a multiple of 65536: the encoder repeats the last\n"
    "  point), so the LAS file holds the padded count. Points come in the stream's order (Morton-sorted per chunk if the\n"
    "  file was encoded that way); colours are the decoded BC1 / BC7 colours; of a stream written without --pad-tails a\n"
    "  thousandth of the points are the tail artefact the render kernels draw as well. The header's scale and offset are\n"
    "  the first batch record's, its min / max the cloud's box as that record carries it (single precision).\n"
    "  --box: only the points p with x0 <= p.x <= x1, y0 <= p.y <= y1, z0 <= p.z <= z1 in world coordinates (integer * scale +\n"
    "  offset, in double precision), selected on the GPU, in the stream's order. A box that holds no point is an error.\n";

// six finite numbers behind --box, or false
static bool parse_box(int argc, char **argv, int at, double lo[3], double hi[3])
{
    if (argc != at + 7 || std::strcmp(argv[at], "--box") != 0) return false;
    for (int k = 0; k < 6; ++k) {
        const char *a = argv[at + 1 + k];
        char *end = nullptr;
        errno = 0;
        const double v = std::strtod(a, &end);
        if (end == a || *end != '\0' || errno == ERANGE || !std::isfinite(v)) return false;
        (k < 3 ? lo[k] : hi[k - 3]) = v;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && (std::strcmp(argv[1], "--help") == 0 || std::strcmp(argv[1], "-h") == 0)) { std::fputs(USAGE, stdout); return 0; }
    double lo[3], hi[3];
    const bool boxed = argc > 3;
    if (argc < 3 || (boxed && !parse_box(argc, argv, 3, lo, hi))) { std::fputs(USAGE, stderr); return 2; }
    const std::string in = argv[1], out = argv[2];
    try {
        Renderer renderer(64, 64, 0);
        auto las = HuffmanLasData::create(in);
        las->load(&renderer);
        // (process() hands the reader thread's tasks over, and throws the reader's error if it had to give up)
        auto progress = std::chrono::steady_clock::now();
        for (int64_t seen = 0; !las->fullyLoaded();) {
            las->process(&renderer);
            const auto now = std::chrono::steady_clock::now();
            if (las->numBatchesLoaded != seen) { seen = las->numBatchesLoaded; progress = now; }
            else if (now - progress > std::chrono::seconds(120)) throw std::runtime_error("loader made no progress");
            else std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        std::vector<pcr_point> points;
        const pcr_las_info info = las->lasInfo();
        if (boxed) {
            const pcr_select_stats st = las->selectBox(boxFromWorld(info, lo, hi), points);
            std::printf("box: batches outside %lld, inside %lld, straddling %lld\n", (long long)st.batches_outside, (long long)st.batches_inside,
                        (long long)st.batches_straddling);
            if (points.empty()) throw std::runtime_error("no points inside the box: nothing written");
        } else {
            las->decodePoints(points);
        }
        las->unload(&renderer);
        if (pcr_write_las_points(out.c_str(), points.data(), (int64_t)points.size(), &info))
            throw std::runtime_error(std::string("pcr_write_las_points: ") + pcr_host_last_error());
        std::printf("points %lld (batches %lld) -> %s\n", (long long)points.size(), (long long)las->numBatches, out.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pcr_decode: %s\n", e.what());
        return 1;
    }
    return 0;
}
