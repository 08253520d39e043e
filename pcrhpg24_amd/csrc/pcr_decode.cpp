// pcr_decode — a .huffman file back to a LAS file, decoded on the GPU (pcr_read_points). The reference has no such tool: its only
// decoder outside the render kernels is the per-chain CPU one of include/huffman.h:433-477.
//     pcr_decode <in.huffman> <out.las> [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --thin CELL [--center | --mean] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --lod CELL LEVELS [--drop-rest] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --denoise CELL MAXCOUNT [--isolated] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --components CELL MINPOINTS [--conn 6|26] [--small] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --radius R MINCOUNT [--sparse] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.ply> --normals R [MINCOUNT] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --sor K MULT R [--outliers] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --polygon FILE [--z LO HI] [--outside]
//     pcr_decode <in.huffman> <out.las> --slab px py pz nx ny nz DIST [--outside] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --view [--size WxH] [--camera yaw pitch radius tx ty tz] [--lod f] [--cull 0|1] [--rect x0 y0 x1 y1]
//                                                [--visible front|surface [--occluder R]]
//     pcr_decode <in.huffman> <out.ppm> --ortho CELL [--box x0 y0 z0 x1 y1 z1] [--dsm out.asc]
//     pcr_decode <in.huffman> <out.asc> --percentile P CELL [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.asc> --dtm CELL [--slope S] [--max-window W] [--initial D] [--max-distance D] [--box x0 y0 z0 x1 y1 z1]
//     pcr_decode <in.huffman> <out.las> --height CELL LO HI [--normalize] [--slope S] [--max-window W] [--initial D] [--max-distance D] [--box ...]
// Loads the file with the loader of the render tools (HuffmanLasData, csrc/pcr_methods.hpp), reads the points back in pieces of
// 64 batches and writes LAS 1.2 / point format 2 (pcr_write_las_points). With --box only the points inside a box of world
// coordinates are read back (pcr_read_box: batches the box misses are not decoded). With --view only the points a frame of that
// camera draws (pcr_render's camera arguments and defaults), and of those the ones inside --rect, a rectangle of pixels
// (pcr_read_screen); with --visible of those only the ones that make up the picture (pcr_read_visible). With --ortho no points are read back at all: the stream is rasterized top-down on the GPU (pcr_read_grid) into
// an orthophoto and, with --dsm, a surface model. With --thin one point per cubic voxel is read back (pcr_read_thin): the cloud
// decimated on the GPU without ever existing in full. With --lod the points come back ordered by nested voxel lattices, coarse
// to fine (pcr_read_lod_order): a file whose every prefix up to a level boundary is a thinned cloud. With --polygon only the points inside a polygon prism of world coordinates are
// read back (pcr_read_polygon). With --denoise the points come back without the isolated ones, or those alone (pcr_read_denoise).
// With --components they come back without the connected components of voxels below a size, or those alone (pcr_read_components).
// With --radius they come back without those that have fewer than a number of points within a radius, or those alone: the radius
// outlier filter on actual point pairs (pcr_read_neighbors). With --normals the points come back with the normal and the curvature
// of their neighbourhood within a radius, as a PLY (pcr_read_local_moments). With --sor they come back without the statistical
// outliers -- by the mean distance to their k nearest neighbours within a radius -- or those alone (pcr_read_knn).
// With --dtm the lowest-point grid goes through the ground filter on the GPU (pcr_read_ground) and the terrain model is written;
// with --height the points whose height above that model lies in a range are read back (pcr_read_height). With --percentile the
// exact P-th percentile of z per cell is written like --dsm's surface model (pcr_read_grid_quantiles).
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "pcr_methods.hpp"

using namespace pcr_host;

static const char *USAGE =
    "usage: pcr_decode <in.huffman> <out.las> [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --thin CELL [--center | --mean] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --lod CELL LEVELS [--drop-rest] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --denoise CELL MAXCOUNT [--isolated] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --components CELL MINPOINTS [--conn 6|26] [--small] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --radius R MINCOUNT [--sparse] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.ply> --normals R [MINCOUNT] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --sor K MULT R [--outliers] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --polygon FILE [--z LO HI] [--outside]\n"
    "       pcr_decode <in.huffman> <out.las> --slab px py pz nx ny nz DIST [--outside] [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --view [--size WxH] [--camera yaw pitch radius tx ty tz] [--lod f] [--cull 0|1]\n"
    "                                                [--rect x0 y0 x1 y1] [--visible front|surface [--occluder R]]\n"
    "       pcr_decode <in.huffman> <out.ppm> --ortho CELL [--box x0 y0 z0 x1 y1 z1] [--dsm out.asc]\n"
    "       pcr_decode <in.huffman> <out.asc> --percentile P CELL [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.asc> --dtm CELL [--slope S] [--max-window W] [--initial D] [--max-distance D]\n"
    "                                                [--box x0 y0 z0 x1 y1 z1]\n"
    "       pcr_decode <in.huffman> <out.las> --height CELL LO HI [--normalize] [--slope S] [--max-window W] [--initial D]\n"
    "                                                [--max-distance D] [--box x0 y0 z0 x1 y1 z1]\n"
    "  Decodes every point of the stream on the GPU and writes a LAS 1.2 file (point format 2, 26-byte records).\n"
    "  A .huffman header stores the point count after padding only (a multiple of 65536: the encoder repeats the last\n"
    "  point), so the LAS file holds the padded count. Points come in the stream's order (Morton-sorted per chunk if the\n"
    "  file was encoded that way); colours are the decoded BC1 / BC7 colours; of a stream written without --pad-tails a\n"
    "  thousandth of the points are the tail artefact the render kernels draw as well. The header's scale and offset are\n"
    "  the first batch record's, its min / max the cloud's box as that record carries it (single precision).\n"
    "  --box: only the points p with x0 <= p.x <= x1, y0 <= p.y <= y1, z0 <= p.z <= z1 in world coordinates (integer * scale +\n"
    "  offset, in double precision), selected on the GPU, in the stream's order. A box that holds no point is an error.\n"
    "  --thin CELL: one point of every cubic voxel of CELL world units (a whole number of the stream's x, y and z lattice steps;\n"
    "  the lattice starts at the min corner of the header's box), thinned on the GPU, in the stream's order: the voxel's first\n"
    "  point in that order, with --center the one nearest to the voxel's centre, with --mean (not with --center) the mean of the\n"
    "  voxel's points instead, position and colour, rounded to the lattice. Only the points inside --box count, or inside\n"
    "  the box of the file's header. No point there is an error.\n"
    "  --lod CELL LEVELS: the points in level-of-detail order. LEVELS (1 .. 16) nested lattices of cubic voxels, the finest of\n"
    "  CELL world units (the lattice of --thin), every coarser one of twice the edge: first the points that are the first of their\n"
    "  voxel of the coarsest lattice, then those of the next finer one, and so on, last the points that are first in no voxel\n"
    "  (--drop-rest: without them); inside a level in the stream's order. The point records of the file cut off where a level\n"
    "  ends (the `level k: n` lines tell the counts) are --thin with that level's cell. Only the points inside --box count, or\n"
    "  inside the box of the file's header. No point there is an error. It combines with no other selecting option.\n"
    "  --denoise CELL MAXCOUNT: the points without the isolated ones, in the stream's order. A point is isolated if the 3 x 3 x 3\n"
    "  cubic voxels of CELL world units around its own (the lattice of --thin) hold at most MAXCOUNT points (a whole number >= 0),\n"
    "  the point itself and exact duplicates included. --isolated: the isolated points instead. Only the points inside --box\n"
    "  count, as neighbours too, or inside the box of the file's header. No point to write is an error.\n"
    "  --components CELL MINPOINTS: the points without the small blobs, in the stream's order. The occupied cubic voxels of CELL\n"
    "  world units (the lattice of --thin) that touch -- by a face, an edge or a corner, with --conn 6 by a face only -- form a\n"
    "  connected component; it is small if it holds fewer than MINPOINTS points (a whole number >= 0), exact duplicates\n"
    "  counted. --small: the points of the small components instead. Only the points inside --box count, or inside the box of\n"
    "  the file's header. No point to write is an error.\n"
    "  --radius R MINCOUNT: the radius outlier filter, exact: the points that have at least MINCOUNT points (a whole number >= 0)\n"
    "  within R world units, the point itself and exact duplicates included, in the stream's order. --sparse: the other points\n"
    "  instead. Only the points inside --box count, as neighbours too, or inside the box of the file's header. No point to write\n"
    "  is an error.\n"
    "  --normals R [MINCOUNT]: the points that have at least MINCOUNT points (a whole number >= 0, 3 if left out) within R world\n"
    "  units, the point itself and exact duplicates included, with the unit normal of that neighbourhood (the eigenvector of the\n"
    "  least eigenvalue of its covariance; z >= 0) and its curvature l0 / (l0 + l1 + l2), in the stream's order, as a binary\n"
    "  little-endian PLY: double x y z, uchar red green blue, float nx ny nz, float curvature. R is at most 32767 lattice steps.\n"
    "  Only the points inside --box count, as neighbours too, or inside the box of the file's header. No point to write is an\n"
    "  error.\n"
    "  --sor K MULT R: the statistical outlier filter with the search capped at R world units (at most 32767 lattice steps): per\n"
    "  point the mean distance to its K (1 .. 16) nearest other points within R, exact duplicates at distance 0; with mu and sigma\n"
    "  the mean and the population standard deviation of those means, the points whose mean is at most mu + MULT * sigma, in the\n"
    "  stream's order. A point with no other point within R is an outlier. --outliers: the outliers instead. Only the points\n"
    "  inside --box count, as neighbours too, or inside the box of the file's header. No point to write is an error.\n"
    "  --polygon FILE: only the points inside a polygon, selected on the GPU, in the stream's order. FILE is text in world\n"
    "  coordinates: one vertex `x y` per line, a blank line starts the next ring (a ring inside another is a hole: the even-odd\n"
    "  rule); a ring has at least 3 vertices and is closed implicitly, all rings together at most 4096. A vertex goes to the\n"
    "  nearest lattice step of the stream. The boundary is half-open: of two polygons that share an edge exactly one takes a\n"
    "  point on it. --z: of those the points with LO <= p.z <= HI; --outside: the points NOT inside the polygon (--z still\n"
    "  applies). A polygon that holds no point is an error.\n"
    "  --slab: only the points within DIST of the plane through (px, py, pz) with the normal (nx, ny, nz), world units, selected\n"
    "  on the GPU in the stream's order; the normal may have any length but zero. --outside: the other points. Only the points\n"
    "  inside --box count, or inside the box of the file's header. No point to write is an error. It combines with no other\n"
    "  selecting option.\n"
    "  --view: only the points a frame of that camera draws (the basic method's cull and level of detail; the options and their\n"
    "  defaults are pcr_render's), in the stream's order; --rect: of those the ones whose pixel lies in the rectangle (pixels,\n"
    "  bounds inclusive, x0 <= x1 and y0 <= y1). A view that shows no point is an error.\n"
    "  --visible: of those only the points that make up the picture, not what lies behind them. front: per pixel the one point\n"
    "  the frame shows (the nearest; ties by colour, then by position in the stream); surface: every point within 1 % of its\n"
    "  pixel's nearest depth. --occluder R (0 .. 8, default 0): a pixel's nearest depth is taken over the pixels within R columns\n"
    "  and rows as well, so that a surface with gaps between its points still hides what is behind it.\n"
    "  --ortho CELL: no LAS file; the stream is rasterized top-down on the GPU into square cells of CELL world units (a whole\n"
    "  number of the stream's x and y lattice steps) and the colour of the highest point of every cell is written as a binary\n"
    "  PPM (empty cells black), rows from north to south. The cells cover the x and y range of --box, of which z0 and z1 clip the\n"
    "  points, or the box of the file's header. --dsm: the height of that point as an ESRI ASCII grid (ncols, nrows, xllcorner,\n"
    "  yllcorner, cellsize, NODATA_value -9999; world units, %.17g), the same rows. A grid no point falls into is an error.\n"
    "  --percentile P CELL: no LAS file; the exact P-th percentile (0 .. 100, a whole number of hundredths) of the heights of every\n"
    "  cell of CELL world units as an ESRI ASCII grid like --dsm's: the z of the point of rank round(P / 100 * (n - 1)) among the\n"
    "  cell's n points sorted by z, a half rounded up, never interpolated. 95 or 99 is a surface model that one stray return does\n"
    "  not set, 2 or 5 a robust lowest plane. The cells cover the x and y range of --box, of which z0 and z1 clip the points, or\n"
    "  the box of the file's header. It combines with no other mode. A grid no point falls into is an error.\n"
    "  --dtm CELL: no LAS file; a terrain model as an ESRI ASCII grid like --dsm's. The lowest point of every cell of CELL world\n"
    "  units goes through a progressive morphological filter on the GPU: windows of 3, 5, 9, ... cells up to --max-window world\n"
    "  units (33), a cell being ground unless an opening lowers it by more than --initial (0.15) at the first window and\n"
    "  min(--max-distance (2.5), --slope (1.0) * the growth of the window + --initial) at the others; the other cells and the\n"
    "  empty ones take the mean of their 8 neighbours, round after round. The cells cover the x and y range of --box, of which\n"
    "  z0 and z1 clip the points, or the box of the file's header. A grid without a ground cell is an error.\n"
    "  --height CELL LO HI: the points whose height above that terrain model lies in LO .. HI world units (multiples of the z\n"
    "  scale), in the stream's order; --normalize: their z is the height. Only the points inside --box count, or inside the box\n"
    "  of the file's header. No point to write is an error.\n";

static bool parse_double(const char *a, double &v)
{
    char *end = nullptr;
    errno = 0;
    v = std::strtod(a, &end);
    return end != a && *end == '\0' && errno != ERANGE && std::isfinite(v);
}

static bool parse_int(const char *a, long lo, long hi, int &v)
{
    char *end = nullptr;
    errno = 0;
    const long x = std::strtol(a, &end, 10);
    if (end == a || *end != '\0' || errno == ERANGE || x < lo || x > hi) return false;
    v = (int)x;
    return true;
}

struct View {
    int w = 1920, h = 1080;
    double cam[6] = {-0.15, -0.57, 3166.32, 2239.05, 1713.63, -202.02};        // pcr_render's default
    double lod = 0.1;
    int cull = 1;
    bool has_rect = false;
    pcr_rect rect{};
    int visible = -1;                           // PCR_VISIBLE_*, -1: --visible not given
    int occluder = -1;                          // --occluder, -1: not given
};

// the options behind --view, every one well formed, or false
static bool parse_view(int argc, char **argv, int at, View &v)
{
    if (argc <= at || std::strcmp(argv[at], "--view") != 0) return false;
    for (int i = at + 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto have = [&](int n) { return i + n < argc; };
        if (a == "--size" && have(1)) {
            char tail = 0;
            if (std::sscanf(argv[++i], "%dx%d%c", &v.w, &v.h, &tail) != 2 || v.w < 1 || v.h < 1 || v.w > 16384 || v.h > 16384) return false;
        } else if (a == "--camera" && have(6)) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], v.cam[k])) return false;
        } else if (a == "--lod" && have(1)) {
            if (!parse_double(argv[++i], v.lod) || v.lod < 0.0 || v.lod > 1.0) return false;
        } else if (a == "--cull" && have(1)) {
            if (!parse_int(argv[++i], 0, 1, v.cull)) return false;
        } else if (a == "--rect" && have(4) && !v.has_rect) {
            int r[4];
            for (int k = 0; k < 4; ++k) if (!parse_int(argv[++i], INT32_MIN, INT32_MAX, r[k])) return false;
            if (r[0] > r[2] || r[1] > r[3]) return false;
            v.rect = pcr_rect{r[0], r[1], r[2], r[3]};
            v.has_rect = true;
        } else if (a == "--visible" && have(1) && v.visible < 0) {
            const std::string m = argv[++i];
            if (m == "front") v.visible = PCR_VISIBLE_FRONT;
            else if (m == "surface") v.visible = PCR_VISIBLE_SURFACE;
            else return false;
        } else if (a == "--occluder" && have(1) && v.occluder < 0) {
            if (!parse_int(argv[++i], 0, PCR_VISIBLE_MAX_RADIUS, v.occluder)) return false;
        } else {
            return false;
        }
    }
    return v.occluder < 0 || v.visible >= 0;    // (--occluder belongs to --visible)
}

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

struct Thin {
    double cell = 0.0;
    bool center = false, mean = false, has_box = false;
    double lo[3], hi[3];
};

// the options behind --thin, every one well formed, or false
static bool parse_thin(int argc, char **argv, int at, Thin &t)
{
    if (argc < at + 2 || std::strcmp(argv[at], "--thin") != 0) return false;
    if (!parse_double(argv[at + 1], t.cell) || !(t.cell > 0.0)) return false;
    for (int i = at + 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !t.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? t.lo[k] : t.hi[k - 3])) return false;
            t.has_box = true;
        } else if (a == "--center" && !t.center) {
            t.center = true;
        } else if (a == "--mean" && !t.mean) {
            t.mean = true;
        } else {
            return false;
        }
    }
    return !(t.center && t.mean);
}

struct Lod {
    double cell = 0.0;
    int levels = 0;
    bool drop_rest = false, has_box = false;
    double lo[3], hi[3];
};

// the options behind --lod, every one well formed, or false
static bool parse_lod(int argc, char **argv, int at, Lod &l)
{
    if (argc < at + 3 || std::strcmp(argv[at], "--lod") != 0) return false;
    if (!parse_double(argv[at + 1], l.cell) || !(l.cell > 0.0)) return false;
    char *end = nullptr;
    errno = 0;
    const long long levels = std::strtoll(argv[at + 2], &end, 10);
    if (end == argv[at + 2] || *end != '\0' || errno == ERANGE || levels < 1 || levels > PCR_LOD_MAX_LEVELS) return false;
    l.levels = (int)levels;
    for (int i = at + 3; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !l.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? l.lo[k] : l.hi[k - 3])) return false;
            l.has_box = true;
        } else if (a == "--drop-rest" && !l.drop_rest) {
            l.drop_rest = true;
        } else {
            return false;                                               // (--thin, --denoise, ...: it combines with no other mode)
        }
    }
    return true;
}

struct Denoise {
    double cell = 0.0;
    long long max_count = 0;
    bool isolated = false, has_box = false;
    double lo[3], hi[3];
};

// the options behind --denoise, every one well formed, or false
static bool parse_denoise(int argc, char **argv, int at, Denoise &d)
{
    if (argc < at + 3 || std::strcmp(argv[at], "--denoise") != 0) return false;
    if (!parse_double(argv[at + 1], d.cell) || !(d.cell > 0.0)) return false;
    char *end = nullptr;
    errno = 0;
    d.max_count = std::strtoll(argv[at + 2], &end, 10);
    if (end == argv[at + 2] || *end != '\0' || errno == ERANGE || d.max_count < 0) return false;
    for (int i = at + 3; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !d.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? d.lo[k] : d.hi[k - 3])) return false;
            d.has_box = true;
        } else if (a == "--isolated" && !d.isolated) {
            d.isolated = true;
        } else {
            return false;
        }
    }
    return true;
}

struct Radius {
    double radius = 0.0;
    long long min_count = 0;
    bool sparse = false, has_box = false;
    double lo[3], hi[3];
};

// the options behind --radius, every one well formed, or false
static bool parse_radius(int argc, char **argv, int at, Radius &r)
{
    if (argc < at + 3 || std::strcmp(argv[at], "--radius") != 0) return false;
    if (!parse_double(argv[at + 1], r.radius) || !(r.radius > 0.0)) return false;
    char *end = nullptr;
    errno = 0;
    r.min_count = std::strtoll(argv[at + 2], &end, 10);
    if (end == argv[at + 2] || *end != '\0' || errno == ERANGE || r.min_count < 0) return false;
    for (int i = at + 3; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !r.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? r.lo[k] : r.hi[k - 3])) return false;
            r.has_box = true;
        } else if (a == "--sparse" && !r.sparse) {
            r.sparse = true;
        } else {
            return false;
        }
    }
    return true;
}

struct Normals {
    double radius = 0.0;
    long long min_count = 3;
    bool has_box = false;
    double lo[3], hi[3];
};

// the options behind --normals, every one well formed, or false
static bool parse_normals(int argc, char **argv, int at, Normals &r)
{
    if (argc < at + 2 || std::strcmp(argv[at], "--normals") != 0) return false;
    if (!parse_double(argv[at + 1], r.radius) || !(r.radius > 0.0)) return false;
    int i = at + 2;
    if (i < argc && std::strncmp(argv[i], "--", 2) != 0) {
        char *end = nullptr;
        errno = 0;
        r.min_count = std::strtoll(argv[i], &end, 10);
        if (end == argv[i] || *end != '\0' || errno == ERANGE || r.min_count < 0) return false;
        ++i;
    }
    for (; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !r.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? r.lo[k] : r.hi[k - 3])) return false;
            r.has_box = true;
        } else {
            return false;
        }
    }
    return true;
}

struct Sor {
    int k = 0;
    double multiplier = 0.0, radius = 0.0;
    bool outliers = false, has_box = false;
    double lo[3], hi[3];
};

// the options behind --sor, every one well formed, or false
static bool parse_sor(int argc, char **argv, int at, Sor &r)
{
    if (argc < at + 4 || std::strcmp(argv[at], "--sor") != 0) return false;
    if (!parse_int(argv[at + 1], 1, PCR_KNN_MAX_K, r.k)) return false;
    if (!parse_double(argv[at + 2], r.multiplier) || r.multiplier < 0.0) return false;
    if (!parse_double(argv[at + 3], r.radius) || !(r.radius > 0.0)) return false;
    for (int i = at + 4; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !r.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? r.lo[k] : r.hi[k - 3])) return false;
            r.has_box = true;
        } else if (a == "--outliers" && !r.outliers) {
            r.outliers = true;
        } else {
            return false;
        }
    }
    return true;
}

// A binary little-endian PLY of the points in world coordinates with their colours, normals and curvatures
static void write_normals_ply(const std::string &path, const pcr_las_info &info, const std::vector<pcr_point> &points, const std::vector<pcr_eigen> &eigen)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error(path + ": cannot open for writing");
    std::fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment pcr_decode --normals\nelement vertex %zu\n"
                    "property double x\nproperty double y\nproperty double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                    "property float nx\nproperty float ny\nproperty float nz\nproperty float curvature\nend_header\n", points.size());
    std::vector<unsigned char> rec(3 * 8 + 3 + 4 * 4);
    for (size_t i = 0; i < points.size(); ++i) {
        const int32_t ints[3] = {points[i].x, points[i].y, points[i].z};
        double w[3];
        for (int k = 0; k < 3; ++k) {                       // (two roundings, as Python's x * scale + offset)
            const double scaled = (double)ints[k] * info.scale[k];
            w[k] = scaled + info.offset[k];
        }
        const pcr_eigen &e = eigen[i];
        const double sum = e.value[0] + e.value[1] + e.value[2];
        const float fl[4] = {(float)e.normal[0], (float)e.normal[1], (float)e.normal[2], (float)(sum != 0.0 ? e.value[0] / sum : 0.0)};
        const unsigned char rgb[3] = {(unsigned char)(points[i].color & 255u), (unsigned char)((points[i].color >> 8) & 255u),
                                      (unsigned char)((points[i].color >> 16) & 255u)};
        std::memcpy(rec.data(), w, 24); std::memcpy(rec.data() + 24, rgb, 3); std::memcpy(rec.data() + 27, fl, 16);
        if (std::fwrite(rec.data(), 1, rec.size(), f) != rec.size()) { std::fclose(f); throw std::runtime_error(path + ": write failed"); }
    }
    if (std::fclose(f) != 0) throw std::runtime_error(path + ": write failed");
}

struct Components {
    double cell = 0.0;
    long long min_points = 0;
    int conn = 26;
    bool small = false, has_box = false, has_conn = false;
    double lo[3], hi[3];
};

// the options behind --components, every one well formed, or false
static bool parse_components(int argc, char **argv, int at, Components &d)
{
    if (argc < at + 3 || std::strcmp(argv[at], "--components") != 0) return false;
    if (!parse_double(argv[at + 1], d.cell) || !(d.cell > 0.0)) return false;
    char *end = nullptr;
    errno = 0;
    d.min_points = std::strtoll(argv[at + 2], &end, 10);
    if (end == argv[at + 2] || *end != '\0' || errno == ERANGE || d.min_points < 0) return false;
    for (int i = at + 3; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !d.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? d.lo[k] : d.hi[k - 3])) return false;
            d.has_box = true;
        } else if (a == "--conn" && i + 1 < argc && !d.has_conn) {
            const std::string v = argv[++i];
            if (v != "6" && v != "26") return false;
            d.conn = v == "6" ? 6 : 26;
            d.has_conn = true;
        } else if (a == "--small" && !d.small) {
            d.small = true;
        } else {
            return false;
        }
    }
    return true;
}

struct Poly {
    std::vector<double> xy;             // world coordinates, ring after ring
    std::vector<int32_t> ring_sizes;
    bool has_z = false, outside = false;
    double z[2] = {0.0, 0.0};
};

// the options behind --polygon, every one well formed and the file read, or false with the reason on stderr
static bool parse_polygon(int argc, char **argv, int at, Poly &p)
{
    if (argc < at + 2 || std::strcmp(argv[at], "--polygon") != 0) return false;
    for (int i = at + 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--z" && i + 2 < argc && !p.has_z) {
            for (int k = 0; k < 2; ++k) if (!parse_double(argv[++i], p.z[k])) return false;
            p.has_z = true;
        } else if (a == "--outside" && !p.outside) {
            p.outside = true;
        } else {
            return false;
        }
    }
    const char *path = argv[at + 1];
    std::ifstream f(path);
    if (!f) { std::fprintf(stderr, "pcr_decode: %s: cannot open the polygon file\n", path); return false; }
    std::string line;
    int32_t ring = 0;
    auto close_ring = [&]() {
        if (ring == 0) return true;
        if (ring < 3) { std::fprintf(stderr, "pcr_decode: %s: a ring of %d vertices (at least 3)\n", path, ring); return false; }
        p.ring_sizes.push_back(ring);
        ring = 0;
        return true;
    };
    for (int no = 1; std::getline(f, line); ++no) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) { if (!close_ring()) return false; continue; }
        std::istringstream in(line);
        std::string sx, sy, more;
        double x = 0.0, y = 0.0;
        if (!(in >> sx >> sy) || (in >> more) || !parse_double(sx.c_str(), x) || !parse_double(sy.c_str(), y)) {
            std::fprintf(stderr, "pcr_decode: %s: line %d is not `x y`\n", path, no);
            return false;
        }
        p.xy.push_back(x); p.xy.push_back(y);
        ++ring;
    }
    if (!close_ring()) return false;
    if (p.ring_sizes.empty()) { std::fprintf(stderr, "pcr_decode: %s: no ring\n", path); return false; }
    if (p.xy.size() / 2 > PCR_POLY_MAX_VERTICES) { std::fprintf(stderr, "pcr_decode: %s: more than %d vertices\n", path, PCR_POLY_MAX_VERTICES); return false; }
    return true;
}

struct SlabOpt {
    double point[3], normal[3], dist = 0.0;
    bool outside = false, has_box = false;
    double lo[3], hi[3];
};

// the options behind --slab, every one well formed, or false
static bool parse_slab(int argc, char **argv, int at, SlabOpt &o)
{
    if (argc < at + 8 || std::strcmp(argv[at], "--slab") != 0) return false;
    for (int k = 0; k < 7; ++k)
        if (!parse_double(argv[at + 1 + k], k < 3 ? o.point[k] : k < 6 ? o.normal[k - 3] : o.dist)) return false;
    if (!(o.dist >= 0.0) || (o.normal[0] == 0.0 && o.normal[1] == 0.0 && o.normal[2] == 0.0)) return false;
    for (int i = at + 8; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !o.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? o.lo[k] : o.hi[k - 3])) return false;
            o.has_box = true;
        } else if (a == "--outside" && !o.outside) {
            o.outside = true;
        } else {
            return false;
        }
    }
    return true;
}

struct Ortho {
    double cell = 0.0;
    bool has_box = false;
    double lo[3], hi[3];
    std::string dsm;
};

// the options behind --ortho, every one well formed, or false
static bool parse_ortho(int argc, char **argv, int at, Ortho &o)
{
    if (argc < at + 2 || std::strcmp(argv[at], "--ortho") != 0) return false;
    if (!parse_double(argv[at + 1], o.cell) || !(o.cell > 0.0)) return false;
    for (int i = at + 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !o.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? o.lo[k] : o.hi[k - 3])) return false;
            o.has_box = true;
        } else if (a == "--dsm" && i + 1 < argc && o.dsm.empty() && argv[i + 1][0] != '\0') {
            o.dsm = argv[++i];
        } else {
            return false;
        }
    }
    return true;
}

struct Percentile {
    uint32_t q = 0;                     // basis points
    double cell = 0.0;
    bool has_box = false;
    double lo[3], hi[3];
};

// the options behind --percentile, every one well formed, or false
static bool parse_percentile(int argc, char **argv, int at, Percentile &p)
{
    if (argc < at + 3 || std::strcmp(argv[at], "--percentile") != 0) return false;
    double pct = 0.0;
    if (!parse_double(argv[at + 1], pct) || pct < 0.0 || pct > 100.0) return false;
    const double bp = std::floor(pct * 100.0 + 0.5);
    if (std::fabs(pct * 100.0 - bp) > 1e-6) return false;               // (not a whole basis point)
    p.q = (uint32_t)bp;
    if (!parse_double(argv[at + 2], p.cell) || !(p.cell > 0.0)) return false;
    for (int i = at + 3; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--box" && i + 6 < argc && !p.has_box) {
            for (int k = 0; k < 6; ++k) if (!parse_double(argv[++i], k < 3 ? p.lo[k] : p.hi[k - 3])) return false;
            p.has_box = true;
        } else {
            return false;                                               // (--ortho, --dtm, --thin, ...: it combines with no other mode)
        }
    }
    return true;
}

struct Ground {
    double cell = 0.0, h_lo = 0.0, h_hi = 0.0;
    double slope = 1.0, max_window = 33.0, initial = 0.15, max_distance = 2.5;
    bool heights = false, normalize = false, has_box = false;
    bool seen[4] = {false, false, false, false};
    double lo[3], hi[3];
};

// the options behind --dtm / --height, every one well formed, or false
static bool parse_ground(int argc, char **argv, int at, Ground &g)
{
    if (argc < at + 2) return false;
    g.heights = std::strcmp(argv[at], "--height") == 0;
    if (!g.heights && std::strcmp(argv[at], "--dtm") != 0) return false;
    if (!parse_double(argv[at + 1], g.cell) || !(g.cell > 0.0)) return false;
    int i = at + 2;
    if (g.heights) {
        if (argc < at + 4 || !parse_double(argv[at + 2], g.h_lo) || !parse_double(argv[at + 3], g.h_hi)) return false;
        i = at + 4;
    }
    static const char *names[4] = {"--slope", "--max-window", "--initial", "--max-distance"};
    double *values[4] = {&g.slope, &g.max_window, &g.initial, &g.max_distance};
    for (; i < argc; ++i) {
        const std::string a = argv[i];
        int k = 0;
        while (k < 4 && a != names[k]) ++k;
        if (k < 4 && i + 1 < argc && !g.seen[k]) {
            if (!parse_double(argv[++i], *values[k]) || *values[k] < 0.0) return false;
            g.seen[k] = true;
        } else if (a == "--box" && i + 6 < argc && !g.has_box) {
            for (int j = 0; j < 6; ++j) if (!parse_double(argv[++i], j < 3 ? g.lo[j] : g.hi[j - 3])) return false;
            g.has_box = true;
        } else if (a == "--normalize" && g.heights && !g.normalize) {
            g.normalize = true;
        } else {
            return false;
        }
    }
    return true;
}

// The ground model of the loaded resource over the x and y range of the box: the grid, the parameters and the ground plane.
static pcr_ground_stats ground_model(HuffmanLasData &las, const pcr_las_info &info, const Ground &g, pcr_grid &grid, std::vector<int32_t> &ground)
{
    const double lo[2] = {g.has_box ? g.lo[0] : info.min[0], g.has_box ? g.lo[1] : info.min[1]};
    const double hi[2] = {g.has_box ? g.hi[0] : info.max[0], g.has_box ? g.hi[1] : info.max[1]};
    grid = gridFromWorld(info, lo, hi, g.cell);
    const pcr_ground_params gp = groundParamsFromWorld(info, g.cell, g.slope, g.initial, g.max_distance, g.max_window);
    pcr_box clip{};
    if (g.has_box && !g.heights) {                          // (--height: the box clips the selection, the model sees every point over its cells)
        const double inf = std::numeric_limits<double>::infinity();
        const double l3[3] = {-inf, -inf, g.lo[2]}, h3[3] = {inf, inf, g.hi[2]};
        clip = boxFromWorld(info, l3, h3);
    }
    const pcr_ground_stats st = las.groundModel(grid, g.has_box && !g.heights ? &clip : nullptr, gp, nullptr, &ground, nullptr);
    std::printf("ground: %d x %d cells of %d lattice steps, %d steps up to radius %d, cells empty %lld, ground %lld, non-ground %lld, filled %lld in %lld rounds, "
                "unfilled %lld\n", grid.width, grid.height, grid.cell, gp.num_steps, gp.radius[gp.num_steps - 1], (long long)st.cells_empty,
                (long long)st.cells_ground, (long long)st.cells_nonground, (long long)st.cells_filled, (long long)st.fill_rounds, (long long)st.cells_unfilled);
    if (!st.cells_ground) throw std::runtime_error("no ground cell inside the grid: nothing written");
    return st;
}

// The terrain model (ESRI ASCII grid) of the loaded resource, rows from north to south, as write_ortho writes the surface model.
static void write_dtm(HuffmanLasData &las, const pcr_las_info &info, const Ground &g, const std::string &asc)
{
    pcr_grid grid{};
    std::vector<int32_t> ground;
    ground_model(las, info, g, grid, ground);
    FILE *f = std::fopen(asc.c_str(), "w");
    if (!f) throw std::runtime_error(asc + ": cannot open for writing");
    const double px = (double)grid.origin_x * info.scale[0], py = (double)grid.origin_y * info.scale[1];
    std::fprintf(f, "ncols %d\nnrows %d\nxllcorner %.17g\nyllcorner %.17g\ncellsize %.17g\nNODATA_value -9999\n", grid.width, grid.height,
                 px + info.offset[0], py + info.offset[1], g.cell);
    size_t filled = 0;
    for (int cy = grid.height - 1; cy >= 0; --cy) {
        for (int cx = 0; cx < grid.width; ++cx) {
            const int32_t z = ground[(size_t)cy * grid.width + cx];
            const double pz = (double)z * info.scale[2];
            if (z != PCR_GROUND_EMPTY) { std::fprintf(f, cx ? " %.17g" : "%.17g", pz + info.offset[2]); ++filled; }
            else std::fputs(cx ? " -9999" : "-9999", f);
        }
        std::fputc('\n', f);
    }
    if (std::fclose(f) != 0) throw std::runtime_error(asc + ": write failed");
    std::printf("cells %zu of %zu with a height -> %s\n", filled, ground.size(), asc.c_str());
}

// The percentile raster (ESRI ASCII grid) of the loaded resource, rows from north to south, as write_ortho writes the surface model.
static void write_percentile(HuffmanLasData &las, const pcr_las_info &info, const Percentile &p, const std::string &asc)
{
    const double lo[2] = {p.has_box ? p.lo[0] : info.min[0], p.has_box ? p.lo[1] : info.min[1]};
    const double hi[2] = {p.has_box ? p.hi[0] : info.max[0], p.has_box ? p.hi[1] : info.max[1]};
    const pcr_grid grid = gridFromWorld(info, lo, hi, p.cell);
    pcr_box clip{};
    if (p.has_box) {
        const double inf = std::numeric_limits<double>::infinity();
        const double l3[3] = {-inf, -inf, p.lo[2]}, h3[3] = {inf, inf, p.hi[2]};
        clip = boxFromWorld(info, l3, h3);
    }
    std::vector<int32_t> plane;
    std::vector<uint32_t> count;
    const pcr_quantile_stats st = las.heightQuantiles(grid, p.has_box ? &clip : nullptr, nullptr, std::vector<uint32_t>{p.q}, plane, &count);
    std::printf("percentile: %u basis points, %d x %d cells of %d lattice steps, batches outside %lld, windowed %lld, direct %lld, cells occupied %lld, "
                "candidates %lld, largest cell %lld\n", p.q, grid.width, grid.height, grid.cell, (long long)st.batches_outside, (long long)st.batches_windowed,
                (long long)st.batches_direct, (long long)st.cells_occupied, (long long)st.candidates, (long long)st.max_cell_points);
    if (!st.candidates) throw std::runtime_error("no points inside the grid: nothing written");
    FILE *f = std::fopen(asc.c_str(), "w");
    if (!f) throw std::runtime_error(asc + ": cannot open for writing");
    const double px = (double)grid.origin_x * info.scale[0], py = (double)grid.origin_y * info.scale[1];
    std::fprintf(f, "ncols %d\nnrows %d\nxllcorner %.17g\nyllcorner %.17g\ncellsize %.17g\nNODATA_value -9999\n", grid.width, grid.height,
                 px + info.offset[0], py + info.offset[1], p.cell);
    for (int cy = grid.height - 1; cy >= 0; --cy) {
        for (int cx = 0; cx < grid.width; ++cx) {
            const size_t g = (size_t)cy * grid.width + cx;
            const double pz = (double)plane[g] * info.scale[2];
            if (count[g]) std::fprintf(f, cx ? " %.17g" : "%.17g", pz + info.offset[2]);
            else std::fputs(cx ? " -9999" : "-9999", f);
        }
        std::fputc('\n', f);
    }
    if (std::fclose(f) != 0) throw std::runtime_error(asc + ": write failed");
    std::printf("cells %lld of %zu filled -> %s\n", (long long)st.cells_occupied, plane.size(), asc.c_str());
}

// The orthophoto (binary PPM) and, with a path, the surface model (ESRI ASCII grid) of the loaded resource, rows from north to south.
static void write_ortho(HuffmanLasData &las, const pcr_las_info &info, const Ortho &o, const std::string &ppm)
{
    const double lo[2] = {o.has_box ? o.lo[0] : info.min[0], o.has_box ? o.lo[1] : info.min[1]};
    const double hi[2] = {o.has_box ? o.hi[0] : info.max[0], o.has_box ? o.hi[1] : info.max[1]};
    const pcr_grid grid = gridFromWorld(info, lo, hi, o.cell);
    pcr_box clip{};
    if (o.has_box) {
        const double inf = std::numeric_limits<double>::infinity();
        const double l3[3] = {-inf, -inf, o.lo[2]}, h3[3] = {inf, inf, o.hi[2]};
        clip = boxFromWorld(info, l3, h3);
    }
    std::vector<uint64_t> top;
    const pcr_grid_stats st = las.readGrid(grid, o.has_box ? &clip : nullptr, &top, nullptr, nullptr);
    std::printf("ortho: %d x %d cells of %d lattice steps, batches outside %lld, windowed %lld, direct %lld\n", grid.width, grid.height, grid.cell,
                (long long)st.batches_outside, (long long)st.batches_windowed, (long long)st.batches_direct);
    size_t filled = 0;
    for (uint64_t w : top) filled += w != 0;
    if (!filled) throw std::runtime_error("no points inside the grid: nothing written");
    std::vector<unsigned char> rgb((size_t)grid.width * 3);
    FILE *f = std::fopen(ppm.c_str(), "wb");
    if (!f) throw std::runtime_error(ppm + ": cannot open for writing");
    std::fprintf(f, "P6\n%d %d\n255\n", grid.width, grid.height);
    for (int cy = grid.height - 1; cy >= 0; --cy) {
        for (int cx = 0; cx < grid.width; ++cx) {
            const uint64_t w = top[(size_t)cy * grid.width + cx];
            for (int k = 0; k < 3; ++k) rgb[(size_t)cx * 3 + k] = (unsigned char)(w >> (8 * k));
        }
        std::fwrite(rgb.data(), 1, rgb.size(), f);
    }
    if (std::fclose(f) != 0) throw std::runtime_error(ppm + ": write failed");
    if (!o.dsm.empty()) {
        f = std::fopen(o.dsm.c_str(), "w");
        if (!f) throw std::runtime_error(o.dsm + ": cannot open for writing");
        const double px = (double)grid.origin_x * info.scale[0], py = (double)grid.origin_y * info.scale[1];
        std::fprintf(f, "ncols %d\nnrows %d\nxllcorner %.17g\nyllcorner %.17g\ncellsize %.17g\nNODATA_value -9999\n", grid.width, grid.height,
                     px + info.offset[0], py + info.offset[1], o.cell);
        for (int cy = grid.height - 1; cy >= 0; --cy) {
            for (int cx = 0; cx < grid.width; ++cx) {
                const uint64_t w = top[(size_t)cy * grid.width + cx];
                const double pz = (double)(int32_t)((uint32_t)(w >> 32) ^ 0x80000000u) * info.scale[2];
                if (w) std::fprintf(f, cx ? " %.17g" : "%.17g", pz + info.offset[2]);
                else std::fputs(cx ? " -9999" : "-9999", f);
            }
            std::fputc('\n', f);
        }
        if (std::fclose(f) != 0) throw std::runtime_error(o.dsm + ": write failed");
    }
    std::printf("cells %zu of %zu filled -> %s%s%s\n", filled, top.size(), ppm.c_str(), o.dsm.empty() ? "" : ", ", o.dsm.c_str());
}

int main(int argc, char **argv)
{
    if (argc >= 2 && (std::strcmp(argv[1], "--help") == 0 || std::strcmp(argv[1], "-h") == 0)) { std::fputs(USAGE, stdout); return 0; }
    double lo[3], hi[3];
    View view;
    Ortho ortho;
    const bool viewed = argc > 3 && std::strcmp(argv[3], "--view") == 0, orthoed = argc > 3 && std::strcmp(argv[3], "--ortho") == 0;
    Thin thin;
    const bool thinned = argc > 3 && std::strcmp(argv[3], "--thin") == 0;
    Lod lod;
    const bool lodded = argc > 3 && std::strcmp(argv[3], "--lod") == 0;
    Poly poly;
    const bool polygoned = argc > 3 && std::strcmp(argv[3], "--polygon") == 0;
    SlabOpt slab;
    const bool slabbed = argc > 3 && std::strcmp(argv[3], "--slab") == 0;
    Denoise noise;
    const bool denoised = argc > 3 && std::strcmp(argv[3], "--denoise") == 0;
    Components comps;
    const bool componented = argc > 3 && std::strcmp(argv[3], "--components") == 0;
    Ground ground;
    const bool grounded = argc > 3 && (std::strcmp(argv[3], "--dtm") == 0 || std::strcmp(argv[3], "--height") == 0);
    Radius rad;
    const bool radiused = argc > 3 && std::strcmp(argv[3], "--radius") == 0;
    Normals nrm;
    const bool normaled = argc > 3 && std::strcmp(argv[3], "--normals") == 0;
    Sor sor;
    const bool sored = argc > 3 && std::strcmp(argv[3], "--sor") == 0;
    Percentile pctl;
    const bool percentiled = argc > 3 && std::strcmp(argv[3], "--percentile") == 0;
    const bool boxed = argc > 3 && !percentiled && !viewed && !orthoed && !thinned && !lodded && !polygoned && !slabbed && !denoised && !componented && !grounded && !radiused && !normaled && !sored;
    if (argc < 3 || (polygoned && !parse_polygon(argc, argv, 3, poly)) || (slabbed && !parse_slab(argc, argv, 3, slab)) || (boxed && !parse_box(argc, argv, 3, lo, hi)) || (viewed && !parse_view(argc, argv, 3, view)) ||
        (orthoed && !parse_ortho(argc, argv, 3, ortho)) || (thinned && !parse_thin(argc, argv, 3, thin)) || (lodded && !parse_lod(argc, argv, 3, lod)) || (denoised && !parse_denoise(argc, argv, 3, noise)) ||
        (componented && !parse_components(argc, argv, 3, comps)) || (grounded && !parse_ground(argc, argv, 3, ground)) ||
        (radiused && !parse_radius(argc, argv, 3, rad)) || (normaled && !parse_normals(argc, argv, 3, nrm)) ||
        (sored && !parse_sor(argc, argv, 3, sor)) || (percentiled && !parse_percentile(argc, argv, 3, pctl))) { std::fputs(USAGE, stderr); return 2; }
    const std::string in = argv[1], out = argv[2];
    try {
        Renderer renderer(viewed ? view.w : 64, viewed ? view.h : 64, 0);
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
        if (orthoed) {
            write_ortho(*las, info, ortho, out);
            las->unload(&renderer);
            return 0;
        }
        if (percentiled) {
            write_percentile(*las, info, pctl, out);
            las->unload(&renderer);
            return 0;
        }
        if (grounded && !ground.heights) {
            write_dtm(*las, info, ground, out);
            las->unload(&renderer);
            return 0;
        }
        if (normaled) {
            const int32_t r = radiusFromWorld(info, nrm.radius);
            const pcr_box clip = boxFromWorld(info, nrm.has_box ? nrm.lo : info.min, nrm.has_box ? nrm.hi : info.max);
            std::vector<pcr_eigen> eigen;
            const pcr_neighbors_stats st = las->normals(r, &clip, nrm.min_count, points, eigen);
            std::printf("normals: %d lattice steps, written %lld, considered %lld, below min count %lld, voxels %lld, pairs bound %lld\n", r,
                        (long long)st.points_written, (long long)st.points_considered, (long long)st.points_sparse, (long long)st.voxels,
                        (long long)st.pairs_bound);
            las->unload(&renderer);
            if (points.empty()) throw std::runtime_error("no points to write: nothing written");
            write_normals_ply(out, info, points, eigen);
            std::printf("points %lld (batches %lld) -> %s\n", (long long)points.size(), (long long)las->numBatches, out.c_str());
            return 0;
        }
        if (grounded) {
            pcr_grid grid{};
            std::vector<int32_t> plane;
            ground_model(*las, info, ground, grid, plane);
            const pcr_box clip = boxFromWorld(info, ground.has_box ? ground.lo : info.min, ground.has_box ? ground.hi : info.max);
            // heights are multiples of the z scale: the offset cancels
            const double a = std::ceil(ground.h_lo / info.scale[2] - 1e-9), b = std::floor(ground.h_hi / info.scale[2] + 1e-9);
            const int32_t h_min = (int32_t)std::max((double)INT32_MIN, std::min((double)INT32_MAX, a));
            const int32_t h_max = (int32_t)std::max((double)INT32_MIN, std::min((double)INT32_MAX, b));
            const pcr_height_stats st = las->pointsByHeight(grid, plane, &clip, h_min, h_max, ground.normalize ? PCR_HEIGHT_REPLACE_Z : 0u, points);
            std::printf("height: %d .. %d z steps, batches outside %lld, decoded %lld, points without ground %lld, selected %lld\n", h_min, h_max,
                        (long long)st.batches_outside, (long long)st.batches_decoded, (long long)st.points_no_ground, (long long)st.points_selected);
            if (points.empty()) throw std::runtime_error("no points in the height range: nothing written");
        } else if (boxed) {
            const pcr_select_stats st = las->selectBox(boxFromWorld(info, lo, hi), points);
            std::printf("box: batches outside %lld, inside %lld, straddling %lld\n", (long long)st.batches_outside, (long long)st.batches_inside,
                        (long long)st.batches_straddling);
            if (points.empty()) throw std::runtime_error("no points inside the box: nothing written");
        } else if (polygoned) {
            PolygonOwner owner;
            polygonFromWorld(info, poly.xy, poly.ring_sizes, poly.has_z ? &poly.z[0] : nullptr, poly.has_z ? &poly.z[1] : nullptr, poly.outside, owner);
            const pcr_polygon_stats st = las->pointsInPolygon(owner.poly, points);
            std::printf("polygon: batches outside %lld, inside %lld, straddling %lld, edges listed %lld, largest list %lld\n", (long long)st.batches_outside,
                        (long long)st.batches_inside, (long long)st.batches_straddling, (long long)st.edges_listed, (long long)st.edges_max);
            if (points.empty()) throw std::runtime_error("no points inside the polygon: nothing written");
        } else if (slabbed) {
            const std::vector<pcr_slab> slabs{slabFromWorld(info, slab.point, slab.normal, slab.dist)};
            const pcr_box clip = boxFromWorld(info, slab.has_box ? slab.lo : info.min, slab.has_box ? slab.hi : info.max);
            const pcr_slab_stats st = las->selectSlabs(slabs, &clip, slab.outside ? PCR_SLAB_INVERT : 0u, points);
            std::printf("slab: normal %d %d %d, %lld .. %lld, written %lld, batches outside %lld, inside %lld, straddling %lld\n", slabs[0].n[0], slabs[0].n[1],
                        slabs[0].n[2], (long long)slabs[0].lo, (long long)slabs[0].hi, (long long)st.points_selected, (long long)st.batches_outside,
                        (long long)st.batches_inside, (long long)st.batches_straddling);
            if (points.empty()) throw std::runtime_error("no points to write: nothing written");
        } else if (thinned) {
            const pcr_voxels vox = voxelsFromWorld(info, thin.cell, info.min);
            const pcr_box clip = boxFromWorld(info, thin.has_box ? thin.lo : info.min, thin.has_box ? thin.hi : info.max);
            std::vector<int64_t> counts;
            const pcr_thin_stats st = thin.mean ? las->voxelMean(vox, &clip, points, counts)
                                                : las->thin(vox, &clip, thin.center ? PCR_THIN_CENTER : PCR_THIN_FIRST, points);
            std::printf("thin: cell of %d lattice steps, batches outside %lld, decoded %lld, points considered %lld, runs %lld, kept %lld, table slots %lld\n",
                        vox.cell, (long long)st.batches_outside, (long long)st.batches_decoded, (long long)st.points_considered, (long long)st.runs,
                        (long long)st.points_kept, (long long)st.table_slots);
            if (points.empty()) throw std::runtime_error("no points inside the box: nothing written");
        } else if (lodded) {
            const pcr_lod nested = lodFromWorld(info, lod.cell, lod.levels, info.min);
            const pcr_box clip = boxFromWorld(info, lod.has_box ? lod.lo : info.min, lod.has_box ? lod.hi : info.max);
            const pcr_lod_stats st = las->lodOrdered(nested, &clip, lod.drop_rest ? PCR_LOD_DROP_REST : 0u, points);
            std::printf("lod: finest cell of %d lattice steps, %d levels, batches outside %lld, decoded %lld, written %lld / considered %lld / runs %lld / "
                        "table slots %lld\n", nested.cell, nested.levels, (long long)st.batches_outside, (long long)st.batches_decoded,
                        (long long)st.points_written, (long long)st.points_considered, (long long)st.runs, (long long)st.table_slots);
            for (int l = 0; l < nested.levels; ++l) std::printf("level %d: %lld\n", l, (long long)st.level_count[l]);
            std::printf("rest: %lld%s\n", (long long)st.level_count[nested.levels], lod.drop_rest ? " (dropped)" : "");
            if (points.empty()) throw std::runtime_error("no points inside the box: nothing written");
        } else if (denoised) {
            const pcr_voxels vox = voxelsFromWorld(info, noise.cell, info.min);
            const pcr_box clip = boxFromWorld(info, noise.has_box ? noise.lo : info.min, noise.has_box ? noise.hi : info.max);
            const pcr_denoise_stats st = las->denoised(vox, &clip, noise.max_count, noise.isolated ? PCR_DENOISE_ISOLATED : PCR_DENOISE_KEEP, points);
            std::printf("denoise: cell of %d lattice steps, batches outside %lld, decoded %lld, points considered %lld, runs %lld, voxels %lld, "
                        "isolated voxels %lld, isolated points %lld, written %lld, table slots %lld\n",
                        vox.cell, (long long)st.batches_outside, (long long)st.batches_decoded, (long long)st.points_considered, (long long)st.runs,
                        (long long)st.voxels, (long long)st.voxels_isolated, (long long)st.points_isolated, (long long)st.points_written,
                        (long long)st.table_slots);
            if (points.empty()) throw std::runtime_error("no points to write: nothing written");
        } else if (radiused) {
            const int32_t r = radiusFromWorld(info, rad.radius);
            const pcr_box clip = boxFromWorld(info, rad.has_box ? rad.lo : info.min, rad.has_box ? rad.hi : info.max);
            const pcr_neighbors_stats st = las->radiusFiltered(r, &clip, rad.min_count, rad.sparse ? PCR_NEIGHBORS_SPARSE : PCR_NEIGHBORS_KEEP, points);
            std::printf("radius: %d lattice steps, written %lld, considered %lld, sparse %lld, voxels %lld, table slots %lld, pairs bound %lld\n", r,
                        (long long)st.points_written, (long long)st.points_considered, (long long)st.points_sparse, (long long)st.voxels,
                        (long long)st.table_slots, (long long)st.pairs_bound);
            if (points.empty()) throw std::runtime_error("no points to write: nothing written");
        } else if (sored) {
            const int32_t r = radiusFromWorld(info, sor.radius);
            const pcr_box clip = boxFromWorld(info, sor.has_box ? sor.lo : info.min, sor.has_box ? sor.hi : info.max);
            int64_t bad = 0;
            const pcr_neighbors_stats st = las->statisticalOutliers(sor.k, sor.multiplier, r, &clip, info.scale[0], sor.outliers, points, &bad);
            std::printf("sor: k %d, %d lattice steps, written %lld, considered %lld, outliers %lld, voxels %lld, pairs bound %lld\n", sor.k, r,
                        (long long)points.size(), (long long)st.points_considered, (long long)bad, (long long)st.voxels, (long long)st.pairs_bound);
            if (points.empty()) throw std::runtime_error("no points to write: nothing written");
        } else if (componented) {
            const pcr_voxels vox = voxelsFromWorld(info, comps.cell, info.min);
            const pcr_box clip = boxFromWorld(info, comps.has_box ? comps.lo : info.min, comps.has_box ? comps.hi : info.max);
            const pcr_components_stats st = las->components(vox, &clip, comps.conn, comps.min_points, comps.small ? PCR_COMPONENTS_SMALL : PCR_COMPONENTS_KEEP, points);
            std::printf("components: cell of %d lattice steps, connectivity %d, batches outside %lld, decoded %lld, points considered %lld, runs %lld, "
                        "voxels %lld, components %lld, small components %lld, small points %lld, largest %lld, written %lld, table slots %lld\n",
                        vox.cell, comps.conn, (long long)st.batches_outside, (long long)st.batches_decoded, (long long)st.points_considered, (long long)st.runs,
                        (long long)st.voxels, (long long)st.components, (long long)st.components_small, (long long)st.points_small,
                        (long long)st.largest_points, (long long)st.points_written, (long long)st.table_slots);
            if (points.empty()) throw std::runtime_error("no points to write: nothing written");
        } else if (viewed) {
            renderer.yaw = view.cam[0]; renderer.pitch = view.cam[1]; renderer.radius = view.cam[2];
            for (int k = 0; k < 3; ++k) renderer.target[k] = view.cam[3 + k];
            Debug::LOD = (float)view.lod;
            Debug::frustumCullingEnabled = view.cull != 0;
            if (view.visible >= 0) {
                const pcr_visible_stats st = las->selectVisible(renderer.params(), view.has_rect ? &view.rect : nullptr, view.visible, std::max(view.occluder, 0),
                                                                &points, nullptr);
                std::printf("view: batches skipped %lld, decoded %lld, hits %lld on %lld pixels, in the rect %lld, visible %lld\n", (long long)st.batches_skipped,
                            (long long)st.batches_decoded, (long long)st.hits, (long long)st.pixels_covered, (long long)st.candidates, (long long)st.selected);
            } else {
                const pcr_screen_stats st = las->selectScreen(renderer.params(), view.has_rect ? &view.rect : nullptr, &points, nullptr);
                std::printf("view: batches skipped %lld, decoded %lld, points tested %lld\n", (long long)st.batches_skipped, (long long)st.batches_decoded,
                            (long long)st.points_tested);
            }
            if (points.empty()) throw std::runtime_error("no points in the view: nothing written");
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
