// Integer lattice arithmetic shared by the top-down grid, the voxel thinning, the voxel denoising and the levels of detail: the
// exact division of a 32-bit difference by a cell, the lattices pcr_thin, pcr_denoise and pcr_lod_order hand to their kernels, and
// the level-byte arithmetic of pcr_lod_order. Plain C++ without a HIP dependency, so a host-only build can call it.
#pragma once
#include <cstdint>

// d / cell for every 32-bit d: a shift for a power of two, else the high half of d * ceil(2^64 / cell) (see grid_div).
struct CellDiv {
    uint32_t shift;                 // cell == 1 << shift; CELL_NO_SHIFT: not a power of two, then
    unsigned long long magic;       // ceil(2^64 / cell)
};
constexpr uint32_t CELL_NO_SHIFT = 32;

inline CellDiv make_cell_div(uint32_t cell)                 // cell >= 1
{
    CellDiv d{};
    if ((cell & (cell - 1)) == 0) { d.shift = (uint32_t)__builtin_ctz(cell); d.magic = 0; }
    else { d.shift = CELL_NO_SHIFT; d.magic = ~0ull / cell + 1; }           // ceil(2^64 / cell): cell does not divide 2^64
    return d;
}

inline int64_t floor_div64(int64_t a, int64_t b)            // b > 0
{
    const int64_t q = a / b;
    return q * b > a ? q - 1 : q;
}

// The lattice of a thinning call, shifted by whole cells so that q.min lies in voxel 0 on every axis: origin' = origin +
// floor((q.min - origin) / cell) * cell in 64 bits. For a point p inside q, d = p - origin' is in [0, q.max - q.min + cell), so
// it fits 32 unsigned bits (the kernels take it modulo 2^32 from the low half of origin'), and v' = d / cell <= (q.max - q.min)
// / cell + 1. Shifting by whole cells changes neither which points share a voxel nor a point's offset inside its voxel.
struct ThinLattice {
    uint32_t origin[3];             // the low 32 bits of origin'
    uint32_t cell;
    CellDiv div;
};
constexpr int THIN_KEY_BITS = 21;                           // per axis: the key is v'x | v'y << 21 | v'z << 42, 63 bits
enum { THIN_LATTICE_OK = 0, THIN_LATTICE_EXTENT = 1, THIN_LATTICE_VOXELS = 2 };

// THIN_LATTICE_EXTENT: q spans 2^31 or more on *axis; THIN_LATTICE_VOXELS: more than 2^21 voxels there. q is not empty.
inline int thin_lattice(const int32_t origin[3], int32_t cell, const int32_t qmin[3], const int32_t qmax[3], ThinLattice *out, int *axis)
{
    for (int k = 0; k < 3; ++k) {
        const int64_t extent = (int64_t)qmax[k] - (int64_t)qmin[k];
        *axis = k;
        if (extent >= (int64_t)1 << 31) return THIN_LATTICE_EXTENT;
        if (extent / cell + 2 > (int64_t)1 << THIN_KEY_BITS) return THIN_LATTICE_VOXELS;
        const int64_t shifted = (int64_t)origin[k] + floor_div64((int64_t)qmin[k] - (int64_t)origin[k], cell) * (int64_t)cell;
        out->origin[k] = (uint32_t)(uint64_t)shifted;
    }
    out->cell = (uint32_t)cell;
    out->div = make_cell_div((uint32_t)cell);
    return THIN_LATTICE_OK;
}

// The lattice of a level-of-detail call (pcr_lod_order): `levels` nested lattices over one origin, level l (0 = coarsest) with
// the cell cell << (levels - 1 - l). The shift of the origin is by whole COARSEST cells C = cell << (levels - 1): origin' = origin +
// floor((q.min - origin) / C) * C in 64 bits. A shift by whole cells of a level changes neither which points share a voxel of
// that level nor the nesting floor(floor(d / c) / 2) == floor(d / 2c), which holds for d >= 0 counted from one origin; C is a
// whole number of cells of every level, a finer cell would not be one of the coarser levels. For a point p inside q, d = p -
// origin' is in [0, q.max - q.min + C): q.min - origin' is in [0, C - 1]. With an extent below 2^31 and C <= 2^30 that is less
// than 2^32, so d fits 32 unsigned bits. The finest index is d / cell <= (q.max - q.min + C - 1) / cell <= (q.max - q.min) / cell
// + 2^(levels - 1), because C / cell = 2^(levels - 1) is whole; the call is refused when (q.max - q.min) / cell + 2^(levels - 1) + 1
// > 2^21, so every finest index fits its 21-bit field of the key. The level-l index is the finest one shifted right by levels - 1
// - l (lod_parent_key, one level at a time). levels == 1 is thin_lattice. Same result codes as thin_lattice. cell >= 1, 1 <=
// levels, cell << (levels - 1) <= 2^30.
inline int lod_lattice(const int32_t origin[3], int32_t cell, int32_t levels, const int32_t qmin[3], const int32_t qmax[3], ThinLattice *out, int *axis)
{
    const int64_t coarsest = (int64_t)cell << (levels - 1);
    for (int k = 0; k < 3; ++k) {
        const int64_t extent = (int64_t)qmax[k] - (int64_t)qmin[k];
        *axis = k;
        if (extent >= (int64_t)1 << 31) return THIN_LATTICE_EXTENT;
        if (extent / cell + ((int64_t)1 << (levels - 1)) + 1 > (int64_t)1 << THIN_KEY_BITS) return THIN_LATTICE_VOXELS;
        const int64_t shifted = (int64_t)origin[k] + floor_div64((int64_t)qmin[k] - (int64_t)origin[k], coarsest) * coarsest;
        out->origin[k] = (uint32_t)(uint64_t)shifted;
    }
    out->cell = (uint32_t)cell;
    out->div = make_cell_div((uint32_t)cell);
    return THIN_LATTICE_OK;
}

// The key of the voxel one level up: every 21-bit field of the key shifted right by one (the bit that leaves a field is dropped)
constexpr unsigned long long lod_parent_key(unsigned long long key)
{
    return (key >> 1) & ~((1ull << (THIN_KEY_BITS - 1)) | (1ull << (2 * THIN_KEY_BITS - 1)) | (1ull << (3 * THIN_KEY_BITS - 1)));
}

// Eight level bytes in a 64-bit word, byte j that of point j (little endian). A byte is a level 0 .. levels, or LOD_NO_LEVEL.
// Flags are 0x80 in the byte they speak of. constexpr, so that the kernels can call them as well.
constexpr uint32_t LOD_NO_LEVEL = 0xFFu;
constexpr unsigned long long LOD_BYTE_LOW7 = 0x7F7F7F7F7F7F7F7Full, LOD_BYTE_FLAGS = 0x8080808080808080ull, LOD_BYTE_ONES = 0x0101010101010101ull;
constexpr unsigned long long lod_bytes_nonzero(unsigned long long w)            // (a sum of two 7-bit values never leaves its byte)
{
    return (((w & LOD_BYTE_LOW7) + LOD_BYTE_LOW7) | w) & LOD_BYTE_FLAGS;
}
constexpr unsigned long long lod_bytes_equal(unsigned long long w, uint32_t v)  // v < 256
{
    return ~lod_bytes_nonzero(w ^ (LOD_BYTE_ONES * v)) & LOD_BYTE_FLAGS;
}
constexpr unsigned long long lod_flags_of_bits(uint32_t bits)                   // bit j of bits -> the flag of byte j
{
    return lod_bytes_nonzero((LOD_BYTE_ONES * (bits & 0xFFu)) & 0x8040201008040201ull);
}
constexpr uint32_t lod_bits_of_flags(unsigned long long flags)                  // the flag of byte j -> bit j (the partial products meet in no bit)
{
    return (uint32_t)(((flags >> 7) * 0x0102040810204080ull) >> 56);
}
// The final bytes: a candidate (bit j of cand) that won at no level (LOD_NO_LEVEL) gets `levels`, the rest; others stay.
constexpr unsigned long long lod_bytes_final(unsigned long long w, uint32_t cand, uint32_t levels)
{
    const unsigned long long full = ((lod_bytes_equal(w, LOD_NO_LEVEL) & lod_flags_of_bits(cand)) >> 7) * 0xFFull;
    return (w & ~full) | (full & (LOD_BYTE_ONES * levels));
}
// The flags of the final bytes a call writes: every level below `classes` (levels + 1, or levels where the rest is dropped)
constexpr unsigned long long lod_bytes_written(unsigned long long w, uint32_t levels, uint32_t classes)
{
    return ~lod_bytes_equal(w, LOD_NO_LEVEL) & (classes > levels ? LOD_BYTE_FLAGS : ~lod_bytes_equal(w, levels)) & LOD_BYTE_FLAGS;
}

// The mean of n >= 1 non-negative integers with sum s, rounded half up: (2 s + n) / (2 n) in unsigned 64-bit integers. Exact for
// n <= 2^32 (PCR_VOXEL_MEAN_MAX_ROWS) and s < 2^62: 2 s + n < 2^63 + 2^32 does not wrap. The result lies between the least and the
// greatest of the integers (a mean does, and both are integers, so rounding cannot leave the interval). constexpr, so that the
// kernels can call it as well.
constexpr unsigned long long voxel_mean_round(unsigned long long s, unsigned long long n)
{
    return (2ull * s + n) / (2ull * n);
}

// The rank pcr_grid_quantiles takes from a cell of n >= 1 candidates sorted ascending for q basis points (q <= 10000 =
// PCR_QUANTILE_ONE): the nearest rank q * (n - 1) / 10000, a half rounded up, in unsigned 64-bit integers. n < 2^32, so the
// product stays below 2^46. q = 0 gives 0, q = 10000 gives n - 1, and the rank never leaves [0, n - 1]. constexpr, so that the
// kernels can call it as well.
constexpr unsigned long long QUANTILE_ONE = 10000ull;
constexpr unsigned long long quantile_rank(unsigned long long q, unsigned long long n)
{
    return (q * (n - 1ull) + QUANTILE_ONE / 2ull) / QUANTILE_ONE;
}

// The lattice of a denoising call: thin_lattice shifted by one whole cell more, origin'' = origin + (floor((q.min - origin) /
// cell) - 1) * cell, so that q.min lies in voxel 1 on every axis. For a point p inside q, d = p - origin'' is in [cell, q.max -
// q.min + 2 * cell) -- at most 2^32 - 1 for an extent below 2^31 and a cell of at most 2^30, so it still fits 32 unsigned bits --
// and v'' = d / cell is in [1, (q.max - q.min) / cell + 2]: every index of the 27 voxels v'' + {-1, 0, 1}^3 lies in [0, (q.max -
// q.min) / cell + 3]. The call is refused when (q.max - q.min) / cell + 4 > 2^21, so no neighbour index leaves its 21-bit field
// of the key and the kernels need no range test. Same result codes as thin_lattice.
inline int noise_lattice(const int32_t origin[3], int32_t cell, const int32_t qmin[3], const int32_t qmax[3], ThinLattice *out, int *axis)
{
    for (int k = 0; k < 3; ++k) {
        const int64_t extent = (int64_t)qmax[k] - (int64_t)qmin[k];
        *axis = k;
        if (extent >= (int64_t)1 << 31) return THIN_LATTICE_EXTENT;
        if (extent / cell + 4 > (int64_t)1 << THIN_KEY_BITS) return THIN_LATTICE_VOXELS;
        const int64_t shifted = (int64_t)origin[k] + (floor_div64((int64_t)qmin[k] - (int64_t)origin[k], cell) - 1) * (int64_t)cell;
        out->origin[k] = (uint32_t)(uint64_t)shifted;
    }
    out->cell = (uint32_t)cell;
    out->div = make_cell_div((uint32_t)cell);
    return THIN_LATTICE_OK;
}
