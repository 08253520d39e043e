// Integer lattice arithmetic shared by the top-down grid, the voxel thinning and the voxel denoising: the exact division of a
// 32-bit difference by a cell, and the lattices pcr_thin and pcr_denoise hand to their kernels. Plain C++ without a HIP dependency, so a host-only build can call it.
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
