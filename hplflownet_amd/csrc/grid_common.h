// grid_common.h -- what the ops that sort a cloud onto a uniform grid share (motion_segment, voxel_grid, icp + icp_plane,
// normals, outlier_filter): the 64-bit cell key and its limits, the float64 cell of a point, the sorted record,
// the pick of a run's bounds, the one-atomic-per-workgroup counter, and the room kept for rocPRIM's temporaries (selfsup_loss takes that alone).  Header only.  Every rule here is a promise about bits: it is stated once.
#pragma once
#include "cloud_common.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace hpl {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------- the key
// (group, cell x, y, z), the group in the bits above three biased 19-bit fields: the order of the keys is the lexicographic
// order of the four, and a key of all ones is no cell's (a biased field is at most 2^19 - 2).
constexpr int GRID_CELL_BITS = 19;
constexpr int GRID_CELL_BIAS = 1 << (GRID_CELL_BITS - 1);
constexpr int GRID_CELL_MASK = (1 << GRID_CELL_BITS) - 1;
constexpr double GRID_CELL_MAX = (double)(GRID_CELL_BIAS - 2);       // |cell| <= 2^18 - 2: the neighbours' fields stay in 19 bits
constexpr double GRID_CELL_MARGIN = 1.001;                           // cell edge / search radius
constexpr int GRID_KEY_BITS = 3 * GRID_CELL_BITS;                    // below the group digit

__host__ __device__ __forceinline__ u64 grid_key(int b, int cx, int cy, int cz) {
    return ((u64)b << (3 * GRID_CELL_BITS)) | ((u64)cx << (2 * GRID_CELL_BITS)) | ((u64)cy << GRID_CELL_BITS) | (u64)cz;
}

// the group and the biased cell of a key that has a cell (two calls: a kernel unpacks in the order it did before)
__host__ __device__ __forceinline__ int grid_group(u64 key) { return (int)(key >> (3 * GRID_CELL_BITS)); }

__host__ __device__ __forceinline__ void grid_cell(u64 key, int *c) {
    c[0] = (int)((key >> (2 * GRID_CELL_BITS)) & (u64)GRID_CELL_MASK);
    c[1] = (int)((key >> GRID_CELL_BITS) & (u64)GRID_CELL_MASK);
    c[2] = (int)(key & (u64)GRID_CELL_MASK);
}

// ---------------------------------------------------------------------------------------------- the cell
// the cell of (x, y, z), biased; false when the point is non-finite or its cell is outside the field range
__host__ __device__ __forceinline__ bool grid_cell_of(double inv_cell, float x, float y, float z, int *c) {
    const double cx = floor((double)x * inv_cell), cy = floor((double)y * inv_cell), cz = floor((double)z * inv_cell);
    if (!(fabs(cx) <= GRID_CELL_MAX && fabs(cy) <= GRID_CELL_MAX && fabs(cz) <= GRID_CELL_MAX)) return false;   // (NaN fails)
    c[0] = (int)cx + GRID_CELL_BIAS;
    c[1] = (int)cy + GRID_CELL_BIAS;
    c[2] = (int)cz + GRID_CELL_BIAS;
    return true;
}

// ---------------------------------------------------------------------------------------------- the record
struct __attribute__((aligned(16))) GridRec {
    float x, y, z;
    int32_t i;                  // the packed index
};

// Point j = (x, y, z) of the cloud that `prefix` gives it: its key -- all ones unless the point has a cell -- and its record.
// Args carries inv_cell, batch, key and rec; they are read where they are used (read ahead of the call, the two pointers cost
// the keys kernels 4 SGPRs more).
template <class Args>
__device__ __forceinline__ void grid_store(const Args &a, const int32_t *prefix, int j, float x, float y, float z) {
    int c[3];
    u64 key = ~0ull;
    if (grid_cell_of(a.inv_cell, x, y, z, c)) key = grid_key(group_of(prefix, a.batch, j), c[0], c[1], c[2]);
    a.key[j] = key;
    GridRec r;
    r.x = x; r.y = y; r.z = z; r.i = j;
    a.rec[j] = r;
}

// (The search for the 9 runs of the 27 cells around a cell is not here: as one function it changed the code of k_normals and
// of the ICP kernels and k_normals<32> was slower; match_point and k_normals keep its text, written with grid_key.  DESIGN.md §31.)

// The element `which` of the 9 runs' bounds v[0 .. 8], written with compile-time indices only (k_normals, k_outlier_search).
// The compiler turns the chain back into an index and keeps the 18 bounds of a lane in LDS (72 bytes a lane, 18 432 a
// workgroup of 256; private slots, no barrier): not scratch.
__device__ __forceinline__ int pick9(const int (&v)[9], int which) {
    int r = v[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) r = which == k ? v[k] : r;
    return r;
}

// ---------------------------------------------------------------------------------------------- the counter
// adds v to stats[group][slot] (4 slots a group) for every lane with v != 0; a workgroup inside one group sends one atomic.
// All lanes of the workgroup call it.
__device__ __forceinline__ void count_into(int32_t *stats, bool uniform, int b, int slot, int v) {
    if (uniform) {
        const int total = __syncthreads_count(v);
        if (threadIdx.x == 0 && total) atomicAdd(&stats[b * 4 + slot], total);
    } else if (v) {
        atomicAdd(&stats[b * 4 + slot], 1);
    }
}

// ---------------------------------------------------------------------------------------------- the sort's room
// what a radix sort of n (Key, Val) pairs over `bits` key bits asks for
template <class Key, class Val>
inline size_t radix_temp_bytes(int64_t n, unsigned bits) {
    size_t s = 0;
    (void)rocprim::radix_sort_pairs(nullptr, s, (const Key *)nullptr, (Key *)nullptr, (const Val *)nullptr, (Val *)nullptr,
                                    (size_t)n, 0u, bits, (hipStream_t) nullptr);
    return s;
}

// rocPRIM does not promise that its temporary storage grows with n.  Two policies keep room for it, and an op keeps the one it
// was written with (its workspace size is part of what callers cache); temp_bytes(n) is what the op's rocPRIM calls ask for.
// room_next_pow2: n and the next power of two (from 1024).
template <class TempBytes>
inline int64_t room_next_pow2(int64_t n, TempBytes temp_bytes) {
    int64_t cap = 1024;
    while (cap < n) cap <<= 1;
    return align256((int64_t)imax((int64_t)temp_bytes(n), (int64_t)temp_bytes(cap)));
}

// room_all_pow2: n and every power of two up to the next one (from 1024), so it never shrinks as n grows.
template <class TempBytes>
inline int64_t room_all_pow2(int64_t n, TempBytes temp_bytes) {
    int64_t room = (int64_t)temp_bytes(n);
    for (int64_t cap = 1024; cap < 2 * imax(n, 1024); cap <<= 1) room = imax(room, (int64_t)temp_bytes(cap));
    return align256(room);
}

}  // namespace hpl
