// The device side of the spatial index (k_neighbours.hip builds it; DESIGN.md section 3, "Neighbours") for the kernels that walk
// it: k_neighbours.hip's own and k_clusters.hip's.  The cell key, its hash bucket and the 27-cell walk are stated here once, so
// that every walk over the index visits the cells the build made.  (What only the build needs -- a position's cell, the scope of a
// call -- stays in k_neighbours.hip.)
//
// The bounds twin counts per translation unit, so the includer names its own site in front of the include:
//     NB_BOUND_BUCKET(idx, limit)   a bucket of the table
#pragma once
#include "gsr_internal.h"

#include <algorithm>

#ifndef NB_BOUND_BUCKET
#error "define NB_BOUND_BUCKET (the translation unit's GSR_BOUND site for a bucket) in front of k_neighbours.h"
#endif

namespace gsr {

constexpr int NB_THREADS = 256;

__device__ __forceinline__ unsigned long long nb_key(int32_t cx, int32_t cy, int32_t cz)
{
    return (unsigned long long)(uint32_t)(cx + NB_CELL_HALF) | (unsigned long long)(uint32_t)(cy + NB_CELL_HALF) << 21 |
           (unsigned long long)(uint32_t)(cz + NB_CELL_HALF) << 42;
}

__device__ __forceinline__ uint32_t nb_bucket(unsigned long long k, uint32_t mask)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k & mask;
}

// f(key, bucket) for each of the 27 cells around the cell of key k that lie inside the clamp, while f returns true
template <class F>
__device__ __forceinline__ void nb_each_cell(unsigned long long k, uint32_t mask, F f)
{
    const int32_t cx = (int32_t)((uint32_t)k & 0x1fffffu) - NB_CELL_HALF, cy = (int32_t)((uint32_t)(k >> 21) & 0x1fffffu) - NB_CELL_HALF,
                  cz = (int32_t)((uint32_t)(k >> 42) & 0x1fffffu) - NB_CELL_HALF;
    for (int32_t z = cz - 1; z <= cz + 1; z++) {
        if (z < -NB_CELL_HALF || z >= NB_CELL_HALF) continue;
        for (int32_t y = cy - 1; y <= cy + 1; y++) {
            if (y < -NB_CELL_HALF || y >= NB_CELL_HALF) continue;
            for (int32_t x = cx - 1; x <= cx + 1; x++) {
                if (x < -NB_CELL_HALF || x >= NB_CELL_HALF) continue;
                const unsigned long long nk = nb_key(x, y, z);
                const uint32_t b = nb_bucket(nk, mask);
                NB_BOUND_BUCKET(b, (uint64_t)mask + 1u);
                if (!f(nk, b)) return;
            }
        }
    }
}

// the grid of a grid-stride kernel over `work` items: NB_WG_PER_CU workgroups per compute unit, NB_MAX_GRID at most
inline uint32_t nb_grid(uint64_t work, int cu_count)
{
    const uint32_t most = std::min<uint32_t>(NB_WG_PER_CU * (uint32_t)std::max(cu_count, 1), NB_MAX_GRID);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((work + NB_THREADS - 1) / NB_THREADS, 1u), most);
}

}  // namespace gsr
