// The device side of the spatial index (k_neighbours.hip builds it; DESIGN.md section 3, "Neighbours") for the kernels that walk
// it: k_neighbours.hip's own, k_clusters.hip's, k_knn.hip's, k_merge.hip's and k_match.hip's.  The cell key, its hash bucket, the
// 27-cell walk, the walk over the entries near one and the walk over the entries near a QUERY point that is no entry are stated
// here once, so that every walk over the index visits the cells the build made and tests pairs the same way.  (What only the
// build needs -- a stored position's cell -- stays in k_neighbours.hip.)
//
// Sites: the includer's bounds sites (k_splat_ops.h): bound_bucket (a bucket of the table), bound_entry (a slot of the entry array).
#pragma once
#include "gsr_internal.h"

#include <algorithm>

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
template <class Sites, class F>
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
                Sites::bound_bucket(b, (uint64_t)mask + 1u);
                if (!f(nk, b)) return;
            }
        }
    }
}

// f(j) for every OTHER entry within the radius of entry s (`me`; j: the other's splat index) that passes pre(j), while f returns
// true.  Per cell the bucket's (population, end) pair and its range of the entry array; the stored cell key is compared BEFORE
// anything else -- two of the 27 cells that hash to one bucket are walked twice and each pass takes only its own cell's entries --
// then pre, then the pair test: near(i, j) := i != j && (dx*dx + dy*dy) + dz*dz <= r2 in f64, in the written order, uncontracted.
// An entry IS a splat, so "i != j" is "another slot".  m: the entries.
template <class Sites, class P, class F>
__device__ __forceinline__ void nb_each_near(const NbIndex& ix, uint32_t m, uint32_t s, const uint4& me, P pre, F f)
{
    const uint2* __restrict__ table = reinterpret_cast<const uint2*>(ix.table);   // (population, one behind the last entry)
    const double x = (double)__uint_as_float(me.x), y = (double)__uint_as_float(me.y), z = (double)__uint_as_float(me.z);
    nb_each_cell<Sites>(ix.key[s], ix.bucket_mask, [&](unsigned long long nk, uint32_t b) {
        const uint2 t = table[b];
        Sites::bound_entry(t.y, (uint64_t)m + 1u);
        if (t.y > m || t.x > t.y) return true;   // (never: a range of the entry array)
        for (uint32_t e = t.y - t.x; e < t.y; e++) {
            if (ix.key[e] != nk || e == s) continue;
            const uint4 o = ix.entry[e];
            if (!pre(o.w)) continue;
            const double ex = x - (double)__uint_as_float(o.x), ey = y - (double)__uint_as_float(o.y), ez = z - (double)__uint_as_float(o.z);
            if ((ex * ex + ey * ey) + ez * ez <= ix.r2 && !f(o.w)) return false;
        }
        return true;
    });
}

// ---- a query: a point that is not an entry of the index (k_match.hip: a splat of ANOTHER scene under a trial transform) ----
// The query's cell coordinate: nb_cell's (k_neighbours.hip) floor and clamp, in f64 in front of the conversion, on a double where
// nb_cell takes a stored float.  The slack argument at the top of k_neighbours.hip holds for it unchanged.
__device__ __forceinline__ int32_t nb_cell_query(double v, double inv_h)
{
    double t = floor(v * inv_h);
    t = t < -(double)NB_CELL_HALF ? -(double)NB_CELL_HALF : t;
    t = t > (double)(NB_CELL_HALF - 1) ? (double)(NB_CELL_HALF - 1) : t;
    return (int32_t)t;
}

// f(j, d2) for every entry within the radius of the query point (x, y, z) whose cell key is k (j: the entry's splat index).  The
// query form of nb_each_near: the point is no entry, so there is no "another slot" test and no pre; the stored cell key is still
// compared BEFORE any f64 arithmetic, and d2 = (ex*ex + ey*ey) + ez*ez with e = query - entry, in f64, in the written order,
// uncontracted, a distance of exactly the radius counting.  The range is taken NB_QUERY_BATCH candidates at a time, their keys and
// entries loaded together in front of any use, as k_knn's walk takes it (a slot behind the range's end repeats the last one and
// is skipped).  m: the entries.
constexpr uint32_t NB_QUERY_BATCH = 4;
template <class Sites, class F>
__device__ __forceinline__ void nb_each_near_query(const NbIndex& ix, uint32_t m, unsigned long long k, double x, double y, double z, F f)
{
    const uint2* __restrict__ table = reinterpret_cast<const uint2*>(ix.table);   // (population, one behind the last entry)
    nb_each_cell<Sites>(k, ix.bucket_mask, [&](unsigned long long nk, uint32_t b) {
        const uint2 t = table[b];
        Sites::bound_entry(t.y, (uint64_t)m + 1u);
        if (t.y > m || t.x > t.y) return true;   // (never: a range of the entry array)
        for (uint32_t e0 = t.y - t.x; e0 < t.y; e0 += NB_QUERY_BATCH) {
            unsigned long long ck[NB_QUERY_BATCH];
            uint4 co[NB_QUERY_BATCH];
#pragma unroll
            for (uint32_t u = 0u; u < NB_QUERY_BATCH; u++) {
                const uint32_t eu = min(e0 + u, t.y - 1u);
                ck[u] = ix.key[eu];
                co[u] = ix.entry[eu];
            }
#pragma unroll
            for (uint32_t u = 0u; u < NB_QUERY_BATCH; u++) {
                if (e0 + u >= t.y || ck[u] != nk) continue;
                const uint4 o = co[u];
                const double ex = x - (double)__uint_as_float(o.x), ey = y - (double)__uint_as_float(o.y), ez = z - (double)__uint_as_float(o.z);
                const double d = (ex * ex + ey * ey) + ez * ez;
                if (d <= ix.r2) f(o.w, d);
            }
        }
        return true;
    });
}

// the grid of a grid-stride kernel over `work` items: NB_WG_PER_CU workgroups per compute unit, NB_MAX_GRID at most
inline uint32_t nb_grid(uint64_t work, int cu_count)
{
    const uint32_t most = std::min<uint32_t>(NB_WG_PER_CU * (uint32_t)std::max(cu_count, 1), NB_MAX_GRID);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((work + NB_THREADS - 1) / NB_THREADS, 1u), most);
}

}  // namespace gsr
