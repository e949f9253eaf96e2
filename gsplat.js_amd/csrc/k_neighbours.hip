// Neighbours ("Neighbours"): for every splat in scope, the number of OTHER splats in scope within `radius` of
// it -- the first thing here that relates splats to each other, so the first that needs a spatial index.  The index lives for
// one call: the scene may have been edited since the last one, and building it costs less than the walk it serves.
//
// Cells.  A uniform grid of side h = radius * (1 + 2^-10); a splat's cell coordinate is floor((double)x * inv_h), inv_h = 1 / h from
// the host, clamped to [-2^20, 2^20) per axis, and three coordinates pack into a 63-bit key.  The side is strictly larger than
// the radius on purpose: with h == radius two splats exactly `radius` apart can land two cells apart after rounding, and a walk
// of +-1 cell would miss a pair the definition counts.  Multiplying by one constant, floor and the clamp are all monotone, and
// 2^-10 of slack is far more than the product's rounding error anywhere inside the clamp (2^20 * 2^-53), so two splats within
// `radius` of each other are never more than one cell apart on any axis: the 27-cell walk is complete.  Everything at or beyond
// the clamp shares the boundary cell, which costs pair tests and no pair.  Nothing in the argument needs the multiplied value to
// have been a float: it holds unchanged for a query point given as a double (nb_cell_query, k_neighbours.h), which is how
// k_match.hip finds the cell of a splat of another scene under a trial transform.
//
// Index.  A hashed grid -- floaters are exactly what stretches a bounding box, so nothing dense -- built as a counting sort by
// bucket: k_nb_cells<false> counts the splats of every bucket with one relaxed atomic each, k_nb_offsets gives every bucket its
// range of the entry array, k_nb_cells<true> scatters (position bits, index) and the cell key through the buckets' cursors.  The
// buckets are a power of two, at least twice the scene's count.  k_nb_offsets is a workgroup scan plus ONE atomic on a global cursor per
// workgroup: the ranges are disjoint and dense but in no particular order across workgroups, which nothing needs -- every
// result below is a count, independent of where an entry sits -- and it saves the second and third pass of a global scan.
// Splats out of scope or with a NaN / infinite component are counted (NbInfo) and never indexed; a run of 64 splats out of scope
// costs its set words and no read of the scene (in_scope, k_splat_ops.h).
//
// Walks.  k_nb_bound and k_nb_count take the ENTRIES in index order, one per lane, so that the lanes of a wave that share a
// bucket share its 27 neighbours.  For each of the 27 cells (those outside the clamp hold nothing and are skipped) the lane reads
// the bucket's (population, end) pair; k_nb_bound adds the population, k_nb_count walks the entries near its own (nb_each_near,
// k_neighbours.h: the stored cell key compared BEFORE any f64 arithmetic, the pair test in f64, in the written order,
// uncontracted); a lane stops at `cap`.  Counts go to counts[index] with ordinary stores; the histogram goes through per-workgroup
// LDS counters and one relaxed agent-scope add per non-zero counter (lds_counters_*, k_splat_ops.h).
//
// Compiled with -ffp-contract=off like the rest of the device code.
#include "gsr_internal.h"
#include "k_splat_ops.h"
#include "k_neighbours.h"   // the key, the bucket, the 27-cell walk and the near walk, shared with the other units over the index

namespace gsr {

GSR_BOUNDS_DECL(neighbours)   // sites: 0 set word, 1 splat index, 2 bucket, 3 entry slot, 4 LDS counter, 5 global counter, 6 selection word, 7 counts word

// the sites of the shared helpers (k_splat_ops.h, k_neighbours.h)
struct nb_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(neighbours, 0, idx, limit); }
    static __device__ __forceinline__ void bound_bucket(unsigned long long idx, unsigned long long limit) { GSR_BOUND(neighbours, 2, idx, limit); }
    static __device__ __forceinline__ void bound_entry(unsigned long long idx, unsigned long long limit) { GSR_BOUND(neighbours, 3, idx, limit); }
    static __device__ __forceinline__ void bound_counter(unsigned long long idx, unsigned long long limit) { GSR_BOUND(neighbours, 5, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(neighbours, 6, idx, limit); }
};

// ---- cells ----
// floor, not truncation; the clamp in f64, in front of the conversion
__device__ __forceinline__ int32_t nb_cell(float v, double inv_h)
{
    double t = floor((double)v * inv_h);
    t = t < -(double)NB_CELL_HALF ? -(double)NB_CELL_HALF : t;
    t = t > (double)(NB_CELL_HALF - 1) ? (double)(NB_CELL_HALF - 1) : t;
    return (int32_t)t;
}

// ---- the index ----
// SCATTER false: the buckets' populations, and the call's counts of splats in scope and of non-finite ones among them (those are
// hist[0]'s: their count is 0).  SCATTER true: the same walk once more, every indexed splat into its bucket's next slot.
template <bool SCATTER>
__global__ __launch_bounds__(NB_THREADS) void k_nb_cells(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz, AttrScope sc,
                                                         uint32_t n, NbIndex ix, uint32_t* __restrict__ hist0)
{
    uint32_t scoped = 0u, nonfinite = 0u;   // splats in scope; of those, non-finite
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS, end = ((uint64_t)n + 63u) & ~63ull;   // whole waves step together
    for (uint64_t i = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; i < end; i += stride) {
        if (!in_scope<nb_sites>(sc, n, i)) continue;
        GSR_BOUND(neighbours, 1, i, n);
        const float x = px[i], y = py[i], z = pz[i];
        scoped++;
        if (!(f32_finite(x) && f32_finite(y) && f32_finite(z))) { nonfinite++; continue; }
        const unsigned long long k = nb_key(nb_cell(x, ix.inv_h), nb_cell(y, ix.inv_h), nb_cell(z, ix.inv_h));
        const uint32_t b = nb_bucket(k, ix.bucket_mask);
        GSR_BOUND(neighbours, 2, b, (uint64_t)ix.bucket_mask + 1u);
        if (!SCATTER) {
            __hip_atomic_fetch_add(&ix.table[2ull * b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const uint32_t slot = __hip_atomic_fetch_add(&ix.table[2ull * b + 1u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            GSR_BOUND(neighbours, 3, slot, n);
            if (slot < n) {   // (always: the cursors were laid out from the same populations)
                ix.entry[slot] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), (uint32_t)i);
                ix.key[slot] = k;
            }
        }
    }
    if (SCATTER) return;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { scoped += __shfl_xor(scoped, d); nonfinite += __shfl_xor(nonfinite, d); }
    if ((threadIdx.x & 63u) != 0u) return;
    if (scoped) __hip_atomic_fetch_add(&ix.info->in_scope, scoped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nonfinite) {
        __hip_atomic_fetch_add(&ix.info->nonfinite, nonfinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (hist0) __hip_atomic_fetch_add(hist0, nonfinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One thread per bucket (the grid covers the table exactly: the buckets are a multiple of NB_THREADS).  The workgroup's
// populations are scanned, the workgroup takes its range of the entry array with one atomic on the cursor info->indexed, and every
// bucket's cursor becomes its first slot.  info->indexed ends as the number of entries.
__global__ __launch_bounds__(NB_THREADS) void k_nb_offsets(NbIndex ix)
{
    __shared__ uint32_t s_wave[NB_THREADS / WAVE];
    __shared__ uint32_t s_base;
    const uint64_t b = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x;
    GSR_BOUND(neighbours, 2, b, (uint64_t)ix.bucket_mask + 1u);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = ix.table[2ull * b];
    uint32_t v = c;   // -> the inclusive sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (int w = 0; w < NB_THREADS / WAVE; w++) { if (w < wave) before += s_wave[w]; total += s_wave[w]; }
    if (threadIdx.x == 0) s_base = total ? __hip_atomic_fetch_add(&ix.info->indexed, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    __syncthreads();
    ix.table[2ull * b + 1u] = s_base + before + (v - c);
}

// ---- the bound ----
// What k_nb_count walks at most (no early exit): per entry the populations of its 27 buckets, a bucket two cells share counted
// twice, as the walk visits it twice.  64-bit sums, reduced per workgroup, one atomic per workgroup.
__global__ __launch_bounds__(NB_THREADS) void k_nb_bound(NbIndex ix, uint32_t n)
{
    const uint32_t m = min(ix.info->indexed, n);
    unsigned long long sum = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < m; s += stride) {
        GSR_BOUND(neighbours, 3, s, n);
        nb_each_cell<nb_sites>(ix.key[s], ix.bucket_mask, [&](unsigned long long, uint32_t b) { sum += ix.table[2ull * b]; return true; });
    }
    workgroup_sum_u64<NB_THREADS>(sum, &ix.info->pair_bound);
}

// ---- the count ----
// near(i, j) := i != j && d2(i, j) <= r2, with d2 in f64 in the header's order.  An entry IS a splat, so "i != j" is "another slot".
template <bool HIST>
__global__ __launch_bounds__(NB_THREADS) void k_nb_count(NbIndex ix, uint32_t m /* entries */, uint32_t n /* splats */, uint32_t cap, uint32_t* __restrict__ counts,
                                                         uint32_t* __restrict__ hist)
{
    extern __shared__ uint32_t s_hist[];   // cap + 1 (HIST)
    if (HIST) lds_counters_zero(s_hist, cap + 1u, NB_THREADS);
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < m; s += stride) {
        GSR_BOUND(neighbours, 3, s, m);
        const uint4 me = ix.entry[s];
        uint32_t count = 0u;
        nb_each_near<nb_sites>(ix, m, (uint32_t)s, me, [](uint32_t) { return true; }, [&](uint32_t) { return ++count < cap; });
        GSR_BOUND(neighbours, 7, me.w, n);
        if (me.w < n) counts[me.w] = count;
        if (HIST) {
            GSR_BOUND(neighbours, 4, count, cap + 1u);
            __hip_atomic_fetch_add(&s_hist[count < cap ? count : cap], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    if (HIST) lds_counters_flush<nb_sites>(s_hist, cap + 1u, NB_THREADS, hist, NB_MAX_CAP + 1u);
}

// ---- the picker ----
// gsr_select_neighbours.  One thread per bit of the mask: in scope, lo <= count && count < hi (a splat in scope that is not
// indexed has the caller's zero).  A wave's ballot is two whole words (mask_store_ballot): every word of the mask is stored.
__global__ __launch_bounds__(NB_THREADS) void k_nb_select(const uint32_t* __restrict__ counts, AttrScope sc, uint32_t n, uint32_t lo, uint32_t hi,
                                                          uint32_t* __restrict__ scratch, uint32_t nwords)
{
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    bool in = false;
    if (in_scope<nb_sites>(sc, n, i)) {
        GSR_BOUND(neighbours, 7, i, n);
        const uint32_t c = counts[i];
        in = lo <= c && c < hi;
    }
    mask_store_ballot<nb_sites>(scratch, nwords, i, __ballot(in));
}

// ---- launchers ----
void launch_nb_build(const NbIndex& ix, const float* px, const float* py, const float* pz, const AttrScope& sc, uint32_t n, int cu_count, uint32_t* hist0,
                     hipStream_t s)
{
    const uint32_t blocks = nb_grid(n, cu_count);
    hipLaunchKernelGGL(k_nb_cells<false>, dim3(blocks), dim3(NB_THREADS), 0, s, px, py, pz, sc, n, ix, hist0);
    hipLaunchKernelGGL(k_nb_offsets, dim3((uint32_t)(((uint64_t)ix.bucket_mask + 1u) / NB_THREADS)), dim3(NB_THREADS), 0, s, ix);
    hipLaunchKernelGGL(k_nb_cells<true>, dim3(blocks), dim3(NB_THREADS), 0, s, px, py, pz, sc, n, ix, (uint32_t*)nullptr);
}

void launch_nb_bound(const NbIndex& ix, uint32_t n, int cu_count, hipStream_t s)
{
    hipLaunchKernelGGL(k_nb_bound, dim3(nb_grid(n, cu_count)), dim3(NB_THREADS), 0, s, ix, n);
}

void launch_nb_count(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t cap, uint32_t* counts, uint32_t* hist, int cu_count, hipStream_t s)
{
    if (!indexed) return;
    const uint32_t blocks = nb_grid(indexed, cu_count);
    if (hist)
        hipLaunchKernelGGL(k_nb_count<true>, dim3(blocks), dim3(NB_THREADS), ((size_t)cap + 1u) * sizeof(uint32_t), s, ix, indexed, n, cap, counts, hist);
    else
        hipLaunchKernelGGL(k_nb_count<false>, dim3(blocks), dim3(NB_THREADS), 0, s, ix, indexed, n, cap, counts, hist);
}

void launch_nb_select(const uint32_t* counts, const AttrScope& sc, uint32_t n, uint32_t lo, uint32_t hi, uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_nb_select, dim3(mask_blocks(nwords, NB_THREADS)), dim3(NB_THREADS), 0, s, counts, sc, n, lo, hi, scratch, nwords);
}

}  // namespace gsr
