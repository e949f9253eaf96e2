// k nearest neighbours ("k nearest neighbours"): for every splat in scope the k nearest OTHER splats in scope
// within `radius` -- their indices and squared distances, ascending by the pair (d2, index) -- and one value per splat from that
// list: the distance to the k-th, or the mean distance to those found.  Statistical outlier removal is a picker on that value.
// The index is k_neighbours.hip's, as it is: scope, cells, the pair test and the treatment of non-finite rows are its own.
//
// The walk.  k_knn takes the ENTRIES in index order, one per lane, grid-stride, and visits the 27 cells (nb_each_cell): one
// 8-byte (population, end) load per cell, the stored cell key compared BEFORE any f64 arithmetic, so that an entry is met once
// however the cells hash.  What is new is that every lane keeps a sorted list.  A register array indexed by a loop variable
// becomes scratch memory, so the list lives in LDS, lane-strided: slot t of lane l at [t * blockDim + l], a column of d2 and a
// column of indices.  Consecutive lanes sit on consecutive banks whatever slot each of them is at, and a lane touches only its
// own column: no conflict and no barrier.  The worst pair kept (d2, j) and the list's length stay in registers.  A candidate
// is rejected by !(d2 <= r2) first, by (d2, j) >= worst once the list is full, and only a survivor pays the shift-insert.  The
// pair order is total over distinct splats, so the list a lane ends with is the k smallest pairs of its neighbourhood in
// ascending order whatever order they arrived in.  Nothing is pruned.
//
// The workgroup is sized by k (knn_threads): 12 bytes per lane and slot, 48 KiB of lists at most, so that three workgroups fit a
// CU's 160 KiB at k = 32.  At the end a lane computes its value from its own column in ascending slot order, stores found, the value
// and (LISTS) its k slots at the splat's row, and adds to the workgroup's LDS histogram of k + 1 counters (lds_counters_*, k_splat_ops.h).
// complete, finite_values, min and max are reduced over the wave and cost one atomic each per wave: the values are
// non-negative doubles, so min and max go through their bit patterns as 64-bit unsigned maxima (KnnInfo).
//
// Compiled with -ffp-contract=off like the rest of the device code.
#include "gsr_internal.h"
#include "k_splat_ops.h"
#include "k_neighbours.h"   // the key, the bucket and the 27-cell walk

namespace gsr {

GSR_BOUNDS_DECL(knn)   // sites: 0 set word, 1 entry slot, 2 bucket, 3 LDS list slot, 4 LDS counter, 5 global counter, 6 selection word, 7 splat row

// the sites of the shared helpers (k_splat_ops.h, k_neighbours.h)
struct knn_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(knn, 0, idx, limit); }
    static __device__ __forceinline__ void bound_bucket(unsigned long long idx, unsigned long long limit) { GSR_BOUND(knn, 2, idx, limit); }
    static __device__ __forceinline__ void bound_counter(unsigned long long idx, unsigned long long limit) { GSR_BOUND(knn, 5, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(knn, 6, idx, limit); }
};

// ---- the rows the walk does not reach ----
// Every row as a splat outside the index has it; the walk then overwrites the rows of its entries.
__global__ __launch_bounds__(NB_THREADS) void k_knn_fill(AttrScope sc, uint32_t n, uint32_t k, KnnArrays a)
{
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS, first = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x;
    for (uint64_t i = first; i < n; i += stride) {
        a.found[i] = 0u;
        a.values[i] = in_scope<knn_sites>(sc, n, i) ? f64_inf() : f64_nan();
    }
    if (!a.idx) return;
    const uint64_t slots = (uint64_t)n * k;
    for (uint64_t t = first; t < slots; t += stride) {
        a.idx[t] = KNN_NONE;
        a.d2[t] = f64_inf();
    }
}

// ---- the walk ----
constexpr uint32_t KNN_BATCH = 4;   // candidates whose loads are in flight together

template <int STAT, bool LISTS>
__global__ __launch_bounds__(NB_THREADS) void k_knn(NbIndex ix, uint32_t m /* entries */, uint32_t n /* splats */, uint32_t k, KnnArrays a, uint32_t* __restrict__ hist)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_knn[];   // k * T doubles, k * T words, k + 1 counters
    const uint32_t T = blockDim.x, slots = k * T;
    double* const s_d2 = reinterpret_cast<double*>(s_knn);
    uint32_t* const s_j = reinterpret_cast<uint32_t*>(s_d2 + slots);
    uint32_t* const s_hist = s_j + slots;
    lds_counters_zero(s_hist, k + 1u, T);
    double* const my_d2 = s_d2 + threadIdx.x;     // this lane's columns: slot t at [t * T]
    uint32_t* const my_j = s_j + threadIdx.x;
    const uint2* __restrict__ table = reinterpret_cast<const uint2*>(ix.table);   // (population, one behind the last entry)
    uint32_t complete = 0u, finite = 0u;
    unsigned long long vmax = 0ull, nvmin = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * T;
    for (uint64_t s = (uint64_t)blockIdx.x * T + threadIdx.x; s < m; s += stride) {
        GSR_BOUND(knn, 1, s, m);
        const uint4 me = ix.entry[s];
        const double x = (double)__uint_as_float(me.x), y = (double)__uint_as_float(me.y), z = (double)__uint_as_float(me.z);
        uint32_t found = 0u, wj = 0u;   // the list's length; (wd, wj): its last pair once it is full
        double wd = 0.0;
        nb_each_cell<knn_sites>(ix.key[s], ix.bucket_mask, [&](unsigned long long nk, uint32_t b) {
            const uint2 t = table[b];
            GSR_BOUND(knn, 1, t.y, (uint64_t)m + 1u);
            if (t.y > m || t.x > t.y) return true;   // (never: a range of the entry array)
            // Not nb_each_near's loop: KNN_BATCH candidates at a time, their keys and entries loaded together in front of any use.
            // With the few waves the lists leave room for, nothing else hides the latency of a load that waits for the one before
            // it (a slot behind the range's end repeats the last one and is skipped below)
            for (uint32_t e0 = t.y - t.x; e0 < t.y; e0 += KNN_BATCH) {
                unsigned long long ck[KNN_BATCH];
                uint4 co[KNN_BATCH];
#pragma unroll
                for (uint32_t u = 0u; u < KNN_BATCH; u++) {
                    const uint32_t eu = min(e0 + u, t.y - 1u);
                    ck[u] = ix.key[eu];
                    co[u] = ix.entry[eu];
                }
#pragma unroll
              for (uint32_t u = 0u; u < KNN_BATCH; u++) {
                const uint32_t e = e0 + u;
                if (e >= t.y || ck[u] != nk || e == (uint32_t)s) continue;
                const uint4 o = co[u];
                const double ex = x - (double)__uint_as_float(o.x), ey = y - (double)__uint_as_float(o.y), ez = z - (double)__uint_as_float(o.z);
                const double d = (ex * ex + ey * ey) + ez * ez;
                const uint32_t j = o.w;
                if (!(d <= ix.r2)) continue;
                if (found == k && !(d < wd || (d == wd && j < wj))) continue;
                // the slot that opens is the one behind the list, or the worst's; pairs above (d, j) move up one slot into it
                uint32_t at = found < k ? found : k - 1u;
                while (at > 0u) {
                    GSR_BOUND(knn, 3, at * T + threadIdx.x, slots);
                    const double pd = my_d2[(at - 1u) * T];
                    const uint32_t pj = my_j[(at - 1u) * T];
                    if (pd < d || (pd == d && pj < j)) break;
                    my_d2[at * T] = pd;
                    my_j[at * T] = pj;
                    at--;
                }
                GSR_BOUND(knn, 3, at * T + threadIdx.x, slots);
                my_d2[at * T] = d;
                my_j[at * T] = j;
                if (found < k) found++;
                if (found == k) { wd = my_d2[(k - 1u) * T]; wj = my_j[(k - 1u) * T]; }
              }
            }
            return true;
        });
        // the value, from the lane's own column in ascending slot order
        double value = f64_inf();
        if (STAT == KNN_KTH) {
            if (found == k) value = __dsqrt_rn(wd);
        } else if (found) {
            double sum = __dsqrt_rn(my_d2[0]);
            for (uint32_t t = 1u; t < found; t++) sum = sum + __dsqrt_rn(my_d2[t * T]);
            value = sum / (double)found;
        }
        GSR_BOUND(knn, 7, me.w, n);
        if (me.w < n) {
            a.found[me.w] = found;
            a.values[me.w] = value;
            if (LISTS) {
                const uint64_t row = (uint64_t)me.w * k;
                for (uint32_t t = 0u; t < k; t++) {
                    a.idx[row + t] = t < found ? my_j[t * T] : KNN_NONE;
                    a.d2[row + t] = t < found ? my_d2[t * T] : f64_inf();
                }
            }
        }
        GSR_BOUND(knn, 4, found, k + 1u);
        __hip_atomic_fetch_add(&s_hist[found < k ? found : k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        complete += found == k ? 1u : 0u;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(value);
        if (bits < 0x7ff0000000000000ull) {   // finite (a value is never negative)
            finite++;
            vmax = bits > vmax ? bits : vmax;
            nvmin = ~bits > nvmin ? ~bits : nvmin;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        complete += __shfl_xor(complete, d);
        finite += __shfl_xor(finite, d);
        const unsigned long long ov = __shfl_xor(vmax, d), on = __shfl_xor(nvmin, d);
        vmax = ov > vmax ? ov : vmax;
        nvmin = on > nvmin ? on : nvmin;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (complete) __hip_atomic_fetch_add(&a.info->complete, complete, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (finite) {
            __hip_atomic_fetch_add(&a.info->finite_values, finite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&a.info->vmax, vmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&a.info->nvmin, nvmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    lds_counters_flush<knn_sites>(s_hist, k + 1u, T, hist, KNN_MAX_K + 1u);
}

// ---- the picker ----
// gsr_select_knn.  One thread per bit of the mask: in scope, lo <= value && (value < hi || hi is +inf).  A wave's ballot is two
// whole words (mask_store_ballot): every word of the mask is stored.
__global__ __launch_bounds__(NB_THREADS) void k_knn_select(const double* __restrict__ values, AttrScope sc, uint32_t n, double lo, double hi, uint32_t open_hi,
                                                           uint32_t* __restrict__ scratch, uint32_t nwords)
{
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    bool in = false;
    if (in_scope<knn_sites>(sc, n, i)) {
        GSR_BOUND(knn, 7, i, n);
        const double v = values[i];
        in = lo <= v && (v < hi || open_hi != 0u);
    }
    mask_store_ballot<knn_sites>(scratch, nwords, i, __ballot(in));
}

// ---- launchers ----
void launch_knn_fill(const AttrScope& sc, uint32_t n, uint32_t k, const KnnArrays& a, int cu_count, hipStream_t s)
{
    hipLaunchKernelGGL(k_knn_fill, dim3(nb_grid(a.idx ? (uint64_t)n * k : n, cu_count)), dim3(NB_THREADS), 0, s, sc, n, k, a);
}

void launch_knn(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t k, int stat, const KnnArrays& a, uint32_t* hist, int cu_count, hipStream_t s)
{
    if (!indexed) return;
    const uint32_t threads = knn_threads(k);
    const uint32_t blocks = nb_grid((uint64_t)indexed * (NB_THREADS / threads), cu_count);   // (nb_grid counts in workgroups of NB_THREADS)
    const size_t lds = (size_t)k * threads * 12u + ((size_t)k + 1u) * sizeof(uint32_t);
    const bool lists = a.idx != nullptr;
    auto kernel = stat == KNN_KTH ? (lists ? k_knn<KNN_KTH, true> : k_knn<KNN_KTH, false>) : (lists ? k_knn<KNN_MEAN, true> : k_knn<KNN_MEAN, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, s, ix, indexed, n, k, a, hist);
}

void launch_knn_select(const double* values, const AttrScope& sc, uint32_t n, double lo, double hi, bool open_hi, uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_knn_select, dim3(mask_blocks(nwords, NB_THREADS)), dim3(NB_THREADS), 0, s, values, sc, n, lo, hi, open_hi ? 1u : 0u, scratch, nwords);
}

}  // namespace gsr
