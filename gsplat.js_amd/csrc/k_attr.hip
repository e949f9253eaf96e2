// Splat data ("Splat data"): what the scene's own attributes look like -- count, NaNs, minimum and maximum
// (k_attr_stats), a histogram over [lo, hi) (k_attr_hist) -- and the splats whose value lies in a range, as a picker
// (k_attr_select).  The value of attribute a of splat i is k_attr.h's attr_value, f64; nothing here states one of its own.
//
// The two reductions are grid-stride loops over runs of 64 splats, one per wave and step, on a grid sized from the device's
// compute units (attr_grid).  A lane's scope bit is in_scope's (k_splat_ops.h), so a wave whose 64 splats are all out of scope has
// no lane left behind the test and loads nothing of the scene: a 1 % selection costs the words' n / 8 bytes.
// Counts are integers, minimum and maximum commute: no result depends on the grid or on the order of arrival.
//
// The histogram is a per-workgroup LDS histogram of bins + 3 counters (below, at or above hi, NaN behind the bins): one LDS atomic
// per lane in scope, and at the end one relaxed agent-scope add per non-zero counter (lds_counters_*, k_splat_ops.h).  The case to fear was every splat in one
// bin -- opacity 255 everywhere, pixels == 0 after a short tour -- where 64 lanes of every wave meet in one LDS address.
// Measured it is the FASTEST case: the LDS serves a wave's 64 same-address adds in well under the time
// its loads take, and a workgroup then flushes one counter instead of hundreds.  What costs is the flush: same-address global
// atomics of many workgroups queue up, so the grid is two workgroups per compute unit, not more.  ATTR_HIST_PEEL, which peels
// the bin of the wave's first lane in scope with a ballot and adds its popcount once, measured 0.2 - 3.4 us SLOWER in every case and
// is kept only as the other side of that A/B (GSR_ATTR_HIST=peel): the same counters.
//
// Compiled with -ffp-contract=off like the rest of the device code.
#include "gsr_internal.h"
#include "k_attr.h"
#include "k_splat_ops.h"

#include <algorithm>

namespace gsr {

GSR_BOUNDS_DECL(attr)   // sites: 0 set word, 1 splat index, 2 LDS counter, 3 global counter, 4 partial slot, 5 selection word

constexpr int ATTR_THREADS = 256;

// the sites of the shared helpers (k_splat_ops.h)
struct attr_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(attr, 0, idx, limit); }
    static __device__ __forceinline__ void bound_counter(unsigned long long idx, unsigned long long limit) { GSR_BOUND(attr, 3, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(attr, 5, idx, limit); }
};

// ---- count, NaNs, minimum, maximum ----
// A value enters min only through `v < min` and max only through `v > max`, in a thread's fold, across lanes, waves and partials
// alike: a NaN is counted apart and never enters, infinities do, and nothing in scope leaves (+inf, -inf).
__device__ __forceinline__ void stats_take(AttrStats& a, uint32_t count, uint32_t nan, double mn, double mx)
{
    a.count += count; a.nan += nan;
    if (mn < a.mn) a.mn = mn;
    if (mx > a.mx) a.mx = mx;
}

__device__ __forceinline__ AttrStats stats_empty()
{
    AttrStats a;
    a.count = 0u; a.nan = 0u;
    a.mn = f64_inf(); a.mx = -f64_inf();
    return a;
}

// every thread's -> the workgroup's, valid in thread 0; s_part: one per wave
__device__ __forceinline__ void stats_reduce(AttrStats& a, AttrStats* s_part)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t oc = __shfl_xor(a.count, d), on = __shfl_xor(a.nan, d);
        const double omn = __shfl_xor(a.mn, d), omx = __shfl_xor(a.mx, d);
        stats_take(a, oc, on, omn, omx);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_part[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < ATTR_THREADS / WAVE; w++) stats_take(a, s_part[w].count, s_part[w].nan, s_part[w].mn, s_part[w].mx);
}

__global__ __launch_bounds__(ATTR_THREADS) void k_attr_stats(int attr, AttrSource src, AttrScope sc, uint32_t n, AttrStats* __restrict__ partial, uint32_t nparts)
{
    __shared__ AttrStats s_part[ATTR_THREADS / WAVE];
    AttrStats a = stats_empty();
    const uint64_t stride = (uint64_t)gridDim.x * ATTR_THREADS, end = ((uint64_t)n + 63u) & ~63ull;   // whole waves step together
    for (uint64_t i = (uint64_t)blockIdx.x * ATTR_THREADS + threadIdx.x; i < end; i += stride) {
        if (!in_scope<attr_sites>(sc, n, i)) continue;
        GSR_BOUND(attr, 1, i, n);
        const double v = attr_value(attr, src, (uint32_t)i);
        if (v != v) stats_take(a, 1u, 1u, a.mn, a.mx);
        else stats_take(a, 1u, 0u, v, v);
    }
    stats_reduce(a, s_part);
    if (threadIdx.x != 0) return;
    GSR_BOUND(attr, 4, blockIdx.x, nparts);
    if (blockIdx.x < nparts) partial[blockIdx.x] = a;
}

// one workgroup: the partials -> *out
__global__ __launch_bounds__(ATTR_THREADS) void k_attr_stats_fold(const AttrStats* __restrict__ partial, uint32_t nparts, AttrStats* __restrict__ out)
{
    __shared__ AttrStats s_part[ATTR_THREADS / WAVE];
    AttrStats a = stats_empty();
    for (uint32_t p = threadIdx.x; p < nparts; p += ATTR_THREADS) {
        GSR_BOUND(attr, 4, p, nparts);
        stats_take(a, partial[p].count, partial[p].nan, partial[p].mn, partial[p].mx);
    }
    stats_reduce(a, s_part);
    if (threadIdx.x == 0) *out = a;
}

// ---- the histogram ----
// The counter of value v: its bin, or bins + 0 (v < lo), bins + 1 (v >= hi), bins + 2 (NaN).  Edges (include/gsplat_hip.h):
// edge(k) = k == bins ? hi : min(lo + (double)k * w, hi) with w = (hi - lo) / (double)bins; the bin of lo <= v < hi is the largest
// b < bins with edge(b) <= v.  An estimate, (v - lo) / w floored, then corrected against the edges themselves: the estimate is
// off by at most a step or two, and what decides is the very comparison a range selection makes.
__device__ __forceinline__ double attr_edge(const AttrRange& r, uint32_t k)
{
    if (k == r.bins) return r.hi;
    const double e = r.lo + (double)k * r.w;
    return e < r.hi ? e : r.hi;
}

__device__ __forceinline__ uint32_t attr_counter(const AttrRange& r, double v)
{
    if (v != v) return r.bins + 2u;
    if (v < r.lo) return r.bins;
    if (!(v < r.hi)) return r.bins + 1u;
    const double t = (v - r.lo) / r.w;   // (w may round to 0 in a range of a few subnormals: inf or NaN here, the last bin below)
    uint32_t b = t < (double)r.bins ? (uint32_t)t : r.bins - 1u;
    while (b + 1u < r.bins && attr_edge(r, b + 1u) <= v) b++;
    while (b > 0u && attr_edge(r, b) > v) b--;
    return b;
}

template <int FORM>
__global__ __launch_bounds__(ATTR_THREADS) void k_attr_hist(int attr, AttrSource src, AttrScope sc, uint32_t n, AttrRange r, uint32_t* __restrict__ counters)
{
    extern __shared__ uint32_t s_hist[];   // bins + 3
    const uint32_t ncounters = r.bins + 3u;
    lds_counters_zero(s_hist, ncounters, ATTR_THREADS);

    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * ATTR_THREADS, end = ((uint64_t)n + 63u) & ~63ull;   // whole waves step together
    for (uint64_t i = (uint64_t)blockIdx.x * ATTR_THREADS + threadIdx.x; i < end; i += stride) {
        const bool in = in_scope<attr_sites>(sc, n, i);
        uint32_t b = 0u;
        if (in) {
            GSR_BOUND(attr, 1, i, n);
            b = attr_counter(r, attr_value(attr, src, (uint32_t)i));
            GSR_BOUND(attr, 2, b, ncounters);
            if (b >= ncounters) b = ncounters - 1u;
        }
        bool mine = in;   // this lane still owes its counter an add
        if (FORM == ATTR_HIST_PEEL) {
            const uint64_t act = __ballot(in);
            if (!act) continue;
            // the counter of the first lane in scope, and every lane that shares it: one add of their number
            const int leader = __builtin_ctzll(act);
            const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
            const uint64_t same = __ballot(in && b == lb);
            if (lane == leader) __hip_atomic_fetch_add(&s_hist[lb], (uint32_t)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            mine = in && b != lb;
        }
        if (mine) __hip_atomic_fetch_add(&s_hist[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    lds_counters_flush<attr_sites>(s_hist, ncounters, ATTR_THREADS, counters, ATTR_MAX_BINS + 3u);
}

// ---- the range picker ----
// gsr_select_attr.  One thread per bit of the mask: lo <= v && v < hi, so a NaN is never picked.  A wave's ballot is two
// whole words of the mask (mask_store_ballot, k_splat_ops.h): every word is stored (splats at and above n vote 0).
__global__ __launch_bounds__(ATTR_THREADS) void k_attr_select(int attr, AttrSource src, uint32_t n, double lo, double hi, uint32_t* __restrict__ scratch,
                                                              uint32_t nwords)
{
    const uint32_t i = blockIdx.x * ATTR_THREADS + threadIdx.x;
    bool in = false;
    if (i < n) {
        GSR_BOUND(attr, 1, i, n);
        const double v = attr_value(attr, src, i);
        in = lo <= v && v < hi;
    }
    mask_store_ballot<attr_sites>(scratch, nwords, i, __ballot(in));
}

// ---- launchers ----
uint32_t attr_grid(uint32_t n, int cu_count, uint32_t per_cu)
{
    const uint32_t cap = per_cu * (uint32_t)std::min(std::max(cu_count, 1), (int)(ATTR_MAX_GRID / per_cu));
    return std::min<uint32_t>(std::max<uint32_t>((uint32_t)(((uint64_t)n + ATTR_THREADS - 1) / ATTR_THREADS), 1u), cap);
}

void launch_attr_stats(int attr, const AttrSource& src, const AttrScope& sc, uint32_t n, int cu_count, AttrStats* partial, AttrStats* out, hipStream_t s)
{
    const uint32_t blocks = attr_grid(n, cu_count, ATTR_STATS_WG_PER_CU);
    hipLaunchKernelGGL(k_attr_stats, dim3(blocks), dim3(ATTR_THREADS), 0, s, attr, src, sc, n, partial, blocks);
    hipLaunchKernelGGL(k_attr_stats_fold, dim3(1), dim3(ATTR_THREADS), 0, s, (const AttrStats*)partial, blocks, out);
}

void launch_attr_hist(int attr, const AttrSource& src, const AttrScope& sc, uint32_t n, uint32_t blocks, const AttrRange& r, int form, uint32_t* counters,
                      hipStream_t s)
{
    blocks = std::max(blocks, 1u);
    const size_t lds = ((size_t)r.bins + 3u) * sizeof(uint32_t);
    if (form == ATTR_HIST_PLAIN)
        hipLaunchKernelGGL(k_attr_hist<ATTR_HIST_PLAIN>, dim3(blocks), dim3(ATTR_THREADS), lds, s, attr, src, sc, n, r, counters);
    else
        hipLaunchKernelGGL(k_attr_hist<ATTR_HIST_PEEL>, dim3(blocks), dim3(ATTR_THREADS), lds, s, attr, src, sc, n, r, counters);
}

void launch_attr_select(int attr, const AttrSource& src, uint32_t n, double lo, double hi, uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_attr_select, dim3(mask_blocks(nwords, ATTR_THREADS)), dim3(ATTR_THREADS), 0, s, attr, src, n, lo, hi, scratch, nwords);
}

}  // namespace gsr
