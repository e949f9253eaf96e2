// Clusters ("Clusters"): the connected islands of the splats in scope at a linking radius -- connected
// components, or DBSCAN with a core threshold -- labelled, sized and picked.  The second operation that relates splats to each
// other; it walks the index k_neighbours.hip builds through k_neighbours.h's nb_each_near: the same keys, buckets, 27 cells and pair
// test, near(i, j) := i != j && (dx*dx + dy*dy) + dz*dz <= r2 in f64, in the written order, uncontracted, the stored cell key
// compared before any f64 arithmetic.
//
// Stages, one launch each, so that what a stage reads is final:
//   core     launch_nb_count with cap = min_pts (k_neighbours.hip): core_i := counts[i] >= min_pts.  Skipped for min_pts == 0.
//   seed     parent[i] = i for every core entry; every other word of parent[] is the host's CL_NONE.
//   union    one lane per entry; a core entry i hooks itself to every near core entry j with j < i.
//   flatten  label[i] = find(i) for core entries (parent[] becomes label[]; no halving here, so that the only store into a word is
//            its own root); size[label] += 1; a root is a cluster.
//   border   a non-core entry takes the smallest label among its near core entries (their labels are final: another launch).
//   sizes    sizes[i] = size[label[i]] per splat; the largest cluster as one 64-bit maximum of size << 32 | ~label, which makes the
//            tie go to the smallest label.
//   pick     a wave's ballot stored as two whole words into the selection's scratch (mask_store_ballot, k_splat_ops.h).
//
// The union is lock-free hooking in ECL-CC's form.  INVARIANT: parent[x] <= x at every instant (CL_NONE words are never followed:
// only core splats are linked, and theirs are seeded).  It holds after the seed (parent[x] == x); a hook is ONE
// atomicCAS(&parent[big], big, small) with small < big, which changes a root's word only, to a smaller index; path halving stores
// into parent[x] a value read from parent[parent[x]], an ancestor of x, which by the invariant is no larger than parent[x].  So
// parent pointers strictly decrease along every path: there is no cycle, a path has fewer than n links, and the root of a tree is
// its smallest index -- hence label = the smallest index of the class with no further pass.
// TERMINATION.  find follows strictly decreasing indices: fewer than n steps.  A hook that fails returns the word it found at
// parent[big], which is != big and, by the invariant, < big: the retry continues from a strictly smaller index, so a lane makes
// fewer than n retries.  No lane ever waits for another lane -- no lock, no flag that is spun on -- so the lockstep of a wave cannot
// livelock it: every lane's loop is bounded by its OWN progress down the indices.  Each loop still carries a step limit of n and
// checks the invariant on every word it follows; a violation (an inconsistent index, memory damaged by something else) sets
// info->fault and ends the lane, the host turns the word into GSR_ERR_HIP: the call ends instead of occupying a shared GPU.
// Parent words are read with relaxed agent-scope atomic loads and written with the CAS or relaxed atomic stores; nothing else
// travels between lanes, and what one stage leaves the next reads behind the kernel boundary.
//
// Every store through an index computed on the device (parent[root], size[label], the selection's words) is guarded in the shipped
// build and is a GSR_BOUND site in the bounds twin.  Compiled with -ffp-contract=off like the rest of the device code.
#include "gsr_internal.h"
#include "k_splat_ops.h"

#include "k_neighbours.h"

namespace gsr {

GSR_BOUNDS_DECL(clusters)   // sites: 0 set word, 1 entry slot, 2 bucket, 3 parent / label word, 4 size word, 5 selection word, 6 counts word, 7 sizes word

// the sites of the shared helpers (k_splat_ops.h, k_neighbours.h)
struct cl_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(clusters, 0, idx, limit); }
    static __device__ __forceinline__ void bound_entry(unsigned long long idx, unsigned long long limit) { GSR_BOUND(clusters, 1, idx, limit); }
    static __device__ __forceinline__ void bound_bucket(unsigned long long idx, unsigned long long limit) { GSR_BOUND(clusters, 2, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(clusters, 5, idx, limit); }
};

__device__ __forceinline__ uint32_t cl_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_fault(ClInfo* info) { __hip_atomic_store(&info->fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree; HALVE: with path halving.  CL_NONE when x is no index, a word breaks the invariant or the walk exceeds n
// steps (info->fault is set): the caller drops what it was doing.  The flatten pass finds without halving: there a lane stores its
// OWN word's root, and a halving store of another lane, holding an older ancestor, could land behind it.
template <bool HALVE>
__device__ __forceinline__ uint32_t cl_find(uint32_t* parent, uint32_t x, uint32_t n, ClInfo* info)
{
    GSR_BOUND(clusters, 3, x, n);
    if (x >= n) { cl_fault(info); return CL_NONE; }
    uint32_t p = cl_load(&parent[x]);
    for (uint32_t steps = 0u; p != x; steps++) {
        if (p > x || steps >= n) { cl_fault(info); return CL_NONE; }   // (p > x covers CL_NONE; p < x < n below)
        const uint32_t g = cl_load(&parent[p]);
        if (HALVE && g < p) cl_store(&parent[x], g);                   // halving: an ancestor, no larger than p
        x = p; p = g;
    }
    return x;
}

// from's tree and j's into one: the larger root hooked onto the smaller with one CAS; a failed CAS continues from the word it found.
// Returns the smaller root -- a node of the merged tree at or near its root, from which the caller's next union starts instead of
// walking up from its own splat again (a stale one only costs the steps to the root); `from` itself after a fault.
__device__ __forceinline__ uint32_t cl_unite(uint32_t* parent, uint32_t from, uint32_t j, uint32_t n, ClInfo* info)
{
    uint32_t a = cl_find<true>(parent, from, n, info), b = cl_find<true>(parent, j, n, info);
    for (uint32_t retries = 0u; a != b; retries++) {
        if (a == CL_NONE || b == CL_NONE) return from;
        const uint32_t big = a > b ? a : b, small = a > b ? b : a;
        GSR_BOUND(clusters, 3, big, n);                                // (big < n: cl_find returned it)
        const uint32_t old = atomicCAS(&parent[big], big, small);
        if (old == big) return small;                                  // hooked
        if (old > big || retries >= n) { cl_fault(info); return from; }   // (never: old != big is < big by the invariant)
        a = cl_find<true>(parent, old, n, info); b = small;            // strictly below big
    }
    return a == CL_NONE ? from : a;
}

// is splat j (an entry's index) core?  counts[] is launch_nb_count's with cap = min_pts (all zero for min_pts == 0)
__device__ __forceinline__ bool cl_core(const uint32_t* __restrict__ counts, uint32_t j, uint32_t n, uint32_t min_pts)
{
    GSR_BOUND(clusters, 6, j, n);
    return j < n && counts[j] >= min_pts;
}

// size[label] += 1 for the lanes with `mine`, one add per distinct label of the wave (entries lie bucket by bucket: the lanes of
// a wave mostly share a label).  Whole waves call it together.
__device__ __forceinline__ void cl_size_add(uint32_t* __restrict__ size, uint32_t label, bool mine, uint32_t n)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t todo = __ballot(mine); todo; ) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t l = __shfl(label, leader);
        const uint64_t same = __ballot(mine && label == l);
        if (lane == leader) {
            GSR_BOUND(clusters, 4, l, n);
            if (l < n) __hip_atomic_fetch_add(&size[l], (uint32_t)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (label == l) mine = false;
        todo &= ~same;
    }
}

// ---- seed ----
__global__ __launch_bounds__(NB_THREADS) void k_cl_seed(NbIndex ix, uint32_t m /* entries */, uint32_t n /* splats */, const uint32_t* __restrict__ counts,
                                                        uint32_t min_pts, ClArrays a)
{
    uint32_t core = 0u;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS, end = ((uint64_t)m + 63u) & ~63ull;   // whole waves step together
    for (uint64_t s = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < end; s += stride) {
        bool is_core = false;
        if (s < m) {
            GSR_BOUND(clusters, 1, s, m);
            const uint32_t i = ix.entry[s].w;
            is_core = cl_core(counts, i, n, min_pts);
            GSR_BOUND(clusters, 3, i, n);
            if (is_core) a.label[i] = i;
        }
        core += (uint32_t)__popcll(__ballot(is_core));
    }
    if ((threadIdx.x & 63u) == 0u && core) __hip_atomic_fetch_add(&a.info->core, core, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- union ----
__global__ __launch_bounds__(NB_THREADS) void k_cl_union(NbIndex ix, uint32_t m, uint32_t n, const uint32_t* __restrict__ counts, uint32_t min_pts, ClArrays a)
{
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < m; s += stride) {
        GSR_BOUND(clusters, 1, s, m);
        const uint4 me = ix.entry[s];
        const uint32_t i = me.w;
        if (!cl_core(counts, i, n, min_pts)) continue;
        uint32_t at = i;   // a node of i's tree, at or near its root
        nb_each_near<cl_sites>(ix, m, (uint32_t)s, me, [&](uint32_t j) { return j < i; }, [&](uint32_t j) {
            if (cl_core(counts, j, n, min_pts)) at = cl_unite(a.label, at, j, n, a.info);
            return true;
        });
    }
}

// ---- flatten ----
__global__ __launch_bounds__(NB_THREADS) void k_cl_flatten(NbIndex ix, uint32_t m, uint32_t n, const uint32_t* __restrict__ counts, uint32_t min_pts, ClArrays a)
{
    uint32_t roots = 0u;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS, end = ((uint64_t)m + 63u) & ~63ull;
    for (uint64_t s = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < end; s += stride) {
        uint32_t label = CL_NONE;
        bool labelled = false;
        if (s < m) {
            GSR_BOUND(clusters, 1, s, m);
            const uint32_t i = ix.entry[s].w;
            if (cl_core(counts, i, n, min_pts)) {
                label = cl_find<false>(a.label, i, n, a.info);
                labelled = label != CL_NONE;
                if (labelled) cl_store(&a.label[i], label);   // (i < n: cl_find took it; the root of i, an ancestor)
                roots += (uint32_t)(label == i);
            }
        }
        cl_size_add(a.size, label, labelled, n);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) roots += __shfl_xor(roots, d);
    if ((threadIdx.x & 63u) == 0u && roots) __hip_atomic_fetch_add(&a.info->clusters, roots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- border ----
__global__ __launch_bounds__(NB_THREADS) void k_cl_border(NbIndex ix, uint32_t m, uint32_t n, const uint32_t* __restrict__ counts, uint32_t min_pts, ClArrays a)
{
    uint32_t border = 0u;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS, end = ((uint64_t)m + 63u) & ~63ull;
    for (uint64_t s = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < end; s += stride) {
        uint32_t label = CL_NONE, i = CL_NONE;
        if (s < m) {
            GSR_BOUND(clusters, 1, s, m);
            const uint4 me = ix.entry[s];
            i = me.w;
            if (i < n && !cl_core(counts, i, n, min_pts)) {
                nb_each_near<cl_sites>(ix, m, (uint32_t)s, me, [&](uint32_t) { return true; }, [&](uint32_t j) {
                    if (cl_core(counts, j, n, min_pts)) label = min(label, a.label[j]);   // (a core entry's word: final, not written here)
                    return true;
                });
            }
        }
        const bool labelled = label != CL_NONE;
        GSR_BOUND(clusters, 3, labelled ? i : 0u, n);
        if (labelled) a.label[i] = label;                     // (a non-core entry's word: nobody reads it here)
        border += (uint32_t)__popcll(__ballot(labelled));
        cl_size_add(a.size, label, labelled, n);
    }
    if ((threadIdx.x & 63u) == 0u && border) __hip_atomic_fetch_add(&a.info->border, border, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- sizes ----
// One lane per splat.  A root (label[i] == i) offers size << 32 | ~i to the maximum: the greatest size, then the smallest label.
__global__ __launch_bounds__(NB_THREADS) void k_cl_sizes(uint32_t n, ClArrays a)
{
    unsigned long long best = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t label = a.label[i];
        uint32_t size = 0u;
        if (label != CL_NONE) {
            GSR_BOUND(clusters, 4, label, n);
            if (label < n) size = a.size[label];
        }
        a.sizes[i] = size;
        if (label == (uint32_t)i) best = max(best, (unsigned long long)size << 32 | (uint32_t)~label);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, d));
    if ((threadIdx.x & 63u) == 0u && best) __hip_atomic_fetch_max(&a.info->largest, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the pickers ----
// One thread per bit of the mask; a wave's ballot is two whole words (mask_store_ballot): every word of the mask is stored.
// gsr_select_clusters: in scope and lo <= size < hi (noise and non-finite splats in scope have size 0)
__global__ __launch_bounds__(NB_THREADS) void k_cl_select_sizes(const uint32_t* __restrict__ sizes, AttrScope sc, uint32_t n, uint32_t lo, uint32_t hi,
                                                                uint32_t* __restrict__ scratch, uint32_t nwords)
{
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    bool in = false;
    if (in_scope<cl_sites>(sc, n, i)) {
        GSR_BOUND(clusters, 7, i, n);
        const uint32_t c = sizes[i];
        in = lo <= c && c < hi;
    }
    mask_store_ballot<cl_sites>(scratch, nwords, i, __ballot(in));
}

// gsr_select_cluster_at: label == target (a labelled splat is in scope; CL_NONE picks nobody)
__global__ __launch_bounds__(NB_THREADS) void k_cl_select_label(const uint32_t* __restrict__ label, uint32_t n, uint32_t target, uint32_t* __restrict__ scratch,
                                                                uint32_t nwords)
{
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    bool in = false;
    if (i < n && target != CL_NONE) {
        GSR_BOUND(clusters, 7, i, n);
        in = label[i] == target;
    }
    mask_store_ballot<cl_sites>(scratch, nwords, i, __ballot(in));
}

// ---- launchers ----
void launch_cl_seed(const NbIndex& ix, uint32_t indexed, uint32_t n, const uint32_t* counts, uint32_t min_pts, const ClArrays& a, int cu_count, hipStream_t s)
{
    if (!indexed) return;
    hipLaunchKernelGGL(k_cl_seed, dim3(nb_grid(indexed, cu_count)), dim3(NB_THREADS), 0, s, ix, indexed, n, counts, min_pts, a);
}

void launch_cl_union(const NbIndex& ix, uint32_t indexed, uint32_t n, const uint32_t* counts, uint32_t min_pts, const ClArrays& a, int cu_count, hipStream_t s)
{
    if (!indexed) return;
    const uint32_t blocks = nb_grid(indexed, cu_count);
    hipLaunchKernelGGL(k_cl_union, dim3(blocks), dim3(NB_THREADS), 0, s, ix, indexed, n, counts, min_pts, a);
    hipLaunchKernelGGL(k_cl_flatten, dim3(blocks), dim3(NB_THREADS), 0, s, ix, indexed, n, counts, min_pts, a);
}

void launch_cl_border(const NbIndex& ix, uint32_t indexed, uint32_t n, const uint32_t* counts, uint32_t min_pts, const ClArrays& a, int cu_count, hipStream_t s)
{
    if (!indexed) return;
    hipLaunchKernelGGL(k_cl_border, dim3(nb_grid(indexed, cu_count)), dim3(NB_THREADS), 0, s, ix, indexed, n, counts, min_pts, a);
}

void launch_cl_sizes(uint32_t n, const ClArrays& a, int cu_count, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_cl_sizes, dim3(nb_grid(n, cu_count)), dim3(NB_THREADS), 0, s, n, a);
}

void launch_cl_select_sizes(const uint32_t* sizes, const AttrScope& sc, uint32_t n, uint32_t lo, uint32_t hi, uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_cl_select_sizes, dim3(mask_blocks(nwords, NB_THREADS)), dim3(NB_THREADS), 0, s, sizes, sc, n, lo, hi, scratch, nwords);
}

void launch_cl_select_label(const uint32_t* label, uint32_t n, uint32_t target, uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_cl_select_label, dim3(mask_blocks(nwords, NB_THREADS)), dim3(NB_THREADS), 0, s, label, n, target, scratch, nwords);
}

}  // namespace gsr
