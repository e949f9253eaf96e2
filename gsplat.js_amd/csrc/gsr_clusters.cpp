// Clusters: the connected islands of the splats in scope at a linking radius -- every splat's label and its cluster's size, the
// islands of a size range as a picker, and the island of one splat or the largest one as a picker (include/gsplat_hip.h,
// "clusters"; kernels: k_clusters.hip over k_neighbours.hip's index).  The calls are blocking, stateless and ordered like
// gsr_select_attr: they wait for every member's stream of a shared scene first, index the scene as it is now, read it and write
// none of it; the two pickers change the selection the way every picker does.  The scratch is the context's neighbour scratch
// (gsr_neighbours.cpp) and three words per splat of its own -- parent / label, size by label, size by splat; the first cluster
// call allocates them, they only grow, the context's end frees them.  A context that never calls these allocates and launches nothing.
//
// The work budget is the neighbour budget: nb_index builds the index, sums what ONE 27-cell walk tests at most and refuses a call
// above its budget before any walk is launched.  A call makes up to three such walks (core test, union, border).
#include "gsr_ctx.h"

#include <cstring>

using namespace gsr;

namespace {

static_assert(sizeof(ClInfo) <= CL_INFO_WORDS * 4, "ClInfo fits its words");
static_assert(CL_NONE == GSR_CLUSTER_NONE && CL_NONE == GSR_CLUSTER_LARGEST, "the header's words");
static_assert(sizeof(gsr_cluster_info) == 48, "the header's layout");

struct ClCall {
    NbCall nb;
    ClArrays a;
};

int cl_check(gsr_ctx* c, const char* who, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget)
{
    return nb_check(c, who, radius, min_pts, scope, budget, 0u, "min_pts");
}

int cl_ensure(gsr_ctx* c, uint32_t n)
{
    gsr_ctx::Clusters& cl = c->cl;
    if (!cl.words) { if (int r = cl.words.alloc(c, CL_INFO_WORDS)) return r; }
    if (cl.rows < n || !cl.label) {
        cl.rows = 0;
        int r;
        if ((r = cl.label.alloc(c, n)) || (r = cl.size.alloc(c, n)) || (r = cl.sizes.alloc(c, n))) return r;
        cl.rows = n;
    }
    for (hipEvent_t& e : cl.ev) if (!e) HIP_TRY(c, hipEventCreate(&e));
    return GSR_OK;
}

gsr_cluster_info cl_zero_info(uint64_t budget)
{
    gsr_cluster_info z{};
    z.budget = budget;
    z.largest_label = GSR_CLUSTER_NONE;
    return z;
}

// Everything up to the pick: the index and its bound (nb_index), then the walks, labels, sizes and *info, final on the device and
// waited for.  GSR_ERR_ARG (with *info's first four fields filled) for a bound above the budget: no walk has been launched.
// n >= 1; the device is current and no member's stream holds work.
int cl_run(gsr_ctx* c, const char* who, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, ClCall* call, gsr_cluster_info* info)
{
    const uint32_t n = c->scene->n;
    if (int r = cl_ensure(c, n)) return r;
    gsr_neighbour_info ni{0u, 0u, 0ull, budget};
    const int r = nb_index(c, who, radius, min_pts, scope, budget, false, &call->nb, &ni);
    info->in_scope = ni.in_scope; info->nonfinite = ni.nonfinite; info->pair_bound = ni.pair_bound; info->budget = ni.budget;
    if (r) return r;
    gsr_ctx::Neighbours& nb = c->nb;
    gsr_ctx::Clusters& cl = c->cl;
    const NbCall& k = call->nb;
    const ClArrays a{cl.label, cl.size, cl.sizes, reinterpret_cast<ClInfo*>(cl.words.p)};
    call->a = a;
    HIP_TRY(c, hipMemsetAsync(cl.words, 0, CL_INFO_WORDS * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(cl.label, 0xff, (size_t)n * 4, c->stream));   // CL_NONE
    HIP_TRY(c, hipMemsetAsync(cl.size, 0, (size_t)n * 4, c->stream));
    // core: counts[i] = min(min_pts, deg_i); for min_pts == 0 nb_index's zeros say "core" of every entry
    if (min_pts) launch_nb_count(k.ix, k.indexed, k.n, min_pts, nb.counts, nullptr, c->cu_count, c->stream);
    launch_cl_seed(k.ix, k.indexed, k.n, nb.counts, min_pts, a, c->cu_count, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(cl.ev[0], c->stream);
    launch_cl_union(k.ix, k.indexed, k.n, nb.counts, min_pts, a, c->cu_count, c->stream);
    hipError_t e2 = hipGetLastError();
    hipError_t e3 = hipEventRecord(cl.ev[1], c->stream);
    if (min_pts) launch_cl_border(k.ix, k.indexed, k.n, nb.counts, min_pts, a, c->cu_count, c->stream);   // (min_pts == 0: no entry is non-core)
    launch_cl_sizes(k.n, a, c->cu_count, c->stream);
    hipError_t e4 = hipGetLastError();
    hipError_t e5 = hipEventRecord(cl.ev[2], c->stream);
    ClInfo got{};
    hipError_t e6 = hipMemcpyAsync(&got, a.info, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e7 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, e4, e5, e6, e7, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    if (got.fault)
        return fail(c, GSR_ERR_HIP, "%s: the union met an inconsistent parent word or ran into its step limit (%u splats)", who, n);
    if ((uint64_t)got.core + got.border > k.indexed)
        return fail(c, GSR_ERR_HIP, "%s: %u core and %u border splats of %u indexed", who, got.core, got.border, k.indexed);
    info->core = got.core; info->border = got.border; info->noise = ni.in_scope - got.core - got.border; info->clusters = got.clusters;
    info->largest_label = got.largest ? ~(uint32_t)got.largest : GSR_CLUSTER_NONE;
    info->largest_size = (uint32_t)(got.largest >> 32);
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (hipEventElapsedTime(&ms[0], nb.ev[0], nb.ev[1]) == hipSuccess && hipEventElapsedTime(&ms[1], nb.ev[1], cl.ev[0]) == hipSuccess &&
        hipEventElapsedTime(&ms[2], cl.ev[0], cl.ev[1]) == hipSuccess && hipEventElapsedTime(&ms[3], cl.ev[1], cl.ev[2]) == hipSuccess)
        std::memcpy(cl.ms, ms, sizeof ms);
    else (void)hipGetLastError();
    return GSR_OK;
}

// what the two pickers share in front of their pick: refusals are the caller's; *proceed false: an empty scene, zeros returned
int cl_select_begin(gsr_ctx* c, const char* who, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, uint32_t* selected, gsr_cluster_info* info,
                    ClCall* call, gsr_cluster_info* got, bool* proceed)
{
    *proceed = false;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    *got = cl_zero_info(budget);
    if (!c->scene->n) {
        if (selected) *selected = 0;
        if (info) *info = *got;
        return GSR_OK;
    }
    if (int r = select_ensure(c)) return r;   // (in front of the scope: a selection never allocated becomes the zeroed mask, the same set)
    const int r = cl_run(c, who, radius, min_pts, scope, budget, call, got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = *got;
    *proceed = r == GSR_OK;
    return r;
}

}  // namespace

extern "C" {

int gsr_clusters(gsr_ctx* c, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, uint32_t* labels, uint32_t* sizes, uint32_t n,
                 gsr_cluster_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = cl_check(c, "gsr_clusters", radius, min_pts, scope, budget)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    if ((labels || sizes) && n != sc.n) return fail(c, GSR_ERR_ARG, "gsr_clusters: n (%u) is not the scene's count (%u)", n, sc.n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    gsr_cluster_info got = cl_zero_info(budget);
    if (!sc.n) {
        if (info) *info = got;
        return GSR_OK;
    }
    ClCall k;
    const int r = cl_run(c, "gsr_clusters", radius, min_pts, scope, budget, &k, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    hipError_t e0 = labels ? hipMemcpyAsync(labels, k.a.label, (size_t)sc.n * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e1 = sizes ? hipMemcpyAsync(sizes, k.a.sizes, (size_t)sc.n * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e2 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_clusters failed: %s", hipGetErrorString(e));
    return GSR_OK;
}

int gsr_select_clusters(gsr_ctx* c, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, uint32_t size_lo, uint32_t size_hi, int32_t op,
                        uint32_t* selected, gsr_cluster_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = cl_check(c, "gsr_select_clusters", radius, min_pts, scope, budget)) return r;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_clusters: unknown op %d", op);
    if (size_lo > size_hi) return fail(c, GSR_ERR_ARG, "gsr_select_clusters: [%u, %u) must satisfy size_lo <= size_hi", size_lo, size_hi);
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    ClCall k;
    gsr_cluster_info got;
    bool proceed;
    if (int r = cl_select_begin(c, "gsr_select_clusters", radius, min_pts, scope, budget, selected, info, &k, &got, &proceed)) return r;
    if (!proceed) return GSR_OK;
    SharedScene& sc = *c->scene;
    launch_cl_select_sizes(k.a.sizes, k.nb.sc, sc.n, size_lo, size_hi, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

int gsr_select_cluster_at(gsr_ctx* c, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, uint32_t seed, int32_t op, uint32_t* selected,
                          gsr_cluster_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = cl_check(c, "gsr_select_cluster_at", radius, min_pts, scope, budget)) return r;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_cluster_at: unknown op %d", op);
    if (seed != GSR_CLUSTER_LARGEST && seed >= c->scene->n)
        return fail(c, GSR_ERR_ARG, "gsr_select_cluster_at: seed (%u) must be a splat index below %u or GSR_CLUSTER_LARGEST", seed, c->scene->n);
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    ClCall k;
    gsr_cluster_info got;
    bool proceed;
    if (int r = cl_select_begin(c, "gsr_select_cluster_at", radius, min_pts, scope, budget, selected, info, &k, &got, &proceed)) return r;
    if (!proceed) return GSR_OK;
    SharedScene& sc = *c->scene;
    uint32_t target = got.largest_label;   // GSR_CLUSTER_NONE without a cluster: the empty set
    if (seed != GSR_CLUSTER_LARGEST) {     // the seed's label: GSR_CLUSTER_NONE for noise and out of scope
        HIP_TRY(c, hipMemcpyAsync(&target, k.a.label + seed, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    launch_cl_select_label(k.a.label, sc.n, target, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

// (index_ms, core_ms, union_ms, border_ms) of the context's last cluster call: the index with its bound, the core test with the
// seed, union with flatten, border with sizes, between events on the stream.  Not part of the ABI (tools/bench_cabi.cpp --clusters).
int gsr_debug_cluster_times(gsr_ctx* c, float* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    std::memcpy(out, c->cl.ms, sizeof c->cl.ms);
    return GSR_OK;
}

}  // extern "C"
