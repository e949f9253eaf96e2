// k nearest neighbours: for every splat in scope the k nearest others in scope within a radius -- indices and squared distances
// in a defined order, how many were found, one value per splat (the distance to the k-th, or the mean distance to those found),
// the histogram of the lists' lengths -- and the splats whose value lies in a range as a picker, which is what statistical
// outlier removal needs (include/gsplat_hip.h, "k nearest neighbours"; kernels: k_knn.hip over k_neighbours.hip's index).
// Both calls are blocking, stateless and ordered like gsr_select_attr: they wait for every member's stream of a shared scene first,
// index the scene as it is now, read it and write none of it; gsr_select_knn changes the selection the way every picker does.
// The scratch is the context's neighbour scratch (gsr_neighbours.cpp), 12 bytes per splat of its own for found and values, and
// 12 bytes per splat and k for the lists of a call that asks for them; the first call allocates it, it only grows, the context's
// end frees it.  A context that never calls these allocates and launches nothing.
//
// The work budget is the neighbour budget: nb_index builds the index, sums what the one 27-cell walk tests at most and refuses a
// call above its budget before the walk is launched.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace gsr;

namespace {

constexpr uint32_t KNN_INFO_WORDS = 8;
static_assert(sizeof(KnnInfo) <= KNN_INFO_WORDS * 4, "KnnInfo fits its words");
static_assert(KNN_MAX_K == GSR_KNN_MAX_K && KNN_NONE == GSR_KNN_NONE && KNN_KTH == GSR_KNN_KTH && KNN_MEAN == GSR_KNN_MEAN, "the header's words");
static_assert(KNN_MAX_K <= NB_MAX_CAP, "the neighbour scratch holds the histogram");
static_assert(sizeof(gsr_knn_info) == 48, "the header's layout");
constexpr double INF = std::numeric_limits<double>::infinity();

int knn_check(gsr_ctx* c, const char* who, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat)
{
    if (int r = nb_check(c, who, radius, k, scope, budget, 1u, "k", GSR_KNN_MAX_K)) return r;
    if (stat != GSR_KNN_KTH && stat != GSR_KNN_MEAN) return fail(c, GSR_ERR_ARG, "%s: unknown stat %d", who, stat);
    return GSR_OK;
}

// the context's scratch for n splats, with lists of k slots each when `lists`: allocated by the first call, only ever grown
int knn_ensure(gsr_ctx* c, uint32_t n, uint32_t k, bool lists)
{
    gsr_ctx::Knn& kn = c->knn;
    if (!kn.words) { if (int r = kn.words.alloc(c, KNN_INFO_WORDS)) return r; }
    if (kn.rows < n || !kn.found) {
        kn.rows = 0;
        int r;
        if ((r = kn.found.alloc(c, n)) || (r = kn.values.alloc(c, n))) return r;
        kn.rows = n;
    }
    const uint64_t slots = (uint64_t)n * k;
    if (lists && (kn.slots < slots || !kn.idx)) {
        kn.slots = 0;
        int r;
        if ((r = kn.idx.alloc(c, slots)) || (r = kn.d2.alloc(c, slots))) return r;
        kn.slots = slots;
    }
    if (!kn.ev) HIP_TRY(c, hipEventCreate(&kn.ev));
    return GSR_OK;
}

gsr_knn_info knn_zero_info(uint64_t budget)
{
    gsr_knn_info z{};
    z.budget = budget;
    z.value_min = INF;
    z.value_max = -INF;
    return z;
}

struct KnnCall {
    NbCall nb;
    KnnArrays a;
};

// Everything up to the read-backs: the index and its bound (nb_index), the fill, the walk and *info, final on the device and
// waited for.  GSR_ERR_ARG (with *info's first four fields filled) for a bound above the budget: no walk has been launched.
// n >= 1; the device is current and no member's stream holds work.
int knn_run(gsr_ctx* c, const char* who, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat, bool lists, KnnCall* call, gsr_knn_info* info)
{
    const uint32_t n = c->scene->n;
    if (int r = knn_ensure(c, n, k, lists)) return r;
    gsr_neighbour_info ni{0u, 0u, 0ull, budget};
    const int r = nb_index(c, who, radius, k, scope, budget, true, &call->nb, &ni);
    info->in_scope = ni.in_scope; info->nonfinite = ni.nonfinite; info->pair_bound = ni.pair_bound; info->budget = ni.budget;
    if (r) return r;
    gsr_ctx::Neighbours& nb = c->nb;
    gsr_ctx::Knn& kn = c->knn;
    const NbCall& b = call->nb;
    const KnnArrays a{kn.found, kn.values, lists ? kn.idx.p : nullptr, lists ? kn.d2.p : nullptr, reinterpret_cast<KnnInfo*>(kn.words.p)};
    call->a = a;
    HIP_TRY(c, hipMemsetAsync(kn.words, 0, KNN_INFO_WORDS * 4, c->stream));
    launch_knn_fill(b.sc, n, k, a, c->cu_count, c->stream);
    launch_knn(b.ix, b.indexed, n, k, stat, a, b.hist, c->cu_count, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(kn.ev, c->stream);
    KnnInfo got{};
    hipError_t e2 = hipMemcpyAsync(&got, a.info, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    if (got.complete > b.indexed || got.finite_values > b.indexed)
        return fail(c, GSR_ERR_HIP, "%s: %u complete lists and %u finite values of %u indexed", who, got.complete, got.finite_values, b.indexed);
    info->complete = got.complete; info->finite_values = got.finite_values;
    if (got.finite_values) {
        const uint64_t lo = ~(uint64_t)got.nvmin, hi = (uint64_t)got.vmax;
        std::memcpy(&info->value_min, &lo, 8);
        std::memcpy(&info->value_max, &hi, 8);
    }
    float ms[2] = {0.0f, 0.0f};
    if (hipEventElapsedTime(&ms[0], nb.ev[0], nb.ev[1]) == hipSuccess && hipEventElapsedTime(&ms[1], nb.ev[1], kn.ev) == hipSuccess) std::memcpy(kn.ms, ms, sizeof ms);
    else (void)hipGetLastError();
    return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_knn(gsr_ctx* c, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat, uint32_t* found, uint32_t* idx, double* d2, double* values,
            uint32_t n, uint32_t* hist, gsr_knn_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = knn_check(c, "gsr_knn", radius, k, scope, budget, stat)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    if ((found || idx || d2 || values) && n != sc.n) return fail(c, GSR_ERR_ARG, "gsr_knn: n (%u) is not the scene's count (%u)", n, sc.n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    gsr_knn_info got = knn_zero_info(budget);
    if (!sc.n) {
        if (hist) std::memset(hist, 0, (size_t)(k + 1u) * 4);
        if (info) *info = got;
        return GSR_OK;
    }
    KnnCall call;
    const int r = knn_run(c, "gsr_knn", radius, k, scope, budget, stat, idx || d2, &call, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    const size_t rows = sc.n, slots = (size_t)sc.n * k;
    hipError_t e0 = found ? hipMemcpyAsync(found, call.a.found, rows * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e1 = values ? hipMemcpyAsync(values, call.a.values, rows * 8, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e2 = idx ? hipMemcpyAsync(idx, call.a.idx, slots * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e3 = d2 ? hipMemcpyAsync(d2, call.a.d2, slots * 8, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e4 = hist ? hipMemcpyAsync(hist, call.nb.hist, (size_t)(k + 1u) * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e5 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, e4, e5})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_knn failed: %s", hipGetErrorString(e));
    return GSR_OK;
}

int gsr_select_knn(gsr_ctx* c, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat, double lo, double hi, int32_t op, uint32_t* selected,
                   gsr_knn_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = knn_check(c, "gsr_select_knn", radius, k, scope, budget, stat)) return r;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_knn: unknown op %d", op);
    if (std::isnan(lo) || std::isnan(hi) || lo > hi) return fail(c, GSR_ERR_ARG, "gsr_select_knn: [%g, %g) must satisfy lo <= hi, neither a NaN", lo, hi);
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    SharedScene& sc = *c->scene;
    gsr_knn_info got = knn_zero_info(budget);
    if (!sc.n) {
        if (selected) *selected = 0;
        if (info) *info = got;
        return GSR_OK;
    }
    if (int r = select_ensure(c)) return r;   // (in front of the scope: a selection never allocated becomes the zeroed mask, the same set)
    KnnCall call;
    const int r = knn_run(c, "gsr_select_knn", radius, k, scope, budget, stat, false, &call, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    launch_knn_select(call.a.values, call.nb.sc, sc.n, lo, hi, hi == INF, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

// (index_ms, walk_ms) of the context's last call: the index with its bound, and the fill with the walk, between events on the
// stream.  Not part of the ABI (tools/bench_cabi.cpp --knn).
int gsr_debug_knn_times(gsr_ctx* c, float* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    std::memcpy(out, c->knn.ms, sizeof c->knn.ms);
    return GSR_OK;
}

// the bytes of device scratch the context holds for these calls beside the neighbour scratch: 0 until the first call.  Not part
// of the ABI (tests/test_gpu_knn.py).
int gsr_debug_knn_scratch(gsr_ctx* c, uint64_t* bytes)
{
    if (!c || !bytes) return GSR_ERR_ARG;
    const gsr_ctx::Knn& kn = c->knn;
    *bytes = (kn.words ? KNN_INFO_WORDS * 4ull : 0ull) + (uint64_t)kn.rows * 12u + kn.slots * 12u;
    return GSR_OK;
}

}  // extern "C"
