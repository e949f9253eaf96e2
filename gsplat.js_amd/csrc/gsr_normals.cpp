// Normals: for every splat in scope a unit surface normal, the surface variation and the length of the list it came from -- by
// the PCA of the k nearest neighbours within a radius, or from the splat's own shortest axis -- and the splats whose n . axis,
// |n . axis| or variation lies in a closed range as a picker (include/gsplat_hip.h, "normals"; kernels: k_normals.hip over
// k_neighbours.hip's index).  Both calls are blocking, stateless and ordered like gsr_knn: they wait for every member's stream of
// a shared scene first, index the scene as it is now, read it and write none of it; gsr_select_normal changes the selection the
// way every picker does.  The scratch is the context's neighbour scratch (gsr_neighbours.cpp, KNN source only) and 12 + 8 + 4
// bytes per splat of its own for normals, variation and found; the first call allocates it, it only grows, the context's end
// frees it.  A context that never calls these allocates and launches nothing.
//
// The work budget of the KNN source is the neighbour budget: nb_index builds the index, sums what the one 27-cell walk tests at
// most and refuses a call above its budget before the walk is launched.  The OWN source walks nothing: pair_bound 0.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace gsr;

namespace {

constexpr uint32_t NORMAL_INFO_WORDS = 8;
static_assert(sizeof(NormalInfo) == NORMAL_INFO_WORDS * 4, "NormalInfo fills its words");
static_assert(NORMAL_KNN == GSR_NORMAL_KNN && NORMAL_OWN == GSR_NORMAL_OWN && NORMAL_DOT == GSR_NORMAL_DOT && NORMAL_ABS_DOT == GSR_NORMAL_ABS_DOT &&
              NORMAL_VARIATION == GSR_NORMAL_VARIATION, "the header's words");
static_assert(sizeof(gsr_normal_options) == 56 && sizeof(gsr_normal_info) == 48, "the header's layout");
constexpr double INF = std::numeric_limits<double>::infinity();

// the context's scratch for n splats: allocated by the first call, only ever grown
int normal_ensure(gsr_ctx* c, uint32_t n)
{
    gsr_ctx::Normals& nm = c->nm;
    if (!nm.words) { if (int r = nm.words.alloc(c, NORMAL_INFO_WORDS)) return r; }
    if (nm.rows < n || !nm.found) {
        nm.rows = 0;
        int r;
        if ((r = nm.normals.alloc(c, (size_t)n * 3u)) || (r = nm.variation.alloc(c, n)) || (r = nm.found.alloc(c, n))) return r;
        nm.rows = n;
    }
    for (hipEvent_t& e : nm.ev) if (!e) HIP_TRY(c, hipEventCreate(&e));
    return GSR_OK;
}

gsr_normal_info normal_zero_info(uint64_t budget)
{
    gsr_normal_info z{};
    z.budget = budget;
    z.variation_min = INF;
    z.variation_max = -INF;
    return z;
}

}  // namespace

namespace gsr {

// the refusals the two calls share, in the header's order.  Nothing is touched by a refused call.
int normal_check(gsr_ctx* c, const char* who, const gsr_normal_options* o)
{
    if (!o) return fail(c, GSR_ERR_ARG, "%s: options is NULL", who);
    if (o->source != GSR_NORMAL_KNN && o->source != GSR_NORMAL_OWN) return fail(c, GSR_ERR_ARG, "%s: unknown source %d", who, o->source);
    if (o->source == GSR_NORMAL_KNN) {
        if (int r = nb_check(c, who, o->radius, o->k, o->scope, o->budget, NORMAL_MIN_K, "k", GSR_KNN_MAX_K)) return r;
    } else if (int r = scope_check(c, who, o->scope, o->budget)) {
        return r;
    }
    if (o->oriented)
        for (int j = 0; j < 3; j++)
            if (!std::isfinite(o->toward[j])) return fail(c, GSR_ERR_ARG, "%s: toward[%d] is %g: it must be finite", who, j, o->toward[j]);
    return GSR_OK;
}

// Everything up to the read-backs: (KNN) the index and its bound (nb_index), the fill and the walk, or (OWN) the one kernel; *info,
// final on the device and waited for.  GSR_ERR_ARG (with *info's first four fields filled) for a bound above the budget: no walk
// has been launched.  n >= 1; the device is current and no member's stream holds work.
int normal_run(gsr_ctx* c, const char* who, const gsr_normal_options* o, uint64_t budget, NormalArrays* arrays, gsr_normal_info* info)
{
    SharedScene& sc = *c->scene;
    const uint32_t n = sc.n;
    if (int r = normal_ensure(c, n)) return r;
    gsr_ctx::Normals& nm = c->nm;
    const NormalArrays a{nm.normals, nm.variation, nm.found, reinterpret_cast<NormalInfo*>(nm.words.p)};
    *arrays = a;
    const NormalOrient orient{o->oriented ? 1u : 0u, o->oriented ? o->toward[0] : 0.0, o->oriented ? o->toward[1] : 0.0, o->oriented ? o->toward[2] : 0.0};
    const bool knn = o->source == GSR_NORMAL_KNN;
    uint32_t rows_most = n;
    if (knn) {
        NbCall call;
        gsr_neighbour_info ni{0u, 0u, 0ull, budget};
        const int r = nb_index(c, who, o->radius, o->k, o->scope, budget, false, &call, &ni);
        info->in_scope = ni.in_scope; info->nonfinite = ni.nonfinite; info->pair_bound = ni.pair_bound; info->budget = ni.budget;
        if (r) return r;
        rows_most = call.indexed;
        HIP_TRY(c, hipMemsetAsync(nm.words, 0, NORMAL_INFO_WORDS * 4, c->stream));
        launch_normals_fill(n, a, c->cu_count, c->stream);
        launch_normals_knn(call.ix, call.indexed, n, o->k, sc.arr.px, sc.arr.py, sc.arr.pz, orient, a, c->cu_count, c->stream);
    } else {
        HIP_TRY(c, hipMemsetAsync(nm.words, 0, NORMAL_INFO_WORDS * 4, c->stream));
        HIP_TRY(c, hipEventRecord(nm.ev[0], c->stream));
        launch_normals_own(sc.arr.view(), scene_scope(sc, o->scope), n, orient, a, c->cu_count, c->stream);
    }
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(nm.ev[1], c->stream);
    NormalInfo got{};
    hipError_t e2 = hipMemcpyAsync(&got, a.info, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    if (!knn) {
        info->in_scope = got.in_scope; info->nonfinite = got.nonfinite; info->pair_bound = 0; info->budget = budget;
        if (got.in_scope > n || got.nonfinite > got.in_scope) return fail(c, GSR_ERR_HIP, "%s: %u splats in scope, %u of them non-finite, of %u", who, got.in_scope, got.nonfinite, n);
        rows_most = got.in_scope;
    }
    if (got.valid > rows_most) return fail(c, GSR_ERR_HIP, "%s: %u valid rows of %u", who, got.valid, rows_most);
    info->valid = got.valid;
    if (got.valid) {
        const uint64_t lo = ~(uint64_t)got.nvmin, hi = (uint64_t)got.vmax;
        std::memcpy(&info->variation_min, &lo, 8);
        std::memcpy(&info->variation_max, &hi, 8);
    }
    float ms[2] = {0.0f, 0.0f};
    const bool timed = knn ? hipEventElapsedTime(&ms[0], c->nb.ev[0], c->nb.ev[1]) == hipSuccess && hipEventElapsedTime(&ms[1], c->nb.ev[1], nm.ev[1]) == hipSuccess
                           : hipEventElapsedTime(&ms[1], nm.ev[0], nm.ev[1]) == hipSuccess;
    if (timed) std::memcpy(nm.ms, ms, sizeof ms);
    else (void)hipGetLastError();
    return GSR_OK;
}

}  // namespace gsr

extern "C" {

int gsr_normals(gsr_ctx* c, const gsr_normal_options* o, float* normals, double* variation, uint32_t* found, uint32_t n, gsr_normal_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = normal_check(c, "gsr_normals", o)) return r;
    const uint64_t budget = o->budget ? o->budget : GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    if ((normals || variation || found) && n != sc.n) return fail(c, GSR_ERR_ARG, "gsr_normals: n (%u) is not the scene's count (%u)", n, sc.n);
    if (o->source == GSR_NORMAL_OWN && sc.n)
        if (int r = require_rows(c)) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    gsr_normal_info got = normal_zero_info(budget);
    if (!sc.n) {
        if (info) *info = got;
        return GSR_OK;
    }
    NormalArrays a;
    const int r = normal_run(c, "gsr_normals", o, budget, &a, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    const size_t rows = sc.n;
    hipError_t e0 = normals ? hipMemcpyAsync(normals, a.normals, rows * 12, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e1 = variation ? hipMemcpyAsync(variation, a.variation, rows * 8, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e2 = found ? hipMemcpyAsync(found, a.found, rows * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_normals failed: %s", hipGetErrorString(e));
    return GSR_OK;
}

int gsr_select_normal(gsr_ctx* c, const gsr_normal_options* o, int32_t stat, const double* axis, double lo, double hi, int32_t op, uint32_t* selected,
                      gsr_normal_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (!o) return fail(c, GSR_ERR_ARG, "gsr_select_normal: options is NULL");
    if (o->source != GSR_NORMAL_KNN && o->source != GSR_NORMAL_OWN) return fail(c, GSR_ERR_ARG, "gsr_select_normal: unknown source %d", o->source);
    if (stat != GSR_NORMAL_DOT && stat != GSR_NORMAL_ABS_DOT && stat != GSR_NORMAL_VARIATION) return fail(c, GSR_ERR_ARG, "gsr_select_normal: unknown stat %d", stat);
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_normal: unknown op %d", op);
    if (int r = normal_check(c, "gsr_select_normal", o)) return r;
    if (stat != GSR_NORMAL_VARIATION) {
        if (!axis) return fail(c, GSR_ERR_ARG, "gsr_select_normal: axis is NULL");
        for (int j = 0; j < 3; j++)
            if (!std::isfinite(axis[j])) return fail(c, GSR_ERR_ARG, "gsr_select_normal: axis[%d] is %g: it must be finite", j, axis[j]);
        if (axis[0] == 0.0 && axis[1] == 0.0 && axis[2] == 0.0) return fail(c, GSR_ERR_ARG, "gsr_select_normal: the axis is zero");
    }
    if (std::isnan(lo) || std::isnan(hi)) return fail(c, GSR_ERR_ARG, "gsr_select_normal: a bound is NaN");
    if (lo > hi) return fail(c, GSR_ERR_ARG, "gsr_select_normal: lo (%g) is above hi (%g)", lo, hi);
    const uint64_t budget = o->budget ? o->budget : GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    if (o->source == GSR_NORMAL_OWN && sc.n)
        if (int r = require_rows(c)) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    gsr_normal_info got = normal_zero_info(budget);
    if (!sc.n) {
        if (selected) *selected = 0;
        if (info) *info = got;
        return GSR_OK;
    }
    if (int r = select_ensure(c)) return r;   // (in front of the scope: a selection never allocated becomes the zeroed mask, the same set)
    NormalArrays a;
    const int r = normal_run(c, "gsr_select_normal", o, budget, &a, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    launch_normals_select(a.normals, a.variation, sc.n, stat, stat == GSR_NORMAL_VARIATION ? nullptr : axis, lo, hi, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

// (index_ms, walk_ms) of the context's last call: the index with its bound (0 for the OWN source), and the fill with the walk or
// the OWN kernel, between events on the stream.  Not part of the ABI (tools/bench_cabi.cpp --normals).
int gsr_debug_normals_times(gsr_ctx* c, float* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    std::memcpy(out, c->nm.ms, sizeof c->nm.ms);
    return GSR_OK;
}

// the bytes of device scratch the context holds for these calls beside the neighbour scratch: 0 until the first call.  Not part
// of the ABI (tests/test_gpu_normals.py).
int gsr_debug_normals_scratch(gsr_ctx* c, uint64_t* bytes)
{
    if (!c || !bytes) return GSR_ERR_ARG;
    const gsr_ctx::Normals& nm = c->nm;
    *bytes = (nm.words ? NORMAL_INFO_WORDS * 4ull : 0ull) + (uint64_t)nm.rows * 24u;
    return GSR_OK;
}

}  // extern "C"
