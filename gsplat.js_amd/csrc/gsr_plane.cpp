// Planes: the dominant plane of the splats in scope fitted on the device by RANSAC, the scoring pass alone over planes of the
// host's, the splats whose signed distance from a plane lies in [lo, hi] as a picker, and the whole-scene rotation and translation
// that take a plane to axis . p = 0 (include/gsplat_hip.h, "planes"; kernels: k_plane.hip).  gsr_fit_plane and gsr_plane_inliers
// are blocking, stateless and ordered like gsr_select_attr: they wait for every member's stream of a shared scene first, read the
// scene and write none of it, and touch no frame state and no selection; gsr_select_plane changes the selection the way every
// picker does; gsr_plane_alignment is a pure function of its arguments and needs no device.  The scratch -- the candidate list, the
// planes, the scores and an info block -- is the context's: the first call allocates it, it only grows, the context's end frees
// it.  A context that never calls these allocates and launches nothing.
//
// The work budget.  hypotheses x candidates is a dense kernel on a shared machine.  So the candidates are listed first, the host
// reads their number, and a call whose tests = hypotheses * candidates lie above its budget is refused before the scoring kernel
// is launched.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>

using namespace gsr;

namespace {

constexpr uint32_t PL_INFO_WORDS = 2u + sizeof(PlBest) / 4u;   // the totals, then PlBest
static_assert(sizeof(PlBest) == 64 && sizeof(gsr_plane_info) == 88, "the info blocks as the header and the kernels lay them out");
static_assert(PLANE_MAX_HYPOTHESES == GSR_PLANE_MAX_HYPOTHESES, "the header's limit");

// the refusals the two scoring calls share, in the header's order.  Nothing is touched by a refused call.
int plane_check(gsr_ctx* c, const char* who, double threshold, uint32_t count, const char* count_name, uint32_t scope, uint64_t budget)
{
    if (!(std::isfinite(threshold) && threshold >= 0.0)) return fail(c, GSR_ERR_ARG, "%s: threshold (%g) must be finite and >= 0", who, threshold);
    if (count < 1u || count > PLANE_MAX_HYPOTHESES) return fail(c, GSR_ERR_ARG, "%s: %s (%u) must be in 1 .. %u", who, count_name, count, PLANE_MAX_HYPOTHESES);
    return scope_check(c, who, scope, budget);
}

// a plane of the host's: four finite entries and a normal that is not zero
int plane_ok(gsr_ctx* c, const char* who, const double* p, uint32_t k)
{
    for (int j = 0; j < 4; j++)
        if (!std::isfinite(p[j])) return fail(c, GSR_ERR_ARG, "%s: plane %u entry %d is %g: it must be finite", who, k, j, p[j]);
    if (p[0] == 0.0 && p[1] == 0.0 && p[2] == 0.0) return fail(c, GSR_ERR_ARG, "%s: plane %u has a zero normal", who, k);
    return GSR_OK;
}

// the context's scratch for n splats: allocated by the first call, only ever grown
int plane_ensure(gsr_ctx* c, uint32_t n)
{
    gsr_ctx::Plane& pl = c->pl;
    int r;
    if (!pl.words) {
        if ((r = pl.words.alloc(c, PL_INFO_WORDS)) || (r = pl.planes.alloc(c, PLANE_MAX_HYPOTHESES)) || (r = pl.triple.alloc(c, PLANE_MAX_HYPOTHESES)) ||
            (r = pl.scores.alloc(c, PLANE_MAX_HYPOTHESES)))
            return r;
    }
    if (pl.rows < n || !pl.cand) {
        pl.rows = 0;
        if ((r = pl.cand.alloc(c, n)) || (r = pl.block.alloc(c, (size_t)plane_blocks(n) + 1u))) return r;
        pl.rows = n;
    }
    for (hipEvent_t& e : pl.ev) if (!e) HIP_TRY(c, hipEventCreate(&e));
    return GSR_OK;
}

PlArrays plane_arrays(gsr_ctx* c)
{
    gsr_ctx::Plane& pl = c->pl;
    return PlArrays{reinterpret_cast<unsigned long long*>(pl.words.p), reinterpret_cast<PlBest*>(pl.words.p + 2), pl.block, pl.cand, pl.rows,
                    pl.planes, pl.triple, pl.scores};
}

// Everything up to the scoring pass: the candidates, their number against the budget, the first two and last two scalar fields of
// *info.  GSR_ERR_ARG (with *info filled) when the tests lie above the budget: no scoring kernel has been launched.  n >= 1; the
// device is current and no member's stream holds work.
int plane_candidates(gsr_ctx* c, const char* who, uint32_t count, uint32_t scope, uint64_t budget, PlArrays* arrays, uint32_t* m, gsr_plane_info* info)
{
    SharedScene& sc = *c->scene;
    const uint32_t n = sc.n;
    if (int r = plane_ensure(c, n)) return r;
    gsr_ctx::Plane& pl = c->pl;
    const PlArrays a = plane_arrays(c);
    HIP_TRY(c, hipMemsetAsync(pl.words, 0, (size_t)PL_INFO_WORDS * 4, c->stream));
    HIP_TRY(c, hipEventRecord(pl.ev[0], c->stream));
    launch_plane_candidates(sc.arr.px, sc.arr.py, sc.arr.pz, scene_scope(sc, scope), n, a, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(pl.ev[1], c->stream);
    unsigned long long totals = 0;
    uint32_t cands = 0;
    hipError_t e2 = hipMemcpyAsync(&totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipMemcpyAsync(&cands, a.block + plane_blocks(n), 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e4 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, e4, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    info->in_scope = (uint32_t)totals; info->nonfinite = (uint32_t)(totals >> 32);
    info->tests = (uint64_t)count * cands; info->budget = budget;
    *arrays = a;
    *m = cands;
    if (cands > n || cands != info->in_scope - info->nonfinite)
        return fail(c, GSR_ERR_HIP, "%s: the list holds %u candidates for %u splats in scope, %u of them non-finite", who, cands, info->in_scope, info->nonfinite);
    if (info->tests > budget)
        return fail(c, GSR_ERR_ARG, "%s: the scoring pass would make %llu tests (%u planes x %u candidates), above the budget of %llu", who,
                    (unsigned long long)info->tests, count, cands, (unsigned long long)budget);
    return GSR_OK;
}

// the two stages' times of a call that ran both, by the events around them (bench_cabi --plane)
void plane_times(gsr_ctx* c)
{
    gsr_ctx::Plane& pl = c->pl;
    float a = 0.0f, b = 0.0f;
    if (hipEventElapsedTime(&a, pl.ev[0], pl.ev[1]) == hipSuccess && hipEventElapsedTime(&b, pl.ev[1], pl.ev[2]) == hipSuccess) { pl.candidates_ms = a; pl.score_ms = b; }
    else (void)hipGetLastError();
}

bool unit3(const double* v, double* out)
{
    const double l = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(l > 0.0) || !std::isfinite(l)) return false;
    out[0] = v[0] / l; out[1] = v[1] / l; out[2] = v[2] / l; out[3] = l;
    return true;
}

}  // namespace

extern "C" {

int gsr_fit_plane(gsr_ctx* c, double threshold, uint32_t hypotheses, uint64_t seed, uint32_t scope, uint64_t budget, uint32_t* scores, gsr_plane_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = plane_check(c, "gsr_fit_plane", threshold, hypotheses, "hypotheses", scope, budget)) return r;
    if (!info) return fail(c, GSR_ERR_ARG, "gsr_fit_plane: info is NULL");
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    SharedScene& sc = *c->scene;
    gsr_plane_info got{};
    got.budget = budget;
    if (scores) std::memset(scores, 0, (size_t)hypotheses * 4);
    if (!sc.n) { *info = got; return GSR_OK; }
    PlArrays a;
    uint32_t m = 0;
    const int r = plane_candidates(c, "gsr_fit_plane", hypotheses, scope, budget, &a, &m, &got);
    if (r == GSR_OK || r == GSR_ERR_ARG) *info = got;
    if (r) return r;
    if (!got.in_scope) return GSR_OK;                 // an empty scope: zeros
    got.hypotheses = hypotheses;
    if (!m) { got.degenerate = hypotheses; *info = got; return GSR_OK; }   // no candidate: no triple exists, every hypothesis is degenerate
    gsr_ctx::Plane& pl = c->pl;
    launch_plane_hypotheses(sc.arr.px, sc.arr.py, sc.arr.pz, hypotheses, seed, m, sc.n, a, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemsetAsync(a.scores, 0, (size_t)hypotheses * 4, c->stream));
    launch_plane_score(sc.arr.px, sc.arr.py, sc.arr.pz, hypotheses, m, sc.n, threshold, true, a, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(pl.ev[2], c->stream);
    launch_plane_best(hypotheses, a, c->stream);
    hipError_t e2 = hipGetLastError();
    PlBest best{};
    hipError_t e3 = hipMemcpyAsync(&best, a.result, sizeof best, hipMemcpyDeviceToHost, c->stream);
    hipError_t e4 = scores ? hipMemcpyAsync(scores, a.scores, (size_t)hypotheses * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e5 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, e4, e5, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_fit_plane failed: %s", hipGetErrorString(e));
    plane_times(c);
    got.degenerate = best.degenerate; got.found = best.found; got.best = best.best; got.inliers = best.inliers;
    for (int k = 0; k < 3; k++) got.triple[k] = best.triple[k];
    for (int k = 0; k < 4; k++) got.plane[k] = best.plane[k];
    *info = got;
    return GSR_OK;
}

int gsr_plane_inliers(gsr_ctx* c, const double* planes, uint32_t count, double threshold, uint32_t scope, uint64_t budget, uint32_t* inliers, gsr_plane_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = plane_check(c, "gsr_plane_inliers", threshold, count, "count", scope, budget)) return r;
    if (!planes || !inliers) return fail(c, GSR_ERR_ARG, "gsr_plane_inliers: %s is NULL", planes ? "inliers" : "planes");
    for (uint32_t k = 0; k < count; k++)
        if (int r = plane_ok(c, "gsr_plane_inliers", planes + 4u * k, k)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    SharedScene& sc = *c->scene;
    gsr_plane_info got{};
    got.budget = budget; got.hypotheses = count;
    if (!sc.n) {
        std::memset(inliers, 0, (size_t)count * 4);
        if (info) *info = got;
        return GSR_OK;
    }
    PlArrays a;
    uint32_t m = 0;
    const int r = plane_candidates(c, "gsr_plane_inliers", count, scope, budget, &a, &m, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    std::memset(inliers, 0, (size_t)count * 4);
    if (!m) return GSR_OK;
    gsr_ctx::Plane& pl = c->pl;
    HIP_TRY(c, hipMemcpyAsync(a.planes, planes, (size_t)count * sizeof(double4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(a.scores, 0, (size_t)count * 4, c->stream));
    launch_plane_score(sc.arr.px, sc.arr.py, sc.arr.pz, count, m, sc.n, threshold, false, a, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(pl.ev[2], c->stream);
    hipError_t e2 = hipMemcpyAsync(inliers, a.scores, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_plane_inliers failed: %s", hipGetErrorString(e));
    plane_times(c);
    return GSR_OK;
}

int gsr_select_plane(gsr_ctx* c, const double* plane, double lo, double hi, int32_t op, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_plane: unknown op %d", op);
    if (!plane) return fail(c, GSR_ERR_ARG, "gsr_select_plane: plane is NULL");
    if (int r = plane_ok(c, "gsr_select_plane", plane, 0)) return r;
    if (std::isnan(lo) || std::isnan(hi)) return fail(c, GSR_ERR_ARG, "gsr_select_plane: a bound is NaN");
    if (lo > hi) return fail(c, GSR_ERR_ARG, "gsr_select_plane: lo (%g) is above hi (%g)", lo, hi);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    SharedScene& sc = *c->scene;
    if (!sc.n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    launch_plane_select(sc.arr.px, sc.arr.py, sc.arr.pz, sc.n, make_double4(plane[0], plane[1], plane[2], plane[3]), lo, hi, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

// The whole-scene rotation q (x, y, z, w) and translation t that take `plane` to axis . p = 0: gsr_scene_rotate(q) then
// gsr_scene_translate(t).  f64, in the written order; no context, no device.
int gsr_plane_alignment(const double* plane, const double* axis, double* q, double* t)
{
    if (!plane || !axis || !q || !t) return fail(nullptr, GSR_ERR_ARG, "gsr_plane_alignment: a NULL pointer");
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(plane[k])) return fail(nullptr, GSR_ERR_ARG, "gsr_plane_alignment: plane entry %d is %g: it must be finite", k, plane[k]);
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(axis[k])) return fail(nullptr, GSR_ERR_ARG, "gsr_plane_alignment: axis entry %d is %g: it must be finite", k, axis[k]);
    double n[4], a[4];
    if (!unit3(plane, n)) return fail(nullptr, GSR_ERR_ARG, "gsr_plane_alignment: the plane's normal is zero (or its length is not finite)");
    if (!unit3(axis, a)) return fail(nullptr, GSR_ERR_ARG, "gsr_plane_alignment: the axis is zero (or its length is not finite)");
    const double d = plane[3] / n[3];
    const double cs = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2];
    double v[3], w;
    if (cs > -1.0 + 1.0 / 1048576.0) {
        v[0] = n[1] * a[2] - n[2] * a[1]; v[1] = n[2] * a[0] - n[0] * a[2]; v[2] = n[0] * a[1] - n[1] * a[0];
        w = 1.0 + cs;
    } else {   // (nearly) antiparallel: a half turn about n x e, e the unit axis of n's smallest component in magnitude (x before y before z)
        int k = 0;
        if (std::fabs(n[1]) < std::fabs(n[k])) k = 1;
        if (std::fabs(n[2]) < std::fabs(n[k])) k = 2;
        double e[3] = {0.0, 0.0, 0.0};
        e[k] = 1.0;
        v[0] = n[1] * e[2] - n[2] * e[1]; v[1] = n[2] * e[0] - n[0] * e[2]; v[2] = n[0] * e[1] - n[1] * e[0];
        w = 0.0;
    }
    const double len = std::sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + w * w);
    q[0] = v[0] / len; q[1] = v[1] / len; q[2] = v[2] / len; q[3] = w / len;
    t[0] = d * a[0]; t[1] = d * a[1]; t[2] = d * a[2];
    return GSR_OK;
}

// (candidates_ms, score_ms) of the context's last call that ran both stages, between events on the stream.  Not part of the ABI
// (tools/bench_cabi.cpp --plane).
int gsr_debug_plane_times(gsr_ctx* c, float* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    out[0] = c->pl.candidates_ms; out[1] = c->pl.score_ms;
    return GSR_OK;
}

}  // extern "C"
