// Splat data: how an attribute of the splats themselves -- position, distance from a point, colour bytes, scales, the
// contribution accumulators -- is distributed over a scene, and the splats whose value lies in a range as a picker
// (include/gsplat_hip.h, "splat data"; kernels: k_attr.hip; the value itself: k_attr.h).  All three calls are blocking and, like
// gsr_select_contrib, wait for every member's stream of a shared scene first, so nothing that writes what they read is in flight.
// They read the scene and write none of it; gsr_select_attr changes the selection the way every picker does.  The device words of
// the two reductions are the context's and are allocated by the first call: a context that never calls these allocates and
// launches nothing.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace gsr;

namespace {

constexpr uint32_t ATTR_HIST_WORDS = (ATTR_MAX_BINS + 3u + 1u) & ~1u;   // the histogram's counters, in whole 8 bytes: AttrStats follow

// The refusals every call shares, in the header's order, and the sources of the attribute's value.  Nothing is touched by a
// refused call.  Afterwards the device is current and no member's stream holds work.
int attr_enter(gsr_ctx* c, const char* who, int32_t attr, const double* origin, AttrSource* src)
{
    if (attr < 0 || attr >= ATTR_COUNT) return fail(c, GSR_ERR_ARG, "%s: unknown attribute %d", who, attr);
    SharedScene& sc = *c->scene;
    AttrSource s{};
    s.px = sc.arr.px; s.py = sc.arr.py; s.pz = sc.arr.pz; s.rgba = sc.arr.rgba;
    if (attr == ATTR_DISTANCE) {
        if (!origin) return fail(c, GSR_ERR_ARG, "%s: GSR_ATTR_DISTANCE needs an origin", who);
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(origin[k])) return fail(c, GSR_ERR_ARG, "%s: origin component %d is %g: it must be finite", who, k, origin[k]);
        s.ox = origin[0]; s.oy = origin[1]; s.oz = origin[2];
    }
    if (attr >= ATTR_SCALE_X && attr <= ATTR_SCALE_MAX) {
        if (int r = require_rows(c)) return r;
        s.scl = sc.arr.scl;
    }
    const bool contrib = attr >= ATTR_CONTRIB_WEIGHT;
    const SharedScene::Contrib& k = sc.contrib;
    if (contrib && !k.live()) return fail(c, GSR_ERR_ARG, "%s: no pass has contributed yet (frames == 0)", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    if (contrib) {
        uint32_t frames = 0;
        HIP_TRY(c, hipMemcpyAsync(&frames, k.counters, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!frames) return fail(c, GSR_ERR_ARG, "%s: no pass has contributed yet (frames == 0)", who);
        s.weight = k.weight; s.peak = k.peak; s.pixels = k.pixels;
    }
    *src = s;
    return GSR_OK;
}

// the context's device words, allocated by the first call that needs them
int attr_ensure(gsr_ctx* c)
{
    if (c->attr.words) return GSR_OK;
    return c->attr.words.alloc(c, ATTR_HIST_WORDS + (size_t)(ATTR_MAX_GRID + 1u) * (sizeof(AttrStats) / 4));
}

}  // namespace

int gsr::scope_check(gsr_ctx* c, const char* who, uint32_t scope, uint64_t budget)
{
    if (scope & ~(ATTR_SCOPE_SELECTED | ATTR_SCOPE_VISIBLE)) return fail(c, GSR_ERR_ARG, "%s: unknown scope flags 0x%x", who, scope);
    if (budget > GSR_NEIGHBOUR_MAX_BUDGET)
        return fail(c, GSR_ERR_ARG, "%s: budget (%llu) is above GSR_NEIGHBOUR_MAX_BUDGET (%llu)", who, (unsigned long long)budget,
                    (unsigned long long)GSR_NEIGHBOUR_MAX_BUDGET);
    return GSR_OK;
}

extern "C" {

int gsr_attr_stats(gsr_ctx* c, int32_t attr, const double* origin, uint32_t scope, uint32_t* count, uint32_t* nan, double* min, double* max)
{
    if (!c) return GSR_ERR_ARG;
    AttrSource src;
    if (int r = scope_check(c, "gsr_attr_stats", scope)) return r;
    const AttrScope sc = scene_scope(*c->scene, scope);
    if (int r = attr_enter(c, "gsr_attr_stats", attr, origin, &src)) return r;
    AttrStats got{0u, 0u, std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
    if (const uint32_t n = c->scene->n) {
        if (int r = attr_ensure(c)) return r;
        AttrStats* partial = reinterpret_cast<AttrStats*>(c->attr.words + ATTR_HIST_WORDS);
        AttrStats* result = partial + ATTR_MAX_GRID;
        launch_attr_stats(attr, src, sc, n, c->cu_count, partial, result, c->stream);
        hipError_t e0 = hipGetLastError();
        hipError_t e1 = hipMemcpyAsync(&got, result, sizeof got, hipMemcpyDeviceToHost, c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        for (hipError_t e : {e0, e1, e2, hipGetLastError()})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_attr_stats failed: %s", hipGetErrorString(e));
    }
    if (count) *count = got.count;
    if (nan) *nan = got.nan;
    if (min) *min = got.mn;
    if (max) *max = got.mx;
    return GSR_OK;
}

int gsr_attr_histogram(gsr_ctx* c, int32_t attr, const double* origin, uint32_t scope, double lo, double hi, uint32_t bins, uint32_t* counts,
                       uint32_t* outside)
{
    if (!c) return GSR_ERR_ARG;
    if (bins < 1u || bins > ATTR_MAX_BINS) return fail(c, GSR_ERR_ARG, "gsr_attr_histogram: bins (%u) must be in 1 .. %u", bins, ATTR_MAX_BINS);
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo)))
        return fail(c, GSR_ERR_ARG, "gsr_attr_histogram: [%g, %g) must be finite, of finite width, with lo < hi", lo, hi);
    AttrSource src;
    if (int r = scope_check(c, "gsr_attr_histogram", scope)) return r;
    const AttrScope sc = scene_scope(*c->scene, scope);
    if (int r = attr_enter(c, "gsr_attr_histogram", attr, origin, &src)) return r;
    const uint32_t ncounters = bins + 3u;
    uint32_t got[ATTR_MAX_BINS + 3u];
    std::memset(got, 0, (size_t)ncounters * 4);
    if (const uint32_t n = c->scene->n) {
        if (int r = attr_ensure(c)) return r;
        const AttrRange range{lo, hi, (hi - lo) / (double)bins, bins};
        HIP_TRY(c, hipMemsetAsync(c->attr.words, 0, (size_t)ncounters * 4, c->stream));
        launch_attr_hist(attr, src, sc, n, c->knobs.attr_hist_grid ? c->knobs.attr_hist_grid : attr_grid(n, c->cu_count, ATTR_HIST_WG_PER_CU), range,
                         c->knobs.attr_hist_peel ? ATTR_HIST_PEEL : ATTR_HIST_PLAIN, c->attr.words, c->stream);
        hipError_t e0 = hipGetLastError();
        hipError_t e1 = hipMemcpyAsync(got, c->attr.words, (size_t)ncounters * 4, hipMemcpyDeviceToHost, c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        for (hipError_t e : {e0, e1, e2, hipGetLastError()})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_attr_histogram failed: %s", hipGetErrorString(e));
    }
    if (counts) std::memcpy(counts, got, (size_t)bins * 4);
    if (outside) std::memcpy(outside, got + bins, 3 * 4);
    return GSR_OK;
}

int gsr_select_attr(gsr_ctx* c, int32_t attr, const double* origin, double lo, double hi, int32_t op, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_attr: unknown op %d", op);
    if (std::isnan(lo) || std::isnan(hi)) return fail(c, GSR_ERR_ARG, "gsr_select_attr: a bound is NaN");
    if (lo > hi) return fail(c, GSR_ERR_ARG, "gsr_select_attr: lo (%g) is above hi (%g)", lo, hi);
    AttrSource src;
    if (int r = attr_enter(c, "gsr_select_attr", attr, origin, &src)) return r;
    SharedScene& sc = *c->scene;
    if (!sc.n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    launch_attr_select(attr, src, sc.n, lo, hi, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

}  // extern "C"
