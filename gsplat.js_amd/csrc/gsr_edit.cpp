// Editing the selection: translate, rotate, scale and recolour the selected splats and nothing else, and the box of their centres
// (include/gsplat_hip.h, "editing the selection"; kernels: k_edit.hip).  An edit is a scene edit, ordered like gsr_scene_translate:
// it runs on this context's stream between edit_begin and edit_end, so frames the other members enqueued before it read the old
// scene and those enqueued behind it the new one, with no host wait, and it marks every member's frame and sorted order as edited.
// The selection, the hidden set and the contribution accumulators are not touched; a scene that never selected launches nothing.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace gsr;

namespace {

// what every edit does first: the refusals (nothing touched), then the members' frame state
int edit_enter(gsr_ctx* c, const char* who, bool linear)
{
    SharedScene& sc = *c->scene;
    if (int r = require_rows(c)) return r;
    if (linear && sc.sh_follow && sc.sh_count)   // the SH frame is one per scene: a partial rotation or scale has none
        return fail(c, GSR_ERR_ARG, "%s: with gsr_set_sh_follow on and SH rows present, a selection cannot be rotated or scaled (the SH frame is one per scene)", who);
    HIP_TRY(c, hipSetDevice(c->device));
    invalidate_members(c, true);   // (a call that would change no bit still counts as an edit)
    return GSR_OK;
}

// the kernel of an edit between edit_begin and edit_end; nothing is launched for a scene that never selected
template <class Launch>
int edit_run(gsr_ctx* c, Launch launch)
{
    SharedScene& sc = *c->scene;
    if (!sc.n || !sc.sel.mask) return GSR_OK;
    if (int r = edit_begin(c)) return r;
    launch(sc.n, sc.arr.view(), (const uint32_t*)sc.sel.mask, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return edit_end(c);
}

}  // namespace

extern "C" {

int gsr_scene_translate_selected(gsr_ctx* c, const double* t)
{
    if (!c || !t) return GSR_ERR_ARG;
    if (int r = edit_enter(c, "gsr_scene_translate_selected", false)) return r;
    return edit_run(c, [&](uint32_t n, const SceneDev& sc, const uint32_t* w, uint32_t nw, hipStream_t s) { launch_edit_translate(n, sc, w, nw, t, s); });
}

int gsr_scene_rotate_selected(gsr_ctx* c, const double* q, const double* pivot)
{
    if (!c || !q) return GSR_ERR_ARG;
    if (int r = edit_enter(c, "gsr_scene_rotate_selected", true)) return r;
    return edit_run(c, [&](uint32_t n, const SceneDev& sc, const uint32_t* w, uint32_t nw, hipStream_t s) { launch_edit_rotate(n, sc, w, nw, q, pivot, s); });
}

int gsr_scene_scale_selected(gsr_ctx* c, const double* sv, const double* pivot)
{
    if (!c || !sv) return GSR_ERR_ARG;
    for (int k = 0; k < 3; k++)   // (0 is allowed: there is no frame to invert here)
        if (!std::isfinite(sv[k])) return fail(c, GSR_ERR_ARG, "gsr_scene_scale_selected: scale component %d is %g: it must be finite", k, sv[k]);
    if (int r = edit_enter(c, "gsr_scene_scale_selected", true)) return r;
    return edit_run(c, [&](uint32_t n, const SceneDev& sc, const uint32_t* w, uint32_t nw, hipStream_t s) { launch_edit_scale(n, sc, w, nw, sv, pivot, s); });
}

int gsr_scene_set_rgba_selected(gsr_ctx* c, uint32_t rgba, uint32_t byte_mask)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = edit_enter(c, "gsr_scene_set_rgba_selected", false)) return r;
    return edit_run(c, [&](uint32_t n, const SceneDev& sc, const uint32_t* w, uint32_t nw, hipStream_t s) { launch_edit_rgba(n, sc, w, nw, rgba, byte_mask, s); });
}

// reduced on the device, 28 bytes copied back: no host loop over n.  No edit: no frame state changes.
int gsr_selection_bounds(gsr_ctx* c, struct gsr_selection_bounds* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    SharedScene& sc = *c->scene;
    out->count = 0;
    for (int k = 0; k < 3; k++) { out->min[k] = std::numeric_limits<float>::infinity(); out->max[k] = -std::numeric_limits<float>::infinity(); }
    if (!sc.n || !sc.sel.mask) return GSR_OK;   // never selected in: the empty selection
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint32_t> work;   // the workgroups' partials, then the result
    const uint32_t blocks = edit_bounds_blocks(sc.n);
    if (int r = work.alloc(c, ((size_t)blocks + 1) * EDIT_PARTIAL_WORDS)) return r;
    uint32_t* result = work + (size_t)blocks * EDIT_PARTIAL_WORDS;
    launch_edit_bounds(sc.n, sc.arr.px, sc.arr.py, sc.arr.pz, sc.sel.mask, sc.sel.words, work, result, c->stream);
    uint32_t got[7] = {0, 0, 0, 0, 0, 0, 0};
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipMemcpyAsync(got, result, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_selection_bounds failed: %s", hipGetErrorString(e));
    out->count = got[0];
    for (int k = 0; k < 3; k++) {
        std::memcpy(&out->min[k], &got[1 + k], 4);
        std::memcpy(&out->max[k], &got[4 + k], 4);
    }
    return GSR_OK;
}

}  // extern "C"
