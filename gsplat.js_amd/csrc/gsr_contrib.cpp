// Contribution: per splat, how much it showed over the frames of a tour -- the sum of its fragments' weights, the largest one and
// the number of pixels it covered -- accumulated on the device by a pass behind a rendered frame (k_contrib.hip), held with the
// scene (SharedScene::contrib) beside the selection, and turned into a selection by gsr_select_contrib, which
// gsr_scene_erase_selected then applies.  Like the depth pass the pass is a separate launch behind the frame on the context's
// stream, never a node of the frame's graph.  The members of a shared scene have one set of accumulators and may run passes
// concurrently on their own streams: the updates are agent-scope integer atomics and commute; the blocking calls wait for every
// member's stream, as gsr_set_scene_sh does.  A context that never calls these allocates nothing.
#include "gsr_ctx.h"

#include <cmath>

using namespace gsr;

// nothing of any member is in flight afterwards: the streams that may hold passes
int gsr::settle_members(gsr_ctx* c)
{
    for (gsr_ctx* m : c->scene->members) HIP_TRY(c, hipStreamSynchronize(m->stream));
    return GSR_OK;
}

namespace {

// gsr_contrib_reset: the accumulators for the scene's count, allocated by the first call, zeroed and final on the device
int reset_accumulators(gsr_ctx* c)
{
    SharedScene& sc = *c->scene;
    SharedScene::Contrib& k = sc.contrib;
    if (int r = settle_members(c)) return r;
    // (the count only changes under calls that drop the accumulators: while they live, rows is the scene's count)
    if (!k.live() || k.rows != sc.n) {
        k.reset();
        int r;
        if ((r = k.weight.alloc(c, sc.n)) || (r = k.peak.alloc(c, sc.n)) || (r = k.pixels.alloc(c, sc.n)) ||
            (r = k.counters.alloc(c, SharedScene::Contrib::COUNTER_WORDS))) { k.reset(); return r; }
        k.rows = k.alloc_rows = sc.n;
    }
    const size_t rows = std::max(k.rows, 1u);
    HIP_TRY(c, hipMemsetAsync(k.weight, 0, rows * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(k.peak, 0, rows * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(k.pixels, 0, rows * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(k.counters, 0, SharedScene::Contrib::COUNTER_WORDS * 4, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_contrib_reset(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return reset_accumulators(c);
}

int gsr_contrib_accumulate_async(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = depth_frame_check(c, "gsr_contrib_accumulate_async")) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    SharedScene& sc = *c->scene;
    if (!sc.contrib.live()) { if (int r = reset_accumulators(c)) return r; }   // the first use: what gsr_contrib_reset does
    const SharedScene::Contrib& k = sc.contrib;
    const ContribBuffers b{frame_lists(c), k.weight, k.peak, k.pixels, k.counters, k.rows};
    launch_contrib(b, make_grid(c), c->cam_frame, c->knobs.depth_skip, c->stream);
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

int gsr_read_contrib(gsr_ctx* c, uint64_t* weight, float* peak, uint32_t* pixels, uint32_t n, uint32_t* frames)
{
    if (!c) return GSR_ERR_ARG;
    const SharedScene& sc = *c->scene;
    const SharedScene::Contrib& k = sc.contrib;
    if (!k.live()) return fail(c, GSR_ERR_ARG, "gsr_read_contrib: nothing was ever reset or accumulated for this scene");
    if (n != sc.n) return fail(c, GSR_ERR_ARG, "gsr_read_contrib: n (%u) is not the scene's count (%u)", n, sc.n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    if (weight && n) HIP_TRY(c, hipMemcpyAsync(weight, k.weight, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    if (peak && n) HIP_TRY(c, hipMemcpyAsync(peak, k.peak, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (pixels && n) HIP_TRY(c, hipMemcpyAsync(pixels, k.pixels, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (frames) HIP_TRY(c, hipMemcpyAsync(frames, k.counters, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_select_contrib(gsr_ctx* c, int32_t stat, double below, int32_t op, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    if (stat < GSR_CONTRIB_WEIGHT || stat > GSR_CONTRIB_PIXELS) return fail(c, GSR_ERR_ARG, "gsr_select_contrib: unknown stat %d", stat);
    if (op < GSR_SELOP_REPLACE || op > GSR_SELOP_INTERSECT) return fail(c, GSR_ERR_ARG, "gsr_select_contrib: unknown op %d", op);
    if (std::isnan(below)) return fail(c, GSR_ERR_ARG, "gsr_select_contrib: below is NaN");
    SharedScene& sc = *c->scene;
    const SharedScene::Contrib& k = sc.contrib;
    // an empty tour would select the whole scene: refused
    if (!k.live()) return fail(c, GSR_ERR_ARG, "gsr_select_contrib: no pass has contributed yet (frames == 0)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    uint32_t frames = 0;
    HIP_TRY(c, hipMemcpyAsync(&frames, k.counters, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!frames) return fail(c, GSR_ERR_ARG, "gsr_select_contrib: no pass has contributed yet (frames == 0)");
    if (!sc.n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    launch_contrib_select(stat, below, sc.n, k.weight, k.peak, k.pixels, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

}  // extern "C"
