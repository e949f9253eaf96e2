// Depth planes and picking: which splat, and how far away, is under a pixel of the last rendered frame.  A separate launch
// behind the frame on the context's stream (k_depth.hip) -- never a node of the frame's graph, nothing of FrameArgs -- over the
// bin lists, records and positions the frame left on the device.  A context that never calls these allocates nothing.
#include "gsr_ctx.h"

#include <cmath>

using namespace gsr;

// the last enqueued frame can be walked: a render frame whose scene, size, band and lists are still the context's
int gsr::depth_frame_check(gsr_ctx* c, const char* who)
{
    if (!c->have_frame) return fail(c, GSR_ERR_ARG, "%s: no frame has been rendered yet (or the scene or the size changed since the last one)", who);
    if (!c->timing.render) return fail(c, GSR_ERR_ARG, "%s: the last frame was sort-only: it has no bin lists", who);
    const BinGrid g = make_grid(c);
    if (!c->frame_lists || c->cam_frame.W != c->W || c->cam_frame.H != c->H || c->cam_frame.band_px0 != g.bx_lo * BIN_PX ||
        c->cam_frame.band_px1 != g.bx_hi * BIN_PX)
        return fail(c, GSR_ERR_ARG, "%s: the band or the list buffers changed since the last frame: render it again", who);
    return GSR_OK;
}

FrameLists gsr::frame_lists(const gsr_ctx* c)
{
    FrameLists f{};
    f.bin_start = c->bin.start; f.list = c->bin.list; f.rec = c->sort.rec;
    f.px = c->scene->arr.px; f.py = c->scene->arr.py; f.pz = c->scene->arr.pz;
    f.overflow = &c->words.fstate->overflow;
    f.capacity = c->bin.capacity;
    f.nsplats = std::max(c->scene->n, 1u);   // (the walk clamps a list entry to nsplats - 1)
    return f;
}

namespace {

constexpr uint32_t MAX_PICKS = 4096;
static_assert(sizeof(PickResult) == sizeof(gsr_pick_result) && offsetof(PickResult, alpha) == offsetof(gsr_pick_result, alpha),
              "the kernel's result is the header's");

// the frame's lists and the planes a pass writes (none: gsr_pick)
DepthBuffers buffers(gsr_ctx* c, uint32_t* invalid, float* mean, float* hit, uint32_t* index)
{
    return DepthBuffers{frame_lists(c), invalid, mean, hit, index, c->depth.hit_alpha};
}

// the context's planes pass behind whatever the stream holds; the planes are then those of the last enqueued frame
int enqueue_planes(gsr_ctx* c)
{
    gsr_ctx::Depth& d = c->depth;
    const size_t np = (size_t)c->W * c->H;
    if (np > d.pixels || !d.planes.hit) {
        if (int r = d.planes.alloc(c, c->W, c->H, 1)) return r;
        d.pixels = np;
        d.planes_serial = 0;
    }
    d.planes.Wd = c->W; d.planes.Hd = c->H;   // (a smaller image than they were allocated for lies at their front)
    if (int r = depth_enqueue(c, d.planes, 1, DEPTH_FILL_PLANES)) return r;
    HIP_TRY(c, hipGetLastError());
    d.planes_serial = c->frame_serial;
    return GSR_OK;
}

}  // namespace

// what gsr_sync does for the frame (a frame that did not fit is rendered again with regrown lists), then the frame's checks again
int gsr::depth_settle_frame(gsr_ctx* c, const char* who)
{
    if (int r = depth_frame_check(c, who)) return r;
    if (int r = sync_and_repair(c)) return r;
    return depth_frame_check(c, who);   // (a regrowth for earlier frames may have taken the lists with it)
}

int gsr::depth_planes_current(gsr_ctx* c, const char* who)
{
    if (int r = depth_settle_frame(c, who)) return r;
    gsr_ctx::Depth& d = c->depth;
    if (!d.planes.hit || d.planes_serial != c->frame_serial) {   // (a repaired frame has a new serial: a pass behind the unfit one is redone)
        if (int r = enqueue_planes(c)) return r;
    }
    uint32_t invalid = 0;
    HIP_TRY(c, hipMemcpyAsync(&invalid, d.planes.invalid, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (invalid) {   // never returned as data
        d.planes_serial = 0;
        return fail(c, GSR_ERR_OVERFLOW, "%s: the frame's bin lists did not fit: the planes are not valid", who);
    }
    return GSR_OK;
}

// One pass for every user: the frame's lists with the frame's camera and the context's hit_alpha of this moment, into `p`.  A band
// context's bins do not cover the image and the pass writes the band's columns only: what the user has in the others (`fill`) is
// written when the planes, the size or the band are new.
int gsr::depth_enqueue(gsr_ctx* c, DepthPlanes& p, int step, DepthFill fill)
{
    const BinGrid g = make_grid(c);
    const int key[4] = {c->W, c->H, g.bx_lo, g.bx_hi};
    if (fill != DEPTH_FILL_NOTHING && !std::equal(key, key + 4, p.fill_key)) {
        const bool whole = g.bx_lo == 0 && g.bx_hi == g.nbx;   // the bins cover the image: no other columns
        const size_t np = (size_t)p.Wd * p.Hd;
        if (!whole && fill == DEPTH_FILL_PLANES) launch_depth_fill(p.mean, p.hit, p.index, (uint32_t)np, c->stream);
        if (!whole && fill == DEPTH_FILL_HIT) HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)p.hit.p, 0x7f800000, np, c->stream));
        std::copy(key, key + 4, p.fill_key);
    }
    launch_depth_planes(buffers(c, p.invalid, p.mean, p.hit, p.index), g, c->cam_frame, c->knobs.depth_skip, step, c->stream);
    return GSR_OK;
}

extern "C" {

int gsr_set_hit_alpha(gsr_ctx* c, float a)
{
    if (!c) return GSR_ERR_ARG;
    if (!(a > 0.0f && a <= 1.0f)) return fail(c, GSR_ERR_ARG, "hit_alpha must be in (0, 1], not %g", (double)a);
    if (a != c->depth.hit_alpha) c->depth.planes_serial = 0;
    c->depth.hit_alpha = a;
    return GSR_OK;
}

int gsr_depth_async(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = depth_frame_check(c, "gsr_depth_async")) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    return enqueue_planes(c);
}

int gsr_read_depth(gsr_ctx* c, float* mean, float* hit, uint32_t* index)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = depth_planes_current(c, "gsr_read_depth")) return r;
    gsr_ctx::Depth& d = c->depth;
    const size_t np = (size_t)c->W * c->H;
    if (mean) HIP_TRY(c, hipMemcpyAsync(mean, d.planes.mean, np * 4, hipMemcpyDeviceToHost, c->stream));
    if (hit) HIP_TRY(c, hipMemcpyAsync(hit, d.planes.hit, np * 4, hipMemcpyDeviceToHost, c->stream));
    if (index) HIP_TRY(c, hipMemcpyAsync(index, d.planes.index, np * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

void* gsr_depth_device_ptr(gsr_ctx* c, int32_t plane)
{
    if (!c) return nullptr;
    const DepthPlanes& p = c->depth.planes;
    return plane == 0 ? (void*)p.mean : plane == 1 ? (void*)p.hit : plane == 2 ? (void*)p.index : nullptr;
}

int gsr_pick(gsr_ctx* c, const int32_t* xy, uint32_t count, gsr_pick_result* out)
{
    if (!c) return GSR_ERR_ARG;
    if (!xy || !out) return fail(c, GSR_ERR_ARG, "gsr_pick: xy or out is NULL");
    if (!count || count > MAX_PICKS) return fail(c, GSR_ERR_ARG, "gsr_pick: count must be 1..%u, not %u", MAX_PICKS, count);
    if (int r = depth_frame_check(c, "gsr_pick")) return r;
    const BinGrid g = make_grid(c);
    const int xlo = g.bx_lo * BIN_PX, xhi = std::min(g.bx_hi * BIN_PX, c->W);
    for (uint32_t k = 0; k < count; k++) {
        const int x = xy[2 * k], y = xy[2 * k + 1];
        if (x < 0 || x >= c->W || y < 0 || y >= c->H) return fail(c, GSR_ERR_ARG, "gsr_pick: pixel (%d, %d) is outside the %dx%d image", x, y, c->W, c->H);
        if (x < xlo || x >= xhi) return fail(c, GSR_ERR_ARG, "gsr_pick: pixel (%d, %d) is outside this context's band [%d, %d)", x, y, xlo, xhi);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = depth_settle_frame(c, "gsr_pick")) return r;
    gsr_ctx::Depth& d = c->depth;
    if (!d.result) {
        if (int r = d.pick_invalid.alloc(c, 1)) return r;
        HIP_TRY(c, hipMemsetAsync(d.pick_invalid, 0, 4, c->stream));
        if (int r = d.query.alloc(c, (size_t)MAX_PICKS * 2)) return r;
        if (int r = d.result.alloc(c, MAX_PICKS)) return r;
    }
    HIP_TRY(c, hipMemcpyAsync(d.query, xy, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
    launch_pick(buffers(c, d.pick_invalid, nullptr, nullptr, nullptr), g, c->cam_frame, d.query, count, d.result, c->stream);
    HIP_TRY(c, hipGetLastError());
    uint32_t invalid = 0;
    HIP_TRY(c, hipMemcpyAsync(&invalid, d.pick_invalid, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (invalid) return fail(c, GSR_ERR_OVERFLOW, "gsr_pick: the frame's bin lists did not fit: nothing was picked");
    HIP_TRY(c, hipMemcpyAsync(out, d.result, (size_t)count * sizeof(gsr_pick_result), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

}  // extern "C"
