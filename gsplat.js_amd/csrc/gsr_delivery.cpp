// ---------------------------------------------------------------------------------------------------------
// Frame delivery: finished frames (RGBA8, or 4:2:0 Y'CbCr as NV12 / I420) reach the host through a ring of pinned blocks while the
// next frames render.
// A slot is FREE, IN_FLIGHT (gsr_deliver_frame_async took it: kernel and copy are enqueued) or HELD (the host acquired it
// and reads its pixels).  It becomes FREE again only through the host -- gsr_release_frame, or a gsr_acquire_frame that
// refuses the frame -- and both come after a wait for the slot's copy: a free slot never has device work outstanding, so
// taking one needs no device-side wait on its previous use.
// ---------------------------------------------------------------------------------------------------------
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>

using namespace gsr;

using DeliverySlot = gsr_ctx::Delivery::Slot;

// BT.709 in 1/256: every chroma row sums to zero, the full-range luma row to 256, so greys are neutral exactly
static YuvParams yuv_params(bool full_range, const uint8_t* bg)
{
    YuvParams k = full_range ? YuvParams{0, {54, 183, 19}, {-29, -99, 128}, {128, -116, -12}, 0, 255, 0}
                             : YuvParams{16, {47, 157, 16}, {-26, -86, 112}, {112, -102, -10}, 16, 240, 0};
    k.bg = (uint32_t)bg[0] | ((uint32_t)bg[1] << 8) | ((uint32_t)bg[2] << 16);
    return k;
}

bool gsr::delivery_frame_held(const gsr_ctx* c)
{
    for (const DeliverySlot& sl : c->delivery.ring) if (sl.state == DeliverySlot::HELD) return true;
    return false;
}

// waits for every copy in flight (and the conversion kernels in front of them), then frees the ring
void gsr::delivery_free(gsr_ctx* c)
{
    if (!c->delivery.ring.empty()) {
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (c->comm.stream) (void)hipStreamSynchronize(c->comm.stream);
    }
    if (c->delivery.copy_stream) (void)hipStreamSynchronize(c->delivery.copy_stream);
    for (DeliverySlot& sl : c->delivery.ring) {
        if (sl.done) (void)hipEventSynchronize(sl.done);   // (a copy issued on an exchange stream this context has left since)
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.host) (void)hipHostFree(sl.host);
    }
    c->delivery.ring.clear();   // (frees the slots' staging buffers)
    if (c->delivery.ev_staged) (void)hipEventDestroy(c->delivery.ev_staged);
    c->delivery.ev_staged = nullptr;
    if (c->delivery.copy_stream) (void)hipStreamDestroy(c->delivery.copy_stream);
    c->delivery.copy_stream = nullptr;
    c->delivery.W = c->delivery.H = 0;
    c->delivery.next = 0;
    c->delivery.depth.planes.reset();   // (the spec stays: gsr_resize reallocates for it)
}

// (re)allocates the ring for the context's current size; frames in flight are waited for and dropped
int gsr::delivery_alloc(gsr_ctx* c, int slots)
{
    delivery_free(c);
    c->delivery.W = c->W; c->delivery.H = c->H;
    gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;
    auto bail = [c](int code) { delivery_free(c); return code; };
    if (dp.spec.on()) { if (int r = dp.planes.alloc(c, c->W, c->H, dp.spec.step)) return bail(r); }
    const size_t bytes = c->delivery.slot_bytes();
    hipError_t e = hipStreamCreateWithFlags(&c->delivery.copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->delivery.ev_staged, hipEventDisableTiming);
    c->delivery.ring.resize((size_t)slots);
    for (DeliverySlot& sl : c->delivery.ring) {
        if (e == hipSuccess) e = hipHostMalloc((void**)&sl.host, bytes, hipHostMallocDefault);
        if (e == hipSuccess && sl.staging.alloc(c, bytes / 4) != GSR_OK) e = hipErrorOutOfMemory;   // (bytes: payload + trailer, whole words)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
    }
    if (e != hipSuccess) return bail(fail(c, GSR_ERR_HIP, "allocating the delivery ring (%d slots of %zu bytes) failed: %s", slots, bytes, hipGetErrorString(e)));
    return GSR_OK;
}

// the slot holding frame `serial` in state `want`; serial 0: the oldest frame in flight
static DeliverySlot* find_slot(gsr_ctx* c, uint64_t serial, DeliverySlot::State want)
{
    DeliverySlot* found = nullptr;
    for (DeliverySlot& sl : c->delivery.ring) {
        if (sl.state != want) continue;
        if (serial ? sl.serial == serial : (!found || sl.serial < found->serial)) found = &sl;
    }
    return found;
}

int gsr::depth_options_check(gsr_ctx* c, const char* who, const gsr_depth_delivery_options* depth)
{
    if (depth->format != GSR_DEPTH_F32 && depth->format != GSR_DEPTH_U16)
        return fail(c, GSR_ERR_ARG, "%s: unknown depth format %d (GSR_DEPTH_NONE, GSR_DEPTH_F32, GSR_DEPTH_U16)", who, depth->format);
    if (depth->step != 1 && depth->step != 2) return fail(c, GSR_ERR_ARG, "%s: depth step %d (1 or 2)", who, depth->step);
    if (depth->format == GSR_DEPTH_U16 && !(depth->near > 0.0f && std::isfinite(depth->near)))
        return fail(c, GSR_ERR_ARG, "%s: GSR_DEPTH_U16 needs a finite near > 0, not %g", who, (double)depth->near);
    if (depth->reserved) return fail(c, GSR_ERR_ARG, "%s: gsr_depth_delivery_options.reserved must be 0", who);
    return GSR_OK;
}

// a depth ring on a context whose group exchanges depth: the ring's spec must be the exchange's (GSR_ERR_ARG names the first field that is not)
static int exchange_mismatch(gsr_ctx* c, const char* who, const DepthSpec& ring)
{
    const gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
    const DepthSpec& ex = dx.spec;
    if (ring == ex && c->W == dx.W && c->H == dx.H) return GSR_OK;
    if (ring.format != ex.format)
        return fail(c, GSR_ERR_ARG, "%s: the ring's depth format (%d) is not the one the group exchanges (%d, gsr_comm_set_depth)", who, ring.format, ex.format);
    if (ring.step != ex.step) return fail(c, GSR_ERR_ARG, "%s: the ring's depth step (%d) is not the one the group exchanges (%d, gsr_comm_set_depth)", who, ring.step, ex.step);
    if (c->W != dx.W || c->H != dx.H) return fail(c, GSR_ERR_ARG, "%s: the size changed since gsr_comm_set_depth: join the group again", who);
    return fail(c, GSR_ERR_ARG, "%s: the ring's depth near (%g) is not the one the group exchanges (%g, gsr_comm_set_depth)", who, (double)ring.near, (double)ex.near);
}

extern "C" {

static int delivery_open_checked(gsr_ctx* c, const char* who, int32_t slots)
{
    if (slots < 2 || slots > 8) return fail(c, GSR_ERR_ARG, "%s: %d slots (2..8)", who, slots);
    if (!c->W || !c->H) return fail(c, GSR_ERR_ARG, "%s: set the framebuffer size first", who);
    if (delivery_frame_held(c)) return fail(c, GSR_ERR_ARG, "%s: a delivered frame is held (gsr_release_frame first)", who);
    return GSR_OK;
}

int gsr_delivery_open(gsr_ctx* c, int32_t slots)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = delivery_open_checked(c, "gsr_delivery_open", slots)) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    c->delivery.format = GSR_FORMAT_RGBA8;
    c->delivery.depth.spec = {};
    c->delivery.overlay = false;
    return delivery_alloc(c, slots);
}

// gsr_delivery_open_ex, and with `depth` gsr_delivery_open_depth: nothing of the context changes unless every argument is accepted
static int delivery_open_options(gsr_ctx* c, const char* who, const gsr_delivery_options* opt, const gsr_depth_delivery_options* depth)
{
    if (!opt) return fail(c, GSR_ERR_ARG, "%s: options are NULL", who);
    if (opt->format != GSR_FORMAT_RGBA8 && opt->format != GSR_FORMAT_NV12 && opt->format != GSR_FORMAT_I420)
        return fail(c, GSR_ERR_ARG, "%s: unknown format %d (GSR_FORMAT_RGBA8, GSR_FORMAT_NV12, GSR_FORMAT_I420)", who, opt->format);
    const DepthSpec spec = DepthSpec::from(depth);
    if (spec.on()) {
        if (int r = depth_options_check(c, who, depth)) return r;
        if (c->comm.joined() && !c->comm.depth.on())
            return fail(c, GSR_ERR_ARG, "%s: this context is in a group: depth is not exchanged between ranks, so a gathered frame has no depth plane to deliver", who);
        // a group that exchanges depth (gsr_comm_set_depth) delivers the gathered plane as it is: the ring's options must be the exchange's
        if (c->comm.joined()) { if (int r = exchange_mismatch(c, who, spec)) return r; }
    }
    if (!c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "%s: a delivery ring is open (gsr_delivery_close first)", who);
    if (int r = delivery_open_checked(c, who, opt->slots)) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    c->delivery.format = opt->format;
    c->delivery.yuv = yuv_params(opt->full_range != 0, opt->background);
    c->delivery.depth.spec = spec;
    c->delivery.overlay = false;
    return delivery_alloc(c, opt->slots);
}

int gsr_delivery_open_ex(gsr_ctx* c, const gsr_delivery_options* opt)
{
    if (!c) return GSR_ERR_ARG;
    return delivery_open_options(c, "gsr_delivery_open_ex", opt, nullptr);
}

int gsr_delivery_open_depth(gsr_ctx* c, const gsr_delivery_options* opt, const gsr_depth_delivery_options* depth)
{
    if (!c) return GSR_ERR_ARG;
    return delivery_open_options(c, "gsr_delivery_open_depth", opt, depth);
}

int gsr_delivery_depth_layout(gsr_ctx* c, gsr_depth_layout* out)
{
    if (!c) return GSR_ERR_ARG;
    if (!out) return fail(c, GSR_ERR_ARG, "gsr_delivery_depth_layout: out is NULL");
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_delivery_depth_layout: no delivery ring (gsr_delivery_open_depth)");
    const gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;
    if (!dp.spec.on()) return fail(c, GSR_ERR_ARG, "gsr_delivery_depth_layout: the ring was opened without a depth plane (gsr_delivery_open_depth)");
    *out = dp.spec.layout(dp.planes.Wd, dp.planes.Hd, c->delivery.depth_offset());
    return GSR_OK;
}

int gsr_delivery_layout(gsr_ctx* c, gsr_frame_layout* out)
{
    if (!c) return GSR_ERR_ARG;
    if (!out) return fail(c, GSR_ERR_ARG, "gsr_delivery_layout: out is NULL");
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_delivery_layout: no delivery ring (gsr_delivery_open)");
    const gsr_ctx::Delivery& d = c->delivery;
    const int32_t W = d.W, H = d.H, Wc = (W + 1) / 2, Hc = (H + 1) / 2;
    *out = gsr_frame_layout{};
    out->format = d.format; out->width = W; out->height = H;
    out->bytes = d.pixel_bytes();
    out->stride[0] = W; out->rows[0] = H;
    if (d.format == GSR_FORMAT_RGBA8) {
        out->planes = 1;
        out->stride[0] = W * 4;
    } else if (d.format == GSR_FORMAT_NV12) {
        out->planes = 2;
        out->offset[1] = (uint64_t)W * H; out->stride[1] = 2 * Wc; out->rows[1] = Hc;
    } else {
        out->planes = 3;
        out->offset[1] = (uint64_t)W * H; out->offset[2] = out->offset[1] + (uint64_t)Wc * Hc;
        out->stride[1] = out->stride[2] = Wc; out->rows[1] = out->rows[2] = Hc;
    }
    return GSR_OK;
}

int gsr_delivery_close(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_delivery_close: no delivery ring (gsr_delivery_open)");
    if (delivery_frame_held(c)) return fail(c, GSR_ERR_ARG, "gsr_delivery_close: a delivered frame is held (gsr_release_frame first): its pixels would be freed");
    HIP_TRY(c, hipSetDevice(c->device));
    delivery_free(c);
    c->delivery.depth.spec = {};
    c->delivery.overlay = false;
    return GSR_OK;
}

int gsr_delivery_set_overlay(gsr_ctx* c, int32_t on)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_delivery_set_overlay: no delivery ring (gsr_delivery_open)");
    if (on && c->comm.joined())
        return fail(c, GSR_ERR_ARG, "gsr_delivery_set_overlay: this context is in a group: the gathered frame is RGBA8 of other ranks, which the overlay cannot tint");
    if (on && !c->overlay.on) return fail(c, GSR_ERR_ARG, "gsr_delivery_set_overlay: no overlay options (gsr_set_overlay first)");
    c->delivery.overlay = on != 0;
    return GSR_OK;
}

int gsr_deliver_frame_async(gsr_ctx* c, uint64_t* serial)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: no delivery ring (gsr_delivery_open)");
    gsr_ctx::Delivery& dl = c->delivery;
    const bool group = c->comm.joined();
    const bool depth = dl.depth.spec.on();
    if (depth && group && !c->comm.depth.on())   // (refused before anything else is looked at: nothing enqueued, no slot taken)
        return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: this context joined a group after it opened a depth ring: depth is not exchanged "
                                    "between ranks, so a gathered frame has no depth plane to deliver (gsr_delivery_close, then a ring without depth)");
    if (depth && group) {   // the group exchanges depth: the gathered plane is delivered as it is, so the ring must have been opened for it
        if (int r = exchange_mismatch(c, "gsr_deliver_frame_async", dl.depth.spec)) return r;
        if (dl.depth.planes.Wd != c->comm.depth.planes.Wd || dl.depth.planes.Hd != c->comm.depth.planes.Hd)
            return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: the size changed since gsr_comm_set_depth: join the group again");
    }
    if (dl.overlay && group)   // (likewise refused before anything else is looked at)
        return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: this context joined a group after gsr_delivery_set_overlay: the gathered frame is RGBA8 of "
                                    "other ranks, which the overlay cannot tint (gsr_delivery_set_overlay(ctx, 0))");
    if (group ? !c->comm.frame8_valid : !c->have_frame)
        return fail(c, GSR_ERR_ARG, group ? "gsr_deliver_frame_async: no gathered frame yet (gsr_allgather_frame_async)" : "gsr_deliver_frame_async: nothing rendered yet");
    // a depth ring needs what gsr_depth_async needs of the frame; refused before a slot is looked for: nothing enqueued, no slot taken
    // (in a group the pass ran with the exchange: gsr_allgather_frame_async has asked the same of the frame it gathered)
    if (depth && !group) { if (int r = depth_frame_check(c, "gsr_deliver_frame_async (depth ring)")) return r; }
    // an overlay ring likewise, and it needs options
    if (dl.overlay) {
        if (!c->overlay.on) return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: the ring delivers the overlay, but the options are off (gsr_set_overlay)");
        if (int r = depth_frame_check(c, "gsr_deliver_frame_async (overlay ring)")) return r;
    }
    DeliverySlot* sl = nullptr;
    const int slots = (int)dl.ring.size();
    for (int k = 0; k < slots && !sl; k++) {
        DeliverySlot& cand = dl.ring[(size_t)((dl.next + k) % slots)];
        if (cand.state == DeliverySlot::FREE) sl = &cand;
    }
    if (!sl) return fail(c, GSR_ERR_BUSY, "gsr_deliver_frame_async: all %d delivery slots are in flight or held (gsr_acquire_frame / gsr_release_frame)", slots);
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t k = dl.serial + 1;
    const size_t bytes = dl.slot_bytes();
    const bool yuv = dl.format != GSR_FORMAT_RGBA8;
    // The source.  The context's own frame: fb and the frame's overflow word; the work goes on the render stream (it has read fb, lists
    // and records before the next frame's chain, which follows there, overwrites them), the copy on the copy stream behind ev_staged.
    // A group's gathered frame: frame8 and the word behind it (one bit per rank whose band is stale), as the de-slab steps left them
    // on the exchange stream; work and copy both go there, in front of the next frame's de-slab.
    // An overlay ring: the overlay pass behind the frame on the render stream, and its image in place of the framebuffer.  One image
    // per context suffices for the reason one framebuffer does: the conversion reads it on the render stream in front of the next pass.
    if (dl.overlay) { if (int r = overlay_enqueue(c)) return r; }
    const float4* fb = group ? nullptr : dl.overlay ? c->overlay.image.p : c->out.fb.p;
    const uint32_t* frame8 = group ? c->comm.frame8.p : nullptr;
    const uint32_t* flag = group ? frame8 + (size_t)c->W * c->H : &c->words.fstate->overflow;
    const hipStream_t work = group ? c->comm.stream : c->stream, copy = group ? c->comm.stream : dl.copy_stream;
    uint8_t* const staging = reinterpret_cast<uint8_t*>(sl->staging.p);
    const void* payload = staging;   // what the copy reads
    hipError_t e = hipSuccess;
    // 1. colour into the slot's staging, with a trailer (flag word, serial, size) behind it
    if (yuv) {
        launch_deliver_yuv(dl.format, fb, frame8, staging, bytes, c->W, c->H, dl.yuv, k, flag, work);
    } else if (!group) {
        launch_deliver_rgba8(fb, sl->staging, c->W, c->H, k, flag, work);
    } else if (depth) {   // gathered pixels are RGBA8 already: a plain copy
        e = hipMemcpyAsync(staging, frame8, (size_t)c->W * c->H * 4, hipMemcpyDeviceToDevice, work);
    } else {              // and without a plane behind them the frame and its flag words are the slot, byte for byte: no staging
        static_assert(SLAB_FLAG_WORDS == DELIVER_TRAILER_WORDS, "the gathered frame's flag words are the delivered frame's trailer");
        payload = frame8;
    }
    // 2. the plane behind it, and THE trailer behind the plane (the one step 1 wrote lies under the padding and the plane)
    if (depth && group) {   // (no pass: gsr_allgather_frame_async ran it for the frame it gathered)
        const gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
        launch_deliver_gathered_depth(dx.plane, (uint32_t)((dx.plane_bytes() + 3) / 4), staging, dl.depth_offset(), dl.trailer_offset(), c->W, c->H, k, flag, work);
    } else if (depth) {     // the frame's pass into the ring's plane, then the plane into the slot
        gsr_ctx::Delivery::DepthPlane& dp = dl.depth;
        if (int r = depth_enqueue(c, dp.planes, dp.spec.step, DEPTH_FILL_HIT)) return r;
        launch_deliver_depth(dp.spec.format, dp.planes.hit, staging, dl.depth_offset(), dl.trailer_offset(), dp.planes.Wd, dp.planes.Hd, dp.spec.near, c->W, c->H, k,
                             flag, work);
    }
    // 3. the slot's one copy to the host, and `done` behind it
    if (e == hipSuccess && payload == staging) e = hipGetLastError();   // (nothing was launched for a frame that goes as it is)
    if (e == hipSuccess && copy != work) e = hipEventRecord(dl.ev_staged, work);
    if (e == hipSuccess && copy != work) e = hipStreamWaitEvent(copy, dl.ev_staged, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(sl->host, payload, bytes, hipMemcpyDeviceToHost, copy);
    if (e == hipSuccess) e = hipEventRecord(sl->done, copy);
    if (e != hipSuccess)   // (the slot was never marked taken: it is still on the free list)
        return fail(c, GSR_ERR_HIP, "gsr_deliver_frame_async: frame %llu: %s", (unsigned long long)k, hipGetErrorString(e));
    sl->serial = dl.serial = k;
    sl->state = DeliverySlot::IN_FLIGHT;
    dl.next = (int)(sl - dl.ring.data() + 1) % slots;
    if (serial) *serial = k;
    return GSR_OK;
}

int gsr_frame_ready(gsr_ctx* c, uint64_t serial)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_frame_ready: no delivery ring (gsr_delivery_open)");
    if (serial && find_slot(c, serial, DeliverySlot::HELD)) return 1;
    DeliverySlot* sl = find_slot(c, serial, DeliverySlot::IN_FLIGHT);
    if (!sl) return fail(c, GSR_ERR_ARG, "gsr_frame_ready: frame %llu is not in the ring", (unsigned long long)serial);
    const hipError_t e = hipEventQuery(sl->done);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return fail(c, GSR_ERR_HIP, "gsr_frame_ready: frame %llu: %s", (unsigned long long)sl->serial, hipGetErrorString(e));
}

int gsr_acquire_frame(gsr_ctx* c, uint64_t serial, gsr_frame* out)
{
    if (!c) return GSR_ERR_ARG;
    if (!out) return fail(c, GSR_ERR_ARG, "gsr_acquire_frame: out is NULL");
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_acquire_frame: no delivery ring (gsr_delivery_open)");
    DeliverySlot* sl = find_slot(c, serial, DeliverySlot::IN_FLIGHT);
    if (!sl) return fail(c, GSR_ERR_ARG, serial ? "gsr_acquire_frame: frame %llu is not in flight" : "gsr_acquire_frame: no frame is in flight", (unsigned long long)serial);
    // this frame's copy only: the frames enqueued behind it keep running
    const hipError_t e = hipEventSynchronize(sl->done);
    if (e != hipSuccess) {
        sl->state = DeliverySlot::FREE;
        return fail(c, GSR_ERR_HIP, "gsr_acquire_frame: frame %llu: %s", (unsigned long long)sl->serial, hipGetErrorString(e));
    }
    uint32_t flag;   // the frame's overflow word; in a group: the ranks whose band is stale
    memcpy(&flag, sl->host + c->delivery.trailer_offset(), 4);
    if (flag) {
        sl->state = DeliverySlot::FREE;
        return fail(c, GSR_ERR_OVERFLOW, "delivered frame %llu was not composited (flags 0x%x): its bin lists did not fit and the framebuffer kept "
                                         "the preceding image; the slot is free again, render and deliver that pose again (gsr_render_async regrows the lists)",
                    (unsigned long long)sl->serial, flag);
    }
    sl->state = DeliverySlot::HELD;
    out->pixels = sl->host;
    out->width = c->delivery.W; out->height = c->delivery.H;
    out->slot = (int32_t)(sl - c->delivery.ring.data());
    out->serial = sl->serial;
    return GSR_OK;
}

int gsr_release_frame(gsr_ctx* c, uint64_t serial)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_release_frame: no delivery ring (gsr_delivery_open)");
    DeliverySlot* sl = serial ? find_slot(c, serial, DeliverySlot::HELD) : nullptr;
    if (!sl) return fail(c, GSR_ERR_ARG, "gsr_release_frame: frame %llu is not held", (unsigned long long)serial);
    sl->state = DeliverySlot::FREE;
    return GSR_OK;
}

void* gsr_delivery_slot_ptr(gsr_ctx* c, int32_t slot, uint64_t* bytes)
{
    if (bytes) *bytes = 0;
    if (!c || slot < 0 || (size_t)slot >= c->delivery.ring.size()) return nullptr;
    if (bytes) *bytes = c->delivery.pixel_bytes();
    return c->delivery.ring[(size_t)slot].host;
}

}  // extern "C"
