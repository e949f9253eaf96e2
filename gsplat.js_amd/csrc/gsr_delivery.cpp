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

// the payload of one frame in the ring's format, and where the trailer lies behind it
static inline size_t ring_pixel_bytes(const gsr_ctx* c)
{
    const gsr_ctx::Delivery& d = c->delivery;
    return d.format == GSR_FORMAT_RGBA8 ? (size_t)d.W * d.H * 4 : yuv420_bytes(d.W, d.H);
}
// a depth ring: the plane behind the payload at the next multiple of 16, the trailer behind the plane at the next multiple of 16
static inline bool ring_has_depth(const gsr_ctx* c) { return c->delivery.depth.format != GSR_DEPTH_NONE; }
static inline size_t ring_depth_offset(const gsr_ctx* c) { return (ring_pixel_bytes(c) + 15) & ~(size_t)15; }
static inline size_t ring_depth_stride(const gsr_ctx* c) { return (size_t)c->delivery.depth.Wd * (c->delivery.depth.format == GSR_DEPTH_U16 ? 2 : 4); }
static inline size_t ring_depth_bytes(const gsr_ctx* c) { return ring_depth_stride(c) * c->delivery.depth.Hd; }
static inline size_t ring_trailer_offset(const gsr_ctx* c)
{
    if (ring_has_depth(c)) return (ring_depth_offset(c) + ring_depth_bytes(c) + 15) & ~(size_t)15;
    return (ring_pixel_bytes(c) + 3) & ~(size_t)3;
}
static inline size_t ring_slot_bytes(const gsr_ctx* c) { return ring_trailer_offset(c) + DELIVER_TRAILER_WORDS * 4; }

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
    gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;   // (format, step and near stay: gsr_resize reallocates for them)
    dp.hit.reset(); dp.mean.reset(); dp.index.reset(); dp.invalid.reset();
    dp.Wd = dp.Hd = 0;
    std::fill(dp.fill_key, dp.fill_key + 4, 0);
}

// (re)allocates the ring for the context's current size; frames in flight are waited for and dropped
int gsr::delivery_alloc(gsr_ctx* c, int slots)
{
    delivery_free(c);
    c->delivery.W = c->W; c->delivery.H = c->H;
    gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;
    if (ring_has_depth(c)) { dp.Wd = (c->W + dp.step - 1) / dp.step; dp.Hd = (c->H + dp.step - 1) / dp.step; }
    const size_t bytes = ring_slot_bytes(c);
    auto bail = [c](int code) { delivery_free(c); return code; };
    if (ring_has_depth(c)) {
        // the pass's own plane(s): the hit plane k_deliver_depth reads; at step 1 the full pass also writes mean and index
        const size_t np = (size_t)dp.Wd * dp.Hd;
        int r = dp.hit.alloc(c, np);
        if (!r && dp.step == 1) { r = dp.mean.alloc(c, np); if (!r) r = dp.index.alloc(c, np); }
        if (!r) r = dp.invalid.alloc(c, 1);
        if (r) return bail(r);
    }
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

// a depth ring on a context whose group exchanges depth: format, step and near must be the exchange's (GSR_ERR_ARG names the first that is not)
static int exchange_mismatch(gsr_ctx* c, const char* who, int format, int step, float near)
{
    const gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
    if (format != dx.format)
        return fail(c, GSR_ERR_ARG, "%s: the ring's depth format (%d) is not the one the group exchanges (%d, gsr_comm_set_depth)", who, format, dx.format);
    if (step != dx.step) return fail(c, GSR_ERR_ARG, "%s: the ring's depth step (%d) is not the one the group exchanges (%d, gsr_comm_set_depth)", who, step, dx.step);
    if (c->W != dx.W || c->H != dx.H) return fail(c, GSR_ERR_ARG, "%s: the size changed since gsr_comm_set_depth: join the group again", who);
    if (near != dx.near)
        return fail(c, GSR_ERR_ARG, "%s: the ring's depth near (%g) is not the one the group exchanges (%g, gsr_comm_set_depth)", who, (double)near, (double)dx.near);
    return GSR_OK;
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
    c->delivery.depth.format = GSR_DEPTH_NONE;
    return delivery_alloc(c, slots);
}

// gsr_delivery_open_ex, and with `depth` gsr_delivery_open_depth: nothing of the context changes unless every argument is accepted
static int delivery_open_options(gsr_ctx* c, const char* who, const gsr_delivery_options* opt, const gsr_depth_delivery_options* depth)
{
    if (!opt) return fail(c, GSR_ERR_ARG, "%s: options are NULL", who);
    if (opt->format != GSR_FORMAT_RGBA8 && opt->format != GSR_FORMAT_NV12 && opt->format != GSR_FORMAT_I420)
        return fail(c, GSR_ERR_ARG, "%s: unknown format %d (GSR_FORMAT_RGBA8, GSR_FORMAT_NV12, GSR_FORMAT_I420)", who, opt->format);
    if (depth) {
        if (int r = depth_options_check(c, who, depth)) return r;
        if (c->comm.joined() && !c->comm.depth.on())
            return fail(c, GSR_ERR_ARG, "%s: this context is in a group: depth is not exchanged between ranks, so a gathered frame has no depth plane to deliver", who);
        // a group that exchanges depth (gsr_comm_set_depth) delivers the gathered plane as it is: the ring's options must be the exchange's
        if (c->comm.joined()) { if (int r = exchange_mismatch(c, who, depth->format, depth->step, depth->format == GSR_DEPTH_U16 ? depth->near : 0.0f)) return r; }
    }
    if (!c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "%s: a delivery ring is open (gsr_delivery_close first)", who);
    if (int r = delivery_open_checked(c, who, opt->slots)) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    c->delivery.format = opt->format;
    c->delivery.yuv = yuv_params(opt->full_range != 0, opt->background);
    gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;
    dp.format = depth ? depth->format : GSR_DEPTH_NONE;
    dp.step = depth ? depth->step : 1;
    dp.near = depth && depth->format == GSR_DEPTH_U16 ? depth->near : 0.0f;
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
    return delivery_open_options(c, "gsr_delivery_open_depth", opt, depth && depth->format != GSR_DEPTH_NONE ? depth : nullptr);
}

int gsr_delivery_depth_layout(gsr_ctx* c, gsr_depth_layout* out)
{
    if (!c) return GSR_ERR_ARG;
    if (!out) return fail(c, GSR_ERR_ARG, "gsr_delivery_depth_layout: out is NULL");
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_delivery_depth_layout: no delivery ring (gsr_delivery_open_depth)");
    if (!ring_has_depth(c)) return fail(c, GSR_ERR_ARG, "gsr_delivery_depth_layout: the ring was opened without a depth plane (gsr_delivery_open_depth)");
    const gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;
    *out = gsr_depth_layout{};
    out->format = dp.format; out->step = dp.step; out->width = dp.Wd; out->height = dp.Hd;
    out->stride = (int32_t)ring_depth_stride(c);
    out->offset = ring_depth_offset(c);
    out->bytes = ring_depth_bytes(c);
    out->near = dp.near;
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
    out->bytes = ring_pixel_bytes(c);
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
    c->delivery.depth.format = GSR_DEPTH_NONE;
    return GSR_OK;
}

int gsr_deliver_frame_async(gsr_ctx* c, uint64_t* serial)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: no delivery ring (gsr_delivery_open)");
    const bool group = c->comm.joined();
    const bool depth = ring_has_depth(c);
    if (depth && group && !c->comm.depth.on())   // (refused before anything else is looked at: nothing enqueued, no slot taken)
        return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: this context joined a group after it opened a depth ring: depth is not exchanged "
                                    "between ranks, so a gathered frame has no depth plane to deliver (gsr_delivery_close, then a ring without depth)");
    if (depth && group) {   // the group exchanges depth: the gathered plane is delivered as it is, so the ring must have been opened for it
        const gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;
        if (int r = exchange_mismatch(c, "gsr_deliver_frame_async", dp.format, dp.step, dp.near)) return r;
        if (dp.Wd != c->comm.depth.Wd || dp.Hd != c->comm.depth.Hd)
            return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: the size changed since gsr_comm_set_depth: join the group again");
    }
    if (group ? !c->comm.frame8_valid : !c->have_frame)
        return fail(c, GSR_ERR_ARG, group ? "gsr_deliver_frame_async: no gathered frame yet (gsr_allgather_frame_async)" : "gsr_deliver_frame_async: nothing rendered yet");
    // a depth ring needs what gsr_depth_async needs of the frame; refused before a slot is looked for: nothing enqueued, no slot taken
    // (in a group the pass ran with the exchange: gsr_allgather_frame_async has asked the same of the frame it gathered)
    if (depth && !group) { if (int r = delivery_depth_check(c, "gsr_deliver_frame_async (depth ring)")) return r; }
    DeliverySlot* sl = nullptr;
    const int slots = (int)c->delivery.ring.size();
    for (int k = 0; k < slots && !sl; k++) {
        DeliverySlot& cand = c->delivery.ring[(size_t)((c->delivery.next + k) % slots)];
        if (cand.state == DeliverySlot::FREE) sl = &cand;
    }
    if (!sl) return fail(c, GSR_ERR_BUSY, "gsr_deliver_frame_async: all %d delivery slots are in flight or held (gsr_acquire_frame / gsr_release_frame)", slots);
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t k = c->delivery.serial + 1;
    const size_t bytes = ring_slot_bytes(c);
    const bool yuv = c->delivery.format != GSR_FORMAT_RGBA8;
    hipError_t e;
    if (group && depth) {
        // exchange stream, behind the de-slab steps and in front of the next ones: the gathered colour into the slot's staging (a plain
        // copy, or the conversion), the gathered plane as it is behind it with THE trailer (the stale mask its first word), then the
        // slot's one copy to the host.  No depth pass: gsr_allgather_frame_async ran it for the frame it gathered.
        const gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
        const uint32_t* stale = c->comm.frame8 + (size_t)c->W * c->H;
        e = hipSuccess;
        if (yuv)
            launch_deliver_yuv(c->delivery.format, nullptr, c->comm.frame8, reinterpret_cast<uint8_t*>(sl->staging.p), bytes, c->W, c->H, c->delivery.yuv, k, stale,
                               c->comm.stream);
        else
            e = hipMemcpyAsync(sl->staging, c->comm.frame8, (size_t)c->W * c->H * 4, hipMemcpyDeviceToDevice, c->comm.stream);
        launch_deliver_gathered_depth(dx.plane, (uint32_t)((dx.plane_bytes() + 3) / 4), reinterpret_cast<uint8_t*>(sl->staging.p), ring_depth_offset(c),
                                      ring_trailer_offset(c), c->W, c->H, k, stale, c->comm.stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(sl->host, sl->staging, bytes, hipMemcpyDeviceToHost, c->comm.stream);
        if (e == hipSuccess) e = hipEventRecord(sl->done, c->comm.stream);
    } else if (group && yuv) {
        // exchange stream, where the plain copy of an RGBA8 ring sits: the conversion reads the gathered frame behind its de-slab
        // kernel and in front of the next one (its stale mask becomes the trailer's first word), the copy follows it there
        launch_deliver_yuv(c->delivery.format, nullptr, c->comm.frame8, reinterpret_cast<uint8_t*>(sl->staging.p), bytes, c->W, c->H, c->delivery.yuv, k,
                           c->comm.frame8 + (size_t)c->W * c->H, c->comm.stream);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(sl->host, sl->staging, bytes, hipMemcpyDeviceToHost, c->comm.stream);
        if (e == hipSuccess) e = hipEventRecord(sl->done, c->comm.stream);
    } else if (group) {
        // the gathered frame and the word behind it (one bit per rank whose band is stale) are what k_unpack_slabs_rgba8 left on the
        // exchange stream; the copy goes behind it there, in front of the next frame's de-slab
        static_assert(SLAB_FLAG_WORDS == DELIVER_TRAILER_WORDS, "the gathered frame's flag words are the delivered frame's trailer");
        e = hipMemcpyAsync(sl->host, c->comm.frame8, bytes, hipMemcpyDeviceToHost, c->comm.stream);
        if (e == hipSuccess) e = hipEventRecord(sl->done, c->comm.stream);
    } else {
        // render stream: the conversion only (it has read fb before the next frame's compositor starts); copy stream: the copy
        if (yuv)
            launch_deliver_yuv(c->delivery.format, c->out.fb, nullptr, reinterpret_cast<uint8_t*>(sl->staging.p), bytes, c->W, c->H, c->delivery.yuv, k,
                               &c->words.fstate->overflow, c->stream);
        else
            launch_deliver_rgba8(c->out.fb, sl->staging, c->W, c->H, k, &c->words.fstate->overflow, c->stream);
        if (depth) {
            // behind the conversion, in front of ev_staged: the frame's depth pass into the ring's plane, then the plane into the slot and
            // THE trailer behind it (the one the conversion wrote at the end of the colour payload lies under the padding and the plane).
            // The next frame's chain follows on this stream, so lists, records and the ring's plane are read before they are overwritten.
            const gsr_ctx::Delivery::DepthPlane& dp = c->delivery.depth;
            if (int r = delivery_depth_enqueue(c)) return r;
            launch_deliver_depth(dp.format, dp.hit, reinterpret_cast<uint8_t*>(sl->staging.p), ring_depth_offset(c), ring_trailer_offset(c), dp.Wd, dp.Hd,
                                 dp.near, c->W, c->H, k, &c->words.fstate->overflow, c->stream);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(c->delivery.ev_staged, c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->delivery.copy_stream, c->delivery.ev_staged, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(sl->host, sl->staging, bytes, hipMemcpyDeviceToHost, c->delivery.copy_stream);
        if (e == hipSuccess) e = hipEventRecord(sl->done, c->delivery.copy_stream);
    }
    if (e != hipSuccess)   // (the slot was never marked taken: it is still on the free list)
        return fail(c, GSR_ERR_HIP, "gsr_deliver_frame_async: frame %llu: %s", (unsigned long long)k, hipGetErrorString(e));
    sl->serial = c->delivery.serial = k;
    sl->state = DeliverySlot::IN_FLIGHT;
    c->delivery.next = (int)(sl - c->delivery.ring.data() + 1) % slots;
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
    memcpy(&flag, sl->host + ring_trailer_offset(c), 4);
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
    if (bytes) *bytes = ring_pixel_bytes(c);
    return c->delivery.ring[(size_t)slot].host;
}

}  // extern "C"
