// ---------------------------------------------------------------------------------------------------------
// Frame delivery: finished RGBA8 frames reach the host through a ring of pinned blocks while the next frames render.
// A slot is FREE, IN_FLIGHT (gsr_deliver_frame_async took it: kernel and copy are enqueued) or HELD (the host acquired it
// and reads its pixels).  It becomes FREE again only through the host -- gsr_release_frame, or a gsr_acquire_frame that
// refuses the frame -- and both come after a wait for the slot's copy: a free slot never has device work outstanding, so
// taking one needs no device-side wait on its previous use.
// ---------------------------------------------------------------------------------------------------------
#include "gsr_ctx.h"

#include <cstring>

using namespace gsr;

using DeliverySlot = gsr_ctx::Delivery::Slot;

static inline size_t ring_pixel_bytes(const gsr_ctx* c) { return (size_t)c->delivery.W * c->delivery.H * 4; }

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
}

// (re)allocates the ring for the context's current size; frames in flight are waited for and dropped
int gsr::delivery_alloc(gsr_ctx* c, int slots)
{
    delivery_free(c);
    c->delivery.W = c->W; c->delivery.H = c->H;
    const size_t bytes = ring_pixel_bytes(c) + DELIVER_TRAILER_WORDS * 4;
    auto bail = [c](int code) { delivery_free(c); return code; };
    hipError_t e = hipStreamCreateWithFlags(&c->delivery.copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->delivery.ev_staged, hipEventDisableTiming);
    c->delivery.ring.resize((size_t)slots);
    for (DeliverySlot& sl : c->delivery.ring) {
        if (e == hipSuccess) e = hipHostMalloc((void**)&sl.host, bytes, hipHostMallocDefault);
        if (e == hipSuccess && sl.staging.alloc(c, bytes / 4) != GSR_OK) e = hipErrorOutOfMemory;   // (bytes: pixels + trailer, whole words)
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

extern "C" {

int gsr_delivery_open(gsr_ctx* c, int32_t slots)
{
    if (!c) return GSR_ERR_ARG;
    if (slots < 2 || slots > 8) return fail(c, GSR_ERR_ARG, "gsr_delivery_open: %d slots (2..8)", slots);
    if (!c->W || !c->H) return fail(c, GSR_ERR_ARG, "gsr_delivery_open: set the framebuffer size first");
    if (delivery_frame_held(c)) return fail(c, GSR_ERR_ARG, "gsr_delivery_open: a delivered frame is held (gsr_release_frame first)");
    HIP_TRY(c, hipSetDevice(c->device));
    return delivery_alloc(c, slots);
}

int gsr_delivery_close(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_delivery_close: no delivery ring (gsr_delivery_open)");
    if (delivery_frame_held(c)) return fail(c, GSR_ERR_ARG, "gsr_delivery_close: a delivered frame is held (gsr_release_frame first): its pixels would be freed");
    HIP_TRY(c, hipSetDevice(c->device));
    delivery_free(c);
    return GSR_OK;
}

int gsr_deliver_frame_async(gsr_ctx* c, uint64_t* serial)
{
    if (!c) return GSR_ERR_ARG;
    if (c->delivery.ring.empty()) return fail(c, GSR_ERR_ARG, "gsr_deliver_frame_async: no delivery ring (gsr_delivery_open)");
    const bool group = c->comm.joined();
    if (group ? !c->comm.frame8_valid : !c->have_frame)
        return fail(c, GSR_ERR_ARG, group ? "gsr_deliver_frame_async: no gathered frame yet (gsr_allgather_frame_async)" : "gsr_deliver_frame_async: nothing rendered yet");
    DeliverySlot* sl = nullptr;
    const int slots = (int)c->delivery.ring.size();
    for (int k = 0; k < slots && !sl; k++) {
        DeliverySlot& cand = c->delivery.ring[(size_t)((c->delivery.next + k) % slots)];
        if (cand.state == DeliverySlot::FREE) sl = &cand;
    }
    if (!sl) return fail(c, GSR_ERR_BUSY, "gsr_deliver_frame_async: all %d delivery slots are in flight or held (gsr_acquire_frame / gsr_release_frame)", slots);
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t k = c->delivery.serial + 1;
    const size_t bytes = ring_pixel_bytes(c) + DELIVER_TRAILER_WORDS * 4;
    hipError_t e;
    if (group) {
        // the gathered frame and the word behind it (one bit per rank whose band is stale) are what k_unpack_slabs_rgba8 left on the
        // exchange stream; the copy goes behind it there, in front of the next frame's de-slab
        static_assert(SLAB_FLAG_WORDS == DELIVER_TRAILER_WORDS, "the gathered frame's flag words are the delivered frame's trailer");
        e = hipMemcpyAsync(sl->host, c->comm.frame8, bytes, hipMemcpyDeviceToHost, c->comm.stream);
        if (e == hipSuccess) e = hipEventRecord(sl->done, c->comm.stream);
    } else {
        // render stream: the conversion only (it has read fb before the next frame's compositor starts); copy stream: the copy
        launch_deliver_rgba8(c->out.fb, sl->staging, c->W, c->H, k, &c->words.fstate->overflow, c->stream);
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
    memcpy(&flag, sl->host + ring_pixel_bytes(c), 4);
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
