// ---------------------------------------------------------------------------------------------------------
// Multi-GPU: the framebuffer all-gather of SURVEY 8(e), issued by the library itself.  One process per GPU; every
// rank renders its band of tile columns and the RGBA8 slabs are exchanged with ONE ncclAllGather over xGMI (RCCL),
// so the per-frame path needs no Python and no torch: renderer.render(scene, camera) on a Node host returns the full
// frame.  RCCL is opened at run time (dlopen "librccl.so.1": in a process that already holds one -- a torch build
// bundles its own -- the loader hands back that copy, so a process never ends up with two), which also keeps
// libgsplat_hip.so loadable on single-GPU hosts without RCCL installed.
// ---------------------------------------------------------------------------------------------------------
#include "gsr_ctx.h"

#include <dlfcn.h>
// RCCL: types and constants only -- the entry points are resolved with dlsym (gsr_comm_*), so the library loads on hosts
// without RCCL; and it BUILDS without the header too: the handful of declarations the calls need are repeated here
// (ABI of rccl.h / nccl.h 2.x: an opaque communicator pointer, a 128-byte id, enum values 0 = success, 1 = uint8).
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct { char internal[NCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclUint8 = 1 } ncclDataType_t;
#endif

#include <cstring>
#include <mutex>

using namespace gsr;

namespace {

struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
    bool ok = false;
};

RcclApi& rccl()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (!h) { api.error = std::string("RCCL is not available: ") + dlerror(); return; }
        api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
        api.AllGather = (decltype(api.AllGather))dlsym(h, "ncclAllGather");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather && api.GetErrorString;
        if (!api.ok) api.error = "librccl.so lacks an expected entry point";
    });
    return api;
}

#define RCCL_TRY(c, expr)                                                                              \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess) return fail((c), GSR_ERR_COMM, "%s failed: %s", #expr, rccl().GetErrorString(r_)); \
    } while (0)

}  // namespace

void gsr::comm_release(gsr_ctx* c)
{
    // A leader that leaves the group (or is destroyed) before the contexts that borrowed its communicator and exchange stream:
    // they are detached first, while both still exist -- afterwards they are plain contexts that have to join again, instead of
    // holders of a destroyed stream (a garbage-collected host destroys contexts in any order).
    while (!c->comm.followers.empty()) comm_release(c->comm.followers.back());
    if (c->comm.leader) {
        auto& fl = c->comm.leader->comm.followers;
        fl.erase(std::remove(fl.begin(), fl.end(), c), fl.end());
        c->comm.leader = nullptr;
    }
    if (c->comm.stream) (void)hipStreamSynchronize(c->comm.stream);
    if (c->comm.nccl && c->comm.owned && rccl().ok) (void)rccl().CommDestroy(c->comm.nccl);
    c->comm.nccl = nullptr;
    c->comm.fn = nullptr; c->comm.fn_user = nullptr;
    if (c->comm.ev_packed) (void)hipEventDestroy(c->comm.ev_packed);
    if (c->comm.ev_slab_free) (void)hipEventDestroy(c->comm.ev_slab_free);
    c->comm.ev_packed = c->comm.ev_slab_free = nullptr;
    if (c->comm.stream && c->comm.owned) (void)hipStreamDestroy(c->comm.stream);
    c->comm.stream = nullptr;
    c->comm.owned = true;
    c->comm.slab.reset(); c->comm.gathered.reset(); c->comm.frame8.reset();
    c->comm.depth.reset();   // (the option belongs to the group's contract: it goes with the group)
    c->comm.world = 0; c->comm.frame8_valid = false;
}

// the slab and the gathered slabs at the size the group's contract gives them now (colour, flag words and, after
// gsr_comm_set_depth, the depth section); the caller has waited for both streams
static int alloc_slabs(gsr_ctx* c, int world)
{
    const size_t words = c->comm.slab_bytes(c->H) / 4;
    int r;
    if ((r = c->comm.slab.alloc(c, words)) || (r = c->comm.gathered.alloc(c, words * world))) return r;
    HIP_TRY(c, hipMemsetAsync(c->comm.slab, 0, words * 4, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

extern "C" {

int gsr_comm_unique_id(uint8_t* id)
{
    if (!id) return GSR_ERR_ARG;
    static_assert(GSR_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "the id is passed through as bytes");
    if (!rccl().ok) return fail(nullptr, GSR_ERR_COMM, "%s", rccl().error.c_str());
    ncclUniqueId u;
    const ncclResult_t r = rccl().GetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, GSR_ERR_COMM, "ncclGetUniqueId failed: %s", rccl().GetErrorString(r));
    memcpy(id, u.internal, GSR_COMM_ID_BYTES);
    return GSR_OK;
}

// everything of gsr_comm_init but the communicator: argument checks, the context's band, slab / gathered / frame buffers,
// the exchange stream (its own, or `shared_stream`) and the two ordering events
static int comm_setup(gsr_ctx* c, const char* who, int32_t rank, int32_t world, const int32_t* x0, const int32_t* x1, hipStream_t shared_stream)
{
    if (!x0 || !x1 || world < 1 || world > MAX_SLABS || rank < 0 || rank >= world)
        return fail(c, GSR_ERR_ARG, "%s: bad argument (1 <= world <= %d, 0 <= rank < world)", who, MAX_SLABS);
    if (!c->W || !c->H) return fail(c, GSR_ERR_ARG, "%s: set the framebuffer size first", who);
    int sw = BIN_PX;
    for (int q = 0; q < world; q++) {
        // every rank must hold the same edges: whole 32-px bin columns, contiguous, covering the image
        const int want0 = q ? x1[q - 1] : 0;
        if (x0[q] != want0 || x1[q] <= x0[q] || x0[q] % BIN_PX || (x1[q] % BIN_PX && x1[q] != c->W) || x1[q] > c->W)
            return fail(c, GSR_ERR_ARG, "%s: band %d = [%d,%d) (bands are contiguous runs of whole %d-px columns)", who, q, x0[q], x1[q], BIN_PX);
        sw = std::max(sw, x1[q] - x0[q]);
    }
    if (x1[world - 1] != c->W) return fail(c, GSR_ERR_ARG, "%s: the bands end at %d, the image is %d wide", who, x1[world - 1], c->W);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    comm_release(c);
    if (int r = gsr_set_band(c, world == 1 ? 0 : x0[rank], world == 1 ? 0 : x1[rank])) return r;
    c->comm.slab_w = sw;
    for (int q = 0; q < world; q++) { c->comm.edges.x0[q] = x0[q]; c->comm.edges.x1[q] = x1[q]; }
    // (a slab = the band's pixels + SLAB_FLAG_WORDS words "this band was not composited"; the assembled frame is followed by
    //  the word that collects those flags: k_pack_band_rgba8 / k_unpack_slabs_rgba8)
    int r;
    if ((r = alloc_slabs(c, world)) || (r = c->comm.frame8.alloc(c, (size_t)c->W * c->H + SLAB_FLAG_WORDS))) return r;
    if (shared_stream) { c->comm.stream = shared_stream; c->comm.owned = false; }
    else HIP_TRY(c, hipStreamCreateWithFlags(&c->comm.stream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->comm.ev_packed, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->comm.ev_slab_free, hipEventDisableTiming));
    c->comm.rank = rank; c->comm.world = world;
    return GSR_OK;
}

int gsr_comm_init(gsr_ctx* c, const uint8_t* id, int32_t rank, int32_t world, const int32_t* x0, const int32_t* x1)
{
    if (!c) return GSR_ERR_ARG;
    if (!id) return fail(c, GSR_ERR_ARG, "gsr_comm_init: id is NULL");
    if (!rccl().ok) return fail(c, GSR_ERR_COMM, "%s", rccl().error.c_str());
    if (int r = comm_setup(c, "gsr_comm_init", rank, world, x0, x1, nullptr)) return r;
    ncclUniqueId u;
    memcpy(u.internal, id, GSR_COMM_ID_BYTES);
    const ncclResult_t nr = rccl().CommInitRank(&c->comm.nccl, world, u, rank);   // collective: returns when every rank has joined
    if (nr != ncclSuccess) {
        c->comm.nccl = nullptr;
        comm_release(c);
        return fail(c, GSR_ERR_COMM, "ncclCommInitRank failed: %s", rccl().GetErrorString(nr));
    }
    return GSR_OK;
}

int gsr_comm_share(gsr_ctx* c, gsr_ctx* leader)
{
    if (!c || !leader) return GSR_ERR_ARG;
    if (c == leader || !leader->comm.joined() || !leader->comm.owned)
        return fail(c, GSR_ERR_ARG, "gsr_comm_share: the other context must have joined a group itself (gsr_comm_init)");
    if (c->device != leader->device || c->W != leader->W || c->H != leader->H)
        return fail(c, GSR_ERR_ARG, "gsr_comm_share: both contexts must be on one device and of one size");
    if (int r = comm_setup(c, "gsr_comm_share", leader->comm.rank, leader->comm.world, leader->comm.edges.x0, leader->comm.edges.x1, leader->comm.stream))
        return r;
    c->comm.nccl = leader->comm.nccl; c->comm.fn = leader->comm.fn; c->comm.fn_user = leader->comm.fn_user;
    c->comm.leader = leader;
    leader->comm.followers.push_back(c);
    return GSR_OK;
}

int gsr_comm_init_custom(gsr_ctx* c, int32_t rank, int32_t world, const int32_t* x0, const int32_t* x1, gsr_allgather_fn fn, void* user)
{
    if (!c) return GSR_ERR_ARG;
    if (!fn) return fail(c, GSR_ERR_ARG, "gsr_comm_init_custom: fn is NULL");
    if (int r = comm_setup(c, "gsr_comm_init_custom", rank, world, x0, x1, nullptr)) return r;
    c->comm.fn = fn; c->comm.fn_user = user;
    return GSR_OK;
}

int gsr_comm_destroy(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    comm_release(c);
    return GSR_OK;
}

int gsr_allgather_frame_async(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    if (!c->comm.joined()) return fail(c, GSR_ERR_ARG, "gsr_allgather_frame_async: gsr_comm_init has not been called");
    if (!c->have_frame) return fail(c, GSR_ERR_ARG, "gsr_allgather_frame_async: nothing rendered yet");
    gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
    // with depth the frame's lists are walked once more: what gsr_depth_async needs of the frame, refused before anything is enqueued
    if (dx.on()) {
        if (dx.W != c->W || dx.H != c->H)
            return fail(c, GSR_ERR_ARG, "gsr_allgather_frame_async: the size changed since gsr_comm_set_depth (%dx%d, now %dx%d): join the group again", dx.W, dx.H, c->W, c->H);
        if (int r = depth_frame_check(c, "gsr_allgather_frame_async (depth exchange)")) return r;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // never ship a band the compositor did not draw: if the device has reported a list overflow, regrow and render
    // the frame again first (lost earlier frames stay counted and are reported by the next gsr_sync)
    if (overflow_pending(c)) {
        if (int r = sync_and_repair(c)) return r;
        if (dx.on()) { if (int r = depth_frame_check(c, "gsr_allgather_frame_async (depth exchange)")) return r; }   // (a regrowth may have taken the lists)
    }
    const BinGrid g = make_grid(c);
    const int x0 = g.bx_lo * BIN_PX, x1 = std::min(g.bx_hi * BIN_PX, c->W);
    // render stream: the previous all-gather must have read the slab before it is overwritten; then pack the band
    if (c->comm.frame8_valid) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->comm.ev_slab_free, 0));
    // (the pack also records, behind the pixels, whether the frame it packs was composited at all: the frame's overflow word,
    //  which the next frame's projection resets -- stream order puts this read in front of it)
    launch_pack_band_rgba8(c->out.fb, c->comm.slab, c->W, c->H, x0, x1, c->comm.slab_w, c->stream, &c->words.fstate->overflow);
    if (dx.on()) {
        // the frame's hit plane on this rank's bin columns (the pass of a depth ring, the same hit_alpha rule), then the band's samples
        // into the slab's depth section.  A frame whose lists did not fit leaves the plane as it was: the slab's flag says so.
        // Only this rank's bin columns are written and only they are packed, so nothing is filled beside them.
        if (int r = depth_enqueue(c, dx.planes, dx.spec.step, DEPTH_FILL_NOTHING)) return r;
        launch_pack_band_depth(dx.spec.format, dx.planes.hit, reinterpret_cast<uint8_t*>(c->comm.slab.p) + dx.offset, dx.planes.Wd, dx.planes.Hd,
                               dx.edges.x0[c->comm.rank], dx.edges.x1[c->comm.rank], dx.stride, dx.spec.near, c->stream);
    }
    HIP_TRY(c, hipEventRecord(c->comm.ev_packed, c->stream));
    // exchange stream: collective + de-slab, overlapping the next frame's kernels on the render stream
    HIP_TRY(c, hipStreamWaitEvent(c->comm.stream, c->comm.ev_packed, 0));
    const size_t slab_bytes = c->comm.slab_bytes(c->H);
    if (c->comm.fn) {
        if (const int r = c->comm.fn(c->comm.fn_user, c->comm.slab, c->comm.gathered, (uint64_t)slab_bytes, (void*)c->comm.stream))
            return fail(c, GSR_ERR_COMM, "the custom all-gather returned %d", r);
    } else {
        RCCL_TRY(c, rccl().AllGather(c->comm.slab, c->comm.gathered, slab_bytes, ncclUint8, c->comm.nccl, c->comm.stream));
    }
    HIP_TRY(c, hipEventRecord(c->comm.ev_slab_free, c->comm.stream));
    launch_unpack_slabs_rgba8(c->comm.gathered, c->comm.frame8, c->W, c->H, c->comm.slab_w, c->comm.world, c->comm.edges, c->comm.stream,
                              c->comm.frame8 + (size_t)c->W * c->H, dx.on() ? slab_bytes / 4 : 0);
    if (dx.on())
        launch_unpack_slabs_depth(dx.spec.format, reinterpret_cast<const uint8_t*>(c->comm.gathered.p), dx.plane, dx.planes.Wd, dx.planes.Hd, slab_bytes, dx.offset,
                                  dx.stride, c->comm.world, dx.edges, c->comm.stream);
    HIP_TRY(c, hipGetLastError());
    c->comm.frame8_valid = true;
    return GSR_OK;
}

// gsr_read_frame_rgba8 / gsr_read_frame_depth: `bytes` at `src` of what the last gsr_allgather_frame_async left, unless that
// gathered frame holds a stale band
static int read_gathered(gsr_ctx* c, void* out, const void* src, size_t bytes)
{
    HIP_TRY(c, hipSetDevice(c->device));
    // A band of the gathered frame may have been packed right behind a frame whose bin lists did not fit: that frame was not
    // composited and the band is the preceding image.  WHICH gathered frame that concerns is decided on the device and seen by
    // the whole group: every slab carries its frame's overflow flag through the all-gather and the de-slab kernel collects the
    // flags of all ranks behind the assembled frame.  So every rank refuses exactly the same frame (GSR_ERR_OVERFLOW) and the
    // group renders and gathers it again together -- no rank repeats a collective alone -- while frames dropped earlier and
    // not reported yet (gsr_sync's business) do not make a good frame unreadable.  The rank that overflowed regrows its lists
    // here, so that the repeated frame fits.
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (overflow_pending(c)) { if (int r = sync_and_repair(c)) return r; }
    uint32_t stale = 0;
    HIP_TRY(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->comm.stream));
    HIP_TRY(c, hipMemcpyAsync(&stale, c->comm.frame8 + (size_t)c->W * c->H, 4, hipMemcpyDeviceToHost, c->comm.stream));
    HIP_TRY(c, hipStreamSynchronize(c->comm.stream));
    if (stale) {
        c->comm.frame8_valid = false;
        return fail(c, GSR_ERR_OVERFLOW, "the gathered frame holds a band that was not composited (the bin lists of rank mask 0x%x did not fit; "
                                         "they have been regrown there): every rank of the group gets this error for this frame and all of them "
                                         "render and gather it again", stale);
    }
    return GSR_OK;
}

int gsr_read_frame_rgba8(gsr_ctx* c, uint8_t* out)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    if (!c->comm.frame8_valid) return fail(c, GSR_ERR_ARG, "gsr_read_frame_rgba8: no gathered frame yet (gsr_allgather_frame_async)");
    return read_gathered(c, out, c->comm.frame8, (size_t)c->W * c->H * 4);
}

int gsr_comm_set_depth(gsr_ctx* c, const gsr_depth_delivery_options* depth)
{
    if (!c) return GSR_ERR_ARG;
    if (!c->comm.joined()) return fail(c, GSR_ERR_ARG, "gsr_comm_set_depth: this context is not in a group (gsr_comm_init, gsr_comm_share)");
    const DepthSpec spec = DepthSpec::from(depth);
    if (spec.on()) { if (int r = depth_options_check(c, "gsr_comm_set_depth", depth)) return r; }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->comm.stream));
    gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
    dx.reset();
    c->comm.frame8_valid = false;   // the slabs change: what was gathered under the old contract is gone
    if (spec.on()) {
        const int st = spec.step, world = c->comm.world;
        int r = dx.planes.alloc(c, c->W, c->H, st);   // (first: the layout below is in its Wd, Hd)
        dx.spec = spec;
        dx.W = c->W; dx.H = c->H;
        // band edges are multiples of 32 (the last may be the image's width): x0 / step is exact, the bands are disjoint and cover Wd
        for (int q = 0; q < world; q++) { dx.edges.x0[q] = c->comm.edges.x0[q] / st; dx.edges.x1[q] = (c->comm.edges.x1[q] + st - 1) / st; }
        dx.stride = ((c->comm.slab_w + st - 1) / st + 7) & ~7;
        dx.offset = ((((size_t)c->comm.slab_w * c->H + SLAB_FLAG_WORDS) * 4) + 15) & ~(size_t)15;
        dx.slab_bytes = dx.offset + (size_t)dx.planes.Hd * dx.stride * spec.sample_bytes();
        const size_t plane_words = (dx.plane_bytes() + 15) / 16 * 4;
        if (!r) r = dx.plane.alloc(c, plane_words);
        if (!r) r = alloc_slabs(c, world);
        if (r) { dx.reset(); (void)alloc_slabs(c, world); return r; }   // (colour only again)
        // (a frame that never fits leaves the plane unwritten: +infinity rather than whatever the allocation held)
        HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)dx.planes.hit.p, 0x7f800000, (size_t)dx.planes.Wd * dx.planes.Hd, c->stream));
        HIP_TRY(c, hipMemsetAsync(dx.plane, 0, plane_words * 4, c->stream));
        return GSR_OK;
    }
    return alloc_slabs(c, c->comm.world);
}

int gsr_frame_depth_layout(gsr_ctx* c, gsr_depth_layout* out)
{
    if (!c) return GSR_ERR_ARG;
    if (!out) return fail(c, GSR_ERR_ARG, "gsr_frame_depth_layout: out is NULL");
    const gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
    if (!c->comm.joined() || !dx.on()) return fail(c, GSR_ERR_ARG, "gsr_frame_depth_layout: this context exchanges no depth (gsr_comm_set_depth)");
    *out = dx.spec.layout(dx.planes.Wd, dx.planes.Hd, 0);
    return GSR_OK;
}

int gsr_read_frame_depth(gsr_ctx* c, void* out, uint64_t out_bytes)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    const gsr_ctx::Comm::DepthExchange& dx = c->comm.depth;
    if (!c->comm.joined() || !dx.on()) return fail(c, GSR_ERR_ARG, "gsr_read_frame_depth: this context exchanges no depth (gsr_comm_set_depth)");
    if (!c->comm.frame8_valid) return fail(c, GSR_ERR_ARG, "gsr_read_frame_depth: no gathered frame yet (gsr_allgather_frame_async)");
    if (out_bytes < dx.plane_bytes())
        return fail(c, GSR_ERR_ARG, "gsr_read_frame_depth: %llu bytes, the plane has %zu", (unsigned long long)out_bytes, dx.plane_bytes());
    return read_gathered(c, out, dx.plane, dx.plane_bytes());
}

void* gsr_frame_depth_device_ptr(gsr_ctx* c) { return c && c->comm.depth.on() ? (void*)c->comm.depth.plane : nullptr; }
void* gsr_frame8_device_ptr(gsr_ctx* c) { return c ? (void*)c->comm.frame8 : nullptr; }
void* gsr_comm_stream_handle(gsr_ctx* c) { return c ? (void*)c->comm.stream : nullptr; }

}  // extern "C"
