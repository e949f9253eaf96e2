// C ABI of libgsplat_hip.so (see include/gsplat_hip.h).  Host side only: owns
// the device buffers, enqueues the per-frame kernels on one HIP stream, and
// never touches a CPU fallback: without a usable AMD GPU every entry point
// fails with GSR_ERR_NO_DEVICE / GSR_ERR_HIP.
// This unit: a context's life, its size, band and camera, the frame entry points and their timings.  The frame itself is
// gsr_frame.cpp, the scene gsr_scene.cpp, read-backs gsr_readback.cpp, the multi-GPU exchange gsr_comm.cpp and frame
// delivery gsr_delivery.cpp; gsr_ctx.h is what they share.
#include "gsr_ctx.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace gsr;

namespace {

thread_local std::string g_create_error;

// the one place the library reads its environment (Knobs, gsr_ctx.h).  A knob that selects among kernels built for a fixed set
// of values (GSR_FRONT_WAVES) refuses anything else: `bad` then says what, and gsr_create fails with it.
Knobs read_knobs(std::string& bad)
{
    Knobs k;
    if (const char* e = getenv("GSR_NO_GRAPH")) k.graphs = atoi(e) == 0;
    if (const char* e = getenv("GSR_FUSE_COMBINE")) k.fuse_combine = atoi(e) != 0;
    if (const char* e = getenv("GSR_SATURATE")) k.saturate = atoi(e) != 0;
    if (const char* e = getenv("GSR_ITEMS_BY_SIZE")) k.items_by_size = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("GSR_LONG_ITEMS")) k.long_items = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("GSR_LONG_TAU")) k.long_tau = (uint32_t)std::max(0L, atol(e));
    if (const char* e = getenv("GSR_BIN_ROUNDS")) k.bin_rounds = std::min(64L, std::max(0L, atol(e)));
    if (const char* e = getenv("GSR_BIN_BIG")) k.bin_big = (uint32_t)std::min(2, std::max(0, atoi(e)));
    if (const char* e = getenv("GSR_BIN_TWO_LEVEL")) k.bin_two_level = atoi(e) ? 1 : 0;
    if (const char* e = getenv("GSR_RECT_CARRY")) { k.rect_carry = atoi(e) != 0; k.rect_carry_bucket = atoi(e) == 2; }
    if (const char* e = getenv("GSR_BLEND_SUB")) k.blend_sub = atoi(e) == 2 ? 2 : atoi(e) == 1 ? 1 : 0;
    if (const char* e = getenv("GSR_SORT_ORDER")) k.sort_order = !strcmp(e, "lsd") ? 0 : !strcmp(e, "bucket") ? 1 : -1;
    if (const char* e = getenv("GSR_TIMING_EVERY")) k.timing_every = (uint32_t)std::max(1L, atol(e));
    if (const char* e = getenv("GSR_CELL_GRID")) { const long v = atol(e); if (v >= 1) k.cell_grid = (uint32_t)std::min(v, 65535L); }
    if (const char* e = getenv("GSR_SEG_TARGET")) { const long v = atol(e); if (v >= 1) k.seg_target = (uint32_t)v; }
    if (const char* e = getenv("GSR_BLEND_GRID")) { const long v = atol(e); if (v >= 1) k.blend_grid = (uint32_t)v; }
    if (const char* e = getenv("GSR_SEG_LEN")) { const long v = atol(e); if (v >= 256) k.seg_len = (uint32_t)(v / 256 * 256); }
    if (const char* e = getenv("GSR_SORT_KPB")) { const long v = atol(e); if (v == 2048 || v == 4096 || v == 8192) k.sort_kpb = (uint32_t)v; }
    if (const char* e = getenv("GSR_FRONT_WAVES")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == 0 && (v == (long)FRONT_WAVES_NARROW || v == (long)FRONT_WAVES_WIDE)) k.front_waves = (uint32_t)v;
        else bad = std::string("GSR_FRONT_WAVES must be ") + std::to_string(FRONT_WAVES_NARROW) + " or " + std::to_string(FRONT_WAVES_WIDE) + ", not \"" + e + "\"";
    }
    if (const char* e = getenv("GSR_DEPTH_SKIP")) k.depth_skip = atoi(e) != 0;
    if (const char* e = getenv("GSR_OVERLAY_TRIM")) k.overlay_trim = atoi(e) != 0;
    if (const char* e = getenv("GSR_ATTR_HIST")) k.attr_hist_peel = strcmp(e, "peel") == 0;
    if (const char* e = getenv("GSR_ATTR_HIST_GRID")) k.attr_hist_grid = (uint32_t)std::min(std::max(atol(e), 0l), 65535l);
    return k;
}

int alloc_fb(gsr_ctx* c)
{
    const size_t np = (size_t)c->W * c->H;
    if (np > c->out.pixels) {
        if (int r = c->out.fb.alloc(c, np)) return r;
        if (int r = c->out.fb8.alloc(c, np)) return r;
        c->out.pixels = np;
    }
    launch_clear_fb(c->out.fb, c->W, c->H, c->stream);
    return GSR_OK;
}

}  // namespace

int gsr::fail(gsr_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) {
        c->error = buf;
        // A chain that stopped half way (a failed launch behind k_project_key, a device error) leaves the frame slots and frame
        // words as that frame had them -- partial min / max, counters -- and nothing would ever clean them: their last reader in a
        // frame (the finalize step) did not run.  The next frame starts with the one-time initialisation again.
        if (code == GSR_ERR_HIP) c->words.slots_need_init = true;
    }
    else g_create_error = buf;
    return code;
}

extern "C" {

const char* gsr_last_error(gsr_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int gsr_create(gsr_ctx** out, const gsr_options* opt)
{
    if (!out) return fail(nullptr, GSR_ERR_ARG, "out is NULL");
    *out = nullptr;
    std::string bad_knob;
    const Knobs knobs = read_knobs(bad_knob);
    if (!bad_knob.empty()) return fail(nullptr, GSR_ERR_ARG, "%s", bad_knob.c_str());
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(nullptr, GSR_ERR_NO_DEVICE, "no HIP device is visible (this library has no CPU path)");
    gsr_options o{};
    if (opt) o = *opt;
    if (o.device < 0 || o.device >= count) return fail(nullptr, GSR_ERR_ARG, "device %d out of range (%d visible)", o.device, count);
    if (o.width < 0 || o.height < 0 || o.width > 8192 || o.height > 8192) return fail(nullptr, GSR_ERR_ARG, "bad framebuffer size %dx%d (up to 8192)", o.width, o.height);
    if (!(o.early_out_eps >= 0.0f && o.early_out_eps < 1.0f)) return fail(nullptr, GSR_ERR_ARG, "early_out_eps must be in [0,1)");
    gsr_ctx* c = new gsr_ctx();
    c->device = o.device;
    c->scene = new SharedScene();
    c->scene->members.push_back(c);
    c->scene_gen = c->scene->generation;
    c->opt = o;
    c->knobs = knobs;
    c->graph.enabled = c->knobs.graphs;
    c->timing.every = c->knobs.timing_every;
    auto bail = [&](int code) {
        g_create_error = c->error;
        gsr_destroy(c);
        return code;
    };
    gsr_ctx::Words& w = c->words;
    const int r = [&]() -> int {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && cus > 0) c->cu_count = cus;
        const size_t slot_words = (size_t)3 * FRAME_SLOTS * FRAME_SLOT_WORDS;   // render frames' set, two sets of the sort-only frames
        if (int r = w.fstate.alloc(c, 1)) return r;
        if (int r = w.cam_dev.alloc(c, 1)) return r;
        if (int r = w.slots.alloc(c, slot_words)) return r;
        HIP_TRY(c, hipMemset(w.slots, 0, sizeof(int32_t) * slot_words));
        w.slots_need_init = true;   // (the first frame's enqueue launches the one-time initialisation: the stream exists by then)
        if (int r = w.accum.alloc(c, 8)) return r;
        HIP_TRY(c, hipMemset(w.accum, 0, 8 * sizeof(uint64_t)));
        HIP_TRY(c, hipHostMalloc((void**)&w.mailbox, 64, hipHostMallocMapped));
        memset(w.mailbox, 0, 64);
        reinterpret_cast<uint32_t*>(w.mailbox)[2] = 0xffffffffu;   // no frame has reported its largest bucket yet
        HIP_TRY(c, hipHostGetDevicePointer((void**)&w.mailbox_dev, w.mailbox, 0));
        HIP_TRY(c, hipHostMalloc((void**)&w.fstate_host, sizeof(FrameState), hipHostMallocDefault));
        memset(w.fstate_host, 0, sizeof(FrameState));
        w.fstate_host->minmax[0] = 0x7fffffff;            // wasm/wasm.cpp:14
        w.fstate_host->minmax[1] = (int32_t)0x80000000;   // wasm/wasm.cpp:15
        HIP_TRY(c, hipMemcpy(w.fstate, w.fstate_host, sizeof(FrameState), hipMemcpyHostToDevice));
        if (o.flags & GSR_FLAG_TIMING) {
            for (auto& set : c->timing.evring)
                for (auto& e : set) HIP_TRY(c, hipEventCreate(&e));
            c->timing.valid = true;
        }
        if (o.width && o.height) {
            if (int r = gsr_resize(c, o.width, o.height)) return r;
            if (o.band_x1 > o.band_x0) {
                if (int r = gsr_set_band(c, o.band_x0, o.band_x1)) return r;
            }
        }
        return GSR_OK;
    }();
    if (r) return bail(r);
    *out = c;
    return GSR_OK;
}

int gsr_destroy(gsr_ctx* c)
{
    if (!c) return GSR_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    comm_release(c);
    delivery_free(c);
    drop_graph(c);
    scene_release(c);   // (the last member of a scene frees it; the others keep rendering it)
    if (c->share_ev) (void)hipEventDestroy(c->share_ev);
    for (auto& set : c->timing.evring)
        for (auto& e : set) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->link_ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->nb.ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->cl.ev) if (e) (void)hipEventDestroy(e);
    if (c->knn.ev) (void)hipEventDestroy(c->knn.ev);
    for (auto& e : c->nm.ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->pl.ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->mt.ev) if (e) (void)hipEventDestroy(e);
    if (c->words.fstate_host) (void)hipHostFree(c->words.fstate_host);
    if (c->words.mailbox) (void)hipHostFree(c->words.mailbox);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;   // (the device is current and nothing is in flight: the context's device buffers are freed here)
    return GSR_OK;
}

int gsr_resize(gsr_ctx* c, int32_t w, int32_t h)
{
    if (!c) return GSR_ERR_ARG;
    if (w <= 0 || h <= 0 || w > 8192 || h > 8192) return fail(c, GSR_ERR_ARG, "bad framebuffer size %dx%d (1..8192)", w, h);
    const gsr_ctx::Delivery& dl = c->delivery;
    const bool new_ring = !dl.ring.empty() && (w != dl.W || h != dl.H);
    if (new_ring && delivery_frame_held(c))
        return fail(c, GSR_ERR_ARG, "gsr_resize: a delivered frame is held (gsr_release_frame first): its pixels would be freed");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->comm.nccl && (w != c->W || h != c->H)) comm_release(c);   // slabs and band edges belong to the old size: join again
    c->W = w; c->H = h;
    c->band_x0 = c->band_x1 = 0;
    c->have_frame = false;
    if (int r = alloc_fb(c)) return r;
    if (new_ring) { if (int r = delivery_alloc(c, (int)dl.ring.size())) return r; }
    return alloc_bins(c);
}

int gsr_set_band(gsr_ctx* c, int32_t x0, int32_t x1)
{
    if (!c) return GSR_ERR_ARG;
    if (x0 == 0 && x1 == 0) { c->band_x0 = c->band_x1 = 0; return alloc_bins(c); }
    if (x0 < 0 || x1 <= x0 || x0 % BIN_PX) return fail(c, GSR_ERR_ARG, "band [%d,%d) must start on a multiple of %d", x0, x1, BIN_PX);
    if (x1 > c->W) x1 = c->W;
    if (x0 >= c->W) return fail(c, GSR_ERR_ARG, "band starts outside the image");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->band_x0 = x0; c->band_x1 = x1;
    launch_clear_fb(c->out.fb, c->W, c->H, c->stream);
    return alloc_bins(c);
}

int gsr_set_list_capacity(gsr_ctx* c, uint32_t entries)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bin.capacity = std::max<uint32_t>(entries, 1024u);
    if (int r = c->bin.list.alloc(c, c->bin.capacity)) return r;
    return alloc_bins(c, true);
}

int gsr_set_camera(gsr_ctx* c, const float* view, const float* proj, const float* vp, float fx, float fy)
{
    if (!c) return GSR_ERR_ARG;
    if (!view || !proj || !vp) return fail(c, GSR_ERR_ARG, "matrix pointer is NULL");
    memcpy(c->cam.view, view, 64);
    memcpy(c->cam.proj, proj, 64);
    c->cam.vp2 = vp[2]; c->cam.vp6 = vp[6]; c->cam.vp10 = vp[10];
    c->cam.fx = fx; c->cam.fy = fy;
    c->have_cam = true;
    return GSR_OK;
}

int gsr_set_depth_fade(gsr_ctx* c, int32_t use_depth_fade, float depth_fade)
{
    if (!c) return GSR_ERR_ARG;
    c->cam.use_fade = use_depth_fade ? 1 : 0;
    c->cam.fade = depth_fade;
    return GSR_OK;
}

int gsr_render_async(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return enqueue_frame(c, true);
}

int gsr_sync(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = sync_and_repair(c)) return r;
    c->overlay.in_flight = false;   // (the render stream is idle: no overlay pass of this context reads the selection any more)
    if (c->comm.stream) HIP_TRY(c, hipStreamSynchronize(c->comm.stream));                 // the frame exchange, if one is in flight
    if (c->delivery.copy_stream) HIP_TRY(c, hipStreamSynchronize(c->delivery.copy_stream));   // frame deliveries in flight
    if (c->words.dropped_unreported) {
        const unsigned long long k = c->words.dropped_unreported;
        c->words.dropped_unreported = 0;
        return fail(c, GSR_ERR_OVERFLOW,
                    "%llu asynchronous frame(s) were not composited: their bin lists did not fit and later frames had already been "
                    "enqueued (the framebuffer kept the preceding image for them); the lists have been regrown, the context stays usable",
                    k);
    }
    return GSR_OK;
}

int gsr_overflow_pending(gsr_ctx* c) { return c && overflow_pending(c) ? 1 : 0; }

int gsr_render(gsr_ctx* c)
{
    if (int r = gsr_render_async(c)) return r;
    c->timing.render = true;
    return gsr_sync(c);
}

int gsr_sort(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = enqueue_frame(c, false)) return r;
    return finish_frame(c);
}

int gsr_get_timings(gsr_ctx* c, gsr_timings* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    if (c->timing.recorded) { if (int r = finish_frame(c)) return r; }
    *out = c->timing.tm;
    out->overflow_frames = c->words.overflow_frames;
    out->dropped_frames = c->words.dropped_frames;
    return GSR_OK;
}

int gsr_set_timing_interval(gsr_ctx* c, uint32_t every)
{
    if (!c || !every) return c ? fail(c, GSR_ERR_ARG, "timing interval must be >= 1") : GSR_ERR_ARG;
    c->timing.every = every;
    c->timing.frame_no = 0;
    return GSR_OK;
}

int gsr_reset_timings(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    if (c->timing.recorded) { if (int r = finish_frame(c)) return r; }
    gsr_timings& tm = c->timing.tm;
    const uint64_t v = tm.visible, b = tm.bin_entries, d = tm.tile_entries;
    tm = gsr_timings{};
    HIP_TRY(c, hipMemsetAsync(c->words.accum, 0, 4 * sizeof(uint64_t), c->stream));
    tm.visible = v; tm.bin_entries = b; tm.tile_entries = d; tm.n = c->scene->n;
    c->timing.frame_no = 0;  // the sampling restarts: the next frame carries the stage events
    return GSR_OK;
}

int gsr_device_info(gsr_ctx* c, char* name, int32_t name_len, int32_t* cus, int32_t* clock_khz)
{
    if (!c) return GSR_ERR_ARG;
    hipDeviceProp_t p;
    HIP_TRY(c, hipGetDeviceProperties(&p, c->device));
    // (the marketing name comes from libdrm's amdgpu.ids and is empty where that file is missing)
    if (name && name_len > 0) snprintf(name, (size_t)name_len, "%s (%s)", p.name[0] ? p.name : "AMD GPU", p.gcnArchName);
    if (cus) *cus = p.multiProcessorCount;
    if (clock_khz) *clock_khz = p.clockRate;
    return GSR_OK;
}

// ---- wasm `sort` drop-in (wasm/wasm.cpp:8-13; call site Worker.ts:39) ----
// Like the wasm export it keeps nothing of the caller's between calls: the positions are copied to the device on
// every call (12 bytes per splat over PCIe; a caller that sorts one scene many times uses gsr_set_scene + gsr_sort,
// which is what the renderer does).  An earlier version cached the upload by buffer address and size; JS hosts
// transform positions in place (Scene.translate/rotate/scale) and a collected Float32Array can come back at the same
// address, so that cache returned stale orders.  On failure depthIndex is zero-filled and the error goes to stderr
// (the reference's signature has no error channel).
void gsplat_sort_host(const float* viewProj, uint32_t vertexCount, const float* fBuffer, uint32_t* depthBuffer,
                      uint32_t* depthIndex, uint32_t* starts, uint32_t* counts)
{
    (void)starts; (void)counts;
    static std::mutex mu;
    static gsr_ctx* ctx = nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto failed = [&](const char* what) {
        fprintf(stderr, "gsplat_sort_host: %s\n", what);
        if (depthIndex && vertexCount) memset(depthIndex, 0, (size_t)vertexCount * sizeof(uint32_t));
    };
    if (!viewProj || !depthIndex || (vertexCount && !fBuffer)) return failed("NULL argument");
    if (!ctx) {
        gsr_options o{};
        if (gsr_create(&ctx, &o) != GSR_OK) { ctx = nullptr; return failed(gsr_last_error(nullptr)); }
    }
    gsr_ctx* c = ctx;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return failed("device unavailable");
    if (vertexCount != c->scene->n || !c->scene->arr.px) {
        if (vertexCount > 0x7fffffffu / 8) return failed("too many splats");
        if (alloc_scene(c, vertexCount, false) != GSR_OK) return failed(gsr_last_error(c));
        c->scene->n = vertexCount;
    }
    c->have_sort = false; c->have_frame = false;
    // What the call keeps between calls is memory of its own, never the caller's data: the device staging buffer for the
    // xyz-interleaved positions lives in the process-wide context and grows with the largest scene seen (round 3 allocated and
    // freed it on every call: two driver round trips of ~0.1 ms each beside a 45 us sort).  The chain of a call: pageable H2D of
    // 12 N bytes -> repack to the SoA the key kernel reads -> key + min/max -> quantise + 17-bit radix sort -> D2H of 4 N bytes
    // (+ 4 N for the keys on request), all on the context's stream, one host wait at the end.
    static DevBuf<float>& stage_pos = *new DevBuf<float>();   // (guarded by mu, like ctx; like ctx never destroyed: no device call at exit)
    static size_t stage_cap = 0;
    if (vertexCount) {
        if ((size_t)vertexCount * 3 > stage_cap) {
            if (stage_pos.alloc(c, (size_t)vertexCount * 3) != GSR_OK) { stage_cap = 0; return failed(gsr_last_error(c)); }
            stage_cap = (size_t)vertexCount * 3;
        }
        const gsr::SceneArrays& sa = c->scene->arr;
        hipError_t e1 = hipMemcpyAsync(stage_pos, fBuffer, (size_t)vertexCount * 12, hipMemcpyHostToDevice, c->stream);
        launch_repack_positions(stage_pos, vertexCount, sa.px, sa.py, sa.pz, c->stream);
        for (hipError_t e : {e1, hipGetLastError()})
            if (e != hipSuccess) return failed(hipGetErrorString(e));
    }
    float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (gsr_set_camera(c, ident, ident, viewProj, 1.f, 1.f) != GSR_OK) return failed(gsr_last_error(c));
    if (hipSetDevice(c->device) != hipSuccess || enqueue_frame(c, false) != GSR_OK) return failed(gsr_last_error(c));
    if (vertexCount) {
        hipError_t e1 = hipMemcpyAsync(depthIndex, c->sort.depth_index, (size_t)vertexCount * 4, hipMemcpyDeviceToHost, c->stream);
        hipError_t e2 = depthBuffer ? hipMemcpyAsync(depthBuffer, c->sort.keys, (size_t)vertexCount * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
        for (hipError_t e : {e1, e2})
            if (e != hipSuccess) return failed(hipGetErrorString(e));
    }
    if (finish_frame(c) != GSR_OK) return failed(gsr_last_error(c));
}

// Identifies the device code this library was built from (a hash of the kernel sources, set by the Makefile):
// measurements taken on one build (profiles/blend_traffic.json) are not attributed to another.
const char* gsr_build_id(void)
{
#ifdef GSR_BUILD_ID
    return GSR_BUILD_ID;
#else
    return "unknown";
#endif
}

}  // extern "C"
