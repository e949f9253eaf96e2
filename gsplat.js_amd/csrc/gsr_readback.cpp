// Read-backs and raw access: the sort's and the frame's buffers copied to the host, the framebuffer as floats or RGBA8,
// device pointers and the stream for hosts that keep the pixels on the GPU, and the slab pack / unpack of a caller-run exchange.
#include "gsr_ctx.h"

#include <cstring>

using namespace gsr;

extern "C" {

int gsr_read_depth_index(gsr_ctx* c, uint32_t* out)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    if (!c->have_sort) return fail(c, GSR_ERR_ARG, "no sort has run yet");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->sort.plan.band) {  // the band's frame sorted only its survivors: the caller wants the whole permutation
        if (int r = enqueue_frame(c, false)) return r;
        if (int r = finish_frame(c)) return r;
    }
    HIP_TRY(c, hipMemcpyAsync(out, c->sort.depth_index, (size_t)c->scene->n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_read_pixels_rgba32f(gsr_ctx* c, float* out)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->out.fb, (size_t)c->W * c->H * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_read_pixels_rgba8(gsr_ctx* c, uint8_t* out)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t np = (uint32_t)c->W * (uint32_t)c->H;
    launch_to_rgba8(c->out.fb, c->out.fb8, np, c->stream);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.fb8, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_read_keys(gsr_ctx* c, uint32_t* keys, int32_t* minmax)
{
    if (!c) return GSR_ERR_ARG;
    if (!c->have_sort) return fail(c, GSR_ERR_ARG, "no sort has run yet");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->sort.plan.band) {
        if (int r = enqueue_frame(c, false)) return r;
        if (int r = finish_frame(c)) return r;
    }
    if (keys) HIP_TRY(c, hipMemcpyAsync(keys, c->sort.keys, (size_t)c->scene->n * 4, hipMemcpyDeviceToHost, c->stream));
    if (minmax) HIP_TRY(c, hipMemcpyAsync(minmax, c->words.fstate->minmax, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_read_records(gsr_ctx* c, float* rec, int32_t* bbox)
{
    if (!c) return GSR_ERR_ARG;
    if (!c->have_frame) return fail(c, GSR_ERR_ARG, "no frame has been rendered yet");
    HIP_TRY(c, hipSetDevice(c->device));
    if (rec) HIP_TRY(c, hipMemcpyAsync(rec, c->sort.rec, (size_t)c->scene->n * 32, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint2> tmp;
    if (bbox) {
        // the pixel boxes are not part of a frame (no kernel reads them): project once more for the frame's camera, records and
        // boxes only (k_project_key, do_project == 2: the same arithmetic, so the same records)
        tmp.resize(c->scene->n);
        if (c->scene->n) {
            DevBuf<uint2> boxes;
            if (int r = boxes.alloc(c, c->scene->n)) return r;
            ProjectLaunch again{};   // (kept / kept_lane null: no packing)
            again.sc = c->scene_soa(); again.n = c->scene->n; again.cam = c->cam_frame; again.do_project = 2;
            again.depth = c->sort.depth; again.slots = c->words.slots; again.rec = c->sort.rec; again.bbox = boxes;
            again.rect = c->sort.rect_idx; again.overflow = &c->words.fstate->overflow;
            launch_project_key(again, c->stream);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(tmp.data(), boxes, (size_t)c->scene->n * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bbox)
        for (uint32_t i = 0; i < c->scene->n; i++) {
            bbox[4 * (size_t)i + 0] = (int32_t)(tmp[i].x & 0xffff);
            bbox[4 * (size_t)i + 1] = (int32_t)(tmp[i].y & 0xffff);
            bbox[4 * (size_t)i + 2] = (int32_t)(tmp[i].x >> 16);
            bbox[4 * (size_t)i + 3] = (int32_t)(tmp[i].y >> 16);
        }
    return GSR_OK;
}

int gsr_read_sh_colors(gsr_ctx* c, float* rgba)
{
    if (!c || !rgba) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    if (!c->have_frame || !c->scene->sh_count) return fail(c, GSR_ERR_ARG, "no frame rendered with SH colours yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(rgba, c->shcol, (size_t)c->scene->n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_read_work_items(gsr_ctx* c, uint32_t* out)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    if (!c->have_frame) return fail(c, GSR_ERR_ARG, "no frame has been rendered yet");
    HIP_TRY(c, hipSetDevice(c->device));
    static_assert(offsetof(FrameState, n_items) == offsetof(FrameState, seg_len) + 4 && offsetof(FrameState, spec) == offsetof(FrameState, seg_len) + 8,
                  "seg_len, n_items, spec are read through one pointer");
    HIP_TRY(c, hipMemcpyAsync(out, &c->words.fstate->seg_len, 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const BinGrid g = make_grid(c);
    out[3] = c->bin.blend.waves_per_tile;
    out[4] = (uint32_t)((g.bx_hi - g.bx_lo) * g.nby);
    return GSR_OK;
}

int gsr_read_bin_totals(gsr_ctx* c, uint32_t* out, int32_t* nbx, int32_t* nby)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "out is NULL") : GSR_ERR_ARG;
    if (!c->have_frame) return fail(c, GSR_ERR_ARG, "no frame has been rendered yet");
    const BinGrid g = make_grid(c);
    const int w = g.bx_hi - g.bx_lo;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->bin.total, (size_t)w * g.nby * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (nbx) *nbx = w;
    if (nby) *nby = g.nby;
    return GSR_OK;
}

int gsr_read_bin_lists(gsr_ctx* c, uint32_t* starts, uint32_t* list, uint64_t list_words)
{
    if (!c || !starts) return c ? fail(c, GSR_ERR_ARG, "starts is NULL") : GSR_ERR_ARG;
    if (!c->have_frame) return fail(c, GSR_ERR_ARG, "no frame has been rendered yet");
    const BinGrid g = make_grid(c);
    const size_t nbins = (size_t)(g.bx_hi - g.bx_lo) * g.nby;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(starts, c->bin.start, (nbins + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t total = starts[nbins];
    if (list) {
        if (total > list_words || total > c->bin.capacity) return fail(c, GSR_ERR_ARG, "the frame's lists hold %llu entries", (unsigned long long)total);
        HIP_TRY(c, hipMemcpyAsync(list, c->bin.list, total * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return GSR_OK;
}

// The work list k_bin_finalize published for the last render frame, for tests (tests/test_gpu_work_items.py compares it with
// tests/work_items_reference.py): items[0 .. n_items) as four words each and seg_start[0 .. bins].  Returns n_items; GSR_ERR_ARG
// where the frame cannot be walked (depth_frame_check) or a buffer is too small.  A frame whose lists did not fit is NOT
// rendered again: the caller sees its n_items == 0, as the compositor did.  Not part of the ABI.
int gsr_debug_read_work_list(gsr_ctx* c, uint32_t* items, uint64_t item_words, uint32_t* seg_start, uint64_t seg_words)
{
    if (!c || !items || !seg_start) return c ? fail(c, GSR_ERR_ARG, "gsr_debug_read_work_list: a buffer is NULL") : GSR_ERR_ARG;
    if (int r = depth_frame_check(c, "gsr_debug_read_work_list")) return r;
    const BinGrid g = make_grid(c);
    const size_t nbins = (size_t)(g.bx_hi - g.bx_lo) * g.nby;
    if (seg_words < nbins + 1) return fail(c, GSR_ERR_ARG, "gsr_debug_read_work_list: seg_start needs %zu words", nbins + 1);
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t n_items = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_items, &c->words.fstate->n_items, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(seg_start, c->bin.seg_start, (nbins + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_items > c->bin.blend.max_items || (uint64_t)n_items * 4 > item_words)
        return fail(c, GSR_ERR_ARG, "gsr_debug_read_work_list: the frame has %u work items", n_items);
    if (n_items) {
        HIP_TRY(c, hipMemcpyAsync(items, c->bin.items, (size_t)n_items * 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return (int)n_items;
}

// What the finalize step of the last render frame saw and decided (FrameState::report[6..11], with the frame's visible splats
// and tile overlaps in front): out[8] = V, D, optical depth sum, raw optical mass sum, list entries, longest list, long_from,
// dense | heavy << 1 | by_size << 2 | fits << 3.  The same checks, and no repair, as gsr_debug_read_work_list.  Not part of the ABI.
int gsr_debug_read_frame_figures(gsr_ctx* c, uint64_t* out)
{
    if (!c || !out) return c ? fail(c, GSR_ERR_ARG, "gsr_debug_read_frame_figures: out is NULL") : GSR_ERR_ARG;
    if (int r = depth_frame_check(c, "gsr_debug_read_frame_figures")) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    static_assert(offsetof(FrameState, tile_entries) == offsetof(FrameState, visible) + 8 && offsetof(FrameState, report) == offsetof(FrameState, visible) + 16,
                  "visible, tile_entries and report are read through one pointer");
    uint64_t w[2 + 12];
    HIP_TRY(c, hipMemcpyAsync(w, &c->words.fstate->visible, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out[0] = w[0]; out[1] = w[1];
    for (int k = 0; k < 6; k++) out[2 + k] = w[2 + 6 + k];
    return GSR_OK;
}

int gsr_convert_rgba8_async(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_to_rgba8(c->out.fb, c->out.fb8, (uint32_t)c->W * (uint32_t)c->H, c->stream);
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

void* gsr_framebuffer8_device_ptr(gsr_ctx* c) { return c ? (void*)c->out.fb8 : nullptr; }

int gsr_pack_band_rgba8_async(gsr_ctx* c, void* slab, int32_t slab_width_px)
{
    if (!c) return GSR_ERR_ARG;
    if (!slab || !c->out.fb) return fail(c, GSR_ERR_ARG, "gsr_pack_band_rgba8_async: no slab / nothing rendered yet");
    const BinGrid g = make_grid(c);
    const int x0 = g.bx_lo * BIN_PX, x1 = std::min(g.bx_hi * BIN_PX, c->W);
    if (slab_width_px < x1 - x0) return fail(c, GSR_ERR_ARG, "gsr_pack_band_rgba8_async: slab narrower than the band");
    HIP_TRY(c, hipSetDevice(c->device));
    launch_pack_band_rgba8(c->out.fb, (uint32_t*)slab, c->W, c->H, x0, x1, slab_width_px, c->stream);
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

int gsr_unpack_slabs_rgba8_async(gsr_ctx* c, const void* gathered, void* image, int32_t slab_width_px, int32_t world,
                                 const int32_t* x0, const int32_t* x1, void* stream)
{
    if (!c) return GSR_ERR_ARG;
    if (!gathered || !image || !x0 || !x1 || world < 1 || world > MAX_SLABS)
        return fail(c, GSR_ERR_ARG, "gsr_unpack_slabs_rgba8_async: bad argument (1 <= world <= 16)");
    SlabEdges e{};
    for (int q = 0; q < world; q++) {
        if (x0[q] < 0 || x1[q] > c->W || x1[q] - x0[q] > slab_width_px)
            return fail(c, GSR_ERR_ARG, "gsr_unpack_slabs_rgba8_async: band outside the image or wider than the slab");
        e.x0[q] = x0[q]; e.x1[q] = x1[q];
    }
    HIP_TRY(c, hipSetDevice(c->device));
    launch_unpack_slabs_rgba8((const uint32_t*)gathered, (uint32_t*)image, c->W, c->H, slab_width_px, world, e, (hipStream_t)stream);
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

void* gsr_framebuffer_device_ptr(gsr_ctx* c) { return c ? (void*)c->out.fb : nullptr; }
void* gsr_stream_handle(gsr_ctx* c) { return c ? (void*)c->stream : nullptr; }

int gsr_stream_order(gsr_ctx* c, void* other_stream, int32_t ctx_waits)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipEvent_t& ev = c->link_ev[ctx_waits ? 1 : 0];
    if (!ev) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipStream_t from = ctx_waits ? (hipStream_t)other_stream : c->stream;
    hipStream_t to = ctx_waits ? c->stream : (hipStream_t)other_stream;
    HIP_TRY(c, hipEventRecord(ev, from));
    HIP_TRY(c, hipStreamWaitEvent(to, ev, 0));
    return GSR_OK;
}

}  // extern "C"
