// Selection: one bit per splat of a scene, held with the scene (SharedScene::sel), changed by screen regions of the last rendered
// frame, world boxes and the host's own words, and applied by gsr_scene_erase_selected, which compacts the scene exactly as
// gsr_scene_limit_box does (scene_compact, gsr_scene.cpp).  Kernels: k_select.hip.  Every call is blocking and ends with a wait
// for the context's stream, so the selection is final on the device when it returns -- which is also why the members of a shared
// scene need no events between their calls.  A context that never calls these allocates nothing.
#include "gsr_ctx.h"

using namespace gsr;

// ---- what the selection and the hidden set share (gsr_ctx.h, SplatSet) ----
int gsr::set_ensure(gsr_ctx* c, SplatSet& s, DevBuf<uint32_t>* spare, uint32_t rows, bool zero_mask)
{
    const uint32_t need = fold_words(rows), cw = counter_words(need);
    if (s.words >= need && s.mask) return GSR_OK;
    // (the count only shrinks under a set -- a new scene resets it, a compaction drops the selection and keeps the hidden set's
    // buffers, growth regrows them first -- so there are no bits to carry over)
    s.reset();
    if (spare) spare->reset();
    int r;
    if ((r = s.mask.alloc(c, need)) || (spare && (r = spare->alloc(c, need))) || (r = s.scratch.alloc(c, need)) || (r = s.counters.alloc(c, cw))) {
        s.reset();
        if (spare) spare->reset();
        return r;
    }
    s.words = need; s.counter_words = cw;
    if (zero_mask) HIP_TRY(c, hipMemsetAsync(s.mask, 0, (size_t)need * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(s.counters, 0, (size_t)cw * 4, c->stream));
    return GSR_OK;
}

int gsr::set_count(gsr_ctx* c, SplatSet& s, const char* what)
{
    uint32_t count = 0;
    hipError_t e1 = hipMemcpyAsync(&count, s.counters, 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e1, e2, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    s.count = count;
    return GSR_OK;
}

int gsr::set_read(gsr_ctx* c, const SplatSet& s, const char* who, uint32_t* words, uint32_t nwords, uint32_t* count)
{
    const uint32_t n = c->scene->n, need = words_of(n);
    if (words && nwords < need) return fail(c, GSR_ERR_ARG, "%s: nwords (%u) is smaller than ceil(%u / 32) = %u", who, nwords, n, need);
    if (count) *count = s.mask ? s.count : 0u;
    if (!words || !need) return GSR_OK;
    if (!s.mask) {   // never allocated: all zeros
        std::fill(words, words + need, 0u);
        return GSR_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(words, s.mask, (size_t)need * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

// the selection's buffers for the scene's count, allocated (the mask zeroed) by the first call that needs them
int gsr::select_ensure(gsr_ctx* c) { return set_ensure(c, c->scene->sel, nullptr, c->scene->n); }

// selection <- selection (op) scratch on the device, its count back to the host: the end of every call that changes it
int gsr::select_fold_and_count(gsr_ctx* c, int op, uint32_t* selected)
{
    SharedScene::Selection& sel = c->scene->sel;
    if (int r = overlay_before_selection_change(c)) return r;   // the members' overlay passes in flight read the mask as it was
    launch_select_apply(op, sel.mask, sel.scratch, c->scene->n, sel.words, sel.counters + 2, sel.counters, c->stream);
    if (int r = set_count(c, sel, "selection update")) return r;
    if (selected) *selected = sel.count;
    return GSR_OK;
}

extern "C" {

int gsr_select_region(gsr_ctx* c, const gsr_region* region, int32_t mode, int32_t op, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    if (!region) return fail(c, GSR_ERR_ARG, "gsr_select_region: region is NULL");
    const gsr_region& q = *region;
    if (mode != GSR_SELECT_CENTRE && mode != GSR_SELECT_HIT) return fail(c, GSR_ERR_ARG, "gsr_select_region: unknown mode %d", mode);
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_region: unknown op %d", op);
    if (q.reserved != 0) return fail(c, GSR_ERR_ARG, "gsr_select_region: reserved must be 0");
    if (int r = depth_frame_check(c, "gsr_select_region")) return r;
    if (!(0 <= q.x0 && q.x0 < q.x1 && q.x1 <= c->W && 0 <= q.y0 && q.y0 < q.y1 && q.y1 <= c->H))
        return fail(c, GSR_ERR_ARG, "gsr_select_region: the rectangle [%d, %d) x [%d, %d) is empty or outside the %dx%d image", q.x0, q.x1, q.y0, q.y1,
                    c->W, c->H);
    const int w = q.x1 - q.x0, h = q.y1 - q.y0;
    if (q.mask && q.mask_stride < w) return fail(c, GSR_ERR_ARG, "gsr_select_region: mask_stride (%d) is smaller than the rectangle's width (%d)", q.mask_stride, w);
    const BinGrid g = make_grid(c);
    const int xlo = g.bx_lo * BIN_PX, xhi = std::min(g.bx_hi * BIN_PX, c->W);
    if (q.x0 < xlo || q.x1 > xhi)
        return fail(c, GSR_ERR_ARG, "gsr_select_region: the rectangle's columns [%d, %d) are outside this context's band [%d, %d)", q.x0, q.x1, xlo, xhi);
    HIP_TRY(c, hipSetDevice(c->device));
    // the frame as gsr_pick / gsr_read_depth have it: settled (one that did not fit is rendered again), in HIT mode with its planes
    if (mode == GSR_SELECT_HIT) { if (int r = depth_planes_current(c, "gsr_select_region")) return r; }
    else if (int r = depth_settle_frame(c, "gsr_select_region")) return r;
    SharedScene& sc = *c->scene;
    if (!sc.n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    SharedScene::Selection& sel = sc.sel;

    SelectRegion reg{q.x0, q.y0, q.x1, q.y1, nullptr, 0, 0u};
    if (q.mask) {
        const size_t nbytes = (size_t)(h - 1) * (size_t)q.mask_stride + (size_t)w;
        if (nbytes > 0xffffffffull) return fail(c, GSR_ERR_ARG, "gsr_select_region: the region's bytes do not fit 32 bits");
        if (nbytes > sel.region_bytes || !sel.region) {
            sel.region_bytes = 0;
            if (int r = sel.region.alloc(c, nbytes)) return r;
            sel.region_bytes = nbytes;
        }
        HIP_TRY(c, hipMemcpyAsync(sel.region, q.mask, nbytes, hipMemcpyHostToDevice, c->stream));
        reg.bytes = sel.region; reg.stride = q.mask_stride; reg.nbytes = (uint32_t)nbytes;
    }
    SelectBuffers b{};
    b.bin_start = c->bin.start; b.list = c->bin.list; b.rec = c->sort.rec;
    b.overflow = &c->words.fstate->overflow;
    b.index = mode == GSR_SELECT_HIT ? (const uint32_t*)c->depth.planes.index : nullptr;
    b.invalid = sel.counters + 1;
    b.scratch = sel.scratch;
    b.capacity = c->bin.capacity;
    b.nsplats = sc.n; b.nwords = sel.words;
    HIP_TRY(c, hipMemsetAsync(sel.scratch, 0, (size_t)sel.words * 4, c->stream));
    launch_select_region(mode, b, g, reg, c->stream);
    HIP_TRY(c, hipGetLastError());
    uint32_t invalid = 0;
    HIP_TRY(c, hipMemcpyAsync(&invalid, sel.counters + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (invalid) return fail(c, GSR_ERR_OVERFLOW, "gsr_select_region: the frame's bin lists did not fit: nothing was selected");
    return select_fold_and_count(c, op, selected);
}

int gsr_select_box(gsr_ctx* c, const double* box, int32_t op, uint32_t* selected)
{
    if (!c || !box) return GSR_ERR_ARG;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_box: unknown op %d", op);
    if (box[0] >= box[1]) return fail(c, GSR_ERR_ARG, "xMin (%g) must be smaller than xMax (%g)", box[0], box[1]);   // as gsr_scene_limit_box
    if (box[2] >= box[3]) return fail(c, GSR_ERR_ARG, "yMin (%g) must be smaller than yMax (%g)", box[2], box[3]);
    if (box[4] >= box[5]) return fail(c, GSR_ERR_ARG, "zMin (%g) must be smaller than zMax (%g)", box[4], box[5]);
    HIP_TRY(c, hipSetDevice(c->device));
    SharedScene& sc = *c->scene;
    if (!sc.n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    launch_select_box(sc.n, sc.arr.px, sc.arr.py, sc.arr.pz, box, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

int gsr_selection_set(gsr_ctx* c, const uint32_t* words, uint32_t nwords, int32_t op, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_selection_set: unknown op %d", op);
    SharedScene& sc = *c->scene;
    const uint32_t need = words_of(sc.n);
    if (words && nwords < need) return fail(c, GSR_ERR_ARG, "gsr_selection_set: nwords (%u) is smaller than ceil(%u / 32) = %u", nwords, sc.n, need);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!sc.n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    HIP_TRY(c, hipMemsetAsync(sc.sel.scratch, 0, (size_t)sc.sel.words * 4, c->stream));
    if (words) HIP_TRY(c, hipMemcpyAsync(sc.sel.scratch, words, (size_t)need * 4, hipMemcpyHostToDevice, c->stream));
    return select_fold_and_count(c, op, selected);   // (host bits at and above n are dropped there)
}

int gsr_selection_invert(gsr_ctx* c, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->scene->n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    return select_fold_and_count(c, SELOP_INVERT, selected);
}

int gsr_read_selection(gsr_ctx* c, uint32_t* words, uint32_t nwords, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    return set_read(c, c->scene->sel, "gsr_read_selection", words, nwords, selected);
}

int gsr_scene_erase_selected(gsr_ctx* c, int32_t keep_selected, uint32_t* new_count)
{
    if (!c) return GSR_ERR_ARG;
    SharedScene& sc = *c->scene;
    if (int r = require_rows(c)) return r;
    const uint32_t n = sc.n, count = sc.sel.mask ? sc.sel.count : 0u;
    // nothing to remove: nothing changes, the last frame stays valid (the count is the one the last fold left: every call is blocking)
    if (!n || (keep_selected ? count == n : count == 0u)) {
        if (new_count) *new_count = n;
        return GSR_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = select_ensure(c)) return r;   // (keep_selected with no selection yet: the zeroed mask, everything goes)
    return scene_compact(c, ScenePred{nullptr, sc.sel.mask, keep_selected ? 1u : 0u, sc.sel.words}, "gsr_scene_erase_selected", new_count);
}

}  // extern "C"
