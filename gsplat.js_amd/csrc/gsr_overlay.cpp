// Selection overlay: the last rendered frame with the selected splats tinted, and per pixel the share of its alpha they supply
// ("Selection overlay").  Like the depth and contribution passes it is a separate launch behind the frame on the
// context's stream (k_overlay.hip) -- never a node of the frame's graph, nothing of FrameArgs -- over the bin lists and records the
// frame left on the device, the scene's selection words and the framebuffer, which it reads and never writes.  The image and the
// cover plane are the context's; the selection is the scene's, so a context notes that it has a pass in flight and the calls that
// change the mask wait for the noted members first.  A context that never calls gsr_set_overlay allocates nothing and launches nothing.
// gsr_set_overlay_outline adds the selection's outline: two more launches behind the pass, which draw the edge of { cover >= threshold }
// into the image in place; without it nothing here differs by a launch.
#include "gsr_ctx.h"

#include <algorithm>
#include <cmath>

using namespace gsr;

namespace {

// the image is the one of this frame, this selection and these options
bool image_current(const gsr_ctx* c)
{
    const gsr_ctx::Overlay& o = c->overlay;
    return o.image && o.serial && o.serial == c->frame_serial && o.sel_version == c->scene->sel_version && o.image_opt_version == o.opt_version;
}

int ensure_buffers(gsr_ctx* c)
{
    gsr_ctx::Overlay& o = c->overlay;
    const size_t np = (size_t)c->W * c->H;
    if (np > o.pixels || !o.image) {
        o.pixels = 0; o.serial = 0;
        o.image8.reset();
        int r;
        if ((r = o.image.alloc(c, np)) || (r = o.cover.alloc(c, np)) || (r = o.invalid.alloc(c, 1))) { o.image.reset(); o.cover.reset(); o.invalid.reset(); return r; }
        o.pixels = np;
    }
    return GSR_OK;
}

// gsr_read_overlay* up to their copies: the frame settled as gsr_read_depth settles it, the image the one of this frame, this
// selection and these options (the pass is run if it is not) and final on the device; GSR_ERR_OVERFLOW for an image a pass marked invalid
int image_final(gsr_ctx* c, const char* who)
{
    gsr_ctx::Overlay& o = c->overlay;
    if (!o.on) return fail(c, GSR_ERR_ARG, "%s: no overlay options (gsr_set_overlay first)", who);
    if (int r = depth_settle_frame(c, who)) return r;
    if (int r = overlay_enqueue(c)) return r;   // (a repaired frame has a new serial: a pass behind the unfit one is redone)
    HIP_TRY(c, hipGetLastError());
    uint32_t invalid = 0;
    HIP_TRY(c, hipMemcpyAsync(&invalid, o.invalid, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    o.in_flight = false;
    if (invalid) {   // never returned as data
        o.serial = 0;
        return fail(c, GSR_ERR_OVERFLOW, "%s: the frame's bin lists did not fit: the overlay is not valid", who);
    }
    return GSR_OK;
}

// the outline's bit plane for this size: the one step of the outline that can fail, taken before anything of the pass is enqueued
int outline_ensure(gsr_ctx* c)
{
    gsr_ctx::Overlay::Outline& ol = c->overlay.outline;
    const size_t words = outline_words(c->W) * (size_t)c->H;
    if (words > ol.words || !ol.bits) {
        ol.words = 0;
        if (int r = ol.bits.alloc(c, words)) return r;   // (hipFree waits for what still reads the old plane)
        ol.words = words;
    }
    return GSR_OK;
}

// the outline behind the pass just launched: the edge of { cover >= threshold } into the image, in place
void outline_enqueue(gsr_ctx* c, const BinGrid& g)
{
    gsr_ctx::Overlay& o = c->overlay;
    gsr_ctx::Overlay::Outline& ol = o.outline;
    OutlineArgs a{};
    a.cover = o.cover; a.overlay = o.image; a.bits = ol.bits; a.invalid = o.invalid;
    a.W = c->W; a.H = c->H;
    a.x_lo = std::min(g.bx_lo * BIN_PX, c->W); a.x_hi = std::min(g.bx_hi * BIN_PX, c->W);   // the band's bin columns inside the image
    a.width = ol.width; a.side = ol.side;
    for (int k = 0; k < 3; k++) a.rgb[k] = ol.rgb[k];
    a.alpha = ol.alpha; a.threshold = ol.threshold;
    // the disc's half-widths, in integers: the largest h with h * h <= width^2 - d^2
    for (int d = 0, h = ol.width; d <= ol.width; d++) {
        while (h * h > ol.width * ol.width - d * d) h--;
        a.hw[d] = (uint8_t)h;
    }
    launch_outline(a, c->stream);
}

}  // namespace

int gsr::overlay_enqueue(gsr_ctx* c)
{
    gsr_ctx::Overlay& o = c->overlay;
    if (int r = ensure_buffers(c)) return r;
    if (image_current(c)) return GSR_OK;
    const SharedScene& sc = *c->scene;
    const BinGrid g = make_grid(c);
    const size_t np = (size_t)c->W * c->H;
    const bool outline = o.outline.on && sc.sel.mask;   // (a scene never selected in: nothing is inside, either side's edge is empty)
    if (outline) { if (int r = outline_ensure(c)) return r; }
    // A band context's bins do not cover the image and the pass writes the band's columns only: elsewhere cover is 0 and the overlay
    // is whatever the framebuffer holds.
    if (!(g.bx_lo == 0 && g.bx_hi == g.nbx)) {
        HIP_TRY(c, hipMemcpyAsync(o.image, c->out.fb, np * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(o.cover, 0, np * sizeof(float), c->stream));
    }
    OverlayBuffers b{frame_lists(c)};
    b.shcol = c->shcol;
    b.sel = sc.sel.mask;            // (null: never selected in)
    b.invalid = o.invalid;
    b.fb = c->out.fb; b.overlay = o.image; b.cover = o.cover;
    b.nwords = sc.sel.mask ? sc.sel.words : 0u;
    for (int k = 0; k < 3; k++) b.tint[k] = o.tint[k];
    b.mix = o.mix;
    launch_overlay(b, g, c->cam_frame, c->knobs.depth_skip, c->knobs.overlay_trim, c->stream);
    if (outline) outline_enqueue(c, g);
    o.serial = c->frame_serial; o.sel_version = sc.sel_version; o.image_opt_version = o.opt_version;
    o.in_flight = true;
    return GSR_OK;
}

int gsr::overlay_before_selection_change(gsr_ctx* c)
{
    SharedScene& sc = *c->scene;
    for (gsr_ctx* m : sc.members) {
        if (m == c || !m->overlay.in_flight) continue;   // (the caller's own passes lie in front of the change on its stream)
        HIP_TRY(c, hipStreamSynchronize(m->stream));
        m->overlay.in_flight = false;
    }
    sc.sel_version++;
    return GSR_OK;
}

extern "C" {

int gsr_set_overlay(gsr_ctx* c, const gsr_overlay_options* opt)
{
    if (!c) return GSR_ERR_ARG;
    gsr_ctx::Overlay& o = c->overlay;
    if (!opt) {   // off: the buffers go (nothing of them is in flight afterwards: the wait is the free's)
        if (o.image) {
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (c->delivery.copy_stream) HIP_TRY(c, hipStreamSynchronize(c->delivery.copy_stream));
        }
        o.reset();
        o.in_flight = false;
        return GSR_OK;
    }
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(opt->tint[k])) return fail(c, GSR_ERR_ARG, "gsr_set_overlay: tint[%d] is not finite", k);
    if (!(opt->mix >= 0.0f && opt->mix <= 1.0f)) return fail(c, GSR_ERR_ARG, "gsr_set_overlay: mix must be in [0, 1], not %g", (double)opt->mix);
    for (int k = 0; k < 4; k++)
        if (opt->reserved[k]) return fail(c, GSR_ERR_ARG, "gsr_set_overlay: gsr_overlay_options.reserved must be 0");
    if (!c->W || !c->H) return fail(c, GSR_ERR_ARG, "gsr_set_overlay: set the framebuffer size first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = ensure_buffers(c)) return r;
    const bool same = o.on && o.mix == opt->mix && o.tint[0] == opt->tint[0] && o.tint[1] == opt->tint[1] && o.tint[2] == opt->tint[2];
    if (!same) o.opt_version++;
    for (int k = 0; k < 3; k++) o.tint[k] = opt->tint[k];
    o.mix = opt->mix;
    o.on = true;
    return GSR_OK;
}

int gsr_set_overlay_outline(gsr_ctx* c, const gsr_outline_options* opt)
{
    if (!c) return GSR_ERR_ARG;
    gsr_ctx::Overlay& o = c->overlay;
    gsr_ctx::Overlay::Outline& ol = o.outline;
    if (opt && !o.on) return fail(c, GSR_ERR_ARG, "gsr_set_overlay_outline: no overlay options (gsr_set_overlay first)");
    if (!opt) {   // off: the bit plane goes (nothing of it is in flight afterwards: the wait is the free's)
        if (ol.on) o.opt_version++;
        if (ol.bits) {
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        ol.reset();
        return GSR_OK;
    }
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(opt->rgb[k])) return fail(c, GSR_ERR_ARG, "gsr_set_overlay_outline: rgb[%d] is not finite", k);
    if (!(opt->alpha >= 0.0f && opt->alpha <= 1.0f)) return fail(c, GSR_ERR_ARG, "gsr_set_overlay_outline: alpha must be in [0, 1], not %g", (double)opt->alpha);
    if (!(std::isfinite(opt->threshold) && opt->threshold > 0.0f))
        return fail(c, GSR_ERR_ARG, "gsr_set_overlay_outline: threshold must be finite and > 0, not %g", (double)opt->threshold);
    if (opt->width < 1 || opt->width > OUTLINE_MAX_WIDTH)
        return fail(c, GSR_ERR_ARG, "gsr_set_overlay_outline: width must be in 1 .. %d, not %d", OUTLINE_MAX_WIDTH, (int)opt->width);
    if (opt->side != GSR_OUTLINE_OUTER && opt->side != GSR_OUTLINE_INNER)
        return fail(c, GSR_ERR_ARG, "gsr_set_overlay_outline: side must be GSR_OUTLINE_OUTER or GSR_OUTLINE_INNER, not %d", (int)opt->side);
    for (int k = 0; k < 5; k++)
        if (opt->reserved[k]) return fail(c, GSR_ERR_ARG, "gsr_set_overlay_outline: gsr_outline_options.reserved must be 0");
    const bool same = ol.on && ol.alpha == opt->alpha && ol.threshold == opt->threshold && ol.width == opt->width && ol.side == opt->side &&
                      ol.rgb[0] == opt->rgb[0] && ol.rgb[1] == opt->rgb[1] && ol.rgb[2] == opt->rgb[2];
    if (!same) o.opt_version++;
    for (int k = 0; k < 3; k++) ol.rgb[k] = opt->rgb[k];
    ol.alpha = opt->alpha; ol.threshold = opt->threshold; ol.width = opt->width; ol.side = opt->side;
    ol.on = true;
    return GSR_OK;
}

int gsr_overlay_async(gsr_ctx* c)
{
    if (!c) return GSR_ERR_ARG;
    if (!c->overlay.on) return fail(c, GSR_ERR_ARG, "gsr_overlay_async: no overlay options (gsr_set_overlay first)");
    if (int r = depth_frame_check(c, "gsr_overlay_async")) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = overlay_enqueue(c)) return r;
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

int gsr_read_overlay(gsr_ctx* c, float* rgba, float* cover)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = image_final(c, "gsr_read_overlay")) return r;
    const size_t np = (size_t)c->W * c->H;
    if (rgba) HIP_TRY(c, hipMemcpyAsync(rgba, c->overlay.image, np * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (cover) HIP_TRY(c, hipMemcpyAsync(cover, c->overlay.cover, np * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_read_overlay_rgba8(gsr_ctx* c, uint8_t* out)
{
    if (!c) return GSR_ERR_ARG;
    if (!out) return fail(c, GSR_ERR_ARG, "gsr_read_overlay_rgba8: out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = image_final(c, "gsr_read_overlay_rgba8")) return r;
    const size_t np = (size_t)c->W * c->H;
    gsr_ctx::Overlay& o = c->overlay;
    if (!o.image8) { if (int r = o.image8.alloc(c, o.pixels)) return r; }
    launch_to_rgba8(o.image, o.image8, (uint32_t)np, c->stream);   // the framebuffer's conversion kernel on another source
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, o.image8, np * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

void* gsr_overlay_device_ptr(gsr_ctx* c, int32_t plane)
{
    if (!c) return nullptr;
    return plane == 0 ? (void*)c->overlay.image.p : plane == 1 ? (void*)c->overlay.cover.p : nullptr;
}

}  // extern "C"
