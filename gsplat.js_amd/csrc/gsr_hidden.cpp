// Hidden splats: one bit per splat of a scene, held with the scene (SharedScene::hid) in the selection's layout.  A hidden splat
// fails the projection's culls (k_project_key), so it is in no list of a frame and everything that walks the lists sees through
// it; nothing is erased, and "show" is the undo.  The folds are the selection's (launch_select_apply, k_select.hip).  A change of
// the set is a scene edit, ordered like gsr_scene_translate: it runs on this context's stream between edit_begin and edit_end,
// so the other members' frames enqueued before it read the old set and those enqueued behind it the new one, and it marks every
// member's frame state as edited.  Every call is blocking: it ends with a wait for this context's stream, to return the count.
// scene_compact (gsr_scene.cpp) carries the set through limitBox and erase.  A scene that never hides allocates nothing.
#include "gsr_ctx.h"

using namespace gsr;

namespace {

// H <- H (op) P as a scene edit; P: `dev` (device words, at least fold_words(n) of them), or `host` (ceil(n / 32) words), or the empty set
int hidden_fold(gsr_ctx* c, const uint32_t* dev, const uint32_t* host, int op, uint32_t* hidden)
{
    SharedScene& sc = *c->scene;
    HIP_TRY(c, hipSetDevice(c->device));
    invalidate_members(c, false);   // (the sorted order does not depend on the set: gsr_read_depth_index still answers)
    if (!sc.n) { if (hidden) *hidden = 0; return GSR_OK; }
    if (int r = hidden_ensure(c)) return r;
    SharedScene::Hidden& hid = sc.hid;
    const uint32_t nw = fold_words(sc.n);
    if (int r = edit_begin(c)) return r;
    if (!dev) {
        HIP_TRY(c, hipMemsetAsync(hid.scratch, 0, (size_t)nw * 4, c->stream));
        if (host) HIP_TRY(c, hipMemcpyAsync(hid.scratch, host, (size_t)words_of(sc.n) * 4, hipMemcpyHostToDevice, c->stream));
        dev = hid.scratch;
    }
    launch_select_apply(op, hid.mask, dev, sc.n, nw, hid.counters + 2, hid.counters, c->stream);   // (host bits at and above n are dropped there)
    HIP_TRY(c, hipGetLastError());
    if (int r = edit_end(c)) return r;
    if (int r = set_count(c, hid, "hidden set update")) return r;
    if (hidden) *hidden = hid.count;
    return GSR_OK;
}

}  // namespace

int gsr::hidden_ensure(gsr_ctx* c) { return set_ensure(c, c->scene->hid, &c->scene->hid.spare, c->scene->n); }

extern "C" {

int gsr_hide_selected(gsr_ctx* c, int32_t op, uint32_t* hidden)
{
    if (!c) return GSR_ERR_ARG;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_hide_selected: unknown op %d", op);
    // (a scene never selected in: the empty set.  The selection is final on the device: every call that changes it is blocking)
    return hidden_fold(c, c->scene->sel.mask ? c->scene->sel.mask.p : nullptr, nullptr, op, hidden);
}

int gsr_hidden_set(gsr_ctx* c, const uint32_t* words, uint32_t nwords, int32_t op, uint32_t* hidden)
{
    if (!c) return GSR_ERR_ARG;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_hidden_set: unknown op %d", op);
    const uint32_t n = c->scene->n, need = words_of(n);
    if (words && nwords < need) return fail(c, GSR_ERR_ARG, "gsr_hidden_set: nwords (%u) is smaller than ceil(%u / 32) = %u", nwords, n, need);
    return hidden_fold(c, nullptr, words, op, hidden);
}

int gsr_read_hidden(gsr_ctx* c, uint32_t* words, uint32_t nwords, uint32_t* hidden)
{
    if (!c) return GSR_ERR_ARG;
    return set_read(c, c->scene->hid, "gsr_read_hidden", words, nwords, hidden);
}

// a picker like the others: P = H into the selection's scratch, then the selection's own fold (which waits for overlay passes in
// flight); neither H nor any frame is touched
int gsr_select_hidden(gsr_ctx* c, int32_t op, uint32_t* selected)
{
    if (!c) return GSR_ERR_ARG;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_hidden: unknown op %d", op);
    HIP_TRY(c, hipSetDevice(c->device));
    SharedScene& sc = *c->scene;
    if (!sc.n) { if (selected) *selected = 0; return GSR_OK; }
    if (int r = select_ensure(c)) return r;
    HIP_TRY(c, hipMemsetAsync(sc.sel.scratch, 0, (size_t)sc.sel.words * 4, c->stream));
    if (sc.hid.mask)
        HIP_TRY(c, hipMemcpyAsync(sc.sel.scratch, sc.hid.mask, (size_t)std::min(sc.sel.words, sc.hid.words) * 4, hipMemcpyDeviceToDevice, c->stream));
    return select_fold_and_count(c, op, selected);
}

}  // extern "C"
