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

uint32_t words_of(uint32_t n) { return (n + 31u) / 32u; }
// words a fold runs over for n splats: what select_ensure and hidden_ensure allocate at least (even, as the box picker's ballots
// store whole pairs), so both masks hold this many whatever count they were allocated for (the count only shrinks under them)
uint32_t fold_words(uint32_t n) { return std::max((words_of(n) + 1u) & ~1u, 2u); }
bool op_ok(int32_t op) { return op >= GSR_SELOP_REPLACE && op <= GSR_SELOP_INTERSECT; }

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
    uint32_t count = 0;
    hipError_t e1 = hipMemcpyAsync(&count, hid.counters, 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e1, e2, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "hidden set update failed: %s", hipGetErrorString(e));
    hid.count = count;
    if (hidden) *hidden = count;
    return GSR_OK;
}

}  // namespace

int gsr::hidden_ensure(gsr_ctx* c)
{
    SharedScene& sc = *c->scene;
    SharedScene::Hidden& hid = sc.hid;
    const uint32_t need = fold_words(sc.n);
    if (hid.words >= need && hid.mask) return GSR_OK;
    // (the count only shrinks under a hidden set -- a new scene resets it, a compaction keeps the buffers -- so there are no bits to carry over)
    hid.reset();
    const uint32_t cw = 2u + (need + SELECT_APPLY_THREADS - 1u) / SELECT_APPLY_THREADS;
    int r;
    if ((r = hid.mask.alloc(c, need)) || (r = hid.spare.alloc(c, need)) || (r = hid.scratch.alloc(c, need)) || (r = hid.counters.alloc(c, cw))) { hid.reset(); return r; }
    hid.words = need; hid.counter_words = cw;
    HIP_TRY(c, hipMemsetAsync(hid.mask, 0, (size_t)need * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(hid.counters, 0, (size_t)cw * 4, c->stream));
    return GSR_OK;
}

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
    const SharedScene& sc = *c->scene;
    const uint32_t need = words_of(sc.n);
    if (words && nwords < need) return fail(c, GSR_ERR_ARG, "gsr_read_hidden: nwords (%u) is smaller than ceil(%u / 32) = %u", nwords, sc.n, need);
    if (hidden) *hidden = sc.hid.mask ? sc.hid.count : 0u;
    if (!words || !need) return GSR_OK;
    if (!sc.hid.mask) {   // never hid anything: all zeros
        std::fill(words, words + need, 0u);
        return GSR_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(words, sc.hid.mask, (size_t)need * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
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
