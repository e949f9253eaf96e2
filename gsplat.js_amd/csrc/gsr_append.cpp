// Growing the scene: duplicate the selection in place, append another context's selected splats device to device, append rows from
// the host, and reserve capacity (include/gsplat_hip.h, "growing the scene"; kernels: k_append.hip).  SharedScene::arr_rows is the
// capacity, SharedScene::n the count: while n + k fits nothing of the scene arrays is re-allocated and no old row is copied.  The
// calls are blocking scene replacements on scene_compact's model: the other members' streams are waited for, the work runs on this
// context's stream, the generation moves so that every member re-sizes its per-splat buffers before its next frame, and every
// member's frame and sorted order are marked as edited.  Indices of existing splats do not move, so the hidden set and the
// contribution accumulators stay (grown where the new count needs more words or rows, the new tail zero) and the context stays in
// its shared scene; the selection becomes exactly the new rows.  A context that never calls these allocates and launches nothing new.
#include "gsr_ctx.h"

using namespace gsr;

namespace {

constexpr uint32_t MAX_ROWS = 0x7fffffffu / 8;   // the upload's limit (gsr_set_scene*)

// the capacity a scene of `capacity` rows takes when it has to hold `need`
uint32_t grown_rows(uint32_t capacity, uint32_t need)
{
    const uint64_t by_half = (uint64_t)capacity + capacity / 2;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need, by_half), MAX_ROWS);
}

// What a call replaced: kept alive until the call has waited for its stream (the copies out of them are in flight until then).
struct Retired {
    SceneArrays arr;
    DevBuf<uint32_t> words[7];
    DevBuf<unsigned long long> weight;
    DevBuf<uint32_t> peak, pixels;
};

// a buffer of `count` elements holding the first `keep` of `old` and zeros behind them; `old` goes to `out`
template <class T>
int regrow(gsr_ctx* c, DevBuf<T>& buf, size_t keep, size_t count, DevBuf<T>& out)
{
    DevBuf<T> fresh;
    if (int r = fresh.alloc(c, count)) return r;
    if (keep) HIP_TRY(c, hipMemcpyAsync(fresh, buf, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    if (count > keep) HIP_TRY(c, hipMemsetAsync(fresh + keep, 0, (count - keep) * sizeof(T), c->stream));
    out = std::move(buf);     // (DevBuf's move assignment swaps: `buf` is empty afterwards only if `out` was)
    buf = std::move(fresh);
    return GSR_OK;
}

// Arrays of `rows` rows (with rotations and scales) that hold the scene's n splats: filled beside the old ones by device copies.
int grown_arrays(gsr_ctx* c, uint32_t rows, SceneArrays& dst)
{
    const SharedScene& sc = *c->scene;
    if (int r = dst.alloc(c, rows, true)) return r;
    return sc.n ? sc.arr.copy_rows(c, dst, sc.n, c->stream) : GSR_OK;
}

// a set that exists and holds less than `need` words regrown, its bits kept (scratch and spare are not carried, the counters' two
// leading words are); old[0..3] take what it held
int regrow_set(gsr_ctx* c, SplatSet& s, DevBuf<uint32_t>* spare, uint32_t need, DevBuf<uint32_t>* old)
{
    if (!s.mask || s.words >= need) return GSR_OK;
    const uint32_t cw = counter_words(need);
    int r;
    if ((r = regrow(c, s.mask, s.words, need, old[0])) || (spare && (r = regrow(c, *spare, 0, need, old[3]))) ||
        (r = regrow(c, s.scratch, 0, need, old[1])) || (r = regrow(c, s.counters, std::min<size_t>(s.counter_words, 2), cw, old[2])))
        return r;
    s.words = need; s.counter_words = cw;
    return GSR_OK;
}

// The per-splat state beside the arrays follows the capacity: the selection words (kept), the hidden words (kept) and the
// contribution accumulators (kept, the new rows zero), each only where it exists and holds less than `rows` splats need.
int grow_side_buffers(gsr_ctx* c, uint32_t rows, Retired& old)
{
    SharedScene& sc = *c->scene;
    const uint32_t need = fold_words(rows);
    if (int r = regrow_set(c, sc.sel, nullptr, need, old.words)) return r;
    if (int r = regrow_set(c, sc.hid, &sc.hid.spare, need, old.words + 3)) return r;
    SharedScene::Contrib& k = sc.contrib;
    if (k.live() && k.alloc_rows < rows) {
        int r;
        if ((r = regrow(c, k.weight, k.rows, rows, old.weight)) || (r = regrow(c, k.peak, k.rows, rows, old.peak)) ||
            (r = regrow(c, k.pixels, k.rows, rows, old.pixels)))
            return r;
        k.alloc_rows = rows;
    }
    return GSR_OK;
}

// capacity >= rows (exactly `rows` where it grows): the arrays replaced by larger ones that carry the old rows, the state beside
// them grown.  The caller has waited for the other members and waits for this stream before `old` goes.
int grow_to(gsr_ctx* c, uint32_t rows, Retired& old)
{
    SharedScene& sc = *c->scene;
    if (rows > sc.arr_rows || !sc.arr.rot) {
        SceneArrays fresh;
        if (int r = grown_arrays(c, std::max(rows, sc.arr_rows), fresh)) return r;
        std::swap(sc.arr, fresh);
        std::swap(old.arr, fresh);
        sc.arr_rows = std::max(rows, sc.arr_rows);
    }
    return grow_side_buffers(c, sc.arr_rows, old);
}

// what every growing call refuses first (GSR_ERR_ARG, nothing touched); m: the rows it would add
int grow_check(gsr_ctx* c, const char* who, uint64_t m, bool empty_ok)
{
    const SharedScene& sc = *c->scene;
    if (!(empty_ok && !sc.n))
        if (int r = require_rows(c)) return r;
    if (sc.sh_count)   // SH rows are indexed by splat order and the bands are index thresholds: a row at the tail has no SH row to read
        return fail(c, GSR_ERR_ARG, "%s: the scene has SH rows (sh_count %u): a splat appended at the tail would fall into the top band and has no SH row",
                    who, sc.sh_count);
    if ((uint64_t)sc.n + m > MAX_ROWS) return fail(c, GSR_ERR_ARG, "%s: %u + %llu splats are too many", who, sc.n, (unsigned long long)m);
    return GSR_OK;
}

// the blocking replacement's entry (scene_compact's): nothing of another member is in flight, this context has followed the scene
int grow_enter(gsr_ctx* c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = sync_members(c)) return r;
    return adopt_scene(c);
}

// ... and its end, once rows [n, n + k) hold the new splats: the state beside the arrays, the selection = the new rows (set on
// the device), the wait, the count, the generation and the members' frame state
int grow_commit(gsr_ctx* c, const char* who, uint32_t k, Retired& old)
{
    SharedScene& sc = *c->scene;
    const uint32_t n = sc.n;
    if (int r = overlay_before_selection_change(c)) return r;   // the members' overlay passes in flight read the mask as it was
    SharedScene::Selection& sel = sc.sel;
    // never selected in (rows from the host, or from another scene): the buffers, for the capacity; every word of the mask is stored below
    if (int r = set_ensure(c, sel, nullptr, sc.arr_rows, false)) return r;
    launch_append_select_range(sel.mask, sel.words, n, k, sel.counters, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    sc.n = n + k;
    sc.given = true;
    sc.have_rows = true;
    sel.count = k;
    if (sc.contrib.live()) sc.contrib.rows = sc.n;   // (the new rows are zero: grow_side_buffers, and nothing ever writes behind `rows`)
    ++sc.generation;   // every member re-sizes its per-splat buffers before its next frame; this one here
    invalidate_members(c, true);
    return adopt_scene(c);
}

// gsr_scene_duplicate_selected and gsr_scene_append_selected: the selected splats of `from`'s scene behind this scene's last one
int append_selected(gsr_ctx* c, gsr_ctx* from, const char* who, uint32_t* first, uint32_t* count)
{
    SharedScene& sc = *c->scene;
    const SharedScene& fs = *from->scene;
    const bool same = &fs == &sc;
    if (!same && c->device != from->device)
        return fail(c, GSR_ERR_ARG, "%s: the contexts are on different devices (%d and %d)", who, c->device, from->device);
    if (!same && !fs.have_rows) return fail(c, GSR_ERR_ARG, "%s: `from` needs a scene built with gsr_set_scene_rows or gsr_set_scene_arrays", who);
    const uint32_t n = sc.n, k = fs.sel.mask ? fs.sel.count : 0u;   // (the count the last fold left: every call that changes it is blocking)
    if (int r = grow_check(c, who, k, false)) return r;
    if (first) *first = n;
    if (count) *count = k;
    if (!k) return GSR_OK;   // nothing selected: nothing touched, no edit, the last frame stays valid
    if (int r = grow_enter(c)) return r;
    hipEvent_t ev = nullptr;
    if (!same) {   // what `from`'s stream holds (an edit of its scene, a fold of its selection's) lies in front of the copy: on the device
        HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e0 = hipEventRecord(ev, from->stream);
        hipError_t e1 = hipStreamWaitEvent(c->stream, ev, 0);
        (void)hipEventDestroy(ev);   // (released once the record has completed)
        for (hipError_t e : {e0, e1})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    }
    Retired old;
    if (n + k > sc.arr_rows) { if (int r = grow_to(c, grown_rows(sc.arr_rows, n + k), old)) return r; }
    else if (int r = grow_side_buffers(c, sc.arr_rows, old)) return r;
    DevBuf<uint32_t> block_sums;
    if (int r = block_sums.alloc(c, (size_t)append_blocks(fs.n) + 1)) return r;
    launch_append_gather(fs.n, fs.arr.view(), sc.arr.view(), n, sc.arr_rows, fs.sel.mask, fs.sel.words, block_sums, c->stream);
    HIP_TRY(c, hipGetLastError());
    return grow_commit(c, who, k, old);   // (waits for the stream: `old` and `block_sums` go behind it)
}

}  // namespace

extern "C" {

int gsr_scene_reserve(gsr_ctx* c, uint32_t rows)
{
    if (!c) return GSR_ERR_ARG;
    SharedScene& sc = *c->scene;
    if (int r = require_rows(c)) return r;
    if (rows > MAX_ROWS) return fail(c, GSR_ERR_ARG, "gsr_scene_reserve: %u rows are too many", rows);
    if (rows <= sc.arr_rows) return GSR_OK;   // never shrinks
    if (int r = grow_enter(c)) return r;
    Retired old;
    if (int r = grow_to(c, rows, old)) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // no splat changes: no edit, the members' frames stay valid (they read the new arrays' same rows)
    return GSR_OK;
}

int gsr_scene_capacity(gsr_ctx* c, uint32_t* rows)
{
    if (!c || !rows) return GSR_ERR_ARG;
    *rows = c->scene->arr_rows;
    return GSR_OK;
}

int gsr_scene_duplicate_selected(gsr_ctx* c, uint32_t* first, uint32_t* count)
{
    if (!c) return GSR_ERR_ARG;
    return append_selected(c, c, "gsr_scene_duplicate_selected", first, count);
}

int gsr_scene_append_selected(gsr_ctx* c, gsr_ctx* from, uint32_t* first, uint32_t* count)
{
    if (!c) return GSR_ERR_ARG;
    if (!from) return fail(c, GSR_ERR_ARG, "gsr_scene_append_selected: from is NULL");
    return append_selected(c, from, "gsr_scene_append_selected", first, count);
}

int gsr_scene_append_arrays(gsr_ctx* c, const uint32_t* data, const float* positions, const float* rotations, const float* scales, uint32_t m,
                            uint32_t* first)
{
    if (!c) return GSR_ERR_ARG;
    const char* who = "gsr_scene_append_arrays";
    if (m && (!data || !positions || !rotations || !scales)) return fail(c, GSR_ERR_ARG, "%s: data/positions/rotations/scales is NULL", who);
    SharedScene& sc = *c->scene;
    if (int r = grow_check(c, who, m, true)) return r;
    const uint32_t n = sc.n;
    if (first) *first = n;
    if (!m) return GSR_OK;
    if (int r = grow_enter(c)) return r;
    // The rows go through gsr_set_scene_arrays' repack and check (upload_rows, gsr_scene.cpp) into views offset by n -- of the scene's arrays where they hold
    // n + m rows, of larger ones filled beside them otherwise, which become the scene only once the upload is accepted: a refused
    // one (GSR_ERR_SCENE) leaves everything as it was, the capacity included.  Rows [0, n) are not written either way.
    const bool grow = n + m > sc.arr_rows || !sc.arr.rot;
    const uint32_t rows = grow ? std::max(grown_rows(sc.arr_rows, n + m), sc.arr_rows) : sc.arr_rows;
    SceneArrays fresh;
    if (grow) { if (int r = grown_arrays(c, rows, fresh)) return r; }
    const SceneDev v = grow ? fresh.view() : sc.arr.view();
    uint32_t flag = 0;
    if (int r = upload_rows(c, who, v, n, m, data, positions, rotations, scales, &flag)) return r;
    if (flag) return fail(c, GSR_ERR_SCENE, "%s: positions differ from data words 0..2 (Scene.ts:141-143 keeps them equal)", who);
    Retired old;
    if (grow) {
        std::swap(sc.arr, fresh);
        std::swap(old.arr, fresh);
        sc.arr_rows = rows;
    }
    if (int r = grow_side_buffers(c, sc.arr_rows, old)) return r;
    return grow_commit(c, who, m, old);
}

}  // extern "C"
