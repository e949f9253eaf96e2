// The scene on the device: upload (packed words, the Scene's four arrays or .splat rows), the transforms and the compaction of
// scenes that carry rotations and scales, spherical harmonics, and the scene's read-back.  alloc_scene sizes everything that holds one entry per splat.
#include "gsr_ctx.h"
#include "k_splat_ops.h"

#include <cmath>

using namespace gsr;

namespace {

// what the projection writes and the sort permutes, one entry per splat: the context's own, whoever holds the scene
int alloc_sort(gsr_ctx* c, uint32_t n)
{
    gsr_ctx::Sort& so = c->sort;
    so.rows = 0;
    const SortSizes z = sort_sizes(n, sort_knobs_of(c));   // (k_sort.hip: what the sort's tables need for n rows)
    int r;
    if ((r = so.depth.alloc(c, n)) || (r = so.keys.alloc(c, n)) ||
        (r = so.keys_tmp.alloc(c, n)) || (r = so.idx_tmp.alloc(c, n)) || (r = so.depth_index.alloc(c, n)) || (r = so.rec.alloc(c, n)) ||
        (r = so.rects.alloc(c, n)) || (r = so.rect_idx.alloc(c, n)) || (r = so.rect_tmp.alloc(c, n)) ||
        (r = so.chunk_tab.alloc(c, z.chunk_tab)) || (r = so.kept.alloc(c, z.kept)) || (r = so.kept_lane.alloc(c, n)) ||
        (r = so.koff.alloc(c, z.koff)) || (r = so.block_hist.alloc(c, z.block_hist)))
        return r;
    so.rows = n;
    return GSR_OK;
}

// a scene of its own for a context that shares one: the others keep theirs untouched
void leave_share(gsr_ctx* c)
{
    if (c->scene->members.size() < 2) return;
    const bool follow = c->scene->sh_follow;
    scene_release(c);
    c->scene = new SharedScene();
    c->scene->members.push_back(c);
    c->scene->sh_follow = follow;   // (a setting of the host's, not of the arrays: it stays as the host left it)
    c->scene_gen = c->scene->generation;
}

}  // namespace

// blocking calls that replace what the members read (limitBox, new SH textures, growth): nothing of any other member is in flight afterwards
int gsr::sync_members(gsr_ctx* c)
{
    for (gsr_ctx* m : c->scene->members)
        if (m != c) HIP_TRY(c, hipStreamSynchronize(m->stream));
    return GSR_OK;
}

// what every transform, compaction and edit of the selection demands of the scene: rotations and scales (the one statement of the refusal)
int gsr::require_rows(gsr_ctx* c)
{
    if (!c->scene->have_rows) return fail(c, GSR_ERR_ARG, "scene transforms need a scene built with gsr_set_scene_rows or gsr_set_scene_arrays");
    return GSR_OK;
}

// the other members' frame state after an edit that arrived through `c`: as if each had run the call itself
void gsr::invalidate_members(gsr_ctx* c, bool lists)
{
    for (gsr_ctx* m : c->scene->members) {
        m->have_frame = false;
        if (lists) { m->have_sort = false; }
    }
}

// Device-side order around an edit of a shared scene (translate, rotate, scale, a change of the hidden set), no host wait: the editing context's stream waits for
// what every other member has enqueued (one event per member, recorded on its render stream) ...
int gsr::edit_begin(gsr_ctx* c)
{
    for (gsr_ctx* m : c->scene->members) {
        if (m == c) continue;
        HIP_TRY(c, hipEventRecord(m->share_ev, m->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, m->share_ev, 0));
    }
    return GSR_OK;
}

// ... and whatever the others enqueue from now on waits for the edit (one event behind the kernel)
int gsr::edit_end(gsr_ctx* c)
{
    if (c->scene->members.size() < 2) return GSR_OK;
    HIP_TRY(c, hipEventRecord(c->share_ev, c->stream));
    for (gsr_ctx* m : c->scene->members)
        if (m != c) HIP_TRY(c, hipStreamWaitEvent(m->stream, c->share_ev, 0));
    return GSR_OK;
}

// (re)allocate everything sized by the splat count; clears SH and per-frame state.  A member of a shared scene leaves it here.
int gsr::alloc_scene(gsr_ctx* c, uint32_t n, bool with_rows)
{
    leave_share(c);
    SharedScene& sc = *c->scene;
    sc.n = 0; sc.arr_rows = 0; c->have_frame = false; c->have_sort = false; sc.have_rows = false;
    c->bin.plan.form = BIN_FINALIZE_ONLY;   // (no splats until the caller's alloc_bins plans for the new count: a frame in between only finalizes)
    if (c->words.mailbox) reinterpret_cast<volatile uint32_t*>(c->words.mailbox)[2] = 0xffffffffu;   // a new scene: LSD order until a frame reports
    sc.drop_sh();
    sc.sel.reset();   // a new scene: the empty selection
    sc.sel_version++;   // (and every member's overlay image is stale)
    sc.contrib.reset();   // and no contribution: "never reset"
    sc.hid.reset();   // and nothing hidden
    c->shcol.reset();
    int r;
    if ((r = sc.arr.alloc(c, n, with_rows)) || (r = alloc_sort(c, n))) return r;
    sc.arr_rows = n;
    return GSR_OK;
}

void gsr::scene_release(gsr_ctx* c)
{
    SharedScene* sc = c->scene;
    if (!sc) return;
    sc->members.erase(std::remove(sc->members.begin(), sc->members.end(), c), sc->members.end());
    if (sc->members.empty()) delete sc;
    c->scene = nullptr;
}

// A member whose scene was replaced through another one (limitBox, new SH textures) does here, before its next frame, what the
// call did for the context it ran on: the sort's buffers where the new count needs larger ones, the evaluated colours, the binning's plan and buffers.
int gsr::adopt_scene(gsr_ctx* c)
{
    SharedScene& sc = *c->scene;
    if (c->scene_gen == sc.generation) return GSR_OK;
    c->have_frame = false; c->have_sort = false;
    if (sc.n > c->sort.rows) { if (int r = alloc_sort(c, sc.n)) return r; }
    if (int r = alloc_bins(c)) return r;
    if (sc.sh_count) {
        if (int r = c->shcol.alloc(c, sc.n)) return r;
        HIP_TRY(c, hipMemsetAsync(c->shcol, 0, (size_t)sc.n * sizeof(float4), c->stream));
    }
    else c->shcol.reset();
    c->scene_gen = sc.generation;
    return GSR_OK;
}

// The host upload path, for a new scene (rows from 0) and for rows appended behind a scene's last (gsr_append.cpp): m rows of
// Scene.data and Scene.positions staged and repacked into rows [at, at + m) of `v` with the repack's check, and, when given,
// rotations (`rot`'s bytes already) and scales beside them; *mismatch <- the check's flag; waits for the stream.  An error of a
// copy, the wait or a launch is "<what> failed: ..".  Covariance words and colours stay the caller's.
int gsr::upload_rows(gsr_ctx* c, const char* what, const SceneDev& v, uint32_t at, uint32_t m, const uint32_t* data, const float* positions,
                     const float* rotations, const float* scales, uint32_t* mismatch)
{
    DevBuf<uint32_t> d_data, d_flag;
    DevBuf<float> d_pos, d_scl;
    int r;
    if ((r = d_data.alloc(c, (size_t)m * 8)) || (r = d_pos.alloc(c, (size_t)m * 3)) || (r = d_flag.alloc(c, 1)) ||
        (rotations && (r = d_scl.alloc(c, (size_t)m * 3))))
        return r;
    hipStream_t s = c->stream;
    hipError_t e[8] = {};   // (hipSuccess)
    e[0] = hipMemcpyAsync(d_data, data, (size_t)m * 32, hipMemcpyHostToDevice, s);
    e[1] = hipMemcpyAsync(d_pos, positions, (size_t)m * 12, hipMemcpyHostToDevice, s);
    e[2] = hipMemsetAsync(d_flag, 0, 4, s);
    launch_repack_scene(d_data, d_pos, m, v.px + at, v.py + at, v.pz + at, v.cov0 + at, v.cov1 + at, v.cov2 + at, v.rgba + at, d_flag, s);
    if (rotations) {
        e[3] = hipMemcpyAsync(v.rot + at, rotations, (size_t)m * 16, hipMemcpyHostToDevice, s);
        e[4] = hipMemcpyAsync(d_scl, scales, (size_t)m * 12, hipMemcpyHostToDevice, s);
        launch_scene_import(d_scl, m, v.scl + at, s);
    }
    e[5] = hipMemcpyAsync(mismatch, d_flag, 4, hipMemcpyDeviceToHost, s);
    e[6] = hipStreamSynchronize(s);
    e[7] = hipGetLastError();
    for (hipError_t x : e)
        if (x != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", what, hipGetErrorString(x));
    return GSR_OK;
}

namespace {

int need_rows(gsr_ctx* c)
{
    if (int r = require_rows(c)) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    invalidate_members(c, true);
    return GSR_OK;
}

// gsr_set_scene (rotations / scales null) and gsr_set_scene_arrays: Scene.data and Scene.positions through the repack and its
// check; with rotations and scales the result is a scene the transforms accept, as if built from rows.
int upload_scene(gsr_ctx* c, const uint32_t* data, const float* positions, const float* rotations, const float* scales, uint32_t n)
{
    const bool with_rows = rotations != nullptr;
    if (n > 0x7fffffffu / 8) return fail(c, GSR_ERR_ARG, "too many splats");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int r;
    // The upload is checked before anything of the context is touched: a refused scene (GSR_ERR_SCENE) leaves the one the context
    // has, its SH state and its last frame as they were.  The arrays are filled beside the old ones and swapped in afterwards.
    SceneArrays sa;
    if (n) {
        uint32_t flag = 0;
        if ((r = sa.alloc(c, n, with_rows)) || (r = upload_rows(c, "scene upload", sa.view(), 0, n, data, positions, rotations, scales, &flag))) return r;
        if (flag) return fail(c, GSR_ERR_SCENE, "positions differ from data words 0..2 (Scene.ts:141-143 keeps them equal)");
    }
    if ((r = alloc_scene(c, n, with_rows))) return r;
    if (n) std::swap(c->scene->arr, sa);   // (the blank arrays alloc_scene made go with `sa`)
    c->scene->given = true;
    c->scene->n = n;
    c->scene->have_rows = with_rows;
    c->bin.capacity = 0;
    return alloc_bins(c);
}

}  // namespace

// gsr_scene_limit_box and gsr_scene_erase_selected: the splats `p` keeps, in order, become the scene
int gsr::scene_compact(gsr_ctx* c, const ScenePred& p, const char* what, uint32_t* kept_out, const SetCarry* also)
{
    if (int r = need_rows(c)) return r;
    const uint32_t n = c->scene->n;
    uint32_t kept = 0;
    if (n) {
        SharedScene& sc = *c->scene;
        if (int r = sync_members(c)) return r;   // the arrays are replaced: nothing of any member reads the old ones any more
        if (int r = adopt_scene(c)) return r;    // (as in gsr_set_scene_sh: the generation below is the next one, never a skipped one)
        const bool follow = sc.sh_follow && sc.sh_count;   // the SH textures are compacted with the scene
        SceneArrays dst;   // the kept splats are compacted into a second set of arrays, which then becomes the scene
        DevBuf<uint32_t> block_count, count;   // count: [0] kept splats, [1..3] those in front of bandsIndices[k] + 1 (follow)
        uint32_t counts[4] = {0, 0, 0, 0};
        int r;
        if ((r = dst.alloc(c, n, true)) || (r = block_count.alloc(c, (n + 1023) / 1024)) || (r = count.alloc(c, 4))) return r;
        launch_scene_compact(n, sc.arr.view(), dst.view(), p, block_count, count, c->stream);
        if (follow) {
            if (sc.sh_spare_rows < sc.sh_count) {   // the second set of textures: allocated on first use, then the two sets take turns
                for (auto& b : sc.sh_spare)
                    if ((r = b.alloc(c, (size_t)sc.sh_count * 8))) { sc.sh_spare_rows = 0; return r; }
                sc.sh_spare_rows = sc.sh_count;
            }
            const uint32_t* in[3] = {sc.sh_r, sc.sh_g, sc.sh_b};
            uint32_t* out[3] = {sc.sh_spare[0], sc.sh_spare[1], sc.sh_spare[2]};
            launch_scene_compact_sh(n, sc.arr.view(), p, block_count, count, sc.band, sc.sh_count, in, out, c->stream);
        }
        // the hidden set keeps naming the same splats: H'[new index of i] = H[i] for every kept i, into the zeroed other buffer, and
        // its count again (an empty fold: H' |= nothing).  Only while something is hidden: an empty set stays the zeros it is.
        SharedScene::Hidden& hid = sc.hid;
        const bool carry = hid.mask && hid.count;
        hipError_t e0 = hipSuccess, e2 = hipSuccess, e3 = hipSuccess;
        if (carry) {
            e0 = hipMemsetAsync(hid.spare, 0, (size_t)hid.words * 4, c->stream);
            launch_scene_compact_bits(n, sc.arr.view(), p, block_count, hid.mask, hid.words, hid.spare, hid.words, c->stream);
            e3 = hipMemsetAsync(hid.scratch, 0, (size_t)hid.words * 4, c->stream);
            launch_select_apply(SELOP_ADD, hid.spare, hid.scratch, n, hid.words, hid.counters + 2, hid.counters, c->stream);
        }
        // (the caller's set goes the same way, into the caller's zeroed words)
        if (also) launch_scene_compact_bits(n, sc.arr.view(), p, block_count, also->in, also->nwords_in, also->out, also->nwords_out, c->stream);
        hipError_t e1 = hipMemcpyAsync(counts, count, follow ? 16 : 4, hipMemcpyDeviceToHost, c->stream);
        if (carry) {   // (its count back: the call's one wait)
            if ((r = set_count(c, hid, what))) return r;
            std::swap(hid.mask, hid.spare);
        }
        else e2 = hipStreamSynchronize(c->stream);
        for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        kept = counts[0];
        std::swap(sc.arr, dst);
        sc.arr_rows = n;   // (what `dst` was allocated for)
        sc.n = kept;   // arrays keep their old capacity; per-frame buffers sized for the old count still fit
        sc.sel.reset();   // the selection's bits are indices of the old numbering: the scene is left with the empty one (nothing is in flight)
        sc.sel_version++;   // (and every member's overlay image is stale)
        sc.contrib.reset();   // the contribution accumulators likewise
        c->scene_gen = ++sc.generation;   // (this context follows below; the other members in adopt_scene, before their next frame)
        // The compaction renumbers the splats, so SH rows (indexed by splat - (bandsIndices[0] + 1)) and the band
        // thresholds no longer belong to them.  With gsr_set_sh_follow on they were renumbered with the scene: the kept rows
        // are in sh_dst, bandsIndices'[k] = (kept splats with index <= bandsIndices[k]) - 1, and the frame stays.  Otherwise
        // the SH state is dropped and the scene falls back to its rgba8 colours until gsr_set_scene_sh is called again.
        // (Scene.limitBox, Scene.ts:307-366, leaves shs_rgb / bandsIndices untouched, i.e. stale.)
        const bool sh_kept = follow && kept > counts[1];
        if (sh_kept) {
            std::swap(sc.sh_r, sc.sh_spare[0]); std::swap(sc.sh_g, sc.sh_spare[1]); std::swap(sc.sh_b, sc.sh_spare[2]);
            std::swap(sc.sh_rows, sc.sh_spare_rows);
            sc.sh_count = kept - counts[1];
            for (int k = 0; k < 3; k++) sc.band[k] = (int32_t)counts[1 + k] - 1;
        }
        else { sc.drop_sh(); c->shcol.reset(); }   // (no SH splat survived: cleared, as gsr_set_scene_sh with sh_count 0 clears it)
        // the binning's plan for the new count (plan_bins): fewer splats can mean fewer rounds and so MORE table rows, which
        // alloc_bins regrows; like every alloc_bins it drops what the last frame left in the lists (they index the old numbering)
        if ((r = alloc_bins(c))) return r;
        // (last: the context is whole whatever this returns) evaluated colours of the old numbering go, as gsr_set_scene_sh leaves them
        if (sh_kept) HIP_TRY(c, hipMemsetAsync(c->shcol, 0, (size_t)kept * sizeof(float4), c->stream));
    }
    if (kept_out) *kept_out = kept;
    return GSR_OK;
}

extern "C" {

int gsr_set_scene(gsr_ctx* c, const uint32_t* data, const float* positions, uint32_t n)
{
    if (!c) return GSR_ERR_ARG;
    if (n && (!data || !positions)) return fail(c, GSR_ERR_ARG, "data/positions is NULL");
    return upload_scene(c, data, positions, nullptr, nullptr, n);
}

int gsr_set_scene_arrays(gsr_ctx* c, const uint32_t* data, const float* positions, const float* rotations, const float* scales, uint32_t n)
{
    if (!c) return GSR_ERR_ARG;
    if (n && (!data || !positions || !rotations || !scales)) return fail(c, GSR_ERR_ARG, "data/positions/rotations/scales is NULL");
    return upload_scene(c, data, positions, rotations, scales, n);
}

int gsr_set_scene_rows(gsr_ctx* c, const uint8_t* rows, uint32_t n)
{
    if (!c) return GSR_ERR_ARG;
    if (n && !rows) return fail(c, GSR_ERR_ARG, "rows is NULL");
    if (n > 0x7fffffffu / 8) return fail(c, GSR_ERR_ARG, "too many splats");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int r;
    if ((r = alloc_scene(c, n, true))) return r;
    if (n) {
        DevBuf<uint8_t> d_rows;
        if ((r = d_rows.alloc(c, (size_t)n * 32))) return r;
        hipError_t e1 = hipMemcpyAsync(d_rows, rows, (size_t)n * 32, hipMemcpyHostToDevice, c->stream);
        launch_build_scene(d_rows, n, c->scene->arr.view(), c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        for (hipError_t e : {e1, e2, hipGetLastError()})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "scene build failed: %s", hipGetErrorString(e));
    }
    c->scene->given = true;
    c->scene->n = n;
    c->scene->have_rows = true;
    c->bin.capacity = 0;
    return alloc_bins(c);
}

int gsr_scene_translate(gsr_ctx* c, const double* t)
{
    if (!c || !t) return GSR_ERR_ARG;
    if (int r = need_rows(c)) return r;
    if (int r = edit_begin(c)) return r;
    launch_scene_translate(c->scene->n, c->scene->arr.view(), t, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (int r = edit_end(c)) return r;
    return GSR_OK;
}

int gsr_scene_rotate(gsr_ctx* c, const double* q)
{
    if (!c || !q) return GSR_ERR_ARG;
    if (int r = need_rows(c)) return r;
    if (int r = edit_begin(c)) return r;
    launch_scene_rotate(c->scene->n, c->scene->arr.view(), q, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (int r = edit_end(c)) return r;
    if (c->scene->sh_follow && c->scene->sh_count) {   // Linv <- Linv . R(q)^T, R as the kernels build it (k_splat_ops.h) (the frame belongs to an SH state)
        double R[9];
        quat_matrix(q[0], q[1], q[2], q[3], R);
        double* L = c->scene->sh_frame;
        double out[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) out[3 * i + j] = (L[3 * i] * R[3 * j] + L[3 * i + 1] * R[3 * j + 1]) + L[3 * i + 2] * R[3 * j + 2];
        for (int k = 0; k < 9; k++) L[k] = out[k];
    }
    return GSR_OK;
}

int gsr_scene_scale(gsr_ctx* c, const double* sv)
{
    if (!c || !sv) return GSR_ERR_ARG;
    if (c->scene->sh_follow)   // the frame is the inverse of the edits: there is none of a scale by 0
        for (int k = 0; k < 3; k++)
            if (!(std::isfinite(sv[k]) && sv[k] != 0.0))
                return fail(c, GSR_ERR_ARG, "scale component %d is %g: with gsr_set_sh_follow on, a scale must be finite and not 0", k, sv[k]);
    if (int r = need_rows(c)) return r;
    if (int r = edit_begin(c)) return r;
    launch_scene_scale(c->scene->n, c->scene->arr.view(), sv, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (int r = edit_end(c)) return r;
    if (c->scene->sh_follow && c->scene->sh_count) {   // Linv <- Linv . diag(1 / sx, 1 / sy, 1 / sz)
        double* L = c->scene->sh_frame;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) L[3 * i + j] = L[3 * i + j] * (1.0 / sv[j]);
    }
    return GSR_OK;
}

int gsr_scene_limit_box(gsr_ctx* c, const double* box, uint32_t* new_count)
{
    if (!c || !box) return GSR_ERR_ARG;
    if (box[0] >= box[1]) return fail(c, GSR_ERR_ARG, "xMin (%g) must be smaller than xMax (%g)", box[0], box[1]);   // Scene.ts:308-316
    if (box[2] >= box[3]) return fail(c, GSR_ERR_ARG, "yMin (%g) must be smaller than yMax (%g)", box[2], box[3]);
    if (box[4] >= box[5]) return fail(c, GSR_ERR_ARG, "zMin (%g) must be smaller than zMax (%g)", box[4], box[5]);
    return scene_compact(c, ScenePred{box, nullptr, 0u, 0u}, "limitBox", new_count);
}

int gsr_share_scene(gsr_ctx* c, gsr_ctx* from)
{
    if (!c || !from) return fail(c, GSR_ERR_ARG, "gsr_share_scene: ctx or from is NULL");
    if (c == from) return fail(c, GSR_ERR_ARG, "gsr_share_scene: a context cannot share its scene with itself");
    if (c->device != from->device)
        return fail(c, GSR_ERR_ARG, "gsr_share_scene: the contexts are on different devices (%d and %d)", c->device, from->device);
    if (c->scene == from->scene) return GSR_OK;   // (it shares that scene already: nothing changes)
    if (!from->scene->given) return fail(c, GSR_ERR_ARG, "gsr_share_scene: `from` has never been given a scene");
    if (delivery_frame_held(c))
        return fail(c, GSR_ERR_ARG, "gsr_share_scene: a delivered frame is held (gsr_release_frame first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // the frames in flight read the scene this context gives up
    for (gsr_ctx* m : {c, from})
        if (!m->share_ev) HIP_TRY(c, hipEventCreateWithFlags(&m->share_ev, hipEventDisableTiming));
    // every edit of the scene is ordered in front of `from`'s stream (edit_end), and this context's frames behind that
    HIP_TRY(c, hipEventRecord(from->share_ev, from->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, from->share_ev, 0));
    scene_release(c);
    SharedScene& sc = *from->scene;
    c->scene = &sc;
    sc.members.push_back(c);
    // the context's own part of a new scene, as alloc_scene and the upload leave it
    c->scene_gen = 0;
    c->have_frame = false; c->have_sort = false;
    c->bin.plan.form = BIN_FINALIZE_ONLY;
    if (c->words.mailbox) reinterpret_cast<volatile uint32_t*>(c->words.mailbox)[2] = 0xffffffffu;
    c->shcol.reset();
    int r;
    if ((r = alloc_sort(c, sc.n))) return r;
    c->bin.capacity = 0;
    if ((r = alloc_bins(c))) return r;
    if (sc.sh_count) {
        if ((r = c->shcol.alloc(c, sc.n))) return r;
        HIP_TRY(c, hipMemsetAsync(c->shcol, 0, (size_t)sc.n * sizeof(float4), c->stream));
    }
    c->scene_gen = sc.generation;
    return GSR_OK;
}

int gsr_scene_sharing(gsr_ctx* c, int32_t* members, uint64_t* scene_bytes)
{
    if (!c) return GSR_ERR_ARG;
    if (members) *members = (int32_t)c->scene->members.size();
    if (scene_bytes) *scene_bytes = c->scene->bytes();
    return GSR_OK;
}

int gsr_read_scene(gsr_ctx* c, uint32_t* data, float* positions, float* rotations, float* scales, uint32_t* count)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n = c->scene->n;
    if (count) *count = n;
    if (!data && !positions && !rotations && !scales) return GSR_OK;  // count only: nothing to copy
    if ((rotations || scales) && !c->scene->have_rows) return fail(c, GSR_ERR_ARG, "rotations/scales exist only for scenes built with gsr_set_scene_rows or gsr_set_scene_arrays");
    if (!n) return GSR_OK;
    // One kernel lays the requested parts out in the callers' layouts in one staging allocation (k_scene_export), then one copy
    // per output.  Rotations are copied from `rot` itself: it has Scene.rotations' layout.
    const size_t data_words = data ? 8 * (size_t)n : 0, pos_words = positions ? 3 * (size_t)n : 0, scl_words = scales ? 3 * (size_t)n : 0;
    DevBuf<uint32_t> stage;
    if (int r = stage.alloc(c, data_words + pos_words + scl_words)) return r;
    uint32_t* d_data = data ? (uint32_t*)stage : nullptr;
    float* d_pos = positions ? (float*)(stage + data_words) : nullptr;
    float* d_scl = scales ? (float*)(stage + data_words + pos_words) : nullptr;
    launch_scene_export(n, c->scene->arr.view(), d_data, d_pos, d_scl, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (data) HIP_TRY(c, hipMemcpyAsync(data, d_data, data_words * 4, hipMemcpyDeviceToHost, c->stream));
    if (positions) HIP_TRY(c, hipMemcpyAsync(positions, d_pos, pos_words * 4, hipMemcpyDeviceToHost, c->stream));
    if (rotations) HIP_TRY(c, hipMemcpyAsync(rotations, c->scene->arr.rot, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    if (scales) HIP_TRY(c, hipMemcpyAsync(scales, d_scl, scl_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_scene_count(gsr_ctx* c, uint32_t* count)
{
    if (!c || !count) return GSR_ERR_ARG;
    *count = c->scene->n;
    return GSR_OK;
}

int gsr_set_scene_sh(gsr_ctx* c, const uint32_t* sh_r, const uint32_t* sh_g, const uint32_t* sh_b, uint32_t sh_count,
                     const int32_t* band_index)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int r = sync_members(c)) return r;   // per-scene state: the textures every member's frames read are replaced
    if (int r = adopt_scene(c)) return r;    // (a generation this context has not followed yet is not skipped by the new one below)
    SharedScene& sc = *c->scene;
    sc.sh_count = 0; sc.band[0] = sc.band[1] = sc.band[2] = -1;
    sc.reset_sh_frame();   // new coefficients are in the scene's frame as it stands
    invalidate_members(c, false);
    c->scene_gen = ++sc.generation;
    if (!sh_count) return GSR_OK;
    if (!sh_r || !sh_g || !sh_b || !band_index) return fail(c, GSR_ERR_ARG, "SH texture or band_index pointer is NULL");
    if (band_index[0] < -1 || (uint64_t)(band_index[0] + 1) + sh_count != c->scene->n)
        return fail(c, GSR_ERR_SCENE, "sh_count (%u) must be vertexCount (%u) - (bandsIndices[0] + 1) (%d)", sh_count, c->scene->n,
                    band_index[0] + 1);
    int r;
    if ((r = sc.sh_r.alloc(c, (size_t)sh_count * 8)) || (r = sc.sh_g.alloc(c, (size_t)sh_count * 8)) ||
        (r = sc.sh_b.alloc(c, (size_t)sh_count * 8)) || (r = c->shcol.alloc(c, (size_t)c->scene->n)))
        return r;
    HIP_TRY(c, hipMemcpyAsync(sc.sh_r, sh_r, (size_t)sh_count * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.sh_g, sh_g, (size_t)sh_count * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.sh_b, sh_b, (size_t)sh_count * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->shcol, 0, (size_t)c->scene->n * sizeof(float4), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    sc.sh_count = sh_count;
    sc.sh_rows = sh_count;
    sc.band[0] = band_index[0]; sc.band[1] = band_index[1]; sc.band[2] = band_index[2];
    return GSR_OK;
}

int gsr_set_sh_follow(gsr_ctx* c, int32_t on)
{
    if (!c) return GSR_ERR_ARG;
    c->scene->sh_follow = on != 0;
    return GSR_OK;
}

int gsr_set_sh_frame(gsr_ctx* c, const double* linv)
{
    if (!c) return GSR_ERR_ARG;
    if (!c->scene->sh_count) return fail(c, GSR_ERR_ARG, "gsr_set_sh_frame: the scene has no SH state (call gsr_set_scene_sh first)");
    if (linv)
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(linv[k])) return fail(c, GSR_ERR_ARG, "gsr_set_sh_frame: entry %d is not finite", k);
    if (linv) for (int k = 0; k < 9; k++) c->scene->sh_frame[k] = linv[k];
    else c->scene->reset_sh_frame();
    invalidate_members(c, false);   // (the evaluated colours of the last frame are another frame's)
    return GSR_OK;
}

int gsr_get_sh_frame(gsr_ctx* c, double* linv, int32_t* follow)
{
    if (!c) return GSR_ERR_ARG;
    if (linv) for (int k = 0; k < 9; k++) linv[k] = c->scene->sh_frame[k];
    if (follow) *follow = c->scene->sh_follow ? 1 : 0;
    return GSR_OK;
}

int gsr_read_scene_sh(gsr_ctx* c, uint32_t* sh_r, uint32_t* sh_g, uint32_t* sh_b, uint32_t* sh_count, int32_t* band_index)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const SharedScene& sc = *c->scene;
    if (sh_count) *sh_count = sc.sh_count;
    if (band_index) for (int k = 0; k < 3; k++) band_index[k] = sc.band[k];
    if (!sc.sh_count || (!sh_r && !sh_g && !sh_b)) return GSR_OK;
    const size_t bytes = (size_t)sc.sh_count * 32;
    if (sh_r) HIP_TRY(c, hipMemcpyAsync(sh_r, sc.sh_r, bytes, hipMemcpyDeviceToHost, c->stream));
    if (sh_g) HIP_TRY(c, hipMemcpyAsync(sh_g, sc.sh_g, bytes, hipMemcpyDeviceToHost, c->stream));
    if (sh_b) HIP_TRY(c, hipMemcpyAsync(sh_b, sc.sh_b, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

}  // extern "C"
