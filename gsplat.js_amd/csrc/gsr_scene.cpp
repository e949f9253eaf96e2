// The scene on the device: upload (packed words, the Scene's four arrays or .splat rows), the transforms and the compaction of
// scenes that carry rotations and scales, spherical harmonics, and the scene's read-back.  alloc_scene sizes everything that holds one entry per splat.
#include "gsr_ctx.h"

using namespace gsr;

// (re)allocate everything sized by the splat count; clears SH and per-frame state
int gsr::alloc_scene(gsr_ctx* c, uint32_t n, bool with_rows)
{
    c->n = 0; c->have_frame = false; c->have_sort = false; c->scene.have_rows = false;
    c->bin.plan.form = BIN_FINALIZE_ONLY;   // (no splats until the caller's alloc_bins plans for the new count: a frame in between only finalizes)
    if (c->words.mailbox) reinterpret_cast<volatile uint32_t*>(c->words.mailbox)[2] = 0xffffffffu;   // a new scene: LSD order until a frame reports
    c->scene.drop_sh();
    gsr_ctx::Sort& so = c->sort;
    int r;
    if ((r = c->scene.arr.alloc(c, n, with_rows)) || (r = so.depth.alloc(c, n)) || (r = so.keys.alloc(c, n)) ||
        (r = so.keys_tmp.alloc(c, n)) || (r = so.idx_tmp.alloc(c, n)) || (r = so.depth_index.alloc(c, n)) || (r = so.rec.alloc(c, n)) ||
        (r = so.rects.alloc(c, n)) || (r = so.rect_idx.alloc(c, n)) || (r = so.rect_tmp.alloc(c, n)) ||
        (r = so.chunk_tab.alloc(c, 4 * ((size_t)n / 4096 + 260))) ||
        (r = so.kept.alloc(c, (size_t)n / PROJ_THREADS + 1)) || (r = so.kept_lane.alloc(c, n)) ||
        (r = so.koff.alloc(c, (size_t)n / PROJ_THREADS + 2)))
        return r;
    // keys per radix workgroup: the scatter stores runs of keys_per_block / 2^bits keys, so larger scenes take larger
    // blocks (longer runs) while small ones keep enough workgroups to fill the chip.  Measured at 20 M splats, the two
    // scatters: 135 + 126 us with 2048 keys, 99 + 98 us with 4096, 113 + 116 us with 8192 (96 KiB of LDS: one
    // workgroup per CU, nothing overlaps its load and store phases).
    so.kpb = c->knobs.sort_kpb ? c->knobs.sort_kpb : n <= (3u << 20) ? 2048 : 4096;
    so.blocks = (n + so.kpb - 1) / so.kpb;
    return so.block_hist.alloc(c, (size_t)std::max(so.blocks, 1u) * RADIX_HI_BINS);
}

namespace {

int need_rows(gsr_ctx* c)
{
    if (!c->scene.have_rows) return fail(c, GSR_ERR_ARG, "scene transforms need a scene built with gsr_set_scene_rows or gsr_set_scene_arrays");
    HIP_TRY(c, hipSetDevice(c->device));
    c->have_frame = false; c->have_sort = false;
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
        DevBuf<uint32_t> d_data, d_flag;
        DevBuf<float> d_pos, d_scl;
        if ((r = sa.alloc(c, n, with_rows)) || (r = d_data.alloc(c, (size_t)n * 8)) || (r = d_pos.alloc(c, (size_t)n * 3)) || (r = d_flag.alloc(c, 1))) return r;
        hipError_t e1 = hipMemcpyAsync(d_data, data, (size_t)n * 32, hipMemcpyHostToDevice, c->stream);
        hipError_t e2 = hipMemcpyAsync(d_pos, positions, (size_t)n * 12, hipMemcpyHostToDevice, c->stream);
        hipError_t e3 = hipMemsetAsync(d_flag, 0, 4, c->stream);
        launch_repack_scene(d_data, d_pos, n, sa.px, sa.py, sa.pz, sa.cov0, sa.cov1, sa.cov2, sa.rgba, d_flag, c->stream);
        hipError_t e6 = hipSuccess, e7 = hipSuccess;
        if (with_rows) {   // covariance words and colours stay the caller's; rotations are `rot`'s bytes already
            if ((r = d_scl.alloc(c, (size_t)n * 3))) return r;
            e6 = hipMemcpyAsync(sa.rot, rotations, (size_t)n * 16, hipMemcpyHostToDevice, c->stream);
            e7 = hipMemcpyAsync(d_scl, scales, (size_t)n * 12, hipMemcpyHostToDevice, c->stream);
            launch_scene_import(d_scl, n, sa.scl, c->stream);
        }
        uint32_t flag = 0;
        hipError_t e4 = hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream);
        hipError_t e5 = hipStreamSynchronize(c->stream);
        for (hipError_t e : {e1, e2, e3, e4, e5, e6, e7, hipGetLastError()})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "scene upload failed: %s", hipGetErrorString(e));
        if (flag) return fail(c, GSR_ERR_SCENE, "positions differ from data words 0..2 (Scene.ts:141-143 keeps them equal)");
    }
    if ((r = alloc_scene(c, n, with_rows))) return r;
    if (n) std::swap(c->scene.arr, sa);   // (the blank arrays alloc_scene made go with `sa`)
    c->n = n;
    c->scene.have_rows = with_rows;
    c->bin.capacity = 0;
    return alloc_bins(c);
}

}  // namespace

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
        launch_build_scene(d_rows, n, c->scene.arr.view(), c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        for (hipError_t e : {e1, e2, hipGetLastError()})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "scene build failed: %s", hipGetErrorString(e));
    }
    c->n = n;
    c->scene.have_rows = true;
    c->bin.capacity = 0;
    return alloc_bins(c);
}

int gsr_scene_translate(gsr_ctx* c, const double* t)
{
    if (!c || !t) return GSR_ERR_ARG;
    if (int r = need_rows(c)) return r;
    launch_scene_translate(c->n, c->scene.arr.view(), t, c->stream);
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

int gsr_scene_rotate(gsr_ctx* c, const double* q)
{
    if (!c || !q) return GSR_ERR_ARG;
    if (int r = need_rows(c)) return r;
    launch_scene_rotate(c->n, c->scene.arr.view(), q, c->stream);
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

int gsr_scene_scale(gsr_ctx* c, const double* sv)
{
    if (!c || !sv) return GSR_ERR_ARG;
    if (int r = need_rows(c)) return r;
    launch_scene_scale(c->n, c->scene.arr.view(), sv, c->stream);
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

int gsr_scene_limit_box(gsr_ctx* c, const double* box, uint32_t* new_count)
{
    if (!c || !box) return GSR_ERR_ARG;
    if (box[0] >= box[1]) return fail(c, GSR_ERR_ARG, "xMin (%g) must be smaller than xMax (%g)", box[0], box[1]);   // Scene.ts:308-316
    if (box[2] >= box[3]) return fail(c, GSR_ERR_ARG, "yMin (%g) must be smaller than yMax (%g)", box[2], box[3]);
    if (box[4] >= box[5]) return fail(c, GSR_ERR_ARG, "zMin (%g) must be smaller than zMax (%g)", box[4], box[5]);
    if (int r = need_rows(c)) return r;
    const uint32_t n = c->n;
    uint32_t kept = 0;
    if (n) {
        SceneArrays dst;   // the kept splats are compacted into a second set of arrays, which then becomes the scene
        DevBuf<uint32_t> block_count, total;
        int r;
        if ((r = dst.alloc(c, n, true)) || (r = block_count.alloc(c, (n + 1023) / 1024)) || (r = total.alloc(c, 1))) return r;
        launch_scene_limit_box(n, c->scene.arr.view(), dst.view(), box, block_count, total, c->stream);
        hipError_t e1 = hipMemcpyAsync(&kept, total, 4, hipMemcpyDeviceToHost, c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        for (hipError_t e : {e1, e2, hipGetLastError()})
            if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "limitBox failed: %s", hipGetErrorString(e));
        std::swap(c->scene.arr, dst);
        c->n = kept;   // arrays keep their old capacity; per-frame buffers sized for the old count still fit
        c->sort.blocks = (kept + c->sort.kpb - 1) / c->sort.kpb;
        // The compaction renumbers the splats, so SH rows (indexed by splat - (bandsIndices[0] + 1)) and the band
        // thresholds no longer belong to them: the SH state is dropped and the scene falls back to its rgba8 colours
        // until gsr_set_scene_sh is called again.  (Scene.limitBox, Scene.ts:307-366, leaves shs_rgb / bandsIndices
        // untouched, i.e. stale; a host that wants SH after limitBox re-packs them for the kept splats.)
        c->scene.drop_sh();
        // the binning's plan for the new count (plan_bins): fewer splats can mean fewer rounds and so MORE table rows, which
        // alloc_bins regrows; like every alloc_bins it drops what the last frame left in the lists (they index the old numbering)
        if ((r = alloc_bins(c))) return r;
    }
    if (new_count) *new_count = kept;
    return GSR_OK;
}

int gsr_read_scene(gsr_ctx* c, uint32_t* data, float* positions, float* rotations, float* scales, uint32_t* count)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n = c->n;
    if (count) *count = n;
    if (!data && !positions && !rotations && !scales) return GSR_OK;  // count only: nothing to copy
    if ((rotations || scales) && !c->scene.have_rows) return fail(c, GSR_ERR_ARG, "rotations/scales exist only for scenes built with gsr_set_scene_rows or gsr_set_scene_arrays");
    if (!n) return GSR_OK;
    // One kernel lays the requested parts out in the callers' layouts in one staging allocation (k_scene_export), then one copy
    // per output.  Rotations are copied from `rot` itself: it has Scene.rotations' layout.
    const size_t data_words = data ? 8 * (size_t)n : 0, pos_words = positions ? 3 * (size_t)n : 0, scl_words = scales ? 3 * (size_t)n : 0;
    DevBuf<uint32_t> stage;
    if (int r = stage.alloc(c, data_words + pos_words + scl_words)) return r;
    uint32_t* d_data = data ? (uint32_t*)stage : nullptr;
    float* d_pos = positions ? (float*)(stage + data_words) : nullptr;
    float* d_scl = scales ? (float*)(stage + data_words + pos_words) : nullptr;
    launch_scene_export(n, c->scene.arr.view(), d_data, d_pos, d_scl, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (data) HIP_TRY(c, hipMemcpyAsync(data, d_data, data_words * 4, hipMemcpyDeviceToHost, c->stream));
    if (positions) HIP_TRY(c, hipMemcpyAsync(positions, d_pos, pos_words * 4, hipMemcpyDeviceToHost, c->stream));
    if (rotations) HIP_TRY(c, hipMemcpyAsync(rotations, c->scene.arr.rot, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    if (scales) HIP_TRY(c, hipMemcpyAsync(scales, d_scl, scl_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int gsr_scene_count(gsr_ctx* c, uint32_t* count)
{
    if (!c || !count) return GSR_ERR_ARG;
    *count = c->n;
    return GSR_OK;
}

int gsr_set_scene_sh(gsr_ctx* c, const uint32_t* sh_r, const uint32_t* sh_g, const uint32_t* sh_b, uint32_t sh_count,
                     const int32_t* band_index)
{
    if (!c) return GSR_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    gsr_ctx::Scene& sc = c->scene;
    sc.sh_count = 0; sc.band[0] = sc.band[1] = sc.band[2] = -1;
    c->have_frame = false;
    if (!sh_count) return GSR_OK;
    if (!sh_r || !sh_g || !sh_b || !band_index) return fail(c, GSR_ERR_ARG, "SH texture or band_index pointer is NULL");
    if (band_index[0] < -1 || (uint64_t)(band_index[0] + 1) + sh_count != c->n)
        return fail(c, GSR_ERR_SCENE, "sh_count (%u) must be vertexCount (%u) - (bandsIndices[0] + 1) (%d)", sh_count, c->n,
                    band_index[0] + 1);
    int r;
    if ((r = sc.sh_r.alloc(c, (size_t)sh_count * 8)) || (r = sc.sh_g.alloc(c, (size_t)sh_count * 8)) ||
        (r = sc.sh_b.alloc(c, (size_t)sh_count * 8)) || (r = sc.shcol.alloc(c, (size_t)c->n)))
        return r;
    HIP_TRY(c, hipMemcpyAsync(sc.sh_r, sh_r, (size_t)sh_count * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.sh_g, sh_g, (size_t)sh_count * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.sh_b, sh_b, (size_t)sh_count * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(sc.shcol, 0, (size_t)c->n * sizeof(float4), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    sc.sh_count = sh_count;
    sc.band[0] = band_index[0]; sc.band[1] = band_index[1]; sc.band[2] = band_index[2];
    return GSR_OK;
}

}  // extern "C"
