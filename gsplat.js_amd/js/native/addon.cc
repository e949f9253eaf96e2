// gsplat_hip.node -- N-API (raw node_api.h, N-API <= 8, Node >= 12) binding of the C ABI in
// include/gsplat_hip.h.  TypedArray backing stores are handed to the library zero-copy for the duration of
// each call; nothing is retained.  Every failure becomes a JavaScript exception carrying gsr_last_error().
// The one thing handed the other way is the delivery ring: its pinned blocks become external ArrayBuffers (see DeliverySlots).
#include <node_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../../include/gsplat_hip.h"

namespace {

#define NAPI_OK_OR_NULL(env, call)                                    \
    do {                                                              \
        if ((call) != napi_ok) {                                      \
            napi_throw_error((env), nullptr, "N-API call failed: " #call); \
            return nullptr;                                           \
        }                                                             \
    } while (0)

napi_value throw_gsr(napi_env env, gsr_ctx* ctx, int rc, const char* what)
{
    char buf[768];
    snprintf(buf, sizeof buf, "%s failed (%d): %s", what, rc, gsr_last_error(ctx));
    napi_throw_error(env, "GSPLAT_HIP", buf);
    return nullptr;
}

void finalize_ctx(napi_env, void* data, void*)
{
    gsr_ctx** slot = static_cast<gsr_ctx**>(data);
    if (*slot) gsr_destroy(*slot);
    delete slot;
}

bool get_args(napi_env env, napi_callback_info info, size_t want, napi_value* argv)
{
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < want) {
        napi_throw_type_error(env, nullptr, "too few arguments");
        return false;
    }
    return true;
}

gsr_ctx* get_ctx(napi_env env, napi_value v)
{
    void* p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !*static_cast<gsr_ctx**>(p)) {
        napi_throw_type_error(env, nullptr, "expected a live renderer handle");
        return nullptr;
    }
    return *static_cast<gsr_ctx**>(p);
}

// data pointer + element count of a TypedArray of the given type (nullptr allowed when `optional`)
bool get_typed(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* len, bool optional = false)
{
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (optional && (t == napi_undefined || t == napi_null)) { *data = nullptr; *len = 0; return true; }
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    napi_typedarray_type type;
    napi_value ab;
    size_t off;
    if (!is_ta || napi_get_typedarray_info(env, v, &type, len, data, &ab, &off) != napi_ok || type != want) {
        napi_throw_type_error(env, nullptr, "wrong TypedArray type");
        return false;
    }
    return true;
}

bool get_i32(napi_env env, napi_value v, int32_t* out) { return napi_get_value_int32(env, v, out) == napi_ok; }
bool get_f64(napi_env env, napi_value v, double* out) { return napi_get_value_double(env, v, out) == napi_ok; }

napi_value undefined(napi_env env) { napi_value u; napi_get_undefined(env, &u); return u; }

// create({device,width,height,earlyOutEps,bandX0,bandX1,timing,throughput}) -> handle
napi_value Create(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_options o;
    memset(&o, 0, sizeof o);
    auto num = [&](const char* key, double dflt) {
        napi_value v;
        bool has = false;
        double d = dflt;
        if (napi_has_named_property(env, argv[0], key, &has) == napi_ok && has &&
            napi_get_named_property(env, argv[0], key, &v) == napi_ok)
            napi_get_value_double(env, v, &d);
        return d;
    };
    o.device = (int32_t)num("device", 0);
    o.width = (int32_t)num("width", 0);
    o.height = (int32_t)num("height", 0);
    o.early_out_eps = (float)num("earlyOutEps", 0);
    o.band_x0 = (int32_t)num("bandX0", 0);
    o.band_x1 = (int32_t)num("bandX1", 0);
    o.flags = (num("timing", 0) != 0 ? GSR_FLAG_TIMING : 0) | (num("throughput", 0) != 0 ? GSR_FLAG_THROUGHPUT : 0);
    gsr_ctx* ctx = nullptr;
    const int rc = gsr_create(&ctx, &o);
    if (rc != GSR_OK) return throw_gsr(env, nullptr, rc, "gsr_create");
    gsr_ctx** slot = new gsr_ctx*(ctx);
    napi_value ext;
    if (napi_create_external(env, slot, finalize_ctx, nullptr, &ext) != napi_ok) {
        gsr_destroy(ctx);
        delete slot;
        napi_throw_error(env, nullptr, "napi_create_external failed");
        return nullptr;
    }
    return ext;
}

napi_value Destroy(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    void* p = nullptr;
    if (napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
        gsr_ctx** slot = static_cast<gsr_ctx**>(p);
        if (*slot) { gsr_destroy(*slot); *slot = nullptr; }
    }
    return undefined(env);
}

napi_value SetScene(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    void *data, *pos;
    size_t nd, np;
    int32_t n;
    if (!get_typed(env, argv[1], napi_uint32_array, &data, &nd) || !get_typed(env, argv[2], napi_float32_array, &pos, &np) ||
        !get_i32(env, argv[3], &n))
        return nullptr;
    if (n < 0 || nd < (size_t)n * 8 || np < (size_t)n * 3) {
        napi_throw_range_error(env, nullptr, "scene buffers are smaller than vertexCount requires");
        return nullptr;
    }
    const int rc = gsr_set_scene(c, (const uint32_t*)data, (const float*)pos, (uint32_t)n);
    return rc ? throw_gsr(env, c, rc, "gsr_set_scene") : undefined(env);
}

// setSceneSh(handle, Uint32Array r, Uint32Array g, Uint32Array b, shCount, Int32Array bandsIndices)
napi_value SetSceneSh(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    void *t[3], *band;
    size_t len[3], nb;
    int32_t count;
    for (int k = 0; k < 3; k++)
        if (!get_typed(env, argv[1 + k], napi_uint32_array, &t[k], &len[k])) return nullptr;
    if (!get_i32(env, argv[4], &count) || !get_typed(env, argv[5], napi_int32_array, &band, &nb)) return nullptr;
    if (count < 0 || nb < 3 || len[0] < (size_t)count * 8 || len[1] < (size_t)count * 8 || len[2] < (size_t)count * 8) {
        napi_throw_range_error(env, nullptr, "SH buffers are smaller than shCount requires");
        return nullptr;
    }
    const int rc = gsr_set_scene_sh(c, (const uint32_t*)t[0], (const uint32_t*)t[1], (const uint32_t*)t[2], (uint32_t)count,
                                    (const int32_t*)band);
    return rc ? throw_gsr(env, c, rc, "gsr_set_scene_sh") : undefined(env);
}

// setSceneRows(handle, Uint8Array rows)
napi_value SetSceneRows(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* rows;
    size_t len;
    if (!c || !get_typed(env, argv[1], napi_uint8_array, &rows, &len)) return nullptr;
    if (len % 32) { napi_throw_range_error(env, nullptr, "rows length must be a multiple of 32"); return nullptr; }
    const int rc = gsr_set_scene_rows(c, (const uint8_t*)rows, (uint32_t)(len / 32));
    return rc ? throw_gsr(env, c, rc, "gsr_set_scene_rows") : undefined(env);
}

// setSceneArrays(handle, Uint32Array data, Float32Array positions, Float32Array rotations, Float32Array scales, vertexCount)
napi_value SetSceneArrays(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    void *data, *pos, *rot, *scl;
    size_t nd, np, nr, ns;
    int32_t n;
    if (!get_typed(env, argv[1], napi_uint32_array, &data, &nd) || !get_typed(env, argv[2], napi_float32_array, &pos, &np) ||
        !get_typed(env, argv[3], napi_float32_array, &rot, &nr) || !get_typed(env, argv[4], napi_float32_array, &scl, &ns) || !get_i32(env, argv[5], &n))
        return nullptr;
    if (n < 0 || nd < (size_t)n * 8 || np < (size_t)n * 3 || nr < (size_t)n * 4 || ns < (size_t)n * 3) {
        napi_throw_range_error(env, nullptr, "scene buffers are smaller than vertexCount requires");
        return nullptr;
    }
    const int rc = gsr_set_scene_arrays(c, (const uint32_t*)data, (const float*)pos, (const float*)rot, (const float*)scl, (uint32_t)n);
    return rc ? throw_gsr(env, c, rc, "gsr_set_scene_arrays") : undefined(env);
}

// sceneTransform(handle, kind, Float64Array args): kind 0 translate(3) 1 rotate(4: x,y,z,w) 2 scale(3) 3 limitBox(6) -> new count
napi_value SceneTransform(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t kind;
    void* a;
    size_t len;
    if (!c || !get_i32(env, argv[1], &kind) || !get_typed(env, argv[2], napi_float64_array, &a, &len)) return nullptr;
    static const size_t need[4] = {3, 4, 3, 6};
    if (kind < 0 || kind > 3 || len < need[kind]) { napi_throw_range_error(env, nullptr, "bad transform arguments"); return nullptr; }
    uint32_t count = 0;
    int rc;
    const double* d = (const double*)a;
    if (kind == 0) rc = gsr_scene_translate(c, d);
    else if (kind == 1) rc = gsr_scene_rotate(c, d);
    else if (kind == 2) rc = gsr_scene_scale(c, d);
    else rc = gsr_scene_limit_box(c, d, &count);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene transform");
    if (kind != 3) gsr_scene_count(c, &count);   // no copy: the transforms exist to keep the scene on the device
    napi_value n;
    napi_create_uint32(env, count, &n);
    return n;
}

// readScene(handle, Uint32Array data | null, Float32Array positions | null) -> count
napi_value ReadScene(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void *data, *pos;
    size_t nd, np;
    if (!c || !get_typed(env, argv[1], napi_uint32_array, &data, &nd, true) || !get_typed(env, argv[2], napi_float32_array, &pos, &np, true))
        return nullptr;
    uint32_t count = 0;
    int rc = gsr_scene_count(c, &count);
    if (!rc) {
        if ((data && nd < (size_t)count * 8) || (pos && np < (size_t)count * 3)) {
            napi_throw_range_error(env, nullptr, "output arrays are smaller than the scene");
            return nullptr;
        }
        rc = gsr_read_scene(c, (uint32_t*)data, (float*)pos, nullptr, nullptr, &count);
    }
    if (rc) return throw_gsr(env, c, rc, "gsr_read_scene");
    napi_value n;
    napi_create_uint32(env, count, &n);
    return n;
}

// readSceneArrays(handle, Uint32Array data | null, Float32Array positions | null, Float32Array rotations | null, Float32Array scales | null) -> count
napi_value ReadSceneArrays(napi_env env, napi_callback_info info)
{
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void *data, *out[3];
    size_t nd, len[3];
    if (!c || !get_typed(env, argv[1], napi_uint32_array, &data, &nd, true)) return nullptr;
    for (int k = 0; k < 3; k++)
        if (!get_typed(env, argv[2 + k], napi_float32_array, &out[k], &len[k], true)) return nullptr;
    uint32_t count = 0;
    int rc = gsr_scene_count(c, &count);
    if (!rc) {
        if ((data && nd < (size_t)count * 8) || (out[0] && len[0] < (size_t)count * 3) || (out[1] && len[1] < (size_t)count * 4) ||
            (out[2] && len[2] < (size_t)count * 3)) {
            napi_throw_range_error(env, nullptr, "output arrays are smaller than the scene");
            return nullptr;
        }
        rc = gsr_read_scene(c, (uint32_t*)data, (float*)out[0], (float*)out[1], (float*)out[2], &count);
    }
    if (rc) return throw_gsr(env, c, rc, "gsr_read_scene");
    napi_value n;
    napi_create_uint32(env, count, &n);
    return n;
}

// setShFollow(handle, on)
napi_value SetShFollow(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t on;
    if (!c || !get_i32(env, argv[1], &on)) return nullptr;
    const int rc = gsr_set_sh_follow(c, on);
    return rc ? throw_gsr(env, c, rc, "gsr_set_sh_follow") : undefined(env);
}

// setShFrame(handle, Float64Array(9) | null)
napi_value SetShFrame(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* m;
    size_t len;
    if (!c || !get_typed(env, argv[1], napi_float64_array, &m, &len, true)) return nullptr;
    if (m && len < 9) { napi_throw_range_error(env, nullptr, "the SH frame has 9 entries"); return nullptr; }
    const int rc = gsr_set_sh_frame(c, (const double*)m);
    return rc ? throw_gsr(env, c, rc, "gsr_set_sh_frame") : undefined(env);
}

// getShFrame(handle, Float64Array(9) out) -> follow (0 / 1)
napi_value GetShFrame(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* m;
    size_t len;
    if (!c || !get_typed(env, argv[1], napi_float64_array, &m, &len)) return nullptr;
    if (len < 9) { napi_throw_range_error(env, nullptr, "the SH frame has 9 entries"); return nullptr; }
    int32_t follow = 0;
    const int rc = gsr_get_sh_frame(c, (double*)m, &follow);
    if (rc) return throw_gsr(env, c, rc, "gsr_get_sh_frame");
    napi_value n;
    napi_create_int32(env, follow, &n);
    return n;
}

// readSceneSh(handle, Uint32Array r | null, Uint32Array g | null, Uint32Array b | null, Int32Array(3) bandsIndices) -> shCount
napi_value ReadSceneSh(napi_env env, napi_callback_info info)
{
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void *t[3], *band;
    size_t len[3], nb;
    if (!c) return nullptr;
    for (int k = 0; k < 3; k++)
        if (!get_typed(env, argv[1 + k], napi_uint32_array, &t[k], &len[k], true)) return nullptr;
    if (!get_typed(env, argv[4], napi_int32_array, &band, &nb)) return nullptr;
    uint32_t count = 0;
    int rc = gsr_read_scene_sh(c, nullptr, nullptr, nullptr, &count, nullptr);
    if (!rc) {
        if (nb < 3 || (t[0] && len[0] < (size_t)count * 8) || (t[1] && len[1] < (size_t)count * 8) || (t[2] && len[2] < (size_t)count * 8)) {
            napi_throw_range_error(env, nullptr, "output arrays are smaller than the SH state");
            return nullptr;
        }
        rc = gsr_read_scene_sh(c, (uint32_t*)t[0], (uint32_t*)t[1], (uint32_t*)t[2], &count, (int32_t*)band);
    }
    if (rc) return throw_gsr(env, c, rc, "gsr_read_scene_sh");
    napi_value n;
    napi_create_uint32(env, count, &n);
    return n;
}

napi_value SetDepthFade(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t use;
    double v;
    if (!c || !get_i32(env, argv[1], &use) || !get_f64(env, argv[2], &v)) return nullptr;
    const int rc = gsr_set_depth_fade(c, use, (float)v);
    return rc ? throw_gsr(env, c, rc, "gsr_set_depth_fade") : undefined(env);
}

napi_value Resize(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t w, h;
    if (!c || !get_i32(env, argv[1], &w) || !get_i32(env, argv[2], &h)) return nullptr;
    const int rc = gsr_resize(c, w, h);
    return rc ? throw_gsr(env, c, rc, "gsr_resize") : undefined(env);
}

napi_value SetBand(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t x0, x1;
    if (!c || !get_i32(env, argv[1], &x0) || !get_i32(env, argv[2], &x1)) return nullptr;
    const int rc = gsr_set_band(c, x0, x1);
    return rc ? throw_gsr(env, c, rc, "gsr_set_band") : undefined(env);
}

// setCamera(handle, Float32Array view, Float32Array proj, Float32Array viewProj, fx, fy)
napi_value SetCamera(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    void* m[3];
    size_t len;
    for (int k = 0; k < 3; k++) {
        if (!get_typed(env, argv[1 + k], napi_float32_array, &m[k], &len)) return nullptr;
        if (len < 16) { napi_throw_range_error(env, nullptr, "matrix needs 16 elements"); return nullptr; }
    }
    double fx, fy;
    if (!get_f64(env, argv[4], &fx) || !get_f64(env, argv[5], &fy)) return nullptr;
    const int rc = gsr_set_camera(c, (const float*)m[0], (const float*)m[1], (const float*)m[2], (float)fx, (float)fy);
    return rc ? throw_gsr(env, c, rc, "gsr_set_camera") : undefined(env);
}

template <int (*FN)(gsr_ctx*)>
napi_value Call0(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    const int rc = FN(c);
    return rc ? throw_gsr(env, c, rc, "libgsplat_hip call") : undefined(env);
}

napi_value ReadDepthIndex(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* out;
    size_t len;
    if (!c || !get_typed(env, argv[1], napi_uint32_array, &out, &len)) return nullptr;
    uint32_t n = 0;
    gsr_scene_count(c, &n);
    if (len < n) { napi_throw_range_error(env, nullptr, "output array is smaller than vertexCount"); return nullptr; }
    const int rc = gsr_read_depth_index(c, (uint32_t*)out);
    return rc ? throw_gsr(env, c, rc, "gsr_read_depth_index") : undefined(env);
}

// readPixels(handle, out, width, height): out is Float32Array (RGBA f32) or Uint8Array (RGBA8)
napi_value ReadPixels(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    int32_t w, h;
    if (!get_i32(env, argv[2], &w) || !get_i32(env, argv[3], &h)) return nullptr;
    napi_typedarray_type type;
    size_t len, off;
    void* data;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[1], &type, &len, &data, &ab, &off) != napi_ok) {
        napi_throw_type_error(env, nullptr, "expected a TypedArray");
        return nullptr;
    }
    if (len < (size_t)w * h * 4) { napi_throw_range_error(env, nullptr, "output array is smaller than width*height*4"); return nullptr; }
    int rc;
    if (type == napi_float32_array) rc = gsr_read_pixels_rgba32f(c, (float*)data);
    else if (type == napi_uint8_array || type == napi_uint8_clamped_array) rc = gsr_read_pixels_rgba8(c, (uint8_t*)data);
    else { napi_throw_type_error(env, nullptr, "expected Float32Array or Uint8Array"); return nullptr; }
    return rc ? throw_gsr(env, c, rc, "gsr_read_pixels") : undefined(env);
}

napi_value GetTimings(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    gsr_timings t;
    const int rc = gsr_get_timings(c, &t);
    if (rc) return throw_gsr(env, c, rc, "gsr_get_timings");
    napi_value o;
    NAPI_OK_OR_NULL(env, napi_create_object(env, &o));
    auto put = [&](const char* k, double v) {
        napi_value n;
        napi_create_double(env, v, &n);
        napi_set_named_property(env, o, k, n);
    };
    put("msProjectKey", t.ms_project_key); put("msSort", t.ms_sort); put("msBin", t.ms_bin); put("msBlend", t.ms_blend); put("msCombine", t.ms_combine);
    put("msTotal", t.ms_total); put("visible", (double)t.visible); put("binEntries", (double)t.bin_entries);
    put("tileEntries", (double)t.tile_entries); put("n", t.n); put("frames", t.frames);
    put("sumMsProjectKey", t.sum_ms_project_key); put("sumMsSort", t.sum_ms_sort); put("sumMsBin", t.sum_ms_bin);
    put("sumMsBlend", t.sum_ms_blend); put("sumMsCombine", t.sum_ms_combine); put("sumMsTotal", t.sum_ms_total);
    put("overflowFrames", (double)t.overflow_frames); put("droppedFrames", (double)t.dropped_frames);
    return o;
}

// overflowPending(handle) -> boolean
napi_value OverflowPending(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    napi_value b;
    napi_get_boolean(env, gsr_overflow_pending(c) != 0, &b);
    return b;
}

// setListCapacity(handle, entries): tuning/test hook
napi_value SetListCapacity(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double v;
    if (!c || !get_f64(env, argv[1], &v)) return nullptr;
    const int rc = gsr_set_list_capacity(c, v < 0 ? 0u : (uint32_t)v);
    return rc ? throw_gsr(env, c, rc, "gsr_set_list_capacity") : undefined(env);
}

// commUniqueId() -> Uint8Array(128): rank 0 makes it, the host hands it to the other ranks
napi_value CommUniqueId(napi_env env, napi_callback_info)
{
    uint8_t id[GSR_COMM_ID_BYTES];
    const int rc = gsr_comm_unique_id(id);
    if (rc) return throw_gsr(env, nullptr, rc, "gsr_comm_unique_id");
    napi_value ab, out;
    void* data = nullptr;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, GSR_COMM_ID_BYTES, &data, &ab));
    memcpy(data, id, GSR_COMM_ID_BYTES);
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint8_array, GSR_COMM_ID_BYTES, ab, 0, &out));
    return out;
}

// commInit(handle, Uint8Array id, rank, world, Int32Array x0, Int32Array x1): collective
napi_value CommInit(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    void *id, *x0, *x1;
    size_t nid, n0, n1;
    int32_t rank, world;
    if (!get_typed(env, argv[1], napi_uint8_array, &id, &nid) || !get_i32(env, argv[2], &rank) || !get_i32(env, argv[3], &world) ||
        !get_typed(env, argv[4], napi_int32_array, &x0, &n0) || !get_typed(env, argv[5], napi_int32_array, &x1, &n1))
        return nullptr;
    if (nid < GSR_COMM_ID_BYTES || world < 1 || n0 < (size_t)world || n1 < (size_t)world) {
        napi_throw_range_error(env, nullptr, "commInit: id needs 128 bytes, x0/x1 one entry per rank");
        return nullptr;
    }
    const int rc = gsr_comm_init(c, (const uint8_t*)id, rank, world, (const int32_t*)x0, (const int32_t*)x1);
    return rc ? throw_gsr(env, c, rc, "gsr_comm_init") : undefined(env);
}

// commShare(handle, leaderHandle): this context joins the group the leader has joined (same rank: another frame in flight)
napi_value CommShare(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    gsr_ctx* leader = get_ctx(env, argv[1]);
    if (!c || !leader) return nullptr;
    const int rc = gsr_comm_share(c, leader);
    return rc ? throw_gsr(env, c, rc, "gsr_comm_share") : undefined(env);
}

// shareScene(handle, fromHandle) -> vertexCount: gsr_share_scene, then the shared scene's count
napi_value ShareScene(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    gsr_ctx* from = get_ctx(env, argv[1]);
    if (!c || !from) return nullptr;
    const int rc = gsr_share_scene(c, from);
    if (rc) return throw_gsr(env, c, rc, "gsr_share_scene");
    uint32_t count = 0;
    gsr_scene_count(c, &count);
    napi_value n;
    napi_create_uint32(env, count, &n);
    return n;
}

// sceneSharing(handle) -> { members, sceneBytes }
napi_value SceneSharing(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    int32_t members = 0;
    uint64_t bytes = 0;
    const int rc = gsr_scene_sharing(c, &members, &bytes);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_sharing");
    napi_value o, m, b;
    napi_create_object(env, &o);
    napi_create_int32(env, members, &m);
    napi_create_double(env, (double)bytes, &b);
    napi_set_named_property(env, o, "members", m);
    napi_set_named_property(env, o, "sceneBytes", b);
    return o;
}

// readFrame(handle, Uint8Array out, width, height): the gathered RGBA8 frame
napi_value ReadFrame(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* out;
    size_t len;
    int32_t w, h;
    if (!c || !get_typed(env, argv[1], napi_uint8_array, &out, &len) || !get_i32(env, argv[2], &w) || !get_i32(env, argv[3], &h)) return nullptr;
    if (len < (size_t)w * h * 4) { napi_throw_range_error(env, nullptr, "output array is smaller than width*height*4"); return nullptr; }
    const int rc = gsr_read_frame_rgba8(c, (uint8_t*)out);
    return rc ? throw_gsr(env, c, rc, "gsr_read_frame_rgba8") : undefined(env);
}

// ---- depth in a group (gsr_comm_set_depth) ----
// commSetDepth(handle, format 0 | 1 | 2, step, near): 0 switches the option off
napi_value CommSetDepth(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t format, step;
    double near;
    if (!c || !get_i32(env, argv[1], &format) || !get_i32(env, argv[2], &step)) return nullptr;
    if (!get_f64(env, argv[3], &near)) { napi_throw_type_error(env, nullptr, "commSetDepth: near must be a number"); return nullptr; }
    const gsr_depth_delivery_options d{format, step, (float)near, 0};
    const int rc = gsr_comm_set_depth(c, format == GSR_DEPTH_NONE ? nullptr : &d);
    return rc ? throw_gsr(env, c, rc, "gsr_comm_set_depth") : undefined(env);
}

// frameDepthLayout(handle) -> depthLayout's object for the gathered plane (offset 0)
napi_value FrameDepthLayout(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    gsr_depth_layout dl;
    const int rc = gsr_frame_depth_layout(c, &dl);
    if (rc) return throw_gsr(env, c, rc, "gsr_frame_depth_layout");
    auto set = [&](napi_value obj, const char* key, double value) {
        napi_value v;
        return napi_create_double(env, value, &v) == napi_ok && napi_set_named_property(env, obj, key, v) == napi_ok;
    };
    napi_value out;
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    if (!(set(out, "format", dl.format) && set(out, "step", dl.step) && set(out, "width", dl.width) && set(out, "height", dl.height) &&
          set(out, "stride", dl.stride) && set(out, "offset", (double)dl.offset) && set(out, "bytes", (double)dl.bytes) && set(out, "near", dl.near))) {
        napi_throw_error(env, nullptr, "frameDepthLayout: building the result failed");
        return nullptr;
    }
    return out;
}

// readFrameDepth(handle, Uint8Array out): the gathered plane's bytes
napi_value ReadFrameDepth(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* out;
    size_t len;
    if (!c || !get_typed(env, argv[1], napi_uint8_array, &out, &len)) return nullptr;
    const int rc = gsr_read_frame_depth(c, out, (uint64_t)len);
    return rc ? throw_gsr(env, c, rc, "gsr_read_frame_depth") : undefined(env);
}

// ---- frame delivery (gsr_delivery_*): the ring's pinned blocks as external ArrayBuffers, wrapped ONCE per slot ----
// An ArrayBuffer must never outlive the block it views.  Two guards: (1) every ArrayBuffer holds a reference to the renderer
// handle until it is collected, so a renderer that is merely dropped keeps its context (and ring) alive as long as any
// `pixels` view is reachable; (2) before the ring is freed or reallocated on purpose (closeDelivery, setSize, dispose) the
// JavaScript side hands the buffers to detachBuffers(): a detached ArrayBuffer has length 0 and its views read nothing.
void release_handle_ref(napi_env env, void*, void* hint)
{
    if (hint) napi_delete_reference(env, static_cast<napi_ref>(hint));
}

// deliverySlots(handle) -> [ArrayBuffer, ...], one per slot of the open ring: the colour payload (a depth ring: up to the depth plane's end)
napi_value DeliverySlots(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    napi_value arr;
    NAPI_OK_OR_NULL(env, napi_create_array(env, &arr));
    for (int32_t k = 0;; k++) {
        uint64_t bytes = 0;
        void* p = gsr_delivery_slot_ptr(c, k, &bytes);
        if (!p) break;
        gsr_depth_layout dl;   // a depth ring: the buffer spans the colour payload AND the depth plane behind it
        if (gsr_delivery_depth_layout(c, &dl) == GSR_OK) bytes = dl.offset + dl.bytes;
        napi_ref keep = nullptr;
        NAPI_OK_OR_NULL(env, napi_create_reference(env, argv[0], 1, &keep));
        napi_value ab;
        if (napi_create_external_arraybuffer(env, p, (size_t)bytes, release_handle_ref, keep, &ab) != napi_ok) {
            napi_delete_reference(env, keep);
            napi_throw_error(env, nullptr, "napi_create_external_arraybuffer failed");
            return nullptr;
        }
        NAPI_OK_OR_NULL(env, napi_set_element(env, arr, (uint32_t)k, ab));
    }
    return arr;
}

// openDelivery(handle, slots) -> [ArrayBuffer, ...]
napi_value OpenDelivery(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t slots;
    if (!c || !get_i32(env, argv[1], &slots)) return nullptr;
    const int rc = gsr_delivery_open(c, slots);
    if (rc) return throw_gsr(env, c, rc, "gsr_delivery_open");
    return DeliverySlots(env, info);
}

// openDeliveryEx(handle, slots, format, fullRange, bgR, bgG, bgB) -> [ArrayBuffer, ...]: a ring in GSR_FORMAT_* (gsr_delivery_open_ex)
napi_value OpenDeliveryEx(napi_env env, napi_callback_info info)
{
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t v[6];
    if (!c) return nullptr;
    for (int k = 0; k < 6; k++)
        if (!get_i32(env, argv[1 + k], &v[k])) { napi_throw_type_error(env, nullptr, "openDeliveryEx(handle, slots, format, fullRange, r, g, b)"); return nullptr; }
    gsr_delivery_options opt{};
    opt.slots = v[0]; opt.format = v[1]; opt.full_range = v[2];
    for (int k = 0; k < 3; k++) opt.background[k] = (uint8_t)std::min(255, std::max(0, v[3 + k]));
    const int rc = gsr_delivery_open_ex(c, &opt);
    if (rc) return throw_gsr(env, c, rc, "gsr_delivery_open_ex");
    return DeliverySlots(env, info);
}

// openDeliveryDepth(handle, slots, format, fullRange, bgR, bgG, bgB, depthFormat, depthStep, depthNear) -> [ArrayBuffer, ...]: openDeliveryEx's
// ring with a depth plane in GSR_DEPTH_* beside every frame (gsr_delivery_open_depth)
napi_value OpenDeliveryDepth(napi_env env, napi_callback_info info)
{
    napi_value argv[10];
    if (!get_args(env, info, 10, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t v[8];
    double near = 0;
    if (!c) return nullptr;
    for (int k = 0; k < 8; k++)
        if (!get_i32(env, argv[1 + k], &v[k])) { napi_throw_type_error(env, nullptr, "openDeliveryDepth(handle, slots, format, fullRange, r, g, b, depthFormat, depthStep, depthNear)"); return nullptr; }
    if (!get_f64(env, argv[9], &near)) { napi_throw_type_error(env, nullptr, "openDeliveryDepth: depthNear must be a number"); return nullptr; }
    gsr_delivery_options opt{};
    opt.slots = v[0]; opt.format = v[1]; opt.full_range = v[2];
    for (int k = 0; k < 3; k++) opt.background[k] = (uint8_t)std::min(255, std::max(0, v[3 + k]));
    gsr_depth_delivery_options depth{};
    depth.format = v[6]; depth.step = v[7]; depth.near = (float)near;
    const int rc = gsr_delivery_open_depth(c, &opt, &depth);
    if (rc) return throw_gsr(env, c, rc, "gsr_delivery_open_depth");
    return DeliverySlots(env, info);
}

// depthLayout(handle) -> { format, step, width, height, stride, offset, bytes, near } of the open depth ring
napi_value DepthLayout(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    gsr_depth_layout dl;
    const int rc = gsr_delivery_depth_layout(c, &dl);
    if (rc) return throw_gsr(env, c, rc, "gsr_delivery_depth_layout");
    auto set = [&](napi_value obj, const char* key, double value) {
        napi_value v;
        return napi_create_double(env, value, &v) == napi_ok && napi_set_named_property(env, obj, key, v) == napi_ok;
    };
    napi_value out;
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    if (!(set(out, "format", dl.format) && set(out, "step", dl.step) && set(out, "width", dl.width) && set(out, "height", dl.height) &&
          set(out, "stride", dl.stride) && set(out, "offset", (double)dl.offset) && set(out, "bytes", (double)dl.bytes) && set(out, "near", dl.near))) {
        napi_throw_error(env, nullptr, "depthLayout: building the result failed");
        return nullptr;
    }
    return out;
}

// deliveryLayout(handle) -> { format, width, height, bytes, planes: [{ offset, stride, rows }, ...] } of the open ring
napi_value DeliveryLayout(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    gsr_frame_layout lay;
    const int rc = gsr_delivery_layout(c, &lay);
    if (rc) return throw_gsr(env, c, rc, "gsr_delivery_layout");
    auto set = [&](napi_value obj, const char* key, double value) {
        napi_value v;
        return napi_create_double(env, value, &v) == napi_ok && napi_set_named_property(env, obj, key, v) == napi_ok;
    };
    napi_value out, planes;
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_create_array(env, &planes));
    bool ok = set(out, "format", lay.format) && set(out, "width", lay.width) && set(out, "height", lay.height) && set(out, "bytes", (double)lay.bytes);
    for (int32_t k = 0; ok && k < lay.planes; k++) {
        napi_value pl;
        ok = napi_create_object(env, &pl) == napi_ok && set(pl, "offset", (double)lay.offset[k]) && set(pl, "stride", lay.stride[k]) &&
             set(pl, "rows", lay.rows[k]) && napi_set_element(env, planes, (uint32_t)k, pl) == napi_ok;
    }
    if (!ok || napi_set_named_property(env, out, "planes", planes) != napi_ok) { napi_throw_error(env, nullptr, "deliveryLayout: building the result failed"); return nullptr; }
    return out;
}

// detachBuffers([ArrayBuffer, ...]): the blocks behind them are about to be freed
napi_value DetachBuffers(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    uint32_t n = 0;
    if (napi_get_array_length(env, argv[0], &n) != napi_ok) { napi_throw_type_error(env, nullptr, "expected an array of ArrayBuffers"); return nullptr; }
    for (uint32_t k = 0; k < n; k++) {
        napi_value ab;
        bool detached = false;
        NAPI_OK_OR_NULL(env, napi_get_element(env, argv[0], k, &ab));
        if (napi_is_detached_arraybuffer(env, ab, &detached) == napi_ok && detached) continue;
        NAPI_OK_OR_NULL(env, napi_detach_arraybuffer(env, ab));
    }
    return undefined(env);
}

// deliverFrame(handle) -> serial (a Number: 2^53 frames are out of reach)
napi_value DeliverFrame(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    uint64_t serial = 0;
    const int rc = gsr_deliver_frame_async(c, &serial);
    if (rc) return throw_gsr(env, c, rc, "gsr_deliver_frame_async");
    napi_value v;
    NAPI_OK_OR_NULL(env, napi_create_double(env, (double)serial, &v));
    return v;
}

bool get_serial(napi_env env, napi_value v, uint64_t* out)
{
    double d = 0;
    if (!get_f64(env, v, &d) || d < 0) { napi_throw_type_error(env, nullptr, "expected a frame serial"); return false; }
    *out = (uint64_t)d;
    return true;
}

// frameReady(handle, serial) -> boolean
napi_value FrameReady(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    uint64_t serial;
    if (!c || !get_serial(env, argv[1], &serial)) return nullptr;
    const int rc = gsr_frame_ready(c, serial);
    if (rc < 0) return throw_gsr(env, c, rc, "gsr_frame_ready");
    napi_value b;
    NAPI_OK_OR_NULL(env, napi_get_boolean(env, rc != 0, &b));
    return b;
}

// acquireFrame(handle, serial) -> [serial, slot]
napi_value AcquireFrame(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    uint64_t serial;
    if (!c || !get_serial(env, argv[1], &serial)) return nullptr;
    gsr_frame f;
    const int rc = gsr_acquire_frame(c, serial, &f);
    if (rc) return throw_gsr(env, c, rc, "gsr_acquire_frame");
    napi_value arr, a, b;
    NAPI_OK_OR_NULL(env, napi_create_array_with_length(env, 2, &arr));
    NAPI_OK_OR_NULL(env, napi_create_double(env, (double)f.serial, &a));
    NAPI_OK_OR_NULL(env, napi_create_int32(env, f.slot, &b));
    NAPI_OK_OR_NULL(env, napi_set_element(env, arr, 0, a));
    NAPI_OK_OR_NULL(env, napi_set_element(env, arr, 1, b));
    return arr;
}

napi_value ReleaseFrame(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    uint64_t serial;
    if (!c || !get_serial(env, argv[1], &serial)) return nullptr;
    const int rc = gsr_release_frame(c, serial);
    return rc ? throw_gsr(env, c, rc, "gsr_release_frame") : undefined(env);
}

napi_value BuildId(napi_env env, napi_callback_info)
{
    napi_value s;
    napi_create_string_utf8(env, gsr_build_id(), NAPI_AUTO_LENGTH, &s);
    return s;
}

napi_value DeviceInfo(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    char name[256] = {0};
    int32_t cus = 0, khz = 0;
    const int rc = gsr_device_info(c, name, sizeof name, &cus, &khz);
    if (rc) return throw_gsr(env, c, rc, "gsr_device_info");
    napi_value o, s, a, b;
    NAPI_OK_OR_NULL(env, napi_create_object(env, &o));
    napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &s);
    napi_create_int32(env, cus, &a);
    napi_create_int32(env, khz, &b);
    napi_set_named_property(env, o, "name", s);
    napi_set_named_property(env, o, "computeUnits", a);
    napi_set_named_property(env, o, "clockKhz", b);
    return o;
}

// sortHost(viewProj f32[16], vertexCount, fBuffer f32, depthBuffer u32|null, depthIndex u32): the 7-argument wasm
// export of wasm/wasm.cpp:8-13 (starts/counts are scratch the device path does not need)
napi_value SortHost(napi_env env, napi_callback_info info)
{
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return nullptr;
    void *vp, *fb, *db, *di;
    size_t lvp, lfb, ldb, ldi;
    int32_t n;
    if (!get_typed(env, argv[0], napi_float32_array, &vp, &lvp) || !get_i32(env, argv[1], &n) ||
        !get_typed(env, argv[2], napi_float32_array, &fb, &lfb) || !get_typed(env, argv[3], napi_uint32_array, &db, &ldb, true) ||
        !get_typed(env, argv[4], napi_uint32_array, &di, &ldi))
        return nullptr;
    if (n < 0 || lvp < 16 || lfb < (size_t)n * 3 || ldi < (size_t)n || (db && ldb < (size_t)n)) {
        napi_throw_range_error(env, nullptr, "buffers are smaller than vertexCount requires");
        return nullptr;
    }
    gsplat_sort_host((const float*)vp, (uint32_t)n, (const float*)fb, (uint32_t*)db, (uint32_t*)di, nullptr, nullptr);
    return undefined(env);
}

// ---- depth planes and picking (gsr_depth_async / gsr_read_depth / gsr_pick) ----
napi_value SetHitAlpha(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double a;
    if (!c || !get_f64(env, argv[1], &a)) return nullptr;
    const int rc = gsr_set_hit_alpha(c, (float)a);
    return rc ? throw_gsr(env, c, rc, "gsr_set_hit_alpha") : undefined(env);
}

// readDepth(handle, mean | null, hit | null, index | null, width, height): Float32Array, Float32Array, Uint32Array of width*height
napi_value ReadDepth(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    void* plane[3];
    size_t len[3];
    int32_t w, h;
    if (!get_typed(env, argv[1], napi_float32_array, &plane[0], &len[0], true) || !get_typed(env, argv[2], napi_float32_array, &plane[1], &len[1], true) ||
        !get_typed(env, argv[3], napi_uint32_array, &plane[2], &len[2], true) || !get_i32(env, argv[4], &w) || !get_i32(env, argv[5], &h))
        return nullptr;
    for (int k = 0; k < 3; k++)
        if (plane[k] && len[k] < (size_t)w * h) { napi_throw_range_error(env, nullptr, "plane array is smaller than width*height"); return nullptr; }
    const int rc = gsr_read_depth(c, (float*)plane[0], (float*)plane[1], (uint32_t*)plane[2]);
    return rc ? throw_gsr(env, c, rc, "gsr_read_depth") : undefined(env);
}

// pick(handle, xy: Int32Array of (x, y) pairs, out: Float32Array of 4 per pixel): out holds index (its bits), depth, mean, alpha
napi_value Pick(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void *xy, *out;
    size_t nxy, nout;
    if (!c || !get_typed(env, argv[1], napi_int32_array, &xy, &nxy) || !get_typed(env, argv[2], napi_float32_array, &out, &nout)) return nullptr;
    if (nout < nxy / 2 * 4) { napi_throw_range_error(env, nullptr, "output array is smaller than 4 per pixel"); return nullptr; }
    static_assert(sizeof(gsr_pick_result) == 16, "four words per result");
    const int rc = gsr_pick(c, (const int32_t*)xy, (uint32_t)(nxy / 2), (gsr_pick_result*)out);
    return rc ? throw_gsr(env, c, rc, "gsr_pick") : undefined(env);
}

// ---- selection (gsr_select_region / _box, gsr_selection_set / _invert, gsr_read_selection, gsr_scene_erase_selected) ----
napi_value count_value(napi_env env, uint32_t count)
{
    napi_value n;
    napi_create_uint32(env, count, &n);
    return n;
}

// selectRegion(handle, Int32Array [x0, y0, x1, y1, stride, mode, op], Uint8Array mask | null) -> selected
napi_value SelectRegion(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void *a, *mask;
    size_t na, nm;
    if (!c || !get_typed(env, argv[1], napi_int32_array, &a, &na) || !get_typed(env, argv[2], napi_uint8_array, &mask, &nm, true)) return nullptr;
    if (na < 7) { napi_throw_range_error(env, nullptr, "selectRegion takes [x0, y0, x1, y1, stride, mode, op]"); return nullptr; }
    const int32_t* v = (const int32_t*)a;
    gsr_region reg{v[0], v[1], v[2], v[3], (const uint8_t*)mask, mask ? v[4] : 0, 0};
    // (the library reads (y1 - y0 - 1) * stride + (x1 - x0) bytes of a mask whose rectangle and stride it accepts)
    if (mask && v[2] > v[0] && v[3] > v[1] && v[4] >= v[2] - v[0] && nm < (size_t)(v[3] - v[1] - 1) * (size_t)v[4] + (size_t)(v[2] - v[0])) {
        napi_throw_range_error(env, nullptr, "mask is smaller than the rectangle and stride require");
        return nullptr;
    }
    uint32_t count = 0;
    const int rc = gsr_select_region(c, &reg, v[5], v[6], &count);
    return rc ? throw_gsr(env, c, rc, "gsr_select_region") : count_value(env, count);
}

// selectBox(handle, Float64Array(6), op) -> selected
napi_value SelectBox(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* box;
    size_t len;
    int32_t op;
    if (!c || !get_typed(env, argv[1], napi_float64_array, &box, &len) || !get_i32(env, argv[2], &op)) return nullptr;
    if (len < 6) { napi_throw_range_error(env, nullptr, "a box has 6 entries"); return nullptr; }
    uint32_t count = 0;
    const int rc = gsr_select_box(c, (const double*)box, op, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_select_box") : count_value(env, count);
}

// setSelection(handle, Uint32Array words | null, op) -> selected
napi_value SetSelection(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* words;
    size_t len;
    int32_t op;
    if (!c || !get_typed(env, argv[1], napi_uint32_array, &words, &len, true) || !get_i32(env, argv[2], &op)) return nullptr;
    uint32_t count = 0;
    const int rc = gsr_selection_set(c, (const uint32_t*)words, (uint32_t)len, op, &count);   // (null: the empty set)
    return rc ? throw_gsr(env, c, rc, "gsr_selection_set") : count_value(env, count);
}

// invertSelection(handle) -> selected
napi_value InvertSelection(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    uint32_t count = 0;
    const int rc = gsr_selection_invert(c, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_selection_invert") : count_value(env, count);
}

// readSelection(handle) -> Uint32Array of ceil(n / 32) words
napi_value ReadSelection(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    uint32_t n = 0;
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    const size_t nwords = ((size_t)n + 31) / 32;
    void* data = nullptr;
    napi_value ab, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, nwords * 4, &data, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, nwords, ab, 0, &out));
    rc = gsr_read_selection(c, nwords ? (uint32_t*)data : nullptr, (uint32_t)nwords, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_read_selection") : out;
}

// eraseSelected(handle, keep) -> new count
napi_value EraseSelected(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t keep;
    if (!c || !get_i32(env, argv[1], &keep)) return nullptr;
    uint32_t count = 0;
    const int rc = gsr_scene_erase_selected(c, keep, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_erase_selected") : count_value(env, count);
}

// ---- hidden splats (gsr_hide_selected, gsr_hidden_set, gsr_read_hidden, gsr_select_hidden) ----
// hideSelected(handle, op) -> hidden
napi_value HideSelected(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t op;
    if (!c || !get_i32(env, argv[1], &op)) return nullptr;
    uint32_t count = 0;
    const int rc = gsr_hide_selected(c, op, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_hide_selected") : count_value(env, count);
}

// setHidden(handle, Uint32Array words | null, op) -> hidden
napi_value SetHidden(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* words;
    size_t len;
    int32_t op;
    if (!c || !get_typed(env, argv[1], napi_uint32_array, &words, &len, true) || !get_i32(env, argv[2], &op)) return nullptr;
    uint32_t count = 0;
    const int rc = gsr_hidden_set(c, (const uint32_t*)words, (uint32_t)len, op, &count);   // (null: the empty set)
    return rc ? throw_gsr(env, c, rc, "gsr_hidden_set") : count_value(env, count);
}

// readHidden(handle) -> Uint32Array of ceil(n / 32) words
napi_value ReadHidden(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    uint32_t n = 0;
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    const size_t nwords = ((size_t)n + 31) / 32;
    void* data = nullptr;
    napi_value ab, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, nwords * 4, &data, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, nwords, ab, 0, &out));
    rc = gsr_read_hidden(c, nwords ? (uint32_t*)data : nullptr, (uint32_t)nwords, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_read_hidden") : out;
}

// selectHidden(handle, op) -> selected
napi_value SelectHidden(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t op;
    if (!c || !get_i32(env, argv[1], &op)) return nullptr;
    uint32_t count = 0;
    const int rc = gsr_select_hidden(c, op, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_select_hidden") : count_value(env, count);
}

// ---- editing the selection (gsr_selection_bounds, gsr_scene_*_selected) ----
// selectionBounds(handle, Float32Array(6) out: min xyz, max xyz) -> count
napi_value SelectionBounds(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* out;
    size_t len;
    if (!c || !get_typed(env, argv[1], napi_float32_array, &out, &len)) return nullptr;
    if (len < 6) { napi_throw_range_error(env, nullptr, "the box has 6 entries"); return nullptr; }
    struct gsr_selection_bounds b;
    const int rc = gsr_selection_bounds(c, &b);
    if (rc) return throw_gsr(env, c, rc, "gsr_selection_bounds");
    for (int k = 0; k < 3; k++) { ((float*)out)[k] = b.min[k]; ((float*)out)[3 + k] = b.max[k]; }
    return count_value(env, b.count);
}

// editSelected(handle, kind, Float64Array args, Float64Array pivot | null): kind 0 translate (3), 1 rotate (4: x, y, z, w), 2 scale (3)
napi_value EditSelected(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t kind;
    void *args, *pivot;
    size_t len, plen;
    if (!c || !get_i32(env, argv[1], &kind) || !get_typed(env, argv[2], napi_float64_array, &args, &len) ||
        !get_typed(env, argv[3], napi_float64_array, &pivot, &plen, true))
        return nullptr;
    if (kind < 0 || kind > 2 || len < (kind == 1 ? 4u : 3u) || (pivot && plen < 3)) {
        napi_throw_range_error(env, nullptr, "editSelected: kind 0..2, 3 (rotate: 4) values, a pivot of 3");
        return nullptr;
    }
    const int rc = kind == 0 ? gsr_scene_translate_selected(c, (const double*)args)
                 : kind == 1 ? gsr_scene_rotate_selected(c, (const double*)args, (const double*)pivot)
                             : gsr_scene_scale_selected(c, (const double*)args, (const double*)pivot);
    return rc ? throw_gsr(env, c, rc, kind == 0 ? "gsr_scene_translate_selected" : kind == 1 ? "gsr_scene_rotate_selected" : "gsr_scene_scale_selected")
              : undefined(env);
}

// paintSelected(handle, rgba, byteMask)
napi_value PaintSelected(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    uint32_t rgba, mask;
    if (!c || napi_get_value_uint32(env, argv[1], &rgba) != napi_ok || napi_get_value_uint32(env, argv[2], &mask) != napi_ok) return nullptr;
    const int rc = gsr_scene_set_rgba_selected(c, rgba, mask);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_set_rgba_selected") : undefined(env);
}

// ---- growing the scene (gsr_scene_reserve / _capacity / _duplicate_selected / _append_selected / _append_arrays) ----
napi_value first_count(napi_env env, uint32_t first, uint32_t count)
{
    napi_value o, f, k;
    napi_create_object(env, &o);
    napi_create_uint32(env, first, &f);
    napi_create_uint32(env, count, &k);
    napi_set_named_property(env, o, "first", f);
    napi_set_named_property(env, o, "count", k);
    return o;
}

// reserveScene(handle, rows)
napi_value ReserveScene(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    uint32_t rows;
    if (!c || napi_get_value_uint32(env, argv[1], &rows) != napi_ok) return nullptr;
    const int rc = gsr_scene_reserve(c, rows);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_reserve") : undefined(env);
}

// sceneCapacity(handle) -> rows
napi_value SceneCapacity(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    uint32_t rows = 0;
    const int rc = gsr_scene_capacity(c, &rows);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_capacity") : count_value(env, rows);
}

// duplicateSelected(handle) -> { first, count }
napi_value DuplicateSelected(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    uint32_t first = 0, count = 0;
    const int rc = gsr_scene_duplicate_selected(c, &first, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_duplicate_selected") : first_count(env, first, count);
}

// appendSelected(handle, from handle) -> { first, count }
napi_value AppendSelected(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    gsr_ctx* from = c ? get_ctx(env, argv[1]) : nullptr;
    if (!c || !from) return nullptr;
    uint32_t first = 0, count = 0;
    const int rc = gsr_scene_append_selected(c, from, &first, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_append_selected") : first_count(env, first, count);
}

// appendArrays(handle, Uint32Array data, Float32Array positions, rotations, scales, m) -> { first, count }
napi_value AppendArrays(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    void *data, *pos, *rot, *scl;
    size_t nd, np, nr, ns;
    int32_t m;
    if (!get_typed(env, argv[1], napi_uint32_array, &data, &nd) || !get_typed(env, argv[2], napi_float32_array, &pos, &np) ||
        !get_typed(env, argv[3], napi_float32_array, &rot, &nr) || !get_typed(env, argv[4], napi_float32_array, &scl, &ns) || !get_i32(env, argv[5], &m))
        return nullptr;
    if (m < 0 || nd < (size_t)m * 8 || np < (size_t)m * 3 || nr < (size_t)m * 4 || ns < (size_t)m * 3) {
        napi_throw_range_error(env, nullptr, "scene buffers are smaller than the appended count requires");
        return nullptr;
    }
    uint32_t first = 0;
    const int rc = gsr_scene_append_arrays(c, (const uint32_t*)data, (const float*)pos, (const float*)rot, (const float*)scl, (uint32_t)m, &first);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_append_arrays") : first_count(env, first, (uint32_t)m);
}

// ---- contribution (gsr_contrib_reset / _accumulate_async, gsr_read_contrib, gsr_select_contrib) ----
// readContrib(handle) -> { weight: BigUint64Array(n), peak: Float32Array(n), pixels: Uint32Array(n), frames }
napi_value ReadContrib(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    uint32_t n = 0, frames = 0;
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    void *weight = nullptr, *peak = nullptr, *pixels = nullptr;
    napi_value ab, out, w, p, x, f;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 8, &weight, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_biguint64_array, n, ab, 0, &w));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &peak, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float32_array, n, ab, 0, &p));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &pixels, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, n, ab, 0, &x));
    rc = gsr_read_contrib(c, n ? (uint64_t*)weight : nullptr, n ? (float*)peak : nullptr, n ? (uint32_t*)pixels : nullptr, n, &frames);
    if (rc) return throw_gsr(env, c, rc, "gsr_read_contrib");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_create_uint32(env, frames, &f));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "weight", w));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "peak", p));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "pixels", x));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "frames", f));
    return out;
}

// selectContrib(handle, stat, below, op) -> selected
napi_value SelectContrib(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t stat, op;
    double below;
    if (!c || !get_i32(env, argv[1], &stat) || !get_i32(env, argv[3], &op)) return nullptr;
    if (!get_f64(env, argv[2], &below)) { napi_throw_type_error(env, nullptr, "selectContrib: below must be a number"); return nullptr; }
    uint32_t count = 0;
    const int rc = gsr_select_contrib(c, stat, below, op, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_select_contrib") : count_value(env, count);
}

// ---- splat data (gsr_attr_stats / gsr_attr_histogram / gsr_select_attr) ----
// the optional origin (Float64Array(3) or null) of the calls below; false: a type error is pending
bool get_origin(napi_env env, napi_value v, const double** origin)
{
    void* data = nullptr;
    size_t len = 0;
    if (!get_typed(env, v, napi_float64_array, &data, &len, true)) return false;
    if (data && len < 3) { napi_throw_range_error(env, nullptr, "origin must hold 3 values"); return false; }
    *origin = (const double*)data;
    return true;
}

napi_value set_u32(napi_env env, napi_value o, const char* name, uint32_t v)
{
    napi_value x;
    NAPI_OK_OR_NULL(env, napi_create_uint32(env, v, &x));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, o, name, x));
    return o;
}

napi_value set_f64(napi_env env, napi_value o, const char* name, double v)
{
    napi_value x;
    NAPI_OK_OR_NULL(env, napi_create_double(env, v, &x));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, o, name, x));
    return o;
}

// attrStats(handle, attr, origin | null, scope) -> { count, nan, min, max }
napi_value AttrStats(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t attr;
    uint32_t scope;
    const double* origin = nullptr;
    if (!c || !get_i32(env, argv[1], &attr) || !get_origin(env, argv[2], &origin) || napi_get_value_uint32(env, argv[3], &scope) != napi_ok) return nullptr;
    uint32_t count = 0, nan = 0;
    double mn = 0, mx = 0;
    const int rc = gsr_attr_stats(c, attr, origin, scope, &count, &nan, &mn, &mx);
    if (rc) return throw_gsr(env, c, rc, "gsr_attr_stats");
    napi_value out;
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    if (!set_u32(env, out, "count", count) || !set_u32(env, out, "nan", nan) || !set_f64(env, out, "min", mn) || !set_f64(env, out, "max", mx)) return nullptr;
    return out;
}

// attrHistogram(handle, attr, origin | null, scope, lo, hi, bins) -> { counts: Uint32Array(bins), below, above, nan }
napi_value AttrHistogram(napi_env env, napi_callback_info info)
{
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t attr;
    uint32_t scope, bins;
    double lo, hi;
    const double* origin = nullptr;
    if (!c || !get_i32(env, argv[1], &attr) || !get_origin(env, argv[2], &origin) || napi_get_value_uint32(env, argv[3], &scope) != napi_ok) return nullptr;
    if (!get_f64(env, argv[4], &lo) || !get_f64(env, argv[5], &hi) || napi_get_value_uint32(env, argv[6], &bins) != napi_ok) {
        napi_throw_type_error(env, nullptr, "attrHistogram: lo, hi and bins must be numbers");
        return nullptr;
    }
    if (bins < 1 || bins > 4096) { napi_throw_range_error(env, nullptr, "attrHistogram: bins must be in 1 .. 4096"); return nullptr; }
    void* counts = nullptr;
    napi_value ab, arr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)bins * 4, &counts, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, bins, ab, 0, &arr));
    uint32_t outside[3] = {0, 0, 0};
    const int rc = gsr_attr_histogram(c, attr, origin, scope, lo, hi, bins, (uint32_t*)counts, outside);
    if (rc) return throw_gsr(env, c, rc, "gsr_attr_histogram");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "counts", arr));
    if (!set_u32(env, out, "below", outside[0]) || !set_u32(env, out, "above", outside[1]) || !set_u32(env, out, "nan", outside[2])) return nullptr;
    return out;
}

// selectAttr(handle, attr, origin | null, lo, hi, op) -> selected
napi_value SelectAttr(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t attr, op;
    double lo, hi;
    const double* origin = nullptr;
    if (!c || !get_i32(env, argv[1], &attr) || !get_origin(env, argv[2], &origin) || !get_i32(env, argv[5], &op)) return nullptr;
    if (!get_f64(env, argv[3], &lo) || !get_f64(env, argv[4], &hi)) { napi_throw_type_error(env, nullptr, "selectAttr: lo and hi must be numbers"); return nullptr; }
    uint32_t count = 0;
    const int rc = gsr_select_attr(c, attr, origin, lo, hi, op, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_select_attr") : count_value(env, count);
}

// ---- neighbours (gsr_neighbours / gsr_select_neighbours) ----
// radius, cap, scope and budget of the two calls below (argv[1 .. 4]; the budget a number, 0: the library's default); false: an
// error is pending
bool get_neighbour_args(napi_env env, napi_value* argv, double* radius, uint32_t* cap, uint32_t* scope, uint64_t* budget)
{
    double b;
    if (!get_f64(env, argv[1], radius) || napi_get_value_uint32(env, argv[2], cap) != napi_ok || napi_get_value_uint32(env, argv[3], scope) != napi_ok ||
        !get_f64(env, argv[4], &b)) {
        napi_throw_type_error(env, nullptr, "neighbours: radius, cap, scope and budget must be numbers");
        return false;
    }
    if (*cap < 1 || *cap > GSR_NEIGHBOUR_MAX_CAP) { napi_throw_range_error(env, nullptr, "neighbours: cap must be in 1 .. 4095"); return false; }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "neighbours: budget must be a non-negative number"); return false; }
    *budget = (uint64_t)b;
    return true;
}

// neighbours(handle, radius, cap, scope, budget) -> { counts: Uint32Array(n), hist: Uint32Array(cap + 1), inScope, nonfinite, pairBound, budget }
napi_value Neighbours(napi_env env, napi_callback_info info)
{
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double radius;
    uint32_t cap, scope, n = 0;
    uint64_t budget;
    if (!c || !get_neighbour_args(env, argv, &radius, &cap, &scope, &budget)) return nullptr;
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    void *counts = nullptr, *hist = nullptr;
    napi_value cb, carr, hb, harr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &counts, &cb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, n, cb, 0, &carr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, ((size_t)cap + 1) * 4, &hist, &hb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, (size_t)cap + 1, hb, 0, &harr));
    gsr_neighbour_info ni{};
    rc = gsr_neighbours(c, radius, cap, scope, budget, n ? (uint32_t*)counts : nullptr, n, (uint32_t*)hist, &ni);
    if (rc) return throw_gsr(env, c, rc, "gsr_neighbours");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "counts", carr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "hist", harr));
    if (!set_u32(env, out, "inScope", ni.in_scope) || !set_u32(env, out, "nonfinite", ni.nonfinite) || !set_f64(env, out, "pairBound", (double)ni.pair_bound) ||
        !set_f64(env, out, "budget", (double)ni.budget)) return nullptr;
    return out;
}

// selectNeighbours(handle, radius, cap, scope, budget, lo, hi, op) -> selected
napi_value SelectNeighbours(napi_env env, napi_callback_info info)
{
    napi_value argv[8];
    if (!get_args(env, info, 8, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double radius;
    uint32_t cap, scope, lo, hi;
    uint64_t budget;
    int32_t op;
    if (!c || !get_neighbour_args(env, argv, &radius, &cap, &scope, &budget)) return nullptr;
    if (napi_get_value_uint32(env, argv[5], &lo) != napi_ok || napi_get_value_uint32(env, argv[6], &hi) != napi_ok || !get_i32(env, argv[7], &op)) {
        napi_throw_type_error(env, nullptr, "selectNeighbours: lo, hi and op must be numbers");
        return nullptr;
    }
    uint32_t count = 0;
    const int rc = gsr_select_neighbours(c, radius, cap, scope, budget, lo, hi, op, &count, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_select_neighbours") : count_value(env, count);
}

// ---- planes (gsr_fit_plane / gsr_plane_inliers / gsr_select_plane / gsr_plane_alignment) ----
// threshold at argv[t], scope and budget at argv[sb], argv[sb + 1] (the budget a number, 0: the library's default); false: an error is pending
bool get_plane_args(napi_env env, napi_value* argv, int t, int sb, double* threshold, uint32_t* scope, uint64_t* budget)
{
    double b;
    if (!get_f64(env, argv[t], threshold) || napi_get_value_uint32(env, argv[sb], scope) != napi_ok || !get_f64(env, argv[sb + 1], &b)) {
        napi_throw_type_error(env, nullptr, "planes: threshold, scope and budget must be numbers");
        return false;
    }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "planes: budget must be a non-negative number"); return false; }
    *budget = (uint64_t)b;
    return true;
}

// a Float64Array of at least `need` values
bool get_f64_array(napi_env env, napi_value v, size_t need, const char* what, const double** out)
{
    void* data = nullptr;
    size_t len = 0;
    if (!get_typed(env, v, napi_float64_array, &data, &len)) return false;
    if (!data || len < need) { napi_throw_range_error(env, nullptr, what); return false; }
    *out = (const double*)data;
    return true;
}

bool set_plane_info(napi_env env, napi_value out, const gsr_plane_info& pi)
{
    return set_u32(env, out, "inScope", pi.in_scope) && set_u32(env, out, "nonfinite", pi.nonfinite) && set_u32(env, out, "hypotheses", pi.hypotheses) &&
           set_f64(env, out, "tests", (double)pi.tests) && set_f64(env, out, "budget", (double)pi.budget);
}

// fitPlane(handle, threshold, hypotheses, seed, scope, budget, wantScores) -> { found, plane: Float64Array(4), best, triple: Uint32Array(3), inliers,
//   degenerate, inScope, nonfinite, hypotheses, tests, budget[, scores: Uint32Array(hypotheses)] }
napi_value FitPlane(napi_env env, napi_callback_info info)
{
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double threshold, seed;
    uint32_t hypotheses, scope;
    uint64_t budget;
    bool want = false;
    if (!c || !get_plane_args(env, argv, 1, 4, &threshold, &scope, &budget)) return nullptr;
    if (napi_get_value_uint32(env, argv[2], &hypotheses) != napi_ok || !get_f64(env, argv[3], &seed) || napi_get_value_bool(env, argv[6], &want) != napi_ok) {
        napi_throw_type_error(env, nullptr, "fitPlane: hypotheses and seed must be numbers, scores a boolean");
        return nullptr;
    }
    if (hypotheses < 1 || hypotheses > GSR_PLANE_MAX_HYPOTHESES) { napi_throw_range_error(env, nullptr, "fitPlane: hypotheses must be in 1 .. 4096"); return nullptr; }
    if (!(seed >= 0.0 && seed <= 9007199254740992.0)) { napi_throw_range_error(env, nullptr, "fitPlane: seed must be a non-negative integer"); return nullptr; }
    void *scores = nullptr, *plane = nullptr, *triple = nullptr;
    napi_value sb, sarr = nullptr, pb, parr, tb, tarr, out;
    if (want) {
        NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)hypotheses * 4, &scores, &sb));
        NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, hypotheses, sb, 0, &sarr));
    }
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, 32, &plane, &pb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, 4, pb, 0, &parr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, 12, &triple, &tb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, 3, tb, 0, &tarr));
    gsr_plane_info pi{};
    const int rc = gsr_fit_plane(c, threshold, hypotheses, (uint64_t)seed, scope, budget, (uint32_t*)scores, &pi);
    if (rc) return throw_gsr(env, c, rc, "gsr_fit_plane");
    std::memcpy(plane, pi.plane, 32);
    std::memcpy(triple, pi.triple, 12);
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "plane", parr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "triple", tarr));
    if (want) NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "scores", sarr));
    if (!set_u32(env, out, "found", pi.found) || !set_u32(env, out, "best", pi.best) || !set_u32(env, out, "inliers", pi.inliers) ||
        !set_u32(env, out, "degenerate", pi.degenerate) || !set_plane_info(env, out, pi)) return nullptr;
    return out;
}

// planeInliers(handle, planes: Float64Array(4 * count), count, threshold, scope, budget) -> { inliers: Uint32Array(count), inScope, nonfinite, hypotheses, tests, budget }
napi_value PlaneInliers(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double threshold;
    uint32_t count, scope;
    uint64_t budget;
    const double* planes = nullptr;
    if (!c || !get_plane_args(env, argv, 3, 4, &threshold, &scope, &budget)) return nullptr;
    if (napi_get_value_uint32(env, argv[2], &count) != napi_ok) { napi_throw_type_error(env, nullptr, "planeInliers: count must be a number"); return nullptr; }
    if (count < 1 || count > GSR_PLANE_MAX_HYPOTHESES) { napi_throw_range_error(env, nullptr, "planeInliers: 1 .. 4096 planes"); return nullptr; }
    if (!get_f64_array(env, argv[1], (size_t)count * 4, "planeInliers: planes must hold 4 values per plane", &planes)) return nullptr;
    void* inl = nullptr;
    napi_value ib, iarr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)count * 4, &inl, &ib));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, count, ib, 0, &iarr));
    gsr_plane_info pi{};
    const int rc = gsr_plane_inliers(c, planes, count, threshold, scope, budget, (uint32_t*)inl, &pi);
    if (rc) return throw_gsr(env, c, rc, "gsr_plane_inliers");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "inliers", iarr));
    if (!set_plane_info(env, out, pi)) return nullptr;
    return out;
}

// selectPlane(handle, plane: Float64Array(4), lo, hi, op) -> selected
napi_value SelectPlane(napi_env env, napi_callback_info info)
{
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    const double* plane = nullptr;
    double lo, hi;
    int32_t op;
    if (!c || !get_f64_array(env, argv[1], 4, "selectPlane: plane must hold 4 values", &plane) || !get_i32(env, argv[4], &op)) return nullptr;
    if (!get_f64(env, argv[2], &lo) || !get_f64(env, argv[3], &hi)) { napi_throw_type_error(env, nullptr, "selectPlane: lo and hi must be numbers"); return nullptr; }
    uint32_t count = 0;
    const int rc = gsr_select_plane(c, plane, lo, hi, op, &count);
    return rc ? throw_gsr(env, c, rc, "gsr_select_plane") : count_value(env, count);
}

// planeAlignment(plane: Float64Array(4), axis: Float64Array(3)) -> { q: Float64Array(4) (x, y, z, w), t: Float64Array(3) }   (no handle: a pure function)
napi_value PlaneAlignment(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    const double *plane = nullptr, *axis = nullptr;
    if (!get_f64_array(env, argv[0], 4, "planeAlignment: plane must hold 4 values", &plane) ||
        !get_f64_array(env, argv[1], 3, "planeAlignment: axis must hold 3 values", &axis)) return nullptr;
    void *q = nullptr, *t = nullptr;
    napi_value qb, qarr, tb, tarr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, 32, &q, &qb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, 4, qb, 0, &qarr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, 24, &t, &tb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, 3, tb, 0, &tarr));
    const int rc = gsr_plane_alignment(plane, axis, (double*)q, (double*)t);
    if (rc) return throw_gsr(env, nullptr, rc, "gsr_plane_alignment");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "q", qarr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "t", tarr));
    return out;
}

// ---- rotating SH coefficients (gsr_sh_rotation, gsr_scene_rotate_sh, gsr_scene_rotate_selected_sh, gsr_scene_bake_sh_frame) ----
napi_value f64_array(napi_env env, size_t count, double** data)
{
    void* p = nullptr;
    napi_value buf, arr;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, count * sizeof(double), &p, &buf));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, count, buf, 0, &arr));
    *data = (double*)p;
    return arr;
}

// shRotation(q: Float64Array(4) (x, y, z, w)) -> Float64Array(83): D_1, D_2, D_3 row-major   (no handle: a pure function)
napi_value ShRotation(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    const double* q = nullptr;
    if (!get_f64_array(env, argv[0], 4, "shRotation: q must hold 4 values", &q)) return nullptr;
    double* m = nullptr;
    napi_value out = f64_array(env, 83, &m);
    if (!out) return nullptr;
    const int rc = gsr_sh_rotation(q, m);
    return rc ? throw_gsr(env, nullptr, rc, "gsr_sh_rotation") : out;
}

// rotateSh(handle, q: Float64Array(4), scope: 0 every SH row | 1 the selected splats' rows) -> rows
napi_value RotateSh(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    const double* q = nullptr;
    int32_t scope;
    if (!c || !get_f64_array(env, argv[1], 4, "rotateSh: q must hold 4 values", &q) || !get_i32(env, argv[2], &scope)) return nullptr;
    uint32_t rows = 0;
    const int rc = gsr_scene_rotate_sh(c, q, (uint32_t)scope, &rows);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_rotate_sh") : count_value(env, rows);
}

// rotateSelectedSh(handle, q: Float64Array(4), pivot: Float64Array(3) | null)
napi_value RotateSelectedSh(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    const double* q = nullptr;
    void* pivot;
    size_t plen;
    if (!c || !get_f64_array(env, argv[1], 4, "rotateSelectedSh: q must hold 4 values", &q) ||
        !get_typed(env, argv[2], napi_float64_array, &pivot, &plen, true))
        return nullptr;
    if (pivot && plen < 3) { napi_throw_range_error(env, nullptr, "rotateSelectedSh: a pivot of 3"); return nullptr; }
    const int rc = gsr_scene_rotate_selected_sh(c, q, (const double*)pivot);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_rotate_selected_sh") : undefined(env);
}

// bakeShFrame(handle) -> Float64Array(4): the quaternion (x, y, z, w) the coefficients were rotated by
napi_value BakeShFrame(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    if (!c) return nullptr;
    double* q = nullptr;
    napi_value out = f64_array(env, 4, &q);
    if (!out) return nullptr;
    const int rc = gsr_scene_bake_sh_frame(c, q);
    return rc ? throw_gsr(env, c, rc, "gsr_scene_bake_sh_frame") : out;
}

// ---- matching and registration (gsr_match / gsr_select_match / gsr_register / gsr_rigid_decompose) ----
// what the three calls share, at argv[1 .. 6]: the target's handle, the transform (Float64Array(12), or null for the identity),
// radius, scope, target scope and budget (a number, 0: the library's default); false: an error is pending
struct MatchArgs { gsr_ctx* target; const double* M; double radius; uint32_t scope, target_scope; uint64_t budget; };
bool get_match_args(napi_env env, napi_value* argv, MatchArgs* a)
{
    a->target = get_ctx(env, argv[1]);
    if (!a->target) return false;
    void* data = nullptr;
    size_t len = 0;
    if (!get_typed(env, argv[2], napi_float64_array, &data, &len, true)) return false;
    if (data && len < 12) { napi_throw_range_error(env, nullptr, "match: transform must hold 12 values"); return false; }
    a->M = (const double*)data;
    double b;
    if (!get_f64(env, argv[3], &a->radius) || napi_get_value_uint32(env, argv[4], &a->scope) != napi_ok || napi_get_value_uint32(env, argv[5], &a->target_scope) != napi_ok ||
        !get_f64(env, argv[6], &b)) {
        napi_throw_type_error(env, nullptr, "match: radius, scope, targetScope and budget must be numbers");
        return false;
    }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "match: budget must be a non-negative number"); return false; }
    a->budget = (uint64_t)b;
    return true;
}

// a Float64Array of `count` values over a fresh buffer; *data: its storage
napi_value new_f64_array(napi_env env, size_t count, void** data)
{
    napi_value ab, arr;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, count * 8, data, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, count, ab, 0, &arr));
    return arr;
}

// matchScene(handle, target, transform | null, radius, scope, targetScope, budget, wantSums) -> { idx: Uint32Array(n), d2: Float64Array(n), inScope, nonfinite,
//   targetIndexed, matched, pairBound, budget, d2Min, d2Max[, pairs, sums: Float64Array(16)] }
napi_value MatchScene(napi_env env, napi_callback_info info)
{
    napi_value argv[8];
    if (!get_args(env, info, 8, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    MatchArgs a;
    bool want = false;
    uint32_t n = 0;
    if (!c || !get_match_args(env, argv, &a)) return nullptr;
    if (napi_get_value_bool(env, argv[7], &want) != napi_ok) { napi_throw_type_error(env, nullptr, "matchScene: sums must be a boolean"); return nullptr; }
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    void *idx = nullptr, *d2 = nullptr, *sum = nullptr;
    napi_value ib, iarr, darr, sarr = nullptr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &idx, &ib));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, n, ib, 0, &iarr));
    if (!(darr = new_f64_array(env, n, &d2))) return nullptr;
    if (want && !(sarr = new_f64_array(env, 16, &sum))) return nullptr;
    gsr_match_info mi{};
    gsr_match_sums ms{};
    rc = gsr_match(c, a.target, a.M, a.radius, a.scope, a.target_scope, a.budget, n ? (uint32_t*)idx : nullptr, n ? (double*)d2 : nullptr, n, want ? &ms : nullptr, &mi);
    if (rc) return throw_gsr(env, c, rc, "gsr_match");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "idx", iarr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "d2", darr));
    if (want) {
        std::memcpy(sum, ms.sum, sizeof ms.sum);
        NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "sums", sarr));
        if (!set_f64(env, out, "pairs", (double)ms.pairs)) return nullptr;
    }
    if (!set_u32(env, out, "inScope", mi.in_scope) || !set_u32(env, out, "nonfinite", mi.nonfinite) || !set_u32(env, out, "targetIndexed", mi.target_indexed) ||
        !set_u32(env, out, "matched", mi.matched) || !set_f64(env, out, "pairBound", (double)mi.pair_bound) || !set_f64(env, out, "budget", (double)mi.budget) ||
        !set_f64(env, out, "d2Min", mi.d2_min) || !set_f64(env, out, "d2Max", mi.d2_max)) return nullptr;
    return out;
}

// selectMatch(handle, target, transform | null, radius, scope, targetScope, budget, lo, hi, op) -> selected
napi_value SelectMatch(napi_env env, napi_callback_info info)
{
    napi_value argv[10];
    if (!get_args(env, info, 10, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    MatchArgs a;
    double lo, hi;
    int32_t op;
    if (!c || !get_match_args(env, argv, &a)) return nullptr;
    if (!get_f64(env, argv[7], &lo) || !get_f64(env, argv[8], &hi) || !get_i32(env, argv[9], &op)) {
        napi_throw_type_error(env, nullptr, "selectMatch: lo, hi and op must be numbers");
        return nullptr;
    }
    uint32_t count = 0;
    const int rc = gsr_select_match(c, a.target, a.M, a.radius, a.scope, a.target_scope, a.budget, lo, hi, op, &count, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_select_match") : count_value(env, count);
}

// registerTo(handle, target, transform | null, radius, scope, targetScope, budget, maxIterations, tolerance, history) -> { transform: Float64Array(12),
//   q: Float64Array(4) (x, y, z, w), t: Float64Array(3), status, iterations, pairs, rms, delta[, stepPairs: Float64Array, stepRms: Float64Array] }
napi_value RegisterTo(napi_env env, napi_callback_info info)
{
    napi_value argv[10];
    if (!get_args(env, info, 10, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    MatchArgs a;
    uint32_t steps;
    double tolerance;
    bool history = false;
    if (!c || !get_match_args(env, argv, &a)) return nullptr;
    if (napi_get_value_uint32(env, argv[7], &steps) != napi_ok || !get_f64(env, argv[8], &tolerance) || napi_get_value_bool(env, argv[9], &history) != napi_ok) {
        napi_throw_type_error(env, nullptr, "registerTo: maxIterations and tolerance must be numbers, history a boolean");
        return nullptr;
    }
    if (steps < 1 || steps > GSR_REGISTER_MAX_ITERATIONS_LIMIT) { napi_throw_range_error(env, nullptr, "registerTo: maxIterations must be in 1 .. 256"); return nullptr; }
    void *M = nullptr, *q = nullptr, *t = nullptr;
    napi_value marr, qarr, tarr, out;
    if (!(marr = new_f64_array(env, 12, &M)) || !(qarr = new_f64_array(env, 4, &q)) || !(tarr = new_f64_array(env, 3, &t))) return nullptr;
    uint64_t step_pairs[GSR_REGISTER_MAX_ITERATIONS_LIMIT];
    double step_rms[GSR_REGISTER_MAX_ITERATIONS_LIMIT];
    gsr_register_info ri{};
    if (history) { ri.step_pairs = step_pairs; ri.step_rms = step_rms; ri.step_rows = steps; }
    int rc = gsr_register(c, a.target, a.M, a.radius, a.scope, a.target_scope, a.budget, steps, tolerance, (double*)M, &ri);
    if (rc) return throw_gsr(env, c, rc, "gsr_register");
    rc = gsr_rigid_decompose((const double*)M, (double*)q, (double*)t);
    if (rc) return throw_gsr(env, nullptr, rc, "gsr_rigid_decompose");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "transform", marr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "q", qarr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "t", tarr));
    if (history) {
        void *sp = nullptr, *sr = nullptr;
        napi_value sparr, srarr;
        if (!(sparr = new_f64_array(env, ri.iterations, &sp)) || !(srarr = new_f64_array(env, ri.iterations, &sr))) return nullptr;
        for (uint32_t k = 0; k < ri.iterations; k++) { ((double*)sp)[k] = (double)step_pairs[k]; ((double*)sr)[k] = step_rms[k]; }
        NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "stepPairs", sparr));
        NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "stepRms", srarr));
    }
    if (!set_u32(env, out, "status", (uint32_t)ri.status) || !set_u32(env, out, "iterations", ri.iterations) || !set_f64(env, out, "pairs", (double)ri.pairs) ||
        !set_f64(env, out, "rms", ri.rms) || !set_f64(env, out, "delta", ri.delta)) return nullptr;
    return out;
}

// ---- point-to-plane registration (gsr_match_surface / gsr_register_surface / gsr_surface_solve) ----
// the target's normals at argv[at .. at + 3]: source (GSR_NORMAL_*), radius, k and budget; the scope is the target scope's; false: an
// error is pending
bool get_surface_normals(napi_env env, napi_value* argv, int at, uint32_t target_scope, gsr_normal_options* o)
{
    double radius, b;
    uint32_t k;
    if (!get_i32(env, argv[at], &o->source) || !get_f64(env, argv[at + 1], &radius) || napi_get_value_uint32(env, argv[at + 2], &k) != napi_ok || !get_f64(env, argv[at + 3], &b)) {
        napi_throw_type_error(env, nullptr, "normals: source, radius, k and budget must be numbers");
        return false;
    }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "normals: budget must be a non-negative number"); return false; }
    o->radius = radius; o->k = k; o->budget = (uint64_t)b; o->scope = target_scope;
    return true;
}

// matchSurface(handle, target, transform | null, radius, scope, targetScope, budget, normalSource, normalRadius, normalK, normalBudget) ->
//   { pairs, surfacePairs, sums: Float64Array(29), inScope, nonfinite, targetIndexed, matched, pairBound, budget, d2Min, d2Max }
napi_value MatchSurface(napi_env env, napi_callback_info info)
{
    napi_value argv[11];
    if (!get_args(env, info, 11, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    MatchArgs a;
    gsr_normal_options no{};
    if (!c || !get_match_args(env, argv, &a) || !get_surface_normals(env, argv, 7, a.target_scope, &no)) return nullptr;
    void* sum = nullptr;
    napi_value sarr, out;
    if (!(sarr = new_f64_array(env, 29, &sum))) return nullptr;
    gsr_match_info mi{};
    gsr_surface_sums ss{};
    const int rc = gsr_match_surface(c, a.target, a.M, a.radius, a.scope, a.target_scope, a.budget, &no, &ss, &mi);
    if (rc) return throw_gsr(env, c, rc, "gsr_match_surface");
    std::memcpy(sum, ss.sum, sizeof ss.sum);
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "sums", sarr));
    if (!set_f64(env, out, "pairs", (double)ss.pairs) || !set_f64(env, out, "surfacePairs", (double)ss.surface_pairs) || !set_u32(env, out, "inScope", mi.in_scope) ||
        !set_u32(env, out, "nonfinite", mi.nonfinite) || !set_u32(env, out, "targetIndexed", mi.target_indexed) || !set_u32(env, out, "matched", mi.matched) ||
        !set_f64(env, out, "pairBound", (double)mi.pair_bound) || !set_f64(env, out, "budget", (double)mi.budget) || !set_f64(env, out, "d2Min", mi.d2_min) ||
        !set_f64(env, out, "d2Max", mi.d2_max)) return nullptr;
    return out;
}

// registerSurface(handle, target, transform | null, radius, scope, targetScope, budget, normalSource, normalRadius, normalK, normalBudget, maxIterations,
//   tolerance, history) -> { transform: Float64Array(12), q: Float64Array(4) (x, y, z, w), t: Float64Array(3), status, iterations, pairs, surfacePairs, rms,
//   surfaceRms, delta, valid[, stepPairs, stepSurfacePairs, stepRms, stepSurfaceRms: Float64Array] }
napi_value RegisterSurface(napi_env env, napi_callback_info info)
{
    napi_value argv[14];
    if (!get_args(env, info, 14, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    MatchArgs a;
    gsr_normal_options no{};
    uint32_t steps;
    double tolerance;
    bool history = false;
    if (!c || !get_match_args(env, argv, &a) || !get_surface_normals(env, argv, 7, a.target_scope, &no)) return nullptr;
    if (napi_get_value_uint32(env, argv[11], &steps) != napi_ok || !get_f64(env, argv[12], &tolerance) || napi_get_value_bool(env, argv[13], &history) != napi_ok) {
        napi_throw_type_error(env, nullptr, "registerSurface: maxIterations and tolerance must be numbers, history a boolean");
        return nullptr;
    }
    if (steps < 1 || steps > GSR_REGISTER_MAX_ITERATIONS_LIMIT) { napi_throw_range_error(env, nullptr, "registerSurface: maxIterations must be in 1 .. 256"); return nullptr; }
    void *M = nullptr, *q = nullptr, *t = nullptr;
    napi_value marr, qarr, tarr, out;
    if (!(marr = new_f64_array(env, 12, &M)) || !(qarr = new_f64_array(env, 4, &q)) || !(tarr = new_f64_array(env, 3, &t))) return nullptr;
    uint64_t step_pairs[GSR_REGISTER_MAX_ITERATIONS_LIMIT], step_surface_pairs[GSR_REGISTER_MAX_ITERATIONS_LIMIT];
    double step_rms[GSR_REGISTER_MAX_ITERATIONS_LIMIT], step_surface_rms[GSR_REGISTER_MAX_ITERATIONS_LIMIT];
    gsr_register_surface_info ri{};
    if (history) { ri.step_pairs = step_pairs; ri.step_surface_pairs = step_surface_pairs; ri.step_rms = step_rms; ri.step_surface_rms = step_surface_rms; ri.step_rows = steps; }
    int rc = gsr_register_surface(c, a.target, a.M, a.radius, a.scope, a.target_scope, a.budget, &no, steps, tolerance, (double*)M, &ri);
    if (rc) return throw_gsr(env, c, rc, "gsr_register_surface");
    rc = gsr_rigid_decompose((const double*)M, (double*)q, (double*)t);
    if (rc) return throw_gsr(env, nullptr, rc, "gsr_rigid_decompose");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "transform", marr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "q", qarr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "t", tarr));
    if (history) {
        const char* names[4] = {"stepPairs", "stepSurfacePairs", "stepRms", "stepSurfaceRms"};
        for (int which = 0; which < 4; which++) {
            void* p = nullptr;
            napi_value arr = new_f64_array(env, ri.iterations, &p);
            if (!arr) return nullptr;
            for (uint32_t k = 0; k < ri.iterations; k++)
                ((double*)p)[k] = which == 0 ? (double)step_pairs[k] : which == 1 ? (double)step_surface_pairs[k] : which == 2 ? step_rms[k] : step_surface_rms[k];
            NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, names[which], arr));
        }
    }
    if (!set_u32(env, out, "status", (uint32_t)ri.status) || !set_u32(env, out, "iterations", ri.iterations) || !set_f64(env, out, "pairs", (double)ri.pairs) ||
        !set_f64(env, out, "surfacePairs", (double)ri.surface_pairs) || !set_f64(env, out, "rms", ri.rms) || !set_f64(env, out, "surfaceRms", ri.surface_rms) ||
        !set_f64(env, out, "delta", ri.delta) || !set_u32(env, out, "valid", ri.valid)) return nullptr;
    return out;
}

// surfaceSolve(surfacePairs, sums: Float64Array(29)) -> { transform: Float64Array(12), rms, degenerate }   (no handle: a pure function)
napi_value SurfaceSolve(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    double pairs;
    const double* sum = nullptr;
    if (!get_f64(env, argv[0], &pairs) || !(pairs >= 0.0 && pairs <= 9007199254740992.0)) { napi_throw_type_error(env, nullptr, "surfaceSolve: surfacePairs must be a non-negative number"); return nullptr; }
    if (!get_f64_array(env, argv[1], 29, "surfaceSolve: sums must hold 29 values", &sum)) return nullptr;
    gsr_surface_sums ss{};
    ss.pairs = ss.surface_pairs = (uint64_t)pairs;
    std::memcpy(ss.sum, sum, sizeof ss.sum);
    void* D = nullptr;
    napi_value darr, out;
    if (!(darr = new_f64_array(env, 12, &D))) return nullptr;
    double rms = 0.0;
    int32_t degenerate = 0;
    const int rc = gsr_surface_solve(&ss, (double*)D, &rms, &degenerate);
    if (rc) return throw_gsr(env, nullptr, rc, "gsr_surface_solve");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "transform", darr));
    if (!set_f64(env, out, "rms", degenerate ? std::nan("") : rms) || !set_u32(env, out, "degenerate", (uint32_t)degenerate)) return nullptr;
    return out;
}

// rigidDecompose(transform: Float64Array(12)) -> { q: Float64Array(4) (x, y, z, w), t: Float64Array(3) }   (no handle: a pure function)
napi_value RigidDecompose(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return nullptr;
    const double* M = nullptr;
    if (!get_f64_array(env, argv[0], 12, "rigidDecompose: transform must hold 12 values", &M)) return nullptr;
    void *q = nullptr, *t = nullptr;
    napi_value qarr, tarr, out;
    if (!(qarr = new_f64_array(env, 4, &q)) || !(tarr = new_f64_array(env, 3, &t))) return nullptr;
    const int rc = gsr_rigid_decompose(M, (double*)q, (double*)t);
    if (rc) return throw_gsr(env, nullptr, rc, "gsr_rigid_decompose");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "q", qarr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "t", tarr));
    return out;
}

// ---- clusters (gsr_clusters / gsr_select_clusters / gsr_select_cluster_at) ----
// radius, min_pts, scope and budget of the three calls below (argv[1 .. 4]; the budget a number, 0: the library's default); false:
// an error is pending
bool get_cluster_args(napi_env env, napi_value* argv, double* radius, uint32_t* min_pts, uint32_t* scope, uint64_t* budget)
{
    double b;
    if (!get_f64(env, argv[1], radius) || napi_get_value_uint32(env, argv[2], min_pts) != napi_ok || napi_get_value_uint32(env, argv[3], scope) != napi_ok ||
        !get_f64(env, argv[4], &b)) {
        napi_throw_type_error(env, nullptr, "clusters: radius, minPts, scope and budget must be numbers");
        return false;
    }
    if (*min_pts > GSR_NEIGHBOUR_MAX_CAP) { napi_throw_range_error(env, nullptr, "clusters: minPts must be in 0 .. 4095"); return false; }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "clusters: budget must be a non-negative number"); return false; }
    *budget = (uint64_t)b;
    return true;
}

bool set_cluster_info(napi_env env, napi_value out, const gsr_cluster_info& ci)
{
    return set_u32(env, out, "inScope", ci.in_scope) && set_u32(env, out, "nonfinite", ci.nonfinite) && set_f64(env, out, "pairBound", (double)ci.pair_bound) &&
           set_f64(env, out, "budget", (double)ci.budget) && set_u32(env, out, "core", ci.core) && set_u32(env, out, "border", ci.border) &&
           set_u32(env, out, "noise", ci.noise) && set_u32(env, out, "clusters", ci.clusters) && set_u32(env, out, "largestLabel", ci.largest_label) &&
           set_u32(env, out, "largestSize", ci.largest_size);
}

// clusters(handle, radius, minPts, scope, budget) -> { labels: Uint32Array(n), sizes: Uint32Array(n), inScope, nonfinite, pairBound, budget, core, border, noise,
// clusters, largestLabel, largestSize }
napi_value Clusters(napi_env env, napi_callback_info info)
{
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double radius;
    uint32_t min_pts, scope, n = 0;
    uint64_t budget;
    if (!c || !get_cluster_args(env, argv, &radius, &min_pts, &scope, &budget)) return nullptr;
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    void *labels = nullptr, *sizes = nullptr;
    napi_value lb, larr, sb, sarr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &labels, &lb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, n, lb, 0, &larr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &sizes, &sb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, n, sb, 0, &sarr));
    gsr_cluster_info ci{};
    rc = gsr_clusters(c, radius, min_pts, scope, budget, n ? (uint32_t*)labels : nullptr, n ? (uint32_t*)sizes : nullptr, n, &ci);
    if (rc) return throw_gsr(env, c, rc, "gsr_clusters");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "labels", larr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "sizes", sarr));
    if (!set_cluster_info(env, out, ci)) return nullptr;
    return out;
}

// selectClusters(handle, radius, minPts, scope, budget, lo, hi, op) -> selected
napi_value SelectClusters(napi_env env, napi_callback_info info)
{
    napi_value argv[8];
    if (!get_args(env, info, 8, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double radius;
    uint32_t min_pts, scope, lo, hi;
    uint64_t budget;
    int32_t op;
    if (!c || !get_cluster_args(env, argv, &radius, &min_pts, &scope, &budget)) return nullptr;
    if (napi_get_value_uint32(env, argv[5], &lo) != napi_ok || napi_get_value_uint32(env, argv[6], &hi) != napi_ok || !get_i32(env, argv[7], &op)) {
        napi_throw_type_error(env, nullptr, "selectClusters: lo, hi and op must be numbers");
        return nullptr;
    }
    uint32_t count = 0;
    const int rc = gsr_select_clusters(c, radius, min_pts, scope, budget, lo, hi, op, &count, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_select_clusters") : count_value(env, count);
}

// selectClusterAt(handle, radius, minPts, scope, budget, seed, op) -> selected   (seed 0xffffffff: the largest cluster)
napi_value SelectClusterAt(napi_env env, napi_callback_info info)
{
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double radius;
    uint32_t min_pts, scope, seed;
    uint64_t budget;
    int32_t op;
    if (!c || !get_cluster_args(env, argv, &radius, &min_pts, &scope, &budget)) return nullptr;
    if (napi_get_value_uint32(env, argv[5], &seed) != napi_ok || !get_i32(env, argv[6], &op)) {
        napi_throw_type_error(env, nullptr, "selectClusterAt: seed and op must be numbers");
        return nullptr;
    }
    uint32_t count = 0;
    const int rc = gsr_select_cluster_at(c, radius, min_pts, scope, budget, seed, op, &count, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_select_cluster_at") : count_value(env, count);
}

// ---- k nearest neighbours (gsr_knn / gsr_select_knn) ----
// radius, k, scope, budget and stat of the two calls below (argv[1 .. 5]; the budget a number, 0: the library's default); false: an
// error is pending
bool get_knn_args(napi_env env, napi_value* argv, double* radius, uint32_t* k, uint32_t* scope, uint64_t* budget, int32_t* stat)
{
    double b;
    if (!get_f64(env, argv[1], radius) || napi_get_value_uint32(env, argv[2], k) != napi_ok || napi_get_value_uint32(env, argv[3], scope) != napi_ok ||
        !get_f64(env, argv[4], &b) || napi_get_value_int32(env, argv[5], stat) != napi_ok) {
        napi_throw_type_error(env, nullptr, "knn: radius, k, scope, budget and stat must be numbers");
        return false;
    }
    if (*k < 1 || *k > GSR_KNN_MAX_K) { napi_throw_range_error(env, nullptr, "knn: k must be in 1 .. 32"); return false; }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "knn: budget must be a non-negative number"); return false; }
    *budget = (uint64_t)b;
    return true;
}

// knn(handle, radius, k, scope, budget, stat, lists) -> { found: Uint32Array(n), values: Float64Array(n), hist: Uint32Array(k + 1), and with lists != 0
// idx: Uint32Array(n * k), d2: Float64Array(n * k); inScope, nonfinite, pairBound, budget, complete, finiteValues, valueMin, valueMax }
napi_value Knn(napi_env env, napi_callback_info info)
{
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double radius;
    uint32_t k, scope, n = 0;
    uint64_t budget;
    int32_t stat, lists;
    if (!c || !get_knn_args(env, argv, &radius, &k, &scope, &budget, &stat) || !get_i32(env, argv[6], &lists)) return nullptr;
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    const size_t slots = lists ? (size_t)n * k : 0;
    void *found = nullptr, *values = nullptr, *hist = nullptr, *idx = nullptr, *d2 = nullptr;
    napi_value fb, farr, vb, varr, hb, harr, ib, iarr, db, darr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &found, &fb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, n, fb, 0, &farr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 8, &values, &vb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, n, vb, 0, &varr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, ((size_t)k + 1) * 4, &hist, &hb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, (size_t)k + 1, hb, 0, &harr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, slots * 4, &idx, &ib));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, slots, ib, 0, &iarr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, slots * 8, &d2, &db));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, slots, db, 0, &darr));
    gsr_knn_info ki{};
    rc = gsr_knn(c, radius, k, scope, budget, stat, n ? (uint32_t*)found : nullptr, slots ? (uint32_t*)idx : nullptr, slots ? (double*)d2 : nullptr,
                 n ? (double*)values : nullptr, n, (uint32_t*)hist, &ki);
    if (rc) return throw_gsr(env, c, rc, "gsr_knn");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "found", farr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "values", varr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "hist", harr));
    if (lists) {
        NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "idx", iarr));
        NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "d2", darr));
    }
    if (!set_u32(env, out, "inScope", ki.in_scope) || !set_u32(env, out, "nonfinite", ki.nonfinite) || !set_f64(env, out, "pairBound", (double)ki.pair_bound) ||
        !set_f64(env, out, "budget", (double)ki.budget) || !set_u32(env, out, "complete", ki.complete) || !set_u32(env, out, "finiteValues", ki.finite_values) ||
        !set_f64(env, out, "valueMin", ki.value_min) || !set_f64(env, out, "valueMax", ki.value_max)) return nullptr;
    return out;
}

// selectKnn(handle, radius, k, scope, budget, stat, lo, hi, op) -> selected   (hi +Infinity: no upper end)
napi_value SelectKnn(napi_env env, napi_callback_info info)
{
    napi_value argv[9];
    if (!get_args(env, info, 9, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double radius, lo, hi;
    uint32_t k, scope;
    uint64_t budget;
    int32_t stat, op;
    if (!c || !get_knn_args(env, argv, &radius, &k, &scope, &budget, &stat)) return nullptr;
    if (!get_f64(env, argv[6], &lo) || !get_f64(env, argv[7], &hi) || !get_i32(env, argv[8], &op)) {
        napi_throw_type_error(env, nullptr, "selectKnn: lo, hi and op must be numbers");
        return nullptr;
    }
    uint32_t count = 0;
    const int rc = gsr_select_knn(c, radius, k, scope, budget, stat, lo, hi, op, &count, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_select_knn") : count_value(env, count);
}

// ---- normals (gsr_normals / gsr_select_normal) ----
// the options of the two calls below from argv[1 .. 9]: source, radius, k, scope, budget (a number, 0: the library's default),
// oriented, and the three components of the viewpoint; false: an error is pending
bool get_normal_options(napi_env env, napi_value* argv, gsr_normal_options* o)
{
    double b;
    int32_t oriented;
    if (!get_i32(env, argv[1], &o->source) || !get_f64(env, argv[2], &o->radius) || napi_get_value_uint32(env, argv[3], &o->k) != napi_ok ||
        napi_get_value_uint32(env, argv[4], &o->scope) != napi_ok || !get_f64(env, argv[5], &b) || !get_i32(env, argv[6], &oriented) ||
        !get_f64(env, argv[7], &o->toward[0]) || !get_f64(env, argv[8], &o->toward[1]) || !get_f64(env, argv[9], &o->toward[2])) {
        napi_throw_type_error(env, nullptr, "normals: source, radius, k, scope, budget, oriented and toward must be numbers");
        return false;
    }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "normals: budget must be a non-negative number"); return false; }
    o->budget = (uint64_t)b;
    o->oriented = oriented ? 1u : 0u;
    return true;
}

// normals(handle, source, radius, k, scope, budget, oriented, tx, ty, tz) -> { normals: Float32Array(3 n), variation: Float64Array(n),
// found: Uint32Array(n); inScope, nonfinite, pairBound, budget, valid, variationMin, variationMax }
napi_value Normals(napi_env env, napi_callback_info info)
{
    napi_value argv[10];
    if (!get_args(env, info, 10, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    gsr_normal_options o{};
    if (!c || !get_normal_options(env, argv, &o)) return nullptr;
    uint32_t n = 0;
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    void *normals = nullptr, *variation = nullptr, *found = nullptr;
    napi_value nb, narr, vb, varr, fb, farr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 12, &normals, &nb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float32_array, (size_t)n * 3, nb, 0, &narr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 8, &variation, &vb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float64_array, n, vb, 0, &varr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, (size_t)n * 4, &found, &fb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, n, fb, 0, &farr));
    gsr_normal_info ni{};
    rc = gsr_normals(c, &o, n ? (float*)normals : nullptr, n ? (double*)variation : nullptr, n ? (uint32_t*)found : nullptr, n, &ni);
    if (rc) return throw_gsr(env, c, rc, "gsr_normals");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "normals", narr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "variation", varr));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "found", farr));
    if (!set_u32(env, out, "inScope", ni.in_scope) || !set_u32(env, out, "nonfinite", ni.nonfinite) || !set_f64(env, out, "pairBound", (double)ni.pair_bound) ||
        !set_f64(env, out, "budget", (double)ni.budget) || !set_u32(env, out, "valid", ni.valid) || !set_f64(env, out, "variationMin", ni.variation_min) ||
        !set_f64(env, out, "variationMax", ni.variation_max)) return nullptr;
    return out;
}

// selectNormal(handle, source, radius, k, scope, budget, oriented, tx, ty, tz, stat, hasAxis, ax, ay, az, lo, hi, op) -> selected
napi_value SelectNormal(napi_env env, napi_callback_info info)
{
    napi_value argv[18];
    if (!get_args(env, info, 18, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    gsr_normal_options o{};
    if (!c || !get_normal_options(env, argv, &o)) return nullptr;
    int32_t stat, has_axis, op;
    double axis[3], lo, hi;
    if (!get_i32(env, argv[10], &stat) || !get_i32(env, argv[11], &has_axis) || !get_f64(env, argv[12], &axis[0]) || !get_f64(env, argv[13], &axis[1]) ||
        !get_f64(env, argv[14], &axis[2]) || !get_f64(env, argv[15], &lo) || !get_f64(env, argv[16], &hi) || !get_i32(env, argv[17], &op)) {
        napi_throw_type_error(env, nullptr, "selectNormal: stat, axis, lo, hi and op must be numbers");
        return nullptr;
    }
    uint32_t count = 0;
    const int rc = gsr_select_normal(c, &o, stat, has_axis ? axis : nullptr, lo, hi, op, &count, nullptr);
    return rc ? throw_gsr(env, c, rc, "gsr_select_normal") : count_value(env, count);
}

// ---- merging cells (gsr_cells / gsr_scene_merge_cells) ----
// cell, scope and budget of the two calls below (the budget a number, 0: the library's default); false: an error is pending
bool get_cell_args(napi_env env, napi_value cell_v, napi_value scope_v, napi_value budget_v, double* cell, uint32_t* scope, uint64_t* budget)
{
    double b;
    if (!get_f64(env, cell_v, cell) || napi_get_value_uint32(env, scope_v, scope) != napi_ok || !get_f64(env, budget_v, &b)) {
        napi_throw_type_error(env, nullptr, "cells: cell, scope and budget must be numbers");
        return false;
    }
    if (!(b >= 0.0 && b <= 18446744073709549568.0)) { napi_throw_range_error(env, nullptr, "cells: budget must be a non-negative number"); return false; }
    *budget = (uint64_t)b;
    return true;
}

bool set_cell_info(napi_env env, napi_value out, const gsr_cell_info& ci)
{
    return set_u32(env, out, "inScope", ci.in_scope) && set_u32(env, out, "candidates", ci.candidates) && set_u32(env, out, "cells", ci.cells) &&
           set_u32(env, out, "mergedCells", ci.merged_cells) && set_u32(env, out, "mergedMembers", ci.merged_members) && set_u32(env, out, "largest", ci.largest) &&
           set_u32(env, out, "rowsAfter", ci.rows_after) && set_f64(env, out, "pairBound", (double)ci.pair_bound) && set_f64(env, out, "budget", (double)ci.budget);
}

// cells(handle, cell, cap, scope, budget, leaders) -> { hist: Uint32Array(cap + 1), and with leaders != 0 leader: Uint32Array(n); inScope,
// candidates, cells, mergedCells, mergedMembers, largest, rowsAfter, pairBound, budget }
napi_value Cells(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double cell;
    uint32_t cap, scope, n = 0;
    uint64_t budget;
    int32_t leaders;
    if (!c || !get_cell_args(env, argv[1], argv[3], argv[4], &cell, &scope, &budget)) return nullptr;
    if (napi_get_value_uint32(env, argv[2], &cap) != napi_ok || !get_i32(env, argv[5], &leaders)) {
        napi_throw_type_error(env, nullptr, "cells: cap and leaders must be numbers");
        return nullptr;
    }
    if (cap < 1 || cap > GSR_NEIGHBOUR_MAX_CAP) { napi_throw_range_error(env, nullptr, "cells: cap must be in 1 .. 4095"); return nullptr; }
    int rc = gsr_scene_count(c, &n);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_count");
    const size_t rows = leaders ? n : 0;
    void *leader = nullptr, *hist = nullptr;
    napi_value lb, larr, hb, harr, out;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, rows * 4, &leader, &lb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, rows, lb, 0, &larr));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, ((size_t)cap + 1) * 4, &hist, &hb));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_uint32_array, (size_t)cap + 1, hb, 0, &harr));
    gsr_cell_info ci{};
    rc = gsr_cells(c, cell, cap, scope, budget, rows ? (uint32_t*)leader : nullptr, rows ? n : 0, (uint32_t*)hist, &ci);
    if (rc) return throw_gsr(env, c, rc, "gsr_cells");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "hist", harr));
    if (leaders) NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "leader", larr));
    return set_cell_info(env, out, ci) ? out : nullptr;
}

// mergeCells(handle, cell, scope, budget) -> { count, and gsr_cell_info's fields as cells() names them }
napi_value MergeCells(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    double cell;
    uint32_t scope, count = 0;
    uint64_t budget;
    if (!c || !get_cell_args(env, argv[1], argv[2], argv[3], &cell, &scope, &budget)) return nullptr;
    gsr_cell_info ci{};
    const int rc = gsr_scene_merge_cells(c, cell, scope, budget, &count, &ci);
    if (rc) return throw_gsr(env, c, rc, "gsr_scene_merge_cells");
    napi_value out;
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    return set_u32(env, out, "count", count) && set_cell_info(env, out, ci) ? out : nullptr;
}

// ---- selection overlay (gsr_set_overlay / gsr_overlay_async / gsr_read_overlay* / gsr_delivery_set_overlay) ----
// setOverlay(handle, on, r, g, b, mix): on = 0 switches the overlay off (the other arguments are not read)
napi_value SetOverlay(napi_env env, napi_callback_info info)
{
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t on;
    if (!c || !get_i32(env, argv[1], &on)) return nullptr;
    if (!on) { const int rc = gsr_set_overlay(c, nullptr); return rc ? throw_gsr(env, c, rc, "gsr_set_overlay") : undefined(env); }
    double v[4];
    for (int k = 0; k < 4; k++)
        if (!get_f64(env, argv[2 + k], &v[k])) { napi_throw_type_error(env, nullptr, "setOverlay(handle, on, r, g, b, mix): numbers"); return nullptr; }
    gsr_overlay_options o{};
    o.tint[0] = (float)v[0]; o.tint[1] = (float)v[1]; o.tint[2] = (float)v[2]; o.mix = (float)v[3];
    const int rc = gsr_set_overlay(c, &o);
    return rc ? throw_gsr(env, c, rc, "gsr_set_overlay") : undefined(env);
}

// setOutline(handle, on, r, g, b, alpha, threshold, width, side): on = 0 switches the outline off (the other arguments are not read)
napi_value SetOutline(napi_env env, napi_callback_info info)
{
    napi_value argv[9];
    if (!get_args(env, info, 9, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t on;
    if (!c || !get_i32(env, argv[1], &on)) return nullptr;
    if (!on) { const int rc = gsr_set_overlay_outline(c, nullptr); return rc ? throw_gsr(env, c, rc, "gsr_set_overlay_outline") : undefined(env); }
    double v[5];
    for (int k = 0; k < 5; k++)
        if (!get_f64(env, argv[2 + k], &v[k])) { napi_throw_type_error(env, nullptr, "setOutline(handle, on, r, g, b, alpha, threshold, width, side): numbers"); return nullptr; }
    gsr_outline_options o{};
    o.rgb[0] = (float)v[0]; o.rgb[1] = (float)v[1]; o.rgb[2] = (float)v[2]; o.alpha = (float)v[3]; o.threshold = (float)v[4];
    if (!get_i32(env, argv[7], &o.width) || !get_i32(env, argv[8], &o.side)) return nullptr;
    const int rc = gsr_set_overlay_outline(c, &o);
    return rc ? throw_gsr(env, c, rc, "gsr_set_overlay_outline") : undefined(env);
}

// readOverlay(handle, width, height) -> { rgba: Float32Array(w * h * 4), cover: Float32Array(w * h) }
napi_value ReadOverlay(napi_env env, napi_callback_info info)
{
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t w, h;
    if (!c || !get_i32(env, argv[1], &w) || !get_i32(env, argv[2], &h)) return nullptr;
    const size_t np = (size_t)w * h;
    void *rgba = nullptr, *cover = nullptr;
    napi_value ab, out, a, b;
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, np * 16, &rgba, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float32_array, np * 4, ab, 0, &a));
    NAPI_OK_OR_NULL(env, napi_create_arraybuffer(env, np * 4, &cover, &ab));
    NAPI_OK_OR_NULL(env, napi_create_typedarray(env, napi_float32_array, np, ab, 0, &b));
    const int rc = gsr_read_overlay(c, (float*)rgba, (float*)cover);
    if (rc) return throw_gsr(env, c, rc, "gsr_read_overlay");
    NAPI_OK_OR_NULL(env, napi_create_object(env, &out));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "rgba", a));
    NAPI_OK_OR_NULL(env, napi_set_named_property(env, out, "cover", b));
    return out;
}

// readOverlayPixels(handle, out, width, height): out is a Uint8Array of width * height * 4 (the overlay as RGBA8)
napi_value ReadOverlayPixels(napi_env env, napi_callback_info info)
{
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    void* out;
    size_t len;
    int32_t w, h;
    if (!c || !get_typed(env, argv[1], napi_uint8_array, &out, &len) || !get_i32(env, argv[2], &w) || !get_i32(env, argv[3], &h)) return nullptr;
    if (len < (size_t)w * h * 4) { napi_throw_range_error(env, nullptr, "output array is smaller than width*height*4"); return nullptr; }
    const int rc = gsr_read_overlay_rgba8(c, (uint8_t*)out);
    return rc ? throw_gsr(env, c, rc, "gsr_read_overlay_rgba8") : undefined(env);
}

// deliverySetOverlay(handle, on)
napi_value DeliverySetOverlay(napi_env env, napi_callback_info info)
{
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return nullptr;
    gsr_ctx* c = get_ctx(env, argv[0]);
    int32_t on;
    if (!c || !get_i32(env, argv[1], &on)) return nullptr;
    const int rc = gsr_delivery_set_overlay(c, on);
    return rc ? throw_gsr(env, c, rc, "gsr_delivery_set_overlay") : undefined(env);
}

napi_value Init(napi_env env, napi_value exports)
{
    struct { const char* name; napi_callback fn; } fns[] = {
        {"create", Create}, {"destroy", Destroy}, {"setScene", SetScene}, {"setSceneSh", SetSceneSh}, {"setShFollow", SetShFollow}, {"setShFrame", SetShFrame}, {"getShFrame", GetShFrame}, {"readSceneSh", ReadSceneSh}, {"setDepthFade", SetDepthFade}, {"setSceneRows", SetSceneRows},
        {"sceneTransform", SceneTransform}, {"readScene", ReadScene}, {"setSceneArrays", SetSceneArrays}, {"readSceneArrays", ReadSceneArrays}, {"resize", Resize}, {"setBand", SetBand},
        {"setCamera", SetCamera}, {"sort", Call0<gsr_sort>}, {"render", Call0<gsr_render>},
        {"renderAsync", Call0<gsr_render_async>}, {"sync", Call0<gsr_sync>}, {"resetTimings", Call0<gsr_reset_timings>},
        {"readDepthIndex", ReadDepthIndex}, {"readPixels", ReadPixels}, {"getTimings", GetTimings},
        {"deviceInfo", DeviceInfo}, {"sortHost", SortHost}, {"overflowPending", OverflowPending},
        {"setListCapacity", SetListCapacity}, {"buildId", BuildId}, {"commUniqueId", CommUniqueId}, {"commInit", CommInit}, {"commShare", CommShare},
        {"commDestroy", Call0<gsr_comm_destroy>}, {"allgatherFrameAsync", Call0<gsr_allgather_frame_async>}, {"readFrame", ReadFrame},
        {"openDelivery", OpenDelivery}, {"closeDelivery", Call0<gsr_delivery_close>}, {"deliverySlots", DeliverySlots}, {"detachBuffers", DetachBuffers},
        {"openDeliveryEx", OpenDeliveryEx}, {"deliveryLayout", DeliveryLayout},
        {"openDeliveryDepth", OpenDeliveryDepth}, {"depthLayout", DepthLayout},
        {"commSetDepth", CommSetDepth}, {"frameDepthLayout", FrameDepthLayout}, {"readFrameDepth", ReadFrameDepth},
        {"deliverFrame", DeliverFrame}, {"frameReady", FrameReady}, {"acquireFrame", AcquireFrame}, {"releaseFrame", ReleaseFrame},
        {"setHitAlpha", SetHitAlpha}, {"depthAsync", Call0<gsr_depth_async>}, {"readDepth", ReadDepth}, {"pick", Pick},
        {"shareScene", ShareScene}, {"sceneSharing", SceneSharing},
        {"selectRegion", SelectRegion}, {"selectBox", SelectBox}, {"setSelection", SetSelection}, {"invertSelection", InvertSelection},
        {"readSelection", ReadSelection}, {"eraseSelected", EraseSelected},
        {"hideSelected", HideSelected}, {"setHidden", SetHidden}, {"readHidden", ReadHidden}, {"selectHidden", SelectHidden},
        {"selectionBounds", SelectionBounds}, {"editSelected", EditSelected}, {"paintSelected", PaintSelected},
        {"shRotation", ShRotation}, {"rotateSh", RotateSh}, {"rotateSelectedSh", RotateSelectedSh}, {"bakeShFrame", BakeShFrame},
        {"reserveScene", ReserveScene}, {"sceneCapacity", SceneCapacity}, {"duplicateSelected", DuplicateSelected}, {"appendSelected", AppendSelected},
        {"appendArrays", AppendArrays},
        {"contribReset", Call0<gsr_contrib_reset>}, {"contribAccumulate", Call0<gsr_contrib_accumulate_async>}, {"readContrib", ReadContrib},
        {"selectContrib", SelectContrib},
        {"attrStats", AttrStats}, {"attrHistogram", AttrHistogram}, {"selectAttr", SelectAttr},
        {"neighbours", Neighbours}, {"selectNeighbours", SelectNeighbours},
        {"fitPlane", FitPlane}, {"planeInliers", PlaneInliers}, {"selectPlane", SelectPlane}, {"planeAlignment", PlaneAlignment},
        {"matchScene", MatchScene}, {"selectMatch", SelectMatch}, {"registerTo", RegisterTo}, {"rigidDecompose", RigidDecompose},
        {"matchSurface", MatchSurface}, {"registerSurface", RegisterSurface}, {"surfaceSolve", SurfaceSolve},
        {"clusters", Clusters}, {"selectClusters", SelectClusters}, {"selectClusterAt", SelectClusterAt},
        {"knn", Knn}, {"selectKnn", SelectKnn},
        {"normals", Normals}, {"selectNormal", SelectNormal},
        {"cells", Cells}, {"mergeCells", MergeCells},
        {"setOverlay", SetOverlay}, {"readOverlay", ReadOverlay}, {"readOverlayPixels", ReadOverlayPixels},
        {"deliverySetOverlay", DeliverySetOverlay}, {"setOutline", SetOutline},
    };
    for (auto& f : fns) {
        napi_value fn;
        if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &fn) != napi_ok ||
            napi_set_named_property(env, exports, f.name, fn) != napi_ok)
            return nullptr;
    }
    return exports;
}

}  // namespace

NAPI_MODULE(gsplat_hip, Init)
