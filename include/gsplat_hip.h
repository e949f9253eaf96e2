/*
 * gsplat_hip.h -- C ABI of libgsplat_hip.so, the MI355X-native drop-in for the
 * per-frame hot path of Lanv1/gsplat.js (sort + project + composite).
 *
 * Plain C: opaque context, plain pointers and sizes, int return codes
 * (0 = ok, <0 = error, text via gsr_last_error).  No function throws, aborts
 * or keeps a caller's pointer after it returns (inputs are copied to the
 * device during the call).  A context is bound to one host thread at a time;
 * distinct contexts are independent -- except the contexts that share a scene
 * (gsr_share_scene): those are bound to one host thread at a time together.
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   wasm `sort(...)`                 wasm/wasm.cpp:8-13, called at
 *                                    src/renderers/webgl/utils/Worker.ts:39
 *                                      -> gsplat_sort_host (same 7 arguments) / gsr_sort
 *   worker scene init                Worker.ts:23-34 (positions copied once per scene)
 *   + texImage2D(scene.data)         src/renderers/WebGLRenderer.ts:185-195
 *                                      -> gsr_set_scene
 *   Scene.setData / translate / rotate / scale / limitBox   src/core/Scene.ts:58-366
 *                                      -> gsr_set_scene_rows / gsr_set_scene_arrays, gsr_scene_* (device-side versions)
 *   setShTextures + u_bandIndex      WebGLRenderer.ts:202-211,321-366
 *                                      -> gsr_set_scene_sh
 *   uniforms projection/view/focal/viewport + postMessage({viewProj})
 *                                    WebGLRenderer.ts:144-159,268-269,275
 *                                      -> gsr_set_camera, gsr_resize
 *   drawArraysInstanced + blend state WebGLRenderer.ts:279-290 with
 *   vertex.glsl.ts:130-231, frag.glsl.ts:13-21
 *                                      -> gsr_render
 *   worker.onmessage depthIndex      WebGLRenderer.ts:223-229
 *                                      -> gsr_read_depth_index
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_ERR_ARG (-1)      /* bad argument / call order */
#define GSR_ERR_HIP (-2)      /* a HIP runtime call failed */
#define GSR_ERR_NO_DEVICE (-3)/* no usable AMD GPU */
#define GSR_ERR_SCENE (-4)    /* scene buffers inconsistent */
#define GSR_ERR_OVERFLOW (-5) /* internal list capacity exceeded even after regrowth; or: asynchronous frames were lost (gsr_sync) */
#define GSR_ERR_COMM (-6)     /* RCCL is unavailable or a collective call failed */
#define GSR_ERR_BUSY (-7)     /* every delivery slot is in flight or held by the caller (gsr_deliver_frame_async) */

typedef struct gsr_ctx gsr_ctx;

typedef struct gsr_options {
    int32_t device;         /* HIP device ordinal */
    int32_t width, height;  /* framebuffer size in pixels (canvas.width/height) */
    float early_out_eps;    /* 0: composite every splat like the reference (no early
                               termination); >0: a 16x16 tile stops once every pixel's
                               remaining transmittance 1-alpha is below this value */
    int32_t band_x0, band_x1; /* multi-GPU: this context composites only pixel columns
                               [band_x0, band_x1): band_x0 a multiple of 32 (whole compositor bins), band_x1 a
                               multiple of 32 or the image width; 0,0 = whole image */
    int32_t flags;          /* GSR_FLAG_* */
} gsr_options;

#define GSR_FLAG_TIMING 1   /* record HIP events around every stage (gsr_get_timings) */
#define GSR_FLAG_THROUGHPUT 2 /* the caller keeps several frames in flight on this device (one
                               context per frame): the other contexts' kernels, not extra pieces of
                               this frame, fill the GPU.  The compositor then cuts a frame into ~1300
                               work items instead of ~5000 and gives every 16x16 tile one wave
                               (k_blend, 7 four-wave workgroups per CU); without the flag a context
                               renders one frame at a time and, up to 4096 bins, gives every tile two
                               waves (k_blend2, 3 eight-wave workgroups per CU), which halves the
                               serial walk that bounds a lone frame.  Same pixels within float
                               rounding (pieces are combined associatively). */

/* Per-stage device times of the last completed gsr_render / gsr_sort, measured
 * with HIP events on the context's stream, plus the frame's list sizes. */
typedef struct gsr_timings {
    float ms_project_key; /* projection + depth key + min/max            */
    float ms_sort;        /* quantise + 2 radix passes -> depthIndex      */
    float ms_bin;         /* coarse bin count/scan/scatter                */
    float ms_blend;       /* k_blend: tile composite (and the fold of multi-segment bins), the dominant kernel */
    float ms_combine;     /* k_combine: fold of the per-segment partials; 0 when the fold runs inside k_blend (default) */
    float ms_total;       /* first event -> last event                    */
    uint64_t visible;     /* V: splats with a non-empty screen bbox (within the band) */
    uint64_t bin_entries; /* entries in the coarse (32x32 px) bin lists   */
    uint64_t tile_entries;/* D: sum over visible splats of 16x16 tiles their bbox overlaps */
    uint32_t n;           /* splats                                       */
    uint32_t frames;      /* frames accumulated in the sums below         */
    double sum_ms_project_key, sum_ms_sort, sum_ms_bin, sum_ms_blend, sum_ms_combine, sum_ms_total;
    /* device-side sums over every frame rendered since gsr_reset_timings (valid after gsr_sync) */
    uint64_t sum_visible, sum_bin_entries, sum_tile_entries, sum_frames;
    /* sticky since gsr_create (gsr_reset_timings does not clear them): */
    uint64_t overflow_frames; /* frames whose bin lists did not fit the list capacity (each made the lists regrow) */
    uint64_t dropped_frames;  /* of those, frames that were never composited: asynchronous frames behind which later
                                 frames had been enqueued before the host noticed (gsr_sync reports them once with
                                 GSR_ERR_OVERFLOW); 0 for callers of the blocking gsr_render */
} gsr_timings;

/* ---- lifetime ---- */
int gsr_create(gsr_ctx **out, const gsr_options *opt);
int gsr_destroy(gsr_ctx *ctx);
const char *gsr_last_error(gsr_ctx *ctx); /* ctx may be NULL: error of the failed gsr_create */

/* ---- per scene ---- */
/* data: Scene.data layout, 8 u32 per splat (src/core/Scene.ts:141-148,174-176);
 * positions: Scene.positions, 3 f32 per splat, must equal data words 0..2 (GSR_ERR_SCENE otherwise: the context then
 * keeps the scene, SH state and frame it had).  Repacked once into SoA on the device. */
int gsr_set_scene(gsr_ctx *ctx, const uint32_t *data, const float *positions, uint32_t n);

/* On-device scene build: rows = .splat bytes, 32 per splat (src/core/Scene.ts:9,126-148).  The
 * device does what Scene.setData does (covariance in f64, truncated halves) and keeps rotations/scales, so the
 * transforms below run as kernels instead of JavaScript loops + full re-upload.  Results are bit-identical to the
 * JavaScript ones (Scene.ts:126-366).  q = (x, y, z, w); box = xMin, xMax, yMin, yMax, zMin, zMax. */
int gsr_set_scene_rows(gsr_ctx *ctx, const uint8_t *rows, uint32_t n);
/* The same kind of scene from a Scene's own four arrays, for a Scene that was loaded or transformed on the host before its
 * first frame: data / positions as gsr_set_scene takes and checks them (GSR_ERR_SCENE: the context keeps what it had),
 * rotations = Scene.rotations (w, x, y, z per splat), scales = Scene.scales (3 per splat).  Nothing is recomputed: the
 * covariance words and colours of `data` are taken as they are, so what the context renders is what gsr_set_scene renders
 * from the same data, and gsr_scene_* / gsr_read_scene work as after gsr_set_scene_rows.  Clears SH and frame state. */
int gsr_set_scene_arrays(gsr_ctx *ctx, const uint32_t *data, const float *positions, const float *rotations, const float *scales,
                         uint32_t n);
int gsr_scene_translate(gsr_ctx *ctx, const double *t /* 3 */);
int gsr_scene_rotate(gsr_ctx *ctx, const double *q /* 4 */);
int gsr_scene_scale(gsr_ctx *ctx, const double *s /* 3 */);
int gsr_scene_limit_box(gsr_ctx *ctx, const double *box /* 6 */, uint32_t *new_count);
/* Any of the outputs may be NULL.  data: 8 u32 per splat; rotations (w,x,y,z) / scales only for scenes built from rows or
 * from the four arrays.  The device lays the outputs out (one kernel), then one copy per output. */
int gsr_read_scene(gsr_ctx *ctx, uint32_t *data, float *positions, float *rotations, float *scales, uint32_t *count);
int gsr_scene_count(gsr_ctx *ctx, uint32_t *count); /* splats in the device scene (changes with gsr_scene_limit_box); no copy */

/* Spherical-harmonics colour (the fork's SH textures): sh_r/g/b = Scene.shs_rgb (8 u32 = 16 truncated halves per
 * SH-carrying splat and channel, src/core/Scene.ts:108-124; uploaded by setShTextures, WebGLRenderer.ts:321-366),
 * band_index = Scene.bandsIndices (uniform u_bandIndex, WebGLRenderer.ts:209-211): splat i > band_index[0] takes its
 * colour from eval_sh_rgb (vertex.glsl.ts:57-104,180-204) with degree 1/2/3 by band_index[1], band_index[2].
 * sh_count must be n - (band_index[0] + 1).  Call after gsr_set_scene (which clears any SH state); sh_count 0 clears.
 * gsr_scene_limit_box renumbers the splats and therefore also clears the SH state (unless gsr_set_sh_follow is on, below). */
int gsr_set_scene_sh(gsr_ctx *ctx, const uint32_t *sh_r, const uint32_t *sh_g, const uint32_t *sh_b, uint32_t sh_count,
                     const int32_t *band_index /* 3 */);
/* SH colour that follows the scene through gsr_scene_rotate / _scale / _limit_box (opt-in; the reference's Scene never touches
 * shs_rgb or bandsIndices, Scene.ts:197-366, so after a rotate its highlights stay where they were and after a limitBox its
 * textures belong to other splats).  An SH state carries a frame: linv, 3x3 row-major f64, the inverse of the linear part of
 * every rotate / scale since the coefficients were supplied; gsr_set_scene* and gsr_set_scene_sh reset it to the identity.
 * While follow is on and an SH state exists, gsr_scene_rotate(q) makes it linv . R(q)^T, gsr_scene_scale(s) linv . diag(1/sx, 1/sy, 1/sz) (a component
 * that is 0 or not finite: GSR_ERR_ARG, nothing changed), and gsr_scene_limit_box compacts the SH textures with the scene:
 * the rows of the kept SH splats in order, band_index'[k] = (kept splats with index <= band_index[k]) - 1, and the SH state
 * cleared when no SH splat is kept.  A frame that is not the identity makes the projection evaluate eval_sh_rgb for
 * normalize(linv . (p - camera)) in f32 -- the direction the scene as supplied would have been seen from; the identity costs
 * nothing and yields the bits it always did.  on: default 0; legal at any time; does not alter the frame. */
int gsr_set_sh_follow(gsr_ctx *ctx, int32_t on);
/* Hand a frame to the SH state, for a host that keeps it itself and re-uploads (linv: 9, row-major; NULL = the identity).  Call
 * after gsr_set_scene_sh; GSR_ERR_ARG when there is no SH state or an entry is not finite (nothing changed). */
int gsr_set_sh_frame(gsr_ctx *ctx, const double *linv /* 9 */);
int gsr_get_sh_frame(gsr_ctx *ctx, double *linv /* 9 */, int32_t *follow); /* either may be NULL; no copy, no wait */
/* The SH state as the device holds it (after a followed gsr_scene_limit_box: the compacted one).  The textures take 8 * sh_count
 * words each and may be NULL; sh_count 0 and band_index -1, -1, -1: no SH state. */
int gsr_read_scene_sh(gsr_ctx *ctx, uint32_t *sh_r, uint32_t *sh_g, uint32_t *sh_b, uint32_t *sh_count, int32_t *band_index /* 3 */);

/* ---- shared scenes: contexts of one GPU render from one device copy ----
 * One context per frame in flight (GSR_FLAG_THROUGHPUT) or per viewer would otherwise hold one copy of the scene each.
 * gsr_share_scene makes ctx give up the scene it has and from now on render the scene `from` renders: the same device arrays,
 * nothing copied or uploaded.  A context that never calls it allocates, launches and returns exactly what it always did.
 *   What the members of a scene hold once: the per-splat arrays (positions, covariance words, colours, rotations / scales and
 * whether the scene has them), the SH textures and their spare set with sh_count, band_index, the SH frame and the follow
 * switch, and the splat count.  Membership is symmetric and counted: there is no leader, gsr_destroy of any member in any order
 * leaves the others rendering, the last member to go frees the arrays.
 *   What stays with each context: everything a frame writes -- the sort's, the binning's and the compositor's buffers, the frame
 * words, framebuffer, depth planes, delivery ring, group exchange, the HIP graph, and the SH colours the projection evaluates
 * for this context's camera.  Members may differ in size, band, flags, camera, depth fade, hit alpha, early-out, ring and group.
 *   Leaving: gsr_set_scene / _rows / _arrays on a member take that member out of the share; it then owns the new scene alone and
 * the others keep the old one untouched.  A refused upload (GSR_ERR_SCENE) leaves the member where it was, still sharing.
 *   SH: gsr_set_scene_sh, gsr_set_sh_follow and gsr_set_sh_frame act on the shared scene (they are per-scene state): every
 * member's later frames use them; gsr_get_sh_frame and gsr_read_scene_sh answer alike through any member.  gsr_set_scene_sh
 * waits for every member's stream, as it waits for its own.
 *   Edits: gsr_scene_translate / _rotate / _scale / _limit_box through any member edit the one copy, once, between frames: every
 * frame, depth pass, pick or depth-ring pass any member enqueued before the call sees the scene as it was, everything enqueued
 * afterwards on any member sees the edited scene.  Translate, rotate and scale add no host wait: the editing context's stream
 * waits on one event per other member (recorded on that member's render stream), the kernel runs on the editing context's stream,
 * and every other member's stream then waits on one event recorded behind it (the events are the contexts', none is created per
 * edit).  gsr_scene_limit_box blocks as it always did and replaces the arrays: it also waits for every member's stream, and every
 * member's frame state is then invalid as if it had run the call itself; each re-sizes its per-splat buffers for the new count
 * where its next frame is enqueued.  The rules that hold "since the frame" hold for edits that arrive through another member:
 * gsr_depth_async, gsr_pick and a depth ring's gsr_deliver_frame_async return GSR_ERR_ARG when the scene was edited behind the
 * last frame, exactly as after an edit on the context itself.  The overflow repair of gsr_sync (the last frame rendered again)
 * renders the scene as it stands then, edits included -- as it does after an edit on the context itself.
 *   Reads: gsr_read_scene and gsr_scene_count through any member return the one scene.
 *   GSR_ERR_ARG, nothing changed: ctx == from or either NULL; contexts on different devices; a `from` that has never been given
 * a scene; a ctx that holds a delivered frame (gsr_release_frame first, as for gsr_resize).  Sharing the scene ctx already
 * shares: GSR_OK, nothing changes.  The call waits for ctx's own stream (its frames in flight read the scene it gives up). */
int gsr_share_scene(gsr_ctx *ctx, gsr_ctx *from);
/* members: contexts that render this context's scene (1: not shared); scene_bytes: device bytes of the scene state that members
 * hold once (SoA arrays, rotations / scales, SH textures and their spare set); either may be NULL; no copy, no wait. */
int gsr_scene_sharing(gsr_ctx *ctx, int32_t *members, uint64_t *scene_bytes);

/* ---- per resize / per frame ---- */
int gsr_resize(gsr_ctx *ctx, int32_t width, int32_t height);
/* Multi-GPU: restrict the context to the pixel columns [x0, x1) (same rule as gsr_options.band_x0/x1; 0,0 = whole
 * image).  A band context projects every splat (the depth key's min/max needs them all) but sorts, bins and composites
 * only the splats whose box touches the band. */
int gsr_set_band(gsr_ctx *ctx, int32_t x0, int32_t x1);
/* view, proj, view_proj: column-major f32[16] exactly as `new Float32Array(m.buffer)`
 * of Camera.viewMatrix / projectionMatrix / viewProj (src/cameras/Camera.ts:81-92). */
int gsr_set_camera(gsr_ctx *ctx, const float *view, const float *proj, const float *view_proj, float fx, float fy);

/* FadeInPass uniforms u_useDepthFade / u_depthFade (src/renderers/webgl/passes/FadeInPass.ts:8-37, consumed at
 * vertex.glsl.ts:214-229): while enabled every splat's axes are scaled by the depth-dependent factor. Off by default. */
int gsr_set_depth_fade(gsr_ctx *ctx, int32_t use_depth_fade, float depth_fade);

int gsr_sort(gsr_ctx *ctx);         /* depth key + sort only (blocking)                    */
int gsr_render(gsr_ctx *ctx);       /* sort + project + bin + composite (blocking)         */
int gsr_render_async(gsr_ctx *ctx); /* enqueue one frame on the context's stream           */
int gsr_sync(gsr_ctx *ctx);         /* wait for the stream; reports deferred errors        */
/* List overflow.  The per-bin splat lists live in one device buffer sized from the scene (6 entries per splat + 1 M);
 * a frame that needs more publishes no compositor work (its framebuffer keeps the preceding image), bumps a sticky
 * device counter and stores it in a host-mapped word.  The blocking gsr_render regrows and renders the frame again, so
 * its caller never sees this.  With gsr_render_async the host learns of it later: gsr_render_async polls the word
 * (a host memory read) and regrows before enqueuing the next frame; gsr_sync regrows, renders the LAST frame again if
 * it was among them, and returns GSR_ERR_OVERFLOW once if earlier frames were lost (gsr_timings.dropped_frames counts
 * them; the context stays usable).  gsr_overflow_pending: 1 while the device has reported an overflow that the host
 * has not handled yet -- a caller about to ship the frame it just enqueued (multi-GPU exchange) calls gsr_sync first. */
int gsr_overflow_pending(gsr_ctx *ctx);
/* Tuning/test hook: set the list capacity in entries (>= 1024).  Call after gsr_set_scene* (which sizes it anew). */
int gsr_set_list_capacity(gsr_ctx *ctx, uint32_t entries);

/* ---- results ---- */
/* The whole permutation (wasm's depthIndex).  On a band context the frame sorted only the band's survivors; this
 * call then runs the full sort first. */
int gsr_read_depth_index(gsr_ctx *ctx, uint32_t *out /* n */);
int gsr_read_pixels_rgba32f(gsr_ctx *ctx, float *out /* w*h*4, premultiplied, row 0 = top */);
int gsr_read_pixels_rgba8(gsr_ctx *ctx, uint8_t *out /* w*h*4, round(clamp(x,0,1)*255)   */);
int gsr_get_timings(gsr_ctx *ctx, gsr_timings *out);
int gsr_reset_timings(gsr_ctx *ctx);
/* With GSR_FLAG_TIMING: record the stage events only on every `every`-th frame (default 1).  The six events of a
 * frame are packets the GPU's command processor has to retire; on short frames (small scenes, one band of a
 * multi-GPU frame) timing every frame costs up to 15 % of the frame rate.  gsr_timings averages the sampled frames;
 * the first frame after this call or after gsr_reset_timings is always sampled.  every = 0xffffffff: no frame is
 * sampled (a context created with GSR_FLAG_TIMING then issues frames exactly like one created without). */
int gsr_set_timing_interval(gsr_ctx *ctx, uint32_t every);

/* ---- parity/debug read-backs (intermediate device buffers of the last frame) ---- */
int gsr_read_keys(gsr_ctx *ctx, uint32_t *keys /* n, 17-bit */, int32_t *minmax /* 2 */);
int gsr_read_records(gsr_ctx *ctx, float *rec /* 8n */, int32_t *bbox /* 4n: x0,y0,x1,y1 */);
int gsr_read_sh_colors(gsr_ctx *ctx, float *rgba /* 4n: evaluated SH colour of every splat that has one */);
/* How the last rendered frame's bin lists were handed to the compositor (the choices change no depth order, only f32
 * association): out[0] = list entries per segment, out[1] = work items, out[2] = 0 (reserved), out[3] = waves
 * per 16x16 tile (1: k_blend, 2: k_blend2), out[4] = bins of the context's band. */
int gsr_read_work_items(gsr_ctx *ctx, uint32_t *out /* 5 */);

/* ---- multi-GPU helpers ---- */
/* Entries per 32x32 bin of the last rendered frame, row-major over the context's band (cost model for balanced bands). */
int gsr_read_bin_totals(gsr_ctx *ctx, uint32_t *out /* nbx*nby */, int32_t *nbx, int32_t *nby);
/* The last rendered frame's bin lists (diagnostic; what the compositor walks: the reference has no counterpart, its GPU
 * rasteriser visits every splat for every pixel, WebGLRenderer.ts:282-296): starts[b] .. starts[b + 1] delimit bin b's
 * entries in `list` (splat indices, front to back), bins row-major over the context's band, starts[nbx * nby] = entries of
 * the frame.  `list` may be NULL (starts only); GSR_ERR_ARG when it holds fewer than that many words. */
int gsr_read_bin_lists(gsr_ctx *ctx, uint32_t *starts /* nbx*nby + 1 */, uint32_t *list, uint64_t list_words);
/* Enqueue the f32 -> RGBA8 conversion of the framebuffer on the context's stream (result: gsr_framebuffer8_device_ptr). */
int gsr_convert_rgba8_async(gsr_ctx *ctx);
void *gsr_framebuffer8_device_ptr(gsr_ctx *ctx); /* uint8[h][w][4] on the device */
/* Sender side of the framebuffer all-gather: convert this context's band columns to RGBA8 and
 * write them into `slab` (device memory, `height` rows of `slab_width_px` pixels, >= band width), on the
 * context's stream.  One pass over the band; replaces gsr_convert_rgba8_async + a strided copy. */
int gsr_pack_band_rgba8_async(gsr_ctx *ctx, void *slab, int32_t slab_width_px);
/* Receiver side: de-slab the gathered buffer [world][height][slab_width_px] (RGBA8) into the row-major
 * [height][width] `image`; rank q's columns are [x0[q], x1[q]).  Runs on `stream` (a hipStream_t: the stream
 * the collective was issued on, e.g. torch's current stream), device = the context's.  world <= 16. */
int gsr_unpack_slabs_rgba8_async(gsr_ctx *ctx, const void *gathered, void *image, int32_t slab_width_px, int32_t world,
                                 const int32_t *x0, const int32_t *x1, void *stream);

/* ---- multi-GPU frame exchange inside the library: RCCL all-gather over xGMI ----
 * One process per GPU, one context per process (or per frame in flight).  Rank 0 makes an id and hands its 128 bytes
 * to the other ranks by whatever the host has (a file, a socket, a torch/gloo broadcast); then EVERY rank calls
 * gsr_comm_init with the same id, world and band edges (x0[q], x1[q]) = pixel columns of rank q: contiguous, whole
 * 32-px bin columns, covering [0, width).  gsr_comm_init is collective (returns when all ranks have joined), sets this
 * context's band to its own columns and allocates the exchange buffers.  Per frame:
 *     gsr_render_async(ctx);            band: project all, sort/bin/composite the band's splats
 *     gsr_allgather_frame_async(ctx);   band -> RGBA8 slab (render stream), ONE ncclAllGather of equal slabs + one
 *                                       de-slab kernel on the context's exchange stream; device-side ordering only,
 *                                       so the next frame's kernels overlap the collective
 * and every rank holds the whole RGBA8 frame: gsr_read_frame_rgba8 (waits for the exchange, copies to the host) or
 * gsr_frame8_device_ptr.  The replaced reference entry is still renderer.render(scene, camera)
 * (src/renderers/WebGLRenderer.ts:241-296): the JS HIPRenderer calls exactly this sequence when it has joined a group.
 * world == 1 is allowed (self test; the band is the whole image). */
#define GSR_COMM_ID_BYTES 128
int gsr_comm_unique_id(uint8_t *id /* GSR_COMM_ID_BYTES */);
int gsr_comm_init(gsr_ctx *ctx, const uint8_t *id, int32_t rank, int32_t world, const int32_t *x0, const int32_t *x1);
/* A second (third, ...) context of the SAME rank -- frames in flight -- joins the group `leader` has joined: it uses
 * leader's communicator and exchange stream (so a rank's collectives are issued on ONE stream, in the order of the
 * gsr_allgather_frame_async calls, which must be the same on every rank) and gets its own slab and frame buffers.
 * Several communicators per device with collectives in flight on different streams are the RCCL/NCCL case that can
 * deadlock when the ranks' collectives are scheduled in different orders; this avoids it.  A leader that is destroyed
 * (or leaves with gsr_comm_destroy) first detaches its sharers: they become plain contexts again and fail
 * gsr_allgather_frame_async with GSR_ERR_ARG until they join a group anew.  A custom collective's `user` pointer must
 * outlive every context that uses it. */
int gsr_comm_share(gsr_ctx *ctx, gsr_ctx *leader);
/* Test hook: gsr_comm_init with the caller's collective in place of ncclAllGather, for hosts that cannot form an RCCL
 * communicator of more than one rank (RCCL refuses two ranks on one device) but want to run the exchange's choreography
 * -- band pack, slab padding to the widest band, event ordering against the render stream, de-slab with unequal edges --
 * with world > 1.  gsr_allgather_frame_async calls fn(user, send, recv, bytes_per_rank, stream) on the host in place of
 * ncclAllGather: send = this rank's slab, recv = [world][bytes_per_rank], both device memory; work enqueued on `stream`
 * (a hipStream_t, the exchange stream) before the call has packed the slab, work enqueued on it afterwards reads recv.
 * fn may block.  Returns non-zero on failure.  No product path uses it. */
typedef int (*gsr_allgather_fn)(void *user, const void *send, void *recv, uint64_t bytes_per_rank, void *stream);
int gsr_comm_init_custom(gsr_ctx *ctx, int32_t rank, int32_t world, const int32_t *x0, const int32_t *x1, gsr_allgather_fn fn,
                         void *user);
int gsr_comm_destroy(gsr_ctx *ctx);
int gsr_allgather_frame_async(gsr_ctx *ctx);
/* Waits for the exchange AND for the render stream.  A band packed behind a frame whose bin lists did not fit is the
 * preceding image: every slab carries its frame's overflow flag through the all-gather, so EVERY rank of the group sees
 * which gathered frame holds a stale band and gets GSR_ERR_OVERFLOW for that frame (the rank concerned has regrown its
 * lists by then): all ranks render and gather it again -- the collective is repeated by the whole group, never by one
 * rank alone.  Frames dropped earlier on this rank (reported once by gsr_sync) do not make a good frame unreadable. */
int gsr_read_frame_rgba8(gsr_ctx *ctx, uint8_t *out /* w*h*4: the gathered frame */);
void *gsr_frame8_device_ptr(gsr_ctx *ctx);    /* uint8[h][w][4], the gathered frame on the device */
void *gsr_comm_stream_handle(gsr_ctx *ctx);   /* hipStream_t the exchange runs on */

/* ---- frame delivery: finished RGBA8 frames reach the host through a pinned ring while the next frames render ----
 * The presenting side of renderer.render (src/renderers/WebGLRenderer.ts:279-290 draws into the canvas every frame).
 * gsr_read_pixels_rgba8 converts, copies into pageable memory and waits for the whole stream; the ring instead gives
 * every frame in flight a slot -- one pinned host block of width * height * 4 bytes plus a 16-byte trailer, one device
 * staging buffer of the same size, one "copy done" event -- and the context a second stream for the copies.  Per frame:
 *     gsr_render_async(ctx);
 *     gsr_deliver_frame_async(ctx, &k);   conversion kernel on the render stream (it reads the framebuffer before the next
 *                                         compositor overwrites it), ONE copy of pixels + trailer on the copy stream, the
 *                                         slot's event behind it; no host wait, nothing allocated
 *     ... further frames ...
 *     gsr_acquire_frame(ctx, k, &f);      waits for THAT frame's copy only, never for the render stream
 *     ... f.pixels ...                    byte for byte what gsr_read_pixels_rgba8 would have returned for frame k
 *     gsr_release_frame(ctx, k);          the slot may be reused
 * Serials count 1, 2, 3 ... per context in gsr_deliver_frame_async order and never restart.  serial 0 means the oldest
 * delivered frame that has not been acquired.  A slot is taken by gsr_deliver_frame_async and stays taken until
 * gsr_release_frame (or a failed gsr_acquire_frame); with every slot taken gsr_deliver_frame_async returns GSR_ERR_BUSY
 * and enqueues nothing.
 * Overflow: an asynchronous frame whose bin lists did not fit was not composited (see "List overflow" above); the trailer
 * carries that frame's overflow word, and gsr_acquire_frame on it frees the slot and returns GSR_ERR_OVERFLOW.  The
 * caller renders that pose again (gsr_render_async regrows the lists before it enqueues).
 * In a group (gsr_comm_init* / gsr_comm_share) the delivered frame is the gathered frame of the last
 * gsr_allgather_frame_async: no conversion kernel, the copy runs on the exchange stream behind the de-slab kernel, and a
 * gathered frame with a stale band is refused with GSR_ERR_OVERFLOW where gsr_read_frame_rgba8 refuses it.
 * gsr_resize to another size and gsr_delivery_close fail with GSR_ERR_ARG while a frame is held (acquired, not released);
 * otherwise they wait for the copies and free or reallocate the ring (frames delivered but not acquired are gone, slot
 * pointers change).  gsr_sync also waits for the copies in flight; gsr_destroy waits and frees the ring. */
typedef struct gsr_frame {
    const uint8_t *pixels;  /* pinned host memory, uint8[height][width][4], row 0 = top (a Y'CbCr ring: plane 0, see
                             * gsr_delivery_layout); valid until gsr_release_frame */
    int32_t width, height, slot;
    uint64_t serial;
} gsr_frame;
int gsr_delivery_open(gsr_ctx *ctx, int32_t slots /* 2..8 */);
int gsr_delivery_close(gsr_ctx *ctx);
int gsr_deliver_frame_async(gsr_ctx *ctx, uint64_t *serial /* out; may be NULL */);
int gsr_frame_ready(gsr_ctx *ctx, uint64_t serial);   /* 1: its copy has finished, 0: not yet, < 0: error; never blocks */
int gsr_acquire_frame(gsr_ctx *ctx, uint64_t serial, gsr_frame *out);
int gsr_release_frame(gsr_ctx *ctx, uint64_t serial);
/* The pinned block of slot `slot` (0 .. slots-1) and its size in pixel bytes, for hosts that wrap every slot once
 * (an external ArrayBuffer per slot); NULL without a ring.  The pointers change only when the ring is reallocated. */
void *gsr_delivery_slot_ptr(gsr_ctx *ctx, int32_t slot, uint64_t *bytes);

/* ---- frame delivery in 4:2:0 Y'CbCr (NV12 / I420), for hosts that feed a video encoder ----
 * A ring opened with gsr_delivery_open_ex delivers every frame in the format chosen there; the conversion runs on the device
 * in front of the copy, which shrinks from 4 to 1.5 bytes per pixel, and slots are allocated at the format's size.
 * Everything above holds for every format: serials, GSR_ERR_BUSY, the overflow refusal, gsr_resize (the layout follows the
 * new size), gsr_sync / gsr_destroy, the gathered frame of a group (converted on the exchange stream).
 * The definition, in integers on the bytes gsr_read_pixels_rgba8 / gsr_read_frame_rgba8 return for the
 * frame, premultiplied (r, g, b, a):
 *     R = min(255, r + ((255 - a) * background[0] + 127) / 255), G and B likewise      (default background: black, R = r)
 *     Y = y0 + ((cYr * R + cYg * G + cYb * B + 128) >> 8)                               per pixel
 *     Cb = clamp(128 + ((cBr * Rs + cBg * Gs + cBb * Bs + 512) >> 10), lo, hi), Cr likewise, per 2 x 2 block, Rs / Gs / Bs the
 *     four pixels' sums; coordinates are clamped to the image, so odd sizes replicate the last column / row
 * BT.709, limited range ("tv", full_range = 0): y0 16, Y (47, 157, 16), Cb (-26, -86, 112), Cr (112, -102, -10), chroma 16..240;
 * full range ("pc", yuvj420p): y0 0, Y (54, 183, 19), Cb (-29, -99, 128), Cr (128, -116, -12), chroma 0..255.
 * A slot, Wc = (width + 1) / 2, Hc = (height + 1) / 2, planes tightly packed, row 0 = top:
 *     NV12: Y at 0 (stride width, height rows), interleaved CbCr at width * height (stride 2 * Wc, Hc rows)
 *     I420: Y at 0, Cb at width * height (stride Wc, Hc rows), Cr at width * height + Wc * Hc
 * -- for even sizes byte for byte what `ffmpeg -f rawvideo -pix_fmt nv12 | yuv420p -s WxH` reads.  gsr_frame.pixels points at
 * plane 0; gsr_delivery_layout gives the rest; gsr_delivery_slot_ptr reports the format's payload bytes. */
#define GSR_FORMAT_RGBA8 0
#define GSR_FORMAT_NV12  1
#define GSR_FORMAT_I420  2
typedef struct gsr_delivery_options {
    int32_t slots;          /* 2..8 */
    int32_t format;         /* GSR_FORMAT_* */
    int32_t full_range;     /* NV12 / I420: 0 limited range, otherwise full range */
    uint8_t background[4];  /* NV12 / I420: R, G, B the premultiplied frame is laid over ([3] is ignored) */
} gsr_delivery_options;
typedef struct gsr_frame_layout {
    int32_t format, width, height, planes;
    uint64_t offset[3];     /* of every plane, in bytes from gsr_frame.pixels */
    int32_t stride[3], rows[3];
    uint64_t bytes;         /* the payload: what gsr_delivery_slot_ptr reports */
} gsr_frame_layout;
/* gsr_delivery_open(ctx, n) is format GSR_FORMAT_RGBA8.  GSR_ERR_ARG: a ring is open already (gsr_delivery_close first), an
 * unknown format, slots outside 2..8, no framebuffer size yet. */
int gsr_delivery_open_ex(gsr_ctx *ctx, const gsr_delivery_options *opt);
/* The layout of the open ring's frames at the current size; GSR_ERR_ARG without a ring. */
int gsr_delivery_layout(gsr_ctx *ctx, gsr_frame_layout *out);

/* ---- frame delivery with depth: a depth plane beside every delivered frame, for clients that reproject ----
 * A ring opened with gsr_delivery_open_depth delivers, with the colour of every frame, the "hit" plane of that frame (see
 * "depth and pick" below: z of the first fragment at which accumulated alpha reaches hit_alpha, +infinity without one; the
 * context's hit_alpha at the time of gsr_deliver_frame_async).  gsr_deliver_frame_async then also enqueues, on the render
 * stream behind the frame and the colour conversion, a depth pass for that frame and its conversion into the slot; the slot's
 * ONE copy carries colour payload, depth plane and trailer, and gsr_acquire_frame for serial k gives the colour of frame k and
 * the depth of frame k.  No host wait is added.  The pass has buffers of its own: gsr_read_depth, gsr_depth_device_ptr and
 * gsr_pick answer exactly as they do without a depth ring.
 * The plane, step s = 1 or 2: Wd = ceil(width / s) columns, Hd = ceil(height / s) rows, row 0 = top;
 * sample (i, j) is the hit value of pixel (s * i, s * j) -- a point sample, bit for bit what gsr_read_depth holds at that
 * pixel; no filter, no minimum over the block.
 *   GSR_DEPTH_F32: the float as it is, stride 4 * Wd.
 *   GSR_DEPTH_U16: inverse depth against `near`, little-endian uint16_t, stride 2 * Wd (ffmpeg: -pix_fmt gray16le -s WdxHd), in
 *     binary32: u = 65535 unless z > 0; otherwise q = min(near / z, 1), u = rint(q * 65535) (ties to even).  No hit is 0,
 *     anything at or in front of `near` is 65535, and z ~ near * 65535 / u.
 * A band context delivers +infinity (F32) / 0 (U16) outside its bin columns.
 * A slot: the colour payload exactly as the same ring without depth holds it (gsr_delivery_layout and gsr_delivery_slot_ptr
 * report the colour payload, as they do for every ring), the plane at gsr_depth_layout.offset bytes from gsr_frame.pixels (a
 * multiple of 16), the trailer behind the plane.
 * Everything said of rings above holds: serials, GSR_ERR_BUSY, gsr_frame_ready, gsr_release_frame, gsr_sync, gsr_destroy,
 * gsr_delivery_close; gsr_resize reallocates the ring and the depth layout follows the new size; a frame whose lists did not fit
 * is refused by gsr_acquire_frame with GSR_ERR_OVERFLOW (the depth pass wrote nothing for it) and its slot is freed.
 * gsr_deliver_frame_async on a depth ring needs what gsr_depth_async needs -- a render frame; scene, size, band and list
 * buffers unchanged since -- and otherwise returns GSR_ERR_ARG, enqueues nothing and takes no slot.
 * Groups: depth is not exchanged between ranks unless the context opts in (gsr_comm_set_depth, "depth in a group" below).  Without
 * that, gsr_delivery_open_depth with a depth format on a context in a group returns GSR_ERR_ARG, and so does
 * gsr_deliver_frame_async on a context that joined a group after it opened a depth ring.
 * A context that never opens a depth ring allocates and launches nothing of this. */
#define GSR_DEPTH_NONE 0
#define GSR_DEPTH_F32  1
#define GSR_DEPTH_U16  2
typedef struct gsr_depth_delivery_options {
    int32_t format;         /* GSR_DEPTH_* */
    int32_t step;           /* 1 or 2 */
    float near;             /* GSR_DEPTH_U16: > 0, finite; ignored otherwise */
    int32_t reserved;       /* 0 */
} gsr_depth_delivery_options;
typedef struct gsr_depth_layout {
    int32_t format, step, width, height;   /* width, height: Wd, Hd */
    int32_t stride, reserved;
    uint64_t offset;        /* of the plane, in bytes from gsr_frame.pixels; a multiple of 16 */
    uint64_t bytes;         /* stride * height */
    float near;
    int32_t reserved2;
} gsr_depth_layout;
/* Colour as gsr_delivery_open_ex(ctx, opt) would deliver it, plus the depth plane.  depth == NULL or format GSR_DEPTH_NONE:
 * exactly gsr_delivery_open_ex.  GSR_ERR_ARG: what gsr_delivery_open_ex refuses; an unknown depth format, a step other than 1
 * or 2, GSR_DEPTH_U16 with a near that is not finite and > 0, reserved != 0, a context in a group that exchanges no depth or
 * exchanges it with other options. */
int gsr_delivery_open_depth(gsr_ctx *ctx, const gsr_delivery_options *opt, const gsr_depth_delivery_options *depth);
/* The depth plane of the open ring's frames at the current size; GSR_ERR_ARG: no ring, or a ring without depth. */
int gsr_delivery_depth_layout(gsr_ctx *ctx, gsr_depth_layout *out);

/* ---- depth in a group: ranks exchange depth slabs beside the colour slabs ----
 * Opt-in per context.  A context that has joined a group and calls gsr_comm_set_depth with a depth format exchanges, with every
 * gsr_allgather_frame_async, the frame's hit plane beside its colour.  The call then also enqueues, on the render stream behind
 * the frame and the colour pack, the hit-plane pass over this rank's bin columns (the pass and the hit_alpha rule of a depth
 * ring, into a plane the exchange owns: gsr_read_depth, gsr_depth_device_ptr and gsr_pick answer as before) and a pack of the
 * band's samples into a depth section of the slab; ONE collective carries colour pixels, flag words and depth section, and one
 * more de-slab step on the exchange stream leaves the gathered plane on every rank.  No host wait is added.  With the option on,
 * gsr_allgather_frame_async needs what gsr_depth_async needs of the frame and otherwise returns GSR_ERR_ARG and enqueues nothing.
 * The gathered plane [Hd][Wd], Wd = ceil(width / step), Hd = ceil(height / step), sample (i, j) = pixel (step * i, step * j), is
 * bit for bit the plane a depth ring with the same options delivers for the same frame on one context rendering the whole image.
 * Band edges are multiples of 32, so rank q owns the plane's columns [x0[q] / step, ceil(x1[q] / step)): disjoint, covering Wd.
 * A slab: pixels and flag words where they are without the option; the depth section at the next multiple of 16 bytes: Hd rows
 * of S samples (f32 or u16), S = ceil(widest band / step) rounded up to a multiple of 8, the band's samples at the front of a row
 * and zeros behind them.  bytes_per_rank of a custom collective grows by the padding and Hd * S * sample size.
 * Overflow: a band packed behind a frame whose lists did not fit carries no valid depth; the slab's flag makes every rank refuse
 * that gathered frame -- gsr_read_frame_depth like gsr_read_frame_rgba8, gsr_acquire_frame likewise: GSR_ERR_OVERFLOW on every
 * rank alike -- and the group renders and gathers it again.
 * Delivery: on such a context gsr_delivery_open_depth accepts depth options equal to the exchange's in format, step and near
 * (GSR_ERR_ARG names the first that differs), and gsr_deliver_frame_async delivers the gathered colour (RGBA8, NV12 or I420) and
 * the gathered plane of the last gsr_allgather_frame_async, on the exchange stream, without a depth pass of its own: serial k
 * carries colour and depth of gathered frame k.  Slot layout, trailer, gsr_delivery_layout and gsr_delivery_depth_layout are a
 * depth ring's; one device-to-host copy per frame.  A ring opened before the context joined works once the options match at
 * the time of gsr_deliver_frame_async.
 * The option is part of the group's contract like the band edges: every rank, and every sharer (gsr_comm_share), passes the same
 * options before its next gsr_allgather_frame_async.  It goes with the group: gsr_comm_destroy, gsr_destroy, joining anew and a
 * gsr_resize that drops the group clear it.  A context that never opts in allocates and launches nothing of this, and its slab
 * is the colour slab byte for byte.  Not exchanged: the mean and index planes; gsr_pick answers for this rank's band only. */
/* Opt a context that has joined a group into exchanging depth.  `depth` has the meaning it has for
 * gsr_delivery_open_depth (format F32 | U16, step 1 | 2, near, reserved 0); NULL or GSR_DEPTH_NONE
 * switches it off again.  Part of the group's contract like the band edges: every rank, and every
 * sharer (gsr_comm_share), passes the same options before its next gsr_allgather_frame_async.
 * GSR_ERR_ARG: a context that is in no group; options gsr_delivery_open_depth refuses.  Waits for the render and exchange
 * streams, reallocates the exchange buffers and drops the gathered frame (gather again before reading or delivering). */
int gsr_comm_set_depth(gsr_ctx *ctx, const gsr_depth_delivery_options *depth);
int gsr_frame_depth_layout(gsr_ctx *ctx, gsr_depth_layout *out);          /* offset 0: the gathered plane */
int gsr_read_frame_depth(gsr_ctx *ctx, void *out, uint64_t out_bytes);    /* blocking; beside gsr_read_frame_rgba8 */
void *gsr_frame_depth_device_ptr(gsr_ctx *ctx);                           /* [Hd][Wd] f32 or u16 on the device */

/* ---- depth and pick: per-pixel depth planes of the last rendered frame, and the splat under a pixel ----
 * No interface of the reference stands behind this section (its renderer returns colour only, WebGLRenderer.ts:241-296): it
 * is what a viewer builds "double-click sets the orbit target" and "click selects" from, and what a compositor or a
 * reprojecting client needs beside the colour.  A separate pass behind the frame on the context's stream, over the bin lists,
 * records and positions the frame left on the device; the frame, its framebuffer and its statistics are not touched, and a
 * context that never calls these functions allocates and launches nothing.
 * Definitions.  A pixel's fragments are the entries of its bin's list, in list order (front to back),
 * that pass the compositor's coverage test, each with the weight B the compositor gives it; z of a splat is the w of its
 * centre's clip position for the frame's camera (view-space depth for a perspective camera).  From T = 1, D = 0:
 *     w = T * B;  D = fma(w, z, D);  T = T - w;  the first fragment with 1 - T >= hit_alpha is the pixel's hit.
 *   plane 0 "mean",  float:    D = sum of T_k B_k z_k, premultiplied like the colour channels (divide by the framebuffer's alpha)
 *   plane 1 "hit",   float:    z of the hit; +infinity when accumulated alpha never reaches hit_alpha
 *   plane 2 "index", uint32_t: the hit's splat index (the index depthIndex and the scene use); 0xffffffff when none
 * Each plane is width * height, row 0 = top.  Early termination (early_out_eps) does not apply: the pass walks every entry.
 * A band context defines the planes on its bin columns only; the other columns hold 0 / +infinity / 0xffffffff.
 * gsr_depth_async enqueues the pass behind the last enqueued frame (legal after gsr_render / gsr_render_async; no host wait).
 * gsr_read_depth and gsr_pick first do what gsr_sync does for the frame (a frame whose lists did not fit is rendered again),
 * run the pass if the planes are not the current frame's, then copy; planes enqueued behind a frame that did not fit are
 * never returned as data.  gsr_pick answers `count` (1..4096) pixels (x, y pairs) without the planes: index, depth (the
 * hit's z), mean and alpha = 1 - T, bit for bit what the planes and the recurrence hold for those pixels.
 * GSR_ERR_ARG: no frame rendered yet, the scene, size, band or list buffers changed since the frame, the last frame was
 * sort-only, a pixel outside the image or the context's band, count 0 or above 4096, hit_alpha outside (0, 1]. */
typedef struct gsr_pick_result { uint32_t index; float depth; float mean; float alpha; } gsr_pick_result;
int gsr_set_hit_alpha(gsr_ctx *ctx, float a);                 /* (0, 1], default 0.5 */
int gsr_depth_async(gsr_ctx *ctx);
int gsr_read_depth(gsr_ctx *ctx, float *mean, float *hit, uint32_t *index);   /* each may be NULL; blocking */
void *gsr_depth_device_ptr(gsr_ctx *ctx, int32_t plane);      /* 0 mean, 1 hit, 2 index; NULL until the planes exist */
int gsr_pick(gsr_ctx *ctx, const int32_t *xy /* count x (x, y) */, uint32_t count, gsr_pick_result *out);   /* blocking */

/* ---- selection ---- screen regions and boxes select, erase compacts
 * No interface of the reference stands behind this section either: it lies between gsr_pick (the splat under one pixel) and
 * gsr_scene_limit_box (a world-axis crop), and is what a viewer that becomes a clean-up tool needs first: delete the floaters in
 * front of the subject, keep only the object inside the lasso.
 * A selection is one bit per splat of a scene, held on the device with the scene: nwords = ceil(n / 32) words of uint32_t, splat
 * i is bit i & 31 of word i >> 5, bits at and above n are always 0, and a scene that has never been selected in reads as all
 * zeros.  The members of a shared scene (gsr_share_scene) have ONE selection, because its bits are splat indices of the one copy.
 * Definitions ("Selection"); P is the set a call picks, S the selection:
 *   GSR_SELECT_CENTRE ("select through"): splat i is picked iff it is listed in the last rendered frame -- it passed the frame's
 *     culls, i.e. it has a non-empty pixel box (on a band context: the box touches the band) -- and its centre pixel
 *     X = (int)floorf(cx), Y = (int)floorf(cy) of the frame's record lies in the region (pixel centres are at +0.5).  A centre
 *     outside the image never selects.
 *   GSR_SELECT_HIT ("select the surface"): splat i is picked iff it is the value of the context's hit-index plane (plane 2 of
 *     "depth and pick", at the context's hit_alpha of that moment, for the last rendered frame) at one or more pixels of the region.
 *   Region: a pixel rectangle [x0, x1) x [y0, y1), 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height; optionally one byte per pixel of
 *     the rectangle, non-zero meaning inside, row stride mask_stride >= x1 - x0, row 0 = y0 (the top): the host rasterises a lasso
 *     or a brush into it.  On a band context the rectangle must lie inside the band's pixel columns, the rule gsr_pick has for a pixel.
 *   gsr_select_box picks the splats inside the box: the same f64 comparisons on the same f32 positions as gsr_scene_limit_box,
 *     with its min >= max refusals.  It needs no frame.
 *   Ops: REPLACE S = P; ADD S = S | P; SUBTRACT S = S & ~P; INTERSECT S = S & P.
 * Common to the calls: `selected` receives the number of set bits afterwards and may be NULL.  Every call is blocking and returns
 * with the selection final on the device; because each call ends with a stream wait, the members of a shared scene may issue these
 * calls in any order with no events between them (the "one host thread at a time, together" rule above covers the rest).
 * gsr_select_region needs of the frame what gsr_pick needs, and first settles the frame as gsr_pick does (a frame whose lists
 * did not fit is rendered again); HIT mode runs the planes pass if the planes are not this frame's, as gsr_read_depth does, and
 * refuses planes a pass marked invalid with GSR_ERR_OVERFLOW.  It does not touch the frame, the framebuffer, the statistics or
 * the planes' validity.  GSR_ERR_ARG, nothing changed: a bad rectangle or stride, an unknown mode or op, reserved != 0, a region
 * outside the band, every frame condition gsr_pick refuses (no frame yet; scene, size, band or list buffers changed since the
 * frame -- a gsr_scene_translate counts; a sort-only last frame).
 * gsr_selection_set / gsr_read_selection need nwords >= ceil(n / 32), else GSR_ERR_ARG; host bits at or above n are dropped;
 * gsr_selection_invert keeps the tail at 0.
 * gsr_scene_erase_selected removes the selected splats, or with keep_selected != 0 the unselected ones.  Everything said of
 * gsr_scene_limit_box holds: order-preserving; needs rotations / scales (a scene from rows or from the four arrays); waits for
 * every member of a shared scene and invalidates their frame state; moves the generation; re-plans the bins; with
 * gsr_set_sh_follow on, compacts the SH textures and recounts band_index, otherwise drops the SH state.  Exception: when nothing
 * would be removed it returns GSR_OK with new_count = n and changes nothing -- the last frame stays valid and gsr_pick still
 * answers.  After a removal the selection is empty.
 * Where the selection is cleared or replaced: gsr_scene_limit_box and gsr_set_scene* also leave the scene with the empty
 * selection (a selection does not survive a limitBox); translate, rotate and scale keep it; after gsr_share_scene, ctx has
 * `from`'s selection; a member that leaves a share starts empty.  gsr_scene_sharing's scene_bytes counts the selection's buffers
 * once they exist.  A context that never calls any of this allocates nothing and launches nothing. */
#define GSR_SELECT_CENTRE 0
#define GSR_SELECT_HIT    1
#define GSR_SELOP_REPLACE 0
#define GSR_SELOP_ADD 1
#define GSR_SELOP_SUBTRACT 2
#define GSR_SELOP_INTERSECT 3
typedef struct gsr_region { int32_t x0, y0, x1, y1; const uint8_t *mask; int32_t mask_stride; int32_t reserved; } gsr_region;
int gsr_select_region(gsr_ctx *ctx, const gsr_region *region, int32_t mode, int32_t op, uint32_t *selected);
int gsr_select_box(gsr_ctx *ctx, const double *box /* 6 */, int32_t op, uint32_t *selected);
int gsr_selection_set(gsr_ctx *ctx, const uint32_t *words, uint32_t nwords, int32_t op, uint32_t *selected); /* words NULL: the empty set */
int gsr_selection_invert(gsr_ctx *ctx, uint32_t *selected);
int gsr_read_selection(gsr_ctx *ctx, uint32_t *words, uint32_t nwords, uint32_t *selected);   /* words may be NULL: count only */
int gsr_scene_erase_selected(gsr_ctx *ctx, int32_t keep_selected, uint32_t *new_count);

/* ---- hidden splats ---- hide the selection without erasing it, show it again
 * No interface of the reference stands behind this section either: its Scene has limitBox and nothing softer
 * (src/core/Scene.ts:307-366).  Between "tinted" (the overlay) and "gone for good" (gsr_scene_erase_selected) lies the step every
 * splat editor has: hide.  It is non-destructive -- undo is "show" -- and isolating an object is gsr_selection_invert + hide.
 * The hidden set H is one bit per splat of a scene, held on the device with the scene, in the selection's layout: ceil(n / 32)
 * words, splat i is bit i & 31 of word i >> 5, bits at and above n are always 0, and a scene that never hid anything reads as all
 * zeros -- such a scene has allocated nothing and gsr_scene_sharing's scene_bytes is unchanged.  The members of a shared scene
 * have ONE hidden set.
 * The frame ("Hidden splats"): a hidden splat fails the frame's culls, as if its pixel box were empty.  It
 *   gets no record and no bin rectangle, is in no bin list, does not count in gsr_timings.visible / bin_entries / tile_entries
 *   nor in the optical-mass words the work-item cut reads, on a band context it is not a survivor, and gsr_read_records reports it
 *   as it reports a culled splat (x0 > x1).  It is still sorted: its depth key, the frame's min / max and gsr_read_depth_index are
 *   bit for bit what they are with nothing hidden, and gsr_sort does not look at H.  Everything downstream follows from the
 *   lists: the compositor, the depth planes and gsr_pick see through it, gsr_select_region does not pick it in either mode, the
 *   contribution pass gives it no weight, the overlay does not draw it; none of them got a new argument.  With H empty the frame
 *   path is exactly the one of a scene that never hid -- the projection is handed a null pointer, not an all-zero mask -- also
 *   after "show all" while the buffers stay allocated.
 * Calls; S is the selection, P a set of the host's:
 *   gsr_hide_selected: H = H op S -- REPLACE H = S; ADD H = H | S (hide); SUBTRACT H = H & ~S (show); INTERSECT H = H & S.
 *   gsr_hidden_set: H = H op P; words NULL is the empty set, so (NULL, 0, GSR_SELOP_REPLACE) is "show all".
 *   gsr_read_hidden: the words and the count; words may be NULL: count only.
 *   gsr_select_hidden: S = S op H, an ordinary picker: it does not touch H or any frame.
 *   op is GSR_SELOP_*; `hidden` / `selected` receive the bit count afterwards and may be NULL; gsr_hidden_set / gsr_read_hidden
 *   need nwords >= ceil(n / 32), else GSR_ERR_ARG, and host bits at or above n are dropped.  A refused call (GSR_ERR_ARG: nwords,
 *   an unknown op, a NULL ctx) changes nothing.
 * A change of H is a scene edit, ordered like gsr_scene_translate, but it needs no rotations / scales: a scene from gsr_set_scene
 *   can hide.  It marks every member's frame state as edited: gsr_depth_async, gsr_pick, gsr_select_region and a depth ring's
 *   gsr_deliver_frame_async return GSR_ERR_ARG until the next frame, exactly as after a translate.  Frames any member enqueued
 *   before the call see the old H, frames enqueued afterwards, on any member, see the new one; there is no host wait on other
 *   members' streams, the call waits for its own stream to return the count.  A call that would change no bit still counts as
 *   an edit.  A captured graph is re-captured when H goes from empty to non-empty or back.
 * Compaction: gsr_scene_limit_box and a removing gsr_scene_erase_selected carry H through: H'[new index of i] = H[i] for every
 *   kept i, in order; the tail is 0 and the count is recomputed (the selection and the contribution state are still dropped
 *   there).  Erasing the hidden splats for good is gsr_select_hidden(REPLACE) + gsr_scene_erase_selected(0); afterwards H is empty.
 * Where H is replaced: gsr_set_scene* leaves nothing hidden; after gsr_share_scene, ctx has `from`'s H; a member that leaves a
 *   share starts with nothing hidden.
 * Interplay: gsr_select_box and gsr_select_contrib range over all splats, hidden ones included; a splat hidden during a tour
 *   accumulates nothing, so `below` picks it -- a host that does not want that folds gsr_select_hidden(SUBTRACT) behind it. */
int gsr_hide_selected(gsr_ctx *ctx, int32_t op, uint32_t *hidden);
int gsr_hidden_set(gsr_ctx *ctx, const uint32_t *words, uint32_t nwords, int32_t op, uint32_t *hidden);   /* words NULL: the empty set */
int gsr_read_hidden(gsr_ctx *ctx, uint32_t *words, uint32_t nwords, uint32_t *hidden);   /* words may be NULL: count only */
int gsr_select_hidden(gsr_ctx *ctx, int32_t op, uint32_t *selected);

/* ---- editing the selection ---- move, rotate, scale and recolour the selected splats and nothing else
 * The reference's Scene.translate / rotate / scale (src/core/Scene.ts:182-305) move the whole scene, and so do gsr_scene_translate /
 * _rotate / _scale.  These calls change the selected splats only -- straighten a tilted object, move a floater cluster back, shrink
 * a blown-up region, make a selection transparent or paint it -- on the device, with no gsr_read_scene / gsr_set_scene_arrays round
 * trip (which re-allocates, drops the selection, the hidden set and the accumulators, and takes the context out of a shared scene).
 * S is the selection (one bit per splat, the section above "hidden splats").
 * Transforms ("Editing the selection"): for every splat i whose selection bit is set, the calls leave the
 *   scene's positions, rotations, scales, covariance words and rgba of i holding exactly what the reference's loops would leave in
 *   a Scene that held only the selected splats: f64 arithmetic in the reference's order, rounded to f32 wherever the reference
 *   stores into a Float32Array, the covariance re-packed as Scene.setData packs it.  Every other splat is not written at all.  With
 *   the whole scene selected and no pivot the result equals gsr_scene_translate / _rotate / _scale bit for bit.  q is (x, y, z, w).
 * Pivot: a pivot is defined as the three-step sequence on that sub-scene, translate(-pivot), the operation, translate(+pivot), each
 *   step rounding to f32 as the reference's stores do (the kernel fuses the three steps: one read and one write per selected
 *   splat).  pivot == NULL means the operation alone, with no translate steps; this is not the same as a pivot of zero, which
 *   turns -0.0 into +0.0.
 * Recolour: gsr_scene_set_rgba_selected does rgba[i] = (rgba[i] & ~byte_mask) | (rgba & byte_mask) for selected i; the word is
 *   data[8i+7]: r, g, b in the low three bytes, opacity in the top byte (0xff000000: opacity only; 0x00ffffff: colour only).  For
 *   splats that take their colour from SH (index > bandsIndices[0]) the projection reads only the opacity byte.
 * Bounds: gsr_selection_bounds returns the number of selected splats and the axis-aligned box of their centres as f32.  A value
 *   enters min only through x < min and max only through x > max, so a NaN coordinate is counted but never enters the box; with
 *   nothing selected count is 0, min is +inf and max is -inf; hidden splats that are selected count like any other.  The result is
 *   order-free, so it is exact (compare values, not bits: which of -0.0 and +0.0 a bound holds is not defined).  It is reduced on
 *   the device and 28 bytes are copied back: no host loop over n.  Blocking; it is no edit and touches no frame state.
 * Ordering: an edit is a scene edit, ordered like gsr_scene_translate.  It runs on the context's stream, with no host wait on
 *   other members' streams: frames that other members of a shared scene enqueued before it read the old scene, frames enqueued
 *   behind it read the new scene.  It marks every member's frame and sorted order as edited: gsr_select_region, gsr_pick,
 *   gsr_depth_async, gsr_contrib_accumulate_async and gsr_overlay_async return GSR_ERR_ARG until the next frame.  A call that
 *   would change no bit still counts as an edit.  With no selection buffers (the scene was never selected in) no kernel is
 *   launched.
 * State that survives: the selection, the hidden set and the contribution accumulators are untouched and indices do not move; the
 *   accumulators then describe the old geometry (gsr_contrib_reset starts a new tour).  The context stays in its shared scene.
 * Requirements and refusals (GSR_ERR_ARG with a message, nothing touched): edits require a scene with rotations / scales (from rows
 *   or from the four arrays), as the whole-scene transforms do.  gsr_scene_rotate_selected and gsr_scene_scale_selected are refused
 *   while gsr_set_sh_follow is on and the scene has SH rows: the SH frame is one per scene and a partial rotation has none;
 *   translate and set_rgba are allowed in that state.  Each scale component must be finite; zero is allowed, because there is no
 *   frame to invert here.  A NULL ctx or a NULL required pointer returns GSR_ERR_ARG with nothing touched.
 * (struct gsr_selection_bounds has no typedef: C keeps a struct tag and a function of one name apart, a typedef it would not.) */
struct gsr_selection_bounds { uint32_t count; float min[3]; float max[3]; };
int gsr_selection_bounds(gsr_ctx *ctx, struct gsr_selection_bounds *out);                       /* blocking */
int gsr_scene_translate_selected(gsr_ctx *ctx, const double *t /* 3 */);
int gsr_scene_rotate_selected(gsr_ctx *ctx, const double *q /* 4: x, y, z, w */, const double *pivot /* 3, or NULL */);
int gsr_scene_scale_selected(gsr_ctx *ctx, const double *s /* 3 */, const double *pivot /* 3, or NULL */);
int gsr_scene_set_rgba_selected(gsr_ctx *ctx, uint32_t rgba, uint32_t byte_mask);

/* ---- rotating SH coefficients ---- a selection turns with its SH colour; a frame is baked into the coefficients
 * The SH frame (gsr_set_sh_follow, above) is one matrix per scene: it answers whole-scene edits and has no answer for "turn these
 * splats about their own centre".  These calls rotate the coefficients themselves, per splat, on the device (DESIGN.md section 4,
 * "Rotating SH coefficients").
 * Basis: B_1 .. B_15 are the direction factors of eval_sh_rgb exactly as vertex.glsl.ts:72-98 writes them, constants and signs
 *   included: band 1 is -C1*y, -C1*z, +C1*x; band 2 is C2[0]*xy .. C2[4]*(xx-yy); band 3 is C3[0]*y*(3xx-yy) .. C3[6]*x*(xx-3yy).
 *   A channel's colour is C0*c_0 + sum c_k B_k(d) + 0.5.
 * Matrices: for a rotation R the band matrices D_1 (3x3), D_2 (5x5), D_3 (7x7) are the unique matrices for which c' = D_l c gives
 *   sum c'_k B_k(R d) = sum c_k B_k(d) for every unit d: after the edit, the colour seen from d is the colour formerly seen from
 *   R^T d, which is what the SH frame does with linv = R^T.  The B_k are +- the orthonormal real SH, so every D_l is orthogonal.
 * gsr_sh_rotation(q, m) is a pure host function that needs no GPU and no context: q = (x, y, z, w) must be finite and non-zero
 *   (GSR_ERR_ARG otherwise; the message is read with gsr_last_error(NULL)); it is normalised in f64, |q| = sqrt(((xx+yy)+zz)+ww);
 *   R is the matrix gsr_scene_rotate builds of the normalised q; m receives D_1, D_2, D_3 row-major, one after the other
 *   (9 + 25 + 49 = 83 doubles).  x = y = z = 0 yields the exact identity.  Each D_l solves the normal equations of
 *   Y_l(S)^T D_l = Y_l(R^T S)^T in f64 over S, 24 Fibonacci-sphere directions (phi = acos(1 - 2(i+0.5)/24),
 *   theta = pi(1+sqrt 5)(i+0.5)); orthogonality, composition and the defining property hold to 2^-40.
 * Apply: one SH row and one channel is 8 words, half 2j in the low 16 bits of word j.  c_j is the half's value, exact; M = (float)m,
 *   rounded once; in f32, uncontracted, per band and for k in band order: s = M[k][j0]*c[j0]; s = s + M[k][j]*c[j] with j ascending
 *   over the band; s is stored as a half rounded to nearest even, subnormals kept, overflow to infinity, any NaN stored as 0x7e00.
 *   Half 0 (DC) keeps its bits.  All three bands are always rotated; a splat's degree only decides which bands the shader reads.
 *   (Uploads truncate; the rotation rounds to nearest, because repeated truncation shrinks coefficients under repeated edits.)
 * gsr_scene_rotate_sh rotates, in place, the coefficients of the SH rows in scope: every SH row (GSR_SH_ALL), or the rows of the
 *   selected splats i > band_index[0] (GSR_SH_SELECTED; selected splats without an SH row are not touched).  rows (may be NULL)
 *   receives the number of rows rotated; for GSR_SH_SELECTED it is counted on the device and copied back, the call's one wait.
 *   It acts in the coefficients' own frame and never reads or writes linv.  No SH state, or GSR_SH_SELECTED with no selection
 *   buffers: GSR_OK, rows = 0, no kernel is launched.  An unknown scope or a bad q: GSR_ERR_ARG, nothing touched.
 * Ordering: a scene edit, ordered and marked exactly like gsr_scene_set_rgba_selected: the context's stream, events among the
 *   members of a shared scene, every member's frame and sorted order marked as edited.  The SH textures are per-scene state, so one
 *   call serves every member.  The selection, the hidden set, the accumulators, the frame and the follow switch are untouched.
 * gsr_scene_rotate_selected_sh is gsr_scene_rotate_selected(q, pivot) followed by gsr_scene_rotate_sh(q, GSR_SH_SELECTED), as one
 *   edit: the geometry goes through the same kernel with q as given, the coefficients use the normalised q.  It is allowed with
 *   follow on or off, provided the SH frame is the identity; otherwise GSR_ERR_ARG with a message naming
 *   gsr_scene_bake_sh_frame, and nothing is touched.  Without SH rows it is gsr_scene_rotate_selected.
 *   gsr_scene_rotate_selected itself keeps its refusal.
 * gsr_scene_bake_sh_frame moves a frame that is a rotation times a positive uniform scale into the coefficients:
 *   s2 = (sum linv_ij^2) / 3; GSR_ERR_ARG with nothing changed unless max |(linv . linv^T)_ij / s2 - delta_ij| <= 2^-20 and
 *   det > 0 (a condition, not a measurement: the projection rounds the frame to f32, so a frame within 2^-20 of a scaled rotation
 *   is one as far as any direction it produces goes; a frame that holds a non-uniform scale has no rotation).  Q = linv / sqrt(s2);
 *   q_used (4, may be NULL) is the quaternion of Q^T by Shepperd's four branches as gsr_rigid_decompose states them; then
 *   gsr_scene_rotate_sh(q_used, GSR_SH_ALL), and the frame becomes the identity.  An identity frame: GSR_OK, q_used = (0, 0, 0, 1),
 *   nothing launched.
 * A NULL ctx or a NULL q returns GSR_ERR_ARG with nothing touched. */
#define GSR_SH_ALL      0u
#define GSR_SH_SELECTED 1u
int gsr_sh_rotation(const double *q /* 4: x, y, z, w */, double *m /* 83 */);
int gsr_scene_rotate_sh(gsr_ctx *ctx, const double *q /* 4: x, y, z, w */, uint32_t scope /* GSR_SH_ALL | GSR_SH_SELECTED */, uint32_t *rows);
int gsr_scene_rotate_selected_sh(gsr_ctx *ctx, const double *q /* 4: x, y, z, w */, const double *pivot /* 3, or NULL */);
int gsr_scene_bake_sh_frame(gsr_ctx *ctx, double *q_used /* 4, may be NULL */);

/* ---- growing the scene ---- duplicate the selection, append another scene's selected splats or rows from the host, reserve capacity
 * Every call above keeps the splat count or lowers it.  These raise it on the device: copy an object, paste one capture's splats
 * into another scene, add rows -- with no gsr_read_scene / host loop / gsr_set_scene_arrays round trip (which re-uploads and
 * re-allocates the whole scene, drops the selection, the hidden set and the accumulators, and takes the context out of a shared
 * scene).  n is the count before the call ("Growing the scene").
 * Duplicate: with idx the selected indices in ascending order and k their number, gsr_scene_duplicate_selected leaves a scene of
 *   n + k splats.  Rows [0, n) are not written at all.  Row n + j holds the bits of row idx[j] in every per-splat array
 *   (positions, covariance words, rgba, rotations, scales): the copy is bit for bit, NaNs and -0.0 included, with no arithmetic
 *   and no re-packing of the covariance.  *first = n, *count = k (either pointer may be NULL).  k is the selection's count, which the
 *   host already knows: nothing is read back to learn it.  With k == 0 the call returns GSR_OK with count 0, touches nothing and is
 *   not an edit: the last frame stays valid.
 * Append selected: gsr_scene_append_selected is duplicate with the rows read from `from`'s scene and `from`'s selection.  `from`
 *   must be on the same device and its scene must have rotations / scales.  from == ctx, or a member of the same shared scene, is
 *   exactly duplicate.  `from`'s scene, selection and frame state are not changed; its stream is waited for on the device, not on
 *   the host.  `from`'s SH rows are not carried: the copies keep their rgba word.
 * Append arrays: the m rows of gsr_scene_append_arrays go through the same repack and check as gsr_set_scene_arrays, into rows
 *   [n, n + m); no new arithmetic.  A refused upload (GSR_ERR_SCENE: positions differ from data words 0..2) leaves everything as it
 *   was, the count and the capacity included.  Rows [0, n) are not written.  A scene with no splats and no rotations / scales
 *   accepts the call and becomes a scene with them.  *first = n (may be NULL); m == 0 touches nothing.
 * State afterwards: the selection becomes exactly the new rows [first, first + count) -- a REPLACE, so the next
 *   gsr_scene_translate_selected moves the copies -- and its version moves; the bits are set on the device, no upload proportional to
 *   n is made.  The hidden set keeps its bits; new rows are visible, and so is the copy of a hidden selected splat.  The
 *   contribution accumulators, if live, keep the old rows' values and `frames`; new rows start at zero (if never reset they stay
 *   "never reset").  Indices of existing splats do not move.  The context stays in its shared scene.
 * Capacity: the scene arrays hold gsr_scene_capacity rows, at least the count.  If n + k <= capacity nothing of the scene arrays is
 *   re-allocated and no old row is copied.  Otherwise the arrays grow to max(n + k, capacity + capacity / 2), capped by the upload's
 *   limit of 0x7fffffff / 8 splats, and the old rows are carried by device copies.  The selection, hidden and contribution buffers
 *   grow with the capacity where they exist.  gsr_scene_reserve performs the growth alone, to exactly `rows`, for a host that will
 *   copy an object many times: capacity >= rows afterwards, it never shrinks, no splat changes and no frame state changes.
 *   gsr_scene_sharing's scene_bytes reports the capacity.  gsr_scene_limit_box and gsr_scene_erase_selected keep their behaviour
 *   (the compacted arrays hold the old count's rows).
 * Ordering: the calls are blocking scene replacements like gsr_scene_limit_box: the other members' streams are waited for, the work
 *   runs on the context's stream, and every member re-sizes its per-splat buffers before its next frame.  They mark every member's
 *   frame and sorted order as edited: gsr_select_region, gsr_pick, gsr_depth_async, gsr_contrib_accumulate_async and
 *   gsr_overlay_async return GSR_ERR_ARG until the next frame.
 * Refusals (GSR_ERR_ARG with a message, nothing touched): a NULL ctx; a NULL `from`; a NULL data / positions / rotations / scales
 *   with m > 0; a destination without rotations / scales (but the empty scene of append arrays above); a `from` on another device or
 *   without rotations / scales; n + k above the upload's limit; and a destination that has SH rows (sh_count != 0): SH rows are
 *   indexed by splat order and the bands are index thresholds, so a row appended at the tail would fall into the top band and has no
 *   SH row to read. */
int gsr_scene_reserve(gsr_ctx *ctx, uint32_t rows);          /* capacity >= rows; never shrinks; no splat changes */
int gsr_scene_capacity(gsr_ctx *ctx, uint32_t *rows);        /* no copy, no wait */
int gsr_scene_duplicate_selected(gsr_ctx *ctx, uint32_t *first, uint32_t *count);
int gsr_scene_append_selected(gsr_ctx *ctx, gsr_ctx *from, uint32_t *first, uint32_t *count);
int gsr_scene_append_arrays(gsr_ctx *ctx, const uint32_t *data, const float *positions, const float *rotations,
                            const float *scales, uint32_t m, uint32_t *first);

/* ---- contribution ---- per-splat weight, peak and pixel counts over views
 * No interface of the reference stands behind this section either.  Every selector above is geometric; this one answers "which
 * splats never show" -- buried inside surfaces, hidden behind them, touching no pixel from any camera of a tour -- and with
 * gsr_scene_erase_selected prunes a scene by rendered contribution, on the device, with no read-back of frames.
 * Definition ("Contribution").  For the last rendered frame, a pixel's fragments, their weight B and the
 * transmittance T are exactly those of "depth and pick": the entries of the pixel's bin list, in list order, that pass q <= 4;
 * w = T * B, then T = T - w, in f32, with no early termination, no saturation skip and no segments.  For every splat i of the
 * scene three accumulators are held on the device with the scene:
 *   weight[i], uint64_t: the sum over the pixels where i is a fragment of (uint64_t)rintf(w * 16777216.0f) -- the fragment's
 *     weight in quanta of 2^-24, ties to even; w <= 1, so one term is at most 2^24.  Integers make the sum independent of the
 *     order in which tiles, bins, contexts and views arrive.
 *   peak[i], float: the maximum over those pixels of w (w >= 0: taken on the bit patterns, exact and order-free).
 *   pixels[i], uint32_t: the number of those pixels -- the fragments with q <= 4 whatever their weight.  It wraps modulo 2^32.
 * and one word, frames: the passes that contributed since the last reset.  Only pixels of the image count (a partial last bin's
 * other pixels have no fragments).  Accumulation continues across calls: sums add, peaks take the maximum.  A band context walks
 * its own bin columns only; bands that partition the pixels on bin columns (multiples of 32) partition the fragments, and the
 * host combines ranks by adding weight and pixels and taking the maximum of peak.
 * gsr_contrib_reset allocates on first use (16 bytes per splat row plus the counter words, 8 bytes), zeroes the accumulators and
 *   frames, and is blocking: it waits for every member's stream of a shared scene, as gsr_set_scene_sh does.
 * gsr_contrib_accumulate_async enqueues the pass behind the last enqueued frame on the context's stream: no host wait, nothing
 *   allocated after the first use.  It needs of the frame exactly what gsr_depth_async needs, otherwise GSR_ERR_ARG and nothing
 *   is enqueued.  Without a prior reset the first call does what gsr_contrib_reset does first.  A frame whose lists did not fit
 *   contributes nothing and does not bump frames (the pass reads the frame's overflow word on the device; render the pose again
 *   after gsr_sync has regrown the lists).  The frame, the framebuffer, the statistics, the depth planes and their validity are
 *   not touched.
 * gsr_read_contrib is blocking: it settles the streams that may hold passes (of a shared scene: every member's), then copies the
 *   accumulators.  Any output may be NULL.  n must equal the scene's count, else GSR_ERR_ARG; GSR_ERR_ARG also when nothing was
 *   ever reset or accumulated.
 * gsr_select_contrib picks P = { i in [0, n) : value_i < below }, compared in f64 on the device over ALL splats of the scene,
 *   where value is (double)weight * 2^-24 ("fully opaque pixels' worth"), (double)peak or (double)pixels; a splat no frame ever
 *   listed has value 0.  P is folded into the selection with `op` (GSR_SELOP_*) exactly as the selection calls fold theirs; it is
 *   blocking, and `selected` means what it means everywhere else.  GSR_ERR_ARG, nothing changed: an unknown stat or op, a NaN
 *   `below`, or frames == 0 -- the last refusal keeps an empty tour from selecting the whole scene.
 * Where the state lives: with the scene, beside the selection.  The members of a shared scene have ONE set of accumulators and
 * may run passes concurrently on their own streams: the updates are agent-scope integer atomics and commute.  gsr_scene_sharing's
 * scene_bytes counts the buffers once they exist.  gsr_scene_translate, _rotate and _scale keep the accumulators (the indices
 * still mean the same splats); gsr_scene_limit_box, an erase that removes something, gsr_set_scene, _arrays and _rows, and leaving
 * a share drop them: back to "never reset".  After gsr_share_scene, ctx sees `from`'s accumulators.  A context that never calls
 * any of this allocates nothing and launches nothing. */
#define GSR_CONTRIB_WEIGHT 0   /* value = (double)weight * 2^-24: "fully opaque pixels' worth" */
#define GSR_CONTRIB_PEAK   1   /* value = (double)peak */
#define GSR_CONTRIB_PIXELS 2   /* value = (double)pixels */
int gsr_contrib_reset(gsr_ctx *ctx);
int gsr_contrib_accumulate_async(gsr_ctx *ctx);
int gsr_read_contrib(gsr_ctx *ctx, uint64_t *weight, float *peak, uint32_t *pixels, uint32_t n, uint32_t *frames);
int gsr_select_contrib(gsr_ctx *ctx, int32_t stat, double below, int32_t op, uint32_t *selected);

/* ---- splat data ---- attribute statistics, histograms and range selection on the device
 * No interface of the reference stands behind this section either.  Every picker above asks where a splat is on the screen, in a
 * box, or how much it showed; these ask about the splats themselves -- how opacity, size, colour and distance from a point are
 * distributed in a scene, and which splats lie in a range of one of them (the near-transparent, the huge, everything farther than
 * r from here) -- with no gsr_read_scene of the whole scene and no host loop.  They also show where the mass of the contribution
 * accumulators lies before gsr_select_contrib is handed a threshold.
 * The value of attribute a of splat i is a double ("Splat data"; stated once on the device, in f64, in the
 * written order, uncontracted):
 *   GSR_ATTR_X, _Y, _Z               (double)position component
 *   GSR_ATTR_DISTANCE                dx = (double)x - origin[0], dy and dz likewise; sqrt((dx*dx + dy*dy) + dz*dz), the square root
 *                                    correctly rounded
 *   GSR_ATTR_RED, _GREEN, _BLUE, _OPACITY   that byte of the colour word, 0 .. 255, numbered as gsr_scene_set_rgba_selected numbers
 *                                    them: r, g, b the low three bytes, opacity the top byte
 *   GSR_ATTR_SCALE_X, _Y, _Z         (double)scale component
 *   GSR_ATTR_SCALE_MIN, _MAX         NaN if any scale component is NaN; otherwise the smallest / largest of the three
 *   GSR_ATTR_CONTRIB_WEIGHT, _PEAK, _PIXELS   exactly the value gsr_select_contrib compares: (double)weight * 2^-24, (double)peak,
 *                                    (double)pixels (one function on the device serves both calls)
 * `origin` (3 doubles) is read for GSR_ATTR_DISTANCE only and ignored otherwise.
 * Scope: GSR_SCOPE_SELECTED counts only splats in the selection, GSR_SCOPE_VISIBLE only splats not in the hidden set; the flags
 *   combine, 0 is every splat.  A scene never selected in has the empty selection, one that never hid has nothing hidden.  A run of
 *   64 splats with none in scope costs its set words and no read of the scene.
 * gsr_attr_stats: count = the splats in scope; nan = those whose value is NaN; min / max over the others, infinities included
 *   (compared as values: -0.0 and 0.0 are equal, and which of them a bound holds is not defined).  With no non-NaN value min is +inf
 *   and max is -inf.  Any out pointer may be NULL.  An empty scene returns zeros and that empty box.
 * gsr_attr_histogram needs 1 <= bins <= 4096, lo < hi, both finite, hi - lo finite.  The edge rule, in f64:
 *     w = (hi - lo) / (double)bins;   edge(k) = k == bins ? hi : min(lo + (double)k * w, hi)
 *   The edges are nondecreasing and edge(0) == lo.  A value v is in range iff lo <= v && v < hi, and its bin is the largest b < bins
 *   with edge(b) <= v -- decided by comparisons against the edges, not by floor((v - lo) / w), which disagrees at the edges.
 *   counts[bins] receives the bins; outside[3] the splats in scope with v < lo, with v >= hi, and with a NaN value, so
 *   sum(counts) + sum(outside) == count of gsr_attr_stats.  Either pointer may be NULL.
 * gsr_select_attr picks P = { i in [0, n) : lo <= v_i && v_i < hi } over ALL splats of the scene, hidden ones included; a NaN value
 *   is never picked.  lo and hi may be infinite (lo = -inf: "below hi"); lo == hi picks nothing.  P is folded into the selection
 *   with `op` (GSR_SELOP_*) exactly as the selection calls fold theirs, and `selected` means what it means everywhere else.
 * The consistency guarantee: for 0 <= a < b <= bins, gsr_select_attr(attr, origin, edge(a), edge(b), GSR_SELOP_REPLACE) selects
 *   exactly sum(counts[a .. b-1]) splats of a scope-0 gsr_attr_histogram over the same [lo, hi) and bins: what the histogram
 *   shows is what the range selects.  A host computes edge(k) with the f64 formula above.
 * All three are blocking and ordered like gsr_select_contrib: they wait for every member's stream of a shared scene first.  They
 *   read the scene and write none of it: no frame state changes.  Counts are integers and min / max commute, so every result is
 *   exact and independent of the order of arrival.
 * Refusals (GSR_ERR_ARG with a message, nothing touched, the selection and its count included): an unknown attribute code, scope
 *   flag or op; for GSR_ATTR_DISTANCE a NULL origin or a non-finite origin component; the scale attributes on a scene without
 *   rotations / scales (as gsr_scene_scale_selected refuses); the contribution attributes while nothing was ever reset or
 *   accumulated or frames == 0 (as gsr_select_contrib refuses); bins, lo or hi outside what the histogram needs; a NaN bound or
 *   lo > hi for gsr_select_attr.
 * The device words the reductions need (a few tens of KB) belong to the context and are allocated by the first call; a context
 * that never calls any of this allocates nothing and launches nothing. */
#define GSR_ATTR_X 0
#define GSR_ATTR_Y 1
#define GSR_ATTR_Z 2
#define GSR_ATTR_DISTANCE 3         /* from `origin` */
#define GSR_ATTR_RED 4
#define GSR_ATTR_GREEN 5
#define GSR_ATTR_BLUE 6
#define GSR_ATTR_OPACITY 7
#define GSR_ATTR_SCALE_X 8
#define GSR_ATTR_SCALE_Y 9
#define GSR_ATTR_SCALE_Z 10
#define GSR_ATTR_SCALE_MIN 11
#define GSR_ATTR_SCALE_MAX 12
#define GSR_ATTR_CONTRIB_WEIGHT 13
#define GSR_ATTR_CONTRIB_PEAK 14
#define GSR_ATTR_CONTRIB_PIXELS 15
#define GSR_SCOPE_SELECTED 1u   /* only splats in the selection */
#define GSR_SCOPE_VISIBLE  2u   /* only splats not in the hidden set */   /* 0: every splat; flags combine */
int gsr_attr_stats(gsr_ctx *ctx, int32_t attr, const double *origin, uint32_t scope,
                   uint32_t *count, uint32_t *nan, double *min, double *max);
int gsr_attr_histogram(gsr_ctx *ctx, int32_t attr, const double *origin, uint32_t scope,
                       double lo, double hi, uint32_t bins, uint32_t *counts, uint32_t *outside);
int gsr_select_attr(gsr_ctx *ctx, int32_t attr, const double *origin, double lo, double hi,
                    int32_t op, uint32_t *selected);

/* ---- neighbours ---- how many other splats lie within a radius of each splat: floaters found by local density
 * No interface of the reference stands behind this section either.  Every picker above judges a splat alone; the clean-up every
 * captured scene needs first is floaters -- isolated splats hanging in empty space -- and what marks a floater is no attribute of
 * its own: it has no neighbours.  Point-cloud tools call the operation radius outlier removal: count the points within r of each
 * point and drop those with fewer than k.  These two calls do it on the device, with no gsr_read_scene and no spatial index on
 * the host:  gsr_select_neighbours(ctx, r, cap, 0, 0, 0, k, GSR_SELOP_REPLACE, ..) then gsr_scene_erase_selected.
 * Definition ("Neighbours").  Scope S is the GSR_SCOPE_SELECTED | GSR_SCOPE_VISIBLE flags of "splat data",
 * with the same meaning; 0 is every splat.  For splats i, j of the scene, in f64, in the written order, uncontracted:
 *     dx = (double)x_i - (double)x_j;  dy, dz likewise
 *     d2(i,j) = (dx*dx + dy*dy) + dz*dz
 *     r2 = radius * radius                      (computed once on the host)
 *     near(i,j)  :=  i != j  &&  d2(i,j) <= r2
 *     count_i = min(cap, #{ j in S : near(i,j) })   for i in S;      count_i = 0   for i not in S
 *   d2 is symmetric.  Distance exactly radius counts.  Coincident splats count each other.  A splat does not count itself.  A NaN
 *   or infinite position component needs no special case: the comparison is false, so such a splat has count 0 and is nobody's
 *   neighbour (it is kept out of the index).  Counts are integers decided by f64 comparisons, so every result is exact and
 *   independent of the order of arrival.
 * gsr_neighbours: counts is n words or NULL; a non-NULL counts with n not equal to the scene's count is refused.  hist is cap + 1
 *   words or NULL: hist[k] is the number of splats in S with count == k, so hist[cap] means "cap or more", and
 *   sum(hist) == info->in_scope.  info may be NULL.  An empty scene, or an empty scope, returns zeros.
 * gsr_select_neighbours picks P = { i in S : lo <= count_i && count_i < hi }, with lo <= hi <= cap + 1, and folds P into the
 *   selection with `op` (GSR_SELOP_*) exactly as the selection calls fold theirs; `selected` means what it means everywhere else.
 *   lo == hi picks nothing.
 * The consistency guarantee: with GSR_SELOP_REPLACE it selects exactly sum(hist[lo .. hi-1]) splats of a gsr_neighbours call with
 *   the same radius, cap and scope: what the histogram shows is what the range selects.
 * info: in_scope = the splats in S; nonfinite = those of them with a NaN or infinite position component (count 0, in hist[0]);
 *   pair_bound and budget as below.
 * The work budget.  These machines are shared and a radius that puts the whole scene into one cell is an O(n^2) kernel.  Both calls
 *   build the index first -- a hashed uniform grid of cells a little wider than radius -- and a cheap pass then computes pair_bound:
 *   for every indexed splat, the sum of the populations of the 27 hash buckets the count pass walks for it, i.e. the pair tests the
 *   count pass makes at most (no early exit), as the implementation counts them; it is never below the exact 27-cell neighbourhood
 *   sum.  If pair_bound > budget the call returns GSR_ERR_ARG with a message naming both numbers; it fills info and launches no
 *   count kernel.  budget == 0 means GSR_NEIGHBOUR_DEFAULT_BUDGET; a budget above GSR_NEIGHBOUR_MAX_BUDGET is refused.
 * Both calls are blocking and stateless: they index the scene as it is now, so nothing can go stale after an edit.  They are
 *   ordered like gsr_select_attr: they wait for every member's stream of a shared scene first.  They read the scene and write none
 *   of it: no frame state changes.
 * Refusals (GSR_ERR_ARG with a message, nothing touched, the selection and its count included): a NULL ctx; a radius that is not
 *   finite, not > 0, or with radius * radius or 1 / radius not finite and normal; cap outside 1 .. 4095; unknown scope flags or op;
 *   lo > hi or hi > cap + 1; a budget above the maximum; a bound above the budget.
 * The device scratch belongs to the context: the index (8 bytes per hash bucket, a power of two of at least twice the scene's
 *   count, and 24 bytes per splat), the counts (4 bytes per splat) and a histogram of at most 4096 counters.  The first call
 *   allocates it, it only grows, and gsr_destroy frees it; a context that never calls any of this allocates nothing and launches
 *   nothing. */
typedef struct gsr_neighbour_info {
    uint32_t in_scope;      /* splats in S */
    uint32_t nonfinite;     /* of those, with a NaN or infinite position component */
    uint64_t pair_bound;    /* pair tests the count pass makes at most (no early exit), as the implementation counts them */
    uint64_t budget;        /* the budget that applied */
} gsr_neighbour_info;
#define GSR_NEIGHBOUR_MAX_CAP 4095u
#define GSR_NEIGHBOUR_DEFAULT_BUDGET (1ull << 34)   /* about 43 ms of count pass at the 4.0e11 pair tests per second measured on one MI355X */
#define GSR_NEIGHBOUR_MAX_BUDGET     (1ull << 38)   /* about 0.7 s at that rate */
int gsr_neighbours(gsr_ctx *ctx, double radius, uint32_t cap, uint32_t scope, uint64_t budget,
                   uint32_t *counts, uint32_t n, uint32_t *hist, gsr_neighbour_info *info);
int gsr_select_neighbours(gsr_ctx *ctx, double radius, uint32_t cap, uint32_t scope, uint64_t budget,
                          uint32_t lo, uint32_t hi, int32_t op, uint32_t *selected, gsr_neighbour_info *info);

/* ---- clusters ---- connected islands of splats labelled, sized and selected
 * No interface of the reference stands behind this section either.  A neighbour count finds thin floaters; it cannot find a dense
 * blob of a few hundred splats hanging in mid-air, or a second object beside the one the user wants: inside such a blob every
 * splat has plenty of neighbours.  Point-cloud tools answer with clustering -- connected components at a linking radius, or DBSCAN
 * with a core threshold -- and two operations rest on it: "remove every island smaller than k splats" / "keep only the largest
 * island", and "select the island under the cursor", the flood select that goes with gsr_pick.  These calls do it on the device,
 * over the index of "neighbours", with no gsr_read_scene and no spatial index on the host.
 * Definition ("Clusters").  Scope S, near(i,j) and the treatment of non-finite rows are exactly those of
 *   "neighbours": the same f64 expression, in the written order, uncontracted, and a distance of exactly radius counts; a splat with
 *   a NaN or infinite position component is in scope, is never indexed and is nobody's neighbour.  With min_pts in
 *   0 .. GSR_NEIGHBOUR_MAX_CAP:
 *     deg_i   = #{ j in S : near(i,j) }                 (only deg_i >= min_pts is ever needed: the count may stop at min_pts)
 *     core_i  := i in S, finite, deg_i >= min_pts       (min_pts == 0: every finite splat in scope is core: plain connected components)
 *     i ~ j   := core_i && core_j && near(i,j);   clusters = the classes of the transitive closure of ~ over core splats
 *     label_i = the smallest splat index in i's class                           for a core splat
 *     label_i = min{ label_j : core_j && near(i,j) }                            for a non-core finite splat in S with such a j ("border")
 *     label_i = GSR_CLUSTER_NONE                                                otherwise (noise, non-finite, out of scope)
 *     size_i  = #{ k : label_k == label_i }  if label_i != GSR_CLUSTER_NONE, else 0
 *   A border splat never joins two clusters: it takes the smaller label, so the result does not depend on any visiting order.  The
 *   largest cluster is the one of greatest size, ties going to the smallest label.  All results are integers decided by f64
 *   comparisons: the same scene, scope, radius and min_pts give the same words on every run, in every context form and through
 *   every member of a shared scene.
 * gsr_clusters: labels and sizes are n words each, or NULL; a non-NULL pointer with n not equal to the scene's count is refused.
 *   sizes is per splat: sizes[i] = size_i.  info may be NULL.  An empty scene, or an empty scope, returns zeros (largest_label
 *   GSR_CLUSTER_NONE).
 * gsr_select_clusters picks P = { i in S : size_lo <= size_i && size_i < size_hi }, with size_lo <= size_hi, and folds P into the
 *   selection with `op` (GSR_SELOP_*) exactly as the selection calls fold theirs; `selected` means what it means everywhere else.
 *   size_lo == size_hi picks nothing.  Noise and non-finite splats in S have size 0.
 * The consistency guarantee: with GSR_SELOP_REPLACE it selects exactly the number of splats in S whose sizes[i] from a gsr_clusters
 *   call with the same radius, min_pts and scope lies in the range.  gsr_select_clusters(.., 0, k, ..) then gsr_scene_erase_selected
 *   removes noise and every island smaller than k.
 * gsr_select_cluster_at picks P = { i : label_i == label_seed && label_seed != GSR_CLUSTER_NONE } and folds it the same way.  seed
 *   is a splat index below the scene's count, or GSR_CLUSTER_LARGEST for the largest cluster.  A seed that is noise or out of
 *   scope, or GSR_CLUSTER_LARGEST when there is no cluster, picks the empty set: the fold still happens.  "Keep the largest
 *   island" is gsr_select_cluster_at(.., GSR_CLUSTER_LARGEST, GSR_SELOP_REPLACE, ..), gsr_selection_invert, gsr_scene_erase_selected.
 * info: in_scope, nonfinite, pair_bound and budget as in gsr_neighbour_info; core, border and noise count the splats in S by kind,
 *   noise including the non-finite ones, so in_scope == core + border + noise; clusters is the number of clusters; largest_label
 *   and largest_size name the largest one (GSR_CLUSTER_NONE and 0 when there is no cluster).
 * The work budget is the neighbour budget, with the same constants and the same pair_bound, checked before any walk is launched:
 *   if pair_bound > budget the call returns GSR_ERR_ARG with a message naming both numbers, fills info's first four fields and
 *   launches no walk.  A call makes up to three 27-cell walks -- the core test (none for min_pts == 0), the union and the border pass
 *   (none for min_pts == 0) -- each of at most pair_bound pair tests: the budget bounds each walk, not their sum.
 * All three calls are blocking and stateless: they index the scene as it is now, so nothing can go stale after an edit.  They are
 *   ordered like gsr_select_attr: they wait for every member's stream of a shared scene first.  They read the scene and write none
 *   of it: no frame state changes.
 * Refusals (GSR_ERR_ARG with a message, nothing touched, the selection and its count included): a NULL ctx; a radius that is not
 *   finite, not > 0, or with radius * radius or 1 / radius not finite and normal; min_pts above 4095; unknown scope flags or op;
 *   size_lo > size_hi; a seed that is neither below the scene's count nor GSR_CLUSTER_LARGEST; a wrong n; a budget above the
 *   maximum; a bound above the budget.  GSR_ERR_HIP, should the union ever meet an inconsistent parent word or exceed its step limit
 *   of n: the call ends instead of occupying the device.
 * The device scratch belongs to the context: the scratch of "neighbours" and 12 bytes per splat (parent / label, size by label,
 *   size by splat).  The first cluster call allocates it, it only grows, and gsr_destroy frees it; a context that never calls any of
 *   this allocates nothing and launches nothing. */
typedef struct gsr_cluster_info {
    uint32_t in_scope;      /* splats in S */
    uint32_t nonfinite;     /* of those, with a NaN or infinite position component (noise) */
    uint64_t pair_bound;    /* pair tests ONE walk makes at most, as the implementation counts them */
    uint64_t budget;        /* the budget that applied */
    uint32_t core;          /* splats in S that are core */
    uint32_t border;        /* non-core splats in S labelled by a core neighbour */
    uint32_t noise;         /* the rest of S, the non-finite ones included */
    uint32_t clusters;      /* number of clusters */
    uint32_t largest_label; /* label of the largest cluster (ties: the smallest label); GSR_CLUSTER_NONE: there is none */
    uint32_t largest_size;  /* its size; 0: there is none */
} gsr_cluster_info;
#define GSR_CLUSTER_NONE    0xffffffffu   /* a label: in no cluster */
#define GSR_CLUSTER_LARGEST 0xffffffffu   /* a seed: the largest cluster */
int gsr_clusters(gsr_ctx *ctx, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget,
                 uint32_t *labels, uint32_t *sizes, uint32_t n, gsr_cluster_info *info);
int gsr_select_clusters(gsr_ctx *ctx, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget,
                        uint32_t size_lo, uint32_t size_hi, int32_t op, uint32_t *selected, gsr_cluster_info *info);
int gsr_select_cluster_at(gsr_ctx *ctx, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget,
                          uint32_t seed, int32_t op, uint32_t *selected, gsr_cluster_info *info);

/* ---- k nearest neighbours ---- per-splat neighbour lists, and statistical outlier removal
 * No interface of the reference stands behind this section either.  A radius count needs the user to know the scene's density in
 * advance and misjudges a capture whose density varies from the subject to the background.  "Mean distance to the k nearest,
 * against the scene's own distribution of that value" adapts by itself: point-cloud tools call the filter statistical outlier
 * removal.  The lists themselves -- indices and squared distances in a defined order -- are what normals, smoothing and
 * density-aware pruning start from.  These calls make them on the device, over the index of "neighbours", with no gsr_read_scene
 * and no spatial index on the host.
 * Definition ("k nearest neighbours").  Scope S, d2(i,j), r2, near(i,j) and the treatment of non-finite rows
 *   are exactly those of "neighbours": the same f64 expression, in the written order, uncontracted, and a distance of exactly radius
 *   counts; a splat with a NaN or infinite position component is in scope, is never indexed and is nobody's neighbour.  The search
 *   is the hybrid form, the k nearest WITHIN radius.  With 1 <= k <= GSR_KNN_MAX_K:
 *     N_i    = { j in S : near(i,j) }, ordered ascending by the pair (d2(i,j), j): equal distances go to the smaller index
 *     m_i    = min(k, |N_i|)   for i in S and finite;   0 otherwise                        ("found")
 *     nn_i[t], dd_i[t] = index and d2 of the t-th element of that order, t < m_i;
 *                        GSR_KNN_NONE and +inf for m_i <= t < k
 *     value_i (GSR_KNN_KTH)  = m_i == k ? sqrt(dd_i[k-1]) : +inf        (sqrt correctly rounded, as GSR_ATTR_DISTANCE states it)
 *     value_i (GSR_KNN_MEAN) = m_i == 0 ? +inf : ( ..((sqrt(dd_i[0]) + sqrt(dd_i[1])) + sqrt(dd_i[2])) .. ) / (double)m_i
 *                              (f64, summed in ascending t, uncontracted)
 *     value_i = NaN (0x7ff8000000000000) for i not in S
 *   A non-finite splat in S has m_i = 0 and value +inf.  The order is total, so the lists do not depend on any visiting order;
 *   every value is a sequence of correctly rounded f64 operations in a stated order: the same scene, scope, radius, k and stat give
 *   the same bits on every run, in every context form and through every member of a shared scene.
 * gsr_knn: found is n words, idx n * k words, d2 n * k doubles, values n doubles, row i of a list at [i * k]; any out pointer may
 *   be NULL; a non-NULL per-splat pointer with n not equal to the scene's count is refused.  Rows outside S hold found = 0,
 *   GSR_KNN_NONE, +inf and NaN.  hist is k + 1 words or NULL: hist[t] is the number of splats in S with m_i == t, so
 *   sum(hist) == info->in_scope.  info may be NULL.  An empty scene, or an empty scope, returns zeros (value_min +inf, value_max -inf).
 * info: in_scope, nonfinite, pair_bound and budget as in gsr_neighbour_info; complete = the splats with m_i == k; finite_values =
 *   the splats in S with a finite value_i; value_min / value_max over those finite values, +inf / -inf when there is none, as in
 *   gsr_attr_stats.  Every field is an integer or a min / max, so every field is exact.
 * gsr_select_knn picks P = { i in S : lo <= value_i && (value_i < hi || hi == +inf) } and folds P into the selection with `op`
 *   (GSR_SELOP_*) exactly as the selection calls fold theirs; `selected` means what it means everywhere else.  +inf is a value
 *   splats really have here -- "no k-th neighbour within radius" -- so hi = +inf means "no upper end": the one difference from
 *   gsr_select_attr.  lo == hi (both finite) picks nothing.  Statistical outlier removal: read values, take the mean mu and the
 *   standard deviation sigma of the finite ones on the host, gsr_select_knn(.., lo = mu + ratio * sigma, hi = +inf, ..), then
 *   gsr_scene_erase_selected.
 * The consistency guarantee: with GSR_SELOP_REPLACE it selects exactly the splats of S whose values[i], from a gsr_knn call with
 *   the same radius, k, scope and stat, satisfy the rule.
 * The work budget is the neighbour budget, with the same constants and the same pair_bound, checked before the walk is launched:
 *   if pair_bound > budget the call returns GSR_ERR_ARG with a message naming both numbers, fills info's first four fields and
 *   launches no walk.  A call makes one 27-cell walk of at most pair_bound pair tests.
 * Both calls are blocking and stateless: they index the scene as it is now, so nothing can go stale after an edit.  They are
 *   ordered like gsr_select_attr: they wait for every member's stream of a shared scene first.  They read the scene and write none
 *   of it: no frame state changes.
 * Refusals (GSR_ERR_ARG with a message, nothing touched, the selection and its count included): a NULL ctx; a radius that is not
 *   finite, not > 0, or with radius * radius or 1 / radius not finite and normal; k outside 1 .. 32; unknown scope flags, stat or
 *   op; a NaN bound or lo > hi; a wrong n; a budget above the maximum; a bound above the budget.
 * The device scratch belongs to the context: the scratch of "neighbours", 4 + 8 bytes per splat for found and values, and 12 bytes
 *   per splat per k for the lists, only when idx or d2 is asked for.  The first call allocates it, it only grows, and gsr_destroy
 *   frees it; a context that never calls any of this allocates nothing and launches nothing. */
typedef struct gsr_knn_info {
    uint32_t in_scope;      /* splats in S */
    uint32_t nonfinite;     /* of those, with a NaN or infinite position component (found 0, value +inf) */
    uint64_t pair_bound;    /* pair tests the walk makes at most, as the implementation counts them */
    uint64_t budget;        /* the budget that applied */
    uint32_t complete;      /* splats in S with a full list: m_i == k */
    uint32_t finite_values; /* splats in S with a finite value */
    double value_min;       /* over the finite values; +inf: there is none */
    double value_max;       /* over the finite values; -inf: there is none */
} gsr_knn_info;
#define GSR_KNN_MAX_K 32u
#define GSR_KNN_NONE  0xffffffffu   /* an empty list slot */
#define GSR_KNN_KTH  0              /* value: the distance to the k-th nearest */
#define GSR_KNN_MEAN 1              /* value: the mean distance to those found */
int gsr_knn(gsr_ctx *ctx, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat,
            uint32_t *found, uint32_t *idx, double *d2, double *values, uint32_t n, uint32_t *hist, gsr_knn_info *info);
int gsr_select_knn(gsr_ctx *ctx, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat,
                   double lo, double hi, int32_t op, uint32_t *selected, gsr_knn_info *info);

/* ---- merging cells ---- voxel simplification: the splats of every grid cell merged into one by moment matching
 * No interface of the reference stands behind this section either.  The calls above prune a scene -- by contribution, outliers or
 * islands -- and none of them makes it coarser.  Point-cloud tools call the operation voxel down-sampling; for Gaussians it is not
 * "keep one point per cell": the splats of a cell are merged into one whose mass, mean and covariance are those of the mixture.
 * gsr_cells is the read-only report, gsr_scene_merge_cells the edit that does exactly what the report announced, on the device,
 * over the index of "neighbours", with no gsr_read_scene.
 * Definition ("Merging cells").  Scope S is the GSR_SCOPE_SELECTED | GSR_SCOPE_VISIBLE flags of "splat data",
 *   with the same meaning; 0 is every splat.
 *   Candidate: splat i is a candidate iff it is in S and all ten floats (position, rotation, scale) are finite.
 *   Cell: inv = 1.0 / cell, computed once on the host; per axis the coordinate is floor((double)x * inv) clamped to [-2^20, 2^20),
 *     the cell coordinate of "neighbours" with no slack, because no radius is involved.  Everything at or beyond the clamp shares
 *     the boundary cell.
 *   Members: the members of a cell are its candidates; m is their number; the leader is the smallest member index.
 * gsr_cells: leader is n words or NULL (a non-NULL leader with n not equal to the scene's count is refused): leader[i] is the leader
 *   of i's cell for a candidate and GSR_CELL_NONE otherwise.  hist is cap + 1 words or NULL, cap in 1 .. 4095: hist[k], for
 *   1 <= k <= cap, is the number of cells with k members, hist[cap] means "cap or more", hist[0] is 0.  info may be NULL.  An
 *   empty scene, or an empty scope, returns zeros (rows_after = the scene's count).
 * info: in_scope = the splats in S; candidates = those of them that are candidates; cells = the occupied cells; merged_cells =
 *   the cells with m >= 2; merged_members = the sum of m over those; largest = the largest m; rows_after = n - merged_members +
 *   merged_cells; pair_bound and budget as below.  Every field is an integer, so every field is exact.
 * gsr_scene_merge_cells: a cell with m == 1, and every non-candidate, is left bit for bit.  A cell with m >= 2 is replaced by one
 *   row, written at its leader's index; its other members are removed by the order-preserving compaction gsr_scene_erase_selected
 *   uses.  The consistency guarantee: *new_count == info->rows_after of a gsr_cells call with the same cell, scope and budget.
 * The merged row.  All arithmetic is f64, uncontracted; every sum runs over the members in ascending index order; division and
 *   square root are correctly rounded.
 *    1. a_i = the opacity byte;  v_i = (fabs(sx) * fabs(sy)) * fabs(sz);  m_i = a_i * v_i;  M = sum m_i.
 *    2. If M > 0: w_i = m_i, W = M.  Otherwise w_i = 1, W = (double)m.
 *    3. mu_k = (sum w_i * p_ik) / W; the stored position is (float)mu_k.
 *    4. S_i = the six sums of the covariance R^T diag(s^2) R of member i, from its stored rotation and scale exactly as the packed
 *       covariance words are computed from them, before the factor 4 and the halves.
 *    5. d_i = p_i - mu, mu unrounded;  C_ab = (sum w_i * (S_i,ab + d_ia * d_ib)) / W  for ab = 00, 01, 02, 11, 12, 22.
 *    6. Cyclic Jacobi, exactly 6 sweeps over the pairs (p, q) = (0,1), (0,2), (1,2) on A = C, V = I, r = 3 - p - q.  A pair with
 *       A_pq == 0 is skipped.  th = (A_qq - A_pp) / (2.0 * A_pq);  t = 1.0 / (fabs(th) + sqrt(th * th + 1.0)), negated if th < 0;
 *       cs = 1.0 / sqrt(t * t + 1.0);  sn = t * cs.  From the old values: A_pp = app - t * apq;  A_qq = aqq + t * apq;
 *       A_pq = 0;  A_rp = cs * arp - sn * arq;  A_rq = sn * arp + cs * arq;  for k = 0..2: V_kp = cs * vkp - sn * vkq,
 *       V_kq = sn * vkp + cs * vkq.  lam_k = A_kk, not sorted.
 *    7. The stored scale is (float)sqrt(lam_k > 0 ? lam_k : 0.0).
 *    8. The renderer's covariance is R^T diag(s^2) R with R built from (x, y, z, w) = (r1, r2, r3, -r0), so R = V^T: row k is
 *       eigenvector k.
 *    9. (x, y, z, w) from R by Shepperd's four branches, in this order: tr = (R00 + R11) + R22 > 0: s = sqrt(tr + 1.0) * 2.0,
 *       w = 0.25 * s, x = (R21 - R12) / s, y = (R02 - R20) / s, z = (R10 - R01) / s;  else R00 > R11 && R00 > R22:
 *       s = sqrt(((1.0 + R00) - R11) - R22) * 2.0, w = (R21 - R12) / s, x = 0.25 * s, y = (R01 + R10) / s, z = (R02 + R20) / s;
 *       else R11 > R22: s = sqrt(((1.0 + R11) - R00) - R22) * 2.0, w = (R02 - R20) / s, x = (R01 + R10) / s, y = 0.25 * s,
 *       z = (R12 + R21) / s;  else: s = sqrt(((1.0 + R22) - R00) - R11) * 2.0, w = (R10 - R01) / s, x = (R02 + R20) / s,
 *       y = (R12 + R21) / s, z = 0.25 * s.  The stored rotation is (r0, r1, r2, r3) = ((float)(-w), (float)x, (float)y, (float)z).
 *   10. The covariance words are those of the stored f32 rotation and scale.
 *   11. Each colour byte is floor((sum w_i * c_i) / W + 0.5).
 *   12. Opacity conserves opacity x volume: v' = (s'x * s'y) * s'z from the stored f32 scales as doubles; if v' > 0: o = M / v',
 *       the byte is 255 if o >= 255, else floor(o + 0.5); otherwise the byte is the largest a_i.
 *   13. Data word 3 stays the leader's.
 *   Every value is a sequence of correctly rounded f64 operations in a stated order: the same scene, cell and scope give the same
 *   bits on every run, in every context form and through every member of a shared scene.
 * State.  The edit is a blocking scene replacement, like a removing gsr_scene_erase_selected: it waits for every member of a
 *   shared scene, invalidates the members' frame state, moves the generation and re-plans the bins; the capacity is kept.  The
 *   hidden set is carried through the compaction, a merged row has its leader's bit; the contribution accumulators are treated
 *   exactly as a removing erase treats them; the selection becomes exactly the merged rows, so the overlay shows what was merged.
 *   Nothing to merge: if no cell has two members the call returns GSR_OK with new_count = n and changes nothing; the last frame
 *   stays valid, and so does the selection.  gsr_cells reads the scene and writes none of it; it is ordered like gsr_neighbours.
 * The work budget is the neighbour budget, with the same constants: pair_bound is the sum, over the indexed candidates, of the
 *   population of the candidate's own hash bucket, i.e. the key tests the walk makes.  budget == 0 means
 *   GSR_NEIGHBOUR_DEFAULT_BUDGET; a budget above GSR_NEIGHBOUR_MAX_BUDGET is refused; if pair_bound > budget the call returns
 *   GSR_ERR_ARG with a message naming both numbers, fills info (in_scope, candidates, pair_bound, budget) and launches no walk.
 * Refusals (GSR_ERR_ARG with a message, nothing touched): a NULL ctx; a cell that is not finite, not > 0, or with 1 / cell not
 *   finite and normal; cap outside 1 .. 4095; unknown scope flags; a budget above the maximum; a non-NULL leader with the wrong n;
 *   a scene without rotations / scales; for the edit, a scene with SH rows (sh_count != 0): a mixture's SH colour is not defined
 *   here, while gsr_cells answers for such a scene; a bound above the budget.
 * The device scratch belongs to the context: the scratch of "neighbours", a mask and 12 bytes per splat for the report, 12 more
 *   bytes per splat and three masks for the edit.  The first call allocates it, it only grows, and gsr_destroy frees it; a context
 *   that never calls any of this allocates nothing and launches nothing. */
#define GSR_CELL_NONE 0xffffffffu   /* a leader: the splat is no candidate */
typedef struct gsr_cell_info {
    uint32_t in_scope, candidates;       /* splats in S; of those, mergeable */
    uint32_t cells, merged_cells;        /* occupied cells; cells with >= 2 members */
    uint32_t merged_members, largest;    /* sum of m over merged cells; the largest m */
    uint32_t rows_after, pad;            /* n - merged_members + merged_cells */
    uint64_t pair_bound, budget;
} gsr_cell_info;
int gsr_cells(gsr_ctx *ctx, double cell, uint32_t cap, uint32_t scope, uint64_t budget,
              uint32_t *leader /* n or NULL */, uint32_t n, uint32_t *hist /* cap + 1 or NULL */, gsr_cell_info *info);
int gsr_scene_merge_cells(gsr_ctx *ctx, double cell, uint32_t scope, uint64_t budget,
                          uint32_t *new_count, gsr_cell_info *info);

/* ---- planes ---- the dominant plane fitted on the device, the splats near it selected, the scene aligned to it
 * No interface of the reference stands behind this section either.  The calls above relate splats to each other; these relate
 * them to a shape, and the first shape every capture needs is its floor, table top or wall: a captured scene arrives tilted and
 * shifted, with floaters under the ground.  gsr_fit_plane finds the plane by RANSAC on the device, with no gsr_read_scene;
 * gsr_select_plane picks by signed distance from it ("everything under the floor"); gsr_plane_alignment turns it into the
 * arguments of gsr_scene_rotate and gsr_scene_translate that put it at axis . p = 0.
 * Definition ("Planes").  All arithmetic is f64, in the written order, uncontracted; / and the square root
 *   are correctly rounded.  Scope S is the GSR_SCOPE_SELECTED | GSR_SCOPE_VISIBLE flags of "splat data", with the same meaning; 0
 *   is every splat.  A candidate is a splat in S whose three position floats are finite; the candidates in ascending index are
 *   cand[0 .. m-1], and nonfinite = in_scope - m.  Rotation and scale are not read, so a scene without them is accepted.
 *   Signed distance of a splat at f32 (x, y, z) from the plane (a, b, c, d):
 *     s = ((a*(double)x + b*(double)y) + c*(double)z) + d
 *   The plane is used as given: the two calls that take planes from the host do not normalise them.  A splat is within t of the
 *   plane iff fabs(s) <= t: a distance of exactly t counts.
 *   Hypothesis h of a fit, 0 <= h < H:
 *     mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *             return z ^ (z >> 31)            (uint64, wrapping: the splitmix64 finaliser)
 *     rank(h, j) = mulhi64(mix(seed + 3*h + j), m)   for j = 0, 1, 2     (the high 64 bits of the 128-bit product)
 *     A, B, C = cand[rank(h, 0..2)];  e1 = B - A, e2 = C - A   (component-wise on the doubles)
 *     N = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x);  l2 = (Nx*Nx + Ny*Ny) + Nz*Nz
 *     degenerate if two ranks are equal, if l2 is not finite, or if l2 == 0;  otherwise n = N / sqrt(l2),
 *     negated when nx < 0 || (nx == 0 && (ny < 0 || (ny == 0 && nz < 0))): the first of nx, ny, nz that is not zero is positive
 *     (a -0.0 that this leaves behind is part of the result);  d = -((nx*Ax + ny*Ay) + nz*Az)
 *   score(h) is the number of candidates within threshold of plane h; a degenerate hypothesis scores 0.  The best hypothesis has
 *   the largest score; ties go to the smallest h.  found = 0 iff every hypothesis is degenerate, which covers m < 3; triple,
 *   inliers, best and plane are then zeros.  Scores are integers decided by f64 comparisons, so every result is exact and
 *   independent of the order of arrival.
 * gsr_fit_plane: scores is `hypotheses` words or NULL; info is required.  tests = hypotheses * m.  An empty scene or an empty
 *   scope returns GSR_OK with zeros (and the budget) and found = 0; a scope whose splats are all non-finite has hypotheses =
 *   degenerate = H.
 * gsr_plane_inliers scores up to 4096 planes of the caller's over the candidates: the scoring pass alone.  A host uses it to
 *   check a plane it refined itself.  It fills in_scope, nonfinite, tests and budget of info, and hypotheses = count; info may be
 *   NULL.
 * gsr_select_plane picks P = { i in [0, n) : lo <= s_i && s_i <= hi } over all splats, hidden ones included -- what
 *   gsr_select_attr does, but closed at both ends -- and folds P into the selection with `op` (GSR_SELOP_*) exactly as the
 *   selection calls fold theirs; `selected` means what it means everywhere else.  A non-finite position gives a NaN or infinite
 *   s; NaN is never picked.  lo and hi may be infinite: (-inf, -t) is "everything under the floor".  NaN or lo > hi is refused.
 * The consistency guarantee: after a scope-0 fit with found, gsr_select_plane(info.plane, -threshold, threshold,
 *   GSR_SELOP_REPLACE) selects exactly info.inliers splats; after a fit over GSR_SCOPE_SELECTED with nothing hidden, the same call
 *   with GSR_SELOP_INTERSECT does too.
 * gsr_plane_alignment is a pure function with no context: it runs on a machine without a GPU.  It returns the whole-scene
 *   rotation q (x, y, z, w) and translation t that take the plane to axis . p = 0; the host then calls gsr_scene_rotate(q) and
 *   gsr_scene_translate(t).  The plane and the axis are each normalised by their own length: n, d = plane / |normal|, a = axis /
 *   |axis|.  With c = n . a, when c > -1 + 2^-20: v = n x a and q = (vx, vy, vz, 1 + c) divided by its length.  Otherwise q is a
 *   half turn about n x e, normalised, with e the unit axis of n's smallest component in magnitude (ties go x before y before z)
 *   and w = 0.  t = d * a.
 * The work budget.  hypotheses x candidates is a dense kernel on a shared machine.  Both scoring calls list the candidates
 *   first; if tests > budget the call returns GSR_ERR_ARG with a message naming both numbers; it fills info and launches no scoring
 *   kernel.  budget == 0 means GSR_NEIGHBOUR_DEFAULT_BUDGET; a budget above GSR_NEIGHBOUR_MAX_BUDGET is refused.
 * gsr_fit_plane and gsr_plane_inliers are blocking and stateless, and ordered like gsr_select_attr: they wait for every member's
 *   stream of a shared scene first.  They read the scene and write none of it: no frame state and no selection changes.
 * Refusals (GSR_ERR_ARG with a message, nothing touched, the selection and its count included): a NULL ctx; a threshold that is
 *   not finite or < 0; hypotheses or count outside 1 .. 4096; unknown scope flags or op; a NULL required pointer; a supplied
 *   plane with a non-finite entry or a zero normal; for the alignment, a non-finite entry or a zero plane normal or axis.
 * The device scratch belongs to the context: the candidate list (4 bytes per splat and 4 per 256 splats), 4096 planes, triples
 *   and scores, and an info block.  The first call allocates it, it only grows, and gsr_destroy frees it; a context that never
 *   calls any of this allocates nothing and launches nothing. */
typedef struct gsr_plane_info {
    uint32_t in_scope, nonfinite;        /* candidates = in_scope - nonfinite */
    uint32_t hypotheses, degenerate;
    uint32_t found, best;                /* best: the winning h */
    uint32_t triple[3];                  /* its three splat indices */
    uint32_t inliers;                    /* its score */
    uint64_t tests, budget;              /* tests = hypotheses * candidates */
    double plane[4];                     /* (nx, ny, nz, d), unit normal */
} gsr_plane_info;                        /* 88 bytes; tests at 40, plane at 56 */
#define GSR_PLANE_MAX_HYPOTHESES 4096u
int gsr_fit_plane(gsr_ctx *ctx, double threshold, uint32_t hypotheses, uint64_t seed, uint32_t scope,
                  uint64_t budget, uint32_t *scores /* [hypotheses] or NULL */, gsr_plane_info *info);
int gsr_plane_inliers(gsr_ctx *ctx, const double *planes /* [count][4] */, uint32_t count, double threshold,
                      uint32_t scope, uint64_t budget, uint32_t *inliers /* [count] */, gsr_plane_info *info);
int gsr_select_plane(gsr_ctx *ctx, const double *plane /* [4] */, double lo, double hi, int32_t op, uint32_t *selected);
int gsr_plane_alignment(const double *plane, const double *axis /* [3] */, double *q_xyzw, double *t /* [3] */);

/* ---- matching and registration ---- a scene matched to another one and aligned with it on the device
 * No interface of the reference stands behind this section either.  gsr_scene_append_selected pastes the splats of another
 * context's scene into this one; nothing above can say where they should go.  Two captures of one place come with different
 * origins and orientations.  These calls are the first that relate two scenes: for every splat of this scene, moved by a trial
 * transform, gsr_match finds the nearest splat of another scene.  That answer is data, a picker ("what does the other capture
 * already have", "what changed") and the inner step of a rigid registration (gsr_register) whose result is the same bits on every
 * run -- with no gsr_read_scene and no spatial index or ICP on the host.
 * Definition ("Matching and registration").  All arithmetic is f64, in the written order, uncontracted; / and
 *   the square root are correctly rounded.
 *   Transform.  M is twelve doubles, row-major 3 x 4 (R | t): M[k][c] = M[4*k + c].  NULL is the identity.
 *   Transformed source point of splat i of ctx, at the stored f32 position p as doubles:
 *     T_k = ((M[k][0]*p_x + M[k][1]*p_y) + M[k][2]*p_z) + M[k][3]       k = 0, 1, 2
 *   Scopes.  S (scope) and S' (target_scope) are the GSR_SCOPE_* flags of "splat data"; S is evaluated on ctx's selection and
 *   hidden set, S' on target's.  A target splat is indexed iff it is in S' and its position is finite.  A source splat is a
 *   query iff it is in S, its position is finite and all three T_k are finite; the others in S are `nonfinite` and unmatched.
 *   Match.  For a query i and an indexed target splat j at the stored f32 position q:
 *     e = T_i - (double)q_j;   d2(i,j) = (ex*ex + ey*ey) + ez*ez;   j is a candidate iff d2 <= radius*radius
 *     match_i = the candidate smallest in the pair (d2, j): equal distances go to the smaller target index
 *   An unmatched splat of S has GSR_MATCH_NONE and +inf; a splat outside S has GSR_MATCH_NONE and NaN (0x7ff8000000000000), which
 *   is gsr_knn's convention.  There is no "other" exclusion: with target == ctx (or a member of the same shared scene) and the
 *   identity every finite splat matches the smallest index among the splats coincident with it, with d2 == 0.
 *   The index is that of "neighbours", built over the TARGET's positions and scope, with the same h = radius * (1 + 2^-10), key,
 *   bucket and 27-cell walk; a query's cell coordinate is floor(T_k * inv_h), clamped as a stored position's is.
 *   Sums.  A matched splat contributes the row of 16 doubles
 *     (T_x, T_y, T_z, Q_x, Q_y, Q_z, T_a*Q_b for ab = 00, 01, 02, 10, 11, 12, 20, 21, 22, d2)      Q = (double)q_match
 *   and every other splat sixteen +0.0.  The rows of splats 0 .. n-1 are summed by a fixed tree: groups of 256 consecutive rows, the
 *   last group padded with +0.0; within a group, for s = 128, 64, .., 1: x[l] = x[l] + x[l + s] for l < s; the group results are
 *   reduced the same way until one row is left.  f64 addition is commutative and no NaN can enter, so the tree decides the bits
 *   and no visiting order does.  pairs is the integer count of matched splats.
 * gsr_match: idx is n words and d2 n doubles, or NULL; a non-NULL one with n not equal to ctx's count is refused.  sums and info
 *   may be NULL; the tree runs only when sums are asked for.  An empty source scene or scope, or an empty target (no splat, or
 *   none indexed), returns GSR_OK with everything unmatched and zeros (d2_min +inf, d2_max -inf).
 * info: in_scope and nonfinite count SOURCE splats; target_indexed the index's entries; matched = pairs; pair_bound and budget as
 *   in gsr_neighbour_info; d2_min / d2_max over the matched splats, +inf / -inf with none.  Every field is an integer or a min /
 *   max, so every field is exact.
 * gsr_select_match picks P = { i in S : lo <= v_i && (v_i < hi || hi == +inf) } with v_i = sqrt(d2_i) (+inf when unmatched) and
 *   folds P into ctx's selection with `op` exactly as gsr_select_knn folds its set.  (lo = 0, hi = r) is "what the other capture
 *   already has within r", (lo = r, hi = +inf) "what it lacks".  The consistency guarantee: with GSR_SELOP_REPLACE it selects
 *   exactly the splats whose d2 from gsr_match with the same arguments satisfies the rule.
 * gsr_rigid_solve is a pure function with no context: Horn's closed form on the sums.  It returns D (3 x 4) with D(T) closest to
 *   Q in the least-squares sense over the pairs, and rms (may be NULL).  With n = (double)pairs, inv = 1.0 / n:
 *     mT_a = sum[a] * inv;  mQ_a = sum[3 + a] * inv;  S_ab = sum[6 + 3*a + b] * inv - mT_a * mQ_b       (x, y, z = 0, 1, 2)
 *     N, symmetric 4 x 4 in the order (w, x, y, z):
 *       N00 = (Sxx + Syy) + Szz;  N01 = Syz - Szy;  N02 = Szx - Sxz;  N03 = Sxy - Syx;  N11 = (Sxx - Syy) - Szz;
 *       N12 = Sxy + Syx;  N13 = Szx + Sxz;  N22 = (Syy - Sxx) - Szz;  N23 = Syz + Szy;  N33 = (Szz - Sxx) - Syy
 *     Cyclic Jacobi, exactly 8 sweeps over the pairs (p, q) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) on A = N, V = I, with the
 *     formulas of "merging cells", step 6: a pair with A_pq == 0 is skipped; th = (A_qq - A_pp) / (2.0 * A_pq);
 *     t = 1.0 / (fabs(th) + sqrt(th * th + 1.0)), negated if th < 0;  cs = 1.0 / sqrt(t * t + 1.0);  sn = t * cs.  From the old
 *     values: A_pp = app - t * apq;  A_qq = aqq + t * apq;  A_pq = 0;  for both r other than p, q: A_rp = cs * arp - sn * arq,
 *     A_rq = sn * arp + cs * arq;  for k = 0..3: V_kp = cs * vkp - sn * vkq, V_kq = sn * vkp + cs * vkq.  lam_k = A_kk.
 *     (w, x, y, z) = column k of V for the largest lam_k, ties to the smallest k, divided by sqrt(((w*w + x*x) + y*y) + z*z) and
 *     negated if its first non-zero component is negative.
 *     R00 = 1.0 - 2.0*(y*y + z*z);  R01 = 2.0*(x*y - z*w);  R02 = 2.0*(x*z + y*w);
 *     R10 = 2.0*(x*y + z*w);  R11 = 1.0 - 2.0*(x*x + z*z);  R12 = 2.0*(y*z - x*w);
 *     R20 = 2.0*(x*z - y*w);  R21 = 2.0*(y*z + x*w);  R22 = 1.0 - 2.0*(x*x + y*y)
 *     t_k = mQ_k - ((R_k0*mT_0 + R_k1*mT_1) + R_k2*mT_2);   D = (R | t);   rms = sqrt(sum[15] * inv)
 *   Refused (GSR_ERR_ARG): a NULL pointer, pairs < 3, a non-finite sum.  A degenerate (collinear) set of pairs gives SOME rotation
 *   about the line and is not detected.  tests/register_reference.py restates this order; the result is bit for bit its result.
 * gsr_rigid_compose: out = D o M (apply M, then D): out[k][c] = (D[k][0]*M[0][c] + D[k][1]*M[1][c]) + D[k][2]*M[2][c], plus
 *   D[k][3] for c == 3.  out may be D or M.
 * gsr_rigid_decompose: q (x, y, z, w) from the 3 x 3 part of M by Shepperd's four branches as "merging cells", step 9, states
 *   them, and t = (M[0][3], M[1][3], M[2][3]).  gsr_scene_rotate(q) then gsr_scene_translate(t) applies M to the scene, once.
 * gsr_register runs the loop on the host, from M_0 (NULL: the identity).  Step t matches under M_t and reduces; with pairs < 3 it
 *   stops with GSR_REGISTER_TOO_FEW and M_t; otherwise it solves D_t and sets M_{t+1} = D_t o M_t; when the largest of the twelve
 *   |D_t - (I | 0)| is <= tolerance it stops with GSR_REGISTER_CONVERGED; after max_iterations steps (1 .. 256) it stops with
 *   GSR_REGISTER_MAX_ITERATIONS.  All three return GSR_OK.  info: status; iterations = the steps that ran; pairs and rms of the
 *   last step's match (rms = sqrt(sum[15] * (1.0 / pairs)), +inf with no pair); delta = the last solved step's largest
 *   |D - (I | 0)| (+inf with none).  info is in / out: step_pairs and step_rms are NULL or the caller's arrays of step_rows >=
 *   max_iterations entries, which receive every step's pairs and rms.  M_out (twelve doubles) and info may be NULL.
 *   The scene is never written: a trial transform is iterated, not the stored f32 positions, so positions and packed covariances
 *   do not drift.  The target does not change between the steps, so its index is built once per call.  Rigid only.
 * The work budget is the neighbour budget, with the same constants.  pair_bound is the sum, over the queries, of the populations of
 *   the 27 buckets their walk visits; it is checked before the walk is launched, at every step of gsr_register: if pair_bound >
 *   budget the call returns GSR_ERR_ARG with a message naming both numbers, with info's first fields filled, and launches no walk.
 * gsr_match, gsr_select_match and gsr_register are blocking and stateless.  They wait for every member's stream of both contexts'
 *   shared scenes first.  target must be on ctx's device.  target's scene, selection, hidden set and frame state are not changed;
 *   ctx's scene is read and never written.
 * Refusals (GSR_ERR_ARG with a message, nothing touched, the selection and its count included): a NULL ctx or target; another
 *   device; the radius rules of "neighbours"; unknown scope flags or op; a NaN bound or lo > hi; a wrong n; a non-finite M; a
 *   tolerance that is NaN or negative; iterations outside 1 .. 256; step arrays shorter than max_iterations; a budget above the
 *   maximum; a bound above the budget.
 * The device scratch belongs to ctx: the scratch of "neighbours" sized for the TARGET's count, 4 + 8 bytes per source splat for
 *   idx and d2, and the tree's partial rows (128 bytes per 256 source splats and level) once sums are asked for.  The first call
 *   allocates it, it only grows, and gsr_destroy frees it; a context that never calls any of this allocates nothing and launches
 *   nothing. */
typedef struct gsr_match_info {
    uint32_t in_scope;        /* source splats in S */
    uint32_t nonfinite;       /* of those, no query: a non-finite position or transformed point */
    uint32_t target_indexed;  /* target splats in S' with a finite position */
    uint32_t matched;
    uint64_t pair_bound;      /* pair tests the walk makes at most, as the implementation counts them */
    uint64_t budget;          /* the budget that applied */
    double d2_min;            /* over the matched splats; +inf: there is none */
    double d2_max;            /* over the matched splats; -inf: there is none */
} gsr_match_info;             /* 48 bytes */
typedef struct gsr_match_sums {
    uint64_t pairs;
    double sum[16];
} gsr_match_sums;             /* 136 bytes */
typedef struct gsr_register_info {
    int32_t status;           /* GSR_REGISTER_* */
    uint32_t iterations;
    uint64_t pairs;
    double rms, delta;
    uint64_t *step_pairs;     /* in: NULL, or step_rows entries */
    double *step_rms;         /* in: NULL, or step_rows entries */
    uint32_t step_rows;       /* in */
    uint32_t reserved;
} gsr_register_info;          /* 56 bytes */
#define GSR_MATCH_NONE 0xffffffffu   /* an unmatched splat */
#define GSR_REGISTER_CONVERGED      0
#define GSR_REGISTER_MAX_ITERATIONS 1
#define GSR_REGISTER_TOO_FEW        2
#define GSR_REGISTER_MAX_ITERATIONS_LIMIT 256u
int gsr_match(gsr_ctx *ctx, gsr_ctx *target, const double *M /* [12] or NULL */, double radius, uint32_t scope,
              uint32_t target_scope, uint64_t budget, uint32_t *idx, double *d2, uint32_t n, gsr_match_sums *sums,
              gsr_match_info *info);
int gsr_select_match(gsr_ctx *ctx, gsr_ctx *target, const double *M, double radius, uint32_t scope, uint32_t target_scope,
                     uint64_t budget, double lo, double hi, int32_t op, uint32_t *selected, gsr_match_info *info);
int gsr_register(gsr_ctx *ctx, gsr_ctx *target, const double *M0, double radius, uint32_t scope, uint32_t target_scope,
                 uint64_t budget, uint32_t max_iterations, double tolerance, double *M_out /* [12] */, gsr_register_info *info);
int gsr_rigid_solve(const gsr_match_sums *sums, double *D /* [12] */, double *rms);
int gsr_rigid_compose(const double *D, const double *M, double *out /* [12] */);
int gsr_rigid_decompose(const double *M, double *q_xyzw, double *t /* [3] */);

/* ---- normals ---- per-splat surface normals on the device, and selection by direction or by surface variation
 * No interface of the reference stands behind this section either.  "Select the walls" (|n . up| small), "select what faces the
 * camera", "select edges and corners" (high surface variation) and "select the flat parts" (low variation) all need a normal per
 * splat, and a host would have to read the scene back and build a k-d tree for it.  These calls make the normals on the device
 * from the lists of "k nearest neighbours", or from the splat's own shortest axis with no index at all.
 * Definition ("Normals").  All arithmetic is f64, in the written order, uncontracted; p_i is the stored f32
 *   position widened to f64; sqrt is correctly rounded.
 *   GSR_NORMAL_KNN.  Scope S, near, the list nn_i[0 .. m_i-1] and m_i are exactly gsr_knn's at the same radius and k (ascending by
 *   (d2, index)), with 2 <= k <= GSR_KNN_MAX_K.
 *     1. q_0 = p_i, q_t = p_{nn_i[t-1]} for t = 1 .. m_i; M = m_i + 1 points.
 *     2. mu_c = ((..(q_0c + q_1c) + ..) + q_{m}c) / (double)M.
 *     3. d_t = q_t - mu; C_e = (sum over ascending t of d_tx * d_ty, starting from 0.0) / (double)M for e = 00, 01, 02, 11, 12, 22.
 *     4. (lam, V) by the Jacobi of "merging cells" step 6: six cyclic sweeps over (0,1), (0,2), (1,2), a rotation skipped when
 *        apq == 0.0, t = 1 / (|th| + sqrt(th*th + 1)) with th's sign, cs = 1 / sqrt(t*t + 1), sn = t * cs, in that section's
 *        update order.
 *     5. l_c = lam_c > 0 ? lam_c : 0; tot = (l_0 + l_1) + l_2; c* = the smallest c with l_c minimal.
 *     6. the splat is VALID when it is in S, finite, m_i >= 2 and tot > 0.
 *     7. u = (V[0][c*], V[1][c*], V[2][c*]), not re-normalised (its norm is within 1e-14 of 1).
 *     8. variation = l_{c*} / tot: 0 on a plane, 1/3 at most.
 *   GSR_NORMAL_OWN.  (r0..r3) and (s0, s1, s2) as stored; b[0..8] the rotation matrix of the packed covariance (Quaternion(r1, r2,
 *   r3, -r0), row-major, in its written order: b[0] = 1 - 2*qy*qy - 2*qz*qz, b[1] = 2*qx*qy - 2*qz*qw, ..); the axis of scale k is
 *   (b[3k], b[3k+1], b[3k+2]).
 *     1. l_k = |s_k| * |s_k|; tot and c* as above (a tie goes to the smallest k).
 *     2. a = that axis; nrm = sqrt((a0*a0 + a1*a1) + a2*a2); u_c = a_c / nrm.
 *     3. VALID: in S; position, rotation and scales all finite; the rotation not all zero (a zero quaternion is no rotation,
 *        though the formula alone would give the identity); tot > 0; nrm > 0 and finite.
 *     4. found = 0.  The scene must carry rotations and scales (as the transforms demand).
 *   Orientation, on u in f64, before the store.  If options->oriented: s = ((u0*(toward0 - px) + u1*(toward1 - py)) + u2*(toward2 -
 *   pz)); s < 0 flips u, s > 0 keeps it.  Otherwise (s == 0, s a NaN, or not oriented) the first non-zero component of u is made
 *   positive: gsr_fit_plane's convention.
 *   Stores.  A valid row: normals[3i..] = (float)u, round to nearest; variation[i] = the value; found[i] = m_i.  A row that is not
 *   valid: 0x7fc00000 three times, 0x7ff8000000000000, and found[i] = m_i when i is in S, else 0.
 * gsr_normals: normals is 3 n floats, variation n doubles, found n words; any out pointer may be NULL; a non-NULL one with n not
 *   equal to the scene's count is refused.  info may be NULL.
 * info: in_scope, nonfinite, pair_bound and budget as in gsr_knn_info (OWN: pair_bound 0); valid = the valid rows; variation_min /
 *   variation_max over them, through their bit patterns (the values are non-negative), +inf / -inf when there is none.  An empty
 *   scene or an empty scope returns zeros and +inf / -inf.
 * gsr_select_normal: value_i is computed from the STORED f32 normal widened to f64 -- a host holding gsr_normals' output
 *   reproduces it exactly: GSR_NORMAL_DOT ((nx*ax + ny*ay) + nz*az), GSR_NORMAL_ABS_DOT its fabs, GSR_NORMAL_VARIATION variation_i.
 *   axis is used as given (finite, not all zero, not normalised; NULL for VARIATION).  P = { i valid : lo <= value_i && value_i <=
 *   hi }, both ends closed, infinite ends allowed, as in gsr_select_plane; P is folded with `op` as every picker folds.
 * The consistency guarantee: with GSR_SELOP_REPLACE exactly the splats that satisfy the rule on gsr_normals' outputs for the same
 *   options are selected.
 * The work budget of the KNN source is the neighbour budget: if pair_bound > budget the call returns GSR_ERR_ARG with a message
 *   naming both numbers, fills info's first four fields and launches no walk.
 * Both calls are blocking and stateless, ordered like gsr_knn: they wait for every member's stream of a shared scene, read the
 *   scene and write none of it; no frame state changes.
 * Refusals (GSR_ERR_ARG with a message, nothing touched, the selection and its count included): a NULL ctx or NULL options; an
 *   unknown source, stat, op or scope flag; KNN: gsr_knn's radius rules and k outside 2 .. 32; a non-finite toward when oriented;
 *   a NULL, non-finite or all-zero axis for the two dot stats; a NaN bound or lo > hi; a wrong n; a budget above the maximum; a
 *   bound above the budget; OWN on a scene without rotations and scales.
 * The device scratch belongs to the context: the scratch of "neighbours" (KNN only) and 12 + 8 + 4 bytes per splat.  The first
 *   call allocates it, it only grows, and gsr_destroy frees it; a context that never calls any of this allocates nothing and
 *   launches nothing. */
#define GSR_NORMAL_KNN 0        /* from the k nearest neighbours within radius (PCA of the neighbourhood) */
#define GSR_NORMAL_OWN 1        /* the splat's own shortest axis; no index, no walk */
#define GSR_NORMAL_DOT 0        /* picker value: n . axis */
#define GSR_NORMAL_ABS_DOT 1    /* |n . axis|, for normals that are not oriented */
#define GSR_NORMAL_VARIATION 2  /* l_min / (l_0 + l_1 + l_2) */
typedef struct gsr_normal_options {
    int32_t source;         /* GSR_NORMAL_KNN | GSR_NORMAL_OWN */
    uint32_t k;             /* KNN: 2 .. GSR_KNN_MAX_K; OWN: ignored */
    double radius;          /* KNN: as gsr_knn's; OWN: ignored */
    uint32_t scope;         /* GSR_SCOPE_* flags, as everywhere */
    uint32_t oriented;      /* != 0: toward[] is read */
    uint64_t budget;        /* the neighbour budget, 0 = default */
    double toward[3];       /* a viewpoint: normals are flipped to face it */
} gsr_normal_options;
typedef struct gsr_normal_info {
    uint32_t in_scope;      /* splats in S */
    uint32_t nonfinite;     /* of those, with a NaN or infinite position component */
    uint64_t pair_bound;    /* as gsr_knn_info; OWN: 0 */
    uint64_t budget;        /* the budget that applied */
    uint32_t valid;         /* splats with a normal */
    double variation_min;   /* over the valid; +inf: there is none */
    double variation_max;   /* over the valid; -inf: there is none */
} gsr_normal_info;
int gsr_normals(gsr_ctx *ctx, const gsr_normal_options *options, float *normals /* 3n */, double *variation /* n */,
                uint32_t *found /* n */, uint32_t n, gsr_normal_info *info);       /* any out pointer may be NULL */
int gsr_select_normal(gsr_ctx *ctx, const gsr_normal_options *options, int32_t stat, const double *axis /* 3; NULL for VARIATION */,
                      double lo, double hi, int32_t op, uint32_t *selected, gsr_normal_info *info);

/* ---- point-to-plane registration ---- a scene aligned with another one along the target's normals
 * No interface of the reference stands behind this section either.  gsr_register pulls every source point toward the nearest
 * target SAMPLE; on floors, walls and table tops, sampled at different points in each capture, that slides slowly and stops at a
 * biased pose.  These calls pull every source point toward the target's SURFACE instead: the residual of a pair is its distance
 * along the target splat's normal ("matching and registration" supplies the match, "normals" the normal), and a step is a 6 x 6
 * linear solve.  The working name is "surface", to keep it apart from the planes of gsr_fit_plane.
 * Definition ("Point-to-plane registration").  All arithmetic is f64, in the written order, uncontracted; /
 *   and sqrt are correctly rounded; no sin, cos or atan appears anywhere, so numpy, this library's host code and the device agree
 *   bit for bit (tests/surface_reference.py).
 *   Match.  The match is gsr_match's, unchanged: index, walk, idx, d2, scopes and budget.
 *   Target normals.  What gsr_normals(target, options) stores: the f32 rows, three NaNs where a splat has none.  They are computed
 *   once per call, by the same device path, into the TARGET context's normals scratch, which is allocated or grown exactly as a
 *   gsr_normals call on the target would.  target's scene, selection, hidden set and frame state are not changed.
 *   options->scope must equal target_scope.  GSR_NORMAL_OWN and GSR_NORMAL_KNN are both allowed; KNN has its own radius, k and
 *   budget under the rules of "neighbours".  oriented is taken as given and cannot matter: every product below is unchanged in
 *   every bit when n is negated (but for the sign of a product that is exactly zero, which -0 + +0 = +0 removes from a sum as
 *   soon as one row of its group is empty or padding).
 *   Row of splat i: 29 doubles, non-zero iff i is matched and its match j has a normal (n_x is not a NaN).  T is the transformed
 *   point of "matching and registration", Q = (double)q_j, n = (double)normal_j, e = T - Q;
 *     r = (n_x*e_x + n_y*e_y) + n_z*e_z
 *     c_x = T_y*n_z - T_z*n_y; c_y = T_z*n_x - T_x*n_z; c_z = T_x*n_y - T_y*n_x
 *     J = (c_x, c_y, c_z, n_x, n_y, n_z)
 *     row[0..20] = J_a*J_b for a <= b, row-major (00, 01, .., 05, 11, .., 55)
 *     row[21+a] = J_a*r, row[27] = r*r, row[28] = d2_i.
 *   Every other splat contributes 29 +0.0.
 *   Sums.  The rows of splats 0 .. n-1 are summed by the fixed tree of "matching and registration", per component: groups of 256
 *   rows, s = 128 .. 1, the group results reduced the same way.  pairs counts the matched splats, surface_pairs the non-zero
 *   rows.  A NaN normal never enters a row.  A product may overflow to infinity; the solve refuses that.
 * gsr_surface_solve(sums, D, rms, degenerate) is a pure function with no context.  Let inv = 1.0 / (double)surface_pairs.
 *     1. A is the symmetric 6 x 6 built from sum[0..20]; g_a = -sum[21+a].
 *     2. floor = max_a A_aa * 2^-40.
 *     3. Cholesky, for j = 0..5: v = A_jj, then v = v - L_jk*L_jk for k = 0..j-1 in order.  If !(v > floor): *degenerate = j + 1,
 *        D = (I | 0), *rms is not written, return GSR_OK.  L_jj = sqrt(v).  For i > j: v = A_ij, then v = v - L_ik*L_jk for k
 *        ascending, then L_ij = v / L_jj.
 *     4. Forward substitution, i ascending: y_i = (g_i - L_i0*y_0 - ..) taken left to right, then / L_ii.
 *     5. Back substitution, i = 5..0, with k ascending from i+1: x_i = (y_i - L_ki*x_k ..) / L_ii.
 *     6. (omega, v) = x.
 *     7. The rotation is the Cayley step, which uses only sqrt and division: w = 1.0; (qx, qy, qz) = 0.5 * omega;
 *        len = sqrt(((w*w + qx*qx) + qy*qy) + qz*qz), and all four are divided by len.  R follows from (x, y, z, w) = (qx, qy, qz,
 *        w) by gsr_rigid_solve's nine formulas.
 *     8. D = (R | v).  rms = sqrt(sum[27] * inv) (rms may be NULL).  *degenerate = 0.
 *     9. Refused with GSR_ERR_ARG: a NULL sums, D or degenerate; surface_pairs < 6; a non-finite sum.
 *   A target of one plane, or of two, leaves directions the residuals cannot see: a pivot is then exactly 0.0 and the solve says
 *   so instead of dividing by it.
 * gsr_match_surface is one step as data: the sums of the match under M.  An empty scene gives zeros, as gsr_match does; gsr_match
 *   with the same arguments gives idx and d2 for a host that wants them.  sums and info may be NULL.
 * gsr_register_surface runs gsr_register's loop.  The target's index and the target's normals are built once per call; the bound
 *   is checked at every step.  Step t matches under M_t and reduces; surface_pairs < 6 ends the loop with GSR_REGISTER_TOO_FEW and
 *   M_t; a degenerate solve ends it with GSR_REGISTER_DEGENERATE and M_t; otherwise M_{t+1} = D_t o M_t by gsr_rigid_compose.
 *   delta, tolerance and max_iterations work as in gsr_register.  All four endings return GSR_OK.  info: status; iterations; the
 *   last step's pairs and surface_pairs; rms = sqrt(sum[28] * (1.0 / pairs)) (+inf with no pair: the point distances of the
 *   non-zero rows over the matched splats); surface_rms = sqrt(sum[27] * (1.0 / surface_pairs)) (+inf with none); delta; valid =
 *   the target splats with a normal.  info is in / out: the four step arrays are NULL or the caller's, of step_rows >=
 *   max_iterations entries.  The scene is never written.
 * Refusals (GSR_ERR_ARG with a message, nothing touched): those of gsr_register and of gsr_normals (OWN on a target without
 *   rotations and scales included; a message about the target's side is ctx's last error); NULL options; options->scope not equal
 *   to target_scope.
 * Both calls are blocking and stateless, ordered like gsr_register.  target == ctx and members of one shared scene are allowed.
 * The device scratch: ctx's scratch of "matching and registration", with 29-wide partial rows (232 bytes per 256 source splats and
 *   level) of their own; target's scratch of "normals" (and of "neighbours" for KNN). */
typedef struct gsr_surface_sums {
    uint64_t pairs;           /* matched splats */
    uint64_t surface_pairs;   /* of those, with a normal at the match: the non-zero rows */
    double sum[29];
} gsr_surface_sums;           /* 248 bytes */
typedef struct gsr_register_surface_info {
    int32_t status;           /* GSR_REGISTER_* */
    uint32_t iterations;
    uint64_t pairs;
    uint64_t surface_pairs;
    double rms, surface_rms, delta;
    uint32_t valid;           /* target splats with a normal */
    uint32_t step_rows;       /* in */
    uint64_t *step_pairs;     /* in: NULL, or step_rows entries */
    uint64_t *step_surface_pairs;
    double *step_rms;
    double *step_surface_rms;
} gsr_register_surface_info;  /* 88 bytes */
#define GSR_REGISTER_DEGENERATE 3
int gsr_match_surface(gsr_ctx *ctx, gsr_ctx *target, const double *M /* [12] or NULL */, double radius, uint32_t scope,
                      uint32_t target_scope, uint64_t budget, const gsr_normal_options *options, gsr_surface_sums *sums,
                      gsr_match_info *info);
int gsr_surface_solve(const gsr_surface_sums *sums, double *D /* [12] */, double *rms, int32_t *degenerate);
int gsr_register_surface(gsr_ctx *ctx, gsr_ctx *target, const double *M0, double radius, uint32_t scope, uint32_t target_scope,
                         uint64_t budget, const gsr_normal_options *options, uint32_t max_iterations, double tolerance,
                         double *M_out /* [12] */, gsr_register_surface_info *info);

/* ---- selection overlay ---- the selected splats tinted, in read-backs and in delivered frames
 * No interface of the reference stands behind this section either.  gsr_read_selection returns bits; this shows them: a second
 * image beside the frame in which the selected splats carry a tint, and per pixel how much of it they are.
 * Definition ("Selection overlay").  For the last rendered frame, a pixel's fragments, their weight B and the
 * transmittance T are exactly those of "depth and pick": the entries of the pixel's bin list, in list order, that pass q <= 4, with
 * no early termination, no saturation skip and no segments.  A splat's colour c = (cr, cg, cb) is the compositor's:
 * (float)byte * (1.0f / 255.0f) of the record's colour bytes, or the frame's evaluated SH colour for an SH-coloured splat.  From
 * T = 1, S = 0, C = (0, 0, 0), in f32:  w = T * B; T = T - w; and if the splat is selected: S = S + w; Cr = fma(w, cr, Cr), Cg and
 * Cb likewise.  Two results, both W x H with row 0 at the top:
 *   cover, float: S, the share of the pixel's alpha that selected splats supply (gsr_set_overlay_outline draws the selection's edge from it).
 *   overlay, float4, premultiplied like the framebuffer: with fb the frame's framebuffer value at the pixel,
 *     out.r = fma(mix, fma(tint[0], S, -Cr), fb.r), g and b likewise; out.a = fb.a.  This is the frame rendered with every selected
 *     splat's colour replaced by lerp(c, tint, mix).  mix == 0, or a pixel with no selected fragment, gives fb bit for bit.
 *     Nothing is clamped here; the RGBA8 and Y'CbCr conversions clamp as they always do.
 * A band context defines both on its own bin columns; elsewhere cover is 0 and overlay is whatever the framebuffer holds.  The pass
 * reads the framebuffer and never writes it: the frame, its statistics, the depth planes and their validity are not touched.
 * gsr_set_overlay supplies the options and allocates the two images (20 bytes per pixel, the context's: gsr_scene_sharing's
 *   scene_bytes does not change); it makes no host wait beyond what allocating needs.  tint and mix must be finite, mix in [0, 1],
 *   reserved 0, else GSR_ERR_ARG and nothing changes.  NULL: off, the buffers are freed.
 * gsr_overlay_async enqueues the pass behind the last enqueued frame on the context's stream: no host wait.  It needs of the frame
 *   exactly what gsr_depth_async needs, otherwise GSR_ERR_ARG and nothing is enqueued; GSR_ERR_ARG also without options.  A scene
 *   never selected in has the empty selection: no mask is allocated, cover is 0 and overlay equals the framebuffer.  A frame whose
 *   lists did not fit is not walked (the pass reads the frame's overflow word on the device) and nothing of it is ever returned as data.
 * gsr_read_overlay and gsr_read_overlay_rgba8 are blocking: they settle the frame as gsr_read_depth does (one that did not fit is
 *   rendered again), run the pass if the image is not the one of this frame, this selection and these options, refuse an invalid pass
 *   with GSR_ERR_OVERFLOW, then copy.  rgba: w * h * 4 floats; cover: w * h floats; either may be NULL.  _rgba8: the overlay through
 *   the framebuffer's RGBA8 rule, round(clamp(x, 0, 1) * 255), w * h * 4 bytes (its first call allocates 4 more bytes per pixel).
 * gsr_overlay_device_ptr: plane 0 the overlay (float4[h][w]), 1 cover (float[h][w]); NULL before gsr_set_overlay.
 * gsr_delivery_set_overlay(ctx, 1) on an open ring: gsr_deliver_frame_async enqueues the pass behind the frame and converts the
 *   overlay image in place of the framebuffer, RGBA8 or Y'CbCr alike; serials, GSR_ERR_BUSY, the overflow refusal, resize and close
 *   behave as before, and a depth ring's plane is still the frame's.  It needs options (GSR_ERR_ARG without) and an open ring.  On
 *   a context in a group it returns GSR_ERR_ARG: the gathered frame is RGBA8 of other ranks, which nothing here can tint.  Off --
 *   the default, and the state of every newly opened ring -- the ring does byte for byte what it does without this call.
 * Shared scenes: the selection belongs to the scene, the images to the context, and passes run on each member's stream.  A context
 * notes that it has a pass in flight (gsr_sync clears the note); every call that changes the selection first waits for the streams
 * of the members with such a note, so a pass already enqueued never sees the change and every later one does.  A changed selection,
 * changed options, a new frame, gsr_scene_limit_box, an erase and gsr_set_scene* make the image stale: the next read runs the pass
 * again (or, without a valid frame, returns GSR_ERR_ARG).  A context that never calls any of this allocates nothing and launches nothing. */
typedef struct gsr_overlay_options {
    float tint[3];        /* the colour selected splats are drawn towards, as the framebuffer's channels (not clamped) */
    float mix;            /* 0: the frame as it is; 1: the tint alone; in [0, 1] */
    int32_t reserved[4];  /* 0 */
} gsr_overlay_options;
int gsr_set_overlay(gsr_ctx *ctx, const gsr_overlay_options *options);   /* NULL: off, buffers freed */
int gsr_overlay_async(gsr_ctx *ctx);
int gsr_read_overlay(gsr_ctx *ctx, float *rgba /* w*h*4 */, float *cover /* w*h */);   /* either NULL; blocking */
int gsr_read_overlay_rgba8(gsr_ctx *ctx, uint8_t *out);
void *gsr_overlay_device_ptr(gsr_ctx *ctx, int32_t plane);   /* 0 overlay, 1 cover */
int gsr_delivery_set_overlay(gsr_ctx *ctx, int32_t on);

/* ---- selection outline ---- the overlay draws the edge of the selection
 * An editor shows a selection by its outline.  With outline options set, every overlay pass is followed by a step that draws the
 * edge of the selected region into the overlay image, so everything that consumes that image -- gsr_read_overlay,
 * gsr_read_overlay_rgba8, gsr_overlay_device_ptr(ctx, 0) and a ring switched with gsr_delivery_set_overlay, RGBA8 and Y'CbCr
 * alike -- gets the outlined image with no further change.  cover is never changed.
 * Definition ("Selection overlay").  The domain is the pixels the pass defines: the whole image, or for a band
 * context the pixels of its own bin columns that lie inside the image.  For p in the domain, inside(p) = (cover[p] >= threshold),
 * an f32 compare: a NaN is not inside.  Pixels outside the domain are neither inside nor outside: the neighbourhood ignores them
 * and they are never written.  With r = width, in integers:
 *   side GSR_OUTLINE_OUTER: edge(p) = !inside(p) and there is a q in the domain with inside(q) and (qx-px)^2 + (qy-py)^2 <= r*r;
 *   side GSR_OUTLINE_INNER: the same with inside and !inside exchanged.
 * With ov the overlay value the pass produced, where edge(p), in f32:  k = 1.0f - alpha;  out.c = fma(ov.c, k, rgb[c] * alpha) for
 * c = r, g, b;  out.a = fma(ov.a, k, alpha).  Everywhere else out = ov bit for bit.  Nothing is clamped here.
 * A pass whose frame did not fit draws nothing.  A scene never selected in has an empty outline on either side.
 * gsr_set_overlay_outline needs overlay options (gsr_set_overlay first); rgb must be finite, alpha in [0, 1], threshold finite
 *   and > 0, width in 1 .. 16, side GSR_OUTLINE_OUTER or GSR_OUTLINE_INNER, reserved 0, else GSR_ERR_ARG and nothing changes.
 *   NULL: off (always accepted); like gsr_set_overlay(ctx, NULL) it waits for the context's stream when it frees the bit plane.
 *   Setting options makes no host wait; one bit per pixel is allocated by the first pass that draws (and again when the image
 *   grows, where freeing the smaller plane waits for what still reads it).
 *   Changed outline options make the image stale exactly as changed overlay options do; equal options do not.
 *   gsr_set_overlay(ctx, NULL) clears the outline too.  Off -- the default -- the overlay is bit for bit and launch for launch
 *   what it is without this call. */
#define GSR_OUTLINE_OUTER 0
#define GSR_OUTLINE_INNER 1
typedef struct gsr_outline_options {
    float rgb[3];         /* the outline's colour, as the framebuffer's channels (not clamped) */
    float alpha;          /* how much of the pixel the outline replaces; in [0, 1] */
    float threshold;      /* a pixel is inside the selection where cover >= threshold; finite, > 0 */
    int32_t width;        /* the outline's width in pixels: the radius of the disc; 1 .. 16 */
    int32_t side;         /* GSR_OUTLINE_OUTER: on the pixels around the selection; GSR_OUTLINE_INNER: on its own border pixels */
    int32_t reserved[5];  /* 0 */
} gsr_outline_options;
int gsr_set_overlay_outline(gsr_ctx *ctx, const gsr_outline_options *options);   /* NULL: off */

/* ---- device interop (torch / RCCL plumbing in the harness) ---- */
void *gsr_framebuffer_device_ptr(gsr_ctx *ctx); /* float4[h][w] on the device */
void *gsr_stream_handle(gsr_ctx *ctx);          /* hipStream_t */
/* Device-side ordering between the context's stream and another stream of the same device (no host wait):
 * ctx_waits = 0: work submitted to `other_stream` after this call waits for everything enqueued on the context so far;
 * ctx_waits = 1: the context's later work waits for everything enqueued on `other_stream` so far. */
int gsr_stream_order(gsr_ctx *ctx, void *other_stream, int32_t ctx_waits);
int gsr_device_info(gsr_ctx *ctx, char *name, int32_t name_len, int32_t *compute_units, int32_t *clock_khz);
/* Hash of the kernel sources this library was built from (hex string; "unknown" for an ad-hoc build): profiler
 * measurements are stamped with it so that they are never attributed to a different build. */
const char *gsr_build_id(void);

/* ---- drop-in for the wasm export, same argument list as wasm/wasm.cpp:8-13.
 * Host pointers; depthBuffer/starts/counts may be NULL (depthBuffer, when given,
 * receives the 17-bit keys like the reference leaves them).  Uses a process-wide
 * context on device 0; returns nothing, like the reference.  The positions are copied
 * to the device on every call (nothing of the caller's is remembered between calls:
 * Worker.ts:23-27 re-copies them on every scene message, and JS hosts edit them in place);
 * on failure depthIndex is zero-filled and the reason is printed to stderr. */
void gsplat_sort_host(const float *viewProj, uint32_t vertexCount, const float *fBuffer, uint32_t *depthBuffer,
                      uint32_t *depthIndex, uint32_t *starts, uint32_t *counts);

#ifdef __cplusplus
}
#endif
#endif
