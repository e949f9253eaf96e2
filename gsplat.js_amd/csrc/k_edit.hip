// Editing the selection ("Editing the selection"): what Scene.translate / rotate / scale (src/core/Scene.ts:182-305)
// would leave in a Scene that held only the selected splats, written into the selected splats' entries of the SoA scene and into
// nothing else; their colour words; and the box of their centres.  The arithmetic is k_scene.hip's: f64 in the reference's order,
// f32 wherever the reference stores into a Float32Array, pack_cov for the covariance words, -ffp-contract=off.
// One thread per splat.  The selection word words[i >> 5] is the same over each half of a wave64, so a wave whose two words are
// zero has no lane left behind the test and ends before it loads anything of the scene: a sparse selection costs the mask's
// n / 8 bytes, not a pass over the scene.
#include "gsr_internal.h"
#include "k_pack_cov.h"
#include "k_splat_ops.h"

#include <algorithm>

namespace gsr {

GSR_BOUNDS_DECL(edit)   // sites: 0 selection word, 1 splat index, 2 partial slot.  Sites 0 and 2 compare an index with an extent the
                        // host passes beside it (nwords, nparts) and can count when the two disagree; site 1 stands behind the
                        // `i < n` guard of the same n, so it counts only if that guard is ever lost: it proves nothing today

constexpr int EDIT_THREADS = 256;
constexpr int BOUNDS_THREADS = 256;
constexpr uint32_t BOUNDS_MAX_BLOCKS = 1024;   // partials of k_edit_bounds: a grid-stride fold beyond that many workgroups

// is splat i selected?  (i >= n: no, whatever the tail bits say)
__device__ __forceinline__ bool edit_selected(const uint32_t* __restrict__ words, uint32_t nwords, uint32_t n, uint32_t i)
{
    if (i >= n) return false;
    GSR_BOUND(edit, 0, i >> 5, nwords);
    GSR_BOUND(edit, 1, i, n);
    return set_bit(words, nwords, i);
}

// Scene.translate / rotate / scale (Scene.ts:182-305) on the selected splats: k_splat_ops.h's arithmetic behind the selection test
__global__ __launch_bounds__(EDIT_THREADS) void k_edit_translate(uint32_t n, SceneDev sc, const uint32_t* __restrict__ words, uint32_t nwords,
                                                                 double tx, double ty, double tz)
{
    const uint32_t i = blockIdx.x * EDIT_THREADS + threadIdx.x;
    if (edit_selected(words, nwords, n, i)) splat_translate(sc, i, tx, ty, tz);
}

// q = (x, y, z, w); PIVOT, m = -pivot and p = pivot as SplatPivot has them
template <bool PIVOT>
__global__ __launch_bounds__(EDIT_THREADS) void k_edit_rotate(uint32_t n, SceneDev sc, const uint32_t* __restrict__ words, uint32_t nwords,
                                                              double x, double y, double z, double w, double mx, double my, double mz,
                                                              double px_, double py_, double pz_)
{
    const uint32_t i = blockIdx.x * EDIT_THREADS + threadIdx.x;
    if (edit_selected(words, nwords, n, i)) splat_rotate<PIVOT>(sc, i, x, y, z, w, SplatPivot{mx, my, mz, px_, py_, pz_});
}

template <bool PIVOT>
__global__ __launch_bounds__(EDIT_THREADS) void k_edit_scale(uint32_t n, SceneDev sc, const uint32_t* __restrict__ words, uint32_t nwords,
                                                             double sx, double sy, double sz, double mx, double my, double mz,
                                                             double px_, double py_, double pz_)
{
    const uint32_t i = blockIdx.x * EDIT_THREADS + threadIdx.x;
    if (edit_selected(words, nwords, n, i)) splat_scale<PIVOT>(sc, i, sx, sy, sz, SplatPivot{mx, my, mz, px_, py_, pz_});
}

// rgba[i] = (rgba[i] & ~byte_mask) | (value & byte_mask) on the selected splats (value arrives masked)
__global__ __launch_bounds__(EDIT_THREADS) void k_edit_rgba(uint32_t n, SceneDev sc, const uint32_t* __restrict__ words, uint32_t nwords,
                                                            uint32_t value, uint32_t byte_mask)
{
    const uint32_t i = blockIdx.x * EDIT_THREADS + threadIdx.x;
    if (!edit_selected(words, nwords, n, i)) return;
    sc.rgba[i] = (sc.rgba[i] & ~byte_mask) | value;
}

// ---- the selected splats' count and the box of their centres ----
// A partial is EDIT_PARTIAL_WORDS words: count, min x y z, max x y z (f32 bits), one pad.  A value enters min only through
// `v < min` and max only through `v > max`, in the fold of a thread, across lanes, across waves and across partials alike: a NaN
// is counted and never enters the box, and nothing selected leaves (+inf, -inf).
struct EditBox { uint32_t count; float mn[3], mx[3]; };

__device__ __forceinline__ void box_take(EditBox& b, uint32_t count, const float* mn, const float* mx)
{
    b.count += count;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (mn[k] < b.mn[k]) b.mn[k] = mn[k];
        if (mx[k] > b.mx[k]) b.mx[k] = mx[k];
    }
}

// every thread's box -> the workgroup's, valid in thread 0; s_box: one EditBox per wave
__device__ __forceinline__ void box_reduce(EditBox& b, EditBox* s_box)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t oc = __shfl_xor(b.count, d);
        float omn[3], omx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { omn[k] = __shfl_xor(b.mn[k], d); omx[k] = __shfl_xor(b.mx[k], d); }
        box_take(b, oc, omn, omx);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_box[wave] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < BOUNDS_THREADS / WAVE; w++) box_take(b, s_box[w].count, s_box[w].mn, s_box[w].mx);
}

__device__ __forceinline__ void box_store(const EditBox& b, uint32_t* __restrict__ out)
{
    out[0] = b.count;
#pragma unroll
    for (int k = 0; k < 3; k++) { out[1 + k] = __float_as_uint(b.mn[k]); out[4 + k] = __float_as_uint(b.mx[k]); }
    out[7] = 0u;
}

__device__ __forceinline__ EditBox box_empty()
{
    EditBox b;
    b.count = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) { b.mn[k] = __builtin_inff(); b.mx[k] = -__builtin_inff(); }
    return b;
}

// each thread folds its splats (grid-stride) and counts its words with __popc; one partial per workgroup
__global__ __launch_bounds__(BOUNDS_THREADS) void k_edit_bounds(uint32_t n, const float* __restrict__ px, const float* __restrict__ py,
                                                                const float* __restrict__ pz, const uint32_t* __restrict__ words, uint32_t nwords,
                                                                uint32_t* __restrict__ partial, uint32_t nparts)
{
    __shared__ EditBox s_box[BOUNDS_THREADS / WAVE];
    EditBox b = box_empty();
    const uint32_t t = blockIdx.x * BOUNDS_THREADS + threadIdx.x, stride = gridDim.x * BOUNDS_THREADS;
    const uint32_t live = (n + 31u) >> 5;   // words that hold a splat
    for (uint32_t wi = t; wi < live; wi += stride) {
        GSR_BOUND(edit, 0, wi, nwords);
        b.count += (uint32_t)__popc(set_word(words, nwords, n, wi));
    }
    for (uint32_t i = t; i < n; i += stride) {   // (i + stride wraps only for n > 2^32 - stride: gsr_set_scene* refuses far less)
        if (!edit_selected(words, nwords, n, i)) continue;
        const float v[3] = {px[i], py[i], pz[i]};
        box_take(b, 0u, v, v);
    }
    box_reduce(b, s_box);
    if (threadIdx.x != 0) return;
    GSR_BOUND(edit, 2, blockIdx.x, nparts);
    if (blockIdx.x < nparts) box_store(b, partial + (size_t)blockIdx.x * EDIT_PARTIAL_WORDS);
}

// one workgroup: the partials -> out (EDIT_PARTIAL_WORDS words)
__global__ __launch_bounds__(BOUNDS_THREADS) void k_edit_bounds_fold(const uint32_t* __restrict__ partial, uint32_t nparts, uint32_t* __restrict__ out)
{
    __shared__ EditBox s_box[BOUNDS_THREADS / WAVE];
    EditBox b = box_empty();
    for (uint32_t p = threadIdx.x; p < nparts; p += BOUNDS_THREADS) {
        GSR_BOUND(edit, 2, p, nparts);
        const uint32_t* w = partial + (size_t)p * EDIT_PARTIAL_WORDS;
        const float mn[3] = {__uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3])};
        const float mx[3] = {__uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6])};
        box_take(b, w[0], mn, mx);
    }
    box_reduce(b, s_box);
    if (threadIdx.x == 0) box_store(b, out);
}

// ---- launchers ----
namespace {
dim3 edit_grid(uint32_t n) { return dim3((n + EDIT_THREADS - 1) / EDIT_THREADS); }
}  // namespace

void launch_edit_translate(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, const double* t, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_edit_translate, edit_grid(n), dim3(EDIT_THREADS), 0, s, n, sc, words, nwords, t[0], t[1], t[2]);
}

void launch_edit_rotate(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, const double* q, const double* pivot, hipStream_t s)
{
    if (!n) return;
    if (pivot)
        hipLaunchKernelGGL(k_edit_rotate<true>, edit_grid(n), dim3(EDIT_THREADS), 0, s, n, sc, words, nwords, q[0], q[1], q[2], q[3],
                           -pivot[0], -pivot[1], -pivot[2], pivot[0], pivot[1], pivot[2]);
    else
        hipLaunchKernelGGL(k_edit_rotate<false>, edit_grid(n), dim3(EDIT_THREADS), 0, s, n, sc, words, nwords, q[0], q[1], q[2], q[3], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
}

void launch_edit_scale(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, const double* sv, const double* pivot, hipStream_t s)
{
    if (!n) return;
    if (pivot)
        hipLaunchKernelGGL(k_edit_scale<true>, edit_grid(n), dim3(EDIT_THREADS), 0, s, n, sc, words, nwords, sv[0], sv[1], sv[2],
                           -pivot[0], -pivot[1], -pivot[2], pivot[0], pivot[1], pivot[2]);
    else
        hipLaunchKernelGGL(k_edit_scale<false>, edit_grid(n), dim3(EDIT_THREADS), 0, s, n, sc, words, nwords, sv[0], sv[1], sv[2], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
}

void launch_edit_rgba(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, uint32_t rgba, uint32_t byte_mask, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_edit_rgba, edit_grid(n), dim3(EDIT_THREADS), 0, s, n, sc, words, nwords, rgba & byte_mask, byte_mask);
}

uint32_t edit_bounds_blocks(uint32_t n)
{
    return std::min<uint32_t>(std::max<uint32_t>((n + BOUNDS_THREADS - 1) / BOUNDS_THREADS, 1u), BOUNDS_MAX_BLOCKS);
}

void launch_edit_bounds(uint32_t n, const float* px, const float* py, const float* pz, const uint32_t* words, uint32_t nwords, uint32_t* partial,
                        uint32_t* out, hipStream_t s)
{
    const uint32_t blocks = edit_bounds_blocks(n);
    hipLaunchKernelGGL(k_edit_bounds, dim3(blocks), dim3(BOUNDS_THREADS), 0, s, n, px, py, pz, words, nwords, partial, blocks);
    hipLaunchKernelGGL(k_edit_bounds_fold, dim3(1), dim3(BOUNDS_THREADS), 0, s, (const uint32_t*)partial, blocks, out);
}

}  // namespace gsr
