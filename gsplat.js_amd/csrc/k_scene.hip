// On-device scene build and transforms: what Scene.setData / translate / rotate / scale /
// limitBox do in JavaScript loops (src/core/Scene.ts:126-366), as kernels over the SoA scene.  The arithmetic is
// f64 in the reference's order of operations with f32 stores where the reference stores into Float32Arrays, and the
// file is compiled with -ffp-contract=off, so every word matches the JavaScript result bit for bit.
#include "gsr_internal.h"
#include "k_pack_cov.h"
#include "k_splat_ops.h"

#include <algorithm>

namespace gsr {

// Scene.setData (Scene.ts:126-177): one 32-byte .splat row per thread
__global__ __launch_bounds__(256) void k_build_scene(const uint4* __restrict__ rows, uint32_t n, SceneDev sc)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 a = rows[2 * (size_t)i], b = rows[2 * (size_t)i + 1];  // pos xyz, scale x | scale yz, rgba, rot
    sc.px[i] = __uint_as_float(a.x); sc.py[i] = __uint_as_float(a.y); sc.pz[i] = __uint_as_float(a.z);
    const float4 scl = make_float4(__uint_as_float(a.w), __uint_as_float(b.x), __uint_as_float(b.y), 0.f);
    const uint32_t rb = b.w;
    const float4 rot = make_float4((float)(((double)(rb & 0xffu) - 128) / 128), (float)(((double)((rb >> 8) & 0xffu) - 128) / 128),
                                   (float)(((double)((rb >> 16) & 0xffu) - 128) / 128), (float)(((double)(rb >> 24) - 128) / 128));
    sc.rgba[i] = b.z;
    sc.rot[i] = rot;
    sc.scl[i] = scl;
    uint32_t c0, c1, c2;
    pack_cov(rot, scl, c0, c1, c2);
    sc.cov0[i] = c0; sc.cov1[i] = c1; sc.cov2[i] = c2;
}

// Scene.translate / rotate / scale (Scene.ts:182-305) on every splat: k_splat_ops.h's arithmetic, no pivot
__global__ __launch_bounds__(256) void k_scene_translate(uint32_t n, SceneDev sc, double tx, double ty, double tz)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) splat_translate(sc, i, tx, ty, tz);
}

__global__ __launch_bounds__(256) void k_scene_rotate(uint32_t n, SceneDev sc, double x, double y, double z, double w)   // q = (x, y, z, w)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) splat_rotate<false>(sc, i, x, y, z, w, SplatPivot{});
}

__global__ __launch_bounds__(256) void k_scene_scale(uint32_t n, SceneDev sc, double sx, double sy, double sz)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) splat_scale<false>(sc, i, sx, sy, sz, SplatPivot{});
}

// ---- Scene.limitBox (Scene.ts:307-366): order-preserving compaction ----
constexpr int BOX_THREADS = 1024;

__device__ __forceinline__ bool in_box(const SceneDev& sc, uint32_t i, const double* box)
{
    const double x = sc.px[i], y = sc.py[i], z = sc.pz[i];
    return x >= box[0] && x <= box[1] && y >= box[2] && y <= box[3] && z >= box[4] && z <= box[5];
}

// The compaction's predicate, "splat i stays": the kernels below are templates over it.  Box: limitBox's six comparisons;
// MaskKeep: one bit per splat of a selection of nwords words (k_splat_ops.h's set layout), the splats whose bit equals `keep` stay
// (gsr_scene_erase_selected).  Both are called for i < n only.
struct Box {
    double v[6];
    __device__ __forceinline__ bool operator()(const SceneDev& sc, uint32_t i) const { return in_box(sc, i, v); }
};
struct MaskKeep {
    const uint32_t* words; uint32_t nwords, keep;
    __device__ __forceinline__ bool operator()(const SceneDev&, uint32_t i) const { return (set_bit(words, nwords, i) ? 1u : 0u) == keep; }
};

// The compaction's prologue.  wave_counts: the wave's ballot of `keep`, its popcount into s_w[wave], and THE barrier (every thread calls
// it).  compact_slot, on top of it: the wave's first output index (the workgroup's offset + the earlier waves' counts) and the lane's.
struct CompactSlot { uint32_t off, o; };

__device__ __forceinline__ uint64_t wave_counts(bool keep, uint32_t* s_w)
{
    const uint64_t m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    return m;
}

__device__ __forceinline__ CompactSlot compact_slot(bool keep, const uint32_t* __restrict__ block_off, uint32_t* s_w)
{
    const uint64_t m = wave_counts(keep, s_w);
    CompactSlot c;
    c.off = block_off[blockIdx.x];
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) c.off += s_w[w];
    c.o = c.off + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    return c;
}

template <class Pred>
__global__ __launch_bounds__(BOX_THREADS) void k_box_count(uint32_t n, SceneDev sc, Pred box, uint32_t* __restrict__ block_count)
{
    __shared__ uint32_t s_w[BOX_THREADS / WAVE];
    const uint32_t i = blockIdx.x * BOX_THREADS + threadIdx.x;
    wave_counts(i < n && box(sc, i), s_w);
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < BOX_THREADS / WAVE; w++) t += s_w[w];
        block_count[blockIdx.x] = t;
    }
}

// one workgroup: block_count -> exclusive offsets in place, total to *total
__global__ __launch_bounds__(BOX_THREADS) void k_box_scan(uint32_t* __restrict__ block_count, uint32_t nblocks, uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_part[BOX_THREADS];
    const uint32_t per = (nblocks + BOX_THREADS - 1) / BOX_THREADS;
    const uint32_t b0 = threadIdx.x * per, b1 = min(b0 + per, nblocks);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += block_count[b];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int t = 0; t < BOX_THREADS; t++) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    uint32_t run = s_part[threadIdx.x];
    for (uint32_t b = b0; b < b1; b++) { const uint32_t v = block_count[b]; block_count[b] = run; run += v; }
}

template <class Pred>
__global__ __launch_bounds__(BOX_THREADS) void k_box_compact(uint32_t n, SceneDev src, SceneDev dst, Pred box,
                                                             const uint32_t* __restrict__ block_off)
{
    __shared__ uint32_t s_w[BOX_THREADS / WAVE];
    const uint32_t i = blockIdx.x * BOX_THREADS + threadIdx.x;
    const bool keep = i < n && box(src, i);
    const CompactSlot c = compact_slot(keep, block_off, s_w);
    if (keep) copy_splat_row(dst, c.o, src, i);
}

// ---- limitBox on a scene whose SH colour follows it (gsr_set_sh_follow): the SH textures are compacted with the scene ----
GSR_BOUNDS_DECL(scene_sh)   // sites: 0 source splat of k_box_thresholds, 1 SH row read by k_box_compact_sh, 2 SH row it stores

GSR_BOUNDS_DECL(scene)   // sites: 0 word of Scene.scales read by k_scene_import, 1 its LDS cell, 2 float4 it stores,
                         //        3 row of Scene.data stored by k_scene_export, 4 its LDS cell, 5 word of positions / scales it stores,
                         //        6 word of the bit set k_box_compact_bits reads, 7 word it stores

// k_box_compact's mask and offsets once more, for a one-bit-per-splat set that has to keep naming the same splats (the hidden set,
// DESIGN.md section 4 "Hidden splats"): out[new index of i] = in[i] for every kept i, in order, into a ZEROED `out` of nwords_out
// words.  A wave's kept lanes take the consecutive new indices [off, off + popcount): at most 64 bits from bit off & 31 of word
// off >> 5 on, so at most three words.  Every lane places its bit in the word of the three it falls into, an OR across the wave
// assembles them, and lane 0 ORs the non-zero ones into `out` (atomically: the run's edge words are shared with the waves
// before and behind; bits of different waves never coincide).
template <class Pred>
__global__ __launch_bounds__(BOX_THREADS) void k_box_compact_bits(uint32_t n, SceneDev src, Pred box, const uint32_t* __restrict__ block_off,
                                                                  const uint32_t* __restrict__ in, uint32_t nwords_in,
                                                                  uint32_t* __restrict__ out, uint32_t nwords_out)
{
    __shared__ uint32_t s_w[BOX_THREADS / WAVE];
    const uint32_t i = blockIdx.x * BOX_THREADS + threadIdx.x;
    const bool keep = i < n && box(src, i);
    const CompactSlot c = compact_slot(keep, block_off, s_w);
    bool bit = false;
    if (keep) {
        GSR_BOUND(scene, 6, i >> 5, nwords_in);
        bit = set_bit(in, nwords_in, i);
    }
    const uint32_t o = c.o, w0 = c.off >> 5, k = (o >> 5) - w0, b = bit ? 1u << (o & 31u) : 0u;   // (k is 0, 1 or 2 for a kept lane)
    uint32_t v0 = k == 0u ? b : 0u, v1 = k == 1u ? b : 0u, v2 = k == 2u ? b : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        v0 |= __shfl_xor(v0, d);
        v1 |= __shfl_xor(v1, d);
        v2 |= __shfl_xor(v2, d);
    }
    if ((threadIdx.x & 63) != 0) return;
    const uint32_t v[3] = {v0, v1, v2};
#pragma unroll
    for (uint32_t j = 0; j < 3; j++) {
        if (!v[j]) continue;
        GSR_BOUND(scene, 7, w0 + j, nwords_out);
        if (w0 + j < nwords_out) atomicOr(&out[w0 + j], v[j]);
    }
}

// The three kept-prefix counts the new band thresholds come from: count[1 + k] = kept splats with index < at[k] (at[k] =
// bandsIndices[k] + 1 clamped to [0, n], by the host), beside the total k_box_scan left in count[0]: the exclusive offset at at[k].
// One workgroup per threshold; it recounts the part of the threshold's block in front of it.
struct BoxThresholds { uint32_t at[3]; };

template <class Pred>
__global__ __launch_bounds__(BOX_THREADS) void k_box_thresholds(uint32_t n, SceneDev sc, Pred box, const uint32_t* __restrict__ block_off,
                                                                BoxThresholds th, uint32_t* __restrict__ count)
{
    __shared__ uint32_t s_w[BOX_THREADS / WAVE];
    const uint32_t at = th.at[blockIdx.x];   // <= n
    const uint32_t block = at / BOX_THREADS, i = block * BOX_THREADS + threadIdx.x;
    const bool keep = i < at && box(sc, i);   // (i < at <= n)
    if (keep) GSR_BOUND(scene_sh, 0, i, n);
    wave_counts(keep, s_w);
    if (threadIdx.x == 0) {
        uint32_t t = at < n ? block_off[block] : count[0];   // (at == n: everything kept lies in front of it)
        if (at < n)
            for (int w = 0; w < BOX_THREADS / WAVE; w++) t += s_w[w];
        count[1 + blockIdx.x] = t;
    }
}

// k_box_compact's mask and offsets once more, for the SH rows: splat i > band0 owns row i - (band0 + 1) of each texture, 8 words
// = two uint4; kept splat number o owns row o - count[1] of the compacted ones (count[1]: the kept splats without SH, above).
// 96 bytes per kept SH splat, whole uint4 loads and stores.
template <class Pred>
__global__ __launch_bounds__(BOX_THREADS) void k_box_compact_sh(uint32_t n, SceneDev src, Pred box, const uint32_t* __restrict__ block_off,
                                                                const uint32_t* __restrict__ count, int32_t band0, uint32_t sh_count,
                                                                const uint4* __restrict__ r_in, const uint4* __restrict__ g_in,
                                                                const uint4* __restrict__ b_in, uint4* __restrict__ r_out,
                                                                uint4* __restrict__ g_out, uint4* __restrict__ b_out)
{
    __shared__ uint32_t s_w[BOX_THREADS / WAVE];
    const uint32_t i = blockIdx.x * BOX_THREADS + threadIdx.x;
    const bool keep = i < n && box(src, i);
    const CompactSlot c = compact_slot(keep, block_off, s_w);
    if (!keep || (int32_t)i <= band0) return;
    const size_t t = i - (uint32_t)(band0 + 1), u = c.o - count[1];   // (every kept splat in front of an SH splat is counted in o)
    GSR_BOUND(scene_sh, 1, t, sh_count);
    GSR_BOUND(scene_sh, 2, u, sh_count);
    if (t >= sh_count || u >= sh_count) return;
    const uint4 r0 = r_in[2 * t], r1 = r_in[2 * t + 1], g0 = g_in[2 * t], g1 = g_in[2 * t + 1], b0 = b_in[2 * t], b1 = b_in[2 * t + 1];
    r_out[2 * u] = r0; r_out[2 * u + 1] = r1;
    g_out[2 * u] = g0; g_out[2 * u + 1] = g1;
    b_out[2 * u] = b0; b_out[2 * u + 1] = b1;
}

// ---- a scene from the Scene's own arrays, and the scene back into them (gsr_set_scene_arrays / gsr_read_scene) ----
// Neither does arithmetic: words move between the SoA scene and the layouts of Scene.data / positions / rotations / scales.
// Scene.rotations is (w, x, y, z) per splat, byte for byte what `rot` holds, so rotations are copied straight in and out and
// no kernel touches them.  The three-float arrays go through LDS, so that a wave loads and stores whole consecutive lines on
// both sides: 256 splats = 768 consecutive words outside, one splat per lane (stride 3 words: no bank conflict) inside.
constexpr int XFER_THREADS = 256;   // (their bounds sites: `scene` 0..5, declared in front of k_box_compact_bits)

// Scene.scales (3 f32 per splat) -> scl (float4 per splat, w = 0 as k_build_scene leaves it)
__global__ __launch_bounds__(XFER_THREADS) void k_scene_import(const float* __restrict__ scales, uint32_t n, float4* __restrict__ scl)
{
    __shared__ float s_in[3 * XFER_THREADS];
    const size_t base = (size_t)blockIdx.x * XFER_THREADS, words = 3 * (size_t)n;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t cell = k * XFER_THREADS + threadIdx.x;
        const size_t w = 3 * base + cell;
        if (w < words) {
            GSR_BOUND(scene, 0, w, words);
            GSR_BOUND(scene, 1, cell, 3 * XFER_THREADS);
            s_in[cell] = scales[w];
        }
    }
    __syncthreads();
    const size_t i = base + threadIdx.x;
    if (i >= n) return;
    GSR_BOUND(scene, 1, 3 * threadIdx.x + 2, 3 * XFER_THREADS);
    GSR_BOUND(scene, 2, i, n);
    scl[i] = make_float4(s_in[3 * threadIdx.x], s_in[3 * threadIdx.x + 1], s_in[3 * threadIdx.x + 2], 0.f);
}

// SoA scene -> Scene.data rows (word 3 = 0), positions x 3, scales x 3; a null output is not produced.  For `data` a lane owns
// one splat: seven coalesced dword loads, two dwordx4 stores (its 32-byte row).
__global__ __launch_bounds__(XFER_THREADS) void k_scene_export(uint32_t n, SceneDev sc, uint4* __restrict__ data, float* __restrict__ positions,
                                                               float* __restrict__ scales)
{
    __shared__ float s_out[2][3 * XFER_THREADS];
    const size_t base = (size_t)blockIdx.x * XFER_THREADS, i = base + threadIdx.x, words = 3 * (size_t)n;
    if (i < n) {
        const float x = sc.px[i], y = sc.py[i], z = sc.pz[i];
        if (data) {
            GSR_BOUND(scene, 3, 2 * i + 1, 2 * (size_t)n);
            data[2 * i] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
            data[2 * i + 1] = make_uint4(sc.cov0[i], sc.cov1[i], sc.cov2[i], sc.rgba[i]);
        }
        GSR_BOUND(scene, 4, 3 * threadIdx.x + 2, 3 * XFER_THREADS);
        if (positions) { s_out[0][3 * threadIdx.x] = x; s_out[0][3 * threadIdx.x + 1] = y; s_out[0][3 * threadIdx.x + 2] = z; }
        if (scales) {
            const float4 s = sc.scl[i];
            s_out[1][3 * threadIdx.x] = s.x; s_out[1][3 * threadIdx.x + 1] = s.y; s_out[1][3 * threadIdx.x + 2] = s.z;
        }
    }
    if (!positions && !scales) return;   // (the same for every lane: nobody is left behind at the barrier)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t cell = k * XFER_THREADS + threadIdx.x;
        const size_t w = 3 * base + cell;
        if (w >= words) break;
        GSR_BOUND(scene, 4, cell, 3 * XFER_THREADS);
        GSR_BOUND(scene, 5, w, words);
        if (positions) positions[w] = s_out[0][cell];
        if (scales) scales[w] = s_out[1][cell];
    }
}

// ---- launchers ----
void launch_build_scene(const uint8_t* rows, uint32_t n, const SceneDev& sc, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_build_scene, dim3((n + 255) / 256), dim3(256), 0, s, (const uint4*)rows, n, sc);
}
void launch_scene_translate(uint32_t n, const SceneDev& sc, const double* t, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_scene_translate, dim3((n + 255) / 256), dim3(256), 0, s, n, sc, t[0], t[1], t[2]);
}
void launch_scene_rotate(uint32_t n, const SceneDev& sc, const double* q, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_scene_rotate, dim3((n + 255) / 256), dim3(256), 0, s, n, sc, q[0], q[1], q[2], q[3]);
}
void launch_scene_scale(uint32_t n, const SceneDev& sc, const double* sv, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_scene_scale, dim3((n + 255) / 256), dim3(256), 0, s, n, sc, sv[0], sv[1], sv[2]);
}
namespace {

template <class Pred>
void compact_with(uint32_t n, const SceneDev& src, const SceneDev& dst, const Pred& b, uint32_t* block_count, uint32_t* total, hipStream_t s)
{
    const uint32_t nblocks = (n + BOX_THREADS - 1) / BOX_THREADS;
    hipLaunchKernelGGL(k_box_count<Pred>, dim3(nblocks), dim3(BOX_THREADS), 0, s, n, src, b, block_count);
    hipLaunchKernelGGL(k_box_scan, dim3(1), dim3(BOX_THREADS), 0, s, block_count, nblocks, total);
    hipLaunchKernelGGL(k_box_compact<Pred>, dim3(nblocks), dim3(BOX_THREADS), 0, s, n, src, dst, b, (const uint32_t*)block_count);
}

template <class Pred>
void compact_sh_with(uint32_t n, const SceneDev& src, const Pred& b, const uint32_t* block_off, uint32_t* count, const int32_t* band,
                     uint32_t sh_count, const uint32_t* const* sh_in, uint32_t* const* sh_out, hipStream_t s)
{
    BoxThresholds th;
    for (int k = 0; k < 3; k++) th.at[k] = (uint32_t)std::min<int64_t>(std::max<int64_t>((int64_t)band[k] + 1, 0), (int64_t)n);
    const uint32_t nblocks = (n + BOX_THREADS - 1) / BOX_THREADS;
    hipLaunchKernelGGL(k_box_thresholds<Pred>, dim3(3), dim3(BOX_THREADS), 0, s, n, src, b, block_off, th, count);
    hipLaunchKernelGGL(k_box_compact_sh<Pred>, dim3(nblocks), dim3(BOX_THREADS), 0, s, n, src, b, block_off, (const uint32_t*)count, band[0], sh_count,
                       (const uint4*)sh_in[0], (const uint4*)sh_in[1], (const uint4*)sh_in[2], (uint4*)sh_out[0], (uint4*)sh_out[1], (uint4*)sh_out[2]);
}

Box box_of(const double* box)
{
    Box b;
    for (int k = 0; k < 6; k++) b.v[k] = box[k];
    return b;
}

}  // namespace

void launch_scene_compact(uint32_t n, const SceneDev& src, const SceneDev& dst, const ScenePred& p, uint32_t* block_count,
                          uint32_t* total, hipStream_t s)
{
    if (!n) return;
    if (p.box) compact_with(n, src, dst, box_of(p.box), block_count, total, s);
    else compact_with(n, src, dst, MaskKeep{p.mask, p.mask_words, p.keep}, block_count, total, s);
}

void launch_scene_compact_sh(uint32_t n, const SceneDev& src, const ScenePred& p, const uint32_t* block_off, uint32_t* count,
                             const int32_t* band, uint32_t sh_count, const uint32_t* const* sh_in, uint32_t* const* sh_out, hipStream_t s)
{
    if (!n) return;
    if (p.box) compact_sh_with(n, src, box_of(p.box), block_off, count, band, sh_count, sh_in, sh_out, s);
    else compact_sh_with(n, src, MaskKeep{p.mask, p.mask_words, p.keep}, block_off, count, band, sh_count, sh_in, sh_out, s);
}

void launch_scene_compact_bits(uint32_t n, const SceneDev& src, const ScenePred& p, const uint32_t* block_off, const uint32_t* in,
                               uint32_t nwords_in, uint32_t* out, uint32_t nwords_out, hipStream_t s)
{
    if (!n) return;
    const uint32_t nblocks = (n + BOX_THREADS - 1) / BOX_THREADS;
    if (p.box) hipLaunchKernelGGL(k_box_compact_bits<Box>, dim3(nblocks), dim3(BOX_THREADS), 0, s, n, src, box_of(p.box), block_off, in, nwords_in, out, nwords_out);
    else hipLaunchKernelGGL(k_box_compact_bits<MaskKeep>, dim3(nblocks), dim3(BOX_THREADS), 0, s, n, src, MaskKeep{p.mask, p.mask_words, p.keep}, block_off, in, nwords_in, out, nwords_out);
}

void launch_scene_import(const float* scales, uint32_t n, float4* scl, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_scene_import, dim3((n + XFER_THREADS - 1) / XFER_THREADS), dim3(XFER_THREADS), 0, s, scales, n, scl);
}
void launch_scene_export(uint32_t n, const SceneDev& sc, uint32_t* data, float* positions, float* scales, hipStream_t s)
{
    if (n && (data || positions || scales))
        hipLaunchKernelGGL(k_scene_export, dim3((n + XFER_THREADS - 1) / XFER_THREADS), dim3(XFER_THREADS), 0, s, n, sc, (uint4*)data, positions, scales);
}

}  // namespace gsr
