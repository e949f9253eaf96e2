// Rotating SH coefficients ("Rotating SH coefficients"): c' = D_l c per band of every SH row in scope, in
// place, for the three channels.  D_1 (3x3), D_2 (5x5) and D_3 (7x7) come from the host (gsr_sh_rotation) as f32 and ride in the
// kernel arguments, so they are wave-uniform and live in scalar registers.  The arithmetic is f32 in the stated order -- the first
// product, then one product and one sum per further column, columns ascending -- compiled with -ffp-contract=off; the store rounds
// to half to nearest even ((_Float16)s), a NaN is stored as 0x7e00, and half 0 (DC) keeps its bits.
// One thread per splat, as in k_edit.hip: the selection word words[i >> 5] is the same over each half of a wave64, so a wave whose
// two words are zero, or whose 64 splats lie at or below bandsIndices[0], has no lane left behind the test and loads nothing.  A
// lane's row is 32 bytes per channel (two uint4 loads, two uint4 stores) and the rows of a wave are contiguous, 2 KB per channel.
// One channel at a time: 16 coefficients in, 15 out.  No LDS.
#include "gsr_internal.h"
#include "k_splat_ops.h"

namespace gsr {

GSR_BOUNDS_DECL(sh_rotate)   // sites: 0 selection word, 1 splat index, 2 the row's second uint4 against the texture's 2 * sh_count.
                             // Site 0 compares with an extent the host passes beside the words (nwords); site 2 with sh_count, which
                             // the host passes beside `first`: it counts when first + sh_count and n disagree; site 1 stands behind
                             // the `i < n` guard of the same n

constexpr int SHROT_THREADS = 256;

__device__ __forceinline__ float shrot_half(uint32_t h)
{
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(h & 0xffffu));   // v_cvt_f32_f16: exact
}

// round to nearest even, subnormals kept, overflow to infinity (v_cvt_f16_f32); any NaN is the one quiet NaN
__device__ __forceinline__ uint32_t shrot_to_half(float s)
{
    if (s != s) return 0x7e00u;
    return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)s);
}

// out[k] = sum over the band's columns of m[k][j] * c[j], j ascending, each product and each sum rounded to f32
template <int W>
__device__ __forceinline__ void shrot_band(const float* m, const float* c, uint32_t* out)
{
#pragma unroll
    for (int k = 0; k < W; k++) {
        float s = m[k * W] * c[0];
#pragma unroll
        for (int j = 1; j < W; j++) s = s + m[k * W + j] * c[j];
        out[k] = shrot_to_half(s);
    }
}

// one row of one channel: halves 1..15 rotated, half 0 as it was
__device__ __forceinline__ void shrot_row(uint4* __restrict__ p, const ShRotation& M)
{
    const uint4 a = p[0], b = p[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    float c[16];
#pragma unroll
    for (int j = 0; j < 8; j++) { c[2 * j] = shrot_half(w[j]); c[2 * j + 1] = shrot_half(w[j] >> 16); }
    uint32_t h[16];
    h[0] = w[0] & 0xffffu;
    shrot_band<3>(M.d1, c + 1, h + 1);
    shrot_band<5>(M.d2, c + 4, h + 4);
    shrot_band<7>(M.d3, c + 9, h + 9);
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = h[2 * j] | (h[2 * j + 1] << 16);
    p[0] = make_uint4(o[0], o[1], o[2], o[3]);
    p[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// first = bandsIndices[0] + 1: the splat of SH row 0.  `base` (a multiple of the workgroup) is the first splat the grid covers.
// counter (may be null): SH_ROTATE_COUNTERS slots, SH_ROTATE_COUNTER_STRIDE words apart (a cache line each); their sum += the rows
// rotated, one relaxed add per wave that has any
template <bool SELECTED>
__global__ __launch_bounds__(SHROT_THREADS) void k_sh_rotate(uint32_t n, uint32_t base, uint32_t first, uint32_t sh_count, uint32_t* __restrict__ sh_r,
                                                             uint32_t* __restrict__ sh_g, uint32_t* __restrict__ sh_b,
                                                             const uint32_t* __restrict__ words, uint32_t nwords, ShRotation M,
                                                             uint32_t* __restrict__ counter)
{
    const uint32_t i = base + blockIdx.x * SHROT_THREADS + threadIdx.x;
    bool in = i < n && i >= first;
    if (SELECTED && in) {
        GSR_BOUND(sh_rotate, 0, i >> 5, nwords);
        GSR_BOUND(sh_rotate, 1, i, n);
        in = set_bit(words, nwords, i);
    }
    if (counter) {   // (15 625 waves adding to ONE word took 150 us at 1 M rows, five times the rotation itself: the waves take turns over the slots)
        const unsigned long long m = __ballot(in);
        const uint32_t slot = (blockIdx.x * (SHROT_THREADS / WAVE) + (threadIdx.x >> 6)) & (SH_ROTATE_COUNTERS - 1u);
        if (m && (threadIdx.x & 63u) == 0u)
            __hip_atomic_fetch_add(counter + slot * SH_ROTATE_COUNTER_STRIDE, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!in) return;
    const uint32_t t = i - first;
    GSR_BOUND(sh_rotate, 2, 2ull * t + 1ull, 2ull * sh_count);
    if (t >= sh_count) return;
    // a loop, not three copies: unrolled, the scheduler hoists the matrix loads of all three and spills scalar registers into lanes
    // (38 of them); rolled, the 83 entries stay in scalar registers across the channels, no spill
#pragma unroll 1
    for (int ch = 0; ch < 3; ch++) {
        uint32_t* tex = ch == 0 ? sh_r : ch == 1 ? sh_g : sh_b;
        shrot_row(reinterpret_cast<uint4*>(tex) + 2 * (size_t)t, M);
    }
}

// words null: every SH row; else the rows of the selected splats.  n = first + sh_count (gsr_set_scene_sh holds them to it)
void launch_sh_rotate(uint32_t n, uint32_t first, uint32_t sh_count, uint32_t* const* tex, const uint32_t* words, uint32_t nwords,
                      const ShRotation& M, uint32_t* counter, hipStream_t s)
{
    if (!sh_count || first >= n) return;
    const uint32_t base = first / SHROT_THREADS * SHROT_THREADS;
    const dim3 grid((n - base + SHROT_THREADS - 1) / SHROT_THREADS);
    if (words)
        hipLaunchKernelGGL(k_sh_rotate<true>, grid, dim3(SHROT_THREADS), 0, s, n, base, first, sh_count, tex[0], tex[1], tex[2], words, nwords, M, counter);
    else
        hipLaunchKernelGGL(k_sh_rotate<false>, grid, dim3(SHROT_THREADS), 0, s, n, base, first, sh_count, tex[0], tex[1], tex[2], words, nwords, M, counter);
}

}  // namespace gsr
