// Contribution: the last frame's bin lists walked once more, keeping the weight of every fragment per SPLAT instead of per pixel.
//
// The fragments of a pixel, their weight B and the transmittance T are exactly those of "depth and pick" (k_depth_walk.h, shared
// with k_depth.hip): the entries of the pixel's bin list, in list order, that pass q <= 4; from T = 1, w = T * B, T = T - w, in f32,
// from the list's first entry to its last -- no early termination, no saturation skip, no segments.  Per splat i, over the pixels
// of the image where i is a fragment ("Contribution"):
//     weight[i] += (uint64_t)rintf(w * 2^24)     quanta of 2^-24, ties to even; w <= 1, so one term is at most 2^24
//     peak[i]    = max(peak[i], w)               on the bit patterns: w >= 0, so the order of the bits is the order of the values
//     pixels[i] += 1                             whatever the weight; modulo 2^32
// Integers and a maximum: the result does not depend on the order in which tiles, bins, contexts and views arrive.
//
// k_contrib walks a bin the way k_depth_walk.h's skeleton does (a 256-thread workgroup per bin, chunks of 256 entries staged into LDS,
// one wave per 16x16 tile, four pixels per lane, the ballot over s_tiles gives list order) but keeps its own loop, as k_pick does, over
// the skeleton's helpers: through walk_bin_list it measured 2.8 % longer (profiles/second_walk_ab.txt, section 6).  No barrier at the
// loop's top: the one in front of the flush does that job, and a thread restages no cell but the one it flushes.  Every chunk cell has
// three LDS accumulators.  Per visited entry a wave counts its covered pixels with four ballots, reduces its lanes' sums and maxima
// across lanes (16-lane rows in 32 bits: a lane's sum is at most 2^26, a row's 2^30; the four row totals are added in 64 bits, since
// the wave's sum reaches 2^32 when every pixel has w = 1) and ONE lane updates the cell -- never 64 LDS atomics on one address, which
// serialise.  After the chunk, thread t flushes cell t with three return-less global atomics, if any pixel was covered: a splat
// occurs once in a bin's list, so global atomics number three per (bin, covering entry).
//
// Compiled with -ffp-contract=off like the rest of the device code: the fused multiply-adds are the explicit ones.
#include "k_attr.h"
#include "k_depth_walk.h"
#include "k_splat_ops.h"

namespace gsr {

GSR_BOUNDS_DECL(contrib)   // sites: 0 - 3 the walk's (WALK_SITE_*: 0 - 2 in its helpers, 3 here), 4 accumulator index, 5 selection word
struct ContribBounds {
    static __device__ __forceinline__ void bound(int site, unsigned long long idx, unsigned long long limit) { GSR_BOUND(contrib, site, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(contrib, 5, idx, limit); }   // (k_splat_ops.h)
};
constexpr int CONTRIB_SELECT_THREADS = 256;
constexpr float CONTRIB_QUANTA = 16777216.0f;   // 2^24

// one pixel's step of the recurrence for a covering fragment: its weight, added to the lane's sum of quanta and folded into its maximum
__device__ __forceinline__ void contrib_step(float& T, float B, bool covered, uint32_t& quanta, uint32_t& peak)
{
    if (covered) {
        const float w = T * B;
        T = T - w;
        quanta += (uint32_t)rintf(w * CONTRIB_QUANTA);
        peak = max(peak, __float_as_uint(w));
    }
}

template <bool SKIP>
__global__ __launch_bounds__(DEPTH_THREADS) void k_contrib(ContribBuffers a, BinGrid g, CamParams cam)
{
    __shared__ float4 s_a[DEPTH_CHUNK];       // ux, uy, ncu, wx
    __shared__ float4 s_b[DEPTH_CHUNK];       // wy, ncw, la, -
    __shared__ uint32_t s_idx[DEPTH_CHUNK];
    __shared__ uint32_t s_tiles[DEPTH_CHUNK]; // one bit per tile of the bin the entry can reach
    __shared__ unsigned long long s_sum[DEPTH_CHUNK];   // the cell's entry over the bin's pixels: quanta,
    __shared__ uint32_t s_cnt[DEPTH_CHUNK];             // covered pixels,
    __shared__ uint32_t s_peak[DEPTH_CHUNK];            // largest weight (bits)

    // A frame whose lists did not fit published no work (k_bin_finalize): nothing of it is walked, nothing is added, and it is
    // not counted as a pass (k_depth_planes has the same rule).
    if (*a.overflow != 0u) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(a.frames, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    const WalkBin w = walk_bin<ContribBounds>(a, g, blockIdx.x);
    const int lane = w.lane, wave = w.wave;
    const float pxf0 = (float)(w.ox + w.lx), pxf1 = pxf0 + 8.0f;
    const float pyf0 = (float)(w.oy + w.ly), pyf1 = pyf0 + 8.0f;
    // the lane's pixels (x + 8i, y + 8j) that are pixels of the image: a partial last bin's other pixels have no fragments
    const int x = w.binX0 + w.ox + w.lx, y = w.binY0 + w.oy + w.ly;
    const bool inx0 = x < g.W, inx1 = x + 8 < g.W, iny0 = y < g.H, iny1 = y + 8 < g.H;
    const uint32_t begin = w.begin, end = w.end;

    float T00 = 1.0f, T10 = 1.0f, T01 = 1.0f, T11 = 1.0f;   // Tij: pixel (x + 8i, y + 8j)

    for (uint32_t base = begin; base < end; base += DEPTH_CHUNK) {
        // (the previous chunk is consumed: the barrier in front of its flush, and a thread flushes the cell it stages)
        const uint32_t e = base + threadIdx.x;
        uint32_t tiles = 0;
        if (e < end) {
            const uint32_t i = walk_list_entry<ContribBounds>(a, e);
            const DepthEntry en = depth_entry(a.rec, a.px, a.py, a.pz, i, cam, w.bx0c, w.by0c);
            s_a[threadIdx.x] = make_float4(en.ux, en.uy, en.ncu, en.wx);
            s_b[threadIdx.x] = make_float4(en.wy, en.ncw, en.la, 0.0f);
            s_idx[threadIdx.x] = en.index;
            tiles = SKIP ? depth_tile_reach(en, a.rec[i].cx, a.rec[i].cy, w.binX0, w.binY0) : 0xfu;
        }
        s_tiles[threadIdx.x] = tiles;
        s_sum[threadIdx.x] = 0ull; s_cnt[threadIdx.x] = 0u; s_peak[threadIdx.x] = 0u;
        __syncthreads();

        const uint32_t cnt = min((uint32_t)DEPTH_CHUNK, end - base);
        for (uint32_t c0 = 0; c0 < cnt; c0 += WAVE) {
            // my tile's entries among these 64, in list order (entries behind the list's end carry no bit)
            uint64_t bal = __ballot(((s_tiles[c0 + lane] >> wave) & 1u) != 0u);
            while (bal) {
                const uint32_t cell = c0 + (uint32_t)__builtin_ctzll(bal);
                bal &= bal - 1ull;
                GSR_BOUND(contrib, WALK_SITE_CELL, cell, DEPTH_CHUNK);
                const float4 ra = s_a[cell], rb = s_b[cell];   // the same address in every lane: a broadcast
                DepthEntry en;
                en.ux = ra.x; en.uy = ra.y; en.ncu = ra.z; en.wx = ra.w; en.wy = rb.x; en.ncw = rb.y; en.la = rb.z; en.z = 0.0f;
                en.index = 0u;
                const float ur0 = depth_row_u(en, pyf0), wr0 = depth_row_w(en, pyf0);
                const float ur1 = depth_row_u(en, pyf1), wr1 = depth_row_w(en, pyf1);
                const float B00 = depth_weight(en, pxf0, ur0, wr0), B10 = depth_weight(en, pxf1, ur0, wr0);
                const float B01 = depth_weight(en, pxf0, ur1, wr1), B11 = depth_weight(en, pxf1, ur1, wr1);
                const bool c00 = inx0 && iny0 && B00 >= 0.0f, c10 = inx1 && iny0 && B10 >= 0.0f;
                const bool c01 = inx0 && iny1 && B01 >= 0.0f, c11 = inx1 && iny1 && B11 >= 0.0f;
                // the tile's covered pixels: four ballots, no cross-lane traffic; none covered: nothing to reduce, nothing to update
                const uint32_t covered = (uint32_t)(__popcll(__ballot(c00)) + __popcll(__ballot(c10)) + __popcll(__ballot(c01)) + __popcll(__ballot(c11)));
                if (!covered) continue;
                uint32_t quanta = 0, peak = 0;   // of the lane's four pixels: at most 4 * 2^24
                contrib_step(T00, B00, c00, quanta, peak);
                contrib_step(T10, B10, c10, quanta, peak);
                contrib_step(T01, B01, c01, quanta, peak);
                contrib_step(T11, B11, c11, quanta, peak);
                // rows of 16 lanes in 32 bits (at most 16 * 2^26 = 2^30) ...
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {
                    quanta += (uint32_t)__shfl_xor((int)quanta, m);
                    peak = max(peak, (uint32_t)__shfl_xor((int)peak, m));
                }
                // ... and the four row totals in 64: the wave's sum is 2^32 when every pixel of the tile has w = 1
                unsigned long long sum = 0;
                uint32_t top = 0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    sum += (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)quanta, 16 * r);
                    top = max(top, (uint32_t)__builtin_amdgcn_readlane((int)peak, 16 * r));
                }
                if (lane == 0) {   // ONE lane per wave and entry; the bin's four waves meet in the cell
                    __hip_atomic_fetch_add(&s_sum[cell], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&s_cnt[cell], covered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_max(&s_peak[cell], top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();   // the chunk's cells are final

        // cell t to the scene's accumulators: relaxed, agent scope, results unused (return-less atomics)
        if (threadIdx.x < cnt && s_cnt[threadIdx.x] != 0u) {
            const uint32_t i = s_idx[threadIdx.x];
            GSR_BOUND(contrib, 4, i, a.rows);
            if (i < a.rows) {
                __hip_atomic_fetch_add(&a.weight[i], s_sum[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&a.pixels[i], s_cnt[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(&a.peak[i], s_peak[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// gsr_select_contrib.  One thread per splat: its value in f64 (attr_value, k_attr.h), compared with `below`.  A wave's ballot is two whole words
// of the mask (mask_store_ballot, k_splat_ops.h): every word of the mask is stored (splats at and above n vote 0).
__global__ __launch_bounds__(CONTRIB_SELECT_THREADS) void k_contrib_select(int stat, double below, uint32_t n, const unsigned long long* __restrict__ weight,
                                                                           const uint32_t* __restrict__ peak, const uint32_t* __restrict__ pixels,
                                                                           uint32_t* __restrict__ scratch, uint32_t nwords)
{
    const uint32_t i = blockIdx.x * CONTRIB_SELECT_THREADS + threadIdx.x;
    bool in = false;
    if (i < n) {
        const AttrSource src{nullptr, nullptr, nullptr, nullptr, nullptr, weight, peak, pixels, 0.0, 0.0, 0.0};
        in = attr_value(ATTR_CONTRIB_WEIGHT + stat, src, i) < below;   // (the one statement of the value: k_attr.h)
    }
    mask_store_ballot<ContribBounds>(scratch, nwords, i, __ballot(in));
}

void launch_contrib(const ContribBuffers& b, const BinGrid& g, const CamParams& cam, bool skip, hipStream_t s)
{
    walk_launch(skip ? k_contrib<true> : k_contrib<false>, b, g, cam, s);
}

void launch_contrib_select(int stat, double below, uint32_t n, const unsigned long long* weight, const uint32_t* peak, const uint32_t* pixels,
                           uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_contrib_select, dim3(mask_blocks(nwords, CONTRIB_SELECT_THREADS)), dim3(CONTRIB_SELECT_THREADS), 0, s, stat, below, n, weight, peak, pixels, scratch, nwords);
}

}  // namespace gsr
