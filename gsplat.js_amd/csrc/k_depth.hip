// Depth planes and picking: the last frame's bin lists walked once more, writing depth instead of colour.
//
// For a pixel, its fragments are the entries of its bin's list, in list order, that pass the compositor's coverage test
// (|vPosition|^2 <= 4, the same f32 expression as k_blend's walk), with weight B = exp2(-q log2(e) + log2(opacity)); z of
// a splat is the w of its centre's clip position, the unfused sums of k_project_key.  Sequentially, from T = 1, D = 0:
//     w = T * B;  D = fma(w, z, D);  T = T - w;  the first fragment with 1 - T >= hit_alpha is the pixel's hit.
// Three planes: mean (D, premultiplied like the colour channels), hit (z of the hit, +inf without one) and index (the hit's
// splat index, 0xffffffff without one).
//
// k_depth_planes: one workgroup per bin, from the list's first entry to its last: no work items, no segments, no partials,
// no saturation skip -- the recurrence above is literally what runs, so the planes do not depend on how the compositor cut
// the frame.  k_pick: one wave per query pixel, the same recurrence in the same order.  Both go through depth_weight /
// depth_accumulate below, and through nothing else, for a fragment.
//
// Compiled with -ffp-contract=off like the rest of the device code: the fused multiply-adds are the explicit ones.
#include "k_depth_walk.h"   // DepthEntry, depth_entry, depth_weight, depth_row_u / _w, depth_tile_reach: shared with k_contrib.hip

namespace gsr {

GSR_BOUNDS_DECL(depth)   // sites: 0 bin -> bin_start, 1 list position, 2 splat index in the list, 3 LDS cell, 4 query pixel,
                         // 5 sample of a strided hit plane
constexpr uint32_t HIT_NONE = 0xffffffffu;

struct DepthPixel {
    float T, D, hit_z;
    uint32_t hit;
};
__device__ __forceinline__ DepthPixel depth_pixel_start()
{
    return DepthPixel{1.0f, 0.0f, __uint_as_float(0x7f800000u), HIT_NONE};
}

// The per-fragment arithmetic is k_depth_walk.h's depth_weight (the weight B of an entry at a pixel, negative where the fragment is
// discarded), in its own step so that k_pick can evaluate the weights of 64 entries across its lanes and still apply them one
// after the other through the recurrence:
__device__ __forceinline__ void depth_accumulate(DepthPixel& p, float B, float z, uint32_t index, float hit_alpha)
{
    if (B >= 0.0f) {
        const float w = p.T * B;
        p.D = __builtin_fmaf(w, z, p.D);
        p.T = p.T - w;
        if (p.hit == HIT_NONE && 1.0f - p.T >= hit_alpha) { p.hit = index; p.hit_z = z; }
    }
}
// SKIP: a wave leaves out the entries that provably cannot reach its 16x16 tile -- a conservative test at staging, k_blend's
// quadrant test at tile size: the tile's pixel centres lie outside the oriented box |vPosition.x|, |vPosition.y| <= 2
// (separating axes u and w), or farther from the centre than the longer semi-axis.  Every fragment left out has q > 4, so the
// planes are bit-identical with and without it (GSR_DEPTH_SKIP=0 is the build of the same walk that visits every entry).
//
// STEP: 1 is the pass above, every pixel, three planes.  2 is the delivery ring's strided pass (gsr_delivery_open_depth): the
// recurrence at the pixels (2i, 2j) only.  A wave still owns a 16x16 tile, but a lane owns ONE pixel of it, (ox + 2 lx,
// oy + 2 ly): one DepthPixel, one pair of row terms and one weight per visited entry instead of four, two and four.  Staging,
// the reach mask, the ballot and the list order are the same, and pxf / pyf are the same small exact integers the full pass
// uses for that pixel, so a sample is the full hit plane's value bit for bit.  It writes the hit plane only, ceil(W / 2) x
// ceil(H / 2) samples (a bin starts on an even pixel: sample (x / 2, y / 2)).
template <bool SKIP, int STEP>
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_planes(DepthBuffers a, BinGrid g, CamParams cam)
{
    __shared__ float4 s_a[DEPTH_CHUNK];       // ux, uy, ncu, wx
    __shared__ float4 s_b[DEPTH_CHUNK];       // wy, ncw, la, z
    __shared__ uint32_t s_idx[DEPTH_CHUNK];
    __shared__ uint32_t s_tiles[DEPTH_CHUNK]; // one bit per tile of the bin the entry can reach
    static_assert(STEP == 1 || STEP == 2, "every pixel, or every second one in both directions");

    // A frame whose lists did not fit published no work (k_bin_finalize): nothing of it is walked, nothing is written, and the
    // host learns at its next synchronisation that the planes are not this frame's.
    const bool unfit = *a.overflow != 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.invalid = unfit ? 1u : 0u;
    if (unfit) return;

    const int nbxb = g.bx_hi - g.bx_lo;
    const int bin = blockIdx.x;
    GSR_BOUND(depth, 0, bin, nbxb * g.nby);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = lane & 7, ly = lane >> 3;
    const int by = bin / nbxb, bxl = bin - by * nbxb;
    const int binX0 = (g.bx_lo + bxl) * BIN_PX, binY0 = by * BIN_PX;
    const int ox = (wave & 1) * TILE, oy = (wave >> 1) * TILE;
    [[maybe_unused]] const float pxf0 = (float)(ox + STEP * lx), pxf1 = pxf0 + 8.0f;   // (pxf1, pyf1: STEP 1, the lane's other column and row)
    [[maybe_unused]] const float pyf0 = (float)(oy + STEP * ly), pyf1 = pyf0 + 8.0f;
    const float bx0c = (float)binX0 + 0.5f, by0c = (float)binY0 + 0.5f;

    const uint32_t end = min(a.bin_start[bin + 1], a.capacity), begin = min(a.bin_start[bin], end);
    GSR_BOUND(depth, 1, a.bin_start[bin + 1], (unsigned long long)a.capacity + 1ull);
    GSR_BOUND(depth, 1, a.bin_start[bin], (unsigned long long)a.bin_start[bin + 1] + 1ull);

    DepthPixel p00 = depth_pixel_start();
    [[maybe_unused]] DepthPixel p10 = p00, p01 = p00, p11 = p00;   // pij: pixel (x + 8i, y + 8j); STEP 2: p00 only

    for (uint32_t base = begin; base < end; base += DEPTH_CHUNK) {
        __syncthreads();   // the previous chunk is consumed
        const uint32_t e = base + threadIdx.x;
        uint32_t tiles = 0;
        if (e < end) {
            GSR_BOUND(depth, 1, e, a.capacity);
            GSR_BOUND(depth, 2, a.list[e], a.nsplats);
            const uint32_t i = min(a.list[e], a.nsplats - 1u);
            const DepthEntry en = depth_entry(a.rec, a.px, a.py, a.pz, i, cam, bx0c, by0c);
            s_a[threadIdx.x] = make_float4(en.ux, en.uy, en.ncu, en.wx);
            s_b[threadIdx.x] = make_float4(en.wy, en.ncw, en.la, en.z);
            s_idx[threadIdx.x] = en.index;
            tiles = SKIP ? depth_tile_reach(en, a.rec + i, binX0, binY0) : 0xfu;
        }
        s_tiles[threadIdx.x] = tiles;
        __syncthreads();

        const uint32_t cnt = min((uint32_t)DEPTH_CHUNK, end - base);
        for (uint32_t c0 = 0; c0 < cnt; c0 += WAVE) {
            // my tile's entries among these 64, in list order (entries behind the list's end carry no bit)
            uint64_t bal = __ballot(((s_tiles[c0 + lane] >> wave) & 1u) != 0u);
            while (bal) {
                const uint32_t cell = c0 + (uint32_t)__builtin_ctzll(bal);
                bal &= bal - 1ull;
                GSR_BOUND(depth, 3, cell, DEPTH_CHUNK);
                const float4 ra = s_a[cell], rb = s_b[cell];   // the same address in every lane: a broadcast
                DepthEntry en;
                en.ux = ra.x; en.uy = ra.y; en.ncu = ra.z; en.wx = ra.w; en.wy = rb.x; en.ncw = rb.y; en.la = rb.z; en.z = rb.w;
                en.index = s_idx[cell];
                const float ur0 = depth_row_u(en, pyf0), wr0 = depth_row_w(en, pyf0);
                if constexpr (STEP == 1) {
                    const float ur1 = depth_row_u(en, pyf1), wr1 = depth_row_w(en, pyf1);
                    depth_accumulate(p00, depth_weight(en, pxf0, ur0, wr0), en.z, en.index, a.hit_alpha);
                    depth_accumulate(p10, depth_weight(en, pxf1, ur0, wr0), en.z, en.index, a.hit_alpha);
                    depth_accumulate(p01, depth_weight(en, pxf0, ur1, wr1), en.z, en.index, a.hit_alpha);
                    depth_accumulate(p11, depth_weight(en, pxf1, ur1, wr1), en.z, en.index, a.hit_alpha);
                } else {
                    depth_accumulate(p00, depth_weight(en, pxf0, ur0, wr0), en.z, en.index, a.hit_alpha);
                }
            }
        }
    }

    if constexpr (STEP == 1) {
        const int x0 = binX0 + ox + lx, x1 = x0 + 8, y0 = binY0 + oy + ly, y1 = y0 + 8;
        auto store = [&](int x, int y, const DepthPixel& p) {
            if (x < g.W && y < g.H) {
                const size_t o = (size_t)y * g.W + x;
                a.mean[o] = p.D; a.hit[o] = p.hit_z; a.index[o] = p.hit;
            }
        };
        store(x0, y0, p00); store(x1, y0, p10); store(x0, y1, p01); store(x1, y1, p11);
    } else {
        const int x = binX0 + ox + STEP * lx, y = binY0 + oy + STEP * ly;   // (even: bins and tiles start on even pixels)
        if (x < g.W && y < g.H) {
            const int Wd = (g.W + STEP - 1) / STEP;
            const size_t o = (size_t)(y / STEP) * Wd + x / STEP;
            GSR_BOUND(depth, 5, o, (size_t)Wd * ((g.H + STEP - 1) / STEP));
            a.hit[o] = p00.hit_z;
        }
    }
}

// One wave per query pixel: 64 entries of the pixel's bin list per step, every lane the weight and z of its entry, then the
// recurrence over the covering entries one after the other in list order (never a scan: the association is the planes kernel's).
__global__ __launch_bounds__(WAVE) void k_pick(DepthBuffers a, BinGrid g, CamParams cam, const int32_t* __restrict__ xy, uint32_t count,
                                               PickResult* __restrict__ out)
{
    const bool unfit = *a.overflow != 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.invalid = unfit ? 1u : 0u;
    if (unfit) return;
    const uint32_t qi = blockIdx.x;
    if (qi >= count) return;
    const int nbxb = g.bx_hi - g.bx_lo;
    const int lane = threadIdx.x;
    // (the host refuses pixels outside the image or the band; the clamp keeps every index below in range whatever arrives)
    const int xlo = g.bx_lo * BIN_PX, xhi = min(g.bx_hi * BIN_PX, g.W) - 1;
    GSR_BOUND(depth, 4, xy[2 * qi] - xlo, xhi - xlo + 1);
    GSR_BOUND(depth, 4, xy[2 * qi + 1], g.H);
    const int x = min(max(xy[2 * qi], xlo), xhi), y = min(max(xy[2 * qi + 1], 0), g.H - 1);
    const int bxl = x / BIN_PX - g.bx_lo, by = y / BIN_PX;
    const int bin = by * nbxb + bxl;
    GSR_BOUND(depth, 0, bin, nbxb * g.nby);
    const int binX0 = (g.bx_lo + bxl) * BIN_PX, binY0 = by * BIN_PX;
    const float pxf = (float)(x - binX0), pyf = (float)(y - binY0);
    const float bx0c = (float)binX0 + 0.5f, by0c = (float)binY0 + 0.5f;
    const uint32_t end = min(a.bin_start[bin + 1], a.capacity), begin = min(a.bin_start[bin], end);

    DepthPixel p = depth_pixel_start();
    for (uint32_t base = begin; base < end; base += WAVE) {
        const uint32_t e = base + lane;
        float B = -1.0f, z = 0.0f;
        uint32_t index = 0;
        if (e < end) {
            GSR_BOUND(depth, 1, e, a.capacity);
            GSR_BOUND(depth, 2, a.list[e], a.nsplats);
            const uint32_t i = min(a.list[e], a.nsplats - 1u);
            const DepthEntry en = depth_entry(a.rec, a.px, a.py, a.pz, i, cam, bx0c, by0c);
            B = depth_weight(en, pxf, depth_row_u(en, pyf), depth_row_w(en, pyf));
            z = en.z; index = en.index;
        }
        uint64_t bal = __ballot(B >= 0.0f);
        while (bal) {
            const int j = __builtin_ctzll(bal);
            bal &= bal - 1ull;
            depth_accumulate(p, __shfl(B, j), __shfl(z, j), __shfl(index, j), a.hit_alpha);
        }
    }
    if (lane == 0) out[qi] = PickResult{p.hit, p.hit_z, p.D, 1.0f - p.T};
}

// the planes of pixels no bin of the context covers (a band context's other columns): 0 / +inf / none
__global__ void k_depth_fill(float* __restrict__ mean, float* __restrict__ hit, uint32_t* __restrict__ index, uint32_t npix)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    mean[i] = 0.0f; hit[i] = __uint_as_float(0x7f800000u); index[i] = HIT_NONE;
}

void launch_depth_planes(const DepthBuffers& b, const BinGrid& g, const CamParams& cam, bool skip, int step, hipStream_t s)
{
    const int nbins = (g.bx_hi - g.bx_lo) * g.nby;
    if (nbins <= 0) return;
    const dim3 grid(nbins), block(DEPTH_THREADS);
    if (step == 2) {
        if (skip) hipLaunchKernelGGL((k_depth_planes<true, 2>), grid, block, 0, s, b, g, cam);
        else hipLaunchKernelGGL((k_depth_planes<false, 2>), grid, block, 0, s, b, g, cam);
    } else {
        if (skip) hipLaunchKernelGGL((k_depth_planes<true, 1>), grid, block, 0, s, b, g, cam);
        else hipLaunchKernelGGL((k_depth_planes<false, 1>), grid, block, 0, s, b, g, cam);
    }
}

void launch_pick(const DepthBuffers& b, const BinGrid& g, const CamParams& cam, const int32_t* xy, uint32_t count, PickResult* out, hipStream_t s)
{
    if (!count || (g.bx_hi - g.bx_lo) * g.nby <= 0) return;
    hipLaunchKernelGGL(k_pick, dim3(count), dim3(WAVE), 0, s, b, g, cam, xy, count, out);
}

void launch_depth_fill(float* mean, float* hit, uint32_t* index, uint32_t npix, hipStream_t s)
{
    if (!npix) return;
    hipLaunchKernelGGL(k_depth_fill, dim3((npix + 255) / 256), dim3(256), 0, s, mean, hit, index, npix);
}

}  // namespace gsr
