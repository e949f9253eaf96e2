// Depth planes and picking: the last frame's bin lists walked once more, writing depth instead of colour.
//
// For a pixel, its fragments are the entries of its bin's list, in list order, that pass the compositor's coverage test
// (|vPosition|^2 <= 4, the same f32 expression as k_blend's walk), with weight B = exp2(-q log2(e) + log2(opacity)); z of
// a splat is the w of its centre's clip position, the unfused sums of k_project_key.  Sequentially, from T = 1, D = 0:
//     w = T * B;  D = fma(w, z, D);  T = T - w;  the first fragment with 1 - T >= hit_alpha is the pixel's hit.
// Three planes: mean (D, premultiplied like the colour channels), hit (z of the hit, +inf without one) and index (the hit's
// splat index, 0xffffffff without one).
//
// k_depth_planes: the walk of one bin (k_depth_walk.h) with DepthPass, from the list's first entry to its last: no work items, no
// segments, no partials, no saturation skip -- the recurrence above is literally what runs, so the planes do not depend on how the
// compositor cut the frame.  k_pick: one wave per query pixel, the same recurrence in the same order, its own loop.  Both go through depth_weight /
// depth_accumulate below, and through nothing else, for a fragment.
//
// Compiled with -ffp-contract=off like the rest of the device code: the fused multiply-adds are the explicit ones.
#include "k_depth_walk.h"   // the per-fragment arithmetic and the walk of one bin: shared with k_contrib.hip and k_overlay.hip

namespace gsr {

GSR_BOUNDS_DECL(depth)   // sites: 0 - 3 the walk's (WALK_SITE_*), 4 query pixel, 5 sample of a strided hit plane
struct DepthBounds {
    static __device__ __forceinline__ void bound(int site, unsigned long long idx, unsigned long long limit) { GSR_BOUND(depth, site, idx, limit); }
};
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
// SKIP: a wave leaves out the entries that provably cannot reach its 16x16 tile (depth_tile_reach, at staging).  Every fragment left
// out has q > 4, so the planes are bit-identical with and without it (GSR_DEPTH_SKIP=0 is the build that visits every entry).
//
// STEP: 1 is the pass above, every pixel, three planes.  2 is the delivery ring's strided pass (gsr_delivery_open_depth): the
// recurrence at the pixels (2i, 2j) only.  A wave still owns a 16x16 tile, but a lane owns ONE pixel of it, (ox + 2 lx,
// oy + 2 ly): one DepthPixel, one pair of row terms and one weight per visited entry instead of four, two and four.  Staging,
// the reach mask, the ballot and the list order are the same, and pxf / pyf are the same small exact integers the full pass
// uses for that pixel, so a sample is the full hit plane's value bit for bit.  It writes the hit plane only, ceil(W / 2) x
// ceil(H / 2) samples (a bin starts on an even pixel: sample (x / 2, y / 2)).
//
// The pass of the walk (k_depth_walk.h): a cell holds z in its spare word and the splat's index beside it; a visit is the recurrence
// at the lane's pixels pij = (x + 8i, y + 8j) (STEP 2: p00 only).
template <int STEP>
struct DepthPass : DepthBounds {
    uint32_t* s_idx;
    float hit_alpha, pxf0, pxf1, pyf0, pyf1;
    DepthPixel &p00, &p10, &p01, &p11;   // the kernel's own locals, by reference: so the updates compile to selects (profiles/second_walk_ab.txt)
    __device__ __forceinline__ float stage(const DepthEntry& en) { s_idx[threadIdx.x] = en.index; return en.z; }
    __device__ __forceinline__ void visit(uint32_t cell, DepthEntry en)
    {
        en.index = s_idx[cell];
        const float ur0 = depth_row_u(en, pyf0), wr0 = depth_row_w(en, pyf0);
        depth_accumulate(p00, depth_weight(en, pxf0, ur0, wr0), en.z, en.index, hit_alpha);
        if constexpr (STEP == 1) {
            const float ur1 = depth_row_u(en, pyf1), wr1 = depth_row_w(en, pyf1);
            depth_accumulate(p10, depth_weight(en, pxf1, ur0, wr0), en.z, en.index, hit_alpha);
            depth_accumulate(p01, depth_weight(en, pxf0, ur1, wr1), en.z, en.index, hit_alpha);
            depth_accumulate(p11, depth_weight(en, pxf1, ur1, wr1), en.z, en.index, hit_alpha);
        }
    }
};

template <bool SKIP, int STEP>
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_planes(DepthBuffers a, BinGrid g, CamParams cam)
{
    __shared__ WalkStage st;
    __shared__ uint32_t s_idx[DEPTH_CHUNK];
    static_assert(STEP == 1 || STEP == 2, "every pixel, or every second one in both directions");
    if (walk_frame_unfit(a.overflow, a.invalid)) return;

    const WalkBin w = walk_bin<DepthBounds>(a, g, blockIdx.x);
    const float pxf0 = (float)(w.ox + STEP * w.lx), pyf0 = (float)(w.oy + STEP * w.ly);   // (STEP 1: + 8, the lane's other column and row)
    DepthPixel p00 = depth_pixel_start(), p10 = p00, p01 = p00, p11 = p00;
    DepthPass<STEP> pass{{}, s_idx, a.hit_alpha, pxf0, pxf0 + 8.0f, pyf0, pyf0 + 8.0f, p00, p10, p01, p11};
    walk_bin_list<SKIP>(st, a, w, cam, w.begin, w.end, pass);

    if constexpr (STEP == 1) {
        const int x0 = w.binX0 + w.ox + w.lx, x1 = x0 + 8, y0 = w.binY0 + w.oy + w.ly, y1 = y0 + 8;
        auto store = [&](int x, int y, const DepthPixel& p) {
            if (x < g.W && y < g.H) {
                const size_t o = (size_t)y * g.W + x;
                a.mean[o] = p.D; a.hit[o] = p.hit_z; a.index[o] = p.hit;
            }
        };
        store(x0, y0, p00); store(x1, y0, p10); store(x0, y1, p01); store(x1, y1, p11);
    } else {
        const int x = w.binX0 + w.ox + STEP * w.lx, y = w.binY0 + w.oy + STEP * w.ly;   // (even: bins and tiles start on even pixels)
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
    if (walk_frame_unfit(a.overflow, a.invalid)) return;
    const uint32_t qi = blockIdx.x;
    if (qi >= count) return;
    const int lane = threadIdx.x;
    // (the host refuses pixels outside the image or the band; the clamp keeps every index below in range whatever arrives)
    const int xlo = g.bx_lo * BIN_PX, xhi = min(g.bx_hi * BIN_PX, g.W) - 1;
    GSR_BOUND(depth, 4, xy[2 * qi] - xlo, xhi - xlo + 1);
    GSR_BOUND(depth, 4, xy[2 * qi + 1], g.H);
    const int x = min(max(xy[2 * qi], xlo), xhi), y = min(max(xy[2 * qi + 1], 0), g.H - 1);
    const WalkBin w = walk_bin<DepthBounds>(a, g, (y / BIN_PX) * (g.bx_hi - g.bx_lo) + (x / BIN_PX - g.bx_lo));
    const float pxf = (float)(x - w.binX0), pyf = (float)(y - w.binY0);

    DepthPixel p = depth_pixel_start();
    for (uint32_t base = w.begin; base < w.end; base += WAVE) {
        const uint32_t e = base + lane;
        float B = -1.0f, z = 0.0f;
        uint32_t index = 0;
        if (e < w.end) {
            const DepthEntry en = depth_entry(a.rec, a.px, a.py, a.pz, walk_list_entry<DepthBounds>(a, e), cam, w.bx0c, w.by0c);
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
    if (step == 2) walk_launch(skip ? k_depth_planes<true, 2> : k_depth_planes<false, 2>, b, g, cam, s);
    else walk_launch(skip ? k_depth_planes<true, 1> : k_depth_planes<false, 1>, b, g, cam, s);
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
