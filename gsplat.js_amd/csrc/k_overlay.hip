// Selection overlay: the last frame's bin lists walked once more, keeping per pixel what the SELECTED splats supplied.
//
// The fragments of a pixel, their weight B and the transmittance T are exactly those of "depth and pick" (k_depth_walk.h, shared
// with k_depth.hip and k_contrib.hip): the entries of the pixel's bin list, in list order, that pass q <= 4, from the list's first
// entry on -- no early termination, no saturation skip, no segments.  A splat's colour c is the compositor's: (float)byte *
// (1.0f / 255.0f) of the record's rgb8, or this frame's shcol[i] where RGB8_IN_SHCOL is set.  From T = 1, S = 0, C = 0, in f32
// ("Selection overlay"):
//     w = T * B;  T = T - w;  selected:  S = S + w;  C = fma(w, c, C)
//     cover   = S
//     overlay = (fma(mix, fma(tint, S, -C), fb.rgb), fb.a)        fb: the frame's framebuffer value, read, never written
// which is the frame with every selected splat's colour replaced by lerp(c, tint, mix).  mix == 0 and pixels without a selected
// fragment give fb bit for bit.
//
// k_overlay keeps the shape of k_depth_planes<SKIP, 1>: one 256-thread workgroup per bin, chunks of 256 entries staged into LDS,
// one wave per 16x16 tile, four pixels per lane, the ballot over s_tiles gives list order.  Staging adds the entry's colour and its
// selection bit to the cell; the visited cell is read at one address by every lane (a broadcast), and whether it is selected is
// uniform over the wave.  TRIM: entries behind the list's last selected entry change T only, which is not a result, so the
// workgroup first finds that entry (one pass over list[] and the mask: a ballot per wave, a maximum in LDS) and walks
// [begin, last + 1): nothing at all in a bin without a selected entry.  The same bits with and without (GSR_OVERLAY_TRIM=0).
//
// Compiled with -ffp-contract=off like the rest of the device code: the fused multiply-adds are the explicit ones.
#include "k_depth_walk.h"

namespace gsr {

GSR_BOUNDS_DECL(overlay)   // sites: 0 bin -> bin_start, 1 list position, 2 splat index in the list, 3 selection word, 4 LDS cell, 5 pixel

struct OverlayPixel {
    float T, S, r, g, b;
};

// one pixel's step of the recurrence for a fragment of weight B (negative: not a fragment); `selected` is uniform over the wave
__device__ __forceinline__ void overlay_step(OverlayPixel& p, float B, bool selected, float cr, float cg, float cb)
{
    if (B >= 0.0f) {
        const float w = p.T * B;
        p.T = p.T - w;
        if (selected) {
            p.S = p.S + w;
            p.r = __builtin_fmaf(w, cr, p.r);
            p.g = __builtin_fmaf(w, cg, p.g);
            p.b = __builtin_fmaf(w, cb, p.b);
        }
    }
}

// bit i of the selection words (a scene never selected in has none: the empty selection)
__device__ __forceinline__ bool overlay_selected(const OverlayBuffers& a, uint32_t i)
{
    if (!a.sel) return false;
    const uint32_t word = i >> 5;
    GSR_BOUND(overlay, 3, word, a.nwords);
    return word < a.nwords && ((a.sel[word] >> (i & 31u)) & 1u) != 0u;
}

template <bool SKIP, bool TRIM>
__global__ __launch_bounds__(DEPTH_THREADS) void k_overlay(OverlayBuffers a, BinGrid g, CamParams cam)
{
    __shared__ float4 s_a[DEPTH_CHUNK];       // ux, uy, ncu, wx
    __shared__ float4 s_b[DEPTH_CHUNK];       // wy, ncw, la, selected (bits: 0 / 1)
    __shared__ float4 s_c[DEPTH_CHUNK];       // the colour: r, g, b, -
    __shared__ uint32_t s_tiles[DEPTH_CHUNK]; // one bit per tile of the bin the entry can reach
    __shared__ uint32_t s_last;               // TRIM: entries of the list up to and including its last selected one

    // A frame whose lists did not fit published no work (k_bin_finalize): nothing of it is walked, nothing is written, and the
    // host learns at its next synchronisation that the image is not this frame's (k_depth_planes has the same rule).
    const bool unfit = *a.overflow != 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.invalid = unfit ? 1u : 0u;
    if (unfit) return;

    const int nbxb = g.bx_hi - g.bx_lo;
    const int bin = blockIdx.x;
    GSR_BOUND(overlay, 0, bin, nbxb * g.nby);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = lane & 7, ly = lane >> 3;
    const int by = bin / nbxb, bxl = bin - by * nbxb;
    const int binX0 = (g.bx_lo + bxl) * BIN_PX, binY0 = by * BIN_PX;
    const int ox = (wave & 1) * TILE, oy = (wave >> 1) * TILE;
    const float pxf0 = (float)(ox + lx), pxf1 = pxf0 + 8.0f;
    const float pyf0 = (float)(oy + ly), pyf1 = pyf0 + 8.0f;
    const float bx0c = (float)binX0 + 0.5f, by0c = (float)binY0 + 0.5f;

    const uint32_t list_end = min(a.bin_start[bin + 1], a.capacity), begin = min(a.bin_start[bin], list_end);
    GSR_BOUND(overlay, 1, a.bin_start[bin + 1], (unsigned long long)a.capacity + 1ull);
    GSR_BOUND(overlay, 1, a.bin_start[bin], (unsigned long long)a.bin_start[bin + 1] + 1ull);

    uint32_t end = list_end;
    if constexpr (TRIM) {
        if (threadIdx.x == 0) s_last = 0u;
        __syncthreads();
        uint32_t last = 0;   // of this wave's entries: the position behind the last selected one, counted from `begin`
        if (a.sel) {
            for (uint32_t base = begin; base < list_end; base += DEPTH_CHUNK) {
                const uint32_t e = base + threadIdx.x;
                bool in = false;
                if (e < list_end) {
                    GSR_BOUND(overlay, 1, e, a.capacity);
                    GSR_BOUND(overlay, 2, a.list[e], a.nsplats);
                    in = overlay_selected(a, min(a.list[e], a.nsplats - 1u));
                }
                const uint64_t bal = __ballot(in);
                if (bal) last = base - begin + (uint32_t)wave * WAVE + (64u - (uint32_t)__builtin_clzll(bal));   // (later chunks lie behind)
            }
        }
        if (lane == 0 && last) __hip_atomic_fetch_max(&s_last, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        end = begin + min(s_last, list_end - begin);
    }

    OverlayPixel p00{1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    OverlayPixel p10 = p00, p01 = p00, p11 = p00;   // pij: pixel (x + 8i, y + 8j)

    for (uint32_t base = begin; base < end; base += DEPTH_CHUNK) {
        __syncthreads();   // the previous chunk is consumed
        const uint32_t e = base + threadIdx.x;
        uint32_t tiles = 0;
        if (e < end) {
            GSR_BOUND(overlay, 1, e, a.capacity);
            GSR_BOUND(overlay, 2, a.list[e], a.nsplats);
            const uint32_t i = min(a.list[e], a.nsplats - 1u);
            const DepthEntry en = depth_entry(a.rec, a.px, a.py, a.pz, i, cam, bx0c, by0c);   // (its z is not used: the loads go)
            // the colour as k_blend's staging reads it
            const uint32_t rgb8 = a.rec[i].rgb8;
            float cr = (float)(rgb8 & 0xffu) * (1.0f / 255.0f), cg = (float)((rgb8 >> 8) & 0xffu) * (1.0f / 255.0f),
                  cb = (float)((rgb8 >> 16) & 0xffu) * (1.0f / 255.0f);
            if ((rgb8 & RGB8_IN_SHCOL) && a.shcol) {   // SH-coloured splat: the projection kernel evaluated its colour for this view
                const float4 sc = a.shcol[i];
                cr = sc.x; cg = sc.y; cb = sc.z;
            }
            s_a[threadIdx.x] = make_float4(en.ux, en.uy, en.ncu, en.wx);
            s_b[threadIdx.x] = make_float4(en.wy, en.ncw, en.la, __uint_as_float(overlay_selected(a, i) ? 1u : 0u));
            s_c[threadIdx.x] = make_float4(cr, cg, cb, 0.0f);
            tiles = SKIP ? depth_tile_reach(en, a.rec + i, binX0, binY0) : 0xfu;
        }
        s_tiles[threadIdx.x] = tiles;
        __syncthreads();

        const uint32_t cnt = min((uint32_t)DEPTH_CHUNK, end - base);
        for (uint32_t c0 = 0; c0 < cnt; c0 += WAVE) {
            // my tile's entries among these 64, in list order (entries behind the walk's end carry no bit)
            uint64_t bal = __ballot(((s_tiles[c0 + lane] >> wave) & 1u) != 0u);
            while (bal) {
                const uint32_t cell = c0 + (uint32_t)__builtin_ctzll(bal);
                bal &= bal - 1ull;
                GSR_BOUND(overlay, 4, cell, DEPTH_CHUNK);
                const float4 ra = s_a[cell], rb = s_b[cell];   // the same address in every lane: a broadcast
                DepthEntry en;
                en.ux = ra.x; en.uy = ra.y; en.ncu = ra.z; en.wx = ra.w; en.wy = rb.x; en.ncw = rb.y; en.la = rb.z; en.z = 0.0f;
                en.index = 0u;
                const bool selected = __float_as_uint(rb.w) != 0u;   // uniform: one entry per step
                float cr = 0.0f, cg = 0.0f, cb = 0.0f;
                if (selected) { const float4 rc = s_c[cell]; cr = rc.x; cg = rc.y; cb = rc.z; }
                const float ur0 = depth_row_u(en, pyf0), wr0 = depth_row_w(en, pyf0);
                const float ur1 = depth_row_u(en, pyf1), wr1 = depth_row_w(en, pyf1);
                overlay_step(p00, depth_weight(en, pxf0, ur0, wr0), selected, cr, cg, cb);
                overlay_step(p10, depth_weight(en, pxf1, ur0, wr0), selected, cr, cg, cb);
                overlay_step(p01, depth_weight(en, pxf0, ur1, wr1), selected, cr, cg, cb);
                overlay_step(p11, depth_weight(en, pxf1, ur1, wr1), selected, cr, cg, cb);
            }
        }
    }

    const int x0 = binX0 + ox + lx, x1 = x0 + 8, y0 = binY0 + oy + ly, y1 = y0 + 8;
    auto store = [&](int x, int y, const OverlayPixel& p) {
        if (x < g.W && y < g.H) {
            const size_t o = (size_t)y * g.W + x;
            GSR_BOUND(overlay, 5, o, (size_t)g.W * g.H);
            float4 v = a.fb[o];
            // (no selected fragment, or mix == 0: fb as it is, whatever its bits)
            if (a.mix != 0.0f && (p.S != 0.0f || p.r != 0.0f || p.g != 0.0f || p.b != 0.0f)) {
                v.x = __builtin_fmaf(a.mix, __builtin_fmaf(a.tint[0], p.S, -p.r), v.x);
                v.y = __builtin_fmaf(a.mix, __builtin_fmaf(a.tint[1], p.S, -p.g), v.y);
                v.z = __builtin_fmaf(a.mix, __builtin_fmaf(a.tint[2], p.S, -p.b), v.z);
            }
            a.overlay[o] = v;
            a.cover[o] = p.S;
        }
    };
    store(x0, y0, p00); store(x1, y0, p10); store(x0, y1, p01); store(x1, y1, p11);
}

void launch_overlay(const OverlayBuffers& b, const BinGrid& g, const CamParams& cam, bool skip, bool trim, hipStream_t s)
{
    const int nbins = (g.bx_hi - g.bx_lo) * g.nby;
    if (nbins <= 0) return;
    const dim3 grid(nbins), block(DEPTH_THREADS);
    if (skip) {
        if (trim) hipLaunchKernelGGL((k_overlay<true, true>), grid, block, 0, s, b, g, cam);
        else hipLaunchKernelGGL((k_overlay<true, false>), grid, block, 0, s, b, g, cam);
    } else {
        if (trim) hipLaunchKernelGGL((k_overlay<false, true>), grid, block, 0, s, b, g, cam);
        else hipLaunchKernelGGL((k_overlay<false, false>), grid, block, 0, s, b, g, cam);
    }
}

}  // namespace gsr
