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
// k_overlay is the walk of one bin (k_depth_walk.h) with OverlayPass.  Staging adds the entry's colour and its selection bit to the
// cell; the visited cell is read at one address by every lane (a broadcast), and whether it is selected is uniform over the wave.
// TRIM: entries behind the list's last selected entry change T only, which is not a result, so the workgroup first finds that entry
// (one pass over list[] and the mask: a ballot per wave, a maximum in LDS) and walks [begin, last + 1): nothing at all in a bin
// without a selected entry.  The same bits with and without (GSR_OVERLAY_TRIM=0).
//
// Compiled with -ffp-contract=off like the rest of the device code: the fused multiply-adds are the explicit ones.
#include "k_depth_walk.h"

namespace gsr {

GSR_BOUNDS_DECL(overlay)   // sites: 0 - 3 the walk's (WALK_SITE_*), 4 selection word, 5 pixel; the outline's: 6 bit-plane word, 7 pixel
struct OverlayBounds {
    static __device__ __forceinline__ void bound(int site, unsigned long long idx, unsigned long long limit) { GSR_BOUND(overlay, site, idx, limit); }
};

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
    GSR_BOUND(overlay, 4, word, a.nwords);
    return word < a.nwords && ((a.sel[word] >> (i & 31u)) & 1u) != 0u;
}

// The pass of the walk: a cell holds the selection bit (0 / 1) in its spare word and the colour beside it; a visit is the recurrence
// at the lane's pixels pij = (x + 8i, y + 8j).
struct OverlayPass : OverlayBounds {
    float4* s_c;   // the colour: r, g, b, -
    const OverlayBuffers& a;
    float pxf0, pxf1, pyf0, pyf1;
    OverlayPixel &p00, &p10, &p01, &p11;   // the kernel's own locals: its stores read them

    __device__ __forceinline__ float stage(const DepthEntry& en)   // (the entry's z is not used: the loads go)
    {
        const uint32_t i = en.index;
        // the colour as k_blend's staging reads it
        const uint32_t rgb8 = a.rec[i].rgb8;
        float cr = (float)(rgb8 & 0xffu) * (1.0f / 255.0f), cg = (float)((rgb8 >> 8) & 0xffu) * (1.0f / 255.0f),
              cb = (float)((rgb8 >> 16) & 0xffu) * (1.0f / 255.0f);
        if ((rgb8 & RGB8_IN_SHCOL) && a.shcol) {   // SH-coloured splat: the projection kernel evaluated its colour for this view
            const float4 sc = a.shcol[i];
            cr = sc.x; cg = sc.y; cb = sc.z;
        }
        s_c[threadIdx.x] = make_float4(cr, cg, cb, 0.0f);
        return __uint_as_float(overlay_selected(a, i) ? 1u : 0u);
    }
    __device__ __forceinline__ void visit(uint32_t cell, const DepthEntry& en)
    {
        const bool selected = __float_as_uint(en.z) != 0u;   // uniform: one entry per step
        float cr = 0.0f, cg = 0.0f, cb = 0.0f;
        if (selected) { const float4 rc = s_c[cell]; cr = rc.x; cg = rc.y; cb = rc.z; }
        const float ur0 = depth_row_u(en, pyf0), wr0 = depth_row_w(en, pyf0);
        const float ur1 = depth_row_u(en, pyf1), wr1 = depth_row_w(en, pyf1);
        overlay_step(p00, depth_weight(en, pxf0, ur0, wr0), selected, cr, cg, cb);
        overlay_step(p10, depth_weight(en, pxf1, ur0, wr0), selected, cr, cg, cb);
        overlay_step(p01, depth_weight(en, pxf0, ur1, wr1), selected, cr, cg, cb);
        overlay_step(p11, depth_weight(en, pxf1, ur1, wr1), selected, cr, cg, cb);
    }
};

template <bool SKIP, bool TRIM>
__global__ __launch_bounds__(DEPTH_THREADS) void k_overlay(OverlayBuffers a, BinGrid g, CamParams cam)
{
    __shared__ WalkStage st;
    __shared__ float4 s_c[DEPTH_CHUNK];
    __shared__ uint32_t s_last;   // TRIM: entries of the list up to and including its last selected one
    if (walk_frame_unfit(a.overflow, a.invalid)) return;

    const WalkBin w = walk_bin<OverlayBounds>(a, g, blockIdx.x);
    uint32_t end = w.end;
    if constexpr (TRIM) {
        if (threadIdx.x == 0) s_last = 0u;
        __syncthreads();
        uint32_t last = 0;   // of this wave's entries: the position behind the last selected one, counted from the list's begin
        if (a.sel) {
            for (uint32_t base = w.begin; base < w.end; base += DEPTH_CHUNK) {
                const uint32_t e = base + threadIdx.x;
                const bool in = e < w.end && overlay_selected(a, walk_list_entry<OverlayBounds>(a, e));
                const uint64_t bal = __ballot(in);
                if (bal) last = base - w.begin + (uint32_t)w.wave * WAVE + (64u - (uint32_t)__builtin_clzll(bal));   // (later chunks lie behind)
            }
        }
        if (w.lane == 0 && last) __hip_atomic_fetch_max(&s_last, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        end = w.begin + min(s_last, w.end - w.begin);
    }

    const float pxf0 = (float)(w.ox + w.lx), pyf0 = (float)(w.oy + w.ly);
    OverlayPixel p00{1.0f, 0.0f, 0.0f, 0.0f, 0.0f}, p10 = p00, p01 = p00, p11 = p00;
    OverlayPass pass{{}, s_c, a, pxf0, pxf0 + 8.0f, pyf0, pyf0 + 8.0f, p00, p10, p01, p11};
    walk_bin_list<SKIP>(st, a, w, cam, w.begin, end, pass);

    const int x0 = w.binX0 + w.ox + w.lx, x1 = x0 + 8, y0 = w.binY0 + w.oy + w.ly, y1 = y0 + 8;
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
    if (skip) walk_launch(trim ? k_overlay<true, true> : k_overlay<true, false>, b, g, cam, s);
    else walk_launch(trim ? k_overlay<false, true> : k_overlay<false, false>, b, g, cam, s);
}

// ---- selection outline --------------------------------------------------------------------------------------------------------
// The edge of inside = { cover >= threshold } within the domain (the band's columns inside the image, every row), drawn into the
// overlay image behind k_overlay, in place ("Selection overlay"):
//     outer: edge(p) = !inside(p), and a q of the domain with inside(q) lies within (qx - px)^2 + (qy - py)^2 <= width^2
//     inner: the same with inside and !inside exchanged
//     at an edge pixel, k = 1 - alpha:  out.rgb = fma(ov.rgb, k, rgb * alpha),  out.a = fma(ov.a, k, alpha)
// Both sides are one dilation: with SOURCE = inside (outer) or domain & !inside (inner), edge = domain & !SOURCE & dilate(SOURCE).
// k_outline_bits ballots SOURCE into a bit plane, one 64-bit word per 64 pixels of a row (bit x & 63 of word (y, x >> 6); columns
// outside the domain give 0).  k_outline_apply, one wave per word, folds the rows y - width .. y + width around it from the centre
// outwards -- F_0 = row y, F_d = dilate(F_{d-1}, hw[d-1] - hw[d]) | row (y + d) | row (y - d), so that a row d away ends up
// spread by hw[d], the disc's half-width there -- on three wave-uniform words (wx - 1, wx, wx + 1: width <= 16 never reaches past
// them), and only the lanes whose edge bit is set read and rewrite their pixel.  An edge bit depends on cover alone, so writing
// the image in place is safe.  A pass that refused its frame (the invalid word) draws nothing.
constexpr int OUTLINE_THREADS = 256, OUTLINE_WAVES = OUTLINE_THREADS / WAVE;   // sites: 6 a word of the bit plane, 7 a pixel

// the domain's bits of word wx: the columns [x_lo, x_hi) that fall into [64 wx, 64 wx + 64)
__device__ __forceinline__ uint64_t outline_domain(const OutlineArgs& a, int wx)
{
    const int lo = max(a.x_lo - wx * 64, 0), hi = min(a.x_hi - wx * 64, 64);
    if (hi <= lo) return 0ull;
    return (hi >= 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
}

// the word this wave owns (uniform), false behind the plane's last one
__device__ __forceinline__ bool outline_word(const OutlineArgs& a, int& nw, uint32_t& word)
{
    nw = (a.W + 63) >> 6;
    word = blockIdx.x * (uint32_t)OUTLINE_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return word < (uint32_t)nw * (uint32_t)a.H;
}

__global__ __launch_bounds__(OUTLINE_THREADS) void k_outline_bits(OutlineArgs a)
{
    if (*a.invalid != 0u) return;
    int nw; uint32_t word;
    if (!outline_word(a, nw, word)) return;
    const int y = (int)(word / (uint32_t)nw), wx = (int)word - y * nw, lane = threadIdx.x & 63, x = wx * 64 + lane;
    bool source = false;
    if (x >= a.x_lo && x < a.x_hi) {
        const size_t o = (size_t)y * a.W + x;
        GSR_BOUND(overlay, 7, o, (size_t)a.W * a.H);
        const bool inside = a.cover[o] >= a.threshold;   // (a NaN is not inside)
        source = inside != (a.side == OUTLINE_INNER);
    }
    const uint64_t bal = __ballot(source);
    if (lane == 0) {
        GSR_BOUND(overlay, 6, word, (size_t)nw * a.H);
        a.bits[word] = bal;
    }
}

__global__ __launch_bounds__(OUTLINE_THREADS) void k_outline_apply(OutlineArgs a)
{
    if (*a.invalid != 0u) return;
    int nw; uint32_t word;
    if (!outline_word(a, nw, word)) return;
    const int y = (int)(word / (uint32_t)nw), wx = (int)word - y * nw, lane = threadIdx.x & 63;
    uint64_t l = 0ull, c = 0ull, r = 0ull;   // F of the words wx - 1, wx, wx + 1
    auto fold_row = [&](int yy) {            // rows outside the image are outside the domain
        if (yy < 0 || yy >= a.H) return;
        const size_t at = (size_t)yy * nw + wx;
        GSR_BOUND(overlay, 6, at, (size_t)nw * a.H);
        c |= a.bits[at];
        if (wx > 0) l |= a.bits[at - 1];
        if (wx + 1 < nw) r |= a.bits[at + 1];
    };
    fold_row(y);
    const uint64_t own = c;
    for (int d = 1; d <= a.width; d++) {
        for (int s = (int)a.hw[d - 1] - (int)a.hw[d]; s > 0; s--) {   // one column to either side per step
            const uint64_t nl = l | (l << 1) | (l >> 1) | (c << 63);
            const uint64_t nc = c | (c << 1) | (c >> 1) | (l >> 63) | (r << 63);
            const uint64_t nr = r | (r << 1) | (r >> 1) | (c >> 63);
            l = nl; c = nc; r = nr;
        }
        fold_row(y + d);
        fold_row(y - d);
    }
    const uint64_t edge = outline_domain(a, wx) & ~own & c;
    if ((edge >> lane) & 1ull) {
        const size_t o = (size_t)y * a.W + (size_t)(wx * 64 + lane);
        GSR_BOUND(overlay, 7, o, (size_t)a.W * a.H);
        float4 v = a.overlay[o];
        const float k = 1.0f - a.alpha;
        v.x = __builtin_fmaf(v.x, k, a.rgb[0] * a.alpha);
        v.y = __builtin_fmaf(v.y, k, a.rgb[1] * a.alpha);
        v.z = __builtin_fmaf(v.z, k, a.rgb[2] * a.alpha);
        v.w = __builtin_fmaf(v.w, k, a.alpha);
        a.overlay[o] = v;
    }
}

void launch_outline(const OutlineArgs& a, hipStream_t s)
{
    const size_t words = outline_words(a.W) * (size_t)a.H;
    if (!words) return;
    const uint32_t blocks = (uint32_t)((words + OUTLINE_WAVES - 1) / OUTLINE_WAVES);
    k_outline_bits<<<blocks, OUTLINE_THREADS, 0, s>>>(a);
    k_outline_apply<<<blocks, OUTLINE_THREADS, 0, s>>>(a);
}

}  // namespace gsr
