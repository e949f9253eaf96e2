// The tile compositor's unit: the two-waves-per-tile kernels (k_blend2, k_blend2_unfused), the stand-alone fold (k_combine),
// the plan, the launch and the small framebuffer kernels.  The compositor itself -- staging, walk and fold -- is
// k_blend_body.h; its one-wave-per-tile kernels (k_blend, k_blend_unfused) are defined in k_blend1.hip, which is built with
// other flags, and reach the launch below through blend1_kernel().
#include "k_blend_body.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace gsr {

// two waves per tile: 512-thread workgroups, three per CU (6 waves per SIMD, 80 registers)
__global__ __launch_bounds__(2 * BLEND_THREADS) __attribute__((amdgpu_waves_per_eu(6, 6))) void k_blend2(GSR_BLEND_PARAMS)
{
    blend_body<2, true>(GSR_BLEND_ARGS);
}
// the same with the partials left to k_combine (GSR_FUSE_COMBINE=0; test reference)
__global__ __launch_bounds__(2 * BLEND_THREADS) __attribute__((amdgpu_waves_per_eu(6, 6))) void k_blend2_unfused(GSR_BLEND_PARAMS)
{
    blend_body<2, false>(GSR_BLEND_ARGS);
}

// The diagnostic builds' readers: this unit's copy of the words merged with k_blend1.hip's (k_blend_body.h).  Counters add up;
// of stamps, which a wave overwrites, the words of the kernel that ran (a process that ran both forms: k_blend's where it
// wrote, k_blend2's elsewhere).
#if defined(GSR_BOUNDS) || defined(GSR_BLEND_STAMPS)
template <size_t N>
static int read_blend_words(int which, const unsigned int (&symbol)[N], unsigned int* out, bool add)
{
    std::vector<unsigned int> other(N);
    if (hipMemcpyFromSymbol(out, symbol, sizeof symbol) != hipSuccess || blend1_read_words(which, other.data()) != 0) return -1;
    for (size_t k = 0; k < N; k++) out[k] = add ? out[k] + other[k] : other[k] ? other[k] : out[k];
    return 0;
}
#endif
#ifdef GSR_BOUNDS
extern "C" int gsr_debug_bounds_blend(unsigned int* out) { return read_blend_words(BLEND_WORDS_BOUNDS, g_bounds_blend, out, true); }
#endif
#ifdef GSR_BLEND_STAMPS
extern "C" int gsr_debug_blend_stamps(unsigned int* out /* 4096*4*16 */) { return read_blend_words(BLEND_WORDS_STAMPS, g_blend_stamps, out, false); }
extern "C" int gsr_debug_bin_info(unsigned int* out /* 16384*8 */) { return read_blend_words(BLEND_WORDS_BIN_INFO, g_bin_info, out, false); }
#endif

// Fold the per-segment partials of every multi-segment bin, front to back -- the stand-alone form (BlendPlan::separate_fold);
// by default the fold runs inside k_blend and this kernel is not launched.  A thread folds its four
// pixels as four independent chains and the segment loop is unrolled, so 16 loads are in flight per
// thread: the kernel is a latency-bound read of the partials (85 MB on C3 with 512-entry segments).
__global__ __launch_bounds__(BLEND_THREADS) void k_combine(const uint32_t* __restrict__ seg_start,
                                                           const float4* __restrict__ partial, float4* __restrict__ fb,
                                                           BinGrid g)
{
    const int nbxb = g.bx_hi - g.bx_lo;
    const int bin = blockIdx.x;
    const uint32_t s0 = seg_start[bin], nseg = seg_start[bin + 1] - s0;
    if (nseg <= 1) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int by = bin / nbxb, bxl = bin - by * nbxb;
    const int X0 = (g.bx_lo + bxl) * BIN_PX + (wave & 1) * TILE, Y0 = by * BIN_PX + (wave >> 1) * TILE;
    const int lx = lane & 7, ly = lane >> 3;
    const float4* p = partial + (size_t)s0 * BIN_PIXELS + wave * (TILE * TILE) + lane;
    float r[4] = {0.f, 0.f, 0.f, 0.f}, gg[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f}, T[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll 4
    for (uint32_t k = 0; k < nseg; k++) {
        float4 v[4];
#pragma unroll
        for (int slot = 0; slot < 4; slot++) v[slot] = p[(size_t)k * BIN_PIXELS + slot * 64];
#pragma unroll
        for (int slot = 0; slot < 4; slot++) {
            r[slot] = __builtin_fmaf(T[slot], v[slot].x, r[slot]);
            gg[slot] = __builtin_fmaf(T[slot], v[slot].y, gg[slot]);
            b[slot] = __builtin_fmaf(T[slot], v[slot].z, b[slot]);
            T[slot] = T[slot] * v[slot].w;
        }
    }
#pragma unroll
    for (int slot = 0; slot < 4; slot++) {
        const int x = X0 + lx + 8 * (slot & 1), y = Y0 + ly + 8 * (slot >> 1);
        if (x < g.W && y < g.H) fb[(size_t)y * g.W + x] = make_float4(r[slot], gg[slot], b[slot], 1.0f - T[slot]);
    }
}

// ---------------------------------------------------------------------------
// The plan: which of the four kernels above a frame runs, on what grid, and how k_bin_finalize cuts the bin lists into its work
// items (BlendPlan, gsr_internal.h).  Every threshold and per-kind figure lives here and nowhere else; alloc_bins allocates by
// the answer, launch_bin hands k_bin_finalize its policy and launch_blend launches by it.
// ---------------------------------------------------------------------------
// Compositor work-item granularity: list entries per (bin, segment) item.  SEG_LEN_WHOLE_BIN (gsr_internal.h) = one item per
// bin, which early termination needs (a segment cannot see whether earlier ones saturated the bin).
constexpr uint32_t SEG_LEN_MIN = 512;            // shortest segment; k_bin_finalize lengthens it so that the frame is cut
                                                 // into about SEG_TARGET_* full segments (multiples of 256 entries)
constexpr uint32_t SEG_TARGET_EXACT = 5000;      // one frame at a time: concurrency from the frame's own segments (C3: 512)
constexpr uint32_t SEG_TARGET_THROUGHPUT = 1300; // GSR_FLAG_THROUGHPUT: concurrency comes from the other frames in flight
                                                 // (C3: 2048-entry segments; a 1/8-screen band stays at 512)
// Persistent compositor workgroups per CU.  k_blend is built for 7 waves per SIMD (72 VGPRs), so 7 four-wave
// workgroups are resident per CU and the grid must not exceed that: a workgroup that is not resident at launch still
// owns its first work item by index (a heavy one: the queue is ordered heaviest first) and starts it only when a
// resident workgroup exits.  With 8 per CU, one item in eight began at 222 us of a 270 us kernel (in-kernel stamps,
// scripts/blend_stamps.py): k_blend 271 -> 252 us on C3 at 7 per CU.
constexpr uint32_t BLEND_WG_PER_CU_EXACT = 7;
// Contexts that overlap with others' kernels (GSR_FLAG_THROUGHPUT): 6 per CU left a wave slot per SIMD to the other
// contexts and was best while the fold of the partials was a kernel of its own; with the fold inside k_blend 7 is
// (bench.py, three frames in flight, C3: 3324 -> 3400 frames/s, reproducible; C2 -0.8 %, C4 and early-out unchanged).
constexpr uint32_t BLEND_WG_PER_CU_THROUGHPUT = 7;
// Two waves per tile (k_blend2, 512-thread workgroups): three workgroups per CU are resident (6 waves per SIMD).
constexpr uint32_t BLEND_WG_PER_CU_SUB2 = 3;
// Waves per tile.  Two (k_blend2) halve a wave's serial walk over a work item -- the pole of a frame rendered alone, where a
// wave needs ~560 cycles per entry visit whatever else the chip does -- and pay with occupancy (24 instead of 28 waves
// per CU) and saturation tests at chunk instead of 64-entry boundaries.  Measured one frame at a time: C3 k_blend 194 ->
// 147 us, C1 20 -> 15; C2 (short segments) 77 -> 86, with 1024-entry segments 80; C4, whose 8160 bins keep every slot
// busy: 412 -> 509; three frames in flight, C3: 5280 -> 4410 frames/s.  So: contexts that render one frame at a time, up
// to SUB2_MAX_BINS bins, with segments of at least 1024 entries.  (Leaving the choice to k_bin_finalize per frame --
// both kernels launched, the other one returning at once -- cost 4.5 us per frame for the idle launch.)
constexpr uint32_t SUB2_MAX_BINS = 4096, SEG_LEN_MIN_SUB2 = 1024;

// Work-item length.  With the saturation skip of k_blend a work item ends as soon as nothing it could still add can change
// a bit of its pixels, and that needs the item to contain the splats that saturate it: a bin cut into 512-entry segments
// never saturates inside one of them (every segment starts from transmittance 1), a bin processed as one item stops
// after the few thousand entries that matter (C3: 3430 -> 4990 frames/s with three frames in flight, 2670 -> 2945 one at
// a time; C4: 292 -> 856).  Where the scene does not saturate (C2: small splats, 9 % of the entries skipped against 53 %
// on C3 and 85 % on C4; or any thin, low-opacity scene) long items only cost balance (C2: 6670 -> 2780 frames/s).
// k_bin_finalize decides per frame, from a figure the projection already has: the frame's optical depth
//     tau = sum over visible splats of opacity x (16x16 tiles its box overlaps) x 256 / pixels
// (C1 14, C2 74, C3 362, C4 1090): items are at least SEG_LEN_LONG entries (in practice whole bins) from LONG_TAU_* on.
// A function of the frame alone: no feedback from earlier frames, the same frame always takes the same path.
// Where long items start to pay (scripts/tau_crossover.py: the C3 and C2 generators at 0.25 .. 1.6 M splats, 1080p): with
// other frames' kernels filling the gaps, between tau 90 and 145 for both generators (tau 90: 10 390 -> 10 080 frames/s,
// tau 145: 7350 -> 8640, tau 250: 4730 -> 6800); one frame at a time the few long items are the frame's tail and the
// crossover depends on the scene (C3 generator: tau ~ 255, C3 itself +23 %; the C2 generator's small splats still lose
// 8 % at tau 390), so the threshold there stays high.
constexpr uint32_t SEG_LEN_LONG = 32768;   // (16384: C4 k_blend 437 instead of 405 us -- its heaviest bins hold 50-100 k entries; 65536 measures the same)
constexpr uint32_t LONG_TAU_EXACT = 340, LONG_TAU_THROUGHPUT = 120;
// a frame that is not dense as a whole: bins far past saturation become one item only where a list entry carries at least this
// optical mass (pixels): C3 14, C2 8, 2 M tiny splats 1.9 -- one frame at a time a 3000-entry serial walk is the frame's tail
constexpr uint32_t LONG_MASS_MIN_EXACT = 12, LONG_MASS_MIN_THROUGHPUT = 0;
constexpr uint32_t LONG_TILES_X2_EXACT = 9;   // one frame at a time: and at least 4.5 tiles per visible splat (k_bin_finalize)
constexpr uint32_t LONG_TILES_X2_THROUGHPUT = 6;   // with frames in flight: 3 (scripts/policy_check.py: 2 M tiny splats, 1.9 tiles each, tau 264:
                                                   // long items -26 %; the C2 generator, 3.6 tiles each: +10 % at the same tau)

BlendPlan plan_blend(uint32_t nbins, uint32_t npix, uint32_t capacity, int cu_count, bool throughput, bool early_out, uint32_t allocated_items,
                     const BlendKnobs& k)
{
    BlendPlan p;
    memset(&p, 0, sizeof p);
    p.waves_per_tile = k.blend_sub >= 2 ? 2u : k.blend_sub == 1 ? 1u : (!throughput && nbins <= SUB2_MAX_BINS) ? 2u : 1u;
    p.threads = (uint32_t)BLEND_THREADS * p.waves_per_tile;
    const uint32_t wg_per_cu = p.waves_per_tile == 2 ? BLEND_WG_PER_CU_SUB2 : throughput ? BLEND_WG_PER_CU_THROUGHPUT : BLEND_WG_PER_CU_EXACT;
    p.grid = k.blend_grid ? k.blend_grid : wg_per_cu * (uint32_t)std::max(cu_count, 1);
    // early termination composites whole bins whatever GSR_SEG_LEN says
    p.seg_len = early_out ? SEG_LEN_WHOLE_BIN : k.seg_len ? k.seg_len : p.waves_per_tile == 2 ? SEG_LEN_MIN_SUB2 : SEG_LEN_MIN;
    p.whole_bin = is_whole_bin(p.seg_len) ? 1u : 0u;
    p.seg_target_items = k.seg_target ? k.seg_target : throughput ? SEG_TARGET_THROUGHPUT : SEG_TARGET_EXACT;
    // segments = work items (each may need a partial slot): one per bin plus one per seg_len entries
    const uint32_t want_items = nbins + capacity / p.seg_len + 16;
    p.max_items = allocated_items ? std::max(allocated_items, want_items) : want_items;
    p.partial_slots = p.whole_bin ? 0u : p.max_items;
    p.queue_start = std::min(p.max_items, p.grid);
    p.fused = k.fuse_combine ? 1u : 0u;
    p.separate_fold = (!p.fused && !p.whole_bin) ? 1u : 0u;
    // work items heaviest first (one frame at a time) or in raster order
    p.items_by_size = k.items_by_size >= 0 ? k.items_by_size : throughput ? 0 : 1;
    p.long_policy = p.whole_bin ? 0 : k.long_items >= 0 ? k.long_items : k.saturate ? -1 : 0;
    p.seg_len_long = SEG_LEN_LONG;
    p.long_tau = throughput ? LONG_TAU_THROUGHPUT : LONG_TAU_EXACT;
    p.long_tiles_x2 = throughput ? LONG_TILES_X2_THROUGHPUT : LONG_TILES_X2_EXACT;
    p.long_tau_bin = k.long_tau;
    p.long_mass_min = throughput ? LONG_MASS_MIN_THROUGHPUT : LONG_MASS_MIN_EXACT;
    p.npix = npix;
    p.saturate = k.saturate ? 1u : 0u;
    return p;
}

// The plan for tests (tests/test_blend_plan.py): no context and no device, so it answers wherever the library loads.  Returns
// sizeof(BlendPlan), for the caller to check its idea of the layout against.
extern "C" int gsr_debug_blend_plan(unsigned int nbins, unsigned int npix, unsigned int capacity, int cu_count, int throughput, int early_out,
                                     unsigned int allocated_items, int fuse_combine, int saturate, int items_by_size, int long_items, unsigned int long_tau,
                                     int blend_sub, unsigned int seg_target, unsigned int blend_grid, unsigned int seg_len, BlendPlan* out)
{
    *out = plan_blend(nbins, npix, capacity, cu_count, throughput != 0, early_out != 0, allocated_items,
                      BlendKnobs{fuse_combine ? 1u : 0u, saturate ? 1u : 0u, items_by_size, long_items, long_tau, blend_sub, seg_target, blend_grid, seg_len});
    return (int)sizeof(BlendPlan);
}

// Every instantiation of the compositor, once: the launch walks this table.  (One wave per tile: k_blend1.hip's kernels, handed
// over by their own unit -- this one never takes the address of a __global__ it does not define.)
struct BlendKernel { BlendFn fn; uint32_t waves_per_tile; bool fused; uint32_t threads; };
static const BlendKernel BLEND_KERNELS[] = {
    {blend1_kernel(true), 1, true, BLEND_THREADS},
    {k_blend2, 2, true, 2 * BLEND_THREADS},
    {blend1_kernel(false), 1, false, BLEND_THREADS},
    {k_blend2_unfused, 2, false, 2 * BLEND_THREADS},
};

void launch_blend(const BlendBuffers& b, const BinGrid& g, float early_out_eps, hipStream_t s, hipEvent_t between)
{
    const BlendPlan& p = b.plan;
    const int nbins = (g.bx_hi - g.bx_lo) * g.nby;
    if (nbins <= 0) return;
    for (const BlendKernel& k : BLEND_KERNELS)
        if (k.waves_per_tile == p.waves_per_tile && k.fused == (p.fused != 0u))
            hipLaunchKernelGGL(k.fn, dim3(p.queue_start), dim3(k.threads), 0, s, b.items, b.seg_start, b.bin_start, b.list, b.rec, b.shcol, b.fb,
                               b.partial, b.queue, g, early_out_eps, b.seg_len_dev, b.capacity, b.nsplats, b.bin_mask, p.saturate);
    if (between) (void)hipEventRecord(between, s);
    if (p.separate_fold)
        hipLaunchKernelGGL(k_combine, dim3(nbins), dim3(BLEND_THREADS), 0, s, b.seg_start, (const float4*)b.partial, b.fb, g);
}

__global__ void k_clear_fb(float4* fb, uint32_t npix)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npix) fb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

void launch_clear_fb(float4* fb, int32_t W, int32_t H, hipStream_t s)
{
    const uint32_t npix = (uint32_t)W * (uint32_t)H;
    if (!npix) return;
    hipLaunchKernelGGL(k_clear_fb, dim3((npix + 255) / 256), dim3(256), 0, s, fb, npix);
}

// round(clamp(x, 0, 1) * 255) per channel (Appendix A of SURVEY.md: output framebuffer contract)
__global__ void k_to_rgba8(const float4* __restrict__ fb, uint32_t* __restrict__ out, uint32_t npix)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    out[i] = to_rgba8(fb[i]);
}

// Multi-GPU exchange, sender side: the band's columns [x0, x1) as RGBA8 straight into the all-gather slab
// ([H][slab_w] pixels), one pass over the band instead of a whole-frame conversion plus a strided copy.
// `overflow` (may be null: the harness's own slabs carry no flag): the frame's overflow word.  A frame whose bin lists did not
// fit was not composited -- the band about to be packed is the PRECEDING image -- and the slab says so in SLAB_FLAG_WORDS
// words behind its pixels, which travel with it through the all-gather: every rank of the group then sees, for the same
// gathered frame, that one of its bands is stale (k_unpack_slabs_rgba8) and refuses it -- a group-wide decision, so that no
// rank redoes a collective alone.
__global__ void k_pack_band_rgba8(const float4* __restrict__ fb, uint32_t* __restrict__ slab, int W, int H, int x0, int x1,
                                  int slab_w, const uint32_t* __restrict__ overflow)
{
    if (overflow && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < SLAB_FLAG_WORDS)
        slab[(size_t)H * slab_w + threadIdx.x] = *overflow != 0u ? 1u : 0u;
    const int x = x0 + blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= x1) return;
    slab[(size_t)y * slab_w + (x - x0)] = to_rgba8(fb[(size_t)y * W + x]);
}

void launch_pack_band_rgba8(const float4* fb, uint32_t* slab, int W, int H, int x0, int x1, int slab_w, hipStream_t s, const uint32_t* overflow)
{
    if (x1 <= x0 || H <= 0) return;
    hipLaunchKernelGGL(k_pack_band_rgba8, dim3((x1 - x0 + 255) / 256, H), dim3(256), 0, s, fb, slab, W, H, x0, x1, slab_w, overflow);
}

// Receiver side: the gathered slabs [world][H][slab_w] -> one row-major [H][W] image.
// `stale` (may be null; then the slabs carry no flag words): out, one bit per rank whose band was not composited (see
// k_pack_band_rgba8) -- the same word on every rank of the group.
// `slab_stride` (words; 0: pixels and flag words and nothing else): from one rank's slab to the next, where the slabs carry a
// depth section behind the flag words (gsr_comm_set_depth).
__global__ void k_unpack_slabs_rgba8(const uint32_t* __restrict__ gathered, uint32_t* __restrict__ image, int W, int H,
                                     int slab_w, int world, SlabEdges e, uint32_t* __restrict__ stale, size_t slab_stride)
{
    const size_t slab_words = slab_stride ? slab_stride : (size_t)H * slab_w + (stale ? SLAB_FLAG_WORDS : 0);
    if (stale && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        uint32_t bits = 0;
        for (int q = 0; q < world; q++)
            if (gathered[(size_t)q * slab_words + (size_t)H * slab_w] != 0u) bits |= 1u << q;
        *stale = bits;
    }
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    uint32_t v = 0;
    for (int q = 0; q < world; q++)
        if (x >= e.x0[q] && x < e.x1[q]) v = gathered[(size_t)q * slab_words + (size_t)y * slab_w + (x - e.x0[q])];
    image[(size_t)y * W + x] = v;
}

void launch_unpack_slabs_rgba8(const uint32_t* gathered, uint32_t* image, int W, int H, int slab_w, int world,
                               const SlabEdges& e, hipStream_t s, uint32_t* stale, size_t slab_stride)
{
    if (W <= 0 || H <= 0) return;
    hipLaunchKernelGGL(k_unpack_slabs_rgba8, dim3((W + 255) / 256, H), dim3(256), 0, s, gathered, image, W, H, slab_w, world, e, stale, slab_stride);
}

void launch_to_rgba8(const float4* fb, uint32_t* out, uint32_t npix, hipStream_t s)
{
    if (!npix) return;
    hipLaunchKernelGGL(k_to_rgba8, dim3((npix + 255) / 256), dim3(256), 0, s, fb, out, npix);
}

}  // namespace gsr
