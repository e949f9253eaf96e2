// The passes that walk the last frame's bin lists once more (k_depth.hip: depth planes and picking; k_contrib.hip: per-splat
// contribution; k_overlay.hip: the selection overlay), stated once.  Device code, and at the end the one host function that launches
// such a pass (walk_launch).  Two halves:
//
// The per-fragment arithmetic: an entry as the walk reads it, the weight B of a fragment at a pixel, the row terms, and the
// staging-time test of which 16x16 tiles of the bin an entry can reach.  For a pixel, its fragments are the entries of its bin's
// list, in list order, that pass the compositor's coverage test (|vPosition|^2 <= 4, the same f32 expression as k_blend's walk),
// with weight B = exp2(-q log2(e) + log2(opacity)); sequentially, from T = 1:  w = T * B;  T = T - w.
//
// The walk of one bin (walk_bin, walk_bin_list, at the end): ONE skeleton -- a 256-thread workgroup per bin, chunks of DEPTH_CHUNK
// entries staged into LDS, one wave per 16x16 tile, a ballot over the staged tile masks gives list order, the visited cell is read
// at one address by every lane -- and the passes that supply only what is their own: what else a cell holds, what a wave does with
// a visited entry, their pixels and their stores (k_depth_planes, k_overlay).  k_pick (one wave per pixel) and k_contrib (its flush and
// barrier scheme) keep loops of their own over walk_bin and walk_list_entry.
//
// Compiled with -ffp-contract=off like the rest of the device code: the fused multiply-adds are the explicit ones.
#pragma once
#include "gsr_internal.h"

namespace gsr {

constexpr int DEPTH_THREADS = 256;
constexpr int DEPTH_CHUNK = DEPTH_THREADS;
constexpr float DEPTH_LOG2E = 1.4426950408889634f;

// One entry as the walk reads it: the record folded to bin-relative form (k_blend's staging: o = centre of the bin's first pixel),
// the splat's depth and its index.
struct DepthEntry {
    float ux, uy, ncu, wx, wy, ncw, la, z;
    uint32_t index;
};

// z of a splat: w of projection * (view * (x, y, z, 1)), k_project_key's sums term by term
__device__ __forceinline__ float depth_of(const CamParams& cam, float x, float y, float z)
{
    float camv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float s = cam.view[0 * 4 + r] * x;
        s = s + cam.view[1 * 4 + r] * y;
        s = s + cam.view[2 * 4 + r] * z;
        s = s + cam.view[3 * 4 + r];
        camv[r] = s;
    }
    float s = cam.proj[0 * 4 + 3] * camv[0];
    s = s + cam.proj[1 * 4 + 3] * camv[1];
    s = s + cam.proj[2 * 4 + 3] * camv[2];
    s = s + cam.proj[3 * 4 + 3] * camv[3];
    return s;
}

__device__ __forceinline__ DepthEntry depth_entry(const Record* __restrict__ rec, const float* __restrict__ px, const float* __restrict__ py,
                                                  const float* __restrict__ pz, uint32_t i, const CamParams& cam, float bx0c, float by0c)
{
    const float4* rp = reinterpret_cast<const float4*>(rec + i);
    const float4 ra = rp[0], rb = rp[1];   // (cx, cy, ux, uy), (wx, wy, la, rgb8)
    const float cxr = ra.x - bx0c, cyr = ra.y - by0c;
    DepthEntry e;
    e.ux = ra.z; e.uy = ra.w; e.ncu = -__builtin_fmaf(ra.w, cyr, ra.z * cxr);
    e.wx = rb.x; e.wy = rb.y; e.ncw = -__builtin_fmaf(rb.y, cyr, rb.x * cxr);
    e.la = rb.z;
    e.z = depth_of(cam, px[i], py[i], pz[i]);
    e.index = i;
    return e;
}

// THE per-fragment arithmetic, in two steps so that k_pick can evaluate the weights of 64 entries across its lanes and still
// apply them one after the other: the weight B of an entry at the pixel (pxf, pyf) (bin-relative, small exact integers), or a
// negative value where the fragment is discarded ...
__device__ __forceinline__ float depth_weight(const DepthEntry& e, float pxf, float ur, float wr)
{
    const float vx = __builtin_fmaf(e.ux, pxf, ur), vy = __builtin_fmaf(e.wx, pxf, wr);
    const float q = __builtin_fmaf(vy, vy, vx * vx);
    return q <= 4.0f ? __builtin_amdgcn_exp2f(__builtin_fmaf(q, -DEPTH_LOG2E, e.la)) : -1.0f;
}
// the row terms of vPosition, shared by the pixels of a row: uy * py - dot(u, c), wy * py - dot(w, c)
__device__ __forceinline__ float depth_row_u(const DepthEntry& e, float pyf) { return __builtin_fmaf(e.uy, pyf, e.ncu); }
__device__ __forceinline__ float depth_row_w(const DepthEntry& e, float pyf) { return __builtin_fmaf(e.wy, pyf, e.ncw); }

// The tiles of the bin at (binX0, binY0) an entry can reach, one bit per 16x16 tile: a conservative test at staging, k_blend's
// quadrant test at tile size: a tile is left out when its pixel centres lie outside the oriented box |vPosition.x|, |vPosition.y| <= 2
// (separating axes u and w), or farther from the centre than the longer semi-axis.  Every fragment left out has q > 4, so a walk
// is bit-identical with and without it.
__device__ __forceinline__ uint32_t depth_tile_reach(const DepthEntry& en, float cx, float cy, int binX0, int binY0)
{
    // vPosition at a tile's centre (pixel offset 7.5 from its first pixel centre) and how far it can move over the
    // tile's pixel centres (7.5 each way); the slack covers the rounding of these sums
    const float eu = 7.5f * (fabsf(en.ux) + fabsf(en.uy)) + 2.0005f;
    const float ew = 7.5f * (fabsf(en.wx) + fabsf(en.wy)) + 2.0005f;
    const float minlen2 = fminf(en.ux * en.ux + en.uy * en.uy, en.wx * en.wx + en.wy * en.wy);
    uint32_t tiles = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const float dx = ((float)(binX0 + (t & 1) * TILE) + 8.0f) - cx, dy = ((float)(binY0 + (t >> 1) * TILE) + 8.0f) - cy;
        const float ddx = fmaxf(fabsf(dx) - 7.5f, 0.0f), ddy = fmaxf(fabsf(dy) - 7.5f, 0.0f);
        const bool reach = fabsf(en.ux * dx + en.uy * dy) <= eu && fabsf(en.wx * dx + en.wy * dy) <= ew &&
                           (ddx * ddx + ddy * ddy) * minlen2 <= 4.002f;
        if (reach) tiles |= 1u << t;
    }
    return tiles;
}

// ---- the walk of one bin ------------------------------------------------------------------------------------------------------
// The sites of the bounds-checked build (-DGSR_BOUNDS) that every unit shares, under the same number in each; a unit's own sites
// follow from 4.  A unit hands its counters in as a type with  static void bound(int site, idx, limit)  over its GSR_BOUND.
constexpr int WALK_SITE_BIN = 0, WALK_SITE_LIST = 1, WALK_SITE_SPLAT = 2, WALK_SITE_CELL = 3;

// A frame whose lists did not fit published no work (k_bin_finalize): nothing of it is walked, nothing is written, and the host
// learns at its next synchronisation that the results are not this frame's.  True: leave.
__device__ __forceinline__ bool walk_frame_unfit(const uint32_t* __restrict__ overflow, uint32_t* __restrict__ invalid)
{
    const bool unfit = *overflow != 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *invalid = unfit ? 1u : 0u;
    return unfit;
}

// A bin, its list and a thread's place in the workgroup that walks it: wave `wave` owns the 16x16 tile at (ox, oy) of the bin, lane
// (lx, ly) of it the pixels (ox + lx + 8i, oy + ly + 8j).  (k_pick, one wave per pixel, reads the bin and its list only.)
struct WalkBin {
    int bin, binX0, binY0;   // the bin and its first pixel
    int lane, wave, lx, ly, ox, oy;
    float bx0c, by0c;        // the centre of the bin's first pixel: records are folded to it (depth_entry)
    uint32_t begin, end;     // the bin's entries of list[], clamped to what the list holds
};
template <class Bounds>
__device__ __forceinline__ WalkBin walk_bin(const FrameLists& a, const BinGrid& g, int bin)
{
    const int nbxb = g.bx_hi - g.bx_lo;
    Bounds::bound(WALK_SITE_BIN, bin, nbxb * g.nby);
    WalkBin w;
    w.bin = bin;
    w.lane = threadIdx.x & 63; w.wave = threadIdx.x >> 6;
    w.lx = w.lane & 7; w.ly = w.lane >> 3;
    const int by = bin / nbxb, bxl = bin - by * nbxb;
    w.binX0 = (g.bx_lo + bxl) * BIN_PX; w.binY0 = by * BIN_PX;
    w.ox = (w.wave & 1) * TILE; w.oy = (w.wave >> 1) * TILE;
    w.bx0c = (float)w.binX0 + 0.5f; w.by0c = (float)w.binY0 + 0.5f;
    w.end = min(a.bin_start[bin + 1], a.capacity); w.begin = min(a.bin_start[bin], w.end);
    Bounds::bound(WALK_SITE_LIST, a.bin_start[bin + 1], (unsigned long long)a.capacity + 1ull);
    Bounds::bound(WALK_SITE_LIST, a.bin_start[bin], (unsigned long long)a.bin_start[bin + 1] + 1ull);
    return w;
}
// entry e of the list: a splat index, clamped to the scene
template <class Bounds>
__device__ __forceinline__ uint32_t walk_list_entry(const FrameLists& a, uint32_t e)
{
    Bounds::bound(WALK_SITE_LIST, e, a.capacity);
    Bounds::bound(WALK_SITE_SPLAT, a.list[e], a.nsplats);
    return min(a.list[e], a.nsplats - 1u);
}

// what every pass stages of a chunk: a kernel declares it __shared__ beside the arrays of its own pass and hands it in
struct WalkStage {
    float4 s_a[DEPTH_CHUNK];         // ux, uy, ncu, wx
    float4 s_b[DEPTH_CHUNK];         // wy, ncw, la, and one word of the pass (Pass::stage)
    uint32_t s_tiles[DEPTH_CHUNK];   // one bit per tile of the bin the entry can reach
};
// The entries [begin, end) of w's list, every wave its tile's entries in list order.  Of a pass:
//   float stage(const DepthEntry&)         thread t stages entry base + t into cell t: what the pass keeps of it beside the walk's
//                                          words, and the word it wants in the cell's s_b.w;
//   void visit(uint32_t cell, DepthEntry)  the whole wave, for an entry its tile can reach: the cell as staged (z: the pass's word,
//                                          index: not staged here).
// INVARIANT: a workgroup barrier lies between any wave's last read of a chunk's cells and the first write of the next chunk's: the
// barrier at the loop's top.  SKIP: entries that provably cannot reach a tile carry no bit for it.
template <bool SKIP, class Pass>
__device__ __forceinline__ void walk_bin_list(WalkStage& st, const FrameLists& a, const WalkBin& w, const CamParams& cam, uint32_t begin, uint32_t end,
                                              Pass& pass)
{
    for (uint32_t base = begin; base < end; base += DEPTH_CHUNK) {
        __syncthreads();   // the previous chunk is consumed
        const uint32_t e = base + threadIdx.x;
        uint32_t tiles = 0;
        if (e < end) {
            const uint32_t i = walk_list_entry<Pass>(a, e);
            const DepthEntry en = depth_entry(a.rec, a.px, a.py, a.pz, i, cam, w.bx0c, w.by0c);
            const float cx = a.rec[i].cx, cy = a.rec[i].cy;   // (with depth_entry's loads of the record, not behind the pass's stores)
            st.s_a[threadIdx.x] = make_float4(en.ux, en.uy, en.ncu, en.wx);
            st.s_b[threadIdx.x] = make_float4(en.wy, en.ncw, en.la, pass.stage(en));
            tiles = SKIP ? depth_tile_reach(en, cx, cy, w.binX0, w.binY0) : 0xfu;
        }
        st.s_tiles[threadIdx.x] = tiles;
        __syncthreads();

        const uint32_t cnt = min((uint32_t)DEPTH_CHUNK, end - base);
        for (uint32_t c0 = 0; c0 < cnt; c0 += WAVE) {
            // my tile's entries among these 64, in list order (entries behind the walk's end carry no bit)
            uint64_t bal = __ballot(((st.s_tiles[c0 + w.lane] >> w.wave) & 1u) != 0u);
            while (bal) {
                const uint32_t cell = c0 + (uint32_t)__builtin_ctzll(bal);
                bal &= bal - 1ull;
                Pass::bound(WALK_SITE_CELL, cell, DEPTH_CHUNK);
                const float4 ra = st.s_a[cell], rb = st.s_b[cell];   // the same address in every lane: a broadcast
                DepthEntry en;
                en.ux = ra.x; en.uy = ra.y; en.ncu = ra.z; en.wx = ra.w; en.wy = rb.x; en.ncw = rb.y; en.la = rb.z; en.z = rb.w;
                en.index = 0u;
                pass.visit(cell, en);
            }
        }
    }
}

// the launch of such a pass: one workgroup per bin of the context, nothing without a bin
template <class Buffers>
inline void walk_launch(void (*kernel)(Buffers, BinGrid, CamParams), const Buffers& b, const BinGrid& g, const CamParams& cam, hipStream_t s)
{
    const int nbins = (g.bx_hi - g.bx_lo) * g.nby;
    if (nbins > 0) hipLaunchKernelGGL(kernel, dim3(nbins), dim3(DEPTH_THREADS), 0, s, b, g, cam);
}

}  // namespace gsr
