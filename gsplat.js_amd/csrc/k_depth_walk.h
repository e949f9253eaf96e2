// The per-fragment arithmetic of the passes that walk the last frame's bin lists once more (k_depth.hip: depth planes and picking;
// k_contrib.hip: per-splat contribution), stated once: an entry as the walk reads it, the weight B of a fragment at a pixel, the row
// terms, and the staging-time test of which 16x16 tiles of the bin an entry can reach.  Device code only.
//
// For a pixel, its fragments are the entries of its bin's list, in list order, that pass the compositor's coverage test
// (|vPosition|^2 <= 4, the same f32 expression as k_blend's walk), with weight B = exp2(-q log2(e) + log2(opacity)); sequentially,
// from T = 1:  w = T * B;  T = T - w.
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
__device__ __forceinline__ uint32_t depth_tile_reach(const DepthEntry& en, const Record* __restrict__ r, int binX0, int binY0)
{
    // vPosition at a tile's centre (pixel offset 7.5 from its first pixel centre) and how far it can move over the
    // tile's pixel centres (7.5 each way); the slack covers the rounding of these sums
    const float eu = 7.5f * (fabsf(en.ux) + fabsf(en.uy)) + 2.0005f;
    const float ew = 7.5f * (fabsf(en.wx) + fabsf(en.wy)) + 2.0005f;
    const float minlen2 = fminf(en.ux * en.ux + en.uy * en.uy, en.wx * en.wx + en.wy * en.wy);
    uint32_t tiles = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const float dx = ((float)(binX0 + (t & 1) * TILE) + 8.0f) - r->cx, dy = ((float)(binY0 + (t >> 1) * TILE) + 8.0f) - r->cy;
        const float ddx = fmaxf(fabsf(dx) - 7.5f, 0.0f), ddy = fmaxf(fabsf(dy) - 7.5f, 0.0f);
        const bool reach = fabsf(en.ux * dx + en.uy * dy) <= eu && fabsf(en.wx * dx + en.wy * dy) <= ew &&
                           (ddx * ddx + ddy * ddy) * minlen2 <= 4.002f;
        if (reach) tiles |= 1u << t;
    }
    return tiles;
}

}  // namespace gsr
