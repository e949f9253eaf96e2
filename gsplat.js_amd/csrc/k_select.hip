// Selection: one bit per splat of a scene ("Selection"): bit i & 31 of word i >> 5, bits at and above n
// always 0.  Three pickers set the picked splats' bits in a scratch mask -- by the centre pixel of the last frame's listed splats
// (k_select_centre), by the frame's hit-index plane (k_select_hit), by a world box (k_select_box) -- and k_select_apply folds the
// scratch mask into the selection with the call's op and counts the result.  Nothing here is a node of the frame's graph or reads
// FrameArgs: like the depth pass (k_depth.hip) it runs behind the frame, on what the frame left on the device.
//
// A bit set is order-independent, so the atomic ORs of the two region pickers give an exact result whatever order they land in.
#include "gsr_internal.h"
#include "k_splat_ops.h"

#include <algorithm>

namespace gsr {

GSR_BOUNDS_DECL(select)   // sites: 0 bin -> bin_start, 1 list position, 2 splat index (list entry or plane value), 3 region byte,
                          //        4 plane pixel, 5 selection word
constexpr int SELECT_THREADS = 256;

// the site of the shared mask store (k_splat_ops.h)
struct select_sites {
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(select, 5, idx, limit); }
};

// the region byte of pixel (x, y) of the rectangle: true without bytes
__device__ __forceinline__ bool region_has(const SelectRegion& r, int x, int y)
{
    if (!r.bytes) return true;
    const size_t o = (size_t)(y - r.y0) * (size_t)r.stride + (size_t)(x - r.x0);
    GSR_BOUND(select, 3, o, r.nbytes);
    return o < r.nbytes && r.bytes[o] != 0;
}

__device__ __forceinline__ void pick_splat(const SelectBuffers& a, uint32_t i)
{
    const uint32_t w = i >> 5;
    GSR_BOUND(select, 5, w, a.nwords);
    if (w < a.nwords) atomicOr(&a.scratch[w], 1u << (i & 31u));
}

// GSR_SELECT_CENTRE.  One workgroup per bin that meets the rectangle (bx0, by0: the first such bin, band-relative column; nbw of them
// across): the bin's list from its first entry to its last, strided across the threads; of every entry the first 8 bytes of its
// record.  A listed splat's centre pixel (floor(cx), floor(cy)) lies in its own pixel box, so in the list of exactly one bin: the
// workgroup of THAT bin claims the splat, when the pixel is also in the rectangle and on a non-zero region byte.  The records are
// read through the lists only (gsr_internal.h, ProjectLaunch: rec[] holds this frame's data for listed splats and nothing else).
__global__ __launch_bounds__(SELECT_THREADS) void k_select_centre(SelectBuffers a, BinGrid g, SelectRegion r, int bx0, int by0, int nbw)
{
    // a frame whose lists did not fit published no work: nothing of it is walked (k_depth_planes has the same rule)
    const bool unfit = *a.overflow != 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.invalid = unfit ? 1u : 0u;
    if (unfit) return;

    const int nbxb = g.bx_hi - g.bx_lo;
    const int bxl = bx0 + (int)(blockIdx.x % (uint32_t)nbw), by = by0 + (int)(blockIdx.x / (uint32_t)nbw);
    const int bin = by * nbxb + bxl;
    GSR_BOUND(select, 0, bin, nbxb * g.nby);
    if (bxl < 0 || bxl >= nbxb || by < 0 || by >= g.nby) return;
    const int binX0 = (g.bx_lo + bxl) * BIN_PX, binY0 = by * BIN_PX;
    // the pixels this workgroup answers for: the bin's, inside the rectangle (small exact integers as floats)
    const int px0 = max(binX0, r.x0), px1 = min(binX0 + BIN_PX, r.x1), py0 = max(binY0, r.y0), py1 = min(binY0 + BIN_PX, r.y1);
    const float fx0 = (float)px0, fx1 = (float)px1, fy0 = (float)py0, fy1 = (float)py1;

    const uint32_t end = min(a.bin_start[bin + 1], a.capacity), begin = min(a.bin_start[bin], end);
    GSR_BOUND(select, 1, a.bin_start[bin + 1], (unsigned long long)a.capacity + 1ull);
    GSR_BOUND(select, 1, a.bin_start[bin], (unsigned long long)a.bin_start[bin + 1] + 1ull);
    for (uint32_t e = begin + threadIdx.x; e < end; e += SELECT_THREADS) {
        GSR_BOUND(select, 1, e, a.capacity);
        GSR_BOUND(select, 2, a.list[e], a.nsplats);
        const uint32_t i = min(a.list[e], a.nsplats - 1u);
        const float2 c = *reinterpret_cast<const float2*>(a.rec + i);   // (cx, cy)
        // floor(c) in [p0, p1) is p0 <= c < p1 for integers p0, p1: decided in floats, so that nothing out of an int's range (or
        // a NaN) is ever converted
        if (!(c.x >= fx0 && c.x < fx1 && c.y >= fy0 && c.y < fy1)) continue;
        const int X = (int)floorf(c.x), Y = (int)floorf(c.y);
        if (region_has(r, X, Y)) pick_splat(a, i);
    }
}

// GSR_SELECT_HIT.  One thread per pixel of the rectangle: the plane's index there, the region byte, the same atomic OR.
__global__ __launch_bounds__(SELECT_THREADS) void k_select_hit(SelectBuffers a, BinGrid g, SelectRegion r)
{
    const uint32_t w = (uint32_t)(r.x1 - r.x0), h = (uint32_t)(r.y1 - r.y0);
    const uint32_t t = blockIdx.x * SELECT_THREADS + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.invalid = 0u;   // (the plane's own pass carries the word that counts: the host has read it)
    if (t >= w * h) return;
    const int x = r.x0 + (int)(t % w), y = r.y0 + (int)(t / w);
    const size_t o = (size_t)y * (size_t)g.W + (size_t)x;
    GSR_BOUND(select, 4, o, (size_t)g.W * (size_t)g.H);
    if (x < 0 || x >= g.W || y < 0 || y >= g.H) return;
    const uint32_t i = a.index[o];
    if (i == 0xffffffffu) return;   // no hit at this pixel
    GSR_BOUND(select, 2, i, a.nsplats);
    if (i >= a.nsplats) return;
    if (region_has(r, x, y)) pick_splat(a, i);
}

// gsr_select_box.  in_box of k_scene.hip per splat -- the same f64 comparisons on the same f32 positions as limitBox's
// compaction.  A wave's ballot is two whole words of the mask (mask_store_ballot, k_splat_ops.h): every word of the
// mask is stored (splats at and above n vote 0), so the caller need not zero it.
struct SelectBox { double v[6]; };
__global__ __launch_bounds__(SELECT_THREADS) void k_select_box(uint32_t n, const float* __restrict__ px, const float* __restrict__ py,
                                                               const float* __restrict__ pz, SelectBox box, uint32_t* __restrict__ scratch,
                                                               uint32_t nwords)
{
    const uint32_t i = blockIdx.x * SELECT_THREADS + threadIdx.x;
    bool in = false;
    if (i < n) {
        const double x = px[i], y = py[i], z = pz[i];
        in = x >= box.v[0] && x <= box.v[1] && y >= box.v[2] && y <= box.v[3] && z >= box.v[4] && z <= box.v[5];
    }
    mask_store_ballot<select_sites>(scratch, nwords, i, __ballot(in));
}

// sel <- sel (op) scratch word by word, the bits at and above n dropped from the result, and the popcount of the result: one sum
// per workgroup; k_select_fold adds them up.
__global__ __launch_bounds__(SELECT_APPLY_THREADS) void k_select_apply(int op, uint32_t* __restrict__ sel, const uint32_t* __restrict__ scratch,
                                                                       uint32_t n, uint32_t nwords, uint32_t* __restrict__ block_sums)
{
    __shared__ uint32_t s_w[SELECT_APPLY_THREADS / WAVE];
    const uint32_t w = blockIdx.x * SELECT_APPLY_THREADS + threadIdx.x;
    uint32_t bits = 0;
    if (w < nwords) {
        GSR_BOUND(select, 5, w, nwords);
        const uint32_t s = sel[w], p = op == SELOP_INVERT ? 0u : scratch[w];
        uint32_t v = op == SELOP_REPLACE ? p : op == SELOP_ADD ? (s | p) : op == SELOP_SUBTRACT ? (s & ~p) : op == SELOP_INTERSECT ? (s & p) : ~s;
        v &= set_live_bits(n, w);   // (0: the word lies behind the last splat)
        sel[w] = v;
        bits = (uint32_t)__popc(v);
    }
    // the wave's sum: its lanes' counts through the ballot of every bit position of a count (at most 32: six bits)
    uint32_t sum = 0;
#pragma unroll
    for (int b = 0; b < 6; b++) sum += (uint32_t)__popcll(__ballot(((bits >> b) & 1u) != 0u)) << b;
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t k = 0; k < SELECT_APPLY_THREADS / WAVE; k++) t += s_w[k];
        block_sums[blockIdx.x] = t;
    }
}

// one workgroup: the per-workgroup sums into *count
__global__ __launch_bounds__(SELECT_APPLY_THREADS) void k_select_fold(const uint32_t* __restrict__ block_sums, uint32_t nblocks, uint32_t* __restrict__ count)
{
    __shared__ uint32_t s_part[SELECT_APPLY_THREADS];
    uint32_t sum = 0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += SELECT_APPLY_THREADS) sum += block_sums[b];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t k = 0; k < SELECT_APPLY_THREADS; k++) t += s_part[k];
        *count = t;
    }
}

// ---- launchers ----
void launch_select_region(int mode, const SelectBuffers& b, const BinGrid& g, const SelectRegion& r, hipStream_t s)
{
    if (r.x1 <= r.x0 || r.y1 <= r.y0) return;
    if (mode == SELECT_HIT) {
        const uint64_t npix = (uint64_t)(r.x1 - r.x0) * (uint64_t)(r.y1 - r.y0);
        hipLaunchKernelGGL(k_select_hit, dim3((uint32_t)((npix + SELECT_THREADS - 1) / SELECT_THREADS)), dim3(SELECT_THREADS), 0, s, b, g, r);
        return;
    }
    // the bins of the context's band whose 32 x 32 pixels meet the rectangle
    const int bx0 = std::max(r.x0 / BIN_PX, g.bx_lo) - g.bx_lo, bx1 = std::min((r.x1 - 1) / BIN_PX, g.bx_hi - 1) - g.bx_lo;
    const int by0 = r.y0 / BIN_PX, by1 = std::min((r.y1 - 1) / BIN_PX, g.nby - 1);
    if (bx1 < bx0 || by1 < by0) return;
    const int nbw = bx1 - bx0 + 1, nbh = by1 - by0 + 1;
    hipLaunchKernelGGL(k_select_centre, dim3((uint32_t)(nbw * nbh)), dim3(SELECT_THREADS), 0, s, b, g, r, bx0, by0, nbw);
}

void launch_select_box(uint32_t n, const float* px, const float* py, const float* pz, const double* box, uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    SelectBox b;
    for (int k = 0; k < 6; k++) b.v[k] = box[k];
    hipLaunchKernelGGL(k_select_box, dim3(mask_blocks(nwords, SELECT_THREADS)), dim3(SELECT_THREADS), 0, s, n, px, py, pz, b, scratch, nwords);
}

void launch_select_apply(int op, uint32_t* sel, const uint32_t* scratch, uint32_t n, uint32_t nwords, uint32_t* block_sums, uint32_t* count, hipStream_t s)
{
    if (!nwords) return;
    const uint32_t blocks = (nwords + SELECT_APPLY_THREADS - 1) / SELECT_APPLY_THREADS;
    hipLaunchKernelGGL(k_select_apply, dim3(blocks), dim3(SELECT_APPLY_THREADS), 0, s, op, sel, scratch, n, nwords, block_sums);
    hipLaunchKernelGGL(k_select_fold, dim3(1), dim3(SELECT_APPLY_THREADS), 0, s, (const uint32_t*)block_sums, blocks, count);
}

}  // namespace gsr
