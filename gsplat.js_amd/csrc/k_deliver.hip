// Frame delivery: the f32 framebuffer as RGBA8 into a delivery slot's device staging buffer, from where ONE asynchronous copy
// takes pixels and trailer to the slot's pinned host block (gsr_deliver_frame_async).  A translation unit of its own so that
// the compositor's (k_blend.hip) code generation does not depend on anything here.
#include "gsr_internal.h"

namespace gsr {

constexpr int DELIVER_THREADS = 256;

// Four pixels per lane: four 16-byte loads in flight before the first conversion, one 16-byte store.  A lane's 64 bytes of
// `fb` are contiguous, so the four loads of a wave cover the same 4 KiB and every line fetched is used whole.  Streams 16
// bytes in and 4 out per pixel (41.5 MB at 1920 x 1080) and does nothing else: bound by HBM.
// The last lane of an image whose pixel count is not a multiple of four takes its 1..3 pixels one by one: nothing is
// read behind fb[npix - 1] and nothing written behind staging[npix - 1] but the trailer.
// The trailer reads the frame's overflow word on the render stream, i.e. behind this frame's chain and in front of the next
// one's k_project_key, which zeroes it -- the way k_pack_band_rgba8 puts it behind a slab.
__global__ __launch_bounds__(DELIVER_THREADS) void k_deliver_rgba8(const float4* __restrict__ fb, uint32_t* __restrict__ staging,
                                                                   uint32_t npix, uint32_t dims, uint32_t serial_lo,
                                                                   uint32_t serial_hi, const uint32_t* __restrict__ overflow)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint4 t;
        t.x = *overflow; t.y = dims; t.z = serial_lo; t.w = serial_hi;
        uint32_t* tr = staging + npix;   // (4-byte aligned only when npix is not a multiple of four)
        tr[0] = t.x; tr[1] = t.y; tr[2] = t.z; tr[3] = t.w;
    }
    const uint32_t p = (blockIdx.x * DELIVER_THREADS + threadIdx.x) * 4u;
    if (p + 4u <= npix) {
        const float4 a = fb[p], b = fb[p + 1], c = fb[p + 2], d = fb[p + 3];
        uint4 o;
        o.x = to_rgba8(a); o.y = to_rgba8(b); o.z = to_rgba8(c); o.w = to_rgba8(d);
        *reinterpret_cast<uint4*>(staging + p) = o;
    } else {
        for (uint32_t i = p; i < npix; i++) staging[i] = to_rgba8(fb[i]);
    }
}

void launch_deliver_rgba8(const float4* fb, uint32_t* staging, int32_t W, int32_t H, uint64_t serial, const uint32_t* overflow, hipStream_t s)
{
    const uint32_t npix = (uint32_t)W * (uint32_t)H;   // (W, H <= 8192)
    const uint32_t lanes = (npix + 3u) / 4u;
    // (an empty image still delivers its trailer)
    hipLaunchKernelGGL(k_deliver_rgba8, dim3(std::max(1u, (lanes + DELIVER_THREADS - 1) / DELIVER_THREADS)), dim3(DELIVER_THREADS), 0, s,
                       fb, staging, npix, (uint32_t)W | ((uint32_t)H << 16), (uint32_t)serial, (uint32_t)(serial >> 32), overflow);
}

}  // namespace gsr
