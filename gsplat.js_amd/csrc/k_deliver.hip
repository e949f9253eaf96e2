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

// ---------------------------------------------------------------------------------------------------------
// 4:2:0 Y'CbCr (NV12 / I420) for video encoders: the definition is DESIGN.md section 4, "Frame delivery in Y'CbCr".
// ---------------------------------------------------------------------------------------------------------
GSR_BOUNDS_DECL(deliver)   // sites: 0 source pixel, 1 byte of the Y plane, 2 byte of the chroma planes, 3 trailer inside the staging buffer,
                           // 4 word of the depth plane, 5 sample of the hit plane a band pack reads, 6 sample of a slab's depth section
                           // (written by the pack, read by the de-slab), 7 sample of the gathered plane

constexpr int YUV_STRIP = 8;   // pixels of a row a lane owns (two rows of them)

// a lane's two rows of YUV_STRIP pixels, all loads issued before anything is converted
template <class Src> struct YuvStrip;
template <> struct YuvStrip<float4> {
    float4 v[2][YUV_STRIP];
    __device__ __forceinline__ void load(const float4* r0, const float4* r1)
    {
#pragma unroll
        for (int i = 0; i < YUV_STRIP; i++) { v[0][i] = r0[i]; v[1][i] = r1[i]; }
    }
    __device__ __forceinline__ uint32_t px(int r, int i) const { return to_rgba8(v[r][i]); }
};
template <> struct YuvStrip<uint32_t> {
    uint4 v[2][YUV_STRIP / 4];
    __device__ __forceinline__ void load(const uint32_t* r0, const uint32_t* r1)
    {
#pragma unroll
        for (int i = 0; i < YUV_STRIP / 4; i++) {
            v[0][i] = reinterpret_cast<const uint4*>(r0)[i];
            v[1][i] = reinterpret_cast<const uint4*>(r1)[i];
        }
    }
    __device__ __forceinline__ uint32_t px(int r, int i) const
    {
        const uint4 q = v[r][i >> 2];
        return (i & 3) == 0 ? q.x : (i & 3) == 1 ? q.y : (i & 3) == 2 ? q.z : q.w;
    }
};
__device__ __forceinline__ uint32_t yuv_source(const float4* p) { return to_rgba8(*p); }
__device__ __forceinline__ uint32_t yuv_source(const uint32_t* p) { return *p; }

// one pixel: laid over the background (nothing is added for black: (t * 0 + 127) / 255 = 0; the three multiply-adds cost less than
// a second form of the kernel), its luma returned, its channels added to the block's sums
__device__ __forceinline__ uint32_t yuv_luma(uint32_t p, const YuvParams& k, int32_t& rs, int32_t& gs, int32_t& bs)
{
    int32_t r = (int32_t)(p & 255u), g = (int32_t)((p >> 8) & 255u), b = (int32_t)((p >> 16) & 255u);
    const uint32_t t = 255u - (p >> 24);
    r = min(255, r + (int32_t)((t * (k.bg & 255u) + 127u) / 255u));
    g = min(255, g + (int32_t)((t * ((k.bg >> 8) & 255u) + 127u) / 255u));
    b = min(255, b + (int32_t)((t * ((k.bg >> 16) & 255u) + 127u) / 255u));
    rs += r; gs += g; bs += b;
    return (uint32_t)(k.y0 + ((k.y[0] * r + k.y[1] * g + k.y[2] * b + 128) >> 8));
}
__device__ __forceinline__ uint32_t yuv_chroma(const int32_t* c, int32_t rs, int32_t gs, int32_t bs, const YuvParams& k)
{
    return (uint32_t)min(max(128 + ((c[0] * rs + c[1] * gs + c[2] * bs + 512) >> 10), k.c_lo), k.c_hi);
}

// a loaded strip converted and stored whole: 8 bytes of Y per row, 8 (NV12) or 4 + 4 (I420) bytes of chroma
template <int Format, class Strip>
__device__ __forceinline__ void yuv_convert_strip(const Strip& in, const YuvParams& k, [[maybe_unused]] const uint8_t* staging, uint8_t* yrow,
                                                  uint8_t* crow, int32_t W, [[maybe_unused]] uint32_t ysize, uint32_t csize)
{
    uint32_t ya[YUV_STRIP / 4] = {}, yb[YUV_STRIP / 4] = {}, cb[YUV_STRIP / 2], cr[YUV_STRIP / 2];
#pragma unroll
    for (int j = 0; j < YUV_STRIP / 2; j++) {
        int32_t rs = 0, gs = 0, bs = 0;
#pragma unroll
        for (int d = 0; d < 2; d++) {
            const int i = 2 * j + d;
            ya[i >> 2] |= yuv_luma(in.px(0, i), k, rs, gs, bs) << (8 * (i & 3));
            yb[i >> 2] |= yuv_luma(in.px(1, i), k, rs, gs, bs) << (8 * (i & 3));
        }
        cb[j] = yuv_chroma(k.cb, rs, gs, bs, k);
        cr[j] = yuv_chroma(k.cr, rs, gs, bs, k);
    }
    static_assert(YUV_STRIP == 8, "the stores below are written for eight pixels");
    GSR_BOUND(deliver, 1, (size_t)(yrow - staging) + W + YUV_STRIP - 1, ysize);
    *reinterpret_cast<uint2*>(yrow) = make_uint2(ya[0], ya[1]);
    *reinterpret_cast<uint2*>(yrow + W) = make_uint2(yb[0], yb[1]);
    if (Format == DELIVER_NV12) {
        GSR_BOUND(deliver, 2, (size_t)(crow - staging) - ysize + YUV_STRIP - 1, 2u * csize);
        *reinterpret_cast<uint2*>(crow) = make_uint2(cb[0] | (cr[0] << 8) | (cb[1] << 16) | (cr[1] << 24), cb[2] | (cr[2] << 8) | (cb[3] << 16) | (cr[3] << 24));
    } else {
        GSR_BOUND(deliver, 2, (size_t)(crow - staging) - ysize + csize + YUV_STRIP / 2 - 1, 2u * csize);
        *reinterpret_cast<uint32_t*>(crow) = cb[0] | (cb[1] << 8) | (cb[2] << 16) | (cb[3] << 24);
        *reinterpret_cast<uint32_t*>(crow + csize) = cr[0] | (cr[1] << 8) | (cr[2] << 16) | (cr[3] << 24);
    }
}

// A lane owns two rows by YUV_STRIP pixels = YUV_STRIP / 2 chroma samples.  Where the strip lies whole inside an image whose
// width is a multiple of YUV_STRIP (every row, chroma row and plane then starts on 8 bytes; 4 for I420's chroma) it issues
// its 16-byte loads -- 2 x 8 of the f32 framebuffer, 2 x 2 of a gathered RGBA8 frame; the lanes of a wave are neighbours in
// the two rows, so every line fetched is used whole -- converts, and stores 8 bytes of Y per row and 8 (NV12) or 4 + 4 (I420)
// bytes of chroma.  Any other lane -- the last row pair of an odd height, every lane of other widths -- goes pixel by pixel with
// the coordinates clamped to the image (the edge column / row is replicated into the block) and stores bytes: it reads
// nothing outside src[W * H] and writes nothing outside the planes.  Streams 16 (or 4) bytes in and 1.5 out per pixel.
// The trailer is k_deliver_rgba8's, at the payload rounded up to whole words.
template <int Format, class Src>
__global__ __launch_bounds__(DELIVER_THREADS) void k_deliver_yuv(const Src* __restrict__ src, uint8_t* __restrict__ staging, int32_t W, int32_t H,
                                                                 YuvParams k, uint32_t serial_lo, uint32_t serial_hi,
                                                                 const uint32_t* __restrict__ overflow, [[maybe_unused]] uint32_t staging_bytes)
{
    const uint32_t Wc = (uint32_t)(W + 1) / 2u, Hc = (uint32_t)(H + 1) / 2u;
    const uint32_t ysize = (uint32_t)W * (uint32_t)H, csize = Wc * Hc;   // (W, H <= 8192: the payload stays below 2^27)
    [[maybe_unused]] const uint32_t payload = ysize + 2u * csize;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t* tr = reinterpret_cast<uint32_t*>(staging + ((payload + 3u) & ~3u));
        GSR_BOUND(deliver, 3, ((payload + 3u) & ~3u) + DELIVER_TRAILER_WORDS * 4 - 1, staging_bytes);
        tr[0] = *overflow; tr[1] = (uint32_t)W | ((uint32_t)H << 16); tr[2] = serial_lo; tr[3] = serial_hi;
    }
    const uint32_t strips = (uint32_t)(W + YUV_STRIP - 1) / YUV_STRIP;
    const uint32_t lane = blockIdx.x * DELIVER_THREADS + threadIdx.x;
    const uint32_t cy = lane / strips, sx = lane - cy * strips;
    if (cy >= Hc) return;
    const uint32_t x0 = sx * YUV_STRIP, y0 = cy * 2u;
    uint8_t* const yrow = staging + (size_t)y0 * W + x0;
    // NV12: one plane of (Cb, Cr) pairs; I420: the Cb plane, then the Cr plane
    uint8_t* const crow = staging + ysize + (Format == DELIVER_NV12 ? (size_t)cy * 2u * Wc + x0 : (size_t)cy * Wc + x0 / 2u);

    if (W % YUV_STRIP == 0 && y0 + 1u < (uint32_t)H) {
        YuvStrip<Src> in;
        GSR_BOUND(deliver, 0, (size_t)(y0 + 1u) * W + x0 + YUV_STRIP - 1, ysize);
        in.load(src + (size_t)y0 * W + x0, src + (size_t)(y0 + 1u) * W + x0);
        __builtin_amdgcn_sched_barrier(0);   // every load is in flight before the first conversion (the scheduler would hold four back)
        yuv_convert_strip<Format>(in, k, staging, yrow, crow, W, ysize, csize);
        return;
    }
    for (uint32_t j = 0; j < YUV_STRIP / 2 && x0 + 2u * j < (uint32_t)W; j++) {
        int32_t rs = 0, gs = 0, bs = 0;
        for (uint32_t d = 0; d < 4u; d++) {
            const uint32_t x = x0 + 2u * j + (d & 1u), y = y0 + (d >> 1);
            const size_t at = (size_t)min(y, (uint32_t)H - 1u) * W + min(x, (uint32_t)W - 1u);
            GSR_BOUND(deliver, 0, at, ysize);
            const uint32_t luma = yuv_luma(yuv_source(src + at), k, rs, gs, bs);
            if (x < (uint32_t)W && y < (uint32_t)H) {
                GSR_BOUND(deliver, 1, (size_t)y * W + x, ysize);
                staging[(size_t)y * W + x] = (uint8_t)luma;
            }
        }
        uint8_t* const c0 = crow + (Format == DELIVER_NV12 ? 2u * j : j);
        uint8_t* const c1 = Format == DELIVER_NV12 ? c0 + 1 : c0 + csize;
        GSR_BOUND(deliver, 2, (size_t)(c0 - staging) - ysize, 2u * csize);
        GSR_BOUND(deliver, 2, (size_t)(c1 - staging) - ysize, 2u * csize);
        *c0 = (uint8_t)yuv_chroma(k.cb, rs, gs, bs, k);
        *c1 = (uint8_t)yuv_chroma(k.cr, rs, gs, bs, k);
    }
}

// ---------------------------------------------------------------------------------------------------------
// The depth plane of a depth ring (gsr_delivery_open_depth; the definition is DESIGN.md section 4, "Frame delivery with depth"):
// the ring's f32 hit plane of n = Wd * Hd samples into the slot's staging at the depth offset (a multiple of 16), as it is or
// quantised to 16 bits, and the slot's trailer behind it -- the one the host reads; the colour kernel in front of this one has
// written its own at the end of the colour payload, where the padding and this plane now lie.
// A lane owns 16 bytes of the output: four samples as f32, eight as u16 (two 16-byte loads, both issued before the first
// division).  The last lane of a plane that is not a multiple of that takes its samples one (f32) or two (u16: a whole
// word, the missing half zero -- the padding in front of the trailer) at a time.  Streams 4 bytes in and 4 or 2 out per sample.
// ---------------------------------------------------------------------------------------------------------
// inverse depth against `near` in 16 bits: 65535 unless z > 0 (NaN included); +infinity is 0.  The division is the correctly
// rounded one (hipcc's default for `/`), the rounding to an integer is to nearest, ties to even (v_rndne_f32).
__device__ __forceinline__ uint32_t depth_u16(float z, float near)
{
    if (!(z > 0.0f)) return 65535u;
    const float q = fminf(near / z, 1.0f);
    return (uint32_t)__builtin_rintf(q * 65535.0f);
}

template <int Format>
__global__ __launch_bounds__(DELIVER_THREADS) void k_deliver_depth(const float* __restrict__ plane, uint32_t* __restrict__ out, uint32_t n, float near,
                                                                   uint32_t* __restrict__ trailer, uint32_t dims, uint32_t serial_lo, uint32_t serial_hi,
                                                                   const uint32_t* __restrict__ overflow, [[maybe_unused]] uint32_t out_words)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *reinterpret_cast<uint4*>(trailer) = make_uint4(*overflow, dims, serial_lo, serial_hi);   // (16-byte aligned: see gsr_ctx::Delivery::trailer_offset)
    }
    constexpr uint32_t PER_LANE = Format == DELIVER_DEPTH_F32 ? 4u : 8u;
    const uint32_t s = (blockIdx.x * DELIVER_THREADS + threadIdx.x) * PER_LANE;
    if (s >= n) return;
    const uint4* in = reinterpret_cast<const uint4*>(plane + s);
    if (Format == DELIVER_DEPTH_F32) {
        if (s + PER_LANE <= n) {
            GSR_BOUND(deliver, 4, s + 3u, out_words);
            *reinterpret_cast<uint4*>(out + s) = in[0];
        } else {
            for (uint32_t i = s; i < n; i++) {
                GSR_BOUND(deliver, 4, i, out_words);
                out[i] = __float_as_uint(plane[i]);
            }
        }
    } else {
        if (s + PER_LANE <= n) {
            const uint4 a = in[0], b = in[1];
            uint4 o;
            o.x = depth_u16(__uint_as_float(a.x), near) | (depth_u16(__uint_as_float(a.y), near) << 16);
            o.y = depth_u16(__uint_as_float(a.z), near) | (depth_u16(__uint_as_float(a.w), near) << 16);
            o.z = depth_u16(__uint_as_float(b.x), near) | (depth_u16(__uint_as_float(b.y), near) << 16);
            o.w = depth_u16(__uint_as_float(b.z), near) | (depth_u16(__uint_as_float(b.w), near) << 16);
            GSR_BOUND(deliver, 4, s / 2u + 3u, out_words);
            *reinterpret_cast<uint4*>(out + s / 2u) = o;
        } else {
            for (uint32_t i = s; i < n; i += 2u) {
                const uint32_t lo = depth_u16(plane[i], near), hi = i + 1u < n ? depth_u16(plane[i + 1u], near) : 0u;
                GSR_BOUND(deliver, 4, i / 2u, out_words);
                out[i / 2u] = lo | (hi << 16);
            }
        }
    }
}

void launch_deliver_depth(int format, const float* plane, uint8_t* staging, size_t depth_offset, size_t trailer_offset, int32_t Wd, int32_t Hd, float near,
                          int32_t W, int32_t H, uint64_t serial, const uint32_t* overflow, hipStream_t s)
{
    const uint32_t n = (uint32_t)Wd * (uint32_t)Hd;   // (Wd, Hd <= 8192)
    const uint32_t per_lane = format == DELIVER_DEPTH_F32 ? 4u : 8u;
    const uint32_t lanes = (n + per_lane - 1u) / per_lane;
    const dim3 grid(std::max(1u, (lanes + DELIVER_THREADS - 1) / DELIVER_THREADS)), block(DELIVER_THREADS);
    uint32_t* out = reinterpret_cast<uint32_t*>(staging + depth_offset);
    uint32_t* trailer = reinterpret_cast<uint32_t*>(staging + trailer_offset);
    const uint32_t out_words = (uint32_t)((trailer_offset - depth_offset) / 4);
    const uint32_t dims = (uint32_t)W | ((uint32_t)H << 16);
    if (format == DELIVER_DEPTH_F32)
        hipLaunchKernelGGL(k_deliver_depth<DELIVER_DEPTH_F32>, grid, block, 0, s, plane, out, n, near, trailer, dims, (uint32_t)serial, (uint32_t)(serial >> 32),
                           overflow, out_words);
    else
        hipLaunchKernelGGL(k_deliver_depth<DELIVER_DEPTH_U16>, grid, block, 0, s, plane, out, n, near, trailer, dims, (uint32_t)serial, (uint32_t)(serial >> 32),
                           overflow, out_words);
}

void launch_deliver_gathered_depth(const uint32_t* plane, uint32_t words, uint8_t* staging, size_t depth_offset, size_t trailer_offset, int32_t W, int32_t H,
                                   uint64_t serial, const uint32_t* stale, hipStream_t s)
{
    const uint32_t lanes = (words + 3u) / 4u;
    hipLaunchKernelGGL(k_deliver_depth<DELIVER_DEPTH_F32>, dim3(std::max(1u, (lanes + DELIVER_THREADS - 1) / DELIVER_THREADS)), dim3(DELIVER_THREADS), 0, s,
                       reinterpret_cast<const float*>(plane), reinterpret_cast<uint32_t*>(staging + depth_offset), words, 0.0f,
                       reinterpret_cast<uint32_t*>(staging + trailer_offset), (uint32_t)W | ((uint32_t)H << 16), (uint32_t)serial, (uint32_t)(serial >> 32), stale,
                       (uint32_t)((trailer_offset - depth_offset) / 4));
}

// ---------------------------------------------------------------------------------------------------------
// Depth in a group (gsr_comm_set_depth): the band's samples of the exchange's hit plane into the slab's depth
// section, and the gathered sections into one plane.  Pure data movement, a few megabytes at most: what counts is that there is
// ONE launch each.  Threads run along a row; a pack lane owns four samples of a section row (rows start on 16 bytes and hold a
// multiple of 8 samples: one 16-byte store as f32, one 8-byte store as u16), a de-slab lane 16 bytes of the gathered plane.
// Loads are single samples -- a plane row starts wherever y * Wd puts it -- and neighbouring lanes read neighbouring addresses.
// ---------------------------------------------------------------------------------------------------------
template <int Format>
__global__ __launch_bounds__(DELIVER_THREADS) void k_pack_band_depth(const float* __restrict__ plane, uint8_t* __restrict__ section, int Wd,
                                                                     [[maybe_unused]] int Hd, int xd0, int xd1, int stride, float near)
{
    const int s = (blockIdx.x * DELIVER_THREADS + threadIdx.x) * 4, y = blockIdx.y;
    if (s >= stride) return;
    const float* row = plane + (size_t)y * Wd;
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = xd0 + s + i;
        v[i] = 0u;   // behind the band's last sample: a narrower band than the widest, and the row's padding
        if (x < xd1) {
            GSR_BOUND(deliver, 5, (size_t)y * Wd + x, (size_t)Wd * Hd);
            v[i] = Format == DELIVER_DEPTH_F32 ? __float_as_uint(row[x]) : depth_u16(row[x], near);
        }
    }
    const size_t at = (size_t)y * stride + s;
    GSR_BOUND(deliver, 6, at + 3, (size_t)Hd * stride);
    if (Format == DELIVER_DEPTH_F32) *reinterpret_cast<uint4*>(section + at * 4) = make_uint4(v[0], v[1], v[2], v[3]);
    else *reinterpret_cast<uint2*>(section + at * 2) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
}

void launch_pack_band_depth(int format, const float* plane, uint8_t* section, int Wd, int Hd, int xd0, int xd1, int stride, float near, hipStream_t s)
{
    if (stride <= 0 || Hd <= 0) return;
    const dim3 grid((stride / 4 + DELIVER_THREADS - 1) / DELIVER_THREADS, Hd), block(DELIVER_THREADS);
    if (format == DELIVER_DEPTH_F32) hipLaunchKernelGGL(k_pack_band_depth<DELIVER_DEPTH_F32>, grid, block, 0, s, plane, section, Wd, Hd, xd0, xd1, stride, near);
    else hipLaunchKernelGGL(k_pack_band_depth<DELIVER_DEPTH_U16>, grid, block, 0, s, plane, section, Wd, Hd, xd0, xd1, stride, near);
}

template <int Format>
__global__ __launch_bounds__(DELIVER_THREADS) void k_unpack_slabs_depth(const uint8_t* __restrict__ gathered, uint32_t* __restrict__ plane, int Wd, uint32_t n,
                                                                        size_t slab_bytes, size_t offset, int stride, int world, SlabEdges e)
{
    constexpr uint32_t PER_LANE = Format == DELIVER_DEPTH_F32 ? 4u : 8u;
    const uint32_t s = (blockIdx.x * DELIVER_THREADS + threadIdx.x) * PER_LANE;
    if (s >= n) return;
    int y = (int)(s / (uint32_t)Wd), x = (int)(s - (uint32_t)y * (uint32_t)Wd);
    uint32_t w[4] = {0u, 0u, 0u, 0u};   // (samples behind the plane's last one stay zero: the padding a delivery slot takes with the plane)
#pragma unroll
    for (uint32_t i = 0; i < PER_LANE; i++) {
        if (s + i < n) {
            uint32_t v = 0u;
            for (int q = 0; q < world; q++) {
                if (x >= e.x0[q] && x < e.x1[q]) {
                    const size_t at = (size_t)y * stride + (x - e.x0[q]);
                    GSR_BOUND(deliver, 6, offset + (at + 1) * (Format == DELIVER_DEPTH_F32 ? 4 : 2) - 1, slab_bytes);
                    const uint8_t* sec = gathered + (size_t)q * slab_bytes + offset;
                    v = Format == DELIVER_DEPTH_F32 ? reinterpret_cast<const uint32_t*>(sec)[at] : (uint32_t)reinterpret_cast<const uint16_t*>(sec)[at];
                }
            }
            if (Format == DELIVER_DEPTH_F32) w[i] = v;
            else w[i >> 1] |= v << (16u * (i & 1u));
        }
        if (++x == Wd) { x = 0; y++; }
    }
    GSR_BOUND(deliver, 7, s / PER_LANE, (n + PER_LANE - 1u) / PER_LANE);
    *reinterpret_cast<uint4*>(plane + s / PER_LANE * 4u) = make_uint4(w[0], w[1], w[2], w[3]);
}

void launch_unpack_slabs_depth(int format, const uint8_t* gathered, uint32_t* plane, int Wd, int Hd, size_t slab_bytes, size_t offset, int stride,
                               int world, const SlabEdges& e, hipStream_t s)
{
    if (Wd <= 0 || Hd <= 0) return;
    const uint32_t n = (uint32_t)Wd * (uint32_t)Hd;   // (Wd, Hd <= 8192)
    const uint32_t per_lane = format == DELIVER_DEPTH_F32 ? 4u : 8u;
    const uint32_t lanes = (n + per_lane - 1u) / per_lane;
    const dim3 grid((lanes + DELIVER_THREADS - 1) / DELIVER_THREADS), block(DELIVER_THREADS);
    if (format == DELIVER_DEPTH_F32)
        hipLaunchKernelGGL(k_unpack_slabs_depth<DELIVER_DEPTH_F32>, grid, block, 0, s, gathered, plane, Wd, n, slab_bytes, offset, stride, world, e);
    else
        hipLaunchKernelGGL(k_unpack_slabs_depth<DELIVER_DEPTH_U16>, grid, block, 0, s, gathered, plane, Wd, n, slab_bytes, offset, stride, world, e);
}

template <class Src>
static void launch_deliver_yuv_from(int format, const Src* src, uint8_t* staging, size_t staging_bytes, int32_t W, int32_t H, const YuvParams& k,
                                    uint64_t serial, const uint32_t* overflow, hipStream_t s)
{
    const uint32_t lanes = (uint32_t)((W + YUV_STRIP - 1) / YUV_STRIP) * (uint32_t)((H + 1) / 2);
    const dim3 grid(std::max(1u, (lanes + DELIVER_THREADS - 1) / DELIVER_THREADS)), block(DELIVER_THREADS);
    if (format == DELIVER_NV12)
        hipLaunchKernelGGL((k_deliver_yuv<DELIVER_NV12, Src>), grid, block, 0, s, src, staging, W, H, k, (uint32_t)serial, (uint32_t)(serial >> 32), overflow,
                           (uint32_t)staging_bytes);
    else
        hipLaunchKernelGGL((k_deliver_yuv<DELIVER_I420, Src>), grid, block, 0, s, src, staging, W, H, k, (uint32_t)serial, (uint32_t)(serial >> 32), overflow,
                           (uint32_t)staging_bytes);
}

void launch_deliver_yuv(int format, const float4* fb, const uint32_t* frame8, uint8_t* staging, size_t staging_bytes, int32_t W, int32_t H,
                        const YuvParams& k, uint64_t serial, const uint32_t* overflow, hipStream_t s)
{
    if (fb) launch_deliver_yuv_from(format, fb, staging, staging_bytes, W, H, k, serial, overflow, s);
    else launch_deliver_yuv_from(format, frame8, staging, staging_bytes, W, H, k, serial, overflow, s);
}

}  // namespace gsr
