// What a kernel does to ONE splat of the SoA scene, and how it reads a one-bit-per-splat set: each contract stated once, beside
// k_pack_cov.h and by the same rule.  Scene.translate / rotate / scale (src/core/Scene.ts:182-305) for the whole scene (k_scene.hip)
// and for the selected splats (k_edit.hip) are the same functions, so "everything selected, no pivot" IS the whole-scene transform;
// the row copy serves the compaction (k_scene.hip) and the growth (k_append.hip); the set layout serves every kernel that reads a
// selection or a hidden set.  f64 in the reference's order of operations, f32 wherever the reference stores into a Float32Array;
// the units that include it are compiled with -ffp-contract=off.
#pragma once
#include "gsr_internal.h"
#include "k_pack_cov.h"

namespace gsr {

// ---- a set of splats: bit i & 31 of word i >> 5; a word at or behind nwords reads as zero; bits at and above n do not count ----
// the bits of word wi that name a splat below n (0: the word lies behind the last splat)
__device__ __forceinline__ uint32_t set_live_bits(uint32_t n, uint32_t wi)
{
    if ((uint64_t)wi * 32u >= n) return 0u;
    const uint32_t rest = n - wi * 32u;
    return rest >= 32u ? 0xffffffffu : (1u << rest) - 1u;
}
// word wi of the set with the bits at and above n dropped
__device__ __forceinline__ uint32_t set_word(const uint32_t* __restrict__ words, uint32_t nwords, uint32_t n, uint32_t wi)
{
    if ((uint64_t)wi * 32u >= n || wi >= nwords) return 0u;   // (nothing is loaded for a word behind either end)
    return words[wi] & set_live_bits(n, wi);
}
// is splat i in the set?  For callers that know i < n already; the others ask `i < n && set_bit(..)`
__device__ __forceinline__ bool set_bit(const uint32_t* __restrict__ words, uint32_t nwords, uint32_t i)
{
    return (i >> 5) < nwords && ((words[i >> 5] >> (i & 31u)) & 1u) != 0u;
}

// ---- the nine arrays of a splat's row, src row i -> dst row o.  Words, not floats: the bits travel as they are (NaN payloads, -0.0)
__device__ __forceinline__ void copy_splat_row(const SceneDev& dst, uint32_t o, const SceneDev& src, uint32_t i)
{
    reinterpret_cast<uint32_t*>(dst.px)[o] = reinterpret_cast<const uint32_t*>(src.px)[i];
    reinterpret_cast<uint32_t*>(dst.py)[o] = reinterpret_cast<const uint32_t*>(src.py)[i];
    reinterpret_cast<uint32_t*>(dst.pz)[o] = reinterpret_cast<const uint32_t*>(src.pz)[i];
    dst.cov0[o] = src.cov0[i]; dst.cov1[o] = src.cov1[i]; dst.cov2[o] = src.cov2[i]; dst.rgba[o] = src.rgba[i];
    reinterpret_cast<uint4*>(dst.rot)[o] = reinterpret_cast<const uint4*>(src.rot)[i];
    reinterpret_cast<uint4*>(dst.scl)[o] = reinterpret_cast<const uint4*>(src.scl)[i];
}

// ---- the transforms ----
// the 3x3 matrix of the quaternion (x, y, z, w), row-major (Matrix3 of Scene.ts:201-213); on the host for the SH frame (gsr_scene.cpp)
__host__ __device__ __forceinline__ void quat_matrix(double x, double y, double z, double w, double* R)
{
    R[0] = 1 - 2 * y * y - 2 * z * z; R[1] = 2 * x * y - 2 * z * w; R[2] = 2 * x * z + 2 * y * w;
    R[3] = 2 * x * y + 2 * z * w; R[4] = 1 - 2 * x * x - 2 * z * z; R[5] = 2 * y * z - 2 * x * w;
    R[6] = 2 * x * z - 2 * y * w; R[7] = 2 * y * z + 2 * x * w; R[8] = 1 - 2 * x * x - 2 * y * y;
}

// PIVOT: translate(-pivot), the operation, translate(+pivot) fused in registers -- every (float) below is a store of the
// reference's into positions; m = -pivot, p = pivot.  Without PIVOT neither is read
struct SplatPivot { double mx, my, mz, px, py, pz; };

// Scene.translate (Scene.ts:182-195)
__device__ __forceinline__ void splat_translate(const SceneDev& sc, uint32_t i, double tx, double ty, double tz)
{
    sc.px[i] = (float)((double)sc.px[i] + tx);
    sc.py[i] = (float)((double)sc.py[i] + ty);
    sc.pz[i] = (float)((double)sc.pz[i] + tz);
}

// Scene.rotate (Scene.ts:197-257), q = (x, y, z, w)
template <bool PIVOT>
__device__ __forceinline__ void splat_rotate(const SceneDev& sc, uint32_t i, double x, double y, double z, double w, const SplatPivot& v)
{
    double R[9]; quat_matrix(x, y, z, w, R);
    double px = sc.px[i], py = sc.py[i], pz = sc.pz[i];
    if (PIVOT) { px = (float)(px + v.mx); py = (float)(py + v.my); pz = (float)(pz + v.mz); }
    float ox = (float)(R[0] * px + R[1] * py + R[2] * pz);
    float oy = (float)(R[3] * px + R[4] * py + R[5] * pz);
    float oz = (float)(R[6] * px + R[7] * py + R[8] * pz);
    if (PIVOT) { ox = (float)((double)ox + v.px); oy = (float)((double)oy + v.py); oz = (float)((double)oz + v.pz); }
    sc.px[i] = ox; sc.py[i] = oy; sc.pz[i] = oz;
    const float4 r = sc.rot[i];  // (w, x, y, z)
    // rotation.multiply(Quaternion(r1, r2, r3, r0)), Quaternion.ts:39-55
    const double w1 = w, x1 = x, y1 = y, z1 = z, w2 = r.x, x2 = r.y, y2 = r.z, z2 = r.w;
    float4 nr;
    nr.y = (float)(w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2);
    nr.z = (float)(w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2);
    nr.w = (float)(w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2);
    nr.x = (float)(w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2);
    sc.rot[i] = nr;
    uint32_t c0, c1, c2;
    pack_cov(nr, sc.scl[i], c0, c1, c2);
    sc.cov0[i] = c0; sc.cov1[i] = c1; sc.cov2[i] = c2;
}

// Scene.scale (Scene.ts:259-305)
template <bool PIVOT>
__device__ __forceinline__ void splat_scale(const SceneDev& sc, uint32_t i, double sx, double sy, double sz, const SplatPivot& v)
{
    double px = sc.px[i], py = sc.py[i], pz = sc.pz[i];
    if (PIVOT) { px = (float)(px + v.mx); py = (float)(py + v.my); pz = (float)(pz + v.mz); }
    float ox = (float)(px * sx), oy = (float)(py * sy), oz = (float)(pz * sz);
    if (PIVOT) { ox = (float)((double)ox + v.px); oy = (float)((double)oy + v.py); oz = (float)((double)oz + v.pz); }
    sc.px[i] = ox; sc.py[i] = oy; sc.pz[i] = oz;
    float4 s = sc.scl[i];
    s.x = (float)((double)s.x * sx); s.y = (float)((double)s.y * sy); s.z = (float)((double)s.z * sz);
    sc.scl[i] = s;
    uint32_t c0, c1, c2;
    pack_cov(sc.rot[i], s, c0, c1, c2);
    sc.cov0[i] = c0; sc.cov1[i] = c1; sc.cov2[i] = c2;
}

}  // namespace gsr
