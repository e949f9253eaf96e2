// What a kernel does to ONE splat of the SoA scene, and how it reads a one-bit-per-splat set: each contract stated once, beside
// k_pack_cov.h and by the same rule.  Scene.translate / rotate / scale (src/core/Scene.ts:182-305) for the whole scene (k_scene.hip)
// and for the selected splats (k_edit.hip) are the same functions, so "everything selected, no pivot" IS the whole-scene transform;
// the row copy serves the compaction (k_scene.hip) and the growth (k_append.hip); the set layout serves every kernel that reads a
// selection or a hidden set; the scope of an analysis call, a picker's mask store and the workgroup reductions serve the analysis
// units (k_attr, k_neighbours, k_knn, k_clusters, k_merge) and the pickers.  f64 in the reference's order of operations, f32
// wherever the reference stores into a Float32Array; the units that include it are compiled with -ffp-contract=off.
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

// ---- bounds sites of shared code.  The bounds twin (GSR_BOUND, gsr_internal.h) counts per translation unit and site, so a helper
// that indexes for its includer takes the includer's sites as a template parameter, as the second walk does (k_depth_walk.h): a
// struct of static __device__ __forceinline__ members, one per shared site, declared beside the unit's GSR_BOUNDS_DECL --
//     struct xx_sites { static .. void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(xx, 5, idx, limit); } .. };
// The members: bound_set_word (a word of the selection or the hidden set), bound_mask_word (a word of a stored mask), bound_counter
// (a global histogram counter), bound_bucket and bound_entry (k_neighbours.h).  A unit declares those its helpers use, so every site
// stays in its own unit's counters under its own number, and the literal GSR_BOUND stays in the unit's file.  In the shipped build
// every member is empty.

// ---- the scope of an analysis call ----
// the bits of word wi whose splats are in scope: below n, selected (ATTR_SCOPE_SELECTED; no words: nothing is), not hidden
// (ATTR_SCOPE_VISIBLE; no words: nothing is hidden)
template <class Sites>
__device__ __forceinline__ uint32_t scope_word(const AttrScope& sc, uint32_t n, uint32_t wi)
{
    uint32_t m = set_live_bits(n, wi);
    if (!m) return 0u;
    if (sc.flags & ATTR_SCOPE_SELECTED) {
        if (!sc.sel) return 0u;
        Sites::bound_set_word(wi, sc.sel_words);
        m &= set_word(sc.sel, sc.sel_words, n, wi);
    }
    if (m && (sc.flags & ATTR_SCOPE_VISIBLE) && sc.hid) {
        Sites::bound_set_word(wi, sc.hid_words);
        m &= ~set_word(sc.hid, sc.hid_words, n, wi);
    }
    return m;
}
// is splat i (any i: at and above n never) in scope?  The selection word and the hidden word of i >> 5 are the same over each
// half of a wave64, so a wave whose 64 splats are all out of scope has no lane left behind the test and loads nothing of the scene
template <class Sites>
__device__ __forceinline__ bool in_scope(const AttrScope& sc, uint32_t n, uint64_t i)
{
    if (i >= n) return false;
    return (scope_word<Sites>(sc, n, (uint32_t)(i >> 5)) & (1u << ((uint32_t)i & 31u))) != 0u;
}

// ---- a picker's mask: one lane per bit, so that every word is stored and the caller need not zero it ----
// A wave's 64-bit ballot m IS the two whole words of the mask that its lanes cover: lane 0 stores them, no atomics.  i: the
// lane's own bit (lane 0's is a multiple of 64, its word even); lanes at and above n have voted 0.  Whole waves call it together.
template <class Sites>
__device__ __forceinline__ void mask_store_ballot(uint32_t* __restrict__ words, uint32_t nwords, uint32_t i, uint64_t m)
{
    if ((threadIdx.x & 63u) != 0u) return;
    const uint32_t w = i >> 5;
    if (w < nwords) { Sites::bound_mask_word(w, nwords); words[w] = (uint32_t)m; }
    if (w + 1u < nwords) { Sites::bound_mask_word(w + 1u, nwords); words[w + 1u] = (uint32_t)(m >> 32); }
}
// the workgroups of `threads` lanes that give every bit of nwords words its lane
inline uint32_t mask_blocks(uint32_t nwords, uint32_t threads) { return (uint32_t)(((uint64_t)nwords * 32u + threads - 1u) / threads); }

// ---- wave and workgroup ----
// A workgroup's LDS histogram of `count` counters, `threads` lanes wide: zeroed and ready for every lane's relaxed workgroup-scope
// adds; at the end, once every lane's adds are in, one relaxed agent-scope add per NON-ZERO counter into global[] (results unused:
// return-less atomics; a counter nobody touched costs nothing).  limit: the extent of global[].  Every lane of the workgroup calls both.
__device__ __forceinline__ void lds_counters_zero(uint32_t* s, uint32_t count, uint32_t threads)
{
    for (uint32_t k = threadIdx.x; k < count; k += threads) s[k] = 0u;
    __syncthreads();
}
template <class Sites>
__device__ __forceinline__ void lds_counters_flush(const uint32_t* s, uint32_t count, uint32_t threads, uint32_t* global, uint32_t limit)
{
    __syncthreads();   // the workgroup's counters are final
    for (uint32_t k = threadIdx.x; k < count; k += threads) {
        const uint32_t c = s[k];
        if (!c) continue;
        Sites::bound_counter(k, limit);
        __hip_atomic_fetch_add(&global[k], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// *total += every lane's 64-bit sum: over the lanes, then the waves, then ONE relaxed agent-scope add per workgroup (none for a
// sum of zero).  Every lane of the workgroup calls it, as the last thing it does.
template <int THREADS>
__device__ __forceinline__ void workgroup_sum_u64(unsigned long long sum, unsigned long long* total)
{
    __shared__ unsigned long long s_part[THREADS / WAVE];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (int w = 1; w < THREADS / WAVE; w++) sum += s_part[w];
    if (sum) __hip_atomic_fetch_add(total, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- f32 and f64 by their bits ----
__device__ __forceinline__ bool f32_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ double f64_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ double f64_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

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
