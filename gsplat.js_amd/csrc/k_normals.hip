// Normals ("Normals"): for every splat in scope a unit surface normal and the surface variation
// l_min / (l_0 + l_1 + l_2) -- from the PCA of its k nearest neighbours within `radius` (NORMAL_KNN), or from its own shortest axis
// (NORMAL_OWN) -- and the splats whose n . axis, |n . axis| or variation lies in a closed range as a picker.  The index is
// k_neighbours.hip's, the lists are k_knn.hip's: scope, cells, the pair test, the order (d2, index) and the treatment of non-finite
// rows are theirs.
//
// The walk.  k_normals_knn takes the ENTRIES in index order, one per lane, grid-stride, and visits the 27 cells (nb_each_cell) with
// batched loads, the stored cell key compared BEFORE any f64 arithmetic, and keeps the lane's sorted (d2, j) list in lane-strided
// LDS exactly as k_knn keeps it: slot t of lane l at [t * blockDim + l], a lane touches only its own column, so there is no bank
// conflict and no barrier; the workgroup is sized by k (knn_threads).  The insertion is k_knn's, restated: k_knn.hip's text is
// pinned by its tests (a later change may state the two once).  When the walk of an entry ends the lane reads its column in
// ascending slot order and gathers px / py / pz of each listed splat twice -- once for the mean, once for the covariance about
// it -- so nothing but (d2, j) lives in LDS; then the six cyclic Jacobi sweeps of k_merge.hip's MG_ROTATE on named scalars,
// restated for the same reason; the smallest eigenvalue's column picked with compares; the orientation; the stores.  No scratch
// memory, no register array indexed by a loop variable.  valid and the variation's min / max are reduced over the wave and cost one
// integer atomic each per wave: a variation is a non-negative double, so min and max go through bit patterns (KnnInfo).  There is
// no floating-point atomic.
//
// Compiled with -ffp-contract=off like the rest of the device code: every output is a stated sequence of correctly rounded f64
// operations.
#include "gsr_internal.h"
#include "k_splat_ops.h"
#include "k_neighbours.h"   // the key, the bucket and the 27-cell walk

namespace gsr {

GSR_BOUNDS_DECL(normals)   // sites: 0 set word, 1 entry slot, 2 bucket, 3 LDS list slot, 4 global counter, 5 mask word, 6 splat row, 7 gathered row

// the sites of the shared helpers (k_splat_ops.h, k_neighbours.h)
struct normals_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(normals, 0, idx, limit); }
    static __device__ __forceinline__ void bound_bucket(unsigned long long idx, unsigned long long limit) { GSR_BOUND(normals, 2, idx, limit); }
    static __device__ __forceinline__ void bound_counter(unsigned long long idx, unsigned long long limit) { GSR_BOUND(normals, 4, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(normals, 5, idx, limit); }
};

constexpr uint32_t NORMAL_NAN_F32 = 0x7fc00000u;

// ---- what both sources end with ----
// the orientation (in f64, before the store): toward the viewpoint when there is one and s decides; otherwise the first non-zero
// component positive, gsr_fit_plane's convention
__device__ __forceinline__ void normal_orient(const NormalOrient& o, double px, double py, double pz, double& u0, double& u1, double& u2)
{
    // (selects, not branches: written as `if (flip) { u0 = -u0; .. }` behind an if / else chain, the compiled code computed the flip of the
    // first-non-zero rule and then stored the unflipped vector; as selects it is three conditional moves and the right bits)
    const double s = (u0 * (o.tx - px) + u1 * (o.ty - py)) + u2 * (o.tz - pz);
    const bool decided = o.oriented != 0u && (s < 0.0 || s > 0.0);
    const bool first_negative = u0 != 0.0 ? u0 < 0.0 : (u1 != 0.0 ? u1 < 0.0 : u2 < 0.0);
    const bool flip = decided ? s < 0.0 : first_negative;
    u0 = flip ? -u0 : u0;
    u1 = flip ? -u1 : u1;
    u2 = flip ? -u2 : u2;
}

// one row's stores
__device__ __forceinline__ void normal_store(const NormalArrays& a, uint32_t i, bool valid, double u0, double u1, double u2, double variation, uint32_t found)
{
    uint32_t* const nw = reinterpret_cast<uint32_t*>(a.normals) + (uint64_t)i * 3u;
    nw[0] = valid ? __float_as_uint((float)u0) : NORMAL_NAN_F32;
    nw[1] = valid ? __float_as_uint((float)u1) : NORMAL_NAN_F32;
    nw[2] = valid ? __float_as_uint((float)u2) : NORMAL_NAN_F32;
    a.variation[i] = valid ? variation : f64_nan();
    a.found[i] = found;
}

// a.info += the lanes' valid rows and the bit patterns of their variations: over the wave, then one integer atomic each per wave.
// Whole waves call it together.
__device__ __forceinline__ void normal_info_reduce(NormalInfo* info, uint32_t valid, unsigned long long vmax, unsigned long long nvmin)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        valid += __shfl_xor(valid, d);
        const unsigned long long ov = __shfl_xor(vmax, d), on = __shfl_xor(nvmin, d);
        vmax = ov > vmax ? ov : vmax;
        nvmin = on > nvmin ? on : nvmin;
    }
    if ((threadIdx.x & 63u) == 0u && valid) {
        __hip_atomic_fetch_add(&info->valid, valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&info->vmax, vmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&info->nvmin, nvmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the rows the walk does not reach ----
// Every row as a splat outside the index has it: no normal, no variation, found 0.  The walk then overwrites the rows of its entries.
__global__ __launch_bounds__(NB_THREADS) void k_normals_fill(uint32_t n, NormalArrays a)
{
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; i < n; i += stride) normal_store(a, (uint32_t)i, false, 0.0, 0.0, 0.0, 0.0, 0u);
}

// ---- the walk ----
constexpr uint32_t NORMAL_BATCH = 4;   // candidates whose loads are in flight together

// one cyclic Jacobi rotation on the pair (p, q), r the third index: k_merge.hip's MG_ROTATE, restated
#define NM_ROTATE(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                     \
    if (apq != 0.0) {                                                                                      \
        const double th = (aqq - app) / (2.0 * apq);                                                       \
        double t = 1.0 / (fabs(th) + __dsqrt_rn(th * th + 1.0));                                           \
        if (th < 0.0) t = -t;                                                                              \
        const double cs = 1.0 / __dsqrt_rn(t * t + 1.0), sn = t * cs;                                      \
        const double npp = app - t * apq, nqq = aqq + t * apq, nrp = cs * arp - sn * arq, nrq = sn * arp + cs * arq; \
        app = npp; aqq = nqq; apq = 0.0; arp = nrp; arq = nrq;                                             \
        const double n0p = cs * v0p - sn * v0q, n0q = sn * v0p + cs * v0q, n1p = cs * v1p - sn * v1q, n1q = sn * v1p + cs * v1q, \
                     n2p = cs * v2p - sn * v2q, n2q = sn * v2p + cs * v2q;                                 \
        v0p = n0p; v0q = n0q; v1p = n1p; v1q = n1q; v2p = n2p; v2q = n2q;                                  \
    }

__global__ __launch_bounds__(NB_THREADS) void k_normals_knn(NbIndex ix, uint32_t m /* entries */, uint32_t n /* splats */, uint32_t k, const float* __restrict__ px,
                                                            const float* __restrict__ py, const float* __restrict__ pz, NormalOrient o, NormalArrays a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_normals[];   // k * T doubles, k * T words
    const uint32_t T = blockDim.x, slots = k * T;
    double* const s_d2 = reinterpret_cast<double*>(s_normals);
    uint32_t* const s_j = reinterpret_cast<uint32_t*>(s_d2 + slots);
    double* const my_d2 = s_d2 + threadIdx.x;     // this lane's columns: slot t at [t * T]
    uint32_t* const my_j = s_j + threadIdx.x;
    const uint2* __restrict__ table = reinterpret_cast<const uint2*>(ix.table);   // (population, one behind the last entry)
    uint32_t valid_rows = 0u;
    unsigned long long vmax = 0ull, nvmin = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * T;
    for (uint64_t s = (uint64_t)blockIdx.x * T + threadIdx.x; s < m; s += stride) {
        GSR_BOUND(normals, 1, s, m);
        const uint4 me = ix.entry[s];
        const double x = (double)__uint_as_float(me.x), y = (double)__uint_as_float(me.y), z = (double)__uint_as_float(me.z);
        uint32_t found = 0u, wj = 0u;   // the list's length; (wd, wj): its last pair once it is full
        double wd = 0.0;
        nb_each_cell<normals_sites>(ix.key[s], ix.bucket_mask, [&](unsigned long long nk, uint32_t b) {
            const uint2 t = table[b];
            GSR_BOUND(normals, 1, t.y, (uint64_t)m + 1u);
            if (t.y > m || t.x > t.y) return true;   // (never: a range of the entry array)
            // NORMAL_BATCH candidates at a time, their keys and entries loaded together in front of any use (a slot behind the
            // range's end repeats the last one and is skipped below)
            for (uint32_t e0 = t.y - t.x; e0 < t.y; e0 += NORMAL_BATCH) {
                unsigned long long ck[NORMAL_BATCH];
                uint4 co[NORMAL_BATCH];
#pragma unroll
                for (uint32_t u = 0u; u < NORMAL_BATCH; u++) {
                    const uint32_t eu = min(e0 + u, t.y - 1u);
                    ck[u] = ix.key[eu];
                    co[u] = ix.entry[eu];
                }
#pragma unroll
                for (uint32_t u = 0u; u < NORMAL_BATCH; u++) {
                    const uint32_t e = e0 + u;
                    if (e >= t.y || ck[u] != nk || e == (uint32_t)s) continue;
                    const uint4 c = co[u];
                    const double ex = x - (double)__uint_as_float(c.x), ey = y - (double)__uint_as_float(c.y), ez = z - (double)__uint_as_float(c.z);
                    const double d = (ex * ex + ey * ey) + ez * ez;
                    const uint32_t j = c.w;
                    if (!(d <= ix.r2)) continue;
                    if (found == k && !(d < wd || (d == wd && j < wj))) continue;
                    // the slot that opens is the one behind the list, or the worst's; pairs above (d, j) move up one slot into it
                    uint32_t at = found < k ? found : k - 1u;
                    while (at > 0u) {
                        GSR_BOUND(normals, 3, at * T + threadIdx.x, slots);
                        const double pd = my_d2[(at - 1u) * T];
                        const uint32_t pj = my_j[(at - 1u) * T];
                        if (pd < d || (pd == d && pj < j)) break;
                        my_d2[at * T] = pd;
                        my_j[at * T] = pj;
                        at--;
                    }
                    GSR_BOUND(normals, 3, at * T + threadIdx.x, slots);
                    my_d2[at * T] = d;
                    my_j[at * T] = j;
                    if (found < k) found++;
                    if (found == k) { wd = my_d2[(k - 1u) * T]; wj = my_j[(k - 1u) * T]; }
                }
            }
            return true;
        });
        // the neighbourhood: the splat itself, then its list in ascending slot order; a listed index is a splat's (below n: the build
        // stored it), and one that is not is left out of both passes alike
        const double M = (double)(found + 1u);
        double sx = x, sy = y, sz = z;
        for (uint32_t t = 0u; t < found; t++) {
            GSR_BOUND(normals, 3, t * T + threadIdx.x, slots);
            const uint32_t j = my_j[t * T];
            GSR_BOUND(normals, 7, j, n);
            if (j >= n) continue;
            sx = sx + (double)px[j]; sy = sy + (double)py[j]; sz = sz + (double)pz[j];
        }
        const double mx = sx / M, my = sy / M, mz = sz / M;
        double a00, a01, a02, a11, a12, a22;
        {
            const double dx = x - mx, dy = y - my, dz = z - mz;
            a00 = 0.0 + dx * dx; a01 = 0.0 + dx * dy; a02 = 0.0 + dx * dz; a11 = 0.0 + dy * dy; a12 = 0.0 + dy * dz; a22 = 0.0 + dz * dz;
        }
        for (uint32_t t = 0u; t < found; t++) {
            const uint32_t j = my_j[t * T];
            if (j >= n) continue;
            const double dx = (double)px[j] - mx, dy = (double)py[j] - my, dz = (double)pz[j] - mz;
            a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz; a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz;
        }
        a00 = a00 / M; a01 = a01 / M; a02 = a02 / M; a11 = a11 / M; a12 = a12 / M; a22 = a22 / M;
        // six cyclic sweeps; V = I
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
        for (int sweep = 0; sweep < 6; sweep++) {
            NM_ROTATE(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)   // (0, 1), r = 2
            NM_ROTATE(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)   // (0, 2), r = 1
            NM_ROTATE(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)   // (1, 2), r = 0
        }
        const double l0 = a00 > 0.0 ? a00 : 0.0, l1 = a11 > 0.0 ? a11 : 0.0, l2 = a22 > 0.0 ? a22 : 0.0;
        const double tot = (l0 + l1) + l2;
        // the smallest c with l_c minimal, by compares; u is column c of V
        double lm = l0, u0 = v00, u1 = v10, u2 = v20;
        if (l1 < lm) { lm = l1; u0 = v01; u1 = v11; u2 = v21; }
        if (l2 < lm) { lm = l2; u0 = v02; u1 = v12; u2 = v22; }
        const bool valid = found >= 2u && tot > 0.0;
        const double variation = lm / tot;
        normal_orient(o, x, y, z, u0, u1, u2);
        GSR_BOUND(normals, 6, me.w, n);
        if (me.w < n) normal_store(a, me.w, valid, u0, u1, u2, variation, found);
        if (valid) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(variation);
            valid_rows++;
            vmax = bits > vmax ? bits : vmax;
            nvmin = ~bits > nvmin ? ~bits : nvmin;
        }
    }
    normal_info_reduce(a.info, valid_rows, vmax, nvmin);
}
#undef NM_ROTATE

// ---- the splat's own shortest axis ----
// Elementwise, one splat per lane, grid-stride.  The selection word and the hidden word of i >> 5 are the same over each half of a
// wave64, so a run of 64 splats out of scope has no lane left behind in_scope and reads nothing of the scene.  The rotation matrix
// is splat_cov's (k_pack_cov.h), in its written order; the axis of scale c is its row c.  Every row is stored: no fill in front of
// it.  The kernel is a few tens of microseconds of memory traffic, so its five totals are folded per WORKGROUP -- lanes in
// registers over the stride, waves by __shfl_xor, the workgroup through LDS -- and the min / max atomics are skipped when a plain
// load shows the word at or beyond the workgroup's value already (the words only grow): with one set of atomics per wave of 64
// splats the same-address atomics, not the memory, bounded the kernel (0.72 ms at 1 M splats).
__global__ __launch_bounds__(NB_THREADS) void k_normals_own(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                            const float4* __restrict__ rot, const float4* __restrict__ scl, AttrScope sc, uint32_t n, NormalOrient o,
                                                            NormalArrays a)
{
    __shared__ unsigned long long s_part[NB_THREADS / WAVE][4];   // per wave: in_scope | nonfinite << 32, valid, vmax, nvmin
    uint32_t in = 0u, nonfinite = 0u, valid_rows = 0u;
    unsigned long long vmax = 0ull, nvmin = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; i < n; i += stride) {
        GSR_BOUND(normals, 6, i, n);
        if (!in_scope<normals_sites>(sc, n, i)) {
            normal_store(a, (uint32_t)i, false, 0.0, 0.0, 0.0, 0.0, 0u);
            continue;
        }
        in++;
        const float fx = px[i], fy = py[i], fz = pz[i];
        const float4 r = rot[i], s = scl[i];
        const bool pos_ok = f32_finite(fx) && f32_finite(fy) && f32_finite(fz);
        nonfinite += pos_ok ? 0u : 1u;
        const bool finite = pos_ok && f32_finite(r.x) && f32_finite(r.y) && f32_finite(r.z) && f32_finite(r.w) && f32_finite(s.x) && f32_finite(s.y) && f32_finite(s.z);
        const double l0 = fabs((double)s.x) * fabs((double)s.x), l1 = fabs((double)s.y) * fabs((double)s.y), l2 = fabs((double)s.z) * fabs((double)s.z);
        const double tot = (l0 + l1) + l2;
        const double qx = r.y, qy = r.z, qz = r.w, qw = -(double)r.x;   // Quaternion(r1, r2, r3, -r0)
        // the smallest c with l_c minimal, by compares; the axis is row c of the matrix
        double lm = l0;
        double a0 = 1 - 2 * qy * qy - 2 * qz * qz, a1 = 2 * qx * qy - 2 * qz * qw, a2 = 2 * qx * qz + 2 * qy * qw;
        if (l1 < lm) { lm = l1; a0 = 2 * qx * qy + 2 * qz * qw; a1 = 1 - 2 * qx * qx - 2 * qz * qz; a2 = 2 * qy * qz - 2 * qx * qw; }
        if (l2 < lm) { lm = l2; a0 = 2 * qx * qz - 2 * qy * qw; a1 = 2 * qy * qz + 2 * qx * qw; a2 = 1 - 2 * qx * qx - 2 * qy * qy; }
        const double nrm = __dsqrt_rn((a0 * a0 + a1 * a1) + a2 * a2);
        const bool turned = r.x != 0.0f || r.y != 0.0f || r.z != 0.0f || r.w != 0.0f;   // (a zero quaternion is no rotation: the formula alone would give the identity)
        const bool valid = finite && turned && tot > 0.0 && nrm > 0.0 && nrm < f64_inf();
        double u0 = a0 / nrm, u1 = a1 / nrm, u2 = a2 / nrm;
        const double variation = lm / tot;
        normal_orient(o, (double)fx, (double)fy, (double)fz, u0, u1, u2);
        normal_store(a, (uint32_t)i, valid, u0, u1, u2, variation, 0u);
        if (valid) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(variation);
            valid_rows++;
            vmax = bits > vmax ? bits : vmax;
            nvmin = ~bits > nvmin ? ~bits : nvmin;
        }
    }
    unsigned long long counts = (unsigned long long)in | (unsigned long long)nonfinite << 32, valid_sum = valid_rows;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        counts += __shfl_xor(counts, d);
        valid_sum += __shfl_xor(valid_sum, d);
        const unsigned long long ov = __shfl_xor(vmax, d), on = __shfl_xor(nvmin, d);
        vmax = ov > vmax ? ov : vmax;
        nvmin = on > nvmin ? on : nvmin;
    }
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* const mine = s_part[threadIdx.x >> 6];
        mine[0] = counts; mine[1] = valid_sum; mine[2] = vmax; mine[3] = nvmin;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (int w = 1; w < NB_THREADS / WAVE; w++) {
        counts += s_part[w][0];
        valid_sum += s_part[w][1];
        vmax = s_part[w][2] > vmax ? s_part[w][2] : vmax;
        nvmin = s_part[w][3] > nvmin ? s_part[w][3] : nvmin;
    }
    const uint32_t in_wg = (uint32_t)counts, nonfinite_wg = (uint32_t)(counts >> 32);
    if (in_wg) __hip_atomic_fetch_add(&a.info->in_scope, in_wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nonfinite_wg) __hip_atomic_fetch_add(&a.info->nonfinite, nonfinite_wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!valid_sum) return;
    __hip_atomic_fetch_add(&a.info->valid, (uint32_t)valid_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (vmax > __hip_atomic_load(&a.info->vmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_max(&a.info->vmax, vmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nvmin > __hip_atomic_load(&a.info->nvmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_max(&a.info->nvmin, nvmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the picker ----
// gsr_select_normal.  One thread per bit of the mask; the value comes from the STORED f32 normal widened to f64, so a host holding
// gsr_normals' output reproduces it exactly.  A row without a normal holds NaN and fails every comparison: outside the scope, not
// finite or not valid, it is never picked.  A wave's ballot is two whole words (mask_store_ballot): every word of the mask is stored.
__global__ __launch_bounds__(NB_THREADS) void k_normals_select(const float* __restrict__ normals, const double* __restrict__ variation, uint32_t n, int stat, double ax,
                                                               double ay, double az, double lo, double hi, uint32_t* __restrict__ scratch, uint32_t nwords)
{
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    bool in = false;
    if (i < n) {
        GSR_BOUND(normals, 6, i, n);
        double v;
        if (stat == NORMAL_VARIATION) {
            v = variation[i];
        } else {
            const double nx = (double)normals[(uint64_t)i * 3u], ny = (double)normals[(uint64_t)i * 3u + 1u], nz = (double)normals[(uint64_t)i * 3u + 2u];
            v = (nx * ax + ny * ay) + nz * az;
            if (stat == NORMAL_ABS_DOT) v = fabs(v);
        }
        in = lo <= v && v <= hi;
    }
    mask_store_ballot<normals_sites>(scratch, nwords, i, __ballot(in));
}

// ---- launchers ----
void launch_normals_fill(uint32_t n, const NormalArrays& a, int cu_count, hipStream_t s)
{
    hipLaunchKernelGGL(k_normals_fill, dim3(nb_grid(n, cu_count)), dim3(NB_THREADS), 0, s, n, a);
}

void launch_normals_knn(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t k, const float* px, const float* py, const float* pz, const NormalOrient& o,
                        const NormalArrays& a, int cu_count, hipStream_t s)
{
    if (!indexed) return;
    const uint32_t threads = knn_threads(k);
    const uint32_t blocks = nb_grid((uint64_t)indexed * (NB_THREADS / threads), cu_count);   // (nb_grid counts in workgroups of NB_THREADS)
    const size_t lds = (size_t)k * threads * 12u;
    hipLaunchKernelGGL(k_normals_knn, dim3(blocks), dim3(threads), lds, s, ix, indexed, n, k, px, py, pz, o, a);
}

void launch_normals_own(const SceneDev& scene, const AttrScope& sc, uint32_t n, const NormalOrient& o, const NormalArrays& a, int cu_count, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_normals_own, dim3(nb_grid(n, cu_count)), dim3(NB_THREADS), 0, s, scene.px, scene.py, scene.pz, scene.rot, scene.scl, sc, n, o, a);
}

void launch_normals_select(const float* normals, const double* variation, uint32_t n, int stat, const double* axis, double lo, double hi, uint32_t* scratch,
                           uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_normals_select, dim3(mask_blocks(nwords, NB_THREADS)), dim3(NB_THREADS), 0, s, normals, variation, n, stat, axis ? axis[0] : 0.0,
                       axis ? axis[1] : 0.0, axis ? axis[2] : 0.0, lo, hi, scratch, nwords);
}

}  // namespace gsr
