// Matching and registration ("Matching and registration"): for every splat in scope of a SOURCE scene, moved by
// a trial transform M (3 x 4, f64), the nearest indexed splat of a TARGET scene within `radius` -- the first operation here that
// relates two scenes.  The index is k_neighbours.hip's, as it is, built over the TARGET's positions and scope: cells, key, bucket,
// the 27-cell walk and the f64 pair test are its own (k_neighbours.h), and a query's cell is nb_cell_query's.
//
// The point.  T_k = ((M[k][0]*x + M[k][1]*y) + M[k][2]*z) + M[k][3] on the stored f32 position as doubles, in the written order,
// uncontracted (match_point): the one statement every kernel below goes through, so the bound, the walk and the tree see one T.
// A source splat is a query iff it is in scope, its three floats are finite and its three T_k are; the others in scope are
// `nonfinite` and unmatched.
//
// The walk.  k_match takes the SOURCE splats in stored order, one per lane, grid-stride, and visits the 27 cells around the
// query's (nb_each_near_query: one 8-byte (population, end) load per cell, NB_QUERY_BATCH candidates' keys and entries loaded
// together, the stored cell key compared BEFORE any f64 arithmetic).  The best pair (d2, j) stays in two registers: no list, no
// LDS, no scratch memory.  The pair order is total over distinct target splats, so the match does not depend on the visiting
// order.  matched, min and max are reduced over the wave and cost one atomic each per wave (MatchInfo: d2 is non-negative, so
// min and max go through the bit patterns as 64-bit unsigned maxima).  Lanes of a wave take source splats in stored order, so
// their walks diverge unless the capture is stored spatially coherently: a first form.
//
// The sums.  A matched splat's row is (T, Q, T_a * Q_b for ab = 00, 01, .., 22, d2), every other splat's is sixteen +0.0, and the
// rows 0 .. n-1 are summed by a fixed tree: groups of MATCH_GROUP consecutive rows, the last padded with +0.0; within a group, for
// s = 128, 64, .., 1: x[l] = x[l] + x[l + s] for l < s; the group results reduced the same way until one row is left.  f64
// addition is commutative and no NaN can enter, so the tree, not the visiting order, decides the bits.  s = 128, 64 go through
// LDS, s = 32 .. 1 through __shfl_down in the first wave (tree_reduce).  Level 1 (k_match_rows) rebuilds each row from idx[i]
// and d2[i]; the further levels (k_match_tree) read the partial rows.  1 M splats are three launches.
//
//
// Point to plane ("Point-to-plane registration").  The same match, reduced to the sums of a 6 x 6 linear solve
// along the TARGET's normals: a row is 29 doubles (J_a * J_b for a <= b, J_a * r, r * r, d2 with J = (T x n, n), r = n . (T - Q)),
// non-zero iff the splat is matched and its match has a normal.  tree_reduce and tree_level are templates over the row width; a
// component's tree does not depend on the other components, so the 29-wide tree is the 16-wide one per component.  One pass: 29 x
// 256 doubles of LDS (59 392 bytes).  k_match_surface_rows also counts its non-zero rows, one atomic per wave.
//
// Compiled with -ffp-contract=off like the rest of the device code.
#include "gsr_internal.h"
#include "k_splat_ops.h"
#include "k_neighbours.h"   // the key, the bucket, the 27-cell walk and the query walk

namespace gsr {

GSR_BOUNDS_DECL(match)   // sites: 0 set word, 1 source row, 2 bucket, 3 entry slot, 4 target row, 5 partial row, 6 selection word, 7 LDS cell
GSR_BOUNDS_DECL(match_surface)   // the sites behind those eight, in words of their own: 8 (word 0) the target's normal row

// the sites of the shared helpers (k_splat_ops.h, k_neighbours.h)
struct match_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(match, 0, idx, limit); }
    static __device__ __forceinline__ void bound_bucket(unsigned long long idx, unsigned long long limit) { GSR_BOUND(match, 2, idx, limit); }
    static __device__ __forceinline__ void bound_entry(unsigned long long idx, unsigned long long limit) { GSR_BOUND(match, 3, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(match, 6, idx, limit); }
};

__device__ __forceinline__ bool f64_finite(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// ---- the transformed source point ----
// false: source splat i (i < n) is no query.  The written order is the header's.
__device__ __forceinline__ bool match_point(const MatchSource& src, uint64_t i, double& tx, double& ty, double& tz)
{
    GSR_BOUND(match, 1, i, src.n);
    const float fx = src.px[i], fy = src.py[i], fz = src.pz[i];
    if (!(f32_finite(fx) && f32_finite(fy) && f32_finite(fz))) return false;
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const double* m = src.xf.m;
    tx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    ty = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    tz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    return f64_finite(tx) && f64_finite(ty) && f64_finite(tz);
}

__device__ __forceinline__ unsigned long long match_key(const NbIndex& ix, double tx, double ty, double tz)
{
    return nb_key(nb_cell_query(tx, ix.inv_h), nb_cell_query(ty, ix.inv_h), nb_cell_query(tz, ix.inv_h));
}

// ---- the bound ----
// What k_match walks at most: per query the populations of its 27 buckets, a bucket two cells share counted twice, as the walk
// visits it twice.  Also the call's counts of source splats in scope and of those that are no query.
__global__ __launch_bounds__(NB_THREADS) void k_match_bound(NbIndex ix, MatchSource src, MatchInfo* __restrict__ info)
{
    uint32_t scoped = 0u, nonfinite = 0u;
    unsigned long long sum = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; i < src.n; i += stride) {
        if (!in_scope<match_sites>(src.sc, src.n, i)) continue;
        scoped++;
        double tx, ty, tz;
        if (!match_point(src, i, tx, ty, tz)) { nonfinite++; continue; }
        nb_each_cell<match_sites>(match_key(ix, tx, ty, tz), ix.bucket_mask, [&](unsigned long long, uint32_t b) { sum += ix.table[2ull * b]; return true; });
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { scoped += __shfl_xor(scoped, d); nonfinite += __shfl_xor(nonfinite, d); }
    if ((threadIdx.x & 63u) == 0u) {
        if (scoped) __hip_atomic_fetch_add(&info->in_scope, scoped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nonfinite) __hip_atomic_fetch_add(&info->nonfinite, nonfinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    workgroup_sum_u64<NB_THREADS>(sum, &info->pair_bound);
}

// ---- the walk ----
__global__ __launch_bounds__(NB_THREADS) void k_match(NbIndex ix, uint32_t m /* entries */, MatchSource src, uint32_t* __restrict__ idx, double* __restrict__ d2,
                                                      MatchInfo* __restrict__ info)
{
    uint32_t matched = 0u;
    unsigned long long vmax = 0ull, nvmin = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; i < src.n; i += stride) {
        uint32_t bj = MATCH_NONE;
        double bd = f64_nan();   // outside the scope
        if (in_scope<match_sites>(src.sc, src.n, i)) {
            bd = f64_inf();
            double tx, ty, tz;
            if (match_point(src, i, tx, ty, tz)) {
                nb_each_near_query<match_sites>(ix, m, match_key(ix, tx, ty, tz), tx, ty, tz, [&](uint32_t j, double d) {
                    if (d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
                });
            }
        }
        GSR_BOUND(match, 1, i, src.n);
        idx[i] = bj;
        d2[i] = bd;
        if (bj != MATCH_NONE) {
            matched++;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(bd);
            vmax = bits > vmax ? bits : vmax;
            nvmin = ~bits > nvmin ? ~bits : nvmin;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        matched += __shfl_xor(matched, d);
        const unsigned long long ov = __shfl_xor(vmax, d), on = __shfl_xor(nvmin, d);
        vmax = ov > vmax ? ov : vmax;
        nvmin = on > nvmin ? on : nvmin;
    }
    if ((threadIdx.x & 63u) == 0u && matched) {
        __hip_atomic_fetch_add(&info->matched, matched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&info->d2max, vmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&info->nd2min, nvmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the tree ----
// One group: every lane's row v of W doubles summed into out[0 .. W) by the tree of the header.  s_rows: W * MATCH_GROUP doubles,
// component c of lane l at [c * MATCH_GROUP + l] (consecutive lanes on consecutive banks).  Every lane of the workgroup calls it.
template <uint32_t W>
__device__ __forceinline__ void tree_reduce(double (&v)[W], double* s_rows, double* __restrict__ out)
{
    const uint32_t l = threadIdx.x;
#pragma unroll
    for (uint32_t c = 0u; c < W; c++) s_rows[c * MATCH_GROUP + l] = v[c];
    __syncthreads();
    if (l < 128u) {
#pragma unroll
        for (uint32_t c = 0u; c < W; c++) {
            GSR_BOUND(match, 7, c * MATCH_GROUP + l + 128u, W * MATCH_GROUP);
            s_rows[c * MATCH_GROUP + l] = s_rows[c * MATCH_GROUP + l] + s_rows[c * MATCH_GROUP + l + 128u];
        }
    }
    __syncthreads();
    if (l >= 64u) return;   // the first wave, whole
#pragma unroll
    for (uint32_t c = 0u; c < W; c++) v[c] = s_rows[c * MATCH_GROUP + l] + s_rows[c * MATCH_GROUP + l + 64u];
    // x[l] = x[l] + x[l + s] for l < s: a lane at or above s adds what no lane below the next s reads
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (uint32_t c = 0u; c < W; c++) v[c] = v[c] + __shfl_down(v[c], s);
    }
    if (l != 0u) return;
#pragma unroll
    for (uint32_t c = 0u; c < W; c++) out[c] = v[c];
}

// level 1: group g = rows [256 g, 256 g + 256) of the source, rebuilt from idx[] and d2[]
__global__ __launch_bounds__(MATCH_GROUP) void k_match_rows(MatchSource src, const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
                                                            uint32_t tn, const uint32_t* __restrict__ idx, const double* __restrict__ d2, double* __restrict__ out,
                                                            uint32_t groups)
{
    __shared__ double s_rows[MATCH_ROW * MATCH_GROUP];
    double v[MATCH_ROW];
#pragma unroll
    for (uint32_t c = 0u; c < MATCH_ROW; c++) v[c] = 0.0;
    const uint64_t i = (uint64_t)blockIdx.x * MATCH_GROUP + threadIdx.x;
    if (i < src.n) {
        const uint32_t j = idx[i];
        double t[3];
        if (j != MATCH_NONE) GSR_BOUND(match, 4, j, tn);
        if (j < tn && match_point(src, i, t[0], t[1], t[2])) {   // (a match is a query: its point is finite)
            const double q[3] = {(double)qx[j], (double)qy[j], (double)qz[j]};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                v[a] = t[a];
                v[3 + a] = q[a];
#pragma unroll
                for (int b = 0; b < 3; b++) v[6 + 3 * a + b] = t[a] * q[b];
            }
            v[15] = d2[i];
        }
    }
    GSR_BOUND(match, 5, blockIdx.x, groups);
    tree_reduce(v, s_rows, out + (uint64_t)blockIdx.x * MATCH_ROW);
}

// a further level: group g = rows [256 g, 256 g + 256) of `in`, `count` rows of W doubles
template <uint32_t W>
__device__ __forceinline__ void tree_level(const double* __restrict__ in, uint32_t count, double* __restrict__ out, uint32_t groups, double* s_rows)
{
    double v[W];
    const uint64_t i = (uint64_t)blockIdx.x * MATCH_GROUP + threadIdx.x;
#pragma unroll
    for (uint32_t c = 0u; c < W; c++) v[c] = i < count ? in[i * W + c] : 0.0;
    GSR_BOUND(match, 5, blockIdx.x, groups);
    tree_reduce(v, s_rows, out + (uint64_t)blockIdx.x * W);
}

__global__ __launch_bounds__(MATCH_GROUP) void k_match_tree(const double* __restrict__ in, uint32_t count, double* __restrict__ out, uint32_t groups)
{
    __shared__ double s_rows[MATCH_ROW * MATCH_GROUP];
    tree_level<MATCH_ROW>(in, count, out, groups, s_rows);
}

// ---- the point-to-plane tree ----
// level 1: the row of source splat i from idx[i], d2[i], the target's position and the target's stored normal.  A NaN n_x is "no
// normal": nothing of that row is computed, so no NaN enters the tree.
__global__ __launch_bounds__(MATCH_GROUP) void k_match_surface_rows(MatchSource src, const float* __restrict__ qx, const float* __restrict__ qy,
                                                                    const float* __restrict__ qz, const float* __restrict__ normals, uint32_t tn,
                                                                    const uint32_t* __restrict__ idx, const double* __restrict__ d2, double* __restrict__ out,
                                                                    uint32_t groups, MatchInfo* __restrict__ info)
{
    __shared__ double s_rows[MATCH_SURFACE_ROW * MATCH_GROUP];
    double v[MATCH_SURFACE_ROW];
#pragma unroll
    for (uint32_t c = 0u; c < MATCH_SURFACE_ROW; c++) v[c] = 0.0;
    bool surface = false;
    const uint64_t i = (uint64_t)blockIdx.x * MATCH_GROUP + threadIdx.x;
    if (i < src.n) {
        const uint32_t j = idx[i];
        double t[3];
        if (j != MATCH_NONE) GSR_BOUND(match, 4, j, tn);
        if (j < tn && match_point(src, i, t[0], t[1], t[2])) {   // (a match is a query: its point is finite)
            GSR_BOUND(match_surface, 0, 3ull * j + 2ull, 3ull * tn);
            const float fx = normals[3ull * j], fy = normals[3ull * j + 1ull], fz = normals[3ull * j + 2ull];
            if (fx == fx) {
                const double n[3] = {(double)fx, (double)fy, (double)fz};
                const double e[3] = {t[0] - (double)qx[j], t[1] - (double)qy[j], t[2] - (double)qz[j]};
                const double r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
                const double J[6] = {t[1] * n[2] - t[2] * n[1], t[2] * n[0] - t[0] * n[2], t[0] * n[1] - t[1] * n[0], n[0], n[1], n[2]};
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int b = a; b < 6; b++) v[6 * a - a * (a - 1) / 2 + (b - a)] = J[a] * J[b];   // 00, 01, .., 05, 11, .., 55
                }
#pragma unroll
                for (int a = 0; a < 6; a++) v[21 + a] = J[a] * r;
                v[27] = r * r;
                v[28] = d2[i];
                surface = true;
            }
        }
    }
    const uint32_t rows = (uint32_t)__popcll(__ballot(surface));
    if ((threadIdx.x & 63u) == 0u && rows) __hip_atomic_fetch_add(&info->surface, rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    GSR_BOUND(match, 5, blockIdx.x, groups);
    tree_reduce(v, s_rows, out + (uint64_t)blockIdx.x * MATCH_SURFACE_ROW);
}

__global__ __launch_bounds__(MATCH_GROUP) void k_match_surface_tree(const double* __restrict__ in, uint32_t count, double* __restrict__ out, uint32_t groups)
{
    __shared__ double s_rows[MATCH_SURFACE_ROW * MATCH_GROUP];
    tree_level<MATCH_SURFACE_ROW>(in, count, out, groups, s_rows);
}

// ---- the picker ----
// gsr_select_match.  One thread per bit of the mask: in scope, lo <= v && (v < hi || hi is +inf) with v = sqrt(d2), correctly
// rounded (+inf for an unmatched splat).  A wave's ballot is two whole words (mask_store_ballot): every word of the mask is stored.
__global__ __launch_bounds__(NB_THREADS) void k_match_select(const double* __restrict__ d2, AttrScope sc, uint32_t n, double lo, double hi, uint32_t open_hi,
                                                             uint32_t* __restrict__ scratch, uint32_t nwords)
{
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    bool in = false;
    if (in_scope<match_sites>(sc, n, i)) {
        GSR_BOUND(match, 1, i, n);
        const double v = __dsqrt_rn(d2[i]);
        in = lo <= v && (v < hi || open_hi != 0u);
    }
    mask_store_ballot<match_sites>(scratch, nwords, i, __ballot(in));
}

// ---- launchers ----
void launch_match_bound(const NbIndex& ix, const MatchSource& src, MatchInfo* info, int cu_count, hipStream_t s)
{
    if (!src.n) return;
    hipLaunchKernelGGL(k_match_bound, dim3(nb_grid(src.n, cu_count)), dim3(NB_THREADS), 0, s, ix, src, info);
}

void launch_match(const NbIndex& ix, uint32_t indexed, const MatchSource& src, uint32_t* idx, double* d2, MatchInfo* info, int cu_count, hipStream_t s)
{
    if (!src.n) return;
    hipLaunchKernelGGL(k_match, dim3(nb_grid(src.n, cu_count)), dim3(NB_THREADS), 0, s, ix, indexed, src, idx, d2, info);
}

void launch_match_tree(const MatchSource& src, const float* qx, const float* qy, const float* qz, uint32_t tn, const uint32_t* idx, const double* d2,
                       double* partial, hipStream_t s)
{
    uint32_t groups = (uint32_t)(((uint64_t)src.n + MATCH_GROUP - 1u) / MATCH_GROUP);
    hipLaunchKernelGGL(k_match_rows, dim3(groups), dim3(MATCH_GROUP), 0, s, src, qx, qy, qz, tn, idx, d2, partial, groups);
    const double* in = partial;
    uint64_t behind = groups;   // rows of the levels so far
    for (uint32_t count = groups; count > 1u;) {
        groups = (count + MATCH_GROUP - 1u) / MATCH_GROUP;
        double* out = partial + behind * MATCH_ROW;
        hipLaunchKernelGGL(k_match_tree, dim3(groups), dim3(MATCH_GROUP), 0, s, in, count, out, groups);
        in = out;
        behind += groups;
        count = groups;
    }
}

void launch_match_surface_tree(const MatchSource& src, const float* qx, const float* qy, const float* qz, const float* normals, uint32_t tn, const uint32_t* idx,
                               const double* d2, double* partial, MatchInfo* info, hipStream_t s)
{
    uint32_t groups = (uint32_t)(((uint64_t)src.n + MATCH_GROUP - 1u) / MATCH_GROUP);
    hipLaunchKernelGGL(k_match_surface_rows, dim3(groups), dim3(MATCH_GROUP), 0, s, src, qx, qy, qz, normals, tn, idx, d2, partial, groups, info);
    const double* in = partial;
    uint64_t behind = groups;   // rows of the levels so far
    for (uint32_t count = groups; count > 1u;) {
        groups = (count + MATCH_GROUP - 1u) / MATCH_GROUP;
        double* out = partial + behind * MATCH_SURFACE_ROW;
        hipLaunchKernelGGL(k_match_surface_tree, dim3(groups), dim3(MATCH_GROUP), 0, s, in, count, out, groups);
        in = out;
        behind += groups;
        count = groups;
    }
}

void launch_match_select(const double* d2, const AttrScope& sc, uint32_t n, double lo, double hi, bool open_hi, uint32_t* scratch, uint32_t nwords, hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_match_select, dim3(mask_blocks(nwords, NB_THREADS)), dim3(NB_THREADS), 0, s, d2, sc, n, lo, hi, open_hi ? 1u : 0u, scratch, nwords);
}

}  // namespace gsr
