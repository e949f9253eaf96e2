// Merging cells ("Merging cells"): voxel simplification of the scene.  The candidates -- the splats in scope
// whose position, rotation and scale are finite -- are indexed by k_neighbours.hip's hashed grid with inv_h = 1 / cell, so a
// grid cell is an index cell and a cell's members lie in ONE bucket.  Every cell of two or more members becomes one splat by
// moment matching: the mass-weighted mean, the covariance of the mixture, and a rotation and scale from its eigen-decomposition.
//
// k_mg_candidates  one lane per bit of the mask: the scope word ANDed with a ballot of "ten finite floats"; a run of 64 splats out
//                  of scope reads nothing of the scene.  The mask is then the SELECTED scope of launch_nb_build.
// k_mg_bound       the sum over the buckets of population^2: what the walk tests at most, checked against the budget first.
// k_mg_walk        one entry per lane, in index order.  The lane walks its OWN bucket and compares the stored key in front of
//                  anything else: it ends with its cell's smallest member index (the leader), the members and its rank among
//                  them.  A leader counts its cell (histogram through LDS counters: lds_counters_*, k_splat_ops.h) and, for two or more members,
//                  takes a slice of the member list and a cell record.  Slices and records are handed out per WAVE: a scan of the
//                  wave's sizes and two atomics by its first lane, so the cursors see one atomic per 64 entries.  Where a slice
//                  lies decides nothing: a cell reads only its own.
// k_mg_members     member[slice of the leader + rank] = i puts every cell's members in ascending order with no sort; the same
//                  lanes ballot the two masks the compaction needs ("member and not leader", "leader of a merged cell").
// k_mg_reduce      one lane per merged cell.  Pass one: M, the weighted and the unweighted position and colour sums and the
//                  largest opacity, in ascending member order; pass two: the mixture's covariance about the unrounded mean.
//                  Then six cyclic Jacobi sweeps with constant indices -- the 3 x 3 state stays in registers, no scratch --
//                  Shepperd's quaternion, pack_cov of the stored f32 values, and the row at the leader's index.  A cell reads
//                  only its own members and writes only its leader, so cells do not disturb each other.
//
// All arithmetic of the merged row is f64 in the header's order; compiled with -ffp-contract=off like the rest of the device code.
#include "gsr_internal.h"
#include "k_splat_ops.h"
#include "k_neighbours.h"   // the key and the bucket

namespace gsr {

GSR_BOUNDS_DECL(merge)   // sites: 0 set word, 1 splat index, 2 bucket, 3 entry slot, 4 LDS counter, 5 cell record, 6 mask word stored, 7 member slot

// the sites of the shared helpers (k_splat_ops.h)
struct mg_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(merge, 0, idx, limit); }
    static __device__ __forceinline__ void bound_counter(unsigned long long idx, unsigned long long limit) { GSR_BOUND(merge, 4, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(merge, 6, idx, limit); }
};

// ---- the candidates ----
__global__ __launch_bounds__(NB_THREADS) void k_mg_candidates(SceneDev scene, AttrScope sc, uint32_t n, MgArrays a)
{
    __shared__ uint32_t s_w[NB_THREADS / WAVE];
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    const bool in = in_scope<mg_sites>(sc, n, i);
    bool cand = false;
    if (in) {
        GSR_BOUND(merge, 1, i, n);
        const float x = scene.px[i], y = scene.py[i], z = scene.pz[i];
        const float4 r = scene.rot[i], s = scene.scl[i];
        cand = f32_finite(x) && f32_finite(y) && f32_finite(z) && f32_finite(r.x) && f32_finite(r.y) && f32_finite(r.z) && f32_finite(r.w) && f32_finite(s.x) &&
               f32_finite(s.y) && f32_finite(s.z);
    }
    const uint64_t ms = __ballot(in), mc = __ballot(cand);
    mask_store_ballot<mg_sites>(a.cand, a.words, i, mc);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(ms);
    __syncthreads();
    if (threadIdx.x != 0u) return;
    uint32_t t = 0u;
    for (int w = 0; w < NB_THREADS / WAVE; w++) t += s_w[w];
    if (t) __hip_atomic_fetch_add(&a.info->in_scope, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the bound ----
// An entry walks its own bucket: population tests for each of the bucket's population entries.
__global__ __launch_bounds__(NB_THREADS) void k_mg_bound(NbIndex ix, MgArrays a)
{
    const uint64_t buckets = (uint64_t)ix.bucket_mask + 1u, stride = (uint64_t)gridDim.x * NB_THREADS;
    unsigned long long sum = 0ull;
    for (uint64_t b = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; b < buckets; b += stride) {
        GSR_BOUND(merge, 2, b, buckets);
        const unsigned long long p = ix.table[2ull * b];
        sum += p * p;
    }
    workgroup_sum_u64<NB_THREADS>(sum, &a.info->pair_bound);
}

// ---- the walk ----
template <bool HIST>
__global__ __launch_bounds__(NB_THREADS) void k_mg_walk(NbIndex ix, uint32_t m /* entries */, uint32_t n /* splats */, uint32_t cap, MgArrays a,
                                                        uint32_t* __restrict__ hist)
{
    extern __shared__ uint32_t s_hist[];   // cap + 1 (HIST)
    if (HIST) lds_counters_zero(s_hist, cap + 1u, NB_THREADS);
    const uint2* __restrict__ table = reinterpret_cast<const uint2*>(ix.table);   // (population, one behind the last entry)
    const uint32_t lane = threadIdx.x & 63u, max_cells = n / 2u + 1u;
    uint32_t cells = 0u, largest = 0u;
    const uint64_t stride = (uint64_t)gridDim.x * NB_THREADS, end = ((uint64_t)m + 63u) & ~63ull;   // whole waves step together
    for (uint64_t s = (uint64_t)blockIdx.x * NB_THREADS + threadIdx.x; s < end; s += stride) {
        uint32_t me = MG_NONE, members = 0u, rank = 0u, lead = MG_NONE;
        if (s < m) {
            GSR_BOUND(merge, 3, s, m);
            me = ix.entry[s].w;
            const unsigned long long key = ix.key[s];
            const uint32_t b = nb_bucket(key, ix.bucket_mask);
            GSR_BOUND(merge, 2, b, (uint64_t)ix.bucket_mask + 1u);
            const uint2 t = table[b];
            GSR_BOUND(merge, 3, t.y, (uint64_t)m + 1u);
            if (t.y <= m && t.x <= t.y) {   // (always: a range of the entry array)
                for (uint32_t e = t.y - t.x; e < t.y; e++) {
                    if (ix.key[e] != key) continue;
                    const uint32_t j = ix.entry[e].w;
                    members++;
                    rank += j < me ? 1u : 0u;
                    lead = min(lead, j);
                }
            }
        }
        const bool is_lead = members != 0u && lead == me, merged = is_lead && members >= 2u;
        // the wave's merged cells take consecutive records and consecutive slices: an inclusive scan of their sizes, two atomics
        const uint64_t bm = __ballot(merged);
        uint32_t incl = merged ? members : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += o;
        }
        uint32_t base_cell = 0u, base_slot = 0u;
        if (bm) {
            const uint32_t total = __shfl(incl, 63);
            if (lane == 0u) {
                base_cell = __hip_atomic_fetch_add(&a.info->merged_cells, (uint32_t)__popcll(bm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                base_slot = __hip_atomic_fetch_add(&a.info->merged_members, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            base_cell = __shfl(base_cell, 0);
            base_slot = __shfl(base_slot, 0);
        }
        if (members) {
            GSR_BOUND(merge, 1, me, n);
            if (me < n) { a.leader[me] = lead; a.count[me] = members; a.rank[me] = rank; }
        }
        if (merged) {
            const uint32_t id = base_cell + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
            const uint32_t slot = base_slot + (incl - members);
            GSR_BOUND(merge, 5, id, max_cells);
            if (a.cells && id < max_cells && me < n) { a.cells[id] = make_uint2(slot, members); a.slice[me] = slot; }   // (the edit only)
        }
        if (is_lead) {
            cells++;
            largest = max(largest, members);
            if (HIST) {
                const uint32_t k = members < cap ? members : cap;
                GSR_BOUND(merge, 4, k, cap + 1u);
                __hip_atomic_fetch_add(&s_hist[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { cells += __shfl_xor(cells, d); largest = max(largest, (uint32_t)__shfl_xor(largest, d)); }
    if (lane == 0u && cells) {
        __hip_atomic_fetch_add(&a.info->cells, cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&a.info->largest, largest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (HIST) lds_counters_flush<mg_sites>(s_hist, cap + 1u, NB_THREADS, hist, NB_MAX_CAP + 1u);
}

// ---- the member lists and the compaction's masks ----
__global__ __launch_bounds__(NB_THREADS) void k_mg_members(uint32_t n, uint32_t merged_members, MgArrays a)
{
    const uint32_t i = blockIdx.x * NB_THREADS + threadIdx.x;
    bool rem = false, mrg = false;
    if (i < n && a.count[i] >= 2u) {
        const uint32_t l = a.leader[i];
        mrg = l == i;
        rem = !mrg;
        GSR_BOUND(merge, 1, l, n);
        const uint32_t slot = l < n ? a.slice[l] + a.rank[i] : MG_NONE;
        GSR_BOUND(merge, 7, slot, merged_members);
        if (slot < merged_members) a.member[slot] = i;
        else __hip_atomic_fetch_add(&a.info->fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t br = __ballot(rem), bg = __ballot(mrg);
    mask_store_ballot<mg_sites>(a.remove, a.words, i, br);
    mask_store_ballot<mg_sites>(a.merged, a.words, i, bg);
}

// ---- the reduction ----
// one cyclic Jacobi rotation on the pair (p, q), r the third index: the header's step 6 on named scalars
#define MG_ROTATE(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                     \
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

__global__ __launch_bounds__(NB_THREADS) void k_mg_reduce(SceneDev scene, uint32_t n, uint32_t merged_cells, uint32_t merged_members, MgArrays a)
{
    const uint32_t c = blockIdx.x * NB_THREADS + threadIdx.x;
    if (c >= merged_cells) return;
    GSR_BOUND(merge, 5, c, n / 2u + 1u);
    const uint2 rec = a.cells[c];
    const uint32_t off = rec.x, m = rec.y;
    GSR_BOUND(merge, 7, (uint64_t)off + m, (uint64_t)merged_members + 1u);
    if (m < 2u || off > merged_members || m > merged_members - off) {   // (never: a slice of the member list)
        __hip_atomic_fetch_add(&a.info->fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // pass one: the weight inputs and both sets of sums, ascending
    double M = 0.0, wx = 0.0, wy = 0.0, wz = 0.0, ux = 0.0, uy = 0.0, uz = 0.0, wr = 0.0, wg = 0.0, wb = 0.0, ur = 0.0, ug = 0.0, ub = 0.0;
    uint32_t amax = 0u;
    for (uint32_t t = 0u; t < m; t++) {
        const uint32_t i = a.member[off + t];
        GSR_BOUND(merge, 1, i, n);
        if (i >= n) { __hip_atomic_fetch_add(&a.info->fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
        const double x = scene.px[i], y = scene.py[i], z = scene.pz[i];
        const float4 s = scene.scl[i];
        const uint32_t rgba = scene.rgba[i];
        const double al = (double)(rgba >> 24), v = (fabs((double)s.x) * fabs((double)s.y)) * fabs((double)s.z), mi = al * v;
        const double r = (double)(rgba & 0xffu), g = (double)((rgba >> 8) & 0xffu), b = (double)((rgba >> 16) & 0xffu);
        M += mi;
        wx += mi * x; wy += mi * y; wz += mi * z;
        ux += x; uy += y; uz += z;
        wr += mi * r; wg += mi * g; wb += mi * b;
        ur += r; ug += g; ub += b;
        amax = max(amax, rgba >> 24);
    }
    const bool massive = M > 0.0;
    const double W = massive ? M : (double)m;
    const double mx = (massive ? wx : ux) / W, my = (massive ? wy : uy) / W, mz = (massive ? wz : uz) / W;
    const double cr = floor((massive ? wr : ur) / W + 0.5), cg = floor((massive ? wg : ug) / W + 0.5), cb = floor((massive ? wb : ub) / W + 0.5);
    // pass two: the mixture's covariance about the unrounded mean
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (uint32_t t = 0u; t < m; t++) {
        const uint32_t i = a.member[off + t];   // (below n: pass one read the same word)
        const float4 s = scene.scl[i];
        double w = 1.0;
        if (massive) w = (double)(scene.rgba[i] >> 24) * ((fabs((double)s.x) * fabs((double)s.y)) * fabs((double)s.z));
        double S[6];
        splat_cov(scene.rot[i], s, S);
        const double dx = (double)scene.px[i] - mx, dy = (double)scene.py[i] - my, dz = (double)scene.pz[i] - mz;
        a00 += w * (S[0] + dx * dx); a01 += w * (S[1] + dx * dy); a02 += w * (S[2] + dx * dz);
        a11 += w * (S[3] + dy * dy); a12 += w * (S[4] + dy * dz); a22 += w * (S[5] + dz * dz);
    }
    a00 = a00 / W; a01 = a01 / W; a02 = a02 / W; a11 = a11 / W; a12 = a12 / W; a22 = a22 / W;
    // six cyclic sweeps; V = I
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int sweep = 0; sweep < 6; sweep++) {
        MG_ROTATE(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)   // (0, 1), r = 2
        MG_ROTATE(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)   // (0, 2), r = 1
        MG_ROTATE(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)   // (1, 2), r = 0
    }
    float4 scl = scene.scl[a.member[off]];   // (the leader's fourth word stays)
    scl.x = (float)__dsqrt_rn(a00 > 0.0 ? a00 : 0.0);
    scl.y = (float)__dsqrt_rn(a11 > 0.0 ? a11 : 0.0);
    scl.z = (float)__dsqrt_rn(a22 > 0.0 ? a22 : 0.0);
    // R = V^T: row k is eigenvector k
    const double R00 = v00, R01 = v10, R02 = v20, R10 = v01, R11 = v11, R12 = v21, R20 = v02, R21 = v12, R22 = v22;
    const double tr = (R00 + R11) + R22;
    double qx, qy, qz, qw;
    if (tr > 0.0) {
        const double s = __dsqrt_rn(tr + 1.0) * 2.0;
        qw = 0.25 * s; qx = (R21 - R12) / s; qy = (R02 - R20) / s; qz = (R10 - R01) / s;
    } else if (R00 > R11 && R00 > R22) {
        const double s = __dsqrt_rn(((1.0 + R00) - R11) - R22) * 2.0;
        qw = (R21 - R12) / s; qx = 0.25 * s; qy = (R01 + R10) / s; qz = (R02 + R20) / s;
    } else if (R11 > R22) {
        const double s = __dsqrt_rn(((1.0 + R11) - R00) - R22) * 2.0;
        qw = (R02 - R20) / s; qx = (R01 + R10) / s; qy = 0.25 * s; qz = (R12 + R21) / s;
    } else {
        const double s = __dsqrt_rn(((1.0 + R22) - R00) - R11) * 2.0;
        qw = (R10 - R01) / s; qx = (R02 + R20) / s; qy = (R12 + R21) / s; qz = 0.25 * s;
    }
    const float4 rot = make_float4((float)(-qw), (float)qx, (float)qy, (float)qz);
    uint32_t c0, c1, c2;
    pack_cov(rot, scl, c0, c1, c2);
    // opacity x volume is conserved
    const double vol = ((double)scl.x * (double)scl.y) * (double)scl.z;
    uint32_t alpha = amax;
    if (vol > 0.0) {
        const double o = M / vol;
        alpha = o >= 255.0 ? 255u : (uint32_t)floor(o + 0.5);
    }
    const uint32_t lead = a.member[off];
    scene.px[lead] = (float)mx; scene.py[lead] = (float)my; scene.pz[lead] = (float)mz;
    scene.rot[lead] = rot; scene.scl[lead] = scl;
    scene.cov0[lead] = c0; scene.cov1[lead] = c1; scene.cov2[lead] = c2;
    scene.rgba[lead] = (uint32_t)cr | ((uint32_t)cg << 8) | ((uint32_t)cb << 16) | (alpha << 24);
}
#undef MG_ROTATE

// ---- launchers ----
void launch_mg_candidates(const SceneDev& scene, const AttrScope& sc, uint32_t n, const MgArrays& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_mg_candidates, dim3(mask_blocks(a.words, NB_THREADS)), dim3(NB_THREADS), 0, s, scene, sc, n, a);
}

void launch_mg_bound(const NbIndex& ix, const MgArrays& a, int cu_count, hipStream_t s)
{
    hipLaunchKernelGGL(k_mg_bound, dim3(nb_grid((uint64_t)ix.bucket_mask + 1u, cu_count)), dim3(NB_THREADS), 0, s, ix, a);
}

void launch_mg_walk(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t cap, const MgArrays& a, uint32_t* hist, int cu_count, hipStream_t s)
{
    if (!indexed) return;
    const uint32_t blocks = nb_grid(indexed, cu_count);
    if (hist) hipLaunchKernelGGL(k_mg_walk<true>, dim3(blocks), dim3(NB_THREADS), ((size_t)cap + 1u) * sizeof(uint32_t), s, ix, indexed, n, cap, a, hist);
    else hipLaunchKernelGGL(k_mg_walk<false>, dim3(blocks), dim3(NB_THREADS), 0, s, ix, indexed, n, cap, a, hist);
}

void launch_mg_members(uint32_t n, uint32_t merged_members, const MgArrays& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_mg_members, dim3(mask_blocks(a.words, NB_THREADS)), dim3(NB_THREADS), 0, s, n, merged_members, a);
}

void launch_mg_reduce(const SceneDev& scene, uint32_t n, uint32_t merged_cells, uint32_t merged_members, const MgArrays& a, hipStream_t s)
{
    if (!merged_cells) return;
    hipLaunchKernelGGL(k_mg_reduce, dim3((merged_cells + NB_THREADS - 1) / NB_THREADS), dim3(NB_THREADS), 0, s, scene, n, merged_cells, merged_members, a);
}

}  // namespace gsr
