// Planes ("Planes"): the dominant plane of the splats in scope by RANSAC, the scoring pass alone over planes
// of the host's, and the splats whose signed distance from a plane lies in a closed interval, as a picker.
//
// The signed distance of a splat at f32 (x, y, z) from the plane (a, b, c, d) is plane_distance below, stated once: f64, in the
// written order, uncontracted (the unit is compiled with -ffp-contract=off like the rest of the device code).  Scores are integers
// decided by f64 comparisons, the hypotheses come from a counter-based generator (splitmix64's finaliser over seed + 3 h + j) and
// ties go to the smaller index, so no result depends on the grid or on the order of arrival.
//
// k_plane_candidates (two steps around one scan, the shape of k_append's gather): the splats in scope with three finite position
//   floats, in ascending index, into cand[].  A wave with no splat in scope loads nothing of the scene (in_scope, k_splat_ops.h).
// k_plane_hypotheses: one lane per hypothesis: three ranks, three rows, the plane, its triple and a degenerate flag.
// k_plane_score, the hot path: lanes are HYPOTHESES, the grid's other dimension is groups of chunks of PLANE_CHUNK candidates.  A
//   workgroup stages a chunk into LDS as doubles -- every float converted once, cooperatively and coalesced through cand[] -- and
//   every lane then walks the chunk: all lanes read the same LDS address per step, a broadcast without a bank conflict; per step
//   three multiplies, three adds, a compare and a private counter.  No ballots and no per-point atomics: one relaxed agent-scope add
//   per lane into scores[h] when the group's chunks are done.
// k_plane_best: one workgroup; the maximum of (score << 32) | ~h over the non-degenerate hypotheses, so the tie rule is the
//   comparison itself.
// k_plane_select: one lane per bit of the mask (mask_store_ballot).
#include "gsr_internal.h"
#include "k_splat_ops.h"

#include <algorithm>

namespace gsr {

GSR_BOUNDS_DECL(plane)   // sites: 0 set word, 1 splat index, 2 block-sum slot, 3 candidate slot, 4 hypothesis slot, 5 selection word, 6 LDS cell

struct plane_sites {
    static __device__ __forceinline__ void bound_set_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(plane, 0, idx, limit); }
    static __device__ __forceinline__ void bound_mask_word(unsigned long long idx, unsigned long long limit) { GSR_BOUND(plane, 5, idx, limit); }
};

// s = ((a*(double)x + b*(double)y) + c*(double)z) + d
__device__ __forceinline__ double plane_distance(double a, double b, double c, double d, double x, double y, double z)
{
    return ((a * x + b * y) + c * z) + d;
}

// ---- the candidates ----
// One lane per splat, a workgroup per PLANE_THREADS splats.  SCATTER false: block[b] <- the workgroup's candidates, *totals += the
// splats in scope and, 32 bits up, those of them that are no candidate.  SCATTER true (block[] scanned): cand[block[b] + the
// candidates in front of the lane] <- the lane's splat.
template <bool SCATTER>
__global__ __launch_bounds__(PLANE_THREADS) void k_plane_candidates(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                                    AttrScope sc, uint32_t n, uint32_t* __restrict__ block, uint32_t nblocks,
                                                                    uint32_t* __restrict__ cand, uint32_t cand_rows, unsigned long long* __restrict__ totals)
{
    __shared__ uint32_t s_wave[PLANE_THREADS / WAVE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * PLANE_THREADS + threadIdx.x;
    const bool in = in_scope<plane_sites>(sc, n, i);
    bool is_cand = false;
    if (in) {
        GSR_BOUND(plane, 1, i, n);
        is_cand = f32_finite(px[i]) && f32_finite(py[i]) && f32_finite(pz[i]);
    }
    const uint64_t m = __ballot(is_cand);
    if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    GSR_BOUND(plane, 2, blockIdx.x, nblocks);
    if (blockIdx.x >= nblocks) return;
    if (!SCATTER) {
        if (threadIdx.x == 0u) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < PLANE_THREADS / WAVE; w++) sum += s_wave[w];
            block[blockIdx.x] = sum;
        }
        workgroup_sum_u64<PLANE_THREADS>((in ? 1ull : 0ull) | ((in && !is_cand) ? 1ull << 32 : 0ull), totals);
        return;
    }
    if (!is_cand) return;
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; w++) before += s_wave[w];
    const uint64_t slot = (uint64_t)block[blockIdx.x] + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    GSR_BOUND(plane, 3, slot, cand_rows);
    if (slot >= cand_rows) return;   // (never: the host sized cand[] for every splat)
    cand[slot] = (uint32_t)i;
}

// one workgroup: block[0 .. nblocks) -> their exclusive prefix sums, in place; block[nblocks] <- the total (k_append_scan's shape)
__global__ __launch_bounds__(PLANE_THREADS) void k_plane_scan(uint32_t* __restrict__ block, uint32_t nblocks)
{
    __shared__ uint32_t s_wave[PLANE_THREADS / WAVE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += PLANE_THREADS) {   // (uniform trip count: every thread meets every barrier)
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < nblocks ? block[b] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += o;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < PLANE_THREADS / WAVE; w++) {
            if (w < wave) before += s_wave[w];
            all += s_wave[w];
        }
        if (b < nblocks) {
            GSR_BOUND(plane, 2, b, nblocks + 1u);
            block[b] = carry + before + incl - v;
        }
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0u) block[nblocks] = carry;
}

// ---- the hypotheses ----
// splitmix64's finaliser, wrapping
__device__ __forceinline__ unsigned long long plane_mix(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(PLANE_THREADS) void k_plane_hypotheses(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                                    uint32_t hypotheses, unsigned long long seed, uint32_t m, const uint32_t* __restrict__ cand,
                                                                    uint32_t cand_rows, uint32_t n, double4* __restrict__ planes, uint4* __restrict__ triple)
{
    const uint32_t h = blockIdx.x * PLANE_THREADS + threadIdx.x;
    if (h >= hypotheses) return;
    GSR_BOUND(plane, 4, h, PLANE_MAX_HYPOTHESES);
    unsigned long long r[3];
    uint32_t t[3];
    double p[3][3];
#pragma unroll
    for (uint32_t j = 0; j < 3u; j++) {
        r[j] = __umul64hi(plane_mix(seed + 3ull * h + j), (unsigned long long)m);   // rank(h, j) < m
        GSR_BOUND(plane, 3, r[j], cand_rows);
        t[j] = r[j] < cand_rows ? cand[r[j]] : 0u;
        GSR_BOUND(plane, 1, t[j], n);
        if (t[j] >= n) t[j] = 0u;   // (never: cand[] holds splat indices)
        p[j][0] = (double)px[t[j]]; p[j][1] = (double)py[t[j]]; p[j][2] = (double)pz[t[j]];
    }
    const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
    const double l2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
    const bool degenerate = r[0] == r[1] || r[0] == r[2] || r[1] == r[2] || !(l2 - l2 == 0.0) || l2 == 0.0;   // (l2 - l2: NaN for a NaN or infinite l2)
    double4 pl = make_double4(0.0, 0.0, 0.0, 0.0);
    if (!degenerate) {
        const double len = __dsqrt_rn(l2);   // the correctly rounded square root, as k_attr.h's
        double nx = Nx / len, ny = Ny / len, nz = Nz / len;
        // the first of nx, ny, nz that is not zero is positive.  One flag and three selects: as `if (..) { nx = -nx; .. }` the
        // compiler's output kept ny and nz as they were when nx == 0 (seen in the assembly and on the device)
        const bool neg = nx < 0.0 || (nx == 0.0 && (ny < 0.0 || (ny == 0.0 && nz < 0.0)));
        nx = neg ? -nx : nx; ny = neg ? -ny : ny; nz = neg ? -nz : nz;   // (a -0.0 this leaves is part of the result)
        pl = make_double4(nx, ny, nz, -((nx * p[0][0] + ny * p[0][1]) + nz * p[0][2]));
    }
    planes[h] = pl;
    triple[h] = make_uint4(t[0], t[1], t[2], degenerate ? 1u : 0u);
}

// ---- the scores: the hot path ----
// grid: (ceil(count / THREADS), groups).  Group g walks the chunks g, g + groups, .. of PLANE_CHUNK candidates each.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_plane_score(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz, uint32_t n,
                                                         const uint32_t* __restrict__ cand, uint32_t m, const double4* __restrict__ planes,
                                                         const uint4* __restrict__ flags, uint32_t count, double threshold, uint32_t* __restrict__ scores)
{
    __shared__ double s_x[PLANE_CHUNK], s_y[PLANE_CHUNK], s_z[PLANE_CHUNK];
    const uint32_t h = blockIdx.x * THREADS + threadIdx.x;
    bool walk = h < count;
    double4 pl = make_double4(0.0, 0.0, 0.0, 0.0);
    if (walk) {
        GSR_BOUND(plane, 4, h, PLANE_MAX_HYPOTHESES);
        if (flags && flags[h].w) walk = false;   // a degenerate hypothesis scores 0: it skips the walk, not the barriers
        else pl = planes[h];
    }
    const uint32_t chunks = (uint32_t)(((uint64_t)m + PLANE_CHUNK - 1u) / PLANE_CHUNK);
    uint32_t mine = 0;
    for (uint32_t ch = blockIdx.y; ch < chunks; ch += gridDim.y) {   // (uniform trip count: every thread meets every barrier)
        const uint32_t first = ch * PLANE_CHUNK, len = m - first < PLANE_CHUNK ? m - first : PLANE_CHUNK;
        for (uint32_t k = threadIdx.x; k < len; k += THREADS) {
            GSR_BOUND(plane, 3, first + k, m);
            uint32_t i = cand[first + k];
            GSR_BOUND(plane, 1, i, n);
            if (i >= n) i = 0u;   // (never)
            GSR_BOUND(plane, 6, k, PLANE_CHUNK);
            s_x[k] = (double)px[i]; s_y[k] = (double)py[i]; s_z[k] = (double)pz[i];
        }
        __syncthreads();
        if (walk)
            for (uint32_t k = 0; k < len; k++)   // every lane reads the same address: a broadcast
                mine += fabs(plane_distance(pl.x, pl.y, pl.z, pl.w, s_x[k], s_y[k], s_z[k])) <= threshold ? 1u : 0u;
        __syncthreads();
    }
    if (walk && mine) __hip_atomic_fetch_add(&scores[h], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the best hypothesis ----
// One workgroup.  key(h) = score << 32 | ~h over the non-degenerate hypotheses: the largest key is the largest score and, among
// equals, the smallest h.  A key is never 0 (h < 4096), so 0 is "every hypothesis is degenerate".
__global__ __launch_bounds__(PLANE_THREADS) void k_plane_best(uint32_t hypotheses, const uint32_t* __restrict__ scores, const uint4* __restrict__ triple,
                                                              const double4* __restrict__ planes, PlBest* __restrict__ out)
{
    __shared__ unsigned long long s_key[PLANE_THREADS / WAVE];
    __shared__ uint32_t s_deg[PLANE_THREADS / WAVE];
    unsigned long long key = 0ull;
    uint32_t deg = 0u;
    for (uint32_t h = threadIdx.x; h < hypotheses; h += PLANE_THREADS) {
        GSR_BOUND(plane, 4, h, PLANE_MAX_HYPOTHESES);
        if (triple[h].w) { deg++; continue; }
        const unsigned long long k = ((unsigned long long)scores[h] << 32) | (unsigned long long)(~h);
        if (k > key) key = k;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long ok = __shfl_xor(key, d);
        deg += __shfl_xor(deg, d);
        if (ok > key) key = ok;
    }
    if ((threadIdx.x & 63u) == 0u) { s_key[threadIdx.x >> 6] = key; s_deg[threadIdx.x >> 6] = deg; }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1; w < PLANE_THREADS / WAVE; w++) {
        if (s_key[w] > key) key = s_key[w];
        deg += s_deg[w];
    }
    PlBest b{};
    b.degenerate = deg;
    if (key) {
        const uint32_t h = ~(uint32_t)key;
        GSR_BOUND(plane, 4, h, hypotheses);
        if (h < hypotheses) {
            b.found = 1u; b.best = h; b.inliers = (uint32_t)(key >> 32);
            b.triple[0] = triple[h].x; b.triple[1] = triple[h].y; b.triple[2] = triple[h].z;
            b.plane[0] = planes[h].x; b.plane[1] = planes[h].y; b.plane[2] = planes[h].z; b.plane[3] = planes[h].w;
        }
    }
    *out = b;
}

// ---- the picker ----
// gsr_select_plane.  One thread per bit of the mask: lo <= s && s <= hi over ALL splats, so a NaN distance is never picked.  A
// wave's ballot is two whole words of the mask: every word is stored (splats at and above n vote 0).
__global__ __launch_bounds__(PLANE_THREADS) void k_plane_select(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz, uint32_t n,
                                                                double4 pl, double lo, double hi, uint32_t* __restrict__ scratch, uint32_t nwords)
{
    const uint32_t i = blockIdx.x * PLANE_THREADS + threadIdx.x;
    bool in = false;
    if (i < n) {
        GSR_BOUND(plane, 1, i, n);
        const double s = plane_distance(pl.x, pl.y, pl.z, pl.w, (double)px[i], (double)py[i], (double)pz[i]);
        in = lo <= s && s <= hi;
    }
    mask_store_ballot<plane_sites>(scratch, nwords, i, __ballot(in));
}

// ---- launchers ----
void launch_plane_candidates(const float* px, const float* py, const float* pz, const AttrScope& sc, uint32_t n, const PlArrays& a, hipStream_t s)
{
    const uint32_t nblocks = plane_blocks(n);
    if (!nblocks) return;
    hipLaunchKernelGGL(k_plane_candidates<false>, dim3(nblocks), dim3(PLANE_THREADS), 0, s, px, py, pz, sc, n, a.block, nblocks, a.cand, a.cand_rows, a.totals);
    hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(PLANE_THREADS), 0, s, a.block, nblocks);
    hipLaunchKernelGGL(k_plane_candidates<true>, dim3(nblocks), dim3(PLANE_THREADS), 0, s, px, py, pz, sc, n, a.block, nblocks, a.cand, a.cand_rows, a.totals);
}

void launch_plane_hypotheses(const float* px, const float* py, const float* pz, uint32_t hypotheses, uint64_t seed, uint32_t m, uint32_t n, const PlArrays& a,
                             hipStream_t s)
{
    hipLaunchKernelGGL(k_plane_hypotheses, dim3((hypotheses + PLANE_THREADS - 1u) / PLANE_THREADS), dim3(PLANE_THREADS), 0, s, px, py, pz, hypotheses,
                       (unsigned long long)seed, m, (const uint32_t*)a.cand, a.cand_rows, n, a.planes, a.triple);
}

void launch_plane_score(const float* px, const float* py, const float* pz, uint32_t count, uint32_t m, uint32_t n, double threshold, bool flagged, const PlArrays& a,
                        hipStream_t s)
{
    const uint32_t chunks = (uint32_t)(((uint64_t)m + PLANE_CHUNK - 1u) / PLANE_CHUNK);
    const uint32_t groups = std::min(std::max(chunks, 1u), PLANE_MAX_CHUNK_GROUPS);
    const uint4* flags = flagged ? a.triple : nullptr;
    // fewer than 256 planes: the chunks are the parallelism, and a workgroup no wider than the planes leaves no lane idle in the walk
    if (count <= 64u)
        hipLaunchKernelGGL(k_plane_score<64>, dim3(1, groups), dim3(64), 0, s, px, py, pz, n, (const uint32_t*)a.cand, m, (const double4*)a.planes, flags, count,
                           threshold, a.scores);
    else
        hipLaunchKernelGGL(k_plane_score<256>, dim3((count + 255u) / 256u, groups), dim3(256), 0, s, px, py, pz, n, (const uint32_t*)a.cand, m,
                           (const double4*)a.planes, flags, count, threshold, a.scores);
}

void launch_plane_best(uint32_t hypotheses, const PlArrays& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_plane_best, dim3(1), dim3(PLANE_THREADS), 0, s, hypotheses, (const uint32_t*)a.scores, (const uint4*)a.triple, (const double4*)a.planes,
                       a.result);
}

void launch_plane_select(const float* px, const float* py, const float* pz, uint32_t n, double4 plane, double lo, double hi, uint32_t* scratch, uint32_t nwords,
                         hipStream_t s)
{
    if (!nwords) return;
    hipLaunchKernelGGL(k_plane_select, dim3(mask_blocks(nwords, PLANE_THREADS)), dim3(PLANE_THREADS), 0, s, px, py, pz, n, plane, lo, hi, scratch, nwords);
}

}  // namespace gsr
