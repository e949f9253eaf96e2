// Growing the scene ("Growing the scene"): the selected splats of a source scene, in ascending order, copied bit
// for bit to the rows behind a destination scene's last splat -- px py pz cov0..2 rgba rot scl, nothing computed, nothing re-packed.
// The selection words are the ballot already (bit i & 31 of word i >> 5), so no predicate is evaluated: a workgroup of 256 source
// splats owns eight words, k_append_count popcounts them, one workgroup scans the sums, and k_append_gather gives lane i the row
//   dst_first + block_off[block] + popcount(earlier words of the block) + popcount(own word & bits below the lane's).
// Every wave of the gather reads its block's eight words itself (one 32-byte line) and takes the prefix with shuffles: no LDS, no
// barrier, so a wave whose two words are zero ends before it loads anything of the scene and a sparse selection costs the mask's
// n / 8 bytes, not a pass over the scene (k_edit.hip's rule).  The selected lanes of a wave write consecutive rows.
// Bits at and above n_src are masked in both kernels alike, whatever the words hold there.
#include "gsr_internal.h"
#include "k_splat_ops.h"

#include <algorithm>

namespace gsr {

GSR_BOUNDS_DECL(append)   // sites: 0 selection word, 1 source index, 2 destination index, 3 block-sum slot.  Site 2 is the one that
                          // matters: it compares the row a lane computed from the scanned sums with the destination's CAPACITY, an
                          // extent the host passes separately from the counts the row was derived from.  Sites 0 and 3 compare with
                          // nwords / nblocks, passed beside the pointers; site 1 stands behind the mask of the bits below n_src

constexpr uint32_t APPEND_THREADS = 256;                       // source splats of a gather workgroup
constexpr uint32_t APPEND_BLOCK_WORDS = APPEND_THREADS / 32;   // its selection words: one entry of the block sums

// selection word wi with the bits at and above n_src dropped (a word behind the mask's end reads as zero)
__device__ __forceinline__ uint32_t append_word(const uint32_t* __restrict__ words, uint32_t nwords, uint32_t n_src, uint32_t wi)
{
    if ((uint64_t)wi * 32u < n_src) GSR_BOUND(append, 0, wi, nwords);
    return set_word(words, nwords, n_src, wi);
}

// one thread per gather workgroup: the selected splats among its 256
__global__ __launch_bounds__(APPEND_THREADS) void k_append_count(const uint32_t* __restrict__ words, uint32_t nwords, uint32_t n_src,
                                                                 uint32_t* __restrict__ block_sums, uint32_t nblocks)
{
    const uint32_t b = blockIdx.x * APPEND_THREADS + threadIdx.x;
    if (b >= nblocks) return;
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < APPEND_BLOCK_WORDS; j++) sum += (uint32_t)__popc(append_word(words, nwords, n_src, b * APPEND_BLOCK_WORDS + j));
    GSR_BOUND(append, 3, b, nblocks);
    block_sums[b] = sum;
}

// one workgroup: block_sums[0 .. nblocks) -> their exclusive prefix sums, in place; block_sums[nblocks] <- the total
__global__ __launch_bounds__(APPEND_THREADS) void k_append_scan(uint32_t* __restrict__ block_sums, uint32_t nblocks)
{
    __shared__ uint32_t s_wave[APPEND_THREADS / WAVE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += APPEND_THREADS) {   // (uniform trip count: every thread meets every barrier)
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < nblocks ? block_sums[b] : 0u;
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
        for (uint32_t w = 0; w < APPEND_THREADS / WAVE; w++) {
            if (w < wave) before += s_wave[w];
            all += s_wave[w];
        }
        if (b < nblocks) {
            GSR_BOUND(append, 3, b, nblocks);
            block_sums[b] = carry + before + incl - v;
        }
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[nblocks] = carry;
}

// one thread per source splat: the selected ones to dst rows dst_first + rank, rank = the splat's place among the selected
__global__ __launch_bounds__(APPEND_THREADS) void k_append_gather(uint32_t n_src, SceneDev src, SceneDev dst, uint32_t dst_first, uint32_t dst_rows,
                                                                  const uint32_t* __restrict__ words, uint32_t nwords,
                                                                  const uint32_t* __restrict__ block_off, uint32_t nblocks)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // lanes 0..7 hold the block's eight words; the wave's own two are words 2 * wave and 2 * wave + 1
    const uint32_t held = lane < APPEND_BLOCK_WORDS ? append_word(words, nwords, n_src, blockIdx.x * APPEND_BLOCK_WORDS + lane) : 0u;
    const uint32_t w0 = __shfl(held, (int)(2u * wave)), w1 = __shfl(held, (int)(2u * wave + 1u));
    if ((w0 | w1) == 0u) return;   // nothing selected in this wave: nothing of the scene is loaded
    uint32_t before = lane < 2u * wave ? (uint32_t)__popc(held) : 0u;   // selected splats of the block in front of this wave
    before += __shfl_xor(before, 1);
    before += __shfl_xor(before, 2);
    before += __shfl_xor(before, 4);
    before = __shfl(before, 0);
    const uint32_t bit = lane & 31u, mine = lane < 32u ? w0 : w1;
    if (((mine >> bit) & 1u) == 0u) return;
    const uint32_t i = blockIdx.x * APPEND_THREADS + threadIdx.x;
    GSR_BOUND(append, 1, i, n_src);
    GSR_BOUND(append, 3, blockIdx.x, nblocks);
    if (blockIdx.x >= nblocks) return;
    const uint32_t rank = before + (lane < 32u ? 0u : (uint32_t)__popc(w0)) + (uint32_t)__popc(mine & ((1u << bit) - 1u));
    const uint64_t row = (uint64_t)dst_first + block_off[blockIdx.x] + rank;
    GSR_BOUND(append, 2, row, dst_rows);
    if (row >= dst_rows) return;   // (never: the host sized the destination for dst_first + the selection's count)
    copy_splat_row(dst, (uint32_t)row, src, i);   // words: the bits travel as they are
}

// the selection becomes exactly [first, first + count): every one of the nwords words is stored (a REPLACE); *total <- count
__global__ __launch_bounds__(APPEND_THREADS) void k_append_select_range(uint32_t* __restrict__ words, uint32_t nwords, uint32_t first, uint32_t count,
                                                                        uint32_t* __restrict__ total)
{
    const uint32_t wi = blockIdx.x * APPEND_THREADS + threadIdx.x;
    if (wi == 0u) *total = count;
    if (wi >= nwords) return;
    const uint64_t lo = (uint64_t)wi * 32u, end = (uint64_t)first + count;
    const uint64_t a = first > lo ? first : lo, b = end < lo + 32u ? end : lo + 32u;   // [a, b): the range's part of this word
    uint32_t v = 0u;
    if (a < b) {
        const uint32_t len = (uint32_t)(b - a);
        v = (len >= 32u ? 0xffffffffu : (1u << len) - 1u) << (uint32_t)(a - lo);
    }
    GSR_BOUND(append, 0, wi, nwords);
    words[wi] = v;
}

// ---- launchers ----
uint32_t append_blocks(uint32_t n_src) { return (n_src + APPEND_THREADS - 1) / APPEND_THREADS; }

void launch_append_gather(uint32_t n_src, const SceneDev& src, const SceneDev& dst, uint32_t dst_first, uint32_t dst_rows, const uint32_t* words,
                          uint32_t nwords, uint32_t* block_sums, hipStream_t s)
{
    const uint32_t nblocks = append_blocks(n_src);
    if (!nblocks) return;
    hipLaunchKernelGGL(k_append_count, dim3((nblocks + APPEND_THREADS - 1) / APPEND_THREADS), dim3(APPEND_THREADS), 0, s, words, nwords, n_src, block_sums, nblocks);
    hipLaunchKernelGGL(k_append_scan, dim3(1), dim3(APPEND_THREADS), 0, s, block_sums, nblocks);
    hipLaunchKernelGGL(k_append_gather, dim3(nblocks), dim3(APPEND_THREADS), 0, s, n_src, src, dst, dst_first, dst_rows, words, nwords,
                       (const uint32_t*)block_sums, nblocks);
}

void launch_append_select_range(uint32_t* words, uint32_t nwords, uint32_t first, uint32_t count, uint32_t* total, hipStream_t s)
{
    const uint32_t blocks = std::max<uint32_t>((nwords + APPEND_THREADS - 1) / APPEND_THREADS, 1u);
    hipLaunchKernelGGL(k_append_select_range, dim3(blocks), dim3(APPEND_THREADS), 0, s, words, nwords, first, count, total);
}

}  // namespace gsr
