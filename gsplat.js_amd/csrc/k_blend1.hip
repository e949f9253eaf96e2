// The compositor with one wave per tile (k_blend, k_blend_unfused): the form of contexts with frames in flight and of frames
// with many bins.  The body is k_blend_body.h, shared with the two-waves-per-tile kernels of k_blend.hip; this unit exists for
// its flags alone: it is built with -fno-slp-vectorize (Makefile, FLAGS_k_blend1).  The SLP vectoriser packed parts of the
// four-axis staging block into v_pk_* f32 operations (51 of the block's 297 vector instructions, plus the moves that gather
// their operands), which cost two issue slots each, and left 20 bytes of scratch per lane; plain operations are the same bits
// (no contraction either way), 72 VGPRs and no scratch.  The flag is per unit, and k_blend2's code must not change with it
// (its legs were tuned on the vectorised form), hence two units.
#include "k_blend_body.h"

namespace gsr {

// 7 waves per SIMD: the kernel needs 74 VGPRs unconstrained (6 waves); capped at 72 the seventh wave hides more of the
// LDS/barrier waits (measured: k_blend -5.7 % alone; 8 waves = 64 VGPRs spills inside the loops and is no better).
__global__ __launch_bounds__(BLEND_THREADS) __attribute__((amdgpu_waves_per_eu(7, 7))) void k_blend(GSR_BLEND_PARAMS)
{
    blend_body<1, true>(GSR_BLEND_ARGS);
}
// the same with the partials left to k_combine (GSR_FUSE_COMBINE=0; test reference)
__global__ __launch_bounds__(BLEND_THREADS) __attribute__((amdgpu_waves_per_eu(7, 7))) void k_blend_unfused(GSR_BLEND_PARAMS)
{
    blend_body<1, false>(GSR_BLEND_ARGS);
}

BlendFn blend1_kernel(bool fused) { return fused ? k_blend : k_blend_unfused; }

#if defined(GSR_BOUNDS) || defined(GSR_BLEND_STAMPS)
int blend1_read_words(int which, unsigned int* out)
{
    hipError_t e = hipErrorInvalidValue;
#ifdef GSR_BOUNDS
    if (which == BLEND_WORDS_BOUNDS) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bounds_blend), sizeof g_bounds_blend);
#endif
#ifdef GSR_BLEND_STAMPS
    if (which == BLEND_WORDS_STAMPS) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_blend_stamps), sizeof g_blend_stamps);
    if (which == BLEND_WORDS_BIN_INFO) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bin_info), sizeof g_bin_info);
#endif
    return e == hipSuccess ? 0 : -1;
}
#endif

}  // namespace gsr
