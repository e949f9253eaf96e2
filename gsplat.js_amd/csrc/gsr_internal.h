// Internal declarations shared by the HIP translation units of libgsplat_hip.so.
// gfx950 (MI355X) only: wave64, 256 CUs in 8 XCDs, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int WAVE = 64;
constexpr uint32_t DEPTH_RANGE = 65536u;   // wasm/wasm.cpp:33
constexpr int KEY_BITS = 17;               // keys are in [0, 65536]
constexpr int RADIX_LO_BITS = 8;           // pass 1 digit: key & 0xff
constexpr int RADIX_HI_BITS = 9;           // pass 2 digit: key >> 8  (0..256)
constexpr int RADIX_LO_BINS = 1 << RADIX_LO_BITS;
constexpr int RADIX_HI_BINS = 1 << RADIX_HI_BITS;

constexpr int TILE = 16;                   // pixels per tile side: one wave per tile, 4 px per lane
constexpr int BIN_TILES = 2;               // tiles per coarse-bin side
constexpr int BIN_PX = TILE * BIN_TILES;   // 32 px: one workgroup (4 waves) per bin

// Camera constants passed by value (kernarg -> SGPRs).
struct CamParams {
    float view[16];
    float proj[16];
    float vp2, vp6, vp10;   // row 2 of viewProj: wasm/wasm.cpp:18-20
    float fx, fy;
    int32_t W, H;
    int32_t sh_on;          // scene carries SH textures
    int32_t band[3];        // Scene.bandsIndices
    int32_t band_px0, band_px1;  // pixel columns [x0, x1) this context composites (multi-GPU band; whole image otherwise)
    int32_t use_fade;       // u_useDepthFade
    float fade;             // u_depthFade
    int32_t sh_frame;       // the SH frame is not the identity: SH directions go through shm first ("SH frame")
    float shm[9];           // the frame, row-major, rounded once from the host's f64 (read only where sh_frame is set)
};

// 32-byte projected record consumed by the tile compositor (image coordinates, row 0 = top).
//   vPosition at pixel centre p is (dot(p-c,u), dot(p-c,w)); coverage |vPosition|^2 <= 4.
struct __attribute__((aligned(16))) Record {
    float cx, cy, ux, uy;
    float wx, wy, la;       // la = log2(opacity)
    uint32_t rgb8;          // r | g<<8 | b<<16; or RGB8_IN_SHCOL: the colour is the float triple shcol[splat]
};
constexpr uint32_t RGB8_IN_SHCOL = 0x01000000u;
static_assert(sizeof(Record) == 32, "record must be 32 bytes");

// Packed inclusive pixel bounding box: x = x0 | x1<<16, y = y0 | y1<<16; invisible when x0 > x1.
constexpr uint32_t BBOX_INVISIBLE_X = 1u;  // x0 = 1, x1 = 0
constexpr uint32_t BBOX_INVISIBLE_Y = 1u;

// Bin rectangle of a splat's pixel box inside a context's band of bin columns [bx_lo, bx_hi), packed in 4 bytes:
// x0 | x1 << 8 | y0 << 16 | y1 << 24 (inclusive bin coordinates, x relative to the band; at most 256 bins per axis);
// 1 = nothing to draw.  Written once per splat by k_project_key.  Where the sort plan says so (SortPlan::carry: the LSD order,
// the bucket order only with GSR_RECT_CARRY=2) they travel through the sort's passes with the keys (SortBuffers::rects_out);
// otherwise k_bin_count gathers them into depth order (4-byte gathers).
constexpr uint32_t RECT_NONE = 1u;
__host__ __device__ inline uint32_t pack_bin_rect(uint32_t bbx, uint32_t bby, int bx_lo, int bx_hi)
{
    const int px0 = (int)(bbx & 0xffffu), px1 = (int)(bbx >> 16), py0 = (int)(bby & 0xffffu), py1 = (int)(bby >> 16);
    if (px0 > px1) return RECT_NONE;
    const int x0 = (px0 / BIN_PX > bx_lo ? px0 / BIN_PX : bx_lo) - bx_lo;
    const int x1 = (px1 / BIN_PX < bx_hi - 1 ? px1 / BIN_PX : bx_hi - 1) - bx_lo;
    if (x0 > x1) return RECT_NONE;
    return (uint32_t)x0 | ((uint32_t)x1 << 8) | ((uint32_t)(py0 / BIN_PX) << 16) | ((uint32_t)(py1 / BIN_PX) << 24);
}

struct SceneSoA {
    const float *px, *py, *pz;
    const uint32_t *cov0, *cov1, *cov2, *rgba;
    const uint32_t *sh_r, *sh_g, *sh_b;  // 8 u32 per SH-carrying splat and channel (null without SH)
    float4* shcol;                       // out: evaluated SH colour per splat (null without SH)
    const uint32_t* hidden;              // the scene's hidden set, one bit per splat (null while nothing is hidden: the frame path as it
                                         // was before hidden splats existed); read by k_project_key's projection only
};

// mutable device scene for the on-device build / transforms (k_scene.hip)
struct SceneDev {
    float *px, *py, *pz;
    uint32_t *cov0, *cov1, *cov2, *rgba;
    float4* rot;   // (w, x, y, z) as Scene._rotations stores them
    float4* scl;   // Scene._scales
};
void launch_build_scene(const uint8_t* rows, uint32_t n, const SceneDev& sc, hipStream_t s);
void launch_scene_translate(uint32_t n, const SceneDev& sc, const double* t, hipStream_t s);
void launch_scene_rotate(uint32_t n, const SceneDev& sc, const double* q_xyzw, hipStream_t s);
void launch_scene_scale(uint32_t n, const SceneDev& sc, const double* sv, hipStream_t s);
// The order-preserving compaction (Scene.limitBox, gsr_scene_erase_selected) and which splats stay: those inside `box` (six f64,
// limitBox's comparisons), or, with box null, those whose bit of the mask_words selection words `mask` equals `keep` (a word
// behind them reads as zero).
struct ScenePred { const double* box; const uint32_t* mask; uint32_t keep; uint32_t mask_words; };
void launch_scene_compact(uint32_t n, const SceneDev& src, const SceneDev& dst, const ScenePred& p, uint32_t* block_count,
                          uint32_t* total, hipStream_t s);
// The compaction of a scene whose SH colour follows it, enqueued behind launch_scene_compact while `src` still holds the source
// positions: count[1..3] <- the kept splats in front of bandsIndices[k] + 1 (count[0]: the total the scan left there), and the
// 8-word rows of the kept SH splats of sh_in[0..2], in order, into sh_out[0..2] (sh_count rows each).
void launch_scene_compact_sh(uint32_t n, const SceneDev& src, const ScenePred& p, const uint32_t* block_off, uint32_t* count,
                             const int32_t* band, uint32_t sh_count, const uint32_t* const* sh_in, uint32_t* const* sh_out, hipStream_t s);
// A one-bit-per-splat set through the same compaction (the hidden set), enqueued behind launch_scene_compact while `src` still
// holds the source: out[new index of i] = in[i] for every kept i; `out` (nwords_out words) has been zeroed by the caller.
void launch_scene_compact_bits(uint32_t n, const SceneDev& src, const ScenePred& p, const uint32_t* block_off, const uint32_t* in,
                               uint32_t nwords_in, uint32_t* out, uint32_t nwords_out, hipStream_t s);
// Scene.scales (3 f32 per splat, device memory) -> scl; and the scene back into the layouts of Scene.data (8 words per splat,
// 16-byte aligned), positions and scales (3 f32 per splat): a null output is skipped.  Rotations need neither: `rot` IS
// Scene.rotations' layout.
void launch_scene_import(const float* scales, uint32_t n, float4* scl, hipStream_t s);
void launch_scene_export(uint32_t n, const SceneDev& sc, uint32_t* data, float* positions, float* scales, hipStream_t s);

// ---- launchers (each enqueues on `s`; none synchronises) ----
void launch_repack_scene(const uint32_t* data, const float* positions, uint32_t n, float* px, float* py, float* pz,
                         uint32_t* cov0, uint32_t* cov1, uint32_t* cov2, uint32_t* rgba, uint32_t* mismatch, hipStream_t s);

void launch_repack_positions(const float* positions, uint32_t n, float* px, float* py, float* pz, hipStream_t s);

// frame_words: the context's per-frame device words, [0] = minDepth, [1] = maxDepth, the rest zero at frame start
void launch_begin_frame(const CamParams& cam, CamParams* dst, uint32_t* frame_words, uint32_t nwords, int32_t* slots, hipStream_t s);
// Frame-wide reductions of k_project_key -- depth min / max over ALL splats (wasm.cpp:14-31), visible splats and the
// 16x16 tiles their boxes overlap (V and D of the byte model) -- go through FRAME_SLOTS accumulators, one 128-byte line
// each: a workgroup folds its values into slot (blockIdx & 63) with four atomics.  ~60 workgroups share a slot over the
// kernel's ~20 us, far from the ~90 same-address atomics per microsecond at which one word saturates (with ONE pair of
// words for 4000 workgroups the kernel stayed alive ~17 us after its last store).  The consumers fold the 64 slots
// themselves (k_quantise_hist, k_bin_finalize): no reduction kernel.
// Blocks are dealt round-robin over the 8 XCDs (observed, used for speed only: MI355X_MICROARCH.md, Workgroup dispatch).
// The kernels that APPEND runs to many output streams (radix digits, bin lists) want neighbouring input blocks on one XCD,
// so that the runs they append to a stream meet in one L2 instead of leaving two XCDs as partial lines: inside every
// group of 64 consecutive blocks, XCD k takes the 8 consecutive blocks [8k, 8k+8).  Groups, not one contiguous range per
// XCD: the input is depth-ordered and the front blocks hold the nearest, largest splats -- a contiguous range per XCD
// gave one XCD all the heavy blocks (C4 binning +17 %).  Bijective for any grid size (the tail keeps its order).
// Measured: k_bin_scatter 330 -> 286 us at 20 M splats, binning -4.5 % on C3 and C4; first radix pass 98 -> 93 us at 20 M.
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t xcd_group_remap(uint32_t bid, uint32_t nwg)
{
    constexpr uint32_t RUN = 8u, G = 8u * RUN;   // blocks per XCD in a group, blocks per group (runs of 16 and 32 measured the same)
    const uint32_t full = nwg - nwg % G;
    if (bid >= full) return bid;
    const uint32_t in = bid % G;
    return (bid - in) + (in % 8u) * RUN + in / 8u;
}
#endif
// -DGSR_BOUNDS (diagnostic build, scripts/build_exp.sh bounds "-DGSR_BOUNDS"; tests/test_gpu_bounds.py runs the parity tests'
// frames on it): every index the kernels derive from device data -- list entries, splat indices, slots, LDS cells -- is
// checked against the extent of what it indexes; a violation is counted per site in the translation unit's g_bounds[]
// (gsr_debug_bounds_*), never trapped: a faulting kernel can take the whole node down.  The stand-in for the GPU
// sanitizers this pool does not offer.  Nothing of it is compiled into the shipped library.
#ifdef GSR_BOUNDS
#define GSR_BOUNDS_DECL(name) __device__ unsigned int g_bounds_##name[8];                                             \
    extern "C" int gsr_debug_bounds_##name(unsigned int* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bounds_##name), sizeof g_bounds_##name) == hipSuccess ? 0 : -1; }
#define GSR_BOUND(name, site, idx, limit) do { if (!((unsigned long long)(idx) < (unsigned long long)(limit))) atomicAdd(&g_bounds_##name[site], 1u); } while (0)
#else
#define GSR_BOUNDS_DECL(name)
#define GSR_BOUND(name, site, idx, limit) do { } while (0)
#endif

// Compositor work items: four words, (bin | segment << 16, first list entry, end, first partial slot of the bin | its segments << 25).
constexpr uint32_t PROJ_THREADS = 256;
constexpr int FRAME_SLOTS = 64;
constexpr int FRAME_SLOT_WORDS = 32;   // words per slot (one 128-byte line): [0] min depth, [1] max depth, [2] visible, [3] tiles,
                                       // [4] sum of opacity byte x tiles / 16 (the frame's optical depth over the splats' boxes, k_bin_finalize),
                                       // [5] sum of opacity byte x footprint pixels / 256 (the optical mass the splats really carry)
// the depth key and the min / max alone (sort-only frames): camera by value, its own frame slots, the next frame's reset
void launch_depth_key(const SceneSoA& sc, uint32_t n, const CamParams& cam, int32_t* depth, int32_t* slots, int32_t* slots_next, hipStream_t s);
// The projection kernel's launch as a value: its arguments and the pointer array hipLaunchKernel / a graph kernel node take.
// (One struct for both, so that the graph replay rewrites exactly what a direct launch passes: the camera.)
struct ProjectLaunch {
    SceneSoA sc; uint32_t n; CamParams cam; int do_project;   // do_project: 1 = project (render frames), 2 = records and pixel boxes only (read-back)
    // INVARIANT (band contexts, `kept` set): depth[] and rect[] are NOT indexed by splat for every splat.  depth[] holds each
    // workgroup's survivors packed to the front of its own 256 slots; rect[i] is written for survivors only.  Every other slot
    // keeps what an OLDER frame (another band, the full frame, a sort-only frame) left there.  Whoever reads them goes through
    // this frame's survivors -- kept[] / kept_lane[] / koff[], or depth_index[0 .. sorted_count) -- and through nothing else; a
    // reader that indexes either by splat gets another frame's data with no warning.  rec[i] likewise is written for splats that
    // pass the culls only (full-frame contexts too): it is read through the bin lists, which hold no other splat.  Pinned by
    // tests/test_gpu_history.py (band -> full -> band, band moved, on the bounds-checked build as well).
    int32_t* depth;
    int32_t* slots;      // FRAME_SLOTS * FRAME_SLOT_WORDS, clean at the start of the frame (the finalize step resets them)
    Record* rec; uint2* bbox;   // bbox may be null (frames: nothing on the path reads the pixel boxes)
    uint32_t* rect;      // n: packed bin rectangle per splat (see the invariant above)
    uint32_t* overflow;  // the frame's overflow word, zeroed by the kernel
    uint32_t* kept;      // band mode: per 256-splat workgroup, the survivors it packed to the front of its depth slots (null: no packing)
    uint8_t* kept_lane;  // band mode: n: the lane (index & 255) a packed slot's splat came from
    void* ptrs[12];
    void bind();
};
const void* project_key_kernel();
dim3 project_key_grid(uint32_t n);
void launch_project_key(ProjectLaunch& a, hipStream_t s);

// Waves per workgroup of the four heavy front-end kernels of the one-level 1080p chain (k_scatter's bucket-order pass, k_local_sort,
// k_bin_count, k_bin_scatter): WIDE everywhere, NARROW in throughput contexts, where a front-end workgroup has to fit the wave
// slots and registers that retiring compositor workgroups of the other frames free on a CU (SortPlan::waves, BinPlan::form).  A
// workgroup owns the same keys / ranks and the same table row at either width, and both widths write the same bits.
constexpr uint32_t FRONT_WAVES_WIDE = 16, FRONT_WAVES_NARROW = 8;

// The sort plan: which of k_sort.hip's forms a frame runs, on what, with what grids and LDS sizes.  plan_sort (k_sort.hip) is
// the one place that decides it; alloc_sort sizes the buffers from sort_sizes, build_frame_args asks plan_sort once per frame
// (the order depends on the bucket size the last frame reported) and takes every pointer that depends on the form from the
// answer, launch_sort launches from it, and -- being part of SortBuffers, hence of FrameArgs -- a captured graph is dropped
// exactly when it changes.  Trivially copyable, filled by name into zeroed storage (FrameArgs is compared as bytes).
enum SortForm : uint32_t {
    SORT_NONE = 0,            // a scene without splats: no launch
    SORT_LSD,                 // low digit, then high digit: k_quantise_hist, scan, k_scatter<8>, k_hist_hi, scan, k_scatter<9> (6 launches)
    SORT_BUCKET_WIDE,         // high digit first, then one workgroup per bucket chunk: k_quantise_hist, scan, k_scatter<9>, k_local_sort<16> (4 launches)
    SORT_BUCKET_NARROW,       // the same at FRONT_WAVES_NARROW (throughput contexts): k_scatter<9, .., 8>, k_local_sort<8>
};
struct SortPlan {
    uint32_t form;               // SortForm
    uint32_t carry;              // 1: the packed bin rectangles travel with the keys (SortBuffers::rects_out is set)
    uint32_t band;               // 1: the kernels run on the band's survivors (SortBuffers::koff is set)
    uint32_t keys_per_block;     // keys of a radix workgroup: 2048, 4096 or 8192
    uint32_t blocks;             // radix workgroups = rows of block_hist in use: ceil(n / keys_per_block)
    uint32_t waves;              // waves per workgroup of k_scatter and k_local_sort: FRONT_WAVES_WIDE, or _NARROW in the narrow form
    uint32_t lds_first, lds_last;   // dynamic LDS bytes of the first and the last k_scatter pass (bucket forms: one pass, lds_last = 0)
    uint32_t local_grid;         // bucket forms: the grid of k_local_sort (at least the frame's bucket chunks)
    uint32_t proj_blocks;        // blocks of k_project_key: the `nb` of k_kept_scan and k_band_gather (band frames)
};
struct SortSizes {               // what the per-splat allocation of `rows` splats needs beside its n-word buffers, in words
    uint32_t keys_per_block;
    size_t block_hist, chunk_tab, kept, koff;
};
struct SortKnobs { int32_t sort_order; uint32_t sort_kpb, rect_carry, rect_carry_bucket; };   // Knobs::sort_order, sort_kpb, rect_carry, rect_carry_bucket
// (n: the scene's splats; rows: the splats the buffers were allocated for, which picked the keys per block; front_waves:
//  FRONT_WAVES_WIDE or _NARROW; cull: the frame composites a band; largest_bucket: the word the last sorted frame left in the
//  mailbox, 0xffffffff before a scene's first.  No HIP call, no environment.)
SortPlan plan_sort(uint32_t n, uint32_t rows, uint32_t front_waves, bool render, bool cull, uint32_t largest_bucket, const SortKnobs& k);
SortSizes sort_sizes(uint32_t rows, const SortKnobs& k);

// radix sort of the 17-bit keys; see k_sort.hip
struct SortBuffers {
    const int32_t* depth;      // n
    const int32_t* slots;      // FRAME_SLOTS partial (min, max) pairs of k_project_key
    int32_t* minmax;           // 2: folded by k_quantise_hist (workgroup 0 stores it for the host / read-backs)
    uint32_t* keys;            // n   17-bit keys, original order
    uint32_t* keys_tmp;        // n   keys after pass 1
    uint32_t* idx_tmp;         // n   indices after pass 1
    uint32_t* depth_index;     // n   result
    uint32_t* block_hist;      // plan.blocks rows of RADIX_HI_BINS (SortSizes::block_hist)
    uint32_t* digit_total;     // RADIX_LO_BINS + RADIX_HI_BINS
    const uint32_t* rect;      // per splat: packed bin rectangle of the projection (carried with the keys when rects_out is set)
    const uint32_t* kept;      // band mode (koff set): per 256 splats, the survivors k_project_key packed to the front of their
    const uint8_t* kept_lane;  //   depth slots, and the lane each came from: everybody else is absent from the sort
    uint32_t* koff;            // band mode (plan.band): SortSizes::koff words: the survivors in front of every block (k_kept_scan); null otherwise
    uint32_t* count;           // out: keys the first pass kept (n, or the band's survivors) = entries of depth_index
    SortPlan plan;             // the form and its launch shapes (plan_sort)
    uint32_t* max_bucket;      // out: keys in the frame's largest high-digit bucket (host-mapped word)
    uint32_t* chunk_tab;       // bucket forms: SortSizes::chunk_tab words: k_local_sort's work list (k_scatter's first workgroup writes it)
    uint32_t* rect_tmp;        // with rects_out, in either order: the rectangles after the first pass
    uint32_t* rects_out;       // plan.carry: out: the packed bin rectangles in depth order -- in the LSD order by default, in the bucket order
                               // too with GSR_RECT_CARRY=2 (null: not carried; the binning gathers them)
};
void launch_sort(const SortBuffers& b, uint32_t n, hipStream_t s);
// column scan (k_sort.hip), shared with the binning
// (live: the frame holds *live keys or ranks, live_unit of them per table row: the rows behind are neither written nor scanned)
void launch_column_scan(uint32_t* table, uint32_t* total, int ncols, uint32_t nrows, hipStream_t s, const uint32_t* live = nullptr, uint32_t live_unit = 1);

struct BinGrid {
    int32_t nbx, nby;          // bins across / down the whole image
    int32_t bx_lo, bx_hi;      // bin columns of this context's band [lo, hi)
    int32_t W, H;
};
// The binning plan: which of k_bin.hip's forms a frame runs, with what grids, LDS sizes and table shape.  plan_bins (k_bin.hip)
// is the one place that decides it; alloc_bins sizes the buffers from it and keeps it, launch_bin launches from it, and -- being
// part of BinBuffers, hence of FrameArgs -- a captured graph is dropped exactly when it changes.  Trivially copyable, filled by
// name into zeroed storage (FrameArgs is compared as bytes).
enum BinForm : uint32_t {
    BIN_FINALIZE_ONLY = 0,    // a scene without splats: k_bin_finalize alone
    BIN_FUSED_WIDE,           // k_bin_count<16> + k_bin_scatter<groups, true> (the finalize step is the scatter's extra workgroup)
    BIN_FUSED_NARROW,         // k_bin_count<8> + k_bin_scatter_narrow<8>: the same at FRONT_WAVES_NARROW (throughput contexts)
    BIN_SEPARATE_FINALIZE,    // k_bin_count<16> + k_bin_finalize + k_bin_scatter<4, false>
    BIN_LARGE_GRID,           // k_bin_count<16> + k_bin_starts + k_bin_scatter_big<4, steps_per_wave>, `rounds` rounds per workgroup
    BIN_TWO_LEVEL,            // k_bin_count<16> + k_cell_scatter1<groups> over cells, then k_cell_count / _scan / k_bin_starts / k_cell_scatter2
};
struct BinSlices { int32_t sx, sy, w, h; };  // sx x sy sub-grids of w x h bins (the last ones may be smaller)
struct BinPlan {
    uint32_t form;               // BinForm
    int32_t nbins;               // bins of the context's band
    uint32_t groups;             // step groups of the scatter workgroup: 8 or 4
    uint32_t steps_per_wave;     // 64-rank steps per wave and round: 2; 4 in the narrow form; 1 in the large-grid form's 1024-rank rounds
    uint32_t rounds;             // rounds of 2048 ranks a binning workgroup takes (> 1 only in the large-grid form)
    uint32_t blocks;             // binning workgroups = table rows in use: ceil(ranks / (2048 * rounds))
    BinSlices slices;            // the scatter's sub-grids (blockIdx.y) -- of cells in the two-level form
    uint32_t count_slices, count_rows;   // the count pass's row slices (blockIdx.y) and the bin rows of one
    uint32_t count_lds, scatter_lds;     // dynamic LDS bytes of the count and the (level-one) scatter kernel
    uint32_t extra_wg;           // 1: the scatter's grid has one more workgroup, the finalize step
    uint32_t table_rows, table_cols;     // the [workgroup][bin] table (two levels: [workgroup][cell + 1]); elements = rows x columns
    int32_t ncx, ncy, ncells;    // cells of 4 x 4 bins across / down the band
    uint32_t cell_grid;          // two levels: workgroups of the level-two kernels (they stride over the frame's chunks)
    uint32_t chunks;             // two levels: entries the per-chunk tables are allocated for
};
struct BinKnobs { int32_t two_level; uint32_t big; int64_t rounds; uint32_t cell_grid; };   // Knobs::bin_two_level, bin_big, bin_rounds, cell_grid
// (capacity: entries of the list; cu_count: the device's compute units; front_waves: FRONT_WAVES_WIDE or _NARROW.  No HIP call.)
BinPlan plan_bins(const BinGrid& g, uint32_t n, uint64_t capacity, int cu_count, uint32_t front_waves, const BinKnobs& k);

// The whole-bin sentinel: a minimum segment length that makes every bin one compositor work item, which early termination needs
// (a segment cannot see whether earlier ones saturated the bin).  The one statement of the value written and of how it is read,
// for the host (plan_blend) and the device (k_bin_finalize) alike.
constexpr uint32_t SEG_LEN_WHOLE_BIN = 0x7fffff00u;
__host__ __device__ inline bool is_whole_bin(uint32_t seg_len) { return seg_len >= 0x40000000u; }

// The compositor plan: which of k_blend.hip's four kernels a frame runs, on what grid, and how k_bin_finalize cuts the bin lists
// into its work items.  plan_blend (k_blend.hip) is the one place that decides it; alloc_bins sizes the work items, the partials
// and the arrival masks from it and keeps it, build_frame_args copies it, launch_bin hands k_bin_finalize its policy, launch_blend
// launches from it, and -- being part of BlendBuffers, hence of FrameArgs -- a captured graph is dropped exactly when it changes.
// Trivially copyable, filled by name into zeroed storage (FrameArgs is compared as bytes).
struct BlendPlan {
    uint32_t waves_per_tile;     // 1 (k_blend, 256-thread workgroups) or 2 (k_blend2: halves a wave's serial walk)
    uint32_t fused;              // 1: the workgroup delivering a bin's last segment folds the bin inside the kernel (arrival masks)
    uint32_t separate_fold;      // 1: k_combine is launched behind the compositor (not fused, and bins are cut into segments)
    uint32_t whole_bin;          // 1: every bin is one work item (is_whole_bin(seg_len)): no partials, nothing to fold
    uint32_t threads;            // per workgroup: BLEND_THREADS x waves_per_tile
    uint32_t grid;               // persistent workgroups wanted: the per-CU figure x CUs (GSR_BLEND_GRID pins it)
    uint32_t queue_start;        // min(max_items, grid): the workgroups launched -- each takes the work item of its own index first --
                                 // and the value k_bin_finalize sets the work-item counter to
    uint32_t seg_len;            // minimum list entries per work item (a multiple of 256), or SEG_LEN_WHOLE_BIN
    uint32_t seg_target_items;   // full segments the frame should be cut into at least (long lists -> longer segments)
    uint32_t max_items;          // work items the item table holds (four words each); only grows unless sized afresh
    uint32_t partial_slots;      // per-segment partials to allocate (BIN_PX x BIN_PX float4 each): max_items, 0 for whole bins
    // the work-item policy k_bin_finalize is handed
    int32_t items_by_size;       // order the bins' last segments by size class (one frame at a time) or leave them in raster order
    int32_t long_policy;         // work items of at least seg_len_long entries: 1 always, 0 never, -1 where the frame's optical depth >= long_tau
    uint32_t seg_len_long, long_tau;
    uint32_t long_tiles_x2;      // long work items also need this many 16x16 tiles per visible splat, times two (0: no such condition)
    uint32_t long_tau_bin;       // 0: the built-in per-bin thresholds (k_bin_finalize); else: bins from this optical depth on are one item (GSR_LONG_TAU)
    uint32_t long_mass_min;      // a frame that is not dense as a whole: its saturated bins become items only from this optical mass per list entry on (pixels)
    uint32_t npix;               // pixels of this context's band (the optical depth is per pixel)
    uint32_t saturate;           // 1: quadrants whose pixels can no longer change are skipped (bit-identical; k_blend); 0: A/B knob
};
// Knobs::fuse_combine, saturate, items_by_size, long_items, long_tau, blend_sub, seg_target, blend_grid, seg_len
struct BlendKnobs { uint32_t fuse_combine, saturate; int32_t items_by_size, long_items; uint32_t long_tau; int32_t blend_sub; uint32_t seg_target, blend_grid, seg_len; };
// (nbins: bins of the context's band; npix: its pixels; capacity: entries of the list; cu_count: the device's compute units;
//  early_out: early termination is on; allocated_items: the work items the item table holds already, 0 = size afresh.
//  No HIP call, no environment.)
BlendPlan plan_blend(uint32_t nbins, uint32_t npix, uint32_t capacity, int cu_count, bool throughput, bool early_out, uint32_t allocated_items,
                     const BlendKnobs& k);

struct BinBuffers {
    const uint32_t* depth_index; // *count entries
    const uint32_t* count;       // ranks to bin (SortBuffers::count)
    uint32_t* table;             // plan.table_rows x plan.table_cols  (counts, then per-workgroup offsets inside each bin)
    int32_t* slots;              // FRAME_SLOTS partial (visible splats, 16x16 tile overlaps) sums of k_project_key; the finalize step,
                                 // their last reader in a frame, resets them for the next one
    const uint32_t* rect_idx;    // n: packed bin rectangle of every splat (k_project_key)
    uint32_t* rects;             // n: the same in depth order (count pass -> scatter pass)
    uint32_t rects_sorted;       // 1: the sort has left them there already (SortBuffers::rects_out)
    uint32_t* bin_total;         // nbins (zeroed by the caller when n == 0)
    uint32_t* bin_start;         // nbins + 1
    uint32_t* bin_start_pre;     // nbins + 1: the same starts, computed ahead of the scatter by k_bin_starts (large-grid form)
    BinPlan plan;                // the form and its launch shapes (plan_bins)
    uint32_t* seg_start;         // nbins + 1: first compositor work item of each bin; [nbins] = item count
    uint32_t* items;             // max_items x 4 words: (bin | segment << 16, first list entry, end, first partial slot of the bin | its segments << 25)
    uint32_t* list;              // capacity entries (splat indices, depth order inside each bin)
    uint32_t* overflow;          // bit 0: list too small, bit 1: item table too small
    uint64_t* visible;           // V counter
    uint64_t* tile_entries;      // D counter (16x16 tiles overlapped by visible bboxes)
    uint64_t* accum;             // [8] running sums over frames: visible, bin entries, tile entries, frames; [4] = entries the last frame needs;
                                 // sticky: [5] = frames that did not fit (never composited), [6] / [7] = most entries / items one of them needed
    uint64_t* mailbox;           // host-mapped word: accum[5] is stored here whenever it changes
    uint64_t* report;            // [6] per-frame copy for the host: accum[0..4] after this frame, [5] = this frame's bin entries
    uint32_t capacity;
    uint32_t* seg_len_dev;       // [0] the frame's segment length (k_bin_finalize raises BlendPlan::seg_len for long lists and publishes the
                                 // frame's value here), [1] its number of work items, [2] reserved (0)
    uint32_t* queue;             // the compositor's work-item counter, set to BlendPlan::queue_start (= its grid size) by k_bin_finalize
    unsigned long long* bin_mask; // nbins: the compositor's per-bin arrival masks (one bit per segment), zeroed by the finalize step (may be null)
    // two-level binning (launch_bin; large bin grids): cells of 4 x 4 bins first, then the cell lists' chunks into the bins
    uint32_t* cell_list;         // 2 x capacity words: (splat index, rectangle in bins) per cell-list entry
    uint32_t* cell_total;        // cells + 1: entries per cell; [cells] = list entries the frame needs
    uint32_t* cell_start;        // cells + 1
    uint32_t* chunk_start;       // cells + 2: first chunk of each cell, the frame's chunks, the frame's need
    uint32_t* chunk_info;        // (capacity / 2048 + cells) x 4: per chunk its cell, first and end entry
    uint32_t* cell_wcnt;         // (capacity / 2048 + cells) x 64 words: per chunk, bin and wave of k_cell_scatter2 one byte: the wave's entries
    uint32_t* cell_table2;       // (capacity / 2048 + cells) x 16: per chunk and bin of its cell: entries, then their first slot
    uint32_t band;               // 1: a band context (the frame holds fewer ranks than the scene: scans and workgroups stop at *count's rows)
    uint32_t n_max;              // entries the rank-ordered buffers hold (the scene's splats): k_bin_count may load that far before it knows *count
};
// (bp: the compositor's plan, of which the finalize step is handed the work-item policy)
void launch_bin(const BinBuffers& b, const BlendPlan& bp, const BinGrid& g, hipStream_t s);

struct BlendBuffers {
    const uint32_t* items;      // work items, four words each (BinBuffers::items)
    const uint32_t* seg_start;  // nbins + 1
    const uint32_t* bin_start;  // nbins + 1
    const uint32_t* list;
    const Record* rec;
    const float4* shcol;        // evaluated SH colours (may be null)
    float4* fb;
    float4* partial;            // plan.partial_slots * 1024 float4: per-segment (colour, transmittance), slot = seg_start[bin] + segment
    uint32_t* queue;            // device-wide work-item counter (k_bin_finalize sets it to plan.queue_start)
    const uint32_t* seg_len_dev; // [0] the frame's segment length, [1] its number of work items (k_bin_finalize)
    uint32_t capacity;          // entries the list can hold
    uint32_t nsplats;
    unsigned long long* bin_mask; // nbins arrival masks, zeroed by the finalize step (plan.fused; null otherwise)
    BlendPlan plan;             // the kernel, its grid and the work-item policy (plan_blend)
};
// `between` (may be null) is recorded after the compositor and before k_combine
void launch_blend(const BlendBuffers& b, const BinGrid& g, float early_out_eps, hipStream_t s, hipEvent_t between);
void launch_clear_fb(float4* fb, int32_t W, int32_t H, hipStream_t s);
void launch_to_rgba8(const float4* fb, uint32_t* out, uint32_t npix, hipStream_t s);
// The one statement of the f32 -> RGBA8 rounding (k_to_rgba8, k_pack_band_rgba8, k_deliver_rgba8): round(clamp(x, 0, 1) * 255),
// built without contraction like the rest of the device code.
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t to_rgba8(float4 v)
{
    auto q = [](float x) -> uint32_t {
        x = fminf(fmaxf(x, 0.0f), 1.0f);
        return (uint32_t)(x * 255.0f + 0.5f);
    };
    return q(v.x) | (q(v.y) << 8) | (q(v.z) << 16) | (q(v.w) << 24);
}
#endif
// Frame delivery (k_deliver.hip): the framebuffer as RGBA8 into a delivery slot's device staging, npix pixels followed by a
// DELIVER_TRAILER_WORDS trailer: [0] the frame's overflow word (non-zero: the frame was not composited, the pixels are the
// preceding image), [1] W | H << 16, [2] / [3] the frame's serial, low / high word.
constexpr int DELIVER_TRAILER_WORDS = 4;
void launch_deliver_rgba8(const float4* fb, uint32_t* staging, int32_t W, int32_t H, uint64_t serial, const uint32_t* overflow, hipStream_t s);
// The same frame as 4:2:0 Y'CbCr ("Frame delivery in Y'CbCr"): everything in integers on the frame's RGBA8
// bytes.  y / cb / cr: the (R, G, B) rows in 1/256; chroma is taken from the sums of a 2 x 2 block, clamped to [c_lo, c_hi].
struct YuvParams {
    int32_t y0, y[3], cb[3], cr[3], c_lo, c_hi;
    uint32_t bg;   // the background the premultiplied pixel is laid over, R | G << 8 | B << 16 (0: black, nothing to add)
};
constexpr int DELIVER_NV12 = 1, DELIVER_I420 = 2;   // (GSR_FORMAT_NV12 / GSR_FORMAT_I420)
// payload bytes of a W x H frame in 4:2:0 (either layout); the trailer follows at the next multiple of four
inline size_t yuv420_bytes(int32_t W, int32_t H) { return (size_t)W * H + 2 * (size_t)((W + 1) / 2) * ((H + 1) / 2); }
// Exactly one of fb (the f32 framebuffer, through to_rgba8) and frame8 (a group's gathered RGBA8 frame) is the source.
// `overflow`: the word the trailer's first word is read from (the frame's overflow word / the gathered frame's stale mask).
// `staging_bytes`: what `staging` holds (payload, padding and trailer; the bounds-checked build compares against it).
void launch_deliver_yuv(int format, const float4* fb, const uint32_t* frame8, uint8_t* staging, size_t staging_bytes, int32_t W, int32_t H,
                        const YuvParams& k, uint64_t serial, const uint32_t* overflow, hipStream_t s);
// The depth plane of a depth ring ("Frame delivery with depth"): `plane`, Wd x Hd f32 hit values, into
// `staging` at `depth_offset` as f32 or as 16-bit inverse depth against `near`, and the slot's trailer (as above, W | H << 16
// the frame's size) at `trailer_offset`; both offsets are multiples of 16, the plane ends at or in front of the trailer.
constexpr int DELIVER_DEPTH_F32 = 1, DELIVER_DEPTH_U16 = 2;   // (GSR_DEPTH_F32 / GSR_DEPTH_U16)
void launch_deliver_depth(int format, const float* plane, uint8_t* staging, size_t depth_offset, size_t trailer_offset, int32_t Wd, int32_t Hd, float near,
                          int32_t W, int32_t H, uint64_t serial, const uint32_t* overflow, hipStream_t s);

// The last frame's lists as the passes behind the frame walk them once more (k_depth_walk.h: depth planes and picking, contribution,
// selection overlay): filled in one place, frame_lists of gsr_depth.cpp.
struct FrameLists {
    const uint32_t* bin_start;   // nbins + 1
    const uint32_t* list;
    const Record* rec;
    const float *px, *py, *pz;   // the scene's positions (a splat's depth is computed from them and the frame's camera)
    const uint32_t* overflow;    // the frame's overflow word: non-zero = its lists did not fit, nothing of it may be walked
    uint32_t capacity;           // entries the list can hold
    uint32_t nsplats;            // splats of the scene, at least 1 (the walk clamps a list entry to nsplats - 1)
};

// Depth planes and picking (k_depth.hip): the lists walked for depth instead of colour.
struct DepthBuffers : FrameLists {
    uint32_t* invalid;           // out: 1 when the pass refused the frame (nothing written), 0 otherwise
    float* mean; float* hit; uint32_t* index;   // the planes, W x H each (null for k_pick)
    float hit_alpha;
};
struct PickResult { uint32_t index; float depth, mean, alpha; };   // gsr_pick_result
// step 1: mean, hit and index, W x H each; step 2: the hit plane only, at the pixels (2i, 2j): ceil(W / 2) x ceil(H / 2) samples
void launch_depth_planes(const DepthBuffers& b, const BinGrid& g, const CamParams& cam, bool skip, int step, hipStream_t s);
void launch_pick(const DepthBuffers& b, const BinGrid& g, const CamParams& cam, const int32_t* xy, uint32_t count, PickResult* out, hipStream_t s);
void launch_depth_fill(float* mean, float* hit, uint32_t* index, uint32_t npix, hipStream_t s);

// Selection (k_select.hip; DESIGN.md section 4, "Selection"): one bit per splat of a scene, bit i & 31 of word i >> 5, bits at and
// above n always 0.  The pickers set the picked splats' bits in a zeroed scratch mask; launch_select_apply folds it into the selection.
constexpr int SELECT_CENTRE = 0, SELECT_HIT = 1;                                            // (GSR_SELECT_*)
constexpr int SELOP_REPLACE = 0, SELOP_ADD = 1, SELOP_SUBTRACT = 2, SELOP_INTERSECT = 3,   // (GSR_SELOP_*)
              SELOP_INVERT = 4;                                                             // gsr_selection_invert: S = ~S, the picked set is not read
constexpr uint32_t SELECT_APPLY_THREADS = 256;   // words per workgroup of k_select_apply = words one entry of `block_sums` counts
struct SelectRegion {
    int32_t x0, y0, x1, y1;      // the pixel rectangle [x0, x1) x [y0, y1), inside the image and the context's band
    const uint8_t* bytes;        // one byte per pixel of the rectangle, non-zero = inside; null: the whole rectangle
    int32_t stride;              // bytes per row (>= x1 - x0)
    uint32_t nbytes;             // what `bytes` holds: (y1 - y0 - 1) * stride + (x1 - x0)
};
struct SelectBuffers {
    const uint32_t* bin_start;   // nbins + 1      (SELECT_CENTRE: the frame's lists and records, as DepthBuffers holds them)
    const uint32_t* list;
    const Record* rec;
    const uint32_t* overflow;    // the frame's overflow word: non-zero = its lists did not fit, nothing of it may be walked
    const uint32_t* index;       // SELECT_HIT: the hit-index plane, W x H
    uint32_t* invalid;           // out: 1 when the picker refused the frame (nothing set), 0 otherwise
    uint32_t* scratch;           // nwords, zeroed by the caller
    uint32_t capacity;           // entries the list can hold
    uint32_t nsplats, nwords;
};
void launch_select_region(int mode, const SelectBuffers& b, const BinGrid& g, const SelectRegion& r, hipStream_t s);
// scratch <- the splats inside `box` (in_box of k_scene.hip): every word of it is stored, no zeroing needed
void launch_select_box(uint32_t n, const float* px, const float* py, const float* pz, const double* box, uint32_t* scratch, uint32_t nwords, hipStream_t s);
// sel <- sel (op) scratch, bits at and above n dropped; *count <- the bits set afterwards (block_sums: ceil(nwords / SELECT_APPLY_THREADS) words)
void launch_select_apply(int op, uint32_t* sel, const uint32_t* scratch, uint32_t n, uint32_t nwords, uint32_t* block_sums, uint32_t* count, hipStream_t s);

// Editing the selection (k_edit.hip; DESIGN.md section 4, "Editing the selection"): Scene.translate / rotate / scale on the splats
// whose bit of `words` (nwords of them, the selection's layout) is set, as a Scene holding only them would be left; no other splat
// is written.  pivot (3 f64, may be null): translate(-pivot), the operation, translate(+pivot), each step rounded to f32 as the
// reference's stores round, fused into one read and one write per selected splat.
void launch_edit_translate(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, const double* t, hipStream_t s);
void launch_edit_rotate(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, const double* q_xyzw, const double* pivot, hipStream_t s);
void launch_edit_scale(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, const double* sv, const double* pivot, hipStream_t s);
// rgba[i] = (rgba[i] & ~byte_mask) | (rgba & byte_mask) for the selected i
void launch_edit_rgba(uint32_t n, const SceneDev& sc, const uint32_t* words, uint32_t nwords, uint32_t rgba, uint32_t byte_mask, hipStream_t s);
// The selected splats' count and the box of their centres: out[0] = count, out[1..3] = min, out[4..6] = max (f32 bits), out[7] = 0.
// partial: edit_bounds_blocks(n) x EDIT_PARTIAL_WORDS words of scratch; out: EDIT_PARTIAL_WORDS words.  n >= 1.
constexpr uint32_t EDIT_PARTIAL_WORDS = 8;
uint32_t edit_bounds_blocks(uint32_t n);
void launch_edit_bounds(uint32_t n, const float* px, const float* py, const float* pz, const uint32_t* words, uint32_t nwords, uint32_t* partial,
                        uint32_t* out, hipStream_t s);

// Rotating SH coefficients (k_sh_rotate.hip; DESIGN.md section 4, "Rotating SH coefficients"): the band matrices D_1, D_2, D_3 of
// gsr_sh_rotation rounded once to f32, row-major; passed by value, so a wave reads them from scalar registers.
struct ShRotation { float d1[9], d2[25], d3[49]; };
// c' = D_l c per band, in place, on the rows of tex[0..2] (sh_count rows of 8 words each; row t belongs to splat first + t, and
// n = first + sh_count): every row (words null), or the rows of the splats whose bit of `words` (nwords of them, the selection's
// layout) is set.  counter (may be null): SH_ROTATE_COUNTERS slots of one word, SH_ROTATE_COUNTER_STRIDE words apart, zeroed by the
// caller; the sum of the slots += the rows rotated.
constexpr uint32_t SH_ROTATE_COUNTERS = 64, SH_ROTATE_COUNTER_STRIDE = 32;
void launch_sh_rotate(uint32_t n, uint32_t first, uint32_t sh_count, uint32_t* const* tex, const uint32_t* words, uint32_t nwords,
                      const ShRotation& M, uint32_t* counter, hipStream_t s);

// Growing the scene (k_append.hip; DESIGN.md section 4, "Growing the scene"): the splats of `src` (n_src of them) whose bit of
// `words` (nwords of them, the selection's layout; bits at and above n_src are not read) is set, in ascending order, copied bit for
// bit into the rows dst_first, dst_first + 1, ... of `dst`, which holds dst_rows rows.  src and dst may be the same arrays (the
// rows read lie below dst_first).  block_sums: append_blocks(n_src) + 1 words of scratch (the scanned per-workgroup counts, then the total).
uint32_t append_blocks(uint32_t n_src);
void launch_append_gather(uint32_t n_src, const SceneDev& src, const SceneDev& dst, uint32_t dst_first, uint32_t dst_rows, const uint32_t* words,
                          uint32_t nwords, uint32_t* block_sums, hipStream_t s);
// words[0 .. nwords) <- exactly the bits [first, first + count); *total <- count
void launch_append_select_range(uint32_t* words, uint32_t nwords, uint32_t first, uint32_t count, uint32_t* total, hipStream_t s);

// Contribution (k_contrib.hip; DESIGN.md section 4, "Contribution"): the last frame's bin lists walked once more, the weight
// w = T * B of every fragment kept per SPLAT and summed over pixels and passes into three accumulators held with the scene.
struct ContribBuffers : FrameLists {   // (a frame that did not fit is neither walked nor counted)
    unsigned long long* weight;  // rows: sum of rintf(w * 2^24) over the splat's fragments
    uint32_t* peak;              // rows: max of w, as the bits of a non-negative f32
    uint32_t* pixels;            // rows: the splat's fragments, modulo 2^32
    uint32_t* frames;            // one word: passes that contributed
    uint32_t rows;               // splats the accumulators were allocated for
};
constexpr int CONTRIB_WEIGHT = 0, CONTRIB_PEAK = 1, CONTRIB_PIXELS = 2;   // (GSR_CONTRIB_*)
void launch_contrib(const ContribBuffers& b, const BinGrid& g, const CamParams& cam, bool skip, hipStream_t s);
// scratch <- the splats i < n whose value (stat) is below `below`, compared in f64: every word of it is stored, no zeroing needed
void launch_contrib_select(int stat, double below, uint32_t n, const unsigned long long* weight, const uint32_t* peak, const uint32_t* pixels,
                           uint32_t* scratch, uint32_t nwords, hipStream_t s);

// Splat data (k_attr.hip; DESIGN.md section 4, "Splat data"): the scene's own attributes reduced, binned and picked by range.
// The value of attribute `attr` of splat i is attr_value (k_attr.h), an f64; the codes are GSR_ATTR_*.
constexpr int ATTR_X = 0, ATTR_Y = 1, ATTR_Z = 2, ATTR_DISTANCE = 3, ATTR_RED = 4, ATTR_GREEN = 5, ATTR_BLUE = 6, ATTR_OPACITY = 7,
              ATTR_SCALE_X = 8, ATTR_SCALE_Y = 9, ATTR_SCALE_Z = 10, ATTR_SCALE_MIN = 11, ATTR_SCALE_MAX = 12,
              ATTR_CONTRIB_WEIGHT = 13, ATTR_CONTRIB_PEAK = 14, ATTR_CONTRIB_PIXELS = 15, ATTR_COUNT = 16;
static_assert(ATTR_CONTRIB_PEAK == ATTR_CONTRIB_WEIGHT + CONTRIB_PEAK && ATTR_CONTRIB_PIXELS == ATTR_CONTRIB_WEIGHT + CONTRIB_PIXELS,
              "the contribution attributes are GSR_CONTRIB_* behind ATTR_CONTRIB_WEIGHT");
// where the values come from; a kernel reads only the arrays its attribute names (the others may be null)
struct AttrSource {
    const float *px, *py, *pz;
    const uint32_t* rgba;                  // r | g << 8 | b << 16 | opacity << 24 (gsr_scene_set_rgba_selected's numbering)
    const float4* scl;                     // Scene._scales
    const unsigned long long* weight;      // the contribution accumulators (ContribBuffers)
    const uint32_t* peak;
    const uint32_t* pixels;
    double ox, oy, oz;                     // ATTR_DISTANCE: the origin
};
constexpr uint32_t ATTR_SCOPE_SELECTED = 1u, ATTR_SCOPE_VISIBLE = 2u;   // (GSR_SCOPE_*)
struct AttrScope {
    uint32_t flags;                        // ATTR_SCOPE_*; 0: every splat
    const uint32_t* sel; uint32_t sel_words;   // the selection's words (null: never selected in, nothing is in a SELECTED scope)
    const uint32_t* hid; uint32_t hid_words;   // the hidden set's words (null: nothing is hidden)
};
struct AttrStats { uint32_t count, nan; double mn, mx; };   // splats in scope, those with a NaN value, min / max of the others ((+inf, -inf): none)
constexpr uint32_t ATTR_MAX_BINS = 4096;                    // bins + 3 counters of 4 bytes: an LDS histogram of 16 KB
constexpr uint32_t ATTR_MAX_GRID = 1024;                    // workgroups of a reduction at most = partials of k_attr_stats
struct AttrRange { double lo, hi, w; uint32_t bins; };      // [lo, hi) in `bins` bins of w = (hi - lo) / (double)bins
constexpr int ATTR_HIST_PLAIN = 0, ATTR_HIST_PEEL = 1;     // k_attr_hist's forms (Knobs::attr_hist_peel)
// Workgroups of a reduction over n splats: per_cu per compute unit -- from the device, not from n -- at most ATTR_MAX_GRID and
// never more than ceil(n / 256).  k_attr_stats takes four per compute unit; k_attr_hist two, because every workgroup ends with
// one global atomic per non-zero counter and same-address atomics of many workgroups queue up (512
// workgroups measured fastest, 1024 a third slower, one per 256 splats nearly four times slower).
constexpr uint32_t ATTR_STATS_WG_PER_CU = 4, ATTR_HIST_WG_PER_CU = 2;
uint32_t attr_grid(uint32_t n, int cu_count, uint32_t per_cu);
// partial: attr_grid(n, cu_count, ATTR_STATS_WG_PER_CU) entries of scratch; *out: the result.  n >= 1.
void launch_attr_stats(int attr, const AttrSource& src, const AttrScope& sc, uint32_t n, int cu_count, AttrStats* partial, AttrStats* out, hipStream_t s);
// counters[0 .. bins) += the bins, [bins] += values below lo, [bins + 1] += at or above hi, [bins + 2] += NaN: zeroed by the caller.  n >= 1.
// (blocks: any number of workgroups gives the same counters; attr_grid unless GSR_ATTR_HIST_GRID pins it)
void launch_attr_hist(int attr, const AttrSource& src, const AttrScope& sc, uint32_t n, uint32_t blocks, const AttrRange& r, int form, uint32_t* counters,
                      hipStream_t s);
// scratch <- the splats i < n with lo <= value < hi: every word of it is stored, no zeroing needed
void launch_attr_select(int attr, const AttrSource& src, uint32_t n, double lo, double hi, uint32_t* scratch, uint32_t nwords, hipStream_t s);

// Neighbours (k_neighbours.hip; DESIGN.md section 4, "Neighbours"): for every splat in scope, how many others in scope lie within
// `radius` of it, through a hashed uniform grid built on the device for the one call.  Cell side h = radius * (1 + 2^-10); a cell
// coordinate is floor((double)x * inv_h) clamped to [-NB_CELL_HALF, NB_CELL_HALF); three of them pack into the 63-bit cell key.
constexpr uint32_t NB_MAX_CAP = 4095;                       // GSR_NEIGHBOUR_MAX_CAP: cap + 1 LDS counters of 4 bytes, 16 KB at most
constexpr int32_t NB_CELL_HALF = 1 << 20;                   // 21 bits per axis
constexpr uint32_t NB_WG_PER_CU = 8;                        // workgroups of the walks (bound, count) per compute unit
constexpr uint32_t NB_MAX_GRID = 4096;                      // and at most
// the device words of one call: zeroed by the host in front of the build
struct NbInfo {
    uint32_t in_scope, nonfinite;          // splats in scope; of those, with a NaN or infinite position component
    uint32_t indexed, pad;                 // the index's entries (k_nb_offsets' cursor): in_scope - nonfinite
    unsigned long long pair_bound;         // k_nb_bound's sum
};
struct NbIndex {
    uint32_t* table;                       // 2 * buckets words: [2b] the bucket's population, [2b + 1] its cursor -- the bucket's first
                                           // entry after k_nb_offsets, one behind its last after k_nb_scatter
    uint32_t bucket_mask;                  // buckets - 1, a power of two >= 2 n
    uint4* entry;                          // n: (bits of x, y, z, the splat's index), bucket by bucket
    unsigned long long* key;               // n: the entry's cell key
    NbInfo* info;
    double inv_h, r2;
};
// the index of the splats in scope with finite positions, info->in_scope / nonfinite / indexed, and hist0 += nonfinite (null: no
// histogram); table and *info zeroed by the caller.  n >= 1.
void launch_nb_build(const NbIndex& ix, const float* px, const float* py, const float* pz, const AttrScope& sc, uint32_t n, int cu_count, uint32_t* hist0,
                     hipStream_t s);
// info->pair_bound += for every entry the populations of the 27 buckets the count pass walks for it
void launch_nb_bound(const NbIndex& ix, uint32_t n, int cu_count, hipStream_t s);
// counts[index] = min(cap, neighbours) for every entry (the other words are the caller's zeros); hist (null: none), cap + 1 words
// zeroed by the caller but for hist0's share, += the entries by their count.  indexed: info->indexed as the host read it; n: the splats.
void launch_nb_count(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t cap, uint32_t* counts, uint32_t* hist, int cu_count, hipStream_t s);
// scratch <- the splats i < n in scope with lo <= counts[i] < hi: every word of it is stored, no zeroing needed
void launch_nb_select(const uint32_t* counts, const AttrScope& sc, uint32_t n, uint32_t lo, uint32_t hi, uint32_t* scratch, uint32_t nwords, hipStream_t s);

// Clusters (k_clusters.hip; DESIGN.md section 4, "Clusters"): the connected islands of the splats in scope at a linking radius, over
// the index above.  A label is the smallest splat index of its cluster; CL_NONE is "in no cluster".
constexpr uint32_t CL_NONE = 0xffffffffu;                   // GSR_CLUSTER_NONE
constexpr uint32_t CL_INFO_WORDS = 8;
// the device words of one call: zeroed by the host in front of the walks
struct ClInfo {
    uint32_t core, border;                 // splats that are core; non-core splats that took a core neighbour's label
    uint32_t clusters, fault;              // roots; non-zero when a find or a hook ran into its step limit or met parent[x] > x
    unsigned long long largest;            // max over roots of size << 32 | ~label (0: no cluster)
};
struct ClArrays {
    uint32_t* label;                       // n: parent[] while the union runs, every splat's label afterwards (CL_NONE: none)
    uint32_t* size;                        // n: size[l] = the splats labelled l (zeroed by the caller)
    uint32_t* sizes;                       // n: every splat's size[label] (0: no label)
    ClInfo* info;
};
// label[i] = i for every core entry (counts[i] >= min_pts), CL_NONE for every other splat; info->core.  indexed, n as launch_nb_count's.
void launch_cl_seed(const NbIndex& ix, uint32_t indexed, uint32_t n, const uint32_t* counts, uint32_t min_pts, const ClArrays& a, int cu_count, hipStream_t s);
// the union over every near pair of core entries, then label[i] = its root for every core entry, size[root] and info->clusters
void launch_cl_union(const NbIndex& ix, uint32_t indexed, uint32_t n, const uint32_t* counts, uint32_t min_pts, const ClArrays& a, int cu_count, hipStream_t s);
// label[i] = the smallest label among the near core entries of every non-core entry that has one; size[] and info->border
void launch_cl_border(const NbIndex& ix, uint32_t indexed, uint32_t n, const uint32_t* counts, uint32_t min_pts, const ClArrays& a, int cu_count, hipStream_t s);
// sizes[i] for every splat and info->largest
void launch_cl_sizes(uint32_t n, const ClArrays& a, int cu_count, hipStream_t s);
// scratch <- the splats i < n in scope with lo <= sizes[i] < hi / with label[i] == target (CL_NONE: nobody): every word of it is stored
void launch_cl_select_sizes(const uint32_t* sizes, const AttrScope& sc, uint32_t n, uint32_t lo, uint32_t hi, uint32_t* scratch, uint32_t nwords, hipStream_t s);
void launch_cl_select_label(const uint32_t* label, uint32_t n, uint32_t target, uint32_t* scratch, uint32_t nwords, hipStream_t s);

// k nearest neighbours (k_knn.hip; DESIGN.md section 4, "k nearest neighbours"): for every splat in scope the k nearest others in
// scope within `radius`, ordered by (d2, index), over the index above; a per-splat value (distance to the k-th, or the mean
// distance to those found) and the splats of a value range as a picker.
constexpr uint32_t KNN_MAX_K = 32;                          // GSR_KNN_MAX_K
constexpr uint32_t KNN_NONE = 0xffffffffu;                  // GSR_KNN_NONE: an empty list slot
constexpr int KNN_KTH = 0, KNN_MEAN = 1;                    // GSR_KNN_KTH / GSR_KNN_MEAN
constexpr uint32_t KNN_LDS_BYTES = 48u * 1024u;             // the lists of one workgroup at most: three workgroups in a CU's 160 KiB
// the device words of one call, zeroed by the host in front of the walk.  The values are non-negative doubles, so their bit
// patterns order as unsigned integers: vmax is the largest pattern, nvmin the largest COMPLEMENT of one (0: no finite value).
struct KnnInfo {
    uint32_t complete, finite_values;      // entries with a full list; entries with a finite value
    unsigned long long nvmin, vmax;
};
struct KnnArrays {
    uint32_t* found;                       // n
    double* values;                        // n
    uint32_t* idx;                         // n * k (null: no lists)
    double* d2;                            // n * k
    KnnInfo* info;
};
// lanes of a workgroup of the walk for this k: the most of 256, 128, 64 whose lists (12 bytes per lane and slot) fit KNN_LDS_BYTES
inline uint32_t knn_threads(uint32_t k) { return k * 12u * 256u <= KNN_LDS_BYTES ? 256u : k * 12u * 128u <= KNN_LDS_BYTES ? 128u : 64u; }
// every row as a splat outside the index has it: found 0, value +inf in scope and NaN outside, the slots KNN_NONE and +inf
void launch_knn_fill(const AttrScope& sc, uint32_t n, uint32_t k, const KnnArrays& a, int cu_count, hipStream_t s);
// the walk: found, value and (a.idx) the k slots of every entry at its splat's row; hist (k + 1 words, zeroed by the caller but for
// hist0's share) += the entries by found; a.info += complete, finite_values, min and max.  indexed, n as launch_nb_count's.
void launch_knn(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t k, int stat, const KnnArrays& a, uint32_t* hist, int cu_count, hipStream_t s);
// scratch <- the splats i < n in scope with lo <= values[i] && (values[i] < hi || open_hi): every word of it is stored
void launch_knn_select(const double* values, const AttrScope& sc, uint32_t n, double lo, double hi, bool open_hi, uint32_t* scratch, uint32_t nwords, hipStream_t s);

// Normals (k_normals.hip; DESIGN.md section 4, "Normals"): per splat in scope a unit normal (3 f32), the surface variation (f64) and
// the list length, from the PCA of the k nearest within `radius` over the index above or from the splat's own shortest axis; and
// the splats whose n . axis, |n . axis| or variation lies in a closed range as a picker.
constexpr int NORMAL_KNN = 0, NORMAL_OWN = 1;                              // GSR_NORMAL_KNN / GSR_NORMAL_OWN
constexpr int NORMAL_DOT = 0, NORMAL_ABS_DOT = 1, NORMAL_VARIATION = 2;    // GSR_NORMAL_DOT / _ABS_DOT / _VARIATION
constexpr uint32_t NORMAL_MIN_K = 2;                                        // a normal needs two neighbours
// the device words of one call, zeroed by the host in front of the kernels.  A variation is a non-negative double, so min and max
// go through bit patterns as KnnInfo's do (0: no valid row).  in_scope and nonfinite are the OWN source's; the KNN source takes
// them from the index.
struct NormalInfo {
    uint32_t valid, in_scope, nonfinite, pad;
    unsigned long long nvmin, vmax;
};
struct NormalArrays {
    float* normals;                        // 3 n
    double* variation;                     // n
    uint32_t* found;                       // n
    NormalInfo* info;
};
struct NormalOrient { uint32_t oriented; double tx, ty, tz; };   // oriented != 0: normals face the viewpoint (tx, ty, tz)
// every row as a splat outside the index has it: three quiet NaNs, a NaN variation, found 0
void launch_normals_fill(uint32_t n, const NormalArrays& a, int cu_count, hipStream_t s);
// the walk: normal, variation and found of every entry at its splat's row; a.info += valid, min and max.  indexed, n as
// launch_nb_count's; px / py / pz: the scene's positions, gathered by the listed indices.  k in NORMAL_MIN_K .. KNN_MAX_K.
void launch_normals_knn(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t k, const float* px, const float* py, const float* pz, const NormalOrient& o,
                        const NormalArrays& a, int cu_count, hipStream_t s);
// every row from the splat's own rotation and scale; a.info += in_scope, nonfinite, valid, min and max
void launch_normals_own(const SceneDev& scene, const AttrScope& sc, uint32_t n, const NormalOrient& o, const NormalArrays& a, int cu_count, hipStream_t s);
// scratch <- the splats i < n with lo <= value_i && value_i <= hi, the value from the stored rows (axis: 3 f64 on the host, null
// for NORMAL_VARIATION): every word of it is stored
void launch_normals_select(const float* normals, const double* variation, uint32_t n, int stat, const double* axis, double lo, double hi, uint32_t* scratch,
                           uint32_t nwords, hipStream_t s);

// Merging cells (k_merge.hip; DESIGN.md section 4, "Merging cells"): the candidates of every cell of a uniform grid -- the splats
// in scope whose ten floats are finite -- found through the index above with inv_h = 1 / cell, and every cell of two or more merged
// into one splat by moment matching, written at its leader's row (the smallest member index).
constexpr uint32_t MG_NONE = 0xffffffffu;                   // GSR_CELL_NONE: a leader word of a splat that is no candidate
constexpr uint32_t MG_INFO_WORDS = 8;
// the device words of one call: zeroed by the host in front of the candidate mask
struct MgInfo {
    uint32_t in_scope;                     // splats in scope (k_mg_candidates)
    uint32_t cells, merged_cells;          // cells with a member; with two or more: the cursor of `cells` below
    uint32_t merged_members;               // members of those: the cursor of the member list
    uint32_t largest, fault;               // the largest cell; non-zero when a slice or an index read back from the arrays lay outside them
    unsigned long long pair_bound;         // the sum over the buckets of population^2: what the walk tests at most
};
struct MgArrays {
    uint32_t* cand;                        // words: the candidate mask (the selection's layout)
    uint32_t words;
    uint32_t* leader;                      // n: the smallest member index of the splat's cell (MG_NONE: no candidate)
    uint32_t* count;                       // n: the members of the splat's cell (0: no candidate)
    uint32_t* rank;                        // n: the members of it with a smaller index
    // the edit only (null in the report: the walk then hands out slices and stores none)
    uint32_t* slice;                       // n: at a leader of a merged cell, the cell's first slot of the member list
    uint32_t* member;                      // n: the merged cells' members, a slice per cell, ascending inside it
    uint2* cells;                          // n / 2: (first slot, members) of every merged cell, in no particular order
    uint32_t* remove;                      // words: member of a merged cell and not its leader
    uint32_t* merged;                      // words: leader of a merged cell
    MgInfo* info;
};
// a.cand <- the splats in `sc` with finite position, rotation and scale: every word of it is stored; info->in_scope.  n >= 1.
void launch_mg_candidates(const SceneDev& scene, const AttrScope& sc, uint32_t n, const MgArrays& a, hipStream_t s);
// info->pair_bound from the built index's populations
void launch_mg_bound(const NbIndex& ix, const MgArrays& a, int cu_count, hipStream_t s);
// leader, count and rank of every splat; hist (null: none; cap + 1 words zeroed by the caller) += the cells by min(members, cap);
// info->cells, merged_cells, merged_members, largest; a.slice and a.cells for the merged cells.  indexed: info->indexed as the host read it.
void launch_mg_walk(const NbIndex& ix, uint32_t indexed, uint32_t n, uint32_t cap, const MgArrays& a, uint32_t* hist, int cu_count, hipStream_t s);
// a.member, a.remove and a.merged (every word stored) from leader, count, rank and slice
void launch_mg_members(uint32_t n, uint32_t merged_members, const MgArrays& a, hipStream_t s);
// every merged cell reduced and written at its leader's row of `scene`
void launch_mg_reduce(const SceneDev& scene, uint32_t n, uint32_t merged_cells, uint32_t merged_members, const MgArrays& a, hipStream_t s);

// Planes (k_plane.hip; DESIGN.md section 4, "Planes"): the dominant plane of the splats in scope by RANSAC -- hypotheses drawn by a
// counter-based generator, every one scored against every candidate in f64 -- the scoring pass alone over planes of the host's, and
// the splats whose signed distance from a plane lies in [lo, hi] as a picker.  A candidate is a splat in scope with a finite position.
constexpr uint32_t PLANE_MAX_HYPOTHESES = 4096;             // GSR_PLANE_MAX_HYPOTHESES
constexpr uint32_t PLANE_CHUNK = 512;                       // candidates a score workgroup stages at a time: 3 * 8 * 512 = 12 KB of LDS,
                                                            // so eight 256-lane workgroups (a compute unit's 32 waves) hold 96 of its 160 KB
constexpr uint32_t PLANE_MAX_CHUNK_GROUPS = 2048;           // the score grid's other dimension at most: a group walks chunks g, g + groups, ..
constexpr uint32_t PLANE_THREADS = 256;                     // splats of a candidate workgroup: one entry of the block sums
// what k_plane_best leaves for the host: behind the totals in the call's words
struct PlBest {
    uint32_t degenerate, found, best, triple[3], inliers, pad;
    double plane[4];
};
struct PlArrays {
    unsigned long long* totals;            // in_scope | nonfinite << 32 (zeroed by the caller)
    PlBest* result;
    uint32_t* block;                       // plane_blocks(n) + 1 words: the candidates per 256 splats, scanned in place; [blocks] their number
    uint32_t* cand;                        // cand_rows: the candidates' splat indices, ascending
    uint32_t cand_rows;
    double4* planes;                       // PLANE_MAX_HYPOTHESES each: (a, b, c, d); the triple and, in .w, 1 for a degenerate hypothesis
    uint4* triple;
    uint32_t* scores;
};
inline uint32_t plane_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + PLANE_THREADS - 1u) / PLANE_THREADS); }
// a.cand[0 .. m) <- the candidates in ascending index, a.block[plane_blocks(n)] <- m, *a.totals += in_scope | nonfinite << 32.  n >= 1.
void launch_plane_candidates(const float* px, const float* py, const float* pz, const AttrScope& sc, uint32_t n, const PlArrays& a, hipStream_t s);
// a.planes[h], a.triple[h] for h < hypotheses from the candidates' positions.  m >= 1.
void launch_plane_hypotheses(const float* px, const float* py, const float* pz, uint32_t hypotheses, uint64_t seed, uint32_t m, uint32_t n, const PlArrays& a,
                             hipStream_t s);
// a.scores[h] (zeroed by the caller) += the candidates within `threshold` of a.planes[h], h < count; with `flagged` a hypothesis
// whose a.triple[h].w is set is skipped.  m >= 1.
void launch_plane_score(const float* px, const float* py, const float* pz, uint32_t count, uint32_t m, uint32_t n, double threshold, bool flagged, const PlArrays& a,
                        hipStream_t s);
// *a.result from the scores, the flags, the triples and the planes
void launch_plane_best(uint32_t hypotheses, const PlArrays& a, hipStream_t s);
// scratch <- the splats i < n with lo <= s_i && s_i <= hi: every word of it is stored, no zeroing needed
void launch_plane_select(const float* px, const float* py, const float* pz, uint32_t n, double4 plane, double lo, double hi, uint32_t* scratch, uint32_t nwords,
                         hipStream_t s);

// Matching and registration (k_match.hip; DESIGN.md section 4, "Matching and registration"): for every splat in scope of a SOURCE
// scene under a trial transform, the nearest indexed splat of a TARGET scene within `radius`, by the pair (d2, index), over the
// index above built on the target; the sums a rigid solve needs, by a fixed tree; and the splats of a distance range as a picker.
constexpr uint32_t MATCH_NONE = 0xffffffffu;                // GSR_MATCH_NONE: an unmatched splat
constexpr uint32_t MATCH_ROW = 16;                          // doubles of a row of sums: T, Q, T_a * Q_b for ab = 00 .. 22, d2
constexpr uint32_t MATCH_GROUP = 256;                       // rows one workgroup of the tree reduces to one
struct MatchXf { double m[12]; };                           // row-major 3 x 4 (R | t)
// the source side of a call: the positions of its n splats, its scope and the trial transform
struct MatchSource {
    const float *px, *py, *pz;
    AttrScope sc;
    uint32_t n;
    MatchXf xf;
};
// the device words of one step, zeroed by the host in front of the bound.  Squared distances are non-negative doubles, so their
// bit patterns order as unsigned integers (KnnInfo): d2max is the largest pattern, nd2min the largest COMPLEMENT of one.
struct MatchInfo {
    uint32_t in_scope, nonfinite;          // source splats in scope; of those, with a non-finite position or transformed point
    uint32_t matched, surface;             // (surface: the non-zero rows of k_match_surface_rows, 0 for every other call)
    unsigned long long nd2min, d2max;
    unsigned long long pair_bound;         // k_match_bound's sum
};
// rows of every level of the tree over n >= 1 rows: ceil(n / 256), ceil of that / 256, .. down to 1; the return value is their sum
inline uint64_t match_tree_rows(uint32_t n)
{
    uint64_t total = 0, rows = n;
    do { rows = (rows + MATCH_GROUP - 1u) / MATCH_GROUP; total += rows; } while (rows > 1u);
    return total;
}
// info->in_scope, nonfinite, and pair_bound += for every query the populations of the 27 buckets the walk visits for it
void launch_match_bound(const NbIndex& ix, const MatchSource& src, MatchInfo* info, int cu_count, hipStream_t s);
// idx[i], d2[i] for every source splat: the match, (MATCH_NONE, +inf) without one, (MATCH_NONE, NaN) outside the scope;
// info->matched, nd2min, d2max.  indexed: the target index's entries as the host read them.
void launch_match(const NbIndex& ix, uint32_t indexed, const MatchSource& src, uint32_t* idx, double* d2, MatchInfo* info, int cu_count, hipStream_t s);
// the tree: level 1 rebuilds every row from idx[] and d2[] (the transformed point again, the target's position gathered; tn: the
// target's splats), every level reduces groups of MATCH_GROUP rows; partial: match_tree_rows(n) rows of MATCH_ROW doubles, the
// levels one behind the other; the result is the last row.  n >= 1.
void launch_match_tree(const MatchSource& src, const float* qx, const float* qy, const float* qz, uint32_t tn, const uint32_t* idx, const double* d2,
                       double* partial, hipStream_t s);
// The point-to-plane tree ("Point-to-plane registration"): level 1 rebuilds every row of MATCH_SURFACE_ROW
// doubles from idx[], d2[], the target's position and the target's stored f32 normal (3 tn floats, three NaNs where a splat has
// none), and adds the non-zero rows to info->surface; the further levels are the tree above at that width.  partial:
// match_tree_rows(n) rows of MATCH_SURFACE_ROW doubles; the result is the last row.  n >= 1.
constexpr uint32_t MATCH_SURFACE_ROW = 29;                  // J_a * J_b for a <= b (21), J_a * r (6), r * r, d2
void launch_match_surface_tree(const MatchSource& src, const float* qx, const float* qy, const float* qz, const float* normals, uint32_t tn, const uint32_t* idx,
                               const double* d2, double* partial, MatchInfo* info, hipStream_t s);
// scratch <- the source splats i < n in scope with lo <= sqrt(d2[i]) && (sqrt(d2[i]) < hi || open_hi): every word of it is stored
void launch_match_select(const double* d2, const AttrScope& sc, uint32_t n, double lo, double hi, bool open_hi, uint32_t* scratch, uint32_t nwords, hipStream_t s);

// Selection overlay (k_overlay.hip; DESIGN.md section 4, "Selection overlay"): the last frame's bin lists walked once more, the
// weight w = T * B of every fragment of a SELECTED splat summed per pixel (cover) and, with the splat's colour, turned into the
// frame with those splats tinted (overlay).  Reads the framebuffer, never writes it.
struct OverlayBuffers : FrameLists {
    const float4* shcol;         // this frame's evaluated SH colours (null without SH)
    const uint32_t* sel;         // the selection words (null: a scene never selected in, the empty selection)
    uint32_t* invalid;           // out: 1 when the pass refused the frame (nothing written), 0 otherwise
    const float4* fb;            // the frame's framebuffer, W x H
    float4* overlay;             // out, W x H
    float* cover;                // out, W x H
    uint32_t nwords;             // words `sel` holds
    float tint[3], mix;
};
// skip: entries that cannot reach a tile are left out (GSR_DEPTH_SKIP); trim: the walk ends behind the list's last selected entry
// (GSR_OVERLAY_TRIM); the same bits in all four forms
void launch_overlay(const OverlayBuffers& b, const BinGrid& g, const CamParams& cam, bool skip, bool trim, hipStream_t s);
// Selection outline (k_overlay.hip; DESIGN.md section 4, "Selection overlay"): the edge of { cover >= threshold } drawn into the
// overlay image behind launch_overlay, in place.  The domain is the grid's band columns inside the image, every row.
constexpr int OUTLINE_MAX_WIDTH = 16;                      // one neighbour word on each side of a 64-pixel word suffices
constexpr int OUTLINE_OUTER = 0, OUTLINE_INNER = 1;        // (gsr_outline_options.side)
struct OutlineArgs {
    const float* cover;          // W x H, read, never written
    float4* overlay;             // W x H: only edge pixels are read and rewritten
    unsigned long long* bits;    // H x outline_words(W) words of scratch: bit x & 63 of word (y, x >> 6) = pixel (x, y) is a source of the dilation
    const uint32_t* invalid;     // the overlay pass's word: non-zero = it refused the frame, nothing is drawn
    int32_t W, H, x_lo, x_hi;    // the image and the domain's columns [x_lo, x_hi), 0 <= x_lo <= x_hi <= W
    int32_t width, side;
    float rgb[3], alpha, threshold;
    uint8_t hw[OUTLINE_MAX_WIDTH + 1];   // hw[d] = floor(sqrt(width^2 - d^2)) for d <= width: the disc's half-width d rows from its centre
};
inline size_t outline_words(int32_t W) { return ((size_t)W + 63) / 64; }
void launch_outline(const OutlineArgs& a, hipStream_t s);

// multi-GPU exchange helpers (RGBA8 slabs of the all-gather)
constexpr int MAX_SLABS = 16;
struct SlabEdges { int32_t x0[MAX_SLABS], x1[MAX_SLABS]; };
// (the library's own slabs carry SLAB_FLAG_WORDS words behind their H x slab_w pixels: "this band was not composited")
constexpr int SLAB_FLAG_WORDS = 4;   // one flag, padded to 16 bytes
void launch_pack_band_rgba8(const float4* fb, uint32_t* slab, int W, int H, int x0, int x1, int slab_w, hipStream_t s, const uint32_t* overflow = nullptr);
void launch_unpack_slabs_rgba8(const uint32_t* gathered, uint32_t* image, int W, int H, int slab_w, int world,
                               const SlabEdges& e, hipStream_t s, uint32_t* stale = nullptr, size_t slab_stride = 0);
// Depth beside the colour (gsr_comm_set_depth; k_deliver.hip, beside the one statement of the 16-bit quantiser).  A slab's depth
// section: Hd rows of `stride` samples (a multiple of 8: every row starts on 16 bytes), f32 or u16, the band's samples
// [xd0, xd1) of the Wd x Hd hit plane at the front of every row and zeros behind them.
void launch_pack_band_depth(int format, const float* plane, uint8_t* section, int Wd, int Hd, int xd0, int xd1, int stride, float near, hipStream_t s);
// [world] slabs of slab_bytes, their depth sections at `offset` -> the gathered plane [Hd][Wd] in whole 16 bytes (the rest zero);
// `e`: the bands in samples
void launch_unpack_slabs_depth(int format, const uint8_t* gathered, uint32_t* plane, int Wd, int Hd, size_t slab_bytes, size_t offset, int stride,
                               int world, const SlabEdges& e, hipStream_t s);
// a gathered plane of `words` words as it is into a delivery slot's staging at `depth_offset`, and the slot's trailer ([0] the
// gathered frame's stale mask) at `trailer_offset`: launch_deliver_depth's kernel on words that are final already
void launch_deliver_gathered_depth(const uint32_t* plane, uint32_t words, uint8_t* staging, size_t depth_offset, size_t trailer_offset, int32_t W, int32_t H,
                                   uint64_t serial, const uint32_t* stale, hipStream_t s);

}  // namespace gsr
