// The host side of libgsplat_hip.so: the context behind the C ABI (include/gsplat_hip.h), shared by the gsr_*.cpp units.
// Host only; what the kernels and their launchers see is gsr_internal.h.
#pragma once
#include "../../include/gsplat_hip.h"
#include "gsr_internal.h"

#include <algorithm>
#include <cstddef>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

struct ncclComm;   // RCCL's communicator (ncclComm_t is a pointer to it); only gsr_comm.cpp knows more

// Everything below is internal to the library's host units and hidden: the library exports the C ABI and the launchers only.
#pragma GCC visibility push(hidden)

namespace gsr {

// records the message in the context (or, without one, for gsr_last_error(NULL)) and returns `code`
int fail(gsr_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(c, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return gsr::fail((c), GSR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// A device allocation and its one owner: freed when the owner goes, never copied.  Reads as the plain pointer.
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) { (void)hipFree(p); p = nullptr; } }
    // frees what it holds, then allocates `count` (at least one) elements
    int alloc(gsr_ctx* c, size_t count)
    {
        reset();
        if (!count) count = 1;
        HIP_TRY(c, hipMalloc((void**)&p, count * sizeof(T)));
        return GSR_OK;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

enum Stage { EV_BEGIN = 0, EV_PROJECT, EV_SORT, EV_BIN, EV_BLEND /* after k_blend */, EV_COMBINE /* after k_combine */, EV_COUNT };

struct FrameState {  // small per-frame device words; initialised once (k_begin_frame), then every frame STORES them -- only `overflow`
                     // is accumulated, and zeroed by k_project_key
    int32_t minmax[2];
    uint32_t overflow;
    uint32_t queue;   // compositor work-item counter
    uint64_t visible;
    uint64_t tile_entries;
    uint64_t report[12]; // written by k_bin_finalize for the host: running sums accum[0..4], this frame's bin entries, and [6..11] what the
                         // step saw and decided (gsr_debug_read_frame_figures): optical depth and raw optical mass sums of the frame slots,
                         // list entries, the longest list, long_from, and dense | heavy << 1 | by_size << 2 | fits << 3
    uint32_t digit_total[RADIX_LO_BINS + RADIX_HI_BINS];
    uint32_t sorted_count;  // entries of depth_index: n, or the band's survivors (SortBuffers::count)
    uint32_t seg_len;       // the frame's compositor segment length (k_bin_finalize -> k_blend)
    uint32_t n_items;       // and its number of work items (directly behind seg_len: k_blend reads both through one pointer)
    uint32_t spec;          // reserved (0)
};

// The environment's tuning and A/B knobs, read once when a context is created: the context keeps
// them for its whole life.  A member holds the parsed, clamped value; "unset" is the default written here.
struct Knobs {
    bool graphs = true;          // GSR_NO_GRAPH=1: individual launches, no HIP graph
    bool fuse_combine = true;    // GSR_FUSE_COMBINE=0: separate k_combine launch
    bool saturate = true;        // GSR_SATURATE=0: composite every entry (no skip of quadrants that can no longer change)
    int items_by_size = -1;      // GSR_ITEMS_BY_SIZE: 0 / 1; -1: by the kind of context (one frame at a time: heaviest first)
    int long_items = -1;         // GSR_LONG_ITEMS: 0 / 1 pin the work-item length policy; -1: where the frame's optical depth says so
    uint32_t long_tau = 0;       // GSR_LONG_TAU: the per-bin optical depth (true mass) from which a bin is one work item (0: the built-in rule)
    long bin_rounds = 0;         // GSR_BIN_ROUNDS: rounds of 2048 ranks per binning workgroup on large grids (0: by the scene's size)
    uint32_t bin_big = 2;        // GSR_BIN_BIG: large bin grids: k_bin_scatter_big (0: the 64-register kernel + k_bin_finalize; 1: 2048-rank rounds)
    int bin_two_level = -1;      // GSR_BIN_TWO_LEVEL: 0 / 1 force the one- / two-level binning; -1: by the bin grid
    bool rect_carry = true;      // GSR_RECT_CARRY=0: LSD sort order: the binning gathers the packed rectangles instead of the sort carrying them
    bool rect_carry_bucket = false;   // GSR_RECT_CARRY=2: carried in the bucket order too (measured: what k_bin_count saves, the two sort
                                      // kernels pay -- C3 sort 35.0 -> 41.8 us, binning 47.6 -> 41.3 us -- so not by default)
    int blend_sub = 0;           // GSR_BLEND_SUB: 1 / 2 compositor waves per 16x16 tile; 0: by the kind of context and the bin grid
    int sort_order = -1;         // GSR_SORT_ORDER=lsd|bucket: 0 / 1; -1: chosen per frame from the reported bucket size
    uint32_t timing_every = 1;   // GSR_TIMING_EVERY: every n-th frame carries the stage events (contexts with GSR_FLAG_TIMING)
    uint32_t cell_grid = 0;      // GSR_CELL_GRID: workgroups of the level-two binning kernels (0: by the device)
    uint32_t seg_target = 0;     // GSR_SEG_TARGET: full segments a frame is cut into at least (0: by the kind of context)
    uint32_t blend_grid = 0;     // GSR_BLEND_GRID: persistent compositor workgroups (0: by the device)
    uint32_t seg_len = 0;        // GSR_SEG_LEN: entries per compositor work item, a multiple of 256 (0: the built-in length)
    uint32_t sort_kpb = 0;       // GSR_SORT_KPB: keys per radix workgroup, 2048, 4096 or 8192 (0: by the scene's size)
    uint32_t front_waves = 0;    // GSR_FRONT_WAVES=8|16: waves per workgroup of the heavy front-end kernels (0: by the kind of context)
    bool depth_skip = true;      // GSR_DEPTH_SKIP=0: the depth pass visits every entry in every tile (no skip of entries that cannot reach a tile)
    bool overlay_trim = true;    // GSR_OVERLAY_TRIM=0: the overlay pass walks every list to its end (no stop behind the last selected entry)
    bool attr_hist_peel = false; // GSR_ATTR_HIST=peel: k_attr_hist peels the bin of each wave's first lane before the LDS atomics (the same counts; measured slower)
    uint32_t attr_hist_grid = 0; // GSR_ATTR_HIST_GRID: workgroups of k_attr_hist (0: by the device)
};

// The scene's per-splat arrays: everything the on-device build, the transforms and the compaction move together.
struct SceneArrays {
    DevBuf<float> px, py, pz;
    DevBuf<uint32_t> cov0, cov1, cov2, rgba;
    DevBuf<float4> rot, scl;   // rotations / scales, only for scenes built on the device from .splat rows
    // the one list of the arrays (view() beside it names them in SceneDev's order): f(a's array, b's, whether it is one of the
    // two that only scenes with rotations and scales have), until one returns non-zero
    template <class A, class B, class F>
    static int each(A& a, B& b, F f)
    {
        int r;
        if ((r = f(a.px, b.px, false)) || (r = f(a.py, b.py, false)) || (r = f(a.pz, b.pz, false)) || (r = f(a.cov0, b.cov0, false)) ||
            (r = f(a.cov1, b.cov1, false)) || (r = f(a.cov2, b.cov2, false)) || (r = f(a.rgba, b.rgba, false)) ||
            (r = f(a.rot, b.rot, true)) || (r = f(a.scl, b.scl, true)))
            return r;
        return GSR_OK;
    }
    int alloc(gsr_ctx* c, size_t n, bool with_rows)
    {
        return each(*this, *this, [&](auto& buf, auto&, bool rows_only) -> int {
            if (rows_only && !with_rows) { buf.reset(); return GSR_OK; }
            return buf.alloc(c, n);
        });
    }
    // the first n rows of every array into dst's, device to device on `s` (both sets with rotations and scales)
    int copy_rows(gsr_ctx* c, SceneArrays& dst, size_t n, hipStream_t s) const
    {
        return each(*this, dst, [&](const auto& from, auto& to, bool) -> int {
            HIP_TRY(c, hipMemcpyAsync(to, from, n * sizeof(*from.p), hipMemcpyDeviceToDevice, s));
            return GSR_OK;
        });
    }
    // bytes of one row over the arrays that are allocated
    size_t row_bytes() const
    {
        size_t t = 0;
        each(*this, *this, [&](const auto& buf, const auto&, bool) -> int { if (buf) t += sizeof(*buf.p); return GSR_OK; });
        return t;
    }
    SceneDev view() const { return SceneDev{px, py, pz, cov0, cov1, cov2, rgba, rot, scl}; }
};

// A set of splats, one bit per splat of a scene: bit i & 31 of word i >> 5, bits at and above the scene's count always 0
// (k_splat_ops.h has the device's side of the layout).  The selection and the hidden set are one each; the functions that size,
// allocate, fold, read back and regrow them are declared below (set_*, gsr_select.cpp).
struct SplatSet {
    DevBuf<uint32_t> mask, scratch;   // `words` words each: the set, and the picked / folded set of the call in progress
    DevBuf<uint32_t> counters;        // [0] the bits set after the last fold, [1] a picker's `invalid` word, [2..] per-workgroup sums
    uint32_t words = 0;               // words the word buffers were allocated for (even, >= ceil(n / 32))
    uint32_t counter_words = 0;
    uint32_t count = 0;               // bits set: every call is blocking and returns with it final
    void reset() { mask.reset(); scratch.reset(); counters.reset(); words = counter_words = 0; count = 0; }
    uint64_t bytes() const { return (uint64_t)words * 8 + (uint64_t)counter_words * 4; }
};
// The sizes, each stated once.  words_of: the words that hold n splats' bits.  fold_words: the words a set is allocated with and a
// fold runs over for `rows` splats (even, as the box picker's ballots store whole pairs; the count only shrinks under a set, so
// one allocated for more holds these).  counter_words: the counters of a set of that many words.  op_ok: the ops a caller may name.
inline uint32_t words_of(uint32_t n) { return (n + 31u) / 32u; }
inline uint32_t fold_words(uint32_t rows) { return std::max((words_of(rows) + 1u) & ~1u, 2u); }
inline uint32_t counter_words(uint32_t words) { return 2u + (words + SELECT_APPLY_THREADS - 1u) / SELECT_APPLY_THREADS; }
inline bool op_ok(int32_t op) { return op >= GSR_SELOP_REPLACE && op <= GSR_SELOP_INTERSECT; }

// The scene state its members hold once (DESIGN.md section 2, and section 4 "Shared scenes"): the per-splat arrays, the SH textures and their spare set, the SH
// frame and the splat count.  It owns these buffers; the contexts that render it are listed in `members` (no leader: the last one
// to go frees it).  Everything a frame writes, `shcol` included, stays with the context.
struct SharedScene {
    SceneArrays arr;
    uint32_t n = 0;                   // splats of the scene
    uint32_t arr_rows = 0;            // rows the arrays were allocated for (gsr_scene_limit_box lowers n, not this)
    bool have_rows = false;
    bool given = false;               // a gsr_set_scene* call has supplied a scene (of any count, 0 included)
    std::vector<gsr_ctx*> members;
    // moves whenever the arrays, the count or the SH textures are replaced: a member whose scene_gen differs re-sizes its per-splat
    // buffers where its next frame is enqueued (adopt_scene)
    uint64_t generation = 1;
    // spherical harmonics (optional)
    DevBuf<uint32_t> sh_r, sh_g, sh_b;
    uint32_t sh_count = 0;
    int32_t band[3] = {-1, -1, -1};
    // (hidden: the mask only while a bit is set -- with nothing hidden the projection is handed null and the frame path is the one
    // of a scene that never hid, buffers allocated or not)
    SceneSoA soa(float4* shcol) const
    {
        return SceneSoA{arr.px, arr.py, arr.pz, arr.cov0, arr.cov1, arr.cov2, arr.rgba, sh_r, sh_g, sh_b, shcol, hid.count ? hid.mask.p : nullptr};
    }
    // The SH frame: the inverse of the linear part of every rotate / scale since the coefficients were
    // supplied, row-major; the projection takes SH directions through it.  Kept up by gsr_scene_rotate / _scale while sh_follow
    // is set; the identity takes the projection's frameless path.
    bool sh_follow = false;
    // the other set of SH textures a followed gsr_scene_limit_box compacts into (then the two sets change places): allocated by
    // the first such call, kept until the SH state goes; sh_rows / sh_spare_rows: the rows each set was allocated for
    DevBuf<uint32_t> sh_spare[3];
    uint32_t sh_rows = 0, sh_spare_rows = 0;
    double sh_frame[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    void reset_sh_frame() { for (int k = 0; k < 9; k++) sh_frame[k] = (k % 4 == 0) ? 1.0 : 0.0; }
    bool sh_frame_is_identity() const
    {
        for (int k = 0; k < 9; k++) if (sh_frame[k] != ((k % 4 == 0) ? 1.0 : 0.0)) return false;
        return true;
    }
    // (the members' evaluated colours, shcol, go with it: the caller resets its own, the other members' go in adopt_scene)
    void drop_sh() { sh_count = 0; band[0] = band[1] = band[2] = -1; sh_r.reset(); sh_g.reset(); sh_b.reset(); reset_sh_frame();
                     for (auto& b : sh_spare) b.reset();
                     sh_rows = sh_spare_rows = 0; }
    // The selection (gsr_select.cpp; DESIGN.md section 4, "Selection"): one bit per splat of THIS copy, so the members have one
    // together.  Nothing is allocated until the first call that selects; a scene without buffers reads as all zeros.
    struct Selection : SplatSet {
        DevBuf<uint8_t> region;           // the region bytes of gsr_select_region: grows on demand
        size_t region_bytes = 0;
        void reset() { SplatSet::reset(); region.reset(); region_bytes = 0; }
        uint64_t bytes() const { return SplatSet::bytes() + region_bytes; }
    } sel;
    // The hidden set (gsr_hidden.cpp; DESIGN.md section 4, "Hidden splats"): one bit per splat of THIS copy, so the members have
    // one together.  A hidden splat fails the projection's culls (k_project_key reads `mask` while count != 0).  Nothing is
    // allocated until the first call that hides; a scene without buffers reads as all zeros.  Unlike the selection it survives
    // a compaction: scene_compact carries it into `spare` (k_box_compact_bits), then the two change places.
    struct Hidden : SplatSet {
        DevBuf<uint32_t> spare;           // `words` words: the other buffer of a compaction
        void reset() { SplatSet::reset(); spare.reset(); }
        uint64_t bytes() const { return SplatSet::bytes() + (uint64_t)words * 4; }
    } hid;
    // Moves with every call that changes the selection's bits (the folds of gsr_select.cpp) or drops them (a new scene, a compaction):
    // a member's overlay image (gsr_overlay.cpp) is the selection's while the version it was enqueued for is this one.
    uint64_t sel_version = 1;
    // The contribution accumulators (gsr_contrib.cpp; DESIGN.md section 4, "Contribution"): per splat of THIS copy, so the members
    // have one set together and their passes add into it with atomics that commute.  Nothing is allocated until the first reset or
    // pass; without buffers the state is "never reset".  Dropped wherever the selection is emptied: the indices are the old numbering's.
    struct Contrib {
        DevBuf<unsigned long long> weight;   // `rows` each: sum of rintf(w * 2^24),
        DevBuf<uint32_t> peak, pixels;       // max of w (bits of a non-negative f32), fragments modulo 2^32
        DevBuf<uint32_t> counters;           // [0] frames: the passes that contributed since the last reset; [1] reserved (0)
        uint32_t rows = 0;                   // splats the accumulators describe (the scene's count at the reset, or since it grew)
        uint32_t alloc_rows = 0;             // rows the arrays were allocated for: `rows`, or more where the scene's capacity was
                                             // reserved (gsr_append.cpp); the rows at and above `rows` are zero
        static constexpr uint32_t COUNTER_WORDS = 2;
        bool live() const { return (bool)counters.p; }
        void reset() { weight.reset(); peak.reset(); pixels.reset(); counters.reset(); rows = alloc_rows = 0; }
        uint64_t bytes() const { return live() ? (uint64_t)alloc_rows * 16 + COUNTER_WORDS * 4 : 0; }
    } contrib;
    // device bytes of the state the members hold once
    uint64_t bytes() const
    {
        return (uint64_t)arr_rows * arr.row_bytes() + ((uint64_t)sh_rows + sh_spare_rows) * 3 * 32 + sel.bytes() + contrib.bytes() + hid.bytes();
    }
};

// k_project_key's arguments but the splat count and the camera (ProjectLaunch without what changes from frame to frame)
struct ProjectArgs {
    SceneSoA sc;
    int32_t* depth; int32_t* slots; Record* rec; uint32_t* rect; uint32_t* overflow; uint32_t* kept; uint8_t* kept_lane;
};

// Everything a frame's launches are handed, except the camera: build_frame_args derives it from the context, enqueue_chain
// launches from it and from nothing else, and a captured graph is replayed exactly while the next frame's FrameArgs equal,
// byte for byte, the ones it was captured from.  Trivially copyable; filled by name into zeroed storage and copied with
// memcpy, so that the comparison never depends on a padding byte.
struct FrameArgs {
    ProjectArgs proj;        // render frames
    int32_t* slots_next;     // sort-only frames: the slot set k_depth_key resets for the next one
    SortBuffers sort;
    BinBuffers bin;
    BinGrid grid;
    BlendBuffers blend;
    float early_out_eps;
    uint32_t n;
    bool render;             // false: a sort-only frame (depth key + sort)
};
static_assert(std::is_trivially_copyable<FrameArgs>::value, "FrameArgs is compared and copied as bytes");

// What a depth plane that leaves the pass's own buffers holds -- a depth ring's (gsr_delivery_open_depth), a group's exchanged one
// (gsr_comm_set_depth): the sample format, every step-th pixel in both directions and, for U16, the near plane.
struct DepthSpec {
    int format = GSR_DEPTH_NONE;   // GSR_DEPTH_*; NONE: no depth plane
    int step = 1;                  // 1 or 2: sample (i, j) is pixel (step * i, step * j)
    float near = 0.0f;             // GSR_DEPTH_U16; 0 otherwise
    // of options depth_options_check has accepted; NULL or GSR_DEPTH_NONE: off, whatever else the struct holds
    static DepthSpec from(const gsr_depth_delivery_options* o)
    {
        if (!o || o->format == GSR_DEPTH_NONE) return {};
        return {o->format, o->step, o->format == GSR_DEPTH_U16 ? o->near : 0.0f};
    }
    bool on() const { return format != GSR_DEPTH_NONE; }
    size_t sample_bytes() const { return format == GSR_DEPTH_U16 ? 2 : 4; }
    bool operator==(const DepthSpec& o) const { return format == o.format && step == o.step && near == o.near; }
    // a plane of Wd x Hd samples, rows packed; the layout of one that lies `offset` bytes into what the caller reads
    size_t plane_bytes(int Wd, int Hd) const { return (size_t)Wd * Hd * sample_bytes(); }
    gsr_depth_layout layout(int Wd, int Hd, uint64_t offset) const
    {
        gsr_depth_layout l{};
        l.format = format; l.step = step; l.width = Wd; l.height = Hd;
        l.stride = (int32_t)plane_bytes(Wd, 1);
        l.offset = offset;
        l.bytes = plane_bytes(Wd, Hd);
        l.near = near;
        return l;
    }
};

// What one user of the depth pass (k_depth.hip) has it write: the context's planes (gsr_depth_async / gsr_read_depth), a depth ring's,
// a group's depth exchange.  Each user has a set of its own, so none disturbs what another reads; gsr_depth.cpp's depth_enqueue fills any.
struct DepthPlanes {
    DevBuf<float> hit;             // Wd x Hd
    DevBuf<float> mean;            // step 1 only (k_depth_planes<.., 1> writes all three planes); scratch for every user but the context
    DevBuf<uint32_t> index;
    DevBuf<uint32_t> invalid;      // one word, stored by every pass: 1 = it refused a frame whose lists did not fit and wrote nothing
    int Wd = 0, Hd = 0;            // ceil(W / step), ceil(H / step): the extent in use, not the capacity (the context's planes only grow
                                   // and hold a smaller image at their front; a ring's and the exchange's are allocated for exactly this)
    int fill_key[4] = {0, 0, 0, 0};   // band contexts: W, H and bin columns the columns outside the band were last filled for
    int alloc(gsr_ctx* c, int W, int H, int step)
    {
        reset();
        Wd = (W + step - 1) / step; Hd = (H + step - 1) / step;
        const size_t np = (size_t)Wd * Hd;
        int r = hit.alloc(c, np);
        if (!r && step == 1) { r = mean.alloc(c, np); if (!r) r = index.alloc(c, np); }
        if (!r) r = invalid.alloc(c, 1);
        if (r) reset();
        return r;
    }
    void reset() { hit.reset(); mean.reset(); index.reset(); invalid.reset(); Wd = Hd = 0; std::fill(fill_key, fill_key + 4, 0); }
};
// what a user of the pass has in the columns outside a band context's bins, which the pass does not write
enum DepthFill { DEPTH_FILL_NOTHING, DEPTH_FILL_HIT /* hit: +inf */, DEPTH_FILL_PLANES /* mean, hit, index: 0, +inf, none */ };

}  // namespace gsr

struct gsr_ctx {
    int device = 0;
    int cu_count = 256;               // compute units of the device (the compositor's persistent grid is sized from it)
    hipStream_t stream = nullptr;
    std::string error;
    gsr_options opt{};
    gsr::Knobs knobs;
    int W = 0, H = 0;
    int band_x0 = 0, band_x1 = 0;
    gsr::CamParams cam{};
    gsr::CamParams cam_frame{};       // the camera of the last rendered frame
    bool have_cam = false, have_frame = false, have_sort = false;
    uint64_t frame_serial = 0;        // render frames enqueued so far (the depth pass remembers which one its planes belong to)
    bool frame_lists = false;         // the last render frame's bin lists are still what the bin buffers hold (alloc_bins drops it)
    hipEvent_t link_ev[2] = {nullptr, nullptr};  // gsr_stream_order

    // The scene the context renders (gsr_scene.cpp): never null.  A context is the only member of its scene until gsr_share_scene
    // makes it a member of another context's; `scene_gen` is the scene's generation this context's per-splat buffers were last sized for.
    gsr::SharedScene* scene = nullptr;
    uint64_t scene_gen = 0;
    gsr::DevBuf<float4> shcol;        // the SH colours the projection evaluates for this context's camera (one per splat, while the scene has SH)
    hipEvent_t share_ev = nullptr;    // orders this context's stream against the other members' around an edit (created by the first share)
    gsr::SceneSoA scene_soa() const { return scene->soa(shcol); }

    struct Sort {    // per splat and frame: what the projection writes and the sort permutes; sized by alloc_scene
        gsr::DevBuf<int32_t> depth;
        gsr::DevBuf<uint32_t> kept;        // band mode: survivors per 256-splat workgroup of k_project_key, packed to the front of its depth slots
        gsr::DevBuf<uint8_t> kept_lane;    // band mode: the lane a packed slot's splat came from
        gsr::DevBuf<uint32_t> koff;        // band mode: survivors in front of every workgroup's block (k_kept_scan)
        gsr::DevBuf<uint32_t> keys, keys_tmp, idx_tmp, depth_index, block_hist;
        gsr::DevBuf<gsr::Record> rec;
        gsr::DevBuf<uint32_t> rect_idx;    // per splat: packed bin rectangle (k_project_key); rects holds them in depth order
        gsr::DevBuf<uint32_t> rects;
        gsr::DevBuf<uint32_t> rect_tmp;    // the rectangles between the sort's two passes, where they are carried (SortPlan::carry)
        gsr::DevBuf<uint32_t> chunk_tab;   // bucket order: k_local_sort's work list
        uint32_t rows = 0;                 // splats the buffers above were allocated for
        int parity = 0;                    // which of the two sort-only slot sets the next sort-only frame uses
        gsr::SortPlan plan{};              // what the last enqueued frame's sort was launched from (plan_sort; valid while have_sort);
                                           // plan.band: it kept only the band's survivors (depth_index / keys are partial)
    } sort;

    struct Bin {     // bin lists and compositor work items; sized by alloc_bins (gsr_frame.cpp)
        gsr::DevBuf<uint32_t> table, total, start, start_pre, list;
        gsr::DevBuf<uint32_t> cell_list, cell_total, cell_start, chunk_start, chunk_info, cell_table2, cell_wcnt;
        gsr::DevBuf<uint32_t> seg_start, items;
        gsr::DevBuf<unsigned long long> mask;   // per-bin arrival masks of the compositor (blend.fused; null otherwise)
        gsr::DevBuf<float4> partial;
        gsr::BinPlan plan{};               // the binning's form and launch shapes for the context as it stands (plan_bins)
        gsr::BlendPlan blend{};            // the compositor's kernel, grid and work-item policy for the same (plan_blend);
                                           // blend.max_items: what `items` was allocated for
        uint32_t cell_capacity_alloc = 0, cell_ncells_alloc = 0;
        uint32_t capacity = 0, table_elems = 0, nbins_alloc = 0;
    } bin;

    struct Words {   // the small device words every frame shares, and what the host knows of them
        gsr::DevBuf<gsr::FrameState> fstate;
        gsr::FrameState* fstate_host = nullptr;  // pinned
        gsr::DevBuf<int32_t> slots;         // 3 x FRAME_SLOTS x 128 B: partial depth (min, max), visible and tile sums of k_project_key
                                            // (the render frames' set, then the two of the sort-only frames)
        bool slots_need_init = true;        // frame words and the three slot sets: initialised once, by the first frame's enqueue
        gsr::DevBuf<gsr::CamParams> cam_dev;  // a camera slot in device memory (written by the one-time initialisation only)
        gsr::DevBuf<uint64_t> accum;        // [8]: sums over frames (visible, bin entries, tile entries, frames), [4] entries of
                                            // the last frame, sticky [5] frames that did not fit, [6]/[7] most entries/items one needed
        uint64_t* mailbox = nullptr;        // pinned host words the device stores into: [0] accum[5] (k_bin_finalize), [1] low half: keys in the
                                            // largest high-digit bucket of the last sorted frame (k_local_sort / last LSD pass)
        uint64_t* mailbox_dev = nullptr;    // its device address
        uint64_t overflow_seen = 0;         // accum[5] as of the last regrowth
        uint64_t overflow_frames = 0;       // frames that did not fit, since the context was created
        uint64_t dropped_frames = 0;        // of those, frames never composited (later frames had been enqueued before the host noticed)
        uint64_t dropped_unreported = 0;    // dropped frames gsr_sync has not reported yet
    } words;

    struct Out {
        gsr::DevBuf<float4> fb;
        gsr::DevBuf<uint32_t> fb8;
        size_t pixels = 0;
    } out;

    // the frame's launch chain replayed as a HIP graph (frames that carry no stage events)
    struct Graph {
        bool enabled = true;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipGraphNode_t project = nullptr;   // the captured chain's projection node: its camera argument is rewritten every replay
        gsr::FrameArgs key;                 // what `exec` was captured from (valid while exec is set)
    } graph;
    gsr::ProjectLaunch proj{};              // the projection kernel's arguments of the current frame

    // timing: a ring of event sets so that frames can be enqueued back to back without a host
    // sync per frame; gsr_sync / gsr_get_timings drain the ring
    struct Timing {
        static constexpr int EV_RING = 128;
        hipEvent_t evring[EV_RING][gsr::EV_COUNT]{};
        bool is_render[EV_RING]{};
        int head = 0, pending = 0;
        hipEvent_t* ev = nullptr;  // the set being recorded
        bool valid = false, recorded = false, render = false;
        uint32_t every = 1, frame_no = 0;
        gsr_timings tm{};
    } timing;

    // multi-GPU exchange (gsr_comm_init): RCCL communicator, its stream, the RGBA8 slab / gathered slabs / full frame
    struct Comm {
        ncclComm* nccl = nullptr;
        gsr_allgather_fn fn = nullptr;    // gsr_comm_init_custom: the caller's collective in place of ncclAllGather
        void* fn_user = nullptr;
        bool owned = true;                // false: communicator and exchange stream belong to another context (gsr_comm_share)
        gsr_ctx* leader = nullptr;        // that context; it lists this one in followers and detaches it when it leaves the group first
        std::vector<gsr_ctx*> followers;
        int rank = 0, world = 0, slab_w = 0;
        hipStream_t stream = nullptr;
        hipEvent_t ev_packed = nullptr, ev_slab_free = nullptr;
        gsr::DevBuf<uint32_t> slab, gathered, frame8;
        gsr::SlabEdges edges{};
        bool frame8_valid = false;
        bool joined() const { return nccl || fn; }
        // depth beside the colour (gsr_comm_set_depth): the band's hit samples travel in a depth section behind the slab's pixels and
        // flag words, and one de-slab step leaves the gathered plane on every rank.  Nothing below is allocated, and the slab is
        // the colour slab byte for byte, until a context opts in.
        struct DepthExchange {
            gsr::DepthSpec spec;            // off: colour only
            gsr::DepthPlanes planes;        // the pass writes this rank's columns of hit, the band pack reads them (`invalid` is never read: the slab's flag decides)
            int W = 0, H = 0;               // the size the buffers and the layout were made for
            int stride = 0;                 // samples per row of a slab's depth section: the widest band's, rounded up to 8
            size_t offset = 0;              // of the section in a slab: behind pixels and flag words, at the next multiple of 16
            size_t slab_bytes = 0;          // offset + Hd * stride * sample size: what one rank hands to the collective
            gsr::SlabEdges edges{};         // the bands in samples: [x0 / step, ceil(x1 / step))
            gsr::DevBuf<uint32_t> plane;    // the gathered plane [Hd][Wd], f32 or u16, in whole 16 bytes (the rest zero)
            bool on() const { return spec.on(); }
            size_t plane_bytes() const { return spec.plane_bytes(planes.Wd, planes.Hd); }
            void reset() { spec = {}; planes.reset(); plane.reset(); W = H = stride = 0; offset = slab_bytes = 0; }
        } depth;
        // what one rank hands to the collective
        size_t slab_bytes(int H) const { return depth.on() ? depth.slab_bytes : ((size_t)slab_w * H + gsr::SLAB_FLAG_WORDS) * 4; }
    } comm;

    // depth planes and picking (gsr_depth.cpp); nothing is allocated until the first call that needs it
    struct Depth {
        gsr::DepthPlanes planes;            // what gsr_read_depth returns: W x H of the last pass in front of `pixels` allocated (they only grow)
        size_t pixels = 0;
        gsr::DevBuf<int32_t> query;         // gsr_pick: MAX_PICKS (x, y) pairs
        gsr::DevBuf<gsr::PickResult> result;
        gsr::DevBuf<uint32_t> pick_invalid; // the pick pass's word, as planes.invalid is the planes pass's
        float hit_alpha = 0.5f;
        uint64_t planes_serial = 0;         // frame_serial of the frame the planes were enqueued behind (0: none, or hit_alpha changed)
    } depth;

    // selection overlay (gsr_overlay.cpp); nothing is allocated until gsr_set_overlay supplies options
    struct Overlay {
        bool on = false;                    // options are set
        float tint[3] = {0.0f, 0.0f, 0.0f}, mix = 0.0f;
        gsr::DevBuf<float4> image;          // W x H in front of `pixels` allocated (they only grow): the frame with the selected splats tinted
        gsr::DevBuf<float> cover;           // likewise: the selected splats' share of the pixel's alpha
        gsr::DevBuf<uint32_t> image8;       // gsr_read_overlay_rgba8's conversion of `image`, allocated by its first call
        gsr::DevBuf<uint32_t> invalid;      // one word, stored by every pass: 1 = it refused a frame whose lists did not fit and wrote nothing
        size_t pixels = 0;
        // what the image was enqueued for: the frame (frame_serial; 0: nothing), the scene's sel_version, the options (a count of the
        // gsr_set_overlay calls that changed them)
        uint64_t serial = 0, sel_version = 0, opt_version = 0, image_opt_version = 0;
        bool in_flight = false;             // a pass has been enqueued since the last gsr_sync: calls that change the mask wait for this stream first
        // the selection's outline (gsr_set_overlay_outline): drawn into `image` behind the pass; off, nothing is allocated or launched
        struct Outline {
            bool on = false;
            float rgb[3] = {0.0f, 0.0f, 0.0f}, alpha = 0.0f, threshold = 0.0f;
            int32_t width = 0, side = 0;
            gsr::DevBuf<unsigned long long> bits;   // the bit plane of k_outline_bits, H x outline_words(W) in front of `words` allocated (they only grow)
            size_t words = 0;
            void reset() { on = false; bits.reset(); words = 0; }
        } outline;
        void reset() { on = false; image.reset(); cover.reset(); image8.reset(); invalid.reset(); pixels = 0; serial = 0; outline.reset(); }
    } overlay;

    // splat data (gsr_attr.cpp): the device words of gsr_attr_stats / gsr_attr_histogram, the context's own; nothing is allocated
    // until the first such call
    struct Attr {
        gsr::DevBuf<uint32_t> words;        // ATTR_HIST_WORDS histogram counters, then ATTR_MAX_GRID + 1 AttrStats (the partials, the result)
    } attr;

    // neighbours (gsr_neighbours.cpp): the device scratch of gsr_neighbours / gsr_select_neighbours, the context's own; the first
    // call allocates it, it only grows, and the context's end frees it
    struct Neighbours {
        gsr::DevBuf<uint32_t> words;            // NB_INFO_WORDS of NbInfo, then NB_MAX_CAP + 1 histogram counters
        gsr::DevBuf<uint32_t> table;            // 2 words per bucket
        uint64_t buckets = 0;                   // buckets `table` was allocated for
        gsr::DevBuf<uint4> entry;               // `rows` each: the index's entries, their cell keys, the counts by splat
        gsr::DevBuf<unsigned long long> key;
        gsr::DevBuf<uint32_t> counts;
        uint32_t rows = 0;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // in front of the build, behind the bound, behind the count
        float build_ms = 0.0f, count_ms = 0.0f;           // of the last call that ran both (gsr_debug_neighbour_times)
    } nb;

    // clusters (gsr_clusters.cpp): what gsr_clusters / gsr_select_clusters / gsr_select_cluster_at hold beside the neighbour scratch,
    // the context's own; the first cluster call allocates it, it only grows, and the context's end frees it
    struct Clusters {
        gsr::DevBuf<uint32_t> words;            // CL_INFO_WORDS of ClInfo
        gsr::DevBuf<uint32_t> label;            // `rows` each: parent[] of the union, every splat's label after it; size[] by label;
        gsr::DevBuf<uint32_t> size;             // every splat's cluster size
        gsr::DevBuf<uint32_t> sizes;
        uint32_t rows = 0;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // behind the core test, behind union and flatten, behind border and sizes
        float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};           // index, core, union + flatten, border + sizes of the last call (gsr_debug_cluster_times)
    } cl;

    // k nearest neighbours (gsr_knn.cpp): what gsr_knn / gsr_select_knn hold beside the neighbour scratch, the context's own; the
    // first such call allocates it, it only grows, and the context's end frees it
    struct Knn {
        gsr::DevBuf<uint32_t> words;            // KNN_INFO_WORDS of KnnInfo
        gsr::DevBuf<uint32_t> found;            // `rows` each: the lists' lengths and the values by splat
        gsr::DevBuf<double> values;
        uint32_t rows = 0;
        gsr::DevBuf<uint32_t> idx;              // `slots` each (rows * k of the calls that asked for lists): indices and squared distances
        gsr::DevBuf<double> d2;
        uint64_t slots = 0;
        hipEvent_t ev = nullptr;                // behind the walk
        float ms[2] = {0.0f, 0.0f};             // index with its bound, fill and walk of the last call (gsr_debug_knn_times)
    } knn;

    // normals (gsr_normals.cpp): what gsr_normals / gsr_select_normal hold beside the neighbour scratch, the context's own; the
    // first such call allocates it, it only grows, and the context's end frees it
    struct Normals {
        gsr::DevBuf<uint32_t> words;            // NORMAL_INFO_WORDS of NormalInfo
        gsr::DevBuf<float> normals;             // 3 * `rows`
        gsr::DevBuf<double> variation;          // `rows` each: the variation and the lists' lengths by splat
        gsr::DevBuf<uint32_t> found;
        uint32_t rows = 0;
        hipEvent_t ev[2] = {nullptr, nullptr};  // in front of the OWN kernel; behind the walk or the OWN kernel
        float ms[2] = {0.0f, 0.0f};             // index with its bound (0 for OWN), fill and walk of the last call (gsr_debug_normals_times)
    } nm;

    // merging cells (gsr_merge.cpp): what gsr_cells / gsr_scene_merge_cells hold beside the neighbour scratch, the context's own; the
    // first such call allocates it, it only grows, and the context's end frees it
    struct Merge {
        gsr::DevBuf<uint32_t> words;            // MG_INFO_WORDS of MgInfo
        gsr::DevBuf<uint32_t> cand;             // `mask_words` words: the candidate mask
        gsr::DevBuf<uint32_t> leader, count, rank;   // `rows` each
        uint32_t rows = 0, mask_words = 0;
        // the edit only
        gsr::DevBuf<uint32_t> slice, member;    // `edit_rows` each
        gsr::DevBuf<uint2> cells;               // edit_rows / 2 + 1
        gsr::DevBuf<uint32_t> remove, merged, carried;   // `edit_words` words each: the compaction's predicate, the merged rows before and after it
        uint32_t edit_rows = 0, edit_words = 0;
    } mg;

    // planes (gsr_plane.cpp): the device scratch of gsr_fit_plane / gsr_plane_inliers, the context's own; the first such call
    // allocates it, it only grows, and the context's end frees it
    struct Plane {
        gsr::DevBuf<uint32_t> words;            // PL_INFO_WORDS: the totals, then PlBest
        gsr::DevBuf<uint32_t> cand, block;      // `rows` candidates; plane_blocks(rows) + 1 block sums
        uint32_t rows = 0;
        gsr::DevBuf<double4> planes;            // PLANE_MAX_HYPOTHESES each
        gsr::DevBuf<uint4> triple;
        gsr::DevBuf<uint32_t> scores;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // in front of the candidates, behind them, behind the scores
        float candidates_ms = 0.0f, score_ms = 0.0f;      // of the last call that ran both (gsr_debug_plane_times)
    } pl;

    // matching and registration (gsr_match.cpp): what gsr_match / gsr_select_match / gsr_register hold beside the neighbour scratch
    // (which they size for the TARGET's count), the context's own; the first such call allocates it, it only grows, and the
    // context's end frees it
    struct Match {
        gsr::DevBuf<uint32_t> words;            // MATCH_INFO_WORDS of MatchInfo
        gsr::DevBuf<uint32_t> idx;              // `rows` each: the match and its squared distance by source splat
        gsr::DevBuf<double> d2;
        uint32_t rows = 0;
        gsr::DevBuf<double> tree;               // `tree_rows` rows of MATCH_ROW doubles: the partial rows of every level (calls that ask for sums)
        uint64_t tree_rows = 0;
        gsr::DevBuf<double> surface_tree;       // `surface_rows` rows of MATCH_SURFACE_ROW doubles: the same for gsr_match_surface / gsr_register_surface
        uint64_t surface_rows = 0;
        hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // around the index; in front of a step's bound, behind it, behind the walk, the tree
        float ms[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // of the last call: the index; bound, walk, tree of its last step; their sums over
                                                                          // its steps; the steps (gsr_debug_match_times)
    } mt;

    // frame delivery (gsr_delivery_open): a ring of pinned host blocks, each with its device staging and "copy done" event
    struct Delivery {
        struct Slot {
            uint8_t* host = nullptr;        // hipHostMalloc: the format's payload (RGBA8: W * H * 4 bytes) rounded up to whole words + the trailer
            gsr::DevBuf<uint32_t> staging;  // device, same size: k_deliver_rgba8 / k_deliver_yuv writes it, the copy reads it
            hipEvent_t done = nullptr;      // recorded behind the slot's copy
            uint64_t serial = 0;
            enum State { FREE, IN_FLIGHT, HELD } state = FREE;
        };
        std::vector<Slot> ring;
        hipStream_t copy_stream = nullptr;
        hipEvent_t ev_staged = nullptr;     // render stream -> copy stream: the conversion kernel has written the staging buffer
        int W = 0, H = 0;
        int format = GSR_FORMAT_RGBA8;      // what the ring was opened for (gsr_delivery_open_ex); gsr_resize keeps it
        gsr::YuvParams yuv{};               // NV12 / I420: the coefficient set and the background
        int next = 0;                       // where the search for a free slot starts: the slots are used in turn
        uint64_t serial = 0;                // the last serial handed out; never restarts
        // a depth ring (gsr_delivery_open_depth): every delivered frame carries its hit plane behind the colour payload.  Nothing of
        // gsr_ctx::Depth but hit_alpha is read, nothing of it written.
        struct DepthPlane {
            gsr::DepthSpec spec;            // off: a ring as it was before depth rings existed, nothing below is allocated
            gsr::DepthPlanes planes;        // allocated with the ring: the pass writes hit, k_deliver_depth reads it; reused by every delivery (in-order on the render stream)
        } depth;
        bool overlay = false;               // gsr_delivery_set_overlay: the conversion reads the overlay image in place of the framebuffer
        // a slot's layout: the frame's payload in the ring's format; in a depth ring the plane behind it at the next multiple of 16; the
        // trailer behind the plane at the next multiple of 16 (without depth: behind the payload at the next whole word)
        size_t pixel_bytes() const { return format == GSR_FORMAT_RGBA8 ? (size_t)W * H * 4 : gsr::yuv420_bytes(W, H); }
        size_t depth_offset() const { return (pixel_bytes() + 15) & ~(size_t)15; }
        size_t depth_bytes() const { return depth.spec.plane_bytes(depth.planes.Wd, depth.planes.Hd); }
        size_t trailer_offset() const { return depth.spec.on() ? (depth_offset() + depth_bytes() + 15) & ~(size_t)15 : (pixel_bytes() + 3) & ~(size_t)3; }
        size_t slot_bytes() const { return trailer_offset() + gsr::DELIVER_TRAILER_WORDS * 4; }
    } delivery;
};

namespace gsr {

inline BinGrid make_grid(const gsr_ctx* c)
{
    BinGrid g;
    g.W = c->W; g.H = c->H;
    g.nbx = (c->W + BIN_PX - 1) / BIN_PX;
    g.nby = (c->H + BIN_PX - 1) / BIN_PX;
    if (c->band_x1 > c->band_x0) {
        g.bx_lo = c->band_x0 / BIN_PX;
        g.bx_hi = std::min((c->band_x1 + BIN_PX - 1) / BIN_PX, g.nbx);
    } else {
        g.bx_lo = 0; g.bx_hi = g.nbx;
    }
    return g;
}

// waves per workgroup of the heavy front-end kernels: throughput contexts run beside other frames' compositors, so their
// front-end workgroups are narrow and fit what a few retired compositor workgroups leave free on a CU
inline uint32_t front_waves_of(const gsr_ctx* c)
{
    return c->knobs.front_waves ? c->knobs.front_waves : (c->opt.flags & GSR_FLAG_THROUGHPUT) ? FRONT_WAVES_NARROW : FRONT_WAVES_WIDE;
}

inline SortKnobs sort_knobs_of(const gsr_ctx* c)
{
    return SortKnobs{c->knobs.sort_order, c->knobs.sort_kpb, c->knobs.rect_carry ? 1u : 0u, c->knobs.rect_carry_bucket ? 1u : 0u};
}

// gsr_frame.cpp
// (fresh_items: the work items are sized afresh -- the list was replaced -- instead of only growing)
int alloc_bins(gsr_ctx* c, bool fresh_items = false);
int enqueue_frame(gsr_ctx* c, bool render);
int finish_frame(gsr_ctx* c);
int sync_and_repair(gsr_ctx* c);
void drop_graph(gsr_ctx* c);
// gsr_scene.cpp
int alloc_scene(gsr_ctx* c, uint32_t n, bool with_rows);
// the context's per-splat buffers follow a scene another member replaced (nothing to do while scene_gen is the scene's generation)
int adopt_scene(gsr_ctx* c);
// the context leaves its scene (the last member frees it); c->scene is null afterwards
void scene_release(gsr_ctx* c);
// what the blocking scene replacements do first (limitBox, erase, new SH textures, growth): waits for every other member's stream
int sync_members(gsr_ctx* c);
// gsr_scene_limit_box from need_rows on, for either predicate (gsr_scene_erase_selected is the other caller): the kept splats, in
// order, become the scene; SH state, generation, bins and the members' frame state as the header says of limitBox; the selection is
// empty afterwards.  `what` names the caller in a HIP error.
// carry (null: none): one more set that keeps naming the same splats, as the hidden set does: out[new index of i] = in[i] for every
// kept i, into `out`, nwords_out words zeroed by the caller (gsr_scene_merge_cells: the merged rows, its selection afterwards)
struct SetCarry { const uint32_t* in; uint32_t nwords_in; uint32_t* out; uint32_t nwords_out; };
int scene_compact(gsr_ctx* c, const ScenePred& p, const char* what, uint32_t* kept_out, const SetCarry* carry = nullptr);
// the host upload path of gsr_set_scene / gsr_set_scene_arrays and gsr_scene_append_arrays: m host rows staged, repacked and checked
// into rows [at, at + m) of `v` (rotations / scales null: a scene without them); *mismatch: positions differ from data words 0..2
int upload_rows(gsr_ctx* c, const char* what, const SceneDev& v, uint32_t at, uint32_t m, const uint32_t* data, const float* positions,
                const float* rotations, const float* scales, uint32_t* mismatch);
// Device-side order around an edit of a shared scene that arrives through `c` (translate, rotate, scale, a change of the hidden
// set), no host wait: edit_begin makes c's stream wait for what every other member has enqueued, edit_end makes whatever the
// others enqueue from now on wait for the edit; invalidate_members marks every member's frame state as edited (lists: the sorted
// order went too)
int edit_begin(gsr_ctx* c);
int edit_end(gsr_ctx* c);
void invalidate_members(gsr_ctx* c, bool lists);
// GSR_ERR_ARG with the message unless the scene carries rotations and scales (built from rows or from the four arrays): what the
// transforms, the compactions and the edits of the selection all demand first
int require_rows(gsr_ctx* c);
// gsr_select.cpp, for either set (`spare`: the hidden set's third word buffer, null for the selection).
// set_ensure: the buffers for `rows` splats, allocated by the first call that needs them -- nothing happens while the set holds
// that many; the counters are zeroed, and the mask unless the caller stores every word of it (zero_mask false).
int set_ensure(gsr_ctx* c, SplatSet& s, DevBuf<uint32_t>* spare, uint32_t rows, bool zero_mask = true);
// set_count: the end of every fold of a set (launch_select_apply, which leaves the bits set in the set's counters): that count to
// the host and into s.count -- the copy, the wait for the stream, and "<what> failed: .." for an error of either or of a launch
// in front of them.  The launch stays with the callers: what lies between it and the copy differs (nothing for the selection,
// edit_end for the hidden set, the compaction's other counts for scene_compact's carry).
int set_count(gsr_ctx* c, SplatSet& s, const char* what);
// gsr_read_selection / gsr_read_hidden (`who`): the count and ceil(n / 32) words, zeros from a set never allocated
int set_read(gsr_ctx* c, const SplatSet& s, const char* who, uint32_t* words, uint32_t nwords, uint32_t* count);
// the two sets for the scene's count (set_ensure), and the end of every call that changes the selection:
// selection <- selection (op) scratch on the device, its count back to the host
int hidden_ensure(gsr_ctx* c);
int select_ensure(gsr_ctx* c);
int select_fold_and_count(gsr_ctx* c, int op, uint32_t* selected);
// The scope of an analysis call (splat data, neighbours, clusters, k nearest neighbours, merging cells).  scope_check (gsr_attr.cpp):
// the two refusals those calls share, in the header's order -- flags outside GSR_SCOPE_*, a budget above GSR_NEIGHBOUR_MAX_BUDGET (a
// call without a budget passes 0); nothing is touched.  scene_scope: the scope as the kernels take it, over the scene's sets as they are.
int scope_check(gsr_ctx* c, const char* who, uint32_t scope, uint64_t budget = 0);
inline AttrScope scene_scope(const SharedScene& sc, uint32_t flags) { return AttrScope{flags, sc.sel.mask, sc.sel.words, sc.hid.mask, sc.hid.words}; }
// gsr_neighbours.cpp, for the calls that walk the spatial index (neighbours, clusters, k nearest neighbours).  NbCall: one call's scope and index.
// nb_check: the refusals they share, in the header's order, with `cap` in cap_min .. cap_max under the name cap_name; nothing is
// touched.  nb_index: everything up to the first walk -- the context's scratch (allocated by the first call,
// only grown), the index, its bound against the budget, *info.  GSR_ERR_ARG (with *info filled) when the bound is above the
// budget: no walk has been launched.  n >= 1; the device is current and no member's stream holds work.
struct NbCall {
    AttrScope sc;
    NbIndex ix;
    uint32_t n, indexed;
    uint32_t* hist;                                   // the device counters (null: the call wants none)
};
int nb_check(gsr_ctx* c, const char* who, double radius, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t cap_min = 1u, const char* cap_name = "cap",
             uint32_t cap_max = GSR_NEIGHBOUR_MAX_CAP);
int nb_index(gsr_ctx* c, const char* who, double radius, uint32_t cap, uint32_t scope, uint64_t budget, bool want_hist, NbCall* call, gsr_neighbour_info* info);
// nb_index's first step, for a caller with cells of its own (gsr_merge.cpp): the context's scratch for the scene's n splats, *ix
// over it with the given inv_h and r2, the words of NbInfo and cap + 1 histogram counters (*hist) and the table zeroed on the stream
int nb_prepare(gsr_ctx* c, const char* who, uint32_t cap, double inv_h, double r2, NbIndex* ix, uint32_t** hist);
// the same for n rows that need not be the context's own scene's (n >= 1): the caller names the arrays to index when it builds
// (gsr_match.cpp indexes ANOTHER context's scene into this context's scratch)
int nb_prepare_rows(gsr_ctx* c, const char* who, uint32_t n, uint32_t cap, double inv_h, double r2, NbIndex* ix, uint32_t** hist);
// gsr_normals.cpp, for gsr_match.cpp's point-to-plane calls, which take the TARGET's normals as gsr_normals stores them.
// normal_check: the refusals gsr_normals and gsr_select_normal share, in the header's order; nothing is touched.  normal_run:
// everything up to the read-backs into the context's normals scratch (*arrays) -- (KNN) the index and its bound (nb_index), the
// fill and the walk, or (OWN) the one kernel -- and *info, final on the device and waited for.  GSR_ERR_ARG (with *info's first
// four fields filled) for a bound above the budget: no walk has been launched.  n >= 1; the device is current and no member's
// stream holds work.
int normal_check(gsr_ctx* c, const char* who, const gsr_normal_options* o);
int normal_run(gsr_ctx* c, const char* who, const gsr_normal_options* o, uint64_t budget, NormalArrays* arrays, gsr_normal_info* info);
// gsr_contrib.cpp: what the blocking calls that read per-splat state of a scene do first: waits for every member's stream, so
// that nothing of any member (a contribution pass, an edit) is in flight afterwards
int settle_members(gsr_ctx* c);
// gsr_comm.cpp
void comm_release(gsr_ctx* c);
// gsr_depth.cpp: the depth pass for the frame enqueued last.  depth_frame_check: what every pass demands of that frame (GSR_ERR_ARG,
// `who` in front of the message; nothing enqueued); depth_enqueue: the pass into `p` behind the frame on the render stream (launch
// errors are left for the caller's hipGetLastError)
int depth_frame_check(gsr_ctx* c, const char* who);
// the lists of that frame as every pass behind it walks them (depth, contribution, overlay): the one place that fills FrameLists
FrameLists frame_lists(const gsr_ctx* c);
int depth_enqueue(gsr_ctx* c, DepthPlanes& p, int step, DepthFill fill);
// what gsr_pick and gsr_read_depth do first: gsr_sync's work for the frame (one that did not fit is rendered again), then the checks again
int depth_settle_frame(gsr_ctx* c, const char* who);
// gsr_read_depth up to its copies: the context's planes are the settled frame's (the pass is run if they are not) and final on the
// device; GSR_ERR_OVERFLOW for planes a pass marked invalid
int depth_planes_current(gsr_ctx* c, const char* who);
// gsr_overlay.cpp: the overlay image is the last enqueued frame's, the selection's and the options' -- the pass is enqueued behind the
// frame on the render stream if it is not (launch errors are left for the caller's hipGetLastError); the caller has run
// depth_frame_check and knows that options are set
int overlay_enqueue(gsr_ctx* c);
// what every call that changes the selection's bits does first: waits for the members' streams that may hold an overlay pass, and
// moves the scene's sel_version
int overlay_before_selection_change(gsr_ctx* c);
// gsr_delivery.cpp
int delivery_alloc(gsr_ctx* c, int slots);
// what gsr_delivery_open_depth demands of depth options other than GSR_DEPTH_NONE (GSR_ERR_ARG, `who` in front of the message)
int depth_options_check(gsr_ctx* c, const char* who, const gsr_depth_delivery_options* depth);
void delivery_free(gsr_ctx* c);
bool delivery_frame_held(const gsr_ctx* c);

// true when the device has counted frames that did not fit (k_bin_finalize, sticky accum[5] mirrored into the
// host-mapped mailbox) that the host has not sized the buffers for yet: a plain host read, no copy, no sync
inline bool overflow_pending(const gsr_ctx* c)
{
    return c->words.mailbox && *reinterpret_cast<volatile const uint64_t*>(c->words.mailbox) != c->words.overflow_seen;
}

}  // namespace gsr

#pragma GCC visibility pop
