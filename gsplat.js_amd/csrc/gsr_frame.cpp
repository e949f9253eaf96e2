// The frame: what its launches are handed (build_frame_args), the chain itself, its capture and replay as a HIP graph,
// stage timing, and the repair of frames whose bin lists did not fit.  Also the sizing of everything the binning and the
// compositor use (alloc_bins), from the two stages' plans: plan_bins (k_bin.hip) and plan_blend (k_blend.hip) hold the policy.
#include "gsr_ctx.h"

#include <algorithm>
#include <cstring>

using namespace gsr;

namespace {

// keys in the largest high-digit bucket of the last sorted frame (the low half of mailbox[1]; 0xffffffff until a frame of this
// scene has reported): what plan_sort picks the sort order from
inline uint32_t largest_bucket_reported(const gsr_ctx* c) { return reinterpret_cast<volatile const uint32_t*>(c->words.mailbox)[2]; }

bool band_is_partial(const BinGrid& g) { return g.bx_lo > 0 || g.bx_hi < g.nbx; }

// What a frame's launches are handed, from the context as it stands: every buffer, size and policy value, by name.
void build_frame_args(const gsr_ctx* c, bool render, FrameArgs& a)
{
    memset(&a, 0, sizeof a);
    const BinGrid g = make_grid(c);
    // the sort's form for this frame (plan_sort, k_sort.hip): the order, the width, whether the rectangles travel with the keys and
    // whether the frame runs on a band's survivors; every pointer below that depends on one of them follows it.
    // band mode (a context that composites only part of the screen): the projection's workgroups pack their survivors (see
    // k_project_key) and only those are sorted and binned; the full depthIndex is produced on demand (gsr_read_depth_index)
    const SortPlan sp = plan_sort(c->scene->n, c->sort.rows, front_waves_of(c), render, band_is_partial(g), largest_bucket_reported(c), sort_knobs_of(c));
    FrameState* fs = c->words.fstate;
    a.render = render;
    a.n = c->scene->n;
    a.grid = g;
    a.early_out_eps = c->opt.early_out_eps;

    // a sort-only frame has its own slots (sets 1 and 2 in turn; set 0 belongs to the render frames and k_begin_frame)
    const size_t slot_set = (size_t)FRAME_SLOTS * FRAME_SLOT_WORDS;
    int32_t* slots_now = render ? c->words.slots.p : c->words.slots + (size_t)(1 + c->sort.parity) * slot_set;
    a.slots_next = render ? nullptr : c->words.slots + (size_t)(2 - c->sort.parity) * slot_set;

    a.proj.sc = c->scene_soa();   // (with the hidden set while a bit of it is set, null otherwise: a change of that re-captures the graph)
    if (!render) a.proj.sc.hidden = nullptr;   // gsr_sort does not look at it: the depth key and the order are the whole scene's
    a.proj.depth = c->sort.depth;
    a.proj.slots = slots_now;
    if (render) {
        a.proj.rec = c->sort.rec;
        a.proj.rect = c->sort.rect_idx;
        a.proj.overflow = &fs->overflow;
        a.proj.kept = sp.band ? c->sort.kept.p : nullptr;
        a.proj.kept_lane = sp.band ? c->sort.kept_lane.p : nullptr;
    }

    SortBuffers& sb = a.sort;
    sb.depth = c->sort.depth;
    sb.slots = slots_now;
    sb.minmax = fs->minmax;
    sb.keys = c->sort.keys;
    sb.keys_tmp = c->sort.keys_tmp;
    sb.idx_tmp = c->sort.idx_tmp;
    sb.depth_index = c->sort.depth_index;
    sb.block_hist = c->sort.block_hist;
    sb.digit_total = fs->digit_total;
    sb.rect = c->sort.rect_idx;
    sb.kept = c->sort.kept;
    sb.kept_lane = c->sort.kept_lane;
    sb.koff = sp.band ? c->sort.koff.p : nullptr;
    sb.count = &fs->sorted_count;
    sb.plan = sp;
    sb.max_bucket = reinterpret_cast<uint32_t*>(c->words.mailbox_dev + 1);
    sb.chunk_tab = c->sort.chunk_tab;
    sb.rect_tmp = c->sort.rect_tmp;
    sb.rects_out = sp.carry ? c->sort.rects.p : nullptr;
    if (!render) return;

    BinBuffers& bb = a.bin;
    bb.depth_index = c->sort.depth_index;
    bb.count = &fs->sorted_count;
    bb.table = c->bin.table;
    bb.slots = c->words.slots;
    bb.rect_idx = c->sort.rect_idx;
    bb.rects = c->sort.rects;
    bb.rects_sorted = sp.carry;
    bb.bin_total = c->bin.total;
    bb.bin_start = c->bin.start;
    bb.bin_start_pre = c->bin.start_pre;
    bb.plan = c->bin.plan;
    bb.seg_start = c->bin.seg_start;
    bb.items = c->bin.items;
    bb.list = c->bin.list;
    bb.overflow = &fs->overflow;
    bb.visible = &fs->visible;
    bb.tile_entries = &fs->tile_entries;
    bb.accum = c->words.accum;
    bb.mailbox = c->words.mailbox_dev;
    bb.report = fs->report;
    bb.capacity = c->bin.capacity;
    bb.seg_len_dev = &fs->seg_len;
    bb.queue = &fs->queue;
    bb.bin_mask = c->bin.mask;
    bb.cell_list = c->bin.cell_list;
    bb.cell_total = c->bin.cell_total;
    bb.cell_start = c->bin.cell_start;
    bb.chunk_start = c->bin.chunk_start;
    bb.chunk_info = c->bin.chunk_info;
    bb.cell_wcnt = c->bin.cell_wcnt;
    bb.cell_table2 = c->bin.cell_table2;
    bb.band = band_is_partial(g) ? 1u : 0u;
    bb.n_max = c->scene->n;

    // the compositor reads what the binning wrote; its kernel, grid and work-item policy are the context's plan (plan_blend)
    BlendBuffers& bl = a.blend;
    bl.items = bb.items;
    bl.seg_start = bb.seg_start;
    bl.bin_start = bb.bin_start;
    bl.list = bb.list;
    bl.rec = c->sort.rec;
    bl.shcol = c->shcol;
    bl.fb = c->out.fb;
    bl.partial = c->bin.partial;
    bl.queue = bb.queue;
    bl.seg_len_dev = bb.seg_len_dev;
    bl.capacity = bb.capacity;
    bl.nsplats = std::max(c->scene->n, 1u);
    bl.bin_mask = bb.bin_mask;
    bl.plan = c->bin.blend;
}

// the projection's launch of this frame: its arguments from `a`, the context's current camera
void set_projection(gsr_ctx* c, const FrameArgs& a)
{
    ProjectLaunch& p = c->proj;
    p.sc = a.proj.sc;
    p.n = a.n;
    p.cam = c->cam;
    p.do_project = 1;
    p.depth = a.proj.depth;
    p.slots = a.proj.slots;
    p.rec = a.proj.rec;
    p.bbox = nullptr;
    p.rect = a.proj.rect;
    p.overflow = a.proj.overflow;
    p.kept = a.proj.kept;
    p.kept_lane = a.proj.kept_lane;
    p.bind();
}

// the frame's device work on the context's stream: projection + depth key, sort, (bin, blend).  Launches from `a` (and, for
// a render frame, c->proj, which set_projection filled from it) and records the stage events; changes nothing in the context.
int enqueue_chain(gsr_ctx* c, const FrameArgs& a, bool timing)
{
    hipStream_t s = c->stream;
    hipEvent_t* ev = c->timing.ev;
    if (timing) HIP_TRY(c, hipEventRecord(ev[EV_BEGIN], s));
    if (a.n) {
        if (a.render) launch_project_key(c->proj, s);
        else launch_depth_key(a.proj.sc, a.n, c->cam, a.proj.depth, a.proj.slots, a.slots_next, s);
    } else {
        // an empty scene runs no kernel that stores the frame's depth range (k_quantise_hist does otherwise): it is the range the
        // reference starts from (wasm/wasm.cpp:14-15), not the one of a scene that is gone
        HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)&a.sort.minmax[0], 0x7fffffff, 1, s));
        HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)&a.sort.minmax[1], (int)0x80000000u, 1, s));
    }
    if (timing) HIP_TRY(c, hipEventRecord(ev[EV_PROJECT], s));
    launch_sort(a.sort, a.n, s);
    if (timing) HIP_TRY(c, hipEventRecord(ev[EV_SORT], s));
    if (a.render) {
        if (!a.n) {
            HIP_TRY(c, hipMemsetAsync(a.bin.bin_total, 0, sizeof(uint32_t) * a.bin.plan.nbins, s));
            HIP_TRY(c, hipMemsetAsync(a.bin.overflow, 0, sizeof(uint32_t), s));   // (k_project_key zeroes it otherwise)
        }
        launch_bin(a.bin, a.blend.plan, a.grid, s);
        if (timing) HIP_TRY(c, hipEventRecord(ev[EV_BIN], s));
        launch_blend(a.blend, a.grid, a.early_out_eps, s, (timing && !a.blend.plan.fused) ? ev[EV_BLEND] : nullptr);
        if (timing) HIP_TRY(c, hipEventRecord(ev[EV_COMBINE], s));
    }
    HIP_TRY(c, hipGetLastError());
    return GSR_OK;
}

// captures the chain of `a` into c->graph; false: this runtime cannot (the caller falls back to individual launches)
bool capture_graph(gsr_ctx* c, const FrameArgs& a)
{
    hipStream_t s = c->stream;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) return false;
    const int r = enqueue_chain(c, a, false);
    hipGraph_t gph = nullptr;
    bool ok = (hipStreamEndCapture(s, &gph) == hipSuccess) && r == GSR_OK && gph;
    hipGraphNode_t project = nullptr;
    if (ok && a.n) {   // the node whose camera argument changes from frame to frame
        size_t nn = 0;
        ok = hipGraphGetNodes(gph, nullptr, &nn) == hipSuccess && nn > 0;
        std::vector<hipGraphNode_t> nodes(nn);
        if (ok) ok = hipGraphGetNodes(gph, nodes.data(), &nn) == hipSuccess;
        for (size_t k = 0; ok && k < nn && !project; k++) {
            hipGraphNodeType ty;
            hipKernelNodeParams kp{};
            if (hipGraphNodeGetType(nodes[k], &ty) == hipSuccess && ty == hipGraphNodeTypeKernel &&
                hipGraphKernelNodeGetParams(nodes[k], &kp) == hipSuccess && kp.func == project_key_kernel())
                project = nodes[k];
        }
        ok = ok && project != nullptr;
    }
    if (ok) ok = hipGraphInstantiate(&c->graph.exec, gph, nullptr, nullptr, 0) == hipSuccess;
    if (ok) { c->graph.graph = gph; c->graph.project = project; memcpy(&c->graph.key, &a, sizeof a); }
    else if (gph) (void)hipGraphDestroy(gph);
    return ok;
}

// the captured graph with this frame's camera in its projection node; false: this runtime cannot rewrite the node
bool set_graph_camera(gsr_ctx* c)
{
    hipKernelNodeParams kp{};
    kp.func = const_cast<void*>(project_key_kernel());
    kp.gridDim = project_key_grid(c->proj.n);
    kp.blockDim = dim3(PROJ_THREADS);
    kp.sharedMemBytes = 0;
    kp.kernelParams = c->proj.ptrs;
    kp.extra = nullptr;
    return hipGraphExecKernelNodeSetParams(c->graph.exec, c->graph.project, &kp) == hipSuccess;
}

// after a synchronised render: pull the frame words of the last frame (counts for gsr_timings, its overflow word)
int check_frame_words(gsr_ctx* c, bool* overflowed)
{
    // one small copy: the frame words up to and including k_bin_finalize's report
    FrameState* host = c->words.fstate_host;
    HIP_TRY(c, hipMemcpyAsync(host, c->words.fstate, offsetof(FrameState, digit_total), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t* acc = host->report;
    gsr_timings& tm = c->timing.tm;
    tm.sum_visible = acc[0]; tm.sum_bin_entries = acc[1]; tm.sum_tile_entries = acc[2]; tm.sum_frames = acc[3];
    tm.visible = host->visible;
    tm.tile_entries = host->tile_entries;
    tm.bin_entries = (uint32_t)host->report[5];
    tm.n = c->scene->n;
    *overflowed = host->overflow != 0;
    return GSR_OK;
}

// Frames did not fit since the host last looked: wait for the stream, regrow the list for the largest of them and
// count them (*newly).  Those frames were not composited: a frame whose lists do not fit publishes no work items, so
// the framebuffer kept the image before it.  The caller decides whether one of them can still be rendered again.
int handle_overflow(gsr_ctx* c, uint64_t* newly)
{
    *newly = 0;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t acc[8];
    HIP_TRY(c, hipMemcpyAsync(acc, c->words.accum, sizeof acc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (acc[5] == c->words.overflow_seen) return GSR_OK;
    *newly = acc[5] - c->words.overflow_seen;
    c->words.overflow_seen = acc[5];
    c->words.overflow_frames += *newly;
    const uint64_t need = acc[6];
    const uint64_t want = need + (need >> 2) + (1u << 20);
    if (want > 0xfffffff0ull) return fail(c, GSR_ERR_OVERFLOW, "bin list would need %llu entries", (unsigned long long)want);
    if (want > c->bin.capacity) {
        c->bin.capacity = (uint32_t)want;
        if (int r = c->bin.list.alloc(c, c->bin.capacity)) return r;
    }
    return alloc_bins(c, true);
}

}  // namespace

namespace gsr {

int alloc_bins(gsr_ctx* c, bool fresh_items)
{
    if (!c->W) return GSR_OK;
    c->frame_lists = false;   // (grid, lists or work items change: what the last frame left in them is not walked again)
    gsr_ctx::Bin& b = c->bin;
    const Knobs& k = c->knobs;
    const BinGrid g = make_grid(c);
    // the binning's form, grids and table shape for this grid, scene and list (plan_bins, k_bin.hip): the buffers follow it
    const uint64_t capacity = b.capacity ? b.capacity : std::max<uint64_t>(6ull * c->scene->n + (1u << 20), 1u << 22);   // (a new scene's list, allocated below)
    b.plan = plan_bins(g, c->scene->n, capacity, c->cu_count, front_waves_of(c), BinKnobs{k.bin_two_level, k.bin_big, k.bin_rounds, k.cell_grid});
    const BinPlan& p = b.plan;
    const uint32_t nbins = (uint32_t)p.nbins;
    // the compositor's kernel, grid and work items for the same (plan_blend, k_blend.hip).  The item table only grows, unless the
    // bins or the list it is sized by are replaced below, or the caller has replaced the list
    const bool items_afresh = fresh_items || nbins > b.nbins_alloc || !b.capacity;
    const uint32_t items_alloc = items_afresh ? 0u : b.blend.max_items;
    b.blend = plan_blend(nbins, (uint32_t)((g.bx_hi - g.bx_lo) * BIN_PX) * (uint32_t)c->H, (uint32_t)capacity, c->cu_count,
                         (c->opt.flags & GSR_FLAG_THROUGHPUT) != 0, c->opt.early_out_eps > 0.0f, items_alloc,
                         BlendKnobs{k.fuse_combine ? 1u : 0u, k.saturate ? 1u : 0u, k.items_by_size, k.long_items, k.long_tau, k.blend_sub, k.seg_target,
                                    k.blend_grid, k.seg_len});
    const size_t table = (size_t)p.table_rows * p.table_cols;
    if (table > b.table_elems) {
        if (int r = b.table.alloc(c, table)) return r;
        b.table_elems = (uint32_t)table;
    }
    if (nbins > b.nbins_alloc) {
        if (int r = b.total.alloc(c, nbins)) return r;
        if (int r = b.start.alloc(c, nbins + 1)) return r;
        if (int r = b.start_pre.alloc(c, nbins + 1)) return r;
        if (int r = b.seg_start.alloc(c, nbins + 1)) return r;
        if (b.blend.fused) {
            if (int r = b.mask.alloc(c, nbins)) return r;
        }
        b.nbins_alloc = nbins;
    }
    if (!b.capacity) {
        b.capacity = (uint32_t)capacity;
        if (int r = b.list.alloc(c, b.capacity)) return r;
    }
    if (p.form == BIN_TWO_LEVEL) {
        const uint32_t ncells = (uint32_t)p.ncells;
        if (ncells > b.cell_ncells_alloc) {
            if (int r = b.cell_total.alloc(c, ncells + 1)) return r;
            if (int r = b.cell_start.alloc(c, ncells + 1)) return r;
            if (int r = b.chunk_start.alloc(c, ncells + 2)) return r;
            b.cell_ncells_alloc = ncells;
            b.cell_capacity_alloc = 0;
        }
        if (b.capacity > b.cell_capacity_alloc) {
            if (int r = b.cell_list.alloc(c, (size_t)b.capacity * 2)) return r;
            if (int r = b.cell_table2.alloc(c, (size_t)p.chunks * 16u)) return r;
            if (int r = b.chunk_info.alloc(c, (size_t)p.chunks * 4u)) return r;
            if (int r = b.cell_wcnt.alloc(c, (size_t)p.chunks * 64u)) return r;
            b.cell_capacity_alloc = b.capacity;
        }
    }
    if (b.blend.max_items > items_alloc) {
        if (int r = b.items.alloc(c, (size_t)b.blend.max_items * 4)) return r;   // (four words per work item: k_bin_finalize)
        if (b.blend.partial_slots) {
            if (int r = b.partial.alloc(c, (size_t)b.blend.partial_slots * BIN_PX * BIN_PX)) return r;
        }
    }
    return GSR_OK;
}

void drop_graph(gsr_ctx* c)
{
    if (c->graph.exec) (void)hipGraphExecDestroy(c->graph.exec);
    if (c->graph.graph) (void)hipGraphDestroy(c->graph.graph);
    c->graph.exec = nullptr; c->graph.graph = nullptr; c->graph.project = nullptr;
}

// enqueue one frame: the chain as individual launches when the frame carries stage events or is sort-only, as one graph
// launch otherwise (13 launches and a copy become one: the host issues a frame in ~12 us instead of ~45 us, which is
// what a rank of a multi-GPU run or a small scene is bound by)
int enqueue_frame(gsr_ctx* c, bool render)
{
    if (!c->have_cam) return fail(c, GSR_ERR_ARG, "gsr_set_camera has not been called");
    if (render && (!c->W || !c->H)) return fail(c, GSR_ERR_ARG, "framebuffer size is 0");
    hipStream_t s = c->stream;
    if (int r = adopt_scene(c)) return r;   // (the scene was replaced through another member: this context's buffers follow)
    if (render && overflow_pending(c)) {
        // an earlier asynchronous frame did not fit: regrow before this one is enqueued.  The frames that overflowed
        // are lost (later frames were already behind them); gsr_sync reports how many.
        uint64_t newly = 0;
        if (int r = handle_overflow(c, &newly)) return r;
        c->words.dropped_frames += newly;
        c->words.dropped_unreported += newly;
    }
    // stage timing is sampled: every timing.every-th frame carries the six events (each is a packet the command
    // processor has to retire; on short frames they cost more than they measure)
    gsr_ctx::Timing& t = c->timing;
    const bool timing = t.valid && t.every != 0xffffffffu && (t.frame_no++ % t.every) == 0;   // (0xffffffff: no frame)
    if (timing) {
        if (t.pending == gsr_ctx::Timing::EV_RING) { if (int r = finish_frame(c)) return r; }
        const int slot = (t.head + t.pending) % gsr_ctx::Timing::EV_RING;
        t.ev = t.evring[slot];
        t.is_render[slot] = render;
    }
    FrameArgs a;
    build_frame_args(c, render, a);
    c->cam.W = c->W; c->cam.H = c->H;
    c->cam.band_px0 = a.grid.bx_lo * BIN_PX;
    c->cam.band_px1 = a.grid.bx_hi * BIN_PX;
    c->cam.sh_on = c->scene->sh_count ? 1 : 0;
    c->cam.band[0] = c->scene->band[0]; c->cam.band[1] = c->scene->band[1]; c->cam.band[2] = c->scene->band[2];
    // the SH frame travels in the camera block: the one argument a graph replay rewrites, so a changed frame reaches the
    // projection like a changed camera.  The identity (every context that never opted in) takes the frameless path.
    c->cam.sh_frame = (c->scene->sh_count && !c->scene->sh_frame_is_identity()) ? 1 : 0;
    for (int k = 0; k < 9; k++) c->cam.shm[k] = c->cam.sh_frame ? (float)c->scene->sh_frame[k] : 0.0f;
    if (render) c->cam_frame = c->cam;   // (gsr_read_records projects once more for this camera to get the pixel boxes)
    // No kernel in front of the frame: the camera is an argument of the projection kernel (k_project_key; k_depth_key in a
    // sort-only frame), the frame slots are left clean by their last reader, the frame words are stored, not accumulated
    // (the overflow word is zeroed by k_project_key).  The context's first frame initialises all of them, once.
    static_assert(offsetof(FrameState, minmax) == 0 && sizeof(FrameState) % 4 == 0, "k_begin_frame initialises the frame words");
    if (c->words.slots_need_init) {
        for (int k = 0; k < 3; k++)   // the render frames' slot set and the two of the sort-only frames
            launch_begin_frame(c->cam, c->words.cam_dev, reinterpret_cast<uint32_t*>(c->words.fstate.p), (uint32_t)(sizeof(FrameState) / 4),
                               c->words.slots + (size_t)k * FRAME_SLOTS * FRAME_SLOT_WORDS, s);
        c->words.slots_need_init = false;
    }
    if (render) set_projection(c, a);

    bool replayed = false;
    if (c->graph.enabled && render && !timing) {
        // the graph is replayed while the frame's launches are, byte for byte, the ones it was captured from
        bool ok = true;
        if (!c->graph.exec || memcmp(&a, &c->graph.key, sizeof a) != 0) {
            drop_graph(c);
            ok = capture_graph(c, a);   // (holds this frame's camera already)
        }
        else if (c->graph.project) ok = set_graph_camera(c);
        if (!ok) {   // this runtime cannot capture the chain or rewrite the node: individual launches from now on
            (void)hipGetLastError();
            drop_graph(c);
            c->graph.enabled = false;
        }
        if (c->graph.exec) {
            HIP_TRY(c, hipGraphLaunch(c->graph.exec, s));   // (a failure marks the frame slots for re-initialisation: fail())
            replayed = true;
        }
    }
    if (!replayed) { if (int r = enqueue_chain(c, a, timing)) return r; }
    // what the context remembers of the frame, whichever way it was issued
    // (the parity names the slot set the last k_depth_key reset for its successor: it moves only when that kernel ran, which it
    // does not for an empty scene -- nothing else ever cleans the sort-only frames' two sets)
    if (!render && a.n) c->sort.parity ^= 1;
    c->sort.plan = a.sort.plan;
    if (timing) t.pending++;
    t.recorded = timing;
    t.render = render;
    c->have_sort = true;
    c->have_frame = c->have_frame || render;
    if (render) { c->frame_serial++; c->frame_lists = true; }
    return GSR_OK;
}

int finish_frame(gsr_ctx* c)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    gsr_ctx::Timing& t = c->timing;
    while (t.pending > 0) {
        hipEvent_t* ev = t.evring[t.head];
        const bool render = t.is_render[t.head];
        float a = 0, b = 0, d = 0, e = 0, f = 0, tot = 0;
        HIP_TRY(c, hipEventElapsedTime(&a, ev[EV_BEGIN], ev[EV_PROJECT]));
        HIP_TRY(c, hipEventElapsedTime(&b, ev[EV_PROJECT], ev[EV_SORT]));
        tot = a + b;
        if (render) {
            HIP_TRY(c, hipEventElapsedTime(&d, ev[EV_SORT], ev[EV_BIN]));
            if (c->bin.blend.fused) {   // the fold of multi-segment bins runs inside k_blend: one stage, no event in between
                HIP_TRY(c, hipEventElapsedTime(&e, ev[EV_BIN], ev[EV_COMBINE]));
            } else {
                HIP_TRY(c, hipEventElapsedTime(&e, ev[EV_BIN], ev[EV_BLEND]));
                HIP_TRY(c, hipEventElapsedTime(&f, ev[EV_BLEND], ev[EV_COMBINE]));
            }
            HIP_TRY(c, hipEventElapsedTime(&tot, ev[EV_BEGIN], ev[EV_COMBINE]));
        }
        t.tm.ms_project_key = a; t.tm.ms_sort = b; t.tm.ms_bin = d; t.tm.ms_blend = e; t.tm.ms_combine = f; t.tm.ms_total = tot;
        t.tm.sum_ms_project_key += a; t.tm.sum_ms_sort += b; t.tm.sum_ms_bin += d; t.tm.sum_ms_blend += e; t.tm.sum_ms_combine += f;
        t.tm.sum_ms_total += tot;
        t.tm.frames++;
        t.head = (t.head + 1) % gsr_ctx::Timing::EV_RING;
        t.pending--;
    }
    t.recorded = false;
    return GSR_OK;
}

// wait for the context's stream; if frames overflowed, regrow and render the last frame again (when it was one of
// them); lost frames are added to dropped_unreported, which gsr_sync turns into one GSR_ERR_OVERFLOW
int sync_and_repair(gsr_ctx* c)
{
    if (int r = finish_frame(c)) return r;
    bool last_ov = false;
    if (c->have_frame && c->timing.render) {
        if (int r = check_frame_words(c, &last_ov)) return r;
    }
    if (overflow_pending(c)) {
        uint64_t newly = 0;
        if (int r = handle_overflow(c, &newly)) return r;   // buffers regrown for the largest frame seen
        if (last_ov && newly) {  // the last frame is one of them and nothing has been enqueued behind it: render it again
            if (int r = enqueue_frame(c, true)) return r;
            if (int r = finish_frame(c)) return r;
            bool again = false;
            if (int r = check_frame_words(c, &again)) return r;
            if (again) return fail(c, GSR_ERR_OVERFLOW, "bin list overflow after regrowth");
            newly -= 1;
        }
        c->words.dropped_frames += newly;
        c->words.dropped_unreported += newly;
    }
    return GSR_OK;
}

}  // namespace gsr

// The plan the context's last enqueued frame sorted from, for tests (tests/test_gpu_sort_plan.py compares it with what
// gsr_debug_sort_plan answers for the context's inputs).  GSR_ERR_ARG before a first frame.  Not part of the ABI.
extern "C" int gsr_debug_last_sort_plan(gsr_ctx* c, SortPlan* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    if (!c->have_sort) return fail(c, GSR_ERR_ARG, "no sort has run yet");
    *out = c->sort.plan;
    return GSR_OK;
}

// The compositor plan the context holds: what alloc_bins sized from and the next frame is launched from (tests/test_gpu_blend_plan.py
// compares it with what gsr_debug_blend_plan answers for the context's inputs).  Not part of the ABI.
extern "C" int gsr_debug_last_blend_plan(gsr_ctx* c, BlendPlan* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    *out = c->bin.blend;
    return GSR_OK;
}
